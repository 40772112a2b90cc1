"""Host side of the persistent launches (csrc/persist*.hip) that every caller shares: the control-word layout and the verdict read from it, the
workgroup counts that verdict expects, the ticket of launches enqueued but not yet checked, and the adaptive fallback's cool-down."""
import os

# Control words of one launch (csrc/persist_common.h, PCTRL_HEAD_WORDS; persist_status_kernel reads the first three the same way):
# workgroups at the start rendezvous | 0, or why the launch gave up | workgroups that ran to the end | slice groups publishing near |
# free-running decoder: rows that stopped, last step
ARRIVALS, ABORT, FINISHED, NEAR_GROUPS, ROWS_FINISHED, LAST_STEP = range(6)

PERSIST_STRIKES = 2          # consecutive uses with a fallback before the persistent plans are switched off ...
PERSIST_COOLDOWN = 200       # ... for this many uses


def decoder_workgroups():
    """Workgroups of a decoder launch - forward, BPTT or free-running: PWG."""
    return 256


def lstm_fwd_workgroups(B, H, ndir):
    """... of an LSTM forward launch over ndir sequences of B rows and H units: LF<H>::WG = H / 8 (EFWG = 32 at H = 256) per 32 rows."""
    return ndir * ((B + 31) // 32) * (H // 8)


def lstm_bwd_workgroups(B, ndir):
    """... of an LSTM BPTT launch (H = 256 only): EBWG = 16 per 32 rows."""
    return ndir * ((B + 31) // 32) * 16


def ran_to_end(words, n_wg):
    """Did the launch with these control words run to its end?  No abort code, and every one of its n_wg workgroups finished."""
    return int(words[ABORT]) == 0 and int(words[FINISHED]) == n_wg


def near_xcd():
    """mstts_persist_desc.near_xcd: MSTTS_PERSIST_NEAR=0 keeps every hand-off out of the XCDs' L2s."""
    return int(os.environ.get("MSTTS_PERSIST_NEAR", "1") != "0")


class Ticket:
    """Launches that are enqueued and not yet checked.  ctrl: their control words on the device; host: the caller's page-locked block to read
    them back into; expect: the workgroup count of the ONE launch whose words ctrl is, or [(row, count), ...] for launches that own a row each."""
    __slots__ = ("ctrl", "host", "expect", "event", "failed")

    def __init__(self, ctrl, host, expect):
        self.ctrl, self.host, self.expect, self.event, self.failed = ctrl, host, expect, None, None

    def enqueue(self, event=None):
        """The read-back, on the CURRENT stream: call on the launching stream right behind the launch (a side stream's wait is a
        barrier in a hardware queue it may share).  `event` is recorded behind it; without one the caller synchronises before redeem()."""
        self.host.copy_(self.ctrl, non_blocking=True)
        self.event = event
        if event is not None:
            event.record()
        return self

    def redeem(self):
        """(verdict, first three status words) once the event has fired; of the first launch that gave up, if any - `failed` is its row."""
        if self.event is not None:
            self.event.synchronize()
        status = ()
        for row, n_wg in [(None, self.expect)] if isinstance(self.expect, int) else self.expect:
            status = tuple((self.host if row is None else self.host[row])[:3].tolist())      # (one read per launch)
            if not ran_to_end(status, n_wg):
                self.failed = row or 0
                return False, status
        return True, status


class CoolDown:
    """`strikes` failures in a row switch the persistent plans off for `cooldown` uses, then they are probed again.  What counts as a failure
    and when the books are closed is the caller's business."""

    def __init__(self):
        self.strikes = self.off = 0              # failures in a row | uses left of the cool-down

    def strike(self, strikes=PERSIST_STRIKES, cooldown=PERSIST_COOLDOWN):
        """A use fell back.  True when that starts a cool-down."""
        self.strikes += 1
        if self.strikes < strikes:
            return False
        self.strikes, self.off = 0, cooldown
        return True

    def clear(self):
        self.strikes = 0

    def admit(self):
        """May this use take the persistent launches?  False takes one use off the cool-down."""
        if self.off > 0:
            self.off -= 1
            return False
        return True
