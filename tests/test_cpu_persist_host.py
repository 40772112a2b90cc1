"""Host side of the persistent launches (multi_speaker_tts_amd/persist.py) on fabricated control words: the verdict, the workgroup counts
the kernels' constants imply, the ticket's order of operations, and the inference engine's cool-down policy at its call site.  No library
load, no device."""
import types
import warnings

import pytest
import torch

from multi_speaker_tts_amd import persist as P


def _words(arrivals, abort, finished, n=16):
    w = torch.zeros(n, dtype=torch.int32)
    w[P.ARRIVALS], w[P.ABORT], w[P.FINISHED] = arrivals, abort, finished
    return w


class _Event:
    """Stand-in for a stream event: runs the "copy" it was recorded behind only when the host waits for it."""

    def __init__(self, log, on_sync=None):
        self.log, self.on_sync = log, on_sync

    def record(self):
        self.log.append("record")

    def synchronize(self):
        self.log.append("synchronize")
        if self.on_sync is not None:
            self.on_sync()


def test_verdict_truth_table():
    assert (P.ARRIVALS, P.ABORT, P.FINISHED, P.NEAR_GROUPS, P.ROWS_FINISHED, P.LAST_STEP) == (0, 1, 2, 3, 4, 5)
    n = P.decoder_workgroups()
    assert P.ran_to_end(_words(n, 0, n), n) is True
    for code in (1, 2, 3):
        assert P.ran_to_end(_words(n, code, 0), n) is False                 # gave up: rendezvous / a wait / self-test
        assert P.ran_to_end(_words(n, code, n), n) is False                 # an abort code with the full count is still a failure
    assert P.ran_to_end(_words(n, 0, n - 1), n) is False
    assert P.ran_to_end(_words(n, 0, n), n + 1) is False                    # a count that drifted never passes
    assert P.ran_to_end([n, 0, n], n) is True                               # any host view of the words


def test_workgroup_counts_mirror_the_kernels():
    assert P.decoder_workgroups() == 256                                    # PWG
    for B in (1, 32):                                                       # the encoder pair: EFWG = 32, EBWG = 16, two directions
        assert P.lstm_fwd_workgroups(B, 256, 2) == 64 and P.lstm_bwd_workgroups(B, 2) == 32
    assert P.lstm_fwd_workgroups(32, 128, 2) == 32                          # LF<128>::WG = 16
    assert P.lstm_fwd_workgroups(33, 256, 1) == 2 * 32 and P.lstm_bwd_workgroups(33, 1) == 2 * 16
    assert P.lstm_fwd_workgroups(320, 256, 1) == 10 * 32 and P.lstm_bwd_workgroups(320, 1) == 10 * 16


def test_ticket_reads_after_its_event():
    log = []
    ctrl, host = _words(256, 0, 256, 272), torch.full((272,), -1, dtype=torch.int32)
    late = _words(256, 0, 256, 272)
    t = P.Ticket(ctrl, host, 256)
    ev = _Event(log, on_sync=lambda: host.copy_(late))                      # what the device wrote is on the host once the event fired
    assert t.enqueue(ev) is t and log == ["record"] and t.event is ev
    late[P.ABORT], late[P.FINISHED] = 3, 17
    assert t.redeem() == (False, (256, 3, 17)) and log == ["record", "synchronize"] and t.failed == 0
    late[P.ABORT], late[P.FINISHED] = 0, 256
    assert t.redeem() == (True, (256, 0, 256))
    assert t.ctrl is ctrl and t.expect == 256                               # what mstts_persist_status is handed


def test_ticket_without_event_and_over_a_slot_array():
    ctrl = torch.zeros(64, 16, dtype=torch.int32)
    ctrl[0, :3] = torch.tensor([64, 0, 64]); ctrl[1, :3] = torch.tensor([32, 0, 32]); ctrl[2, :3] = torch.tensor([96, 0, 96])
    host = torch.zeros(64, 16, dtype=torch.int32)
    t = P.Ticket(ctrl, host, [(0, 64), (1, 32), (2, 96)]).enqueue()         # (the caller synchronises the stream itself)
    assert t.event is None and torch.equal(host, ctrl)
    assert t.redeem() == (True, (96, 0, 96)) and t.failed is None
    ctrl[1, 2] = 31
    t.enqueue()
    assert t.redeem() == (False, (32, 0, 31)) and t.failed == 1


def test_deferred_check_is_redeemed_once():
    from multi_speaker_tts_amd.inference import _DeferredCheck
    log = []
    eng = types.SimpleNamespace(_deferred_host_pool=[], persist_lstm_selftest=0)
    ctrl = torch.zeros(64, 16, dtype=torch.int32)
    ctrl[0, :3] = torch.tensor([96, 0, 96])
    host = torch.zeros(64, 16, dtype=torch.int32)
    chk = _DeferredCheck(eng, None, (), {}, P.Ticket(ctrl, host, [(0, 96)]).enqueue(_Event(log)))
    assert chk.pending == [(0, 96)] and chk.host is host
    assert chk.ok() is True and log == ["record", "synchronize"] and chk.host is None
    assert len(eng._deferred_host_pool) == 1 and eng._deferred_host_pool[0] is host      # the block went back to the pool
    with pytest.raises(RuntimeError, match="redeemed once"):
        chk.ok()
    assert len(eng._deferred_host_pool) == 1
    # the self-test hook turns a good ticket into a failure, after the block is back in the pool
    eng.persist_lstm_selftest = 1
    chk = _DeferredCheck(eng, None, (), {}, P.Ticket(ctrl, eng._deferred_host_pool.pop(), [(0, 96)]).enqueue(_Event(log)))
    assert chk.ok() is False and eng.persist_lstm_selftest == 0 and len(eng._deferred_host_pool) == 1


def test_cooldown_object():
    c = P.CoolDown()
    assert c.admit() and c.strike() is False and c.strikes == 1
    c.clear()
    assert c.strikes == 0 and c.strike() is False and c.strike() is True and (c.strikes, c.off) == (0, P.PERSIST_COOLDOWN)
    assert (P.PERSIST_STRIKES, P.PERSIST_COOLDOWN) == (2, 200)
    c = P.CoolDown()
    assert c.strike(1, 2) is True and [c.admit() for _ in range(4)] == [False, False, True, True]


def _infer_policy_obj(monkeypatch, outcomes):
    """InferEngine._decode_persistent on a bare object: the shape is covered, the launch is a ticket over fabricated words."""
    from multi_speaker_tts_amd import inference as I
    monkeypatch.setattr(I.lib, "load", lambda: types.SimpleNamespace(mstts_persist_infer_supported=lambda *a: 1))
    o = types.SimpleNamespace(d=types.SimpleNamespace(dec_lstm=1024, att=128, prenet=256, n_mel=80, mem=768, att_k=31), persist_infer=True,
                              _persist_cool=P.CoolDown(), persist_disabled_decodes=0, persist_infer_fallbacks=0, persist_infer_launches=0,
                              persist_infer_status=None, launched=0)

    def launch(q, values, w0f, mk, B, T):
        o.launched += 1
        good = outcomes.pop(0)
        w = _words(256, 0 if good else 1, 256 if good else 0, 272)
        w[P.ROWS_FINISHED], w[P.LAST_STEP] = 4, 7
        return P.Ticket(w, torch.zeros(272, dtype=torch.int32), 256).enqueue()
    o._persist_infer_launch = launch
    o.decode = lambda: I.InferEngine._decode_persistent(o, None, None, None, None, 4, 40, 100)
    return I, o


def test_inference_engine_cooldown_policy(monkeypatch):
    I, o = _infer_policy_obj(monkeypatch, [True, False, True, False, False, True])
    monkeypatch.setattr(I, "PERSIST_COOLDOWN", 3)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        assert o.decode() == 7 and o.persist_infer_status == (256, 0, 256, 4, 7)          # the launch's last step
        assert o.decode() is None and o._persist_cool.strikes == 1                         # one strike: still trying
        assert o.decode() == 7 and o._persist_cool.strikes == 0                            # a success in between clears it
        assert o.decode() is None and o._persist_cool.strikes == 1 and not rec
        assert o.decode() is None and o.persist_infer_status == (256, 1, 0, 4, 7)          # two in a row: the cool-down starts at the failure
        assert len(rec) == 1 and "two consecutive persistent decoder launches gave up" in str(rec[0].message)
        assert "for the next 3 batches" in str(rec[0].message)
        assert o.persist_infer_fallbacks == 3 and o.launched == 5
        for i in range(3):                                                                 # ... three decodes that launch nothing
            assert o.decode() is None and o.persist_disabled_decodes == i + 1 and o.launched == 5
        assert o.decode() == 7 and o.launched == 6 and o.persist_disabled_decodes == 3     # then a probe
    assert o.persist_infer_launches == 3 and len(rec) == 1


def test_inference_engine_warns_at_every_cooldown(monkeypatch):
    I, o = _infer_policy_obj(monkeypatch, [False] * 4)
    monkeypatch.setattr(I, "PERSIST_COOLDOWN", 1)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        assert [o.decode() for _ in range(6)] == [None] * 6                                # fail, fail, off, fail, fail, off
    assert len(rec) == 2 and o.persist_disabled_decodes == 2 and o.persist_infer_fallbacks == 4


def test_derived_operands_follow_the_params_version():
    """InferEngine._derived_at_version on a bare object: built once per ParamStore.version, refilled after a bump into the same buffers,
    and one key's refill leaves the others alone."""
    from multi_speaker_tts_amd.inference import InferEngine
    o = types.SimpleNamespace(params=types.SimpleNamespace(version=3), _derived={})
    log = []

    def get(key, value):
        def alloc():
            log.append(("alloc", key))
            return torch.zeros(2)

        def fill(buf):
            log.append(("fill", key))
            buf.fill_(value)
        return InferEngine._derived_at_version(o, key, alloc, fill)
    a = get("a", 1.0)
    assert log == [("alloc", "a"), ("fill", "a")] and a.tolist() == [1.0, 1.0]
    assert get("a", 9.0) is a and a.tolist() == [1.0, 1.0] and len(log) == 2               # same version: neither built nor filled again
    b = get("b", 2.0)
    assert b is not a and log[2:] == [("alloc", "b"), ("fill", "b")] and a.tolist() == [1.0, 1.0]
    o.params.version += 1                                                                  # a load, or a trainer's Adam step on a shared store
    assert get("a", 5.0) is a and log[4:] == [("fill", "a")] and a.tolist() == [5.0, 5.0]  # refilled in place, no new buffer
    assert b.tolist() == [2.0, 2.0] and o._derived["b"][0] == 3                            # "b" is still the version-3 build ...
    assert get("b", 6.0) is b and log[5:] == [("fill", "b")] and b.tolist() == [6.0, 6.0]  # ... until it is asked for
    assert get("a", 7.0) is a and get("b", 8.0) is b and len(log) == 6


def test_near_xcd_is_read_in_one_place(monkeypatch):
    monkeypatch.delenv("MSTTS_PERSIST_NEAR", raising=False)
    assert P.near_xcd() == 1
    monkeypatch.setenv("MSTTS_PERSIST_NEAR", "0")
    assert P.near_xcd() == 0
