"""lib.fork / lib.join: the one way the engines move work to a side stream and wait for it."""
import pytest
import torch

from multi_speaker_tts_amd import lib
from multi_speaker_tts_amd.lib import call, ptr

pytestmark = pytest.mark.gpu
N, CHAIN = 1024, 200


def test_fork_orders_both_ways_and_exposes_its_event_only_when_asked(dev):
    """The main stream counts x up CHAIN times (dependent launches: about a millisecond of device time that a stream which did not wait would
    overtake); work in a fork reads x == CHAIN; the main stream, behind join, reads the fork's result.  done=False: no event."""
    lib.load()
    side = torch.cuda.Stream(device=dev)
    x, y, z = (torch.empty(N, dtype=torch.float32, device=dev) for _ in range(3))
    one, zero = torch.ones(N, device=dev), torch.zeros(N, device=dev)
    main = torch.cuda.current_stream()
    call("mstts_fill", ptr(x), 0.0, N)
    call("mstts_fill", ptr(y), -1.0, N)
    for _ in range(CHAIN):
        call("mstts_add", ptr(x), ptr(one), ptr(x), N)
    with lib.fork(side) as f:
        assert torch.cuda.current_stream() == side and f.done is None
        for i in range(CHAIN):                                   # (the fork's own work takes as long: the join below has something to wait for)
            call("mstts_add", ptr(y if i else x), ptr(one if i else zero), ptr(y), N)
    assert torch.cuda.current_stream() == main and isinstance(f.done, torch.cuda.Event)
    lib.join(f.done)
    call("mstts_add", ptr(y), ptr(one), ptr(z), N)               # on the main stream, behind the join
    with lib.fork(side, done=False) as g:
        call("mstts_add", ptr(z), ptr(one), ptr(zero), N)        # (zero <- z + 1, behind everything on the main stream so far)
    assert g.done is None and torch.cuda.current_stream() == main
    torch.cuda.synchronize()
    assert torch.equal(x, torch.full_like(x, CHAIN))
    assert torch.equal(y, torch.full_like(y, 2 * CHAIN - 1))     # CHAIN read from x, then CHAIN - 1 increments
    assert torch.equal(z, torch.full_like(z, 2 * CHAIN))
    assert torch.equal(zero, torch.full_like(zero, 2 * CHAIN + 1))
