"""mstts_decoder_train_bwd_desc.ctx_dead / mstts_persist_desc.ctx_dead through TrainEngine at the reference widths: the BPTT that skips the
speaker columns of the context gradient (persistent launch, live width 512) against the same launch at the full width (ctx_dead = 0, the
earlier pack) and against the launch-per-step loop, on ONE forward state per shape.  The algebra is tests/test_cpu_ctx_dead.py's.

Bounds: what tests/test_gpu_persist.py::test_persistent_bptt_equals_launch_per_step grants the two drivers against each other, 5e-5 of the
largest element for L <= 20 and 5e-4 above - the change is another summation of the same gradient, short of a term that is zero in exact
arithmetic."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import dims_pair, rel_err, t2n, to_dev
from oracle import model as OM, train as OT
from multi_speaker_tts_amd import lib
from multi_speaker_tts_amd.engine import TrainEngine
from multi_speaker_tts_amd.params import CELL, LSA

pytestmark = pytest.mark.gpu

WIDE = dict(emb=64, enc_conv_ch=64, enc_lstm=256, spk=256, prenet=256, dec_lstm=1024, n_mel=16, post_ch=32)      # tests/test_gpu_persist.py::WIDE
BWD = ("dg0", "dg1", "dq_hist", "de_hist")
DEAD = 256
SENTINEL = 12345.0
# the partial-d_ctx ring inside the BPTT launch's exchange buffer (csrc/persist_bwd.hip: BDG, BPART, BPCTX, BO_PCTX; 4 slots), in floats
PRING, BDG, BPART, BPCTX = 4, 8 * 8 * 2 * 4 * 256, 256 * 8 * 32 * 4, 32 * 192 * 8 * 4
BO_PCTX = 2 * PRING * BDG + 3 * PRING * BPART
PCTX_LIVE = 32 * 128 * 8 * 4                # floats of a slot that 128 four-column blocks per row reach


@pytest.fixture(scope="module")
def engine(dev):
    pd, od = dims_pair(**WIDE)
    values = OM.init_params(od, 3)
    g = np.random.default_rng(4)
    for k in values:
        if k.endswith(("bias", "bias_b")):
            values[k] = g.normal(0, 0.1, values[k].shape)
    eng = TrainEngine(pd, device=dev, values=values)
    if not (eng.persist and eng.persist_bwd):
        pytest.skip("persistent BPTT not available on this device (needs 256 CUs and one workgroup per CU)")
    assert eng.ctx_dead == DEAD and eng.d.mem == 768
    return eng, od


def _snapshot(eng, w, parts):
    Ml = eng.d.mem - DEAD
    out = {k: t2n(getattr(w, k)).copy() for k in BWD}
    out["d_ctx_live"] = t2n(w.d_in0[:parts, 1:, :, :Ml].double().sum(0)).copy()
    out["grad"] = t2n(eng.params.grad).copy()
    return out


def _ring_tail(w):
    """[slot][words beyond the 128 blocks per row] of the partial-d_ctx ring, as int32 (a launch arms the whole ring with 0xFF bytes)."""
    x = w.xch_b.view(torch.int32)[BO_PCTX:BO_PCTX + PRING * BPCTX].view(PRING, BPCTX)
    return x[:, PCTX_LIVE:], x[:, :PCTX_LIVE]


def _repack(eng, dead):
    """The BPTT launch's packed kernels, cut for `dead` (0: through the earlier entry point)."""
    k1, o1 = eng.P(CELL % 1 + "kernel"); wq, oq = eng.P(LSA + "query_layer/kernel")
    args = (lib.ptr(eng.w0f), lib.ptr(k1, o1), lib.ptr(wq, oq), lib.ptr(eng.pkb[0]), lib.ptr(eng.pkb[1]), lib.ptr(eng.pkb[2]))
    if dead:
        lib.call("mstts_persist_bwd_pack_live", *args, dead)
    else:
        lib.call("mstts_persist_bwd_pack", *args)


def _copy(desc):
    out = type(desc)()
    C.memmove(C.byref(out), C.byref(desc), C.sizeof(desc))
    return out


def _compare(a, b, L, what):
    bound = 5e-4 if L > 20 else 5e-5
    errs = {k: rel_err(a[k], b[k]) for k in a}
    print(what, " ".join("%s=%.2e" % kv for kv in errs.items()))
    for k in a:
        assert np.isfinite(a[k]).all() and np.isfinite(b[k]).all(), (what, k)
    bad = {k: e for k, e in errs.items() if not e <= bound}
    assert not bad, (what, bad)


@pytest.mark.parametrize("B,Te,L", [(32, 128, 9),       # 128-position kernel, two row tiles
                                    (8, 160, 12),       # 256-position kernel, one row tile
                                    (5, 128, 3),        # rows < 16
                                    (32, 100, 24)])     # more steps than ring slots
def test_bptt_without_the_speaker_columns(dev, engine, B, Te, L):
    eng, od = engine
    H, M = eng.d.dec_lstm, eng.d.mem
    Ml = M - DEAD
    batch = to_dev(OT.synthetic_batch(od, B, Te, L, seed=5, ragged=True), dev)
    seed = OT.step_seed(1234, 0)
    w = eng.plan(B, Te, L)
    assert w.persist_bwd and w.dec_b.ctx_dead == DEAD and w.pdesc_b.ctx_dead == DEAD
    fallbacks0 = eng.persist_bwd_fallbacks
    eng.forward(batch, w, seed=seed)

    def sentinels():
        w.d_in0[..., Ml:M] = SENTINEL
        w.d_pj[..., H + Ml:] = SENTINEL
        w.d_values[..., Ml:] = SENTINEL

    def complete():
        torch.cuda.synchronize()
        st = w.pctrl_b.cpu().numpy()
        assert eng.persist_bwd_fallbacks == fallbacks0 and st[1] == 0 and st[2] == 256, st[:3]

    # ---- (1) the persistent launch at the live width
    sentinels()
    eng.loss_and_backward(w)
    complete()
    a = _snapshot(eng, w, 1)
    d_in0_1 = t2n(w.d_in0[0]).copy()
    assert (w.d_in0[..., Ml:M] == SENTINEL).all() and (w.d_pj[..., H + Ml:] == SENTINEL).all() and (w.d_values[..., Ml:] == SENTINEL).all()
    tail, head = _ring_tail(w)
    assert (tail == -1).all()                                # never written: still the launch's 0xFF fill
    assert (head[:min(L + 1, PRING)] != -1).any(dim=1).all()    # (the part inside the 128 blocks is in use)
    # ---- determinism: the launch alone, twice more on the same state
    for _ in range(2):
        for k in BWD:
            getattr(w, k).zero_()
        lib.call("mstts_decoder_train_bwd_persistent", C.byref(w.dec_b), C.byref(w.pdesc_b))
        complete()
        for k in BWD:
            assert np.array_equal(a[k], t2n(getattr(w, k))), k
        assert np.array_equal(d_in0_1, t2n(w.d_in0[0]))
    # ---- (2) the same launch with every context column (the earlier pack, the field cleared in both descriptors)
    w.d_pj[..., H + Ml:] = 0.0
    w.d_in0.zero_()
    w.dec_b.ctx_dead = w.pdesc_b.ctx_dead = 0
    _repack(eng, 0)
    try:
        eng.loss_and_backward(w)
        complete()
        b = _snapshot(eng, w, 1)
        assert (_ring_tail(w)[0][0] != -1).any()             # (the full-width launch does use the words beyond the 128 blocks)
        assert float(w.d_in0[0, 1:, :, Ml:M].abs().max()) > 0
    finally:
        w.dec_b.ctx_dead = w.pdesc_b.ctx_dead = DEAD
        _repack(eng, DEAD)
    _compare(a, b, L, "live width against full width:")
    # ---- (3) the launch-per-step loop
    for k in BWD:
        getattr(w, k).zero_()
    w.d_in0.zero_()
    w.d_in0[..., Ml:M] = SENTINEL
    w.persist_bwd = False
    try:
        eng.loss_and_backward(w)
        torch.cuda.synchronize()
    finally:
        w.persist_bwd = True
    c = _snapshot(eng, w, w.d_in0_parts)
    assert (w.d_in0[..., Ml:M] == 0).all()                   # cleared behind the loop, in every slab
    _compare(a, c, L, "live width against launch per step:")
    # ---- validation
    L_ = lib.load()
    bd, pb = _copy(w.dec_b), _copy(w.pdesc_b)
    bd.ctx_dead = pb.ctx_dead = 128
    assert L_.mstts_decoder_train_bwd(C.byref(bd), lib.stream()) == -1                           # MSTTS_ERR_SHAPE
    assert L_.mstts_decoder_train_bwd_persistent(C.byref(bd), C.byref(pb), lib.stream()) == -1
    fwd0 = _copy(w.dec)
    fwd0.S = 0
    bd0 = _copy(w.dec_b)
    bd0.fwd = C.pointer(fwd0)
    assert L_.mstts_decoder_train_bwd(C.byref(bd0), lib.stream()) == 0                           # no step: nothing to clear, no error
    torch.cuda.synchronize()
    # ---- abort path: the launch gives up at its third step, the launch-per-step loop takes over
    eng.persist_bwd_selftest = 3
    try:
        eng.forward(batch, w, seed=seed)
        eng.loss_and_backward(w)
        torch.cuda.synchronize()
    finally:
        eng.persist_bwd_selftest = 0
    assert eng.persist_bwd_fallbacks == fallbacks0 + 1 and eng.persist_last_status[1] == 3
    e = rel_err(t2n(eng.params.grad), c["grad"])
    print("fallback step against launch per step: grad=%.2e" % e)
    assert e <= (5e-4 if L > 20 else 5e-5)
    assert (w.d_in0[..., Ml:M] == 0).all()
