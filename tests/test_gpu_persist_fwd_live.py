"""mstts_persist_desc.ctx_dead on the forward launch (csrc/persist.hip, template parameter MC = live context width 512): the persistent
teacher-forced decoder loop that neither forms nor ships nor multiplies the 256 speaker columns of the context, against the same launch at
the full width (ctx_dead = 0) and both against the fp64 oracle (tests/decoder_loop_ref.py::unrolled_decoder: oracle.model's cells and
attention step).  The C entries are called directly on descriptors built by hand (tests/test_gpu_decoder_loop_ref.py's helpers), the
inputs are float32 arrays drawn once on the host and keep the promise of ctx_dead: values = [encoder 512 | speaker 256 tiled over the
row's positions], zero past the row's length.  The algebra is tests/test_cpu_ctx_live_fwd.py's.

Shapes: B in {1, 5, 32} x T in {7, 128}, ragged lengths (row 0 full, row 1 length 1), S = 2 (the first step has no incoming context: the
constant gate term must not be added there) and S = 13 (the four-slot rings wrap three times, the generation bit flips twice): the
smallest at which row padding, slice cuts and ring reuse can go wrong.

Bound (the rule of tests/test_gpu_persist_fwd_qown.py): per compared tensor, max |difference| / max |reference| of the live launch against
fp64 is at most 2 x the full-width launch's on the same inputs, and below 1e-3 (tests/test_gpu_depth.py).  The live launch drops no term:
the speaker columns' share of the cell-0 gates is an fp32 FMA chain over 256 terms instead of part of a split matrix-core sum."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.helpers import rel_err, t2n
from multi_speaker_tts_amd import lib
from tests import decoder_loop_ref as R
from tests.test_gpu_decoder_loop_ref import A, KS, _fwd_desc, _nan, _pdesc, _weights

pytestmark = pytest.mark.gpu

BOUND = 1e-3
DEAD, LIVE_W = 256, 512
HISTORIES = ("pj", "in0", "in1", "q_hist", "align_hist", "cum_hist")
UNPACKED = ("acts0", "acts1", "craw0", "craw1", "c0", "c1")          # what mstts_persist_unpack_history restores from opk


@pytest.fixture(scope="module")
def wcache():
    cache = {}
    yield cache
    cache.clear()


def _case(B, T, S, seed=0):
    """Inputs of one shape at the WIDE widths, as decoder_loop_ref.case_data draws them, with the value tail that ctx_dead promises."""
    cd = dict(widths="WIDE", B=B, Te=T, S=S, name="live_%d_%d_%d" % (B, T, S), **R.dims_of("WIDE"))
    H, M, P = cd["H"], cd["M"], cd["P"]
    assert M == LIVE_W + DEAD
    g = np.random.default_rng(1000 * B + 10 * T + S + seed)
    w = R.weights("WIDE")
    lens = g.integers(1, T + 1, B)
    lens[0] = T
    if B > 1:
        lens[1] = 1
    cd["lens"] = torch.tensor(lens.astype(np.int32))
    live = np.arange(T)[None, :] < lens[:, None]
    memory = g.normal(0, 1, (B, T, M)).astype(np.float32)
    cd["spk"] = g.normal(0, 1, (B, DEAD)).astype(np.float32)
    memory[:, :, LIVE_W:] = cd["spk"][:, None, :]
    cd["values"] = R._f32(memory * live[:, :, None])
    cd["keys"] = (cd["values"].double() @ w["wmem"].double()).float()
    cd["pre"] = R._f32(np.maximum(g.normal(0, 1, (S, B, P)), 0) * (g.random((S, B, P)) > 0.5) * 2.0)
    cd["xw0"] = (cd["pre"].double() @ w["wx0"].double() + w["b0"].double()).float()
    for k in R.MASKS:
        cd[k] = torch.tensor((g.random((S, B, H)) > R.RATE).astype(np.uint8))
    for k in R.WEIGHTS:
        cd[k] = w[k]
    return cd


def _oracle(cd):
    lv = {k: cd[k].double() for k in ("w0f", "w1", "b1", "wq", "keys", "values", "pre", "wx0", "b0") + R.LSA_NAMES}
    with torch.no_grad():
        o = R.unrolled_decoder(lv, cd["lens"], {k: cd[k] for k in R.MASKS}, R.RATE)
    return {k: v.numpy() for k, v in o.items()}


def _upload(dev, cd):
    return {k: cd[k].to(dev).contiguous() for k in ("keys", "values", "lens", "xw0", "pre") + R.MASKS}


def _launch(dev, cd, w, u, ctx_dead, bf16=0, fail_step=0):
    """One persistent forward launch in the form the train step uses (pre / b0, opk) on output buffers of its own, NaN-filled."""
    L = lib.load()
    d, f = _fwd_desc(dev, cd, w, u, "persistent", packed=True)
    p, pt = _pdesc(dev, w["pk"], int(L.mstts_persist_fwd_ws_bytes()), recurrent_bf16=bf16)
    f["opk"] = _nan(dev, int(L.mstts_persist_opk_floats(cd["S"])))
    p.opk, p.pre, p.b0 = lib.ptr(f["opk"]), lib.ptr(u["pre"]), lib.ptr(w["b0"])
    p.ctx_dead, p.selftest_fail_step = ctx_dead, fail_step
    f["_keep"] = (p, pt, d)
    rc = L.mstts_decoder_train_fwd_persistent(C.byref(d), C.byref(p), lib.stream())
    torch.cuda.synchronize()
    return rc, d, p, pt, f


def _ended(pt):
    c = pt["ctrl"].cpu().numpy()
    assert c[1] == 0 and c[2] == 256, c[:4]


def _got(d, f):
    lib.call("mstts_persist_unpack_history", lib.ptr(f["opk"]), C.byref(d))
    torch.cuda.synchronize()
    return {k: t2n(f[k]).copy() for k in HISTORIES + UNPACKED + ("opk",)}


def _errors(cd, got, ref):
    """max |got - ref| / max |ref| per tensor; the slots no loop writes (decoder_loop_ref.exclude_unwritten) take the reference's values."""
    g = R.exclude_unwritten(got, ref, packed=True)
    return {k: rel_err(np.asarray(g[k], np.float64), ref[k]) for k in HISTORIES + UNPACKED}


@pytest.mark.parametrize("S", [2, 13])
@pytest.mark.parametrize("B,T", [(1, 7), (5, 7), (32, 7), (1, 128), (5, 128), (32, 128)])
def test_live_width_against_full_width_and_oracle(dev, wcache, B, T, S):
    L = lib.load()
    cd = _case(B, T, S)
    if not L.mstts_persist_fwd_supported(B, cd["H"], cd["M"], A, T, KS):
        pytest.skip("persistent loop not available on this device (needs 256 CUs and one workgroup per CU)")
    w, u = _weights(dev, wcache, "WIDE"), _upload(dev, cd)
    ref = _oracle(cd)
    rc, d0, p0, pt0, f0 = _launch(dev, cd, w, u, 0)
    assert rc == 0
    _ended(pt0)
    full = _got(d0, f0)
    rc, d1, p1, pt1, f1 = _launch(dev, cd, w, u, DEAD)
    assert rc == 0
    _ended(pt1)
    # ---- sentinels: every element of slots 0 .. S (in0) / steps 0 .. S-1 (pj) written over its NaN fill, the dead columns spk[b] bit for bit
    spk = cd["spk"]
    H = cd["H"]
    for twice in range(2):
        in0, pj = t2n(f1["in0"]), t2n(f1["pj"])
        assert np.isfinite(in0).all() and np.isfinite(pj).all()
        assert not in0[0].any()                                        # slot 0: the zero state, all 768 context columns
        assert np.array_equal(in0[1:, :, LIVE_W:LIVE_W + DEAD], np.broadcast_to(spk, (S, B, DEAD)))
        assert np.array_equal(pj[:, :, H + LIVE_W:], np.broadcast_to(spk, (S, B, DEAD)))
        if twice == 0:
            live = _got(d1, f1)
            f1["in0"].zero_(); f1["pj"].zero_()
            lib.call("mstts_decoder_train_fwd_persistent", C.byref(d1), C.byref(p1))       # (zeroed: they are written again)
            torch.cuda.synchronize()
            _ended(pt1)
    # ---- determinism: the second launch on the same inputs, bit for bit
    again = _got(d1, f1)
    for k in live:
        assert np.array_equal(live[k], again[k], equal_nan=True), "%s differs between two launches on the same inputs" % k
    # ---- against fp64, and against the full width's error on the same inputs
    e_full, e_live = _errors(cd, full, ref), _errors(cd, live, ref)
    print("B %d T %d S %d  (live, full) vs fp64: %s" % (B, T, S, "  ".join("%s %.2e %.2e" % (k, e_live[k], e_full[k]) for k in e_live)))
    print("B %d T %d S %d  opk live vs full: %.2e" % (B, T, S, rel_err(live["opk"], full["opk"])))
    bad = {k: (e_live[k], e_full[k]) for k in e_live if not (e_live[k] < BOUND and e_live[k] <= 2.0 * e_full[k])}
    assert not bad, bad
    assert rel_err(live["opk"], full["opk"]) < BOUND


def test_ctx_dead_is_validated(dev, wcache):
    """Anything but 0 or 256 is MSTTS_ERR_SHAPE (-1, the code the BPTT entry gives), and nothing is launched or cleared."""
    L = lib.load()
    cd = _case(5, 7, 2)
    if not L.mstts_persist_fwd_supported(5, cd["H"], cd["M"], A, 7, KS):
        pytest.skip("persistent loop not available on this device")
    w, u = _weights(dev, wcache, "WIDE"), _upload(dev, cd)
    for bad in (1, 128, 512):
        rc, d, p, pt, f = _launch(dev, cd, w, u, bad)
        assert rc == -1, (bad, rc)
        assert not pt["ctrl"].cpu().numpy().any()                      # no workgroup arrived
        assert torch.isnan(f["in0"]).all() and torch.isnan(f["pj"]).all() and torch.isnan(f["q_hist"]).all()


@pytest.mark.parametrize("T,bf16", [(160, 0), (40, 1)])
def test_calls_without_a_live_instantiation_run_the_full_width(dev, wcache, T, bf16):
    """More than 128 positions and the bf16 form have no live-width kernel: ctx_dead = 256 selects the full-width one, as ctx_dead = 0 does."""
    L = lib.load()
    cd = _case(8, T, 13)
    if not L.mstts_persist_fwd_supported(8, cd["H"], cd["M"], A, T, KS):
        pytest.skip("persistent loop not available on this device")
    w, u = _weights(dev, wcache, "WIDE"), _upload(dev, cd)
    out = []
    for dead in (0, DEAD):
        rc, d, p, pt, f = _launch(dev, cd, w, u, dead, bf16=bf16)
        assert rc == 0
        _ended(pt)
        out.append(_got(d, f))
    errs = {k: rel_err(out[1][k], out[0][k]) for k in HISTORIES + ("opk",)}
    print("T %d bf16 %d  ctx_dead 256 vs 0: %s" % (T, bf16, errs))
    assert all(np.isfinite(out[1][k]).all() for k in ("pj", "q_hist", "align_hist"))
    assert max(errs.values()) < BOUND, errs
    if not bf16:
        ref = _oracle(cd)
        e0, e1 = _errors(cd, out[0], ref), _errors(cd, out[1], ref)
        bad = {k: (e1[k], e0[k]) for k in e1 if not (e1[k] < BOUND and e1[k] <= 2.0 * e0[k])}
        assert not bad, bad


def test_abort_on_the_live_instantiation_falls_back(dev, wcache):
    """The self-test knob once: workgroup 0 raises the abort word at step 3 of a live-width launch, the launch ends early and says so in its
    control words; the launch-per-step loop, which the caller runs then, gives the reference result."""
    L = lib.load()
    B, T, S = 8, 40, 10
    cd = _case(B, T, S)
    if not L.mstts_persist_fwd_supported(B, cd["H"], cd["M"], A, T, KS):
        pytest.skip("persistent loop not available on this device")
    w, u = _weights(dev, wcache, "WIDE"), _upload(dev, cd)
    rc, d, p, pt, f = _launch(dev, cd, w, u, DEAD, fail_step=4)
    assert rc == 0
    c = pt["ctrl"].cpu().numpy()
    assert c[1] == 3 and c[2] < 256, c[:4]
    d2, f2 = _fwd_desc(dev, cd, w, u, "full")
    lib.call("mstts_decoder_train_fwd", C.byref(d2))
    torch.cuda.synchronize()
    ref = _oracle(cd)
    got = {k: t2n(f2[k]) for k in R.FORWARD_Q}
    g = R.exclude_unwritten(got, ref, packed=False)
    errs = {k: rel_err(np.asarray(g[k], np.float64), ref[k]) for k in R.FORWARD_Q}
    print("launch-per-step re-run vs fp64:", errs)
    assert max(errs.values()) < BOUND, errs
