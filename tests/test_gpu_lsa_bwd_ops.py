"""Op tests of the attention backward (csrc/lsa.hip) in the form the train step calls it (mstts_decoder_train_bwd), each kernel against
tests/lsa_ref.py (fp64; pinned on the CPU by tests/test_cpu_lsa_ref.py, negative controls included).

Rules of every case, as in tests/test_gpu_glue_ops.py: fully written outputs are NaN-filled before the call (with a guard behind them
that must keep its value) and must be finite afterwards; accumulating outputs (dq, d_keys, d_loc_k, d_score_w, d_score_b) are prefilled
with a known non-zero pattern which the reference adds; strided inputs sit inside larger allocations whose other elements are 1e30, so a
read outside the specified region ruins the result instead of faulting; the inputs of every call are the fp64 reference's values rounded
to fp32 (teacher forcing), so each call's error is its own.  Errors are helpers.rel_err figures: max |got - ref| over max |ref|; where a
prefill was added, the denominator is the gradient's maximum WITHOUT the prefill, so the pattern cannot dilute the figure."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from multi_speaker_tts_amd import lib
from tests import lsa_ref as R
from tests.helpers import t2n

pytestmark = pytest.mark.gpu
A, CH, HLD, HH = R.A, R.CH, R.HLD, 64          # HH: the width of the other column block of the caller's rows ([m1 | ctx] / [ctx | h0])
NAN, BIG, GUARD = float("nan"), 1e30, 64
TOL_G, TOL = 2e-5, 5e-5                        # what test_lsa_step_fwd_bwd allows against fp64: the carried G; everything behind a tanh / a long dot
TOL_CONV = 1e-4                                # ... and the unfolded conv kernel / bias
TOL_FORMS = 1e-5                               # single-launch against two-launch form (same test)
CAP = 5e-3                                     # test_train_step_parity's bound: no measured bound may exceed it

# ---- measured bounds (MI355X; three runs each, the largest figure kept; the assertion allows four times it, never more than CAP).  Summation
# order of the fp32 atomics is the only variable run to run.  profiles/lsa_bwd_ops_parity.txt lists the same figures.
ATOMIC_MEASURED = {
    "32-128-34-31-free": dict(d_keys=6.215e-07, dense_k=4.148e-06, score_w=2.656e-06, score_b=3.118e-06, conv_k=3.834e-06, conv_b=9.370e-06),
    "3-37-7-31-det": dict(d_keys=1.281e-07, dense_k=8.124e-07, score_w=2.530e-07, score_b=3.556e-07, conv_k=1.672e-06, conv_b=9.754e-07),
    "3-37-7-31-free": dict(d_keys=2.483e-07, dense_k=8.124e-07, score_w=5.855e-07, score_b=4.392e-07, conv_k=1.571e-06, conv_b=1.189e-06),
    "2-520-3-31-free": dict(d_keys=2.194e-07, dense_k=7.278e-07, score_w=8.454e-07, score_b=8.694e-07, conv_k=3.043e-06, conv_b=2.062e-06),
    "5-70-5-7-free": dict(d_keys=2.075e-07, dense_k=7.554e-07, score_w=5.750e-07, score_b=6.833e-07, conv_k=1.227e-06, conv_b=1.263e-06),
    "1-1-1-1-free": dict(d_keys=1.476e-07, dense_k=1.990e-07, score_w=1.854e-07, score_b=1.476e-07, conv_k=1.127e-06, conv_b=5.152e-07),
}
LOOP_MEASURED = dict(G=4.214e-07, d_e=6.485e-07, dq=1.167e-06, h=7.408e-07, d_keys=4.651e-07, dense_k=7.089e-07, score_w=4.299e-07, score_b=1.320e-06, conv_k=5.878e-07, conv_b=5.709e-07)


def _f32(dev, a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=dev).contiguous()


class _Out:
    """A NaN-filled output of n floats with a guard behind it."""
    def __init__(self, dev, *shape, fill=NAN):
        self.shape, self.n = shape, int(np.prod(shape))
        self.buf = torch.full((self.n + GUARD,), 7.0, dtype=torch.float32, device=dev)
        self.buf[:self.n] = fill
        self.ptr = lib.ptr(self.buf)

    def get(self, what, finite=True):
        got = t2n(self.buf)
        assert (got[self.n:] == 7.0).all(), what + ": written past its end"
        got = got[:self.n].reshape(self.shape)
        if finite:
            assert np.isfinite(got).all(), what + ": NaN / inf in the output (an element was not written, or a sentinel was read)"
        return got

    def untouched(self):
        got = t2n(self.buf)
        return bool(np.isnan(got[:self.n]).all() and (got[self.n:] == 7.0).all())


def _pattern(dev, shape, scale):
    """The prefill of an accumulating output: non-zero, not constant, of the gradient's own magnitude (so its rounding stays below 2^-23 of it)."""
    n = int(np.prod(shape))
    v = (0.5 + (np.arange(n) % 7) / 8.0) * (scale if scale > 0 else 1.0) * np.where(np.arange(n) % 2, 1.0, -1.0)
    return _f32(dev, v.reshape(shape))


def _err(got, ref, den_of=None, scale=None):
    """rel_err of got against ref with the denominator max |den_of| (default ref).  A reference that is identically zero (the gradients behind
    a softmax over ONE position) has no maximum to measure by: `scale`, the magnitude of the terms that cancel, stands in."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    den = float(np.abs(ref if den_of is None else den_of).max())
    if den == 0.0:
        assert scale is not None and scale > 0
        den = scale
    return float(np.abs(got - ref).max() / den)


def _chk(what, got, ref, tol, **kw):
    e = _err(got, ref, **kw)
    print("%-28s %.3e  (bound %.1e)" % (what, e, tol))
    assert e < tol, (what, e, tol)
    return e


class _Lsa:
    """Device copy of a problem: the constant block with the folded filter, every tensor kept alive."""
    def __init__(self, dev, pr):
        B, T, M, KS = pr["B"], pr["T"], pr["M"], pr["KS"]
        p = pr["p"]
        self.dev, self.pr = dev, pr
        self.keys, self.values = _f32(dev, pr["keys"]), _f32(dev, pr["values"])
        self.lengths = None if pr["lengths"] is None else torch.tensor(pr["lengths"], dtype=torch.int32, device=dev)
        self.v = {k: _f32(dev, p[k]) for k in ("conv_k", "conv_b", "dense_k", "score_w", "score_b")}
        self.loc_k, self.loc_b, self.loc_kt = torch.full((KS, A), NAN, device=dev), torch.full((A,), NAN, device=dev), torch.full((A, 36), NAN, device=dev)
        c = self.c = lib.LsaConst()
        c.B, c.T, c.A, c.M, c.KS, c.CH = B, T, A, M, KS, CH
        c.keys, c.values, c.lengths = lib.ptr(self.keys), lib.ptr(self.values), lib.ptr(self.lengths)
        c.conv_k, c.conv_b, c.dense_k, c.score_w, c.score_b = (lib.ptr(self.v[k]) for k in ("conv_k", "conv_b", "dense_k", "score_w", "score_b"))
        lib.call("mstts_lsa_fold_location", c.conv_k, c.conv_b, c.dense_k, lib.ptr(self.loc_k), lib.ptr(self.loc_b), KS, CH, A)
        lib.call("mstts_lsa_filter_by_unit", lib.ptr(self.loc_k), lib.ptr(self.loc_kt), KS, A)
        c.loc_k, c.loc_b, c.loc_kt = lib.ptr(self.loc_k), lib.ptr(self.loc_b), lib.ptr(self.loc_kt)

    def byref(self):
        return C.byref(self.c)


def _rows_in(dev, rows, ld, col0):
    """[..., n] rows placed at columns col0 .. col0 + n - 1 of rows of stride ld; everything else 1e30."""
    rows = np.asarray(rows)
    buf = np.full(rows.shape[:-1] + (ld,), BIG, np.float32)
    buf[..., col0:col0 + rows.shape[-1]] = rows
    return _f32(dev, buf)


def _slabs_in(dev, slabs, ld, pstride):
    """[parts, B, M] slabs as rows [B, ld] (the context gradient in columns 0 .. M - 1) at slab stride pstride >= B * ld; the rest 1e30."""
    parts, B, M = slabs.shape
    assert pstride >= B * ld and pstride % 4 == 0
    buf = np.full(parts * pstride + 8, BIG, np.float32)
    for pp in range(parts):
        v = buf[pp * pstride:pp * pstride + B * ld].reshape(B, ld)
        v[:, :M] = slabs[pp]
    return _f32(dev, buf)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2a. one step in the caller's form
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _step_ref(B, T, M, KS, parts, rows):
    pr, G_next, h_next = R.step_problem(B, T, M, KS, parts, rows)
    return pr, G_next, h_next, R.chain(pr, G_last=R.fold_h(G_next, h_next, KS))


def _run_step_bwd(L, ref, G_next, h_next, parts, single):
    """One backward step in the decoder's form.  d_ctx: columns HH .. of [B, HH + M] rows; d_ctx2: `parts` slabs of [B, M + HH] rows at a slab
    stride above B (M + HH); forward context at stride HH + M.  Returns G, d_align (two-launch form only), d_e, dq - prefill, h and the prefill."""
    pr, dev = L.pr, L.dev
    B, T, M = pr["B"], pr["T"], pr["M"]
    WP, W0 = HH + M, M + HH
    pstride = B * W0 + 12
    dpj = _rows_in(dev, pr["d_ctx"][0], WP, HH)
    d2 = _slabs_in(dev, pr["slabs"][0], W0, pstride)
    pj = _rows_in(dev, ref["ctx"][0], WP, HH)
    al, q, cum = _f32(dev, ref["align"][0]), _f32(dev, ref["q"][0]), _f32(dev, ref["cum"][0])
    Gn, hn = _f32(dev, G_next), _f32(dev, h_next)
    G, de, h, da = _Out(dev, B, T), _Out(dev, B, T), _Out(dev, B, T, HLD), _Out(dev, B, T)
    pre = _pattern(dev, (B, A), float(np.abs(ref["dq"][0]).max()))
    dq = pre.clone()
    if single:
        lib.call("mstts_lsa_step_bwd", L.byref(), lib.ptr(dpj, HH), WP, lib.ptr(d2), W0, parts, pstride, lib.ptr(Gn), lib.ptr(hn), G.ptr,
                 lib.ptr(al), lib.ptr(q), lib.ptr(cum), lib.ptr(pj, HH), WP, de.ptr, lib.ptr(dq), h.ptr)
    else:
        lib.call("mstts_lsa_dalign_bwd", L.byref(), lib.ptr(dpj, HH), WP, lib.ptr(d2), W0, parts, pstride, lib.ptr(Gn), lib.ptr(hn), G.ptr, da.ptr)
        lib.call("mstts_lsa_denergy_bwd", L.byref(), lib.ptr(al), da.ptr, lib.ptr(q), lib.ptr(cum), de.ptr, lib.ptr(dq), h.ptr)
    torch.cuda.synchronize()
    out = dict(G=G.get("G"), d_e=de.get("d_e"), h=h.get("h"), dq=t2n(dq).astype(np.float64) - t2n(pre).astype(np.float64))
    if not single:
        out["d_align"] = da.get("d_align")
    else:
        assert da.untouched()
    return out


def _cancel_scales(pr, ref, L):
    """Magnitudes of the terms that cancel in d_e = a (d_a - dot(a, d_a)) and behind it - used only where the reference is identically zero."""
    s_de = float(np.abs(ref["align"][0] * ref["d_align"][0]).max())
    s_g = s_de * float(np.abs(pr["p"]["score_w"]).max())
    return dict(d_e=s_de, dq=s_g * pr["T"], h=s_g * float(np.abs(ref["loc_k"]).sum(axis=1).max()))


@pytest.mark.parametrize("B,T,M,KS,parts,rows", R.STEP_CASES)
def test_step_bwd_in_the_callers_form(dev, B, T, M, KS, parts, rows):
    """mstts_lsa_dalign_bwd + mstts_lsa_denergy_bwd and mstts_lsa_step_bwd with the operands laid out as mstts_decoder_train_bwd passes them
    (column blocks of wider rows, the second gradient operand as partial slabs), against fp64: G at 2e-5, d_align / d_e / dq / h at 5e-5
    (test_lsa_step_fwd_bwd's bounds against fp64), h[:, :, KS:] exactly zero, the two forms within 1e-5 of each other.  parts = 0 with d_ctx2 set
    reads one slab like parts = 1: bit-identical G, d_align, d_e and h (dq is a sum of fp32 atomics of several workgroups per row, whose
    order is not fixed: 1e-6)."""
    pr, G_next, h_next, ref = _step_ref(B, T, M, KS, parts, rows)
    L = _Lsa(dev, pr)
    two = _run_step_bwd(L, ref, G_next, h_next, parts, single=False)
    one = _run_step_bwd(L, ref, G_next, h_next, parts, single=True)
    sc = _cancel_scales(pr, ref, L)
    for form, got in (("two-launch", two), ("single-launch", one)):
        _chk(form + " G", got["G"], ref["G"][0], TOL_G)
        for k in ("d_e", "dq", "h"):
            _chk("%s %s" % (form, k), got[k], ref[k][0], TOL, scale=sc[k])
        assert (got["h"][:, :, KS:] == 0.0).all(), form + ": taps past KS must be written as zero"
    _chk("two-launch d_align", two["d_align"], ref["d_align"][0], TOL)
    _chk("forms G", one["G"], two["G"], 1e-6)
    for k in ("d_e", "dq", "h"):
        _chk("forms " + k, one[k], two[k], TOL_FORMS, den_of=ref[k][0], scale=sc[k])
    if parts == 0:
        for single, base in ((False, two), (True, one)):
            other = _run_step_bwd(L, ref, G_next, h_next, 1, single=single)
            for k in base:
                if k == "dq":
                    _chk("parts 0 / 1 dq", base[k], other[k], 1e-6, den_of=ref[k][0], scale=sc[k])
                else:
                    assert np.array_equal(base[k], other[k]), "parts = 0 and parts = 1 differ in " + k


@pytest.mark.parametrize("B,T,M,KS", [(2, 520, 16, 31), (1, 1024, 16, 31)])
def test_two_launch_forward_above_512(dev, B, T, M, KS):
    """mstts_lsa_energy_fwd + mstts_lsa_context_fwd at T above 512 and at T_MAX: ctx rows at stride M + 4 (pad columns keep their
    sentinel), the second copy set, against fp64 at test_lsa_step_fwd_bwd's 2e-5."""
    pr, _, _, ref = _step_ref(B, T, M, KS, 1, "ragged")
    L = _Lsa(dev, pr)
    q, cum = _f32(dev, ref["q"][0]), _f32(dev, ref["cum"][0])
    en, al, cn = _Out(dev, B, T), _Out(dev, B, T), _Out(dev, B, T)
    cx = torch.full((B, M + 4), NAN, device=dev)
    cx[:, M:] = BIG
    cx2 = _Out(dev, B, M)
    lib.call("mstts_lsa_energy_fwd", L.byref(), lib.ptr(q), 1, 0, None, lib.ptr(cum), en.ptr)
    lib.call("mstts_lsa_context_fwd", L.byref(), en.ptr, lib.ptr(cum), al.ptr, cn.ptr, lib.ptr(cx), M + 4, cx2.ptr, M)
    torch.cuda.synchronize()
    st = R.step({k: torch.tensor(v) for k, v in pr["p"].items()}, torch.tensor(pr["keys"]), torch.tensor(pr["values"]), torch.tensor(pr["mask"]),
                torch.tensor(ref["q"][0]), torch.tensor(ref["cum"][0]))
    _chk("energy", en.get("energy"), st["energy"].numpy(), TOL_G)
    _chk("align", al.get("align"), ref["align"][0], TOL_G)
    _chk("cum_next", cn.get("cum_next"), st["cum_next"].numpy(), TOL_G)
    got = t2n(cx)
    assert (got[:, M:] == np.float32(BIG)).all(), "pad columns of the ctx rows were written"
    assert np.isfinite(got[:, :M]).all()
    _chk("ctx", got[:, :M], ref["ctx"][0], TOL_G)
    assert np.array_equal(cx2.get("ctx2"), got[:, :M])


# ---------------------------------------------------------------------------------------------------------------------------------
# 2b. refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(dev):
    """Argument errors are return codes, found on the host before any launch: every output keeps its fill.  T above T_MAX = 1024 at every
    entry point; more than eight d_ctx2 slabs (the kernels hold eight slots); a slab stride that is no multiple of 4 floats with d_ctx2
    set (the slabs are read as float4); a parameter-gradient workspace at 4 mod 8 bytes.  mstts_lsa_param_bwd with S = 0 is no error and
    writes nothing."""
    B, T, M, KS = 2, 9, 16, 3
    pr = R.problem(B, T, M, KS, parts=1)
    L, lb = _Lsa(dev, pr), lib.load()
    s = lib.stream()
    n = 1025                                             # (buffers sized for the refused T too: a launch, if one were made, stays in bounds)
    big = torch.zeros(B * n * max(A, M), device=dev)
    outs = [_Out(dev, B * n * HLD) for _ in range(6)]
    acc = [torch.full((B * n * A,), 3.0, device=dev) for _ in range(4)]
    ws = torch.full((int(lb.mstts_lsa_param_bwd_ws_floats(B, n, 2)) + 4,), NAN, device=dev)
    gran = torch.zeros(B * n + 8, dtype=torch.int64, device=dev)
    p, o = lib.ptr(big), [x.ptr for x in outs]

    def dalign(c, parts=1, pstride=B * (M + HH), d2=p):
        return lb.mstts_lsa_dalign_bwd(c, p, M, d2, M, parts, pstride, p, p, o[0], o[1], s)

    def step_bwd(c, parts=1, pstride=B * (M + HH), d2=p):
        return lb.mstts_lsa_step_bwd(c, p, M, d2, M, parts, pstride, p, p, o[0], p, p, p, p, M, o[1], lib.ptr(acc[0]), o[2], s)

    def param(c, S, w):
        return lb.mstts_lsa_param_bwd(c, S, p, p, p, lib.ptr(acc[0]), lib.ptr(acc[1]), lib.ptr(acc[2]), lib.ptr(acc[3]), w, s)

    L.c.T = n
    c = L.byref()
    assert lb.mstts_lsa_energy_fwd(c, p, 1, 0, None, p, o[0], s) != 0
    assert lb.mstts_lsa_context_fwd(c, p, p, o[0], o[1], o[2], M, None, 0, s) != 0
    assert lb.mstts_lsa_step_fwd(c, p, 1, 0, None, p, o[0], o[1], o[2], M, None, 0, None, lib.ptr(gran), 1, s) != 0
    assert dalign(c) != 0 and step_bwd(c) != 0
    assert lb.mstts_lsa_denergy_bwd(c, p, p, p, p, o[0], lib.ptr(acc[0]), o[1], s) != 0
    assert param(c, 2, lib.ptr(ws)) != 0
    L.c.T = T
    assert dalign(c, parts=9) != 0 and step_bwd(c, parts=9) != 0
    assert dalign(c, parts=-1) != 0 and step_bwd(c, parts=-1) != 0
    for bad in (B * (M + HH) + 1, B * (M + HH) + 2):
        assert dalign(c, parts=2, pstride=bad) != 0 and step_bwd(c, parts=2, pstride=bad) != 0
    assert param(c, 2, lib.ptr(ws, 1)) != 0
    assert b"8-byte" in lb.mstts_last_error()
    assert param(c, 0, lib.ptr(ws)) == 0 and param(c, 0, None) == 0
    torch.cuda.synchronize()
    assert all(x.untouched() for x in outs)
    assert all(bool((x == 3.0).all()) for x in acc) and bool(torch.isnan(ws).all()) and int(gran.abs().max()) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 2c. the parameter gradients over S steps
# ---------------------------------------------------------------------------------------------------------------------------------
PT, LP_GROUPS, LP_BLOCK, CHUNK_TARGET = 32, 16, 34 * 128, 2048


def _param_geometry(B, T, S, fixed_order):
    """lsa_param_geometry (csrc/lsa.hip) restated: position tiles, step chunks, steps per workgroup."""
    nt = -(-T // PT)
    ch = max(1, CHUNK_TARGET // (B * nt))
    if fixed_order:
        ch = 1
    ch = min(ch, S)
    spb = -(-S // ch)
    return nt, -(-S // spb), spb


#            (B, T, S, KS, deterministic)  -> (tiles, chunks, steps per workgroup, steps of the last chunk)
PARAM_GEOMETRY = {(32, 128, 34, 31, False): (4, 12, 3, 1),       # 1536 partial blocks; the last chunk holds one step
                  (3, 37, 7, 31, True): (2, 1, 7, 7),            # one workgroup walks all 7 steps; 6 blocks < LP_GROUPS; the second tile holds 5 positions
                  (3, 37, 7, 31, False): (2, 7, 1, 1),           # the chunked form of the same
                  (2, 520, 3, 31, False): (17, 3, 1, 1),         # T > 512
                  (5, 70, 5, 7, False): (3, 5, 1, 1),            # fewer taps
                  (1, 1, 1, 1, False): (1, 1, 1, 1)}


@functools.lru_cache(maxsize=None)
def _param_ref(B, T, S, KS):
    pr = R.param_problem(B, T, S, KS)
    ch = R.chain(pr)
    de = ch["d_e"]
    if T == 1:          # a softmax over one position has no gradient: the chain's d_e is identically zero and would test nothing
        de = np.random.default_rng(5).normal(0, 0.1, de.shape)
    return pr, dict(q=ch["q"].astype(np.float32), cum=ch["cum"].astype(np.float32), d_e=de.astype(np.float32))


def _run_param(L, hist, S, ws_form, prefill):
    """mstts_lsa_param_bwd + mstts_lsa_unfold_location_grad on prefilled accumulators; returns the raw outputs and the unfolded gradients."""
    dev, pr = L.dev, L.pr
    B, T, KS = pr["B"], pr["T"], pr["KS"]
    lb = lib.load()
    q, cum, de = (_f32(dev, hist[k]) for k in ("q", "cum", "d_e"))
    out = {k: v.clone() for k, v in prefill.items()}
    ws = None
    if ws_form:
        n = int(lb.mstts_lsa_param_bwd_ws_floats(B, T, S))
        ws = torch.full((n + GUARD,), NAN, device=dev)
        ws[n:] = 7.0
    lib.call("mstts_lsa_param_bwd", L.byref(), S, lib.ptr(q), lib.ptr(cum), lib.ptr(de), lib.ptr(out["d_keys"]), lib.ptr(out["d_loc_k"]),
             lib.ptr(out["d_score_w"]), lib.ptr(out["d_score_b"]), lib.ptr(ws))
    gk, gb, gd = torch.zeros(KS, CH, device=dev), torch.zeros(CH, device=dev), torch.zeros(CH, A, device=dev)
    lib.call("mstts_lsa_unfold_location_grad", L.c.conv_k, L.c.conv_b, L.c.dense_k, lib.ptr(out["d_loc_k"]), lib.ptr(out["d_score_b"]),
             lib.ptr(gk), lib.ptr(gb), lib.ptr(gd), KS, CH, A)
    torch.cuda.synchronize()
    if ws_form:
        assert bool((ws[n:] == 7.0).all()), "workspace written past mstts_lsa_param_bwd_ws_floats"
    raw = {k: t2n(v) for k, v in out.items()}
    return raw, dict(d_keys=raw["d_keys"], score_w=raw["d_score_w"], score_b=raw["d_score_b"], conv_k=t2n(gk), conv_b=t2n(gb), dense_k=t2n(gd))


_DIRECT = {}


def _param_direct(L, hist, key):
    """lsa_ref.param_bwd_direct on what the kernel reads: the fp32 keys, histories, score layer and the filter folded on the device (once a shape)."""
    if key not in _DIRECT:
        _DIRECT[key] = R.param_bwd_direct(t2n(L.keys), hist["q"], hist["cum"], hist["d_e"], t2n(L.loc_k), t2n(L.loc_b), t2n(L.v["score_w"]),
                                          t2n(L.v["score_b"]), key[3])
    return _DIRECT[key]


PARAM_TOL = dict(d_keys=TOL, dense_k=TOL, score_w=TOL, score_b=TOL, conv_k=TOL_CONV, conv_b=TOL_CONV)


@pytest.mark.parametrize("ws_form", [True, False], ids=["ws", "atomics"])
@pytest.mark.parametrize("B,T,S,KS,det", list(PARAM_GEOMETRY), ids=lambda v: str(int(v)))
def test_param_bwd_over_steps(dev, B, T, S, KS, det, ws_form):
    """mstts_lsa_param_bwd over S steps on the fp32-rounded histories of lsa_ref.chain, against lsa_ref.param_bwd_direct on exactly those
    arrays (and the kernel's own folded filter), unfolded by mstts_lsa_unfold_location_grad; every accumulator prefilled.  The geometry each
    case is there for is asserted from the kernel's formulas.  With the workspace (fp64 block reduction): 5e-5 for d_keys, the dense kernel,
    the score weight and bias, 1e-4 for the conv kernel and bias - test_lsa_step_fwd_bwd's bounds.  Without it (fp32 atomics): four times
    the largest error of three runs on an MI355X (ATOMIC_MEASURED), at most 5e-3.  Measured there: d_keys 1.3e-7 .. 6.2e-7; the other
    five tensors 1.5e-7 .. 3.0e-6 at the five small shapes and 2.7e-6 .. 9.4e-6 (conv bias) at (32, 128, 34, 31) with its 1536 partials per
    element - at these shapes the atomics cost nothing measurable over the workspace form (same figures to within 10 %).  Reproducibility as include/mstts.h promises: under
    lib.deterministic_gemm two runs agree bit for bit in all four outputs (workspace form; d_keys in the atomic form too), and the workspace form gives
    bit-identical d_loc_k, d_score_w, d_score_b in either mode."""
    lb = lib.load()
    nt, chunks, spb = _param_geometry(B, T, S, det)
    assert (nt, chunks, spb, S - (chunks - 1) * spb) == PARAM_GEOMETRY[(B, T, S, KS, det)]
    nt0, chunks0, _ = _param_geometry(B, T, S, False)
    assert int(lb.mstts_lsa_param_bwd_ws_floats(B, T, S)) == B * nt0 * chunks0 * LP_BLOCK + 2 * LP_GROUPS * LP_BLOCK
    if (B, T, S) == (32, 128, 34):
        assert B * nt * chunks == 1536
    if det:
        assert B * nt * chunks == 6 < LP_GROUPS and spb == S and T - PT == 5
    pr, hist = _param_ref(B, T, S, KS)
    L = _Lsa(dev, pr)
    d = _param_direct(L, hist, (B, T, S, KS))
    prefill = {k: _pattern(dev, d[k].shape, float(np.abs(d[k]).max())) for k in ("d_keys", "d_loc_k", "d_score_w", "d_score_b")}
    f32 = lambda k: t2n(L.v[k]).astype(np.float64)

    def unfolded(d_loc_k, d_b):
        return R.unfold_location_grad(f32("conv_k"), f32("conv_b"), f32("dense_k"), d_loc_k, d_b)

    pf = {k: t2n(v).astype(np.float64) for k, v in prefill.items()}
    pure = dict(d_keys=d["d_keys"], score_w=d["d_score_w"], score_b=d["d_score_b"], **unfolded(d["d_loc_k"], d["d_score_b"]))
    total = dict(d_keys=d["d_keys"] + pf["d_keys"], score_w=d["d_score_w"] + pf["d_score_w"], score_b=d["d_score_b"] + pf["d_score_b"],
                 **unfolded(d["d_loc_k"] + pf["d_loc_k"], d["d_score_b"] + pf["d_score_b"]))
    case = "%d-%d-%d-%d-%s" % (B, T, S, KS, "det" if det else "free")
    runs = []
    for _ in range(2 if ws_form else 3):
        if det:
            with lib.deterministic_gemm():
                runs.append(_run_param(L, hist, S, ws_form, prefill))
        else:
            runs.append(_run_param(L, hist, S, ws_form, prefill))
    worst = {k: max(_err(got[k], total[k], den_of=pure[k]) for _, got in runs) for k in PARAM_TOL}
    for k, e in worst.items():
        assert all(np.isfinite(got[k]).all() for _, got in runs), k
        print("param %s %s %-8s %.3e" % (case, "ws" if ws_form else "atomics", k, e))
    if ws_form:
        for k, e in worst.items():
            assert e < PARAM_TOL[k], (k, e, PARAM_TOL[k])
        same = ("d_keys", "d_loc_k", "d_score_w", "d_score_b") if det else ("d_loc_k", "d_score_w", "d_score_b")
    else:
        assert case in ATOMIC_MEASURED, "no measured bound for " + case
        for k, e in worst.items():
            bound = min(4.0 * ATOMIC_MEASURED[case][k], CAP)
            assert e < bound, (k, e, bound)
        same = ("d_keys",) if det else ()
    for k in same:
        assert np.array_equal(runs[0][0][k], runs[1][0][k]), k + " differs run to run"


# ---------------------------------------------------------------------------------------------------------------------------------
# 2d. the loop as mstts_decoder_train_bwd wires it
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _loop_ref():
    pr = R.loop_problem()
    return pr, R.chain(pr)


def _run_loop(L, ref, single):
    """Steps S - 1 .. 0 with G and h ping-ponged (NULL at the last step), d_ctx / d_ctx2 / the forward context as column blocks of the step
    histories, d_e into de_hist; then the parameter gradients (workspace form) and the unfold."""
    pr, dev = L.pr, L.dev
    B, T, M, KS, S, parts = pr["B"], pr["T"], pr["M"], pr["KS"], pr["S"], pr["parts"]
    WP, W0 = HH + M, M + HH
    slab = S * B * W0                                          # the decoder's slab stride: one d_in0 history per slab
    lb = lib.load()
    d_pj = _rows_in(dev, pr["d_ctx"], WP, HH)                  # [S, B, WP]
    pj = _rows_in(dev, ref["ctx"], WP, HH)
    d_in0 = _rows_in(dev, np.transpose(pr["slabs"], (1, 0, 2, 3)), W0, 0)      # [parts, S, B, W0]
    al, q, cum = _f32(dev, ref["align"]), _f32(dev, ref["q"]), _f32(dev, ref["cum"])
    G, h = [_Out(dev, B, T), _Out(dev, B, T)], [_Out(dev, B, T, HLD), _Out(dev, B, T, HLD)]
    da = _Out(dev, B, T)
    de_hist = _Out(dev, S, B, T)
    pre_dq = _pattern(dev, (S, B, A), float(np.abs(ref["dq"]).max()))
    dq_hist = pre_dq.clone()
    got = dict(G=[None] * S, h=[None] * S)
    cur = 0
    for st in range(S - 1, -1, -1):
        nxt, last = cur ^ 1, st == S - 1
        args = (L.byref(), lib.ptr(d_pj, st * B * WP + HH), WP, lib.ptr(d_in0, st * B * W0), W0, parts, slab,
                None if last else G[cur].ptr, None if last else h[cur].ptr, G[nxt].ptr)
        hist = (lib.ptr(al, st * B * T), lib.ptr(q, st * B * A), lib.ptr(cum, st * B * T))
        de, dq = de_hist.ptr + 4 * st * B * T, lib.ptr(dq_hist, st * B * A)
        if single:
            lib.call("mstts_lsa_step_bwd", *args, *hist, lib.ptr(pj, st * B * WP + HH), WP, de, dq, h[nxt].ptr)
        else:
            lib.call("mstts_lsa_dalign_bwd", *args, da.ptr)
            lib.call("mstts_lsa_denergy_bwd", L.byref(), hist[0], da.ptr, hist[1], hist[2], de, dq, h[nxt].ptr)
        torch.cuda.synchronize()
        got["G"][st], got["h"][st] = G[nxt].get("G"), h[nxt].get("h")
        cur = nxt
    got["d_e"] = de_hist.get("de_hist")
    got["dq"] = t2n(dq_hist).astype(np.float64) - t2n(pre_dq).astype(np.float64)
    got["G"], got["h"] = np.stack(got["G"]), np.stack(got["h"])
    dk = torch.zeros(B, T, A, device=dev)
    dlk, gw, gsb = torch.zeros(KS, A, device=dev), torch.zeros(A, device=dev), torch.zeros(A, device=dev)
    ws = torch.full((int(lb.mstts_lsa_param_bwd_ws_floats(B, T, S)),), NAN, device=dev)
    lib.call("mstts_lsa_param_bwd", L.byref(), S, lib.ptr(q), lib.ptr(cum), de_hist.ptr, lib.ptr(dk), lib.ptr(dlk), lib.ptr(gw), lib.ptr(gsb), lib.ptr(ws))
    gk, gb, gd = torch.zeros(KS, CH, device=dev), torch.zeros(CH, device=dev), torch.zeros(CH, A, device=dev)
    lib.call("mstts_lsa_unfold_location_grad", L.c.conv_k, L.c.conv_b, L.c.dense_k, lib.ptr(dlk), lib.ptr(gsb), lib.ptr(gk), lib.ptr(gb), lib.ptr(gd), KS, CH, A)
    torch.cuda.synchronize()
    got.update(d_keys=t2n(dk), score_w=t2n(gw), score_b=t2n(gsb), conv_k=t2n(gk), conv_b=t2n(gb), dense_k=t2n(gd))
    return got


LOOP_STEP_TENSORS = ("G", "d_e", "dq", "h")
LOOP_SUM_TENSORS = ("d_keys", "score_w", "score_b", "conv_k", "conv_b", "dense_k")


def test_loop_as_the_decoder_wires_it(dev):
    """Seven chained backward steps at (B, T, M, KS) = (3, 37, 48, 31) with three d_ctx2 slabs, wired as mstts_decoder_train_bwd wires
    them, then mstts_lsa_param_bwd and the unfold, against lsa_ref.chain's autograd step by step and tensor by tensor.  Only the forward
    histories are teacher-forced here: every step's G and h are the kernel's own, so errors compound through G and the bound is measured -
    four times the figure seen on an MI355X (LOOP_MEASURED: per tensor, the worst step and the worse form), at most 5e-3.  Measured there:
    G 4.2e-7, d_e 6.5e-7, dq 1.2e-6, h 7.4e-7, d_keys 4.7e-7, dense kernel 7.1e-7, score weight 4.3e-7, score bias 1.3e-6, conv kernel 5.9e-7,
    conv bias 5.7e-7 - seven steps compound to no more than one step's own error.  The last step's G is exactly zero.
    The two-launch loop agrees with the single-launch loop to 1e-5."""
    pr, ref = _loop_ref()
    S = pr["S"]
    L = _Lsa(dev, pr)
    one, two = _run_loop(L, ref, single=True), _run_loop(L, ref, single=False)
    g = ref["grads"]
    want = dict(ref, score_w=g["score_w"], score_b=g["score_b"], conv_k=g["conv_k"][:, 0, :], conv_b=g["conv_b"], dense_k=g["dense_k"])
    worst_of = {}
    for form, got in (("single-launch", one), ("two-launch", two)):
        assert (got["G"][S - 1] == 0.0).all() and (ref["G"][S - 1] == 0.0).all()
        assert (got["h"][..., pr["KS"]:] == 0.0).all()
        worst = worst_of[form] = {}
        for k in LOOP_STEP_TENSORS:
            per_step = [_err(got[k][s], want[k][s]) for s in range(S) if not (k == "G" and s == S - 1)]
            worst[k] = max(per_step)
            print("loop %s %-8s per step: %s" % (form, k, " ".join("%.2e" % e for e in per_step)))
        for k in LOOP_SUM_TENSORS:
            worst[k] = _err(got[k], want[k])
        for k, e in worst.items():
            print("loop %s %-8s %.3e" % (form, k, e))
    for form, worst in worst_of.items():
        for k, e in worst.items():
            assert k in LOOP_MEASURED, "no measured bound for " + k
            bound = min(4.0 * LOOP_MEASURED[k], CAP)
            assert e < bound, (form, k, e, bound)
    for k in LOOP_STEP_TENSORS + LOOP_SUM_TENSORS:
        if k == "G":
            _chk("loop forms G", two[k][:S - 1], one[k][:S - 1], TOL_FORMS)
        else:
            _chk("loop forms " + k, two[k], one[k], TOL_FORMS)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2e. the packed copy of the context
# ---------------------------------------------------------------------------------------------------------------------------------
def test_step_fwd_packed_context_copy(dev):
    """mstts_lsa_step_fwd's third copy of the context (ctx_p: columns col0 .. col0 + M - 1 of a fused cell's packed activation block, the
    layout of mstts_pack_cell_act): after the step, the block equals the packing of the row-major matrix with the kernel's own row-major
    context inserted - bit for bit, every other element of the block untouched."""
    B, T, M, KS = 3, 37, 48, 31
    K, col0 = 128, 64                                        # packed_dst_from: K % 64 == 0, K <= 2048, col0 + M <= K
    pr, _, _, ref = _step_ref(B, T, M, KS, 1, "short")
    L, lb = _Lsa(dev, pr), lib.load()
    n = int(lb.mstts_cell_act_floats(B, K))
    X = _f32(dev, 100.0 + np.arange(B * K).reshape(B, K))
    blocks = [torch.full((n + GUARD,), -5.0, device=dev) for _ in range(2)]
    for blk in blocks:
        lib.call("mstts_pack_cell_act", lib.ptr(X), K, lib.ptr(blk), B, K)
    assert torch.equal(blocks[0], blocks[1])
    q, cum = _f32(dev, ref["q"][0]), _f32(dev, ref["cum"][0])
    al, cn, cx = _Out(dev, B, T), _Out(dev, B, T), _Out(dev, B, M)
    gran = torch.zeros(int(lb.mstts_lsa_step_ws_bytes(B, T)) // 8, dtype=torch.int64, device=dev)
    dst = lib.CellPackedDst()
    dst.base, dst.K, dst.col0, dst.bf16 = lib.ptr(blocks[0]), K, col0, 0
    lib.call("mstts_lsa_step_fwd", L.byref(), lib.ptr(q), 1, 0, None, lib.ptr(cum), al.ptr, cn.ptr, cx.ptr, M, None, 0, C.byref(dst), lib.ptr(gran), 1)
    torch.cuda.synchronize()
    assert int(gran[-1]) == 0
    ctx = cx.get("ctx")
    _chk("ctx", ctx, ref["ctx"][0], TOL_G)
    _chk("align", al.get("align"), ref["align"][0], TOL_G)
    X[:, col0:col0 + M] = torch.tensor(ctx, device=dev)
    lib.call("mstts_pack_cell_act", lib.ptr(X), K, lib.ptr(blocks[1]), B, K)
    torch.cuda.synchronize()
    assert not torch.equal(blocks[0][:n], torch.full_like(blocks[0][:n], -5.0))
    assert torch.equal(blocks[0].view(torch.int32), blocks[1].view(torch.int32)), "%d packed elements differ" % int((blocks[0] != blocks[1]).sum())
    assert bool((blocks[0][n:] == -5.0).all())
