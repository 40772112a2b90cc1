"""mstts_bn_train_fwd_seg (nseg batch-norm layers side by side in one strided block, optional fused max-pool along time, optional statistics-only
form) against what it replaces: one mstts_bn_train_fwd call per segment on a contiguous copy, then mstts_maxpool2_same over the concatenation.
The bound is the one tests/test_gpu_ops.py::test_bn_dropout_fwd_bwd holds mstts_bn_train_fwd to against its reference."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from multi_speaker_tts_amd import lib
from tests.helpers import rel_err, t2n

pytestmark = pytest.mark.gpu
TOL = 2e-5
MOM, EPS = 0.99, 1e-3
NAN, SENTINEL = float("nan"), 777.0

# name -> (B, T, nseg, cseg, gap floats between rows, write y, float offset of x from a 16-byte boundary)
CASES = {
    "3x9_3x4": (3, 9, 3, 4, 0, True, 0),
    "one_row_8x128": (1, 1, 8, 128, 0, True, 0),
    "4x300_8x128_strided": (4, 300, 8, 128, 64, True, 0),          # more than one row block (16 rows each), ld > C
    "stats_only": (3, 9, 3, 4, 0, False, 0),
    "stats_only_strided": (4, 300, 8, 128, 64, False, 0),
    "unaligned_scalar": (3, 9, 3, 4, 0, True, 1),                  # x off the 16-byte grid: the scalar form
    "unaligned_scalar_strided": (2, 21, 2, 36, 3, True, 1),        # ... with an odd row stride and two row lanes' worth of rows
}


def _r(dev, *shape, seed=0, scale=1.0, mean=0.0):
    g = np.random.default_rng(seed)
    return torch.tensor(g.normal(mean, scale, size=shape), dtype=torch.float32, device=dev)


@functools.lru_cache(maxsize=None)
def _problem(name):
    """Inputs of a case and its reference, computed once: x as a dense [rows, C] tensor, per-segment parameters (separate allocations: not
    contiguous), and per segment mstts_bn_train_fwd's batch statistics / moving statistics / normalised output."""
    B, T, nseg, cseg, gap, _, _ = CASES[name]
    dev = torch.device("cuda:0")
    rows, Cc = B * T, nseg * cseg
    x = _r(dev, rows, Cc, seed=1, scale=1.5, mean=0.3)
    seg = [dict(gamma=_r(dev, cseg, seed=10 + i) + 1.5, beta=_r(dev, cseg, seed=30 + i), mm=_r(dev, cseg, seed=50 + i),
                mv=_r(dev, cseg, seed=70 + i).abs() + 0.5) for i in range(nseg)]
    ref = dict(mean=[], rstd=[], mm=[], mv=[], z=[])
    ws = torch.zeros(2 * cseg, device=dev)
    for i, s in enumerate(seg):
        xs = x[:, i * cseg:(i + 1) * cseg].contiguous()
        y, sm, sr = torch.zeros_like(xs), torch.zeros(cseg, device=dev), torch.zeros(cseg, device=dev)
        mm, mv = s["mm"].clone(), s["mv"].clone()
        lib.call("mstts_bn_train_fwd", lib.ptr(xs), lib.ptr(s["gamma"]), lib.ptr(s["beta"]), lib.ptr(mm), lib.ptr(mv), lib.ptr(y), lib.ptr(sm),
                 lib.ptr(sr), None, 1.0, MOM, EPS, rows, cseg, lib.ptr(ws))
        for k, v in (("mean", sm), ("rstd", sr), ("mm", mm), ("mv", mv), ("z", y)):
            ref[k].append(v)
    z = torch.cat(ref["z"], dim=1).contiguous()
    pooled = torch.zeros_like(z)
    lib.call("mstts_maxpool2_same", lib.ptr(z), lib.ptr(pooled), B, T, Cc)
    torch.cuda.synchronize()
    out = {k: t2n(torch.cat(v)) for k, v in ref.items() if k != "z"}
    out.update(z=t2n(z), pooled=t2n(pooled))
    return x, seg, out


def _run(name, pool):
    """One mstts_bn_train_fwd_seg call of the case from the problem's initial state; NaN in the gaps of x and behind it, a sentinel behind every output."""
    B, T, nseg, cseg, gap, want_y, off = CASES[name]
    x, seg, _ = _problem(name)
    dev = x.device
    rows, Cc = B * T, nseg * cseg
    ld = Cc + gap
    xb = torch.full((off + rows * ld + 8,), NAN, device=dev)
    xb[off:off + rows * ld].view(rows, ld)[:, :Cc] = x
    mm, mv = [s["mm"].clone() for s in seg], [s["mv"].clone() for s in seg]
    tab = lib.BnSegTable()
    for i, s in enumerate(seg):
        tab.seg[i].gamma, tab.seg[i].beta = lib.ptr(s["gamma"]), lib.ptr(s["beta"])
        tab.seg[i].moving_mean, tab.seg[i].moving_var = lib.ptr(mm[i]), lib.ptr(mv[i])
    y = torch.full((rows * Cc + 8,), SENTINEL, device=dev)
    stat = torch.full((2 * Cc + 8,), SENTINEL, device=dev)
    ws = torch.full((4 * Cc + 8,), SENTINEL, device=dev)
    lib.call("mstts_bn_train_fwd_seg", lib.ptr(xb, off), ld, C.byref(tab), nseg, lib.ptr(y) if want_y else None, lib.ptr(stat), lib.ptr(stat, Cc),
             MOM, EPS, rows, Cc, T if pool else 0, lib.ptr(ws))
    torch.cuda.synchronize()
    assert bool((y[rows * Cc:] == SENTINEL).all()) and bool((stat[2 * Cc:] == SENTINEL).all()) and bool((ws[4 * Cc:] == SENTINEL).all())
    if not want_y:
        assert bool((y == SENTINEL).all()) and bool((ws[2 * Cc:] == SENTINEL).all())        # statistics only: 2 C floats of scratch, y untouched
    assert bool(torch.isnan(xb[:off]).all()) and bool(torch.isnan(xb[off + rows * ld:]).all())
    return dict(mean=t2n(stat[:Cc]), rstd=t2n(stat[Cc:2 * Cc]), mm=t2n(torch.cat(mm)), mv=t2n(torch.cat(mv)),
                y=t2n(y[:rows * Cc]).reshape(rows, Cc) if want_y else None)


# (the pool is part of the apply pass: the statistics-only cases have nothing to pool)
@pytest.mark.parametrize("name,pool", [(n, p) for n in sorted(CASES) for p in (False, True) if CASES[n][5] or not p])
def test_bn_seg_against_per_segment_calls(dev, name, pool):
    B, T, nseg, cseg, gap, want_y, off = CASES[name]
    _, _, ref = _problem(name)
    got = _run(name, pool)
    for k in ("mean", "rstd", "mm", "mv"):
        e = rel_err(got[k], ref[k])
        print("%s pool=%d %s: %.3g" % (name, pool, k, e))
        assert np.isfinite(got[k]).all() and e < TOL, (k, e)
    if want_y:
        e = rel_err(got["y"], ref["pooled"] if pool else ref["z"])
        print("%s pool=%d y: %.3g" % (name, pool, e))
        assert np.isfinite(got["y"]).all() and e < TOL, e


@pytest.mark.parametrize("name", ["3x9_3x4", "4x300_8x128_strided", "unaligned_scalar_strided"])
def test_bn_seg_deterministic_mode(dev, name):
    """Under mstts_gemm_deterministic the column sums take their one-add-per-element form: two calls are bit-identical, with the pool and
    without.  The statistics of the pooled and the plain call are then the same bits too, so the pool's rule can be checked exactly: the last
    frame of every batch row is its own normalised value, every other frame the larger of its own and its successor's."""
    B, T, nseg, cseg, _, _, _ = CASES[name]
    with lib.deterministic_gemm():
        a, b = _run(name, True), _run(name, True)
        plain, plain2 = _run(name, False), _run(name, False)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(plain[k], plain2[k]), k
    for k in ("mean", "rstd", "mm", "mv"):
        assert np.array_equal(a[k], plain[k]), k
    z, y = plain["y"].reshape(B, T, -1), a["y"].reshape(B, T, -1)
    assert np.array_equal(y[:, -1], z[:, -1])
    assert np.array_equal(y[:, :-1], np.maximum(z[:, :-1], z[:, 1:]))
