"""Op-level checks of the glue kernels around the hard ones (csrc/elementwise.hip, the inference pointwise kernels of csrc/waveglow.hip, the
exported pair forms) and of the row-keyed mask generator, each against a plain fp64 / NumPy statement of the same operation written here.

Rules of every case: outputs are NaN-filled (uint8: 0xAB) before the call; an output written through a stride or an offset sits inside a
larger sentinel-filled allocation and everything outside the specified region must be unchanged; data movement is compared bit for bit,
arithmetic with helpers.rel_err against fp64 at TOL (what tests/test_gpu_ops.py uses for this family).  Sizes past the launch caps
(grid_for: 2048 x 256 threads, wg_grid: 8192 x 256) make the second trip of every grid-stride loop part of the comparison."""
import ctypes as C

import numpy as np
import pytest
import torch

from multi_speaker_tts_amd import lib, masks
from oracle import rng as orng, train as OT
from tests.helpers import dims_pair, rel_err, t2n

pytestmark = pytest.mark.gpu
TOL = 2e-5
CAP = 2048 * 256                 # grid_for: threads of the largest launch
WG_CAP = 8192 * 256              # wg_grid
NBIG = 4 * CAP + 1031            # past the cap for one-element-per-thread and for float4 kernels alike; n % 4 == 3
SEED = 0x9E3779B97F4A7C15        # both key words nonzero
NAN = float("nan")


def _r(dev, *shape, seed=0, scale=1.0, mean=0.0):
    g = np.random.default_rng(seed)
    return torch.tensor(g.normal(mean, scale, size=shape), dtype=torch.float32, device=dev)


def _nan(dev, *shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=dev)


def _f64(t):
    return t2n(t).astype(np.float64)


def _bits(dev, *shape, seed=0, p=0.5):
    return torch.tensor((np.random.default_rng(seed).random(shape) < p).astype(np.uint8), device=dev)


def _chk(what, got, ref, tol=TOL):
    got = t2n(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = t2n(ref) if isinstance(ref, torch.Tensor) else np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    e = rel_err(got, ref)
    print("%s: %.3e" % (what, e))
    assert np.isfinite(got).all(), what + ": NaN / inf in the output (an element was not written?)"
    assert e < tol, (what, e)
    return e


def _same(what, got, ref):
    got = t2n(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = t2n(ref) if isinstance(ref, torch.Tensor) else np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    assert np.array_equal(got, ref), "%s: %d of %d elements differ" % (what, int((got != ref).sum()), got.size)


# ---------------------------------------------------------------------------------------------------------------------------------
# keep masks
# ---------------------------------------------------------------------------------------------------------------------------------
def _rows_ref(outer, B, inner, seed, stream, sample0, keep):
    if outer == 1:                       # batch-major [B, inner]
        return orng.keep_mask_rows((B, 1, inner), 0, seed, stream, sample0, keep).reshape(-1)
    return orng.keep_mask_rows((outer, B, inner), 1, seed, stream, sample0, keep).reshape(-1)


ROWS_SHAPES = [(1, 4, 21 * 32),          # batch-major, uchar4 path
               (1, 3, 7 * 9),            # batch-major, scalar path, n % 4 == 3
               (13, 5, 32),
               (13, 5, 30),              # scalar path, a four-draw block straddles two rows of `outer`
               (2, 1, 1),
               (900, 32, 80)]            # 18 000 draw blocks x 32 samples = 576 000 > 524 288 threads: second grid-stride trip


@pytest.mark.parametrize("keep", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("sample0", [0, 7, 2 ** 32 - 2])
@pytest.mark.parametrize("outer,B,inner", ROWS_SHAPES)
def test_philox_keep_mask_rows_bit_exact(dev, outer, B, inner, sample0, keep):
    """mstts_philox_keep_mask_rows against oracle.rng.keep_mask_rows (tests/test_cpu_rng_rows.py pins that reference): both paths, both
    layouts, nonzero first sample (every rank above 0) up to the 32-bit wrap of the sample counter, a 64-bit seed, more draw blocks than
    the launch has threads; the bytes behind the mask keep the sentinel."""
    n = outer * B * inner
    assert (outer, B, inner) != (900, 32, 80) or ((outer * inner + 3) // 4) * B > CAP
    buf = torch.full(((n + 3) // 4 * 4 + 64,), 0xAB, dtype=torch.uint8, device=dev)
    lib.call("mstts_philox_keep_mask_rows", lib.ptr(buf), outer, B, inner, SEED, 41, sample0, keep)
    got = t2n(buf)
    ref = _rows_ref(outer, B, inner, SEED, 41, sample0, keep)
    _same("mask", got[:n], ref)
    assert (got[n:] == 0xAB).all()
    if n > 1000:
        assert abs(float(ref.mean()) - keep) < 0.05          # (the reference is a Bernoulli(keep) draw, not a constant)


def test_philox_keep_mask_rows_low_seed_and_rejections(dev):
    """A seed with a zero high word draws another mask than the same low word under a nonzero high word (the high word is key word 1);
    host-side rejections: a vector-path mask on a pointer that is not 4-byte aligned, a negative extent."""
    out = []
    for seed in (1234, 1234 + (5 << 32)):
        buf = torch.full((13 * 5 * 32 + 64,), 0xAB, dtype=torch.uint8, device=dev)
        lib.call("mstts_philox_keep_mask_rows", lib.ptr(buf), 13, 5, 32, seed, 3, 0, 0.5)
        _same("mask", t2n(buf)[:13 * 5 * 32], _rows_ref(13, 5, 32, seed, 3, 0, 0.5))
        out.append(t2n(buf))
    assert not np.array_equal(out[0], out[1])
    L = lib.load()
    buf = torch.full((256,), 0xAB, dtype=torch.uint8, device=dev)
    assert L.mstts_philox_keep_mask_rows(lib.ptr(buf, 1), 2, 3, 8, 1, 1, 0, 0.5, lib.stream()) != 0
    assert L.mstts_philox_keep_mask_rows(lib.ptr(buf), -1, 3, 8, 1, 1, 0, 0.5, lib.stream()) != 0
    assert L.mstts_philox_keep_mask(lib.ptr(buf, 1), 8, 1, 1, 0.5, lib.stream()) != 0
    torch.cuda.synchronize()
    assert (t2n(buf) == 0xAB).all()


def test_maskset_draw_is_the_oracles_masks_on_rank_1(dev):
    """masks.MaskSet(rank=1).draw: every buffer of a training-shape table (vocoder and speaker stack included; prenet width 18 and vocoder
    width 6 are not multiples of 4) equals oracle.train.make_masks for that rank, and the pad bytes of each buffer keep the sentinel."""
    pd, od = dims_pair(prenet=18, birnn=6)
    B, T_enc, S, W = 3, 7, 5, 5                  # 5 x 3 x 18 and 5 x 3 x 6 bytes: lengths that are not multiples of 4 either
    raw = []

    def alloc(nbytes):
        raw.append(torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=dev))
        return raw[-1]
    ms = masks.MaskSet(pd, B, T_enc, S, True, dev, rank=1, alloc=alloc, vocoder=True, speaker_windows=W)
    seed = OT.step_seed(SEED, 3)
    ms.draw(seed)
    ref = OT.make_masks(od, B, T_enc, S, True, seed=seed, rank=1, vocoder=True, speaker_windows=W)
    assert set(ref) == set(ms.buf) and len(ref) == len(raw) and any(int(np.prod(v.shape)) % 4 for v in ref.values())
    for (name, _, shape, _), store in zip(ms.spec, raw):
        n = int(np.prod(shape))
        _same(name, ms[name], ref[name].numpy().reshape(shape))
        assert (t2n(store)[n:] == 0xAB).all(), name
    rank0 = OT.make_masks(od, B, T_enc, S, True, seed=seed, rank=0, vocoder=True, speaker_windows=W)
    assert not np.array_equal(rank0["dec_zc_0"].numpy(), ref["dec_zc_0"].numpy())


def test_philox_keep_mask_past_the_cap(dev):
    n = 4 * CAP + 5                      # 524 290 draw blocks, 524 288 threads; the last block is a one-element tail
    buf = torch.full(((n + 3) // 4 * 4 + 64,), 0xAB, dtype=torch.uint8, device=dev)
    lib.call("mstts_philox_keep_mask", lib.ptr(buf), n, SEED, 9, 0.9)
    got = t2n(buf)
    _same("mask", got[:n], orng.keep_mask((n,), SEED, 9, 0.9))
    assert (got[n:] == 0xAB).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# flat elementwise kernels, second trip of the grid-stride loop included
# ---------------------------------------------------------------------------------------------------------------------------------
def test_add_past_the_cap(dev):
    a, b, y = _r(dev, NBIG, seed=1), _r(dev, NBIG, seed=2), _nan(dev, NBIG + 8)
    lib.call("mstts_add", lib.ptr(a), lib.ptr(b), lib.ptr(y), NBIG)
    _chk("add", y[:NBIG], _f64(a) + _f64(b))
    assert np.isnan(t2n(y[NBIG:])).all()


def test_dropout_and_relu_dropout_bwd_past_the_cap(dev):
    """keep = 0.5: 1 / keep is exact, so y = mask ? 2 x : 0 bit for bit; keep = 0.8 against fp64."""
    x, dy, m = _r(dev, NBIG, seed=1), _r(dev, NBIG, seed=2), _bits(dev, NBIG, seed=3)
    mn = t2n(m).astype(bool)
    y = _nan(dev, NBIG + 8)
    lib.call("mstts_dropout", lib.ptr(x), lib.ptr(m), 0.5, lib.ptr(y), NBIG)
    _same("dropout", y[:NBIG], np.where(mn, t2n(x) * np.float32(2), np.float32(0)))
    assert np.isnan(t2n(y[NBIG:])).all()
    y8 = _nan(dev, NBIG)
    lib.call("mstts_dropout", lib.ptr(x), lib.ptr(m), 0.8, lib.ptr(y8), NBIG)
    _chk("dropout keep 0.8", y8, np.where(mn, _f64(x) / 0.8, 0.0))
    ys = torch.relu(_r(dev, NBIG, seed=4))
    dx = _nan(dev, NBIG + 8)
    lib.call("mstts_relu_dropout_bwd", lib.ptr(dy), lib.ptr(ys), lib.ptr(m), 0.5, lib.ptr(dx), NBIG)
    _same("relu_dropout_bwd", dx[:NBIG], np.where(mn & (t2n(ys) > 0), t2n(dy) * np.float32(2), np.float32(0)))
    assert np.isnan(t2n(dx[NBIG:])).all()
    dx8 = _nan(dev, NBIG)
    lib.call("mstts_relu_dropout_bwd", lib.ptr(dy), lib.ptr(ys), lib.ptr(m), 0.8, lib.ptr(dx8), NBIG)
    _chk("relu_dropout_bwd keep 0.8", dx8, np.where(mn & (t2n(ys) > 0), _f64(dy) / 0.8, 0.0))


@pytest.mark.parametrize("off", [4, 5])         # 16-byte aligned start (float4 body + scalar tail) / one float further (all scalar)
@pytest.mark.parametrize("n", [1, 3, 4, 4099, NBIG])
def test_fill(dev, n, off):
    y = _nan(dev, n + 16)
    lib.call("mstts_fill", lib.ptr(y, off), -2.5, n)
    got = t2n(y)
    _same("fill", got[off:off + n], np.full(n, -2.5, np.float32))
    assert np.isnan(got[:off]).all() and np.isnan(got[off + n:]).all()


def test_highway_combine_fwd_bwd_past_the_cap(dev):
    n = NBIG
    hp, tp, x, dy = _r(dev, n, seed=1), _r(dev, n, seed=2, scale=2.0), _r(dev, n, seed=3), _r(dev, n, seed=4)
    y = _nan(dev, n)
    lib.call("mstts_highway_combine", lib.ptr(hp), lib.ptr(tp), lib.ptr(x), lib.ptr(y), n)
    h, t, xs, g = _f64(hp), _f64(tp), _f64(x), _f64(dy)
    H, T = np.maximum(h, 0.0), 1.0 / (1.0 + np.exp(-t))
    _chk("highway_combine", y, H * T + xs * (1.0 - T))
    dh, dt, dx = _nan(dev, n), _nan(dev, n), _nan(dev, n)
    lib.call("mstts_highway_combine_bwd", lib.ptr(hp), lib.ptr(tp), lib.ptr(x), lib.ptr(dy), lib.ptr(dh), lib.ptr(dt), lib.ptr(dx), n)
    _chk("highway dh", dh, np.where(h > 0, g * T, 0.0))
    _chk("highway dt", dt, g * (H - xs) * T * (1.0 - T))
    _chk("highway dx", dx, g * (1.0 - T))


def test_maxpool2_same_fwd_bwd_past_the_cap(dev):
    """[32, 801, 82] with inputs rounded to one decimal: ties between neighbours are common, the gradient goes to the first maximum."""
    B, T, Cc = 32, 801, 82
    assert B * T * Cc > CAP
    x = torch.round(_r(dev, B, T, Cc, seed=1) * 10) / 10
    dy = _r(dev, B, T, Cc, seed=2)
    y, dx = _nan(dev, B, T, Cc), _nan(dev, B, T, Cc)
    lib.call("mstts_maxpool2_same", lib.ptr(x), lib.ptr(y), B, T, Cc)
    xn, g = t2n(x), _f64(dy)
    nxt = np.concatenate([xn[:, 1:], np.full_like(xn[:, :1], -np.inf)], 1)
    _same("maxpool2_same", y, np.maximum(xn, nxt))
    lib.call("mstts_maxpool2_same_bwd", lib.ptr(x), lib.ptr(dy), lib.ptr(dx), B, T, Cc)
    assert int((xn[:, :-1] == xn[:, 1:]).sum()) > 1000
    ref = np.where(xn >= nxt, g, 0.0)                                   # window t = {t, t + 1}: x[t] takes it on >= (alone at the end)
    ref[:, 1:] += np.where(xn[:, 1:] > xn[:, :-1], g[:, :-1], 0.0)      # window t - 1: x[t] takes it only when strictly larger
    _chk("maxpool2_same_bwd", dx, ref)


def test_adam_tf_past_the_cap(dev):
    n = NBIG
    p, g = _r(dev, n, seed=1), _r(dev, n, seed=2)
    m, v = _r(dev, n, seed=3) * 0.1, torch.abs(_r(dev, n, seed=4)) * 0.01
    wd = _bits(dev, n, seed=5)
    pn, gn, mn, vn = [_f64(t) for t in (p, g, m, v)]
    lib.call("mstts_adam_tf", lib.ptr(p), lib.ptr(g), lib.ptr(m), lib.ptr(v), lib.ptr(wd), 1e-6, 0.5, 3e-4, 0.9, 0.999, 1e-6, n)
    gt = gn * 0.5 + 1e-6 * pn * t2n(wd)
    mr = 0.9 * mn + 0.1 * gt; vr = 0.999 * vn + 0.001 * gt * gt
    _chk("adam p", p, pn - 3e-4 * mr / (np.sqrt(vr) + 1e-6)); _chk("adam m", m, mr); _chk("adam v", v, vr)


def test_l1_and_l2_losses_past_the_cap(dev):
    """Long fp32 sums (2 098 183 terms: per-thread strided partials, a block sum, one atomic per block) against fp64 at TOL (measured: 5e-7 at
    most, so no wider bound is stated); exact ties of
    the L1 term get gradient 0; the L2 sum ADDS to its output (with and without a mask)."""
    n = NBIG
    p, t = _r(dev, n, seed=1), _r(dev, n, seed=2)
    p[::1000] = t[::1000]
    loss, dp = _nan(dev, 1), _nan(dev, n)
    lib.call("mstts_l1_loss_fwd_bwd", lib.ptr(p), lib.ptr(t), n, lib.ptr(loss), lib.ptr(dp))
    d = _f64(p) - _f64(t)
    _chk("l1 loss", loss, np.array([np.abs(d).mean()]))
    _chk("l1 d_pred", dp, np.sign(d) / n)
    assert (t2n(dp)[::1000] == 0).all()
    loss2 = _nan(dev, 1)
    lib.call("mstts_l1_loss_fwd_bwd", lib.ptr(p), lib.ptr(t), n, lib.ptr(loss2), None)
    _chk("l1 loss, no gradient", loss2, np.array([np.abs(d).mean()]))
    m = _bits(dev, n, seed=3, p=0.3)
    for mask in (None, m):
        out = torch.full((1,), 1.5, device=dev)
        lib.call("mstts_l2_loss_acc", lib.ptr(p), lib.ptr(mask), n, lib.ptr(out))
        sq = _f64(p) ** 2
        _chk("l2 loss", out, np.array([1.5 + 0.5 * (sq if mask is None else sq * t2n(m)).sum()]))


@pytest.mark.parametrize("rows,cols,lds,ldd", [(7, 5, 9, 11), (1, 1, 3, 2), (1, 5, 6, 8), (6, 1, 2, 3), (1024 + 768, 81, 81, 128), (4100, 129, 131, 130)])
@pytest.mark.parametrize("acc", [0, 1])
def test_copy2d(dev, rows, cols, lds, ldd, acc):
    """dst[r * ldd + c] (+)= src[r * lds + c]: lds != ldd != cols, one row, one column, the engine's [H + M, n_mel + 1] block into its 128-wide
    pad, 528 900 elements (past the cap); everything of dst outside the [rows, cols] window is unchanged."""
    src = _r(dev, rows, lds, seed=1)
    base = _r(dev, rows, ldd, seed=2) if acc else _nan(dev, rows, ldd)
    dst = base.clone()
    lib.call("mstts_copy2d", lib.ptr(src), lds, lib.ptr(dst), ldd, rows, cols, acc)
    got, b0 = t2n(dst), t2n(base)
    if acc:
        _chk("copy2d accumulate", got[:, :cols], b0[:, :cols].astype(np.float64) + _f64(src)[:, :cols])
        _same("outside", got[:, cols:], b0[:, cols:])
    else:
        _same("copy2d", got[:, :cols], t2n(src)[:, :cols])
        assert np.isnan(got[:, cols:]).all()


@pytest.mark.parametrize("D0,D1,Cc", [(3, 5, 7), (1, 4, 1), (37, 111, 512)])
def test_transpose01(dev, D0, D1, Cc):
    src, dst = _r(dev, D0, D1, Cc, seed=1), _nan(dev, D1, D0, Cc)
    lib.call("mstts_transpose01", lib.ptr(src), lib.ptr(dst), D0, D1, Cc)
    _same("transpose01", dst, np.ascontiguousarray(t2n(src).transpose(1, 0, 2)))


def test_shift_frames_and_conv_kernel_flip_past_the_cap(dev):
    B, L, Cc = 32, 800, 82
    mel, fr = _r(dev, B, L, Cc, seed=1), _nan(dev, L + 1, B, Cc)
    lib.call("mstts_shift_frames", lib.ptr(mel), lib.ptr(fr), B, L, Cc)
    _same("shift_frames", fr, np.concatenate([np.zeros((1, B, Cc), np.float32), t2n(mel).transpose(1, 0, 2)], 0))
    K, cin, cout = 5, 130, 1024
    assert K * cin * cout > CAP
    w, wt = _r(dev, K, cin, cout, seed=2), _nan(dev, K, cout, cin)
    lib.call("mstts_conv_kernel_flip", lib.ptr(w), lib.ptr(wt), K, cin, cout)
    _same("conv_kernel_flip", wt, np.ascontiguousarray(t2n(w)[::-1].transpose(0, 2, 1)))      # wt[K-1-k][o][c] = w[k][c][o]


def test_embedding_fwd_bwd_past_the_cap(dev):
    n, vocab, width = 8200, 42, 256                # 524 800 float4 gathers; 2 099 200 scatter-adds, ~195 rows per table entry
    assert n * width // 4 > CAP
    tab = _r(dev, vocab, width, seed=1)
    tok = torch.tensor(np.random.default_rng(2).integers(0, vocab, size=n), dtype=torch.int32, device=dev)
    out = _nan(dev, n, width)
    lib.call("mstts_embedding_fwd", lib.ptr(tok), lib.ptr(tab), lib.ptr(out), n, vocab, width)
    _same("embedding_fwd", out, t2n(tab)[t2n(tok)])
    dout, dt = _r(dev, n, width, seed=3), _r(dev, vocab, width, seed=4)
    ref = _f64(dt); np.add.at(ref, t2n(tok), _f64(dout))
    lib.call("mstts_embedding_bwd", lib.ptr(tok), lib.ptr(dout), lib.ptr(dt), n, vocab, width)
    _chk("embedding_bwd", dt, ref)


@pytest.mark.parametrize("width", [64, 100])
def test_embedding_bwd_fixed_order(dev, width):
    """The fixed-order scatter-add of mstts_gemm_deterministic(1) (one thread per table column walks the rows) with repeated tokens, onto a
    pre-filled table, against np.add.at in fp64 - and bit-equal from run to run."""
    n, vocab = 300, 17
    tok = torch.tensor(np.random.default_rng(2).integers(0, vocab, size=n), dtype=torch.int32, device=dev)
    assert len(np.unique(t2n(tok))) < n
    dout, dt0 = _r(dev, n, width, seed=3), _r(dev, vocab, width, seed=4)
    ref = _f64(dt0); np.add.at(ref, t2n(tok), _f64(dout))
    outs = []
    with lib.deterministic_gemm():
        for _ in range(2):
            dt = dt0.clone()
            lib.call("mstts_embedding_bwd", lib.ptr(tok), lib.ptr(dout), lib.ptr(dt), n, vocab, width)
            outs.append(t2n(dt))
    _chk("embedding_bwd fixed order", outs[0], ref)
    _same("second run", outs[1], outs[0])


def test_bf16_conversions_past_the_cap(dev):
    x = _r(dev, NBIG, seed=1) * torch.logspace(-6, 3, NBIG, device=dev)
    y = torch.full((NBIG + 8,), NAN, dtype=torch.bfloat16, device=dev)
    lib.call("mstts_f32_to_bf16", lib.ptr(x), lib.ptr(y), NBIG)
    assert torch.equal(y[:NBIG], x.to(torch.bfloat16)) and bool(torch.isnan(y[NBIG:]).all())
    z = _nan(dev, NBIG + 8)
    lib.call("mstts_bf16_to_f32", lib.ptr(y), lib.ptr(z), NBIG)
    assert torch.equal(z[:NBIG], y[:NBIG].float()) and bool(torch.isnan(z[NBIG:]).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# decoder layout glue
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,Cc,ldp", [(1, 2, 4, 8), (5, 13, 80, 128), (2, 3, 4, 5)])
def test_unpack_proj_pack_dproj(dev, B, S, Cc, ldp):
    """proj [S, B, ldp] (columns 0..C-1 linear, column C stop, pad behind) <-> linear [B, S, C], stop [B, S]; pack writes exact zeros into
    the pad columns of a NaN-filled destination; pack then unpack is the identity."""
    proj = _r(dev, S, B, ldp, seed=1)
    lin, stop = _nan(dev, B, S, Cc), _nan(dev, B, S)
    lib.call("mstts_unpack_proj", lib.ptr(proj), ldp, lib.ptr(lin), lib.ptr(stop), B, S, Cc)
    pn = t2n(proj)
    _same("linear", lin, np.ascontiguousarray(pn[:, :, :Cc].transpose(1, 0, 2)))
    _same("stop", stop, np.ascontiguousarray(pn[:, :, Cc].T))
    dlin, dstop = _r(dev, B, S, Cc, seed=2), _r(dev, B, S, seed=3)
    dproj = _nan(dev, S, B, ldp)
    lib.call("mstts_pack_dproj", lib.ptr(dlin), lib.ptr(dstop), lib.ptr(dproj), ldp, B, S, Cc)
    ref = np.zeros((S, B, ldp), np.float32)
    ref[:, :, :Cc] = t2n(dlin).transpose(1, 0, 2); ref[:, :, Cc] = t2n(dstop).T
    _same("d_proj", dproj, ref)
    assert ldp == Cc + 1 or (t2n(dproj)[:, :, Cc + 1:] == 0).all()
    lin2, stop2 = _nan(dev, B, S, Cc), _nan(dev, B, S)
    lib.call("mstts_unpack_proj", lib.ptr(dproj), ldp, lib.ptr(lin2), lib.ptr(stop2), B, S, Cc)
    _same("round trip linear", lin2, t2n(dlin)); _same("round trip stop", stop2, t2n(dstop))


@pytest.mark.parametrize("with_len", [True, False])
@pytest.mark.parametrize("B,T,M,off,width", [(3, 7, 24, 8, 6), (1, 1, 3, 0, 2), (4, 9, 40, 5, 33)])
def test_speaker_tile(dev, B, T, M, off, width, with_len):
    """values[b, t, off + j] = (t < lengths[b]) ? spk[b, j] : 0, columns outside [off, off + width) untouched (off + width < M)."""
    assert off + width < M
    spk = _r(dev, B, width, seed=1)
    ln = np.array(([T, 0, 3, T + 2] * B)[:B], np.int32)
    values, lens = _nan(dev, B, T, M), torch.tensor(ln, device=dev)
    lib.call("mstts_speaker_tile", lib.ptr(spk), lib.ptr(lens) if with_len else None, lib.ptr(values), B, T, M, off, width)
    got = t2n(values)
    live = (np.arange(T)[None, :] < ln[:, None]) if with_len else np.ones((B, T), bool)
    _same("tile", got[:, :, off:off + width], np.where(live[:, :, None], t2n(spk)[:, None, :], np.float32(0)).astype(np.float32))
    assert np.isnan(got[:, :, :off]).all() and np.isnan(got[:, :, off + width:]).all()


@pytest.mark.parametrize("B,samples,T,E", [(1, 1, 1, 4), (3, 5, 7, 32), (9, 5, 3, 256)])
def test_speaker_finalize(dev, B, samples, T, E):
    """Mean over `samples` of the last frame, then ONE L2 norm over the whole [B, E] block (tf.nn.l2_normalize with axis=None - which is
    also what oracle.model.speaker_encoder does); B * E = 2304 makes the single 1024-thread workgroup loop; an all-zero input meets the
    1e-12 floor and gives zeros."""
    x, out = _r(dev, B * samples, T, E, seed=1), _nan(dev, B, E)
    lib.call("mstts_speaker_finalize", lib.ptr(x), lib.ptr(out), B, samples, T, E)
    e = _f64(x)[:, -1, :].reshape(B, samples, E).mean(1)
    _chk("speaker_finalize", out, e / np.sqrt(max((e * e).sum(), 1e-12)))
    _chk("unit norm", np.array([float((_f64(out) ** 2).sum())]), np.array([1.0]))
    z, x0 = _nan(dev, B, E), torch.zeros_like(x)
    lib.call("mstts_speaker_finalize", lib.ptr(x0), lib.ptr(z), B, samples, T, E)
    assert (t2n(z) == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# loss
# ---------------------------------------------------------------------------------------------------------------------------------
def _tts_loss_ref(lin, post, mel, stop, mlen, use_l1, gs):
    """oracle.train.losses (MSTTS_SV.py:127-144) and its gradient, in fp64."""
    B, S, nm = lin.shape
    L = S - 1
    out, grads = [], []
    for p in (lin, post):
        e = p[:, :L] - mel
        val = (e * e).mean() + (np.abs(e).mean() if use_l1 else 0.0)
        g = np.zeros_like(p)
        g[:, :L] = (2.0 * e + (np.sign(e) if use_l1 else 0.0)) / e.size
        out.append(val); grads.append(g * gs)
    y = (np.arange(S)[None, :] >= mlen[:, None]).astype(np.float64)
    out.append((np.maximum(stop, 0.0) - stop * y + np.log1p(np.exp(-np.abs(stop)))).mean())
    grads.append((1.0 / (1.0 + np.exp(-stop)) - y) / stop.size * gs)
    return np.array(out), grads


@pytest.mark.parametrize("gs", [1.0, 0.125])
@pytest.mark.parametrize("use_l1", [0, 1])
@pytest.mark.parametrize("B,S,nm", [(3, 7, 8), (2, 2, 5), (32, 801, 80)])
def test_tts_loss_fwd_bwd(dev, B, S, nm, use_l1, gs):
    """mstts_tts_loss_fwd_bwd against the oracle's loss definition in fp64: ragged mel_length with 0 and >= S among them, S = 2, exact ties
    lin == mel (sign term 0), stop logits of +-40, [32, 801, 80] (2 050 560 elements: past the cap, the three scalars each the sum of 2048
    atomics of 256-thread block sums of 4-term partials - measured 6e-7 against fp64, so plain TOL holds and no wider bound is stated); the gradient of the last step is
    exactly 0; the scalars ADD to what the buffer holds (include/mstts.h: "accumulated atomically: zero them first")."""
    L = S - 1
    g = np.random.default_rng(7)
    mel = _r(dev, B, L, nm, seed=1)
    lin, post = _r(dev, B, S, nm, seed=2), _r(dev, B, S, nm, seed=3)
    lin[:, :L][:, :, ::3] = mel[:, :, ::3]                         # exact ties in a third of the columns
    stop = _r(dev, B, S, seed=4, scale=3.0)
    stop[0, 0], stop[-1, -1], stop[0, -1] = 40.0, -40.0, -40.0
    mlen = g.integers(1, S + 3, B).astype(np.int32)
    mlen[0] = 0; mlen[-1] = S + 1
    if B > 2:
        mlen[1] = S
    ml = torch.tensor(mlen, device=dev)
    ref, (rl, rp, rs) = _tts_loss_ref(_f64(lin), _f64(post), _f64(mel), _f64(stop), mlen, use_l1, gs)

    def run(scal):
        dl, dp, ds = _nan(dev, B, S, nm), _nan(dev, B, S, nm), _nan(dev, B, S)
        lib.call("mstts_tts_loss_fwd_bwd", lib.ptr(lin), lib.ptr(post), lib.ptr(mel), lib.ptr(stop), lib.ptr(ml), B, S, nm, use_l1, gs,
                 lib.ptr(scal), lib.ptr(dl), lib.ptr(dp), lib.ptr(ds))
        return dl, dp, ds
    scal = torch.zeros(4, device=dev); scal[3] = NAN
    dl, dp, ds = run(scal)
    assert np.isnan(t2n(scal)[3])
    _chk("scalars", scal[:3], ref)
    _chk("d_linear", dl, rl); _chk("d_post", dp, rp); _chk("d_stop", ds, rs)
    assert (t2n(dl)[:, L] == 0).all() and (t2n(dp)[:, L] == 0).all()
    tie = t2n(dl)[:, :L][:, :, ::3]
    assert (tie == 0).all()
    run(scal)                                                       # a second call into the same buffer: twice the loss
    _chk("scalars after two calls", scal[:3], 2.0 * ref)
    pre = torch.tensor([0.5, -1.0, 2.0], device=dev)
    run(pre)
    _chk("scalars onto a pre-filled buffer", pre, np.array([0.5, -1.0, 2.0]) + ref)


def test_tts_loss_rejects_one_step(dev):
    z = torch.zeros(64, device=dev)
    ml = torch.ones(2, dtype=torch.int32, device=dev)
    assert lib.load().mstts_tts_loss_fwd_bwd(lib.ptr(z), lib.ptr(z), lib.ptr(z), lib.ptr(z), lib.ptr(ml), 2, 1, 4, 1, C.c_float(1.0), lib.ptr(z), lib.ptr(z),
                                             lib.ptr(z), lib.ptr(z), lib.stream()) != 0


# ---------------------------------------------------------------------------------------------------------------------------------
# column statistics: colsum, batch norm
# ---------------------------------------------------------------------------------------------------------------------------------
BN_ROWS = [1, 31, 32, 33, 127, 1025, 8990]
BN_C = [4, 48, 256, 260, 512]
EPS, MOM = 1e-3, 0.99


class _maybe_det:
    def __init__(self, on):
        self.cm = lib.deterministic_gemm() if on else None

    def __enter__(self):
        if self.cm:
            self.cm.__enter__()

    def __exit__(self, *a):
        if self.cm:
            self.cm.__exit__(*a)
        return False


def _colsum_case(dev, rows, Cc, ld, det):
    x = _r(dev, rows, ld, seed=rows + Cc)
    ref = _f64(x)[:, :Cc].sum(0)
    outs = []
    with _maybe_det(det):
        for _ in range(2 if det else 1):
            out = _nan(dev, Cc + 4)
            lib.call("mstts_colsum", lib.ptr(x), rows, Cc, ld, lib.ptr(out), 0)
            outs.append(t2n(out))
        acc = torch.full((Cc + 4,), NAN, device=dev); acc[:Cc] = 2.0
        lib.call("mstts_colsum", lib.ptr(x), rows, Cc, ld, lib.ptr(acc), 1)
    # (columns of N(0, 1) sum to ~sqrt(rows): rel_err's scale is the largest column sum, the error a few ulp of the partial sums)
    _chk("colsum %d x %d ld %d" % (rows, Cc, ld), outs[0][:Cc], ref)
    _chk("colsum accumulate", t2n(acc)[:Cc], 2.0 + ref)
    assert np.isnan(outs[0][Cc:]).all() and np.isnan(t2n(acc)[Cc:]).all()
    if det:
        _same("second run", outs[1][:Cc], outs[0][:Cc])


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("Cc", BN_C)
@pytest.mark.parametrize("rows", BN_ROWS)
def test_colsum(dev, rows, Cc, det):
    _colsum_case(dev, rows, Cc, Cc, det)


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("rows,Cc,ld", [(1025, 7, 12), (33, 7, 12), (1025, 64, 128), (8990, 64, 128), (31, 260, 264)])
def test_colsum_row_stride(dev, rows, Cc, ld, det):
    """ld > C: the scalar kernel (C = 7) and the float4 kernel (C = 64, 260) read only the first C columns of every row."""
    _colsum_case(dev, rows, Cc, ld, det)


def _bn_fwd_ref(x, gamma, beta, mask, keep):
    mean = x.mean(0); var = ((x - mean) ** 2).mean(0)
    rstd = 1.0 / np.sqrt(var + EPS)
    y = (x - mean) * rstd * gamma + beta
    if mask is not None:
        y = y * mask / keep
    return mean, var, rstd, y


def _bn_fwd_call(dev, x, gamma, beta, mm, mv, mask, keep, rows, Cc):
    y, sm, sr, ws = _nan(dev, rows, Cc), _nan(dev, Cc), _nan(dev, Cc), _nan(dev, 2 * Cc)
    lib.call("mstts_bn_train_fwd", lib.ptr(x), lib.ptr(gamma), lib.ptr(beta), lib.ptr(mm), lib.ptr(mv), lib.ptr(y), lib.ptr(sm), lib.ptr(sr),
             lib.ptr(mask), keep, MOM, EPS, rows, Cc, lib.ptr(ws))
    return y, sm, sr


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("Cc", BN_C)
@pytest.mark.parametrize("rows", BN_ROWS)
def test_bn_train_fwd(dev, rows, Cc, det):
    """Batch moments (biased variance), normalise, scale / shift, dropout; saved mean / rstd; moving statistics - with and without a mask,
    at row counts around the chunk (32) and unroll (4 x 8 rows) boundaries and column counts on both sides of one 256-column block."""
    x = _r(dev, rows, Cc, seed=rows * 7 + Cc)
    gamma, beta = _r(dev, Cc, seed=2) + 1.5, _r(dev, Cc, seed=3)
    mask = _bits(dev, rows, Cc, seed=4)
    with _maybe_det(det):
        for mk, keep in ((None, 1.0), (mask, 0.5)):
            mm0, mv0 = _r(dev, Cc, seed=5), torch.abs(_r(dev, Cc, seed=6)) + 0.5
            mean, var, rstd, yr = _bn_fwd_ref(_f64(x), _f64(gamma), _f64(beta), None if mk is None else _f64(mk), keep)
            runs = []
            for _ in range(2 if det else 1):
                mm, mv = mm0.clone(), mv0.clone()
                y, sm, sr = _bn_fwd_call(dev, x, gamma, beta, mm, mv, mk, keep, rows, Cc)
                runs.append([t2n(t) for t in (y, sm, sr, mm, mv)])
            y, sm, sr, mm, mv = runs[0]
            _chk("y", y, yr); _chk("save_mean", sm, mean); _chk("save_rstd", sr, rstd)
            _chk("moving_mean", mm, MOM * _f64(mm0) + (1 - MOM) * mean); _chk("moving_var", mv, MOM * _f64(mv0) + (1 - MOM) * var)
            if det:
                for a, b in zip(*runs):
                    _same("second run", b, a)


def _bn_bwd_ref(dy, x, gamma, mean, rstd, mask, keep, act):
    n = x.shape[0]
    dyn = dy if mask is None else dy * mask / keep
    xhat = (x - mean) * rstd
    s1, s2 = dyn.sum(0), (dyn * xhat).sum(0)
    dz = gamma * rstd * (dyn - s1 / n - xhat * s2 / n)
    if act == lib.ACT_RELU:
        dz = np.where(x > 0, dz, 0.0)
    elif act == lib.ACT_TANH:
        dz = dz * (1.0 - x * x)
    return dz, s2, s1


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("Cc", BN_C)
@pytest.mark.parametrize("rows", BN_ROWS)
def test_bn_train_bwd(dev, rows, Cc, det):
    """dz = dBN(dy * mask / keep) * act'(x) with act' taken from x itself (x is the activation's OUTPUT: relu -> x > 0, tanh -> 1 - x^2),
    dgamma / dbeta / dbias ADD to what they hold: ReLU and tanh, with and without a mask, dbias on and off.  The saved statistics handed
    in are the fp64 batch moments rounded to fp32, so this is the backward alone."""
    z = _r(dev, rows, Cc, seed=rows * 5 + Cc)
    dy = _r(dev, rows, Cc, seed=rows * 3 + Cc + 1)
    gamma = _r(dev, Cc, seed=2) + 1.5
    mask = _bits(dev, rows, Cc, seed=4)
    with _maybe_det(det):
        for act in (lib.ACT_RELU, lib.ACT_TANH):
            x = torch.relu(z) if act == lib.ACT_RELU else torch.tanh(z)
            mean64, _, rstd64, _ = _bn_fwd_ref(_f64(x), 1.0, 0.0, None, 1.0)
            sm, sr = torch.tensor(mean64, dtype=torch.float32, device=dev), torch.tensor(rstd64, dtype=torch.float32, device=dev)
            for mk, keep in ((None, 1.0), (mask, 0.5)):
                dzr, dgr, dbr = _bn_bwd_ref(_f64(dy), _f64(x), _f64(gamma), _f64(sm), _f64(sr), None if mk is None else _f64(mk), keep, act)
                for with_dbias in (1, 0):
                    runs = []
                    for _ in range(2 if det else 1):
                        dz, ws = _nan(dev, rows, Cc), _nan(dev, 2 * Cc)
                        dg, db, dbias = torch.full((Cc,), 1.0, device=dev), torch.full((Cc,), -2.0, device=dev), torch.full((Cc,), 0.5, device=dev)
                        lib.call("mstts_bn_train_bwd", lib.ptr(dy), lib.ptr(x), lib.ptr(gamma), lib.ptr(sm), lib.ptr(sr), lib.ptr(mk), keep, act, lib.ptr(dz),
                                 lib.ptr(dg), lib.ptr(db), lib.ptr(dbias) if with_dbias else None, rows, Cc, lib.ptr(ws))
                        runs.append([t2n(t) for t in (dz, dg, db, dbias)])
                    dz, dg, db, dbias = runs[0]
                    tag = "act %d mask %d dbias %d: " % (act, mk is not None, with_dbias)
                    _chk(tag + "dz", dz, dzr); _chk(tag + "dgamma", dg, 1.0 + dgr); _chk(tag + "dbeta", db, -2.0 + dbr)
                    if with_dbias:
                        _chk(tag + "dbias", dbias, 0.5 + dzr.sum(0))
                    else:
                        assert (dbias == 0.5).all()
                    if det:
                        for a, b in zip(*runs):
                            _same("second run", b, a)


def test_bn_train_fwd_offset_inputs(dev):
    """The one-pass variance E[x^2] - mean^2 on inputs that are not centred: N(3, 1) (E[x^2] ~ 10 var) stays under TOL; N(30, 1)
    (E[x^2] ~ 900 var: the difference of two fp32 numbers near 901) is printed, not asserted - measured: batch variance 1.2e-3, save_rstd
    6.2e-4, y 4.0e-4 off the fp64 values, against 1.1e-7 / 5.0e-6 / 3.9e-6 at N(3, 1)."""
    rows, Cc = 8990, 48
    gamma, beta = _r(dev, Cc, seed=2) + 1.5, _r(dev, Cc, seed=3)
    for mu in (3.0, 30.0):
        x = _r(dev, rows, Cc, seed=11, mean=mu)
        mm, mv = torch.zeros(Cc, device=dev), torch.ones(Cc, device=dev)
        y, sm, sr = _bn_fwd_call(dev, x, gamma, beta, mm, mv, None, 1.0, rows, Cc)
        mean, var, rstd, yr = _bn_fwd_ref(_f64(x), _f64(gamma), _f64(beta), None, 1.0)
        if mu == 3.0:
            _chk("N(3,1) y", y, yr); _chk("N(3,1) save_rstd", sr, rstd); _chk("N(3,1) moving_var", mv, MOM + (1 - MOM) * var)
            _chk("N(3,1) moving_mean", mm, (1 - MOM) * mean)
        else:
            print("N(30,1), not asserted: y %.3e, save_rstd %.3e, batch variance %.3e" %
                  (rel_err(t2n(y), yr), rel_err(t2n(sr), rstd), rel_err((_f64(mv) - MOM) / (1 - MOM), var)))


@pytest.mark.parametrize("rows,Cc", [(5, 4), (333, 48), (8200, 256)])
def test_bn_infer_fwd(dev, rows, Cc):
    """y = (x - moving_mean) / sqrt(moving_var + eps) * gamma + beta (the variance branch of the apply kernel); 8200 x 256 is past the cap."""
    x = _r(dev, rows, Cc, seed=1)
    gamma, beta, mm, mv = _r(dev, Cc, seed=2) + 1.5, _r(dev, Cc, seed=3), _r(dev, Cc, seed=4), torch.abs(_r(dev, Cc, seed=5)) * 0.01
    y = _nan(dev, rows, Cc)
    lib.call("mstts_bn_infer_fwd", lib.ptr(x), lib.ptr(gamma), lib.ptr(beta), lib.ptr(mm), lib.ptr(mv), lib.ptr(y), EPS, rows, Cc)
    _chk("bn_infer_fwd", y, (_f64(x) - _f64(mm)) / np.sqrt(_f64(mv) + EPS) * _f64(gamma) + _f64(beta))


# ---------------------------------------------------------------------------------------------------------------------------------
# WaveGlow inference pointwise kernels (formulas: include/mstts.h, oracle/waveglow.py wavenet / coupling_reverse)
# ---------------------------------------------------------------------------------------------------------------------------------
def _sg(v):
    return 1.0 / (1.0 + np.exp(-v))


@pytest.mark.parametrize("rows,Cc,pad", [(301, 8, 0), (301, 8, 8), (1, 1, 0), (WG_CAP // 8 + 77, 8, 0)])
def test_wg_gate(dev, rows, Cc, pad):
    lda = 2 * Cc + pad
    a, z = _r(dev, rows, lda, seed=1), _nan(dev, rows * Cc + 8)
    lib.call("mstts_wg_gate", lib.ptr(a), lda, lib.ptr(z), rows, Cc)
    an = _f64(a)
    _chk("wg_gate", z[:rows * Cc].view(rows, Cc), np.tanh(an[:, :Cc]) * _sg(an[:, Cc:2 * Cc]))
    assert np.isnan(t2n(z[rows * Cc:])).all()


@pytest.mark.parametrize("rows,Cc", [(301, 4), (301, 256), (1, 4)])
def test_wg_gate_add(dev, rows, Cc):
    lda = 2 * Cc + 4
    a, b, z = _r(dev, rows, lda, seed=1), _r(dev, rows, 2 * Cc, seed=2), _nan(dev, rows, Cc)
    lib.call("mstts_wg_gate_add", lib.ptr(a), lda, lib.ptr(b), lib.ptr(z), rows, Cc)
    an, bn = _f64(a), _f64(b)
    _chk("wg_gate_add", z, np.tanh(an[:, :Cc] + bn[:, :Cc]) * _sg(an[:, Cc:2 * Cc] + bn[:, Cc:]))
    assert lib.load().mstts_wg_gate_add(lib.ptr(a), 2 * Cc + 2, lib.ptr(b), lib.ptr(z), rows, Cc, lib.stream()) != 0      # lda % 4


@pytest.mark.parametrize("last,first", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("rows,Cc", [(301, 8), (WG_CAP // 8 + 77, 8)])
def test_wg_res_skip(dev, rows, Cc, last, first):
    """!last: x = z + rs[:, :C], skip = rs[:, C:]; last: skip = rs [rows, C], x untouched; out = first ? skip : out + skip."""
    z, rs = _r(dev, rows, Cc, seed=1), _r(dev, rows, Cc if last else 2 * Cc, seed=2)
    out0 = _r(dev, rows, Cc, seed=3)
    x, out = _nan(dev, rows, Cc), (_nan(dev, rows, Cc) if first else out0.clone())
    lib.call("mstts_wg_res_skip", lib.ptr(z), lib.ptr(rs), lib.ptr(x), lib.ptr(out), rows, Cc, last, first)
    rn = _f64(rs)
    skip = rn if last else rn[:, Cc:]
    _chk("out", out, skip if first else _f64(out0) + skip)
    if last:
        assert np.isnan(t2n(x)).all()
    else:
        _chk("x", x, _f64(z) + rn[:, :Cc])


@pytest.mark.parametrize("rows", [1, 257, 100003])
@pytest.mark.parametrize("ce", [0, 2])
@pytest.mark.parametrize("c", [2, 8, 16])
def test_wg_coupling_inv(dev, c, ce, rows):
    """a1 = (audio[:, c/2:] - b) * exp(-log_s), out[:, ce:] = [a0 | a1] . w_inv, out[:, :ce] = early * sigma."""
    h = c // 2
    audio, lsb = _r(dev, rows, c, seed=1), _r(dev, rows, c, seed=2, scale=0.4)
    winv = _r(dev, c, c, seed=3, scale=1.0 / np.sqrt(c))
    early = _r(dev, rows, ce, seed=4) if ce else None
    out = _nan(dev, rows * (c + ce) + 8)
    lib.call("mstts_wg_coupling_inv", lib.ptr(audio), lib.ptr(lsb), lib.ptr(winv), lib.ptr(early), 0.6, lib.ptr(out), rows, c, ce)
    an, ln = _f64(audio), _f64(lsb)
    xcat = np.concatenate([an[:, :h], (an[:, h:] - ln[:, h:]) * np.exp(-ln[:, :h])], 1)
    ref = xcat @ _f64(winv)
    if ce:
        ref = np.concatenate([_f64(early) * np.float64(np.float32(0.6)), ref], 1)
    _chk("wg_coupling_inv", out[:rows * (c + ce)].view(rows, c + ce), ref)
    assert np.isnan(t2n(out[rows * (c + ce):])).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# exported pair forms: each member against the fp64 reference, and at the tolerance, its single form has
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,R,N", [(32, 1792, 4096), (32, 1024, 128), (7, 192, 256), (33, 40, 64)])
def test_skinny_bwd_pair(dev, M, R, N):
    """mstts_skinny_bwd_pair: two products dG . W^T of one shape in one launch (tests/test_gpu_ops.py::test_skinny_bwd is the single form)."""
    ns = lib.load().mstts_skinny_bwd_splits(R, N)
    assert ns >= 1
    dG = [_r(dev, M, N, seed=3), _r(dev, M, N, seed=13)]
    W = [_r(dev, R, N, seed=4, scale=0.1), _r(dev, R, N, seed=14, scale=0.1)]
    P = [_nan(dev, ns, M, R), _nan(dev, ns, M, R)]
    lib.call("mstts_skinny_bwd_pair", lib.ptr(dG[0]), lib.ptr(dG[1]), N, lib.ptr(W[0]), lib.ptr(W[1]), N, lib.ptr(P[0]), lib.ptr(P[1]), 0, M, R, N, ns)
    for k in range(2):
        _chk("member %d" % k, _f64(P[k]).sum(0), _f64(dG[k]) @ _f64(W[k]).T)
    assert not np.array_equal(t2n(P[0]), t2n(P[1]))


def _cell_case(dev, B, H, K, mode, seed):
    L = lib.load()
    ldx, hld, old = K + 8, H + 4, H + 12
    t = dict(X=_r(dev, B, ldx, seed=seed + 1), W=_r(dev, K, 4 * H, seed=seed + 2, scale=1.0 / np.sqrt(K)),
             xw=_r(dev, B, 4 * H, seed=seed + 3) if mode == "xw" else None, bias=_r(dev, 4 * H, seed=seed + 4, scale=0.3) if mode == "bias" else None,
             cp=_r(dev, B, H, seed=seed + 5), hp=_r(dev, B, hld, seed=seed + 6), zc=_bits(dev, B, H, seed=seed + 7), zh=_bits(dev, B, H, seed=seed + 8),
             out=_nan(dev, B, old), cn=_nan(dev, B, H), hn=_nan(dev, B, hld), acts=_nan(dev, B, 4 * H), craw=_nan(dev, B, H))
    t["Wp"] = torch.zeros(K * 4 * H, device=dev)
    lib.call("mstts_pack_cell_fwd", lib.ptr(t["W"]), 4 * H, lib.ptr(t["Wp"]), K, H)
    t["Xp"] = torch.full((int(L.mstts_cell_act_floats(B, K)),), NAN, device=dev)
    lib.call("mstts_pack_cell_act", lib.ptr(t["X"]), ldx, lib.ptr(t["Xp"]), B, K)
    d = lib.CellFwd()
    d.B, d.H, d.K, d.Xp, d.Wp = B, H, K, lib.ptr(t["Xp"]), lib.ptr(t["Wp"])
    d.xw, d.xw_ld, d.bias = lib.ptr(t["xw"]), 4 * H, lib.ptr(t["bias"])
    d.c_prev, d.h_prev, d.h_prev_ld, d.zc, d.zh, d.zoneout = lib.ptr(t["cp"]), lib.ptr(t["hp"]), hld, lib.ptr(t["zc"]), lib.ptr(t["zh"]), 0.1
    d.out, d.out_ld, d.c_next, d.h_next, d.h_next_ld = lib.ptr(t["out"]), old, lib.ptr(t["cn"]), lib.ptr(t["hn"]), hld
    d.acts, d.c_raw = lib.ptr(t["acts"]), lib.ptr(t["craw"])
    return d, t


@pytest.mark.parametrize("B,H,K,mode", [(32, 1024, 1792, "xw"), (32, 1024, 2048, "bias"), (5, 64, 192, "xw"), (17, 8, 64, "bias"), (40, 16, 128, "none")])
def test_cell_fwd_pair(dev, B, H, K, mode):
    """mstts_cell_fwd_pair: two fused cell steps (different operands) in one launch, each against the zoneout cell in fp64
    (ZoneoutLSTMCell.py:228-271) at the tolerance of the single form (tests/test_gpu_ops.py::test_cell_fwd_fused); columns behind H of the
    strided outputs are untouched."""
    assert lib.load().mstts_cell_fwd_supported(H, K) == 1
    (da, ta), (db, tb) = _cell_case(dev, B, H, K, mode, 0), _cell_case(dev, B, H, K, mode, 100)
    lib.call("mstts_cell_fwd_pair", C.byref(da), C.byref(db))
    for k, t in enumerate((ta, tb)):
        gates = _f64(t["X"])[:, :K] @ _f64(t["W"])
        if t["xw"] is not None:
            gates = gates + _f64(t["xw"])
        if t["bias"] is not None:
            gates = gates + _f64(t["bias"])
        i, j, f, o = np.split(gates, 4, axis=1)
        cp, hp = _f64(t["cp"]), _f64(t["hp"])[:, :H]
        c = _sg(f + 1.0) * cp + _sg(i) * np.tanh(j)
        m = _sg(o) * np.tanh(c)
        tag = "member %d " % k
        _chk(tag + "out", t["out"][:, :H], m); _chk(tag + "c_next", t["cn"], 0.9 * t2n(t["zc"]) * (c - cp) + cp)
        _chk(tag + "h_next", t["hn"][:, :H], 0.9 * t2n(t["zh"]) * (m - hp) + hp)
        _chk(tag + "c_raw", t["craw"], c); _chk(tag + "acts", t["acts"], np.concatenate([_sg(i), np.tanh(j), _sg(f + 1.0), _sg(o)], 1))
        assert np.isnan(t2n(t["out"])[:, H:]).all() and np.isnan(t2n(t["hn"])[:, H:]).all()
    assert not np.array_equal(t2n(ta["out"]), t2n(tb["out"]))


def _point_case(dev, B, H, seed):
    """tests/test_gpu_model.py::test_lstm_point_fwd_bwd's case: forward through mstts_lstm_point_fwd (saves acts / c_raw), fp64 autograd."""
    gates = _r(dev, B, 4 * H, seed=seed + 1); bias = _r(dev, 4 * H, seed=seed + 2, scale=0.1)
    cp, hp = _r(dev, B, H, seed=seed + 3), _r(dev, B, H, seed=seed + 4)
    zc, zh = _bits(dev, B, H, seed=seed + 5), _bits(dev, B, H, seed=seed + 6)
    out, cn, hn = _nan(dev, B, H), _nan(dev, B, H), _nan(dev, B, H)
    acts, craw = _nan(dev, B, 4 * H), _nan(dev, B, H)
    d = lib.LstmPointFwd()
    d.B, d.H, d.gates_h, d.bias = B, H, lib.ptr(gates), lib.ptr(bias)
    d.c_prev, d.h_prev, d.zc, d.zh, d.zoneout = lib.ptr(cp), lib.ptr(hp), lib.ptr(zc), lib.ptr(zh), 0.1
    d.out, d.out_sb, d.c_next, d.h_next, d.acts_out, d.c_raw = lib.ptr(out), H, lib.ptr(cn), lib.ptr(hn), lib.ptr(acts), lib.ptr(craw)
    lib.call("mstts_lstm_point_fwd", C.byref(d))
    g64 = (gates.double().cpu() + bias.double().cpu()).requires_grad_(True)
    cp64, hp64 = cp.double().cpu().requires_grad_(True), hp.double().cpu().requires_grad_(True)
    i, j, f, o = g64.chunk(4, 1)
    c = torch.sigmoid(f + 1.0) * cp64 + torch.sigmoid(i) * torch.tanh(j)
    m = torch.sigmoid(o) * torch.tanh(c)
    c2 = 0.9 * (c - cp64) * zc.cpu().double() + cp64
    h2 = 0.9 * (m - hp64) * zh.cpu().double() + hp64
    dm, dc2, dh2 = _r(dev, B, H, seed=seed + 7), _r(dev, B, H, seed=seed + 8), _r(dev, B, H, seed=seed + 9)
    ((m * dm.double().cpu()).sum() + (c2 * dc2.double().cpu()).sum() + (h2 * dh2.double().cpu()).sum()).backward()
    dg, dcp, dhp = _nan(dev, B, 4 * H), _nan(dev, B, H), _nan(dev, B, H)
    b = lib.LstmPointBwd()
    b.B, b.H, b.d_out, b.dout_sb = B, H, lib.ptr(dm), H
    b.d_c_state, b.d_h_state, b.acts, b.c_raw, b.c_prev = lib.ptr(dc2), lib.ptr(dh2), lib.ptr(acts), lib.ptr(craw), lib.ptr(cp)
    b.zc, b.zh, b.zoneout, b.dgates, b.d_c_prev, b.d_h_prev = lib.ptr(zc), lib.ptr(zh), 0.1, lib.ptr(dg), lib.ptr(dcp), lib.ptr(dhp)
    keep = (gates, bias, cp, hp, zc, zh, out, cn, hn, acts, craw, dm, dc2, dh2)
    return b, dict(dg=dg, dcp=dcp, dhp=dhp, rg=t2n(g64.grad), rc=t2n(cp64.grad), rh=t2n(hp64.grad), keep=keep)


@pytest.mark.parametrize("B,H", [(5, 24), (32, 256)])
def test_lstm_point_bwd_pair(dev, B, H):
    """mstts_lstm_point_bwd_pair: the pointwise backward of two cells (different operands) in one launch, each against fp64 autograd of the
    cell at the single form's tolerance (tests/test_gpu_model.py::test_lstm_point_fwd_bwd: 2e-5)."""
    (ba, ta), (bb, tb) = _point_case(dev, B, H, 0), _point_case(dev, B, H, 50)
    lib.call("mstts_lstm_point_bwd_pair", C.byref(ba), C.byref(bb))
    for k, t in enumerate((ta, tb)):
        _chk("member %d dgates" % k, t["dg"], t["rg"], 2e-5); _chk("member %d d_c_prev" % k, t["dcp"], t["rc"], 2e-5)
        _chk("member %d d_h_prev" % k, t["dhp"], t["rh"], 2e-5)
    assert not np.array_equal(t2n(ta["dg"]), t2n(tb["dg"]))
    bb.H = H + 4                                                    # members of different shape: a host-side rejection
    assert lib.load().mstts_lstm_point_bwd_pair(C.byref(ba), C.byref(bb), lib.stream()) != 0


# ---------------------------------------------------------------------------------------------------------------------------------
# every dispatch arm of mstts_lstm_point_fwd / _bwd / _bwd_pair (csrc/elementwise.hip; the cell math is csrc/lstm_cell.h), each against the
# zoneout cell in fp64 (ZoneoutLSTMCell.py:228-271) at the tolerances of tests/test_gpu_model.py::test_lstm_point_fwd_bwd: 1e-5 forward,
# 2e-5 backward.  (5, 24): flat grid, ragged last block; (3, 128): the backward's grid of (H / 128, B) blocks.
# ---------------------------------------------------------------------------------------------------------------------------------
POINT_SHAPES = [(5, 24), (3, 128)]
POINT_T, POINT_STEP = 4, 2
POINT_LEN = [4, 3, 2, 1, 3]         # at step 2: rows 2 and 3 are dead, step 2 is the last live step of rows 1 and 4


def _point_rows(B, form):
    """(lengths or None, live [B], pos [B]) of a case: 'plain' has no lengths and position 0, 'seq' / 'rev' are dynamic_rnn's two directions."""
    if form == "plain":
        return None, np.ones(B, bool), np.zeros(B, np.int64)
    lengths = np.array(POINT_LEN[:B], np.int32)
    live = POINT_STEP < lengths
    pos = np.where(live & (form == "rev"), lengths - 1 - POINT_STEP, POINT_STEP).astype(np.int64)
    return lengths, live, pos


def _only_at(what, got, ref, tol):
    """`ref` holds NaN wherever the call must not write: those elements of `got` still hold their NaN filling, the others meet `tol`."""
    got, w = t2n(got), ~np.isnan(ref)
    assert np.isnan(got[~w]).all(), what + ": written outside its region"
    _chk(what, got[w], ref[w], tol)


def _point_fwd_run(dev, B, H, parts, mode, form, wide, out_null=False, saves=None, seed=0):
    T, seq = POINT_T, form != "plain"
    lengths, live, pos = _point_rows(B, form)
    saves = (not seq) if saves is None else saves
    hpl, hnl, old = (H + 4, H + 8, H + 12) if wide else (H, H, H)
    gates = _r(dev, parts, B, 4 * H, seed=seed + 1, scale=1.0 / np.sqrt(parts))
    add = _r(dev, *((B, T, 4 * H) if seq else (B, 4 * H)), seed=seed + 2) if mode == "xw" else _r(dev, 4 * H, seed=seed + 2, scale=0.1)
    cp, hp = _r(dev, B, H, seed=seed + 3), _r(dev, B, hpl, seed=seed + 4)
    zc, zh = _bits(dev, B, H, seed=seed + 5), _bits(dev, B, H, seed=seed + 6)
    res = _r(dev, B, T, H, seed=seed + 7) if seq else None
    out = None if out_null else _nan(dev, *((B, T, old) if seq else (B, old)))
    cn, hn = _nan(dev, B, H), _nan(dev, B, hnl)
    acts, craw = (_nan(dev, B, 4 * H), _nan(dev, B, H)) if saves else (None, None)
    d = lib.LstmPointFwd()
    d.B, d.H, d.gates_h, d.gates_parts, d.gates_pstride = B, H, lib.ptr(gates), parts, B * 4 * H
    if mode == "xw":
        d.xw, d.xw_sb, d.xw_st = lib.ptr(add), (T * 4 * H if seq else 4 * H), (4 * H if seq else 0)
    else:
        d.bias = lib.ptr(add)
    d.c_prev, d.h_prev, d.h_prev_ld, d.zc, d.zh, d.zoneout = lib.ptr(cp), lib.ptr(hp), (hpl if wide else 0), lib.ptr(zc), lib.ptr(zh), 0.1
    if seq:
        lens = torch.tensor(lengths, device=dev)
        d.lengths, d.step, d.reverse, d.residual, d.res_sb, d.res_st = lib.ptr(lens), POINT_STEP, int(form == "rev"), lib.ptr(res), T * H, H
    d.out, d.out_sb, d.out_st = lib.ptr(out), (T * old if seq else old), (old if seq else 0)
    d.c_next, d.h_next, d.h_next_ld, d.acts_out, d.c_raw = lib.ptr(cn), lib.ptr(hn), (hnl if wide else 0), lib.ptr(acts), lib.ptr(craw)
    lib.call("mstts_lstm_point_fwd", C.byref(d))
    rows = np.arange(B)
    g = _f64(gates).sum(0) + (_f64(add)[rows, pos] if (mode == "xw" and seq) else _f64(add))
    i, j, f, o = np.split(g, 4, axis=1)
    si, tj, sf, so = _sg(i), np.tanh(j), _sg(f + 1.0), _sg(o)
    cp64, hp64, lv = _f64(cp), _f64(hp)[:, :H], live[:, None]
    c = sf * cp64 + si * tj
    m = so * np.tanh(c)
    tag = "fwd %s parts %d %s%s: " % (form, parts, mode, " wide" if wide else "")
    if not out_null:
        ref = np.full(tuple(out.shape), np.nan)
        o_ref = np.where(lv, m + (_f64(res)[rows, pos] if seq else 0.0), 0.0)
        if seq:
            ref[rows, pos, :H] = o_ref
        else:
            ref[:, :H] = o_ref
        _only_at(tag + "out", out, ref, 1e-5)
    _chk(tag + "c_next", cn, np.where(lv, 0.9 * t2n(zc) * (c - cp64) + cp64, cp64), 1e-5)
    ref = np.full((B, hnl), np.nan)
    ref[:, :H] = np.where(lv, 0.9 * t2n(zh) * (m - hp64) + hp64, hp64)
    _only_at(tag + "h_next", hn, ref, 1e-5)
    if saves:
        _chk(tag + "acts", acts, np.where(lv, np.concatenate([si, tj, sf, so], 1), 0.0), 1e-5)
        _chk(tag + "c_raw", craw, np.where(lv, c, cp64), 1e-5)


@pytest.mark.parametrize("mode", ["bias", "xw"])            # the bias alone / a hoisted input product with the bias folded in
@pytest.mark.parametrize("parts", [1, 2, 3, 4, 7, 8, 16])    # 3: no instantiation of its own, the run-time slab count
@pytest.mark.parametrize("B,H", POINT_SHAPES)
def test_lstm_point_fwd_arms(dev, B, H, parts, mode):
    """mstts_lstm_point_fwd for every slab count it has a kernel for and one it has none for, in the plain form and in the sequence form
    (lengths with a dead row and a row at its last live step, both directions, residual, nonzero out_st / xw_st, no saves), with default
    and with wider state / output row strides (columns behind H keep their NaN)."""
    for form in ("plain", "seq", "rev"):
        for wide in (False, True):
            _point_fwd_run(dev, B, H, parts, mode, form, wide)


@pytest.mark.parametrize("form", ["plain", "seq", "rev"])
@pytest.mark.parametrize("B,H", POINT_SHAPES)
def test_lstm_point_fwd_without_out_and_with_saves(dev, B, H, form):
    """out == NULL (states and saves only) and the sequence form with the BPTT saves: a dead row saves zero activations and c_raw = c_prev."""
    for parts in (1, 3):
        _point_fwd_run(dev, B, H, parts, "bias", form, True, out_null=True, saves=True)
        _point_fwd_run(dev, B, H, parts, "xw", form, False, saves=True)


def _point_bwd_run(dev, B, H, po, po2, ph, form, masks=True, dout=True, dout2=False, dhs2=False, fuse=None, seed=0, launch=True):
    """One backward case: (descriptor, checker).  po / po2 / ph: slabs of d_out / d_out2 / d_h_state2; fuse: None or dq_bf16 (0 / 1)."""
    T, seq, A = POINT_T, form != "plain", 128
    lengths, live, pos = _point_rows(B, form)
    rows, lv = np.arange(B), torch.tensor(live)[:, None]
    ld2 = H + 4
    g64 = torch.tensor(np.random.default_rng(seed + 1).normal(size=(B, 4 * H)), dtype=torch.float64, requires_grad=True)
    cp, hp = _r(dev, B, H, seed=seed + 3), _r(dev, B, H, seed=seed + 4)
    zc, zh = (_bits(dev, B, H, seed=seed + 5), _bits(dev, B, H, seed=seed + 6)) if masks else (None, None)
    cp64, hp64 = cp.double().cpu().requires_grad_(True), hp.double().cpu().requires_grad_(True)
    i, j, f, o = g64.chunk(4, 1)
    si, tj, sf, so = torch.sigmoid(i), torch.tanh(j), torch.sigmoid(f + 1.0), torch.sigmoid(o)
    c = sf * cp64 + si * tj
    m = so * torch.tanh(c)
    kc, kh = (0.9 * zc.cpu().double(), 0.9 * zh.cpu().double()) if masks else (0.9, 0.9)
    c2, h2 = torch.where(lv, kc * (c - cp64) + cp64, cp64), torch.where(lv, kh * (m - hp64) + hp64, hp64)
    acts, craw = torch.cat([si, tj, sf, so], 1).detach().float().to(dev), c.detach().float().to(dev)
    d_o = _r(dev, *((po, B, T, H) if seq else (po, B, H)), seed=seed + 7) if dout else None
    d_o2 = _r(dev, po2, B, H, seed=seed + 8) if dout2 else None
    dcs, dhs = _r(dev, B, H, seed=seed + 9), _r(dev, B, H, seed=seed + 10)
    d_h2 = _r(dev, ph, B, ld2, seed=seed + 11) if dhs2 else None
    dm64 = torch.zeros(B, H, dtype=torch.float64)
    if dout:
        dm64 = dm64 + torch.tensor(_f64(d_o).sum(0)[rows, pos] if seq else _f64(d_o).sum(0))
    if dout2:
        dm64 = dm64 + d_o2.double().cpu().sum(0)
    dhs64 = dhs.double().cpu() + (d_h2.double().cpu().sum(0)[:, :H] if dhs2 else 0.0)
    dq = wq = wq_t = None
    if fuse is not None:
        dq, wq = _r(dev, B, A, seed=seed + 12), _r(dev, H, A, seed=seed + 13, scale=0.2)
        wq_t = wq.view(H, A // 4, 4).permute(1, 0, 2).contiguous()           # [A/4][H][4] (mstts_transpose01(Wq, wq_t, H, A/4, 4))
        rnd = (lambda t: t.bfloat16().double().cpu()) if fuse else (lambda t: t.double().cpu())
        dm64 = dm64 + rnd(dq) @ rnd(wq).T
    ((torch.where(lv, m, torch.zeros_like(m)) * dm64).sum() + (c2 * dcs.double().cpu()).sum() + (h2 * dhs64).sum()).backward()
    dg, dcp, dhp = _nan(dev, B, 4 * H), _nan(dev, B, H), _nan(dev, B, H)
    dgp = _nan(dev, B, T, 4 * H) if seq else None
    b = lib.LstmPointBwd()
    b.B, b.H = B, H
    if dout:
        b.d_out, b.dout_sb, b.dout_st, b.dout_parts, b.dout_pstride = lib.ptr(d_o), (T * H if seq else H), (H if seq else 0), po, d_o[0].numel()
    if dout2:
        b.d_out2, b.dout2_parts, b.dout2_pstride = lib.ptr(d_o2), po2, B * H
    b.d_c_state, b.d_h_state = lib.ptr(dcs), lib.ptr(dhs)
    if dhs2:
        b.d_h_state2, b.dhs2_ld, b.dhs2_parts, b.dhs2_pstride = lib.ptr(d_h2), ld2, ph, B * ld2
    b.acts, b.c_raw, b.c_prev, b.zc, b.zh, b.zoneout = lib.ptr(acts), lib.ptr(craw), lib.ptr(cp), lib.ptr(zc), lib.ptr(zh), 0.1
    lens = torch.tensor(lengths, device=dev) if seq else None
    if seq:
        b.lengths, b.step, b.reverse, b.dgates_pos, b.dgp_sb, b.dgp_st = lib.ptr(lens), POINT_STEP, int(form == "rev"), lib.ptr(dgp), T * 4 * H, 4 * H
    b.dgates, b.d_c_prev, b.d_h_prev = lib.ptr(dg), lib.ptr(dcp), lib.ptr(dhp)
    if fuse is not None:
        b.dq, b.wq_t, b.A, b.dq_bf16 = lib.ptr(dq), lib.ptr(wq_t), A, fuse
    keep = (cp, hp, zc, zh, acts, craw, d_o, d_o2, dcs, dhs, d_h2, dq, wq_t, lens)
    tag = "bwd %s (%d,%d,%d)%s%s%s%s: " % (form, po, po2, ph, "" if masks else " no masks", "" if dout else " no d_out", " d_out2" if dout2 else "",
                                           " dhs2" if dhs2 else "")

    def check(tol=2e-5):
        errs = [_chk(tag + "dgates", dg, t2n(g64.grad), tol), _chk(tag + "d_c_prev", dcp, t2n(cp64.grad), tol),
                _chk(tag + "d_h_prev", dhp, t2n(hp64.grad), tol)]
        if seq:
            ref = np.full((B, T, 4 * H), np.nan)
            ref[rows, pos] = t2n(g64.grad)
            _only_at(tag + "dgates_pos", dgp, ref, tol)
        return max(errs), keep

    if launch:
        lib.call("mstts_lstm_point_bwd", C.byref(b))
    return b, check


# (form, masks, d_out, d_out2, d_h_state2) - a slab count above 1 needs its operand whatever the row says
POINT_BWD_VARIANTS = [("plain", True, True, True, True), ("plain", False, True, False, False), ("seq", True, True, False, True),
                      ("seq", True, False, True, False), ("rev", False, True, True, True), ("rev", True, True, False, False)]


@pytest.mark.parametrize("po,po2,ph", [(1, 1, 1), (1, 1, 4), (4, 1, 4), (1, 1, 8), (8, 1, 8), (8, 1, 1), (1, 1, 2),      # the instantiated triples
                                       (2, 1, 1), (1, 3, 1)])                                                        # none of them: run-time slab counts
@pytest.mark.parametrize("B,H", POINT_SHAPES)
def test_lstm_point_bwd_arms(dev, B, H, po, po2, ph):
    """mstts_lstm_point_bwd for every (d_out, d_out2, d_h_state2) slab triple it has a kernel for and two it has none for (one of them
    d_out2 in 3 slabs), plain and sequence form (dead row, reverse, dgates_pos written at the row's position only), with and without
    keep masks, d_out, d_out2 and d_h_state2 (row stride wider than H)."""
    for form, masks, dout, dout2, dhs2 in POINT_BWD_VARIANTS:
        _point_bwd_run(dev, B, H, po, po2, ph, form, masks, dout or po > 1, dout2 or po2 > 1, dhs2 or ph > 1)[1]()


@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("ph", [1, 2, 4, 8])
def test_lstm_point_bwd_fused_query(dev, ph, bf16):
    """The query layer's data gradient dq . Wq^T folded into the output gradient (B, H, A = 3, 128, 128), fp32 and with both operands
    rounded to bf16 (the reference rounds them the same way before its fp64 product)."""
    for masks, dhs2 in ((True, True), (False, ph > 1)):
        _point_bwd_run(dev, 3, 128, 1, 1, ph, "plain", masks, True, False, dhs2, fuse=bf16)[1]()


def test_lstm_point_bwd_fused_query_refusals(dev):
    """What the fused query gradient does not cover is refused on the host, nothing is launched (the outputs keep their NaN)."""
    L = lib.load()
    b, check = _point_bwd_run(dev, 5, 24, 1, 1, 1, "plain", fuse=0, launch=False)              # H % 128 != 0
    assert L.mstts_lstm_point_bwd(C.byref(b), lib.stream()) != 0
    b, check = _point_bwd_run(dev, 3, 128, 1, 1, 1, "plain", dout2=True, fuse=0, launch=False)  # with d_out2
    assert L.mstts_lstm_point_bwd(C.byref(b), lib.stream()) != 0
    b, check = _point_bwd_run(dev, 3, 128, 1, 1, 1, "plain", fuse=0, launch=False)
    b.A = 64                                                                                  # A != 128
    assert L.mstts_lstm_point_bwd(C.byref(b), lib.stream()) != 0
    b.A, b.wq_t = 128, b.wq_t + 4                                                             # wq_t off its 16-byte alignment
    assert L.mstts_lstm_point_bwd(C.byref(b), lib.stream()) != 0
    b.wq_t -= 4
    lib.call("mstts_lstm_point_bwd", C.byref(b))                                              # the same descriptor, repaired, runs
    check()


@pytest.mark.parametrize("ph", [1, 2, 4, 8])
@pytest.mark.parametrize("B,H", POINT_SHAPES)
def test_lstm_point_bwd_pair_arms(dev, B, H, ph):
    """mstts_lstm_point_bwd_pair for each d_h_state2 slab count it covers: the two directions of a BiLSTM step (lengths, dgates_pos, the
    second member reversed), each member against fp64 autograd of its own cell."""
    for dhs2 in ((True, False) if ph == 1 else (True,)):
        (ba, ca), (bb, cb) = (_point_bwd_run(dev, B, H, 1, 1, ph, form, dhs2=dhs2, seed=seed, launch=False) for form, seed in (("seq", 0), ("rev", 50)))
        lib.call("mstts_lstm_point_bwd_pair", C.byref(ba), C.byref(bb))
        ca(); cb()
