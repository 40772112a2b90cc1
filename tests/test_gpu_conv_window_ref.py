"""The conv-window GEMMs against the fp64 checker tests/conv_window_ref.py (the window view as per-tap slice copies in NumPy, pinned to
oracle.model.conv1d_same and its autograd by tests/test_cpu_conv_window_ref.py), every form on its own - never one form against another.

Per case the three products of a conv block in the form training.conv_fwd / conv_bn_bwd and waveglow_trainer build them: lib.gemm with
win=(T, cin, pad[, dil]); bias and activation fused into the forward; the weight gradient with trans_a on the same window and
split_k = max(2, training._split_k(K cin, cout, rows)) into a pre-filled slab; the data gradient through the kernel mstts_conv_kernel_flip
makes (held bit for bit to the documented layout), win_pad = K - 1 - pad, once plain and once with `accumulate` onto a start value.
Forms (process-wide switches, restored in a `finally`: split3 1, split_big 1, bf16_big 1, minimums 160 / 160, deterministic off):
    f32_mfma     mstts_gemm_f32 after mstts_gemm_split3(0): v_mfma_f32_32x32x2_f32 for everything
    split_128    split3 with mstts_gemm_split_big(0): gemm_split_kernel wherever its conditions hold
    split_big    split3, big tiles and mstts_gemm_big_min_workgroups(1, 1): gemm_split_big_kernel wherever M, N >= 192
    default_det  the defaults under lib.deterministic_gemm(): no K-cut of the library's own
    bf16_128     mstts_gemm_bf16 after mstts_gemm_bf16_big(0), against the checker's bf16-rounded statements
    bf16_big     mstts_gemm_bf16 with big tiles and the minimum lowered: gemm_bf16_big_kernel wherever M, N >= 192

Buffers: x and dz lie inside larger NaN-filled allocations with (K - 1) dil (at least 1) guard rows before and after, so a read outside the
operand shows as NaN in the result; every output has a row pitch of N + 8 and two rows before and after it, all NaN-filled apart from the
slab's and the `accumulate` form's start values: the product's M x N elements must be finite afterwards and everything around them still NaN.

Judged per slice on the slice's own scale (y, dx, dx_acc: every output row; dw: every tap's [cin, cout] block); bound 8 x e32, e32 = the worst
slice error of the checker's float32 evaluation, floor 1e-6.

Which kernel the dispatch conditions (csrc/gemm.hip, csrc/gemm_bf16.hip; restated by conv_window_ref.selected_kernel, printed by every
test) select, per case, product (dx and dx_acc are one product) and form.  F: gemm_kernel on v_mfma_f32_32x32x2_f32 (F32: its 32-row tile);
S: gemm_split_kernel, Sc: with every tile cut along K by the library, Sca: and the tail activation kernel behind it; SB: gemm_split_big_kernel;
b: gemm_bf16_kernel (bc: a K-cut of the library's own is possible), bB: gemm_bf16_big_kernel:
  case              M x N x K, split_k     f32_mfma     split_128    split_big    default_det  bf16_128     bf16_big
  bank_k1       y   165 x 128 x 80         F            F            F            F            b            b
  bank_k1       dw  80 x 128 x 165, 2      F            S            S            S            b            b
  bank_k1       dx  165 x 80 x 128         F            F            F            F            bc           bc
  bank_k2       y   165 x 128 x 160        F            S            S            S            b            b
  bank_k2       dw  160 x 128 x 165, 2     F            S            S            S            b            b
  bank_k2       dx  165 x 80 x 256         F            S            S            S            bc           bc
  bank_k3       y   165 x 128 x 240        F            S            S            S            b            b
  bank_k3       dw  240 x 128 x 165, 2     F            S            S            S            b            b
  bank_k3       dx  165 x 80 x 384         F            S            S            S            bc           bc
  bank_k4       y   165 x 128 x 320        F            S            S            S            b            b
  bank_k4       dw  320 x 128 x 165, 2     F            S            S            S            b            b
  bank_k4       dx  165 x 80 x 512         F            Sc           Sc           S            bc           bc
  bank_k5       y   165 x 128 x 400        F            S            S            S            b            b
  bank_k5       dw  400 x 128 x 165, 2     F            S            S            S            b            b
  bank_k5       dx  165 x 80 x 640         F            Sc           Sc           S            bc           bc
  bank_k6       y   165 x 128 x 480        F            S            S            S            b            b
  bank_k6       dw  480 x 128 x 165, 2     F            S            S            S            b            b
  bank_k6       dx  165 x 80 x 768         F            Sc           Sc           S            bc           bc
  bank_k7       y   165 x 128 x 560        F            Sca          Sca          S            b            b
  bank_k7       dw  560 x 128 x 165, 2     F            S            S            S            b            b
  bank_k7       dx  165 x 80 x 896         F            Sc           Sc           S            bc           bc
  bank_k8       y   165 x 128 x 640        F            Sca          Sca          S            b            b
  bank_k8       dw  640 x 128 x 165, 2     F            S            S            S            b            b
  bank_k8       dx  165 x 80 x 1024        F            Sc           Sc           S            bc           bc
  t32           y   192 x 48 x 160         F            S            S            S            bc           bc
  t32           dw  160 x 48 x 192, 2      F            S            S            S            b            b
  t32           dx  192 x 32 x 240         F            S            S            S            bc           bc
  t31           y   186 x 48 x 160         F            F            F            F            bc           bc
  t31           dw  160 x 48 x 186, 2      F            F            F            F            b            b
  t31           dx  186 x 32 x 240         F            F            F            F            bc           bc
  t_below_k     y   12 x 128 x 640         F32          F32          F32          F32          b            b
  t_below_k     dw  640 x 128 x 12, 2      F            F            F            F            b            b
  t_below_k     dx  12 x 80 x 1024         F32          F32          F32          F32          bc           bc
  t_one         y   1 x 128 x 640          F32          F32          F32          F32          b            b
  t_one         dw  640 x 128 x 1, 2       F            F            F            F            b            b
  t_one         dx  1 x 80 x 1024          F32          F32          F32          F32          bc           bc
  proj1         y   194 x 256 x 3072       F            Sca          SB           S            b            bB
  proj1         dw  3072 x 256 x 194, 2    F            S            SB           S            b            bB
  proj1         dx  194 x 1024 x 768       F            Sc           SB           S            bc           bB
  proj2         y   194 x 80 x 768         F            Sc           Sc           S            bc           bc
  proj2         dw  768 x 80 x 194, 2      F            S            S            S            b            b
  proj2         dx  194 x 256 x 240        F            S            SB           S            bc           bB
  enc_post      y   201 x 512 x 2560       F            Sca          SB           S            b            bB
  enc_post      dw  2560 x 512 x 201, 2    F            S            SB           S            b            bB
  enc_post      dx  201 x 512 x 2560       F            Sc           SB           S            bc           bB
  enc_post_out  y   201 x 80 x 2560        F            Sca          Sca          S            b            b
  enc_post_out  dw  2560 x 80 x 201, 2     F            S            S            S            b            b
  enc_post_out  dx  201 x 512 x 400        F            S            SB           S            bc           bB
  enc_post_in   y   201 x 512 x 400        F            S            SB           S            b            bB
  enc_post_in   dw  400 x 512 x 201, 2     F            S            SB           S            b            bB
  enc_post_in   dx  201 x 80 x 2560        F            Sc           Sc           S            bc           bc
  wn_d1         y   280 x 512 x 768        F            Sc           SB           S            bc           bB
  wn_d1         dw  768 x 512 x 280, 2     F            S            SB           S            b            bB
  wn_d1         dx  280 x 256 x 1536       F            Sc           SB           S            bc           bB
  wn_d4         y   280 x 512 x 768        F            Sc           SB           S            bc           bB
  wn_d4         dw  768 x 512 x 280, 2     F            S            SB           S            b            bB
  wn_d4         dx  280 x 256 x 1536       F            Sc           SB           S            bc           bB
  wn_d128       y   280 x 512 x 768        F            Sc           SB           S            bc           bB
  wn_d128       dw  768 x 512 x 280, 2     F            S            SB           S            b            bB
  wn_d128       dx  280 x 256 x 1536       F            Sc           SB           S            bc           bB
  wn_d256       y   280 x 512 x 768        F            Sc           SB           S            bc           bB
  wn_d256       dw  768 x 512 x 280, 2     F            S            SB           S            b            bB
  wn_d256       dx  280 x 256 x 1536       F            Sc           SB           S            bc           bB
  bank_long_k1  dw  80 x 128 x 16441, 64   F            S            S            S            b            b
  bank_long_k8  dw  640 x 128 x 16441, 51  F            S            S            S            b            b

Measured on an MI355X, per case and quantity the form with the largest error / bound, in units of 1e-7, e32 -> kernel; left the four
mstts_gemm_f32 forms, right the two mstts_gemm_bf16 forms against the bf16-rounded statements (e32 is the float32 evaluation on the CPU of
that run):
  case          y           dw          dx          dx_acc      |  y           dw          dx          dx_acc
  bank_k1       5.4->5.4    4.8->2.4    6.3->6.3    4.9->4.9    |  2.5->2.2    1.4->1.0    2.1->1.9    1.7->1.5
  bank_k2       7.7->7.7    4.3->2.9    7.5->7.5    7.9->7.9    |  3.3->1.8    2.1->1.3    3.6->1.7    2.8->1.3
  bank_k3       8.0->8.9    5.2->4.1    10.0->10.0  9.9->9.9    |  4.4->2.7    2.2->1.9    4.2->2.0    3.7->1.4
  bank_k4       10.0->10.0  4.8->2.9    8.6->11.0   7.4->8.7    |  5.4->3.3    2.6->1.6    3.8->1.6    3.1->1.5
  bank_k5       10.0->10.0  5.7->3.6    8.7->12.0   5.6->9.0    |  6.5->4.4    2.6->2.1    3.5->1.6    3.2->1.7
  bank_k6       6.5->13.0   5.9->3.1    9.5->16.0   7.2->12.0   |  2.5->3.8    2.4->1.5    5.4->1.8    4.4->1.8
  bank_k7       7.0->13.0   5.4->3.0    12.0->14.0  11.0->12.0  |  3.3->3.9    2.2->1.6    5.4->1.8    3.5->2.1
  bank_k8       6.7->12.0   5.5->3.6    9.9->17.0   7.3->13.0   |  4.3->5.0    2.4->1.7    4.4->2.6    3.7->2.0
  t32           8.2->8.2    4.7->2.6    8.3->8.7    5.8->7.1    |  2.4->1.8    2.5->1.1    3.2->2.7    2.9->2.9
  t31           7.1->7.1    4.7->3.5    8.6->8.6    7.8->7.8    |  2.6->2.3    2.5->1.4    3.3->2.3    3.1->1.8
  t_below_k     7.8->7.8    1.2->1.2    6.0->6.0    4.3->4.3    |  2.5->2.0    0.8->0.7    3.5->1.4    2.0->1.0
  t_one         0.6->1.0    0.5->0.5    1.7->2.7    0.6->1.0    |  0.8->0.8    0.4->0.4    0.9->0.6    0.3->0.5
  proj1         7.8->31.0   6.7->4.3    10.0->17.0  5.3->8.5    |  3.8->11.0   2.9->1.4    4.8->5.0    2.1->2.2
  proj2         9.1->15.0   5.8->3.5    7.6->7.6    3.7->3.7    |  5.8->2.0    2.9->1.2    3.3->2.4    1.6->1.4
  enc_post      21.0->44.0  6.7->4.2    7.3->27.0   5.6->21.0   |  8.1->16.0   3.2->1.5    3.3->11.0   2.3->7.2
  enc_post_out  16.0->32.0  6.5->4.0    12.0->12.0  4.0->4.0    |  7.1->10.0   3.4->1.5    5.8->3.4    2.1->1.3
  enc_post_in   18.0->18.0  6.4->4.0    8.0->29.0   7.4->25.0   |  7.9->5.4    2.8->1.6    3.6->2.5    3.4->3.3
  wn_d1         9.6->17.0   8.1->3.9    8.5->20.0   6.9->17.0   |  5.5->4.7    2.5->1.9    5.1->7.2    4.0->6.6
  wn_d4         9.5->17.0   6.4->5.1    11.0->24.0  8.3->18.0   |  4.0->5.3    3.3->1.7    4.3->9.8    4.6->7.2
  wn_d128       9.2->11.0   7.9->4.2    8.4->15.0   6.0->11.0   |  4.3->3.0    3.0->1.4    4.6->5.0    2.6->4.2
  wn_d256       4.7->7.9    6.5->3.9    9.7->15.0   6.5->10.0   |  2.2->2.7    3.2->1.5    5.3->4.5    4.1->3.1
  bank_long_k1  -           4.1->4.3    -           -           |  -           2.4->2.6    -           -
  bank_long_k8  -           4.8->5.0    -           -           |  -           4.1->3.0    -           -
No form of any case needs more than 4.0 x e32 (y of proj1 on the f32-input MFMA, a 3 072-term fmaf chain: 3.1e-6 against e32 7.8e-7); the
worst error / bound is 0.50.  Where a figure equals its e32 the fallback kernel's fmaf chain and the CPU's float32 product add the terms in
the same order.  Every output stayed NaN outside its M x N elements, none of them kept a NaN, no operand changed.
"""
import numpy as np
import pytest
import torch

from multi_speaker_tts_amd import lib
from tests import conv_window_ref as R
from tests.gemm_forms import FORMS, _defaults, _form        # the six forms, shared with tests/test_gpu_gemm_plain_ref.py

pytestmark = pytest.mark.gpu
SLACK, EDGE = 8, 2            # NaN columns right of every output row, NaN rows before and after every output


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def uploads():
    cache = {}
    yield cache
    cache.clear()


def _t(dev, a):
    return torch.tensor(np.array(a, np.float32), device=dev)          # (a copy: the case data is read-only)


def _guarded(dev, a, guard):
    """(allocation, view): the rows of `a` [rows, C] inside a NaN-filled allocation with `guard` rows before and after."""
    rows, C = a.shape
    full = torch.full((rows + 2 * guard, C), float("nan"), device=dev)
    full[guard:guard + rows] = _t(dev, a)
    return full, full[guard:guard + rows]


def _upload(dev, cache, name):
    """The operands of a case on the device, shared by its forms (one case kept at a time); the flipped kernel from mstts_conv_kernel_flip."""
    if name in cache:
        return cache[name]
    cache.clear()
    cd = R.case_data(name)
    rows, cin, cout, K = cd["B"] * cd["T"], cd["cin"], cd["cout"], cd["K"]
    guard = max((K - 1) * cd["dil"], 1)
    u = dict(guard=guard)
    u["x_full"], u["x"] = _guarded(dev, cd["x"].reshape(rows, cin), guard)
    u["dz_full"], u["dz"] = _guarded(dev, cd["dz"].reshape(rows, cout), guard)
    u["w"] = _t(dev, cd["w"])
    u["bias"] = _t(dev, cd["bias"])
    u["wt"] = torch.full((K, cout, cin), float("nan"), device=dev)
    lib.call("mstts_conv_kernel_flip", lib.ptr(u["w"]), lib.ptr(u["wt"]), K, cin, cout)
    torch.cuda.synchronize()
    assert np.array_equal(u["wt"].cpu().numpy(), R.flip(cd["w"])), "mstts_conv_kernel_flip: not wt[K-1-k][o][c] = w[k][c][o]"
    cache[name] = u
    return u


def _out(dev, M, N, start=None):
    """A NaN-filled [EDGE + M + EDGE, N + SLACK] allocation, the product's M x N elements set to `start` where given; (allocation, element offset)."""
    buf = torch.full((M + 2 * EDGE, N + SLACK), float("nan"), device=dev)
    if start is not None:
        buf[EDGE:EDGE + M, :N] = _t(dev, start).reshape(M, N)
    return buf, EDGE * (N + SLACK)


def _take(buf, M, N, what, failures):
    """The product's elements as float64; records a failure if one is not finite or anything around them is no longer NaN."""
    got = buf[EDGE:EDGE + M, :N].double().cpu().numpy()
    if not np.isfinite(got).all():
        failures.append((what, "not finite: the output kept its NaN fill or the product read outside its operand"))
    around = bool(torch.isnan(buf[:EDGE]).all()) and bool(torch.isnan(buf[EDGE + M:]).all()) and bool(torch.isnan(buf[:, N:]).all())
    if not around:
        failures.append((what, "wrote outside the product's rows and columns"))
    return got


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(R.CASES))
def test_conv_window_products_against_the_checker(dev, uploads, name, form):
    assert (lib.ACT_NONE, lib.ACT_RELU, lib.ACT_TANH) == (R.ACTS["none"], R.ACTS["relu"], R.ACTS["tanh"])
    cd = R.case_data(name)
    B, T, cin, cout, K, dil = (cd[k] for k in ("B", "T", "cin", "cout", "K", "dil"))
    rows, pad = B * T, R.pad_of(K)
    want = R.quantities(name)
    prods = R.products(name)
    u = _upload(dev, uploads, name)
    snap = {k: u[k].clone() for k in ("x_full", "dz_full", "w", "wt", "bias")}
    failures, got = [], {}
    with _form(form) as f:
        g = dict(bf16=f["bf16"])
        if "y" in want:
            y, off = _out(dev, rows, cout)
            lib.gemm(u["x"], u["w"], y, rows, cout, K * cin, cin, cout, cout + SLACK, bias=u["bias"], act=R.ACTS[cd["act"]], win=(T, cin, pad, dil), c_off=off, **g)
        if "dw" in want:
            dw, off = _out(dev, K * cin, cout, cd["dw0"])
            lib.gemm(u["x"], u["dz"], dw, K * cin, cout, rows, cin, cout, cout + SLACK, trans_a=True, win=(T, cin, pad, dil), split_k=prods["dw"][6], c_off=off, **g)
        if "dx" in want:
            dx, off = _out(dev, rows, cin)
            lib.gemm(u["dz"], u["wt"], dx, rows, cin, K * cout, cout, cin, cin + SLACK, win=(T, cout, K - 1 - pad, dil), c_off=off, **g)
            dxa, off = _out(dev, rows, cin, cd["dx0"])
            lib.gemm(u["dz"], u["wt"], dxa, rows, cin, K * cout, cout, cin, cin + SLACK, win=(T, cout, K - 1 - pad, dil), accumulate=True, c_off=off, **g)
        torch.cuda.synchronize()
    if "y" in want:
        got["y"] = _take(y, rows, cout, "y", failures)
    if "dw" in want:
        got["dw"] = _take(dw, K * cin, cout, "dw", failures)
    if "dx" in want:
        got["dx"], got["dx_acc"] = _take(dx, rows, cin, "dx", failures), _take(dxa, rows, cin, "dx_acc", failures)
    for k, v in snap.items():
        if not torch.equal(v.view(torch.int32), u[k].view(torch.int32)):
            failures.append((k, "an operand changed"))
    ref, e32 = R.reference(name, rounded=f["bf16"])
    line = []
    for k in want:
        err, bound = R.judge(k, got[k], ref[k], e32[k])
        line.append("%s %.1e/%.1e%s" % (k, err, e32[k], "" if err <= bound else " FAIL"))
        if not err <= bound:
            failures.append((k, "err %.3e" % err, "e32 %.3e" % e32[k], "bound %.3e" % bound))
    print("%-13s %-11s %s   [%s]" % (name, form, "  ".join(line), "; ".join("%s: %s" % (k, R.selected_kernel(form, *prods[k])) for k in prods)))
    assert not failures, failures


def test_switches_are_back_at_their_defaults(dev):
    """What a form leaves behind: the default schedule gives, bit for bit, what a fresh _defaults() gives (a form that leaked split3(0) or a
    lowered minimum would move summation orders), and deterministic mode is off on this thread (nesting depth 0)."""
    assert getattr(lib.deterministic_gemm._depth, "n", 0) == 0
    name = "proj2"
    cd = R.case_data(name)
    rows, cin, cout, K, T = cd["B"] * cd["T"], cd["cin"], cd["cout"], cd["K"], cd["T"]
    x = _t(dev, cd["x"]).reshape(rows, cin)
    dz = _t(dev, cd["dz"]).reshape(rows, cout)
    outs = []
    for fresh in (False, True):
        if fresh:
            _defaults(lib.load())
        dw = torch.zeros(K * cin, cout, device=dev)
        with lib.deterministic_gemm():        # split_k = 1: one fixed summation order per element, so equal settings give equal bits
            lib.gemm(x, dz, dw, K * cin, cout, rows, cin, cout, cout, trans_a=True, win=(T, cin, R.pad_of(K)))
        outs.append(dw.cpu())
    assert torch.equal(outs[0], outs[1])
