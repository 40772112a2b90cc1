"""The plain (win_T == 0) products of mstts_gemm_f32 / mstts_gemm_bf16 against the fp64 checker tests/gemm_plain_ref.py (pinned without a GPU by
tests/test_cpu_gemm_plain_ref.py: an independent formulation, planted faults, path coverage), every form of tests/gemm_forms.py on its own -
never one form against another.  The window half of the kernel table is tests/test_gpu_conv_window_ref.py's.

A case is a descriptor; its operands are the checker's flat float32 buffers, uploaded as they are: NaN in every pitch element, in at least one row
before the base (plus the case's offset) and after the last row, and in the gaps between batches, so a read past K, past a row's end or in front
of a misaligned base shows as NaN in the result.  The output is a NaN-filled [2 + M + 2, ldc] allocation (per batch, NaN gaps between), ldc >=
N + 8, holding start values only where the product lands on them (accumulate, split_k > 1).  Afterwards the M x N elements are finite, everything
around them is still NaN, and both operands and the bias are bit-identical to their snapshots.

Judged per output row on the row's own scale; bound 8 x e32 (e32 = the worst row error of the checker's float32 evaluation), floor 1e-6 - the
project's rule (slice_err, MARGIN, FLOOR of tests/lstm_seq_ref.py); the mstts_gemm_bf16 forms against the checker's bf16-rounded statements.

test_selection_products checks the exact-split claim of include/mstts.h where the answer is known: every output is ONE product (one operand
holds a single non-zero per reduction, the other full-mantissa values), at 132 x 136 x 164 and 194 x 260 x 768 (big tiles), nn and nt.  f32_mfma
gives the selected element exactly where the selector's entries are 1.0, the bf16 forms the product of the bf16-rounded pair exactly, the three
split forms the exact product within gemm_plain_ref.SPLIT_BOUND = 6 (1 + 2^-7) 2^-24 + (1 + 2^-9) 2^-26 = 3.76e-7 of it (derived there from the
header's statement: six fp32 accumulations, dropped terms <= 2^-26); the CPU test shows that a lost plane or product leaves that bound.

K == 0 (k0_nn, k0_acc_nn) is the empty sum in every form: act(bias), and C0 + bias with accumulate (stated in include/mstts.h).

Which kernel the dispatch conditions (csrc/gemm.hip, csrc/gemm_bf16.hip; restated by gemm_plain_ref.selected_kernel, printed by every test)
select, per case and form.  F32 / F64 / F128: gemm_kernel on v_mfma_f32_32x32x2_f32 at its 32- / 64- / 128-row tile, +t: body + tail, +ta: with the
tail activation kernel; S: gemm_split_kernel, whole tiles, Sc: every tile cut along K by the library, Sca: and the tail activation behind it,
Sta: body + tail with the tail activation; SB: gemm_split_big_kernel; b: gemm_bf16_kernel, bN: cut into N pieces by the library; bB:
gemm_bf16_big_kernel.  Loads: v vector, s scalar through (d)imensions, (b)ase, (p)itch or batch stride:
  case                     M x N x K                        loads   f32_mfma    split_128   split_big   default_det bf16_128    bf16_big
  lay_vec_nn           nn  132 x 136 x 164                  v       F64         S           S           S           b           b
  lay_scalar_nn        nn  131 x 83 x 161                   s(d,p)  F64         S           S           S           b           b
  rows32_nn            nn  32 x 136 x 260                   v       F32         F32         F32         F32         b2          b2
  rows33_nn            nn  33 x 136 x 260                   v       F128        S           S           S           b2          b2
  big_nn               nn  194 x 260 x 768                  v       F64         Sca         SB          S           b           bB
  lay_vec_nt           nt  132 x 136 x 164                  v       F64         S           S           S           b           b
  lay_scalar_nt        nt  131 x 83 x 161                   s(d,p)  F64         S           S           S           b           b
  rows32_nt            nt  32 x 136 x 260                   v       F32         F32         F32         F32         b2          b2
  rows33_nt            nt  33 x 136 x 260                   v       F128        S           S           S           b2          b2
  big_nt               nt  194 x 260 x 768                  v       F64         Sc          SB          S           b6          bB
  lay_vec_tn           tn  132 x 136 x 164                  v       F64         S           S           S           b           b
  lay_scalar_tn        tn  131 x 83 x 161                   s(d)    F64         S           S           S           b           b
  rows32_tn            tn  32 x 136 x 260                   v       F32         F32         F32         F32         b2          b2
  rows33_tn            tn  33 x 136 x 260                   s(d,p)  F128        S           S           S           b2          b2
  big_tn               tn  194 x 260 x 768                  s(d,p)  F64         Sc          SB          S           b6          bB
  lay_vec_tt           tt  132 x 136 x 164                  v       F64         S           S           S           b           b
  lay_scalar_tt        tt  131 x 83 x 161                   s(d,p)  F64         S           S           S           b           b
  rows32_tt            tt  32 x 136 x 260                   v       F32         F32         F32         F32         b2          b2
  rows33_tt            tt  33 x 136 x 260                   s(d,p)  F128        S           S           S           b2          b2
  big_tt               tt  194 x 260 x 768                  s(d,p)  F64         Sc          SB          S           b6          bB
  lay_offset_nn        nn  132 x 136 x 164                  s(b)    F64         S           S           S           b           b
  lay_pitch1_nn        nn  132 x 136 x 164                  s(p)    F64         S           S           S           b           b
  lay_offset_nt        nt  132 x 136 x 164                  s(b)    F64         S           S           S           b           b
  lay_pitch1_nt        nt  132 x 136 x 164                  s(p)    F64         S           S           S           b           b
  lay_offset_tn        tn  132 x 136 x 164                  s(b)    F64         S           S           S           b           b
  lay_pitch1_tn        tn  132 x 136 x 164                  s(p)    F64         S           S           S           b           b
  k159_nn              nn  132 x 136 x 159                  s(d)    F64         F64         F64         F64         b           b
  k160_nn              nn  132 x 136 x 160                  v       F64         S           S           S           b           b
  k159_nt              nt  132 x 136 x 159                  s(d,p)  F64         F64         F64         F64         b           b
  k160_nt              nt  132 x 136 x 160                  v       F64         S           S           S           b           b
  one_nn               nn  1 x 1 x 52                       s(d,p)  F32         F32         F32         F32         b           b
  col1_nn              nn  70 x 1 x 36                      s(d,p)  F64         F64         F64         F64         b           b
  one_tn               tn  1 x 1 x 52                       s(d,p)  F32         F32         F32         F32         b           b
  col1_tn              tn  70 x 1 x 36                      s(d,p)  F64         F64         F64         F64         b           b
  big_ktail_tn         tn  256 x 192 x 168, split_k 2       v       F64         S           SB          S           b           bB
  dx_form_nt           nt  165 x 80 x 512                   v       F64         Sc          Sc          S           b4          b4
  dx_form_act_nt       nt  165 x 80 x 512                   v       F64         Sca         Sca         S           b           b
  acc_act_nn           nn  165 x 80 x 512                   v       F64         S           S           S           b           b
  splitk_empty_tn      tn  132 x 136 x 164, split_k 8       v       F64         S           S           S           b           b
  alpha_nn             nn  132 x 136 x 164                  v       F64         S           S           S           b           b
  alpha_tt             tt  132 x 136 x 164                  v       F64         S           S           S           b           b
  batch_tn             tn  68 x 72 x 164, batch 3, split 2  v       F64         S           S           S           b           b
  batch_odd_nn         nn  68 x 72 x 164, batch 3           s(p)    F64         S           S           S           b           b
  f128_nn              nn  256 x 1024 x 36, batch 16        v       F128        F128        F128        F128        -           -
  tail_f_nt            nt  2112 x 1024 x 512                v       F64+t       S           SB          S           b3          bB
  tail_s_nt            nt  4224 x 1024 x 512                v       F64+ta      Sta         SB          S           b           bB
  tail_f_mixed_nt      nt  2112 x 1152 x 512                v       F64+t       S           SB          S           b3          bB
  band_nn              nn  260 x 2820 x 164                 v       F64         S           SB          S           b           bB
  big_splitk_empty_tn  tn  256 x 192 x 168, split_k 8       v       F64         S           SB          S           b           bB
  k0_nn                nn  40 x 24 x 0                      v       F128        F128        F128        F128        b           b
  k0_acc_nn            nn  40 x 24 x 0                      v       F128        F128        F128        F128        b           b

Measured on an MI355X, per case the form with the largest error / bound, in units of 1e-7, e32 -> that form's error; left the four mstts_gemm_f32 forms,
right the two mstts_gemm_bf16 forms against the bf16-rounded statements (e32 is the float32 evaluation on the CPU of that run):
  case                 mstts_gemm_f32 forms     |  mstts_gemm_bf16 forms
  lay_vec_nn           7.2->7.2 f32_mfma        |  2.9->2.2 bf16_128
  lay_scalar_nn        6.5->6.5 f32_mfma        |  3.1->2.1 bf16_128
  rows32_nn            7.7->7.7 f32_mfma        |  2.3->1.7 bf16_128
  rows33_nn            7.5->7.5 f32_mfma        |  3.7->1.8 bf16_128
  big_nn               22.9->21.5 f32_mfma      |  10.4->7.5 bf16_128
  lay_vec_nt           7.5->7.5 f32_mfma        |  3.2->2.0 bf16_128
  lay_scalar_nt        5.8->5.8 f32_mfma        |  3.3->2.8 bf16_128
  rows32_nt            6.9->6.9 f32_mfma        |  3.9->1.7 bf16_128
  rows33_nt            6.8->9.8 split_128       |  3.3->1.6 bf16_128
  big_nt               10.6->16.3 f32_mfma      |  4.2->5.2 bf16_big
  lay_vec_tn           7.0->7.5 split_128       |  3.8->2.0 bf16_128
  lay_scalar_tn        7.1->7.1 f32_mfma        |  2.4->2.1 bf16_128
  rows32_tn            6.7->6.7 f32_mfma        |  2.9->2.0 bf16_128
  rows33_tn            9.5->9.5 f32_mfma        |  4.8->2.0 bf16_128
  big_tn               7.1->14.4 f32_mfma       |  3.7->4.9 bf16_big
  lay_vec_tt           6.1->7.0 split_128       |  2.7->2.0 bf16_128
  lay_scalar_tt        6.7->6.7 split_128       |  3.0->2.1 bf16_128
  rows32_tt            6.3->6.3 f32_mfma        |  3.5->2.1 bf16_128
  rows33_tt            6.0->7.9 split_128       |  2.8->1.4 bf16_128
  big_tt               8.7->15.1 f32_mfma       |  4.3->6.3 bf16_big
  lay_offset_nn        8.2->8.2 f32_mfma        |  2.9->2.1 bf16_128
  lay_pitch1_nn        9.2->9.2 f32_mfma        |  2.8->2.7 bf16_128
  lay_offset_nt        6.3->6.3 f32_mfma        |  3.0->2.1 bf16_128
  lay_pitch1_nt        5.7->5.7 f32_mfma        |  2.8->2.2 bf16_128
  lay_offset_tn        7.4->7.4 f32_mfma        |  3.2->2.4 bf16_128
  lay_pitch1_tn        5.9->5.9 f32_mfma        |  3.2->2.2 bf16_128
  k159_nn              8.9->8.9 f32_mfma        |  3.1->2.1 bf16_128
  k160_nn              6.5->6.7 split_128       |  2.5->2.1 bf16_128
  k159_nt              6.3->6.3 f32_mfma        |  2.7->1.7 bf16_128
  k160_nt              6.2->7.6 split_128       |  2.6->2.8 bf16_128
  one_nn               0.6->0.5 f32_mfma        |  0.6->0.6 bf16_128
  col1_nn              17.3->39.8 f32_mfma      |  2.6->2.6 bf16_128
  one_tn               0.4->1.6 f32_mfma        |  0.4->0.4 bf16_128
  col1_tn              12.1->15.8 f32_mfma      |  11.3->3.1 bf16_128
  big_ktail_tn         6.1->3.6 split_big       |  2.6->1.5 bf16_128
  dx_form_nt           6.9->10.0 f32_mfma       |  2.6->1.4 bf16_128
  dx_form_act_nt       7.3->11.9 f32_mfma       |  5.0->4.1 bf16_128
  acc_act_nn           5.8->5.8 f32_mfma        |  1.9->1.9 bf16_128
  splitk_empty_tn      4.7->2.2 default_det     |  1.9->1.1 bf16_big
  alpha_nn             4.0->4.0 f32_mfma        |  1.6->1.4 bf16_128
  alpha_tt             3.9->3.9 f32_mfma        |  1.8->1.4 bf16_128
  batch_tn             4.7->4.5 split_128       |  2.1->1.4 bf16_128
  batch_odd_nn         7.1->7.4 split_128       |  2.8->2.5 bf16_128
  f128_nn              4.5->4.5 f32_mfma        |  -
  tail_f_nt            8.6->13.7 f32_mfma       |  4.2->4.9 bf16_big
  tail_s_nt            8.9->15.2 f32_mfma       |  3.9->5.5 bf16_128
  tail_f_mixed_nt      9.3->13.9 split_128      |  4.8->4.6 bf16_big
  band_nn              7.5->7.5 f32_mfma        |  3.4->2.2 bf16_128
  big_splitk_empty_tn  5.8->2.1 default_det     |  2.1->1.9 bf16_big
  k0_nn                0.0->0.0 f32_mfma        |  0.0->0.0 bf16_128
  k0_acc_nn            0.5->0.5 f32_mfma        |  0.5->0.5 bf16_128
No form of any case needs more than 2.3 x e32 (col1_nn in f32_mfma: 4.0e-06 against e32 1.7e-06; cases on the 1e-6 floor aside); the worst error / bound is 0.29
(col1_nn in f32_mfma).  Where a figure equals its e32 the fallback kernel's fmaf chain and the CPU's float32 product add the terms in the same order.
Every output stayed NaN outside its M x N elements, none of them kept a NaN, no operand changed.
Selection products: the three split forms are within 0.71 x SPLIT_BOUND of the exact product (2.66e-07, s132_b_selects_val_nn in all three) and give the selected
element exactly (error 0) where the selector's entries are 1.0; f32_mfma is exact there and within 5.9e-08 (one rounding) on the full-mantissa
selectors; both bf16 forms give the product of the bf16-rounded pair exactly.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from multi_speaker_tts_amd import lib
from tests import gemm_plain_ref as R
from tests.gemm_forms import FORMS, _defaults, _form

pytestmark = pytest.mark.gpu
PAIRS = [(n, f) for n, c in R.CASES.items() for f in FORMS if f in c["forms"]]
SPLIT_FORMS = ("split_128", "split_big", "default_det")


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


def _upload(dev, cache, cd):
    """The flat operands of a case on the device with their snapshots, shared by its forms (one case kept at a time)."""
    if cd["name"] not in cache:
        cache.clear()
        u = {k: _t(dev, cd[k]) for k in ("flat_a", "flat_b", "bias_v")}
        u["snap"] = {k: v.clone() for k, v in u.items()}
        cache[cd["name"]] = u
    return cache[cd["name"]]


def _run(dev, uploads, cd, form, failures):
    """The product of a case in a form: the flat output back on the host, (what, ...) appended to `failures` for every broken invariant."""
    assert (lib.ACT_NONE, lib.ACT_RELU, lib.ACT_TANH) == (R.ACTS["none"], R.ACTS["relu"], R.ACTS["tanh"])
    assert lib.load().mstts_abi_version() == lib.ABI_VERSION == 5
    u = _upload(dev, uploads, cd)
    out = _t(dev, cd["flat_c"])
    with _form(form) as f:
        lib.gemm(u["flat_a"], u["flat_b"], out, cd["M"], cd["N"], cd["K"], cd["lda"], cd["ldb"], cd["ldc"], bias=u["bias_v"] if cd["bias"] else None,
                 trans_a=cd["ta"], trans_b=cd["tb"], act=R.ACTS[cd["act"]], accumulate=cd["accumulate"], split_k=cd["split_k"], batch=cd["batch"],
                 strides=(cd["stride_a"], cd["stride_b"], cd["stride_c"]), alpha=cd["alpha"], a_off=cd["a_off"], b_off=cd["b_off"], c_off=cd["c_off"],
                 bf16=f["bf16"])
        torch.cuda.synchronize()
    flat = out.cpu().numpy()
    if not np.isfinite(R.taken(cd, flat)).all():
        failures.append(("C", "not finite: the output kept its NaN fill or the product read outside its operand"))
    if not R.outside_is_nan(cd, flat):
        failures.append(("C", "wrote outside the product's rows and columns"))
    for k, v in u["snap"].items():
        if not torch.equal(v.view(torch.int32), u[k].view(torch.int32)):
            failures.append((k, "an operand changed"))
    return flat, f


@pytest.mark.parametrize("name,form", PAIRS)
def test_plain_products_against_the_checker(dev, uploads, name, form):
    cd = R.case_data(name)
    failures = []
    flat, f = _run(dev, uploads, cd, form, failures)
    ref, e32 = R.reference(name, rounded=f["bf16"])
    err, bound = R.judge(R.taken(cd, flat), ref, e32)
    print("%-18s %-11s err %.3e  e32 %.3e  bound %.3e%s   [%s; %s]" % (name, form, err, e32, bound, "" if err <= bound else " FAIL", R.selected_kernel(form, cd), R.loads(cd)))
    if not err <= bound:
        failures.append(("C", "err %.3e" % err, "e32 %.3e" % e32, "bound %.3e" % bound))
    assert not failures, failures


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", R.SEL_NAMES)
def test_selection_products(dev, uploads, name, form):
    cd = R.selection_data(name)
    failures = []
    flat, f = _run(dev, uploads, cd, form, failures)
    want, bound = cd["exact"], R.SPLIT_BOUND
    if f["bf16"]:        # the product of the bf16-rounded pair: 8 + 8 significand bits, exact in fp32, plus zeros
        want, bound = R.bf16_round(cd["op_a"]).astype(np.float64) @ R.bf16_round(cd["op_b"]).astype(np.float64), 0.0
    elif form == "f32_mfma" and cd["way"].endswith("_one"):           # the selected element itself
        bound = 0.0
    err = R.selection_err(R.taken(cd, flat), want)
    print("%-26s %-11s err %.3e  bound %.3e%s   [%s]" % (name, form, err, bound, "" if err <= bound else " FAIL", R.selected_kernel(form, cd)))
    if not err <= bound:
        failures.append(("C", "err %.3e" % err, "bound %.3e" % bound))
    assert not failures, failures


def _desc(out, a, b, M, N, K, **kw):
    d = lib.GemmDesc()
    d.A, d.B, d.C = lib.ptr(a), lib.ptr(b), lib.ptr(out)
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc = M, N, K, max(K, 1), max(N, 1), max(N, 1) + 8
    d.alpha = 1.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_refusals_and_empty_products(dev):
    """gemm_args_from's host-side answers, none of which launches anything: an empty product is MSTTS_OK and writes nothing; split_k with an
    activation, a null operand and (mstts_gemm_f32 only: 32-bit tile-relative offsets) a row stride of 2^24 return a non-zero status, name their
    entry point in mstts_last_error() and write nothing."""
    L = lib.load()
    a, b = torch.ones(64, 64, device=dev), torch.ones(64, 64, device=dev)
    out = torch.full((20, 24), float("nan"), device=dev)
    for fn, who in ((L.mstts_gemm_f32, "gemm:"), (L.mstts_gemm_bf16, "gemm_bf16:")):
        for M, N in ((0, 16), (16, 0), (0, 0)):
            assert fn(C.byref(_desc(out, a, b, M, N, 16)), lib.stream()) == 0
        assert fn(C.byref(_desc(out, None, None, 0, 16, 16)), lib.stream()) == 0          # (nothing of an empty product is looked at)
        refused = [_desc(out, a, b, 16, 16, 16, split_k=2, act=lib.ACT_RELU), _desc(out, None, b, 16, 16, 16), _desc(out, a, None, 16, 16, 16),
                   _desc(None, a, b, 16, 16, 16)]
        if who == "gemm:":
            refused.append(_desc(out, a, b, 16, 16, 16, lda=1 << 24))
        for d in refused:
            assert fn(C.byref(d), lib.stream()) != 0
            assert L.mstts_last_error().decode().startswith(who), L.mstts_last_error()
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())


def test_switches_are_back_at_their_defaults(dev):
    """What a form leaves behind: the default schedule gives, bit for bit, what a fresh _defaults() gives (a form that leaked split3(0), a lowered
    minimum or mstts_gemm_bf16_big(0) would move summation orders), and deterministic mode is off on this thread (nesting depth 0)."""
    assert getattr(lib.deterministic_gemm._depth, "n", 0) == 0
    cd = R.case_data("big_nt")
    a, b = _t(dev, cd["flat_a"]), _t(dev, cd["flat_b"])
    outs = []
    for fresh in (False, True):
        if fresh:
            _defaults(lib.load())
        for bf16 in (False, True):
            out = torch.zeros(cd["size_c"], device=dev)
            with lib.deterministic_gemm():        # no cut of the library's own: one fixed summation order per element, so equal settings give equal bits
                lib.gemm(a, b, out, cd["M"], cd["N"], cd["K"], cd["lda"], cd["ldb"], cd["ldc"], trans_b=True, a_off=cd["a_off"], b_off=cd["b_off"],
                         c_off=cd["c_off"], bf16=bf16)
            outs.append(out.cpu())
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3])
