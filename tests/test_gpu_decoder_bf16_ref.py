"""The bf16 forms (BASELINE config 3) of the teacher-forced decoder loop drivers and their BPTT, stage by stage against the fp64 checker
tests/decoder_bf16_ref.py - every form on its own, every stage of every step evaluated from the history the form itself stored, so that the
checker and the kernel round identical fp32 numbers to bf16 and the kernels are held to fp32-accumulation accuracy (the ~1e-6 of their fp32
siblings in tests/test_gpu_decoder_loop_ref.py) instead of the trajectory's flip noise (2e-3 .. 1e-1 in test_train_step_parity_bf16_* and
test_persistent_bf16_equals_launch_per_step_bf16):
    launch-per-step bf16, products   mstts_decoder_train_fwd / _bwd with the six bf_* copies only (w0p16 = w1p16 = act_p = wq_t = lsa.loc_kt = NULL):
                                     mstts_skinny_fwd_bf16 / mstts_skinny_bwd_bf16 for all six products, the query gradient as a product launch,
                                     mstts_lsa_step_fwd
    launch-per-step bf16, full       the same plus w0p16 / w1p16 / act_p, loc_kt + granule room, wq_t: fused bf16 cell steps (cell_fwd_bf16_kernel),
                                     mstts_lsa_step_fwd_q(bf16 = 1) and dq_bf16 inside cell 1's pointwise backward - at WIDE; MID admits none of the
                                     three (M + H = 192 is no multiple of 128, H = 64 none of 128) and runs the product launches again, asserted
    persistent bf16 forward          mstts_decoder_train_fwd_persistent, recurrent_bf16 = 1, pre / b0, opk = NULL (row-major histories); judged
                                     against the pre-form stages; xw0 points at NaN
    persistent bf16 forward + BPTT   the same with opk, mstts_decoder_train_bwd_persistent(recurrent_bf16 = 1) behind it, then
                                     mstts_persist_unpack_history; d_ctx from the first slab only, ctrl[1] == 0, ctrl[2] == 256
    plain_h32 with all six bf_*      mstts_decoder_bf16_splits admits no H = 32: the driver must run fp32, judged by decoder_loop_ref.judge
Descriptors are built by hand with the helpers of tests/test_gpu_decoder_loop_ref.py from the case data of tests/decoder_loop_ref.py; the bf16
copies are made as engine.py makes them.  Cases: those of decoder_loop_ref.CASES whose widths mstts_decoder_bf16_splits admits (asserted):
fused_h64, two_pass_t140 (MID), wide_one_tile, wide_two_tiles, wide_full, wide_t131 (WIDE).

Every buffer a form writes in full is NaN-filled and must be finite before anything is judged; decoder_loop_ref.exact_failures; the context
columns of in0 slot s + 1 bit-identical to those of pj slot s; d_pj bit-identical after either BPTT; the forms of a case share no output buffer.
Bound per quantity: MARGIN (8) x e32, e32 = the worst slice difference of the checker's own float32 and float64 evaluations on the form's
history; floor 1e-6.

The one family of rounding sites that is not fed from a stored tensor bit for bit (decoder_bf16_ref.PERSISTENT_SITES): the persistent launches
round the copy of m0, h0, h1, m1, the context and the gate gradients that ARRIVED through their rings, which carries the ring slot's generation in
its last mantissa bit (csrc/persist_common.h), while the histories keep the exact value.  Judged against bf(stored value), 1 - 3 elements of a
case (2^-17 of 1e5 .. 5e5) rounded the other way on an MI355X: wide_two_tiles acts0 3.3e-04 and acts1 2.3e-05, wide_full q_hist 3.4e-04,
wide_t131 acts1 5.5e-05 - 18 .. 180 x the bound in that one stage and step, every other stage at its usual 0.3 .. 2 x e32; wide_one_tile had
none.  The exchanged copy is a deterministic function of the stored value and the step, so the checker rounds exchanged_copy(stored value,
generation) - the number the kernel rounds - and the persistent forms meet the same 8 x e32 as every other form; no kernel changed.  (The
size is what the CPU controls predict for ONE operand element off by a bf16 ulp: truncate_cell1_operand does that to half of the 128 elements
of every row of one step and is reported at 2e3 x the bound.)

Measured on an MI355X, the form with the largest error / bound per case and quantity, in units of 1e-7, e32 -> kernel (q, align, cum, de, dq: the
*_hist tensors; e32 is the checker's float32 evaluation on that form's history, on that machine's CPU):
  case           acts0     craw0     c0        in0_h0    in1_m0    acts1     craw1     c1        in1_h1    pj_m1     q         align     cum       pj_ctx
  fused_h64      2.8->1.5  2.1->1.6  2.5->1.7  3.0->3.3  2.3->2.7  1.4->1.1  1.7->2.0  1.6->2.2  1.8->3.0  2.1->3.8  1.6->1.0  2.0->1.8  1.9->1.3  2.1->1.6
  two_pass_t140  2.1->1.5  1.3->1.6  1.3->1.8  2.5->3.6  1.8->3.2  1.0->0.9  1.5->1.5  1.2->1.6  1.7->3.1  2.1->3.1  1.1->1.1  1.1->1.0  0.8->0.6  1.6->3.3
  wide_one_tile  17.0->2.8 10.0->1.9 10.0->2.1 10.0->3.7 10.0->3.2 7.7->1.2  6.1->2.2  6.0->2.5  5.9->3.5  6.0->2.9  6.3->3.0  1.2->2.3  1.0->1.3  1.4->2.3
  wide_two_tiles 11.0->3.6 6.4->2.1  6.6->2.8  5.9->3.8  6.3->3.4  5.1->1.8  5.0->2.5  4.1->2.6  3.6->4.5  4.0->4.1  6.2->2.7  2.0->2.1  1.7->1.7  2.3->2.7
  wide_full      2.3->2.4  1.8->2.4  1.9->2.7  2.3->4.1  2.0->3.2  1.2->1.3  1.7->3.0  2.0->3.5  2.6->4.3  2.2->4.3  2.0->3.2  2.5->3.1  2.0->2.9  2.3->3.8
  wide_t131      6.5->3.5  4.7->2.6  3.5->2.4  4.1->3.0  4.7->3.0  3.6->1.2  4.3->2.0  4.3->2.1  4.4->3.4  4.7->3.2  4.7->2.2  2.0->2.0  1.1->1.5  2.4->2.8
  case           de        dq        dg1       dg0       d_in0     d_ctx     dw0f      dw1       db1       dwq       d_values
  fused_h64      3.1->3.2  5.0->9.0  1.9->2.2  2.3->2.3  1.8->1.2  1.8->1.0  0.4->0.3  0.2->0.2  1.0->1.1  0.5->0.6  1.5->1.4
  two_pass_t140  3.3->2.3  3.2->8.4  2.1->1.7  3.6->2.0  2.0->1.0  2.0->1.0  1.1->0.6  0.4->0.9  0.9->0.6  1.4->2.2  2.1->2.2
  wide_one_tile  2.4->3.7  4.6->14.0 2.9->2.4  9.6->3.9  6.9->1.1  8.9->1.5  1.8->0.6  1.3->0.6  1.5->1.4  1.4->1.4  1.8->2.0
  wide_two_tiles 4.0->6.4  11.0->31.0 3.0->3.0 5.8->3.0  6.4->1.4  7.6->2.0  0.3->0.4  0.1->0.1  0.9->1.0  0.4->0.6  2.0->2.8
  wide_full      3.9->7.4  7.1->13.0 2.7->2.7  4.6->3.2  3.1->1.3  3.4->2.0  0.2->0.2  0.1->0.1  0.8->1.0  0.2->0.4  2.6->3.0
  wide_t131      2.2->2.9  5.0->9.4  2.0->2.1  6.0->4.4  9.6->1.0  11.0->2.3 0.4->0.7  0.4->0.4  1.1->1.1  1.6->1.6  1.8->2.7
No form of any case needs more than 3.0 x e32 (dq_hist of wide_one_tile, launch-per-step bf16 full: 1.4e-6 against e32 4.6e-7 - the query
gradient cancels, as in the fp32 forms); the worst error / bound is 0.38.  At MID the two
launch-per-step forms select the same launches and agree to the last digit.  plain_h32 with the six bf_* pointers given reproduces the fp32 forms'
figures of test_gpu_decoder_loop_ref.py digit for digit.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from multi_speaker_tts_amd import lib
from tests import decoder_bf16_ref as Q
from tests import decoder_loop_ref as R
from tests.test_gpu_decoder_loop_ref import (A, KS, LPS_Q, _bwd_desc, _collect, _fwd_desc, _judge, _nan, _pdesc, _ran_to_its_end, _upload, _weights)

pytestmark = pytest.mark.gpu
LPS_BF16_Q = Q.FORWARD_Q + Q.BACKWARD_Q + Q.HOST_Q
WRITTEN = R.FORWARD_Q + ("dg0", "dg1", "dq_hist", "de_hist", "d_in0", "d_ctx")


@pytest.fixture(scope="module")
def wcache():
    cache = {}
    yield cache
    cache.clear()


def _judge_stagewise(name, label, form, got, notes, quantities, failures, packed=False, exchanged=False):
    """One printed line per form, in the format of test_gpu_decoder_loop_ref._judge: quantity error/e32.  exchanged: a persistent launch - its
    products round the exchanged copies of the stored values (decoder_bf16_ref.PERSISTENT_SITES)."""
    cd = R.case_data(name)
    before = len(failures)
    for k in WRITTEN:               # (the slots nothing writes - decoder_loop_ref.exclude_unwritten - were zeroed by _fwd_desc, not NaN-filled)
        if k in got and not np.isfinite(got[k]).all():
            failures.append((label, k, "not finite: a buffer the form writes in full kept its NaN fill"))
    for msg in notes + R.exact_failures(cd, got) + Q.context_identity_failures(cd, got):
        failures.append((label, msg))
    if len(failures) > before:
        return
    rows, errs, bounds = Q.judge(cd, form, got, quantities, packed=packed, exchanged=exchanged)
    print("%-15s %-30s %s" % (name, label, "  ".join("%s %.1e/%.1e%s" % (k, err, e32, "" if err <= bound else " FAIL") for k, e32, err, bound in rows)))
    for k, e32, err, bound in rows:
        if not err <= bound:
            failures.append((label, k, "err %.3e" % err, "e32 %.3e" % e32, "bound %.3e" % bound))
    over = [(st, s, "%.1f x bound" % v) for st, s, v in Q.judged_sequence(cd, errs, bounds) if v > 1.0]
    if over:
        failures.append((label, "first stage over its bound, in judged order", over[0]))


def _assert_bf16_tier(cd, w, full):
    """The full bf16 descriptor selects what the form is named after."""
    L = lib.load()
    B, T, H, M = cd["B"], cd["Te"], cd["H"], cd["M"]
    assert w["bf_ok"] and min(w["bf_splits"]) >= 1 and all(getattr(full, "bf_" + k) for k in ("w0f_f", "w1_f", "wq_f", "w0f_b", "w1_b", "wq_b"))
    wide = cd["widths"] == "WIDE"
    fused_cells = bool(L.mstts_cell_fwd_bf16_supported(H, M + H)) and bool(L.mstts_cell_fwd_bf16_supported(H, 2 * H))
    assert fused_cells == wide and bool(full.w0p16 and full.w1p16) == wide
    assert L.mstts_lsa_step_q_supported(T, M, H) == int(wide)
    if wide:
        assert full.act_p and M % 4 == 0                                                                             # fused bf16 cell steps
        assert full.lsa.loc_kt and full.energy_ws_floats >= L.mstts_lsa_step_q_ws_bytes(B, T) // 4 and (H + M) % 4 == 0    # query inside the attention launch, bf16 = 1
        assert full.wq_t and H % 128 == 0 and w["bf_splits"][4] in (1, 2, 4, 8) and B * H * 4 < 1 << 30              # dq_bf16 inside cell 1's pointwise backward
    else:
        assert H % 128 != 0                                                                                          # ... the query gradient stays a product launch


def test_the_cases_are_those_the_bf16_path_admits():
    L = lib.load()
    for name in R.CASES:
        dm = R.dims_of(R.CASES[name]["widths"])
        assert bool(L.mstts_decoder_bf16_splits(dm["H"], dm["M"], A, None)) == (name in Q.BF16_CASES), name
    assert Q.BF16_CASES == ("fused_h64", "two_pass_t140", "wide_one_tile", "wide_two_tiles", "wide_full", "wide_t131")


@pytest.mark.parametrize("name", Q.BF16_CASES)
def test_launch_per_step_bf16_forms_stage_by_stage(dev, wcache, name):
    cd = R.case_data(name)
    w, u = _weights(dev, wcache, cd["widths"], bf16=True), _upload(dev, cd)
    failures = []
    for form, tier in (("products", "nulled"), ("full", "full")):
        d, f = _fwd_desc(dev, cd, w, u, tier, bf16=form)
        if form == "full":
            _assert_bf16_tier(cd, w, d)
        else:
            assert not (d.w0p16 or d.w1p16 or d.act_p or d.wq_t or d.lsa.loc_kt) and w["bf_ok"]
        b, g = _bwd_desc(dev, cd, u, d, persistent=False)
        lib.call("mstts_decoder_train_fwd", C.byref(d))
        lib.call("mstts_decoder_train_bwd", C.byref(b))
        torch.cuda.synchronize()
        got, notes = _collect(cd, u, f, g)
        _judge_stagewise(name, "launch-per-step bf16, " + form, "xw0", got, notes, LPS_BF16_Q, failures)
    assert not failures, failures


@pytest.mark.parametrize("name", [n for n in Q.BF16_CASES if R.CASES[n]["widths"] == "WIDE"])
def test_persistent_bf16_forms_stage_by_stage(dev, wcache, name):
    cd = R.case_data(name)
    B, T, S, H, M = cd["B"], cd["Te"], cd["S"], cd["H"], cd["M"]
    L = lib.load()
    if not L.mstts_persist_fwd_supported(B, H, M, A, T, KS):
        pytest.skip("persistent loop not available on this device (needs 256 CUs and one workgroup per CU)")
    w, u = _weights(dev, wcache, cd["widths"], bf16=True), _upload(dev, cd)
    failures = []

    def forward(packed):
        d, f = _fwd_desc(dev, cd, w, u, "persistent", packed=packed)
        f["xw0_unused"] = _nan(dev, S, B, 4 * H)                    # the pre / b0 form ignores xw0
        d.xw0 = lib.ptr(f["xw0_unused"])
        p, pt = _pdesc(dev, w["pk"], int(L.mstts_persist_fwd_ws_bytes()), recurrent_bf16=1)
        p.pre, p.b0 = lib.ptr(u["pre"]), lib.ptr(w["b0"])
        if packed:
            f["opk"] = _nan(dev, int(L.mstts_persist_opk_floats(S)))
            p.opk = lib.ptr(f["opk"])
        lib.call("mstts_decoder_train_fwd_persistent", C.byref(d), C.byref(p))
        _ran_to_its_end(pt, "bf16 forward" + (", opk" if packed else ""))
        return d, f

    # ---- forward, row-major histories
    d, f = forward(False)
    got, notes = _collect(cd, u, f)
    _judge_stagewise(name, "persistent bf16 fwd", "pre", got, notes, Q.FORWARD_Q, failures, exchanged=True)
    # ---- forward packing the cell operands, the persistent BPTT behind it
    d, f = forward(True)
    bwd = w["persist_bwd"] and bool(L.mstts_persist_bwd_supported(B, H, M, A, T, KS))
    g = None
    if bwd:
        b, g = _bwd_desc(dev, cd, u, d, persistent=True)
        pb, pbt = _pdesc(dev, w["pkb"], int(L.mstts_persist_bwd_ws_bytes()), recurrent_bf16=1)
        pb.opk = lib.ptr(f["opk"])
        lib.call("mstts_decoder_train_bwd_persistent", C.byref(b), C.byref(pb))
        _ran_to_its_end(pbt, "bf16 BPTT")
    lib.call("mstts_persist_unpack_history", lib.ptr(f["opk"]), C.byref(d))
    torch.cuda.synchronize()
    got, notes = _collect(cd, u, f, g, persistent=True)
    _judge_stagewise(name, "persistent bf16 fwd, opk" + (" + BPTT" if bwd else ""), "pre", got, notes,
                     Q.FORWARD_Q + ((Q.PERSIST_BWD_Q + Q.HOST_Q) if bwd else ()), failures, packed=True, exchanged=True)
    assert not failures, failures


def test_plain_h32_with_bf16_copies_runs_fp32(dev, wcache):
    """mstts_decoder_bf16_splits admits no H = 32: with all six bf_* pointers given the drivers run their fp32 path, whole - judged as the fp32
    forms are (a driver half in bf16 is 1e-3 off this; the copies are zero-filled, so one that read them would be far off)."""
    name = "plain_h32"
    cd = R.case_data(name)
    w, u = _weights(dev, wcache, cd["widths"], bf16=True), _upload(dev, cd)
    assert not w["bf_ok"] and lib.load().mstts_decoder_bf16_splits(cd["H"], cd["M"], A, None) == 0
    d, f = _fwd_desc(dev, cd, w, u, "full", bf16="full")
    assert d.bf_w0f_f and d.bf_w1_f and d.bf_wq_f and d.bf_w0f_b and d.bf_w1_b and d.bf_wq_b
    b, g = _bwd_desc(dev, cd, u, d, persistent=False)
    lib.call("mstts_decoder_train_fwd", C.byref(d))
    lib.call("mstts_decoder_train_bwd", C.byref(b))
    torch.cuda.synchronize()
    got, notes = _collect(cd, u, f, g)
    failures = []
    _judge(name, "launch-per-step, six bf_* given", "xw0", got, notes, LPS_Q, failures)
    assert not failures, failures
