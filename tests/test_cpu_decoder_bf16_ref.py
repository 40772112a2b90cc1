"""Pins tests/decoder_bf16_ref.py, the stage-wise fp64 checker of tests/test_gpu_decoder_bf16_ref.py, without a GPU.  The "form" judged here is
synthetic: the bf16-emulated loop and BPTT evaluated in float32 on the CPU (decoder_bf16_ref.synthetic_form), held bit for bit to
decoder_loop_ref.evaluate under oracle.model.RECURRENT_BF16.  It passes every bound; each negative control - one site of one step - is reported
at 10 x the bound or more in its own stage and step while every stage judged before it stays inside its bound; the first four are shown to
sit under the trajectory tests' whole-tensor bounds; and the straight-through / stored-gradient machinery without rounding, fed with the fp64
evaluation's own tensors, is decoder_loop_ref.evaluate.

e32 of the checker on the synthetic form (worst slice difference of its float32 and float64 evaluations; the bound is 8 x e32, at least 1e-6), in
units of 1e-7 - the values the GPU test's table starts from:
  case (form)          acts0 craw0 c0  in0_h0 in1_m0 acts1 craw1 c1  in1_h1 pj_m1 q   align cum pj_ctx de  dq  dg1 dg0 d_in0 d_ctx dw0f dw1 db1 dwq d_val
  fused_h64 (xw0)      2.8   2.1   2.5 2.8    2.3    1.4   1.7   1.7 1.9    2.2   1.6 2.0   1.9 2.1    2.7 4.7 1.8 1.8 1.2   1.2   0.4  0.2 1.1 0.8 2.2
  two_pass_t140 (xw0)  2.1   1.3   1.3 1.8    2.2    1.0   1.5   1.5 1.7    2.1   1.1 0.9   0.8 1.5    3.3 4.2 2.1 2.0 0.9   0.9   0.5  0.4 0.8 1.8 1.7
  wide_one_tile (pre)  5.9   2.7   2.6 3.2    3.2    1.6   2.0   1.6 2.0    1.9   1.8 1.5   1.1 1.6    4.0 5.2 1.8 3.4 3.8   3.8   0.8  0.7 1.0 0.9 1.3
(figures of one machine.  The synthetic form is itself a float32 evaluation of the same statement: its error equals e32.)
"""
import numpy as np
import pytest
import torch

from oracle import model as OM
from tests import decoder_bf16_ref as Q
from tests import decoder_loop_ref as R

MID_CASES = ("fused_h64", "two_pass_t140")
ALL_Q = Q.FORWARD_Q + Q.BACKWARD_Q + Q.HOST_Q
FAULT_CASE, FAULT_STEP = "fused_h64", 2
# fault -> the stage that must report it (at FAULT_STEP; the two controls of unrolled_decoder act at every step: the first step that shows them)
WHERE = {"truncate_cell1_operand": ("cell1", FAULT_STEP), "query_operand_unrounded": ("query", FAULT_STEP), "xw0_rounded": ("cell0", FAULT_STEP),
         "dg0_product_fp32": ("cell0_product", FAULT_STEP), "dq_hist_stored_rounded": ("attention_bwd", FAULT_STEP),
         "dg1_wrong_half": ("cell0_bwd", FAULT_STEP), "zh0_in_cell1": ("cell1", 0), "stale_cum": ("attention", 1)}
# The whole-tensor error of a faulted trajectory, as a fraction of the trajectory tests' bound, against the stage-wise error as a fraction of
# its bound: the printed figures give 1.1e4 and more for every one of the four (the least: xw0_rounded, 0.13 against 1446); asserted at 1000.
INVISIBLE_BY = 1000.0


@pytest.fixture(scope="module")
def forms():
    cache = {}

    def get(name, form="xw0", fault=None, step=None):
        key = (name, form, fault, step)
        if key not in cache:
            cache[key] = Q.synthetic_form(R.case_data(name), form, fault, step)
        return cache[key]
    yield get
    cache.clear()


def test_emulation_is_the_oracles(forms):
    """The synthetic form is unrolled_decoder around oracle.model._BF16MatMul (RECURRENT_BF16), bit for bit."""
    cd = R.case_data("fused_h64")
    assert not OM.RECURRENT_BF16 and not OM.GEMM_BF16
    OM.RECURRENT_BF16 = True
    try:
        want = R.evaluate(cd, "xw0", torch.float32)
    finally:
        OM.RECURRENT_BF16 = False
    got = forms("fused_h64")
    for k in R.FORWARD_Q + R.BACKWARD_Q:
        assert np.array_equal(np.asarray(got[k], np.float64), want[k]), k
    plain = R.evaluations("fused_h64")[1]
    assert R.slice_err(got["pj"], plain["pj"]).max() > 1e-4                       # ... and the rounding is really in it


@pytest.mark.parametrize("name,form", [(n, "xw0") for n in MID_CASES] + [("wide_one_tile", "pre")])
def test_synthetic_form_passes_every_bound(forms, name, form):
    cd = R.case_data(name)
    got = forms(name, form)
    assert R.exact_failures(cd, got) == [] and Q.context_identity_failures(cd, got) == []
    rows, errs, bounds = Q.judge(cd, form, got, ALL_Q)
    print("%-14s %s" % (name, " ".join("%s %.1f" % (k, e32 * 1e7) for k, e32, _, _ in rows)))
    print("%-14s %s" % ("  err", " ".join("%s %.1f" % (k, err * 1e7) for k, _, err, _ in rows)))
    for k, e32, err, bound in rows:
        assert 1e-9 < e32 < 2e-5 and bound == max(R.MARGIN * e32, R.FLOOR), (k, e32)
        assert err <= bound, (k, err, e32, bound)
    assert all(w <= 1.0 for _, _, w in Q.judged_sequence(cd, errs, bounds))


@pytest.mark.parametrize("fault", Q.FAULTS)
def test_negative_controls_are_detected_and_localised(forms, fault):
    cd = R.case_data(FAULT_CASE)
    assert 0 < FAULT_STEP < cd["S"] - 1
    got = forms(FAULT_CASE, "xw0", fault, FAULT_STEP)
    rows, errs, bounds = Q.judge(cd, "xw0", got, Q.FORWARD_Q + Q.BACKWARD_Q)
    seq = Q.judged_sequence(cd, errs, bounds)
    first = next(i for i, (_, _, w) in enumerate(seq) if w > 1.0)
    stage, step, w = seq[first]
    print("%-24s first over its bound: %s of step %d at %.0f x the bound; over anywhere: %s" % (
        fault, stage, step, w, sorted({(st, s) for st, s, v in seq if v > 1.0})))
    assert (stage, step) == WHERE[fault], (fault, stage, step, w)
    assert w >= 10.0, (fault, w)
    assert all(v <= 1.0 for _, _, v in seq[:first])
    if fault in Q.FAULTS[:6]:
        # One site of one step.  Forward, every stage is judged from the form's own history: nothing else is over.  In the BPTT the checker carries
        # the cell-state and attention gradients itself, and the form's derivatives come from the saves it stored: the steps judged AFTER the
        # faulted one (the earlier steps) may differ too, none judged before it.
        fwd_stages = [st for st, _ in Q.FORWARD_STAGES]
        assert {(st, s) for st, s, v in seq if v > 1.0 and st in fwd_stages} <= {WHERE[fault]}, fault
        assert all(s <= FAULT_STEP for st, s, v in seq if v > 1.0 and st not in fwd_stages), fault
    if fault in Q.FAULTS[:4]:
        clean = forms(FAULT_CASE)
        rel = lambda k: float(np.abs(np.asarray(got[k], np.float64) - clean[k]).max() / np.abs(clean[k]).max())
        print("%-24s whole trajectory against the unfaulted run: pj %.1e  align_hist %.1e (bound 2e-3)   dg0 %.1e (bound 2e-2)   stage-wise: %.0f x its bound"
              % (fault, rel("pj"), rel("align_hist"), rel("dg0"), w))
        seen = max(rel("pj") / 2e-3, rel("align_hist") / 2e-3, rel("dg0") / 2e-2)
        assert seen < 1.0 and seen * INVISIBLE_BY <= w, (fault, seen, w)


@pytest.mark.parametrize("name", MID_CASES)
def test_machinery_without_rounding_is_the_fp64_evaluation(name):
    """Replaced states and stored-gradient products, fed with the fp64 evaluation's own tensors and no rounding: every replacement is the
    identity, every stored gradient the incoming one - decoder_loop_ref.evaluate to 1e-12."""
    cd = R.case_data(name)
    ref = R.evaluations(name, "xw0")[0]
    out = Q.stagewise(cd, "xw0", ref, torch.float64, rounding=False)
    for k in R.QUANTITIES:
        assert out[k].shape == ref[k].shape and np.abs(out[k] - ref[k]).max() <= 1e-12 * np.abs(ref[k]).max(), k


def test_exchanged_copies_are_what_the_persistent_launches_round(forms):
    """decoder_bf16_ref.PERSISTENT_SITES: the generation bit, and one operand element of cell 1 placed one float32 ulp above a bf16 tie - its
    exchanged copy of generation 0 IS the tie and rounds to even, the stored value rounds up: the two statements differ by one bf16 ulp of
    that element in that (step, row) and nowhere else, which the plain statement's bound sees."""
    a = np.array([1.0, -1.0, 0.0, 3.0000002], np.float32)
    for gen in (0, 1):
        c = Q.exchanged_copy(a, gen)
        assert ((c.view(np.uint32) & 1) == gen).all() and ((c.view(np.uint32) >> 1) == (a.view(np.uint32) >> 1)).all()
    cd = R.case_data("fused_h64")
    got = dict(forms("fused_h64"))
    s, b, j = 2, 3, 5
    got["in1"] = got["in1"].copy()
    bits = got["in1"][s:s + 1, b, j].view(np.uint32)
    bits[0] = (bits[0] & np.uint32(0x7FFE0000)) | np.uint32(0x8001)              # positive: even bf16 value + half an ulp + one float32 ulp
    plain, xch = (Q.stagewise(cd, "xw0", got, torch.float64, exchanged=e) for e in (False, True))
    diff = np.abs(plain["acts1"] - xch["acts1"]).max(-1)
    assert diff[s, b] > 1e-6 and np.count_nonzero(diff) == 1
    for k in ("acts0", "q_hist", "align_hist"):
        assert np.array_equal(plain[k], xch[k]), k
    x = torch.tensor(got["in1"][s, b, j:j + 1])
    assert float(Q.bf(x)) > float(x) > float(Q.bf(torch.tensor(Q.exchanged_copy(x.numpy(), 0))))


def test_context_identity_and_truncation():
    cd = R.case_data("fused_h64")
    ref = R.evaluations("fused_h64")[1]
    got = {k: ref[k].astype(np.float32) for k in ("in0", "pj")}
    assert Q.context_identity_failures(cd, got) == []
    got["in0"][2, 1, 3] = np.nextafter(got["in0"][2, 1, 3], np.float32(9.0))
    assert len(Q.context_identity_failures(cd, got)) == 1
    x = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -9, -(1.0 + 2.0 ** -8 + 2.0 ** -9), 1.0 + 2.0 ** -7])
    assert Q.bf_truncate(x).tolist() == [1.0, -1.0, 1.0 + 2.0 ** -7] and Q.bf(x).tolist() == [1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -7), 1.0 + 2.0 ** -7]
