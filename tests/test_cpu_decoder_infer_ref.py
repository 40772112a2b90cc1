"""Pins tests/decoder_infer_ref.py, the fp64 checker of tests/test_gpu_decoder_infer_ref.py, without a GPU: the unrolled free-running loop in its
plain form is oracle.model.decoder(training=False) - outputs and loop length - to 1e-12, the folded form (what csrc/persist_infer.hip computes)
equals the plain one in fp64 to 1e-12, every designed stop column keeps |stop| >= 0.99 and gives the designed loop length after its rounding to
float32, every case's e32 is finite, the float32 evaluations - correct implementations - stay inside every bound, and the judge fails six wrong
implementations (decoder_infer_ref.FAULTS) at the bound the GPU test uses."""
import numpy as np
import pytest
import torch

from oracle import model as OM
from tests import decoder_infer_ref as R
from tests import decoder_loop_ref as RL

DESIGNED = [n for n in R.CASES if R.CASES[n]["stops"] == "designed"]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("name", ["plain_h32", "wide80_one_tile"])
def test_plain_form_is_the_oracles_decoder(name):
    """A defaults-width and a reference-width case, both with designed stops: the cell-0 kernel is unfolded again ([wx0 ; first context block ;
    k0b ; recurrent rows], its two context blocks adding up to w0f's), the keys are the memory layer's own fp64 product."""
    cd = R.case_data(name)
    w = RL.WIDTHS[cd["widths"]]
    H, M, NM, S = cd["H"], cd["M"], cd["n_mel"], cd["Smax"]
    d = OM.Dims(dec_lstm=w["dec_lstm"], enc_lstm=w["enc_lstm"], spk=w["spk"], prenet=w["prenet"], n_mel=NM, max_inf=S - 1, att=R.A, att_k=R.KS, att_ch=R.CH,
                zoneout=R.RATE, prenet_drop=R.PRENET_DROP)
    assert d.mem == M
    lv = R.operands(cd, torch.float64)
    wmem = R.weights(cd["widths"], NM)["wmem"].double()
    lv["keys"] = lv["values"] @ wmem
    p = dict(RL.lsa_params(lv))
    p[OM.P_CELL % 0 + "kernel"] = torch.cat([lv["wx0"], lv["w0f"][:M] - lv["k0b"], lv["k0b"], lv["w0f"][M:]])
    p[OM.P_CELL % 0 + "bias"], p[OM.P_CELL % 1 + "kernel"], p[OM.P_CELL % 1 + "bias"] = lv["b0"], lv["w1"], lv["b1"]
    p["attention/memory_layer/kernel"] = wmem
    for i, (k, b) in enumerate((("pw0", "pb0"), ("pw1", "pb1"))):
        p[R.P_PRE % i + "kernel"], p[R.P_PRE % i + "bias"] = lv[k], lv[b]
    p[R.P_PROJ + "kernel"], p[R.P_PROJ + "bias"] = lv["wproj"], lv["bproj"]
    with torch.no_grad():
        out = OM.decoder(p, d, lv["values"], cd["lens"], None, None, False, {"prenet_drop_0": cd["pm0"], "prenet_drop_1": cd["pm1"]})
        o = R.unrolled_free_decoder(lv, cd["lens"], cd["pm0"], cd["pm1"], R.RATE, S)
    assert out["linear"].shape[1] == o["n"] == R.designed_length(cd)
    assert _rel(o["linear"].transpose(0, 1), out["linear"]) <= 1e-12
    assert _rel(o["stop"].transpose(0, 1), out["stop"]) <= 1e-12
    assert _rel(o["align_hist"].permute(1, 2, 0), out["align"]) <= 1e-12
    # the states returned are those after the last step: the context is the last pj row's, the cumulative alignment the sum of the alignments
    assert torch.equal(o["pj_hist"][-1], torch.cat([o["m1"], o["ctx"]], dim=1))
    assert float((o["cum"] - o["align_hist"].sum(0)).abs().max()) < 1e-14


@pytest.mark.parametrize("name", ["plain_h32", "fused_h64", "wide80_one_tile", "wide80_t131"])
def test_folded_form_equals_plain_in_fp64(name):
    cd = R.case_data(name)
    with torch.no_grad():
        a = R.unrolled_free_decoder(R.operands(cd, torch.float64), cd["lens"], cd["pm0"], cd["pm1"], R.RATE, cd["Smax"], run_all=True)
        b = R.unrolled_free_decoder(R.operands(cd, torch.float64, folded="exact"), cd["lens"], cd["pm0"], cd["pm1"], R.RATE, cd["Smax"], form="folded", run_all=True)
    assert a["n"] == b["n"] == cd["Smax"]
    for k in R.QUANTITIES:
        assert _rel(b[k], a[k]) <= 1e-12, (k, _rel(b[k], a[k]))


@pytest.mark.parametrize("name", DESIGNED)
def test_stop_design_holds_after_rounding(name):
    """The rounded stop column, evaluated in fp64: every kept stop logit at least 0.99 from 0, rows stop at two or more different steps, row 0
    last and at most at Smax - 2, and the loop ends right there - in fp64 and in both float32 evaluations."""
    cd = R.case_data(name)
    ref, r32 = R.evaluations(name)
    first = R.stop_steps(cd)
    n = R.designed_length(cd)
    assert len(set(first.tolist())) >= 2 and first.max() == first[0] == n - 1 <= cd["Smax"] - 2 and (first[1:] < first[0]).all()
    assert ref["n"] == r32["plain"]["n"] == r32["folded"]["n"] == n
    stop = ref["stop"]
    assert stop.shape == (n, cd["B"])
    print("%s: min |stop| %.4f, float32 moves the stop logits by at most %.1e" % (name, np.abs(stop).min(), max(np.abs(r32[f]["stop"] - stop).max() for f in r32)))
    assert np.abs(stop).min() >= 0.99
    want = np.where(np.arange(n)[:, None] == first[None, :], 1.0, -1.0)
    assert np.array_equal(np.sign(stop), want)                       # -1 before the row's step, +1 at it, -1 after it
    assert float(cd["bproj"][cd["n_mel"]]) == 0.0


def test_cases_are_what_the_table_says():
    for name, c in R.CASES.items():
        cd = R.case_data(name)
        lens = cd["lens"].numpy()
        assert lens[0] == c["Te"] and (c["B"] == 1 or lens[1] == 1) and c["Smax"] <= 8
        assert c["Smax"] * c["B"] < cd["H"] + cd["M"] or c["stops"] == "forced"
        if c["stops"] == "forced":
            assert float(cd["bproj"][c["n_mel"]]) == -100.0 and R.evaluations(name)[0]["n"] == c["Smax"]
        elif c["Smax"] >= 5:          # a step remains that the persistent launch, which runs one step beyond the valid ones, must leave untouched
            assert R.designed_length(cd) + 1 < c["Smax"]
        assert cd["vp"].dtype ==cd["u"].dtype == cd["wfm"].dtype == cd["bf"].dtype == cd["pre0"].dtype == torch.float32


@pytest.mark.parametrize("name", list(R.CASES))
def test_e32_is_finite_and_float32_stays_inside_every_bound(name):
    cd = R.case_data(name)
    ref, r32 = R.evaluations(name)
    for algebra, forms in R.ALGEBRAS.items():
        _, e32, bound = R.reference(name, algebra)
        print("%-22s %-10s e32 %s" % (name, algebra, "  ".join("%s %.1e" % (k, e32[k]) for k in R.QUANTITIES)))
        for k in R.QUANTITIES:
            # (a designed stop column has the norm the least-squares problem gives it and carries the trajectory's float32 error into the stop
            # logits amplified: up to 1.2e-4 of their unit size at the reference widths - the sign is never in question)
            cap = 2e-4 if k == "stop" and cd["stops"] == "designed" else 2e-5
            assert np.isfinite(e32[k]) and e32[k] < cap, (k, e32[k])
            assert bound[k] == max(R.MARGIN * e32[k], R.FLOOR) and e32[k] <= bound[k] < 10 * cap
        for f in forms:
            assert all(err <= b for _, _, err, b in R.judge(name, algebra, r32[f], R.QUANTITIES))
            assert R.exact_failures(cd, r32[f]["align_hist"]) == []
    assert R.exact_failures(cd, ref["align_hist"]) == [] and all(err == 0.0 for _, _, err, _ in R.judge(name, "plain", ref, R.QUANTITIES))


def _over(name, algebra, got):
    """The quantities of `got` the judge fails, over the steps both ran; "n" when the loop length differs."""
    ref = R.evaluations(name)[0]
    n = min(got["n"], ref["n"])
    cut_ref = {k: (v[:n] if k in R.OUTPUTS else v) for k, v in ref.items()}
    _, e32, bound = R.reference(name, algebra)
    qs = R.OUTPUTS + (R.STATES if got["n"] == ref["n"] else ())
    bad = {k for k in qs if not R.judged_err(k, got[k][:n] if k in R.OUTPUTS else got[k], cut_ref).max() <= bound[k]}
    return bad | ({"n"} if got["n"] != ref["n"] else set())


@pytest.mark.parametrize("name", ["plain_h32", "wide80_one_tile"])
def test_the_judge_fails_wrong_implementations(name):
    """Each control evaluated in fp64 - its only error is the fault - at the bounds the GPU test uses."""
    cd = R.case_data(name)
    for algebra in R.ALGEBRAS:
        assert _over(name, algebra, R.evaluations(name)[0]) == set()
        # the prenet that feeds step s + 1 taken with the masks of step s: step 0 is untouched, everything after it moves
        bad = _over(name, algebra, R.evaluate(cd, "plain", torch.float64, fault="masks_of_previous_step"))
        assert {"linear", "align_hist"} <= bad, bad
        # the context entering cell 0 once instead of twice
        bad = _over(name, algebra, R.evaluate(cd, "plain", torch.float64, fault="context_once"))
        assert {"linear", "align_hist"} <= bad, bad
        # the zoneout blend dropped: new state = raw state
        bad = _over(name, algebra, R.evaluate(cd, "plain", torch.float64, fault="no_zoneout"))
        assert {"linear", "align_hist"} <= bad, bad
        # the cumulative alignment not accumulated
        bad = _over(name, algebra, R.evaluate(cd, "plain", torch.float64, fault="cum_not_accumulated"))
        assert {"align_hist", "linear"} <= bad, bad
        # a row that un-finishes: the loop runs on to the forced stop
        got = R.evaluate(cd, "plain", torch.float64, fault="row_unfinishes")
        assert got["n"] == cd["Smax"] != R.designed_length(cd) and "n" in _over(name, algebra, got)
    # bf without the b1p term, in the folded form (fp64 on the rounded operands: against the persistent launch's bound)
    good = R.evaluate(cd, "folded", torch.float64)
    assert _over(name, "persistent", good) == set()
    bad = _over(name, "persistent", R.evaluate(cd, "folded", torch.float64, fault="bf_without_b1p"))
    assert "linear" in bad and bad & {"align_hist", "n"}, bad
