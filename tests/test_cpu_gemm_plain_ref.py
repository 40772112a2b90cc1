"""Pins tests/gemm_plain_ref.py, the fp64 checker of tests/test_gpu_gemm_plain_ref.py, without a GPU, before that judge is trusted:
  - its reference equals an independently written one on every case: np.einsum on operands that a second, loop-based reading of the flat buffers
    extracts row by row (so the layout arithmetic of the cases - offsets, pitches, batch strides, both transpositions - is checked as well);
  - the flat buffers are NaN everywhere outside the operands' elements, with the guard rows and output pitch the GPU test relies on;
  - the float32 evaluation - a correct implementation - stays inside every bound, and nine wrong implementations exceed it on the cases named
    for them (the ninth, an output cleared over ldc instead of N columns, by the NaN-pitch rule);
  - selected_kernel, the restated dispatch of csrc/gemm.hip and csrc/gemm_bf16.hip, reaches every kernel and every K-cut of the library at least
    once over the (case, form) pairs, and every case the path it is named for;
  - the six-product split emulated in NumPy on the very operands of the selection test stays inside SPLIT_BOUND, and leaves it on at least one
    output as soon as any one of the six products is removed or any one plane of either operand is zeroed."""
import numpy as np
import pytest

from tests import gemm_plain_ref as R
from tests.gemm_forms import FORMS

SMALL = [n for n, c in R.CASES.items() if c["batch"] * c["M"] * c["N"] * max(c["K"], 1) <= 20_000_000]


def _rows(flat, off, ld, trans, rows, cols):
    """op(X) [rows, cols] read out of a flat buffer one stored row at a time (trans: the stored rows are op(X)'s columns)."""
    out = np.empty((rows, cols), np.float64)
    if trans:
        for c in range(cols):
            out[:, c] = flat[off + c * ld:off + c * ld + rows]
    else:
        for r in range(rows):
            out[r] = flat[off + r * ld:off + r * ld + cols]
    return out


def _independent(cd, rounded):
    M, N, K = cd["M"], cd["N"], cd["K"]
    rnd = R.bf16_round if rounded else (lambda a: a)
    outs = []
    for b in range(cd["batch"]):
        A = _rows(rnd(cd["flat_a"]), cd["a_off"] + b * cd["stride_a"], cd["lda"], cd["ta"], M, K)
        B = _rows(rnd(cd["flat_b"]), cd["b_off"] + b * cd["stride_b"], cd["ldb"], cd["tb"], K, N)
        v = cd["alpha"] * np.einsum("mk,kn->mn", A, B, optimize=M * N * K > 20_000_000)
        if cd["bias"]:
            v = v + cd["bias_v"].astype(np.float64)[None, :]
        v = {"none": lambda x: x, "relu": lambda x: np.where(x > 0, x, 0.0), "tanh": np.tanh}[cd["act"] if cd["split_k"] <= 1 else "none"](v)
        if cd["accumulate"] or cd["split_k"] > 1:
            v = _rows(cd["flat_c"], cd["c_off"] + b * cd["stride_c"], cd["ldc"], False, M, N) + v
        outs.append(v)
    return np.concatenate(outs, 0)


@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_is_an_independent_formulation(name):
    cd = R.case_data(name)
    for rounded in ((False, True) if name in SMALL else (False,)):
        ref, want = R.reference(name, rounded)[0], _independent(cd, rounded)
        assert ref.shape == want.shape == (cd["batch"] * cd["M"], cd["N"]) and np.isfinite(want).all()
        assert np.abs(ref - want).max() <= 1e-12 * np.abs(want).max(), (name, rounded, np.abs(ref - want).max())


@pytest.mark.parametrize("name", list(R.CASES) + R.SEL_NAMES)
def test_buffers_are_nan_outside_the_operands(name):
    cd = R.case_data(name) if name in R.CASES else R.selection_data(name)
    M, N, K, nb = cd["M"], cd["N"], cd["K"], cd["batch"]
    for flat, idx, off, ld in ((cd["flat_a"], R.index_a(cd), cd["a_off"], cd["lda"]), (cd["flat_b"], R.index_b(cd), cd["b_off"], cd["ldb"])):
        assert flat.dtype == np.float32 and not flat.flags.writeable
        assert len(np.unique(idx)) == idx.size and np.isfinite(flat[idx]).all() and np.isfinite(flat).sum() == idx.size
        assert off >= ld and np.isnan(flat[:off]).all() and np.isnan(flat[-ld:]).all() and (idx.size == 0 or idx.max() < flat.size - ld)
    ic = R.index_c(cd)
    assert cd["ldc"] >= N + 8 and cd["c_off"] == R.EDGE * cd["ldc"] and ic.max() == cd["flat_c"].size - R.EDGE * cd["ldc"] - (cd["ldc"] - N) - 1
    assert np.isfinite(cd["flat_c"]).sum() == (ic.size if R.starts(cd) else 0) and R.outside_is_nan(cd, cd["flat_c"])
    assert (cd["a_off"] - cd["xa"]) % 4 == 0 and (cd["b_off"] - cd["xb"]) % 4 == 0
    if nb > 1:
        assert cd["stride_a"] > cd["rows_a"] * cd["lda"] and cd["stride_b"] > cd["rows_b"] * cd["ldb"] and cd["stride_c"] > M * cd["ldc"]
        assert cd["stride_a"] != cd["stride_b"]
    assert cd["split_k"] == 1 or cd["act"] == "none"


@pytest.mark.parametrize("rounded", [False, True])
@pytest.mark.parametrize("name", list(R.CASES))
def test_float32_evaluation_stays_inside_every_bound(name, rounded):
    cd = R.case_data(name)
    ref, e32 = R.reference(name, rounded)
    assert np.isfinite(e32) and e32 < 2e-5, e32
    err, bound = R.judge(R.evaluate(cd, np.float32, rounded), ref, e32)
    assert bound == max(R.MARGIN * e32, R.FLOOR) and err <= bound < 2e-4, (err, bound)
    assert R.judge(ref, ref, e32)[0] == 0.0
    assert R.outside_is_nan(cd, R.written(cd, ref)) and np.array_equal(R.taken(cd, R.written(cd, ref)), ref.astype(np.float32).astype(np.float64))
    if rounded and cd["K"] > 0:      # the rounded reference is another function: the unrounded one is far outside its bound
        assert R.judge(R.reference(name, False)[0], ref, e32)[0] > 30 * bound


def _exceeds(name, fault, rounded=False):
    ref, e32 = R.reference(name, rounded)
    err, bound = R.judge(R.evaluate(R.case_data(name), np.float64, rounded, fault=fault), ref, e32)
    return not err <= bound


def test_the_judge_fails_planted_faults():
    c = R.CASES
    for name in SMALL + ["tail_f_nt"]:                                    # the last K % 32 terms dropped
        assert _exceeds(name, "k_tail_dropped") == (c[name]["K"] % 32 != 0), name
    assert sum(c[n]["K"] % 32 != 0 for n in SMALL) >= 30
    for name in SMALL:                                                    # bias added once per split piece
        assert _exceeds(name, "bias_per_piece") == (c[name]["split_k"] > 1 and c[name]["bias"]), name
    assert _exceeds("splitk_empty_tn", "bias_per_piece") and _exceeds("splitk_empty_tn", "bias_per_piece", rounded=True)
    for name in SMALL:                                                    # alpha applied to the bias
        assert _exceeds(name, "alpha_on_bias") == (c[name]["alpha"] != 1.0 and c[name]["bias"]), name
    assert _exceeds("alpha_nn", "alpha_on_bias") and _exceeds("alpha_tt", "alpha_on_bias")
    for name in SMALL:                                                    # act(C0 + ...) instead of C0 + act(...)
        assert _exceeds(name, "act_outside") == (c[name]["act"] != "none" and c[name]["accumulate"]), name
    assert _exceeds("acc_act_nn", "act_outside")
    for name in SMALL:                                                    # pitch ignored: every case with a contraction has pitched operands
        assert _exceeds(name, "pitch_ignored") == (c[name]["K"] > 0), name
    for name in SMALL:                                                    # base offset ignored
        assert _exceeds(name, "offset_ignored") == (c[name]["xa"] != 0 or c[name]["xb"] != 0), name
    assert all(_exceeds(n, "offset_ignored") for n in ("lay_offset_nn", "lay_offset_nt", "lay_offset_tn", "dx_form_nt"))
    for name in SMALL + ["f128_nn"]:                                      # batch stride of A taken for B
        assert _exceeds(name, "stride_mixup") == (c[name]["batch"] > 1), name
    assert all(_exceeds(n, "stride_mixup") for n in ("batch_tn", "batch_odd_nn", "f128_nn"))
    for name in ("lay_vec_nt", "lay_vec_tt", "k160_nt", "big_nt", "dx_form_nt"):       # trans_b ignored (132 x 136 x 164: square-ish, the same buffer read the other way)
        assert _exceeds(name, "trans_b_ignored"), name
    assert not _exceeds("lay_vec_nn", "trans_b_ignored")
    for name in ("dx_form_act_nt", "big_nn", "batch_odd_nn", "k0_nn", "lay_vec_tn"):   # the output cleared over ldc instead of N columns: the NaN-pitch rule
        cd, ref = R.case_data(name), R.reference(name)[0]
        flat = R.written(cd, ref, fault="clear_ldc")
        assert np.array_equal(R.taken(cd, flat), R.taken(cd, R.written(cd, ref))) and not R.outside_is_nan(cd, flat) and R.outside_is_nan(cd, R.written(cd, ref))
    # one output row off by 3e-5 of itself where its values are small next to the matrix's largest; one element written one row too far
    cd = R.case_data("lay_vec_nn")
    ref, e32 = R.reference("lay_vec_nn")
    got = ref.copy()
    row = int(np.abs(ref).max(1).argmin())
    got[row] *= 1 + 3e-5
    assert R.judge(got, ref, e32)[0] > R.bound_of(e32) and np.abs(got - ref).max() / np.abs(ref).max() < 2e-5      # (the global metric at its 2e-5 passes it)
    flat = R.written(cd, ref)
    flat[cd["c_off"] + cd["M"] * cd["ldc"]] = 0.0
    assert not R.outside_is_nan(cd, flat)


PATHS = {
    "32-row tile": "f32 MFMA, 32-row tile", "64-row tile": "f32 MFMA, 64-row tile", "128-row tile": "f32 MFMA, 128-row tile",
    "fallback body + tail": "f32 MFMA, 64-row tile, body + tail", "split whole tiles": "split 128x128",
    "split every-tile cut": "split 128x128, every tile K-cut", "split every-tile cut + tail activation": "split 128x128, every tile K-cut + tail act",
    "split body + tail": "split 128x128, body + tail + tail act", "split 256 x 256": "split 256x256",
    "bf16 128 x 128": "bf16 128x128", "bf16 128 x 128 with a cut of the library's own": "bf16 128x128, library K-cut x", "bf16 256 x 256": "bf16 256x256",
}


def _sel(name, form):
    return R.selected_kernel(form, R.CASES[name])


def test_every_path_is_reached():
    assert R.ALL_FORMS == tuple(FORMS) and R.F32_FORMS == tuple(f for f in FORMS if not FORMS[f]["bf16"])
    seen = {_sel(n, f) for n, c in R.CASES.items() for f in c["forms"]}
    for what, text in PATHS.items():
        assert any(s == text or (text.endswith(" x") and s.startswith(text)) for s in seen), (what, sorted(seen))
    assert {R.loads(c).split(" (")[-1].rstrip(")") for c in R.CASES.values()} >= {"vector", "dims", "base", "pitch"}        # each scalar trigger alone


def test_cases_reach_what_they_are_named_for():
    c = R.CASES
    for lay in ("nn", "nt", "tn", "tt"):
        assert R.loads(c["lay_vec_" + lay]) == "vector" and "dims" in R.loads(c["lay_scalar_" + lay])
        assert _sel("lay_vec_" + lay, "f32_mfma").startswith("f32 MFMA") and all(_sel("lay_vec_" + lay, f) == "split 128x128" for f in R.F32_FORMS[1:])
        assert all(_sel("rows32_" + lay, f) == "f32 MFMA, 32-row tile" for f in R.F32_FORMS)
        assert all(_sel("rows33_" + lay, f) == "split 128x128" for f in R.F32_FORMS[1:])
        assert (_sel("big_" + lay, "split_big"), _sel("big_" + lay, "bf16_big")) == ("split 256x256", "bf16 256x256")
        assert _sel("big_" + lay, "split_128") == "split 128x128, every tile K-cut" + (" + tail act" if lay == "nn" else "")
    for lay in ("nn", "nt", "tn"):
        assert R.loads(c["lay_offset_" + lay]) == "scalar (base)" and R.loads(c["lay_pitch1_" + lay]) == "scalar (pitch)"
        assert all(c["lay_offset_" + lay][k] % 4 == 0 for k in ("M", "N", "K", "lda", "ldb")) and c["lay_pitch1_" + lay]["lda"] % 4 == 1
    for lay in ("nn", "nt"):
        assert all(_sel("k159_" + lay, f).startswith("f32 MFMA") for f in R.F32_FORMS)
        assert all(_sel("k160_" + lay, f) == "split 128x128" for f in R.F32_FORMS[1:]) and c["k160_" + lay]["K"] == 5 * 32
    assert R.loads(c["batch_tn"]) == "vector" and R.loads(c["batch_odd_nn"]) == "scalar (pitch)" and c["batch_odd_nn"]["lda"] % 4 == 0 == c["batch_odd_nn"]["ldb"] % 4
    assert (_sel("big_ktail_tn", "split_big"), _sel("big_ktail_tn", "bf16_big")) == ("split 256x256", "bf16 256x256")
    k, s = c["big_ktail_tn"]["K"], c["big_ktail_tn"]["split_k"]
    for bk in (16, 32):                                                  # gemm_k_per_split: the second piece ends 8 into a K-tile of either depth
        kps = -(-(-(-k // s)) // bk) * bk
        assert (k - kps) % bk == 8 and 0 < k - kps < kps
    for f in ("split_128", "split_big"):
        assert _sel("dx_form_nt", f) == "split 128x128, every tile K-cut" and _sel("dx_form_act_nt", f) == "split 128x128, every tile K-cut + tail act"
        assert _sel("acc_act_nn", f) == "split 128x128"
    assert _sel("dx_form_nt", "bf16_128").startswith("bf16 128x128, library K-cut x") and _sel("dx_form_act_nt", "bf16_128") == "bf16 128x128"
    assert c["dx_form_nt"]["ldc"] == c["dx_form_nt"]["N"] + 8 and c["dx_form_nt"]["xb"] % 4 == 0 and R.loads(c["dx_form_nt"]) == "vector"
    k, s = c["splitk_empty_tn"]["K"], c["splitk_empty_tn"]["split_k"]
    for bk, empty in ((32, 2), (64, 5)):                                 # pieces with kbeg >= K
        kps = max(-(-(-(-k // s)) // bk) * bk, bk)
        assert sum(p * kps >= k for p in range(s)) == empty
    assert all(_sel("f128_nn", f) == "f32 MFMA, 128-row tile" for f in R.F32_FORMS) and c["f128_nn"]["forms"] == R.F32_FORMS
    assert _sel("tail_f_nt", "f32_mfma") == "f32 MFMA, 64-row tile, body + tail"
    assert _sel("tail_s_nt", "split_128") == "split 128x128, body + tail + tail act" and _sel("tail_s_nt", "f32_mfma").endswith("body + tail + tail act")
    m = c["tail_f_mixed_nt"]                                             # 297 half tiles, body 256: the tail starts inside a tile row
    assert _sel("tail_f_mixed_nt", "f32_mfma") == "f32 MFMA, 64-row tile, body + tail" and 256 % -(-m["N"] // 128) != 0 and -(-m["M"] // 64) * -(-m["N"] // 128) == 297
    b = c["band_nn"]
    assert all(_sel("band_nn", f) == "split 128x128" for f in ("split_128", "default_det")) and -(-b["N"] // 128) == 23 > 8
    assert -(-b["M"] // 128) * 23 == 69 >= 64 and 69 % 8 != 0 and _sel("band_nn", "bf16_128") == "bf16 128x128"
    k, s = c["big_splitk_empty_tn"]["K"], c["big_splitk_empty_tn"]["split_k"]
    assert (_sel("big_splitk_empty_tn", "split_big"), _sel("big_splitk_empty_tn", "bf16_big")) == ("split 256x256", "bf16 256x256")
    assert all(sum(p * max(-(-(-(-k // s)) // bk) * bk, bk) >= k for p in range(s)) == 2 for bk in (16, 32))
    assert all(_sel(n, "default_det") in("split 128x128", "f32 MFMA, 32-row tile", "f32 MFMA, 64-row tile", "f32 MFMA, 128-row tile") for n in c)
    assert c["k0_nn"]["K"] == 0 == c["k0_acc_nn"]["K"] and c["k0_acc_nn"]["accumulate"]
    assert all(len(v["why"]) > 10 for v in c.values())
    for name in R.SEL_NAMES:
        cd = R.selection_data(name)
        big = name.startswith("s194")
        assert R.selected_kernel("split_big", cd) == ("split 256x256" if big else "split 128x128") and R.selected_kernel("split_128", cd).startswith("split 128x128")
        assert R.selected_kernel("bf16_big", cd) == ("bf16 256x256" if big else "bf16 128x128") and R.loads(cd) == "vector"


@pytest.mark.parametrize("name", R.SEL_NAMES)
def test_six_product_emulation_separates_a_lost_term(name):
    cd = R.selection_data(name)
    exact, way = cd["exact"], cd["way"]
    A, B = cd["op_a"].astype(np.float64), cd["op_b"].astype(np.float64)
    assert np.array_equal(A @ B, exact) and (np.abs(exact) > 0).all()               # one term plus zeros: the contraction IS the single product
    assert ((cd["op_a"] != 0).sum(1) == 1).all() if way.startswith("a_") else ((cd["op_b"] != 0).sum(0) == 1).all()
    for x in (cd["op_a"], cd["op_b"]):                                              # the split is exact, and the value operand loads all three planes
        hi, mid, lo = R.planes(x)
        assert np.array_equal(hi.astype(np.float64) + mid + lo, x.astype(np.float64))
    vals = cd["op_b"] if way.startswith("a_") else cd["op_a"]
    assert all((np.abs(p) > 0).mean() > 0.9 for p in R.planes(vals))
    assert 3.7e-7 < R.SPLIT_BOUND < 3.8e-7
    assert R.selection_err(R.split_emulation(cd), exact) <= R.SPLIT_BOUND
    value_side = "b" if way.startswith("a_") else "a"
    if way.endswith("_val"):
        for drop in range(6):
            assert R.selection_err(R.split_emulation(cd, drop_product=drop), exact) > R.SPLIT_BOUND, drop
        sides = ("a", "b")
    else:                                                                            # entries 1.0 = hi alone: only the value operand's planes carry weight
        assert R.selection_err(R.split_emulation(cd, drop_product=3), exact) <= R.SPLIT_BOUND
        sides = (value_side,)
    for side in sides:
        for p in range(3):
            assert R.selection_err(R.split_emulation(cd, zero_plane=(side, p)), exact) > R.SPLIT_BOUND, (side, p)
    # what the other forms must give: f32_mfma the exact product rounded once (exactly the selected element where the entries are 1.0)
    if way.endswith("_one"):
        assert np.array_equal(exact.astype(np.float32).astype(np.float64), exact)


def test_gpu_docstring_names_every_case():
    import re
    from tests import test_gpu_gemm_plain_ref as G
    doc = G.__doc__
    rows = set(re.findall(r"^  (\w+) +\w\w +\d+ x \d+ x \d+", doc, re.M))
    assert rows == set(R.CASES), rows ^ set(R.CASES)
