"""fp64 checker of the plain (win_T == 0) products of mstts_gemm_f32 / mstts_gemm_bf16 (tests/test_gpu_gemm_plain_ref.py; pinned without a GPU
by tests/test_cpu_gemm_plain_ref.py).  The window half of the kernel table is tests/conv_window_ref.py's.

A case is a descriptor (include/mstts.h, mstts_gemm_desc) in Python: M, N, K, ta, tb, element offsets a_off / b_off / c_off and pitches lda / ldb /
ldc, bias, act, accumulate, split_k, alpha, batch and stride_a / stride_b / stride_c.  case_data(name) draws the FLAT float32 buffers the
descriptor points into, once, from a fixed seed, read-only - the very arrays that are uploaded: A with unit variance, B with variance 1 / K, bias
with sigma 0.3, start values of C N(0, 1) where the product lands on start values (accumulate, split_k > 1).  Every element of the three buffers
that is not an element of its operand is NaN: the pitch, at least one row before the base (plus the case's extra offset) and after the last row,
the gaps between batches; the output has two NaN rows before and after and at least 8 NaN columns right of every row.

The reference reads op(A)(m, k) and op(B)(k, n) out of the flat buffers by the header's addressing rules,
    A(m,k) = A[m*lda + k] (trans_a: A[k*lda + m]),   B(k,n) = B[k*ldb + n] (trans_b: B[n*ldb + k]),   batch b at + b*stride,
and evaluates in float64
    C = [C0 +] act(alpha * op(A) . op(B) + bias)          split_k > 1:  C = C0 + alpha * op(A) . op(B) + bias
evaluate(..., dtype=np.float32) is the same in float32 (its worst row error is e32); rounded=True rounds both operands to bf16 (conv_window_ref.
bf16_round; C0, bias and alpha are not rounded): the reference of the mstts_gemm_bf16 forms.

Judging (slice_err, MARGIN, FLOOR of tests/lstm_seq_ref.py): every output row (b, m) on its own scale, bound 8 x e32, never less than 1e-6.
outside_is_nan: everything of a flat output outside the product's M x N elements is still NaN."""
import functools

import numpy as np

from tests.conv_window_ref import act_fn, bf16_round
from tests.lstm_seq_ref import FLOOR, MARGIN, slice_err      # noqa: F401  (the project's constants, not copies)

ACTS = {"none": 0, "relu": 1, "tanh": 2}                      # lib.ACT_* (asserted by the GPU test)
F32_FORMS = ("f32_mfma", "split_128", "split_big", "default_det")
ALL_FORMS = F32_FORMS + ("bf16_128", "bf16_big")              # tests/gemm_forms.FORMS (asserted by the CPU test)
EDGE = 2                                                      # NaN rows before and after every output


def _case(M, N, K, lay, pa=4, pb=4, pc=8, xa=0, xb=0, bias=False, act="none", accumulate=False, split_k=1, alpha=1.0, batch=1, gaps=(0, 0, 0),
          forms=ALL_FORMS, why=""):
    """A descriptor from its shape.  lay: "nn" / "nt" / "tn" / "tt" (trans_a, trans_b); pa / pb / pc: how much wider than its row the pitch of
    A / B / C is; xa / xb: elements the base of A / B lies behind its one NaN guard row; gaps: NaN elements between consecutive batches."""
    ta, tb = lay[0] == "t", lay[1] == "t"
    assert pc >= 8 and set(forms) <= set(ALL_FORMS)
    ra, ca = (K, M) if ta else (M, K)                         # rows and row length of A, B as stored
    rb, cb = (N, K) if tb else (K, N)
    lda, ldb, ldc = ca + pa, cb + pb, N + pc
    up4 = lambda v: (v + 3) // 4 * 4                          # the guard in front of a base: one row, rounded up so that xa / xb alone decide its alignment
    c = dict(M=M, N=N, K=K, lay=lay, ta=ta, tb=tb, lda=lda, ldb=ldb, ldc=ldc, a_off=up4(lda) + xa, b_off=up4(ldb) + xb, c_off=EDGE * ldc, xa=xa, xb=xb,
             bias=bias, act=act, accumulate=accumulate, split_k=split_k, alpha=alpha, batch=batch, forms=tuple(forms), why=why,
             rows_a=ra, rows_b=rb)
    c["stride_a"], c["stride_b"], c["stride_c"] = (ra * lda + gaps[0], rb * ldb + gaps[1], M * ldc + gaps[2]) if batch > 1 else (0, 0, 0)
    c["size_a"] = c["a_off"] + (batch - 1) * c["stride_a"] + ra * lda + lda + 3
    c["size_b"] = c["b_off"] + (batch - 1) * c["stride_b"] + rb * ldb + ldb + 3
    c["size_c"] = c["c_off"] + (batch - 1) * c["stride_c"] + M * ldc + EDGE * ldc
    return c


CASES = {}
for _l in ("nn", "nt", "tn", "tt"):
    CASES["lay_vec_" + _l] = _case(132, 136, 164, _l, pa=4, pb=8, pc=12, bias=True, why="every pitch 4, 8 or 12 wider than its row, vector loads; K ends 4 "
                                   "into a K-tile of 32 / 16 / 64; two tiles in M and in N")
    CASES["lay_scalar_" + _l] = _case(131, 83, 161, _l, pa=1, pb=1, pc=9, bias=True, why="odd dimensions, pitches dim + 1: scalar loads through the dimensions, a "
                                      "one-element K tail, ragged last row and column tile")
    CASES["rows32_" + _l] = _case(32, 136, 260, _l, why="the last row count on the 32-row tile of the fallback kernel")
    CASES["rows33_" + _l] = _case(33, 136, 260, _l, why="the first row count on the split kernel (K >= 160)")
    CASES["big_" + _l] = _case(194, 260, 768, _l, pa=8, pb=4, pc=12, bias=True, act="tanh" if _l == "nn" else "none", why="256 x 256 tiles ragged in M and in N "
                               "(256 + 4) once the workgroup minimum is lowered; otherwise six 128 x 128 tiles, every one cut along K (nn: with the tail activation)")
for _l in ("nn", "nt", "tn"):
    CASES["lay_offset_" + _l] = _case(132, 136, 164, _l, pa=4, pb=8, xa=1, xb=3, why="dimensions and pitches multiples of 4, A 1 element and B 3 elements into "
                                      "their allocations: scalar loads through the base pointers alone")
    CASES["lay_pitch1_" + _l] = _case(132, 136, 164, _l, pa=5, pb=8, why="aligned bases, dimensions multiples of 4, lda % 4 == 1: scalar loads through one pitch alone")
for _l in ("nn", "nt"):
    CASES["k159_" + _l] = _case(132, 136, 159, _l, pa=1, why="the last K on the fallback kernel")
    CASES["k160_" + _l] = _case(132, 136, 160, _l, why="the first K on the split kernel: exactly five K-tiles, no tail")
for _l in ("nn", "tn"):
    CASES["one_" + _l] = _case(1, 1, 52, _l, bias=True, why="a one-element output")
    CASES["col1_" + _l] = _case(70, 1, 36, _l, bias=True, why="a one-column output")
CASES.update({
    "big_ktail_tn": _case(256, 192, 168, "tn", split_k=2, why="split_k = 2 onto start values; the second piece (K 96 .. 168) ends 8 into a 16-deep and a 32-deep "
                          "K-tile of the big kernels"),
    "dx_form_nt": _case(165, 80, 512, "nt", xb=5000, accumulate=True, why="the trainers' data gradient: B at an offset in a slab, accumulate onto start values, "
                        "ldc = N + 8: every tile cut along K by the library (split kernel), bf16 autocut"),
    "dx_form_act_nt": _case(165, 80, 512, "nt", bias=True, act="relu", why="the every-tile cut with the tail activation kernel: the clearing stops at column N "
                            "and row M"),
    "acc_act_nn": _case(165, 80, 512, "nn", bias=True, act="tanh", accumulate=True, why="C0 + tanh(...): the one combination for which the library makes no cut"),
    "splitk_empty_tn": _case(132, 136, 164, "tn", bias=True, split_k=8, why="pieces past the last K-tile (two at BK = 32, five at 64) add nothing; bias once"),
    "alpha_nn": _case(132, 136, 164, "nn", bias=True, accumulate=True, alpha=-0.5, why="alpha scales the product, not the bias"),
    "alpha_tt": _case(132, 136, 164, "tt", bias=True, accumulate=True, alpha=-0.5, why="alpha scales the product, not the bias"),
    "batch_tn": _case(68, 72, 164, "tn", batch=3, gaps=(16, 40, 24), split_k=2, why="three batches with NaN gaps (strides multiples of 4), split_k = 2 onto start "
                      "values: the blockIdx.z decomposition"),
    "batch_odd_nn": _case(68, 72, 164, "nn", batch=3, gaps=(13, 7, 5), bias=True, act="relu", why="odd batch strides: scalar loads through a stride alone"),
    "f128_nn": _case(256, 1024, 36, "nn", batch=16, gaps=(8, 8, 16), forms=F32_FORMS, why="256 tiles of 128 rows through batch: the smallest list on which the "
                     "fallback kernel takes its 128-row tile"),
    "tail_f_nt": _case(2112, 1024, 512, "nt", why="264 half tiles, 8 over a round: fallback kernel body + tail in f32_mfma"),
    "tail_s_nt": _case(4224, 1024, 512, "nt", bias=True, act="relu", why="264 tiles of the split kernel: body + tail, the tail activation over whole tile rows"),
    "tail_f_mixed_nt": _case(2112, 1152, 512, "nt", why="297 half tiles of nine per row, 41 over a round: the tail starts inside tile row 28, whose first four tiles "
                             "are body tiles that overwrite what the clearing of the tail's rows left"),
    "band_nn": _case(260, 2820, 164, "nn", bias=True, why="69 tiles in 23 columns: the split kernel's tile list in column bands of 8, 8 and 7 under the "
                     "XCD-aware order of a list of 64 tiles or more that is no multiple of 8"),
    "big_splitk_empty_tn": _case(256, 192, 168, "tn", bias=True, split_k=8, why="the big kernels' pieces past the last K-tile (two at 16 and at 32 deep) add "
                                 "nothing; bias once"),
    "k0_nn": _case(40, 24, 0, "nn", bias=True, act="relu", why="the empty sum: act(bias)"),
    "k0_acc_nn": _case(40, 24, 0, "nn", bias=True, accumulate=True, why="the empty sum onto start values: C0 + bias"),
})
del _l


def index(off, stride, ld, trans, rows, cols, batch):
    """Flat element indices [batch, rows, cols] of op(X)(r, c): X[r*ld + c], trans: X[c*ld + r]; batch b at + b*stride."""
    b = np.arange(batch, dtype=np.int64)[:, None, None]
    r = np.arange(rows, dtype=np.int64)[None, :, None]
    c = np.arange(cols, dtype=np.int64)[None, None, :]
    return off + b * stride + (c * ld + r if trans else r * ld + c)


def index_a(c):
    return index(c["a_off"], c["stride_a"], c["lda"], c["ta"], c["M"], c["K"], c["batch"])


def index_b(c):
    return index(c["b_off"], c["stride_b"], c["ldb"], c["tb"], c["K"], c["N"], c["batch"])


def index_c(c):
    return index(c["c_off"], c["stride_c"], c["ldc"], False, c["M"], c["N"], c["batch"])


def starts(c):
    """Whether the product lands on start values (else every one of its elements is written, and starts as NaN)."""
    return bool(c["accumulate"]) or c["split_k"] > 1


def _freeze(cd):
    for k in ("flat_a", "flat_b", "flat_c", "bias_v"):
        cd[k].setflags(write=False)
    return cd


@functools.lru_cache(maxsize=None)
def case_data(name):
    """The case with its flat float32 buffers flat_a / flat_b / flat_c (C before the call) and bias_v [N] - never modified."""
    cd = dict(CASES[name], name=name)
    g = np.random.default_rng(list(CASES).index(name) + 977)
    nan = lambda n: np.full(n, np.nan, np.float32)
    cd["flat_a"], cd["flat_b"], cd["flat_c"] = nan(cd["size_a"]), nan(cd["size_b"]), nan(cd["size_c"])
    ia, ib, ic = index_a(cd), index_b(cd), index_c(cd)
    cd["flat_a"][ia] = g.normal(0, 1, ia.shape)
    cd["flat_b"][ib] = g.normal(0, 1.0 / np.sqrt(max(cd["K"], 1)), ib.shape)
    cd["bias_v"] = np.asarray(g.normal(0, 0.3, cd["N"]), np.float32)
    if starts(cd):
        cd["flat_c"][ic] = g.normal(0, 1, ic.shape)
    return _freeze(cd)


FAULTS = ("k_tail_dropped", "bias_per_piece", "alpha_on_bias", "act_outside", "pitch_ignored", "offset_ignored", "stride_mixup", "trans_b_ignored")


def evaluate(cd, dtype=np.float64, rounded=False, fault=None):
    """The product of a case in `dtype`, as a float64 array [batch M, N] (the judged layout: one slice per output row).
    fault: the wrong implementations tests/test_cpu_gemm_plain_ref.py holds the judge against (FAULTS)."""
    c = dict(cd)
    M, N, K, nb = c["M"], c["N"], c["K"], c["batch"]
    if fault == "pitch_ignored":                              # both operands read as if tight
        c["lda"], c["ldb"] = (M if c["ta"] else K), (K if c["tb"] else N)
    if fault == "offset_ignored":                             # the bases without the elements they lie into their allocations
        c["a_off"], c["b_off"] = c["a_off"] - c["xa"], c["b_off"] - c["xb"]
    if fault == "stride_mixup":                               # batch stride of A taken for B
        c["stride_b"] = c["stride_a"]
    if fault == "trans_b_ignored":
        c["tb"] = False
    rnd = bf16_round if rounded else (lambda a: a)
    A = rnd(np.take(cd["flat_a"], index_a(c), mode="clip")).astype(dtype)         # (a wrong implementation may index past the end: the NaN guard)
    B = rnd(np.take(cd["flat_b"], index_b(c), mode="clip")).astype(dtype)
    if fault == "k_tail_dropped":                             # the last K % 32 terms
        A, B = A[:, :, :K // 32 * 32], B[:, :K // 32 * 32]
    bias = (cd["bias_v"] if c["bias"] else np.zeros(N, np.float32)).astype(dtype)
    c0 = cd["flat_c"][index_c(cd)].astype(dtype) if starts(c) else None
    alpha = dtype(c["alpha"])
    prod = np.matmul(A, B) if K > 0 else np.zeros((nb, M, N), dtype)
    if fault == "alpha_on_bias":
        v = alpha * (prod + bias)
    else:
        v = alpha * prod + bias * dtype(c["split_k"] if fault == "bias_per_piece" else 1)
    assert v.dtype == dtype
    if c["split_k"] > 1:
        assert c["act"] == "none"
        out = c0 + v
    elif fault == "act_outside" and c["accumulate"]:
        out = act_fn(c0 + v, c["act"])
    else:
        out = act_fn(v, c["act"])
        if c["accumulate"]:
            out = c0 + out
    assert out.dtype == dtype
    return np.asarray(out, np.float64).reshape(nb * M, N)


@functools.lru_cache(maxsize=None)
def reference(name, rounded=False):
    """(fp64 product [batch M, N], e32) of a case: e32 = the worst row error of the float32 evaluation; rounded: the bf16-operand statements,
    reference and float32 evaluation alike.  Computed once per process, never modified."""
    cd = case_data(name)
    ref, r32 = evaluate(cd, np.float64, rounded), evaluate(cd, np.float32, rounded)
    ref.setflags(write=False)
    return ref, float(slice_err(r32, ref).max())


def bound_of(e32):
    return max(MARGIN * e32, FLOOR)


def judge(got, ref, e32):
    """(worst row error, bound): got against ref row by row on the row's own scale; bound = MARGIN x e32, at least FLOOR."""
    got = np.asarray(got, np.float64).reshape(ref.shape)
    return float(slice_err(got, ref).max()), bound_of(e32)


def written(cd, values, fault=None):
    """The flat output after a call that wrote `values` [batch M, N].  fault "clear_ldc": ... and cleared the rows over ldc instead of N columns."""
    flat = cd["flat_c"].copy()
    if fault == "clear_ldc":
        flat[index(cd["c_off"], cd["stride_c"], cd["ldc"], False, cd["M"], cd["ldc"], cd["batch"])] = 0.0
    else:
        assert fault is None, fault
    flat[index_c(cd)] = np.asarray(values, np.float32).reshape(cd["batch"], cd["M"], cd["N"])
    return flat


def outside_is_nan(cd, flat):
    """Everything of the flat output outside the product's elements is (still) NaN."""
    out = np.ones(flat.shape, bool)
    out[index_c(cd)] = False
    return bool(np.isnan(flat[out]).all())


def taken(cd, flat):
    """The product's elements of a flat output, [batch M, N] float64."""
    return np.asarray(flat, np.float64)[index_c(cd)].reshape(cd["batch"] * cd["M"], cd["N"])


# ---- which kernel the dispatch conditions select (csrc/gemm.hip mstts_gemm_f32, csrc/gemm_bf16.hip mstts_gemm_bf16) for a plain product in
# a form of tests/gemm_forms.FORMS, restated so that it can be tabulated and asserted without a GPU; printed beside every measured figure.
def loads(c):
    """"vector", or which of gemm_args_from's three independent triggers sends the product to the scalar loads."""
    why = []
    if (c["M"] if c["ta"] else c["K"]) % 4 or (c["K"] if c["tb"] else c["N"]) % 4:
        why.append("dims")
    if c["a_off"] % 4 or c["b_off"] % 4:                      # (every allocation is 16-byte aligned: the element offset decides)
        why.append("base")
    if c["lda"] % 4 or c["ldb"] % 4 or c["stride_a"] % 4 or c["stride_b"] % 4:
        why.append("pitch")
    return "scalar (%s)" % ", ".join(why) if why else "vector"


def bf16_autocut(M, N, K):
    """The number of pieces mstts_gemm_bf16 cuts a product without a cut of its own into (its cost model; 1: none)."""
    cdiv = lambda a, b: -(-a // b)
    tiles, best, best_cost = cdiv(M, 128) * cdiv(N, 128), 1, 0.0
    for sk in range(1, 65):
        if sk > 1 and K // sk < 128:
            break
        cost = cdiv(tiles * sk, 512) * (K / sk + 300.0) * (1.0 + 0.02 * sk)
        if sk == 1 or cost < best_cost * 0.97:
            best, best_cost = sk, cost
    return best


def selected_kernel(form, c):
    cdiv = lambda a, b: -(-a // b)
    M, N, K, batch, split, act, acc = c["M"], c["N"], c["K"], c["batch"], max(c["split_k"], 1), c["act"], c["accumulate"]
    if form.startswith("bf16"):
        if form == "bf16_big" and M >= 192 and N >= 192 and cdiv(M, 256) * cdiv(N, 256) * batch * split >= 1:
            return "bf16 256x256"
        cut = bf16_autocut(M, N, K) if split == 1 and act == "none" and batch == 1 else 1
        return "bf16 128x128" + (", library K-cut x%d" % cut if cut > 1 else "")
    if M <= 32:
        return "f32 MFMA, 32-row tile"
    det = form == "default_det"
    split3 = form != "f32_mfma" and K >= 160
    t128, t64 = cdiv(M, 128) * cdiv(N, 128) * batch * split, cdiv(M, 64) * cdiv(N, 128) * batch * split
    e128, e64 = t128 / (cdiv(t128, 256) * 256.0), t64 / (cdiv(t64, 256) * 256.0)
    bm, tail_s, tail_rem = (64 if e64 * 0.95 > e128 and not split3 else 128), 1, 0
    if not det and batch == 1 and split == 1 and (act == "none" or not acc):
        best = float(cdiv(t128, 256)) if bm == 128 else cdiv(t64, 256) * 0.54
        ktiles = cdiv(K, 32)
        for cand in ((128,) if split3 else (128, 64)):
            tn = cdiv(N, 128)
            t = cdiv(M, cand) * tn
            rem = t % 256
            if act != "none":
                rem = t - (t - rem) // tn * tn
            if split3 and t <= 128:
                rem = t
            elif t <= 256 or rem == 0 or rem > 128:
                continue
            s = min(256 // rem, 16, ktiles // 8)
            if s < 2:
                continue
            cost = (t // 256 + 1.25 / s + 0.06) * (1.0 if cand == 128 else 0.54)
            if cost < best:
                best, bm, tail_s, tail_rem = cost, cand, s, rem
    if split3 and form in ("split_big", "default_det") and M >= 192 and N >= 192 and (act == "none" or split == 1):
        if cdiv(M, 256) * cdiv(N, 256) * batch * split >= (1 if form == "split_big" else 160):
            return "split 256x256"
    tiles = cdiv(M, bm) * cdiv(N, 128)
    tail = "" if tail_s == 1 else (", every tile K-cut" if tail_rem == tiles else ", body + tail") + (" + tail act" if act != "none" else "")
    return ("split 128x128" if split3 else "f32 MFMA, %d-row tile" % bm) + tail


# ---- selection products: every output is ONE product, so its exact value is known and no accumulation order enters --------------------------
# The claim (include/mstts.h at mstts_gemm_split3, csrc/gemm_split.inc): x = hi + mid + lo exactly, a b evaluated as the six bf16 products
# hi.hi + hi.mid + mid.hi + mid.mid + hi.lo + lo.hi accumulated in fp32; dropped: mid.lo + lo.mid + lo.lo.
# Bound of ONE such product against its exact value a b, relative to |a b|, u = 2^-24 (fp32 unit roundoff), |mid| <= 2^-9 |x|, |lo| <= 2^-18 |x|,
# |hi| <= (1 + 2^-9) |x|:
#   dropped terms      |mid.lo + lo.mid + lo.lo| <= (2 x 2^-27 + 2^-36) |a b| <= 2^-26 (1 + 2^-9) |a b|                 (the header's figure)
#   accumulation       six additions into the fp32 accumulator (the last one is the final rounding; all the other K - 1 terms of the
#                      contraction are exact zeros and add nothing), each rounding a partial sum of at most (1 + 2^-7) |a b| by at most u of
#                      it:  6 u (1 + 2^-7) |a b|
#   epilogue           alpha = 1, no bias, no activation: exact
# SPLIT_BOUND = 6 (1 + 2^-7) 2^-24 + (1 + 2^-9) 2^-26 = 3.76e-7.  A lost plane or product moves an output by up to 2^-17 |a b| = 7.6e-6 (a term
# with `lo`) or 2^-8 |a b| (a term with `mid`): twenty times the bound and more on most outputs.
SPLIT_BOUND = 6 * (1 + 2.0 ** -7) * 2.0 ** -24 + (1 + 2.0 ** -9) * 2.0 ** -26
SEL_SHAPES = {"s132": (132, 136, 164), "s194": (194, 260, 768)}          # the second on the big-tile kernels where the form has them
SEL_WAYS = ("b_selects_one", "a_selects_one", "b_selects_val", "a_selects_val")
SEL_NAMES = ["%s_%s_%s" % (s, w, l) for s in SEL_SHAPES for w in SEL_WAYS for l in ("nn", "nt")]


def _full_mantissa(g, shape):
    """float32 values +-2^e (1 + f 2^-23) with all 23 fraction bits drawn at random, e in -2 .. 1."""
    bits = g.integers(0, 1 << 23, shape, dtype=np.uint32) | np.uint32(127 << 23)
    v = bits.view(np.float32) * np.exp2(g.integers(-2, 2, shape)).astype(np.float32)
    return v * g.choice(np.asarray([-1.0, 1.0], np.float32), shape)


@functools.lru_cache(maxsize=None)
def selection_data(name):
    """A selection case in case_data's form (flat NaN-guarded buffers), plus "exact": the exact value of every output, float64 [M, N].
    b_selects_*: op(B) [K, N] has ONE non-zero per column n, at row sel[n]: C(m, n) = A(m, sel[n]) . B(sel[n], n); a_selects_*: op(A) [M, K]
    has one non-zero per row m, at column sel[m]: C(m, n) = A(m, sel[m]) . B(sel[m], n).  *_one: the selector's entries are 1.0; *_val:
    full-mantissa values themselves.  The other operand holds full-mantissa values.  sel covers k = 0 and k = K - 1."""
    shape, rest = name.split("_", 1)
    way, lay = rest.rsplit("_", 1)
    M, N, K = SEL_SHAPES[shape]
    cd = dict(_case(M, N, K, lay, why="selection product"), name=name)
    g = np.random.default_rng(SEL_NAMES.index(name) + 4099)
    a_sel = way.startswith("a_")
    n_sel = M if a_sel else N
    sel = g.integers(0, K, n_sel)
    sel[0], sel[-1], sel[1] = 0, K - 1, (K - 1) // 32 * 32    # first, last (inside the K tail) and the first element of the last K-tile
    entries = _full_mantissa(g, n_sel) if way.endswith("_val") else np.ones(n_sel, np.float32)
    A, B = _full_mantissa(g, (M, K)), _full_mantissa(g, (K, N))
    if a_sel:
        A = np.zeros((M, K), np.float32)
        A[np.arange(M), sel] = entries
    else:
        B = np.zeros((K, N), np.float32)
        B[sel, np.arange(N)] = entries
    nan = lambda n: np.full(n, np.nan, np.float32)
    cd["flat_a"], cd["flat_b"], cd["flat_c"], cd["bias_v"] = nan(cd["size_a"]), nan(cd["size_b"]), nan(cd["size_c"]), np.zeros(N, np.float32)
    cd["flat_a"][index_a(cd)] = A[None]
    cd["flat_b"][index_b(cd)] = B[None]
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    if a_sel:
        exact = entries.astype(np.float64)[:, None] * B64[sel]                     # [M, N]: exact in float64 (24 + 24 significand bits)
    else:
        exact = A64[:, sel] * entries.astype(np.float64)[None]
    exact.setflags(write=False)
    cd.update(exact=exact, op_a=A, op_b=B, way=way)
    A.setflags(write=False)
    B.setflags(write=False)
    return _freeze(cd)


def planes(x):
    """The exact three-way split of csrc/gemm_split.inc: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid), in float32."""
    x = np.asarray(x, np.float32)
    hi = bf16_round(x)
    mid = bf16_round(x - hi)
    lo = bf16_round(x - hi - mid)
    return hi, mid, lo


SPLIT_PRODUCTS = ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0))      # (plane of a, plane of b) in gemm_split_kernel's order


def split_emulation(cd, drop_product=None, zero_plane=None):
    """The six-product split of a selection case's single products in NumPy: planes by bf16_round, products and sums in float32, in the kernel's
    order.  drop_product: index into SPLIT_PRODUCTS left out; zero_plane: ("a" | "b", plane index) zeroed.  float64 [M, N]."""
    a_sel = cd["way"].startswith("a_")
    A, B = cd["op_a"], cd["op_b"]
    if a_sel:
        sel = np.abs(A).argmax(1)
        a, b = A[np.arange(cd["M"]), sel][:, None] * np.ones((1, cd["N"]), np.float32), B[sel]
    else:
        sel = np.abs(B).argmax(0)
        a, b = A[:, sel], B[sel, np.arange(cd["N"])][None] * np.ones((cd["M"], 1), np.float32)
    pa, pb = list(planes(a)), list(planes(b))
    if zero_plane is not None:
        side = pa if zero_plane[0] == "a" else pb
        side[zero_plane[1]] = np.zeros_like(side[zero_plane[1]])
    acc = np.zeros(a.shape, np.float32)
    for i, (p, q) in enumerate(SPLIT_PRODUCTS):
        if i != drop_product:
            acc = acc + pa[p] * pb[q]
            assert acc.dtype == np.float32
    return acc.astype(np.float64)


def selection_err(got, exact):
    """The worst |got - exact| / |exact| over the outputs (every exact value is non-zero)."""
    got = np.asarray(got, np.float64).reshape(exact.shape)
    with np.errstate(invalid="ignore"):
        e = np.abs(got - exact) / np.abs(exact)
    return float(np.where(np.isfinite(got), e, np.inf).max())
