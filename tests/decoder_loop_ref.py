"""fp64 checker of the teacher-forced decoder loop drivers and their BPTT (tests/test_gpu_decoder_loop_ref.py; pinned without a GPU by
tests/test_cpu_decoder_loop_ref.py).

The reference is `unrolled_decoder`: the training branch of oracle.model.decoder's loop written out around oracle.model.zoneout_lstm_cell and
oracle.model.lsa_step, on the HOISTED inputs the drivers take - xw0 [S,B,4H] (or the prenet output `pre` with the prenet rows wx0 of the cell-0
kernel and b0: the persistent launch's pre / b0 form), the cell-0 kernel with its two context blocks folded as oracle.model.decoder folds them,
w1, b1, wq, the five attention variables, keys, values, token lengths, the four zoneout keep-masks - and keeping everything the drivers store,
in their layout (include/mstts.h, the block above mstts_decoder_train_desc).  Gradients are torch.autograd's of loss = (pj * d_pj).sum().  The
drivers' gradient outputs belong to intermediate nodes; each is obtained from a zero-valued leaf ("probe") added at that node:
    dg0     = d / d xw0 (xw0 enters the cell-0 gates additively; the pre form has a probe there instead)
    dg1     = probe on the cell-1 gates
    dq_hist = probe on the query q
    de_hist = probe on the energy before the length mask
    d_in0   = probe on the [ctx | h0] rows cell 0 of step s multiplies by the folded kernel = dg0[s] . w0f^T, the gradient through cell 0 only
oracle.model.lsa_step has no place for the probes on q and on the energy: `lsa_step_probed` restates its lines for those two, and the CPU
test holds it to lsa_step bit for bit.

Judging (slice_err, MARGIN, FLOOR, SLICE_EPS of tests/lstm_seq_ref.py): every slice over the last axis - every (step, row) of every quantity -
on its own scale max|ref slice| + 1e-3 max|ref|; the bound of a quantity is 8 x e32, e32 = the worst slice error of THIS checker evaluated in
float32 on the CPU, never less than 1e-6.  The query gradient cancels (the softmax makes sum_t d_e = 0); its e32 carries the same
cancellation, which is why the bound is relative to it."""
import functools

import numpy as np
import torch

from oracle import model as OM
from tests.lstm_seq_ref import FLOOR, MARGIN, SLICE_EPS, slice_err      # noqa: F401  (the project's constants, not copies)

RATE = 0.1
A, CH, KS = 128, 32, 31             # the attention widths the kernels are built for (tests/helpers.py::small_dims)
# decoder / encoder / speaker / prenet widths: tests/helpers.py::small_dims, test_gpu_loop_tiers.py::MID, test_gpu_persist.py::WIDE (the GPU
# test asserts that they still agree); M = 2 * enc_lstm + spk
WIDTHS = {
    "defaults": dict(dec_lstm=32, enc_lstm=16, spk=16, prenet=16),
    "MID": dict(dec_lstm=64, enc_lstm=32, spk=64, prenet=32),
    "WIDE": dict(dec_lstm=1024, enc_lstm=256, spk=256, prenet=256),
    # tests/decoder_infer_ref.py only: MID's cells with a prenet of 64, the narrowest the free-running driver's weight-streaming path takes
    # (the name sorts last: the draws of the three above stay what they were)
    "h64_p64": dict(dec_lstm=64, enc_lstm=32, spk=64, prenet=64),
}
# S counts decoder steps.  Row 0 has token length Te, row 1 length 1 (a softmax over one position: d_e = 0), the others anything in 1..Te.
CASES = {
    "two_steps": dict(widths="defaults", B=1, Te=7, S=2),          # smallest batch; one live BPTT hand-over; no fused cells, cell 0's forward product on the tiled GEMM
    "plain_h32": dict(widths="defaults", B=3, Te=9, S=4),          # tiled-GEMM forward products, one-slab backward products
    "fused_h64": dict(widths="MID", B=5, Te=18, S=5),              # fused cell steps without the fused query, skinny K-splits
    "two_pass_t140": dict(widths="MID", B=2, Te=140, S=3),         # more tokens than one attention pass
    "wide_one_tile": dict(widths="WIDE", B=3, Te=7, S=4),          # fused query, folded query gradient, several d_in0 slabs; persistent launches
    "wide_two_tiles": dict(widths="WIDE", B=17, Te=12, S=4),       # both MFMA row tiles live
    "wide_full": dict(widths="WIDE", B=32, Te=128, S=3),           # full batch at the 128-token geometry
    "wide_t131": dict(widths="WIDE", B=5, Te=131, S=3),            # the 256-position persistent instantiation
}
FORWARD_Q = ("in0", "in1", "pj", "c0", "c1", "acts0", "acts1", "craw0", "craw1", "q_hist", "align_hist", "cum_hist")
# d_ctx = the context columns of d_in0 slots 1 .. S-1: all of d_in0 that the persistent BPTT writes (complete, in its first slab)
BACKWARD_Q = ("dg0", "dg1", "dq_hist", "de_hist", "d_in0", "d_ctx")
HOST_Q = ("dw0f", "dw1", "db1", "dwq", "d_values")
QUANTITIES = FORWARD_Q + BACKWARD_Q + HOST_Q
LSA_NAMES = ("conv_k", "conv_b", "dense_k", "score_w", "score_b")
LSA_PATHS = dict(conv_k="attention_convolution_dense_layer/conv1d/kernel", conv_b="attention_convolution_dense_layer/conv1d/bias",
                 dense_k="attention_convolution_dense_layer/dense/kernel", score_w="score_layer/weight_w", score_b="score_layer/bias_b")
WEIGHTS = ("w0f", "w1", "b1", "wq", "wx0", "b0") + LSA_NAMES
MASKS = ("zc0", "zh0", "zc1", "zh1")

# Slots that neither loop writes or reads (tests/test_gpu_persist.py::_snapshot), excluded HERE and nowhere else: the comparison sees the
# reference's own numbers there.
#   in1 slot S, m0 half: in1[s] = [m0 of step s | h1 state before step s]; there is no step S, so only the h1 half of slot S exists.
#   c0 / c1 slot S, packed persistent form only: the packed operand blocks (opk) carry what the BPTT reads, and the state behind the last
#   step is no BPTT operand - mstts_persist_unpack_history cannot restore it.
def exclude_unwritten(got, ref, packed):
    """Copy of `got` with the excluded slots replaced by the reference's values."""
    out = dict(got)
    H = ref["c0"].shape[-1]
    out["in1"] = np.array(got["in1"], np.float64)
    out["in1"][-1, :, :H] = ref["in1"][-1, :, :H]
    if packed:
        for k in ("c0", "c1"):
            out[k] = np.array(got[k], np.float64)
            out[k][-1] = ref[k][-1]
    return out


def dims_of(widths):
    w = WIDTHS[widths]
    return dict(H=w["dec_lstm"], M=2 * w["enc_lstm"] + w["spk"], P=w["prenet"])


def _f32(a):
    return torch.tensor(np.asarray(a, np.float32))


@functools.lru_cache(maxsize=None)
def weights(widths):
    """The variables of one set of widths as float32 CPU tensors (what is uploaded), shared by the cases of those widths: weights
    N(0, 1 / sqrt(fan_in)), biases N(0, 0.1).  The cell-0 kernel is drawn whole, [P + 2M + H, 4H]; w0f = its two context blocks added and its
    recurrent rows, as oracle.model.decoder folds them, in fp64 and rounded once; wx0 = its prenet rows."""
    dm = dims_of(widths)
    H, M, P = dm["H"], dm["M"], dm["P"]
    g = np.random.default_rng(sorted(WIDTHS).index(widths) + 101)
    n = lambda fan_in, *s: g.normal(0, 1.0 / np.sqrt(fan_in), s).astype(np.float32)
    b = lambda *s: g.normal(0, 0.1, s).astype(np.float32)
    k0 = n(P + 2 * M + H, P + 2 * M + H, 4 * H)
    fold = np.concatenate([k0[P:P + M].astype(np.float64) + k0[P + M:P + 2 * M].astype(np.float64), k0[P + 2 * M:].astype(np.float64)])
    w = dict(w0f=_f32(fold), wx0=_f32(k0[:P]), b0=_f32(b(4 * H)), w1=_f32(n(2 * H, 2 * H, 4 * H)), b1=_f32(b(4 * H)), wq=_f32(n(H, H, A)),
             wmem=_f32(n(M, M, A)), conv_k=_f32(n(KS, KS, 1, CH)), conv_b=_f32(b(CH)), dense_k=_f32(n(CH, CH, A)), score_w=_f32(n(A, 1, 1, A)),
             score_b=_f32(b(1, 1, A)))
    return w


@functools.lru_cache(maxsize=None)
def case_data(name):
    """The inputs of a case as float32 / uint8 / int32 CPU tensors - the very arrays that are uploaded and that the reference reads.  values = a
    drawn memory zeroed past the row's length and keys = values . W_mem (oracle.model.attention_memory) formed in fp64 and rounded once;
    xw0 = pre . wx0 + b0 formed in fp64 and rounded once (the forms that read xw0 are judged against a reference that reads xw0, the pre / b0
    form against one that reads pre, wx0 and b0)."""
    cd = dict(CASES[name], name=name, **dims_of(CASES[name]["widths"]))
    B, T, S, H, M, P = cd["B"], cd["Te"], cd["S"], cd["H"], cd["M"], cd["P"]
    g = np.random.default_rng(sorted(CASES).index(name) + 11)
    w = weights(cd["widths"])
    lens = g.integers(1, T + 1, B)
    lens[0] = T
    if B > 1:
        lens[1] = 1
    cd["lens"] = torch.tensor(lens.astype(np.int32))
    live = np.arange(T)[None, :] < lens[:, None]
    memory = g.normal(0, 1, (B, T, M)).astype(np.float32) * live[:, :, None]
    cd["values"] = _f32(memory)
    cd["keys"] = (cd["values"].double() @ w["wmem"].double()).float()
    cd["pre"] = _f32(np.maximum(g.normal(0, 1, (S, B, P)), 0) * (g.random((S, B, P)) > 0.5) * 2.0)      # a prenet output: ReLU, dropout at 0.5
    cd["xw0"] = (cd["pre"].double() @ w["wx0"].double() + w["b0"].double()).float()
    for k in MASKS:
        cd[k] = torch.tensor((g.random((S, B, H)) > RATE).astype(np.uint8))
    cd["d_pj"] = _f32(g.normal(0, 0.5, (S, B, H + M)))
    for k in WEIGHTS:
        cd[k] = w[k]
    return cd


def live_mask(cd):
    """[B, Te] bool: token position t of row b lies inside the row's length."""
    return (torch.arange(cd["Te"])[None, :] < cd["lens"].long()[:, None]).numpy()


def lsa_params(lv):
    """The attention variables under oracle.model.lsa_step's names."""
    p = {OM.P_LSA + path: lv[k] for k, path in LSA_PATHS.items()}
    p[OM.P_LSA + "query_layer/kernel"] = lv["wq"]
    return p


def lsa_step_probed(p, keys, values, length_mask, query_in, cum, q_probe, e_probe):
    """oracle.model.lsa_step with a probe added to the query and one to the energy before the length mask (both zero-valued leaves); also
    returns q.  tests/test_cpu_decoder_loop_ref.py holds it to lsa_step bit for bit."""
    q = OM.rmm(query_in, p[OM.P_LSA + "query_layer/kernel"]) + q_probe
    f = OM.conv1d_same(cum[:, :, None], p[OM.P_LSA + "attention_convolution_dense_layer/conv1d/kernel"],
                       p[OM.P_LSA + "attention_convolution_dense_layer/conv1d/bias"])
    loc = f @ p[OM.P_LSA + "attention_convolution_dense_layer/dense/kernel"]
    w = p[OM.P_LSA + "score_layer/weight_w"].reshape(-1)
    b = p[OM.P_LSA + "score_layer/bias_b"].reshape(-1)
    energy = (w * torch.tanh(keys + q[:, None, :] + loc + b)).sum(dim=2) + e_probe
    energy = torch.where(length_mask, energy, torch.full_like(energy, -float("inf")))
    align = torch.softmax(energy, dim=1)
    ctx = (align[:, :, None] * values).sum(dim=1)
    return q, align, cum + align, ctx


def cell_saves(gates, c_prev, H):
    """What the drivers save of a cell step for the BPTT: the four gate activations (the forget gate as sigmoid(f + 1)) and the cell value
    before zoneout - the two save lines of tests/lstm_seq_ref.py::unrolled."""
    i, j, f, o = gates.chunk(4, dim=1)
    a = torch.cat([torch.sigmoid(i), torch.tanh(j), torch.sigmoid(f + 1.0), torch.sigmoid(o)], dim=1)
    return a, a[:, 2 * H:3 * H] * c_prev + a[:, :H] * a[:, H:2 * H]


def unrolled_decoder(lv, lens, masks, rate, probes=None, fault=None):
    """The training branch of oracle.model.decoder's loop on hoisted inputs.  lv: xw0 [S,B,4H] (or pre [S,B,P], wx0 [P,4H], b0), w0f
    [M+H,4H], w1, b1, wq, the five attention variables, keys [B,T,A], values [B,T,M]; masks: zc0, zh0, zc1, zh1 [S,B,H] keep-masks.
    probes: None (the attention step is oracle.model.lsa_step itself) or dict(in0 [S,B,M+H], g0, g1 [S,B,4H], q [S,B,A], e [S,B,T]) of
    zero-valued leaves (g0 optional).  fault: negative controls of the CPU test only - "zh0_in_cell1", "stale_cum".
    Returns the histories in the drivers' layout; the m0 half of in1 slot S, which does not exist, is 0."""
    keys, values, w0f, w1, b1, wq = lv["keys"], lv["values"], lv["w0f"], lv["w1"], lv["b1"], lv["wq"]
    B, T, _ = keys.shape
    H = w1.shape[0] // 2
    g0_in = lv["xw0"] if "xw0" in lv else OM.gmm(lv["pre"], lv["wx0"]) + lv["b0"]
    S = g0_in.shape[0]
    p = lsa_params(lv)
    lmask = torch.arange(T)[None, :] < lens.long()[:, None]
    z = lambda n: keys.new_zeros(B, n)
    c0, h0, c1, h1, ctx, cum = z(H), z(H), z(H), z(H), z(values.shape[2]), z(T)
    o = {k: [] for k in ("in0", "in1", "pj", "acts0", "acts1", "craw0", "craw1", "q_hist", "align_hist")}
    o["c0"], o["c1"], o["cum_hist"] = [c0], [c1], [cum]
    for s in range(S):
        rows0 = torch.cat([ctx, h0], dim=1)                      # in0 slot s: what cell 0 of step s multiplies by the folded kernel
        x0 = rows0 if probes is None else rows0 + probes["in0"][s]
        g0 = g0_in[s] + OM.rmm(x0, w0f)
        if probes is not None and "g0" in probes:
            g0 = g0 + probes["g0"][s]
        a0, cr0 = cell_saves(g0, c0, H)
        m0, c0n, h0n = OM.zoneout_lstm_cell(x0, c0, h0, None, None, masks["zc0"][s], masks["zh0"][s], rate, True, gates=g0)
        rows1 = torch.cat([m0, h1], dim=1)                       # in1 slot s
        g1 = OM.rmm(rows1, w1) + b1
        if probes is not None:
            g1 = g1 + probes["g1"][s]
        a1, cr1 = cell_saves(g1, c1, H)
        zh1 = masks["zh0" if fault == "zh0_in_cell1" else "zh1"][s]
        m1, c1n, h1n = OM.zoneout_lstm_cell(rows1, c1, h1, None, None, masks["zc1"][s], zh1, rate, True, gates=g1)
        cum_in = o["cum_hist"][s - 1] if fault == "stale_cum" and s > 0 else cum
        if probes is None:
            align, cum_n, ctx_n = OM.lsa_step(p, None, keys, values, lmask, m1, cum_in)
            q = OM.rmm(m1, wq)
        else:
            q, align, cum_n, ctx_n = lsa_step_probed(p, keys, values, lmask, m1, cum_in, probes["q"][s], probes["e"][s])
        for k, v in (("in0", rows0), ("in1", rows1), ("pj", torch.cat([m1, ctx_n], dim=1)), ("acts0", a0), ("acts1", a1), ("craw0", cr0),
                     ("craw1", cr1), ("q_hist", q), ("align_hist", align)):
            o[k].append(v)
        c0, h0, c1, h1, ctx, cum = c0n, h0n, c1n, h1n, ctx_n, cum_n
        o["c0"].append(c0); o["c1"].append(c1); o["cum_hist"].append(cum)
    o["in0"].append(torch.cat([ctx, h0], dim=1))
    o["in1"].append(torch.cat([z(H), h1], dim=1))
    return {k: torch.stack(v) for k, v in o.items()}


def leaves(cd, form, dtype):
    """Fresh leaves of a case: form "xw0" (xw0 is a leaf) or "pre" (pre, wx0, b0 are)."""
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_()      # never the cached tensor itself
    names = ("w0f", "w1", "b1", "wq", "keys", "values") + LSA_NAMES + (("xw0",) if form == "xw0" else ("pre", "wx0", "b0"))
    return {k: leaf(cd[k]) for k in names}


def make_probes(cd, form, dtype):
    B, T, S, H, M = cd["B"], cd["Te"], cd["S"], cd["H"], cd["M"]
    zl = lambda *s: torch.zeros(*s, dtype=dtype, requires_grad=True)
    pr = dict(in0=zl(S, B, M + H), g1=zl(S, B, 4 * H), q=zl(S, B, A), e=zl(S, B, T))
    if form != "xw0":
        pr["g0"] = zl(S, B, 4 * H)
    return pr


def host_grads(cd, t):
    """What the drivers' caller forms from their outputs, here in fp64 on the host (no GEMM kernel): dW0f = sum_s in0[s]^T dg0[s],
    dW1 = sum_s in1[s]^T dg1[s], db1 = sum dg1, dWq = sum_s m1[s]^T dq[s] and d_values[b] = sum_s align[s,b]^T (d_pj context columns [s] +
    d_in0 context columns [s+1]) - the context-gradient wiring with its slab sum, what engine.py's memory_gradient forms before the
    memory-layer terms.  t: in0, in1, pj, align_hist, dg0, dg1, dq_hist and d_ctx [S-1,B,M] (the slabs already summed)."""
    S, H = cd["S"], cd["H"]
    t = {k: np.asarray(t[k], np.float64) for k in ("in0", "in1", "pj", "align_hist", "dg0", "dg1", "dq_hist", "d_ctx")}
    d_c = cd["d_pj"].double().numpy()[:, :, H:].copy()
    d_c[:S - 1] += t["d_ctx"]
    return dict(dw0f=np.einsum("sbk,sbg->kg", t["in0"][:S], t["dg0"]), dw1=np.einsum("sbk,sbg->kg", t["in1"][:S], t["dg1"]),
                db1=t["dg1"].sum((0, 1))[None, :], dwq=np.einsum("sbk,sba->ka", t["pj"][:, :, :H], t["dq_hist"]),
                d_values=np.einsum("sbt,sbm->btm", t["align_hist"], d_c))


def _n(t):
    return t.detach().double().numpy()


def evaluate(cd, form, dtype, fault=None):
    """Every compared quantity from the checker in `dtype`, as float64 arrays: histories and saves are unrolled_decoder's, the drivers'
    gradient outputs its probes' gradients, the host-formed sums (HOST_Q) autograd's gradients of the leaves."""
    M = cd["M"]
    lv, pr = leaves(cd, form, dtype), make_probes(cd, form, dtype)
    o = unrolled_decoder(lv, cd["lens"], {k: cd[k] for k in MASKS}, RATE, probes=pr, fault=fault)
    (o["pj"] * cd["d_pj"].to(dtype)).sum().backward()
    q = {k: _n(o[k]) for k in FORWARD_Q}
    q["dg0"] = _n(lv["xw0"].grad if form == "xw0" else pr["g0"].grad)
    q["dg1"], q["dq_hist"], q["de_hist"], q["d_in0"] = _n(pr["g1"].grad), _n(pr["q"].grad), _n(pr["e"].grad), _n(pr["in0"].grad)
    q["d_ctx"] = q["d_in0"][1:, :, :M].copy()
    q["dw0f"], q["dw1"], q["db1"], q["dwq"], q["d_values"] = (_n(lv["w0f"].grad), _n(lv["w1"].grad), _n(lv["b1"].grad)[None, :], _n(lv["wq"].grad),
                                                              _n(lv["values"].grad))
    return q


# The host-formed weight gradients are sums of S * B outer products, row k of dW = sum_r X[r, k] . G[r, :] (r = (step, row)).  The drivers give -
# and any float32 evaluation gives - every operand row X[r, :] to a precision relative to THAT row's largest element, so the error of row k of
# dW is about eps . sum_r max|X[r, :]| . max|G[r, :]| whatever the size of X[:, k] itself: a row of dW that belongs to a small element of the
# operands (a context or state element near 0) has a relative error of its own up to 1 / SLICE_EPS times eps, and with few terms in the sum
# (two_steps: ONE live outer product, slot 0 of in0 being 0) the worst such row is a heavy-tailed draw - e32 of dw0f of two_steps came out at
# 4.3e-6 on one CPU and 0.79e-6 on another, and mstts_decoder_train_fwd / _bwd, whose in0 and dg0 are each within 1.3 x e32 of their own, at
# 6.7e-6 = 8.5 x the smaller of the two.  For these three quantities a slice's scale therefore also holds the magnitude of the terms of the sum,
# computed from the reference alone: sum_r max|X_ref[r, :]| . max|G_ref[r, :]|.  What they are there for - a gate gradient paired with the wrong
# slot, a step or a term dropped - moves whole rows by the size of those terms.
TERM_SCALED = {"dw0f": ("in0", "dg0"), "dw1": ("in1", "dg1"), "dwq": ("pj", "dq_hist")}


def term_scale(k, ref):
    """sum over (step, row) of max|operand row| . max|gate-gradient row| of a host-formed weight gradient, from the reference."""
    xk, gk = TERM_SCALED[k]
    S = ref[gk].shape[0]
    x = ref[xk][:S] if k != "dwq" else ref[xk][:, :, :ref["c0"].shape[-1]]
    return float((np.abs(x).max(-1) * np.abs(ref[gk]).max(-1)).sum())


def judged_err(k, got, ref):
    """The error of every slice of quantity k on the slice's scale: slice_err's, for TERM_SCALED quantities with term_scale added to the scale."""
    if k not in TERM_SCALED:
        return slice_err(got, ref[k])
    got, r = np.asarray(got, np.float64), ref[k]
    assert got.shape == r.shape, (got.shape, r.shape)
    err = np.abs(got - r).max(-1) / (np.abs(r).max(-1) + SLICE_EPS * np.abs(r).max() + term_scale(k, ref))
    return np.where(np.isfinite(got).all(-1), err, np.inf)


@functools.lru_cache(maxsize=None)
def evaluations(name, form="xw0"):
    """(the fp64 evaluation, the float32 evaluation) of a case in the given input form; computed once per process, never modified."""
    cd = case_data(name)
    ref, r32 = evaluate(cd, form, torch.float64), evaluate(cd, form, torch.float32)
    for v in list(ref.values()) + list(r32.values()):
        v.setflags(write=False)
    return ref, r32


@functools.lru_cache(maxsize=None)
def reference(name, form="xw0"):
    """(fp64 quantities, e32 per quantity, bound per quantity) of a case in the given input form."""
    ref, r32 = evaluations(name, form)
    e32 = {k: float(judged_err(k, r32[k], ref).max()) for k in QUANTITIES}
    bound = {k: max(MARGIN * e32[k], FLOOR) for k in e32}
    return ref, e32, bound


def exact_failures(cd, got):
    """Names of the exact conditions that `got` (any subset of the quantities) breaks: align_hist, de_hist and the increments of cum_hist past a
    row's token length are 0; slot 0 of in0, c0, c1, cum_hist and the state half of in1 slot 0 are 0."""
    dead = ~live_mask(cd)
    H = cd["H"]
    bad = []
    for k in ("align_hist", "de_hist"):
        if k in got and np.any(np.asarray(got[k])[:, dead] != 0.0):
            bad.append(k + ": not exactly 0 past a row's length")
    if "cum_hist" in got:
        cum = np.asarray(got["cum_hist"])
        if np.any((cum[1:] - cum[:-1])[:, dead] != 0.0):
            bad.append("cum_hist: increments not exactly 0 past a row's length")
    for k in ("in0", "c0", "c1", "cum_hist"):
        if k in got and np.any(np.asarray(got[k])[0] != 0.0):
            bad.append(k + ": slot 0 not exactly 0")
    if "in1" in got and np.any(np.asarray(got["in1"])[0][:, H:] != 0.0):
        bad.append("in1: state half of slot 0 not exactly 0")
    return bad


def judge(name, form, got, quantities, packed=False):
    """[(quantity, e32, worst slice error, bound)] of `got` against the reference, the excluded slots taken out."""
    ref, e32, bound = reference(name, form)
    got = exclude_unwritten(got, ref, packed) if "in1" in got else got
    return [(k, e32[k], float(judged_err(k, got[k], ref).max()), bound[k]) for k in quantities]
