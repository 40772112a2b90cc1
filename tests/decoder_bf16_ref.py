"""Stage-wise fp64 checker of the bf16 forms of the teacher-forced decoder loop drivers and their BPTT (tests/test_gpu_decoder_bf16_ref.py;
pinned without a GPU by tests/test_cpu_decoder_bf16_ref.py).  bf(x) = x.to(torch.bfloat16) widened again (round to nearest even).

Why stage-wise.  Rounding to 8 mantissa bits is discontinuous: two evaluations of the loop that differ by 1e-7 round a few operands differently
and the loop amplifies each flip, which is why the trajectory comparisons of the bf16 forms carry bounds of 2e-3 .. 1e-1.  The drivers store,
in fp32, the very arrays their products round (in0, in1, pj; dg0, dg1, dq_hist - unrounded, include/mstts.h), so this checker never follows a
trajectory of its own: every stage of every step is evaluated from the history the form itself stored ("got"), the checker and the kernel
round identical numbers, no flip can occur, and the bf16 kernels are held to fp32-accumulation accuracy - the bounds of their fp32 siblings.

Forward, one step ahead, for every step s (slot s + 1 of a history is written by step s):
    cell 0      gates = xw0[s] (NOT rounded) + bf(got.in0[s]) . bf(w0f)          [pre form: b0 + bf(pre[s]) . bf(wx0) + bf(got.in0[s]) . bf(w0f)]
                cell update with got.c0[s], the h0 columns of got.in0[s]          -> acts0[s], craw0[s], c0[s+1], in0[s+1] h0 columns, in1[s] m0 columns
    cell 1      gates = b1 + bf(got.in1[s]) . bf(w1), got.c1[s]                    -> acts1[s], craw1[s], c1[s+1], in1[s+1] h1 columns, pj[s] m1 columns
    query       bf(m1 columns of got.pj[s]) . bf(wq)                               -> q_hist[s]
    attention   lsa_step (fp32 in every form) on got.q_hist[s], got.cum_hist[s]    -> align_hist[s], cum_hist[s+1], pj[s] context columns
and, exactly, the context columns of in0[s+1] are bit-identical to those of pj[s] (context_identity_failures; a trajectory test gets this for
free, a stage-wise one does not).  in0 / in1 / pj are judged per column block (in0_h0, in1_m0, in1_h1, pj_m1, pj_ctx), each block's slices
on their own scale; the excluded slots and the exact conditions are decoder_loop_ref's (exclude_unwritten, exact_failures).

BPTT.  Given a forward history the BPTT is linear in d_pj and its only rounding sites are the left operands of the three data-gradient
products, which the drivers store unrounded.  The checker is autograd through the same loop with (a) every state replaced IN VALUE by the
form's stored one while the gradient flows on to the checker's own graph (_Replace: forward returns the stored tensor bit for bit) and (b)
products whose backward multiplies bf(the form's stored gradient) instead of the incoming one (_StoredGradProduct):
    [d_m0 | d_h1] = bf(got.dg1[s]) . bf(w1)^T      [d_ctx | d_h0] = bf(got.dg0[s]) . bf(w0f)^T      d_m1 (query) = bf(got.dq_hist[s]) . bf(wq)^T
The incoming gradients are what decoder_loop_ref's probes report: dg0[s], dg1[s], dq_hist[s], de_hist[s], d_in0[s] (= the middle product
above) and d_ctx.  The cell-state gradients and the attention's carried gradients (cum, location features) are smooth and carried by the
graph itself.  So step s is judged from the form's outputs of step s + 1, which the previous iteration has just judged.  The host-formed
dw0f, dw1, db1, dwq, d_values are decoder_loop_ref.host_grads of the form's tensors against host_grads of the expected ones (unrounded
operands, as the kernels and oracle.model._BF16MatMul form them), TERM_SCALED included.

Bounds: MARGIN (8) x e32 per quantity, never less than FLOOR (1e-6), on decoder_loop_ref's slice scale; e32 = the worst slice difference
between THIS checker evaluated in float32 and in float64 on the same `got` - a property of the checker's two evaluations, never of the judged
tensors (which must be finite before anything is judged: the caller NaN-fills every buffer a form writes in full).

What today's trajectory bounds do not see (tests/test_cpu_decoder_bf16_ref.py, case fused_h64, one site of step 2 of 5 faulted in the synthetic
float32 form; whole-tensor max|diff| / max|ref| over the full trajectory against the unfaulted run, beside test_train_step_parity_bf16_recurrent's
2e-3 on linear-side tensors and 2e-2 on gradients; then the stage-wise error / bound at the faulted stage and step):
    fault                      pj       align_hist  (2e-3)    dg0      (2e-2)    stage-wise
    truncate_cell1_operand     1.7e-04  1.1e-05               9.9e-04            cell1 of step 2 at 2135 x its bound
    query_operand_unrounded    3.0e-05  5.6e-06               6.5e-04            query of step 2 at 1595 x
    xw0_rounded                8.4e-05  1.4e-05               2.6e-03            cell0 of step 2 at 1446 x
    dg0_product_fp32           0        0                     2.1e-04            cell0_product of step 2 at 1492 x
At most 0.13 of a trajectory bound, each; the other controls (dq_hist_stored_rounded 618 x, dg1_wrong_half 8e5 x, zh0_in_cell1, stale_cum) are
reported in their stage and step likewise, nothing judged before it over its bound.

The persistent launches round an exchanged copy of what they store: PERSISTENT_SITES below.
"""
import contextlib

import numpy as np
import torch

from oracle import model as OM
from tests import decoder_loop_ref as R
from tests.decoder_loop_ref import (CASES, FLOOR, MARGIN, SLICE_EPS, case_data, cell_saves, host_grads, lsa_params, lsa_step_probed,     # noqa: F401
                                    slice_err, weights)

# the cases whose widths mstts_decoder_bf16_splits(H, M, A) admits (multiples of 64); the GPU test asserts the query per case
BF16_CASES = tuple(n for n in CASES if CASES[n]["widths"] in ("MID", "WIDE"))
# judged column blocks of the three row-block histories: name -> (history, columns as a function of (H, M))
BLOCKS = {"in0_h0": ("in0", lambda H, M: slice(M, M + H)), "in1_m0": ("in1", lambda H, M: slice(0, H)), "in1_h1": ("in1", lambda H, M: slice(H, 2 * H)),
          "pj_m1": ("pj", lambda H, M: slice(0, H)), "pj_ctx": ("pj", lambda H, M: slice(H, H + M))}
# the stages in the order a step runs them, with what each is judged by; histories with S + 1 slots: slot j is written by step j - 1
FORWARD_STAGES = (("cell0", ("acts0", "craw0", "c0", "in0_h0", "in1_m0")), ("cell1", ("acts1", "craw1", "c1", "in1_h1", "pj_m1")),
                  ("query", ("q_hist",)), ("attention", ("align_hist", "cum_hist", "pj_ctx")))
BACKWARD_STAGES = (("attention_bwd", ("de_hist", "dq_hist")), ("cell1_bwd", ("dg1",)), ("cell0_bwd", ("dg0",)), ("cell0_product", ("d_in0", "d_ctx")))
SLOT_OF_NEXT_STEP = ("c0", "c1", "in0_h0", "in1_h1", "cum_hist")
FORWARD_Q = tuple(k for _, ks in FORWARD_STAGES for k in ks)
BACKWARD_Q = tuple(k for _, ks in BACKWARD_STAGES for k in ks)
PERSIST_BWD_Q = ("de_hist", "dq_hist", "dg1", "dg0", "d_ctx")
HOST_Q = R.HOST_Q
FAULTS = ("truncate_cell1_operand", "query_operand_unrounded", "xw0_rounded", "dg0_product_fp32", "dq_hist_stored_rounded", "dg1_wrong_half",
          "zh0_in_cell1", "stale_cum")


def bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def bf_truncate(t):
    """float32 -> bf16 by dropping the low 16 bits (the negative control; never what a kernel may do)."""
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


class _Replace(torch.autograd.Function):
    """Straight-through state: the value is `stored` bit for bit (not own + (stored - own), which rounds), the gradient goes to `own`."""
    @staticmethod
    def forward(ctx, own, stored):
        return stored.clone()

    @staticmethod
    def backward(ctx, g):
        return g, None


class _StoredGradProduct(torch.autograd.Function):
    """y = r(x) . r(w); dx = r(g_stored) . r(w)^T with the form's STORED gradient of y in place of the incoming one (which the probe
    added to y reports); r = bf, or the identity for the CPU test's no-rounding check."""
    @staticmethod
    def forward(ctx, x, w, g_stored, rounding, x_operand=None):
        """x_operand: what the kernel rounds where that is not x bit for bit (exchanged_copy), else None."""
        r = bf if rounding else (lambda v: v)
        ctx.save_for_backward(r(w), None if g_stored is None else r(g_stored))
        return r(x if x_operand is None else x_operand) @ r(w)

    @staticmethod
    def backward(ctx, g):
        wr, gs = ctx.saved_tensors
        return gs @ wr.t(), None, None, None, None


def exchanged_copy(a, gen):
    """What a consumer of the persistent launches' rings receives of the float32 array `a`: the value with the ring slot's GENERATION in the
    lowest bit of its mantissa (csrc/persist_common.h, "the data is the flag"; 2^-24 relative, deterministic).  The persistent bf16 launches
    round THIS copy, not the exact value they store for the BPTT / the weight-gradient products - see PERSISTENT_SITES."""
    a = np.ascontiguousarray(a, np.float32)
    return ((a.view(np.uint32) & np.uint32(0xFFFFFFFE)) | np.uint32(gen)).view(np.float32)


# The one family of rounding sites that is not fed from a stored tensor bit for bit.  The persistent launches hand m0, h0, h1, m1, the context
# and the gate gradients from workgroup to workgroup with the ring slot's generation in the last mantissa bit, and their bf16 instantiations
# round the copy that ARRIVED (slice_complete_bf16 / the m1 row in csrc/persist.hip, PROD_GATHER in csrc/persist_bwd.hip), while the histories
# keep the exact value.  A stored value within one float32 ulp of a bf16 rounding boundary (2^-17 of all elements) then rounds the other way:
# one bf16 ulp of ONE operand element, 2e-5 .. 3e-4 of a gate or query slice - measured on an MI355X before the checker knew of it: 1 - 3 such
# elements per case of 1e5 .. 5e5 operand elements (wide_two_tiles: cell 0 and cell 1; wide_full: the query; wide_t131: cell 1), 18 .. 180 x
# the bound, every other stage at 0.3 .. 2 x e32.  The copy is a deterministic function of the stored value and the step, so the site is
# teacher-forced after all: the checker rounds exchanged_copy(stored value, generation), the very number the kernel rounds, and the bound stays
# 8 x e32.  Generations (ring of 4 slots): forward step s publishes with (s >> 2) & 1 - consumed in the same step (m0, m1) or by step s + 1
# (context, h0, h1); BPTT step s with ((S - 1 - s) >> 2) & 1 (dg0, dg1).  pre is read from memory and dq_hist is rounded where it is formed:
# neither is exchanged before its rounding.
PERSISTENT_SITES = ("in0[s]: context and h0 columns, generation of step s - 1", "in1[s]: m0 columns, generation of step s; h1 columns, of step s - 1",
                    "pj[s]: m1 columns, generation of step s", "dg0[s], dg1[s]: generation of BPTT step S - 1 - s")


def stagewise(cd, form, got, dtype, rounding=True, exchanged=False):
    """Every compared quantity as float64 arrays, in the drivers' layout, each stage of each step evaluated in `dtype` from the history
    `got` (arrays or tensors: in0, in1, pj, c0, c1, q_hist, cum_hist; with dg0, dg1, dq_hist also the BPTT).  form: "xw0" or "pre".
    exchanged: the persistent launches - the products round the exchanged copies of the stored values (PERSISTENT_SITES)."""
    B, T, S, H, M = cd["B"], cd["Te"], cd["S"], cd["H"], cd["M"]
    t = lambda a: torch.tensor(np.array(a)).to(dtype)               # (a copy: the caller's arrays may be read-only)
    g = {k: t(got[k]) for k in ("in0", "in1", "pj", "c0", "c1", "q_hist", "cum_hist")}
    bwd = "dg0" in got
    gs = {k: t(got[k]) if bwd else [None] * S for k in ("dg0", "dg1", "dq_hist")}
    xop = {k: [None] * S for k in ("in0", "in1", "m1")}
    if exchanged:
        gen = lambda k: (k >> 2) & 1
        for s in range(S):
            xop["in0"][s] = t(exchanged_copy(got["in0"][s], gen(s - 1))) if s else None         # (slot 0 is 0 and is not exchanged)
            xop["in1"][s] = t(np.concatenate([exchanged_copy(got["in1"][s][:, :H], gen(s)),
                                              exchanged_copy(got["in1"][s][:, H:], gen(s - 1)) if s else np.asarray(got["in1"][s][:, H:], np.float32)], axis=1))
            xop["m1"][s] = t(exchanged_copy(got["pj"][s][:, :H], gen(s)))
            if bwd:
                for k in ("dg0", "dg1"):
                    gs[k][s] = t(exchanged_copy(got[k][s], gen(S - 1 - s)))
    lv = {k: cd[k].to(dtype) for k in ("w0f", "w1", "b1", "wq", "keys", "values") + R.LSA_NAMES}
    r = bf if rounding else (lambda v: v)
    g0_in = cd["xw0"].to(dtype) if form == "xw0" else cd["b0"].to(dtype) + r(cd["pre"].to(dtype)) @ r(cd["wx0"].to(dtype))
    pr = R.make_probes(cd, "pre", dtype)            # ("pre": with a probe on the cell-0 gates; xw0 is no leaf here)
    p = lsa_params(lv)
    lmask = torch.arange(T)[None, :] < cd["lens"].long()[:, None]
    masks = {k: cd[k] for k in R.MASKS}
    z = lambda n: torch.zeros(B, n, dtype=dtype)
    prod = lambda x, w, gst, xo=None: _StoredGradProduct.apply(x, w, gst, rounding, xo)
    c0, h0, c1, h1, ctx, cum = z(H), z(H), z(H), z(H), z(M), z(T)
    o = {k: [] for k in ("in0", "in1", "pj", "acts0", "acts1", "craw0", "craw1", "q_hist", "align_hist")}
    o["c0"], o["c1"], o["cum_hist"] = [c0], [c1], [cum]
    for s in range(S):
        exp0 = torch.cat([ctx, h0], dim=1)                              # expected in0 slot s, from the stages of step s - 1
        rows0 = _Replace.apply(exp0, g["in0"][s])
        x0 = rows0 + pr["in0"][s]
        gt0 = g0_in[s] + prod(x0, lv["w0f"], gs["dg0"][s], xop["in0"][s]) + pr["g0"][s]
        c0_in = _Replace.apply(c0, g["c0"][s])
        a0, cr0 = cell_saves(gt0, c0_in, H)
        m0, c0, h0 = OM.zoneout_lstm_cell(x0, c0_in, rows0[:, M:], None, None, masks["zc0"][s], masks["zh0"][s], R.RATE, True, gates=gt0)
        exp1 = torch.cat([m0, h1], dim=1)                               # expected in1 slot s
        rows1 = _Replace.apply(exp1, g["in1"][s])
        gt1 = prod(rows1, lv["w1"], gs["dg1"][s], xop["in1"][s]) + lv["b1"] + pr["g1"][s]
        c1_in = _Replace.apply(c1, g["c1"][s])
        a1, cr1 = cell_saves(gt1, c1_in, H)
        m1, c1, h1 = OM.zoneout_lstm_cell(rows1, c1_in, rows1[:, H:], None, None, masks["zc1"][s], masks["zh1"][s], R.RATE, True, gates=gt1)
        q = prod(_Replace.apply(m1, g["pj"][s][:, :H]), lv["wq"], gs["dq_hist"][s], xop["m1"][s]) + pr["q"][s]
        # the attention step from the stored query and cumulative alignment: lsa_step_probed's own product multiplies zeros, its query
        # probe carries the query
        _, align, cum_n, ctx = lsa_step_probed(p, lv["keys"], lv["values"], lmask, z(H), _Replace.apply(cum, g["cum_hist"][s]),
                                               _Replace.apply(q, g["q_hist"][s]), pr["e"][s])
        for k, v in (("in0", exp0), ("in1", exp1), ("pj", torch.cat([m1, ctx], dim=1)), ("acts0", a0), ("acts1", a1), ("craw0", cr0), ("craw1", cr1),
                     ("q_hist", q), ("align_hist", align)):
            o[k].append(v)
        cum = cum_n
        o["c0"].append(c0); o["c1"].append(c1); o["cum_hist"].append(cum)
    o["in0"].append(torch.cat([ctx, h0], dim=1))
    o["in1"].append(torch.cat([z(H), h1], dim=1))
    o = {k: torch.stack(v) for k, v in o.items()}
    n = lambda v: v.detach().double().numpy()
    out = {k: n(o[k]) for k in R.FORWARD_Q}
    if bwd:
        (o["pj"] * cd["d_pj"].to(dtype)).sum().backward()
        out.update(dg0=n(pr["g0"].grad), dg1=n(pr["g1"].grad), dq_hist=n(pr["q"].grad), de_hist=n(pr["e"].grad), d_in0=n(pr["in0"].grad))
        out["d_ctx"] = out["d_in0"][1:, :, :M].copy()
        out.update(host_grads(cd, out))
    return out


def blocks(cd, t):
    """`t` with in0 / in1 / pj cut into the judged column blocks (views)."""
    H, M = cd["H"], cd["M"]
    out = {k: v for k, v in t.items() if k not in ("in0", "in1", "pj")}
    for k, (src, cols) in BLOCKS.items():
        if src in t:
            out[k] = np.asarray(t[src])[:, :, cols(H, M)]
    return out


def context_identity_failures(cd, got):
    """The context a step's attention writes, in both of its places: bit-identical."""
    H, M = cd["H"], cd["M"]
    a, b = np.ascontiguousarray(np.asarray(got["in0"])[1:, :, :M]), np.ascontiguousarray(np.asarray(got["pj"])[:, :, H:])
    same = a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return [] if same else ["in0 / pj: the context columns of in0 slot s + 1 are not bit-identical to those of pj slot s"]


def judge(cd, form, got, quantities, packed=False, exchanged=False):
    """(rows [(quantity, e32, worst slice error, bound)], per-slice errors {quantity: array}, bounds) of `got` against this checker evaluated
    on `got` itself; quantities: from FORWARD_Q + BACKWARD_Q + HOST_Q."""
    need = ("in0", "in1", "pj", "c0", "c1", "q_hist", "cum_hist") + (("dg0", "dg1", "dq_hist") if "dg0" in got else ())
    for k in need:
        assert np.isfinite(np.asarray(got[k])[:cd["S"]]).all(), k + ": the checker reads it and it is not finite"
    ref, r32 = stagewise(cd, form, got, torch.float64, exchanged=exchanged), stagewise(cd, form, got, torch.float32, exchanged=exchanged)
    g = R.exclude_unwritten(got, ref, packed)
    rb, r32b, gb = blocks(cd, ref), blocks(cd, r32), blocks(cd, g)
    rows, errs, bounds = [], {}, {}
    for k in quantities:
        if k in R.TERM_SCALED or k in HOST_Q:
            e32, err = R.judged_err(k, r32[k], ref), R.judged_err(k, g[k], ref)
        else:
            e32, err = slice_err(r32b[k], rb[k]), slice_err(gb[k], rb[k]).reshape(rb[k].shape[:-1])        # err: [slot, row]
        errs[k], bounds[k] = err, max(MARGIN * float(e32.max()), FLOOR)
        rows.append((k, float(e32.max()), float(err.max()), bounds[k]))
    return rows, errs, bounds


def judged_sequence(cd, errs, bounds):
    """[(stage, step, worst error / bound)] in the order the stages are judged: forward steps 0 .. S-1, then the BPTT S-1 .. 0."""
    S = cd["S"]

    def worst(ks, s):
        # (d_ctx[j] = the context columns of d_in0 slot j + 1: step j + 1's)
        v = [float(np.max(errs[k][s + 1 if k in SLOT_OF_NEXT_STEP else s - 1 if k == "d_ctx" else s]) / bounds[k]) for k in ks
             if k in errs and not (k == "d_ctx" and s == 0)]
        return max(v) if v else None
    seq = [(st, s, worst(ks, s)) for s in range(S) for st, ks in FORWARD_STAGES]
    seq += [(st, s, worst(ks, s)) for s in reversed(range(S)) for st, ks in BACKWARD_STAGES]
    return [(st, s, w) for st, s, w in seq if w is not None]


# ---- the synthetic form of the CPU test: the bf16-emulated loop and BPTT in float32 on the CPU = decoder_loop_ref.unrolled_decoder with
# oracle.model.rmm's products rounded as oracle.model._BF16MatMul rounds them, plus the negative controls, each at ONE site of ONE step
class _EmulatedProduct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, fault):
        ctx.save_for_backward(x, w)
        ctx.fault = fault
        xr = bf_truncate(x) if fault == "truncate_cell1_operand" else x if fault == "query_operand_unrounded" else bf(x)
        return xr @ bf(w)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        dx = (g if ctx.fault == "dg0_product_fp32" else bf(g)) @ bf(w).t()
        if ctx.fault == "dg1_wrong_half":
            dx = torch.roll(dx, dx.shape[1] // 2, dims=1)
        return dx, x.t() @ g, None


@contextlib.contextmanager
def _emulated_rmm(fault, step):
    """oracle.model.rmm replaced by the emulated product for the duration; unrolled_decoder calls it three times a step (cell 0, cell 1,
    query), which is how a fault finds its site."""
    site = {"truncate_cell1_operand": 1, "query_operand_unrounded": 2, "dg0_product_fp32": 0, "dg1_wrong_half": 1}.get(fault)
    calls = [0]

    def rmm(x, w):
        s, k = divmod(calls[0], 3)
        calls[0] += 1
        return _EmulatedProduct.apply(x, w, fault if (s, k) == (step, site) else None)
    saved = OM.rmm
    OM.rmm = rmm
    try:
        yield
    finally:
        OM.rmm = saved


def synthetic_form(cd, form, fault=None, step=None):
    """Everything a bf16 form returns (decoder_loop_ref.QUANTITIES as arrays; histories float32), from the emulated loop in float32."""
    dtype = torch.float32
    M = cd["M"]
    lv, pr = R.leaves(cd, form, dtype), R.make_probes(cd, "pre", dtype)
    if form == "pre":
        lv["xw0"] = lv["b0"] + bf(lv["pre"]) @ bf(lv["wx0"])
    elif fault == "xw0_rounded":
        x = lv["xw0"].detach().clone()
        x[step] = bf(x[step])
        lv["xw0"] = x
    with _emulated_rmm(fault, step):
        o = R.unrolled_decoder(lv, cd["lens"], {k: cd[k] for k in R.MASKS}, R.RATE, probes=pr,
                               fault=fault if fault in ("zh0_in_cell1", "stale_cum") else None)
        (o["pj"] * cd["d_pj"]).sum().backward()
    n = lambda v: v.detach().numpy().copy()
    out = {k: n(o[k]) for k in R.FORWARD_Q}
    out.update(dg0=n(pr["g0"].grad), dg1=n(pr["g1"].grad), dq_hist=n(pr["q"].grad), de_hist=n(pr["e"].grad), d_in0=n(pr["in0"].grad))
    if fault == "dq_hist_stored_rounded":
        out["dq_hist"][step] = bf(torch.tensor(out["dq_hist"][step])).numpy()
    out["d_ctx"] = out["d_in0"][1:, :, :M].copy()
    out.update(host_grads(cd, out))
    return out
