"""fp64 restatement of the location-sensitive attention step, of S chained steps with their gradients, and of the four sums of the
post-loop parameter-gradient kernel (csrc/lsa.hip).  Plain NumPy / torch fp64, no GPU: tests/test_cpu_lsa_ref.py pins it against
oracle.model.lsa_step and against itself (autograd vs the explicit sums); tests/test_gpu_lsa_bwd_ops.py uses it as the checker.

Shapes: keys [B,T,A], values [B,T,M], q [B,A] (the query AFTER the query layer), cum [B,T]; A = 128 units, CH = 32 conv channels, the
filter-transpose operand h is padded to HLD = 32 taps."""
import numpy as np
import torch

A, CH, HLD, HQ = 128, 32, 32, 40
VARS = ("query_k", "conv_k", "conv_b", "dense_k", "score_w", "score_b")      # the six attention variables


def problem(B, T, M, KS, S=1, parts=0, seed=3, lengths="ragged", short_row=False, scale=1.0):
    """Inputs in the distribution of test_lsa_step_fwd_bwd (weights 0.2 / 0.3 / 0.5, unit keys and values, zero past a row's length), for
    S steps: a query-layer input and an upstream context gradient (d_ctx plus `parts` slabs) per step, and the cumulative alignment the
    first step starts from.  lengths: "ragged" (row 0 full, the others in [T/2, T]), None (no mask) or an array; short_row gives the
    LAST row length 1 (B >= 2).  scale multiplies the upstream gradients."""
    g = np.random.default_rng(seed)
    p = {"query_k": g.normal(0, 0.2, (HQ, A)), "conv_k": g.normal(0, 0.3, (KS, 1, CH)), "conv_b": g.normal(0, 0.1, (CH,)),
         "dense_k": g.normal(0, 0.3, (CH, A)), "score_w": g.normal(0, 0.5, (A,)), "score_b": g.normal(0, 0.1, (A,))}
    ragged = np.array([T] + list(g.integers(max(1, T // 2), T + 1, B - 1)), np.int32)
    if lengths is None:
        lens = None
    elif isinstance(lengths, str):
        lens = ragged
        if short_row and B >= 2:
            lens[-1] = 1
    else:
        lens = np.asarray(lengths, np.int32)
    mask = np.ones((B, T), bool) if lens is None else np.arange(T)[None, :] < lens[:, None]
    return dict(B=B, T=T, M=M, KS=KS, S=S, parts=parts, p=p, lengths=lens, mask=mask,
                keys=g.normal(0, 1, (B, T, A)) * mask[:, :, None], values=g.normal(0, 1, (B, T, M)) * mask[:, :, None],
                query_in=g.normal(0, 1, (S, B, HQ)), cum0=np.abs(g.normal(0, 0.5, (B, T))) * mask,
                d_ctx=scale * g.normal(0, 1, (S, B, M)), slabs=scale * g.normal(0, 1, (S, parts, B, M)))


def _windows(cum, KS):
    """win[b, t, j] = cum[b, t + j - pad] (0 outside the sequence), pad = (KS - 1) // 2: the 'same' padding of the location conv."""
    pad = (KS - 1) // 2
    fn = torch.nn.functional.pad if isinstance(cum, torch.Tensor) else None
    if fn is not None:
        return fn(cum, (pad, KS - 1 - pad)).unfold(1, KS, 1)
    xp = np.pad(cum, ((0, 0), (pad, KS - 1 - pad)))
    return np.lib.stride_tricks.sliding_window_view(xp, KS, axis=1)


def step(p, keys, values, mask, q, cum):
    """One attention step (oracle/model.py lsa_step behind the query layer) with its intermediates: the location features go through the conv
    (KS taps, 1 -> CH, + bias) and the bias-free dense layer CH -> A; pre = keys + q + loc + score_b; u = tanh(pre); energy = u . score_w,
    -inf past the row's length; align = softmax; cum_next = cum + align; ctx = align . values.  torch fp64 in, dict of tensors out."""
    KS = p["conv_k"].shape[0]
    f = _windows(cum, KS) @ p["conv_k"][:, 0, :] + p["conv_b"]            # [B,T,CH]
    loc = f @ p["dense_k"]                                              # [B,T,A]
    pre = keys + q[:, None, :] + loc + p["score_b"]
    u = torch.tanh(pre)
    energy = (u * p["score_w"]).sum(dim=2)
    masked = torch.where(mask, energy, torch.full_like(energy, -float("inf")))
    align = torch.softmax(masked, dim=1)
    ctx = (align[:, :, None] * values).sum(dim=1)
    return dict(pre=pre, u=u, energy=energy, align=align, cum_next=cum + align, ctx=ctx)


def fold_h(G_next, h_next, KS):
    """G[b, t] = G_next[b, t] + sum_j h_next[b, t + pad - j, j]: the transpose of the location filter applied to the next step's h."""
    B, T = G_next.shape
    pad = (KS - 1) // 2
    G = np.array(G_next, np.float64)
    for j in range(KS):
        lo, hi = max(0, j - pad), min(T, T + j - pad)              # t with 0 <= t + pad - j < T
        if lo < hi:
            G[:, lo:hi] += h_next[:, lo + pad - j:hi + pad - j, j]
    return G


def upstream(B, T, seed=11):
    """The upstream gradients of the one-step cases: G_next [B,T] and the next step's filter-transpose operand h_next [B,T,32]."""
    g = np.random.default_rng(seed)
    return g.normal(0, 1, (B, T)), g.normal(0, 1, (B, T, HLD))


def chain(pr, drop_last_step=False, drop_last_slab=False, G_last=None):
    """S chained steps, cum_{s+1} = cum_s + align_s, query q_s = query_in[s] . query_k, objective
        sum_s ctx_s . (d_ctx[s] + sum_p slabs[s, p])   (+ cum_S . G_last when given: an upstream gradient on the last cumulative state)
    by torch fp64 autograd.  drop_last_step / drop_last_slab leave the last step / the last slab of every step out of the objective (the
    negative controls).  Returns NumPy fp64: per step q, align, cum (the step's INPUT), ctx, d_align, d_e, dq, G (= dL/d cum_{s+1}) and
    h[s, b, t, j] = sum_k g[s, b, t, k] loc_k[j, k] (g = dL/d pre; [S,B,T,32], taps >= KS zero); d_keys; `grads` of the six variables;
    the folded filter loc_k [KS,A] / loc_b [A]."""
    S, B, T, KS = pr["S"], pr["B"], pr["T"], pr["KS"]
    t64 = lambda a, rg=False: torch.tensor(np.asarray(a, np.float64), requires_grad=rg)
    p = {k: t64(v, True) for k, v in pr["p"].items()}
    keys, values, mask = t64(pr["keys"], True), t64(pr["values"]), torch.tensor(pr["mask"])
    query_in = t64(pr["query_in"])
    slabs = pr["slabs"][:, :pr["parts"] - 1] if drop_last_slab else pr["slabs"]
    d_tot = t64(pr["d_ctx"] + slabs.sum(axis=1))
    cum = t64(pr["cum0"])
    steps, obj = [], 0.0
    for s in range(S):
        q = query_in[s] @ p["query_k"]
        st = step(p, keys, values, mask, q, cum)
        st.update(q=q, cum=cum)
        for k in ("q", "pre", "energy", "align", "cum_next"):
            st[k].retain_grad()
        if not (drop_last_step and s == S - 1):
            obj = obj + (st["ctx"] * d_tot[s]).sum()
        steps.append(st)
        cum = st["cum_next"]
    if G_last is not None:
        obj = obj + (cum * t64(G_last)).sum()
    obj.backward()
    n = lambda t: t.detach().numpy()
    gr = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()
    loc_k = pr["p"]["conv_k"][:, 0, :] @ pr["p"]["dense_k"]
    out = {k: np.stack([n(st[k]) for st in steps]) for k in ("q", "align", "cum", "ctx")}
    out.update(d_align=np.stack([gr(st["align"]) for st in steps]), d_e=np.stack([gr(st["energy"]) for st in steps]),
               dq=np.stack([gr(st["q"]) for st in steps]), G=np.stack([gr(st["cum_next"]) for st in steps]))
    h = np.zeros((S, B, T, HLD))
    h[..., :KS] = np.stack([gr(st["pre"]) for st in steps]) @ loc_k.T
    out.update(h=h, d_keys=gr(keys), grads={k: gr(v) for k, v in p.items()}, loc_k=loc_k, loc_b=pr["p"]["conv_b"] @ pr["p"]["dense_k"])
    return out


def param_bwd_direct(keys, q_hist, cum_hist, de_hist, loc_k, loc_b, score_w, score_b, KS):
    """The four sums of mstts_lsa_param_bwd written out in fp64 over every (step s, row b, position t), on the arrays given (the kernel's own
    fp32 inputs, widened):  pre = keys[b,t] + q[s,b] + score_b + loc_b + sum_j cum[s,b,t+j-pad] loc_k[j] ; u = tanh(pre) ;
    g = d_e[s,b,t] w (1 - u^2) ;  d_keys[b,t] += g ; d_loc_k[j] += cum[s,b,t+j-pad] g ; d_score_w += d_e u ; d_score_b += g.
    The loops over s and b are explicit; the positions of a row are one array operation."""
    f = lambda a: np.asarray(a, np.float64)
    keys, q_hist, cum_hist, de_hist, loc_k, loc_b, score_w, score_b = map(f, (keys, q_hist, cum_hist, de_hist, loc_k, loc_b, score_w, score_b))
    S, B, T = cum_hist.shape
    d_keys, d_loc_k, d_w, d_b = np.zeros((B, T, A)), np.zeros((KS, A)), np.zeros(A), np.zeros(A)
    for s in range(S):
        win = _windows(cum_hist[s], KS)                                # [B,T,KS]
        for b in range(B):
            u = np.tanh(keys[b] + q_hist[s, b] + score_b + loc_b + win[b] @ loc_k)
            g = de_hist[s, b][:, None] * score_w * (1.0 - u * u)       # [T,A]
            d_keys[b] += g
            d_loc_k += win[b].T @ g
            d_w += de_hist[s, b] @ u
            d_b += g.sum(axis=0)
    return dict(d_keys=d_keys, d_loc_k=d_loc_k, d_score_w=d_w, d_score_b=d_b)


def unfold_location_grad(conv_k, conv_b, dense_k, d_loc_k, d_loc_b):
    """mstts_lsa_unfold_location_grad's formula in fp64: loc_k = conv_k . dense_k and loc_b = conv_b . dense_k, so
    d_conv_k = d_loc_k . dense_k^T ; d_conv_b = d_loc_b . dense_k^T ; d_dense_k = conv_k^T . d_loc_k + conv_b (x) d_loc_b."""
    ck = np.asarray(conv_k, np.float64).reshape(-1, CH)
    cb, dk = np.asarray(conv_b, np.float64), np.asarray(dense_k, np.float64)
    return dict(conv_k=d_loc_k @ dk.T, conv_b=d_loc_b @ dk.T, dense_k=ck.T @ d_loc_k + np.outer(cb, d_loc_b))


# The shapes the GPU tests run; the CPU test proves the negative controls at every one of them.
# One step, (B, T, M, KS, parts, rows): rows = "ragged" | "short" (the last row has length 1) | "nomask" (lengths = NULL).  parts = 0 is
# run on the data of parts = 1 (with d_ctx2 set the two must agree).
STEP_CASES = [(3, 37, 48, 31, 1, "short"), (3, 37, 48, 31, 0, "short"), (2, 128, 768, 31, 3, "ragged"), (2, 128, 768, 31, 8, "ragged"),
              (2, 9, 1032, 3, 3, "ragged"), (2, 520, 16, 31, 1, "ragged"), (1, 1024, 16, 31, 1, "ragged"), (3, 5, 16, 31, 1, "ragged"),
              (1, 1, 16, 1, 1, "ragged"), (3, 37, 48, 31, 3, "nomask")]
PARAM_CASES = [(32, 128, 34, 31), (3, 37, 7, 31), (2, 520, 3, 31), (5, 70, 5, 7), (1, 1, 1, 1)]   # (B, T, S, KS), at M = 16 and 3 slabs
PARAM_M, PARAM_PARTS = 16, 3
LOOP_CASE = (3, 37, 48, 31, 7, 3)                                                             # (B, T, M, KS, S, parts)


def step_problem(B, T, M, KS, parts, rows):
    """The problem of one STEP_CASES entry with its upstream gradients: (problem, G_next, h_next)."""
    pr = problem(B, T, M, KS, S=1, parts=max(parts, 1), lengths=None if rows == "nomask" else "ragged", short_row=(rows == "short"))
    return (pr,) + upstream(B, T)


def param_problem(B, T, S, KS):
    return problem(B, T, PARAM_M, KS, S=S, parts=PARAM_PARTS, short_row=True)


def loop_problem():
    B, T, M, KS, S, parts = LOOP_CASE
    return problem(B, T, M, KS, S=S, parts=parts, short_row=True)
