"""fp64 checker of the sequence-LSTM drivers (tests/test_gpu_lstm_seq_ref.py; pinned without a GPU by tests/test_cpu_lstm_seq_ref.py).

The reference is oracle.model.run_lstm - tf.nn.dynamic_rnn over the zoneout cell with lengths, reversed direction, residual wrapper and
masks in processing order - in float64, differentiated by torch.autograd.  The drivers take the HOISTED input product xw = x . Wx + bias, so
the leaves are chosen to let it enter exactly: cin = 4H, kernel [I ; Wh], bias 0 make gates = xw + h . Wh with xw the leaf.  The residual
wrapper needs cin == H: there a real Wx / bias are the leaves and the driver gets xw formed in fp64 and rounded once.

Three things run_lstm does not return come from `unrolled`, the same loop written out around oracle.model.zoneout_lstm_cell (same masking,
same gather): the state histories, the BPTT saves (acts, c_raw) and the per-step gate gradients.  test_cpu_lstm_seq_ref.py holds it to
run_lstm bit for bit and its two save lines to the cell's own outputs.

Judging: every (row, step) slice of a quantity on its own scale, scale = max|ref slice| + 1e-3 max|ref|; the bound of a quantity is MARGIN
times the error of THE SAME oracle function evaluated in float32 on the CPU (e32), never less than FLOOR."""
import functools

import numpy as np
import torch

from oracle import model as OM

RATE = 0.1
# Bound = MARGIN x e32 (the float32 evaluation of the reference, same normalisation), at least FLOOR.  The factor covers what the kernels do
# differently from a plain fp32 evaluation: the recurrent product summed slab by slab (K- / N-splits, MFMA accumulation order) and
# activations through v_exp_f32 / v_rcp_f32, each a few ulps.  Measured on an MI355X over all cases, forms and quantities: e32 between 0.5e-7
# and 1.6e-6 (1.3e-7 .. 4.9e-7 outside the residual case), the kernels' worst slice error between 0.6e-7 and 7.6e-7, at most 3.0 x the e32 of
# the same quantity and direction and at most 0.38 of its bound; the full table is in the docstring of tests/test_gpu_lstm_seq_ref.py.
MARGIN = 8.0
FLOOR = 1e-6
SLICE_EPS = 1e-3

# B, T, H; layout "bilstm": both directions into one [B, T, 2H] buffer at column direction * H (pair forms apply); "single": every direction
# a sequence of its own through the single-sequence entry points.  lens "short": every row but row 0 is shorter than T - 1 (the state
# gradient crosses several dead steps); "mixed": anything in 1..T; None: lengths = NULL.  Row 0 always has length T, row 1 length 1.
CASES = {
    "single_step": dict(B=1, T=1, H=64, layout="bilstm", dirs=(0, 1), lens="mixed", training=True, residual=False),
    "fused_h64": dict(B=5, T=9, H=64, layout="bilstm", dirs=(0, 1), lens="short", training=True, residual=False),
    "unfused_h24": dict(B=7, T=5, H=24, layout="bilstm", dirs=(0, 1), lens="mixed", training=True, residual=False),
    "pair_h256": dict(B=32, T=12, H=256, layout="bilstm", dirs=(0, 1), lens="mixed", training=True, residual=False),
    "groups_h256": dict(B=33, T=6, H=256, layout="single", dirs=(0, 1), lens="short", training=True, residual=False),
    "residual_h256": dict(B=7, T=5, H=256, layout="single", dirs=(0, 1), lens="mixed", training=True, residual=True),
    "inference_h64": dict(B=5, T=9, H=64, layout="bilstm", dirs=(0, 1), lens="mixed", training=False, residual=False),
    "no_lengths_h64": dict(B=5, T=9, H=64, layout="single", dirs=(0,), lens=None, training=True, residual=False),
}
FORWARD_Q = ("out", "c_hist", "h_hist", "acts", "c_raw")
BACKWARD_Q = ("dgs", "dgp", "dwh", "db")
RESIDUAL_Q = ("dx", "dwx")


def quantities(cd):
    return FORWARD_Q + BACKWARD_Q + (RESIDUAL_Q if cd["residual"] else ())


def make_lengths(kind, B, T, g):
    if kind is None:
        return None
    lens = g.integers(1, max(2, T - 1), B) if kind == "short" else g.integers(1, T + 1, B)
    lens[0] = T
    if B > 1:
        lens[1] = 1
    return torch.tensor(lens.astype(np.int32))


@functools.lru_cache(maxsize=None)
def case_data(name):
    """The inputs of a case as float32 / uint8 / int32 CPU tensors (what is uploaded); per-direction entries are dicts keyed by direction."""
    cd = dict(CASES[name], name=name)
    B, T, H = cd["B"], cd["T"], cd["H"]
    g = np.random.default_rng(sorted(CASES).index(name) + 11)
    f32 = lambda a: torch.tensor(np.asarray(a, np.float32))
    cd["lens"] = make_lengths(cd["lens"], B, T, g)
    for k in ("wh", "xw", "zc", "zh", "dout", "x", "wx", "bias"):
        cd[k] = {}
    for d in cd["dirs"]:
        cd["wh"][d] = f32(g.normal(0, 1.0 / np.sqrt(H), (H, 4 * H)))
        cd["zc"][d] = torch.tensor((g.random((T, B, H)) > RATE).astype(np.uint8)) if cd["training"] else None
        cd["zh"][d] = torch.tensor((g.random((T, B, H)) > RATE).astype(np.uint8)) if cd["training"] else None
        cd["dout"][d] = f32(g.normal(0, 0.5, (B, T, H)))
        if cd["residual"]:
            cd["x"][d], cd["wx"][d], cd["bias"][d] = f32(g.normal(0, 1, (B, T, H))), f32(g.normal(0, 1.0 / np.sqrt(H), (H, 4 * H))), f32(g.normal(0, 0.3, 4 * H))
            cd["xw"][d] = (cd["x"][d].double() @ cd["wx"][d].double() + cd["bias"][d].double()).float()      # hoisted in fp64, rounded once
        else:
            cd["xw"][d] = f32(g.normal(0, 0.8, (B, T, 4 * H)))
    return cd


def live_mask(cd):
    """[B, T] bool: position (= step) t of row b lies inside the row's length."""
    B, T = cd["B"], cd["T"]
    lens = torch.full((B,), T, dtype=torch.long) if cd["lens"] is None else cd["lens"].long()
    return (torch.arange(T)[None, :] < lens[:, None]).numpy()


def positions(cd, d):
    """[B, T] int: the position step t of row b reads and writes (reversed direction: len - 1 - t while the row is live)."""
    B, T = cd["B"], cd["T"]
    ar = np.broadcast_to(np.arange(T)[None, :], (B, T))
    if not d:
        return ar.copy()
    lens = cd["lens"].numpy().astype(np.int64)[:, None]
    return np.where(ar < lens, lens - 1 - ar, ar)


def leaves(cd, d, dtype):
    """(x, kernel, bias, leaves) for run_lstm / unrolled: [I ; Wh] with xw as the input, or a real [Wx ; Wh] in the residual case."""
    H = cd["H"]
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_()      # never the cached tensor itself
    lv = {"wh": leaf(cd["wh"][d])}
    if cd["residual"]:
        lv["x"], lv["wx"], lv["bias"] = (leaf(cd[k][d]) for k in ("x", "wx", "bias"))
        return lv["x"], torch.cat([lv["wx"], lv["wh"]]), lv["bias"], lv
    lv["xw"] = leaf(cd["xw"][d])
    lv["bias"] = torch.zeros(4 * H, dtype=dtype, requires_grad=True)
    return lv["xw"], torch.cat([torch.eye(4 * H, dtype=dtype), lv["wh"]]), lv["bias"], lv


def unrolled(x, lengths, kernel, bias, H, zc, zh, rate, training, reverse=False, residual=False, states=None):
    """run_lstm's loop around oracle.model.zoneout_lstm_cell, keeping what run_lstm drops: state histories [T + 1, B, H], the gate
    pre-activations of every step (graph nodes with retained gradients) and the BPTT saves the drivers store - acts = the four gate
    activations (0 on dead rows), c_raw = the cell value before zoneout (the carried state on dead rows).  states: optional list that receives
    the (c, h) graph nodes after every step, gradients retained."""
    B, T, _ = x.shape
    c = x.new_zeros(B, H)
    h = x.new_zeros(B, H)
    lengths = torch.full((B,), T, dtype=torch.long) if lengths is None else lengths.long()
    ar = torch.arange(T)
    if reverse:
        idx = torch.where(ar[None, :] < lengths[:, None], lengths[:, None] - 1 - ar[None, :], ar[None, :])
        x = torch.gather(x, 1, idx[:, :, None].expand(-1, -1, x.shape[2]))
    outs, cs, hs, gates, acts, craw = [], [c], [h], [], [], []
    for t in range(T):
        g = torch.cat([x[:, t], h], dim=1) @ kernel + bias
        if g.requires_grad:
            g.retain_grad()
        m, c2, h2 = OM.zoneout_lstm_cell(x[:, t], c, h, kernel, bias, None if zc is None else zc[t], None if zh is None else zh[t], rate, training, gates=g)
        i, j, f, o = g.chunk(4, dim=1)
        a = torch.cat([torch.sigmoid(i), torch.tanh(j), torch.sigmoid(f + 1.0), torch.sigmoid(o)], dim=1)
        cr = a[:, 2 * H:3 * H] * c + a[:, :H] * a[:, H:2 * H]
        if residual:
            m = m + x[:, t]
        live = (t < lengths)[:, None]
        acts.append(torch.where(live, a, torch.zeros_like(a)))
        craw.append(torch.where(live, cr, c))
        outs.append(torch.where(live, m, torch.zeros_like(m)))
        c = torch.where(live, c2, c)
        h = torch.where(live, h2, h)
        cs.append(c); hs.append(h); gates.append(g)
        if states is not None:
            c.retain_grad(); h.retain_grad()
            states.append((c, h))
    y = torch.stack(outs, dim=1)
    if reverse:
        y = torch.gather(y, 1, idx[:, :, None].expand(-1, -1, H))
    return y, torch.stack(cs), torch.stack(hs), gates, torch.stack(acts), torch.stack(craw)


def scatter_steps(cd, d, dgs):
    """Per-step gate gradients [T, B, 4H] -> position order [B, T, 4H] (live steps at their position, everything else 0)."""
    B, T = cd["B"], cd["T"]
    pos, live = positions(cd, d), live_mask(cd)
    dgp = np.zeros((B, T, dgs.shape[2]), dgs.dtype)
    for b in range(B):
        for t in range(T):
            if live[b, t]:
                dgp[b, pos[b, t]] = dgs[t, b]
    return dgp


def host_grads(cd, d, h_hist, dgs, dgp):
    """What the drivers' caller forms from their outputs, here in fp64 on the host (no GEMM kernel): dWh = sum_t h_hist[t]^T . dgates_step[t],
    the bias gradient = column sum of dgates_pos and, in the residual case, dWx = sum x^T . dgates_pos and d_x = dgates_pos . Wx^T + d_out on
    live positions.  h_hist: [T + 1, B, H] (slot 0 = the zero state) or its slots 0 .. T - 1."""
    T = cd["T"]
    h_hist, dgs, dgp = (np.asarray(a, np.float64) for a in (h_hist, dgs, dgp))
    o = {"dwh": np.einsum("tbk,tbg->kg", h_hist[:T], dgs), "db": dgp.sum((0, 1))[None, :]}
    if cd["residual"]:
        x, wx, dout = (cd[k][d].double().numpy() for k in ("x", "wx", "dout"))
        o["dwx"] = np.einsum("btk,btg->kg", x, dgp)
        o["dx"] = dgp @ wx.T + dout * live_mask(cd)[:, :, None]
    return o


def _n(t):
    return t.detach().double().numpy()


def evaluate(cd, d, dtype):
    """Every compared quantity of direction d from the oracle in `dtype`, as float64 arrays.  out and the parameter / input gradients are
    run_lstm's and its autograd's; histories, saves and per-step gate gradients are `unrolled`'s."""
    H, lens, zc, zh, tr, res = cd["H"], cd["lens"], cd["zc"][d], cd["zh"][d], cd["training"], cd["residual"]
    dout = cd["dout"][d].to(dtype)
    x, kernel, bias, lv = leaves(cd, d, dtype)
    y = OM.run_lstm(x, lens, kernel, bias, H, zc, zh, RATE, tr, reverse=bool(d), residual=res)
    (y * dout).sum().backward()
    q = {"out": _n(y), "dwh": _n(lv["wh"].grad), "db": _n(lv["bias"].grad)[None, :]}
    x2, kernel2, bias2, _ = leaves(cd, d, dtype)
    y2, cs, hs, gates, acts, craw = unrolled(x2, lens, kernel2, bias2, H, zc, zh, RATE, tr, reverse=bool(d), residual=res)
    (y2 * dout).sum().backward()
    q["c_hist"], q["h_hist"], q["acts"], q["c_raw"] = _n(cs[1:]), _n(hs[1:]), _n(acts), _n(craw)
    q["dgs"] = np.stack([_n(g.grad) if g.grad is not None else np.zeros(tuple(g.shape)) for g in gates])
    if res:
        q["dgp"] = scatter_steps(cd, d, q["dgs"])           # run_lstm has no xw to differentiate by here; d_x and dWx below are its own
        q["dx"], q["dwx"] = _n(lv["x"].grad), _n(lv["wx"].grad)
    else:
        q["dgp"] = _n(lv["xw"].grad)
    q["_unrolled_out"], q["_h0"] = _n(y2), _n(hs)
    return q


@functools.lru_cache(maxsize=None)
def reference(name, d):
    """(fp64 quantities, e32 per quantity, bound per quantity) of direction d of a case; computed once per process, never modified."""
    cd = case_data(name)
    ref, r32 = evaluate(cd, d, torch.float64), evaluate(cd, d, torch.float32)
    for v in ref.values():
        v.setflags(write=False)
    e32 = {k: float(slice_err(r32[k], ref[k]).max()) for k in quantities(cd)}
    bound = {k: max(MARGIN * e32[k], FLOOR) for k in e32}
    return ref, e32, bound


def slice_err(got, ref):
    """Error of every slice (all leading indices; the last axis is the slice) on the slice's own scale.  A reference that is identically 0
    (dWh of a single step: the state before it is 0) admits only exact zeros."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    g2, r2 = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    top = np.abs(r2).max()
    if top == 0.0:
        return np.where(np.abs(g2).max(1) == 0.0, 0.0, np.inf)
    err = np.abs(g2 - r2).max(1) / (np.abs(r2).max(1) + SLICE_EPS * top)
    return np.where(np.isfinite(g2).all(1), err, np.inf)


def dead_is_zero(cd, d, out=None, dgs=None, dgp=None):
    """Names of the tensors that break 'exactly 0 past a row's length': out / dgates_pos by position, dgates_step by step."""
    dead = ~live_mask(cd)
    bad = []
    if out is not None and np.any(np.asarray(out)[dead] != 0.0):
        bad.append("out")
    if dgp is not None and np.any(np.asarray(dgp)[dead] != 0.0):
        bad.append("dgp")
    if dgs is not None and np.any(np.asarray(dgs)[dead.T] != 0.0):
        bad.append("dgs")
    return bad
