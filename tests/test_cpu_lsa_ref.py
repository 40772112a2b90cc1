"""Pins tests/lsa_ref.py, the fp64 checker of tests/test_gpu_lsa_bwd_ops.py, without a GPU: its step is the oracle's step, its explicit
parameter-gradient sums are its autograd gradients, and at every shape and slab count the GPU tests run, leaving the last step or the last
slab out of the objective moves every compared tensor by far more than any bound used there (so a kernel that drops one cannot pass)."""
import numpy as np
import pytest
import torch

from oracle import model as OM
from tests import lsa_ref as R
from tests.helpers import rel_err

CONTROL = 1e-2                   # 200 x the tightest bound of the GPU tests (5e-5)


@pytest.mark.parametrize("B,T,M,KS,lengths", [(3, 37, 48, 31, "ragged"), (2, 9, 16, 3, None), (4, 40, 8, 7, "ragged"), (1, 1, 4, 1, "ragged")])
def test_step_is_the_oracle_step(B, T, M, KS, lengths):
    pr = R.problem(B, T, M, KS, lengths=lengths, short_row=True)
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    p = {k: t(v) for k, v in pr["p"].items()}
    q = t(pr["query_in"][0]) @ p["query_k"]
    st = R.step(p, t(pr["keys"]), t(pr["values"]), torch.tensor(pr["mask"]), q, t(pr["cum0"]))
    L = OM.P_LSA
    po = {L + "query_layer/kernel": p["query_k"], L + "attention_convolution_dense_layer/conv1d/kernel": p["conv_k"],
          L + "attention_convolution_dense_layer/conv1d/bias": p["conv_b"], L + "attention_convolution_dense_layer/dense/kernel": p["dense_k"],
          L + "score_layer/weight_w": p["score_w"].reshape(1, 1, -1), L + "score_layer/bias_b": p["score_b"].reshape(1, 1, -1)}
    align, cum_next, ctx = OM.lsa_step(po, OM.Dims(att_k=KS, dec_lstm=R.HQ), t(pr["keys"]), t(pr["values"]), torch.tensor(pr["mask"]),
                                       t(pr["query_in"][0]), t(pr["cum0"]))
    for name, got, ref in (("align", st["align"], align), ("cum_next", st["cum_next"], cum_next), ("ctx", st["ctx"], ctx)):
        assert float((got - ref).abs().max()) < 1e-12, name
    # the intermediates are what they are named: energy = u . w with u = tanh(pre); masked positions carry no weight
    assert float((st["energy"] - (torch.tanh(st["pre"]) * p["score_w"]).sum(2)).abs().max()) < 1e-12
    assert float(st["align"][~torch.tensor(pr["mask"])].abs().sum()) == 0.0


def test_fold_h_is_the_filter_transpose():
    """fold_h against the scalar loops of test_lsa_step_fwd_bwd, window longer than the sequence included."""
    for B, T, KS in ((2, 37, 31), (3, 5, 31), (1, 1, 1), (2, 9, 3)):
        G_next, h_next = R.upstream(B, T, seed=5)
        pad = (KS - 1) // 2
        ref = G_next.copy()
        for j in range(KS):
            for t_ in range(T):
                tau = t_ + pad - j
                if 0 <= tau < T:
                    ref[:, t_] += h_next[:, tau, j]
        assert np.abs(R.fold_h(G_next, h_next, KS) - ref).max() < 1e-12


def _compared(ch, pr):
    """Every tensor the GPU tests compare, from one chain result: the per-step ones stacked, d_keys, and the variables' gradients."""
    out = {k: ch[k] for k in ("d_align", "d_e", "dq", "h", "d_keys")}
    if pr["S"] > 1:
        out["G"] = ch["G"]                     # (of one step with a given G_last it is that input alone)
    out.update(ch["grads"])
    return out


@pytest.mark.parametrize("B,T,S,KS", [(3, 37, 7, 31), (5, 70, 5, 7), (2, 40, 3, 1)])
def test_param_bwd_direct_is_the_autograd_gradient(B, T, S, KS):
    pr = R.problem(B, T, R.PARAM_M, KS, S=S, parts=R.PARAM_PARTS, short_row=True)
    ch = R.chain(pr)
    p = pr["p"]
    d = R.param_bwd_direct(pr["keys"], ch["q"], ch["cum"], ch["d_e"], ch["loc_k"], ch["loc_b"], p["score_w"], p["score_b"], KS)
    un = R.unfold_location_grad(p["conv_k"], p["conv_b"], p["dense_k"], d["d_loc_k"], d["d_score_b"])
    g = ch["grads"]
    for name, got, ref in (("d_keys", d["d_keys"], ch["d_keys"]), ("score_w", d["d_score_w"], g["score_w"]), ("score_b", d["d_score_b"], g["score_b"]),
                           ("conv_k", un["conv_k"], g["conv_k"][:, 0, :]), ("conv_b", un["conv_b"], g["conv_b"]), ("dense_k", un["dense_k"], g["dense_k"])):
        assert rel_err(got, ref) < 1e-9, (name, rel_err(got, ref))
    # the query layer's gradient closes through the per-step dq, and the cumulative state's through G and h
    assert rel_err(np.einsum("sbh,sba->ha", pr["query_in"], ch["dq"]), g["query_k"]) < 1e-9
    for s in range(S - 1):
        # G_s = dL/d cum_{s+1} = G_{s+1} + filter^T h_{s+1}
        assert rel_err(R.fold_h(ch["G"][s + 1], ch["h"][s + 1], KS), ch["G"][s]) < 1e-9


def _controls(pr, G_last, step_control, slab_control):
    full = _compared(R.chain(pr, G_last=G_last), pr)
    worst = {}
    variants = ([("last step dropped", dict(drop_last_step=True))] if step_control else []) + ([("last slab dropped", dict(drop_last_slab=True))] if slab_control else [])
    for what, kw in variants:
        other = _compared(R.chain(pr, G_last=G_last, **kw), pr)
        for name, ref in full.items():
            worst[(what, name)] = rel_err(other[name], ref)
    return worst


@pytest.mark.parametrize("B,T,S,KS", [c for c in R.PARAM_CASES if c[1] > 1])
def test_negative_controls_param_shapes(B, T, S, KS):
    """(1, 1, 1, 1) is left out by arithmetic, not by choice: the softmax over one position is the constant 1, so d_e and every gradient
    behind it are exactly zero there whatever the objective (the GPU case at that shape draws its d_e instead)."""
    worst = _controls(R.param_problem(B, T, S, KS), None, True, True)
    print(min(worst.items(), key=lambda kv: kv[1]))
    assert min(worst.values()) > CONTROL, sorted(worst.items(), key=lambda kv: kv[1])[:3]


def test_negative_controls_loop_shape():
    worst = _controls(R.loop_problem(), None, True, True)
    print(min(worst.items(), key=lambda kv: kv[1]))
    assert min(worst.values()) > CONTROL, sorted(worst.items(), key=lambda kv: kv[1])[:3]


@pytest.mark.parametrize("B,T,M,KS,parts,rows", [c for c in R.STEP_CASES if c[4] > 0])
def test_negative_controls_step_shapes(B, T, M, KS, parts, rows):
    """One step with upstream G_next / h_next: the slab control on the tensors that depend on d_ctx.  At T = 1 only d_align does (d_e = 0)."""
    pr, G_next, h_next = R.step_problem(B, T, M, KS, parts, rows)
    worst = _controls(pr, R.fold_h(G_next, h_next, KS), False, True)
    names = ("d_align",) if T == 1 else ("d_align", "d_e", "dq", "h")
    worst = {k: v for k, v in worst.items() if k[1] in names}
    print(min(worst.items(), key=lambda kv: kv[1]))
    assert len(worst) == len(names) and min(worst.values()) > CONTROL, sorted(worst.items(), key=lambda kv: kv[1])[:3]
