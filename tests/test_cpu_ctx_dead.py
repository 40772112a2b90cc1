"""The algebra behind mstts_decoder_train_bwd_desc.ctx_dead, in fp64 where it is exact (tests/decoder_loop_ref.py's chain).

memory = [encoder | speaker embedding tiled over the row's positions, zero past its length], so the last 256 context columns are the same
per-row constant at every step.  Their gradient reaches the rest of the graph only through d_alignment[t] = values[t] . d_ctx, where it adds
ONE number per row to every position inside the length, and the softmax backward a (d_a - sum a d_a) removes a constant.  Dropping those
columns of d_ctx - both the projection's share (d_pj) and the next step's cell-0 share (d_in0) - therefore changes nothing but the gradient
of the dead value columns themselves, which has no reader.

"Without" is the same chain with the dead context columns cut out of the graph where the attention step returns them (what the persistent
BPTT launch with ctx_dead = 256 computes); every other backward quantity must agree with the full chain to 1e-12 of its largest element."""
import numpy as np
import pytest
import torch

from tests import decoder_loop_ref as R

DEAD = 256
TOL = 1e-12
CASE = "wide_one_tile"          # reference widths (M = 2 x 256 + 256), B = 3 ragged rows (lengths Te, 1, anything), 4 steps


def _case():
    """case_data(CASE) with the last DEAD value columns replaced by a per-row constant masked by the row's length; keys re-formed from it."""
    cd = dict(R.case_data(CASE))
    B, T, M = cd["B"], cd["Te"], cd["M"]
    g = np.random.default_rng(2024)
    spk = g.normal(0, 1, (B, 1, DEAD))
    values = cd["values"].double().numpy().copy()
    values[:, :, M - DEAD:] = spk * R.live_mask(cd)[:, :, None]
    cd["values"] = torch.tensor(values.astype(np.float32))
    cd["keys"] = (cd["values"].double() @ R.weights(cd["widths"])["wmem"].double()).float()
    return cd


def _backward_quantities(cd, cut, monkeypatch):
    """Every backward quantity of the chain in fp64; cut: the dead context columns carry no gradient."""
    M, Ml = cd["M"], cd["M"] - DEAD
    orig = R.lsa_step_probed

    def probed(*a, **k):
        q, align, cum, ctx = orig(*a, **k)
        if cut:
            ctx = torch.cat([ctx[:, :Ml], ctx[:, Ml:].detach()], dim=1)
        return q, align, cum, ctx

    with monkeypatch.context() as mp:
        mp.setattr(R, "lsa_step_probed", probed)
        lv, pr = R.leaves(cd, "xw0", torch.float64), R.make_probes(cd, "xw0", torch.float64)
        o = R.unrolled_decoder(lv, cd["lens"], {k: cd[k] for k in R.MASKS}, R.RATE, probes=pr)
    (o["pj"] * cd["d_pj"].double()).sum().backward()
    n = lambda t: t.grad.detach().numpy().copy()
    d_in0 = n(pr["in0"])
    out = dict(de=n(pr["e"]), dq=n(pr["q"]), dg1=n(pr["g1"]), dg0=n(lv["xw0"]),
               d_in0_live=np.concatenate([d_in0[:, :, :Ml], d_in0[:, :, M:]], axis=2), d_values_live=n(lv["values"])[:, :, :Ml],
               d_keys=n(lv["keys"]))
    for k in ("w0f", "w1", "b1", "wq") + R.LSA_NAMES:
        out["d_" + k] = n(lv[k])
    out["_d_in0_dead"] = d_in0[:, :, Ml:M]
    out["_ctx_dead"] = o["pj"].detach().numpy()[:, :, cd["H"] + Ml:]
    out["_align"] = o["align_hist"].detach().numpy()
    return out


def test_dead_context_columns_cancel_in_fp64(monkeypatch):
    cd = _case()
    full, cut = _backward_quantities(cd, False, monkeypatch), _backward_quantities(cd, True, monkeypatch)
    # the premise: the dead context columns are the row's constant at every step (sum_t a[t] = 1 over the row's length) ...
    spk = cd["values"].double().numpy()[:, 0, cd["M"] - DEAD:]
    assert np.abs(full["_ctx_dead"] - spk[None]).max() < 1e-13
    # ... and the test is not vacuous: their gradient is as large as the live columns', and a step attends to more than one position
    assert np.abs(full["_d_in0_dead"][1:]).max() > 0.1 * np.abs(full["d_in0_live"][1:]).max() > 0
    assert (full["_align"][:, 0] > 1e-3).sum(-1).min() > 1
    bad = {}
    for k in full:
        if k.startswith("_"):
            continue
        scale = np.abs(full[k]).max()
        assert scale > 0, k
        e = np.abs(full[k] - cut[k]).max() / scale
        if not e <= TOL:
            bad[k] = e
    assert not bad, bad


def test_a_constant_that_is_not_masked_does_not_cancel(monkeypatch):
    """Negative control: the cancellation needs the dead columns to be CONSTANT over the positions the row attends to.  With drawn values in
    those columns (decoder_loop_ref's own case) cutting them changes the energy gradient."""
    cd = dict(R.case_data(CASE))
    full, cut = _backward_quantities(cd, False, monkeypatch), _backward_quantities(cd, True, monkeypatch)
    assert np.abs(full["de"] - cut["de"]).max() / np.abs(full["de"]).max() > 1e-3
