"""The algebra behind mstts_persist_desc.ctx_dead on the FORWARD launch, in fp64 where it is exact (oracle.model.lsa_step inside
tests/decoder_loop_ref.py's unrolled loop).

memory = [encoder | speaker embedding tiled over the row's positions, zero past its length]; energies past the length are -inf, so the
alignments of a row sum to one over its length and the last 256 context columns are spk[b] at every step.  The live-width launch therefore
forms, ships and multiplies only columns 0 .. 511 and adds the constant columns' share of the cell-0 gates, spk[b] . w0f[rows 512 .. 767], as
a per-row constant - from step 1 on: step 0 has no incoming context."""
import numpy as np
import torch

from tests import decoder_loop_ref as R

DEAD = 256
TOL = 1e-12
CASE = "wide_one_tile"          # reference widths (M = 2 x 256 + 256), B = 3 ragged rows (lengths Te, 1, anything), 4 steps


def _forward(cd):
    lv = {k: cd[k].double() for k in ("w0f", "w1", "b1", "wq", "keys", "values", "xw0") + R.LSA_NAMES}
    with torch.no_grad():
        o = R.unrolled_decoder(lv, cd["lens"], {k: cd[k] for k in R.MASKS}, R.RATE)       # probes None: the attention step is oracle.model.lsa_step itself
    return {k: v.numpy() for k, v in o.items()}


def _promised_case():
    cd = dict(R.case_data(CASE))
    B, M = cd["B"], cd["M"]
    spk = np.random.default_rng(2025).normal(0, 1, (B, 1, DEAD))
    values = cd["values"].double().numpy().copy()
    values[:, :, M - DEAD:] = spk * R.live_mask(cd)[:, :, None]
    cd["values"] = torch.tensor(values.astype(np.float32))
    cd["keys"] = (cd["values"].double() @ R.weights(cd["widths"])["wmem"].double()).float()
    return cd


def test_dead_context_columns_are_the_speaker_embedding_and_their_gate_share_is_constant():
    cd = _promised_case()
    H, M, S = cd["H"], cd["M"], cd["S"]
    Ml = M - DEAD
    lens = cd["lens"].numpy()
    assert lens.min() == 1 and lens.max() == cd["Te"] and len(set(lens)) > 1          # ragged
    o = _forward(cd)
    spk = cd["values"].double().numpy()[:, 0, Ml:]                                     # position 0 is below every length
    ctx = o["pj"][:, :, H:]                                                            # the context of steps 0 .. S-1
    assert np.abs(ctx[:, :, Ml:] - spk[None]).max() < TOL
    assert (o["align_hist"][:, 0] > 1e-3).sum(-1).min() > 1                            # (not vacuous: a step attends to more than one position)
    w0f = cd["w0f"].double().numpy()
    const = spk @ w0f[Ml:M]                                                            # [B, 4H], the same at every step
    assert np.abs(const).max() > 0.1
    for s in range(S + 1):
        full = o["in0"][s] @ w0f
        live = o["in0"][s][:, :Ml] @ w0f[:Ml] + o["in0"][s][:, M:] @ w0f[M:]
        if s == 0:                                                                     # no incoming context: nothing to add
            assert not o["in0"][0].any() and not full.any()
            continue
        assert np.abs(live + const - full).max() <= TOL * np.abs(full).max(), s
        assert np.abs(live - full).max() > 1e-2 * np.abs(full).max(), s                # (the constant is no rounding term)


def test_a_drawn_tail_is_no_constant():
    """Counter-case: with drawn values in the last 256 columns (decoder_loop_ref's own case) the context there moves with the alignments: the
    identity needs the caller's promise."""
    cd = dict(R.case_data(CASE))
    H, M = cd["H"], cd["M"]
    o = _forward(cd)
    tail = cd["values"].double().numpy()[:, 0, M - DEAD:]
    row0 = o["pj"][:, 0, H + M - DEAD:]                                                # row 0 attends to all Te positions
    assert np.abs(row0 - tail[0][None]).max() > 1e-2
    assert np.abs(row0[1] - row0[0]).max() > 1e-3                                      # ... and differs from step to step
