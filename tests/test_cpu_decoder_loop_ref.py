"""Pins tests/decoder_loop_ref.py, the fp64 checker of tests/test_gpu_decoder_loop_ref.py, without a GPU: the unrolled loop on hoisted inputs is
oracle.model.decoder (outputs and every gradient), its saves are the cells' own intermediates, the probes change no value, the restated
energy lines are oracle.model.lsa_step bit for bit, the host-formed sums reproduce autograd's leaf gradients, the exact conditions hold in
the reference, and the judge fails four wrong implementations while the float32 evaluation - a correct implementation - stays inside every bound.

e32 (the worst slice error of the float32 evaluation; a quantity's bound is 8 x e32, at least 1e-6) per case and quantity, xw0 form, in units of 1e-7:
  case           in0   in1   pj    c0    c1    acts0 acts1 craw0 craw1 q     align cum   dg0   dg1   dq    de    d_in0 d_ctx dw0f  dw1   db1   dwq   d_val
  two_steps      1.0   1.2   1.0   1.1   1.5   1.1   0.7   1.2   1.4   1.9   0.7   0.8   2.1   1.3   2.9   1.0   2.3   2.3   1.1   0.9   0.6   1.6   1.2
  plain_h32      1.9   2.1   1.9   2.6   1.8   2.3   1.8   2.3   1.7   3.4   1.8   1.1   2.4   1.9   4.3   2.2   3.1   3.1   0.6   0.8   0.9   0.8   1.7
  fused_h64      1.8   6.6   1.7   4.7   3.1   6.9   2.4   4.8   3.1   3.3   1.5   1.0   3.6   2.8   5.7   3.3   3.9   3.9   0.4   0.7   1.2   0.5   2.6
  two_pass_t140  2.0   2.7   2.0   3.1   1.8   4.5   1.6   3.1   1.9   2.9   1.2   0.8   3.0   1.8   6.5   2.1   3.0   3.0   1.2   1.0   1.2   2.0   2.2
  wide_one_tile  1.8   6.9   1.4   5.8   4.2   9.3   3.8   5.7   4.4   5.4   1.1   0.8   4.8   2.3   3.5   3.2   5.6   5.6   1.2   1.7   1.3   0.8   2.1
  wide_two_tiles 2.2   6.0   2.2   6.3   3.1   7.8   3.1   6.4   3.4   6.7   2.0   1.9   6.3   2.5   10.5  3.6   8.5   8.5   0.8   0.3   1.4   0.5   2.2
  wide_full      2.9   5.4   2.9   4.8   3.3   8.5   3.1   4.6   3.3   7.2   4.1   2.9   7.7   2.4   9.0   3.7   8.4   8.4   0.4   0.2   1.1   0.4   3.3
  wide_t131      2.2   9.0   2.3   7.3   3.7   12.1  3.1   8.0   3.7   5.9   2.4   1.2   4.7   2.5   4.1   3.2   6.6   6.6   1.4   1.5   1.3   1.6   2.2
(the pre / b0 form of the WIDE cases lies within 0.6x .. 2.2x of these; dw0f, dw1 and dwq with the magnitude of the sum's terms in the scale,
decoder_loop_ref.TERM_SCALED; figures of one machine: the worst slice of a float32 evaluation depends on the CPU's summation orders.)"""
import numpy as np
import pytest
import torch

from oracle import model as OM
from tests import decoder_loop_ref as R

SMALL = ("two_steps", "plain_h32", "fused_h64")
FORMS = [(n, f) for n in R.CASES for f in (("xw0", "pre") if R.CASES[n]["widths"] == "WIDE" else ("xw0",))]


def _oracle_problem(lengths, mel_lengths, seed):
    """A small decoder problem with real prenet variables: (dims, params with gradients, memory leaf, lengths, mel, masks)."""
    d = OM.Dims(enc_lstm=3, spk=4, att=12, att_k=5, att_ch=4, prenet=6, dec_lstm=8, n_mel=5)
    g = np.random.default_rng(seed)
    values = OM.init_params(d, seed)
    for k in values:
        if k.endswith(("bias", "bias_b")):
            values[k] = g.normal(0, 0.1, values[k].shape)
    p = OM.to_torch(values, requires_grad=True)
    B, T, L = len(lengths), max(lengths), max(mel_lengths)
    S = L + 1
    memory = torch.tensor(g.normal(0, 1, (B, T, d.mem)), requires_grad=True)
    mel = torch.tensor(g.normal(0, 1, (B, L, d.n_mel)))
    keep = lambda rate, *s: torch.tensor((g.random(s) > rate).astype(np.uint8))
    masks = {"prenet_drop_%d" % i: keep(0.5, S, B, d.prenet) for i in range(d.prenet_n)}
    for l in range(2):
        masks["dec_zc_%d" % l], masks["dec_zh_%d" % l] = keep(0.1, S, B, d.dec_lstm), keep(0.1, S, B, d.dec_lstm)
    return d, p, memory, torch.tensor(lengths), mel, torch.tensor(mel_lengths), masks, g


@pytest.mark.parametrize("lengths,mel_lengths,seed", [((6, 1, 4), (3, 2, 3), 5), ((5, 5), (4, 4), 6)])
def test_unrolled_decoder_is_the_oracles_decoder(lengths, mel_lengths, seed):
    """pj rows of unrolled_decoder through the projection = oracle.model.decoder(training=True)'s linear, stop and align within 1e-12, and
    autograd through both gives the same gradient of every decoder, attention and prenet variable and of the memory; xw0 is formed in-graph
    from oracle.model.prenet, the folded kernel in-graph from the cell-0 kernel."""
    d, p, memory, tlen, mel, mlen, masks, g = _oracle_problem(lengths, mel_lengths, seed)
    B, S, H, M, Pn = len(lengths), int(mlen.max()) + 1, d.dec_lstm, d.mem, d.prenet
    out = OM.decoder(p, d, memory, tlen, mel, mlen, True, masks)
    r = {k: torch.tensor(g.normal(0, 1, tuple(v.shape))) for k, v in out.items()}
    leaves_ = [v for v in p.values() if v.requires_grad] + [memory]
    names = [k for k, v in p.items() if v.requires_grad] + ["memory"]
    ga = torch.autograd.grad(sum((out[k] * r[k]).sum() for k in out), leaves_, allow_unused=True)
    # the same through the unrolled loop
    keys, values, _ = OM.attention_memory(p, memory, tlen)
    frames = [torch.zeros(B, d.n_mel, dtype=torch.float64)] + [mel[:, t] for t in range(S - 1)]
    K0, b0 = p[OM.P_CELL % 0 + "kernel"], p[OM.P_CELL % 0 + "bias"]
    pre = torch.stack([OM.prenet(p, d, frames[s], masks, s) for s in range(S)])
    lv = dict(xw0=pre @ K0[:Pn] + b0, w0f=torch.cat([K0[Pn:Pn + M] + K0[Pn + M:Pn + 2 * M], K0[Pn + 2 * M:]]), w1=p[OM.P_CELL % 1 + "kernel"],
              b1=p[OM.P_CELL % 1 + "bias"], wq=p[OM.P_LSA + "query_layer/kernel"], keys=keys, values=values)
    for k, path in R.LSA_PATHS.items():
        lv[k] = p[OM.P_LSA + path]
    zm = dict(zc0=masks["dec_zc_0"], zh0=masks["dec_zh_0"], zc1=masks["dec_zc_1"], zh1=masks["dec_zh_1"])
    o = R.unrolled_decoder(lv, tlen, zm, d.zoneout, probes=None)
    proj = o["pj"] @ p["decoder/decoder/linear_projection/dense/kernel"] + p["decoder/decoder/linear_projection/dense/bias"]
    mine = {"linear": proj[:, :, :d.n_mel].transpose(0, 1), "stop": proj[:, :, d.n_mel].transpose(0, 1), "align": o["align_hist"].permute(1, 2, 0)}
    for k in out:
        assert mine[k].shape == out[k].shape
        assert float((mine[k] - out[k]).detach().abs().max()) <= 1e-12 * float(out[k].detach().abs().max()), k
    gb = torch.autograd.grad(sum((mine[k] * r[k]).sum() for k in out), leaves_, allow_unused=True)
    seen = 0
    for n, a, b in zip(names, ga, gb):
        assert (a is None) == (b is None), n
        if a is not None:
            seen += 1
            assert float((a - b).abs().max()) <= 1e-12 * max(float(a.abs().max()), 1e-30), n
    # every prenet, cell, attention and projection variable, the memory layer and the memory took part
    want = [k for k in p if k.startswith(("decoder/decoder/", "attention/"))] + ["memory"]
    assert all(ga[names.index(k)] is not None and float(ga[names.index(k)].abs().max()) > 0 for k in want) and seen >= len(want)
    assert int(tlen.min()) == 1 or len(set(lengths)) == 1


def test_restated_energy_lines_are_lsa_step_bit_for_bit():
    for name in SMALL:
        cd = R.case_data(name)
        lv = {k: cd[k].double() for k in ("wq", "keys", "values") + R.LSA_NAMES}
        B, T, H = cd["B"], cd["Te"], cd["H"]
        g = torch.Generator().manual_seed(1)
        m1 = torch.randn(B, H, generator=g, dtype=torch.float64)
        cum = torch.rand(B, T, generator=g, dtype=torch.float64) * torch.tensor(R.live_mask(cd))
        lmask = torch.tensor(R.live_mask(cd))
        p = R.lsa_params(lv)
        a, c, x = OM.lsa_step(p, None, lv["keys"], lv["values"], lmask, m1, cum)
        q2, a2, c2, x2 = R.lsa_step_probed(p, lv["keys"], lv["values"], lmask, m1, cum, torch.zeros(B, R.A, dtype=torch.float64), torch.zeros(B, T, dtype=torch.float64))
        assert torch.equal(a, a2) and torch.equal(c, c2) and torch.equal(x, x2) and torch.equal(q2, m1 @ lv["wq"])


@pytest.mark.parametrize("name", SMALL)
def test_probes_change_no_value_and_saves_are_the_cells(name):
    """The probed evaluation (the reference) equals the loop around oracle.model.lsa_step itself bit for bit; acts / craw are the cells' own
    intermediates: the cell outputs and next states follow from them by the cell's last two lines."""
    cd = R.case_data(name)
    ref, _, _ = R.reference(name, "xw0")
    lv = {k: cd[k].double() for k in ("xw0", "w0f", "w1", "b1", "wq", "keys", "values") + R.LSA_NAMES}
    o = R.unrolled_decoder(lv, cd["lens"], {k: cd[k] for k in R.MASKS}, R.RATE, probes=None)
    for k in R.FORWARD_Q:
        assert np.array_equal(o[k].numpy(), ref[k]), k
    S, H, M = cd["S"], cd["H"], cd["M"]
    for cell, out_of in (("0", ref["in1"][:S, :, :H]), ("1", ref["pj"][:, :, :H])):
        acts, craw, c = ref["acts" + cell], ref["craw" + cell], ref["c" + cell]
        m = acts[:, :, 3 * H:] * np.tanh(craw)
        assert np.abs(m - out_of).max() < 1e-14
        kc = (1 - R.RATE) * cd["zc" + cell].double().numpy()
        kh = (1 - R.RATE) * cd["zh" + cell].double().numpy()
        assert np.abs(kc * (craw - c[:-1]) + c[:-1] - c[1:]).max() < 1e-14
        h = ref["in0"][:, :, M:] if cell == "0" else ref["in1"][:, :, H:]
        assert np.abs(kh * (m - h[:-1]) + h[:-1] - h[1:]).max() < 1e-14
    assert np.array_equal(ref["pj"][:, :, H:], ref["in0"][1:, :, :M])                                   # the context, in both of its places
    assert np.abs(ref["cum_hist"][1:] - ref["cum_hist"][:-1] - ref["align_hist"]).max() < 1e-15
    assert np.abs(ref["q_hist"] - ref["pj"][:, :, :H] @ cd["wq"].double().numpy()).max() < 1e-13      # the query is taken from m1


@pytest.mark.parametrize("name,form", FORMS)
def test_host_sums_reproduce_autograd_and_float32_stays_inside_every_bound(name, form):
    cd = R.case_data(name)
    ref, e32, bound = R.reference(name, form)
    got = R.host_grads(cd, ref)
    for k in R.HOST_Q:
        assert np.abs(got[k] - ref[k]).max() <= 1e-12 * np.abs(ref[k]).max(), k
        assert R.slice_err(got[k], ref[k]).max() < 1e-11, k
    assert np.abs(ref["d_in0"] - ref["dg0"] @ cd["w0f"].double().numpy().T).max() < 1e-12              # the gradient through cell 0 only
    for k in R.QUANTITIES:
        assert np.isfinite(e32[k]) and 1e-9 < e32[k] < 2e-5, (k, e32[k])                               # neither collapses to the floor nor admits anything
        assert bound[k] == max(R.MARGIN * e32[k], R.FLOOR) and e32[k] <= bound[k] < 2e-4
    assert R.exact_failures(cd, ref) == []
    r32 = R.evaluations(name, form)[1]
    assert R.exact_failures(cd, r32) == []                                                              # ... and a float32 implementation can meet them
    assert all(err <= b for _, _, err, b in R.judge(name, form, r32, R.QUANTITIES))
    if cd["B"] > 1:
        dead = ~R.live_mask(cd)
        assert dead[1, 1:].all() and not dead[0].any() and not ref["de_hist"][:, 1].any() and not ref["dq_hist"][:, 1].any()      # row 1: d_e = 0


@pytest.mark.parametrize("name", ["plain_h32", "fused_h64"])
def test_the_judge_fails_wrong_implementations(name):
    cd = R.case_data(name)
    ref, e32, bound = R.reference(name, "xw0")
    over = lambda got, qs: {k for k, _, err, b in R.judge(name, "xw0", got, qs) if not err <= b}
    # cell 1 given cell 0's zoneout mask
    bad = over(R.evaluate(cd, "xw0", torch.float64, fault="zh0_in_cell1"), R.QUANTITIES)
    assert {"in1", "c1", "pj", "dg1", "dw1"} <= bad, bad
    # the cumulative alignment carried from the wrong slot
    bad = over(R.evaluate(cd, "xw0", torch.float64, fault="stale_cum"), R.QUANTITIES)
    assert {"cum_hist", "align_hist", "pj", "de_hist"} <= bad, bad
    # the d_in0[s + 1] context term dropped from d_values
    got = dict(ref)
    got["d_ctx"] = np.zeros_like(ref["d_ctx"])
    got.update(R.host_grads(cd, got))
    assert over(got, R.HOST_Q) == {"d_values"}
    # one (step, row) slice of dg1 off by 1e-4
    got = dict(ref)
    got["dg1"] = ref["dg1"].copy()
    got["dg1"][cd["S"] - 2, cd["B"] - 1] *= 1 + 1e-4
    assert over(got, R.FORWARD_Q + R.BACKWARD_Q) == {"dg1"}
    assert not over(ref, R.QUANTITIES)


def test_exact_conditions_are_noticed():
    cd = R.case_data("plain_h32")
    ref, _, _ = R.reference("plain_h32", "xw0")
    b, t = np.argwhere(~R.live_mask(cd))[0]
    for k, idx in (("align_hist", (1, b, t)), ("de_hist", (0, b, t)), ("cum_hist", (2, b, t)), ("in0", (0, 0, 3)), ("c1", (0, 1, 0)),
                   ("in1", (0, 0, cd["H"] + 1))):
        got = {k: ref[k].copy()}
        got[k][idx] = 1e-30
        assert len(R.exact_failures(cd, got)) == 1, k
    got = {"in1": ref["in1"].copy()}
    got["in1"][0, 0, 0] = 1.0                      # (the m0 half of slot 0 is cell 0's output, not a zero)
    assert R.exact_failures(cd, got) == []
    # the excluded slots are the two named in decoder_loop_ref.exclude_unwritten, and nothing else is replaced
    nan = {k: np.full_like(ref[k], np.nan) for k in ("in1", "c0", "c1")}
    ex = R.exclude_unwritten(nan, ref, packed=True)
    assert np.isfinite(ex["in1"]).sum() == cd["B"] * cd["H"] and np.isfinite(ex["c0"]).sum() == cd["B"] * cd["H"] == np.isfinite(ex["c1"]).sum()
    assert np.isfinite(R.exclude_unwritten(nan, ref, packed=False)["c0"]).sum() == 0
