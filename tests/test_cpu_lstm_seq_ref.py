"""Pins tests/lstm_seq_ref.py, the fp64 checker of tests/test_gpu_lstm_seq_ref.py, without a GPU: the [I ; Wh] construction is run_lstm with
a real Wx, the unrolled loop is run_lstm, the host-side gradient sums reproduce autograd from the reference's own gate gradients, the float32
error the bounds are measured from is finite and non-zero for every quantity of every case, and the reference's gradients are exactly 0
past a row's length (so the "exactly 0" assertions of the GPU tests are satisfiable)."""
import numpy as np
import pytest
import torch

from oracle import model as OM
from tests import lstm_seq_ref as R

CASE_DIRS = [(n, d) for n in R.CASES for d in R.CASES[n]["dirs"]]


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("training", [True, False])
def test_identity_kernel_construction_is_run_lstm_with_a_real_wx(reverse, training):
    """gates = x . Wx + b + h . Wh: run_lstm on (x, [Wx ; Wh], b) and on (xw = x . Wx + b, [I ; Wh], 0) give the same outputs, the same
    dWh, and gradients that map onto each other (dWx = sum x^T . d_xw, db = column sum of d_xw, d_x = d_xw . Wx^T), in fp64."""
    B, T, H, Cin = 4, 6, 8, 5
    g = torch.Generator().manual_seed(3)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, wx, wh, b, dout = rn(B, T, Cin).requires_grad_(), rn(Cin, 4 * H).requires_grad_(), (rn(H, 4 * H) / 3).requires_grad_(), rn(4 * H).requires_grad_(), rn(B, T, H)
    lens = torch.tensor([T, 1, 3, 4])
    zc = (torch.rand(T, B, H, generator=g) > 0.3).to(torch.uint8) if training else None
    zh = (torch.rand(T, B, H, generator=g) > 0.3).to(torch.uint8) if training else None
    y = OM.run_lstm(x, lens, torch.cat([wx, wh]), b, H, zc, zh, R.RATE, training, reverse=reverse)
    (y * dout).sum().backward()
    xw = (x.detach() @ wx.detach() + b.detach()).requires_grad_()
    wh2 = wh.detach().clone().requires_grad_()
    y2 = OM.run_lstm(xw, lens, torch.cat([torch.eye(4 * H, dtype=torch.float64), wh2]), torch.zeros(4 * H, dtype=torch.float64), H, zc, zh, R.RATE, training, reverse=reverse)
    (y2 * dout).sum().backward()
    tol = 1e-12
    assert float((y - y2).detach().abs().max()) < tol
    assert float((wh.grad - wh2.grad).abs().max()) < tol
    assert float((torch.einsum("btk,btg->kg", x.detach(), xw.grad) - wx.grad).abs().max()) < tol
    assert float((xw.grad.sum((0, 1)) - b.grad).abs().max()) < tol
    assert float((xw.grad @ wx.detach().t() - x.grad).abs().max()) < tol


@pytest.mark.parametrize("name,d", CASE_DIRS)
def test_unrolled_loop_is_run_lstm_and_its_saves_are_the_cells(name, d):
    """`unrolled` = run_lstm bit for bit (outputs and every leaf gradient); acts / c_raw are the cell's own intermediates: the cell's output and
    next state follow from them by the cell's last two lines; slot T of the histories holds every row's state after its own last live step."""
    cd = R.case_data(name)
    H, T = cd["H"], cd["T"]
    ref, _, _ = R.reference(name, d)
    assert np.array_equal(ref["_unrolled_out"], ref["out"])
    x, kernel, bias, lv = R.leaves(cd, d, torch.float64)
    y, cs, hs, gates, acts, craw = R.unrolled(x, cd["lens"], kernel, bias, H, cd["zc"][d], cd["zh"][d], R.RATE, cd["training"], reverse=bool(d), residual=cd["residual"])
    (y * cd["dout"][d].double()).sum().backward()
    assert np.array_equal(lv["wh"].grad.numpy(), ref["dwh"]) and np.array_equal(lv["bias"].grad.numpy()[None], ref["db"])
    if not cd["residual"]:
        assert np.array_equal(lv["xw"].grad.numpy(), ref["dgp"])
    live, pos = R.live_mask(cd), R.positions(cd, d)
    lens = live.sum(1)
    cs, hs, acts, craw, y = (a.detach().numpy() for a in (cs, hs, acts, craw, y))
    res = cd["x"][d].double().numpy() if cd["residual"] else None
    for t in range(T):
        for b in range(cd["B"]):
            if not live[b, t]:
                assert np.array_equal(cs[t + 1, b], cs[t, b]) and np.array_equal(hs[t + 1, b], hs[t, b]) and not acts[t, b].any()
                continue
            so = acts[t, b, 3 * H:]
            m = so * np.tanh(craw[t, b])
            kc = (1 - R.RATE) * (cd["zc"][d][t, b].numpy() if cd["training"] else 1.0)
            kh = (1 - R.RATE) * (cd["zh"][d][t, b].numpy() if cd["training"] else 1.0)
            assert np.abs(m + (res[b, pos[b, t]] if cd["residual"] else 0.0) - y[b, pos[b, t]]).max() < 1e-14
            assert np.abs(kc * (craw[t, b] - cs[t, b]) + cs[t, b] - cs[t + 1, b]).max() < 1e-14
            assert np.abs(kh * (m - hs[t, b]) + hs[t, b] - hs[t + 1, b]).max() < 1e-14
    for b in range(cd["B"]):
        assert np.array_equal(cs[T, b], cs[lens[b], b]) and np.array_equal(hs[T, b], hs[lens[b], b])


@pytest.mark.parametrize("name,d", CASE_DIRS)
def test_host_sums_reproduce_autograd_from_the_references_own_gate_gradients(name, d):
    cd = R.case_data(name)
    ref, _, _ = R.reference(name, d)
    dgp = R.scatter_steps(cd, d, ref["dgs"])
    if not cd["residual"]:
        assert np.abs(dgp - ref["dgp"]).max() < 1e-12              # per-step gate gradients at their positions = autograd's d / d xw
    got = R.host_grads(cd, d, ref["_h0"], ref["dgs"], dgp)
    for k in ("dwh", "db") + (R.RESIDUAL_Q if cd["residual"] else ()):
        assert np.abs(got[k] - ref[k]).max() < 1e-12, k
        if np.abs(ref[k]).max() > 0:
            assert R.slice_err(got[k], ref[k]).max() < 1e-12, k


@pytest.mark.parametrize("name,d", CASE_DIRS)
def test_float32_error_is_finite_and_non_zero(name, d):
    """The measured base of every bound: neither 0 (the bound would collapse to the floor) nor large (it would admit anything)."""
    cd = R.case_data(name)
    ref, e32, bound = R.reference(name, d)
    for k in R.quantities(cd):
        if cd["T"] == 1 and k == "dwh":                             # h before the only step is 0: dWh is identically 0, judged as exact zeros
            assert not ref[k].any() and e32[k] == 0.0
            continue
        assert np.isfinite(e32[k]) and 1e-9 < e32[k] < 2e-5, (k, e32[k])
        assert bound[k] == max(R.MARGIN * e32[k], R.FLOOR) and bound[k] < 2e-4


@pytest.mark.parametrize("name,d", CASE_DIRS)
def test_reference_is_exactly_zero_past_the_lengths(name, d):
    cd = R.case_data(name)
    ref, _, _ = R.reference(name, d)
    assert R.dead_is_zero(cd, d, out=ref["out"], dgs=ref["dgs"], dgp=ref["dgp"]) == []
    dead = ~R.live_mask(cd)
    if cd["lens"] is not None and cd["B"] > 1:
        assert dead.any() and dead[1, 1:].all() and not dead[0].any()
        if CASES_SHORT(cd):
            assert dead[1:, cd["T"] - 2:].all()                     # the last two steps are dead for every row but row 0
    # ... and the checker notices one wrong element there
    bad = ref["dgp"].copy()
    if dead.any():
        b, t = np.argwhere(dead)[0]
        bad[b, t, 0] = 1e-30
        assert R.dead_is_zero(cd, d, dgp=bad) == ["dgp"]


@pytest.mark.parametrize("name,d", CASE_DIRS)
def test_no_state_gradient_reaches_a_dead_step(name, d):
    """The drivers take no gradient of the final state, so the gradient of the state AFTER step t is exactly 0 for every row with
    t >= len - 1: "carrying the state gradient through dead steps" carries zeros, and the d_h slabs a dead row receives (dgates of the
    later, equally dead step times Wh^T) are zeros too.  A BPTT kernel cannot be wrong there in a way any caller could observe; what dead
    steps must get right is the forward carry (histories, slot T) and the exact zeros of dgates_step / dgates_pos."""
    cd = R.case_data(name)
    x, kernel, bias, _ = R.leaves(cd, d, torch.float64)
    states = []
    y = R.unrolled(x, cd["lens"], kernel, bias, cd["H"], cd["zc"][d], cd["zh"][d], R.RATE, cd["training"], reverse=bool(d), residual=cd["residual"], states=states)[0]
    (y * cd["dout"][d].double()).sum().backward()
    live = R.live_mask(cd)
    seen_live = False
    for t, (c, h) in enumerate(states):
        last_or_dead = torch.tensor(~live[:, t + 1] if t + 1 < cd["T"] else np.ones(cd["B"], bool))
        for s in (c, h):
            g = torch.zeros_like(s) if s.grad is None else s.grad
            assert not g[last_or_dead].any()
            seen_live = seen_live or bool(g[~last_or_dead].any())
    assert seen_live or cd["T"] == 1


def CASES_SHORT(cd):
    return R.CASES[cd["name"]]["lens"] == "short"


def test_slice_error_sees_one_short_row():
    """A whole-tensor maximum hides a row whose values are small; the slice scale does not."""
    ref = np.ones((3, 4, 8))
    ref[1, 2] *= 1e-2
    got = ref.copy()
    got[1, 2, 5] *= 1.01
    assert np.abs(got - ref).max() / np.abs(ref).max() < 2e-4
    e = R.slice_err(got, ref)
    assert e.shape == (12,) and e.max() > 5e-3 and np.count_nonzero(e) == 1
    got[0, 0, 0] = np.nan
    assert np.isinf(R.slice_err(got, ref)[0])
