"""WaveGlow training direction (multi_speaker_tts_amd/waveglow_trainer.py, csrc/waveglow_train.hip) against an fp64 restatement of the
reference's Glow_Train / Glow_Loss (WaveGlow/Modules.py:135-175,329-352,373-385; Inv1x1.py:21-27) built here from the oracle's forward
pieces (oracle/waveglow.py) and differentiated with torch.autograd on the CPU."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from multi_speaker_tts_amd import lib
from multi_speaker_tts_amd import waveglow as WG
from multi_speaker_tts_amd import waveglow_trainer as WT
from oracle import train as OT
from oracle import waveglow as OW
from tests.helpers import rel_err, t2n

pytestmark = pytest.mark.gpu

CFGS = [dict(n_mel=8, flows=4, groups=8, early_every=2, early_size=2, up_k=16, up_stride=4, layers=3, ch=32, k=3),
        dict(n_mel=16, flows=12, groups=8, early_every=4, early_size=2, up_k=32, up_stride=8, layers=4, ch=64, k=3),
        dict(n_mel=8, flows=6, groups=4, early_every=3, early_size=2, up_k=8, up_stride=4, layers=8, ch=32, k=3)]
REF_WG = dict(n_mel=80, flows=12, groups=8, early_every=4, early_size=2, up_k=1024, up_stride=256, layers=8, ch=512, k=3)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _rn(dev, *shape, seed=0, scale=1.0):
    return torch.tensor(np.random.default_rng(seed).normal(0, scale, shape), dtype=torch.float32, device=dev)


# ---- the fp64 reference ---------------------------------------------------------------------------------------------------------------
def ref_losses(p, od, audio, mel):
    """Restructure_Train_Data + Glow_Train + Glow_Loss (sigma = 1) in whatever dtype p / audio / mel carry.  Returns (losses, latents)."""
    N, La = audio.shape
    G = od.groups
    L = La // G * G
    up = OW.upsample_mel(p, od, mel)
    if up.shape[1] < L:
        raise ValueError("mel too short")
    melg = up[:, :L].reshape(N, L // G, G * od.n_mel)
    a = audio[:, :L].reshape(N, L // G, G)
    outs, names, log_s_sum, logdet_sum = [], [], 0.0, 0.0
    for f in range(od.flows):
        if f % od.early_every == 0 and f > 0:
            outs.append(a[:, :, :od.early_size]); names.append("early_%d" % f)
            a = a[:, :, od.early_size:]
        pre = OW.P_WG + "affine_coupling_layer_%d/" % f
        W = p[pre + "invertible_1x1/kernel"]
        c = W.shape[0]
        logdet_sum = logdet_sum + (torch.log(torch.linalg.det(W.double() * 1e3) + 1e-6) - c * math.log(1e3)) * (N * (L // G))
        y = a @ W
        a0, a1 = y.chunk(2, dim=-1)
        ls, b = OW.wavenet(p, od, pre + "wavenet/", a0, melg)
        ls = torch.clamp(ls, max=8.0)
        log_s_sum = log_s_sum + ls.sum()
        a = torch.cat([a0, torch.exp(ls) * a1 + b], dim=-1)
    outs.append(a); names.append("z")
    z = torch.cat(outs, dim=-1)
    size = z.numel()
    out = {"Log_S_Loss": -log_s_sum / size, "Log_Det_W_Loss": -logdet_sum / size, "Audio_Loss": (z ** 2).sum() / 2 / size}
    out["Loss"] = out["Log_S_Loss"] + out["Log_Det_W_Loss"] + out["Audio_Loss"]
    return out, dict(zip(names, outs))


def ref_step(values, od, audio, mel, state=None, step=0):
    """One reference step in fp64: losses, raw gradients, clipped TF-Adam update (oracle.train.adam_tf with the clip factor)."""
    p = {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for k, v in values.items()}
    losses, _ = ref_losses(p, od, torch.tensor(audio, dtype=torch.float64), torch.tensor(mel, dtype=torch.float64))
    names = list(p)
    grads = torch.autograd.grad(losses["Loss"], [p[k] for k in names])
    grads = dict(zip(names, grads))
    gn = math.sqrt(sum(float((g ** 2).sum()) for g in grads.values()))
    scale = 0.1 / max(gn, 0.1)
    state = state or {"m": {k: torch.zeros_like(g) for k, g in grads.items()}, "v": {k: torch.zeros_like(g) for k, g in grads.items()}}
    new = {}
    lr = WT.learning_rate(step)
    for k in names:
        new[k], state["m"][k], state["v"][k] = OT.adam_tf(p[k].detach(), grads[k] * scale, state["m"][k], state["v"][k], step + 1, lr, eps=1e-8)
    return {k: float(v) for k, v in losses.items()}, {k: t2n(g) for k, g in grads.items()}, {k: t2n(v) for k, v in new.items()}, state, gn


def _values(od, seed=3, scale_out=1.0):
    """trained_like values (the reference's zero output conv would zero every WaveNet gradient at step 1) with non-zero biases and
    orthogonal 1x1 kernels (det > 0): N(0, 1) kernels grow the audio by ~sqrt(c) per flow, 1e5 over 12 flows, and the test would
    compare round-off of an exploded flow."""
    v = OW.init_params(od, seed=seed, trained_like=True)
    g = np.random.default_rng(seed + 100)
    for k in v:
        if k.endswith("invertible_1x1/kernel"):
            q, _ = np.linalg.qr(np.asarray(v[k]))
            if np.linalg.det(q) < 0:
                q[:, 0] *= -1
            v[k] = q
        if k.endswith("bias"):
            v[k] = g.normal(0, 0.05, np.shape(v[k]))
        if k.endswith("wavenet/conv1d/kernel"):
            v[k] = np.asarray(v[k]) * scale_out
    return v


def _batch(od, N, T, La, seed=8):
    g = np.random.default_rng(seed)
    return np.clip(g.normal(0, 0.3, (N, La)), -0.99, 0.99), np.clip(g.normal(0, 1.5, (N, T, od.n_mel)), -4, 4)


def _dt(a, dev):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=dev).contiguous()


# ---- kernels ---------------------------------------------------------------------------------------------------------------------------
def test_weight_norm_fwd_bwd_kernels(dev):
    """One launch over a descriptor table of mixed shapes (one written into a wider matrix at a column offset, one with a column whose
    squared sum is below 1e-5: the clamp branch) against fp64 autograd of g * v * rsqrt(max(sum v^2, 1e-5))."""
    shapes = [(3, 5, 1, 0, None), (96, 130, 3, 0, None), (40, 64, 1, 16, 100), (7, 9, 1, 0, None)]
    descs_f, descs_b, keep, ref = [], [], [], []
    for i, (rows, cols, K, col0, ldw) in enumerate(shapes):
        v = np.random.default_rng(i).normal(0, 0.5, (rows, cols))
        if i == 3:
            v[:, 2] = 1e-4                                            # sum of squares 7e-8 < 1e-5
        g = np.random.default_rng(10 + i).uniform(0.5, 1.5, cols)
        dw = np.random.default_rng(20 + i).normal(0, 1, (rows, cols))
        ld = ldw or cols
        tv, tg = _dt(v, dev), _dt(g, dev)
        tw = torch.zeros(rows, ld, device=dev)
        tdw = torch.zeros(rows, ld, device=dev); tdw[:, col0:col0 + cols] = _dt(dw, dev)
        tdv, tdg = torch.zeros(rows, cols, device=dev), torch.zeros(cols, device=dev)
        keep += [tv, tg, tw, tdw, tdv, tdg]
        for lst, wbuf in ((descs_f, tw), (descs_b, tdw)):
            q = lib.WgWnDesc()
            q.v, q.g, q.w, q.ldw, q.dv, q.dg, q.rows, q.cols = lib.ptr(tv), lib.ptr(tg), lib.ptr(wbuf, col0), ld, lib.ptr(tdv), lib.ptr(tdg), rows, cols
            lst.append(q)
        vv = torch.tensor(v, requires_grad=True); gg = torch.tensor(g, requires_grad=True)
        w = gg * vv * torch.rsqrt(torch.clamp((vv * vv).sum(0, keepdim=True), min=1e-5))
        dv, dg = torch.autograd.grad(w, [vv, gg], torch.tensor(dw))
        ref.append((t2n(w), t2n(dv), t2n(dg), tw, tdv, tdg, col0, cols))
    tabs = []
    for lst in (descs_f, descs_b):
        arr = (lib.WgWnDesc * len(lst))(*lst)
        tabs.append(torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev))
    lib.call("mstts_wg_weight_norm_fwd", lib.ptr(tabs[0]), len(shapes), 130)
    lib.call("mstts_wg_weight_norm_bwd", lib.ptr(tabs[1]), len(shapes), 130)
    torch.cuda.synchronize()
    for w, dv, dg, tw, tdv, tdg, col0, cols in ref:
        assert rel_err(t2n(tw)[:, col0:col0 + cols], w) < 1e-5
        assert rel_err(t2n(tdv), dv) < 1e-5 and rel_err(t2n(tdg), dg) < 1e-5


@pytest.mark.parametrize("C", [32, 6])
def test_gate_and_res_skip_bwd_kernels(dev, C):
    rows, lda = 37, 2 * C + 8
    a, dz = _rn(dev, rows, lda, seed=1, scale=1.5), _rn(dev, rows, C, seed=2)
    dpre, dpre2 = torch.zeros(rows, 2 * C, device=dev), torch.zeros(rows, 3 * C, device=dev)
    lib.call("mstts_wg_gate_bwd", lib.ptr(a), lda, lib.ptr(dz), lib.ptr(dpre), lib.ptr(dpre2, C // 2 * 2), 3 * C, rows, C)
    at = a.double().cpu()[:, :2 * C].clone().requires_grad_(True)
    zt = torch.tanh(at[:, :C]) * torch.sigmoid(at[:, C:])
    ref, = torch.autograd.grad(zt, [at], dz.double().cpu())
    assert rel_err(t2n(dpre), t2n(ref)) < 1e-5
    assert rel_err(t2n(dpre2)[:, C // 2 * 2:C // 2 * 2 + 2 * C], t2n(ref)) < 1e-5
    # res / skip routing: x_next = z + rs[:, :C], skip = rs[:, C:] (last layer: skip = rs)
    for last in (0, 1):
        nres = C if last else 2 * C
        dxn, dskip = _rn(dev, rows, C, seed=3), _rn(dev, rows, C, seed=4)
        drs, dzz = torch.zeros(rows, nres, device=dev), torch.full((rows, C), 7.0, device=dev)
        lib.call("mstts_wg_res_skip_bwd", None if last else lib.ptr(dxn), lib.ptr(dskip), lib.ptr(drs), lib.ptr(dzz), rows, C, last)
        z = torch.zeros(rows, C, dtype=torch.float64, requires_grad=True)
        rs = torch.zeros(rows, nres, dtype=torch.float64, requires_grad=True)
        if last:
            out = (rs * dskip.double().cpu()).sum()
        else:
            out = ((z + rs[:, :C]) * dxn.double().cpu()).sum() + (rs[:, C:] * dskip.double().cpu()).sum()
        gz, grs = torch.autograd.grad(out, [z, rs], allow_unused=True)
        assert rel_err(t2n(drs), t2n(grs)) < 1e-5
        if last:
            assert float(dzz.abs().max()) == 0.0
        else:
            assert rel_err(t2n(dzz), t2n(gz)) < 1e-5


def test_coupling_fwd_bwd_kernel(dev):
    """Affine coupling with an early chunk leaving into z, rows with log_s > 8 (clamped: no gradient) and log_s == 8 (gradient passes),
    and the log-s loss accumulation."""
    rows, c, ce, G, zcol = 300, 8, 2, 8, 2
    h = c // 2
    y = _rn(dev, rows, c, seed=1)
    lsb = _rn(dev, rows, c, seed=2, scale=2.0)
    lsb[:50, :h] = 9.0                         # clamped
    lsb[50:100, :h] = 8.0                      # tie: passes
    z = torch.zeros(rows, G, device=dev)
    nxt = torch.zeros(rows, c - ce, device=dev)
    loss = torch.zeros(4, device=dev)
    lib.call("mstts_wg_coupling_fwd", lib.ptr(y), lib.ptr(lsb), lib.ptr(nxt), lib.ptr(z), G, zcol, ce, lib.ptr(loss), rows, c)
    yt = y.double().cpu().requires_grad_(True); lt = lsb.double().cpu().requires_grad_(True)
    ls = torch.clamp(lt[:, :h], max=8.0)
    o = torch.cat([yt[:, :h], torch.exp(ls) * yt[:, h:] + lt[:, h:]], dim=-1)
    assert rel_err(t2n(z)[:, zcol:zcol + ce], t2n(o[:, :ce])) < 1e-6 and rel_err(t2n(nxt), t2n(o[:, ce:])) < 1e-6
    assert abs(float(loss[0]) - float(ls.detach().sum())) < 1e-5 * float(ls.detach().abs().sum())
    # backward: d_o = [z chunk / size | d_next]; the loss's -1/size per unclamped log_s
    inv_size = 1.0 / 977
    d_next = _rn(dev, rows, c - ce, seed=5)
    d_y, d_lsb = torch.zeros(rows, c, device=dev), torch.zeros(rows, c, device=dev)
    lib.call("mstts_wg_coupling_bwd", lib.ptr(y), lib.ptr(lsb), lib.ptr(z), G, zcol, ce, lib.ptr(d_next), inv_size, lib.ptr(d_y), lib.ptr(d_lsb), rows, c)
    zc = z.double().cpu()[:, zcol:zcol + ce]
    obj = (o[:, :ce] * zc * inv_size).sum() + (o[:, ce:] * d_next.double().cpu()).sum() - ls.sum() * inv_size
    gy, gl = torch.autograd.grad(obj, [yt, lt])
    assert rel_err(t2n(d_y), t2n(gy)) < 1e-5 and rel_err(t2n(d_lsb), t2n(gl)) < 1e-5
    assert float(d_lsb[:50, :h].abs().max()) == 0.0 and float(d_lsb[50:100, :h].abs().min()) > 0.0


def test_inv1x1_logdet_kernel(dev):
    """c in {2, 4, 6, 8}: log(det(1e3 W) + 1e-6) - c log(1e3) into the loss, grad_scale det/(det+1e-6) W^-T into the gradient; det < 0: NaN."""
    mats = []
    for i, c in enumerate((2, 4, 6, 8)):
        m = np.random.default_rng(i).normal(0, 1, (c, c))
        if np.linalg.det(m) < 0:
            m[:, 0] *= -1
        mats.append(m)
    offs, n = [], 0
    for m in mats:
        offs.append(n); n += (m.size + 3) // 4 * 4
    params, grad = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    for o, m in zip(offs, mats):
        params[o:o + m.size] = _dt(m.reshape(-1), dev)
    grad += 0.25                                                   # accumulates onto what is there
    table = torch.tensor([v for o, m in zip(offs, mats) for v in (o, m.shape[0])], dtype=torch.int64, device=dev)
    loss = torch.zeros(1, device=dev)
    lib.call("mstts_wg_inv1x1_logdet", lib.ptr(params), lib.ptr(grad), lib.ptr(table), len(mats), -0.125, lib.ptr(loss))
    ref = 0.0
    for o, m in zip(offs, mats):
        W = torch.tensor(m, requires_grad=True)
        sign, lad = torch.linalg.slogdet(W.detach() * 1e3)
        assert float(sign) > 0
        val = torch.log(torch.linalg.det(W * 1e3) + 1e-6) - m.shape[0] * math.log(1e3)
        ref += float(val)
        gW, = torch.autograd.grad(val, [W])
        assert np.allclose(t2n(gW), np.linalg.inv(m).T, rtol=1e-6, atol=1e-9)
        got = t2n(grad)[o:o + m.size].reshape(m.shape) - 0.25
        assert rel_err(got, -0.125 * t2n(gW)) < 1e-5
        assert abs(float(lad) - m.shape[0] * math.log(1e3) - float(val)) < 1e-6
    assert abs(float(loss[0]) - ref) < 1e-5 * max(1.0, abs(ref))
    neg = mats[1].copy(); neg[:, 0] *= -1                         # det < 0
    params[offs[1]:offs[1] + neg.size] = _dt(neg.reshape(-1), dev)
    loss.zero_()
    lib.call("mstts_wg_inv1x1_logdet", lib.ptr(params, offs[1]), lib.ptr(grad, offs[1]), lib.ptr(torch.tensor([0, 4], dtype=torch.int64, device=dev)), 1, -0.125, lib.ptr(loss))
    assert math.isnan(float(loss[0]))


def test_overlap_add_bwd_and_upsampler_grads(dev):
    """Tap-gradient gather + dW = dY^T mel + db = colsum against F.conv_transpose1d autograd, with L shorter than the upsampled length."""
    N, T, K, S, Cc = 2, 6, 16, 4, 8
    Lup = (T - 1) * S + K
    L = Lup - 10
    mel, w, b = _rn(dev, N, T, Cc, seed=1), _rn(dev, 1, K, Cc, Cc, seed=2, scale=0.3), _rn(dev, Cc, seed=3)
    dup = _rn(dev, N, L, Cc, seed=4)
    dY = torch.full((N * T, K * Cc), 5.0, device=dev)
    lib.call("mstts_wg_overlap_add_bwd", lib.ptr(dup), lib.ptr(dY), N, T, K, S, Cc, L)
    gw, gb = torch.zeros(K * Cc, Cc, device=dev), torch.zeros(Cc, device=dev)
    lib.gemm(dY, mel, gw, K * Cc, Cc, N * T, K * Cc, Cc, Cc, trans_a=True)
    lib.call("mstts_colsum", lib.ptr(dup), N * L, Cc, Cc, lib.ptr(gb), 0)
    wt = w.double().cpu().requires_grad_(True); bt = b.double().cpu().requires_grad_(True)
    up = F.conv_transpose1d(mel.double().cpu().transpose(1, 2), wt[0].permute(2, 1, 0), stride=S).transpose(1, 2) + bt
    out = (up[:, :L] * dup.double().cpu()).sum()
    rw, rb = torch.autograd.grad(out, [wt, bt])
    assert rel_err(t2n(gw).reshape(1, K, Cc, Cc), t2n(rw)) < 1e-5 and rel_err(t2n(gb), t2n(rb)) < 1e-5
    with pytest.raises(lib.MsttsError):
        lib.call("mstts_wg_overlap_add_bwd", lib.ptr(dup), lib.ptr(dY), N, T, K, S, Cc, Lup + 1)


@pytest.mark.parametrize("gscale", [1e-3, 10.0])
def test_adam_clip_by_global_norm(dev, gscale):
    """Gradient norms below and above 0.1: parameters, m and v against TF-Adam on clip_by_global_norm(g, 0.1) in fp64."""
    n = 1001
    p, g = _rn(dev, n, seed=1), _rn(dev, n, seed=2, scale=gscale / math.sqrt(n))
    m, v = _rn(dev, n, seed=3, scale=1e-3), _rn(dev, n, seed=4, scale=1e-3).abs()
    p0, g0, m0, v0 = (t.double().cpu() for t in (p, g, m, v))
    ss = torch.zeros(4, device=dev)
    lib.call("mstts_l2_loss_acc", lib.ptr(g), None, n, lib.ptr(ss))
    lr_t = 1e-3 * math.sqrt(1 - 0.999 ** 3) / (1 - 0.9 ** 3)
    lib.call("mstts_adam_tf_clip", lib.ptr(p), lib.ptr(g), lib.ptr(m), lib.ptr(v), lib.ptr(ss), 2.0, 0.1, lr_t, 0.9, 0.999, 1e-8, n)
    gn = float(g0.norm())
    assert (gn > 0.1) == (gscale > 1)
    gc = g0 * 0.1 / max(gn, 0.1)
    rp, rm, rv = OT.adam_tf(p0, gc, m0, v0, 3, 1e-3, eps=1e-8)
    for got, ref in ((p, rp), (m, rm), (v, rv)):
        assert np.allclose(t2n(got), t2n(ref), rtol=1e-6, atol=1e-6 * float(ref.abs().max()))


# ---- the engine --------------------------------------------------------------------------------------------------------------------------
def _compare_step(eng, w, ref_losses_, ref_grads, loss_tol, grad_tol):
    """Losses relative to themselves, floored at 0.1 (orthogonal 1x1 kernels put log det W at 0, where fp32's log(det(1e3 W) + 1e-6) - c log(1e3)
    keeps a round-off of ~1e-7 absolute, as in TF); each raw gradient relative to its own maximum.  A one-row weight-normed kernel (the initial
    conv of a flow with c = 2: w = g sign(v)) has a gradient that is zero in exact arithmetic except in clamped columns: it is held relative to
    the larger of its own and its gain's gradient."""
    got = eng.scalars(w)
    for k in ("Log_S_Loss", "Log_Det_W_Loss", "Audio_Loss", "Loss"):
        assert abs(got[k] - ref_losses_[k]) <= loss_tol * max(abs(ref_losses_[k]), 0.1), (k, got[k], ref_losses_[k])
    grads = eng.params.export(grads=True)
    bad = []
    for k in ref_grads:
        if k.endswith("/kernel") and "/wavenet/" in k and ref_grads[k].shape[:3] == (1, 1, 1):
            scale = max(np.abs(ref_grads[k]).max(), np.abs(ref_grads[k[:-len("kernel")] + "g"]).max())
            if np.abs(grads[k] - ref_grads[k]).max() > grad_tol * scale:
                bad.append((k, float(np.abs(grads[k] - ref_grads[k]).max() / scale)))
        elif rel_err(grads[k], ref_grads[k]) > grad_tol:
            bad.append((k, rel_err(grads[k], ref_grads[k])))
    assert not bad, bad[:5]
    return got


@pytest.mark.parametrize("cfg", range(len(CFGS)))
def test_waveglow_train_step_parity(dev, cfg):
    """Two steps on a few hundred rows: losses (1e-5), every raw gradient (1e-4 of its maximum), the parameters after the clipped Adam (2e-3)."""
    cfg = CFGS[cfg]
    od, pd = OW.WGDims(**cfg), WG.WGDims(**cfg)
    values = _values(od, scale_out=0.5)              # log-scales of a few tenths: fp32 round-off is not amplified through exp(log_s) x 12 flows
    N, T = 2, 100
    La = (T - 1) * od.up_stride + od.up_k - 3          # 100 .. 204 rows; cut to a multiple of G, the upsampled mel sliced to it
    audio, mel = _batch(od, N, T, La)
    eng = WT.WaveGlowTrainEngine(pd, device=dev, values=values)
    state, cur = None, values
    for step in range(2):
        rl, rg, rnew, state, gn = ref_step(cur, od, audio, mel, state, step)
        w = eng.plan(N, T, La)
        eng.forward(_dt(audio, dev), _dt(mel, dev), w)
        eng.loss_and_backward(w)
        got = _compare_step(eng, w, rl, rg, 1e-5, 1e-4)
        assert abs(got["Global_Norm"] - gn) < 1e-4 * gn
        eng.adam_step(w)
        now = eng.values()
        bad = [(k, rel_err(now[k], rnew[k])) for k in rnew if rel_err(now[k], rnew[k]) > 2e-3]
        assert not bad, bad[:5]
        cur = rnew
    with pytest.raises(ValueError):
        eng.plan(N, 2, (2 - 1) * od.up_stride + od.up_k + od.groups)          # the mel is too short for the audio


def test_waveglow_train_step_reference_width(dev):
    """One step at the reference widths (n_mel 80, 512 channels, 8 layers, upsampler 1024 / 256, G = 8) with 4 of the 12 flows (all channel
    counts of the first two early groups; keeps the fp64 autograd side on the host short) at N = 1 x 2 048 samples (256 rows).

    Tolerance: the couplings multiply last-bit differences of the 3 x 512 x 1 024 contractions through exp(log_s); the inference test at
    this width (test_glow_inference_reference_size) measures 3e-4 .. 4e-3 for ANY fp32 evaluation of 12 flows against fp64.  With 4 flows
    and output convolutions scaled like a trained network's, the losses are held to 1e-4 and each gradient to 2e-3 of its maximum -
    twenty times the small-width bound, the same headroom over fp32 round-off as that test's."""
    cfg = dict(REF_WG, flows=4)
    od, pd = OW.WGDims(**cfg), WG.WGDims(**cfg)
    values = _values(od, scale_out=0.05)
    N, La = 1, 2048
    T = -(-(La - od.up_k) // od.up_stride) + 1
    audio, mel = _batch(od, N, T, La)
    torch.set_num_threads(16)
    rl, rg, _, _, _ = ref_step(values, od, audio, mel)
    eng = WT.WaveGlowTrainEngine(pd, device=dev, values=values)
    w = eng.plan(N, T, La)
    eng.forward(_dt(audio, dev), _dt(mel, dev), w)
    eng.loss_and_backward(w)
    _compare_step(eng, w, rl, rg, 1e-4, 2e-3)


def test_trained_checkpoint_inverts_through_the_inference_engine(dev, tmp_path, monkeypatch):
    """Train three steps, Save(), load waveglow.pt as Tacotron2.Vocoder_Load does, and run the shipped inference engine on the trained
    forward's own latents: it must give back the training audio (audio length = (T-1) S + K, so both directions see the same conditioning)."""
    from multi_speaker_tts_amd import Hyper_Parameters as hp
    from multi_speaker_tts_amd.WaveGlow import WaveGlow
    cfg = CFGS[0]
    od, pd = OW.WGDims(**cfg), WG.WGDims(**cfg)
    monkeypatch.setattr(hp.WaveGlow, "Checkpoint_Path", str(tmp_path / "wg"))
    N, T = 2, 13
    La = (T - 1) * od.up_stride + od.up_k              # 64: a multiple of G, as the inference path requires
    audio, mel = _batch(od, N, T, La)
    pattern = {"Audio": audio.astype(np.float32), "Mel": mel.astype(np.float32)}
    tr = WaveGlow(device=dev, dims=pd, values=_values(od))
    for _ in range(3):
        r = tr.Train_Step(pattern)
        assert np.isfinite(r["Loss"])
    tr.Save()
    f = tmp_path / "wg" / "waveglow.pt"
    values = {k: np.asarray(v) for k, v in torch.load(str(f), map_location="cpu").items()}          # MSTTS_SV.Vocoder_Load
    inf = WG.WaveGlowEngine(pd, device=dev, values=values)
    eng = tr.engine
    w = eng.plan(N, T, La)
    eng.forward(_dt(audio, dev), _dt(mel, dev), w)
    got = inf.infer(mel.astype(np.float32), noise=eng.latents(w))
    assert got.shape == (N, La)
    assert rel_err(t2n(got), audio) < 1e-3, rel_err(t2n(got), audio)
    tr2 = WaveGlow(device=dev, dims=pd, values=_values(od, seed=9))
    tr2.Restore()
    assert tr2.engine.global_step == 3 and all(np.array_equal(tr2.engine.values()[k], eng.values()[k]) for k in values if not k.startswith("__"))


def test_waveglow_loss_decreases(dev):
    """30 steps on one fixed synthetic batch at small width: the total loss falls and stays finite."""
    cfg = CFGS[0]
    od, pd = OW.WGDims(**cfg), WG.WGDims(**cfg)
    eng = WT.WaveGlowTrainEngine(pd, device=dev, values=WG.random_values(pd, seed=5))
    N, T = 4, 20
    La = (T - 1) * od.up_stride + od.up_k
    audio, mel = _batch(od, N, T, La)
    a, m = _dt(audio, dev), _dt(mel, dev)
    losses = []
    for _ in range(30):
        w = eng.train_step(a, m)
        losses.append(eng.scalars(w)["Loss"])
    assert all(np.isfinite(losses)), losses
    assert losses[-1] < losses[0] and np.mean(losses[-5:]) < np.mean(losses[:5]), losses
