"""Stage-wise judge of WaveGlowEngine.infer(arith="bf16") (config 3 for the vocoder) and a float32 torch emulation of the mode.

The mode's contract (multi_speaker_tts_amd/waveglow.py, WaveGlowEngine.infer): every contraction multiplies operands rounded to bf16
(round-to-nearest-even) and accumulates in fp32; biases, the gate, the residual stream, the skip sum, the coupling inverse, latents and
overlap-add stay fp32.  The rounded activations are stored tensors: melg_b = bf(melg), zb = bf(z), xb_0 = bf(x), xb_{i+1} = bf(fl32(z_i + res_i)).

`check` follows no trajectory: every stage is judged from what the engine itself stored as that stage's inputs (the `stages` hook of
infer), so a rounding flip in one stage cannot show up anywhere else, and every bound is derived, none is measured on the code under test:

  contraction of STORED bf16 operands: a bf16 x bf16 product is exact in fp32, so only the K + 2 fp32 additions (K products, bias, the
      value accumulated onto) round:  |C - ref64| <= 2 (K + 2) 2^-24 (|A| |B| + |bias| + |C0|), ref64 in float64 from the same bf16 values;
      the factor 2 covers the matrix cores' internal order.  Where two products meet in one buffer (pre-activation = cond + conv), K is
      the sum of both;
  gate: z against the float64 gate of the stored pre-activation, relative bound GATE_REL (below);
  zb, xb: exact (a lone IEEE add and a round-to-nearest-even conversion are reproducible);
  skip sum: `layers` fp32 additions of stored values: 2 layers 2^-24 sum |skip_i|;
  coupling inverse: expf <= 2 ulp, the subtraction and the product half an ulp each, then c products and additions:
      2 (c + 8) 2^-24 |x| |w_inv|;
  melg_b (from the caller's mel): the upsampler's two contraction-like sums to the bound above, plus the final rounding's 2^-8 |melg| (bf16 keeps 8 significant bits).
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
# The fp32 gate kernel's own accuracy is the yardstick for z: GATE_KERNEL_REL is the smallest relative bound (two digits, rounded up) under which
# the EXISTING mstts_wg_gate passes against the float64 gate - measured on the MI355X on the pre-activations the bf16 engine stores in every case of
# tests/test_gpu_waveglow_bf16.py (1.9e-7 .. 2.7e-7) and on normal draws of scale 0.3 .. 6 (2.5e-7 .. 2.8e-7; tanhf and expf are a few ulp each);
# test_gate_bf16 there prints the figure for its input and asserts it has not grown.  The tolerance for z is twice that.
GATE_KERNEL_REL = 2.8e-7
GATE_REL = 2 * GATE_KERNEL_REL


def bf(t):
    """Round to bf16 (round-to-nearest-even) and widen again."""
    return t.to(torch.bfloat16).to(t.dtype if t.dtype in (torch.float32, torch.float64) else torch.float32)


def im2col(x, N, Lg, k, dil, pad, shift=None):
    """The implicit im2col view of x [N * Lg, C]: [N * Lg, k * C], tap j reads row t + (j - pad) * dil of the same sequence, zero outside it.
    shift: {tap: extra rows} (a planted fault)."""
    C = x.shape[1]
    xs = x.reshape(N, Lg, C)
    cols = []
    for j in range(k):
        s = (j - pad) * dil + (shift or {}).get(j, 0)
        o = torch.zeros_like(xs)
        if s >= 0:
            if s < Lg:
                o[:, :Lg - s] = xs[:, s:]
        elif -s < Lg:
            o[:, -s:] = xs[:, :Lg + s]
        cols.append(o)
    return torch.cat(cols, dim=2).reshape(N * Lg, k * C)


def gate64(pre):
    C = pre.shape[1] // 2
    p = pre.double()
    return torch.tanh(p[:, :C]) * torch.sigmoid(p[:, C:])


def _shape(d, mel):
    N, T = mel.shape[0], mel.shape[1]
    L = (T - 1) * d.up_stride + d.up_k
    return N, T, L, L // d.groups


def _upsample64(eng, mel, dt=torch.float64):
    """(melg, bound) of Upsample_Mel from bf16-rounded operands: [rows, G * n_mel] each."""
    d = eng.d
    N, T, L, Lg = _shape(d, mel)
    dev = eng.up_w.device
    m = bf(torch.as_tensor(np.asarray(mel), dtype=torch.float32).to(dev)).to(dt).reshape(N * T, d.n_mel)
    w = bf(eng.up_w).to(dt)
    Y, Ya = (m @ w).reshape(N, T, d.up_k, d.n_mel), (m.abs() @ w.abs()).reshape(N, T, d.up_k, d.n_mel)
    out = eng.up_b.to(dt).expand(N, L, d.n_mel).clone()
    oa = out.abs()
    for t in range(T):
        out[:, t * d.up_stride:t * d.up_stride + d.up_k] += Y[:, t]
        oa[:, t * d.up_stride:t * d.up_stride + d.up_k] += Ya[:, t]
    taps = -(-d.up_k // d.up_stride)
    return out.reshape(N * Lg, d.groups * d.n_mel), 2 * (d.n_mel + taps + 2) * U * oa.reshape(N * Lg, d.groups * d.n_mel)


# --------------------------------------------------------------------------------------------------------------------- emulation
FAULTS = ("truncate", "xb_unrounded", "round_before_add", "conv_fp32_x", "weight_other_rounding", "tap_shift")


def _truncate(t):
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def _other_rounding(w):
    """bf16 values of w, except that every element within a quarter of a bf16 ulp of a rounding tie takes the OTHER neighbour: what rounding
    the float64 fold directly (instead of the fp32 fold the engine packs) does to an element near a tie, on enough elements to be seen."""
    bits = w.contiguous().view(torch.int32)
    low = bits & 0xFFFF
    down, up = (bits & -65536).view(torch.float32), ((bits & -65536) + 65536).view(torch.float32)
    rne = bf(w)
    near = (low >= 0x6000) & (low <= 0xA000) & (low != 0x8000)
    return torch.where(near, torch.where(rne == down, up, down), rne)


def emulate(eng, mel, noise, sigma=1.0, fault=None, at=(1, 1)):
    """WaveGlowEngine.infer(arith="bf16") restated in float32 torch on the engine's device-side constants (an engine built with device="cpu" serves):
    same rounding sites, `stages` in the engine's layout.  Returns (wav, stages).  fault: one of FAULTS, planted at (flow, layer) `at`."""
    assert fault is None or fault in FAULTS
    d = eng.d
    N, T, L, Lg = _shape(d, mel)
    rows, cm, ch, pad = N * Lg, d.groups * d.n_mel, d.ch, (d.k - 1) // 2
    f32 = torch.float32
    mm = lambda a, b: bf(a) @ bf(b)                       # bf16 operands (exact products), fp32 accumulation
    melg = _upsample64(eng, mel, f32)[0]
    melg_b = bf(melg)
    stages = {"resident": {"cond": False, "conv": False, "res_skip": False}}
    audio = torch.as_tensor(np.asarray(noise["z"]), dtype=f32).reshape(rows, d.z_channels)
    for f in reversed(range(d.flows)):
        F = eng.flow[f]
        c = F["c"]
        h = c // 2
        x = mm(audio[:, :h], F["w_init"]) + F["b_init"]
        cond = mm(melg_b, F["w_cond"]) + F["b_cond"]
        stages[f] = {"melg_b": melg_b.to(torch.bfloat16), "audio": audio.clone(), "x": x.clone()}
        xb = bf(x)
        out = None
        for i in range(d.layers):
            here = fault is not None and (f, i) == tuple(at)
            last = i == d.layers - 1
            w = bf(F["w_in"][i])
            a = xb
            if here and fault == "conv_fp32_x":
                a = x
            if here and fault == "weight_other_rounding":
                w = _other_rounding(F["w_in"][i])
            A = im2col(a, N, Lg, d.k, 2 ** i, pad, shift={0: 2 ** i - 1} if here and fault == "tap_shift" else None)
            st = stages[(f, i)] = {"xb": xb.clone()}
            pre = cond[:, i * 2 * ch:(i + 1) * 2 * ch] + A @ w
            z = gate64(pre).to(f32)
            zb = bf(z)
            rs = zb @ bf(F["w_res"][i]) + F["b_res"][i]
            st.update(pre=pre, z=z, zb=zb, rs=rs)
            if last:
                skip = rs
            else:
                x = z + rs[:, :ch]
                xb = bf(x)
                nxt_here = fault is not None and (f, i + 1) == tuple(at)
                if nxt_here and fault == "truncate":
                    xb = _truncate(x)
                if nxt_here and fault == "xb_unrounded":
                    xb = x
                if nxt_here and fault == "round_before_add":
                    xb = bf(zb + rs[:, :ch])
                skip = rs[:, ch:]
            out = skip.clone() if i == 0 else out + skip
        ls_b = mm(out, F["w_out"]) + F["b_out"]
        early = f % d.early_every == 0 and f > 0
        ce = d.early_size if early else 0
        xs = torch.cat([audio[:, :h], (audio[:, h:] - ls_b[:, h:]) * torch.exp(-ls_b[:, :h])], dim=1)
        nxt = xs @ F["w_inv"]
        if early:
            e = torch.as_tensor(np.asarray(noise["early_%d" % f]), dtype=f32).reshape(rows, ce)
            nxt = torch.cat([e * sigma, nxt], dim=1)
        stages[f].update(out=out, ls_b=ls_b, next=nxt)
        audio = nxt
    return audio.reshape(N, Lg * d.groups), stages


# --------------------------------------------------------------------------------------------------------------------- the judge
def check(stages, eng, mel, noise=None, sigma=1.0, wav=None, raise_=True):
    """Judge every stage of one infer(arith="bf16", stages=stages) call (see the module docstring).  Returns the findings in the order the
    engine computes the stages, [(stage, flow, layer or None, worst excess over the bound)]; raise_: AssertionError when there are any."""
    d = eng.d
    N, T, L, Lg = _shape(d, mel)
    rows, cm, ch, pad = N * Lg, d.groups * d.n_mel, d.ch, (d.k - 1) // 2
    dev = stages[d.flows - 1]["x"].device
    D = lambda t: t.to(dev).double()
    found = []

    def within(stage, f, i, got, ref, bound):
        got, ref = D(got), D(ref)
        assert got.shape == ref.shape, (stage, f, i, got.shape, ref.shape)
        ok = torch.isfinite(got).all() and bool(((got - ref).abs() <= bound).all())
        if not ok:
            found.append((stage, f, i, float(((got - ref).abs() - bound).nan_to_num(nan=math.inf).max())))

    def exact(stage, f, i, got, ref):
        got, ref = got.to(dev).float(), ref.to(dev).float()
        assert got.shape == ref.shape, (stage, f, i, got.shape, ref.shape)
        if not torch.equal(got.view(torch.int32), ref.view(torch.int32)):
            found.append((stage, f, i, float((got.double() - ref.double()).abs().nan_to_num(nan=math.inf).max())))

    def product(stage, f, i, got, A, W, bias, K, base=None, base_abs=None):
        """got against A . W + bias (+ base) from float64 copies of the stored operands; K: the number of products per element"""
        ref, mag = A @ W + D(bias), A.abs() @ W.abs() + D(bias).abs()
        if base is not None:
            ref, mag = ref + base, mag + base_abs
        within(stage, f, i, got, ref, 2 * (K + 2) * U * mag)

    melg, melg_bound = _upsample64(eng, mel)
    melg, melg_bound = melg.to(dev), melg_bound.to(dev)
    Wp = eng.packed()
    prev = None
    for f in reversed(range(d.flows)):
        F, S = eng.flow[f], stages[f]
        c = F["c"]
        h = c // 2
        audio = D(S["audio"])
        if prev is None:
            if noise is not None:
                exact("audio", f, None, S["audio"], torch.as_tensor(np.asarray(noise["z"]), dtype=torch.float32).reshape(rows, d.z_channels))
        else:
            exact("audio", f, None, S["audio"], prev)
        within("melg_b", f, None, S["melg_b"].float(), melg, melg_bound + 2.0 ** -8 * melg.abs())
        mb = D(S["melg_b"].float())
        product("x", f, None, S["x"], D(bf(S["audio"].float()[:, :h])), D(bf(F["w_init"])), F["b_init"], h)
        Wc, bc = D(Wp[f]["w_cond"].float()).t(), D(F["b_cond"])
        skips = []
        for i in range(d.layers):
            st = stages[(f, i)]
            last = i == d.layers - 1
            if i == 0:
                exact("xb", f, i, st["xb"], bf(S["x"].float()))
            else:
                p = stages[(f, i - 1)]
                exact("xb", f, i, st["xb"], bf(p["z"].float() + p["rs"].float()[:, :ch]))
            band = slice(i * 2 * ch, (i + 1) * 2 * ch)
            cref, cabs = mb @ Wc[:, band] + bc[band], mb.abs() @ Wc[:, band].abs() + bc[band].abs()
            A = im2col(D(st["xb"].float()), N, Lg, d.k, 2 ** i, pad)
            product("pre", f, i, st["pre"], A, D(Wp[f]["w_in"][i].float()).t(), torch.zeros(2 * ch), cm + d.k * ch, base=cref, base_abs=cabs)
            z64 = gate64(D(st["pre"]))
            within("z", f, i, st["z"], z64, GATE_REL * z64.abs() + 1e-37)
            exact("zb", f, i, st["zb"], bf(st["z"].float()))
            product("rs", f, i, st["rs"], D(st["zb"].float()), D(Wp[f]["w_res"][i].float()).t(), F["b_res"][i], ch)
            skips.append(D(st["rs"]) if last else D(st["rs"])[:, ch:])
        within("out", f, None, S["out"], sum(skips), 2 * d.layers * U * sum(s.abs() for s in skips))
        product("ls_b", f, None, S["ls_b"], D(bf(S["out"].float())), D(bf(F["w_out"])), F["b_out"], ch)
        early = f % d.early_every == 0 and f > 0
        ce = d.early_size if early else 0
        ls = D(S["ls_b"])
        xs = torch.cat([audio[:, :h], (audio[:, h:] - ls[:, h:]) * torch.exp(-ls[:, :h])], dim=1)
        winv = D(F["w_inv"])
        within("next", f, None, S["next"][:, ce:], xs @ winv, 2 * (c + 8) * U * (xs.abs() @ winv.abs()))
        if early and noise is not None:
            e = torch.as_tensor(np.asarray(noise["early_%d" % f]), dtype=torch.float32).reshape(rows, ce).to(dev)
            exact("early", f, None, S["next"][:, :ce], e * torch.tensor(sigma, dtype=torch.float32))
        prev = S["next"]
    if wav is not None:
        exact("wav", 0, None, wav.reshape(rows, -1), prev)
    if raise_ and found:
        raise AssertionError("bf16 WaveGlow stages over their bounds (stage, flow, layer, excess): %s" % found[:8])
    return found
