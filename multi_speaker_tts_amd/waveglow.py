"""WaveGlow vocoder, inference direction, on the MI355X (reference: WaveGlow/Modules.py:177-208,210-327,354-371,
WaveGlow/Inv1x1.py:9-41; wired at MSTTS_SV.py:117-125,325-389).

Python owns buffers and the schedule; every arithmetic step is a libmstts_hip.so call:
  * the transposed-conv mel upsampler = one GEMM (frame x all taps) + mstts_wg_overlap_add,
  * per coupling layer: the initial 1x1 conv, ONE GEMM for the conditioning 1x1 convs of all WaveNet layers, then per
    layer the dilated K=3 conv as an implicit-im2col GEMM (win_dil) accumulated onto its conditioning block,
    mstts_wg_gate, the res/skip 1x1 GEMM, mstts_wg_res_skip; the zero-initialised output conv; mstts_wg_coupling_inv
    (affine inverse + inverse 1x1 conv + early-latent re-injection),
  * tf.random.normal -> mstts_philox_normal (or injected arrays, which is what the parity tests use).
infer(arith="bf16") is the same schedule in BASELINE config 3 arithmetic: bf16 operands in every contraction, fp32 accumulate, the three big
products on operands that are bf16 in memory (mstts_gemm_bf16_res).  The schedule is written once: `wavenet` runs the network inside a
coupling for inference and for the training forward (waveglow_trainer.py), `WaveNetOps` holds what depends on the arithmetic.
Weight normalisation (g * v / ||v||, WaveGlow/Modules.py:9-34) and the matrix inverses of the 1x1 kernels are
constants of a checkpoint and are folded once at load time on the host.
"""
from __future__ import annotations

from dataclasses import dataclass
import math
import os

import numpy as np
import torch

from . import lib
from .lib import call, gemm, gemm_res, gemm_res_supported, ptr

P_WG = "waveglow/"
ARITHS = ("f32", "bf16")


def resolve_arith(arith, default=None):
    """The vocoder's arithmetic: the argument, else the engine's default, else MSTTS_WG_ARITH, else "f32"."""
    for a in (arith, default, os.environ.get("MSTTS_WG_ARITH") or None):
        if a is not None:
            if a not in ARITHS:
                raise ValueError("WaveGlow arithmetic must be one of %s, not %r" % (ARITHS, a))
            return a
    return "f32"


def resolve_denoise(strength, default=None):
    """The denoiser's strength: the argument, else the caller's default, else MSTTS_WG_DENOISE, else 0.0 (off).  Negative or not a
    number: ValueError."""
    for v, what in ((strength, "denoiser strength"), (default, "denoiser strength"), (os.environ.get("MSTTS_WG_DENOISE") or None, "MSTTS_WG_DENOISE")):
        if v is not None:
            try:
                f = float(v)
            except (TypeError, ValueError):
                raise ValueError("%s must be a number, not %r" % (what, v))
            if not (0.0 <= f < float("inf")):
                raise ValueError("%s must be finite and not negative, not %r" % (what, v))
            return f
    return 0.0


@dataclass
class WGDims:
    """hp.WaveGlow / hp.Sound.Mel_Dim (Hyper_Parameters.py:196-210)."""
    n_mel: int = 80
    flows: int = 12
    groups: int = 8
    early_every: int = 4
    early_size: int = 2
    up_k: int = 1024
    up_stride: int = 256
    layers: int = 8
    ch: int = 512
    k: int = 3

    def channels(self, flow):
        return self.groups - (flow // self.early_every) * self.early_size

    @property
    def z_channels(self):
        return self.groups - (int(math.ceil(self.flows / self.early_every)) - 1) * self.early_size

    @classmethod
    def from_hp(cls, hp):
        w = hp.WaveGlow
        return cls(n_mel=hp.Sound.Mel_Dim, flows=w.Flows, groups=w.Groups, early_every=w.Early_Every, early_size=w.Early_Size,
                   up_k=w.Upsample.Kernel_Size, up_stride=w.Upsample.Strides, layers=w.WaveNet.Layers, ch=w.WaveNet.Channels,
                   k=w.WaveNet.Kernel_Size)


def variable_table(d: WGDims):
    """[(name, shape)] in the reference's variable scopes (inferred; unverified against a real checkpoint)."""
    t = [(P_WG + "conv2d_transpose/kernel", (1, d.up_k, d.n_mel, d.n_mel)), (P_WG + "conv2d_transpose/bias", (d.n_mel,))]
    cm = d.groups * d.n_mel
    for f in range(d.flows):
        c = d.channels(f)
        p = P_WG + "affine_coupling_layer_%d/" % f
        t.append((p + "invertible_1x1/kernel", (c, c)))

        def wn(name, k, cin, cout):
            t.extend([(p + "wavenet/" + name + "/g", (cout,)), (p + "wavenet/" + name + "/kernel", (1, k, cin, cout)),
                      (p + "wavenet/" + name + "/bias", (cout,))])
        wn("audio_initial_conv", 1, c // 2, d.ch)
        for i in range(d.layers):
            wn("audio_in_%d" % i, d.k, d.ch, 2 * d.ch)
            wn("mel_cond_%d" % i, 1, cm, 2 * d.ch)
            wn("res_%d" % i, 1, d.ch, 2 * d.ch if i < d.layers - 1 else d.ch)
        t.append((p + "wavenet/conv1d/kernel", (1, d.ch, c)))
        t.append((p + "wavenet/conv1d/bias", (c,)))
    return t


def random_values(d: WGDims, seed=0):
    """The reference's initialisers (uniform(0, .02) upsampler, glorot weight-norm kernels, N(0,1) 1x1 kernels with
    positive determinant, zero output conv).  A WaveGlow initialised like this is the identity coupling."""
    g = np.random.default_rng(seed)
    out = {}
    for name, shape in variable_table(d):
        if name.endswith("bias") or "wavenet/conv1d" in name:
            v = np.zeros(shape)
        elif "conv2d_transpose/kernel" in name:
            v = g.uniform(0, 0.02, shape)
        elif "invertible_1x1" in name:
            v = g.normal(0, 1, shape)
            if np.linalg.det(v) < 0:
                v[:, 0] *= -1
        elif name.endswith("/g"):
            v = g.uniform(-1, 1, shape) * math.sqrt(6.0 / (2 * shape[0]))
        else:
            rf = int(np.prod(shape[:-2]))
            lim = math.sqrt(6.0 / (shape[-2] * rf + shape[-1] * rf))
            v = g.uniform(-lim, lim, shape)
        out[name] = v.astype(np.float32)
    return out


def _weight_norm(g, v):
    v = np.asarray(v, np.float64)
    ss = (v * v).sum(axis=(0, 1, 2), keepdims=True)
    return np.asarray(g, np.float64) * v / np.sqrt(np.maximum(ss, 1e-5))


def _conv_two_pieces(rows, n_out):
    """Whether the dilated convolution [rows, k ch] x [k ch, n_out] runs as two reduction pieces onto a zeroed buffer (see WaveNetOps).
    Fitted to tools/wg_conv_ab.py at the reference widths (per-layer microseconds, one piece | two pieces: batch 1: 92 | 64, 2: 99 | 118,
    4: 185 | 164, 5: 187 | 174, 6: 277 | 322, 8: 268 | 330, 12: 534 | 501, 16: 571 | 518, 24: 838 | 853, 32: 923 | 1050): the 128 x 128-tile kernel's
    time steps at 256, 512 and then every 1 024 tiles, the 256 x 256-tile kernel's at every 256 workgroups; in units of the latter's round."""
    cols128, cols256 = -(-n_out // 128), -(-n_out // 256)
    t128 = -(-rows // 128) * cols128
    w256 = -(-rows // 256) * cols256 * 2
    if t128 <= 128:                      # a fraction of the chip either way: two pieces of the small kernel fill it better
        return True
    if w256 < 160:                       # (below the library's threshold for the big tile)
        return False
    one = 0.58 if t128 <= 256 else 1.12 if t128 <= 512 else 1.65 * -(-t128 // 1024)
    return -(-w256 // 256) < one


_at = lambda w: w if isinstance(w, tuple) else (w, 0)     # (tensor, element offset) of a weight or bias given as that pair or as a bare tensor


class WaveNetOps:
    """The part of the schedule that depends on the arithmetic, resolved once per call: which entry point each product goes to, the dilated
    convolution's form, the gate and the res/skip kernel.  The default is the plain fp32 schedule (the training forward's).
    bf16: operands rounded to bf16 in every contraction; res_cond / res_conv / res_rs: that product reads the STORED bf16 copy of its
    activation and the packed weight (mstts_gemm_bf16_res).  The convolution (fp32 forms): one piece accumulated onto its band of cond
    (mstts_gemm_f32 takes 64-row tiles for such shapes, 688 at batch 4 x 40 frames: no atomics; split_in > 1 splits its reduction), or
    `two`: exactly two reduction pieces (split_k = 2) onto a ZEROED buffer of its own, which the gate adds.  0 + p + q is the same float
    whichever piece's atomic lands first (three pieces would not be order-free), so the flow stays bit-reproducible per latent seed, and
    at batch 4 x 40 frames 22 x 4 tiles x 2 pieces = 176 workgroups reach the 256 x 256-tile kernel (csrc/gemm_split.inc) where the
    128 x 128 one runs 344 tiles as a round and a third: 185 -> 164 us per layer.  _conv_two_pieces decides, a fixed function of the shape."""

    def __init__(self, bf16=False, res_cond=False, res_conv=False, res_rs=False, two=False, split_in=1):
        assert not (two and (bf16 or split_in != 1)) and (bf16 or not (res_cond or res_conv or res_rs))
        self.bf16, self.res_cond, self.res_conv, self.res_rs, self.two, self.split_in = bf16, res_cond, res_conv, res_rs, two, split_in

    def product(self, resident, A, Ab, W, Wb, Cm, M, N, K, lda, ldc, bias=None, **kw):
        """Cm [M, N] (pitch ldc) = A . W + bias.  A: the fp32 operand [M, K], Ab its stored bf16 copy, both at pitch lda; W: the fp32 weight
        [K, N] (ldb = N), Wb the packed one, TRANSPOSED [N, K] (ldb = K).  resident picks the bf16 pair.  kw: accumulate, split_k, win, c_off."""
        (W, b_off), (bias, bias_off) = _at(Wb if resident else W), _at(bias)
        if resident:
            gemm_res(Ab, W, Cm, M, N, K, lda, K, ldc, bias=bias, b_off=b_off, bias_off=bias_off, **kw)
        else:
            gemm(A, W, Cm, M, N, K, lda, N, ldc, bias=bias, b_off=b_off, bias_off=bias_off, bf16=self.bf16, **kw)

    def gate(self, cond, band, ldc, conv, z, zb, rows, ch):
        if self.two:
            call("mstts_wg_gate_add", ptr(cond, band), ldc, ptr(conv), ptr(z), rows, ch)
        elif self.res_rs:
            call("mstts_wg_gate_bf16", ptr(cond, band), ldc, ptr(z), ptr(zb), rows, ch)
        else:
            call("mstts_wg_gate", ptr(cond, band), ldc, ptr(z), rows, ch)

    def res_skip(self, z, rs, x, xb, out, rows, ch, last, first):
        if self.res_conv:
            call("mstts_wg_res_skip_bf16", ptr(z), ptr(rs), ptr(xb), ptr(out), rows, ch, int(last), int(first))
        else:
            call("mstts_wg_res_skip", ptr(z), ptr(rs), ptr(x), ptr(out), rows, ch, int(last), int(first))


def wavenet(ops, d, rows, Lg, W, Wp, a, lda, melg, cond, xs, zs, rs, out, ls_b, melg_b=None, xb=None, zb=None, conv=None, stages=None, f=None):
    """The network inside one coupling (WaveGlow/Modules.py:251-327), inference and training forward alike: initial conv of a[:, :c/2]
    (read in place at pitch lda), ONE product for the conditioning convs of all layers, per layer the dilated conv accumulated onto its
    conditioning band / gate / res-skip product / res-skip glue, the output conv into ls_b.  2 + 3 layers + 1 launches (+ 1 rounding of x
    when the convolution is resident).
    W: the coupling's c, w_init, b_init, w_cond, b_cond, w_in[i], w_res[i], b_res[i], w_out, b_out as (tensor, element offset) pairs or
    bare tensors; Wp: its packed bf16 weights (w_cond, w_in[i], w_res[i]) where a product is resident.  xs[i] / zs[i]: layer i's input and
    gated activation ([rows, ch]; xs[layers] is the last layer's unused residual output and may be None); cond [rows, layers 2 ch], rs
    [rows, 2 ch], out = the skip sum; melg_b, xb, zb: the stored bf16 copies (resident products only); conv: the two-piece convolution's
    buffer.  stages, f: the bf16 mode's test hook (WaveGlowEngine.infer)."""
    ch, cm, ldc, c = d.ch, d.groups * d.n_mel, d.layers * 2 * d.ch, W["c"]
    bf = lambda t: t.to(torch.bfloat16)
    ops.product(False, a, None, W["w_init"], None, xs[0], rows, ch, c // 2, lda, ch, bias=W["b_init"])
    if ops.res_conv:
        call("mstts_round_bf16", ptr(xs[0]), ptr(xb), rows * ch)
    ops.product(ops.res_cond, melg, melg_b, W["w_cond"], Wp and Wp["w_cond"], cond, rows, ldc, cm, cm, ldc, bias=W["b_cond"])
    if stages is not None:
        stages[f] = {"melg_b": melg_b.clone() if ops.res_cond else bf(melg.view(rows, cm)), "x": xs[0].clone()}
    for i in range(d.layers):
        last, band, win = i == d.layers - 1, i * 2 * ch, (Lg, ch, (d.k - 1) // 2, 2 ** i)
        if stages is not None:
            st = stages[(f, i)] = {"xb": xb.clone() if ops.res_conv else bf(xs[i])}
        if ops.two:
            conv.zero_()
            ops.product(False, xs[i], None, W["w_in"][i], None, conv, rows, 2 * ch, d.k * ch, ch, 2 * ch, split_k=2, win=win)
        else:
            ops.product(ops.res_conv, xs[i], xb, W["w_in"][i], Wp and Wp["w_in"][i], cond, rows, 2 * ch, d.k * ch, ch, ldc, accumulate=True,
                        split_k=ops.split_in, win=win, c_off=band)
        ops.gate(cond, band, ldc, conv, zs[i], zb, rows, ch)
        nres = ch if last else 2 * ch
        ops.product(ops.res_rs, zs[i], zb, W["w_res"][i], Wp and Wp["w_res"][i], rs, rows, nres, ch, ch, nres, bias=W["b_res"][i])
        if stages is not None:
            st.update(pre=cond[:, band:band + 2 * ch].clone(), z=zs[i].clone(), zb=zb.clone() if ops.res_rs else bf(zs[i]),
                      rs=rs.view(-1)[:rows * nres].view(rows, nres).clone())
        ops.res_skip(zs[i], rs, xs[i + 1], xb, out, rows, ch, last, i == 0)
    ops.product(False, out, None, W["w_out"], None, ls_b, rows, c, ch, ch, c, bias=W["b_out"])


class WaveGlowEngine:
    def __init__(self, dims: WGDims = None, device="cuda", values=None, seed=1234, arith=None):
        self.d = dims or WGDims()
        if arith is not None:
            resolve_arith(arith)
        self.arith = arith         # default of infer(arith=None): "f32" | "bf16" (config 3: bf16 operands in every contraction) | None = MSTTS_WG_ARITH, else "f32"
        self.device = torch.device(device)
        self.seed = seed
        lib.load()
        vals = values if values is not None else random_values(self.d, seed)
        missing = [n for n, _ in variable_table(self.d) if n not in vals]
        if missing:
            raise ValueError("WaveGlow variables missing: %s ..." % missing[:3])
        self.load(vals)
        self._keep = []
        self.split_in = 0          # > 1: split the dilated-conv GEMM's reduction (atomic accumulation); 0 / 1 = off (see WaveNetOps)
        self.conv_two_pieces = os.environ.get("MSTTS_WG_TWO_PIECES", "1") != "0"     # the dilated convolution as two reduction pieces onto a zeroed buffer (see WaveNetOps)

    # ------------------------------------------------------------------ checkpoint constants, folded on the host once
    def _dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)

    def load(self, v):
        d = self.d
        self._packed = None
        self._bias = {}            # bias_spectrum's cache: a property of the checkpoint
        # conv2d_transpose kernel [1,K,Cout,Cin] -> [Cin, K*Cout]: one GEMM gives every tap product of a frame
        wt = np.asarray(v[P_WG + "conv2d_transpose/kernel"], np.float64)[0]
        self.up_w = self._dev(wt.transpose(2, 0, 1).reshape(d.n_mel, d.up_k * d.n_mel))
        self.up_b = self._dev(v[P_WG + "conv2d_transpose/bias"])
        self.flow = []
        for f in range(d.flows):
            c = d.channels(f)
            p = P_WG + "affine_coupling_layer_%d/wavenet/" % f
            wn = lambda n: _weight_norm(v[p + n + "/g"], v[p + n + "/kernel"])[0]
            F = {"c": c}
            F["w_init"], F["b_init"] = self._dev(wn("audio_initial_conv")[0]), self._dev(v[p + "audio_initial_conv/bias"])
            # the conditioning convs of all layers side by side; the bias of each layer's dilated conv rides along
            F["w_cond"] = self._dev(np.concatenate([wn("mel_cond_%d" % i)[0] for i in range(d.layers)], axis=1))
            F["b_cond"] = self._dev(np.concatenate([np.asarray(v[p + "mel_cond_%d/bias" % i], np.float64) + np.asarray(v[p + "audio_in_%d/bias" % i], np.float64)
                                                    for i in range(d.layers)]))
            F["w_in"] = [self._dev(wn("audio_in_%d" % i).reshape(d.k * d.ch, 2 * d.ch)) for i in range(d.layers)]
            F["w_res"] = [self._dev(wn("res_%d" % i)[0]) for i in range(d.layers)]
            F["b_res"] = [self._dev(v[p + "res_%d/bias" % i]) for i in range(d.layers)]
            F["w_out"], F["b_out"] = self._dev(np.asarray(v[p + "conv1d/kernel"])[0]), self._dev(v[p + "conv1d/bias"])
            F["w_inv"] = self._dev(np.linalg.inv(np.asarray(v[P_WG + "affine_coupling_layer_%d/invertible_1x1/kernel" % f], np.float64)))
            self.flow.append(F)

    def packed(self):
        """The bf16 mode's resident weights: the folded fp32 tensors rounded once (round-to-nearest-even) and stored transposed, [N, K]
        k-contiguous, as mstts_gemm_bf16_res reads them.  Built on first use, cached per load()."""
        if self._packed is None:
            t = lambda w: w.t().contiguous().to(torch.bfloat16)
            self._packed = [{"w_cond": t(F["w_cond"]), "w_in": [t(w) for w in F["w_in"]], "w_res": [t(w) for w in F["w_res"]]} for F in self.flow]
        return self._packed

    def _b(self, *shape):
        t = torch.empty(shape, dtype=torch.bfloat16, device=self.device)
        self._keep.append(t)
        return t

    def _f(self, *shape):
        n = int(np.prod(shape))
        t = torch.empty((n + 3) // 4 * 4, dtype=torch.float32, device=self.device)[:n].view(shape)
        self._keep.append(t)
        return t

    # ------------------------------------------------------------------ Glow_Inference
    def _begin(self, mel):
        """Start of a call: drops the previous call's buffers; mel as a contiguous fp32 device tensor [N, T, n_mel] and the upsampled length."""
        d = self.d
        self._keep = []
        mel = (mel if torch.is_tensor(mel) else torch.from_numpy(np.asarray(mel))).to(self.device, torch.float32).contiguous()
        N, T, C = mel.shape
        assert C == d.n_mel
        L = (T - 1) * d.up_stride + d.up_k
        if L % d.groups:
            raise ValueError("upsampled length %d is not a multiple of Groups=%d" % (L, d.groups))
        return mel, N, T, C, L

    def _latent(self, noise, seed, rows, key, width, stream, scale):
        """[rows, width] latent: the injected noise[key], else Philox normals of (seed, stream)."""
        t = self._f(rows, width)
        if noise is not None:
            t.copy_((noise[key] if torch.is_tensor(noise[key]) else torch.from_numpy(np.asarray(noise[key]))).to(self.device, torch.float32).reshape(rows, width))
        else:
            call("mstts_philox_normal", ptr(t), rows * width, seed, stream, scale)
        return t

    @lib.deterministic_gemm()          # bit-reproducible per latent seed: no K-cuts with atomics inside the flow's contractions
    def infer(self, mel, noise=None, seed=None, sigma=1.0, arith=None, stages=None):
        """mel [N, T, n_mel] (tensor or array) -> wav tensor [N, (T-1)*stride + kernel].  noise: {"z": [N,L/G,z_channels],
        "early_<flow>": [N,L/G,early_size]} to inject the latents, else Philox normals of `seed`.  arith: "f32" | "bf16" (resolve_arith).

        "bf16" is BASELINE config 3 for the vocoder: every contraction multiplies operands rounded to bf16 (round-to-nearest-even) and
        accumulates in fp32; biases, the gate, the residual stream, the skip sum, the coupling inverse (with w_inv), latents and overlap-add
        stay fp32.  The rounded activations are STORED tensors - melg_b = bf(melg), zb = bf(z), xb_{i+1} = bf(fl32(z_i + res_i)), xb_0 = bf(x) -
        written by the glue kernels (mstts_round_bf16, mstts_wg_gate_bf16, mstts_wg_res_skip_bf16), and the three big products (conditioning,
        dilated convolution, res/skip: 204 of a call's launches) read them and the packed weights as they are (mstts_gemm_bf16_res).  The
        dilated convolution is always one piece accumulated onto its band of `cond`; conv_two_pieces and split_in are fp32-mode features.  The
        upsampler, the initial conv (K <= 4) and the output conv (N <= 8) have fp32 operands anyway and run on mstts_gemm_bf16.  A product
        mstts_gemm_bf16_res does not take (ch % 8 != 0), and all three with MSTTS_WG_BF16_RESIDENT=0 (the A/B leg), falls back to
        mstts_gemm_bf16 on the fp32 buffers: same rounding sites (the kernel rounds the same fp32 values), same contract.

        stages: a test hook of the bf16 mode (the fp32 mode leaves it alone: its parity tests compare the waveform).  It receives "resident"
        (which products ran resident), per flow f a dict stages[f] of melg_b, audio (the flow's input), x (the initial conv's output), out (the
        skip sum), ls_b and next (the coupling inverse's output), and per layer stages[(f, i)] = pre (the layer's band of cond after the conv
        accumulated), z, zb, rs, xb (as consumed)."""
        d = self.d
        mel, N, T, C, L = self._begin(mel)
        Lg, rows, cm, ch, ldc = L // d.groups, N * (L // d.groups), d.groups * C, d.ch, d.layers * 2 * d.ch
        # everything the schedule depends on, once
        bf16 = resolve_arith(arith, self.arith) == "bf16"
        resident = bf16 and os.environ.get("MSTTS_WG_BF16_RESIDENT", "1") != "0"
        split_in = 1 if bf16 else self.split_in or 1
        ops = WaveNetOps(bf16=bf16, split_in=split_in,
                         res_cond=resident and gemm_res_supported(rows, ldc, cm, cm, cm),
                         res_conv=resident and gemm_res_supported(rows, 2 * ch, d.k * ch, ch, d.k * ch, win=(Lg, ch)),
                         res_rs=resident and gemm_res_supported(rows, 2 * ch, ch, ch, ch),
                         two=not bf16 and self.conv_two_pieces and split_in == 1 and ch % 4 == 0 and _conv_two_pieces(rows, 2 * ch))
        Wp = self.packed() if (ops.res_cond or ops.res_conv or ops.res_rs) else None
        keep = stages if bf16 else None
        if keep is not None:
            keep["resident"] = {"cond": ops.res_cond, "conv": ops.res_conv, "res_skip": ops.res_rs}
        # Upsample_Mel: every tap product of every frame, then overlap-add (+ bias)
        Y = self._f(N * T, d.up_k * C)
        ops.product(False, mel, None, self.up_w, None, Y, N * T, d.up_k * C, C, C, d.up_k * C)
        melg = self._f(N, L, C)                       # viewed as [rows, G*C]: contiguous regrouping (:180-187)
        call("mstts_wg_overlap_add", ptr(Y), ptr(self.up_b), ptr(melg), N, T, d.up_k, d.up_stride, C)
        melg_b = None
        if ops.res_cond:
            melg_b = self._b(rows, cm)
            call("mstts_round_bf16", ptr(melg), ptr(melg_b), rows * cm)
        seed = self.seed if seed is None else seed
        latent = lambda key, width, stream, scale: self._latent(noise, seed, rows, key, width, stream, scale)
        audio = latent("z", d.z_channels, 70, 1.0)
        x, z, out = self._f(rows, ch), self._f(rows, ch), self._f(rows, ch)
        cond, rs = self._f(rows, ldc), self._f(rows, 2 * ch)
        # (rounded copies only where their consumer is resident; the two-piece convolution's own output buffer)
        xb = self._b(rows, ch) if ops.res_conv else None
        zb = self._b(rows, ch) if ops.res_rs else None
        conv = self._f(rows, 2 * ch) if ops.two else None
        for f in reversed(range(d.flows)):
            F = self.flow[f]
            c = F["c"]
            ls_b = self._f(rows, c)
            wavenet(ops, d, rows, Lg, F, Wp and Wp[f], audio, c, melg, cond, [x] * (d.layers + 1), [z] * d.layers, rs, out, ls_b,
                    melg_b=melg_b, xb=xb, zb=zb, conv=conv, stages=keep, f=f)
            early = f % d.early_every == 0 and f > 0
            ce = d.early_size if early else 0
            e = latent("early_%d" % f, ce, 71 + f, 1.0) if early else None
            nxt = self._f(rows, c + ce)
            call("mstts_wg_coupling_inv", ptr(audio), ptr(ls_b), ptr(F["w_inv"]), ptr(e) if early else None, float(sigma), ptr(nxt), rows, c, ce)
            if keep is not None:
                keep[f].update(audio=audio.clone(), out=out.clone(), ls_b=ls_b.clone(), next=nxt.clone())
            audio = nxt
        return audio.view(N, Lg * d.groups)


    # ------------------------------------------------------------------ denoiser
    def bias_spectrum(self, arith=None, n_fft=1024, hop=256, win=1024, frames=88, mel_value=0.0):
        """The network's stationary bias as a magnitude spectrum, device tensor [n_fft / 2 + 1]: `infer` on a constant mel
        [1, frames, n_mel] of mel_value with every latent injected as zeros, then |X_0| of that waveform - frame 0 of the STFT only, as the
        published denoiser takes it - through mstts_stft_fft (raw magnitudes, no pre-emphasis).  Cached per argument tuple and resolved
        arithmetic; load() drops the cache."""
        from . import Audio
        d = self.d
        key = (resolve_arith(arith, self.arith), int(n_fft), int(hop), int(win), int(frames), float(mel_value))
        if key in self._bias:
            return self._bias[key]
        n_fft, hop, win, frames = key[1:5]
        L = (frames - 1) * d.up_stride + d.up_k
        if L <= n_fft // 2:
            raise ValueError("the bias waveform of %d frames has %d samples, shorter than the STFT's reflect padding (%d samples)" % (frames, L, n_fft // 2))
        if not lib.load().mstts_stft_fft_supported(n_fft, win) or hop < 1:
            raise ValueError("bias_spectrum: n_fft must be a power of two in [512, 4096] and win <= n_fft (n_fft %d, hop %d, win %d)" % (n_fft, hop, win))
        zeros = lambda width: torch.zeros(1, L // d.groups, width, dtype=torch.float32, device=self.device)
        noise = {"z": zeros(d.z_channels)}
        noise.update({"early_%d" % f: zeros(d.early_size) for f in range(d.flows) if f % d.early_every == 0 and f > 0})
        mel = torch.full((1, frames, d.n_mel), key[5], dtype=torch.float32, device=self.device)
        wav = self.infer(mel, noise=noise, arith=key[0]).reshape(-1).contiguous()
        hann, tw = Audio._fft_constants_samples(n_fft, win, str(self.device))
        offs = torch.tensor([0, L, 0, 1], dtype=torch.int64, device=self.device)
        spec = torch.empty(n_fft // 2 + 1, dtype=torch.float32, device=self.device)
        call("mstts_stft_fft", ptr(wav), ptr(offs), ptr(offs, 2), 1, 0.0, ptr(hann), ptr(tw), None, None, n_fft, hop, win, 0, 1.0, 0.0, None,
             ptr(spec), 1, None, None, 0.0, 2)
        self._bias[key] = spec
        return spec

    def denoise(self, wavs, strength, arith=None, n_fft=1024, hop=256, win=1024, frames=88, mel_value=0.0, return_tensor=False):
        """Audio.spectral_denoise_batch with this network's bias spectrum: strength * bias_spectrum(...) subtracted from the magnitude of
        every STFT bin of every waveform (list of arrays or device tensors), one device call -> list of float32 waveforms of the same lengths."""
        from . import Audio
        bias = self.bias_spectrum(arith, n_fft, hop, win, frames, mel_value)
        return Audio.spectral_denoise_batch(wavs, bias, strength, n_fft, hop, win, device=self.device, return_tensor=return_tensor)

    def _denoise_rows(self, rows, index, strength, arith=None, n_fft=1024, hop=256, win=1024, frames=88, mel_value=0.0):
        """`denoise` on rows [chunks, L] of a device tensor of which waveform i is the rows index[i][0] .. index[i][1]: consecutive rows
        are one contiguous range each, which is the packed layout of mstts_wg_denoise as it stands - no copy -> list of host arrays."""
        from . import Audio
        if not Audio.spectral_denoise_supported(n_fft, hop, win):
            return self.denoise([rows[a:b].reshape(-1) for a, b in index], strength, arith, n_fft, hop, win, frames, mel_value)
        assert rows.is_contiguous() and [a for a, _ in index[1:]] == [b for _, b in index[:-1]] and index[0][0] == 0 and index[-1][1] == rows.shape[0]
        bias = self.bias_spectrum(arith, n_fft, hop, win, frames, mel_value)
        hann, tw = Audio._fft_constants_samples(int(n_fft), int(win), str(self.device))
        return Audio._denoise_packed(rows.reshape(-1), [(b - a) * rows.shape[1] for a, b in index], bias, strength, n_fft, hop, win, hann, tw, False)


# ---- MSTTS_SV.Inference_WaveGlow host logic (MSTTS_SV.py:335-375,452-458) ----------------------------------------------
def split_mels(mels, split):
    """Every mel cut into `split`-frame chunks; index[i] = (first, last+1) chunk of utterance i."""
    chunks, index = [], []
    for mel in mels:
        parts = [mel[x:x + split] for x in range(0, mel.shape[0], split)]
        start = index[-1][1] if index else 0
        chunks.extend(parts)
        index.append((start, start + len(parts)))
    return chunks, index


def vocode(engine: WaveGlowEngine, mels, split, batch, noise_seed=None, arith=None, denoise=None, denoise_args=None):
    """Chunk, zero-pad to the longest chunk, run `batch` chunks at a time, stitch (the per-chunk tail of kernel - stride
    samples is NOT trimmed, as in the reference: WaveGlow/Modules.py:179 is commented out).  denoise: the denoiser's strength
    (`resolve_denoise`: None = MSTTS_WG_DENOISE, else off); when positive the stitched utterances stay on the device, go through
    WaveGlowEngine.denoise in ONE call (denoise_args: its n_fft / hop / win / frames / mel_value, where not the defaults) and are copied
    to the host once.  Off, nothing of that runs and the result is what it was without the argument, bit for bit."""
    strength = resolve_denoise(denoise)
    chunks, index = split_mels(mels, split)
    tmax = max(c.shape[0] for c in chunks)
    pat = np.zeros((len(chunks), tmax, engine.d.n_mel), np.float32)
    for i, c in enumerate(chunks):
        pat[i, :c.shape[0]] = c
    wavs = []
    for b0 in range(0, len(chunks), batch):
        seed = None if noise_seed is None else noise_seed + b0
        wav = engine.infer(pat[b0:b0 + batch], seed=seed, arith=arith)        # (held by reference: infer drops its own list of buffers at each call)
        wavs.append(wav if strength > 0 else wav.cpu().numpy())
    if strength > 0:
        return engine._denoise_rows(torch.cat(wavs, dim=0), index, strength, arith=arith, **(denoise_args or {}))
    allw = np.concatenate(wavs, axis=0)
    return [allw[a:b].reshape(-1) for a, b in index]


def export_length(stop, frame_shift_ms, sample_rate):
    stop = np.asarray(stop)
    cut = int(np.argmax(stop > 0.5)) if (stop > 0.5).any() else stop.shape[0]
    return int(cut * frame_shift_ms / 1000 * sample_rate)
