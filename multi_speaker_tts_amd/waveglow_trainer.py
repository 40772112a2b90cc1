"""Training step of the WaveGlow vocoder (reference: WaveGlow/WaveGlow.py:37-85 with WaveGlow/Modules.py:9-34,135-175,198-352,373-385
and WaveGlow/Inv1x1.py:9-41) on the MI355X: Restructure_Train_Data (upsample the mel, slice it to the audio, fold G samples into
channels) -> Glow_Train (12 affine couplings: invertible 1x1 conv, WaveNet, exp(min(log_s, 8)) a1 + b, early outputs every 4 flows)
-> Glow_Loss (log-s, log-det and audio terms over size = N * L) -> tf.clip_by_global_norm(0.1) -> TF-Adam.

Python owns buffers and the schedule, every arithmetic step is a libmstts_hip.so call: the contractions on mstts_gemm_f32 (dilated
K = 3 convs in window mode in both directions, 1x1 convs, one conditioning product per flow), the rest in csrc/waveglow_train.hip
(one weight-norm launch for all 300 weight-normed convs each way, coupling forward / backward, fp64 log-determinants, gate and
res / skip backwards, the upsampler's tap-gradient gather, the device-side clip factor of Adam).  Every activation the backward needs
is kept (no recomputation through the inverse).  A step has no host synchronisation: the loss terms and the global norm stay in a
device buffer until `scalars` reads them.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import lib
from .lib import call, gemm, ptr
from .params import ParamStore
from .training import Engine, Workspace, _split_k, exponential_decay
from .waveglow import P_WG, WGDims, WaveNetOps, random_values, variable_table, wavenet

CLIP_NORM = 0.1          # tf.clip_by_global_norm(gradients, 0.1) (WaveGlow.py:69)
S_LOG_S, S_LOG_DET, S_AUDIO, S_SUMSQ = 0, 1, 2, 3       # device scalars: sum min(log_s, 8), sum logdet_f, 0.5 sum z^2, 0.5 sum g^2


def learning_rate(step):
    """tf.train.exponential_decay(1e-3, step, 100000, 0.5) (not staircase), floored at Min (WaveGlow.py:53-60)."""
    from . import Hyper_Parameters as hp
    return exponential_decay(hp.WaveGlow.Train.Learning_Rate, step)


def restructure(d: WGDims, N, audio_len, T):
    """Restructure_Train_Data's shapes (Modules.py:135-175): the audio is cut to L = floor(L_a / G) * G samples, the upsampled mel
    ((T - 1) * S + K samples) is sliced to the first L.  Returns (L, L / G, upsampled length); a mel too short for the audio is the
    reference's TF shape error."""
    L = audio_len // d.groups * d.groups
    up_len = (T - 1) * d.up_stride + d.up_k
    if L < d.groups:
        raise ValueError("audio of %d samples is shorter than one group of %d" % (audio_len, d.groups))
    if up_len < L:
        raise ValueError("the upsampled mel has %d samples, fewer than the %d audio samples it must condition ((T-1)*%d+%d with T=%d)"
                         % (up_len, L, d.up_stride, d.up_k, T))
    return L, L // d.groups, up_len


def early_chunk(d: WGDims, f):
    """(z column, width) of the chunk that leaves the flow stack at the output of flow f (Glow_Train :333-336,348-350): an early
    chunk when flow f + 1 starts with one, the whole output after the last flow, else None."""
    n_early = (d.flows - 1) // d.early_every
    if f == d.flows - 1:
        return n_early * d.early_size, d.channels(f)
    if (f + 1) % d.early_every == 0:
        return ((f + 1) // d.early_every - 1) * d.early_size, d.early_size
    return None


class WaveGlowTrainEngine(Engine):
    def __init__(self, dims: WGDims = None, device="cuda", seed=1234, values=None, adam=None):
        from . import Hyper_Parameters as hp
        self.d = dims or WGDims()
        self.device = torch.device(device)
        self.seed = seed
        lib.load()
        vals = values if values is not None else random_values(self.d, seed)
        missing = [n for n, _ in variable_table(self.d) if n not in vals]
        if missing:
            raise ValueError("WaveGlow variables missing: %s ..." % missing[:3])
        self.params = ParamStore(self.d, self.device, seed=seed, values=vals, trainable_fn=lambda n: True, weight_reg_fn=lambda n: False,
                                 table=variable_table(self.d))
        a = hp.WaveGlow.Train.ADAM
        self.adam = adam or (a.Beta1, a.Beta2, a.Epsilon)
        self.global_step = 0
        self._plans = {}
        self._last = None
        self._static()

    # ------------------------------------------------------------------ per-model constants: effective-kernel slabs and device tables
    def _wp(self, flow, name):
        return P_WG + "affine_coupling_layer_%d/" % flow + name

    def _static(self):
        d, ps = self.d, self.params
        ch, ldc, cm = d.ch, d.layers * 2 * d.ch, d.groups * d.n_mel
        # effective (weight-normalised) kernels and their gradients: one flat slab each, 16-byte aligned pieces
        layout, n = [], 0

        def take(shape):
            nonlocal n
            o = n
            n += (int(np.prod(shape)) + 3) // 4 * 4
            layout.append((o, shape))
            return len(layout) - 1
        self.eff = []
        for f in range(d.flows):
            c = d.channels(f)
            E = {"init": take((c // 2, ch)), "cond": take((cm, ldc)),
                 "in": [take((d.k * ch, 2 * ch)) for _ in range(d.layers)],
                 "res": [take((ch, 2 * ch if i < d.layers - 1 else ch)) for i in range(d.layers)]}
            self.eff.append(E)
        self.weff, self.dweff = self._f(max(n, 4)), self._f(max(n, 4))
        self._layout = layout
        # weight-norm descriptor tables (forward: w = the effective kernel; backward: w = its gradient)
        descs_f, descs_b, self.max_cols = [], [], 1
        for f in range(d.flows):
            E = self.eff[f]

            def add(name, idx, rows, cols, col0=0, ldw=None):
                o, shape = layout[idx]
                vt, vo = ps.p(self._wp(f, "wavenet/%s/kernel" % name)); gt, go = ps.p(self._wp(f, "wavenet/%s/g" % name))
                dvt, dvo = ps.g(self._wp(f, "wavenet/%s/kernel" % name)); dgt, dgo = ps.g(self._wp(f, "wavenet/%s/g" % name))
                for slab, lst in ((self.weff, descs_f), (self.dweff, descs_b)):
                    q = lib.WgWnDesc()
                    q.v, q.g, q.w = ptr(vt, vo), ptr(gt, go), ptr(slab, o + col0)
                    q.ldw = ldw or cols
                    q.dv, q.dg, q.rows, q.cols = ptr(dvt, dvo), ptr(dgt, dgo), rows, cols
                    lst.append(q)
                self.max_cols = max(self.max_cols, cols)
            c = d.channels(f)
            add("audio_initial_conv", E["init"], c // 2, ch)
            for i in range(d.layers):
                add("audio_in_%d" % i, E["in"][i], d.k * ch, 2 * ch)
                add("mel_cond_%d" % i, E["cond"], cm, 2 * ch, col0=i * 2 * ch, ldw=ldc)
                add("res_%d" % i, E["res"][i], ch, 2 * ch if i < d.layers - 1 else ch)
        self.n_wn = len(descs_f)

        def dev_bytes(structs):
            arr = (lib.WgWnDesc * len(structs))(*structs)
            return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device)
        self.wn_fwd, self.wn_bwd = dev_bytes(descs_f), dev_bytes(descs_b)
        # conditioning bias per flow = mel_cond_i/bias + audio_in_i/bias (the dilated conv accumulates onto the conditioning block)
        fold = []
        for f in range(d.flows):
            for i in range(d.layers):
                fold += [ps.offset[self._wp(f, "wavenet/mel_cond_%d/bias" % i)], ps.offset[self._wp(f, "wavenet/audio_in_%d/bias" % i)]]
        self.fold_table = torch.tensor(fold, dtype=torch.int64, device=self.device)
        self.b_cond = self._f(d.flows, ldc)
        self.logdet_table = torch.tensor([v for f in range(d.flows) for v in (ps.offset[self._wp(f, "invertible_1x1/kernel")], d.channels(f))],
                                         dtype=torch.int64, device=self.device)
        self.flip = self._f(d.k, 2 * ch, ch)
        # what `wavenet` reads per flow: (tensor, element offset) of the effective kernels in their slab and of the biases
        self.wn = []
        for f in range(d.flows):
            E, P = self.eff[f], lambda name: ps.p(self._wp(f, "wavenet/" + name))
            self.wn.append({"c": d.channels(f), "w_init": self._E(self.weff, E["init"]), "b_init": P("audio_initial_conv/bias"),
                            "w_cond": self._E(self.weff, E["cond"]), "b_cond": (self.b_cond, f * ldc),
                            "w_in": [self._E(self.weff, e) for e in E["in"]], "w_res": [self._E(self.weff, e) for e in E["res"]],
                            "b_res": [P("res_%d/bias" % i) for i in range(d.layers)], "w_out": P("conv1d/kernel"), "b_out": P("conv1d/bias")})

    def _E(self, slab, idx, off=0):
        """(tensor, element offset) of effective-kernel piece idx."""
        return slab, self._layout[idx][0] + off

    # ------------------------------------------------------------------ buffers
    def plan(self, N, T, L):
        """Workspaces for N utterances of L (grouped) audio samples conditioned on T mel frames."""
        return self._cached_plan((N, T, L), self._new_plan)

    def _new_plan(self, N, T, L):
        d, f = self.d, self._f
        L, Lg, up_len = restructure(d, N, L, T)
        w = Workspace()
        w.N, w.T, w.L, w.Lg, w.up_len = N, T, L, Lg, up_len
        rows, ch, ldc, cm = N * Lg, d.ch, d.layers * 2 * d.ch, d.groups * d.n_mel
        w.rows = rows
        w.Y = f(N * T, d.up_k * d.n_mel)                          # tap products (forward) / tap gradients (backward)
        w.up = f(N, up_len, d.n_mel)
        w.melg = f(rows, cm)
        w.z = f(rows, d.groups)
        w.ain = [f(rows, d.channels(i)) for i in range(d.flows)]
        w.y = [f(rows, d.channels(i)) for i in range(d.flows)]
        w.lsb = [f(rows, d.channels(i)) for i in range(d.flows)]
        w.cond = [f(rows, ldc) for _ in range(d.flows)]
        w.xs = [[f(rows, ch) for _ in range(d.layers)] for _ in range(d.flows)]
        w.zs = [[f(rows, ch) for _ in range(d.layers)] for _ in range(d.flows)]
        w.skip = [f(rows, ch) for _ in range(d.flows)]
        w.rs = f(rows, 2 * ch)
        w.scal = f(8)
        cmax = d.groups
        w.d_y, w.d_lsb, w.d_ain = f(rows, cmax), f(rows, cmax), f(rows, cmax)
        w.d_skip, w.d_x, w.d_z = f(rows, ch), f(rows, ch), f(rows, ch)
        w.d_rs, w.d_pre = f(rows, 2 * ch), f(rows, 2 * ch)
        w.d_cond, w.d_melg = f(rows, ldc), f(rows, cm)
        return w

    # ------------------------------------------------------------------ forward (Restructure_Train_Data + Glow_Train)
    def forward(self, audio, mel, w):
        """audio [N, L_a], mel [N, T, n_mel] (contiguous fp32 device tensors)."""
        d = self.d
        N, T, L, Lg, rows = w.N, w.T, w.L, w.Lg, w.rows
        assert mel.shape == (N, T, d.n_mel) and audio.shape[0] == N and audio.shape[1] // d.groups * d.groups == L
        ch, ldc, cm, C = d.ch, d.layers * 2 * d.ch, d.groups * d.n_mel, d.n_mel
        ps = self.params
        w.mel, w.audio = mel, audio
        call("mstts_wg_weight_norm_fwd", ptr(self.wn_fwd), self.n_wn, self.max_cols)
        call("mstts_wg_bias_fold", ptr(ps.train), ptr(self.fold_table), ptr(self.b_cond), d.flows * d.layers, 2 * ch)
        # Upsample_Mel: every tap product of every frame (the [1, K, Cout, Cin] kernel read transposed), overlap-add + bias, slice to L
        uk, uo = self.P(P_WG + "conv2d_transpose/kernel"); ub, ubo = self.P(P_WG + "conv2d_transpose/bias")
        gemm(mel, uk, w.Y, N * T, d.up_k * C, C, C, C, d.up_k * C, trans_b=True, b_off=uo)
        call("mstts_wg_overlap_add", ptr(w.Y), ptr(ub, ubo), ptr(w.up), N, T, d.up_k, d.up_stride, C)
        call("mstts_copy2d", ptr(w.up), w.up_len * C, ptr(w.melg), L * C, N, L * C, 0)
        call("mstts_copy2d", ptr(audio), audio.shape[1], ptr(w.ain[0]), L, N, L, 0)
        w.scal.zero_()
        ops = WaveNetOps()                    # the plain fp32 schedule
        for f in range(d.flows):
            c = d.channels(f)
            wt, wo = self.P(self._wp(f, "invertible_1x1/kernel"))
            gemm(w.ain[f], wt, w.y[f], rows, c, c, c, c, c, b_off=wo)
            # every layer keeps its own input and gated activation for the backward; a0 is read in place (lda = c); the last layer has no residual output
            wavenet(ops, d, rows, Lg, self.wn[f], None, w.y[f], c, w.melg, w.cond[f], w.xs[f] + [None], w.zs[f], w.rs, w.skip[f], w.lsb[f])
            zc, ce = early_chunk(d, f) or (0, 0)
            nxt = w.ain[f + 1] if f + 1 < d.flows else None
            call("mstts_wg_coupling_fwd", ptr(w.y[f]), ptr(w.lsb[f]), ptr(nxt), ptr(w.z), d.groups, zc, ce, ptr(w.scal, S_LOG_S), rows, c)
        call("mstts_l2_loss_acc", ptr(w.z), None, rows * d.groups, ptr(w.scal, S_AUDIO))
        self._last = w
        return w.z

    # ------------------------------------------------------------------ Glow_Loss + backward
    def loss_and_backward(self, w):
        d, ps = self.d, self.params
        N, T, L, Lg, rows = w.N, w.T, w.L, w.Lg, w.rows
        ch, ldc, cm, C = d.ch, d.layers * 2 * d.ch, d.groups * d.n_mel, d.n_mel
        inv_size = 1.0 / (rows * d.groups)
        ps.grad.zero_()
        self.dweff.zero_()
        # log-det terms and their W gradient (-(1/G) det/(det+1e-6) W^-T: N L/G / size = 1/G); the contractions below accumulate onto it
        call("mstts_wg_inv1x1_logdet", ptr(ps.train), ptr(ps.grad), ptr(self.logdet_table), d.flows, -1.0 / d.groups, ptr(w.scal, S_LOG_DET))
        d_next = None
        for f in reversed(range(d.flows)):
            c = d.channels(f)
            h = c // 2
            E = self.eff[f]
            p = "wavenet/"
            zc, ce = early_chunk(d, f) or (0, 0)
            call("mstts_wg_coupling_bwd", ptr(w.y[f]), ptr(w.lsb[f]), ptr(w.z), d.groups, zc, ce, ptr(d_next), inv_size, ptr(w.d_y), ptr(w.d_lsb), rows, c)
            # output conv (plain conv1d, no weight norm)
            kt, ko = self.P(self._wp(f, p + "conv1d/kernel"))
            gk, gko = self.G(self._wp(f, p + "conv1d/kernel")); gb, gbo = self.G(self._wp(f, p + "conv1d/bias"))
            gemm(w.skip[f], w.d_lsb, gk, ch, c, rows, ch, c, c, trans_a=True, accumulate=True, split_k=_split_k(ch, c, rows), c_off=gko)
            call("mstts_colsum", ptr(w.d_lsb), rows, c, c, ptr(gb, gbo), 1)
            gemm(w.d_lsb, kt, w.d_skip, rows, ch, c, c, c, ch, trans_b=True, b_off=ko)
            for i in reversed(range(d.layers)):
                last = i == d.layers - 1
                nres = ch if last else 2 * ch
                call("mstts_wg_res_skip_bwd", None if last else ptr(w.d_x), ptr(w.d_skip), ptr(w.d_rs), ptr(w.d_z), rows, ch, int(last))
                sl, so = self._E(self.dweff, E["res"][i]); gb, gbo = self.G(self._wp(f, p + "res_%d/bias" % i))
                gemm(w.zs[f][i], w.d_rs, sl, ch, nres, rows, ch, nres, nres, trans_a=True, accumulate=True, split_k=_split_k(ch, nres, rows), c_off=so)
                call("mstts_colsum", ptr(w.d_rs), rows, nres, nres, ptr(gb, gbo), 1)
                sl, so = self._E(self.weff, E["res"][i])
                gemm(w.d_rs, sl, w.d_z, rows, ch, nres, nres, nres, ch, trans_b=True, accumulate=True, b_off=so)
                call("mstts_wg_gate_bwd", ptr(w.cond[f], i * 2 * ch), ldc, ptr(w.d_z), ptr(w.d_pre), ptr(w.d_cond, i * 2 * ch), ldc, rows, ch)
                win = (Lg, ch, (d.k - 1) // 2, 2 ** i)
                sl, so = self._E(self.dweff, E["in"][i])
                gemm(w.xs[f][i], w.d_pre, sl, d.k * ch, 2 * ch, rows, ch, 2 * ch, 2 * ch, trans_a=True, accumulate=True, win=win,
                     split_k=_split_k(d.k * ch, 2 * ch, rows), c_off=so)
                sl, so = self._E(self.weff, E["in"][i])
                call("mstts_conv_kernel_flip", ptr(sl, so), ptr(self.flip), d.k, ch, 2 * ch)
                gemm(w.d_pre, self.flip, w.d_x, rows, ch, d.k * 2 * ch, 2 * ch, ch, ch, win=(Lg, 2 * ch, d.k - 1 - (d.k - 1) // 2, 2 ** i))
            # x_0 = a0 . w_init + b
            sl, so = self._E(self.dweff, E["init"]); gb, gbo = self.G(self._wp(f, p + "audio_initial_conv/bias"))
            gemm(w.y[f], w.d_x, sl, h, ch, rows, c, ch, ch, trans_a=True, accumulate=True, split_k=_split_k(h, ch, rows), c_off=so)
            call("mstts_colsum", ptr(w.d_x), rows, ch, ch, ptr(gb, gbo), 1)
            sl, so = self._E(self.weff, E["init"])
            gemm(w.d_x, sl, w.d_y, rows, h, ch, ch, ch, c, trans_b=True, accumulate=True, b_off=so)
            # the conditioning product of all layers: weight gradient, bias gradients (shared by mel_cond_i and audio_in_i), d melg
            sl, so = self._E(self.dweff, E["cond"])
            gemm(w.melg, w.d_cond, sl, cm, ldc, rows, cm, ldc, ldc, trans_a=True, accumulate=True, split_k=_split_k(cm, ldc, rows), c_off=so)
            for i in range(d.layers):
                for nm in ("mel_cond_%d/bias", "audio_in_%d/bias"):
                    gb, gbo = self.G(self._wp(f, p + nm % i))
                    call("mstts_colsum", ptr(w.d_cond, i * 2 * ch), rows, 2 * ch, ldc, ptr(gb, gbo), 1)
            sl, so = self._E(self.weff, E["cond"])
            gemm(w.d_cond, sl, w.d_melg, rows, cm, ldc, ldc, ldc, cm, trans_b=True, accumulate=f < d.flows - 1, b_off=so)
            # invertible 1x1: y = audio_in . W
            wt, wo = self.P(self._wp(f, "invertible_1x1/kernel")); gw, gwo = self.G(self._wp(f, "invertible_1x1/kernel"))
            gemm(w.ain[f], w.d_y, gw, c, c, rows, c, c, c, trans_a=True, accumulate=True, split_k=_split_k(c, c, rows), c_off=gwo)
            if f > 0:
                gemm(w.d_y, wt, w.d_ain, rows, c, c, c, c, c, trans_b=True, b_off=wo)
                d_next = w.d_ain
        call("mstts_wg_weight_norm_bwd", ptr(self.wn_bwd), self.n_wn, self.max_cols)
        # upsampler: tap gradients gathered from the sliced d melg, then dW = dY^T mel lands in the [1, K, Cout, Cin] layout
        call("mstts_wg_overlap_add_bwd", ptr(w.d_melg), ptr(w.Y), N, T, d.up_k, d.up_stride, C, L)
        gk, gko = self.G(P_WG + "conv2d_transpose/kernel"); gb, gbo = self.G(P_WG + "conv2d_transpose/bias")
        gemm(w.Y, w.mel, gk, d.up_k * C, C, N * T, d.up_k * C, C, C, trans_a=True, accumulate=True, split_k=_split_k(d.up_k * C, C, N * T), c_off=gko)
        call("mstts_colsum", ptr(w.d_melg), N * L, C, C, ptr(gb, gbo), 1)
        call("mstts_l2_loss_acc", ptr(ps.grad), None, ps.n_train, ptr(w.scal, S_SUMSQ))       # 0.5 * global norm^2, stays on the device
        self._last = w

    def adam_step(self, w=None):
        """tf.clip_by_global_norm(grads, 0.1) + TF-Adam; the clip factor is formed on the device from the gradient's sum of squares."""
        w = w or self._last
        lr = learning_rate(self.global_step)
        self._adam(lr, clip=(ptr(w.scal, S_SUMSQ), CLIP_NORM))
        return lr

    def scalars(self, w):
        s = w.scal.detach().cpu().numpy().astype(np.float64)
        size = float(w.rows * self.d.groups)
        log_s = -s[S_LOG_S] / size
        log_det = -s[S_LOG_DET] * (w.N * w.Lg) / size
        audio = s[S_AUDIO] / size
        return {"Log_S_Loss": log_s, "Log_Det_W_Loss": log_det, "Audio_Loss": audio, "Loss": log_s + log_det + audio,
                "Global_Norm": math.sqrt(max(2.0 * s[S_SUMSQ], 0.0))}

    def train_step(self, audio, mel):
        """audio [N, L_a], mel [N, T, n_mel] (device tensors, contiguous fp32)."""
        N, T, _ = mel.shape
        w = self.plan(N, T, audio.shape[1])
        self.forward(audio, mel, w)
        self.loss_and_backward(w)
        self.adam_step(w)
        return w

    def latents(self, w):
        """The forward's outputs in the `noise` format WaveGlowEngine.infer consumes: {"z": [N, L/G, z_channels], "early_<f>": [N, L/G, early_size]}."""
        d = self.d
        z = w.z.view(w.N, w.Lg, d.groups)
        out = {}
        for f in range(d.flows):
            zc, width = early_chunk(d, f) or (None, None)
            if zc is None:
                continue
            out["z" if f == d.flows - 1 else "early_%d" % (f + 1)] = z[:, :, zc:zc + width].clone()
        return out

    def values(self):
        return self.params.export()
