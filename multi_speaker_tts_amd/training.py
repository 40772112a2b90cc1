"""Host plumbing shared by the training engines (engine.TrainEngine, taco1_trainer, speaker_trainer, waveglow_trainer) and the drop-in
trainer classes (Taco1_Mel_to_Spect.Mel_to_Spect, Speaker_Embedding.Speaker_Embedding, WaveGlow.WaveGlow): the weight-gradient split
heuristics, the batch-norm constants, the learning-rate schedule, the TF-Adam step, the layer blocks the engines (inference.InferEngine
too) write their graphs with, and a drop-in class's checkpoint file and Train loop.  The engines own their buffers and schedules.
"""
from __future__ import annotations

import math
import os
import time

import numpy as np
import torch

from . import Hyper_Parameters as hp
from . import lib
from .lib import ACT_NONE, call, ptr

BN_MOM, BN_EPS = 0.99, 1e-3

MAX_PLANS = 3      # workspace sets an auxiliary engine keeps (one per batch shape); a reference-width set holds a few GB


def _split_k(M, N, K, n_cu=256, max_split=16):
    """Reduction split of a weight-gradient GEMM (atomic accumulation into the gradient slab).  128x128 output tiles are
    spread round-robin over the CUs, so a CU runs c = ceil(tiles * sk / n_cu) workgroups of K / sk each: pick the sk with the
    least work on the busiest CU (448 tiles: sk = 4 -> 7 per CU exactly, 127 TFLOP/s, where sk = 2 leaves 3.5 -> 4 per CU,
    107 TFLOP/s; tools/gemm_split_probe.py), with a small per-split charge for the atomics.  Long reductions (the 25 632-row
    products) also weigh HOW MANY workgroups share a CU: one per CU is one wave per SIMD, nothing hides its load / store phases
    (2 560 x 512 x 25 632: sk = 3 -> 240 tiles, 91 TFLOP/s; sk = 9 -> 720 tiles = 3 per CU, 117 TFLOP/s)."""
    tiles = math.ceil(M / 128) * math.ceil(N / 128)
    if K >= 16384:
        ktiles, best, best_cost = K / 32.0, 1, None
        if tiles * max_split < n_cu:             # a handful of tiles (the Taco1 convolution bank: 1..8): split until the chip is covered once
            max_split = min(64, max(max_split, n_cu // tiles))
        for sk in range(1, max_split + 1):
            c = math.ceil(tiles * sk / n_cu)
            cost = c * (ktiles / sk + 6.0) / (0.75 if c == 1 else 0.92 if c == 2 else 1.0) * (1.0 + 0.004 * sk)
            if best_cost is None or cost < best_cost * (1.0 - 1e-9):
                best, best_cost = sk, cost
        return best
    best, best_cost = 1, None
    for sk in range(1, max_split + 1):
        if sk > 1 and K // sk < 512:
            break
        cost = math.ceil(tiles * sk / n_cu) / sk + 0.004 * sk
        if best_cost is None or cost < best_cost - 1e-9:
            best, best_cost = sk, cost
    return best


def _split_k_big(M, N, K, requested, n_cu=256):
    """Reduction split of a weight-gradient product on the 256 x 256-tile kernels (gemm_split_big_kernel / gemm_bf16_big_kernel: one workgroup
    per CU, taken from 160 workgroups on): rounds x (K-tiles per piece + a fixed cost per piece), pieces of at least 1 024 rows.  Returns
    `requested` (the split chosen for 128 x 128 tiles) when no split reaches those kernels."""
    tiles = math.ceil(M / 256) * math.ceil(N / 256)
    if M < 192 or N < 192:
        return requested
    best, best_cost = None, None
    for sk in range(1, 65):
        if sk > 1 and K // sk < 1024:
            break
        if tiles * sk < 160:
            continue
        cost = math.ceil(tiles * sk / n_cu) * (K / sk + 300.0) * (1.0 + 0.01 * sk)      # (+1 % per piece: its atomics onto the shared output)
        if best_cost is None or cost < best_cost - 1e-9:
            best, best_cost = sk, cost
    return best if best is not None else requested


def exponential_decay(lr, step):
    """tf.train.exponential_decay (not staircase) of the hyper-parameter group `lr` at `step`, floored at lr.Min.  A group with a
    Decay_Start_Step (Tacotron2, Taco1) counts the decay from that step and is capped at lr.Initial; one without (speaker encoder,
    WaveGlow) is not."""
    if "Decay_Start_Step" in lr:
        v = lr.Initial * lr.Decay_Rate ** ((step - lr.Decay_Start_Step) / lr.Decay_Step)
        return min(max(v, lr.Min), lr.Initial)
    return max(lr.Initial * lr.Decay_Rate ** (step / lr.Decay_Step), lr.Min)


class Workspace:
    """Attribute bag of one batch shape's device buffers."""


class Engine:
    """What the training engines share: zeroed device buffers, (slab, offset) of a variable and of its gradient, the TF-Adam step, and - for
    the auxiliary engines; TrainEngine carves its sets from an arena - the cache of workspace sets by batch shape in `_plans`."""

    def _f(self, *shape):
        """Zeroed fp32 buffer of `shape` (allocated in whole float4s)."""
        n = int(np.prod(shape))
        return torch.zeros((n + 3) // 4 * 4, dtype=torch.float32, device=self.device)[:n].view(shape)

    def P(self, name):
        return self.params.p(name)

    def G(self, name):
        return self.params.g(name)

    def _cached_plan(self, key, build):
        """The workspace set of batch shape `key`, now the most recently used; a new one is build(*key), made after the least recently used
        sets beyond MAX_PLANS - 1 are dropped (variable-length training: no workspace per shape forever)."""
        if key in self._plans:
            self._plans[key] = self._plans.pop(key)
        else:
            while len(self._plans) >= MAX_PLANS:
                self._plans.pop(next(iter(self._plans)))
            self._plans[key] = build(*key)
        return self._plans[key]

    def _adam(self, lr, wr_rate=0.0, grad_scale=1.0, clip=None):
        """One TF-Adam update of the trainable slab at the bias-corrected rate lr sqrt(1 - b2^t) / (1 - b1^t), t = global_step + 1:
        mstts_adam_tf (gradients x grad_scale, + wr_rate x the gradient of the weight regulariser over wd_mask), or with clip = (device
        address of 0.5 |g|^2, norm) mstts_adam_tf_clip (tf.clip_by_global_norm first, the factor formed on the device).  Advances
        global_step; returns that rate."""
        ps = self.params
        b1, b2, eps = self.adam
        t = self.global_step + 1
        lr_t = lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
        if clip is None:
            call("mstts_adam_tf", ptr(ps.train), ptr(ps.grad), ptr(ps.adam_m), ptr(ps.adam_v), ptr(ps.wd_mask), float(wr_rate),
                 float(grad_scale), float(lr_t), b1, b2, eps, ps.n_train)
        else:
            call("mstts_adam_tf_clip", ptr(ps.train), ptr(ps.grad), ptr(ps.adam_m), ptr(ps.adam_v), clip[0], 2.0, clip[1],
                 float(lr_t), b1, b2, eps, ps.n_train)
        self.global_step += 1
        ps.touch(frozen=False)               # (an InferEngine sharing this store keys its packed / folded kernels on the version; Adam writes `train` only)
        return lr_t


# ---- LSTM layers ----------------------------------------------------------------------------------------------------------------------
# kernel, wh, out and d_out are (tensor, element offset) pairs, every other buffer a tensor or None.  kernel is the cell's stacked kernel
# [cin + H, 4 H] (row stride 4 H), wh its recurrent rows; out / d_out hold [B, T, .] blocks at sb / st floats per batch row / time step.  The
# caller attaches the fused cell step's packed kernel and h blocks (wh_p, h_p) where it uses them.
def lstm_seq_fwd(B, T, H, cin, xw, kernel, lengths, reverse, zoneout, zc, zh, out, out_sb, out_st, c_hist, h_hist, acts, c_raw, gates_ws,
                 residual=None):
    """lib.LstmSeqFwd of one LSTM layer over a sequence (xw = x W_x + b over the kernel's cin input rows; acts / c_raw None: inference mode)."""
    return lib.LstmSeqFwd(B=B, T=T, H=H, xw=ptr(xw), wh=ptr(kernel[0], kernel[1] + cin * 4 * H), wh_ld=4 * H, lengths=ptr(lengths),
                          reverse=reverse, zoneout=zoneout, zc=ptr(zc), zh=ptr(zh), residual=ptr(residual), out=ptr(*out), out_sb=out_sb,
                          out_st=out_st, c_hist=ptr(c_hist), h_hist=ptr(h_hist), acts=ptr(acts), c_raw=ptr(c_raw), gates_ws=ptr(gates_ws))


def lstm_seq_bwd(B, T, H, wh, lengths, reverse, zoneout, zc, zh, d_out, dout_sb, dout_st, c_hist, acts, c_raw, dgates_step, dgates_pos, ws):
    """lib.LstmSeqBwd of one LSTM layer's BPTT (the gate gradients land step-major in dgates_step, batch-major in dgates_pos)."""
    return lib.LstmSeqBwd(B=B, T=T, H=H, wh=ptr(*wh), wh_ld=4 * H, lengths=ptr(lengths), reverse=reverse, zoneout=zoneout,
                          zc=ptr(zc), zh=ptr(zh), d_out=ptr(*d_out), dout_sb=dout_sb, dout_st=dout_st, c_hist=ptr(c_hist), acts=ptr(acts),
                          c_raw=ptr(c_raw), dgates_step=ptr(dgates_step), dgates_pos=ptr(dgates_pos), ws=ptr(ws))


def lstm_layer_fwd(eng, gemm, cell, x, xw, B, T, cin, H, *seq, **kw):
    """One LSTM layer of scope `cell` over x [B * T, cin], forward: the gate product x W_x + b into the caller's xw, and the lib.LstmSeqFwd of
    its steps, which the caller launches (seq, kw: lstm_seq_fwd's arguments from `lengths` on).  gemm: TrainEngine._gemm or lib.gemm."""
    k, ok = eng.P(cell + "kernel"); b, ob = eng.P(cell + "bias")
    gemm(x, k, xw, B * T, 4 * H, cin, cin, 4 * H, 4 * H, bias=b, b_off=ok, bias_off=ob)
    return lstm_seq_fwd(B, T, H, cin, xw, (k, ok), *seq, **kw)


def lstm_layer_grads(eng, gemm, cell, x, h, dgp, dgs, dx, rows, cin, H, dx_accumulate=False):
    """After one LSTM layer's BPTT: x^T dgp and h^T dgs into the gradient of the kernel of scope `cell`, the bias gradient (column sum of
    dgs), and dx = dgp W_x^T (+= with dx_accumulate).  gemm: TrainEngine._gemm or lib.gemm."""
    k, ok = eng.P(cell + "kernel")
    gk, ogk = eng.G(cell + "kernel"); gb, ogb = eng.G(cell + "bias")
    gemm(x, dgp, gk, cin, 4 * H, rows, cin, 4 * H, 4 * H, trans_a=True, split_k=max(2, _split_k(cin, 4 * H, rows)), c_off=ogk)
    gemm(h, dgs, gk, H, 4 * H, rows, H, 4 * H, 4 * H, trans_a=True, split_k=max(2, _split_k(H, 4 * H, rows)), c_off=ogk + cin * 4 * H)
    call("mstts_colsum", ptr(dgs), rows, 4 * H, 4 * H, ptr(gb, ogb), 1)
    gemm(dgp, k, dx, rows, cin, 4 * H, 4 * H, 4 * H, cin, trans_b=True, accumulate=dx_accumulate, b_off=ok)


# ---- dense, conv and batch-norm blocks ------------------------------------------------------------------------------------------------
def dense_fwd(eng, gemm, x, rows, cin, cout, scope, out, act=ACT_NONE, lda=None, bias=True):
    """x [rows, cin] (row pitch lda; None: cin) times the kernel of scope `scope`, + its bias unless bias=False, + activation, into out."""
    k, ok = eng.P(scope + "/kernel")
    b, ob = eng.P(scope + "/bias") if bias else (None, 0)
    gemm(x, k, out, rows, cout, cin, lda or cin, cout, cout, bias=b, act=act, b_off=ok, bias_off=ob)


def conv_fwd(eng, gemm, x, rows, T, cin, cout, K, conv, out, act):
    """conv1d 'same' of x [rows = batch x T, cin] with the kernel and bias of scope `conv`, + activation, into out."""
    k, ok = eng.P(conv + "/kernel"); b, ob = eng.P(conv + "/bias")
    gemm(x, k, out, rows, cout, K * cin, cin, cout, cout, bias=b, act=act, win=(T, cin, (K - 1) // 2), b_off=ok, bias_off=ob)


def bn_train_fwd(eng, bn, a, y, mean, rstd, mask, keep, rows, C, ws):
    """Training-mode batch norm of scope `bn` over a [rows, C] block (+ dropout with keep-mask `mask`; None and 1.0: none): the batch
    statistics to mean / rstd, the moving statistics updated."""
    g, og = eng.P(bn + "gamma"); b, ob = eng.P(bn + "beta")
    mm, omm = eng.P(bn + "moving_mean"); mv, omv = eng.P(bn + "moving_variance")
    call("mstts_bn_train_fwd", ptr(a), ptr(g, og), ptr(b, ob), ptr(mm, omm), ptr(mv, omv), ptr(y), ptr(mean), ptr(rstd),
         ptr(mask), float(keep), BN_MOM, BN_EPS, rows, C, ptr(ws))


def bn_infer_fwd(eng, bn, a, y, rows, C):
    """Inference-mode batch norm of scope `bn` over a [rows, C] block: the moving statistics, nothing updated."""
    g, og = eng.P(bn + "gamma"); b, ob = eng.P(bn + "beta")
    mm, omm = eng.P(bn + "moving_mean"); mv, omv = eng.P(bn + "moving_variance")
    call("mstts_bn_infer_fwd", ptr(a), ptr(g, og), ptr(b, ob), ptr(mm, omm), ptr(mv, omv), ptr(y), BN_EPS, rows, C)


def conv_bn_bwd(eng, gemm, conv, bn, dy, x_in, a, mean, rstd, mask, keep, act, rows, T, cin, cout, K, dz, dx, ws, dx_accumulate=False,
                wgrad_stream=None):
    """y = dropout(BN(act(conv(x)))): dy -> dz (the conv's pre-activation gradient), the parameter gradients into the gradient slab, dx (or
    None; += with dx_accumulate) through the flipped kernel (cached in eng.flip).  wgrad_stream: run the kernel's weight-gradient product
    (read by nothing before Adam) on that stream, behind this block's dz."""
    g, og = eng.P(bn + "gamma")
    gg, ogg = eng.G(bn + "gamma"); gb, ogb = eng.G(bn + "beta"); gbias, ogbias = eng.G(conv + "/bias")
    call("mstts_bn_train_bwd", ptr(dy), ptr(a), ptr(g, og), ptr(mean), ptr(rstd), ptr(mask), float(keep), act, ptr(dz),
         ptr(gg, ogg), ptr(gb, ogb), ptr(gbias, ogbias), rows, cout, ptr(ws))
    gk, ogk = eng.G(conv + "/kernel")
    pad = (K - 1) // 2
    wgrad = lambda: gemm(x_in, dz, gk, K * cin, cout, rows, cin, cout, cout, trans_a=True, win=(T, cin, pad),
                         split_k=max(2, _split_k(K * cin, cout, rows)), c_off=ogk)
    if wgrad_stream is None:
        wgrad()
    else:
        with lib.fork(wgrad_stream, done=False):         # (the caller joins the stream once, behind the last block)
            wgrad()
    if dx is not None:
        k, ok = eng.P(conv + "/kernel")
        key = (conv, K, cin, cout)
        if key not in eng.flip:
            eng.flip[key] = eng._f(K, cout, cin)
        wt = eng.flip[key]
        call("mstts_conv_kernel_flip", ptr(k, ok), ptr(wt), K, cin, cout)
        gemm(dz, wt, dx, rows, cin, K * cout, cout, cin, cin, win=(T, cout, K - 1 - pad), accumulate=dx_accumulate)


# ---- drop-in trainer classes ----------------------------------------------------------------------------------------------------------
class DropIn:
    """What the drop-in trainer classes share.  The checkpoint file <hp.<HP>.Checkpoint_Path>/<FILE> holds the variables whose names start
    with SCOPE, the Adam slots under `__adam_m__` / `__adam_v__` and the global step under `__global_step__` (Tacotron2.Vocoder_Load and
    Speaker_Embedding_Load read these files).  Train prints the time, the global step and the COLUMNS ((format, result key) pairs) of each
    step and saves every Checkpoint_Save_Timing steps; `_after_step(result)` is the per-step hook: here the status check of a device
    corpus feeder (`feeder`, from `_corpus_feeder`), a class adds its own."""
    HP = FILE = SCOPE = None
    COLUMNS = ()
    feeder = None

    def _file(self):
        return os.path.join(getattr(hp, self.HP).Checkpoint_Path.replace("\\", "/"), self.FILE)

    def _slots(self):
        """Optimizer state saved beside the variables: {key: tensor}."""
        return {"__adam_m__": self.params.adam_m, "__adam_v__": self.params.adam_v}

    def Restore(self):
        f = self._file()
        if not os.path.exists(f):
            print("There is no checkpoint.")
            return
        state = torch.load(f, map_location="cpu")
        self.params.load({k: v for k, v in state.items() if k.startswith(self.SCOPE)})
        if "__adam_m__" in state:
            for k, t in self._slots().items():
                t.copy_(state[k])
        self.engine.global_step = int(state.get("__global_step__", 0))
        print("Checkpoint '%s' is loaded." % f)

    def Save(self):
        f = self._file()
        os.makedirs(os.path.dirname(f), exist_ok=True)
        state = {k: torch.from_numpy(v) for k, v in self.params.export().items() if k.startswith(self.SCOPE)}
        state.update({k: t.cpu() for k, t in self._slots().items()})
        state["__global_step__"] = self.engine.global_step
        torch.save(state, f)

    def _upload(self, a):
        """A pattern array as a contiguous fp32 tensor on the engine's device (a tensor already there is taken as it is: no host round trip)."""
        if torch.is_tensor(a):
            return a.to(self.engine.device, torch.float32).contiguous()
        return torch.as_tensor(np.asarray(a, np.float32)).to(self.engine.device).contiguous()

    def _corpus_feeder(self):
        """The feeder Train() draws its patterns from when it is given no pattern_fn, made once; None: Train_Step(None), a class's
        synthetic pattern."""
        return None

    def Train(self, max_steps=None, pattern_fn=None):
        if pattern_fn is None:
            if self.feeder is None:
                self.feeder = self._corpus_feeder()
            if self.feeder is not None:
                pattern_fn = self.feeder.Get_Train_Pattern
        while max_steps is None or self.engine.global_step < max_steps:
            t0 = time.time()
            r = self.Train_Step(pattern_fn() if pattern_fn else None)
            print("\t\t".join(["Time: {:0.3f}".format(time.time() - t0), "Global step: {}".format(r["Global_Step"])] +
                              [fmt.format(r[k]) for fmt, k in self.COLUMNS]))
            if (r["Global_Step"] + 1) % getattr(hp, self.HP).Train.Checkpoint_Save_Timing == 0:
                self.Save()
            self._after_step(r)

    def _after_step(self, result):
        if hasattr(self.feeder, "check_status"):
            self.feeder.check_status()               # right behind the loss read of Train_Step: the stream is already drained
