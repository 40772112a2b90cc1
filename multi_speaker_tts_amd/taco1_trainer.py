"""Training step of the Taco1 mel -> spectrogram vocoder (reference: Taco1_Mel_to_Spect/Taco1_Mel_to_Spect.py:24-100 with
Taco1_Mel_to_Spect/Modules.py:8-108) on the MI355X: ConvBank (8 convs + BN, max-pool, two projections + BN, residual) ->
4 highway layers -> BiLSTM(128, zoneout .1, no length mask) -> dense 256 -> 1025; loss = mean |pred - spectrogram| +
1e-6 * sum l2_loss(v) over variables whose lower-cased name has none of 'bias', 'lstm', 'rnn'; TF-Adam; BN moving statistics
updated by the same step.  Python owns buffers and the schedule, the arithmetic is libmstts_hip.so (the same GEMM / BN /
LSTM-sequence kernels as the Tacotron2 trainer plus mstts_maxpool2_same_bwd, mstts_highway_combine_bwd, mstts_l1_loss_fwd_bwd).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import lib
from .lib import ACT_NONE, ACT_RELU, call, gemm, ptr
from .masks import step_seed
from .params import VOC, Dims, ParamStore, bank_suffix
from .training import (Engine, Workspace, _split_k, bn_train_fwd, conv_bn_bwd, conv_fwd, dense_fwd, exponential_decay, lstm_layer_fwd,
                       lstm_layer_grads, lstm_seq_bwd)

BIRNN = VOC + "birnn/stack_bidirectional_rnn/cell_0/bidirectional_rnn/%s/zoneout_lstm_cell/"


def is_trainable(name):
    return name.startswith(VOC) and not name.endswith(("moving_mean", "moving_variance"))


def in_weight_reg(name):
    """Taco1_Mel_to_Spect.py:45-53."""
    low = name.lower()
    return not any(s in low for s in ("bias", "lstm", "rnn"))


def learning_rate(step):
    """Taco1_Mel_to_Spect.py:63-69."""
    from . import Hyper_Parameters as hp
    return exponential_decay(hp.Taco1_Mel_to_Spect.Train.Learning_Rate, step)


class Taco1TrainEngine(Engine):
    def __init__(self, dims: Dims = None, device="cuda", seed=1234, values=None, wr_rate=None, adam=None):
        from . import Hyper_Parameters as hp
        self.d = dims or Dims()
        self.device = torch.device(device)
        self.seed = seed
        lib.load()
        self.params = ParamStore(self.d, self.device, seed=seed, values=values, trainable_fn=is_trainable, weight_reg_fn=in_weight_reg)
        tr = hp.Taco1_Mel_to_Spect.Train
        self.wr_rate = tr.Weight_Regularization_Rate if wr_rate is None else wr_rate
        self.adam = adam or (tr.ADAM.Beta1, tr.ADAM.Beta2, tr.ADAM.Epsilon)
        self.global_step = 0
        self.flip = {}
        self._plans = {}          # workspace sets keyed by batch shape, least recently used first (at most MAX_PLANS kept)

    # ------------------------------------------------------------------ buffers
    def plan(self, B, S):
        return self._cached_plan((B, S), self._new_plan)

    def _new_plan(self, B, S):
        d, f = self.d, self._f
        w = Workspace()
        w.B, w.S = B, S
        rows, C1, Hh = B * S, d.bank_k * d.bank_ch, d.birnn
        w.bank_a = [f(rows, d.bank_ch) for _ in range(d.bank_k)]
        w.bank_mean = [f(d.bank_ch) for _ in range(d.bank_k)]; w.bank_rstd = [f(d.bank_ch) for _ in range(d.bank_k)]
        w.cat, w.pool = f(rows, C1), f(rows, C1)
        w.p1_a, w.p1_y, w.p1_mean, w.p1_rstd = f(rows, d.proj1_ch), f(rows, d.proj1_ch), f(d.proj1_ch), f(d.proj1_ch)
        w.p2_a, w.p2_y, w.p2_mean, w.p2_rstd = f(rows, d.n_mel), f(rows, d.n_mel), f(d.n_mel), f(d.n_mel)
        w.hx = [f(rows, d.n_mel) for _ in range(d.highway_n + 1)]
        w.hh = [f(rows, d.n_mel) for _ in range(d.highway_n)]; w.ht = [f(rows, d.n_mel) for _ in range(d.highway_n)]
        w.xw = {dr: f(rows, 4 * Hh) for dr in ("fw", "bw")}
        w.c = {dr: f(S + 1, B, Hh) for dr in ("fw", "bw")}; w.h = {dr: f(S + 1, B, Hh) for dr in ("fw", "bw")}
        w.acts = {dr: f(S, B, 4 * Hh) for dr in ("fw", "bw")}; w.craw = {dr: f(S, B, Hh) for dr in ("fw", "bw")}
        w.zc = {dr: torch.zeros(S * B * Hh, dtype=torch.uint8, device=self.device) for dr in ("fw", "bw")}
        w.zh = {dr: torch.zeros(S * B * Hh, dtype=torch.uint8, device=self.device) for dr in ("fw", "bw")}
        lb = lib.load()
        w.gates = f(int(lb.mstts_lstm_seq_ws_floats(B, Hh, 0)))
        w.bwd_ws = {dr: f(int(lb.mstts_lstm_seq_ws_floats(B, Hh, 1))) for dr in ("fw", "bw")}
        # fused cell steps (one launch per step for both directions): packed recurrent kernels + packed h blocks
        w.fused = bool(lb.mstts_cell_fwd_supported(Hh, Hh))
        if w.fused:
            w.whp = {dr: f(Hh * 4 * Hh) for dr in ("fw", "bw")}
            w.hp = {dr: f(2 * int(lb.mstts_cell_act_floats(B, Hh))) for dr in ("fw", "bw")}
        w.rnn = f(rows, 2 * Hh)
        w.pred, w.d_pred = f(rows, d.n_spec), f(rows, d.n_spec)
        w.lengths = torch.full((B,), S, dtype=torch.int32, device=self.device)
        w.bn_ws = f(4 * max(C1, d.proj1_ch, d.n_mel, d.bank_ch) + 64)
        w.scalars = f(4)
        # backward
        w.d_rnn = f(rows, 2 * Hh)
        w.dgs = {dr: f(S, B, 4 * Hh) for dr in ("fw", "bw")}; w.dgp = {dr: f(B, S, 4 * Hh) for dr in ("fw", "bw")}
        w.dx = [f(rows, d.n_mel) for _ in range(2)]
        w.dh, w.dt = f(rows, d.n_mel), f(rows, d.n_mel)
        w.d_p1y, w.d_pool, w.d_cat = f(rows, d.proj1_ch), f(rows, C1), f(rows, C1)
        w.dz_big = f(rows, max(d.proj1_ch, d.bank_ch, d.n_mel))
        w.d_bank, w.d_mel = f(rows, d.bank_ch), f(rows, d.n_mel)
        return w

    # ------------------------------------------------------------------ forward
    def forward(self, mel, w, seed=None, masks=None):
        """mel [B,S,n_mel] device tensor -> w.pred [B*S, n_spec]; saves what the backward needs."""
        d = self.d
        B, S = w.B, w.S
        rows, C1, Hh = B * S, d.bank_k * d.bank_ch, d.birnn
        self._w = w
        w.mel = mel
        if masks is not None:
            for dr in ("fw", "bw"):
                w.zc[dr].copy_(torch.as_tensor(np.asarray(masks["v_zc_" + dr], np.uint8)).reshape(-1))
                w.zh[dr].copy_(torch.as_tensor(np.asarray(masks["v_zh_" + dr], np.uint8)).reshape(-1))
        else:
            sd = seed if seed is not None else step_seed(self.seed, self.global_step)
            for i, dr in enumerate(("fw", "bw")):
                call("mstts_philox_keep_mask", ptr(w.zc[dr]), S * B * Hh, sd, 50 + 2 * i, 1 - d.zoneout)
                call("mstts_philox_keep_mask", ptr(w.zh[dr]), S * B * Hh, sd, 51 + 2 * i, 1 - d.zoneout)
        for k in range(1, d.bank_k + 1):
            sfx = bank_suffix(k)
            conv_fwd(self, gemm, mel, rows, S, d.n_mel, d.bank_ch, k, VOC + "convbank_0/conv1d%s" % sfx, w.bank_a[k - 1], ACT_RELU)
            y = w.dz_big                                   # scratch for the normalised block before it is copied into the concat
            bn_train_fwd(self, VOC + "convbank_0/batch_normalization%s/" % sfx, w.bank_a[k - 1], y, w.bank_mean[k - 1], w.bank_rstd[k - 1], None, 1.0,
                         rows, d.bank_ch, w.bn_ws)
            call("mstts_copy2d", ptr(y), d.bank_ch, ptr(w.cat, (k - 1) * d.bank_ch), C1, rows, d.bank_ch, 0)
        call("mstts_maxpool2_same", ptr(w.cat), ptr(w.pool), B, S, C1)
        conv_fwd(self, gemm, w.pool, rows, S, C1, d.proj1_ch, d.proj1_k, VOC + "convbank_0/conv1d_8", w.p1_a, ACT_RELU)
        bn_train_fwd(self, VOC + "convbank_0/batch_normalization_8/", w.p1_a, w.p1_y, w.p1_mean, w.p1_rstd, None, 1.0, rows, d.proj1_ch, w.bn_ws)
        conv_fwd(self, gemm, w.p1_y, rows, S, d.proj1_ch, d.n_mel, d.proj2_k, VOC + "convbank_0/conv1d_9", w.p2_a, ACT_NONE)
        bn_train_fwd(self, VOC + "convbank_0/batch_normalization_9/", w.p2_a, w.p2_y, w.p2_mean, w.p2_rstd, None, 1.0, rows, d.n_mel, w.bn_ws)
        call("mstts_add", ptr(mel), ptr(w.p2_y), ptr(w.hx[0]), rows * d.n_mel)
        for i in range(d.highway_n):
            dense_fwd(self, gemm, w.hx[i], rows, d.n_mel, d.n_mel, VOC + "highway_%d/dense" % i, w.hh[i])
            dense_fwd(self, gemm, w.hx[i], rows, d.n_mel, d.n_mel, VOC + "highway_%d/dense_1" % i, w.ht[i])
            call("mstts_highway_combine", ptr(w.hh[i]), ptr(w.ht[i]), ptr(w.hx[i]), ptr(w.hx[i + 1]), rows * d.n_mel)
        x = w.hx[d.highway_n]
        seqs = []
        for di, dr in enumerate(("fw", "bw")):
            q = lstm_layer_fwd(self, gemm, BIRNN % dr, x, w.xw[dr], B, S, d.n_mel, Hh, w.lengths, di, d.zoneout, w.zc[dr], w.zh[dr],
                               (w.rnn, di * Hh), S * 2 * Hh, 2 * Hh, w.c[dr], w.h[dr], w.acts[dr], w.craw[dr], w.gates)
            if w.fused:
                call("mstts_pack_cell_fwd", q.wh, 4 * Hh, ptr(w.whp[dr]), Hh, Hh)
                q.wh_p, q.h_p = ptr(w.whp[dr]), ptr(w.hp[dr])
            seqs.append(q)
        call("mstts_lstm_seq_fwd_pair", C.byref(seqs[0]), C.byref(seqs[1]))     # both directions advance together
        dense_fwd(self, gemm, w.rnn, rows, 2 * Hh, d.n_spec, VOC + "dense", w.pred)
        return w.pred

    # ------------------------------------------------------------------ loss + backward
    def loss_and_backward(self, w, spectrogram):
        d = self.d
        B, S = w.B, w.S
        rows, C1, Hh = B * S, d.bank_k * d.bank_ch, d.birnn
        ps = self.params
        ps.grad.zero_()
        w.scalars.zero_()
        call("mstts_l1_loss_fwd_bwd", ptr(w.pred), ptr(spectrogram), rows * d.n_spec, ptr(w.scalars), ptr(w.d_pred))
        call("mstts_l2_loss_acc", ptr(ps.train), ptr(ps.wd_mask), ps.n_train, ptr(w.scalars, 1))
        # projection
        kk, ok = self.P(VOC + "dense/kernel"); gk, ogk = self.G(VOC + "dense/kernel"); gb, ogb = self.G(VOC + "dense/bias")
        gemm(w.rnn, w.d_pred, gk, 2 * Hh, d.n_spec, rows, 2 * Hh, d.n_spec, d.n_spec, trans_a=True, split_k=max(2, _split_k(2 * Hh, d.n_spec, rows)), c_off=ogk)
        call("mstts_colsum", ptr(w.d_pred), rows, d.n_spec, d.n_spec, ptr(gb, ogb), 1)
        gemm(w.d_pred, kk, w.d_rnn, rows, 2 * Hh, d.n_spec, d.n_spec, d.n_spec, 2 * Hh, trans_b=True, b_off=ok)
        # BiLSTM
        x_in = w.hx[d.highway_n]
        dy = w.dx[0]
        bseqs = []
        for di, dr in enumerate(("fw", "bw")):
            k, ok = self.P(BIRNN % dr + "kernel")
            bseqs.append(lstm_seq_bwd(B, S, Hh, (k, ok + d.n_mel * 4 * Hh), w.lengths, di, d.zoneout, w.zc[dr], w.zh[dr], (w.d_rnn, di * Hh),
                                      S * 2 * Hh, 2 * Hh, w.c[dr], w.acts[dr], w.craw[dr], w.dgs[dr], w.dgp[dr], w.bwd_ws[dr]))
        call("mstts_lstm_seq_bwd_pair", C.byref(bseqs[0]), C.byref(bseqs[1]))
        for di, dr in enumerate(("fw", "bw")):
            lstm_layer_grads(self, gemm, BIRNN % dr, x_in, w.h[dr], w.dgp[dr], w.dgs[dr], dy, rows, d.n_mel, Hh, dx_accumulate=di == 1)
        # highway (reverse)
        for i in range(d.highway_n - 1, -1, -1):
            pre = VOC + "highway_%d/" % i
            dxn = w.dx[1] if dy is w.dx[0] else w.dx[0]
            call("mstts_highway_combine_bwd", ptr(w.hh[i]), ptr(w.ht[i]), ptr(w.hx[i]), ptr(dy), ptr(w.dh), ptr(w.dt), ptr(dxn), rows * d.n_mel)
            for nm, dpre in (("dense", w.dh), ("dense_1", w.dt)):
                kk, ok = self.P(pre + nm + "/kernel"); gk, ogk = self.G(pre + nm + "/kernel"); gb, ogb = self.G(pre + nm + "/bias")
                gemm(w.hx[i], dpre, gk, d.n_mel, d.n_mel, rows, d.n_mel, d.n_mel, d.n_mel, trans_a=True,
                     split_k=max(2, _split_k(d.n_mel, d.n_mel, rows)), c_off=ogk)
                call("mstts_colsum", ptr(dpre), rows, d.n_mel, d.n_mel, ptr(gb, ogb), 1)
                gemm(dpre, kk, dxn, rows, d.n_mel, d.n_mel, d.n_mel, d.n_mel, d.n_mel, trans_b=True, accumulate=True, b_off=ok)
            dy = dxn
        # conv bank (the residual `inputs + new` sends dy to the mel input too; the mel is data here, so only the bank path matters)
        cb, ws = VOC + "convbank_0/", self._w.bn_ws
        conv_bn_bwd(self, gemm, cb + "conv1d_9", cb + "batch_normalization_9/", dy, w.p1_y, w.p2_a, w.p2_mean, w.p2_rstd, None, 1.0, ACT_NONE,
                    rows, S, d.proj1_ch, d.n_mel, d.proj2_k, w.dz_big, w.d_p1y, ws)
        conv_bn_bwd(self, gemm, cb + "conv1d_8", cb + "batch_normalization_8/", w.d_p1y, w.pool, w.p1_a, w.p1_mean, w.p1_rstd, None, 1.0, ACT_RELU,
                    rows, S, C1, d.proj1_ch, d.proj1_k, w.dz_big, w.d_pool, ws)
        call("mstts_maxpool2_same_bwd", ptr(w.cat), ptr(w.d_pool), ptr(w.d_cat), B, S, C1)
        for k in range(1, d.bank_k + 1):
            sfx = bank_suffix(k)
            call("mstts_copy2d", ptr(w.d_cat, (k - 1) * d.bank_ch), C1, ptr(w.d_bank), d.bank_ch, rows, d.bank_ch, 0)
            conv_bn_bwd(self, gemm, cb + "conv1d%s" % sfx, cb + "batch_normalization%s/" % sfx, w.d_bank, w.mel, w.bank_a[k - 1], w.bank_mean[k - 1],
                        w.bank_rstd[k - 1], None, 1.0, ACT_RELU, rows, S, d.n_mel, d.bank_ch, k, w.dz_big, None, ws)

    def adam_step(self, w=None):
        lr = learning_rate(self.global_step)
        self._adam(lr, wr_rate=self.wr_rate)
        return lr

    def scalars(self, w):
        s = w.scalars.detach().cpu().numpy()
        wr = float(s[1]) * self.wr_rate
        return {"Loss": float(s[0]) + wr, "L1_Loss": float(s[0]), "Weight_Regularization_Loss": wr}

    def train_step(self, mel, spectrogram, masks=None, seed=None):
        """mel [B,S,n_mel], spectrogram [B,S,n_spec] (device tensors, contiguous)."""
        B, S, _ = mel.shape
        w = self.plan(B, S)
        self.forward(mel, w, seed=seed, masks=masks)
        self.loss_and_backward(w, spectrogram)
        self.adam_step()
        return w
