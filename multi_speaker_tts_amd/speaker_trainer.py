"""Training step of the speaker encoder with the GE2E loss (reference: Speaker_Embedding/Speaker_Embedding.py:27-80,
Speaker_Embedding/Modules.py:6-98) on the MI355X: dense 80 -> 256, three ZoneoutLSTM(256) with residual wrappers on the first
two, the last frame l2-normalised per row, scaled-cosine softmax loss against leave-one-out / speaker centroids with trainable
(weight, bias) = (10, -5), plain TF-Adam (eps 1e-8; the gradient-clipped op of :62-66 is overwritten at :69-72 and never runs),
learning rate max(exponential_decay, Min).  Python owns buffers and the schedule; arithmetic is libmstts_hip.so
(mstts_gemm_f32, mstts_lstm_seq_fwd/bwd, mstts_ge2e_loss_fwd_bwd, mstts_adam_tf).  hp.Speaker_Embedding.Train.Loss_Calc_Method
"Contrast" (Modules.py:93-94) runs mstts_ge2e_contrast_fwd_bwd instead; anything but the two raises, as the reference does.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import lib
from .lib import call, gemm, ptr
from .masks import step_seed
from .params import SPK, SPK_CELL, Dims, ParamStore
from .persist import Ticket, lstm_bwd_workgroups, lstm_fwd_workgroups
from .training import Engine, Workspace, _split_k, dense_fwd, exponential_decay, lstm_layer_fwd, lstm_layer_grads, lstm_seq_bwd


def is_trainable(name):
    return name.startswith(SPK)


def learning_rate(step):
    """Speaker_Embedding.py:46-52."""
    from . import Hyper_Parameters as hp
    return exponential_decay(hp.Speaker_Embedding.Train.Learning_Rate, step)


LOSS_CALLS = {"SOFTMAX": "mstts_ge2e_loss_fwd_bwd", "CONTRAST": "mstts_ge2e_contrast_fwd_bwd"}


def loss_call(loss_method=None):
    """Entry point of a Loss_Calc_Method (None: hp.Speaker_Embedding.Train.Loss_Calc_Method), case-insensitive (Modules.py:88-96)."""
    from . import Hyper_Parameters as hp
    method = hp.Speaker_Embedding.Train.Loss_Calc_Method if loss_method is None else loss_method
    if str(method).upper() not in LOSS_CALLS:
        raise ValueError("Unsupported loss calc method")
    return LOSS_CALLS[str(method).upper()]


class SpeakerTrainEngine(Engine):
    def __init__(self, dims: Dims = None, device="cuda", seed=1234, values=None, adam=None, loss_method=None):
        from . import Hyper_Parameters as hp
        self.loss_call = loss_call(loss_method)
        self.d = dims or Dims()
        self.device = torch.device(device)
        self.seed = seed
        lib.load()
        self.params = ParamStore(self.d, self.device, seed=seed, values=values, trainable_fn=is_trainable, weight_reg_fn=lambda n: False)
        a = hp.Speaker_Embedding.Train.ADAM
        self.adam = adam or (a.Beta1, a.Beta2, a.Epsilon)
        # the loss's own variables 'loss/weight', 'loss/bias' (Modules.py:61-62) with their Adam slots: [w, b, pad, pad]
        self.wb = torch.tensor([10.0, -5.0, 0.0, 0.0], dtype=torch.float32, device=self.device)
        self.wb_m, self.wb_v = torch.zeros(4, device=self.device), torch.zeros(4, device=self.device)
        self.wb_mask = torch.zeros(4, dtype=torch.uint8, device=self.device)
        self.global_step = 0
        self._plans = {}          # workspace sets keyed by batch shape, least recently used first (at most MAX_PLANS kept)
        self._last = None         # the set of the last loss_and_backward (its out3 holds the loss variables' gradients)
        # persistent LSTM launches (csrc/persist_lstm.hip): all T steps of a layer in one launch each way; MSTTS_PERSIST_ENC=0 keeps the
        # launch-per-step loops, which are also the fallback
        self.persist_lstm = os.environ.get("MSTTS_PERSIST_ENC", "1") != "0"
        self.persist_lstm_fallbacks = 0

    def plan(self, N, T):
        return self._cached_plan((N, T), self._new_plan)

    def _new_plan(self, N, T):
        d, f = self.d, self._f
        H, L = d.spk_lstm, d.spk_lstm_n
        w = Workspace()
        w.N, w.T = N, T
        w.x = [f(N, T, d.spk) for _ in range(L + 1)]            # x[0] = dense output, x[l+1] = output of cell l
        w.xw = f(N * T, 4 * H)
        w.c = [f(T + 1, N, H) for _ in range(L)]; w.h = [f(T + 1, N, H) for _ in range(L)]
        w.acts = [f(T, N, 4 * H) for _ in range(L)]; w.craw = [f(T, N, H) for _ in range(L)]
        w.zc = [torch.zeros(T * N * H, dtype=torch.uint8, device=self.device) for _ in range(L)]
        w.zh = [torch.zeros(T * N * H, dtype=torch.uint8, device=self.device) for _ in range(L)]
        lb = lib.load()
        w.gates = f(int(lb.mstts_lstm_seq_ws_floats(N, H, 0))); w.bwd_ws = f(int(lb.mstts_lstm_seq_ws_floats(N, H, 1)))
        # fused cell steps (one launch per step): packed recurrent kernel + packed h blocks; the residual wrapper's sum (output = cell
        # output + input, state untouched) is then applied once per sequence
        w.fused = bool(lb.mstts_cell_fwd_supported(H, H)) and d.spk == H
        if w.fused:
            w.whp, w.hp, w.y = f(H * 4 * H), f(2 * int(lb.mstts_cell_act_floats(N, H))), f(N, T, H)
        w.lengths = torch.full((N,), T, dtype=torch.int32, device=self.device)
        # (the persistent launches take no residual input: they need the fused form's "one add per sequence afterwards")
        w.persist = self.persist_lstm and w.fused and bool(lb.mstts_persist_lstm_supported_n(N, H, 1))
        if w.persist:
            n = int(lb.mstts_persist_lstm_pack_floats())
            w.pk = [(f(n), f(n)) for _ in range(L)]                                   # (forward order, BPTT order) per layer, refreshed per step
            w.pxch = f(int(lb.mstts_persist_lstm_ws_bytes_n(N, 1)) // 4)
            w.pctrl = torch.zeros(16, dtype=torch.int32, device=self.device)
            w.pctrl_host = torch.zeros(16, dtype=torch.int32).pin_memory()
            w.phist = [f(int(lb.mstts_persist_lstm_hist_floats_n(T, N, 1))) for _ in range(L)]   # packed history per layer (the BPTT reads it)
            w.pbws = f(int(lb.mstts_persist_lstm_bwd_floats_n(T, N, 1)))
            w.phist_valid = [False] * L
        w.loss_ws = f(int(lb.mstts_ge2e_ws_floats(N, d.spk, 256)))
        w.out3 = f(4)
        w.d_out = f(N, T, d.spk)                                # gradient of a cell's output sequence
        w.d_in = f(N, T, d.spk)
        w.dgs, w.dgp = f(T, N, 4 * H), f(N, T, 4 * H)
        return w

    def forward(self, mel, w, seed=None, masks=None):
        """mel [N,T,n_mel] -> w.x[-1] [N,T,spk] (training mode: Philox or injected zoneout masks)."""
        d = self.d
        N, T, H = w.N, w.T, d.spk_lstm
        w.mel = mel
        for i in range(d.spk_lstm_n):
            if masks is not None:
                w.zc[i].copy_(torch.as_tensor(np.asarray(masks["s_zc_%d" % i], np.uint8)).reshape(-1))
                w.zh[i].copy_(torch.as_tensor(np.asarray(masks["s_zh_%d" % i], np.uint8)).reshape(-1))
            else:
                sd = seed if seed is not None else step_seed(self.seed, self.global_step)
                call("mstts_philox_keep_mask", ptr(w.zc[i]), T * N * H, sd, 60 + 2 * i, 1 - d.zoneout)
                call("mstts_philox_keep_mask", ptr(w.zh[i]), T * N * H, sd, 61 + 2 * i, 1 - d.zoneout)
        dense_fwd(self, gemm, mel, N * T, d.n_mel, d.spk, SPK + "dense", w.x[0])
        for i in range(d.spk_lstm_n):
            cell, res = SPK_CELL % (i, i), i < d.spk_lstm_n - 1
            q = lstm_layer_fwd(self, gemm, cell, w.x[i], w.xw, N, T, d.spk, H, w.lengths, 0, d.zoneout, w.zc[i], w.zh[i],
                               (w.y if (res and w.fused) else w.x[i + 1], 0), T * H, H, w.c[i], w.h[i], w.acts[i], w.craw[i], w.gates,
                               residual=w.x[i] if (res and not w.fused) else None)
            done = False
            if getattr(w, "persist", False):
                call("mstts_persist_lstm_pack", q.wh, 4 * H, ptr(w.pk[i][0]), ptr(w.pk[i][1]))
                call("mstts_lstm_seq_fwd_persistent", C.byref(q), ptr(w.pk[i][0]), ptr(w.pxch), ptr(w.pctrl), ptr(w.phist[i]))
                done = w.phist_valid[i] = self._persist_ok(w, lstm_fwd_workgroups(N, H, 1))
            if not done:
                if w.fused:
                    call("mstts_pack_cell_fwd", q.wh, 4 * H, ptr(w.whp), H, H)
                    q.wh_p, q.h_p = ptr(w.whp), ptr(w.hp)
                call("mstts_lstm_seq_fwd", C.byref(q))
            if res and w.fused:
                call("mstts_add", ptr(w.y), ptr(w.x[i]), ptr(w.x[i + 1]), N * T * H)
        return w.x[-1]

    def _persist_ok(self, w, n_wg):
        """Control words of the persistent launch just enqueued: True when it ran to its end (else the caller runs the launch-per-step loop)."""
        ticket = Ticket(w.pctrl, w.pctrl_host, n_wg).enqueue()
        torch.cuda.current_stream().synchronize()
        ok, _ = ticket.redeem()
        if not ok:
            self.persist_lstm_fallbacks += 1
        return ok

    def loss_and_backward(self, w, batch_per_speaker):
        d = self.d
        N, T, H, Dm = w.N, w.T, d.spk_lstm, d.spk
        P_ = batch_per_speaker
        S = N // P_
        assert S * P_ == N
        self.params.grad.zero_()
        w.d_out.zero_()
        # loss on the last frame; its gradient lands in the last time row of d_out
        last = (T - 1) * Dm
        call(self.loss_call, ptr(w.x[-1], last), T * Dm, S, P_, Dm, ptr(self.wb), ptr(w.out3), ptr(w.d_out, last), T * Dm, ptr(w.loss_ws))
        d_out = w.d_out
        for i in range(d.spk_lstm_n - 1, -1, -1):
            k, ok = self.P(SPK_CELL % (i, i) + "kernel")
            q = lstm_seq_bwd(N, T, H, (k, ok + Dm * 4 * H), w.lengths, 0, d.zoneout, w.zc[i], w.zh[i], (d_out, 0), T * H, H,
                             w.c[i], w.acts[i], w.craw[i], w.dgs, w.dgp, w.bwd_ws)
            done = False
            if getattr(w, "persist", False) and w.phist_valid[i]:       # (the persistent BPTT reads the packed history of a persistent forward)
                call("mstts_lstm_seq_bwd_persistent", C.byref(q), ptr(w.pk[i][1]), ptr(w.pxch), ptr(w.pctrl), ptr(w.phist[i]), ptr(w.pbws))
                done = self._persist_ok(w, lstm_bwd_workgroups(N, 1))
            if not done:
                call("mstts_lstm_seq_bwd", C.byref(q))
            d_in = w.d_in if d_out is w.d_out else w.d_out
            lstm_layer_grads(self, gemm, SPK_CELL % (i, i), w.x[i], w.h[i], w.dgp, w.dgs, d_in, N * T, Dm, H)
            if i < d.spk_lstm_n - 1:                             # ResidualWrapper: the output gradient also reaches the input
                call("mstts_add", ptr(d_in), ptr(d_out), ptr(d_in), N * T * Dm)
            d_out = d_in
        gk, ogk = self.G(SPK + "dense/kernel"); gb, ogb = self.G(SPK + "dense/bias")
        gemm(w.mel, d_out, gk, d.n_mel, Dm, N * T, d.n_mel, Dm, Dm, trans_a=True, split_k=max(2, _split_k(d.n_mel, Dm, N * T)), c_off=ogk)
        call("mstts_colsum", ptr(d_out), N * T, Dm, Dm, ptr(gb, ogb), 1)
        self._last = w

    def adam_step(self, w=None):
        w = w or self._last
        lr = learning_rate(self.global_step)
        rate = self._adam(lr)
        # the loss's (weight, bias) at the same bias-corrected rate: gradients sit in out3[1:3]
        b1, b2, eps = self.adam
        call("mstts_adam_tf", ptr(self.wb), ptr(w.out3, 1), ptr(self.wb_m), ptr(self.wb_v), ptr(self.wb_mask), 0.0, 1.0, float(rate), b1, b2, eps, 2)
        return lr

    def train_step(self, mel, batch_per_speaker, masks=None, seed=None):
        N, T, _ = mel.shape
        w = self.plan(N, T)
        self.forward(mel, w, seed=seed, masks=masks)
        self.loss_and_backward(w, batch_per_speaker)
        self.adam_step(w)
        return w
