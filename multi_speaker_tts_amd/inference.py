"""Inference forward of the Tacotron2 graph (Tacotron2.Inference_Mel_to_Spectrogram's Session.run,
MSTTS_SV.py:301-308) as a schedule of libmstts_hip.so calls:

  speaker encoder (Speaker_Embedding/Modules.py:6-37,127-137) -> encoder in inference mode
  (Modules.py:15-73: BN moving statistics, no dropout, deterministic zoneout) -> memory/keys ->
  free-running attention decoder with stop-token gating (Modules.py:212-237; native loop driver) ->
  postnet + residual (Modules.py:121-143) -> Taco1 mel->spectrogram (Taco1_Mel_to_Spect/Modules.py:8-105).

Prenet dropout stays active (quirk Q9): its keep-masks are Philox streams, or injected for tests.
"""
from __future__ import annotations

import ctypes as C
import os
import time
import warnings

import numpy as np
import torch

from . import lib
from .lib import ACT_NONE, ACT_RELU, ACT_TANH, gemm, ptr, call
from .masks import MaskSet, step_seed
from .params import CELL, ENC_CELL, LSA, SPK, SPK_CELL, VOC, VOC_CELL, Dims, ParamStore, bank_suffix
from .persist import LAST_STEP, PERSIST_COOLDOWN, PERSIST_STRIKES, ROWS_FINISHED, CoolDown, Ticket, decoder_workgroups, lstm_fwd_workgroups, near_xcd
from .training import bn_infer_fwd, conv_fwd, dense_fwd, lstm_seq_fwd
SPK_OVERLAP = os.environ.get("MSTTS_SPK_OVERLAP", "1") != "0"     # inference forward: the speaker stack on its own stream beside the text encoder


class _PersistRetry(RuntimeError):
    pass


def to_host(tensors):
    """{name: device tensor} -> {name: numpy array}: every tensor copied asynchronously into its own page-locked host block, ONE synchronisation, the
    arrays are views of those blocks (each array owns its block; torch's caching host allocator hands the block out again once the array is
    dropped, so only the first call pays for pinning).  33.8 MB of results of a batch-16 forward: 2.7 ms through `.cpu()` (a pageable destination,
    12.7 GB/s) against 0.9 ms this way."""
    host = {}
    for k, v in tensors.items():
        v = v.detach()
        h = torch.empty(v.shape, dtype=v.dtype, pin_memory=True)
        h.copy_(v, non_blocking=True)
        host[k] = h
    torch.cuda.synchronize()
    return {k: h.numpy() for k, h in host.items()}


class _DeferredCheck:
    """Ticket of a sub-graph whose persistent LSTM launches have not been checked yet (InferEngine.speaker_embedding(defer=True))."""

    def __init__(self, eng, fn, a, k, ticket):
        self.eng, self.fn, self.a, self.k, self.ticket, self.pending, self.host = eng, fn, a, k, ticket, ticket.expect, ticket.host

    def ok(self):
        """After (or as) the caller's host sync: did every launch of the sub-graph run to its end?  The ticket owns its page-locked read-back
        block (a second deferred call before this one is redeemed - batch prefetch - reads back into ANOTHER block); it goes back to the
        engine's pool here."""
        eng, host = self.eng, self.host
        if host is None:
            raise RuntimeError("a deferred check is redeemed once")
        good, _ = self.ticket.redeem()
        self.host = None
        eng._deferred_host_pool.append(host)
        if eng.persist_lstm_selftest > 0:
            eng.persist_lstm_selftest -= 1
            return False
        return good

    def redo(self):
        """The sub-graph again, launch by launch (same stream); returns its output."""
        with lib.deterministic_gemm():
            return self.eng._launch_by_launch(self.fn, *self.a, **self.k)


class InferEngine:
    def __init__(self, dims: Dims = None, device="cuda", seed=1234, params: ParamStore = None, values=None, chunk=50):
        lib.load()
        self.d = dims or Dims()
        self.device = torch.device(device)
        self.seed = seed
        self.params = params if params is not None else ParamStore(self.d, self.device, seed=seed, values=values)
        self.chunk = chunk
        self._keep = []          # keeps temporaries alive until the stream is synchronised
        # persistent launches (csrc/persist_infer.hip, persist_lstm.hip): MSTTS_PERSIST_INFER=0 keeps the launch-per-step drivers
        self.persist_infer = os.environ.get("MSTTS_PERSIST_INFER", "1") != "0"
        self.persist_infer_launches = 0      # decoder loops that ran as one launch
        self.persist_infer_fallbacks = 0     # ... that gave up (bounded waits / no co-residency) and were re-run launch by launch
        self.persist_infer_selftest = 0      # tests: k > 0 makes the launch abort at step k - 1
        self.persist_infer_stamps = None     # bench: 256 x 24 int64 tensor -> per-stage ticks of the next launch
        self.persist_infer_status = None
        self._persist_cool = CoolDown()      # PERSIST_STRIKES consecutive fallbacks switch the launch off for PERSIST_COOLDOWN decodes
        self.persist_disabled_decodes = 0
        self.non_persistent_decodes = 0      # decodes at the reference widths whose shape the persistent loop does not cover
        self._warned_shapes = set()
        # recurrent layers around the decoder (encoder BiLSTM, speaker-encoder stack: H = 256; Taco1 BiRNN: H = 128) as ONE persistent launch per
        # layer (csrc/persist_lstm.hip) instead of a launch per step; their control words are read at the forward pass's existing sync points
        self.persist_lstm = os.environ.get("MSTTS_PERSIST_LSTM", "1") != "0"
        self.persist_lstm_launches = 0
        self.persist_lstm_fallbacks = 0      # forward passes re-run without them because a launch gave up
        self.persist_lstm_selftest = 0       # tests: k > 0 makes the next k control-word checks report a launch that gave up
        self._lstm_retry = False
        self._lstm_pending = []              # (slot, workgroups expected to have left in order)
        self._lstm_ctrl = None
        self._spk_stream = None
        self._lstm_ctrl_host = None
        self._lstm_ticket = None             # read-back of the launches pending so far, once enqueued
        self._derived = {}                   # operands derived from the variables, by key: (ParamStore.version they were built at, buffers)

    # ------------------------------------------------------------------ helpers
    def _buf(self, *shape, zero=True):
        """fp32 buffer of `shape` (whole float4s) that the caller holds; zero=False: uninitialised, for what its first user overwrites."""
        n = int(np.prod(shape))
        return (torch.zeros if zero else torch.empty)((n + 3) // 4 * 4, dtype=torch.float32, device=self.device)[:n].view(shape)

    def _f(self, *shape):
        t = self._buf(*shape)
        self._keep.append(t)
        return t

    def P(self, name):
        return self.params.p(name)

    def _derived_at_version(self, key, alloc, fill):
        """The operands derived from the variables kept under `key` (packed, folded, padded kernels): alloc() makes their buffers at the first
        use, fill(buffers) forms them then and again, into the same buffers, whenever ParamStore.version has moved (a load, an Adam step)."""
        ent = self._derived.get(key)
        if ent is None or ent[0] != self.params.version:
            bufs = alloc() if ent is None else ent[1]
            fill(bufs)
            self._derived[key] = ent = (self.params.version, bufs)
        return ent[1]

    def _lstm_seq_desc(self, x, B, T, cin, H, cell_prefix, out, out_sb, out_st, out_off=0, lengths=None, reverse=0, residual=None, zc=None, zh=None, fused=True):
        """Descriptor of one ZoneoutLSTMCell over a sequence: inference mode without masks (0.9*new + 0.1*old), training-mode zoneout
        with keep-masks zc / zh [T, B, H] (ZoneoutLSTMCell.py:259-271).  Where the fused cell step covers the shape (no residual) the
        packed recurrent kernel and packed h blocks are attached, so every step is one launch."""
        # (not training.lstm_layer_fwd: the scratch below is made BEHIND the gate product, so that its zero fills are enqueued while the product
        #  runs - the host paces these launch chains, and in front of it they cost the product's ~10 us per layer)
        k, ok = self.P(cell_prefix + "kernel"); b, ob = self.P(cell_prefix + "bias")
        xw = self._f(B * T, 4 * H)
        gemm(x, k, xw, B * T, 4 * H, cin, cin, 4 * H, 4 * H, bias=b, b_off=ok, bias_off=ob)
        if reverse and lengths is None:            # tf.reverse_sequence over the full length
            lengths = torch.full((B,), T, dtype=torch.int32, device=self.device)
            self._keep.append(lengths)
        L_ = lib.load()
        q = lstm_seq_fwd(B, T, H, cin, xw, (k, ok), lengths, reverse, self.d.zoneout, zc, zh, (out, out_off), out_sb, out_st,
                         self._f(T + 1, B, H), self._f(T + 1, B, H), None, None, self._f(int(L_.mstts_lstm_seq_ws_floats(B, H, 0))),
                         residual=residual)
        if fused and residual is None and L_.mstts_cell_fwd_supported(H, H):
            whp = self._f(H * 4 * H)             # (packed per call: the parameters may have been reloaded in between; 1 small launch)
            call("mstts_pack_cell_fwd", q.wh, 4 * H, ptr(whp), H, H)
            q.wh_p, q.h_p = ptr(whp), ptr(self._f(2 * int(L_.mstts_cell_act_floats(B, H))))
        return q

    # ---- persistent recurrent layers
    def _lstm_persist_args(self, ndir, B, T, H):
        """Ring, a fresh control-word slot and history scratch for one persistent LSTM launch over ndir directions; None when the shape /
        device is not covered or this forward pass is a retry without them."""
        L_ = lib.load()
        if not self.persist_lstm or self._lstm_retry or not L_.mstts_persist_lstm_fwd_supported_n(B, H, ndir):
            return None
        if self._lstm_ctrl is None:
            self._lstm_ctrl = torch.zeros(64, 16, dtype=torch.int32, device=self.device)
            self._lstm_ctrl_host = torch.zeros(64, 16, dtype=torch.int32).pin_memory()
        if len(self._lstm_pending) >= 64:
            return None
        xch = self._buf(L_.mstts_persist_lstm_ws_bytes_n(B, ndir) // 4, zero=False)
        hist = self._buf(L_.mstts_persist_lstm_hist_floats_n(T, B, ndir), zero=False)
        self._keep.extend((xch, hist))
        slot = len(self._lstm_pending)
        self._lstm_pending.append((slot, lstm_fwd_workgroups(B, H, ndir)))
        self.persist_lstm_launches += 1
        return ptr(xch), ptr(self._lstm_ctrl, slot * 16), ptr(hist)

    def _lstm_packed(self, cell_prefix, q):
        """The cell's recurrent kernel q.wh in a persistent LSTM launch's order, kept until the variables change."""
        return ptr(self._derived_at_version(cell_prefix, lambda: self._buf(q.H * 4 * q.H, zero=False),
                                            lambda pk: call("mstts_persist_lstm_pack_fwd", q.wh, 4 * q.H, q.H, ptr(pk))))

    def _lstm_ctrl_copy(self):
        """Enqueue the read-back of the control words of the persistent LSTM launches so far (call in front of a host sync)."""
        if len(self._lstm_pending) > (len(self._lstm_ticket.expect) if self._lstm_ticket is not None else 0):
            self._lstm_ticket = Ticket(self._lstm_ctrl, self._lstm_ctrl_host, list(self._lstm_pending)).enqueue()

    def _lstm_verify(self):
        """After a host sync: did every persistent LSTM launch read back so far run to its end?  Raises _PersistRetry otherwise (the
        forward pass is then re-run with the launch-per-step drivers)."""
        ticket = self._lstm_ticket
        if self.persist_lstm_selftest > 0 and ticket is not None:
            self.persist_lstm_selftest -= 1
            raise _PersistRetry("persistent LSTM launch 0: self-test")
        ok, status = ticket.redeem() if ticket is not None else (True, ())
        if not ok:
            raise _PersistRetry("persistent LSTM launch %d: control words %r" % (ticket.failed, list(status)))

    def _lstm_seq(self, x, B, T, cin, H, cell_prefix, out, out_sb, out_st, out_off=0, residual=None, **kw):
        # residual wrapper (output = cell output + input, state untouched): with a dense [B, T, H] output the fused steps run without it
        # and one add over the whole sequence follows - the same fp32 sum, 2 launches per step less
        post_add = (residual is not None and out_off == 0 and out_st == H and out_sb == T * H and
                    bool(lib.load().mstts_cell_fwd_supported(H, H)))
        dst = self._f(B, T, H) if post_add else out
        pa = self._lstm_persist_args(1, B, T, H) if (residual is None or post_add) else None
        q = self._lstm_seq_desc(x, B, T, cin, H, cell_prefix, dst, out_sb, out_st, out_off=out_off, residual=None if post_add else residual,
                                fused=pa is None, **kw)
        if pa is not None:
            call("mstts_lstm_seq_fwd_persistent", C.byref(q), self._lstm_packed(cell_prefix, q), *pa)
        else:
            call("mstts_lstm_seq_fwd", C.byref(q))
        if post_add:
            call("mstts_add", ptr(dst), ptr(residual), ptr(out), B * T * H)

    def _bilstm_seq(self, x, B, T, cin, H, cell_fmt, out, out_sb, out_st, lengths=None):
        """Forward and backward direction of a bidirectional layer advancing together: one launch per step where the fused form applies
        (mstts_lstm_seq_fwd_pair falls back to two sequential loops otherwise)."""
        pa = self._lstm_persist_args(2, B, T, H)
        qs = [self._lstm_seq_desc(x, B, T, cin, H, cell_fmt % dr, out, out_sb, out_st, out_off=di * H, lengths=lengths, reverse=di, fused=pa is None)
              for di, dr in enumerate(("fw", "bw"))]
        if pa is not None:
            call("mstts_lstm_seq_fwd_pair_persistent", C.byref(qs[0]), C.byref(qs[1]), self._lstm_packed(cell_fmt % "fw", qs[0]),
                 self._lstm_packed(cell_fmt % "bw", qs[1]), *pa)
        else:
            call("mstts_lstm_seq_fwd_pair", C.byref(qs[0]), C.byref(qs[1]))

    # ------------------------------------------------------------------ sub-graphs
    @lib.deterministic_gemm()
    def _guarded(self, fn, *a, **k):
        """A sub-graph called on its own (outside forward): the control words of its persistent LSTM launches are checked before its
        result is handed out (one stream sync), and the sub-graph is re-run launch by launch if one of them gave up."""
        self._lstm_pending, self._lstm_ticket = [], None
        try:
            out = fn(*a, **k)
            if self._lstm_pending:
                self._lstm_ctrl_copy()
                torch.cuda.current_stream().synchronize()
                self._lstm_verify()
            return out
        except _PersistRetry as e:
            warnings.warn("multi_speaker_tts_amd: %s; re-running launch by launch" % (e,), RuntimeWarning, stacklevel=3)
            return self._launch_by_launch(fn, *a, **k)

    def _launch_by_launch(self, fn, *a, **k):
        """fn again (same stream) with the launch-per-step LSTM drivers, after a persistent launch of its sub-graph gave up."""
        self.persist_lstm_fallbacks += 1
        self._lstm_retry = True
        try:
            return fn(*a, **k)
        finally:
            self._lstm_retry = False
            self._lstm_pending, self._lstm_ticket = [], None

    def speaker_embedding(self, spk_mel, masks=None, defer=False):
        """defer=True (the TRAIN step's frozen speaker stack, MSTTS_SV.py:49-56,211): no host sync here.  Returns (embedding, ticket);
        the caller hands the ticket to TrainEngine.forward (batch["_speaker_ticket"]), which redeems it at its one existing sync point and
        re-runs the sub-graph launch by launch - and its own pass - if a persistent launch of the stack gave up."""
        if not defer:
            return self._guarded(self._speaker_embedding, spk_mel, masks=masks)
        return self._deferred(self._speaker_embedding, spk_mel, masks=masks)

    @lib.deterministic_gemm()
    def _deferred(self, fn, *a, **k):
        self._lstm_pending, self._lstm_ticket = [], None
        out = fn(*a, **k)
        pending = list(self._lstm_pending)
        if not pending:
            return out, None
        # one page-locked read-back block PER TICKET (pooled: page-locking is a system call): the copy below is ordered behind this call's launches
        # and in front of the next call's, which reuse the device slots from 0 - tickets may be outstanding together
        pool = self.__dict__.setdefault("_deferred_host_pool", [])
        host = pool.pop() if pool else torch.zeros(64, 16, dtype=torch.int32).pin_memory()
        return out, _DeferredCheck(self, fn, a, k, Ticket(self._lstm_ctrl, host, pending).enqueue(torch.cuda.Event()))

    def encoder(self, token, token_length, spk):
        return self._guarded(self._encoder, token, token_length, spk)

    def mel_to_spectrogram(self, mel, B, S):
        return self._guarded(self._mel_to_spectrogram, mel, B, S)

    def _speaker_embedding(self, spk_mel, masks=None):
        """[5B,64,80] float32 device tensor -> [B, spk] (MSTTS_SV.py:49-56).  masks: optional {'s_zc_<i>', 's_zh_<i>'} uint8
        keep-masks [64, 5B, cell] - the reference feeds Is_Training into this (frozen) stack too, so a Tacotron2 TRAIN step sees
        stochastic zoneout in the speaker encoder (MSTTS_SV.py:49-56, ZoneoutLSTMCell.py:259-260)."""
        d = self.d
        NB, T, _ = spk_mel.shape
        B = NB // d.spk_samples
        x = self._f(NB * T, d.spk)
        dense_fwd(self, gemm, spk_mel, NB * T, d.n_mel, d.spk, SPK + "dense", x)
        for i in range(d.spk_lstm_n):
            y = self._f(NB, T, d.spk_lstm)
            self._lstm_seq(x, NB, T, d.spk, d.spk_lstm, SPK_CELL % (i, i), y, T * d.spk_lstm, d.spk_lstm,
                           residual=x if i < d.spk_lstm_n - 1 else None,
                           zc=masks["s_zc_%d" % i] if masks is not None else None, zh=masks["s_zh_%d" % i] if masks is not None else None)
            x = y
        e = self._f(B, d.spk)
        call("mstts_speaker_finalize", ptr(x), ptr(e), B, d.spk_samples, T, d.spk)
        return e

    def _encoder(self, token, token_length, spk, spk_done=None):
        """-> values [B,T,M] (memory masked past Token_Length), keys [B,T,A].  spk_done: event behind the speaker embedding when another stream forms it."""
        d = self.d
        B, T = token.shape
        M, He = d.mem, d.enc_lstm
        emb, oe = self.P("encoder/embedding_variable")
        x = self._f(B * T, d.emb)
        call("mstts_embedding_fwd", ptr(token), ptr(emb, oe), ptr(x), B * T, d.n_tok, d.emb)
        cin = d.emb
        for i in range(d.enc_conv_n):
            a = self._f(B * T, d.enc_conv_ch)
            conv_fwd(self, gemm, x, B * T, T, cin, d.enc_conv_ch, d.enc_conv_k, "encoder/conv_%d/conv1d" % i, a, ACT_RELU)
            x = self._f(B * T, d.enc_conv_ch)
            bn_infer_fwd(self, "encoder/conv_%d/batch_normalization/" % i, a, x, B * T, d.enc_conv_ch)
            cin = d.enc_conv_ch
        values = self._f(B, T, M)
        self._bilstm_seq(x, B, T, cin, He, ENC_CELL, values, T * M, M, lengths=token_length)
        if spk_done is not None:
            torch.cuda.current_stream().wait_event(spk_done)
        call("mstts_speaker_tile", ptr(spk), ptr(token_length), ptr(values), B, T, M, 2 * He, d.spk)
        keys = self._f(B, T, d.att)
        dense_fwd(self, gemm, values, B * T, M, d.att, "attention/memory_layer", keys, bias=False)
        return values, keys

    @lib.deterministic_gemm()
    def decode(self, values, keys, token_length, masks=None, seed=None, max_steps=None):
        """Free-running decoder.  Returns step-major linear [S,B,n_mel], stop logits [S,B], align [S,B,T]."""
        d = self.d
        B, T, M = values.shape
        H, A, Pn, NM = d.dec_lstm, d.att, d.prenet, d.n_mel
        Smax = (max_steps if max_steps is not None else d.max_inf) + 1
        mk = MaskSet(d, B, T, Smax, False, self.device)
        if masks is not None:
            mk.load(masks)
        else:
            mk.draw(seed if seed is not None else step_seed(self.seed, 0))
        self._keep.append(mk)
        k0, o0 = self.P(CELL % 0 + "kernel"); b0, ob0 = self.P(CELL % 0 + "bias")
        wpj, owpj = self.P("decoder/decoder/linear_projection/dense/kernel")
        npad = (NM + 1 + 3) // 4 * 4
        # variable-derived operands shared by both drivers: cell-0 kernel with its two context row blocks folded, the folded
        # location filter, the projection kernel in rows of whole float4s (the padding zero)
        def fold(c):
            call("mstts_fold_rows", ptr(k0, o0 + Pn * 4 * H), ptr(c["w0f"]), 2 * M + H, 4 * H, 0, M)
            lib.lsa_fold(self.P, c["loc_k"], c["loc_b"], c["loc_kt"], d.att_k, d.att_ch, A)
            call("mstts_copy2d", ptr(wpj, owpj), NM + 1, ptr(c["wp_pad"]), npad, H + M, NM + 1, 0)
        c = self._derived_at_version("decoder", lambda: dict(w0f=self._buf(M + H, 4 * H), loc_k=self._buf(d.att_k, A), loc_b=self._buf(A),
                                                             loc_kt=self._buf(A, 36) if d.att_k <= 31 else None,
                                                             wp_pad=self._buf(H + M, npad)), fold)
        w0f, self._dec = c["w0f"], dict(c, vp=None)          # (what the drivers of this call read beside their arguments)
        q = lib.DecoderInfer()
        q.B, q.H, q.P, q.n_mel, q.Smax = B, H, Pn, NM, Smax
        lib.lsa_fill(q.lsa, self.P, B, T, A, M, d.att_k, d.att_ch, keys, values, token_length, c["loc_k"], c["loc_b"], c["loc_kt"])
        for field, name in (("pw0", "decoder/decoder/prenet_0/dense/kernel"), ("pb0", "decoder/decoder/prenet_0/dense/bias"),
                            ("pw1", "decoder/decoder/prenet_1/dense/kernel"), ("pb1", "decoder/decoder/prenet_1/dense/bias"),
                            ("w1", CELL % 1 + "kernel"), ("b1", CELL % 1 + "bias"), ("wq", LSA + "query_layer/kernel"),
                            ("wproj", "decoder/decoder/linear_projection/dense/kernel"), ("bproj", "decoder/decoder/linear_projection/dense/bias")):
            t, o = self.P(name)
            setattr(q, field, ptr(t, o))
        q.pm0, q.pm1, q.prenet_keep = ptr(mk["prenet_drop_0"]), ptr(mk["prenet_drop_1"]), 1 - d.prenet_drop
        q.wx0, q.b0, q.w0f = ptr(k0, o0), ptr(b0, ob0), ptr(w0f)
        q.zoneout = d.zoneout
        # (outputs: every row of the steps that ran is written by whichever driver runs; no clearing pass)
        linear, stop, align = self._buf(Smax, B, NM, zero=False), self._buf(Smax, B, zero=False), self._buf(Smax, B, T, zero=False)
        self._keep.extend((linear, stop, align))
        q.linear, q.stop, q.align_hist = ptr(linear), ptr(stop), ptr(align)
        # ONE launch for the whole loop where the shape and the device allow it, else a launch chain per step
        S = self._decode_persistent(q, values, w0f, mk, B, T, Smax)
        if S is None:
            S = self._decode_stepwise(q, values, w0f, stop)
        return linear[:S], stop[:S], align[:S], S

    def _projected_values(self, values):
        """vp = values . wp_pad[H:, :], a loop invariant of one decode call like the keys: formed at the call's first request."""
        dec = self._dec
        if dec["vp"] is None:
            (B, T, M), npad = values.shape, dec["wp_pad"].shape[1]
            dec["vp"] = self._f(B * T, npad)
            gemm(values, dec["wp_pad"], dec["vp"], B * T, npad, M, M, npad, npad, b_off=self.d.dec_lstm * npad)
        return dec["vp"]

    def _decode_stepwise(self, q, values, w0f, stop):
        """The free-running loop as a launch chain per step, self.chunk steps between two stop checks.  Returns the number of steps."""
        d, L_ = self.d, lib.load()
        B, T, M = values.shape
        H, A, Pn, NM, Smax = d.dec_lstm, d.att, d.prenet, d.n_mel, q.Smax
        q.in0, q.in1, q.pj = ptr(self._f(2, B, Pn + M + H)), ptr(self._f(2, B, 2 * H)), ptr(self._f(B, H + M))
        if L_.mstts_decoder_infer_fast(B, H, Pn, M, A, NM):
            # weight-streaming path: cell-0 kernel with the prenet rows stacked on the folded [ctx ; h] rows, padded projection
            w0s = self._f(Pn + M + H, 4 * H)
            call("mstts_copy2d", q.wx0, 4 * H, ptr(w0s), 4 * H, Pn, 4 * H, 0)
            call("mstts_copy2d", ptr(w0f), 4 * H, ptr(w0s, Pn * 4 * H), 4 * H, M + H, 4 * H, 0)
            wp_pad = self._dec["wp_pad"]
            npad = wp_pad.shape[1]
            q.w0s, q.wp_pad = ptr(w0s), ptr(wp_pad)
            if L_.mstts_cell_fwd_supported(H, Pn + M + H) and L_.mstts_cell_fwd_supported(H, 2 * H):
                # fused cell steps: both cell kernels in the lanes' order + packed activation blocks (csrc/cell.hip)
                w0sp, w1p = self._f((Pn + M + H) * 4 * H), self._f(2 * H * 4 * H)
                k1, o1 = self.P(CELL % 1 + "kernel")
                call("mstts_pack_cell_fwd", ptr(w0s), 4 * H, ptr(w0sp), Pn + M + H, H)
                call("mstts_pack_cell_fwd", ptr(k1, o1), 4 * H, ptr(w1p), 2 * H, H)
                act_p = self._f(2 * int(L_.mstts_cell_act_floats(B, Pn + M + H) + L_.mstts_cell_act_floats(B, 2 * H)))
                q.w0sp, q.w1p, q.act_p = ptr(w0sp), ptr(w1p), ptr(act_p)
                if L_.mstts_lsa_step_qp_supported(T, M, H, npad):
                    # output projection inside the attention launch: the m1 rows of the kernel packed by owner slice, and the projected values
                    wp_own = self._f(int(L_.mstts_lsa_proj_pack_floats()))
                    call("mstts_lsa_proj_pack", ptr(wp_pad), npad, H, npad, ptr(wp_own))
                    q.wp_own, q.vp = ptr(wp_own), ptr(self._projected_values(values))
        q.c0, q.c1, q.cum = ptr(self._f(2, B, H)), ptr(self._f(2, B, H)), ptr(self._f(2, B, T))
        q.pre_ws = ptr(self._f(int(L_.mstts_decoder_infer_ws_floats(B, H, Pn, T, A, NM))))
        # Decoder_Dynamic_Decode stops after the first step at which every row has raised its stop flag
        # (stop_logit >= 0 OR time >= Max_Inference_Length, OR-accumulated; Modules.py:216-219,395,409).
        self._lstm_ctrl_copy()
        finished = np.zeros(B, bool)
        done, S = 0, None
        limit = Smax - 1                         # time index at which the forced stop fires
        while S is None and done < Smax:
            n = min(self.chunk, Smax - done)
            call("mstts_decoder_infer_steps", C.byref(q), done, n)
            st = stop[done:done + n].cpu().numpy()          # synchronises the stream for this chunk
            for i in range(n):
                t = done + i
                finished |= (st[i] >= 0.0) | (t >= limit)
                if finished.all():
                    S = t + 1
                    break
            done += n
        return S

    def _decode_persistent(self, q, values, w0f, mk, B, T, Smax):
        """The whole free-running loop as ONE launch (mstts_decoder_infer_persistent).  Returns the number of steps, or None when the
        shape / device is not covered, the persistent plans are cooling down, or the launch gave up - the caller then runs the
        launch-per-step loop, which rewrites every output."""
        d, L_ = self.d, lib.load()
        H, A, Pn, NM, M = d.dec_lstm, d.att, d.prenet, d.n_mel, d.mem
        if not self.persist_infer:
            return None
        if not L_.mstts_persist_infer_supported(B, H, Pn, M, A, T, d.att_k, NM):
            if L_.mstts_persist_infer_supported(1, H, Pn, M, A, 1, d.att_k, NM):      # widths and device fit, this batch shape does not
                self.non_persistent_decodes += 1
                if (B, T) not in self._warned_shapes:
                    self._warned_shapes.add((B, T))
                    warnings.warn("multi_speaker_tts_amd: batch %d x %d tokens is outside the persistent free-running decoder's range "
                                  "(mstts_persist_infer_supported); decoding launch by launch" % (B, T), RuntimeWarning, stacklevel=4)
            return None
        if not self._persist_cool.admit():
            self.persist_disabled_decodes += 1
            return None
        ticket = self._persist_infer_launch(q, values, w0f, mk, B, T)
        ok, status = ticket.redeem()
        rows, last = ticket.host[ROWS_FINISHED:LAST_STEP + 1].tolist()
        self.persist_infer_status = status + (rows, last)
        if not ok:
            self.persist_infer_fallbacks += 1
            if self._persist_cool.strike(PERSIST_STRIKES, PERSIST_COOLDOWN):
                warnings.warn("multi_speaker_tts_amd: two consecutive persistent decoder launches gave up (status %r); decoding launch by "
                              "launch for the next %d batches" % (self.persist_infer_status, PERSIST_COOLDOWN), RuntimeWarning, stacklevel=4)
            return None
        self._persist_cool.clear()
        self.persist_infer_launches += 1
        return last if last > 0 else Smax

    def _persist_infer_launch(self, q, values, w0f, mk, B, T):
        """Operands, the launch, the read-back of its control words and the stream's sync behind them; returns the ticket."""
        d, L_ = self.d, lib.load()
        H, A, Pn, NM, M = d.dec_lstm, d.att, d.prenet, d.n_mel, d.mem
        prenet0, prenet1 = "decoder/decoder/prenet_0/dense", "decoder/decoder/prenet_1/dense"
        wp_pad = self._dec["wp_pad"]
        NP = wp_pad.shape[1]

        def fill(c):
            k0, o0 = self.P(CELL % 0 + "kernel"); k1, o1 = self.P(CELL % 1 + "kernel"); wq, oq = self.P(LSA + "query_layer/kernel")
            bpj, obpj = self.P("decoder/decoder/linear_projection/dense/bias")
            call("mstts_copy2d", ptr(bpj, obpj), NM + 1, ptr(c["bp_pad"]), NP, 1, NM + 1, 0)
            dense_fwd(self, gemm, wp_pad, H, NM, Pn, prenet0, c["wfm"], lda=NP, bias=False)
            c["bp4"][0].copy_(c["bp_pad"])                # (a 4-row product: row 0 is bp, the other rows are zero)
            dense_fwd(self, gemm, c["bp4"], 4, NM, Pn, prenet0, c["bf"], lda=NP)
            # (w0f: the caller's folded cell-0 kernel - its values depend on the variables only)
            call("mstts_persist_pack", ptr(w0f), ptr(k1, o1), ptr(wq, oq), ptr(k0, o0), ptr(c["pk"][0]), ptr(c["pk"][1]), ptr(c["pk"][2]))
            call("mstts_persist_infer_pack", ptr(wq, oq), ptr(wp_pad), NP, ptr(c["wfm"]), ptr(c["wqppk"]))
        # what depends on the variables only (padded projection bias, first prenet layer folded onto its m1 half, kernels in the lanes' order),
        # with the launch's exchange block and control words
        c = self._derived_at_version("persist_infer", lambda: dict(
            bp_pad=self._buf(NP), wfm=self._buf(H, Pn), bf=self._buf(4, Pn), bp4=self._buf(4, NP),
            pk=[self._buf(L_.mstts_persist_pack_floats(i), zero=False) for i in range(3)],
            wqppk=self._buf(L_.mstts_persist_infer_pack_floats(), zero=False), xch=self._buf(L_.mstts_persist_infer_ws_bytes() // 4, zero=False),
            ctrl=torch.zeros(272, dtype=torch.int32, device=self.device), ctrl_host=torch.zeros(272, dtype=torch.int32).pin_memory()), fill)
        # loop invariants of this batch (see include/mstts.h): projected values, and the first prenet layer applied to them
        vp, u = self._projected_values(values), self._f(B * T, Pn)
        dense_fwd(self, gemm, vp, B * T, NM, Pn, prenet0, u, lda=NP, bias=False)
        # prenet of the all-zero start frame with the masks of step 0 (Modules.py:178-185)
        zf, pa, pb = self._f(B, NM), self._f(B, Pn), self._f(B, Pn)
        dense_fwd(self, gemm, zf, B, NM, Pn, prenet0, pa, act=ACT_RELU)
        call("mstts_dropout", ptr(pa), ptr(mk["prenet_drop_0"]), 1 - d.prenet_drop, ptr(pb), B * Pn)
        dense_fwd(self, gemm, pb, B, Pn, Pn, prenet1, pa, act=ACT_RELU)
        pre0 = self._f(B, Pn)
        call("mstts_dropout", ptr(pa), ptr(mk["prenet_drop_1"]), 1 - d.prenet_drop, ptr(pre0), B * Pn)
        pd = lib.PersistInferDesc()
        pd.w0pk, pd.w1pk, pd.wqppk = ptr(c["pk"][0]), ptr(c["pk"][1]), ptr(c["wqppk"])
        pd.pre0, pd.bf, pd.u, pd.vp, pd.bp_pad = ptr(pre0), ptr(c["bf"]), ptr(u), ptr(vp), ptr(c["bp_pad"])
        pd.xch, pd.ctrl = ptr(c["xch"]), ptr(c["ctrl"])
        pd.stamps = ptr(self.persist_infer_stamps) if self.persist_infer_stamps is not None else None
        pd.selftest_fail_step = int(self.persist_infer_selftest)
        pd.near_xcd = near_xcd()
        call("mstts_decoder_infer_persistent", C.byref(q), C.byref(pd))
        self._lstm_ctrl_copy()
        ticket = Ticket(c["ctrl"], c["ctrl_host"], decoder_workgroups()).enqueue()
        torch.cuda.current_stream().synchronize()
        return ticket

    def postnet(self, linear_bsc, B, S):
        d = self.d
        x, cin = linear_bsc, d.n_mel
        for i in range(d.post_n):
            cout = d.post_ch if i < d.post_n - 1 else d.n_mel
            a = self._f(B * S, cout)
            conv_fwd(self, gemm, x, B * S, S, cin, cout, d.post_k, "decoder/conv_%d/conv1d" % i, a, ACT_TANH)
            x = self._f(B * S, cout)
            bn_infer_fwd(self, "decoder/conv_%d/batch_normalization/" % i, a, x, B * S, cout)
            cin = cout
        mel = self._f(B, S, d.n_mel)
        call("mstts_add", ptr(linear_bsc), ptr(x), ptr(mel), B * S * d.n_mel)
        return mel

    def _mel_to_spectrogram(self, mel, B, S):
        """ConvBank -> Highway -> BiRNN -> Projection (MSTTS_SV.py:100-115), inference mode."""
        d = self.d
        rows, C1 = B * S, d.bank_k * d.bank_ch
        cat, cb = self._f(rows, C1), VOC + "convbank_0/"
        for k in range(1, d.bank_k + 1):
            a = self._f(rows, d.bank_ch)
            conv_fwd(self, gemm, mel, rows, S, d.n_mel, d.bank_ch, k, cb + "conv1d" + bank_suffix(k), a, ACT_RELU)
            y = self._f(rows, d.bank_ch)
            bn_infer_fwd(self, cb + "batch_normalization%s/" % bank_suffix(k), a, y, rows, d.bank_ch)
            call("mstts_copy2d", ptr(y), d.bank_ch, ptr(cat, (k - 1) * d.bank_ch), C1, rows, d.bank_ch, 0)
        p = self._f(rows, C1)
        call("mstts_maxpool2_same", ptr(cat), ptr(p), B, S, C1)
        for sfx, cin, cout, K, act in (("_8", C1, d.proj1_ch, d.proj1_k, ACT_RELU), ("_9", d.proj1_ch, d.n_mel, d.proj2_k, ACT_NONE)):
            a = self._f(rows, cout)
            conv_fwd(self, gemm, p, rows, S, cin, cout, K, cb + "conv1d" + sfx, a, act)
            p = self._f(rows, cout)
            bn_infer_fwd(self, cb + "batch_normalization%s/" % sfx, a, p, rows, cout)
        x = self._f(rows, d.n_mel)
        call("mstts_add", ptr(mel), ptr(p), ptr(x), rows * d.n_mel)
        for i in range(d.highway_n):
            hp_, tp_ = self._f(rows, d.n_mel), self._f(rows, d.n_mel)
            dense_fwd(self, gemm, x, rows, d.n_mel, d.n_mel, VOC + "highway_%d/dense" % i, hp_)
            dense_fwd(self, gemm, x, rows, d.n_mel, d.n_mel, VOC + "highway_%d/dense_1" % i, tp_)
            y = self._f(rows, d.n_mel)
            call("mstts_highway_combine", ptr(hp_), ptr(tp_), ptr(x), ptr(y), rows * d.n_mel)
            x = y
        rnn = self._f(B, S, 2 * d.birnn)
        self._bilstm_seq(x, B, S, d.n_mel, d.birnn, VOC_CELL, rnn, S * 2 * d.birnn, 2 * d.birnn)
        spec = self._f(rows, d.n_spec)
        dense_fwd(self, gemm, rnn, rows, 2 * d.birnn, d.n_spec, VOC + "dense", spec)
        return spec.view(B, S, d.n_spec)

    # ------------------------------------------------------------------ whole forward
    @lib.deterministic_gemm()
    def forward(self, pattern, masks=None, seed=None, max_steps=None, with_vocoder=True):
        """See _forward.  A persistent LSTM launch that gave up (bounded waits, no co-residency) invalidates what was computed from its output:
        the pass is run again with the launch-per-step drivers."""
        try:
            return self._forward(pattern, masks, seed, max_steps, with_vocoder)
        except _PersistRetry as e:
            warnings.warn("multi_speaker_tts_amd: %s; re-running the forward pass launch by launch" % (e,), RuntimeWarning, stacklevel=2)
            return self._launch_by_launch(self._forward, pattern, masks, seed, max_steps, with_vocoder)

    def _forward(self, pattern, masks=None, seed=None, max_steps=None, with_vocoder=True):
        """pattern: dict with Token [B,T] int32, Token_Length [B] int32 and either Speaker_Embedding_Mel
        [5B,64,80] or Speaker_Embedding [B,spk] (numpy or tensors).  Returns the reference's
        inference_Tensor_Dict as numpy arrays: Linear, Mel, Stop (sigmoid), Attention_History [B,T,S], Spectrogram."""
        self._keep = []
        self._lstm_pending, self._lstm_ticket = [], None
        dev = self.device
        prof = getattr(self, "profile_phases", False)          # tools/infer_bench.py: wall time per phase (adds a synchronisation behind each)
        marks = [("start", time.perf_counter())]

        def mark(name):
            if prof:
                torch.cuda.synchronize()
                marks.append((name, time.perf_counter()))
        t = lambda a, dt: (a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))).to(dev, dt).contiguous()
        token, tlen = t(pattern["Token"], torch.int32), t(pattern["Token_Length"], torch.int32)
        B, T = token.shape
        spk_done = None
        if "Speaker_Embedding" in pattern:
            spk = t(pattern["Speaker_Embedding"], torch.float32)
        else:
            spk_mel = t(pattern["Speaker_Embedding_Mel"], torch.float32)
            if SPK_OVERLAP and dev.type == "cuda" and not prof:
                # the speaker stack (three 64-step recurrent layers on 80 rows: 96 workgroups each) and the text encoder (convolutions, BiLSTM: 64 workgroups)
                # meet only at the memory's speaker columns: the stack runs on its own stream beside the encoder.  (Its temporaries live until the end of
                # the pass, self._keep; the control words of its launches are copied behind the join.)
                if self._spk_stream is None:
                    self._spk_stream = torch.cuda.Stream(device=dev)
                with lib.fork(self._spk_stream) as side:
                    spk = self._speaker_embedding(spk_mel)
                spk_done = side.done
            else:
                spk = self._speaker_embedding(spk_mel)
        mark("uploads + speaker encoder")
        values, keys = self._encoder(token, tlen, spk, spk_done)
        mark("text encoder")
        lin_s, stop_s, align_s, S = self.decode(values, keys, tlen, masks=masks, seed=seed, max_steps=max_steps)
        mark("free-running decoder")
        self._lstm_verify()                  # (decode synchronised the stream behind the read-back of their control words)
        d = self.d
        linear = self._f(B, S, d.n_mel)
        call("mstts_transpose01", ptr(lin_s), ptr(linear), S, B, d.n_mel)
        mel = self.postnet(linear, B, S)
        out = {"Linear": linear, "Mel": mel, "Stop_Logit": stop_s.t().contiguous(), "Attention_History": align_s.permute(1, 2, 0).contiguous(),
               "Speaker_Embedding": spk}
        if with_vocoder:
            out["Spectrogram"] = self._mel_to_spectrogram(mel, B, S)
        self._lstm_ctrl_copy()
        torch.cuda.synchronize()
        self._lstm_verify()
        mark("postnet + Taco1 vocoder")
        res = to_host(out)
        res["Stop"] = 1.0 / (1.0 + np.exp(-res["Stop_Logit"]))
        mark("results to the host")
        if prof:
            self.phase_ms = {b[0]: (b[1] - a[1]) * 1e3 for a, b in zip(marks[:-1], marks[1:])}
        self._keep = []
        return res
