"""The tiers of the launch-per-step decoder drivers (csrc/decoder.hip) against each other, at the driver level: mstts_decoder_train_fwd
and _bwd called directly on one engine's descriptors, once as the engine built them (fused cell steps, query projection inside the
attention launch, packed BPTT products, query gradient folded into cell 1's pointwise backward) and once on a copy with every optional
derived-copy pointer nulled (skinny products + pointwise launches, row-major BPTT products).  Same fp32 products in another summation
order: the bound is the project's figure for that at L <= 20, 5e-5 relative (test_gpu_persist.py::test_persistent_equals_launch_per_step).
An error both tiers share passes here: each tier on its own against oracle.model.decoder's loop in fp64, per (step, row) slice, is
tests/test_gpu_decoder_loop_ref.py.

Shapes: the smallest at which the fused tiers exist and both MFMA row tiles are live - the WIDE widths of test_gpu_persist.py (decoder
1024, memory 768, attention 128), B = 3 (one row tile) and 17 (two), L = 3 ragged - and one MID case (5, 18, 4): fused cells without the
fused query.  mstts_lsa_step_q_supported has no lower threshold in the encoder length (it returns 1 from Te = 1, asserted below), and a
one-token batch cannot be ragged, so the WIDE cases run at Te = 7, the shortest text the engine-level tests of this suite use.

Measured once on the parent commit's library (MI355X), worst of the three cases per tensor, all below the bound of 5e-5, so the bound stays:
    in0 2.1e-07  in1 3.3e-07  pj 1.9e-07  c0 2.6e-07  c1 4.9e-07  acts0 2.1e-07  acts1 1.6e-07  craw0 2.3e-07  craw1 4.8e-07
    q_hist 7.0e-07  align_hist 1.5e-07  cum_hist 1.5e-07  dg0 1.6e-07  dg1 2.3e-07  dq_hist 1.1e-05  de_hist 2.4e-07  d_in0 2.2e-07
(dq_hist: the query gradient is summed with atomics by the attention backward, 4.4e-06 ... 1.1e-05 from run to run.)
"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import dims_pair, rel_err, t2n, to_dev
from oracle import model as OM, train as OT
from multi_speaker_tts_amd import lib
from multi_speaker_tts_amd.engine import TrainEngine

pytestmark = pytest.mark.gpu

WIDE = dict(emb=64, enc_conv_ch=64, enc_lstm=256, spk=256, prenet=256, dec_lstm=1024, n_mel=16, post_ch=32)      # = test_gpu_persist.py
MID = dict(dec_lstm=64, enc_lstm=32, spk=64, prenet=32)                                                          # = test_gpu_model.py
HIST = ("in0", "in1", "pj", "c0", "c1", "acts0", "acts1", "craw0", "craw1", "q_hist", "align_hist", "cum_hist")

NULLED = ("act_p", "w0p", "w1p", "w0f_bp", "w1_bp", "wq_bp", "wq_t")        # ... and lsa.loc_kt
BWD = ("dg0", "dg1", "dq_hist", "de_hist", "d_in0")
BOUND = 5e-5


def _copy(desc):
    d = type(desc)()
    C.memmove(C.byref(d), C.byref(desc), C.sizeof(desc))
    return d


@pytest.mark.parametrize("kw,B,Te,L,fused_query", [(WIDE, 3, 7, 3, True), (WIDE, 17, 7, 3, True), (MID, 5, 18, 4, False)])
def test_decoder_tiers_agree(dev, kw, B, Te, L, fused_query):
    L_ = lib.load()
    pd, od = dims_pair(**kw)
    H, M, A = pd.dec_lstm, pd.mem, pd.att
    assert L_.mstts_lsa_step_q_supported(1, 768, 1024) == 1              # (no smallest supported Te: see the module docstring)
    eng = TrainEngine(pd, device=dev, values=OM.init_params(od, 3))
    batch = to_dev(OT.synthetic_batch(od, B, Te, L, seed=5, ragged=True), dev)
    w = eng.plan(B, Te, L)
    w.persist = w.persist_bwd = False
    eng.forward(batch, w, seed=11)                                       # builds the descriptors, the derived copies and the loop's inputs
    eng.loss_and_backward(w)
    torch.cuda.synchronize()
    full = w.dec
    # the fused tiers really are selected by the full descriptor - else this would compare a tier with itself
    assert L_.mstts_cell_fwd_supported(H, M + H) == 1 and L_.mstts_cell_fwd_supported(H, 2 * H) == 1 and M % 4 == 0
    assert full.act_p and full.w0p and full.w1p and full.w0f_bp and full.w1_bp and full.wq_bp
    assert min(L_.mstts_skinny_bwd_splits(M + H, 4 * H), L_.mstts_skinny_bwd_splits(2 * H, 4 * H), L_.mstts_skinny_bwd_splits(H, A)) >= 1
    assert min(L_.mstts_skinny_fwd_splits(4 * H, M + H), L_.mstts_skinny_fwd_splits(4 * H, 2 * H), L_.mstts_skinny_fwd_splits(A, H)) >= 1
    assert L_.mstts_lsa_step_q_supported(Te, M, H) == int(fused_query)
    if fused_query:
        assert full.lsa.loc_kt and A == 128 and full.energy_ws_floats >= L_.mstts_lsa_step_q_ws_bytes(B, Te) // 4
        assert full.wq_t and H % 128 == 0 and L_.mstts_skinny_bwd_splits(2 * H, 4 * H) in (1, 2, 4, 8) and B * H * 4 < 1 << 30      # fused query gradient
        assert (H + M) % 4 == 0 and H % 4 == 0                                                                                    # fused query, single-launch attention backward
    plain = _copy(full)
    for name in NULLED:
        setattr(plain, name, None)
    plain.lsa.loc_kt = None
    got = {}
    for tier, dec in (("fused", full), ("plain", plain)):
        for k in HIST + BWD:
            getattr(w, k).zero_()
        db = _copy(w.dec_b)
        db.fwd = C.pointer(dec)
        lib.call("mstts_decoder_train_fwd", C.byref(dec))
        lib.call("mstts_decoder_train_bwd", C.byref(db))
        torch.cuda.synchronize()
        got[tier] = {k: t2n(getattr(w, k)).copy() for k in HIST + BWD}
        got[tier]["d_in0"] = got[tier]["d_in0"].reshape(w.d_in0_parts, -1).sum(0)      # fold the partial slabs
    errs = {k: rel_err(got["fused"][k], got["plain"][k]) for k in HIST + BWD}
    print("fused vs plain tiers, B=%d Te=%d L=%d: %s" % (B, Te, L, " ".join("%s %.1e" % (k, errs[k]) for k in HIST + BWD)))
    for k in HIST + BWD:
        assert np.isfinite(got["fused"][k]).all() and np.abs(got["fused"][k]).max() > 0, k
    bad = {k: e for k, e in errs.items() if not e <= BOUND}
    assert not bad, bad
