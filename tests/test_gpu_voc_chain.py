"""The vocoder statistics side chain of a train step (quirk Q20, TrainEngine._vocoder_bn_update) in its fused form - two packed bank products, a
segmented batch norm with the pool on its way out, the projections, the last layer's statistics alone - against oracle.model.taco1_convbank in
fp64, next to the chain per bank width it replaces (engine.VOC_FUSED = False), both from the same state and the same predicted mel."""
import functools

import numpy as np
import pytest
import torch

from multi_speaker_tts_amd import engine as E
from multi_speaker_tts_amd.engine import TrainEngine
from multi_speaker_tts_amd.params import VOC, bank_suffix
from oracle import model as OM
from tests.convbank_ref import bank_pack_reference
from tests.helpers import dims_pair, rel_err, t2n

pytestmark = pytest.mark.gpu
KW = dict(bank_ch=128, proj1_ch=256, n_mel=80)           # the reference bank: 8 x 128 channels, 256, 80
# (B, T_enc, L): B x (L + 1) frames.  The last one has 66 rows: past the 32-row kernels, so the packed products run in the split form of the headline shape
SHAPES = [(2, 12, 5), (3, 20, 9), (1, 8, 1), (3, 20, 21)]
PARITY_BOUND = 2e-3                                      # tests/test_gpu_model.py::test_train_two_steps_parity's bound on every variable, moving statistics included
CB = VOC + "convbank_0/"
BN_SCOPES = [CB + "batch_normalization%s/" % bank_suffix(k) for k in range(1, 9)] + [CB + "batch_normalization_8/", CB + "batch_normalization_9/"]
STATS = [s + m for s in BN_SCOPES for m in ("moving_mean", "moving_variance")]


@functools.lru_cache(maxsize=None)
def _values():
    pd, od = dims_pair(**KW)
    values = OM.init_params(od, 11)
    g = np.random.default_rng(12)
    for k in values:                                     # nothing at its trivial initial value: biases, BN scales / shifts, the moving statistics
        if k.startswith(CB):
            if k.endswith(("bias", "beta", "moving_mean")):
                values[k] = g.normal(0, 0.2, values[k].shape)
            elif k.endswith(("gamma", "moving_variance")):
                values[k] = g.uniform(0.5, 1.5, values[k].shape)
    return pd, od, values


@functools.lru_cache(maxsize=None)
def _engine(fused):
    pd, _, values = _values()
    old, E.VOC_FUSED = E.VOC_FUSED, fused                # (read when a batch shape is planned)
    try:
        eng = TrainEngine(pd, device="cuda:0", values=values, seed=3)
        for B, Te, L in SHAPES:
            assert eng.plan(B, Te, L).voc_fused == fused
    finally:
        E.VOC_FUSED = old
    return eng


@functools.lru_cache(maxsize=None)
def _oracle(shape):
    """The predicted mel of a shape (fp32 values) and the ten layers' moving statistics after one oracle evaluation in fp64."""
    _, od, values = _values()
    B, _, L = shape
    mel = np.random.default_rng(100 + B).normal(0, 1.0, (B, L + 1, od.n_mel)).astype(np.float32)
    stats = {}
    OM.taco1_convbank(OM.to_torch(values), od, torch.from_numpy(mel).double(), True, stats_out=stats)
    assert sorted(stats) == sorted(STATS)
    return mel, {k: t2n(v) for k, v in stats.items()}


def _chain(fused, shape):
    """One _vocoder_bn_update from the initial state; returns (moving statistics, non-trainable slab before, after, engine)."""
    _, _, values = _values()
    eng = _engine(fused)
    eng.params.load(values)
    mel, _ = _oracle(shape)
    w = eng.plan(*shape)
    w.mel_out.copy_(torch.from_numpy(mel))
    before = (eng.params.frozen.clone(), eng.params.train.clone())
    eng._vocoder_bn_update(w)
    torch.cuda.synchronize()
    got = {k: t2n(eng.params.view(k)).copy() for k in STATS}
    return got, before, (eng.params.frozen.clone(), eng.params.train.clone()), eng


@pytest.mark.parametrize("shape", SHAPES)
def test_fused_chain_against_the_oracle_and_the_chain_per_width(dev, shape):
    """Per tensor: the fused chain's error against fp64 is at most the larger of 1.5 x the replaced chain's error (the packed products group the K sum
    differently: zero taps add exact zeros, width 1 moves from the f32-input matrix cores to the split form the other widths already use) and the
    two-step parity test's bound.  Measured pairs: profiles/voc_chain_fused_parity.txt."""
    _, ref = _oracle(shape)
    fused, before, after, eng = _chain(True, shape)
    parent, _, _, _ = _chain(False, shape)
    bad = {}
    for k in STATS:
        ef, ep = rel_err(fused[k], ref[k]), rel_err(parent[k], ref[k])
        print("%s %s: fused %.3g, per width %.3g" % (shape, k[len(CB):], ef, ep))
        if not (np.isfinite(fused[k]).all() and ef <= max(1.5 * ep, PARITY_BOUND)):
            bad[k] = (ef, ep)
    assert not bad, bad
    # The two chains against each other, tighter than either bound above (a moving statistic is 0.99 x old + 0.01 x batch, so those leave the
    # batch statistics two decimal orders of slack): both round the stored value once (2 x 2^-24 = 1.2e-7) and may differ in the batch
    # statistic by the fp32 summation error of a product of K <= 640 terms and a column sum of <= 30 rows, 5e-5 relative at the outside,
    # which enters at 1 %: 1.2e-7 + 0.01 x 2 x 5e-5 = 1.1e-6.
    for k in STATS:
        e = rel_err(fused[k], parent[k])
        print("%s %s: fused against per width %.3g" % (shape, k[len(CB):], e))
        assert e <= 1.1e-6, (k, e)
    # nothing but the twenty moving-statistics vectors changed in either slab
    ps = eng.params
    keep = torch.ones_like(before[0], dtype=torch.bool)
    for k in STATS:
        assert not ps.trainable[k]
        keep[ps.offset[k]:ps.offset[k] + int(np.prod(ps.shape[k]))] = False
    assert torch.equal(before[0][keep], after[0][keep]) and torch.equal(before[1], after[1])
    assert not torch.equal(before[0][~keep], after[0][~keep])


def test_packed_copy_follows_the_frozen_slab(dev, monkeypatch):
    """The packed bank is the rule of tests/convbank_ref.py, bit for bit, and is rebuilt after params.touch() - a load, a broadcast - and
    only then: not per call, and not by an optimizer step (touch(frozen=False): it writes the trainable slab)."""
    pd, _, values = _values()
    eng = _engine(True)
    calls, inner = [], E.call

    def spy(name, *a):
        calls.append(name)
        return inner(name, *a)
    monkeypatch.setattr(E, "call", spy)
    packs = lambda: calls.count("mstts_convbank_pack")
    eng.params.load(values)                              # (touches)
    w = eng.plan(*SHAPES[0])
    w.mel_out.copy_(torch.from_numpy(_oracle(SHAPES[0])[0]))
    eng._vocoder_bn_update(w)
    eng._vocoder_bn_update(w)
    assert packs() == 1
    eng.params.touch(frozen=False)
    eng._vocoder_bn_update(w)
    assert packs() == 1
    eng.params.touch()
    eng._vocoder_bn_update(w)
    eng._vocoder_bn_update(w)
    assert packs() == 2
    assert calls.count("mstts_bn_train_fwd_seg") == 15   # three batch norms in each of the five calls (the products go through lib.gemm) ...
    assert not {"mstts_bn_train_fwd", "mstts_copy2d", "mstts_maxpool2_same"} & set(calls), calls      # ... and nothing of the chain per width
    torch.cuda.synchronize()
    kernels = [np.asarray(values[CB + "conv1d%s/kernel" % bank_suffix(k)], np.float32) for k in range(1, 9)]
    biases = [np.asarray(values[CB + "conv1d%s/bias" % bank_suffix(k)], np.float32) for k in range(1, 9)]
    mats, bias = bank_pack_reference(kernels, biases, eng.voc_bank["groups"][0][1])
    assert np.array_equal(t2n(eng.voc_bank["w"]), np.concatenate([m.reshape(-1) for m in mats]))
    assert np.array_equal(t2n(eng.voc_bank["bias"]), bias)
