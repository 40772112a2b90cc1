"""Host side of the WaveGlow trainer (no GPU): learning-rate schedule, Restructure_Train_Data's shape rules, the wav feeder
(WaveGlow/Feeder.py:30-114), the parameter store on the WaveGlow variable table, and the new entry points' declarations."""
import math
import os
import re

import numpy as np
import pytest

from multi_speaker_tts_amd import Hyper_Parameters as hp
from multi_speaker_tts_amd import lib
from multi_speaker_tts_amd import waveglow as WG
from multi_speaker_tts_amd import waveglow_trainer as WT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(n_mel=8, flows=4, groups=8, early_every=2, early_size=2, up_k=16, up_stride=4, layers=3, ch=32, k=3)
NEW_ENTRY_POINTS = ["mstts_wg_weight_norm_fwd", "mstts_wg_weight_norm_bwd", "mstts_wg_coupling_fwd", "mstts_wg_coupling_bwd",
                    "mstts_wg_inv1x1_logdet", "mstts_wg_gate_bwd", "mstts_wg_res_skip_bwd", "mstts_wg_overlap_add_bwd", "mstts_wg_bias_fold",
                    "mstts_adam_tf_clip"]


def test_learning_rate_schedule_is_tf_exponential_decay():
    """tf.train.exponential_decay(1e-3, step, 100000, 0.5), not staircase, floored at 1e-5 (WaveGlow.py:53-60)."""
    for step in (0, 1, 999, 50000, 100000, 123456, 650000, 700000, 2000000):
        want = max(1e-3 * 0.5 ** (step / 100000.0), 1e-5)
        assert math.isclose(WT.learning_rate(step), want, rel_tol=1e-12)
    assert WT.learning_rate(10 ** 7) == 1e-5


def test_restructure_rules():
    d = WG.WGDims(**SMALL)
    # audio cut to a multiple of G; the upsampled mel ((T-1)*S + K) sliced to it
    assert WT.restructure(d, 2, 61, 12) == (56, 7, 60)
    assert WT.restructure(d, 1, 60, 12) == (56, 7, 60)
    assert WT.restructure(d, 1, 64, 13) == (64, 8, 64)
    with pytest.raises(ValueError):
        WT.restructure(d, 1, 72, 13)                  # 64 upsampled samples cannot condition 72
    # the reference batch: 8000 samples, 29 frames -> 8192 upsampled samples
    r = WG.WGDims()
    assert WT.restructure(r, 4, 8000, 29) == (8000, 1000, 8192)
    # chunks leaving the flow stack: early at flows 4 and 8 (columns 0, 2), the last flow's 4 channels at column 4
    assert [WT.early_chunk(r, f) for f in range(12)] == [None, None, None, (0, 2), None, None, None, (2, 2), None, None, None, (4, 4)]
    assert WT.early_chunk(d, 1) == (0, 2) and WT.early_chunk(d, 3) == (2, 6) and d.z_channels == 6


def _write_wav(path, sr, sig):
    from scipy.io import wavfile
    wavfile.write(str(path), sr, (np.clip(sig, -1, 1) * 32767).astype(np.int16))


def test_feeder_crop_pad_peak_and_mel_frames(tmp_path, monkeypatch):
    from multi_speaker_tts_amd import WaveGlow as W
    monkeypatch.setattr(hp.WaveGlow.Train, "Max_Signal_Length", 4000)
    sr = hp.WaveGlow.Export_Sample_Rate
    g = np.random.default_rng(0)
    t = np.arange(12000) / sr
    _write_wav(tmp_path / "long.wav", sr, 0.5 * np.sin(2 * np.pi * 220 * t) + 0.01 * g.normal(size=t.shape))
    _write_wav(tmp_path / "short.wav", sr, 0.3 * np.sin(2 * np.pi * 330 * t[:1500]))
    rng = np.random.default_rng(1)
    long = W.train_signal(str(tmp_path / "long.wav"), rng)
    short = W.train_signal(str(tmp_path / "short.wav"), rng)
    assert long.shape == (4000,) and short.shape == (4000,)
    assert 0.9 < np.abs(long).max() <= 0.99 + 1e-6                      # a cropped window of a peak-0.99 signal
    assert abs(np.abs(short).max() - 0.99) < 1e-6
    nz = np.nonzero(short)[0]
    assert nz[-1] < 1500 and np.all(short[1500:] == 0)              # zero-padded at the end
    # the mel is computed from the signal resampled to Sound.Sample_Rate; the audio target stays at Export_Sample_Rate
    res = W.resample_for_mel(long)
    n16 = int(round(4000 * hp.Sound.Sample_Rate / sr))
    assert abs(res.shape[0] - n16) <= 1
    hop = int(hp.Sound.Frame_Shift / 1000 * hp.Sound.Sample_Rate)
    assert hop == 200 and W.mel_frames(res.shape[0]) == 1 + res.shape[0] // 200
    # the reference batch: 8000 samples at 22 050 Hz -> 5805 at 16 kHz -> 30 frames, whose 7 680 + 1 024 upsampled samples cover 8000
    assert W.mel_frames(int(round(8000 * 16000 / 22050))) == 30 and WT.restructure(WG.WGDims(), 4, 8000, 30)[0] == 8000
    # batch padding to the longest item with an injected mel function (the real one is a GPU launch)
    batch = W.train_batch([str(tmp_path / "long.wav"), str(tmp_path / "short.wav")], rng,
                          mel_fn=lambda s: np.ones((W.mel_frames(W.resample_for_mel(s).shape[0]), hp.Sound.Mel_Dim), np.float32))
    assert batch["Audio"].shape == (2, 4000) and batch["Mel"].shape == (2, W.mel_frames(res.shape[0]), 80)
    assert W.wav_paths(str(tmp_path)) == sorted([str(tmp_path / "long.wav"), str(tmp_path / "short.wav")])


def test_param_store_on_the_waveglow_table():
    import torch
    from multi_speaker_tts_amd.params import ParamStore
    d = WG.WGDims(**SMALL)
    table = WG.variable_table(d)
    vals = WG.random_values(d, seed=2)
    ps = ParamStore(d, "cpu", values=vals, trainable_fn=lambda n: True, weight_reg_fn=lambda n: False, table=table)
    assert [n for n, _, _ in ps.table] == [n for n, _ in table]
    assert all(ps.shape[n] == tuple(s) for n, s in table)
    assert all(ps.offset[n] % 4 == 0 for n, _ in table)                         # 16-byte aligned
    assert ps.n_train == sum((int(np.prod(s)) + 3) // 4 * 4 for _, s in table) and ps.n_frozen == 0
    out = ps.export()
    assert sorted(out) == sorted(vals) and all(np.array_equal(out[k], vals[k]) for k in vals)
    ps2 = ParamStore(d, "cpu", values=out, trainable_fn=lambda n: True, weight_reg_fn=lambda n: False, table=table)
    assert torch.equal(ps2.train, ps.train) and int(ps.wd_mask.sum()) == 0
    # the Tacotron2 default is unchanged
    from multi_speaker_tts_amd.params import variable_table
    from tests.helpers import dims_pair
    pd, _ = dims_pair()
    assert ParamStore(pd, "cpu", seed=3).table == variable_table(pd)


def test_new_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "mstts.h")).read()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in lib.SIGNATURES, name
    assert lib.ABI_VERSION == 5
    import ctypes
    assert ctypes.sizeof(lib.WgWnDesc) == 8 * 8
