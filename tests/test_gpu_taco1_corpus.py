"""The Taco1 vocoder trainer on a corpus: the signal-bank STFT kernel against mstts_stft_fft (bit for bit) and the fp64 oracle, its
invalid rows, and the way from a directory of wavs through the pattern generator, both feeders and Train() to the periodic inference."""
import os
import pickle

import numpy as np
import pytest
import torch

from multi_speaker_tts_amd import lib
from oracle import audio as OA
from tests.helpers import t2n

pytestmark = pytest.mark.gpu

LENGTHS = (1025, 4000, 4321, 7400, 16000)      # barely over the 2048-point transform's reflect padding (6 frames); a multiple of hop; ...
FILES = (4, 0, 2, 2, 3, 1)                      # a repeated file; the longest row has no padding at T = its frame count
HOP = 200
# (num_freq, frame_length_ms, num_mels): the reference transform (n_fft 2048, win 800) and n_fft 512, win 400
TRANSFORMS = {"ref": (1025, 50, 80), "small": (257, 25, 40)}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def signals():
    g = np.random.default_rng(3)
    out = []
    for n in LENGTHS:
        t = np.arange(n) / 16000.0
        out.append((0.25 * np.sin(2 * np.pi * (150 + 40 * len(out)) * t) + 0.05 * g.normal(size=n)).astype(np.float32))
    return out


@pytest.fixture(scope="module")
def features(dev, signals):
    """Audio.stft_features of every signal under both transforms, computed once: {name: [(mel, spec) host arrays]}."""
    from multi_speaker_tts_amd import Audio
    out = {}
    for name, (num_freq, fl, n_mel) in TRANSFORMS.items():
        feats = Audio.stft_features(signals, num_freq, 12.5, fl, 16000, num_mels=n_mel, max_abs_value=4, want_mel=True, want_spec=True, device=dev)
        out[name] = [(t2n(m), t2n(s)) for m, s in feats]
    return out


def _bank_batch(dev, sigs, files, T, transform, want_mel=True, want_spec=True):
    """One mstts_stft_bank_batch launch into NaN-filled outputs with a guard behind each -> (mel, spec, status)."""
    from multi_speaker_tts_amd import Audio
    num_freq, fl, n_mel = TRANSFORMS[transform]
    n_fft, hop, win, hann, tw, fb, rng = Audio._fft_constants(num_freq, 12.5, fl, n_mel, 16000, str(dev))
    off = np.concatenate([[0], np.cumsum([len(x) for x in sigs])]).astype(np.int64)
    bank_d, off_d = torch.tensor(np.concatenate(sigs), device=dev), torch.tensor(off, device=dev)
    files_d = torch.tensor(np.asarray(files, np.int32), device=dev)
    N, guard = len(files), 512
    bufs = []
    for want, width in ((want_mel, n_mel), (want_spec, num_freq)):
        b = torch.full((N * T * width + guard,), float("nan"), device=dev) if want else None
        if want:
            b[N * T * width:] = 12345.0
        bufs.append(b)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    lib.call("mstts_stft_bank_batch", lib.ptr(bank_d), lib.ptr(off_d), len(sigs), lib.ptr(files_d), N, T, 0.97, lib.ptr(hann), lib.ptr(tw),
             lib.ptr(fb), lib.ptr(rng), n_fft, hop, win, n_mel, 4.0, 20.0, lib.ptr(bufs[0]) if want_mel else None,
             lib.ptr(bufs[1]) if want_spec else None, lib.ptr(status))
    out = []
    for b, width in zip(bufs, (n_mel, num_freq)):
        if b is None:
            out.append(None)
            continue
        h = b.cpu().numpy()
        assert np.all(h[N * T * width:] == 12345.0)                               # nothing written behind the batch
        out.append(h[:N * T * width].reshape(N, T, width))
    return out[0], out[1], int(status.item())


def _want(feats, files, T):
    """The padded batch by the reference's rule from per-signal features."""
    mel = np.zeros((len(files), T, feats[0][0].shape[1]), np.float32)
    spec = np.zeros((len(files), T, feats[0][1].shape[1]), np.float32)
    for r, f in enumerate(files):
        mel[r, :feats[f][0].shape[0]] = feats[f][0]
        spec[r, :feats[f][1].shape[0]] = feats[f][1]
    return mel, spec


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("extra", [0, 3])                  # T = the longest row's frame count; T + 3: every row is padded
@pytest.mark.parametrize("transform", ["ref", "small"])
def test_stft_bank_batch_matches_stft_features(dev, signals, features, transform, extra):
    T = 1 + max(LENGTHS) // HOP + extra
    want_mel, want_spec = _want(features[transform], FILES, T)
    assert features[transform][0][0].shape[0] == 6 and want_mel.shape[1] == 81 + extra
    mel, spec, status = _bank_batch(dev, signals, FILES, T, transform)
    assert not np.isnan(mel).any() and not np.isnan(spec).any()                   # every element was stored
    assert _same_bits(mel, want_mel) and _same_bits(spec, want_spec)              # valid frames: mstts_stft_fft's bits; pad frames: +0.0
    assert status == 0
    for r, f in enumerate(FILES):
        F = 1 + LENGTHS[f] // HOP
        assert not mel[r, F:].any() and not spec[r, F:].any()
    only_mel, none, status = _bank_batch(dev, signals, FILES, T, transform, want_spec=False)
    assert none is None and status == 0 and _same_bits(only_mel, want_mel)
    none, only_spec, status = _bank_batch(dev, signals, FILES, T, transform, want_mel=False)
    assert none is None and status == 0 and _same_bits(only_spec, want_spec)


@pytest.mark.parametrize("transform", ["ref", "small"])
def test_stft_bank_batch_against_fp64(dev, signals, transform):
    """The same rows against the fp64 oracle, at the bounds test_stft_fft_batch_spectrogram_and_sizes holds this transform to:
    mel 2e-3 absolute on [-4, 4], spectrogram 1e-3 absolute on [0, 1]."""
    num_freq, fl, n_mel = TRANSFORMS[transform]
    T = 1 + max(LENGTHS) // HOP + 3
    mel, spec, status = _bank_batch(dev, signals, FILES, T, transform)
    assert status == 0
    ref = [OA.spectrogram_and_mel(y, num_freq, 12.5, fl, 16000, 20, n_mel, 4) for y in signals]
    for r, f in enumerate(FILES):
        rs, rm = ref[f]
        F = rm.shape[1]
        assert F == 1 + LENGTHS[f] // HOP
        em, es = np.abs(mel[r, :F].T - rm).max(), np.abs(spec[r, :F].T - rs).max()
        print(transform, "row", r, "file", f, "mel err", em, "spec err", es)
        assert em < 2e-3 and es < 1e-3
        assert not mel[r, F:].any() and not spec[r, F:].any()


def test_stft_bank_batch_flags_bad_rows(dev, signals, features):
    from multi_speaker_tts_amd import taco1_feeder as TF
    g = np.random.default_rng(8)
    sigs = list(signals) + [g.normal(0, 0.1, 1024).astype(np.float32)]            # file 5: exactly n_fft / 2 samples
    feats = features["ref"]
    T = 38                                                                         # 7400 samples: 38 frames; file 4 (81 frames) does not fit
    good = [3, 0, 2, 1]
    mel0, spec0, status = _bank_batch(dev, sigs, good, T, "ref")
    want_mel, want_spec = _want(feats, good, T)
    assert status == 0 and _same_bits(mel0, want_mel) and _same_bits(spec0, want_spec)
    feeder = TF.Taco1Feeder(TF.SignalBank.from_signals(sigs, device=dev), seed=1, batch_size=4)
    assert (feeder.n_fft, feeder.hop) == (2048, 200)
    feeder.check_files(good, T)
    for bad in (6, -1, 4, 5):                                                      # n_files; -1; F_r > T; len == n_fft / 2
        files = [3, 0, bad, 2, 1]
        with pytest.raises(ValueError):
            feeder.check_files(files, T)                                           # refused on the host before any launch
        mel, spec, status = _bank_batch(dev, sigs, files, T, "ref")
        assert status & 1, bad
        assert not np.isnan(mel).any() and not np.isnan(spec).any()
        assert not mel[2].any() and not spec[2].any(), bad                         # the bad row: all zeros
        keep = [0, 1, 3, 4]
        assert _same_bits(mel[keep], want_mel) and _same_bits(spec[keep], want_spec), bad          # the good rows: unchanged
    feeder.check_status()                                                          # (the feeder itself launched nothing)


def _write_corpus(root):
    """Twelve wavs of 0.3 - 0.9 s of tones + noise at 16 kHz between 0.1 s of near silence on either side."""
    from scipy.io import wavfile
    g = np.random.default_rng(31)
    os.makedirs(root)
    paths = []
    for k in range(12):
        n = int(g.integers(4800, 14401))
        t = np.arange(n) / 16000.0
        y = sum(a * np.sin(2 * np.pi * (120.0 + 25 * k) * h * t + g.uniform(0, 6.28)) for h, a in ((1, 0.3), (2, 0.2), (3, 0.1), (7, 0.1)))
        y = np.concatenate([np.zeros(1600), y + g.normal(0, 0.02, n), np.zeros(1600)]) + g.normal(0, 1e-4, n + 3200)
        p = os.path.join(root, "p225_%03d.wav" % (k + 1))
        wavfile.write(p, 16000, np.clip(y * 32767, -32767, 32767).astype(np.int16))
        paths.append(p)
    return paths


def test_taco1_corpus_end_to_end(dev, tmp_path, monkeypatch):
    from multi_speaker_tts_amd import Audio, Hyper_Parameters as hp
    from multi_speaker_tts_amd import Taco1_Mel_to_Spect_Pattern_Generate as PG
    from multi_speaker_tts_amd import taco1_feeder as TF
    from multi_speaker_tts_amd.Taco1_Mel_to_Spect import INFERENCE_IN_TRAIN_FILE, Mel_to_Spect
    from multi_speaker_tts_amd.params import Dims
    tr = hp.Taco1_Mel_to_Spect.Train
    monkeypatch.setattr(hp.Sound, "Spectrogram_Dim", 257)
    monkeypatch.setattr(hp.Sound, "Frame_Length", 25)
    monkeypatch.setattr(hp.Taco1_Mel_to_Spect, "Checkpoint_Path", str(tmp_path / "voc"))
    monkeypatch.setattr(hp.Taco1_Mel_to_Spect, "Griffin_Lim_Iteration", 5)
    monkeypatch.setattr(tr, "Pattern_Path", str(tmp_path / "patterns"))
    monkeypatch.setattr(tr, "Batch_Size", 4)
    monkeypatch.setattr(tr, "Checkpoint_Save_Timing", 4)
    monkeypatch.setattr(tr, "Inference_Timing", 3)
    monkeypatch.setattr(tr.Inference, "Path", str(tmp_path / "mts"))
    monkeypatch.chdir(tmp_path)
    paths = _write_corpus(str(tmp_path / "VCTK"))

    # the generator: the reference's two keys and the signal they are the STFT of
    md = PG.main(["-vctk", str(tmp_path / "VCTK"), "-batch", "5"], device=dev)
    names = ["P225_%03d.PICKLE" % (k + 1) for k in range(12)]
    assert md["File_List"] == names and sorted(os.listdir(tmp_path / "patterns")) == sorted(names + ["METADATA.PICKLE"])
    assert set(md) == {"Sample_Rate", "Spectrogram_Dim", "Mel_Dim", "Frame_Shift", "Frame_Length", "File_List", "Mel_Length_Dict", "Signal_Length_Dict"}
    sigs = []
    for name in names:
        with open(tmp_path / "patterns" / name, "rb") as f:
            d = pickle.load(f)
        assert sorted(d) == ["Mel", "Signal", "Spectrogram"] and all(d[k].dtype == np.float32 for k in d)
        n = d["Signal"].shape[0]
        assert 4000 <= n <= 14400 + 400 and d["Mel"].shape == (1 + n // HOP, 80) and d["Spectrogram"].shape == (1 + n // HOP, 257)     # trimmed
        assert md["Mel_Length_Dict"][name] == 1 + n // HOP and md["Signal_Length_Dict"][name] == n
        (mel, spec), = Audio.stft_features([d["Signal"]], 257, 12.5, 25, 16000, num_mels=80, max_abs_value=4, want_mel=True, want_spec=True, device=dev)
        assert _same_bits(t2n(mel), d["Mel"]) and _same_bits(t2n(spec), d["Spectrogram"])
        sigs.append(d["Signal"])

    # one seed: the host feeder and the device feeder deliver the same batches, bit for bit, over one epoch
    bank = TF.SignalBank.from_patterns(device=dev)
    assert bank.names == names and all(np.array_equal(t2n(bank.bank[int(a):int(b)]), s) for a, b, s in zip(bank._offsets, bank._offsets[1:], sigs))
    host, device = TF.PatternFeeder(seed=1234), TF.Taco1Feeder(bank, seed=1234)
    try:
        first = None
        for _ in range(3):
            ph, pd = host.Get_Train_Pattern(), device.Get_Train_Pattern()
            assert sorted(ph) == sorted(pd) == ["Mel", "Spectrogram"] and pd["Mel"].shape[0] == 4 and pd["Mel"].is_cuda
            assert _same_bits(t2n(pd["Mel"]), ph["Mel"]) and _same_bits(t2n(pd["Spectrogram"]), ph["Spectrogram"])
            first = first or ph
    finally:
        host.close()
    device.check_status()

    # Train() on the bank: finite losses, step 0 is Train_Step on that first batch, a checkpoint and the periodic inference
    with open(tmp_path / INFERENCE_IN_TRAIN_FILE, "w") as f:
        f.write("\n".join(paths[:2]) + "\n")
    dims = Dims(emb=32, enc_conv_ch=32, enc_lstm=16, spk=64, prenet=16, dec_lstm=32, post_ch=16, bank_ch=8, proj1_ch=16, birnn=8, n_spec=257,
                spk_lstm=64, max_inf=4)
    m = Mel_to_Spect(device=dev, dims=dims)
    losses, step = [], m.Train_Step
    monkeypatch.setattr(m, "Train_Step", lambda pattern=None: (lambda r: (losses.append(r["Loss"]), r)[1])(step(pattern)))
    m.Train(max_steps=6)
    assert isinstance(m.feeder, TF.Taco1Feeder) and len(losses) == 6 and m.engine.global_step == 6
    print("losses", losses)
    assert np.all(np.isfinite(losses))
    by_hand = Mel_to_Spect(device=dev, dims=dims).Train_Step(first)["Loss"]
    # The same batch, variables and zoneout masks: the two steps differ only where the engine does.  Its loss scalar is an fp32 atomicAdd
    # of one partial sum per workgroup of l1_loss_kernel (at most ceil(n / 256) of them, all >= 0) in arrival order, so two runs of ONE
    # step may differ by the roundings of that sum: each of the G - 1 additions errs by at most 2^-24 of the running sum <= the loss.
    G = -(-first["Spectrogram"].size // 256)
    print("step 0", losses[0], "by hand", by_hand, "bound", 2 * G * 2.0 ** -24 * by_hand)
    assert abs(losses[0] - by_hand) <= 2 * G * 2.0 ** -24 * by_hand
    assert os.path.exists(tmp_path / "voc" / "mel_to_spectrogram.pt")
    state = torch.load(tmp_path / "voc" / "mel_to_spectrogram.pt", map_location="cpu")
    assert state["__global_step__"] == 4
    wavs = sorted(os.listdir(tmp_path / "mts" / "WAV"))
    assert wavs == ["GS_3.IDX_0.WAV", "GS_3.IDX_1.WAV", "GS_6.IDX_0.WAV", "GS_6.IDX_1.WAV"]
