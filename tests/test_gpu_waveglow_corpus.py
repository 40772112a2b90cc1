"""The WaveGlow trainer on a corpus: the crop kernel (mstts_wg_crop_batch) against the composed path of existing kernels on host-made
crops (bit for bit) and against fp64, its invalid rows, and the way from a directory of wavs through the bank, the feeder and Train()."""
import os

import numpy as np
import pytest
import torch

from multi_speaker_tts_amd import lib
from oracle import audio as OA
from tests.helpers import t2n

pytestmark = pytest.mark.gpu

# name -> ((num_freq, frame_length_ms, num_mels), L, bank lengths): the reference transform (n_fft 2048, win 800) on crops of 8 000, and
# n_fft 512, win 400 on crops of 1 000; the lengths straddle L the same way: far below, equal, one more, a little more, 1.5 L, 2.5 L
CASES = {"ref": ((1025, 50, 80), 8000, (700, 8000, 8001, 8300, 12345, 20000)),
         "small": ((257, 25, 40), 1000, (90, 1000, 1001, 1040, 1543, 2500))}
RATIOS = [(320, 441), (1, 1), (2, 3)]           # 22 050 -> 16 000 (the reference's); no conversion; 24 000 -> 16 000 (a table of 2 rows)
HOP = 200


def _table(case):
    """Zero pad; len == L; len = L + 1 at start 0 and flush with the end; a middle crop of the longest file; a short count inside a long
    file (start > len - L); the longest file again, flush with its end."""
    _, L, n = CASES[case]
    return np.asarray([(0, 0), (1, 0), (2, 0), (2, 1), (5, (n[5] - L) // 2 + 1), (4, n[4] - L // 3), (5, n[5] - L)], np.int32)


FULL_ROWS = [1, 2, 3, 4, 6]                      # the rows of _table without zero padding


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def banks():
    """{case: (bank [total] float32, offsets int64)}: tone + 0.05 noise, each file around its own offset so that a neighbour's samples show."""
    g = np.random.default_rng(3)
    out = {}
    for case, (_, _, lengths) in CASES.items():
        sigs = []
        for k, n in enumerate(lengths):
            t = np.arange(n) / 22050.0
            sigs.append((0.1 * (k - 2.5) + 0.25 * np.sin(2 * np.pi * (150 + 40 * k) * t) + 0.05 * g.normal(size=n)).astype(np.float32))
        out[case] = (np.concatenate(sigs), np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64))
    return out


def _transform(case):
    from multi_speaker_tts_amd.waveglow_feeder import Transform
    num_freq, fl, n_mel = CASES[case][0]
    return Transform(num_freq, 12.5, fl, n_mel, 16000, 4)


@pytest.fixture(scope="module")
def composed(dev, banks):
    """crop_batch_host of _table under every case and ratio, computed once: {(case, ratio): (audio [N, L], mel [N, F, n_mel])}."""
    from multi_speaker_tts_amd import waveglow_feeder as WF
    return {(case, ud): WF.crop_batch_host(*banks[case], _table(case), CASES[case][1], *ud, transform=_transform(case), device=dev)
            for case in CASES for ud in RATIOS}


def _crop_batch(dev, bank, table, case, ud, T):
    """One mstts_wg_crop_batch launch into NaN-filled outputs with a guard behind each -> (audio, mel, status)."""
    from multi_speaker_tts_amd import waveglow_feeder as WF
    samples, off = bank
    L, n_mel = CASES[case][1], CASES[case][0][2]
    bank_d, off_d = torch.tensor(samples, device=dev), torch.tensor(off, device=dev)
    table = np.ascontiguousarray(table, np.int32)
    table_d = torch.tensor(table, device=dev)
    N, guard = table.shape[0], 512
    bufs = []
    for size in (N * L, N * T * n_mel):
        b = torch.full((size + guard,), float("nan"), device=dev)
        b[size:] = 12345.0
        bufs.append(b)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    WF.crop_batch(bank_d, off_d, len(off) - 1, table_d, N, L, T, *ud, _transform(case), bufs[0], bufs[1], status)
    out = []
    for b, shape in zip(bufs, ((N, L), (N, T, n_mel))):
        h = b.cpu().numpy()
        size = int(np.prod(shape))
        assert np.all(h[size:] == 12345.0)                                        # nothing written behind the batch
        out.append(h[:size].reshape(shape))
    return out[0], out[1], int(status.item())


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("ud", RATIOS, ids=lambda ud: "%d_%d" % ud)
@pytest.mark.parametrize("case", ["ref", "small"])
def test_wg_crop_batch_matches_the_composed_path(dev, banks, composed, case, ud):
    from multi_speaker_tts_amd import waveglow_feeder as WF
    (samples, off), table, L = banks[case], _table(case), CASES[case][1]
    want_audio, want_mel = composed[case, ud]
    Lr, F = WF.crop_frames(L, *ud, _transform(case))
    assert want_mel.shape[1] == F and (case != "ref" or ud != (320, 441) or (Lr, F) == (5805, 30))
    # the audio by its definition: the bank's bits, +0.0 behind them
    by_hand = np.zeros((len(table), L), np.float32)
    for r, (f, start) in enumerate(table):
        c = min(L, int(off[f + 1] - off[f]) - start)
        by_hand[r, :c] = samples[off[f] + start:off[f] + start + c]
    assert _same_bits(want_audio, by_hand) and [int(np.count_nonzero(row)) < L for row in by_hand] == [True, False, False, False, False, True, False]
    for extra in (0, 3):                                                          # T = F; T = F + 3: every row is padded
        T = F + extra
        audio, mel, status = _crop_batch(dev, banks[case], table, case, ud, T)
        assert not np.isnan(audio).any() and not np.isnan(mel).any()              # every element was stored
        assert status == 0
        assert _same_bits(audio, by_hand)
        assert _same_bits(mel[:, :F], want_mel)                                   # mstts_wav_resample + mstts_stft_fft's bits
        assert _same_bits(mel[:, F:], np.zeros((len(table), extra, mel.shape[2]), np.float32))        # pad frames: +0.0
    for r in range(len(table)):                                                    # a row alone: the same bits as anywhere in the batch
        audio, mel, status = _crop_batch(dev, banks[case], table[r:r + 1], case, ud, F)
        assert status == 0 and _same_bits(audio[0], by_hand[r]) and _same_bits(mel[0], want_mel[r]), r


@pytest.mark.parametrize("case", ["ref", "small"])
def test_wg_crop_batch_against_fp64(dev, banks, case):
    """Rows without zero padding (frames over exact zeros sit on the 1e-5 floor of the dB scale, where no bound is meaningful) against
    scipy.signal.resample_poly in float64 followed by the fp64 oracle's mel.  The transform's own bound is 2e-3 absolute on [-4, 4] and
    does not include the resampler, so the composed path of the existing kernels is measured first against the same values and the new
    kernel is held to max(2e-3, twice that error); the factor 2 is headroom for the choice of worst element only."""
    from scipy.signal import resample_poly
    from multi_speaker_tts_amd import waveglow_feeder as WF
    (samples, off), L, ud = banks[case], CASES[case][1], (320, 441)
    num_freq, fl, n_mel = CASES[case][0]
    table = _table(case)[FULL_ROWS]
    F = WF.crop_frames(L, *ud, _transform(case))[1]
    ref = []
    for f, start in table:
        x = samples[off[f] + start:off[f] + start + L].astype(np.float64)
        assert x.shape[0] == L
        ref.append(OA.spectrogram_and_mel(resample_poly(x, *ud), num_freq, 12.5, fl, 16000, 20, n_mel, 4)[1].T)
    ref = np.stack(ref)
    assert ref.shape == (len(table), F, n_mel)
    _, composed_mel = WF.crop_batch_host(samples, off, table, L, *ud, transform=_transform(case), device=dev)
    _, mel, status = _crop_batch(dev, banks[case], table, case, ud, F)
    e_composed, e_kernel = np.abs(composed_mel - ref).max(), np.abs(mel - ref).max()
    print("waveglow_feeder_parity", case, "mel vs fp64 resample_poly + oracle: composed path", e_composed, "mstts_wg_crop_batch", e_kernel)
    assert status == 0 and e_kernel <= max(2e-3, 2 * e_composed)


def test_wg_crop_batch_flags_bad_rows(dev, banks, composed):
    from multi_speaker_tts_amd import waveglow_feeder as WF
    case, ud = "small", (320, 441)
    (samples, off), L = banks[case], CASES[case][1]
    lengths = np.diff(off)
    good = _table(case)[[4, 0, 5, 2]]
    want_audio, want_mel = (x[[4, 0, 5, 2]] for x in composed[case, ud])
    F = want_mel.shape[1]
    WF.check_table(good, lengths)
    for bad in ((-1, 0), (len(lengths), 0), (3, -1), (3, int(lengths[3]))):        # file -1; file n_files; start -1; start = len
        table = np.asarray([good[0], good[1], bad, good[2], good[3]], np.int32)
        with pytest.raises(ValueError):
            WF.check_table(table, lengths)                                         # refused on the host before any launch
        audio, mel, status = _crop_batch(dev, banks[case], table, case, ud, F)
        assert status & 1, bad
        assert not np.isnan(audio).any() and not np.isnan(mel).any()
        assert not audio[2].any() and not mel[2].any(), bad                        # the bad row: all zeros
        keep = [0, 1, 3, 4]
        assert _same_bits(audio[keep], want_audio) and _same_bits(mel[keep], want_mel), bad        # the good rows: unchanged
    table = np.asarray([good[0], (3, int(lengths[3]) - 1), good[1]], np.int32)     # start = len - 1: a crop of one sample is valid
    WF.check_table(table, lengths)
    audio, mel, status = _crop_batch(dev, banks[case], table, case, ud, F)
    assert status == 0 and audio[1, 0] == samples[off[4] - 1] and not audio[1, 1:].any()


def _write_corpus(root):
    """Eight wavs of 0.3 - 1.2 s of tones + noise at 48 kHz between 0.1 s of near silence on either side."""
    from scipy.io import wavfile
    g = np.random.default_rng(41)
    os.makedirs(root)
    paths = []
    for k in range(8):
        n = int(g.integers(14400, 57601))
        t = np.arange(n) / 48000.0
        y = sum(a * np.sin(2 * np.pi * (120.0 + 25 * k) * h * t + g.uniform(0, 6.28)) for h, a in ((1, 0.3), (2, 0.2), (3, 0.1), (7, 0.1)))
        y = np.concatenate([np.zeros(4800), y + g.normal(0, 0.02, n), np.zeros(4800)]) + g.normal(0, 1e-4, n + 9600)
        p = os.path.join(root, "p225_%03d.wav" % (k + 1)).replace("\\", "/")
        wavfile.write(p, 48000, np.clip(y * (0.5 + 0.05 * k) * 32767, -32767, 32767).astype(np.int16))
        paths.append(p)
    return paths


def test_waveglow_corpus_end_to_end(dev, tmp_path, monkeypatch):
    from multi_speaker_tts_amd import Audio, Feeder, Hyper_Parameters as hp
    from multi_speaker_tts_amd import taco1_feeder as TF
    from multi_speaker_tts_amd import waveglow as WG
    from multi_speaker_tts_amd import waveglow_feeder as WF
    from multi_speaker_tts_amd.WaveGlow import WaveGlow
    tr = hp.WaveGlow.Train
    L, B = 640, 3
    monkeypatch.setattr(hp.Sound, "Spectrogram_Dim", 257)
    monkeypatch.setattr(hp.Sound, "Frame_Length", 25)
    monkeypatch.setattr(hp.WaveGlow, "Checkpoint_Path", str(tmp_path / "wg"))
    monkeypatch.setattr(tr, "Pattern_Path", str(tmp_path / "wav48"))
    monkeypatch.setattr(tr, "Batch_Size", B)
    monkeypatch.setattr(tr, "Max_Signal_Length", L)
    monkeypatch.setattr(tr, "Checkpoint_Save_Timing", 2)
    monkeypatch.delenv("MSTTS_WG_FEEDER", raising=False)
    paths = _write_corpus(str(tmp_path / "wav48"))

    # the bank: the front end's waveform of every file, bit for bit, at a peak of 0.99
    bank = WF.bank_from_wavs(paths, device=dev, chunk=3)
    assert isinstance(bank, TF.SignalBank) and bank.names == paths
    decoded = [Feeder.decode_wav(p, "scipy") for p in paths]
    want = Audio.wav_front_end([d for _, d in decoded], [48000] * 8, 22050, top_db=15, frame=32, hop=16, scale=0.99, peak_normalize=True,
                               device=dev, rule="scipy")
    bank_host = t2n(bank.bank)
    for k, (a, b, s) in enumerate(zip(bank._offsets, bank._offsets[1:], want)):
        assert _same_bits(bank_host[int(a):int(b)], s), k
        assert 22050 * 0.25 < s.shape[0] < 22050 * 1.3                             # trimmed: the 0.1 s of near silence on either side is gone
        assert abs(float(np.abs(s).max()) - 0.99) <= 2.0 ** -22                    # fp32(0.99) / peak * peak: three roundings of 2^-24
    assert bank.lengths.min() > L

    # one seed: over one epoch the feeder delivers crop_batch_host of the same plan, bit for bit
    d = WG.WGDims(n_mel=80, flows=4, groups=8, early_every=2, early_size=2, up_k=1024, up_stride=256, layers=3, ch=32, k=3)
    feeder = WF.WaveGlowFeeder(bank, seed=1234, dims=d)
    assert (feeder.L, feeder.up, feeder.down, feeder.Lr, feeder.F) == (L, 320, 441, 465, 3)
    rng = np.random.default_rng(1234)
    groups = TF.epoch_batches(rng, range(8), bank.lengths, B, False)
    assert sorted(len(x) for x in groups) == [2, 3, 3]
    first = None
    for group in groups:
        table = WF.crop_plan(rng, bank.lengths, group, L)
        got = feeder.Get_Train_Pattern()
        want_audio, want_mel = WF.crop_batch_host(bank_host, bank._offsets, table, L, 320, 441, device=dev)
        assert sorted(got) == ["Audio", "Mel"] and got["Audio"].is_cuda and got["Mel"].shape == (len(group), 3, 80)
        assert _same_bits(t2n(got["Audio"]), want_audio) and _same_bits(t2n(got["Mel"]), want_mel)
        first = first or {"Audio": want_audio, "Mel": want_mel}
    feeder.check_status()
    with pytest.raises(ValueError):                                                # restructure() refuses (L, F): 24 upsampled samples for 640
        WF.WaveGlowFeeder(bank, dims=WG.WGDims(n_mel=80, flows=4, groups=8, early_every=2, early_size=2, up_k=16, up_stride=4, layers=3, ch=32, k=3))

    # Train() on the bank: finite losses, step 0 is Train_Step on that first batch, a checkpoint
    values = WG.random_values(d, seed=5)
    m = WaveGlow(device=dev, dims=d, values=values, feeder="device")
    results, step = [], m.Train_Step
    monkeypatch.setattr(m, "Train_Step", lambda pattern=None: (lambda r: (results.append(r), r)[1])(step(pattern)))
    m.Train(max_steps=4)
    assert isinstance(m.feeder, WF.WaveGlowFeeder) and len(results) == 4 and m.engine.global_step == 4
    m.feeder.check_status()
    keys = ("Log_S_Loss", "Log_Det_W_Loss", "Audio_Loss")
    print("losses", [[r[k] for k in keys] for r in results])
    assert np.all(np.isfinite([[r[k] for k in keys] for r in results]))
    by_hand = WaveGlow(device=dev, dims=d, values=values).Train_Step(first)
    # The same batch and variables.  N Lg = 3 * 80 = 240 rows: every coupling launch and the audio loss's launch (1 920 elements) is ONE
    # workgroup, so those two sums are atomic adds of one partial per launch in stream order: fixed.  The log-determinant is one launch
    # with a workgroup per flow, each adding its term in arrival order: each of the flows - 1 additions errs by at most 2^-24 of a running
    # sum that is at most sum_f |term_f|, in either run; the loss is that sum times N Lg / (N Lg groups).
    assert results[0]["Log_S_Loss"] == by_hand["Log_S_Loss"] and results[0]["Audio_Loss"] == by_hand["Audio_Loss"]
    terms = [abs(np.log(np.linalg.det(1e3 * np.asarray(v, np.float64).reshape(v.shape[-2:])) + 1e-6) - v.shape[-1] * np.log(1e3))
             for k, v in values.items() if k.endswith("invertible_1x1/kernel")]
    assert len(terms) == d.flows
    bound = 2 * (d.flows - 1) * 2.0 ** -24 * sum(terms) / d.groups
    print("step 0 log det", results[0]["Log_Det_W_Loss"], "by hand", by_hand["Log_Det_W_Loss"], "bound", bound)
    assert abs(results[0]["Log_Det_W_Loss"] - by_hand["Log_Det_W_Loss"]) <= bound
    assert os.path.exists(tmp_path / "wg" / "waveglow.pt")
    assert torch.load(tmp_path / "wg" / "waveglow.pt", map_location="cpu")["__global_step__"] == 4
