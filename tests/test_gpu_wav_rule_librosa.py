"""The waveform front end by librosa's rules on the MI355X (csrc/wav_front_end.hip; Audio.resample_kaiser_best_batch,
trim_bounds_batch / wav_front_end / wav_features with rule="librosa", Feeder.load_wav_batch and Get_Inference_Pattern) against the
float64 host rules of tests/test_cpu_wav_rule_librosa.py.

The resampler's bound.  The device multiplies an fp32 copy of the float64 table against fp32 samples in one fmaf chain of `taps` steps.
With u = 2^-24: rounding the table moves an output by at most u sum_i |c_i| |x_i| <= u S max|x| (S = the largest row sum of |table|),
and each of the `taps` fmaf steps rounds a partial sum that never exceeds S max|x| (up to a factor 1 + taps u), adding at most
u S max|x| each.  Together (taps + 1) 2^-24 S max|x|: 5.4e-5 max|x| at 386 taps (S = 2.33), 1.1e-4 at the 772 taps of 1 : 6.
The measured errors are in profiles/r10_wav_rule_librosa_parity.txt."""
import os
import warnings

import numpy as np
import pytest
import torch

from tests.test_cpu_wav_front_end import envelope_ratios, voiced
from tests.test_cpu_wav_rule_librosa import MARGIN_DB, TRIM_FRAMES, TRIM_KATS, TRIM_RATES, host_kaiser_best, trim_reference_centred

pytestmark = pytest.mark.gpu

FIR_RATIOS = envelope_ratios() + [r for r in ((147, 160), (1, 6), (2, 1)) if r not in envelope_ratios()]
LENGTHS = (1, 37, 0, 1500, 5000)                             # one call; the zero-length waveform sits in the middle
FILE_SEED = 11                                               # chosen on the CPU as TRIM_SEED was: `_assert_decided` states the precondition


def fir_bound(up, down):
    """(taps + 1) 2^-24 max_r sum |row_r| - times max |x| it bounds |device - float64 table form| (module docstring)."""
    from multi_speaker_tts_amd import Audio
    table = Audio.kaiser_best_table(up, down)
    return (table.shape[1] + 1) * 2.0 ** -24 * np.abs(table).sum(axis=1).max()


def _noise(n, seed):
    return np.random.default_rng(seed).normal(size=n).astype(np.float32)


@pytest.mark.parametrize("up,down", FIR_RATIOS)
def test_fir_resampler_against_the_float64_table_form(dev, up, down):
    from multi_speaker_tts_amd import Audio
    sigs = [_noise(n, 300 + i) for i, n in enumerate(LENGTHS)]
    bound = fir_bound(up, down)
    got = Audio.resample_kaiser_best_batch(sigs, down, up, device=dev)
    worst = 0.0
    for x, y in zip(sigs, got):
        n_valid, n_out = Audio.kaiser_best_out_len(x.shape[0], up, down)
        ref = Audio.resample_kaiser_best(x.astype(np.float64), up, down)
        assert y.dtype == np.float32 and y.shape == ref.shape == (n_out,), (x.shape, y.shape, ref.shape)
        assert not y[n_valid:].any()                                                       # fix_length's zeros, exactly
        if n_out:
            err = np.abs(y - ref).max() / np.abs(x).max()
            worst = max(worst, err)
            print("kaiser_best %d:%d, n = %d -> %d valid of %d: max |dev - fp64| / max |x| = %.3g" % (up, down, x.shape[0], n_valid, n_out, err))
    print("kaiser_best %d:%d: taps %d, worst %.3g, bound %.3g" % (up, down, Audio.kaiser_best_table(up, down).shape[1], worst, bound))
    assert worst <= bound
    again = Audio.resample_kaiser_best_batch(sigs, down, up, device=dev)
    alone = [Audio.resample_kaiser_best_batch([s], down, up, device=dev)[0] for s in sigs]
    assert all(np.array_equal(a, b) for a, b in zip(got, again))                           # run to run
    assert all(np.array_equal(a, b) for a, b in zip(got, alone))                           # alone / in the batch


@pytest.mark.parametrize("up,down", ((320, 441), (1, 3), (441, 160)))
def test_fir_tilings_give_the_same_bits(dev, up, down):
    """Phase-major (rows and span in LDS) and row-major (rows through L1 / L2) on ratios both serve: one fmaf chain per output either way."""
    from multi_speaker_tts_amd import Audio, lib
    assert lib.load().mstts_wav_resample_fir_supported(up, down, Audio.kaiser_best_table(up, down).shape[1]) == 2
    sigs = [_noise(n, 400 + i) for i, n in enumerate((5000, 0, 37, 12001))]
    auto, row, phase = (Audio.resample_kaiser_best_batch(sigs, down, up, device=dev, tiling=t) for t in (0, 1, 2))
    for a, r, p in zip(auto, row, phase):
        assert np.array_equal(r, p) and np.array_equal(a, p)


def test_fir_row_major_serves_a_row_longer_than_lds(dev):
    """A synthetic 2-row table of 20 001 taps (80 KB a row: the phase-major tiling cannot hold it) through the entry point itself,
    against the same sum in float64."""
    from multi_speaker_tts_amd import Audio, lib
    up, down, taps = 2, 3, 20001
    assert lib.load().mstts_wav_resample_fir_supported(up, down, taps) == 1
    g = np.random.default_rng(7)
    table = (g.normal(size=(up, taps)) / taps).astype(np.float32)
    x = _noise(12000, 8)
    n_out, n_valid, origin = 6000, 5990, 5 * up
    buf = torch.cat([torch.as_tensor(x), torch.full((n_out,), float("nan"))]).to(dev)
    meta = torch.as_tensor(np.asarray([0, 12000, 12000, 12000 + n_out, n_valid], np.int64)).to(dev)
    tab = torch.as_tensor(table.reshape(-1)).to(dev)
    lib.call("mstts_wav_resample_fir", lib.ptr(buf), lib.ptr(meta, 0), lib.ptr(meta, 2), lib.ptr(meta, 4), 1, n_out, lib.ptr(tab), up, down, taps,
             origin, 0, lib.ptr(buf))
    y = buf[12000:].cpu().numpy()
    xp = np.concatenate([np.zeros(taps), x.astype(np.float64), np.zeros(taps)])
    m = np.arange(n_valid)
    q = origin + m * down
    ref = np.asarray([np.dot(table[qq % up].astype(np.float64), xp[qq // up + 1:qq // up + 1 + taps]) for qq in q[::97]])
    err = np.abs(y[:n_valid:97] - ref).max() / np.abs(x).max()
    bound = (taps + 1) * 2.0 ** -24 * np.abs(table).sum(axis=1).max()
    print("row-major, %d taps: max |dev - fp64| / max |x| = %.3g (bound %.3g)" % (taps, err, bound))
    assert err <= bound and not y[n_valid:].any() and np.isfinite(y).all()


@pytest.mark.parametrize("frame,hop", TRIM_FRAMES)
def test_centred_trim_against_the_float64_restatement(dev, frame, hop):
    from multi_speaker_tts_amd import Audio
    xs = [host_kaiser_best(rate, 16000) for rate in TRIM_RATES]
    refs = [trim_reference_centred(x, 15.0, frame, hop) for x in xs]
    for rate, (s, e, margin) in zip(TRIM_RATES, refs):                                     # the precondition, on the reference, first
        print("%d -> 16000, frame %d: reference [%d, %d), deciding frames >= %.4f dB from the threshold" % (rate, frame, s, e, margin))
        assert margin >= MARGIN_DB
    start, end, peak = Audio.trim_bounds_batch(xs, 15.0, frame, hop, device=dev, rule="librosa")
    for k, (x, (s, e, _)) in enumerate(zip(xs, refs)):
        want_peak = np.abs(x[s:e]).max()
        print("%d: device [%d, %d) peak %.9g, reference [%d, %d) peak %.9g" % (TRIM_RATES[k], start[k], end[k], peak[k], s, e, want_peak))
        assert (start[k], end[k]) == (s, e) and peak[k] == want_peak
    one = Audio.trim_bounds_batch(xs[2:3], 15.0, frame, hop, device=dev, rule="librosa")
    assert (one[0][0], one[1][0], one[2][0]) == (start[2], end[2], peak[2])
    old = Audio.trim_bounds_batch(xs, 15.0, frame, hop, device=dev, rule="scipy")
    assert np.array_equal(old[0], Audio.trim_bounds_batch(xs, 15.0, frame, hop, device=dev)[0])    # the default is today's trim


def test_centred_trim_kats_on_the_device(dev):
    from multi_speaker_tts_amd import Audio
    by_frame = {}
    for name, (x, frame, hop, want) in TRIM_KATS.items():
        by_frame.setdefault((frame, hop), []).append((name, x.astype(np.float32), want))
    for (frame, hop), cases in by_frame.items():                                           # one call per frame size, the empty waveform inside it
        start, end, peak = Audio.trim_bounds_batch([x for _, x, _ in cases], 15.0, frame, hop, device=dev, rule="librosa")
        for k, (name, x, want) in enumerate(cases):
            want_peak = np.abs(x[want[0]:want[1]]).max() if want[1] > want[0] else 0.0
            print("%s: device [%d, %d) peak %g, by hand %s" % (name, start[k], end[k], peak[k], want))
            assert (start[k], end[k]) == want and peak[k] == np.float32(want_peak), name
    x = voiced(16000, seconds=0.5, seed=2).astype(np.float32) / 32768.0                    # frame 2048 on a wave per frame, hop 1 on 8001 frames
    for frame, hop in ((2048, 512), (33, 7), (256, 1)):
        s, e, margin = trim_reference_centred(x, 15.0, frame, hop)
        start, end, peak = Audio.trim_bounds_batch([x], 15.0, frame, hop, device=dev, rule="librosa")
        print("0.5 s, frame %d hop %d: device [%d, %d), reference [%d, %d), margin %.3f dB" % (frame, hop, start[0], end[0], s, e, margin))
        assert margin >= MARGIN_DB and (start[0], end[0]) == (s, e) and peak[0] == np.abs(x[s:e]).max()


def _write_files(tmp_path):
    """48 kHz int16, 22.05 kHz int16, 16 kHz float32 -> paths."""
    from scipy.io import wavfile
    paths = []
    for name, rate, seconds, as_float in (("a48.wav", 48000, 3.5, False), ("b22.wav", 22050, 2.5, False), ("c16.wav", 16000, 3.5, True)):
        x = voiced(rate, seconds=seconds, seed=FILE_SEED)
        p = str(tmp_path / name)
        wavfile.write(p, rate, (x.astype(np.float32) / 32768.0) if as_float else x)
        paths.append(p)
    return paths


def _assert_decided(paths, frame=32, hop=16):
    """The precondition of every comparison of trimmed lengths, on the float64 host rules alone: each deciding frame of the
    host-converted samples lies at least 0.01 dB from the threshold."""
    from multi_speaker_tts_amd import Audio, Feeder
    for p in paths:
        rate, x = Feeder.decode_wav(p, rule="librosa")
        if rate != 16000:
            x = Audio.resample_kaiser_best(x, *Audio.resample_ratio(rate, 16000)).astype(np.float32)
        margin = trim_reference_centred(x, 15.0, frame, hop)[2]
        print("%s -> 16000 Hz, frame %d: deciding frames >= %.4f dB from the threshold" % (os.path.basename(p), frame, margin))
        assert margin >= MARGIN_DB, p


def test_load_wav_batch_against_load_wav(dev, tmp_path):
    from multi_speaker_tts_amd import Audio, Feeder
    paths = _write_files(tmp_path)
    _assert_decided(paths)
    got = Feeder.load_wav_batch(paths, sample_rate=16000, device=dev, rule="librosa")
    for p, y in zip(paths, got):
        ref = Feeder.load_wav(p, sample_rate=16000, rule="librosa")
        rate, x = Feeder.decode_wav(p, rule="librosa")
        assert y.dtype == np.float32 and y.shape == ref.shape, (p, y.shape, ref.shape)
        if rate == 16000:
            assert np.array_equal(y, ref)                                                  # no conversion: the same bits
            continue
        bound = 0.99 * fir_bound(*Audio.resample_ratio(rate, 16000)) * np.abs(x).max()
        err = np.abs(y - ref).max()
        print("%s (%d Hz): %d samples, max |dev - host| = %.3g (bound %.3g)" % (os.path.basename(p), rate, y.shape[0], err, bound))
        assert err <= bound
    default = Feeder.load_wav_batch(paths, sample_rate=16000, device=dev)
    assert all(np.array_equal(a, b) for a, b in zip(default, Feeder.load_wav_batch(paths, sample_rate=16000, device=dev, rule="scipy")))
    assert default[0].shape != got[0].shape or not np.array_equal(default[0], got[0])


def _mel_args():
    from multi_speaker_tts_amd import Hyper_Parameters as hp
    return dict(num_freq=hp.Sound.Spectrogram_Dim, frame_shift_ms=hp.Sound.Frame_Shift, frame_length_ms=hp.Sound.Frame_Length,
                num_mels=hp.Sound.Mel_Dim, sample_rate=hp.Sound.Sample_Rate)


def test_wav_features_mels_and_one_host_read(dev, tmp_path):
    """Mels of the device front end under the rule against load_wav(rule="librosa") + Audio.melspectrogram (2e-3, the bound of
    tests/test_gpu_wav_front_end.py for the same comparison), and at most one synchronisation between upload and feature launch,
    counted under torch's sync debug mode after the switch is proven on a plain .item()."""
    from multi_speaker_tts_amd import Audio, Feeder, Hyper_Parameters as hp
    paths = _write_files(tmp_path)
    _assert_decided(paths)
    decoded = [Feeder.decode_wav(p, rule="librosa") for p in paths]
    sigs, rates = [d for _, d in decoded], [r for r, _ in decoded]
    feats, lens = Audio.wav_features(sigs, rates, max_abs_value=hp.Sound.Max_Abs_Mel, device=dev, return_lengths=True, rule="librosa", **_mel_args())
    worst = 0.0
    for p, (mel, spec), n in zip(paths, feats, lens):
        sig = Feeder.load_wav(p, rule="librosa")
        ref = Audio.melspectrogram(y=sig, max_abs_value=hp.Sound.Max_Abs_Mel, device=dev, **_mel_args()).T
        assert spec is None and n == sig.shape[0] and mel.shape == ref.shape, (p, n, sig.shape, mel.shape, ref.shape)
        worst = max(worst, np.abs(mel - ref).max())
    print("wav_features(rule='librosa'): worst |mel(device front end) - mel(host front end)| = %.3g (bound 2e-3)" % worst)
    assert worst <= 2e-3
    run = lambda: Audio.wav_features(sigs, rates, max_abs_value=hp.Sound.Max_Abs_Mel, device=dev, return_tensor=True, rule="librosa", **_mel_args())
    run()
    torch.cuda.synchronize()
    probe = torch.ones(3, device=dev)
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            probe.sum().item()
        proof = [w for w in seen if "synchroniz" in str(w.message).lower()]
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            out = run()
        syncs = [w for w in seen if "synchroniz" in str(w.message).lower()]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    print("sync debug mode: .item() warned %d time(s); wav_features(rule='librosa') warned %d time(s)" % (len(proof), len(syncs)))
    assert len(proof) >= 1, "torch.cuda.set_sync_debug_mode('warn') does not report a plain .item() in this build: the check cannot be made"
    assert len(syncs) <= 1
    assert all(m.is_cuda and m.shape[1] == hp.Sound.Mel_Dim for m, _ in out)


def test_inference_pattern_under_the_rule(dev, tmp_path, monkeypatch):
    from tests.test_gpu_wav_front_end import _small_tacotron
    monkeypatch.delenv("MSTTS_WAV_FRONT_END", raising=False)
    monkeypatch.delenv("MSTTS_WAV_RULE", raising=False)
    dims, t = _small_tacotron(dev, tmp_path, monkeypatch)
    paths = _write_files(tmp_path)
    _assert_decided(paths)
    texts = ["Please call Stella.", "Who knows?", "His voice is tested now."]
    host = t.feeder.Get_Inference_Pattern(paths, texts, front_end="host", rule="librosa")
    device = t.feeder.Get_Inference_Pattern(paths, texts, front_end="device", rule="librosa")
    assert device["Speaker_Embedding_Mel"].shape == host["Speaker_Embedding_Mel"].shape and device["Speaker_Embedding_Mel"].dtype == np.float32
    err = np.abs(device["Speaker_Embedding_Mel"] - host["Speaker_Embedding_Mel"]).max()
    print("Get_Inference_Pattern(rule='librosa'): max |windows(device) - windows(host)| = %.3g (bound 2e-3)" % err)
    assert err <= 2e-3
    for front_end in ("host", "device"):                                                   # rule "scipy" is the front end as it was
        plain = t.feeder.Get_Inference_Pattern(paths, texts, front_end=front_end)
        scipy_rule = t.feeder.Get_Inference_Pattern(paths, texts, front_end=front_end, rule="scipy")
        for k in plain:
            assert np.array_equal(plain[k], scipy_rule[k]), (front_end, k)
        assert not np.array_equal(plain["Speaker_Embedding_Mel"], host["Speaker_Embedding_Mel"])
    monkeypatch.setenv("MSTTS_WAV_RULE", "librosa")
    env = t.feeder.Get_Inference_Pattern(paths, texts, front_end="host")
    assert np.array_equal(env["Speaker_Embedding_Mel"], host["Speaker_Embedding_Mel"])
    monkeypatch.delenv("MSTTS_WAV_RULE")
    from oracle import model as OM, train as OT
    od = OM.Dims(**{f: getattr(dims, f) for f in ("emb", "enc_conv_ch", "enc_lstm", "spk", "prenet", "dec_lstm", "post_ch", "bank_ch", "proj1_ch",
                                                 "birnn", "spk_lstm", "max_inf")})
    masks = {k: v.numpy() for k, v in OT.make_masks(od, 3, host["Token"].shape[1], od.max_inf + 1, False, seed=31).items()}
    out = t.Inference(paths, texts, masks=masks, export=False, front_end="device", wav_rule="librosa")
    assert out["Mel"].shape[0] == 3 and np.isfinite(out["Mel"]).all()
