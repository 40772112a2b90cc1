"""The waveform front end on the MI355X (csrc/wav_front_end.hip, Audio.wav_front_end / wav_features, Feeder.load_wav_batch and the
surfaces that use them) against the host path it replaces: scipy.signal.resample_poly in float64, Feeder.load_wav, and
Audio.melspectrogram on load_wav's output.  Every figure is printed before it is asserted.

Bounds.  Resampler: max |y_dev - y_ref| <= 1e-5 max |x|.  An fp32 sum of T products errs by at most (T + 1) 2^-24 sum|h_phase| max|x|;
over the ten ratios of the envelope T <= 61 and sum|h_phase| <= 2.2415 (asserted in tests/test_cpu_wav_front_end.py), i.e. 8.3e-6,
the fp32 rounding of the taps included.  load_wav_batch against load_wav: both sides are fp32 evaluations of the same sum, so twice
that, times the 0.99 scale.  Mels: the 2e-3 tests/test_gpu_model.py gives a mel against the oracle on the [-4, 4] scale.
Measured on the MI355X (profiles/r09_wav_front_end_parity.txt): resampler 1.6e-7 - 3.2e-7 of max |x| over the ten ratios, bit-equal alone,
in a batch and run to run; trim bounds and peaks equal; load_wav_batch 3.0e-7; mels 2.6e-5 (wav_features), 2.5e-5 (speaker windows),
3.3e-5 / 4.0e-5 (Mel_Generate_Batch without / with spectral subtraction); one synchronisation warning around wav_features."""
import os
import warnings

import numpy as np
import pytest
import torch

from tests.test_cpu_wav_front_end import MARGIN_DB, SOURCE_RATES, TARGET_RATES, TRIM_CASES, envelope_ratios, host_resampled, trim_reference, voiced

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 31, 441, 4001, 96000)


def _signal(n, seed):
    g = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    return (0.5 * np.sin(2 * np.pi * 220 * t + g.random()) + 0.2 * g.normal(size=n)).astype(np.float32)


@pytest.mark.parametrize("up,down", envelope_ratios())
def test_resampler_against_scipy_fp64(dev, up, down):
    from scipy.signal import resample_poly
    from multi_speaker_tts_amd import Audio
    sigs = [_signal(n, 100 + i) for i, n in enumerate(LENGTHS)]
    worst = 0.0
    for x in sigs:                                                                         # each length alone
        y, = Audio.resample_poly_batch([x], up, down, device=dev)
        ref = resample_poly(x.astype(np.float64), up, down)
        assert y.dtype == np.float32 and y.shape == ref.shape, (x.shape, y.shape, ref.shape)
        err = np.abs(y - ref).max() / np.abs(x).max()
        worst = max(worst, err)
        print("resample %d/%d, n = %d -> %d: max |dev - fp64| / max |x| = %.3g" % (up, down, x.shape[0], y.shape[0], err))
    mixed = [sigs[3], sigs[5], sigs[0], sigs[4], sigs[2]]                                  # a batch of mixed lengths
    for x, y in zip(mixed, Audio.resample_poly_batch(mixed, up, down, device=dev)):
        ref = resample_poly(x.astype(np.float64), up, down)
        assert y.shape == ref.shape
        err = np.abs(y - ref).max() / np.abs(x).max()
        worst = max(worst, err)
        print("resample %d/%d, batch member n = %d: %.3g" % (up, down, x.shape[0], err))
    print("resample %d/%d: worst %.3g (bound 1e-5)" % (up, down, worst))
    assert worst <= 1e-5


def test_resampler_batch_independence(dev):
    from multi_speaker_tts_amd import Audio
    lens = (96000, 17, 4001, 1, 30011, 441, 2)
    sigs = [_signal(n, 200 + i) for i, n in enumerate(lens)]
    for up, down in ((1, 3), (320, 441), (441, 160)):
        a = Audio.resample_poly_batch(sigs, up, down, device=dev)
        b = Audio.resample_poly_batch(sigs, up, down, device=dev)
        same_run = all(np.array_equal(x, y) for x, y in zip(a, b))
        alone = [Audio.resample_poly_batch([s], up, down, device=dev)[0] for s in sigs]
        same_alone = [bool(np.array_equal(x, y)) for x, y in zip(a, alone)]
        print("resample %d/%d: two runs bit-equal %s, batch member == alone %s" % (up, down, same_run, same_alone))
        assert same_run and all(same_alone)


def test_default_resampler_is_the_fir_at_a_fixed_origin(dev):
    """mstts_wav_resample gives the bits of mstts_wav_resample_fir fed the float32 `resample_phase_table`, taps = `resample_taps`,
    origin = 10 max(up, down) and n_valid = the output lengths, under the row-major and the phase-major tiling: the default rule IS that
    FIR at a fixed origin, and keeps a kernel of its own only for speed.  One batch of 1 (shorter than a filter row), 700
    (shorter than a tile) and 5 000 samples (several workgroups)."""
    from multi_speaker_tts_amd import Audio, lib
    lens = (1, 700, 5000)
    x = torch.as_tensor(np.concatenate([_signal(n, 500 + i) for i, n in enumerate(lens)]))
    for up, down in ((1, 3), (320, 441), (2, 1)):
        assert (up, down) in envelope_ratios() and Audio.resample_supported(up, down)
        out_lens = [Audio.resample_out_len(n, up, down) for n in lens]
        in_off = np.concatenate([[0], np.cumsum(lens)])
        out_off = in_off[-1] + np.concatenate([[0], np.cumsum(out_lens)])
        meta = torch.as_tensor(np.concatenate([in_off, out_off, out_lens]).astype(np.int64)).to(dev)      # 4 + 4 + 3 words
        table = torch.as_tensor(Audio.resample_phase_table(up, down).astype(np.float32).reshape(-1)).to(dev)
        taps, origin = Audio.resample_taps(up, down), 10 * max(up, down)
        got = []
        for tiling in (None, 1, 2):                                                        # None: mstts_wav_resample
            buf = torch.cat([x, torch.full((sum(out_lens),), float("nan"))]).to(dev)
            if tiling is None:
                lib.call("mstts_wav_resample", lib.ptr(buf), lib.ptr(meta, 0), lib.ptr(meta, 4), 3, max(out_lens), lib.ptr(table), up, down, lib.ptr(buf))
            else:
                assert lib.load().mstts_wav_resample_fir_supported(up, down, taps) == 2
                lib.call("mstts_wav_resample_fir", lib.ptr(buf), lib.ptr(meta, 0), lib.ptr(meta, 4), lib.ptr(meta, 8), 3, max(out_lens), lib.ptr(table),
                         up, down, taps, origin, tiling, lib.ptr(buf))
            got.append(buf[in_off[-1]:].cpu().numpy())
        same = [bool(np.array_equal(got[0].view(np.uint32), g.view(np.uint32))) for g in got[1:]]
        print("resample %d/%d: %d outputs, mstts_wav_resample == FIR row-major %s, == FIR phase-major %s" % (up, down, got[0].shape[0], *same))
        assert np.isfinite(got[0]).all() and all(same)


@pytest.mark.parametrize("frame,hop", ((32, 16), (2048, 512)))
def test_trim_against_fp64_restatement(dev, frame, hop):
    """trim_bounds_batch on the float32 arrays load_wav trims (host rate conversion, uploaded as they are): start and end of the fp64
    restatement, the peak exactly."""
    from multi_speaker_tts_amd import Audio
    cases = sorted({(r, t) for r, t, _, _ in TRIM_CASES})
    xs = [host_resampled(r, t) for r, t in cases]
    refs = [trim_reference(x, 15.0, frame, hop) for x in xs]
    for (r, t), (s, e, margin) in zip(cases, refs):                                        # the precondition, on the reference, first
        print("%d -> %d, frame %d: reference [%d, %d), deciding frames >= %.4f dB from the threshold" % (r, t, frame, s, e, margin))
        assert margin >= MARGIN_DB
    start, end, peak = Audio.trim_bounds_batch(xs, 15.0, frame, hop, device=dev)
    for k, (x, (s, e, _)) in enumerate(zip(xs, refs)):
        want_peak = np.abs(x[s:e]).max()
        print("%s: device [%d, %d) peak %.9g, reference [%d, %d) peak %.9g" % (cases[k], start[k], end[k], peak[k], s, e, want_peak))
        assert (start[k], end[k]) == (s, e) and peak[k] == want_peak
    one = Audio.trim_bounds_batch(xs[3:4], 15.0, frame, hop, device=dev)
    assert (one[0][0], one[1][0], one[2][0]) == (start[3], end[3], peak[3])


def _load_wav_trim(x, top_db, frame, hop):
    """load_wav's own float32 arithmetic on decoded samples -> (start, end)."""
    data = np.asarray(x, np.float32)
    if data.shape[0] >= frame:
        n = 1 + (data.shape[0] - frame) // hop
        idx = np.arange(frame)[None, :] + hop * np.arange(n)[:, None]
        rms = np.sqrt((data[idx] ** 2).mean(axis=1))
        db = 20.0 * np.log10(np.maximum(rms, 1e-10) / max(rms.max(), 1e-10))
        keep = np.nonzero(db > -top_db)[0]
        if keep.size:
            return int(keep[0] * hop), int(min(data.shape[0], (keep[-1] + 1) * hop))
    return 0, int(data.shape[0])


def test_trim_edge_cases(dev):
    from multi_speaker_tts_amd import Audio
    g = np.random.default_rng(5)
    quiet = lambda n: (1e-4 * g.normal(size=n)).astype(np.float32)
    loud = lambda n: (0.5 * g.normal(size=n)).astype(np.float32)
    cases = {"shorter than a frame": loud(20), "all zeros": np.zeros(500, np.float32),
             "loud frame at the very start": np.concatenate([loud(32), quiet(1000)]),
             "loud frame at the very end": np.concatenate([quiet(1003), loud(32)]),       # len - frame = 1003: no multiple of hop
             "len - frame not a multiple of hop": np.concatenate([quiet(300), loud(400), quiet(309)]),
             "exactly one frame": loud(32)}
    names, xs = list(cases), list(cases.values())
    start, end, peak = Audio.trim_bounds_batch(xs, 15.0, 32, 16, device=dev)
    for k, name in enumerate(names):
        s, e = _load_wav_trim(xs[k], 15.0, 32, 16)
        rs, re_, margin = trim_reference(xs[k], 15.0, 32, 16)
        want_peak = np.abs(xs[k][s:e]).max() if e > s else 0.0
        print("%s: device [%d, %d) peak %.9g; load_wav's rule [%d, %d) peak %.9g; fp64 margin %s" % (name, start[k], end[k], peak[k], s, e, want_peak, margin))
        assert (rs, re_) == (s, e) and (margin is None or margin >= MARGIN_DB)
        assert (start[k], end[k]) == (s, e) and peak[k] == np.float32(want_peak)
    assert (start[0], end[0]) == (0, 20) and (start[1], end[1]) == (0, 480) and start[2] == 0 and end[3] == 1008


def _write_test_wavs(tmp_path):
    """int16 mono at 16 000 / 22 050 / 48 000 Hz, one stereo, one uint8 -> paths."""
    from scipy.io import wavfile
    paths = []
    def put(name, rate, data):
        p = str(tmp_path / name)
        wavfile.write(p, rate, data)
        paths.append(p)
    put("a16.wav", 16000, voiced(16000))
    put("b22.wav", 22050, voiced(22050, seconds=4.0))
    put("c48.wav", 48000, voiced(48000))
    x = voiced(48000, seconds=3.0)
    put("d48_stereo.wav", 48000, np.stack([x, (x // 3).astype(np.int16)], axis=1))
    y = voiced(22050, seconds=3.0)
    put("e22_u8.wav", 22050, ((y.astype(np.int32) >> 8) + 128).astype(np.uint8))
    put("f16.wav", 16000, voiced(16000, seconds=2.5))
    return paths


def _assert_trim_is_decided(paths, target, frame, hop):
    """The precondition of every comparison of trimmed lengths: on the host-converted samples, in the fp64 restatement, each deciding
    frame is at least 0.01 dB from the threshold."""
    from scipy.signal import resample_poly
    from multi_speaker_tts_amd import Audio, Feeder
    for p in paths:
        rate, x = Feeder.decode_wav(p)
        if rate != target:
            x = resample_poly(x, *Audio.resample_ratio(rate, target)).astype(np.float32)
        margin = trim_reference(x, 15.0, frame, hop)[2]
        print("%s -> %d Hz, frame %d: deciding frames >= %.4f dB from the threshold" % (os.path.basename(p), target, frame, margin))
        assert margin >= MARGIN_DB, p


def test_load_wav_batch_against_load_wav(dev, tmp_path):
    from multi_speaker_tts_amd import Feeder
    paths = _write_test_wavs(tmp_path)
    _assert_trim_is_decided(paths, 16000, 32, 16)
    _assert_trim_is_decided(paths[:3], 22050, 2048, 512)
    got = Feeder.load_wav_batch(paths, device=dev)
    worst = 0.0
    for p, y in zip(paths, got):
        ref = Feeder.load_wav(p)
        rate, x = Feeder.decode_wav(p)
        assert y.dtype == np.float32 and y.shape == ref.shape, (p, y.shape, ref.shape)
        err = np.abs(y - ref).max() / (0.99 * np.abs(x).max())
        worst = max(worst, err)
        print("%s (%d Hz): %d samples, max |dev - host| / (0.99 max |x|) = %.3g" % (os.path.basename(p), rate, y.shape[0], err))
    print("load_wav_batch: worst %.3g (bound 2e-5)" % worst)
    assert worst <= 2e-5
    for k in (0, 5):                                                                       # no rate conversion: the same bits
        assert np.array_equal(got[k], Feeder.load_wav(paths[k]))
    at22 = Feeder.load_wav_batch(paths[:3], sample_rate=22050, frame=2048, hop=512, device=dev)
    for p, y in zip(paths[:3], at22):
        ref = Feeder.load_wav(p, sample_rate=22050, frame=2048, hop=512)
        assert y.shape == ref.shape and np.abs(y - ref).max() <= 2e-5 * 0.99 * 0.8


def _mel_args():
    from multi_speaker_tts_amd import Hyper_Parameters as hp
    return dict(num_freq=hp.Sound.Spectrogram_Dim, frame_shift_ms=hp.Sound.Frame_Shift, frame_length_ms=hp.Sound.Frame_Length,
                num_mels=hp.Sound.Mel_Dim, sample_rate=hp.Sound.Sample_Rate)


def test_mel_end_to_end(dev, tmp_path):
    from multi_speaker_tts_amd import Audio, Feeder, Hyper_Parameters as hp
    paths = _write_test_wavs(tmp_path)
    _assert_trim_is_decided(paths, 16000, 32, 16)
    decoded = [Feeder.decode_wav(p) for p in paths]
    feats, lens = Audio.wav_features([d for _, d in decoded], [r for r, _ in decoded], max_abs_value=hp.Sound.Max_Abs_Mel, device=dev,
                                     return_lengths=True, **_mel_args())
    worst = 0.0
    for p, (mel, spec), n in zip(paths, feats, lens):
        sig = Feeder.load_wav(p)
        ref = Audio.melspectrogram(y=sig, max_abs_value=hp.Sound.Max_Abs_Mel, device=dev, **_mel_args()).T
        assert spec is None and n == sig.shape[0] and mel.shape == ref.shape, (p, n, sig.shape, mel.shape, ref.shape)
        err = np.abs(mel - ref).max()
        worst = max(worst, err)
        print("%s: %d frames, max |mel(device front end) - mel(host front end)| = %.3g" % (os.path.basename(p), mel.shape[0], err))
    print("wav_features: worst %.3g (bound 2e-3)" % worst)
    assert worst <= 2e-3
    short = [np.zeros(40000, np.float32), np.concatenate([np.zeros(3000), 0.5 * np.ones(500), np.zeros(3000)]).astype(np.float32)]
    with pytest.raises(ValueError, match="waveform 1"):                                    # 512 samples survive the trim: <= n_fft / 2
        Audio.wav_features(short, [16000, 16000], max_abs_value=4, device=dev, **_mel_args())
    both = Audio.wav_features([decoded[0][1]], [decoded[0][0]], want_spec=True, max_abs_value=4, device=dev, **_mel_args())
    assert both[0][1].shape == (both[0][0].shape[0], hp.Sound.Spectrogram_Dim)


def _small_tacotron(dev, tmp_path, monkeypatch):
    from multi_speaker_tts_amd import Hyper_Parameters as hp
    from multi_speaker_tts_amd.MSTTS_SV import Tacotron2
    from multi_speaker_tts_amd.params import Dims
    monkeypatch.setattr(hp, "Checkpoint_Path", str(tmp_path / "ckpt"))
    monkeypatch.setattr(hp, "Inference_Path", str(tmp_path / "inf"))
    dims = Dims(emb=32, enc_conv_ch=32, enc_lstm=16, spk=256, prenet=16, dec_lstm=32, post_ch=16, bank_ch=8, proj1_ch=16, birnn=8,
                spk_lstm=256, max_inf=6)
    return dims, Tacotron2(is_Training=False, device=dev, dims=dims, allow_random_init=True)


def test_inference_surface_device_front_end(dev, tmp_path, monkeypatch):
    from oracle import model as OM, train as OT
    monkeypatch.delenv("MSTTS_WAV_FRONT_END", raising=False)
    dims, t = _small_tacotron(dev, tmp_path, monkeypatch)
    paths = _write_test_wavs(tmp_path)[:3]
    _assert_trim_is_decided(paths, 16000, 32, 16)
    texts = ["Please call Stella.", "Who knows?", "His voice is tested now."]
    host = t.feeder.Get_Inference_Pattern(paths, texts, front_end="host")
    device = t.feeder.Get_Inference_Pattern(paths, texts, front_end="device")
    default = t.feeder.Get_Inference_Pattern(paths, texts)
    assert device["Speaker_Embedding_Mel"].shape == host["Speaker_Embedding_Mel"].shape and device["Speaker_Embedding_Mel"].dtype == np.float32
    err = np.abs(device["Speaker_Embedding_Mel"] - host["Speaker_Embedding_Mel"]).max()
    print("Get_Inference_Pattern: max |windows(device) - windows(host)| = %.3g (bound 2e-3)" % err)
    assert err <= 2e-3
    assert np.array_equal(device["Token"], host["Token"]) and np.array_equal(device["Token_Length"], host["Token_Length"])
    for k in host:
        assert np.array_equal(default[k], host[k]), k                                      # the default is the host path, bit for bit
    monkeypatch.setenv("MSTTS_WAV_FRONT_END", "device")
    env = t.feeder.Get_Inference_Pattern(paths, texts)
    assert np.array_equal(env["Speaker_Embedding_Mel"], device["Speaker_Embedding_Mel"])
    monkeypatch.delenv("MSTTS_WAV_FRONT_END")
    od = OM.Dims(**{f: getattr(dims, f) for f in ("emb", "enc_conv_ch", "enc_lstm", "spk", "prenet", "dec_lstm", "post_ch", "bank_ch", "proj1_ch",
                                                 "birnn", "spk_lstm", "max_inf")})
    masks = {k: v.numpy() for k, v in OT.make_masks(od, 3, host["Token"].shape[1], od.max_inf + 1, False, seed=31).items()}
    a = t.Inference(paths, texts, masks=masks, export=False, front_end="host")
    b = t.Inference(paths, texts, masks=masks, export=False, front_end="device")
    assert set(a) == set(b)
    for k in ("Linear", "Mel", "Stop", "Spectrogram"):
        assert b[k].shape[0] == 3 and np.isfinite(b[k]).all(), k


def test_mel_generate_batch_against_mel_generate(dev, tmp_path, monkeypatch):
    from scipy.io import wavfile
    from multi_speaker_tts_amd import Pattern_Generate as PG
    paths = _write_test_wavs(tmp_path)
    p = str(tmp_path / "too_short.wav")                                                    # 0.4 s: rejected by Use_Wav_Length_Range (500 ms)
    wavfile.write(p, 16000, voiced(16000, seconds=6.0)[40000:46400])
    paths.insert(2, p)
    _assert_trim_is_decided(paths, 16000, 2048, 512)
    for subtract in (False, True):
        got = PG.Mel_Generate_Batch(paths, spectral_Subtract=subtract, device=dev)
        worst = 0.0
        for path, mel in zip(paths, got):
            ref = PG.Mel_Generate(path, spectral_Subtract=subtract, device=dev)
            assert (mel is None) == (ref is None), path
            if ref is not None:
                assert mel.dtype == np.float32 and mel.shape == ref.shape, (path, mel.shape, ref.shape)
                worst = max(worst, np.abs(mel - ref).max())
        print("Mel_Generate_Batch, spectral_Subtract %s: Nones %s, worst |mel - Mel_Generate| = %.3g (bound 2e-3)" % (subtract, [m is None for m in got], worst))
        assert got[2] is None and sum(m is None for m in got) == 1 and worst <= 2e-3
    every = PG.Mel_Generate_Batch(paths, range_Ignore=True, device=dev)
    assert all(m is not None for m in every) and every[2].shape == PG.Mel_Generate(p, range_Ignore=True, device=dev).shape


def test_pattern_generate_cli_batched(dev, tmp_path, monkeypatch):
    import pickle
    from scipy.io import wavfile
    from multi_speaker_tts_amd import Hyper_Parameters as hp
    from multi_speaker_tts_amd import Pattern_Generate as PG
    lj = tmp_path / "LJ"
    (lj / "wavs").mkdir(parents=True)
    rows = []
    sentences = ["Please call Stella.", "Who knows much believes the less.", "His voice is tested now.", "Things are always at their best.",
                 "Ask her to bring these things.", "Too short to keep."]
    for i, text in enumerate(sentences):
        rate = (16000, 22050, 48000)[i % 3]
        y = voiced(rate, seconds=0.45 if i == 5 else 1.6 + 0.2 * i, seed=20 + i)
        wavfile.write(str(lj / "wavs" / ("LJ001-%04d.wav" % i)), rate, y)
        rows.append("LJ001-%04d|%s|%s" % (i, text, text))
    (lj / "metadata.csv").write_text("\n".join(rows) + "\n", encoding="utf-8")
    _assert_trim_is_decided([str(lj / "wavs" / ("LJ001-%04d.wav" % i)) for i in range(6)], 16000, 2048, 512)
    out = {}
    for mode, extra in (("plain", []), ("batch", ["-batch", "4"])):
        monkeypatch.setattr(hp.Train, "Pattern_Path", str(tmp_path / ("patterns_" + mode)))
        written = PG.main(["-lj", str(lj)] + extra, device=dev)
        with open(tmp_path / ("patterns_" + mode) / "METADATA.PICKLE", "rb") as f:
            out[mode] = (written, sorted(os.listdir(tmp_path / ("patterns_" + mode))), pickle.load(f))
    (wa, na, ma), (wb, nb, mb) = out["plain"], out["batch"]
    print("Pattern_Generate: file by file wrote %d %s; -batch 4 wrote %d %s" % (wa, na, wb, nb))
    assert wa == wb == 5 and na == nb and "LJ.LJ001-0005.PICKLE" not in na
    assert set(ma) == set(mb) and ma["File_List"] == mb["File_List"]
    assert ma["Mel_Length_Dict"] == mb["Mel_Length_Dict"] and ma["Token_Length_Dict"] == mb["Token_Length_Dict"] and ma["Dataset_Dict"] == mb["Dataset_Dict"]
    for name in na:
        if name == "METADATA.PICKLE":
            continue
        with open(tmp_path / "patterns_plain" / name, "rb") as f:
            a = pickle.load(f)
        with open(tmp_path / "patterns_batch" / name, "rb") as f:
            b = pickle.load(f)
        assert set(a) == set(b) and a["Text"] == b["Text"] and np.array_equal(a["Token"], b["Token"]) and np.abs(a["Mel"] - b["Mel"]).max() <= 2e-3


def test_one_host_read(dev, tmp_path):
    """Between the upload and the feature launch the host reads the device once (the lengths): under torch's sync debug mode
    wav_features(return_tensor=True) emits at most one synchronisation warning.  The switch is proven first on a plain .item()."""
    from multi_speaker_tts_amd import Audio, Hyper_Parameters as hp
    sigs = [voiced(r).astype(np.float32) / 32767.0 for r in (48000, 22050, 16000, 48000)]
    rates = [48000, 22050, 16000, 48000]
    run = lambda: Audio.wav_features(sigs, rates, max_abs_value=hp.Sound.Max_Abs_Mel, device=dev, return_tensor=True, **_mel_args())
    run()                                                                                  # constants, tables and the library are loaded
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
            feats = run()
        syncs = [w for w in seen if "synchroniz" in str(w.message).lower()]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    print("sync debug mode: .item() warned %d time(s); wav_features warned %d time(s): %s" % (len(proof), len(syncs), [str(w.message)[:60] for w in syncs]))
    assert len(proof) >= 1, "torch.cuda.set_sync_debug_mode('warn') does not report a plain .item() in this build: the check cannot be made"
    assert len(syncs) <= 1
    assert all(m.is_cuda and m.shape[1] == hp.Sound.Mel_Dim for m, _ in feats)
