"""The waveform front end on the GPU (mstts_wav_resample / mstts_wav_trim / mstts_wav_gather_scale, Audio.wav_front_end), the parts that
need no GPU: the entry points exist in the header, the library and the binding; the resampler's envelope and the host-side parameter
checks; the host filter helper and its phase layout against scipy in float64; and an fp64 restatement of Feeder.load_wav's trim rule,
which is what tests/test_gpu_wav_front_end.py checks the device trim against, together with the inputs both files use."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mstts_wav_resample_supported", "mstts_wav_resample", "mstts_wav_trim", "mstts_wav_gather_scale")
SOURCE_RATES = (8000, 16000, 22050, 24000, 44100, 48000)
TARGET_RATES = (16000, 22050)
RATIOS = ((320, 441), (1, 3), (147, 320), (160, 441), (2, 1))
MARGIN_DB = 0.01
# Seed of the test utterance.  Chosen on the float64 restatement alone (no device involved): of the seeds 0 .. 11 it keeps the deciding
# frames furthest from the threshold over all sixteen TRIM_CASES (0.19 dB); seeds 0, 4, 5, 7 and 10 miss the 0.01 dB precondition.
SEED = 6


def envelope_ratios():
    """(up, down) in lowest terms of every source -> target pair of the envelope list, identity excluded: ten ratios."""
    out = []
    for t in TARGET_RATES:
        for s in SOURCE_RATES:
            g = int(np.gcd(s, t))
            if s != t and (t // g, s // g) not in out:
                out.append((t // g, s // g))
    return out


def voiced(rate, seconds=6.0, seed=SEED, f0=None):
    """The test utterance: 19 harmonics of a 110 - 150 Hz fundamental with seeded phases, amplitude 1 / k, under the envelope
    clip(3 sin(pi clip((t - 0.3) / (T - 0.6), 0, 1)), 0, 1)^2 (0.3 s of silence at both ends, smooth rise and fall), scaled by 0.2, plus
    1e-3 Gaussian noise, normalised to a peak of 0.8 -> int16 samples."""
    g = np.random.default_rng(seed)
    f0 = f0 if f0 is not None else 110.0 + 40.0 * g.random()
    t = np.arange(int(rate * seconds)) / float(rate)
    y = np.zeros_like(t)
    for k in range(1, 20):
        y += np.sin(2 * np.pi * f0 * k * t + 2 * np.pi * g.random()) / k
    env = np.clip(3 * np.sin(np.pi * np.clip((t - 0.3) / (seconds - 0.6), 0, 1)), 0, 1) ** 2
    y = 0.2 * env * y + 1e-3 * g.normal(size=t.shape[0])
    y = 0.8 * y / np.abs(y).max()
    return np.round(y * 32767).astype(np.int16)


def trim_reference(x, top_db=15.0, frame=32, hop=16):
    """Feeder.load_wav's trim rule restated in float64 -> (start, end, margin): the kept range and the distance in dB from -top_db of the
    nearest DECIDING frame - the first and last kept frame and every frame outside the kept range (None when nothing is decided:
    shorter than a frame)."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    if n < frame:
        return 0, n, None
    nf = 1 + (n - frame) // hop
    idx = np.arange(frame)[None, :] + (hop * np.arange(nf))[:, None]
    rms = np.sqrt((x[idx] ** 2).mean(axis=1))
    db = 20.0 * np.log10(np.maximum(rms, 1e-10) / max(rms.max(), 1e-10))
    keep = np.nonzero(db > -top_db)[0]
    if not keep.size:
        return 0, n, float(np.abs(db + top_db).min())
    first, last = int(keep[0]), int(keep[-1])
    deciding = np.concatenate([db[:first], db[first:first + 1], db[last:last + 1], db[last + 1:]])
    return first * hop, min(n, (last + 1) * hop), float(np.abs(deciding + top_db).min())


def host_resampled(rate, target, seed=SEED):
    """The float32 array load_wav trims for the test utterance at `rate`: int16 -> [-1, 1] -> resample_poly to `target`."""
    from scipy.signal import resample_poly
    x = voiced(rate, seed=seed).astype(np.float32) / 32767.0
    if rate != target:
        g = int(np.gcd(rate, target))
        x = resample_poly(x, target // g, rate // g).astype(np.float32)
    return x


TRIM_CASES = [(rate, target, frame, hop) for rate in (16000, 22050, 44100, 48000) for target in TARGET_RATES
              for frame, hop in ((32, 16), (2048, 512))]


def test_entry_points_in_header_library_and_binding():
    from multi_speaker_tts_amd import build, lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mstts.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mstts_[a-z0-9_]+)\s*\(", text))
    cdll = ctypes.CDLL(build.build())
    for name in ENTRY_POINTS:
        assert name in declared and name in lib.SIGNATURES and hasattr(cdll, name), name
    assert lib.ABI_VERSION == 5 and lib.load().mstts_abi_version() == 5                    # additions only
    assert "wav_front_end.hip" in build.SOURCES


def test_no_synchronisation_in_the_kernel_file():
    text = open(os.path.join(ROOT, "multi_speaker_tts_amd", "csrc", "wav_front_end.hip")).read()
    assert "hipStreamSynchronize" not in text and "hipDeviceSynchronize" not in text and "hipMemcpy" not in text


def test_envelope_holds_every_listed_rate_pair():
    from multi_speaker_tts_amd import Audio, lib
    L = lib.load()
    ratios = envelope_ratios()
    assert len(ratios) == 10 and set(RATIOS) <= set(ratios)
    for up, down in ratios:
        assert L.mstts_wav_resample_supported(up, down) == 1, (up, down)
        assert Audio.resample_supported(up, down)
        assert L.mstts_wav_resample_taps(up, down) == Audio.resample_taps(up, down) == Audio.resample_phase_table(up, down).shape[1]
    assert L.mstts_wav_resample_supported(0, 1) == 0 and L.mstts_wav_resample_supported(1, 0) == 0 and L.mstts_wav_resample_supported(-2, 3) == 0
    assert L.mstts_wav_resample_supported(1000, 1001) == 0                                 # a 20 000-tap table does not fit in LDS
    assert not Audio.resample_supported(1000, 1001)
    for s in SOURCE_RATES:
        for t in TARGET_RATES:
            assert Audio.resample_ratio(s, t) == (t // np.gcd(s, t), s // np.gcd(s, t))


def test_bad_parameters_are_refused_before_any_launch():
    """up = 0, down = 0, nw = 0 (and frame / hop = 0 of the trim, stft_hop = 0 of the gather) return -1 with the error text set; the
    pointers are dummies that are never dereferenced, so this runs without a GPU."""
    from multi_speaker_tts_amd import lib
    L = lib.load()
    one = ctypes.c_void_p(16)
    def resample(nw=2, up=1, down=3, max_out=100):
        return L.mstts_wav_resample(one, one, one, nw, max_out, one, up, down, one, None)
    assert resample(up=0) == -1 and b"up = 0" in L.mstts_last_error()
    assert resample(down=0) == -1 and b"down = 0" in L.mstts_last_error()
    assert resample(nw=0) == -1 and b"0 waveforms" in L.mstts_last_error()
    assert resample(up=1000, down=1001) == -1 and b"envelope" in L.mstts_last_error()
    assert resample(max_out=-1) == -1
    def trim(nw=2, frame=32, hop=16):
        return L.mstts_wav_trim(one, one, nw, 1000, 600, frame, hop, 15.0, one, one, one, None)
    assert trim(nw=0) == -1 and trim(frame=0) == -1 and trim(hop=0) == -1 and b"hop = 0" in L.mstts_last_error()
    def gather(nw=2, stft_hop=200, max_len=10):
        return L.mstts_wav_gather_scale(one, one, one, one, nw, max_len, 0.99, 0, stft_hop, one, one, one, None)
    assert gather(nw=0) == -1 and gather(stft_hop=0) == -1 and gather(max_len=-5) == -1


@pytest.mark.parametrize("up,down", RATIOS)
def test_filter_helper_and_phase_layout_equal_scipy(up, down):
    """The host helper is up * firwin(2 half + 1, 1 / max(up, down), kaiser 5.0) in float64, and its phase layout, multiplied out by
    the formula the kernel implements, is resample_poly."""
    from scipy.signal import firwin, resample_poly
    from multi_speaker_tts_amd import Audio
    half = 10 * max(up, down)
    h = Audio.resample_filter(up, down)
    want = up * firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0))
    assert h.dtype == np.float64 and h.shape == want.shape and np.abs(h - want).max() <= 1e-12
    tab = Audio.resample_phase_table(up, down)
    T = tab.shape[1]
    assert tab.dtype == np.float64 and tab.shape[0] == up and T % 2 == 1 and T == Audio.resample_taps(up, down)
    assert np.isclose(np.sort(np.abs(tab).ravel())[::-1][:h.shape[0]].sum(), np.abs(h).sum(), rtol=0, atol=1e-9)     # every tap once, zeros elsewhere
    x = np.random.default_rng(up * 1000 + down).normal(size=1500)
    ref = resample_poly(x, up, down)
    n_out = Audio.resample_out_len(x.shape[0], up, down)
    assert n_out == ref.shape[0]
    pad = T + 8
    xp = np.concatenate([np.zeros(pad), x, np.zeros(pad + (half + n_out * down) // up)])
    m = np.arange(n_out)
    q = half + m * down
    rows = tab[q % up]                                                                     # [n_out, T]
    cols = (q // up - (T - 1))[:, None] + np.arange(T)[None, :] + pad
    y = (rows * xp[cols]).sum(axis=1)
    err = np.abs(y - ref).max()
    print("up/down %d/%d: taps %d, max |phase layout - resample_poly| = %.3g, max row sum |h| = %.4f" % (up, down, T, err, np.abs(tab).sum(1).max()))
    assert err <= 1e-12
    assert T <= 61 and np.abs(tab).sum(axis=1).max() <= 2.2415                             # what the GPU test's error bound is derived from


@pytest.mark.parametrize("up,down", RATIOS)
def test_output_length_equals_scipy(up, down):
    from scipy.signal import resample_poly
    from multi_speaker_tts_amd import Audio
    for n in range(1, 2001):
        assert Audio.resample_out_len(n, up, down) == resample_poly(np.zeros(n), up, down).shape[0], n


@pytest.mark.parametrize("rate,target,frame,hop", TRIM_CASES)
def test_trim_restatement_agrees_with_load_wav(rate, target, frame, hop, tmp_path):
    """The fp64 restatement cuts where load_wav cuts, on the inputs the GPU test uses, and those inputs keep every deciding frame at least
    0.01 dB from the threshold (the precondition of the GPU trim test)."""
    from scipy.io import wavfile
    from multi_speaker_tts_amd import Feeder
    p = str(tmp_path / "v.wav")
    wavfile.write(p, rate, voiced(rate))
    got = Feeder.load_wav(p, sample_rate=target, frame=frame, hop=hop)
    x = host_resampled(rate, target)
    start, end, margin = trim_reference(x, 15.0, frame, hop)
    print("%d -> %d, frame %d hop %d: kept [%d, %d) of %d, nearest deciding frame %.4f dB from the threshold" % (rate, target, frame, hop, start, end, x.shape[0], margin))
    assert margin >= MARGIN_DB
    assert 0 < start < end < x.shape[0]
    assert got.shape[0] == end - start and np.array_equal(got, x[start:end] * 0.99)


def test_trim_restatement_edge_cases():
    g = np.random.default_rng(5)
    short = g.normal(size=20)
    assert trim_reference(short, 15.0, 32, 16) == (0, 20, None)
    assert trim_reference(np.zeros(500), 15.0, 32, 16)[:2] == (0, 480)                     # every frame is at 0 dB: all 30 kept, [0, 30 hop)
    loud_start = np.concatenate([0.5 * g.normal(size=32), 1e-4 * g.normal(size=1000)])
    assert trim_reference(loud_start, 15.0, 32, 16)[:2] == (0, 32)                          # frames 0 and 1 hold loud samples: [0, 2 hop)
    loud_end = np.concatenate([1e-4 * g.normal(size=1003), 0.5 * g.normal(size=32)])       # 1035 samples: len - frame = 1003 is no multiple of 16
    s, e, _ = trim_reference(loud_end, 15.0, 32, 16)
    assert e == min(1035, ((1035 - 32) // 16 + 1) * 16) and s >= 976


def test_decode_wav_is_load_wav_without_the_signal_processing(tmp_path):
    """Feeder.decode_wav (what load_wav_batch uploads) followed by load_wav's host arithmetic is load_wav: int16, uint8, stereo."""
    from scipy.io import wavfile
    from scipy.signal import resample_poly
    from multi_speaker_tts_amd import Feeder
    x = voiced(22050, seconds=1.5, seed=2)
    cases = {"i16": x, "u8": ((x.astype(np.int32) >> 8) + 128).astype(np.uint8), "stereo": np.stack([x, x // 2], axis=1)}
    for name, data in cases.items():
        p = str(tmp_path / (name + ".wav"))
        wavfile.write(p, 22050, data)
        rate, sig = Feeder.decode_wav(p)
        assert rate == 22050 and sig.dtype == np.float32 and sig.ndim == 1
        y = resample_poly(sig, 320, 441).astype(np.float32)
        s, e, _ = trim_reference(y)
        assert np.array_equal(Feeder.load_wav(p), y[s:e] * 0.99), name
    assert Feeder.wav_front_end_mode(None) == os.environ.get("MSTTS_WAV_FRONT_END", "host")
    assert Feeder.wav_front_end_mode("device") == "device"
    with pytest.raises(ValueError):
        Feeder.wav_front_end_mode("gpu")
