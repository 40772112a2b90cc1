"""The waveform front end by librosa's rules (rule="librosa": resampy's kaiser_best rate conversion, librosa.effects.trim's centred
frames; csrc/wav_front_end.hip), the parts that need no GPU: entry points and defaults, the filter against an
independent restatement, the polyphase table form against a literal transcription of resampy's sequential loop, an analytic signal,
hand-derived trim cases and the metadata key.  Neither resampy nor librosa is installed where this was written: the transcription and
the restatements below are made from the published algorithms, parity with the packages themselves is unpinned.  The helpers here are
also what tests/test_gpu_wav_rule_librosa.py checks the device against."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

from tests.test_cpu_wav_front_end import SOURCE_RATES, TARGET_RATES, envelope_ratios, voiced

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mstts_wav_resample_fir_supported", "mstts_wav_resample_fir", "mstts_wav_trim_centred_ws_floats", "mstts_wav_trim_centred")
ROLLOFF, BETA = 0.9475937167399596, 14.769656459379492
RATIOS = envelope_ratios() + [r for r in [(147, 160)] if r not in envelope_ratios()]     # (147 : 160 is 24 000 -> 22 050 Hz, one of the ten)
SOURCE_RATE = {(147, 160): 48000}                            # ratio -> a source rate that has it (48 000 -> 44 100 Hz for 147 : 160)
for _t in TARGET_RATES:
    for _s in SOURCE_RATES:
        SOURCE_RATE.setdefault((_t // int(np.gcd(_s, _t)), _s // int(np.gcd(_s, _t))), _s)
MARGIN_DB = 0.01
# Seed of the 1 s utterance of the device trim test.  Chosen on the float64 restatement alone (no device involved), on the host
# kaiser_best conversion of voiced(rate, seconds=1.0) for 16 000 / 22 050 / 48 000 Hz -> 16 000 Hz and the frames 32 / 16 and 2048 / 512.
# Nearest deciding frame over the six cases, seeds 0 .. 11: 0.090, 0.692, 0.014, 0.753, 0.011, 0.067, 0.720, 0.363, 0.121, 0.009, 2.077,
# 0.379 dB.  Seed 9 misses the 0.01 dB precondition, seeds 2 and 4 all but miss it; seed 6 (tests/test_cpu_wav_front_end.py's, 0.186 dB
# at 6 s under the scipy resampler) keeps 0.72 dB for this input; seed 10 keeps the most and is used.
TRIM_SEED = 10
TRIM_RATES = (16000, 22050, 48000)
TRIM_FRAMES = ((32, 16), (2048, 512))


def window_restated():
    """resampy's sinc_window(num_zeros=64, precision=9, window=kaiser(beta), rolloff) written out independently of Audio.py."""
    from scipy.signal.windows import kaiser
    n = 512 * 64
    taper = kaiser(2 * n + 1, BETA, sym=True)[n:]
    t = np.arange(n + 1) / 512.0
    arg = np.pi * ROLLOFF * t
    sinc = np.ones(n + 1)
    sinc[1:] = np.sin(arg[1:]) / arg[1:]
    return ROLLOFF * sinc * taper


def sequential(x, up, down):
    """A literal transcription of resampy 0.2.x's resample_f for one channel in float64, the accumulated time register included ->
    (y [int(n ratio)], n_used [same]): the outputs and the integer part of the time register each output was computed at."""
    win = window_restated()
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    sample_ratio = float(up) / down
    if sample_ratio < 1:
        win = win * sample_ratio
        delta = delta * sample_ratio
    num_table = 512
    x = np.asarray(x, np.float64)
    y = np.zeros(int(x.shape[0] * sample_ratio))
    used = np.zeros(y.shape[0], np.int64)
    scale = min(1.0, sample_ratio)
    time_increment = 1.0 / sample_ratio
    index_step = int(scale * num_table)
    time_register = 0.0
    nwin = win.shape[0]
    n_orig = x.shape[0]
    for t in range(y.shape[0]):
        n = int(time_register)
        used[t] = n
        frac = scale * (time_register - n)
        index_frac = frac * num_table
        offset = int(index_frac)
        eta = index_frac - offset
        i_max = min(n + 1, (nwin - offset) // index_step)
        acc = 0.0
        for i in range(i_max):
            acc += (win[offset + i * index_step] + eta * delta[offset + i * index_step]) * x[n - i]
        frac = scale - frac
        index_frac = frac * num_table
        offset = int(index_frac)
        eta = index_frac - offset
        k_max = min(n_orig - n - 1, (nwin - offset) // index_step)
        for k in range(k_max):
            acc += (win[offset + k * index_step] + eta * delta[offset + k * index_step]) * x[n + k + 1]
        y[t] = acc
        time_register += time_increment
    return y, used


def table_form(x, up, down):
    """The formula the device kernel implements, multiplied out in float64 from Audio.kaiser_best_table with plain loops over the outputs'
    rows: y[t] = sum_i table[(t down) % up, i] x[(t down) // up - L + 1 + i], zeros outside the signal and from n_valid on."""
    from multi_speaker_tts_amd import Audio
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    table = Audio.kaiser_best_table(up, down)
    L = table.shape[1] // 2
    n_valid, n_out = Audio.kaiser_best_out_len(n, up, down)
    xp = np.concatenate([np.zeros(L), x, np.zeros(2 * L + 2)])
    y = np.zeros(n_out)
    for t in range(n_valid):
        q = t * down
        n0 = q // up
        y[t] = np.dot(table[q % up], xp[n0 + 1:n0 + 1 + 2 * L])
    return y


def trim_reference_centred(x, top_db=15.0, frame=32, hop=16):
    """librosa.effects.trim restated in float64 with plain index arithmetic -> (start, end, margin): the kept range and the distance in dB
    from -top_db of the nearest DECIDING frame (the first and last kept frame and every frame outside them); margin None when nothing
    is decided (n = 0, or n <= frame // 2 where the whole signal is kept)."""
    x = np.asarray(x, np.float64)
    n, pad = x.shape[0], frame // 2
    if n == 0:
        return 0, 0, None
    if n <= pad:
        return 0, n, None
    nf = 1 + (n + 2 * pad - frame) // hop
    j = (hop * np.arange(nf))[:, None] - pad + np.arange(frame)[None, :]
    j = np.where(j < 0, -j, j)
    j = np.where(j > n - 1, 2 * (n - 1) - j, j)
    mse = (x[j] ** 2).mean(axis=1)
    db = 10.0 * np.log10(np.maximum(1e-10, mse)) - 10.0 * np.log10(max(1e-10, mse.max()))
    keep = np.nonzero(db > -top_db)[0]
    if not keep.size:
        return 0, 0, float(np.abs(db + top_db).min())
    first, last = int(keep[0]), int(keep[-1])
    deciding = np.concatenate([db[:first + 1], db[last:]])
    return first * hop, min(n, (last + 1) * hop), float(np.abs(deciding + top_db).min())


def host_kaiser_best(rate, target, seconds=1.0, seed=TRIM_SEED):
    """The float32 array load_wav(rule="librosa") trims for the test utterance: int16 / 32768 -> kaiser_best to `target`."""
    from multi_speaker_tts_amd import Audio
    x = voiced(rate, seconds=seconds, seed=seed).astype(np.float32) / 32768.0
    if rate != target:
        x = Audio.resample_kaiser_best(x, *Audio.resample_ratio(rate, target)).astype(np.float32)
    return x


TRIM_KATS = {                                                # name -> (x, frame, hop, the hand-derived result)
    # frames centred on 0, 16, ...: [i 16 - 16, i 16 + 16).  Frame 2 = [16, 48) holds 8 ones, frames 3 and 4 hold 20 and 12, frame 5 none:
    # 10 log10(8 / 20) = -4.0 dB and 10 log10(12 / 20) = -2.2 dB are kept -> [2 * 16, 5 * 16).  The uncentred rule gives (16, 64).
    "block": (np.concatenate([np.zeros(40), np.ones(20), np.zeros(40)]), 32, 16, (32, 80)),
    # frame 0 = x[reflect(-16 .. 15)] sees x[1:4] twice (6 ones), frame 1 = [0, 32) once (3 ones: -3.0 dB), frame 2 = [16, 48) none -> [0, 32)
    "reflected start": (np.concatenate([np.zeros(1), np.ones(3), np.zeros(60)]), 32, 16, (0, 32)),
    "all zeros": (np.zeros(100), 32, 16, (0, 100)),          # every frame at 0 dB: frames 0 .. 6 kept, min(100, 7 * 16)
    "empty": (np.zeros(0), 32, 16, (0, 0)),
    "not longer than the padding": (np.ones(10), 32, 16, (0, 10)),
    "hop 1": (np.concatenate([np.zeros(5), np.ones(4), np.zeros(5)]), 4, 1, (4, 11)),   # 15 frames for 14 samples; frames 4 .. 10 hold >= 1 one of at most 4 (-6.0 dB)
}


def test_entry_points_defaults_and_refusals(tmp_path, monkeypatch):
    from scipy.io import wavfile
    from multi_speaker_tts_amd import build, lib, Feeder
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mstts.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mstts_[a-z0-9_]+)\s*\(", text))
    cdll = ctypes.CDLL(build.build())
    for name in ENTRY_POINTS:
        assert name in declared and name in lib.SIGNATURES and hasattr(cdll, name), name
    assert lib.ABI_VERSION == 5 and lib.load().mstts_abi_version() == 5                    # additions only
    assert "wav_front_end.hip" in build.SOURCES                                             # both rule sets live in the one file
    src = open(os.path.join(ROOT, "multi_speaker_tts_amd", "csrc", "wav_front_end.hip")).read()
    assert "hipStreamSynchronize" not in src and "hipDeviceSynchronize" not in src and "hipMemcpy" not in src
    L = lib.load()
    one = ctypes.c_void_p(16)                                                              # dummies, never dereferenced
    def fir(nw=2, up=1, down=3, taps=386, max_out=100, origin=193, tiling=0, table=one):
        return L.mstts_wav_resample_fir(one, one, one, one, nw, max_out, table, up, down, taps, origin, tiling, one, None)
    assert fir(nw=0) == -1 and b"0 waveforms" in L.mstts_last_error()
    assert fir(up=0) == -1 and b"up = 0" in L.mstts_last_error()
    assert fir(down=0) == -1 and fir(taps=0) == -1 and b"taps = 0" in L.mstts_last_error()
    assert fir(up=4097, down=4096, taps=130) == -1 and b"envelope" in L.mstts_last_error()
    assert fir(up=4096, down=4095, taps=1025) == -1 and b"envelope" in L.mstts_last_error()       # up taps > 2^22
    assert fir(up=1, down=512, taps=65538, tiling=2) == -1 and b"tiling" in L.mstts_last_error()  # a row longer than LDS: row-major only
    assert fir(tiling=3) == -1 and fir(max_out=-1) == -1 and fir(origin=-1) == -1 and fir(table=None) == -1
    assert L.mstts_wav_resample_fir_supported(1, 3, 386) == 2 and L.mstts_wav_resample_fir_supported(320, 441, 178) == 2
    assert L.mstts_wav_resample_fir_supported(1, 512, 65538) == 1 and L.mstts_wav_resample_fir_supported(4096, 4095, 130) == 2
    assert L.mstts_wav_resample_fir_supported(0, 1, 4) == 0 and L.mstts_wav_resample_fir_supported(1, 0, 4) == 0 and L.mstts_wav_resample_fir_supported(1, 1, 0) == 0
    def trim(nw=2, frame=32, hop=16, ws=one):
        return L.mstts_wav_trim_centred(one, one, nw, 1000, 600, frame, hop, 15.0, ws, one, one, None)
    assert trim(nw=0) == -1 and trim(frame=0) == -1 and trim(hop=0) == -1 and b"hop = 0" in L.mstts_last_error() and trim(ws=None) == -1
    assert L.mstts_wav_trim_centred_ws_floats(1000, 3) >= 1000 + 3 + 3                     # n + 1 frames per waveform at hop 1, one maximum each
    # the default rule is today's front end, byte for byte
    p = str(tmp_path / "v.wav")
    wavfile.write(p, 48000, voiced(48000, seconds=1.0))
    monkeypatch.delenv("MSTTS_WAV_RULE", raising=False)
    a, b, c = Feeder.load_wav(p), Feeder.load_wav(p, rule="scipy"), Feeder.load_wav(p, rule="librosa")
    assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert c.dtype == np.float32 and not np.array_equal(a, c)
    assert Feeder.wav_rule(None) == "scipy" and Feeder.wav_rule("librosa") == "librosa"
    with pytest.raises(ValueError):
        Feeder.wav_rule("resampy")
    r0, d0 = Feeder.decode_wav(p)
    r1, d1 = Feeder.decode_wav(p, rule="librosa")
    x = voiced(48000, seconds=1.0)
    assert r0 == r1 == 48000 and np.array_equal(d0, x.astype(np.float32) / 32767.0) and np.array_equal(d1, x.astype(np.float32) / 32768.0)
    p32 = str(tmp_path / "v32.wav")
    wavfile.write(p32, 16000, x.astype(np.int32) << 16)
    assert np.array_equal(Feeder.decode_wav(p32, rule="librosa")[1], d1[:x.shape[0]])


def test_filter_equals_an_independent_restatement():
    from multi_speaker_tts_amd import Audio
    W, D = Audio.kaiser_best_window()
    want = window_restated()
    assert W.dtype == np.float64 and W.shape == (32769,) and D.shape == (32769,)
    assert W[0] == ROLLOFF and D[-1] == 0.0 and np.array_equal(D[:-1], np.diff(W))
    err = np.abs(W - want).max()
    print("max |W - restatement| = %.3g" % err)
    assert err <= 1e-15
    for (up, down), taps in (((1, 3), 386), ((320, 441), 178), ((160, 441), 356), ((2, 1), 130), ((441, 320), 130)):
        tab = Audio.kaiser_best_table(up, down)
        scale, step, L = Audio.kaiser_best_step(up, down)
        assert tab.dtype == np.float64 and tab.shape == (up, taps) and taps == 2 * L
        assert step == int(min(1.0, float(up) / down) * 512)                               # truncated: 170 at 1 : 3
        rows = np.abs(tab).sum(axis=1).max()
        print("%d:%d  step %d, taps %d, max row sum %.4f" % (up, down, step, taps, rows))
        assert 2.33 - 0.005 <= rows <= 2.56 + 0.005
    assert Audio.kaiser_best_step(1, 3)[1] == 170
    with pytest.raises(ValueError):
        Audio.kaiser_best_step(1, 1000)


@pytest.mark.parametrize("up,down", RATIOS)
def test_table_form_against_the_sequential_transcription(up, down):
    """The table form at the exact positions t down / up equals the sequential algorithm with its accumulated time register wherever both
    look at the same input sample; where they do not, the register has fallen one ulp short of an integer that the exact position
    reaches (t down = 0 mod up) - never when up is 1 or 2, whose increments are exact in binary."""
    from multi_speaker_tts_amd import Audio
    n = int(0.05 * SOURCE_RATE[(up, down)])
    x = np.random.default_rng(1000 * up + down).normal(size=n)
    seq, used = sequential(x, up, down)
    tab = table_form(x, up, down)
    fast = Audio.resample_kaiser_best(x, up, down)
    n_valid, n_out = Audio.kaiser_best_out_len(n, up, down)
    assert seq.shape[0] == n_valid and tab.shape[0] == fast.shape[0] == n_out
    assert np.abs(fast - tab).max() <= 1e-12 * np.abs(x).max()                              # the by-row product is the plain loop
    t = np.arange(n_valid)
    excluded = used != (t * down) // up
    assert np.all((t[excluded] * down) % up == 0)
    if up in (1, 2):
        assert not excluded.any()
    err = np.abs(seq - tab[:n_valid])[~excluded].max() / np.abs(x).max()
    at = np.abs(seq - tab[:n_valid])[excluded].max() if excluded.any() else 0.0
    print("%d:%d  n %d -> %d: %d outputs excluded (max diff there %.3g, max |x| %.3g), elsewhere max |seq - table| / max |x| = %.3g" % (
        up, down, n, n_valid, int(excluded.sum()), at, np.abs(x).max(), err))
    assert err <= 1e-9


def test_analytic_signal_and_output_lengths():
    """16 000 -> 22 050 Hz of a 1 kHz sine + 0.5: the interior is the analytic signal to 1e-6 (measured 1.2e-7 in float64).  Lengths
    follow resampy + librosa's fix_length in doubles: int(n ratio) computed samples, zeros up to int(ceil(n ratio)).  For n = 96 000 at
    1 : 3 the double product 96000 * (1.0 / 3) rounds to exactly 32000.0, so both are 32 000 there (the product is exact for every
    multiple of 3 up to 300 000); the trailing zero appears where n ratio is no integer, as at n = 96 001."""
    from multi_speaker_tts_amd import Audio
    x = np.sin(2 * np.pi * 1000 * np.arange(16000) / 16000.0) + 0.5
    y = Audio.resample_kaiser_best(x, *Audio.resample_ratio(16000, 22050))
    ref = np.sin(2 * np.pi * 1000 * np.arange(y.shape[0]) / 22050.0) + 0.5
    err = np.abs(y - ref)[400:-400].max()
    print("1 kHz sine + 0.5, 16000 -> 22050: interior max error %.3g" % err)
    assert y.shape[0] == 22050 and err <= 1e-6
    assert Audio.kaiser_best_out_len(96000, 1, 3) == (int(96000 * (1.0 / 3)), int(np.ceil(96000 * (1.0 / 3)))) == (32000, 32000)
    assert Audio.kaiser_best_out_len(96001, 1, 3) == (32000, 32001)
    g = np.random.default_rng(3)
    z = Audio.resample_kaiser_best(g.normal(size=96001), 1, 3)
    assert z.shape == (32001,) and z[-1] == 0.0 and z[-2] != 0.0
    for n, want in ((0, (0, 0)), (1, (0, 1)), (2, (0, 1))):
        assert Audio.kaiser_best_out_len(n, 1, 3) == want
        out = Audio.resample_kaiser_best(np.ones(n), 1, 3)
        assert out.shape == (want[1],) and not out.any()
    assert Audio.kaiser_best_out_len(2, 441, 320) == (2, 3) and Audio.resample_kaiser_best(np.ones(2), 441, 320)[2] == 0.0


@pytest.mark.parametrize("name", list(TRIM_KATS))
def test_trim_kats(name):
    from multi_speaker_tts_amd import Audio
    x, frame, hop, want = TRIM_KATS[name]
    assert Audio.trim_bounds_centred(x, 15.0, frame, hop) == want
    assert trim_reference_centred(x, 15.0, frame, hop)[:2] == want


def test_trim_differs_from_the_default_rule_and_load_wav_follows_it(tmp_path):
    from scipy.io import wavfile
    from tests.test_cpu_wav_front_end import trim_reference
    from multi_speaker_tts_amd import Audio, Feeder
    x = TRIM_KATS["block"][0]
    assert trim_reference(x, 15.0, 32, 16)[:2] == (16, 64)                                 # today's rule on the same block
    p = str(tmp_path / "v.wav")
    wavfile.write(p, 48000, voiced(48000))
    y = host_kaiser_best(48000, 16000, seconds=6.0, seed=6)
    for frame, hop in TRIM_FRAMES:
        s, e, margin = trim_reference_centred(y, 15.0, frame, hop)
        assert Audio.trim_bounds_centred(y, 15.0, frame, hop) == (s, e) and 0 < s < e < y.shape[0]
        got = Feeder.load_wav(p, sample_rate=16000, frame=frame, hop=hop, rule="librosa")
        print("voiced, 48000 -> 16000 by kaiser_best, frame %d hop %d: kept [%d, %d) of %d, margin %.4f dB" % (frame, hop, s, e, y.shape[0], margin))
        assert got.dtype == np.float32 and np.array_equal(got, y[s:e] * 0.99)
        assert (s, e) == {32: (8752, 87232), 2048: (8704, 87552)}[frame]                   # today's rule: [8736, 87216) and [7680, 86528)
        assert (s % hop, e % hop) == (0, 0)


def test_trim_seed_keeps_the_margin():
    """The precondition of the device trim test, on the float64 restatement alone: at TRIM_SEED every deciding frame of every case lies at
    least 0.01 dB from the threshold."""
    worst = None
    for rate in TRIM_RATES:
        x = host_kaiser_best(rate, 16000)
        for frame, hop in TRIM_FRAMES:
            s, e, margin = trim_reference_centred(x, 15.0, frame, hop)
            print("%d -> 16000, frame %d hop %d: [%d, %d) of %d, margin %.4f dB" % (rate, frame, hop, s, e, x.shape[0], margin))
            assert 0 < s < e < x.shape[0]
            worst = margin if worst is None else min(worst, margin)
    assert worst >= MARGIN_DB


def test_pattern_generate_writes_the_rule_only_when_it_is_not_the_default(tmp_path, monkeypatch):
    """`Pattern_Generate -rule librosa` on two tiny wavs records Wav_Rule = "librosa" in METADATA.PICKLE, the default writes no such key,
    and check_metadata refuses a set made under another rule than the one in force.  The mel launch (the only step that needs a GPU) is
    replaced by a stand-in that keeps the frame count."""
    from scipy.io import wavfile
    from multi_speaker_tts_amd import Audio, Feeder, Hyper_Parameters as hp, Pattern_Generate as PG
    monkeypatch.delenv("MSTTS_WAV_RULE", raising=False)
    lj = tmp_path / "LJ"
    (lj / "wavs").mkdir(parents=True)
    rows = []
    for i, text in enumerate(["Please call Stella.", "Who knows?"]):
        wavfile.write(str(lj / "wavs" / ("LJ001-%04d.wav" % i)), 22050, voiced(22050, seconds=2.0, seed=20 + i))
        rows.append("LJ001-%04d|%s|%s" % (i, text, text))
    (lj / "metadata.csv").write_text("\n".join(rows) + "\n", encoding="utf-8")
    lengths = []
    def fake_mel(y, **kw):
        lengths.append((y.shape[0], float(np.abs(y).sum())))
        return np.zeros((hp.Sound.Mel_Dim, 1 + y.shape[0] // 200), np.float32)
    monkeypatch.setattr(Audio, "melspectrogram", fake_mel)
    md = {}
    for mode, extra in (("default", []), ("librosa", ["-rule", "librosa"])):
        monkeypatch.setattr(hp.Train, "Pattern_Path", str(tmp_path / ("patterns_" + mode)))
        assert PG.main(["-lj", str(lj)] + extra, device="cpu") == 2
        with open(tmp_path / ("patterns_" + mode) / "METADATA.PICKLE", "rb") as f:
            md[mode] = pickle.load(f)
    assert "Wav_Rule" not in md["default"] and md["librosa"]["Wav_Rule"] == "librosa"
    assert set(md["librosa"]) - set(md["default"]) == {"Wav_Rule"} and md["default"]["File_List"] == md["librosa"]["File_List"]
    assert len(lengths) == 4 and lengths[:2] != lengths[2:]                                # the two rules gave different waveforms
    Feeder.check_metadata(md["default"])
    Feeder.check_metadata(md["librosa"], rule="librosa")
    with pytest.raises(ValueError, match="rule"):
        Feeder.check_metadata(md["librosa"])
    with pytest.raises(ValueError, match="rule"):
        Feeder.check_metadata(md["default"], rule="librosa")
    monkeypatch.setenv("MSTTS_WAV_RULE", "librosa")
    Feeder.check_metadata(md["librosa"])
