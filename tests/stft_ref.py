"""fp64 statements, fp32 CPU restatements and case tables of the STFT kernel family (csrc/fft_stages.h, csrc/stft_frame.h, csrc/stft_parts.h:
stft_fft_kernel, stft_bank_batch_kernel, wg_crop_batch_kernel, griffin_lim_kernel, wg_denoise_frames_kernel).  Plain NumPy / torch on the CPU, no
GPU: tests/test_cpu_stft_ref.py pins it against Audio's host functions and torch.stft / torch.istft; tests/test_gpu_stft_ref.py uses it as the
checker.

Everything is stated in SAMPLES, a transform being the triple (n_fft, hop, win); `ms_args` gives the (num_freq, frame_shift_ms, frame_length_ms,
sample_rate) of the wrappers that take milliseconds, at sample_rate = 1000.  Spectra are frame-major, [frames, n_fft // 2 + 1], the layout the
kernels write.  Every function takes dtype = np.float64 (the reference: np.fft) or np.float32 (the restatement: torch.fft on float32 frames,
complex64 spectra, float32 overlap-add in frame order, float32 filters) - one text for both, so that the restatement's error against the
reference is the error of the number format in these operations and of nothing else."""
import contextlib
import functools

import numpy as np
import torch

from oracle import rng as ORNG

# ---- case tables -------------------------------------------------------------------------------------------------------------------------------
SETS = {                                   # (n_fft, hop, win): what it enters
    "odd_off": (512, 128, 510),            # off = 1 (odd); win no multiple of hop; N2 = 256 (the stages return bufa)
    "off161": (1024, 300, 702),            # off = 161; win / hop = 2.34; N2 = 512 (bufb)
    "odd_win": (4096, 600, 1801),          # odd win; off = 1147; N2 = 2048 (bufa); win just above 3 hop
    "full4096": (4096, 1024, 4096),        # the largest transform at full window
    "sparse": (512, 200, 300),             # hop <= win < 2 hop: Griffin-Lim and forward only, the denoiser refuses it
    "tiny": (512, 2, 8),                   # Griffin-Lim: 2, 3, 40 frames = 2, 4, 78 samples under a 256-sample pad (reflection period 2)
    "win_hop": (512, 256, 256),            # win == hop: stft_ola's den > tiny fallback; Griffin-Lim at zero iterations only
    "anchor": (2048, 200, 800),            # the reference's own
}
FORWARD_ONLY = {"gaps": (512, 300, 200)}   # hop > win: no round trip exists, the forward transform does
GL_ONLY = ("tiny", "win_hop")
RAW_SETS = tuple(k for k in SETS if k not in GL_ONLY) + ("gaps",)
DENOISE_SETS = ("odd_off", "off161", "odd_win", "full4096", "anchor")          # 2 hop <= win <= 4 hop of the issue's table
# (512, 2, 8) satisfies 2 hop <= win <= 4 hop as well, so mstts_wg_denoise_supported ADMITS it (tests/test_cpu_stft_ref.py asserts what the
# predicate says); the denoiser tests therefore run it too, on top of the sets above.
DENOISE_EXTRA = ("tiny",)
GL_SETS = tuple(k for k in SETS if k != "win_hop")
GL_FRAMES = (2, 3, 40)
SEEDED_SETS = ("odd_off", "odd_win")
SEEDED_FRAMES = (2, 5, 9)
SEEDS = (0, (1 << 32) + 5, (1 << 64) - 1)  # the middle one: the high key word is live
MEL_COUNTS = (1, 84, 85, 86, 128, 255)     # one pass of 85 filters, its edge on both sides, two passes, three passes
MEL_LENGTHS = (0, 1, 2, 3, 4, 7, None)     # filter range lengths, None = all n_fft // 2 + 1 bins
PREEMPH = 0.97
RULER = 5.4e-7                             # tests/test_gpu_griffin_lim.py's one-iteration figure for the stft / istft pair, of the peak
MARGIN = 4.0                               # device bound = MARGIN x the largest fp32 restatement figure of the test's table
CEIL_RAW, CEIL_TRIP, CEIL_MEL = 1e-5, 10 * RULER, 1e-6


def triple(name):
    return SETS[name] if name in SETS else FORWARD_ONLY[name]


def ms_args(n_fft, hop, win):
    """The wrappers' (num_freq, frame_shift_ms, frame_length_ms, sample_rate) of a transform in samples, at 1000 samples a second."""
    return n_fft // 2 + 1, hop, win, 1000


def lengths(n_fft, hop, win=None):
    """Waveform lengths per set: the shortest admitted, one that is no multiple of hop (5 hop + 19, raised by n_fft // 2 where it would not be
    admitted) and a multiple of hop (six frames' worth, or two hops past n_fft // 2): ten frames at the most at n_fft = 4096."""
    mid = 5 * hop + 19
    if mid <= n_fft // 2:
        mid += n_fft // 2
    if mid % hop == 0:
        mid += 1
    return n_fft // 2 + 1, mid, hop * max(6, n_fft // 2 // hop + 2)


# ---- the operations, dtype = float64 (reference) or float32 (restatement) --------------------------------------------------------------------------
def hann(win, dtype=np.float64):
    """scipy.signal.get_window('hann', win, fftbins=True), built in float64 and rounded (the device table is built the same way)."""
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win) / win)).astype(dtype)


def padded_window(n_fft, win, dtype=np.float64):
    w = np.zeros(n_fft, dtype)
    off = (n_fft - win) // 2
    w[off:off + win] = hann(win, dtype)
    return w


_F32_FFT = ["torch"]                      # whose float32 transform the restatement uses: "torch" (the ruler) or "numpy" (see second_fft)


@contextlib.contextmanager
def second_fft():
    """Inside it the float32 restatement takes NumPy's own float32 transform (pocketfft) instead of torch's: a second factorisation and
    summation order on the CPU.  Not a ruler - a screen: a Griffin-Lim case on which two float32 transforms already part company (a bin near zero
    whose phase flips) cannot judge a third one, the device's, and which of them parts depends on the machine's FFT library."""
    _F32_FFT.append("numpy")
    try:
        yield
    finally:
        _F32_FFT.pop()


def _rfft(frames, dtype):
    if dtype == np.float64:
        return np.fft.rfft(np.asarray(frames, np.float64), axis=1)
    if _F32_FFT[-1] == "numpy":
        out = np.fft.rfft(np.ascontiguousarray(frames, np.float32), axis=1)
    else:
        out = torch.fft.rfft(torch.from_numpy(np.ascontiguousarray(frames, np.float32)), dim=1).numpy()
    assert out.dtype == np.complex64
    return out


def _irfft(D, n_fft, dtype):
    if dtype == np.float64:
        return np.fft.irfft(np.asarray(D, np.complex128), n=n_fft, axis=1)
    if _F32_FFT[-1] == "numpy":
        out = np.fft.irfft(np.ascontiguousarray(D, np.complex64), n=n_fft, axis=1)
    else:
        out = torch.fft.irfft(torch.from_numpy(np.ascontiguousarray(D, np.complex64)), n=n_fft, dim=1).numpy()
    assert out.dtype == np.float32
    return out


def preemphasis(x, coef=PREEMPH, dtype=np.float64):
    """lfilter([1, -coef], [1], x): y[j] = x[j] - coef x[j - 1], x[-1] = 0."""
    x = np.asarray(x, dtype)
    y = x.copy()
    y[1:] -= dtype(coef) * x[:-1]
    return y


def deemphasis(x, coef=PREEMPH, dtype=np.float64):
    """lfilter([1], [1, -coef], x): y[j] = x[j] + coef y[j - 1], in `dtype` sample by sample."""
    from scipy import signal
    y = signal.lfilter(np.asarray([1], dtype), np.asarray([1, -coef], dtype), np.asarray(x, dtype))
    assert y.dtype == dtype
    return y


def stft(x, n_fft, hop, win, dtype=np.float64):
    """librosa.stft(center=True, pad_mode='reflect', periodic Hann centred in the frame) -> [1 + len(x) // hop, n_fft // 2 + 1]."""
    xp = np.pad(np.asarray(x, dtype), n_fft // 2, mode="reflect")
    T = 1 + (xp.shape[0] - n_fft) // hop
    idx = np.arange(n_fft)[None, :] + hop * np.arange(T)[:, None]
    fr = xp[idx] * padded_window(n_fft, win, dtype)[None, :]
    assert fr.dtype == dtype
    return _rfft(fr, dtype)


def raw_magnitudes(x, n_fft, hop, win, coef=PREEMPH, dtype=np.float64):
    """|rfft(window * reflect_pad(preemph(x)))| per frame: what stft_frame_body stores under flags & 2."""
    return np.abs(stft(preemphasis(x, coef, dtype), n_fft, hop, win, dtype))


def window_square_sum(T, n_fft, hop, win, dtype=np.float64):
    w2 = padded_window(n_fft, win, dtype) ** 2
    wss = np.zeros(n_fft + hop * (T - 1), dtype)
    for t in range(T):
        wss[t * hop:t * hop + n_fft] += w2
    return wss


def istft(D, n_fft, hop, win, length=None, dtype=np.float64):
    """librosa.istft / torch.istft: windowed overlap-add of the inverse transforms in frame order, divided by the window-square sum where that
    exceeds float32 tiny; n_fft // 2 samples dropped in front, hop (T - 1) kept (length = None, Audio._istft) or exactly `length`
    (Audio._istft_samples)."""
    T = D.shape[0]
    fr = _irfft(D, n_fft, dtype) * padded_window(n_fft, win, dtype)[None, :]
    n = n_fft + hop * (T - 1)
    y = np.zeros(n, dtype)
    for t in range(T):
        y[t * hop:t * hop + n_fft] += fr[t]
    wss = window_square_sum(T, n_fft, hop, win, dtype)
    nz = wss > np.finfo(np.float32).tiny
    y[nz] /= wss[nz]
    assert y.dtype == dtype
    if length is None:
        return y[n_fft // 2:n - n_fft // 2]
    assert length + n_fft // 2 <= n
    return y[n_fft // 2:n_fft // 2 + length]


def denoise(x, bias, strength, n_fft, hop, win, dtype=np.float64):
    """Audio.spectral_denoise: max(|X| - strength bias, 0) X / |X| (0 where X = 0), back to len(x) samples."""
    X = stft(x, n_fft, hop, win, dtype)
    mag = np.abs(X)
    gain = np.where(mag > 0, np.maximum(mag - dtype(strength) * np.asarray(bias, dtype)[None, :], 0) / np.where(mag > 0, mag, 1), 0).astype(dtype)
    return istft(X * gain, n_fft, hop, win, len(x), dtype)


def amplitudes(spec, power=1.5, ref_db=20.0):
    """(10 ^ ((clip(s, 0, 1) 100 - 100 + ref_db) / 20)) ^ power in float64 (the prepare launch computes it in float64 too and rounds once)."""
    return np.power(10.0, (np.clip(np.asarray(spec, np.float64), 0, 1) * 100 - 100 + ref_db) * 0.05) ** power


def griffin_lim(spec, u, iters, n_fft, hop, win, power=1.5, ref_db=20.0, dtype=np.float64, deemph=True):
    """Audio.inv_spectrogram on a [frames, bins] spectrogram with the initial-phase uniforms u [frames, bins]: A e^{2 pi i u}, istft, then `iters`
    rounds of stft -> X / |X| ((1, 0) at 0) -> istft, then inv_preemphasis."""
    ctype = np.complex128 if dtype == np.float64 else np.complex64
    A = amplitudes(spec, power, ref_db).astype(dtype)
    ang = (2 * np.pi * np.asarray(u, np.float64))
    Y = (A * np.cos(ang).astype(dtype)) + 1j * (A * np.sin(ang).astype(dtype))
    y = istft(Y.astype(ctype), n_fft, hop, win, None, dtype)
    for _ in range(iters):
        X = stft(y, n_fft, hop, win, dtype)
        m = np.abs(X)
        P = np.where(m > 0, X / np.where(m > 0, m, 1), 1).astype(ctype)
        y = istft((A * P).astype(ctype), n_fft, hop, win, None, dtype)
    return deemphasis(y, PREEMPH, dtype) if deemph else y


def normalised(M, ref_db=20.0):
    """Audio._normalize(amp_to_db(M) - ref_db): [0, 1] float32."""
    return np.clip((20 * np.log10(np.maximum(1e-5, M)) - ref_db + 100) / 100, 0, 1).astype(np.float32)


# ---- signals ---------------------------------------------------------------------------------------------------------------------------------------
def tone_plus_noise(n, seed):
    """tests/test_gpu_wg_denoise.py's signal: a tone of amplitude 0.3 (frequency by the seed) in white noise of deviation 0.05 - every bin carries
    signal.  float32."""
    g = np.random.default_rng(seed)
    f = 0.01 + 0.02 * (seed % 7)
    return (0.3 * np.sin(2 * np.pi * f * np.arange(n) + seed) + 0.05 * g.normal(size=n)).astype(np.float32)


def impulse(n_fft, hop):
    """(x, p): a unit impulse at p, a multiple of hop, more than n_fft // 2 samples from both ends (no reflection meets it).  Without
    pre-emphasis frame t sees it at frame position n_fft // 2 + p - t hop: its magnitudes are flat, the window's value there."""
    p = hop * (n_fft // 2 // hop + 1)
    x = np.zeros(p + n_fft // 2 + 2, np.float32)
    x[p] = 1.0
    return x, p


def impulse_answer(n_fft, hop, win, n, p):
    """The known answer of `impulse`: [frames] the flat magnitude of each frame."""
    w = padded_window(n_fft, win)
    pos = n_fft // 2 + p - hop * np.arange(1 + n // hop)
    return np.where((pos >= 0) & (pos < n_fft), w[np.clip(pos, 0, n_fft - 1)], 0.0)


def speech_like(n, seed=0):
    """tests/test_gpu_griffin_lim.py's signal, in samples: its 140 Hz fundamental at 16 kHz is 8.75 Hz at the 1000 samples a second of `ms_args`,
    0.00875 cycles a sample either way; 24 decaying harmonics, a slow vibrato and tremolo, a little noise, quiet ends."""
    g = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    f0 = 140.0 * (1 + 0.05 * np.sin(2 * np.pi * 0.7 * t))
    ph = 2 * np.pi * np.cumsum(f0) / 16000.0
    y = sum(np.sin(h * ph + 0.3 * h) / h ** 1.2 for h in range(1, 25))
    y = y * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t)) + 0.01 * g.normal(size=n)
    fade = np.minimum(1.0, np.minimum(np.arange(n), np.arange(n)[::-1]) / (n / 8.0)) ** 2
    return 0.05 * y * (0.002 + fade)


# ---- shared, read-only case data (computed once per process) --------------------------------------------------------------------------------------
def _ro(a):
    a.setflags(write=False)
    return a


def frame_peak_err(got, ref):
    """The raw-magnitude measure, per frame: max_k |got - ref| / max_k ref; a frame whose reference is all zero must be all zero (error 0, else inf)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    peak, d = ref.max(axis=1), np.abs(got - ref).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(peak > 0, d / np.where(peak > 0, peak, 1), np.where(d == 0, 0.0, np.inf))


@functools.lru_cache(maxsize=None)
def raw_case(name):
    """Per set: three tone-plus-noise waveforms (the three lengths) and the impulse, their fp64 raw magnitudes, and the fp32 restatement's
    frame-peak errors (the largest per waveform)."""
    n_fft, hop, win = triple(name)
    k = list(RAW_SETS).index(name)
    wavs = [tone_plus_noise(n, 31 * k + i) for i, n in enumerate(lengths(n_fft, hop))]
    ref = [_ro(raw_magnitudes(w, n_fft, hop, win)) for w in wavs]
    e32 = [float(frame_peak_err(raw_magnitudes(w, n_fft, hop, win, dtype=np.float32), r).max()) for w, r in zip(wavs, ref)]
    x, p = impulse(n_fft, hop)
    iref = _ro(raw_magnitudes(x, n_fft, hop, win, coef=0.0))
    ie32 = float(frame_peak_err(raw_magnitudes(x, n_fft, hop, win, coef=0.0, dtype=np.float32), iref).max())
    return dict(wavs=[_ro(w) for w in wavs], ref=ref, e32=e32, imp=_ro(x), imp_p=p, imp_ref=iref, imp_e32=ie32)


def raw_table():
    """The largest restatement figure over every set and signal of the raw-magnitude test."""
    return max(max(raw_case(k)["e32"] + [raw_case(k)["imp_e32"]]) for k in RAW_SETS)


@functools.lru_cache(maxsize=None)
def denoise_case(name):
    """Per set: three waveforms (the three lengths), the bias = the per-bin median of their own |X| over all their frames (fp64, rounded to
    float32), the share of bins the fp64 side clamps at strength 1, the fp64 results at strengths 0.1 and 1 and the restatement's errors
    (max |y - want| / max |x|) at strengths 0, 0.1 and 1 - at 0 against the INPUT, the identity."""
    n_fft, hop, win = triple(name)
    k = list(SETS).index(name)
    wavs = [_ro(tone_plus_noise(n, 17 * k + i + 3)) for i, n in enumerate(lengths(n_fft, hop))]
    mags = np.concatenate([np.abs(stft(w, n_fft, hop, win)) for w in wavs], axis=0)
    bias = _ro(np.median(mags, axis=0).astype(np.float32))
    clamped = float(np.mean(mags < bias.astype(np.float64)[None, :]))
    want = {s: [_ro(denoise(w, bias, s, n_fft, hop, win)) for w in wavs] for s in (0.1, 1.0)}
    e32 = {}
    for s in (0.0, 0.1, 1.0):
        refs = [w.astype(np.float64) for w in wavs] if s == 0.0 else want[s]
        e32[s] = max(float(np.abs(denoise(w, bias, s, n_fft, hop, win, np.float32) - r).max() / np.abs(w).max()) for w, r in zip(wavs, refs))
    return dict(wavs=wavs, bias=bias, clamped=clamped, want=want, e32=e32)


def denoise_table(strengths):
    return max(denoise_case(k)["e32"][s] for k in DENOISE_SETS + DENOISE_EXTRA for s in strengths)


# Griffin-Lim cases: (set, frames) -> the seed of the speech-like signal.  A case is usable only if it is not fragile on the CPU alone: the fp32
# restatement must agree with the fp64 host within 10 x RULER of the peak at 3 iterations (phase recovery is discontinuous where a bin is near
# zero).  Which float32 transform trips over such a bin depends on the transform: with seed 0 at (2048, 200, 800), 40 frames, torch's here measured
# 6.6e-7, NumPy's 2.5e-6, torch's on the MI355X host 3.5e-6 and the device 4.1e-6 - all inside the condition, none telling anything about a
# kernel.  So the seeds are the first of 0, 1, ... for which BOTH float32 transforms (`second_fft`) stay below 8e-7 at 0, 1 and 3 iterations,
# a stricter choice than the condition asks.  GL_FIGURES: (set, frames) -> (seed, torch's figure at 1 iteration, at 3, NumPy's at 1, at 3) as
# measured when the seeds were chosen (tests/test_cpu_stft_ref.py prints the figures of the day and asserts the condition for both);
# GL_DROPPED would list the cases no seed satisfies, with the reason - one in eight at the most; none had to be.  Rejected: seed 0 at
# (4096, 600, 1801) two frames (torch 2.9e-6 at 3 iterations) and at (2048, 200, 800) 40 frames.  Seeds that FAIL the condition itself exist and
# are what it is for: (1024, 300, 702) two frames seed 1: 1.96e-5; (2048, 200, 800) three frames seed 1: 1.29e-4 at one iteration;
# (512, 2, 8) two frames seed 2: 1.58e-3 at one iteration.
GL_FIGURES = {
    ("odd_off", 2): (0, 3.18e-07, 4.53e-07, 4.56e-07, 4.54e-07), ("odd_off", 3): (0, 4.02e-07, 4.54e-07, 3.56e-07, 3.82e-07), ("odd_off", 40): (0, 4.06e-07, 5.08e-07, 4.12e-07, 4.07e-07),
    ("off161", 2): (0, 4.77e-07, 5.11e-07, 4.71e-07, 3.37e-07), ("off161", 3): (0, 5.99e-07, 4.32e-07, 3.10e-07, 3.45e-07), ("off161", 40): (0, 3.60e-07, 4.32e-07, 3.60e-07, 4.01e-07),
    ("odd_win", 2): (1, 5.86e-07, 5.09e-07, 3.34e-07, 5.75e-07), ("odd_win", 3): (0, 4.60e-07, 4.52e-07, 4.79e-07, 3.87e-07), ("odd_win", 40): (0, 4.96e-07, 6.75e-07, 5.76e-07, 5.62e-07),
    ("full4096", 2): (0, 4.81e-07, 5.23e-07, 4.69e-07, 5.04e-07), ("full4096", 3): (0, 6.45e-07, 6.02e-07, 6.51e-07, 5.87e-07), ("full4096", 40): (0, 4.73e-07, 5.16e-07, 5.06e-07, 6.20e-07),
    ("sparse", 2): (0, 5.44e-07, 4.95e-07, 5.77e-07, 3.69e-07), ("sparse", 3): (0, 3.81e-07, 5.42e-07, 4.45e-07, 5.88e-07), ("sparse", 40): (0, 5.69e-07, 5.52e-07, 6.27e-07, 5.06e-07),
    ("tiny", 2): (0, 8.00e-08, 8.00e-08, 8.00e-08, 8.00e-08), ("tiny", 3): (0, 2.02e-07, 1.02e-07, 7.73e-08, 1.22e-07), ("tiny", 40): (0, 3.10e-07, 5.26e-07, 3.10e-07, 5.26e-07),
    ("anchor", 2): (0, 3.39e-07, 4.55e-07, 3.54e-07, 5.63e-07), ("anchor", 3): (0, 3.58e-07, 4.86e-07, 3.71e-07, 3.91e-07), ("anchor", 40): (1, 4.99e-07, 4.61e-07, 5.14e-07, 5.25e-07),
}
GL_SEEDS = {k: v[0] for k, v in GL_FIGURES.items()}
GL_DROPPED = {}


def gl_cases():
    return [(k, t) for k in GL_SETS for t in GL_FRAMES if (k, t) not in GL_DROPPED]


def peak_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / np.abs(want).max())


def uniforms(T, nb, seed):
    """Initial-phase uniforms [T, nb]: drawn in float64, rounded to float32 (what the device reads), handed to every side as the rounded values."""
    return _ro(np.random.RandomState(seed).rand(nb, T).astype(np.float32).astype(np.float64).T.copy())


@functools.lru_cache(maxsize=None)
def gl_case(name, T, seed=None):
    """A Griffin-Lim case: the normalised spectrogram [T, bins] (float32, by the host stft of the pre-emphasised speech-like signal of hop (T - 1)
    samples), the uniforms, the fp64 results at 0, 1 and 3 iterations and the restatement's peak-relative errors."""
    n_fft, hop, win = triple(name)
    seed = GL_SEEDS.get((name, T), 0) if seed is None else seed
    y = speech_like(hop * (T - 1), seed)
    spec = _ro(normalised(raw_magnitudes(y, n_fft, hop, win)))
    assert spec.shape == (T, n_fft // 2 + 1)
    u = uniforms(T, n_fft // 2 + 1, 100 + seed)
    want = {it: _ro(griffin_lim(spec, u, it, n_fft, hop, win)) for it in (0, 1, 3)}
    e32 = {it: peak_err(griffin_lim(spec, u, it, n_fft, hop, win, dtype=np.float32), want[it]) for it in (0, 1, 3)}
    with second_fft():
        screen = {it: peak_err(griffin_lim(spec, u, it, n_fft, hop, win, dtype=np.float32), want[it]) for it in (0, 1, 3)}
    return dict(spec=spec, u=u, want=want, e32=e32, screen=screen, seed=seed)


def gl_table(iters):
    return max(gl_case(k, t)["e32"][iters] for k, t in gl_cases())


def weighted_err(got, want, n_fft, hop, win, T):
    """The measure where win == hop (the window-square sum reaches 0 at each frame's first sample and istft's quotient is as large as 1 / window
    beside it): both sides back through lfilter([1, -0.97], [1]) in float64, the difference times sqrt(wss[j]) - the host's own window-square sum
    at that sample - over the peak of the host signal weighted the same way."""
    wss = window_square_sum(T, n_fft, hop, win)[n_fft // 2:n_fft // 2 + hop * (T - 1)]
    a, b = preemphasis(np.asarray(got, np.float64)), preemphasis(np.asarray(want, np.float64))
    s = np.sqrt(wss)
    return float(np.abs((a - b) * s).max() / np.abs(b * s).max())


@functools.lru_cache(maxsize=None)
def win_hop_case():
    """win == hop, zero iterations, three utterances (2, 3 and 40 frames): spectrogram, uniforms, the fp64 result and the restatement's weighted error."""
    n_fft, hop, win = SETS["win_hop"]
    out = []
    for T in GL_FRAMES:
        spec = _ro(normalised(raw_magnitudes(speech_like(hop * (T - 1), T), n_fft, hop, win)))
        u = uniforms(T, n_fft // 2 + 1, 200 + T)
        want = _ro(griffin_lim(spec, u, 0, n_fft, hop, win))
        e32 = weighted_err(griffin_lim(spec, u, 0, n_fft, hop, win, dtype=np.float32), want, n_fft, hop, win, T)
        out.append(dict(T=T, spec=spec, u=u, want=want, e32=e32))
    return out


# ---- the seeded initial phase ------------------------------------------------------------------------------------------------------------------
def seeded_uniforms(T, nb, seed):
    """griffin_lim_kernel's own uniforms [T, nb], float64 values exact in float32: Philox4x32-10 with counter (k >> 2, frame, 0x474c494d, 0) and
    the key (low word, high word) of the utterance's seed, word k & 3 of the block, its top 24 bits times 2^-24."""
    k, f = np.arange(nb, dtype=np.uint32)[None, :], np.arange(T, dtype=np.uint32)[:, None]
    c0, c1 = np.broadcast_arrays(k >> np.uint32(2), f)
    seed = int(seed) % (1 << 64)
    words = ORNG.philox4x32_10(c0, c1, np.full(c0.shape, 0x474c494d, np.uint32), np.zeros(c0.shape, np.uint32), seed & 0xFFFFFFFF, seed >> 32)
    w = np.take_along_axis(np.stack(words, axis=2), (np.broadcast_to(k, c0.shape) & 3)[:, :, None].astype(np.int64), axis=2)[:, :, 0]
    return (w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


# ---- the mel stage alone ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mel_case(n_mel, n_fft=512, frames=3):
    """A synthetic filterbank [n_mel, NB] (float32, zero outside each filter's range) with its ranges [n_mel, 2] (int32) - lengths cycling through
    MEL_LENGTHS, starting at filter n_mel's own phase of the cycle so that every count meets every length at its edges, at positions spread over
    the bins - and magnitudes [frames, NB] (float32) such that every non-empty filter's sum lies in (1e-4, 1e-1), inside both clips."""
    NB = n_fft // 2 + 1
    g = np.random.default_rng(7000 + n_mel)
    fb, rng = np.zeros((n_mel, NB), np.float32), np.zeros((n_mel, 2), np.int32)
    for c in range(n_mel):
        L = MEL_LENGTHS[(c + n_mel) % len(MEL_LENGTHS)]
        L = NB if L is None else L
        lo = int(g.integers(0, NB - L + 1))
        rng[c] = (lo, lo + L)
        if L:
            fb[c, lo:lo + L] = g.uniform(0.5, 1.5, L) * 10.0 ** g.uniform(-3.0, -1.7) / L
    mag = g.uniform(0.5, 1.5, (frames, NB)).astype(np.float32)
    sums = mag.astype(np.float64) @ fb.astype(np.float64).T
    ne = rng[:, 1] > rng[:, 0]
    assert (sums[:, ne] > 1e-4).all() and (sums[:, ne] < 1e-1).all() and (sums[:, ~ne] == 0).all()
    return dict(fb=_ro(fb), rng=_ro(rng), mag=_ro(mag), empty=_ro(~ne))


def mel_stage(mag, fb, rng, max_abs=None, dtype=np.float64):
    """The mel stage of stft_frame_body: filter sums over each filter's range, 20 log10(max(1e-5, .)), then the [0, 1] normalisation
    (max_abs None, Audio._normalize) or the symmetric one -> [frames, n_mel] in `dtype`."""
    mag, fb = np.asarray(mag, dtype), np.asarray(fb, dtype)
    m = np.stack([mag[:, lo:hi] @ fb[c, lo:hi] if hi > lo else np.zeros(mag.shape[0], dtype) for c, (lo, hi) in enumerate(np.asarray(rng))], axis=1)
    db = dtype(20) * np.log10(np.maximum(dtype(1e-5), m))
    v = (db + dtype(100)) * dtype(0.01)
    out = np.clip(v, 0, 1) if max_abs is None else np.clip(dtype(2 * max_abs) * v - dtype(max_abs), -max_abs, max_abs)
    assert out.dtype == dtype
    return out


def mel_table():
    """The largest restatement figure of the mel-stage test, on the [0, 1] scale (the symmetric run at 128 filters divided by 2 max_abs)."""
    figs = []
    for n_mel in MEL_COUNTS:
        c = mel_case(n_mel)
        figs.append(float(np.abs(mel_stage(c["mag"], c["fb"], c["rng"], dtype=np.float32) - mel_stage(c["mag"], c["fb"], c["rng"])).max()))
    c = mel_case(128)
    figs.append(float(np.abs(mel_stage(c["mag"], c["fb"], c["rng"], 4.0, np.float32) - mel_stage(c["mag"], c["fb"], c["rng"], 4.0)).max()) / 8.0)
    return max(figs)


WRAPPER_MEL = {2048: (1025, 12.5, 50), 512: (257, 8, 32)}          # (num_freq, frame_shift_ms, frame_length_ms) at 16 kHz: hop 200 win 800, hop 128 win 512


@functools.lru_cache(maxsize=None)
def wrapper_mel_case(n_fft):
    """The real 128-filter Slaney bank at 16 kHz through the whole frame (transform + mel stage, [0, 1] normalisation): a tone-plus-noise waveform
    of a handful of frames, oracle.audio's fp64 mel [frames, 128] and the restatement's error on that scale.  At n_fft = 512 the lowest filters
    are one bin wide."""
    from oracle import audio as OA
    num_freq, shift, length = WRAPPER_MEL[n_fft]
    _, hop, win = OA.stft_parameters(num_freq, shift, length, 16000)
    y = _ro(np.float32(0.05) * tone_plus_noise(n_fft // 2 + 5 * hop + 19, 50 + n_fft))      # (scaled so that the tone stays below the upper clip)
    ref = _ro(np.ascontiguousarray(OA.melspectrogram(y.astype(np.float64), num_freq, shift, length, 128, 16000, max_abs_value=None).T))
    fb = OA.mel_basis(16000, n_fft, 128).astype(np.float32)
    rng = filter_ranges(fb)
    r32 = mel_stage(raw_magnitudes(y, n_fft, hop, win, dtype=np.float32), fb, rng, dtype=np.float32)
    return dict(wav=y, ref=ref, e32=float(np.abs(r32 - ref).max()), widths=_ro(rng[:, 1] - rng[:, 0]), args=(num_freq, shift, length, 128, 16000))


def filter_ranges(fb):
    """Audio._fft_constants' ranges of a filterbank: [first non-zero bin, last + 1) per filter, (0, 0) for an empty one."""
    rng = np.zeros((fb.shape[0], 2), np.int32)
    for c in range(fb.shape[0]):
        nz = np.nonzero(fb[c])[0]
        if len(nz):
            rng[c] = (nz[0], nz[-1] + 1)
    return rng
