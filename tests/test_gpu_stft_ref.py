"""The STFT kernel family (csrc/fft_stages.h, csrc/stft_frame.h, csrc/stft_parts.h) against the fp64 statements of tests/stft_ref.py across the
envelope its entry points declare: odd window offsets, windows that are no multiple of the hop and odd, n_fft = 4096 (both buffers the Stockham
stages can return), hop <= win < 2 hop, win == hop, utterances of two samples, more than 85 mel filters and filter ranges of 0, 1 and 2 bins, and
the seeded initial phase restated on the host.

Bounds: no bound comes from the device.  Per test the fp32 CPU restatement (torch.fft in float32 on float32 frames, float32 overlap-add) is
measured against the same fp64 reference with the same error measure on the same inputs; the device must stay within MARGIN = 4 times the LARGEST
restatement figure of the test's table (room for another factorisation and summation order, which is what separates the device FFT from torch's),
and below the ceilings - 1e-5 of the frame peak for raw magnitudes, ten times the 5.4e-7 ruler of tests/test_gpu_griffin_lim.py for the round trips,
1e-6 on the [0, 1] scale for the mel stage alone - above which a figure is a defect to be found: both are asserted, so the bound in force is the
smaller of the two.  The restatement is computed where the test runs, so its figures move a little with the host's FFT library; those quoted in
the docstrings are the MI355X host's.  Every figure is printed before it is asserted (run with -s); the figures of the MI355X run stand in the
docstrings and in profiles/stft_ref_parity.txt."""
import numpy as np
import pytest
import torch

from multi_speaker_tts_amd import Audio, lib
from tests import stft_ref as R

pytestmark = pytest.mark.gpu
GUARD = 512


def _guarded(dev, n):
    """A NaN-filled output of n floats with a guard pattern behind it."""
    b = torch.full((n + GUARD,), float("nan"), device=dev)
    b[n:] = 12345.0
    return b


def _taken(buf, n):
    h = buf.cpu().numpy()
    assert np.all(h[n:] == 12345.0), "written behind the output"
    return h[:n]


def _raw(dev, wavs, n_fft, hop, win, coef):
    """mstts_stft_fft with flags = 2, spec_out set and no mel - Audio._stft_packed's first spectral-subtraction launch - on a packed batch ->
    list of [frames, n_fft // 2 + 1] raw magnitudes."""
    hann, tw = Audio._fft_constants_samples(n_fft, win, str(dev))
    lens = [int(w.shape[0]) for w in wavs]
    frames = [1 + n // hop for n in lens]
    woff = torch.tensor(Audio._offsets(lens), device=dev)
    foff = torch.tensor(Audio._offsets(frames), device=dev)
    cat = torch.tensor(np.concatenate(wavs), device=dev)
    total, nb = sum(frames), n_fft // 2 + 1
    out = _guarded(dev, total * nb)
    lib.call("mstts_stft_fft", lib.ptr(cat), lib.ptr(woff), lib.ptr(foff), len(wavs), float(coef), lib.ptr(hann), lib.ptr(tw), None, None, n_fft, hop, win,
             0, 1.0, 20.0, None, lib.ptr(out), total, None, None, 0.0, 2)
    h = _taken(out, total * nb).reshape(total, nb)
    assert np.isfinite(h).all()
    return [h[a:b] for a, b in zip(np.cumsum([0] + frames[:-1]), np.cumsum(frames))]


@pytest.mark.parametrize("name", R.RAW_SETS)
def test_gpu_raw_magnitudes(dev, name):
    """Raw magnitudes (flags & 2) of three tone-plus-noise waveforms in one launch, and of a frame-aligned unit impulse without pre-emphasis (flat
    magnitudes at the window's value: a mis-indexed bin or a mis-placed window shows), against fp64 |rfft(window * reflect_pad(preemph(x)))| frame
    by frame, error max_k |dev - ref| / max_k ref; a frame the impulse's window does not reach must be exactly zero.  Bound: 4 x 4.186e-07 (the
    restatement's largest, (4096, 600, 1801)), ceiling 1e-5.  mstts_stft_bank_batch takes no flags argument, so its raw form cannot be entered.
    Measured on the MI355X, worst frame of the three waveforms / of the impulse (restatement's in brackets): (512, 128, 510) 3.092e-07 / 1.468e-08
    (2.203e-07 / 1.468e-08); (1024, 300, 702) 1.006e-07 / 1.350e-07 (9.923e-08 / 1.350e-07); (4096, 600, 1801) 3.988e-07 / 1.425e-07 (4.186e-07 /
    2.950e-07); (4096, 1024, 4096) 1.652e-07 / 2.2e-16 (1.631e-07 / 2.2e-16); (512, 200, 300) 1.953e-07 / 0 (2.440e-07 / 0); (2048, 200, 800)
    1.907e-07 / 1.788e-07 (1.738e-07 / 2.384e-07); (512, 300, 200) 1.441e-07 / 0 (1.297e-07 / 0) (profiles/stft_ref_parity.txt)."""
    n_fft, hop, win = R.triple(name)
    c = R.raw_case(name)
    bound = R.MARGIN * R.raw_table()
    got = _raw(dev, c["wavs"], n_fft, hop, win, R.PREEMPH)
    errs = [float(R.frame_peak_err(g, r).max()) for g, r in zip(got, c["ref"])]
    imp, = _raw(dev, [c["imp"]], n_fft, hop, win, 0.0)
    e_imp = float(R.frame_peak_err(imp, c["imp_ref"]).max())
    print("stft_ref raw magnitudes: %-8s %s: device %s impulse %.3e | fp32 restatement %s impulse %.3e | bound %.3e"
          % (name, (n_fft, hop, win), " ".join("%.3e" % e for e in errs), e_imp, " ".join("%.3e" % e for e in c["e32"]), c["imp_e32"], bound))
    assert max(errs + [e_imp]) < R.CEIL_RAW, "a defect, not a bound to be widened"
    assert max(errs + [e_imp]) < bound, (name, errs, e_imp, bound)


def _mel_alone(dev, mag, fb, rng, max_abs):
    """The mag_in path of mstts_stft_fft with sub = None: no transform, the given magnitudes against the given filterbank -> [frames, n_mel]."""
    frames, nb = mag.shape
    n_fft, n_mel = 2 * (nb - 1), fb.shape[0]
    hann, tw = Audio._fft_constants_samples(n_fft, n_fft, str(dev))
    one = torch.tensor([0, 0], dtype=torch.int64, device=dev)
    up = lambda a: torch.tensor(np.ascontiguousarray(a), device=dev)
    mag_d, fb_d, rng_d, wav = up(mag), up(fb), up(rng), torch.zeros(16, device=dev)
    assert fb_d.dtype == torch.float32 and rng_d.dtype == torch.int32 and mag_d.dtype == torch.float32
    out = _guarded(dev, frames * n_mel)
    lib.call("mstts_stft_fft", lib.ptr(wav), lib.ptr(one), lib.ptr(one), 1, R.PREEMPH, lib.ptr(hann), lib.ptr(tw), lib.ptr(fb_d), lib.ptr(rng_d), n_fft,
             n_fft // 4, n_fft, n_mel, 1.0 if max_abs is None else float(max_abs), 20.0, lib.ptr(out), None, frames, lib.ptr(mag_d), None, 0.0,
             1 if max_abs is None else 0)
    return _taken(out, frames * n_mel).reshape(frames, n_mel)


@pytest.mark.parametrize("n_mel", R.MEL_COUNTS)
def test_gpu_mel_stage_alone(dev, n_mel):
    """The mel stage on given magnitudes (n_fft 512, three frames) with synthetic banks whose ranges have 0, 1, 2, 3, 4, 7 and all 257 bins, at 1,
    84, 85, 86, 128 and 255 filters - one, two and three passes of the 85-filter loop - in the [0, 1] normalisation; at 128 filters the symmetric
    one as well, judged on the same scale (divided by 2 max_abs).  An empty range gives exactly the clipped floor.  Bound: 4 x 1.124e-07, ceiling
    1e-6.  Measured on the MI355X at 1 / 84 / 85 / 86 / 128 / 255 filters: 5.387e-08, 9.996e-08, 1.020e-07, 1.118e-07, 1.265e-07 (symmetric / 8:
    1.265e-07), 1.318e-07; the restatement: 6.752e-08, 9.688e-08, 9.856e-08, 1.106e-07, 1.124e-07, 1.112e-07 (profiles/stft_ref_parity.txt)."""
    c = R.mel_case(n_mel)
    bound = R.MARGIN * R.mel_table()
    runs = [(None, 1.0)] + ([(4.0, 8.0)] if n_mel == 128 else [])
    for max_abs, scale in runs:
        ref = R.mel_stage(c["mag"], c["fb"], c["rng"], max_abs)
        got = _mel_alone(dev, c["mag"], c["fb"], c["rng"], max_abs)
        assert np.isfinite(got).all(), "a filter was not written"
        e = float(np.abs(got - ref).max() / scale)
        print("stft_ref mel stage: n_mel %3d %s: device %.3e | bound %.3e" % (n_mel, "symmetric / 8" if max_abs else "[0, 1]     ", e, bound))
        assert (got[:, c["empty"]] == (0.0 if max_abs is None else -max_abs)).all()
        assert e < R.CEIL_MEL, "a defect, not a bound to be widened"
        assert e < bound, (n_mel, max_abs, e, bound)


@pytest.mark.parametrize("n_fft", sorted(R.WRAPPER_MEL))
def test_gpu_real_mel_bank_through_the_wrapper(dev, n_fft):
    """Audio.melspectrogram with the real 128-filter Slaney bank at 16 kHz (two passes of the filter loop; one-bin filters at n_fft 512), [0, 1]
    normalisation, against oracle.audio in fp64.  Bound: 4 x the larger of the restatement's two figures (1.633e-06: the tone stands 35 dB above the
    noise bins, whose error is relative to the frame's peak).  Measured on the MI355X: n_fft 512 1.687e-06 (restatement 1.367e-06), n_fft 2048
    9.171e-07 (1.633e-06) on the [0, 1] scale (profiles/stft_ref_parity.txt)."""
    c = R.wrapper_mel_case(n_fft)
    bound = R.MARGIN * max(R.wrapper_mel_case(k)["e32"] for k in R.WRAPPER_MEL)
    num_freq, shift, length, n_mel, rate = c["args"]
    got = Audio.melspectrogram(c["wav"].copy(), num_freq, shift, length, n_mel, rate, max_abs_value=None, device=dev).T
    assert got.shape == c["ref"].shape and np.isfinite(got).all()
    e = float(np.abs(got - c["ref"]).max())
    print("stft_ref real mel bank: n_fft %4d: device %.3e | fp32 restatement %.3e | bound %.3e" % (n_fft, e, c["e32"], bound))
    assert e < bound, (n_fft, e, bound)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("name", R.DENOISE_SETS + R.DENOISE_EXTRA)
def test_gpu_denoiser_is_the_identity_at_strength_zero(dev, name):
    """strength = 0 with a non-zero bias: the output is the input - a reference that needs no host code.  Three lengths in one batch per set,
    error max |y - x| / max |x|; an all-zero waveform in the middle of the batch comes back exactly zero and leaves its neighbours' bits what
    they are without it.  Bound: 4 x 4.848e-07 (the restatement's largest), ceiling 5.4e-6.  Measured on the MI355X, the largest
    of the three lengths (restatement's in brackets): (512, 128, 510) 3.108e-07 (2.331e-07); (1024, 300, 702) 2.257e-07 (4.848e-07);
    (4096, 600, 1801) 2.556e-07 (3.195e-07); (4096, 1024, 4096) 2.707e-07 (3.374e-07); (2048, 200, 800) 2.146e-07 (2.047e-07); (512, 2, 8)
    1.466e-07 (1.997e-07) (profiles/stft_ref_parity.txt)."""
    n_fft, hop, win = R.triple(name)
    c = R.denoise_case(name)
    bound = R.MARGIN * R.denoise_table((0.0,))
    got = Audio.spectral_denoise_batch(c["wavs"], c["bias"], 0.0, n_fft, hop, win, device=dev)
    errs = []
    for x, y in zip(c["wavs"], got):
        assert y.dtype == np.float32 and y.shape == x.shape and np.isfinite(y).all()
        errs.append(float(np.abs(y.astype(np.float64) - x).max() / np.abs(x).max()))
    print("stft_ref denoiser identity: %-8s %s: device %s | fp32 restatement %.3e | bound %.3e"
          % (name, (n_fft, hop, win), " ".join("%.3e" % e for e in errs), c["e32"][0.0], bound))
    zero = np.zeros(c["wavs"][1].shape[0], np.float32)
    with_zero = Audio.spectral_denoise_batch([c["wavs"][0], zero, c["wavs"][2]], c["bias"], 1.0, n_fft, hop, win, device=dev)
    without = Audio.spectral_denoise_batch([c["wavs"][0], c["wavs"][2]], c["bias"], 1.0, n_fft, hop, win, device=dev)
    assert np.isfinite(with_zero[1]).all() and not with_zero[1].any(), "an all-zero waveform must come back exactly zero"
    assert _same_bits(with_zero[0], without[0]) and _same_bits(with_zero[2], without[1])
    assert max(errs) < R.CEIL_TRIP, "a defect, not a bound to be widened"
    assert max(errs) < bound, (name, errs, bound)


@pytest.mark.parametrize("name", R.DENOISE_SETS + R.DENOISE_EXTRA)
def test_gpu_denoiser_parity(dev, name):
    """Strengths 0.1 and 1 against the fp64 statement (Audio.spectral_denoise's arithmetic, tests/test_cpu_stft_ref.py), bias = the per-bin median
    of the inputs' own magnitudes, so that half of the bins are clamped at strength 1 (asserted without a GPU for every set).  Bound: 4 x
    4.178e-07, ceiling 5.4e-6.  Measured on the MI355X at strengths 0.1 / 1, the largest of the three lengths (restatement's in brackets):
    (512, 128, 510) 2.352e-07 / 1.843e-07 (2.911e-07 / 2.243e-07); (1024, 300, 702) 3.089e-07 / 2.530e-07 (4.178e-07 / 2.094e-07);
    (4096, 600, 1801) 2.588e-07 / 2.315e-07 (2.472e-07 / 2.284e-07); (4096, 1024, 4096) 2.864e-07 / 2.318e-07 (3.292e-07 / 2.920e-07);
    (2048, 200, 800) 2.496e-07 / 2.126e-07 (2.488e-07 / 1.704e-07); (512, 2, 8) 1.382e-07 / 4.200e-08 (1.923e-07 / 7.962e-08)
    (profiles/stft_ref_parity.txt)."""
    n_fft, hop, win = R.triple(name)
    c = R.denoise_case(name)
    bound = R.MARGIN * R.denoise_table((0.1, 1.0))
    worst = {}
    for s in (0.1, 1.0):
        got = Audio.spectral_denoise_batch(c["wavs"], c["bias"], s, n_fft, hop, win, device=dev)
        errs = []
        for x, y, w in zip(c["wavs"], got, c["want"][s]):
            assert y.dtype == np.float32 and y.shape == x.shape == w.shape and np.isfinite(y).all()
            errs.append(float(np.abs(y - w).max() / np.abs(x).max()))
        worst[s] = max(errs)
        print("stft_ref denoiser parity: %-8s %s strength %.1f: device %s | fp32 restatement %.3e | bound %.3e"
              % (name, (n_fft, hop, win), s, " ".join("%.3e" % e for e in errs), c["e32"][s], bound))
    assert max(worst.values()) < R.CEIL_TRIP, "a defect, not a bound to be widened"
    assert max(worst.values()) < bound, (name, worst, bound)


def test_gpu_denoiser_refuses_what_the_envelope_excludes(dev):
    """(512, 200, 300) - win < 2 hop - is refused by the entry's return code, and the wrapper answers through the host function."""
    n_fft, hop, win = R.SETS["sparse"]
    x = R.tone_plus_noise(700, 1)
    buf = torch.zeros(4096, device=dev)
    off = torch.tensor([0, 700, 0, 4], dtype=torch.int64, device=dev)
    import ctypes
    with pytest.raises(lib.MsttsError, match="2 hop <= win"):
        lib.call("mstts_wg_denoise", lib.ptr(buf), (ctypes.c_int64 * 2)(0, 700), lib.ptr(off), lib.ptr(off, 2), 1, lib.ptr(buf), 1.0, lib.ptr(buf),
                 lib.ptr(buf), n_fft, hop, win, lib.ptr(buf), lib.ptr(buf))
    bias = np.full(n_fft // 2 + 1, 0.5, np.float32)
    y, = Audio.spectral_denoise_batch([x], bias, 1.0, n_fft, hop, win, device=dev)
    assert np.array_equal(y, Audio.spectral_denoise(x, bias, 1.0, n_fft, hop, win).astype(np.float32))


@pytest.mark.parametrize("iters", [0, 1, 3])
@pytest.mark.parametrize("name", R.GL_SETS)
def test_gpu_griffin_lim(dev, name, iters):
    """Utterances of 2, 3 and 40 frames in one call, 0, 1 and 3 iterations, against the fp64 statement (Audio.inv_spectrogram's arithmetic) with the
    same float32-rounded uniforms; spectrograms of the speech-like signal by the host stft, seeds for which the fp32 restatement is not fragile
    (stft_ref.GL_FIGURES).  Error peak-relative.  Bounds: 4 x 7.285e-07 / 6.471e-07 / 7.545e-07 (the restatement's largest at 0 / 1 / 3
    iterations), ceiling 5.4e-6.  Measured on the MI355X, the largest of the 21 cases at 0 / 1 / 3 iterations: 6.416e-07 ((512, 200, 300), 2 frames) /
    7.448e-07 / 7.144e-07 (both (512, 128, 510), 3 frames); the two-sample utterance of (512, 2, 8): 3.446e-07 / 3.283e-08 / 7.996e-08; every case
    in profiles/stft_ref_parity.txt."""
    n_fft, hop, win = R.triple(name)
    cases = [R.gl_case(k, t) for k, t in R.gl_cases() if k == name]
    assert len(cases) == len(R.GL_FRAMES)                                  # no case of the table is dropped
    bound = R.MARGIN * R.gl_table(iters)
    got = Audio.griffin_lim_batch([c["spec"] for c in cases], *R.ms_args(n_fft, hop, win), griffin_lim_iters=iters, phase=[c["u"].T for c in cases], device=dev)
    errs = []
    for c, y in zip(cases, got):
        assert y.dtype == np.float32 and np.isfinite(y).all() and y.shape == c["want"][iters].shape
        errs.append(R.peak_err(y, c["want"][iters]))
    print("stft_ref griffin_lim: %-8s %s %d iterations, %s frames: device %s | fp32 restatement %s | bound %.3e"
          % (name, (n_fft, hop, win), iters, "/".join(str(c["spec"].shape[0]) for c in cases), " ".join("%.3e" % e for e in errs),
             " ".join("%.3e" % c["e32"][iters] for c in cases), bound))
    assert max(errs) < R.CEIL_TRIP, "a defect, not a bound to be widened"
    assert max(errs) < bound, (name, iters, errs, bound)


def test_gpu_griffin_lim_where_win_equals_hop(dev):
    """(512, 256, 256), zero iterations: istft divides by a window-square sum that is exactly 0 at each frame's first sample (stft_ola's
    den > tiny fallback: the sample stays undivided) and tiny beside it.  Every device sample is finite.  The error undoes the de-emphasis on both
    sides in fp64, weights the difference by sqrt(wss[j]) and divides by the peak of the host signal weighted the same way.  Bound: 4 x 4.642e-05,
    the restatement's largest.  The round trips' ceiling of 5.4e-6 cannot be asked in this measure: the fp64 result merely rounded to float32
    stands at 2.0e-6 / 2.2e-5 / 3.5e-5 (2 / 3 / 40 frames; tests/test_cpu_stft_ref.py), the de-emphasis carrying the spikes through every stored
    sample.  Measured on the MI355X at 2 / 3 / 40 frames: 1.173e-05 / 7.243e-05 / 1.324e-04 (restatement 2.545e-06 / 4.010e-05 /
    4.642e-05): up to three times the restatement's - supposed, not shown, to be the blocked scan of gl_deemphasis_kernel, which
    rounds several partial states of the spikes' size per sample where the sample-by-sample filter rounds one (profiles/stft_ref_parity.txt)."""
    n_fft, hop, win = R.SETS["win_hop"]
    cases = R.win_hop_case()
    bound = R.MARGIN * max(c["e32"] for c in cases)
    got = Audio.griffin_lim_batch([c["spec"] for c in cases], *R.ms_args(n_fft, hop, win), griffin_lim_iters=0, phase=[c["u"].T for c in cases], device=dev)
    errs = []
    for c, y in zip(cases, got):
        assert y.dtype == np.float32 and y.shape == c["want"].shape
        assert np.isfinite(y).all(), "0 / 0 where the window-square sum vanishes"
        errs.append(R.weighted_err(y, c["want"], n_fft, hop, win, c["T"]))
    print("stft_ref griffin_lim win == hop: device %s | fp32 restatement %s | bound %.3e"
          % (" ".join("%.3e" % e for e in errs), " ".join("%.3e" % c["e32"] for c in cases), bound))
    assert max(errs) < bound, (errs, bound)


@pytest.mark.parametrize("name", R.SEEDED_SETS)
def test_gpu_seeded_phase_is_the_host_philox(dev, name):
    """seed = [s0, s1, s2] against phase = the same uniforms built on the host from oracle.rng.philox4x32_10 by the rule in griffin_lim.hip's comment
    (counter (k >> 2, frame, 0x474c494d, 0), key = the seed's low and high word, word k & 3, >> 8, times 2^-24): equal bits, three utterances of
    2, 5 and 9 frames, 3 iterations, seeds 0, 2^32 + 5 and 2^64 - 1."""
    n_fft, hop, win = R.triple(name)
    nb = n_fft // 2 + 1
    specs = [R.normalised(R.raw_magnitudes(R.speech_like(hop * (t - 1), 20 + t), n_fft, hop, win)) for t in R.SEEDED_FRAMES]
    args = R.ms_args(n_fft, hop, win)
    seeded = Audio.griffin_lim_batch(specs, *args, griffin_lim_iters=3, seed=list(R.SEEDS), device=dev)
    given = Audio.griffin_lim_batch(specs, *args, griffin_lim_iters=3, phase=[R.seeded_uniforms(t, nb, s).T for t, s in zip(R.SEEDED_FRAMES, R.SEEDS)],
                                    device=dev)
    for t, a, b in zip(R.SEEDED_FRAMES, seeded, given):
        assert a.shape == (hop * (t - 1),) and np.isfinite(a).all() and np.abs(a).max() > 0
        assert _same_bits(a, b), (name, t, float(np.abs(a - b).max()))
    low_only = Audio.griffin_lim_batch(specs[1:2], *args, griffin_lim_iters=3, seed=[5], device=dev)
    assert not np.array_equal(low_only[0], seeded[1])                      # the high key word is live
