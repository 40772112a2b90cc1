"""tests/stft_ref.py checked without a GPU: its fp64 statements in samples are Audio's host functions at the anchor set and torch's stft / istft
at two of the new sets (odd `off` included); the conditions the GPU tests rely on hold for every case of the tables (the parameter triples through
Audio._stft_parameters, the envelope predicates, the denoiser's clamp share, the Griffin-Lim cases' fragility condition, the mel case's value
ranges, the impulse's known answer, the seeded uniforms' grouping); and the fp32 restatement's figures - the rulers of
tests/test_gpu_stft_ref.py - are printed (run with -s to read them)."""
import numpy as np
import pytest
import torch

from multi_speaker_tts_amd import Audio, lib
from oracle import rng as ORNG
from tests import stft_ref as R

ANCHOR_MS = (1025, 12.5, 50, 16000)


def test_parameter_sets_and_envelopes():
    """Every triple comes back from Audio._stft_parameters at 1000 samples a second; mstts_stft_fft takes all of them; Griffin-Lim takes every
    set of the table and refuses hop > win; the denoiser takes 2 hop <= win <= 4 hop - which (512, 2, 8) satisfies, so it is ADMITTED (the
    GPU tests run it) - and refuses (512, 200, 300), (512, 256, 256) and hop > win.  The lengths are what the tests say they are."""
    L = lib.load()
    for name in list(R.SETS) + list(R.FORWARD_ONLY):
        n_fft, hop, win = R.triple(name)
        assert Audio._stft_parameters(*R.ms_args(n_fft, hop, win)) == (n_fft, hop, win), name
        assert L.mstts_stft_fft_supported(n_fft, win) == 1, name
        assert bool(L.mstts_griffin_lim_supported(n_fft, hop, win)) == (name in R.SETS), name
        assert Audio.griffin_lim_supported(*R.ms_args(n_fft, hop, win), frames=list(R.GL_FRAMES)) == (name in R.SETS), name
        assert bool(L.mstts_wg_denoise_supported(n_fft, hop, win)) == (name in R.DENOISE_SETS + R.DENOISE_EXTRA) == (2 * hop <= win <= 4 * hop), name
        assert Audio.spectral_denoise_supported(n_fft, hop, win) == (name in R.DENOISE_SETS + R.DENOISE_EXTRA), name
        a, b, c = R.lengths(n_fft, hop)
        assert a == n_fft // 2 + 1 and b > n_fft // 2 and b % hop != 0 and c > n_fft // 2 and c % hop == 0
        assert n_fft < 4096 or 1 + c // hop <= 10
    offs = {k: (v[0] - v[2]) >> 1 for k, v in R.SETS.items()}
    assert offs["odd_off"] == 1 and offs["off161"] == 161 and offs["odd_win"] == 1147 and R.SETS["odd_win"][2] % 2 == 1
    assert [2 * (t - 1) for t in R.GL_FRAMES] == [2, 4, 78]                # the samples of (512, 2, 8): reflection period 2 at two frames
    assert set(R.GL_SETS) == set(R.SETS) - {"win_hop"} and set(R.RAW_SETS) == (set(R.SETS) - set(R.GL_ONLY)) | {"gaps"}


def test_fp64_statements_are_audios_at_the_anchor():
    """stft / istft / denoise / griffin_lim in samples against Audio._stft / _stft_samples / _istft / _istft_samples / spectral_denoise /
    inv_spectrogram at (2048, 200, 800): the same arithmetic, to 1e-13 of the peak (measured: 0 to 4e-16)."""
    n_fft, hop, win = R.SETS["anchor"]
    x = R.tone_plus_noise(2043, 5).astype(np.float64)
    X = R.stft(x, n_fft, hop, win)
    for other in (Audio._stft(x, *ANCHOR_MS), Audio._stft_samples(x, n_fft, hop, win)):
        assert np.abs(X.T - other).max() <= 1e-13 * np.abs(other).max()
    g = np.random.default_rng(0)
    Y = X * g.uniform(0.2, 1.0, X.shape)
    assert R.peak_err(R.istft(Y, n_fft, hop, win), Audio._istft(Y.T, *ANCHOR_MS)) <= 1e-13
    assert R.peak_err(R.istft(Y, n_fft, hop, win, 2043), Audio._istft_samples(Y.T, n_fft, hop, win, 2043)) <= 1e-13
    bias = np.median(np.abs(X), axis=0)
    for s in (0.0, 0.1, 1.0):
        assert R.peak_err(R.denoise(x, bias, s, n_fft, hop, win), Audio.spectral_denoise(x, bias, s, n_fft, hop, win)) <= 1e-13
    from scipy import signal
    assert np.abs(R.preemphasis(x) - signal.lfilter([1, -0.97], [1], x)).max() <= 1e-15
    assert R.peak_err(R.deemphasis(x), Audio.inv_preemphasis(x)) <= 1e-15
    assert R.deemphasis(x.astype(np.float32), dtype=np.float32).dtype == np.float32


def test_griffin_lim_statement_is_the_host_path_on_every_case():
    """R.griffin_lim (fp64, in samples) against Audio.inv_spectrogram through the millisecond arguments with the same uniforms, every case of the
    table at 3 iterations, and win == hop at 0: two texts of the same arithmetic, 1e-9 of the peak (measured: 1e-15 or better)."""
    worst = 0.0
    for name, T in R.gl_cases():
        n_fft, hop, win = R.triple(name)
        c = R.gl_case(name, T)
        host = Audio.inv_spectrogram(c["spec"].astype(np.float64).T, *R.ms_args(n_fft, hop, win), griffin_lim_iters=3, rng=Audio._FixedPhase(c["u"].T))
        assert host.shape == (hop * (T - 1),)
        worst = max(worst, R.peak_err(c["want"][3], host))
    n_fft, hop, win = R.SETS["win_hop"]
    for c in R.win_hop_case():
        host = Audio.inv_spectrogram(c["spec"].astype(np.float64).T, *R.ms_args(n_fft, hop, win), griffin_lim_iters=0, rng=Audio._FixedPhase(c["u"].T))
        worst = max(worst, R.peak_err(c["want"], host))
    print("stft_ref: griffin_lim statement against Audio.inv_spectrogram, worst of the tables: %.2e of the peak" % worst)
    assert worst <= 1e-9


@pytest.mark.parametrize("name", ["odd_off", "odd_win"])
def test_statements_are_torchs_stft_and_istft(name):
    """torch.stft(center=True, pad_mode="reflect", periodic Hann of win_length < n_fft centred) and torch.istft(length=n) in float64 at two of the
    new sets - off = 1 and an odd window with off = 1147 - to 1e-12 relative (measured: 5e-16 or better)."""
    n_fft, hop, win = R.SETS[name]
    g = np.random.default_rng(n_fft + hop)
    window = torch.hann_window(win, periodic=True, dtype=torch.float64)
    assert np.abs(window.numpy() - R.hann(win)).max() <= 1e-15
    for n in R.lengths(n_fft, hop):
        x = g.normal(0, 0.3, n)
        X = R.stft(x, n_fft, hop, win)
        Xt = torch.stft(torch.tensor(x), n_fft, hop, win, window, center=True, pad_mode="reflect", return_complex=True).numpy()
        assert X.shape == (1 + n // hop, n_fft // 2 + 1) == Xt.T.shape
        e_fwd = float(np.abs(X.T - Xt).max() / np.abs(Xt).max())
        Y = X * g.uniform(0.2, 1.0, X.shape)
        yt = torch.istft(torch.tensor(np.ascontiguousarray(Y.T)), n_fft, hop, win, window, center=True, length=n).numpy()
        e_inv = R.peak_err(R.istft(Y, n_fft, hop, win, n), yt)
        print("stft_ref torch pin: %s n %5d: stft %.2e istft %.2e" % (R.SETS[name], n, e_fwd, e_inv))
        assert e_fwd <= 1e-12 and e_inv <= 1e-12


def test_raw_magnitude_restatement_and_the_impulse_answer():
    """The fp32 restatement's frame-peak errors per set (the ruler of the raw-magnitude GPU test) stay below the ceiling 1e-5, and the
    impulse's fp64 magnitudes are flat at the window's value (to 1e-15), zero where the window does not reach it."""
    for name in R.RAW_SETS:
        n_fft, hop, win = R.triple(name)
        c = R.raw_case(name)
        print("stft_ref raw magnitudes fp32 restatement: %-8s %s: %s impulse %.3e" % (name, (n_fft, hop, win), " ".join("%.3e" % e for e in c["e32"]), c["imp_e32"]))
        assert max(c["e32"]) < R.CEIL_RAW and c["imp_e32"] < R.CEIL_RAW
        assert [r.shape for r in c["ref"]] == [(1 + n // hop, n_fft // 2 + 1) for n in R.lengths(n_fft, hop)]
        flat = R.impulse_answer(n_fft, hop, win, c["imp"].shape[0], c["imp_p"])
        assert np.abs(c["imp_ref"] - flat[:, None]).max() <= 1e-15 and flat.max() > 0.99 and (flat > 0).sum() >= (2 if win >= 2 * hop else 1)
        assert c["imp_p"] % hop == 0 and c["imp_p"] > n_fft // 2 and c["imp"].shape[0] - 1 - c["imp_p"] > n_fft // 2
    print("stft_ref raw magnitudes: largest restatement figure of the table %.3e" % R.raw_table())


def test_denoiser_cases():
    """Per set: the fp64 identity at strength 0 (1e-12 of the peak; measured 8e-16), the share of clamped bins at strength 1 in [0.2, 0.8] (0.5 by
    the bias' construction) so that the GPU test never has to skip a case, strength 1 moving the signal by far more than any bound, and the
    restatement's figures at strengths 0, 0.1 and 1 below ten times the ruler."""
    for name in R.DENOISE_SETS + R.DENOISE_EXTRA:
        n_fft, hop, win = R.triple(name)
        c = R.denoise_case(name)
        ident = max(float(np.abs(R.denoise(w.astype(np.float64), c["bias"], 0.0, n_fft, hop, win) - w).max() / np.abs(w).max()) for w in c["wavs"])
        moved = max(float(np.abs(y - w).max()) for y, w in zip(c["want"][1.0], c["wavs"]))
        print("stft_ref denoiser: %-8s %s: fp64 identity %.1e, clamped share %.3f, strength 1 moves %.3f; fp32 restatement at 0 / 0.1 / 1: %.3e %.3e %.3e"
              % (name, (n_fft, hop, win), ident, c["clamped"], moved, c["e32"][0.0], c["e32"][0.1], c["e32"][1.0]))
        assert ident <= 1e-12 and 0.2 <= c["clamped"] <= 0.8 and moved > 0.01
        assert max(c["e32"].values()) < R.CEIL_TRIP
        assert [w.shape[0] for w in c["wavs"]] == list(R.lengths(n_fft, hop))


def test_griffin_lim_cases_are_not_fragile():
    """Every (set, frame count) case: the fp32 restatement agrees with the fp64 statement within 10 x the ruler (5.4e-6 of the peak) at 3
    iterations - phase recovery is discontinuous where a bin is near zero, and a case where fp32 on the CPU alone parts from fp64 cannot judge a
    kernel.  The same is asked of the restatement with a second float32 transform (NumPy's): which transform trips over a near-zero bin depends
    on the transform, so a case two of them disagree on cannot judge a third.  No case had to be dropped (at most one in eight may be); the
    figures of the chosen seeds are printed beside those recorded in stft_ref.GL_FIGURES."""
    full = [(k, t) for k in R.GL_SETS for t in R.GL_FRAMES]
    assert set(R.GL_FIGURES) == set(full) and all(k in full for k in R.GL_DROPPED) and 8 * len(R.GL_DROPPED) <= len(full)
    for name, T in R.gl_cases():
        c = R.gl_case(name, T)
        seed, f1, f3, s1, s3 = R.GL_FIGURES[(name, T)]
        print("stft_ref griffin_lim fp32 restatement: %-8s %2d frames seed %d: 0 / 1 / 3 iterations %.3e %.3e %.3e (recorded %.2e %.2e); with NumPy's "
              "transform %.3e %.3e %.3e (recorded %.2e %.2e)" % (name, T, seed, c["e32"][0], c["e32"][1], c["e32"][3], f1, f3, c["screen"][0],
                                                                  c["screen"][1], c["screen"][3], s1, s3))
        assert max(c["screen"].values()) < R.CEIL_TRIP, (name, T, c["screen"])
        assert c["seed"] == seed and c["spec"].shape == (T, R.triple(name)[0] // 2 + 1)
        assert c["spec"].max() > 0.03 and (T < 40 or c["spec"].max() > 0.3)  # a signal above the clip floor (two samples of the faded-in start are quiet)
        assert c["e32"][3] < R.CEIL_TRIP and c["e32"][1] < R.CEIL_TRIP and c["e32"][0] < R.CEIL_TRIP, (name, T, c["e32"])
    print("stft_ref griffin_lim: largest restatement figures of the table at 0 / 1 / 3 iterations: %.3e %.3e %.3e" % (R.gl_table(0), R.gl_table(1), R.gl_table(3)))


def test_win_equals_hop_case():
    """win == hop: the host's window-square sum is exactly 0 at each frame's first sample (the sample stays undivided) and tiny beside it, the
    host output's peak is far above the signal's, and in the weighted measure the fp64 result merely ROUNDED to float32 already stands at
    2e-6 .. 4e-5 (the de-emphasis carries the spikes' memory through every stored sample) - above the round trips' ceiling of 5.4e-6, which
    therefore cannot be asked of any float32 output in this measure; the transform's own share is 2e-7."""
    n_fft, hop, win = R.SETS["win_hop"]
    for c in R.win_hop_case():
        T = c["T"]
        wss = R.window_square_sum(T, n_fft, hop, win)[n_fft // 2:n_fft // 2 + hop * (T - 1)]
        assert (wss[hop // 2::hop] == 0).all() and 0 < wss[hop // 2 + 1] < 1e-6
        rounded = R.weighted_err(c["want"].astype(np.float32), c["want"], n_fft, hop, win, T)
        a = R.griffin_lim(c["spec"], c["u"], 0, n_fft, hop, win, dtype=np.float32, deemph=False)
        b = R.griffin_lim(c["spec"], c["u"], 0, n_fft, hop, win, deemph=False)
        s = np.sqrt(wss)
        own = float(np.abs((a - b) * s).max() / np.abs(b * s).max())
        print("stft_ref win == hop: %2d frames: host peak %.1f; weighted error of the fp32 restatement %.3e, of the fp64 result rounded to float32 %.3e, "
              "of the fp32 transform before the de-emphasis %.3e" % (T, np.abs(c["want"]).max(), c["e32"], rounded, own))
        assert np.isfinite(c["want"]).all() and np.abs(c["want"]).max() > 2.0
        assert own < R.CEIL_TRIP and c["e32"] < 1e-3


def test_seeded_uniforms():
    """The host restatement of griffin_lim_kernel's Philox uniforms: all in [0, 1) and exact in float32; the grouping by fours gives distinct
    values at k = 4m .. 4m + 3 and at k, k + 4; frame 0 is oracle.rng.uniform_words of stream 0x474c494d; the seed's high word, the frame and the
    seed all change the draw."""
    T, nb = 9, 2049
    for seed in R.SEEDS:
        u = R.seeded_uniforms(T, nb, seed)
        assert u.shape == (T, nb) and u.dtype == np.float64 and (u >= 0).all() and (u < 1).all()
        assert np.array_equal(u.astype(np.float32).astype(np.float64), u) and np.array_equal(u * 2.0 ** 24, np.floor(u * 2.0 ** 24))
        quads = u[:, :2048].reshape(T, 512, 4)
        assert all(len(set(q)) == 4 for q in quads.reshape(-1, 4))         # four different words of one block
        assert (u[:, :-4] != u[:, 4:]).all()                                # the next block is another draw
        words = ORNG.uniform_words(nb, seed, 0x474c494d)
        assert np.array_equal(u[0], (words >> np.uint32(8)).astype(np.float64) * 2.0 ** -24)
        assert not np.array_equal(u[0], u[1])
        assert 0.45 < u.mean() < 0.55
    a, b, c = (R.seeded_uniforms(2, 257, s) for s in (5, (1 << 32) + 5, (1 << 64) - 1))
    assert not np.array_equal(a, b) and not np.array_equal(b, c)
    assert np.array_equal(R.seeded_uniforms(2, 257, -1), c)                  # seeds are taken modulo 2^64, as griffin_lim_batch takes them


def test_mel_cases():
    """The synthetic banks: every count has ranges of length 0, 1, 2 (threads of the three-per-filter split without work) and, from 7 filters on,
    all seven lengths; the filters at the pass edges (84, 85, 86 / 169, 170) exist where the count reaches them; every non-empty sum lies in
    (1e-4, 1e-1) (asserted when the case is built), so the [0, 1] values lie in (0.2, 0.8) and an empty range gives exactly 0.0 - in both
    arithmetics.  The restatement's figures are printed; the largest must be below the ceiling 1e-6.  The real 128-filter banks at 16 kHz:
    none empty, one-bin filters at n_fft = 512."""
    for n_mel in R.MEL_COUNTS:
        c = R.mel_case(n_mel)
        lens = set((c["rng"][:, 1] - c["rng"][:, 0]).tolist())
        assert lens == ({0, 1, 2, 3, 4, 7, 257} if n_mel >= 7 else {1})     # (a single filter: one bin)
        ref, r32 = R.mel_stage(c["mag"], c["fb"], c["rng"]), R.mel_stage(c["mag"], c["fb"], c["rng"], dtype=np.float32)
        assert (ref[:, c["empty"]] == 0.0).all() and (r32[:, c["empty"]] == 0.0).all()
        assert (ref[:, ~c["empty"]] > 0.2).all() and (ref[:, ~c["empty"]] < 0.8).all()
        print("stft_ref mel stage fp32 restatement: n_mel %3d: %.3e on the [0, 1] scale" % (n_mel, np.abs(r32 - ref).max()))
    sym = R.mel_stage(R.mel_case(128)["mag"], R.mel_case(128)["fb"], R.mel_case(128)["rng"], 4.0)
    assert (sym[:, R.mel_case(128)["empty"]] == -4.0).all() and np.abs(sym).max() < 4.0 + 1e-12
    print("stft_ref mel stage: largest restatement figure of the table %.3e" % R.mel_table())
    assert R.mel_table() < R.CEIL_MEL
    for n_fft in (2048, 512):
        c = R.wrapper_mel_case(n_fft)
        fb = Audio.mel_filterbank(16000, n_fft, 128)
        assert np.array_equal(R.filter_ranges(fb.astype(np.float32))[:, 1] - R.filter_ranges(fb.astype(np.float32))[:, 0], c["widths"])
        assert c["widths"].min() >= 1 and (c["widths"].min() == 1) == (n_fft == 512)
        assert c["ref"].shape[1] == 128 and 3 <= c["ref"].shape[0] <= 20 and c["ref"].min() > 0.0 and c["ref"].max() < 1.0
        print("stft_ref real mel bank through the frame, fp32 restatement: n_fft %4d (%d frames, narrowest filter %d bins): %.3e on the [0, 1] scale"
              % (n_fft, c["ref"].shape[0], c["widths"].min(), c["e32"]))
