"""Batched Griffin-Lim (mstts_griffin_lim, Audio.griffin_lim_batch), the parts that need no GPU: the entry points exist in the header,
the library and the binding; the supported envelope; the layout helpers; and the host-side drawing of initial phases, which must be
exactly what the host path Audio.Griffin_Lim draws, because that is what makes the device path checkable against it."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mstts_griffin_lim_supported", "mstts_griffin_lim_ws_floats", "mstts_griffin_lim")


def test_entry_points_in_header_library_and_binding():
    from multi_speaker_tts_amd import build, lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mstts.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mstts_[a-z0-9_]+)\s*\(", text))
    cdll = ctypes.CDLL(build.build())
    for name in ENTRY_POINTS:
        assert name in declared and name in lib.SIGNATURES and hasattr(cdll, name), name
    assert lib.ABI_VERSION == 5 and lib.load().mstts_abi_version() == 5                    # additions only
    assert "griffin_lim.hip" in build.SOURCES


def test_supported_envelope():
    from multi_speaker_tts_amd import Audio, lib
    L = lib.load()
    assert L.mstts_griffin_lim_supported(2048, 200, 800) == 1                              # the reference's n_fft, hop, win
    assert L.mstts_griffin_lim_supported(2000, 200, 800) == 0                              # not a power of two
    assert L.mstts_griffin_lim_supported(2048, 199, 800) == 0                              # five frames over one sample: win > 4 hop
    assert L.mstts_griffin_lim_supported(2048, 900, 800) == 0                              # gaps between the windows
    assert L.mstts_griffin_lim_supported(256, 64, 256) == 0 and L.mstts_griffin_lim_supported(8192, 2048, 8192) == 0
    assert L.mstts_griffin_lim_supported(512, 128, 512) == 1 and L.mstts_griffin_lim_supported(4096, 1024, 2048) == 1
    assert L.mstts_griffin_lim_ws_floats(10, 2048, 800) == 10 * 1025 + 2 * 10 * 800
    args = (1025, 12.5, 50, 16000)
    assert Audio.griffin_lim_supported(*args) and Audio.griffin_lim_supported(*args, frames=[2, 401])
    assert not Audio.griffin_lim_supported(*args, frames=[401, 1])                         # the "too short" rule
    assert not Audio.griffin_lim_supported(1001, 12.5, 50, 16000)


def test_unsupported_shapes_are_refused_before_any_launch():
    """The C entry point checks parameters and every utterance's frame count on the host (frame_off_host) and returns an error code;
    the pointers are never used, so this runs without a GPU."""
    from multi_speaker_tts_amd import lib
    L = lib.load()
    one = ctypes.c_void_p(16)                                                              # never dereferenced
    def run(off, n_fft=2048, hop=200, win=800, iters=1):
        host = (ctypes.c_int64 * len(off))(*off)
        return L.mstts_griffin_lim(one, one, None, host, one, len(off) - 1, one, one, n_fft, hop, win, 1.5, 20.0, 0.97, iters, one, one, None)
    assert run([0, 5, 6]) == -1 and b"utterance 1" in L.mstts_last_error()                 # one frame
    assert run([0, 5], n_fft=2000) == -1 and run([0, 5], hop=100) == -1 and run([0, 5], iters=-1) == -1
    assert run([1, 5]) == -1


def test_offsets_give_hop_times_frames_minus_one_samples():
    from multi_speaker_tts_amd import Audio
    frames = [401, 2, 37, 120]
    foff, woff = Audio.griffin_lim_offsets(frames, 200)
    assert foff.dtype == np.int64 and woff.dtype == np.int64
    assert foff.tolist() == [0, 401, 403, 440, 560]
    assert np.diff(woff).tolist() == [200 * (t - 1) for t in frames] and woff[0] == 0
    assert all(woff[i] == 200 * (foff[i] - i) for i in range(5))                           # what the kernels derive from frame_off alone
    # the host path's own length rule
    args = (1025, 12.5, 50, 16000)
    D = np.ones((1025, 7), np.complex128)
    assert Audio._istft(D, *args).shape[0] == 200 * 6 and Audio._stft(Audio._istft(D, *args), *args).shape[1] == 7


class _Recorder:
    def __init__(self, rng):
        self.rng, self.drawn = rng, []

    def rand(self, *shape):
        self.drawn.append(self.rng.rand(*shape))
        return self.drawn[-1]


def test_rng_draws_what_the_host_path_draws(monkeypatch):
    from multi_speaker_tts_amd import Audio, Hyper_Parameters as hp
    monkeypatch.setattr(hp.Taco1_Mel_to_Spect, "Griffin_Lim_Iteration", 0)
    g = np.random.default_rng(0)
    frames = [9, 7, 12]
    specs = [g.uniform(0, 1, (t, hp.Sound.Spectrogram_Dim)).astype(np.float32) for t in frames]
    rec = _Recorder(np.random.RandomState(11))
    for s in specs:                                                                        # the host path, one utterance after the other
        Audio.Griffin_Lim(s, rng=rec)
    ours = Audio.griffin_lim_phases(frames, hp.Sound.Spectrogram_Dim, np.random.RandomState(11))
    assert len(ours) == len(rec.drawn) == 3
    for a, b, t in zip(ours, rec.drawn, frames):
        assert a.shape == (hp.Sound.Spectrogram_Dim, t) and np.array_equal(a, b)


def test_batch_argument_checks_and_host_path_outside_the_envelope():
    """n_fft = 2000 is outside the device envelope: griffin_lim_batch runs the host path and, given the same uniforms, returns what
    inv_spectrogram returns (float32).  Bad arguments raise before anything runs."""
    from multi_speaker_tts_amd import Audio
    args = (1001, 12.5, 50, 16000)
    g = np.random.default_rng(1)
    specs = [g.uniform(0.3, 0.9, (t, 1001)).astype(np.float32) for t in (8, 7)]
    u = Audio.griffin_lim_phases([8, 7], 1001, np.random.RandomState(2))
    got = Audio.griffin_lim_batch(specs, *args, griffin_lim_iters=2, phase=u, device="cpu")
    want = [Audio.inv_spectrogram(s.T, *args, griffin_lim_iters=2, rng=Audio._FixedPhase(p)) for s, p in zip(specs, u)]
    for a, b in zip(got, want):
        assert a.dtype == np.float32 and a.shape == (200 * (b.shape[0] // 200),) and np.array_equal(a, b.astype(np.float32))
    again = Audio.griffin_lim_batch(specs, *args, griffin_lim_iters=2, rng=np.random.RandomState(2), device="cpu")
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    with pytest.raises(ValueError):
        Audio.griffin_lim_batch([specs[0][:1]], *args)
    with pytest.raises(ValueError):
        Audio.griffin_lim_batch(specs, *args, phase=u[:1])
    with pytest.raises(ValueError):
        Audio.griffin_lim_batch(specs, *args, seed=[1])
    with pytest.raises(ValueError):
        Audio.griffin_lim_batch([specs[0][:, :5]], *args)
