"""The WaveGlow denoiser's fp64 statement (Audio.spectral_denoise and the in-samples helpers beside Audio._stft / _istft), pinned
against torch's stft / istft, a known-answer case, the strength's precedence and the new exports.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from multi_speaker_tts_amd import Audio
from multi_speaker_tts_amd import lib
from multi_speaker_tts_amd import waveglow as WG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = [(1024, 256, 1024), (512, 128, 512), (2048, 200, 800)]           # the last: a window shorter than n_fft
lengths = lambda n_fft, hop: (n_fft // 2 + 1, 37 * hop + 19, 121 * hop)


@pytest.mark.parametrize("n_fft,hop,win", PARAMS)
def test_transforms_are_torchs_stft_and_istft(n_fft, hop, win):
    """Audio._stft_samples / _istft_samples against torch.stft(center=True, pad_mode="reflect", periodic Hann) and torch.istft(length=n)
    in float64 to 1e-12 relative; spectral_denoise at strength 0 gives the input back to 1e-12 absolute.  Measured: 4.5e-16 or better, round trip 4.4e-16."""
    g = np.random.default_rng(n_fft + hop)
    window = torch.hann_window(win, periodic=True, dtype=torch.float64)
    for n in lengths(n_fft, hop):
        x = g.normal(0, 0.3, n)
        X = Audio._stft_samples(x, n_fft, hop, win)
        Xt = torch.stft(torch.tensor(x), n_fft, hop, win, window, center=True, pad_mode="reflect", return_complex=True)
        assert X.shape == (n_fft // 2 + 1, 1 + n // hop) == tuple(Xt.shape)
        e_fwd = float(np.abs(X - Xt.numpy()).max() / np.abs(Xt.numpy()).max())
        # an arbitrary spectrum, not one that came from a signal: the inverse is pinned on its own
        Y = X * g.uniform(0.2, 1.0, X.shape)
        y = Audio._istft_samples(Y, n_fft, hop, win, n)
        yt = torch.istft(torch.tensor(Y), n_fft, hop, win, window, center=True, length=n).numpy()
        assert y.shape == (n,) == yt.shape
        e_inv = float(np.abs(y - yt).max() / np.abs(yt).max())
        e_id = float(np.abs(Audio.spectral_denoise(x, np.zeros(n_fft // 2 + 1), 0.0, n_fft, hop, win) - x).max())
        e_id2 = float(np.abs(Audio.spectral_denoise(x, np.ones(n_fft // 2 + 1), 0.0, n_fft, hop, win) - x).max())
        print("wg_denoise host pin: n_fft %d hop %d win %d n %6d: stft %.2e istft %.2e (relative), strength 0 round trip %.2e / %.2e"
              % (n_fft, hop, win, n, e_fwd, e_inv, e_id, e_id2))
        assert e_fwd <= 1e-12 and e_inv <= 1e-12 and e_id <= 1e-12 and e_id2 <= 1e-12


def test_a_stationary_tone_on_an_exact_bin_is_removed():
    """0.3 sin(2 pi 64 j / 1024) over 60 hops, bias = |X_10| of the signal itself, strength 1: more than n_fft samples from either end at
    most 1e-9 of the amplitude remains (measured: 3.8e-13) - what the denoiser is for, as a known answer."""
    n_fft, hop, win = 1024, 256, 1024
    x = 0.3 * np.sin(2 * np.pi * 64 * np.arange(60 * hop) / 1024)
    bias = np.abs(Audio._stft_samples(x, n_fft, hop, win))[:, 10]
    y = Audio.spectral_denoise(x, bias, 1.0, n_fft, hop, win)
    assert y.shape == x.shape
    left = float(np.abs(y[n_fft + 1:-(n_fft + 1)]).max() / 0.3)
    print("wg_denoise host: stationary tone, remainder %.2e of the amplitude" % left)
    assert left <= 1e-9
    half = Audio.spectral_denoise(x, bias, 0.5, n_fft, hop, win)          # half the strength leaves half the tone
    assert abs(float(np.abs(half[n_fft + 1:-(n_fft + 1)]).max()) / 0.3 - 0.5) < 1e-3


def test_host_refusals():
    x = np.zeros(2000)
    with pytest.raises(ValueError, match="reflect padding"):
        Audio.spectral_denoise(np.zeros(512), np.zeros(513), 1.0)
    with pytest.raises(ValueError, match="negative"):
        Audio.spectral_denoise(x, np.zeros(513), -0.1)
    with pytest.raises(ValueError, match="513"):
        Audio.spectral_denoise(x, np.zeros(512), 1.0)
    assert np.array_equal(Audio.spectral_denoise(x, np.ones(513), 1.0), x)          # zero bins stay zero: max(0 - s b, 0) (1, 0) = 0


def test_resolve_denoise_precedence(monkeypatch):
    monkeypatch.delenv("MSTTS_WG_DENOISE", raising=False)
    assert WG.resolve_denoise(None) == 0.0 and WG.resolve_denoise(0.25) == 0.25 and WG.resolve_denoise(None, 0.5) == 0.5
    monkeypatch.setenv("MSTTS_WG_DENOISE", "0.125")
    assert WG.resolve_denoise(None) == 0.125
    assert WG.resolve_denoise(None, 0.5) == 0.5 and WG.resolve_denoise(0.0) == 0.0 and WG.resolve_denoise(0.25, 0.5) == 0.25
    monkeypatch.setenv("MSTTS_WG_DENOISE", "")
    assert WG.resolve_denoise(None) == 0.0
    for bad in ("-1", "loud", "nan", "inf"):
        monkeypatch.setenv("MSTTS_WG_DENOISE", bad)
        with pytest.raises(ValueError, match="MSTTS_WG_DENOISE"):
            WG.resolve_denoise(None)
    with pytest.raises(ValueError, match="strength"):
        WG.resolve_denoise(-0.5)


def test_new_exports_in_header_library_and_binding():
    names = ("mstts_wg_denoise_supported", "mstts_wg_denoise_ws_floats", "mstts_wg_denoise")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mstts.h")).read(), flags=re.S)
    L = lib.load()
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert n in lib.SIGNATURES and hasattr(L, n), n
    assert L.mstts_abi_version() == lib.ABI_VERSION == 5
    # the envelope and the workspace are host-only questions
    ok = lambda *a: bool(L.mstts_wg_denoise_supported(*a))
    assert ok(1024, 256, 1024) and ok(512, 128, 512) and ok(2048, 200, 800) and ok(4096, 1024, 4096) and ok(1024, 512, 1024)
    assert not ok(256, 64, 256) and not ok(1000, 250, 1000) and not ok(8192, 2048, 8192)          # n_fft: a power of two in [512, 4096]
    assert not ok(1024, 513, 1024) and not ok(1024, 255, 1024) and not ok(1024, 0, 1024) and not ok(1024, 256, 1025)
    assert L.mstts_wg_denoise_ws_floats(117, 800) == 117 * 800 and L.mstts_wg_denoise_ws_floats(0, 800) == 0
    assert "wg_denoise.hip" in __import__("multi_speaker_tts_amd.build", fromlist=["SOURCES"]).SOURCES


def test_denoiser_tables_are_the_fft_constants_tables():
    """`_fft_constants_samples` (the transform in samples) hands out the very tables `_fft_constants` (in milliseconds) builds."""
    n_fft, hop, win, hann, tw, _, _ = Audio._fft_constants(1025, 12.5, 50, 1, 16000, "cpu")
    assert (n_fft, hop, win) == (2048, 200, 800)
    h2, t2 = Audio._fft_constants_samples(2048, 800, "cpu")
    assert torch.equal(hann, h2) and torch.equal(tw, t2)
