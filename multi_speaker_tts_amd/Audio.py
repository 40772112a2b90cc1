"""Drop-in for the reference's ``Audio.melspectrogram`` (Audio.py:29-32) on the MI355X.

Host side only prepares constants (windowed DFT basis, Slaney mel filterbank - both functions of
the hyper parameters, built once in float64 and cached on the device); the waveform -> mel
computation itself is ``mstts_stft_mel`` in libmstts_hip.so.
"""
from __future__ import annotations

import ctypes
import functools
from typing import Callable, NamedTuple

import numpy as np
import torch

from . import lib


def _stft_parameters(num_freq, frame_shift_ms, frame_length_ms, sample_rate):
    return (num_freq - 1) * 2, int(frame_shift_ms / 1000 * sample_rate), int(frame_length_ms / 1000 * sample_rate)


def _slaney_mel_to_hz(m):
    f_sp, min_hz = 200.0 / 3, 1000.0
    min_mel, step = min_hz / f_sp, np.log(6.4) / 27.0
    m = np.asarray(m, np.float64)
    return np.where(m >= min_mel, min_hz * np.exp(step * (m - min_mel)), f_sp * m)


def _slaney_hz_to_mel(f):
    f_sp, min_hz = 200.0 / 3, 1000.0
    min_mel, step = min_hz / f_sp, np.log(6.4) / 27.0
    f = np.asarray(f, np.float64)
    return np.where(f >= min_hz, min_mel + np.log(np.maximum(f, 1e-10) / min_hz) / step, f / f_sp)


def mel_filterbank(sample_rate, n_fft, n_mels):
    """Triangular Slaney-scale filters with area normalisation: what ``librosa.filters.mel(sr,
    n_fft, n_mels)`` returns with its defaults (the call at Audio.py:84)."""
    freqs = np.linspace(0, sample_rate / 2.0, 1 + n_fft // 2)
    edges = _slaney_mel_to_hz(np.linspace(_slaney_hz_to_mel(0.0), _slaney_hz_to_mel(sample_rate / 2.0), n_mels + 2))
    fb = np.zeros((n_mels, 1 + n_fft // 2))
    for i in range(n_mels):
        lo, ce, hi = edges[i], edges[i + 1], edges[i + 2]
        up = (freqs - lo) / (ce - lo)
        down = (hi - freqs) / (hi - ce)
        fb[i] = np.maximum(0.0, np.minimum(up, down)) * (2.0 / (hi - lo))
    return fb


@functools.lru_cache(maxsize=8)
def _constants(num_freq, frame_shift_ms, frame_length_ms, num_mels, sample_rate, device):
    n_fft, hop, win = _stft_parameters(num_freq, frame_shift_ms, frame_length_ms, sample_rate)
    nb = (n_fft // 2 + 1 + 3) // 4 * 4
    off = (n_fft - win) // 2                      # the Hann window sits centred in the n_fft frame
    n = np.arange(win)
    hann = 0.5 - 0.5 * np.cos(2 * np.pi * n / win)
    ang = 2 * np.pi * np.outer(n + off, np.arange(n_fft // 2 + 1)) / n_fft
    basis = np.zeros((win, 2 * nb))
    basis[:, : n_fft // 2 + 1] = hann[:, None] * np.cos(ang)
    basis[:, nb: nb + n_fft // 2 + 1] = -hann[:, None] * np.sin(ang)
    fb_t = np.zeros((nb, num_mels))
    fb_t[: n_fft // 2 + 1] = mel_filterbank(sample_rate, n_fft, num_mels).T
    dev = torch.device(device)
    return (n_fft, hop, win, nb, torch.tensor(basis, dtype=torch.float32, device=dev),
            torch.tensor(fb_t, dtype=torch.float32, device=dev))


def _fft_tables(n_fft, win):
    """The window and twiddle tables of `_fft_constants` for a transform given in samples, float64: the periodic Hann window [win] and
    (cos, -sin)(2 pi k / n_fft) [n_fft, 2]."""
    n = np.arange(win)
    hann = 0.5 - 0.5 * np.cos(2 * np.pi * n / win)
    k = np.arange(n_fft)
    tw = np.stack([np.cos(2 * np.pi * k / n_fft), -np.sin(2 * np.pi * k / n_fft)], axis=1)
    return hann, tw


@functools.lru_cache(maxsize=8)
def _fft_constants_samples(n_fft, win, device):
    """`_fft_constants` for callers that state the transform in samples (the denoiser: 256 samples at 22 050 Hz is no whole number of
    milliseconds, `_stft_parameters` would truncate it to 255) -> (hann, twiddle) on the device, the same fp64-built tables."""
    dev = torch.device(device)
    hann, tw = _fft_tables(n_fft, win)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)
    return t(hann), t(tw)


@functools.lru_cache(maxsize=8)
def _fft_constants(num_freq, frame_shift_ms, frame_length_ms, num_mels, sample_rate, device):
    """Tables of the one-launch FFT path (mstts_stft_fft): periodic Hann window, e^{-2 pi i k / n_fft} twiddles, the mel filterbank
    row-major with each filter's non-zero bin range - all built in float64."""
    n_fft, hop, win = _stft_parameters(num_freq, frame_shift_ms, frame_length_ms, sample_rate)
    dev = torch.device(device)
    hann, tw = _fft_tables(n_fft, win)
    fb = mel_filterbank(sample_rate, n_fft, num_mels).astype(np.float32)
    rng = np.zeros((num_mels, 2), np.int32)
    for c in range(num_mels):
        nz = np.nonzero(fb[c])[0]
        if len(nz):
            rng[c] = (nz[0], nz[-1] + 1)
    t = lambda a, dt: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    return n_fft, hop, win, t(hann, torch.float32), t(tw, torch.float32), t(fb, torch.float32), t(rng, torch.int32)


def stft_features(wavs, num_freq, frame_shift_ms, frame_length_ms, sample_rate, num_mels=None, max_abs_value=4, ref_level_db=20,
                  want_mel=True, want_spec=False, spectral_subtract=False, device="cuda"):
    """Mel and / or linear spectrogram features of SEVERAL waveforms in one kernel launch (mstts_stft_fft): returns a list of
    (mel [frames, num_mels] or None, spec [frames, num_freq] or None) device tensors, one pair per waveform.
    max_abs_value None: the mel is normalised to [0, 1] (Audio._normalize) instead of symmetrically.  spectral_subtract
    (Audio.py:45-46): a first launch leaves the raw magnitudes, a tenth of each waveform's per-bin time mean is subtracted
    (clipped at 0) by a second launch that finishes the features - three launches per waveform instead of one for the batch."""
    n_fft, hop, win, hann, tw, fb, rng = _fft_constants(num_freq, frame_shift_ms, frame_length_ms, num_mels or 1, sample_rate, str(device))
    dev = hann.device
    ws = [torch.as_tensor(np.asarray(y, dtype=np.float32)) if not torch.is_tensor(y) else y.to(torch.float32).reshape(-1) for y in wavs]
    lens = [int(w.numel()) for w in ws]
    if any(n <= n_fft // 2 for n in lens):
        raise ValueError("waveform shorter than the STFT's reflect padding (%d samples)" % (n_fft // 2))
    frames = [1 + n // hop for n in lens]
    woff = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64, device=dev)
    foff = torch.tensor(np.concatenate([[0], np.cumsum(frames)]), dtype=torch.int64, device=dev)
    cat = torch.cat([w.to(dev) for w in ws]).contiguous()
    return _stft_packed(cat, woff, foff, frames, (n_fft, hop, win, hann, tw, fb, rng), num_mels, max_abs_value, ref_level_db, want_mel, want_spec,
                        spectral_subtract)


def _stft_packed(cat, woff, foff, frames, consts, num_mels, max_abs_value, ref_level_db, want_mel, want_spec, spectral_subtract):
    """The launches of `stft_features` / `wav_features` on waveforms that already lie back to back on the device: cat = the samples,
    woff / foff = device int64 offset arrays of len(frames) + 1 entries, frames = the frame counts (host)."""
    n_fft, hop, win, hann, tw, fb, rng = consts
    dev = hann.device
    nw = len(frames)
    total, nb = int(sum(frames)), n_fft // 2 + 1
    mel = torch.empty(total, num_mels, dtype=torch.float32, device=dev) if want_mel else None
    spec = torch.empty(total, nb, dtype=torch.float32, device=dev) if want_spec else None
    flags = 1 if max_abs_value is None else 0
    mabs = float(max_abs_value) if max_abs_value is not None else 1.0
    common = (lib.ptr(fb) if want_mel else None, lib.ptr(rng) if want_mel else None, n_fft, hop, win, int(num_mels or 0), mabs, float(ref_level_db))
    if not spectral_subtract:
        lib.call("mstts_stft_fft", lib.ptr(cat), lib.ptr(woff), lib.ptr(foff), nw, 0.97, lib.ptr(hann), lib.ptr(tw), *common,
                 lib.ptr(mel) if want_mel else None, lib.ptr(spec) if want_spec else None, total, None, None, 0.0, flags)
    else:
        mag = torch.empty(total, nb, dtype=torch.float32, device=dev)
        lib.call("mstts_stft_fft", lib.ptr(cat), lib.ptr(woff), lib.ptr(foff), nw, 0.97, lib.ptr(hann), lib.ptr(tw), None, None,
                 n_fft, hop, win, 0, mabs, float(ref_level_db), None, lib.ptr(mag), total, None, None, 0.0, 2)
        sub = torch.empty(nb, dtype=torch.float32, device=dev)
        one = torch.tensor([0, 0], dtype=torch.int64, device=dev)
        f0 = 0
        for fr in frames:                                   # the mean runs over one waveform's frames
            lib.call("mstts_colsum", lib.ptr(mag, f0 * nb), fr, nb, nb, lib.ptr(sub), 0)
            lib.call("mstts_stft_fft", lib.ptr(cat), lib.ptr(one), lib.ptr(one), 1, 0.97, lib.ptr(hann), lib.ptr(tw), *common,
                     lib.ptr(mel, f0 * num_mels) if want_mel else None, lib.ptr(spec, f0 * nb) if want_spec else None, fr,
                     lib.ptr(mag, f0 * nb), lib.ptr(sub), 0.1 / fr, flags)
            f0 += fr
    out, f0 = [], 0
    for fr in frames:
        out.append((mel[f0:f0 + fr] if want_mel else None, spec[f0:f0 + fr] if want_spec else None))
        f0 += fr
    return out


def _fft_ok(num_freq, frame_shift_ms, frame_length_ms, sample_rate):
    n_fft, hop, win = _stft_parameters(num_freq, frame_shift_ms, frame_length_ms, sample_rate)
    return bool(lib.load().mstts_stft_fft_supported(n_fft, win))


def spectrogram(y, num_freq, frame_shift_ms, frame_length_ms, sample_rate, ref_level_db=20, spectral_subtract=False, device="cuda",
                return_tensor=False):
    """Audio.py:19-22: normalised linear spectrogram [num_freq, frames] in [0, 1]."""
    (_, spec), = stft_features([y], num_freq, frame_shift_ms, frame_length_ms, sample_rate, ref_level_db=ref_level_db, want_mel=False,
                               want_spec=True, spectral_subtract=spectral_subtract, device=device)
    spec = spec.t()
    return spec if return_tensor else spec.cpu().numpy()


def spectrogram_and_mel(y, num_freq, frame_shift_ms, frame_length_ms, sample_rate, spect_ref_level_db=20, num_mels=80, max_abs_mels=None,
                        spectral_subtract=False, device="cuda", return_tensor=False):
    """Audio.py:34-40: both features from one STFT -> (spectrogram [num_freq, frames], mel [num_mels, frames])."""
    (mel, spec), = stft_features([y], num_freq, frame_shift_ms, frame_length_ms, sample_rate, num_mels=num_mels, max_abs_value=max_abs_mels,
                                 ref_level_db=spect_ref_level_db, want_mel=True, want_spec=True, spectral_subtract=spectral_subtract,
                                 device=device)
    spec, mel = spec.t(), mel.t()
    return (spec, mel) if return_tensor else (spec.cpu().numpy(), mel.cpu().numpy())


def melspectrogram(y, num_freq, frame_shift_ms, frame_length_ms, num_mels, sample_rate, max_abs_value=None,
                   spectral_subtract=False, device="cuda", return_tensor=False, use_fft=True):
    """Same signature and result layout ([num_mels, frames]) as the reference function.  One launch (FFT in LDS) when n_fft is a
    power of two - the reference's 2048 is; the DFT-as-GEMM form below covers any other size (use_fft=False forces it)."""
    if (use_fft or spectral_subtract or max_abs_value is None) and _fft_ok(num_freq, frame_shift_ms, frame_length_ms, sample_rate):
        (mel, _), = stft_features([y], num_freq, frame_shift_ms, frame_length_ms, sample_rate, num_mels=num_mels, max_abs_value=max_abs_value,
                                  spectral_subtract=spectral_subtract, device=device)
        mel = mel.t()
        return mel if return_tensor else mel.cpu().numpy()
    if spectral_subtract or max_abs_value is None:
        raise ValueError("spectral_subtract / the [0, 1] normalisation need a power-of-two transform size (the one-launch FFT path)")
    n_fft, hop, win, nb, basis, fb_t = _constants(num_freq, frame_shift_ms, frame_length_ms, num_mels, sample_rate, str(device))
    wav = torch.as_tensor(np.asarray(y, dtype=np.float32)).to(basis.device) if not torch.is_tensor(y) else y.to(basis.device, torch.float32)
    wav = wav.contiguous()
    n = wav.numel()
    frames = 1 + n // hop
    L = lib.load()
    ws = torch.empty(int(L.mstts_stft_mel_ws_floats(n, n_fft, frames)), dtype=torch.float32, device=basis.device)
    out = torch.empty(frames, num_mels, dtype=torch.float32, device=basis.device)
    lib.call("mstts_stft_mel", lib.ptr(wav), n, 0.97, lib.ptr(basis), lib.ptr(fb_t), n_fft, hop, win, num_mels,
             float(max_abs_value), lib.ptr(ws), lib.ptr(out), frames)
    out = out.t()
    return out if return_tensor else out.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# Spectrogram -> waveform (Griffin-Lim), the export leg of Tacotron2.Inference with the Taco1 vocoder
# (Audio.py:15-27,50-60,84-99; Taco1_Mel_to_Spect/Modules.py:110-119; MSTTS_SV.py:403-412).  Host plumbing like in
# the reference (it runs in the export thread there; BASELINE config 1 calls it "plumbing, no GPU"): NumPy rFFTs.
# ---------------------------------------------------------------------------------------------------------------------
def _padded_window(n_fft, win_length):
    """librosa.util.pad_center(scipy.signal.get_window('hann', win_length, fftbins=True), n_fft)."""
    w = np.zeros(n_fft)
    lpad = (n_fft - win_length) // 2
    w[lpad:lpad + win_length] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win_length) / win_length)
    return w


def _stft(y, num_freq, frame_shift_ms, frame_length_ms, sample_rate):
    """librosa.stft(y, n_fft, hop_length, win_length): center=True, reflect padding -> [num_freq, 1 + len(y) // hop]."""
    n_fft, hop, win = _stft_parameters(num_freq, frame_shift_ms, frame_length_ms, sample_rate)
    w = _padded_window(n_fft, win)
    yp = np.pad(np.asarray(y, np.float64), n_fft // 2, mode="reflect")
    n_frames = 1 + (len(yp) - n_fft) // hop
    idx = np.arange(n_fft)[None, :] + hop * np.arange(n_frames)[:, None]
    return np.fft.rfft(yp[idx] * w[None, :], axis=1).T


def _istft(D, num_freq, frame_shift_ms, frame_length_ms, sample_rate):
    """librosa.istft(D, hop_length, win_length): windowed overlap-add of the inverse rFFTs, divided by the summed squared
    window where that is non-negligible, centre padding (n_fft // 2 each side) removed."""
    n_fft, hop, win = _stft_parameters(num_freq, frame_shift_ms, frame_length_ms, sample_rate)
    w = _padded_window(n_fft, win)
    n_frames = D.shape[1]
    frames = np.fft.irfft(D.T, n=n_fft, axis=1) * w[None, :]
    n = n_fft + hop * (n_frames - 1)
    y, wss = np.zeros(n), np.zeros(n)
    for i in range(n_frames):
        y[i * hop:i * hop + n_fft] += frames[i]
        wss[i * hop:i * hop + n_fft] += w * w
    nz = wss > np.finfo(np.float32).tiny
    y[nz] /= wss[nz]
    return y[n_fft // 2:n - n_fft // 2]


def _stft_samples(y, n_fft, hop, win):
    """`_stft` with the transform given in samples -> [n_fft // 2 + 1, 1 + len(y) // hop] (the same arithmetic)."""
    w = _padded_window(n_fft, win)
    yp = np.pad(np.asarray(y, np.float64), n_fft // 2, mode="reflect")
    n_frames = 1 + (len(yp) - n_fft) // hop
    idx = np.arange(n_fft)[None, :] + hop * np.arange(n_frames)[:, None]
    return np.fft.rfft(yp[idx] * w[None, :], axis=1).T


def _istft_samples(D, n_fft, hop, win, length):
    """`_istft` with the transform given in samples and torch.istft's `length`: the first n_fft // 2 samples of the normalised overlap-add
    are dropped and exactly `length` samples kept (not the hop (frames - 1) of `_istft`)."""
    w = _padded_window(n_fft, win)
    n_frames = D.shape[1]
    frames = np.fft.irfft(D.T, n=n_fft, axis=1) * w[None, :]
    n = n_fft + hop * (n_frames - 1)
    if length + n_fft // 2 > n:
        raise ValueError("%d frames do not cover %d samples" % (n_frames, length))
    y, wss = np.zeros(n), np.zeros(n)
    for i in range(n_frames):
        y[i * hop:i * hop + n_fft] += frames[i]
        wss[i * hop:i * hop + n_fft] += w * w
    nz = wss > np.finfo(np.float32).tiny
    y[nz] /= wss[nz]
    return y[n_fft // 2:n_fft // 2 + length]


def spectral_denoise(x, bias, strength, n_fft=1024, hop=256, win=1024):
    """The WaveGlow denoiser in float64, the checker of `spectral_denoise_batch`: strength * bias [n_fft // 2 + 1] is subtracted from the
    magnitude of every STFT bin of x (clipped at 0), the phase kept ((1, 0) where a bin is 0), and the result transformed back to
    len(x) samples.  librosa's conventions as `_stft`; x needs more than n_fft // 2 samples (the reflect padding)."""
    x = np.asarray(x, np.float64).reshape(-1)
    bias = np.asarray(bias, np.float64).reshape(-1)
    if x.shape[0] <= n_fft // 2:
        raise ValueError("waveform of %d samples is shorter than the STFT's reflect padding (%d samples)" % (x.shape[0], n_fft // 2))
    if bias.shape[0] != n_fft // 2 + 1 or (bias < 0).any():
        raise ValueError("bias must hold %d non-negative magnitudes" % (n_fft // 2 + 1))
    if not strength >= 0:
        raise ValueError("denoiser strength must not be negative (%r)" % (strength,))
    X = _stft_samples(x, n_fft, hop, win)
    mag = np.abs(X)
    direction = np.where(mag > 0, X / np.where(mag > 0, mag, 1.0), 1.0)
    Y = np.maximum(mag - float(strength) * bias[:, None], 0.0) * direction
    return _istft_samples(Y, n_fft, hop, win, x.shape[0])


def spectral_denoise_supported(n_fft, hop, win):
    """Does the device path cover this transform (mstts_wg_denoise_supported: a power-of-two n_fft in [512, 4096], win <= n_fft,
    2 hop <= win <= 4 hop)?"""
    return bool(lib.load().mstts_wg_denoise_supported(int(n_fft), int(hop), int(win)))


def spectral_denoise_batch(wavs, bias, strength, n_fft=1024, hop=256, win=1024, device="cuda", return_tensor=False):
    """`spectral_denoise` for several waveforms in ONE device call (mstts_wg_denoise: two launches for the whole batch, fp32).  wavs: list
    of arrays or device tensors; bias: [n_fft // 2 + 1] array or device tensor (WaveGlowEngine.bias_spectrum) -> list of float32
    waveforms of the same lengths (NumPy, or device tensors with return_tensor).  A transform outside the device envelope
    (`spectral_denoise_supported`) goes through the host function waveform by waveform; a waveform of n_fft // 2 samples or fewer and a
    negative strength are errors on both."""
    if not len(wavs):
        return []
    if not float(strength) >= 0:
        raise ValueError("denoiser strength must not be negative (%r)" % (strength,))
    lens = [int(w.numel()) if torch.is_tensor(w) else int(np.asarray(w).size) for w in wavs]
    for i, n in enumerate(lens):
        if n <= n_fft // 2:
            raise ValueError("waveform %d: %d samples, shorter than the STFT's reflect padding (%d samples)" % (i, n, n_fft // 2))
    if not spectral_denoise_supported(n_fft, hop, win):
        b = bias.detach().cpu().numpy() if torch.is_tensor(bias) else bias
        out = []
        for w in wavs:
            w = w.detach().cpu().numpy() if torch.is_tensor(w) else w
            y = spectral_denoise(w, b, strength, n_fft, hop, win).astype(np.float32)
            out.append(torch.as_tensor(y).to(device) if return_tensor else y)
        return out
    hann, tw = _fft_constants_samples(int(n_fft), int(win), str(device))
    dev = hann.device
    up = lambda a: (a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a, np.float32))).to(dev, torch.float32).reshape(-1)
    cat = torch.cat([up(w) for w in wavs]).contiguous()
    return _denoise_packed(cat, lens, up(bias).contiguous(), strength, n_fft, hop, win, hann, tw, return_tensor)


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64).reshape(-1))]).astype(np.int64)


def _packed_offsets(lens, frames, dev, host):
    """Layout of a packed batch, utterance i owning lens[i] samples and frames[i] frames -> (wav_off, frame_off, offs, host_off): the two
    int64 offset arrays of len(lens) + 1 entries, both on the device in one upload (offs [2, n + 1]: row 0 the samples), and the one named
    by `host` ("wav" or "frame") as the ctypes array the entry point checks every shape from before it launches anything."""
    wav_off, frame_off = _offsets(lens), _offsets(frames)
    return (wav_off, frame_off, torch.as_tensor(np.stack([wav_off, frame_off])).to(dev),
            (ctypes.c_int64 * (len(lens) + 1))(*(wav_off if host == "wav" else frame_off).tolist()))


def _cut_packed(packed, off, return_tensor):
    """The per-utterance list of a packed device result: views of it with return_tensor, else NumPy copies of one read-back (which
    synchronises: the call's inputs and workspace may go once it returns)."""
    if not return_tensor:
        packed = packed.cpu().numpy()
    parts = [packed[int(a):int(b)] for a, b in zip(off[:-1], off[1:])]
    return parts if return_tensor else [p.copy() for p in parts]


def _denoise_packed(cat, lens, bias, strength, n_fft, hop, win, hann, tw, return_tensor):
    """The device call of `spectral_denoise_batch` on waveforms of the lengths `lens` that already lie back to back in `cat`."""
    dev, nw = cat.device, len(lens)
    if bias.numel() != n_fft // 2 + 1:
        raise ValueError("bias must hold %d magnitudes" % (n_fft // 2 + 1))
    wav_off, frame_off, offs, host_off = _packed_offsets(lens, [1 + n // hop for n in lens], dev, "wav")
    ws = torch.empty(max(int(lib.load().mstts_wg_denoise_ws_floats(int(frame_off[-1]), win)), 1), dtype=torch.float32, device=dev)
    out = torch.empty_like(cat)
    lib.call("mstts_wg_denoise", lib.ptr(cat), host_off, lib.ptr(offs), lib.ptr(offs, nw + 1), nw, lib.ptr(bias), float(strength),
             lib.ptr(hann), lib.ptr(tw), int(n_fft), int(hop), int(win), lib.ptr(ws), lib.ptr(out))
    return _cut_packed(out, wav_off, return_tensor)


def inv_preemphasis(x, preemphasis=0.97):
    """scipy.signal.lfilter([1], [1, -preemphasis], x) (Audio.py:15-16)."""
    from scipy import signal
    return signal.lfilter([1], [1, -preemphasis], x)


def _denormalize(S, min_level_db=-100):
    return (np.clip(S, 0, 1) * -min_level_db) + min_level_db


def _db_to_amp(x):
    return np.power(10.0, x * 0.05)


def _griffin_lim(S, num_freq, frame_shift_ms, frame_length_ms, sample_rate, griffin_lim_iters=60, rng=None):
    """Audio.py:50-60: random initial phase, then `iters` rounds of istft -> stft -> keep the phase."""
    rng = rng if rng is not None else np.random
    angles = np.exp(2j * np.pi * rng.rand(*S.shape))
    S_complex = np.abs(S).astype(np.complex128)
    args = (num_freq, frame_shift_ms, frame_length_ms, sample_rate)
    y = _istft(S_complex * angles, *args)
    for _ in range(griffin_lim_iters):
        angles = np.exp(1j * np.angle(_stft(y, *args)))
        y = _istft(S_complex * angles, *args)
    return y


def inv_spectrogram(spectrogram, num_freq, frame_shift_ms, frame_length_ms, sample_rate, ref_level_db=20, power=1.5,
                    griffin_lim_iters=60, rng=None):
    """Same signature as the reference (Audio.py:24-27); spectrogram is [num_freq, frames], normalised to [0, 1]."""
    S = _db_to_amp(_denormalize(np.asarray(spectrogram, np.float64)) + ref_level_db)
    return inv_preemphasis(_griffin_lim(S ** power, num_freq, frame_shift_ms, frame_length_ms, sample_rate,
                                        griffin_lim_iters=griffin_lim_iters, rng=rng))


def Griffin_Lim(spectrogram, rng=None):
    """Taco1_Mel_to_Spect/Modules.py:110-119: spectrogram [Time, Dim] -> waveform at hp.Sound.Sample_Rate."""
    from . import Hyper_Parameters as hp
    return inv_spectrogram(np.asarray(spectrogram).transpose(), num_freq=hp.Sound.Spectrogram_Dim, frame_shift_ms=hp.Sound.Frame_Shift,
                           frame_length_ms=hp.Sound.Frame_Length, sample_rate=hp.Sound.Sample_Rate,
                           griffin_lim_iters=hp.Taco1_Mel_to_Spect.Griffin_Lim_Iteration, rng=rng)


# ---------------------------------------------------------------------------------------------------------------------
# The same algorithm on the GPU for a whole batch (mstts_griffin_lim, csrc/griffin_lim.hip): fp32, one launch per iteration for all
# utterances.  The host functions above stay what they are and are its checker.
# ---------------------------------------------------------------------------------------------------------------------
def griffin_lim_offsets(frames, hop):
    """Layout of the batched call: (frame_off, wav_off) int64 arrays of len(frames) + 1 entries.  Utterance i owns the frames
    frame_off[i] .. frame_off[i + 1] of the concatenated spectrograms and, T_i frames giving hop (T_i - 1) samples (istft with the
    centre padding removed), the samples wav_off[i] .. wav_off[i + 1] of the concatenated waveforms."""
    frames = np.asarray(frames, np.int64).reshape(-1)
    return _offsets(frames), _offsets(hop * np.maximum(frames - 1, 0))


def griffin_lim_phases(frames, num_freq, rng):
    """The initial-phase uniforms of a batch, drawn utterance by utterance in list order exactly as the host path draws them
    (`_griffin_lim`: rng.rand(num_freq, frames) per call) -> list of float64 arrays [num_freq, frames_i]."""
    return [rng.rand(num_freq, int(t)) for t in frames]


def griffin_lim_supported(num_freq, frame_shift_ms, frame_length_ms, sample_rate, frames=None):
    """Does the device path cover these STFT parameters (a power-of-two n_fft in [512, 4096], hop <= win <= 4 hop) and, when given,
    utterances of these frame counts (two frames and two samples at least)?"""
    n_fft, hop, win = _stft_parameters(num_freq, frame_shift_ms, frame_length_ms, sample_rate)
    if not lib.load().mstts_griffin_lim_supported(n_fft, hop, win):
        return False
    return frames is None or all(int(t) >= 2 and hop * (int(t) - 1) >= 2 for t in frames)


class _FixedPhase:
    """`rng` of the host path that hands out given uniforms."""

    def __init__(self, u):
        self.u = np.asarray(u, np.float64)

    def rand(self, *shape):
        assert tuple(shape) == self.u.shape, (shape, self.u.shape)
        return self.u


def griffin_lim_batch(spectrograms, num_freq, frame_shift_ms, frame_length_ms, sample_rate, ref_level_db=20, power=1.5,
                      griffin_lim_iters=60, phase=None, rng=None, seed=0, device="cuda", return_tensor=False):
    """`inv_spectrogram` for several utterances at once on the GPU.  spectrograms: list of [frames_i, num_freq] arrays or device
    tensors normalised to [0, 1] (the layout Inference returns and `Griffin_Lim` takes) -> list of float32 waveforms of
    hop (frames_i - 1) samples (NumPy, or device tensors with return_tensor).

    Initial phase e^{2 pi i u}: `phase` = the uniforms themselves, one [num_freq, frames_i] array per utterance as the host draws
    them; else `rng` = a NumPy RandomState, drawn per utterance in list order exactly as the host path would; else a device generator:
    utterance i uses seed + i (`seed` an int) or seed[i] (a sequence) - the same seed gives the same bits, alone or in any batch.
    STFT parameters outside the device envelope (`griffin_lim_supported`) go through the host path utterance by utterance; an
    utterance of fewer than two frames is an error on both."""
    frames = [int(s.shape[0]) for s in spectrograms]
    if any(tuple(s.shape) != (t, num_freq) for s, t in zip(spectrograms, frames)):
        raise ValueError("spectrograms must be [frames, %d]" % num_freq)
    n_fft, hop, win = _stft_parameters(num_freq, frame_shift_ms, frame_length_ms, sample_rate)
    if any(t < 2 or hop * (t - 1) < 2 for t in frames):
        raise ValueError("a spectrogram of fewer than two frames has no waveform")
    nu = len(frames)
    if nu == 0:
        return []
    if phase is not None and (len(phase) != nu or any(tuple(u.shape) != (num_freq, t) for u, t in zip(phase, frames))):
        raise ValueError("phase must hold one [num_freq, frames] array per utterance")
    if phase is None and rng is not None:
        phase = griffin_lim_phases(frames, num_freq, rng)
    seeds = [int(seed) + i for i in range(nu)] if np.isscalar(seed) else [int(s) for s in seed]
    if len(seeds) != nu:
        raise ValueError("seed must be an int or one int per utterance")
    if not griffin_lim_supported(num_freq, frame_shift_ms, frame_length_ms, sample_rate):
        out = []
        for i, s in enumerate(spectrograms):
            s = s.detach().cpu().numpy() if torch.is_tensor(s) else np.asarray(s)
            u = phase[i].detach().cpu().numpy() if phase is not None and torch.is_tensor(phase[i]) else (phase[i] if phase is not None else None)
            r = _FixedPhase(u) if u is not None else np.random.RandomState(seeds[i] % (1 << 32))
            y = inv_spectrogram(s.T, num_freq, frame_shift_ms, frame_length_ms, sample_rate, ref_level_db=ref_level_db, power=power,
                                griffin_lim_iters=griffin_lim_iters, rng=r).astype(np.float32)
            out.append(torch.as_tensor(y).to(device) if return_tensor else y)
        return out
    _, _, _, hann, tw, _, _ = _fft_constants(num_freq, frame_shift_ms, frame_length_ms, 1, sample_rate, str(device))
    dev = hann.device
    up = lambda a: (a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a, np.float32))).to(dev, torch.float32)
    spec = torch.cat([up(s) for s in spectrograms]).contiguous()
    u = torch.cat([up(p).t() for p in phase]).contiguous() if phase is not None else None
    wav_off, frame_off, offs, host_off = _packed_offsets([hop * (t - 1) for t in frames], frames, dev, "frame")       # = griffin_lim_offsets
    sd = torch.as_tensor(np.asarray([s % (1 << 64) for s in seeds], np.uint64).view(np.int64)).to(dev) if u is None else None
    ws = torch.empty(int(lib.load().mstts_griffin_lim_ws_floats(int(frame_off[-1]), n_fft, win)), dtype=torch.float32, device=dev)
    wav = torch.empty(int(wav_off[-1]), dtype=torch.float32, device=dev)
    lib.call("mstts_griffin_lim", lib.ptr(spec), lib.ptr(u), lib.ptr(sd), host_off, lib.ptr(offs, nu + 1), nu, lib.ptr(hann), lib.ptr(tw), n_fft,
             hop, win, float(power), float(ref_level_db), 0.97, int(griffin_lim_iters), lib.ptr(ws), lib.ptr(wav))
    return _cut_packed(wav, wav_off, return_tensor)


def Griffin_Lim_Batch(spectrograms, phase=None, rng=None, seed=0, device="cuda", return_tensor=False):
    """`Griffin_Lim` for a list of [Time, Dim] spectrograms in one device call, hp defaults (power 1.5, ref_level_db 20,
    hp.Taco1_Mel_to_Spect.Griffin_Lim_Iteration iterations) -> list of float32 waveforms at hp.Sound.Sample_Rate."""
    from . import Hyper_Parameters as hp
    return griffin_lim_batch(spectrograms, num_freq=hp.Sound.Spectrogram_Dim, frame_shift_ms=hp.Sound.Frame_Shift,
                             frame_length_ms=hp.Sound.Frame_Length, sample_rate=hp.Sound.Sample_Rate,
                             griffin_lim_iters=hp.Taco1_Mel_to_Spect.Griffin_Lim_Iteration, phase=phase, rng=rng, seed=seed, device=device,
                             return_tensor=return_tensor)


# ---------------------------------------------------------------------------------------------------------------------
# Waveform front end on the GPU (csrc/wav_front_end.hip): what Feeder.load_wav does to decoded samples - polyphase rate conversion
# (scipy.signal.resample_poly's arithmetic), the frame-RMS silence trim, the 0.99 scale - for a batch of waveforms, packed so that
# the result feeds mstts_stft_fft without a copy back.  Feeder.load_wav stays what it is and is the checker.  rule="librosa" selects
# the second rule set (kaiser_best, centred trim) in every function that takes `rule`: what the two differ in is the table `_rule` reads.
# ---------------------------------------------------------------------------------------------------------------------
def resample_ratio(rate, sample_rate):
    """(up, down) of a conversion rate -> sample_rate in lowest terms, as load_wav forms them."""
    g = int(np.gcd(int(rate), int(sample_rate)))
    return int(sample_rate) // g, int(rate) // g


def resample_out_len(n, up, down):
    """Samples resample_poly(x, up, down) returns for len(x) = n: ceil(n up / down)."""
    return -(-int(n) * int(up) // int(down))


def resample_filter(up, down):
    """The filter resample_poly designs at its defaults, float64: up * firwin(2 half + 1, 1 / max(up, down), window=('kaiser', 5.0)) with
    half = 10 max(up, down) - a Kaiser-windowed sinc, centred on tap `half`."""
    from scipy.signal import firwin
    mx = max(int(up), int(down))
    return int(up) * firwin(20 * mx + 1, 1.0 / mx, window=("kaiser", 5.0))


def resample_taps(up, down):
    """Taps per output sample in the phase layout: ceil((2 half + 1) / up), made odd (mstts_wav_resample_taps)."""
    return (-(-(20 * max(int(up), int(down)) + 1) // int(up))) | 1


def resample_phase_table(up, down):
    """The filter laid out by phase, float64 [up, T]: table[p, i] = h[p + (T - 1 - i) up] (0 beyond the filter).  With q = half + m down,
    output m is  sum_i table[q % up, i] * x[q // up - (T - 1) + i]  (x = 0 outside the signal): one row against a contiguous run of
    the input, in ascending sample order."""
    up, down = int(up), int(down)
    h = resample_filter(up, down)
    T = resample_taps(up, down)
    idx = np.arange(up)[:, None] + (T - 1 - np.arange(T))[None, :] * up
    table = np.zeros((up, T))
    ok = idx < h.shape[0]
    table[ok] = h[idx[ok]]
    return table


def resample_supported(up, down):
    return int(up) >= 1 and int(down) >= 1 and bool(lib.load().mstts_wav_resample_supported(int(up), int(down)))


# --- the second rule set, rule = "librosa": librosa.core.load (resampy 0.2.x's kaiser_best) and librosa.effects.trim, restated from the
# published algorithms in float64 (parity with the packages is unpinned).  The host functions are the checkers of the
# device path under that rule.
KAISER_BEST = dict(num_zeros=64, precision=9, rolloff=0.9475937167399596, beta=14.769656459379492)


def wav_rule(rule=None):
    """Feeder.wav_rule: "scipy" or "librosa" - the argument, else the environment variable MSTTS_WAV_RULE, else "scipy"."""
    from .Feeder import wav_rule as _wav_rule
    return _wav_rule(rule)


@functools.lru_cache(maxsize=1)
def kaiser_best_window():
    """resampy's sinc_window at the kaiser_best settings -> (W, D): the right half of a Kaiser(14.77)-windowed sinc with 64 zero
    crossings at 512 samples per crossing (32 769 entries, W[0] = rolloff) and its forward differences (D[-1] = 0), float64."""
    P, Z = 2 ** KAISER_BEST["precision"], KAISER_BEST["num_zeros"]
    N = P * Z
    W = np.kaiser(2 * N + 1, KAISER_BEST["beta"])[N:] * KAISER_BEST["rolloff"] * np.sinc(KAISER_BEST["rolloff"] * np.linspace(0, Z, N + 1))
    D = np.zeros_like(W)
    D[:-1] = np.diff(W)
    W.setflags(write=False)
    D.setflags(write=False)
    return W, D


def kaiser_best_step(up, down):
    """(scale, step, L): scale = min(1, up / down), step = int(scale 512) - TRUNCATED, as resampy does - and the taps per wing
    L = 32768 // step + 1.  step = 0 (a ratio below 1 / 512) raises ValueError: resampy cannot convert it either."""
    scale = min(1.0, float(up) / down)
    step = int(scale * 2 ** KAISER_BEST["precision"])
    if step < 1:
        raise ValueError("kaiser_best cannot convert %d / %d: the filter step truncates to 0" % (up, down))
    return scale, step, 32768 // step + 1


def kaiser_best_table(up, down):
    """resampy's resample_f at the exact time positions t down / up, as a polyphase table, float64 [up, 2 L]: output t with q = t down,
    n0 = q // up, r = q % up is  sum_i table[r, i] x[n0 - L + 1 + i]  (x = 0 outside the signal).  Column L - 1 - i holds the left-wing
    weight W[off + i step] + eta D[off + i step] of x[n0 - i] (off + eta = scale (r / up) 512), column L + k the right-wing weight of
    x[n0 + 1 + k] (off + eta = (scale - scale (r / up)) 512); W and D are scaled by up / down when that is below 1."""
    up, down = int(up), int(down)
    W, D = kaiser_best_window()
    ratio = float(up) / down
    if ratio < 1:
        W, D = W * ratio, D * ratio
    scale, step, L = kaiser_best_step(up, down)
    P, nwin = 2 ** KAISER_BEST["precision"], W.shape[0]
    table = np.zeros((up, 2 * L))
    for r in range(up):
        frac = scale * (float(r) / up)
        for wing, f in ((0, frac), (1, scale - frac)):
            pos = f * P
            off = int(pos)
            eta = pos - off
            idx = off + step * np.arange((nwin - off) // step)
            w = W[idx] + eta * D[idx]
            if wing == 0:
                table[r, L - 1 - np.arange(idx.shape[0])] = w
            else:
                table[r, L + np.arange(idx.shape[0])] = w
    return table


def kaiser_best_out_len(n, up, down):
    """(n_valid, n_out) for n input samples: resampy computes int(n ratio) samples, librosa's fix_length pads with zeros to
    int(ceil(n ratio)); ratio = float(up) / down, evaluated in doubles exactly as the packages do."""
    ratio = float(up) / down
    return int(n * ratio), int(np.ceil(n * ratio))


@functools.lru_cache(maxsize=8)
def _kaiser_best_table_cached(up, down):
    t = kaiser_best_table(up, down)
    t.setflags(write=False)
    return t


def resample_kaiser_best(x, up, down):
    """librosa.core.resample(x, res_type="kaiser_best") by the table form, float64 in and out: n_out samples, the last
    n_out - n_valid of them zero.  One matrix product per table row over the outputs that share it."""
    up, down = int(up), int(down)
    x = np.asarray(x, np.float64).reshape(-1)
    n = x.shape[0]
    n_valid, n_out = kaiser_best_out_len(n, up, down)
    y = np.zeros(n_out)
    if n_valid == 0:
        return y
    table = _kaiser_best_table_cached(up, down)
    L = table.shape[1] // 2
    q = np.arange(n_valid, dtype=np.int64) * down
    n0, r = q // up, q % up
    xp = np.concatenate([np.zeros(L - 1), x, np.zeros(L + 1 + max(0, int(n0[-1]) - (n - 1)))])       # xp[j + L - 1] = x[j]
    win = np.lib.stride_tricks.sliding_window_view(xp, 2 * L)                                      # win[n0] = x[n0 - L + 1 .. n0 + L]
    order = np.argsort(r, kind="stable")
    cuts = np.searchsorted(r[order], np.arange(up + 1))
    for row in range(up):
        t = order[cuts[row]:cuts[row + 1]]
        for a in range(0, t.shape[0], 16384):                                                  # (bounds the gathered windows: 16384 x 2 L doubles)
            y[t[a:a + 16384]] = win[n0[t[a:a + 16384]]] @ table[row]
    return y


def trim_bounds_centred(x, top_db=15.0, frame=2048, hop=512):
    """librosa.effects.trim's kept range (start, end) in float64: frames of `frame` samples centred on i hop (x[i hop - pad, i hop - pad
    + frame), pad = frame // 2, reflect-indexed outside the signal), i < 1 + (n + 2 pad - frame) // hop, kept when
    10 log10(max(1e-10, mse_i)) - 10 log10(max(1e-10, max mse)) > -top_db -> (first hop, min(n, (last + 1) hop)); (0, 0) when no frame
    is kept.  An all-zero signal keeps everything (every frame sits at 0 dB).  Our own choices: n = 0 gives (0, 0), and 0 < n <= pad - where
    nothing can be reflected and librosa's answer depends on the NumPy version - keeps the whole signal."""
    x = np.asarray(x, np.float64).reshape(-1)
    n, pad = x.shape[0], int(frame) // 2
    if n == 0:
        return 0, 0
    if n <= pad:
        return 0, n
    xp = np.pad(x, pad, mode="reflect")
    nf = 1 + (n + 2 * pad - frame) // hop
    mse = (np.lib.stride_tricks.sliding_window_view(xp, frame)[::hop][:nf] ** 2).mean(axis=1)
    db = 10.0 * np.log10(np.maximum(1e-10, mse)) - 10.0 * np.log10(max(1e-10, mse.max()))
    keep = np.nonzero(db > -top_db)[0]
    if not keep.size:
        return 0, 0
    return int(keep[0]) * hop, min(n, (int(keep[-1]) + 1) * hop)


def kaiser_best_supported(up, down):
    """The device resampler serves this ratio (mstts_wav_resample_fir_supported); otherwise the host path of the same rule is used."""
    try:
        L = kaiser_best_step(up, down)[2]
    except ValueError:
        return False
    return int(up) <= 4096 and int(down) <= 4096 and bool(lib.load().mstts_wav_resample_fir_supported(int(up), int(down), 2 * L))


def _pinned(array):
    """Host array -> page-locked tensor (what a non-blocking upload needs)."""
    a = torch.as_tensor(np.ascontiguousarray(array))
    p = torch.empty(a.shape, dtype=a.dtype, pin_memory=True)
    p.copy_(a)
    return p


def _upload(array, dtype, dev):
    """Host array -> device tensor of `dtype` through page-locked memory, enqueued on the current stream (no synchronisation)."""
    return _pinned(np.asarray(array, dtype={torch.float32: np.float32, torch.int64: np.int64}[dtype])).to(dev, non_blocking=True)


def _as_host_wav(y):
    if torch.is_tensor(y):
        y = y.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(y, dtype=np.float32).reshape(-1))


class _Rule(NamedTuple):
    """What one rule set of the front end is made of; everything else below is shared."""
    out_len: Callable        # (n, up, down) -> (n_valid, n_out): computed samples, samples returned (the rest are zeros)
    supported: Callable      # (up, down) -> the device resampler serves this ratio
    host: Callable           # (x, up, down) -> float32: the host converter, for ratios outside the device envelope
    table: Callable          # (up, down) -> (float64 phase table [up, taps], origin) of the device resampler
    valid: bool              # n_valid is uploaded, for mstts_wav_resample_fir; else every output is valid: mstts_wav_resample
    trim: str                # the trim entry's name


def _host_resample_poly(x, up, down):
    from scipy.signal import resample_poly
    return resample_poly(x, up, down).astype(np.float32)


_RULES = {
    "scipy": _Rule(out_len=lambda n, up, down: (resample_out_len(n, up, down),) * 2, supported=resample_supported, host=_host_resample_poly,
                   table=lambda up, down: (resample_phase_table(up, down), 10 * max(up, down)), valid=False, trim="mstts_wav_trim"),
    "librosa": _Rule(out_len=kaiser_best_out_len, supported=kaiser_best_supported,
                     host=lambda x, up, down: resample_kaiser_best(x, up, down).astype(np.float32),
                     table=lambda up, down: (_kaiser_best_table_cached(up, down), kaiser_best_step(up, down)[2] * up),
                     valid=True, trim="mstts_wav_trim_centred"),
}


def _rule(name):
    return _RULES[name]


@functools.lru_cache(maxsize=32)
def _device_table(rule, up, down, device):
    """(the rule's phase table on the device as float32, taps, origin)."""
    table, origin = _rule(rule).table(up, down)
    return _upload(table.astype(np.float32).reshape(-1), torch.float32, torch.device(device)), table.shape[1], origin


def _resample_groups(sigs, ups_downs, dev, rule="scipy", tiling=0):
    """Upload and rate-convert: sigs = float32 host arrays, ups_downs = (up, down) per signal, (1, 1) = as it is.  One upload of all
    samples, one of all offsets (and of the valid lengths, where the rule has them), one resample launch per distinct ratio.  Returns
    (buf, off, order, lens): the converted waveforms lie back to back in buf from off[0] on, in the order `order` (indices into sigs),
    off = device int64 [len + 1] absolute offsets into buf, lens = their lengths (host, in that order)."""
    r = _rule(rule)
    groups = {}
    for i, ud in enumerate(ups_downs):
        groups.setdefault(ud, []).append(i)
    plain = groups.pop((1, 1), [])
    order = plain + [i for ud in groups for i in groups[ud]]
    raw_order = [i for ud in groups for i in groups[ud]] + plain            # the upload: raw groups first, then the signals that stay
    host = np.concatenate([sigs[i] for i in raw_order]) if raw_order else np.zeros(0, np.float32)
    raw_start = dict(zip(raw_order, np.concatenate([[0], np.cumsum([sigs[i].shape[0] for i in raw_order])]).tolist()))
    n_raw = int(host.shape[0])
    lens = [sigs[i].shape[0] if ups_downs[i] == (1, 1) else r.out_len(sigs[i].shape[0], *ups_downs[i])[1] for i in order]
    base = raw_start[plain[0]] if plain else n_raw                           # the converted set begins where the unchanged signals lie
    off_host = base + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    meta, launches, pos = [off_host], [], len(plain)
    cursor = off_host.shape[0]
    for ud, members in groups.items():
        in_off = np.asarray([raw_start[i] for i in members] + [raw_start[members[-1]] + sigs[members[-1]].shape[0]], np.int64)
        out_off = off_host[pos:pos + len(members) + 1]
        launches.append((ud, len(members), cursor, cursor + len(members) + 1, int(max(lens[pos:pos + len(members)]))))
        meta += [in_off, out_off]
        cursor += 2 * (len(members) + 1)
        if r.valid:
            meta.append(np.asarray([r.out_len(sigs[i].shape[0], *ud)[0] for i in members], np.int64))
            cursor += len(members)
        pos += len(members)
    buf = torch.empty(max(int(off_host[-1]), 1), dtype=torch.float32, device=dev)
    if n_raw:
        buf[:n_raw].copy_(_pinned(host), non_blocking=True)
    meta_dev = _upload(np.concatenate(meta), torch.int64, dev)
    for (up, down), n, a, b, longest in launches:
        table, taps, origin = _device_table(rule, up, down, str(dev))
        if r.valid:
            lib.call("mstts_wav_resample_fir", lib.ptr(buf), lib.ptr(meta_dev, a), lib.ptr(meta_dev, b), lib.ptr(meta_dev, b + n + 1), n, longest,
                     lib.ptr(table), up, down, taps, origin, int(tiling), lib.ptr(buf))
        else:                                                    # (the entry restates this rule's taps and origin)
            assert lib.load().mstts_wav_resample_taps(up, down) == taps and origin == 10 * max(up, down)
            lib.call("mstts_wav_resample", lib.ptr(buf), lib.ptr(meta_dev, a), lib.ptr(meta_dev, b), n, longest, lib.ptr(table), up, down, lib.ptr(buf))
    return buf, meta_dev[:len(order) + 1], order, lens


def _resample_batch(rule, wavs, up, down, device, return_tensor, tiling=0):
    """A list of waveforms at one ratio (lowest terms) under `rule`: one launch, or the rule's host converter outside its device envelope."""
    sigs = [_as_host_wav(y) for y in wavs]
    if not sigs:
        return []
    dev = torch.device(device)
    if not _rule(rule).supported(up, down):
        out = [_rule(rule).host(s, up, down) for s in sigs]
        return [torch.as_tensor(o).to(dev) for o in out] if return_tensor else out
    buf, off, order, lens = _resample_groups(sigs, [(up, down)] * len(sigs), dev, rule, tiling)
    bounds = np.concatenate([[0], np.cumsum(lens)]) + (0 if (up, down) == (1, 1) else sum(s.shape[0] for s in sigs))
    res = buf if return_tensor else buf.cpu().numpy()
    out = [None] * len(sigs)
    for k, i in enumerate(order):
        piece = res[int(bounds[k]):int(bounds[k + 1])]
        out[i] = piece if return_tensor else piece.copy()
    return out


def resample_poly_batch(wavs, up, down, device="cuda", return_tensor=False):
    """scipy.signal.resample_poly(x, up, down) for a list of waveforms in one launch (mstts_wav_resample), float32 ->
    list of ceil(len up / down)-sample waveforms.  Ratios outside the device envelope (`resample_supported`) take the host path."""
    g = int(np.gcd(int(up), int(down))) if up >= 1 and down >= 1 else 1
    return _resample_batch("scipy", wavs, int(up) // g, int(down) // g, device, return_tensor)


def resample_kaiser_best_batch(wavs, sr_orig, sr_new, device="cuda", return_tensor=False, tiling=0):
    """librosa.core.resample(x, sr_orig, sr_new) at res_type="kaiser_best" for a list of waveforms in one launch
    (mstts_wav_resample_fir), float32 -> list of int(ceil(len ratio))-sample waveforms whose last sample is zero where resampy computes
    one fewer.  Ratios outside the device envelope (`kaiser_best_supported`) take the host path of the same rule.  tiling: 0 = the
    library's choice, 1 = row-major, 2 = phase-major (both give the same bits)."""
    return _resample_batch("librosa", wavs, *resample_ratio(sr_orig, sr_new), device, return_tensor, tiling)


def _trim(buf, off, lens, top_db, frame, hop, rule="scipy"):
    """The rule's trim entry on waveforms of the (host-known) lengths `lens` at the device offsets `off` into buf -> device (bounds [nw, 2], peak [nw])."""
    nw, total = len(lens), int(sum(lens))
    bounds = torch.empty(nw, 2, dtype=torch.int64, device=buf.device)
    peak = torch.empty(nw, dtype=torch.float32, device=buf.device)
    name = _rule(rule).trim
    ws = torch.empty(max(int(getattr(lib.load(), name + "_ws_floats")(total, nw)), 1), dtype=torch.float32, device=buf.device)
    lib.call(name, lib.ptr(buf), lib.ptr(off), nw, total, int(max(lens)), int(frame), int(hop), float(top_db), lib.ptr(ws),
             lib.ptr(bounds), lib.ptr(peak))
    return bounds, peak


def trim_bounds_batch(wavs, top_db=15.0, frame=32, hop=16, device="cuda", rule=None):
    """The silence trim of Feeder.load_wav for a list of waveforms in one launch (mstts_wav_trim; rule "librosa": the centred trim,
    mstts_wav_trim_centred) -> (start, end, peak): int64 arrays of the kept range [start, end) of each waveform and float32 max |x|
    inside it."""
    rule = wav_rule(rule)
    sigs = [_as_host_wav(y) for y in wavs]
    dev = torch.device(device)
    nw = len(sigs)
    cat = _upload(np.concatenate(sigs), torch.float32, dev) if sum(s.shape[0] for s in sigs) else torch.zeros(1, dtype=torch.float32, device=dev)
    off = _upload(np.concatenate([[0], np.cumsum([s.shape[0] for s in sigs])]).astype(np.int64), torch.int64, dev)
    bounds, peak = _trim(cat, off, [s.shape[0] for s in sigs], top_db, frame, hop, rule)
    b = bounds.cpu().numpy()
    return b[:, 0].copy(), b[:, 1].copy(), peak.cpu().numpy()


def _front_end_packed(signals, rates, sample_rate, top_db, frame, hop, scale, peak_normalize, stft_hop, dev, rule="scipy"):
    """Everything of the front end up to (not including) the one host read: returns (packed, offs, order) - packed = the trimmed,
    scaled waveforms back to back, offs = device int64 [2, nw + 1] (sample offsets; frame offsets for an STFT of hop `stft_hop`),
    order = which input each packed waveform is."""
    sigs = [_as_host_wav(y) for y in signals]
    ratios = []
    for i, r in enumerate(rates):
        ud = resample_ratio(r, sample_rate) if int(r) != int(sample_rate) else (1, 1)
        if ud != (1, 1) and not _rule(rule).supported(*ud):           # outside the device envelope: the host path of the same rule
            sigs[i], ud = _rule(rule).host(sigs[i], *ud), (1, 1)
        ratios.append(ud)
    nw = len(sigs)
    buf, off, order, lens = _resample_groups(sigs, ratios, dev, rule)
    bounds, peak = _trim(buf, off, lens, top_db, frame, hop, rule)
    packed = torch.empty(max(sum(lens), 1), dtype=torch.float32, device=dev)
    offs = torch.empty(2, nw + 1, dtype=torch.int64, device=dev)
    lib.call("mstts_wav_gather_scale", lib.ptr(buf), lib.ptr(off), lib.ptr(bounds), lib.ptr(peak), nw, int(max(lens)), float(scale),
             int(bool(peak_normalize)), int(stft_hop), lib.ptr(packed), lib.ptr(offs), lib.ptr(offs, nw + 1))
    return packed, offs, order


def wav_front_end(signals, rates, sample_rate, top_db=15.0, frame=32, hop=16, scale=0.99, peak_normalize=False, device="cuda",
                  return_tensor=False, rule=None):
    """The trimmed, scaled waveforms Feeder.load_wav returns for the same decoded samples, for a batch: signals = float mono arrays,
    rates = their sample rates.  Signals of one source rate are converted in one launch, signals already at sample_rate skip it; one
    trim, one gather.  peak_normalize: scale / max |x| of the kept range instead of scale.  rule: "scipy" (resample_poly, uncentred RMS
    trim), "librosa" (kaiser_best, centred power trim) or None = `wav_rule`.  -> list of float32 waveforms."""
    rule = wav_rule(rule)
    if len(signals) != len(rates):
        raise ValueError("one sample rate per signal")
    if not len(signals):
        return []
    dev = torch.device(device)
    packed, offs, order = _front_end_packed(signals, rates, sample_rate, top_db, frame, hop, scale, peak_normalize, 1, dev, rule)
    o = offs[0].cpu().numpy()                                    # (the one host read: the lengths)
    res = packed if return_tensor else packed[:int(o[-1])].cpu().numpy()
    out = [None] * len(order)
    for k, i in enumerate(order):
        piece = res[int(o[k]):int(o[k + 1])]
        out[i] = piece if return_tensor else piece.copy()
    return out


def wav_features(signals, rates, num_freq, frame_shift_ms, frame_length_ms, sample_rate, num_mels=None, max_abs_value=4, ref_level_db=20,
                 want_mel=True, want_spec=False, spectral_subtract=False, top_db=15.0, frame=32, hop=16, scale=0.99, peak_normalize=False,
                 length_range=None, device="cuda", return_tensor=False, return_lengths=False, rule=None):
    """`wav_front_end` followed by the one-launch STFT (mstts_stft_fft) on the packed buffer, without a copy back: list of
    (mel [frames, num_mels] or None, spec [frames, num_freq] or None), the options of `stft_features`.  One host read (the trimmed
    lengths) lies between the upload and the feature launch.  A waveform whose trimmed length is not longer than n_fft / 2 raises the ValueError
    `stft_features` raises.  length_range = (lo, hi) in samples: a waveform whose trimmed length lies outside it gets (None, None) and
    no transform.  return_lengths: also the list of trimmed lengths in samples.  rule: as in `wav_front_end`."""
    rule = wav_rule(rule)
    if len(signals) != len(rates):
        raise ValueError("one sample rate per signal")
    if not len(signals):
        return ([], []) if return_lengths else []
    consts = _fft_constants(num_freq, frame_shift_ms, frame_length_ms, num_mels or 1, sample_rate, str(device))
    n_fft, stft_hop = consts[0], consts[1]
    dev = consts[3].device
    packed, offs, order = _front_end_packed(signals, rates, sample_rate, top_db, frame, hop, scale, peak_normalize, stft_hop, dev, rule)
    o = offs.cpu().numpy()                                       # (the one host read: sample and frame offsets)
    nw = len(order)
    lens, frames = [int(v) for v in np.diff(o[0])], [int(v) for v in np.diff(o[1])]
    keep = [length_range is None or length_range[0] <= n <= length_range[1] for n in lens]
    for k, i in enumerate(order):
        if keep[k] and lens[k] <= n_fft // 2:
            raise ValueError("waveform %d: %d samples after the trim, shorter than the STFT's reflect padding (%d samples)" % (i, lens[k], n_fft // 2))
    feats = [(None, None)] * nw
    args = (consts, num_mels, max_abs_value, ref_level_db, want_mel, want_spec, spectral_subtract)
    if all(keep):
        feats = _stft_packed(packed, offs[0], offs[1], frames, *args)
    else:                                                        # a launch per run of kept waveforms: the sample offsets are absolute, the frame offsets restart
        a = 0
        while a < nw:
            b = a
            while b < nw and keep[b] == keep[a]:
                b += 1
            if keep[a]:
                foff = _upload(np.concatenate([[0], np.cumsum(frames[a:b])]).astype(np.int64), torch.int64, dev)
                feats[a:b] = _stft_packed(packed, offs[0, a:b + 1], foff, frames[a:b], *args)
            a = b
    out, out_len = [None] * nw, [0] * nw
    for k, i in enumerate(order):
        m, s = feats[k]
        out[i] = (m, s) if return_tensor else (m.cpu().numpy() if m is not None else None, s.cpu().numpy() if s is not None else None)
        out_len[i] = lens[k]
    return (out, out_len) if return_lengths else out
