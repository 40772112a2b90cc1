"""Evidence that a refactor of the STFT round-trip kernels changed no bit: run this file UNCHANGED in a checkout of the parent commit and in
the branch and compare the two outputs line by line (profiles/stft_parts_refactor_digests.txt is such a record).  Every line is the SHA-256
(first 16 hex digits) of one output from seeded inputs.  Tables come from Audio._fft_tables and the round-trip entry points are called
through lib.call, so their parameters are given in samples; only Audio.stft_features is used of the Python surface above them.

  mstts_griffin_lim  (n_fft, hop, win) = (2048, 200, 800) hp.Sound's, a window shorter than n_fft | (512, 128, 512) win = 4 hop |
                     (512, 512, 512) hop = win, one frame per sample | (1024, 256, 1000) an even window with off > 0;  one batch of three
                     utterances of 2 (the entry's minimum: the periodic reflection), 7 and 23 frames and each of them alone;  0, 1 and 3
                     iterations;  given phase uniforms and seeds.
  mstts_wg_denoise   (1024, 256, 1024) | (512, 128, 512) | (2048, 200, 800) | (512, 256, 512) win = 2 hop;  strengths 0, 0.1, 1;  one batch
                     of three waveforms of n_fft / 2 + 1 samples (the minimum), a multiple of hop and a non-multiple, and each alone;  a
                     seeded positive bias spectrum.
  mstts_stft_fft     hp.Sound's transform on a batch of two waveforms of different lengths: mel, spectrogram, and both in the
                     spectral-subtraction form, through Audio.stft_features.
A batch line and the `alone` line under it agree when a waveform's bits do not depend on its neighbours."""
import ctypes
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from multi_speaker_tts_amd import Audio, lib                             # noqa: E402
from multi_speaker_tts_amd import Hyper_Parameters as hp                 # noqa: E402

DEV = torch.device("cuda:0")
GL_PARAMS = [(2048, 200, 800), (512, 128, 512), (512, 512, 512), (1024, 256, 1000)]
GL_FRAMES = [2, 7, 23]
DN_PARAMS = [(1024, 256, 1024), (512, 128, 512), (2048, 200, 800), (512, 256, 512)]


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def up(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dtype)


def offsets(counts):
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return off, (ctypes.c_int64 * len(off))(*off.tolist())


def tables(n_fft, win):
    hann, tw = Audio._fft_tables(n_fft, win)
    return up(hann), up(tw)


def griffin_lim(spec, u, seeds, frames, hann, tw, n_fft, hop, win, iters):
    """One call on the utterances of `frames` frames: spec / u [sum frames, n_fft / 2 + 1], u None: seeds -> the packed waveform."""
    foff, host_off = offsets(frames)
    total, nu = int(foff[-1]), len(frames)
    ws = torch.empty(int(lib.load().mstts_griffin_lim_ws_floats(total, n_fft, win)), dtype=torch.float32, device=DEV)
    wav = torch.empty(hop * (total - nu), dtype=torch.float32, device=DEV)
    sd, foff_dev = up(np.asarray(seeds, np.int64), torch.int64) if u is None else None, up(foff, torch.int64)
    lib.call("mstts_griffin_lim", lib.ptr(spec), lib.ptr(u), lib.ptr(sd), host_off, lib.ptr(foff_dev), nu, lib.ptr(hann), lib.ptr(tw),
             n_fft, hop, win, 1.5, 20.0, 0.97, iters, lib.ptr(ws), lib.ptr(wav))
    torch.cuda.synchronize()
    return wav


def digest_griffin_lim():
    for n_fft, hop, win in GL_PARAMS:
        hann, tw = tables(n_fft, win)
        g = np.random.default_rng(n_fft + hop + win)
        nb, foff = n_fft // 2 + 1, offsets(GL_FRAMES)[0]
        spec = up(g.uniform(0.0, 1.0, (int(foff[-1]), nb)))
        u = up(g.uniform(0.0, 1.0, (int(foff[-1]), nb)))
        seeds = [11, 2 ** 40 + 5, 7]
        for iters in (0, 1, 3):
            for mode, uu in (("uniforms", u), ("seeds", None)):
                wav = griffin_lim(spec, uu, seeds, GL_FRAMES, hann, tw, n_fft, hop, win, iters)
                woff = hop * (foff - np.arange(len(foff)))
                name = "griffin_lim %4d %3d %4d iters %d %-8s" % (n_fft, hop, win, iters, mode)
                print("%s batch %s finite %d" % (name, " ".join(sha(wav[woff[i]:woff[i + 1]]) for i in range(3)), int(torch.isfinite(wav).all())))
                alone = [griffin_lim(spec[foff[i]:foff[i + 1]], None if uu is None else uu[foff[i]:foff[i + 1]], seeds[i:i + 1], GL_FRAMES[i:i + 1],
                                     hann, tw, n_fft, hop, win, iters) for i in range(3)]
                print("%s alone %s" % (name, " ".join(sha(w) for w in alone)))


def denoise(cat, lens, bias, strength, hann, tw, n_fft, hop, win):
    woff, host_off = offsets(lens)
    foff = offsets([1 + n // hop for n in lens])[0]
    offs = up(np.stack([woff, foff]), torch.int64)
    nw = len(lens)
    ws = torch.empty(max(int(lib.load().mstts_wg_denoise_ws_floats(int(foff[-1]), win)), 1), dtype=torch.float32, device=DEV)
    out = torch.empty_like(cat)
    lib.call("mstts_wg_denoise", lib.ptr(cat), host_off, lib.ptr(offs), lib.ptr(offs, nw + 1), nw, lib.ptr(bias), float(strength), lib.ptr(hann),
             lib.ptr(tw), n_fft, hop, win, lib.ptr(ws), lib.ptr(out))
    torch.cuda.synchronize()
    return out


def digest_denoise():
    for n_fft, hop, win in DN_PARAMS:
        hann, tw = tables(n_fft, win)
        g = np.random.default_rng(3 * n_fft + hop + win)
        k = (n_fft // 2 + 1 + hop - 1) // hop + 3
        lens = [n_fft // 2 + 1, k * hop, k * hop + hop // 2 + 1]
        woff = offsets(lens)[0]
        cat = up(g.normal(0.0, 0.3, int(woff[-1])))
        bias = up(np.abs(g.normal(0.0, 0.5, n_fft // 2 + 1)) + 1e-3)
        for strength in (0.0, 0.1, 1.0):
            out = denoise(cat, lens, bias, strength, hann, tw, n_fft, hop, win)
            name = "wg_denoise %4d %3d %4d strength %.1f" % (n_fft, hop, win, strength)
            print("%s batch %s finite %d" % (name, " ".join(sha(out[woff[i]:woff[i + 1]]) for i in range(3)), int(torch.isfinite(out).all())))
            alone = [denoise(cat[woff[i]:woff[i + 1]].clone(), lens[i:i + 1], bias, strength, hann, tw, n_fft, hop, win) for i in range(3)]
            print("%s alone %s" % (name, " ".join(sha(w) for w in alone)))


def digest_stft():
    g = np.random.default_rng(5)
    wavs = [(0.3 * g.normal(size=n)).astype(np.float32) for n in (3000, 5477)]
    args = dict(num_freq=hp.Sound.Spectrogram_Dim, frame_shift_ms=hp.Sound.Frame_Shift, frame_length_ms=hp.Sound.Frame_Length,
                sample_rate=hp.Sound.Sample_Rate, num_mels=hp.Sound.Mel_Dim, max_abs_value=hp.Sound.Max_Abs_Mel, device=DEV)
    for name, kw in (("mel", dict(want_mel=True, want_spec=False)), ("spec", dict(want_mel=False, want_spec=True)),
                     ("subtract", dict(want_mel=True, want_spec=True, spectral_subtract=True))):
        out = Audio.stft_features(wavs, **args, **kw)
        torch.cuda.synchronize()
        print("stft_fft %-8s %s" % (name, " ".join("%s:%s" % (k, sha(t)) for pair in out for k, t in zip(("mel", "spec"), pair) if t is not None)))


if __name__ == "__main__":
    digest_griffin_lim()
    digest_denoise()
    digest_stft()
