"""The WaveGlow denoiser on the GPU (Audio.spectral_denoise_batch -> mstts_wg_denoise) against the host loop (Audio.spectral_denoise, NumPy
fp64, one utterance at a time) in one process, legs alternated: 16 utterances of 3 s at 22 050 Hz, n_fft 1024 / hop 256 / win 1024.
  * device call by HIP events (device tensors in and out; --calls calls between one pair of events, so the window is not the clock's),
  * end to end by the host clock from host arrays to host arrays (upload, two launches, read-back),
  * the kernel pair alone (mstts_wg_denoise on preallocated buffers, --calls calls between events) against its byte floor: read n,
    write and read total_frames * win, write n floats, at 8 TB/s,
  * the one-off cost of WaveGlowEngine.bias_spectrum at the reference's size (first call, and again after load() dropped the cache),
  * max |device - host| of the timed inputs, relative to the input's peak.
Prints one line per figure and a JSON line; exits non-zero if the device batch is not faster than the host loop."""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from multi_speaker_tts_amd import Audio, lib
from multi_speaker_tts_amd import waveglow as WG

ap = argparse.ArgumentParser()
ap.add_argument("--utterances", type=int, default=16)
ap.add_argument("--seconds", type=float, default=3.0)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--calls", type=int, default=100)
ap.add_argument("--strength", type=float, default=0.1)
ap.add_argument("--no-engine", action="store_true", help="skip the bias_spectrum timing (the bias is then a seeded random spectrum)")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("wg_denoise_bench: no GPU")
dev = torch.device("cuda:0")
RATE, N_FFT, HOP, WIN = 22050, 1024, 256, 1024
n = int(RATE * a.seconds)
g = np.random.default_rng(0)
t = np.arange(n) / RATE
wavs = [(0.3 * np.sin(2 * np.pi * (150 + 13 * i) * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t)) + 0.01 * g.normal(size=n)).astype(np.float32)
        for i in range(a.utterances)]
res = {"utterances": a.utterances, "samples": n, "n_fft": N_FFT, "hop": HOP, "win": WIN, "strength": a.strength, "gpu": torch.cuda.get_device_name(0)}


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


if a.no_engine:
    bias = torch.as_tensor(np.abs(g.normal(0, 0.5, N_FFT // 2 + 1)).astype(np.float32)).to(dev)
else:
    eng = WG.WaveGlowEngine(WG.WGDims(), device=dev, values=WG.random_values(WG.WGDims(), seed=1))
    for F in eng.flow:                                           # (a freshly initialised flow has zero output convs and no bias signal)
        F["b_out"].copy_(torch.as_tensor(g.normal(0, 0.05, tuple(F["b_out"].shape)).astype(np.float32)))
    bias, first = sync_time(lambda: eng.bias_spectrum())
    eng._bias = {}
    bias, again = sync_time(lambda: eng.bias_spectrum())
    res["bias_spectrum_first_ms"], res["bias_spectrum_again_ms"] = first, again
    print("bias_spectrum at the reference's size (88 frames, 23 296 samples): %.1f ms the first time (code objects, tables), %.1f ms again" % (first, again))
bias_host = bias.cpu().numpy().astype(np.float64)

on_dev = [torch.as_tensor(w).to(dev) for w in wavs]
Audio.spectral_denoise_batch(wavs, bias, a.strength, N_FFT, HOP, WIN, device=dev)                     # warm-up: code objects, tables, allocator
ev, wall, host = [], [], []
for r in range(a.repeats):                                      # the legs alternate
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(a.calls):
        out = Audio.spectral_denoise_batch(on_dev, bias, a.strength, N_FFT, HOP, WIN, device=dev, return_tensor=True)
    e1.record()
    torch.cuda.synchronize()
    ev.append(e0.elapsed_time(e1) / a.calls)
    t0 = time.perf_counter()
    got = Audio.spectral_denoise_batch(wavs, bias, a.strength, N_FFT, HOP, WIN, device=dev)          # host arrays in, host arrays out (synchronises)
    wall.append(1e3 * (time.perf_counter() - t0))
    t0 = time.perf_counter()
    want = [Audio.spectral_denoise(w, bias_host, a.strength, N_FFT, HOP, WIN) for w in wavs]
    host.append(1e3 * (time.perf_counter() - t0))
err = max(float(np.abs(y - w).max() / np.abs(x).max()) for x, y, w in zip(wavs, got, want))
med = lambda xs: float(np.median(xs))
res.update(device_call_ms=med(ev), wall_ms=med(wall), wall_ms_min=min(wall), wall_ms_max=max(wall), host_loop_ms=med(host), host_loop_ms_min=min(host),
           max_err_of_peak=err)
print("device call, %d x %d samples: %.3f ms by events (%d calls per window), %.2f ms end to end from host arrays (%.2f - %.2f)"
      % (a.utterances, n, med(ev), a.calls, med(wall), min(wall), max(wall)))
print("host loop (Audio.spectral_denoise, fp64): %.1f ms (best %.1f); device end to end / host loop: %.4f; max |device - host| %.3e of the peak"
      % (med(host), min(host), med(wall) / med(host), err))

# the kernel pair alone against its byte floor
lens = [n] * a.utterances
wav_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
frame_off = np.concatenate([[0], np.cumsum([1 + m // HOP for m in lens])]).astype(np.int64)
total = int(frame_off[-1])
offs = torch.as_tensor(np.stack([wav_off, frame_off])).to(dev)
hann, tw = Audio._fft_constants_samples(N_FFT, WIN, str(dev))
cat, ws, out = torch.cat(on_dev).contiguous(), torch.empty(total * WIN, device=dev), torch.empty(n * a.utterances, device=dev)
host_off = (ctypes.c_int64 * (a.utterances + 1))(*[int(v) for v in wav_off])
pair = lambda: lib.call("mstts_wg_denoise", lib.ptr(cat), host_off, lib.ptr(offs), lib.ptr(offs, a.utterances + 1), a.utterances, lib.ptr(bias),
                        float(a.strength), lib.ptr(hann), lib.ptr(tw), N_FFT, HOP, WIN, lib.ptr(ws), lib.ptr(out))
pair()
kt = []
for r in range(a.repeats):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(a.calls):
        pair()
    e1.record()
    torch.cuda.synchronize()
    kt.append(1e3 * e0.elapsed_time(e1) / a.calls)
nbytes = 4 * (2 * n * a.utterances + 2 * total * WIN)
floor_us = nbytes / 8e12 * 1e6
res.update(kernel_pair_us=med(kt), kernel_pair_us_min=min(kt), kernel_pair_us_max=max(kt), bytes=nbytes, byte_floor_us=floor_us, frames=total)
print("kernel pair, %d frames: %.1f us per call back to back (%.1f - %.1f; enqueue included); byte floor %.2f MB at 8 TB/s = %.2f us: %.1f x the floor"
      % (total, med(kt), min(kt), max(kt), nbytes / 1e6, floor_us, med(kt) / floor_us))
print(json.dumps(res))
if not med(wall) < med(host):
    sys.exit("wg_denoise_bench: the device batch is not faster than the host loop")
