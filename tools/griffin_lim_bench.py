"""Batched Griffin-Lim on the GPU (Audio.griffin_lim_batch -> mstts_griffin_lim) against the host path (Audio.Griffin_Lim, NumPy fp64) in one
process: 100 iterations, power 1.5, hp.Sound's STFT (n_fft 2048, hop 200, win 800) on
  (a) 1 x 400 frames  - BASELINE config 1's Griffin-Lim shape,
  (b) 16 x 401 frames - the inference line's batch.
Device time by HIP events around the call with device tensors in and out, wall time end to end from host arrays to host waveforms
(upload, launches, read-back), warm-up excluded, median of --repeats.  The host path on ONE [400, 1025] spectrogram is the yardstick.
Prints one line per case and a JSON line; --once runs a single call of case (b) and nothing else (for a kernel trace)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from multi_speaker_tts_amd import Audio, Hyper_Parameters as hp

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--iters", type=int, default=hp.Taco1_Mel_to_Spect.Griffin_Lim_Iteration)
ap.add_argument("--host-repeats", type=int, default=2)
ap.add_argument("--once", action="store_true")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("griffin_lim_bench: no GPU")
dev = torch.device("cuda:0")
ARGS = dict(num_freq=hp.Sound.Spectrogram_Dim, frame_shift_ms=hp.Sound.Frame_Shift, frame_length_ms=hp.Sound.Frame_Length,
            sample_rate=hp.Sound.Sample_Rate, griffin_lim_iters=a.iters, device=dev)
n_fft, hop, win = Audio._stft_parameters(hp.Sound.Spectrogram_Dim, hp.Sound.Frame_Shift, hp.Sound.Frame_Length, hp.Sound.Sample_Rate)


def spectrogram(frames, seed):
    """Normalised spectrogram of tones with a tremolo and noise (bench.py's Griffin-Lim input is of the same kind)."""
    g = np.random.default_rng(seed)
    t = np.arange(hop * (frames - 1)) / hp.Sound.Sample_Rate
    y = sum(0.02 / h * np.sin(2 * np.pi * (150 + 13 * seed) * h * t + h) for h in range(1, 12)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t))
    y = y + 0.0005 * g.normal(size=t.shape)
    return np.transpose(Audio.spectrogram(y.astype(np.float32), hp.Sound.Spectrogram_Dim, hp.Sound.Frame_Shift, hp.Sound.Frame_Length,
                                          hp.Sound.Sample_Rate, device=dev)).copy()


def median(xs):
    return float(np.median(xs))


def device_case(specs):
    on_dev = [torch.as_tensor(s).to(dev) for s in specs]
    Audio.griffin_lim_batch(specs, seed=1, **ARGS)                                     # warm-up: code objects, tables, allocator
    ev, wall = [], []
    for r in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = Audio.griffin_lim_batch(on_dev, seed=1, return_tensor=True, **ARGS)
        e1.record()
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        wavs = Audio.griffin_lim_batch(specs, seed=1, **ARGS)                         # host arrays in, host arrays out (synchronises)
        wall.append(1e3 * (time.perf_counter() - t0))
    assert all(w.shape == (hop * (s.shape[0] - 1),) and np.isfinite(w).all() for w, s in zip(wavs, specs))
    return median(ev), median(wall), min(wall), max(wall)


if a.once:
    specs = [spectrogram(401, i) for i in range(16)]
    Audio.griffin_lim_batch(specs, seed=1, **ARGS)
    sys.exit(0)

res = {"iters": a.iters, "n_fft": n_fft, "hop": hop, "win": win, "gpu": torch.cuda.get_device_name(0)}
one = [spectrogram(400, 0)]
host = []
for r in range(a.host_repeats):
    t0 = time.perf_counter()
    Audio.Griffin_Lim(one[0], rng=np.random.RandomState(0))
    host.append(time.perf_counter() - t0)
res["host_one_400_frames_s"] = min(host)
print("host Audio.Griffin_Lim, 1 x [400, 1025], %d iterations: %.3f s (best of %d)" % (a.iters, min(host), len(host)))
for name, specs in (("a_1x400", one), ("b_16x401", [spectrogram(401, i) for i in range(16)])):
    ev, wall, lo, hi = device_case(specs)
    frames = sum(s.shape[0] for s in specs)
    res[name] = {"frames": frames, "device_ms": ev, "wall_ms": wall, "wall_ms_min": lo, "wall_ms_max": hi,
                 "us_per_iteration": 1e3 * ev / max(a.iters, 1)}
    print("device %-9s %5d frames: %8.2f ms by events, %8.2f ms wall end to end (%.2f - %.2f), %.1f us per iteration"
          % (name, frames, ev, wall, lo, hi, 1e3 * ev / max(a.iters, 1)))
res["b_wall_over_host_one"] = res["b_16x401"]["wall_ms"] / (1e3 * res["host_one_400_frames_s"])
print("16 utterances on the device / 1 utterance on the host: %.4f" % res["b_wall_over_host_one"])
print(json.dumps(res))
if not res["b_wall_over_host_one"] < 1.0:
    sys.exit("griffin_lim_bench: the batch of 16 on the device is not faster than one utterance on the host")
