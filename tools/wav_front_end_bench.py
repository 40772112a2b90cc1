"""The waveform front end on the GPU (Audio.wav_features: resample, trim, scale, mel on the device) against the host path it replaces, in
one process: synthetic utterances of 6 s at 48 kHz and at 22.05 kHz -> 16 kHz mels, batches of 16, 1 and 256.
  (a) host: load_wav's arithmetic per wav (scipy.signal.resample_poly, the NumPy frame-RMS trim, x 0.99) + one Audio.melspectrogram
      launch and one copy back per wav - what Feeder.Get_Inference_Pattern and Pattern_Generate.Mel_Generate do today;
  (b) device: one Audio.wav_features call for the batch, host arrays in, host mels out.
File decoding is excluded from both; the upload and the one host read are inside (b).  Wall clock and HIP events around each path,
--warmup + --repeats repetitions, median.  Prints one line per case and a JSON line; exits non-zero when (b) is slower than (a) at
batch 16 or batch 1 of the 48 kHz case.  --once runs a single device call of 16 x 6 s at 48 kHz and nothing else (for a kernel trace).
--rule librosa: both paths under the second rule set (kaiser_best rate conversion, centred trim): (a) is then the float64 host rule of
Feeder.load_wav(rule="librosa"), (b) Audio.wav_features(rule="librosa"); no target is set for it, the exit status is 0.  --big 0 leaves
the large batch out."""
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
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--seconds", type=float, default=6.0)
ap.add_argument("--big", type=int, default=256)
ap.add_argument("--once", action="store_true")
ap.add_argument("--rule", choices=("scipy", "librosa"), default="scipy")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("wav_front_end_bench: no GPU")
dev = torch.device("cuda:0")
SR = hp.Sound.Sample_Rate
MEL = dict(num_freq=hp.Sound.Spectrogram_Dim, frame_shift_ms=hp.Sound.Frame_Shift, frame_length_ms=hp.Sound.Frame_Length, num_mels=hp.Sound.Mel_Dim,
           sample_rate=SR, max_abs_value=hp.Sound.Max_Abs_Mel, device=dev)


def utterance(rate, seed):
    """Harmonics of a 110 - 150 Hz fundamental under a smooth envelope with 0.3 s of near silence at both ends, float32 in [-1, 1]."""
    g = np.random.default_rng(seed)
    t = np.arange(int(rate * a.seconds)) / float(rate)
    f0 = 110.0 + 40.0 * g.random()
    y = sum(np.sin(2 * np.pi * f0 * k * t + 2 * np.pi * g.random()) / k for k in range(1, 20))
    env = np.clip(3 * np.sin(np.pi * np.clip((t - 0.3) / (a.seconds - 0.6), 0, 1)), 0, 1) ** 2
    y = 0.2 * env * y + 1e-3 * g.normal(size=t.shape[0])
    return (0.8 * y / np.abs(y).max()).astype(np.float32)


def host_front_end(data, rate, top_db=15.0, frame=32, hop=16):
    """Feeder.load_wav from the decoded samples on."""
    if a.rule == "librosa":
        if rate != SR:
            data = Audio.resample_kaiser_best(data, *Audio.resample_ratio(rate, SR)).astype(np.float32)
        start, end = Audio.trim_bounds_centred(data, top_db, frame, hop)
        return data[start:end] * 0.99
    from scipy.signal import resample_poly
    if rate != SR:
        g = np.gcd(int(rate), int(SR))
        data = resample_poly(data, SR // g, rate // g).astype(np.float32)
    if data.shape[0] >= frame:
        n = 1 + (data.shape[0] - frame) // hop
        idx = np.arange(frame)[None, :] + hop * np.arange(n)[:, None]
        rms = np.sqrt((data[idx] ** 2).mean(axis=1))
        db = 20.0 * np.log10(np.maximum(rms, 1e-10) / max(rms.max(), 1e-10))
        keep = np.nonzero(db > -top_db)[0]
        if keep.size:
            data = data[keep[0] * hop: min(data.shape[0], (keep[-1] + 1) * hop)]
    return data * 0.99


def path_a(sigs, rate):
    return [np.transpose(Audio.melspectrogram(y=host_front_end(s, rate), **MEL)) for s in sigs]


def path_b(sigs, rate):
    return [m for m, _ in Audio.wav_features(sigs, [rate] * len(sigs), rule=a.rule, **MEL)]


def timed(fn, sigs, rate, repeats):
    for _ in range(a.warmup):
        out = fn(sigs, rate)
    wall, ev = [], []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        t0 = time.perf_counter()
        out = fn(sigs, rate)
        e1.record()
        torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
        ev.append(e0.elapsed_time(e1))
    return float(np.median(wall)), float(np.median(ev)), out


if a.once:
    sigs = [utterance(48000, i) for i in range(16)]
    path_b(sigs, 48000)
    torch.cuda.synchronize()
    sys.exit(0)

res = {"gpu": torch.cuda.get_device_name(0), "rule": a.rule, "seconds": a.seconds, "repeats": a.repeats, "warmup": a.warmup}
print("%-22s %12s %12s %12s %12s %8s" % ("case", "host wall ms", "host ev ms", "dev wall ms", "dev ev ms", "a / b"))
for rate in (48000, 22050):
    pool = [utterance(rate, i) for i in range(16)]
    for batch in (16, 1) + ((a.big,) if a.big > 0 else ()):
        sigs = [pool[i % 16] for i in range(batch)]
        wa, ea, ma = timed(path_a, sigs, rate, a.repeats if batch <= 16 else 2)
        wb, eb, mb = timed(path_b, sigs, rate, a.repeats)
        assert all(x.shape == y.shape for x, y in zip(ma, mb))
        diff = max(float(np.abs(x - y).max()) for x, y in zip(ma, mb))
        name = "%d x %g s @ %d" % (batch, a.seconds, rate)
        res[name] = {"host_wall_ms": wa, "host_event_ms": ea, "device_wall_ms": wb, "device_event_ms": eb, "host_over_device": wa / wb,
                     "max_mel_diff": diff}
        print("%-22s %12.3f %12.3f %12.3f %12.3f %8.1f   (max |mel a - mel b| %.2g)" % (name, wa, ea, wb, eb, wa / wb, diff))
print(json.dumps(res))
slow = [k for k in ("16 x %g s @ 48000" % a.seconds, "1 x %g s @ 48000" % a.seconds) if not res[k]["host_over_device"] >= 1.0]
if slow and a.rule == "scipy":
    sys.exit("wav_front_end_bench: the device path is slower than the host path for " + ", ".join(slow))
