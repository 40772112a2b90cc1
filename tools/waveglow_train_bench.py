"""WaveGlow training step time at the reference shape (hp.WaveGlow.Train: batch 4 x Max_Signal_Length 8 000 samples, all reference
widths: 12 flows x 8 WaveNet layers of 512 channels, upsampler 1024 / 256): 2 warm-up steps, 5 timed steps, ms/step and samples/s."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from multi_speaker_tts_amd.waveglow import WGDims
from multi_speaker_tts_amd.waveglow_trainer import WaveGlowTrainEngine
dev = torch.device("cuda:0")
d = WGDims()
N, La = int(os.environ.get("N", 4)), int(os.environ.get("SAMPLES", 8000))
WARMUP, STEPS = int(os.environ.get("WARMUP", 2)), int(os.environ.get("STEPS", 5))
T = -(-(La - d.up_k) // d.up_stride) + 1
g = np.random.default_rng(0)
audio = torch.tensor(np.clip(g.normal(0, 0.3, (N, La)), -0.99, 0.99), dtype=torch.float32, device=dev)
mel = torch.tensor(np.clip(g.normal(0, 1.5, (N, T, d.n_mel)), -4, 4), dtype=torch.float32, device=dev)
eng = WaveGlowTrainEngine(d, device=dev)
rows = N * (La // d.groups)
flop = 0                                  # forward multiply-adds x 2; the step counts the forward three times (forward + two backward products)
for f in range(d.flows):
    c = d.channels(f)
    flop += 2 * rows * (c * c + (c // 2) * d.ch + d.groups * d.n_mel * d.layers * 2 * d.ch + d.layers * d.k * d.ch * 2 * d.ch
                        + (d.layers - 1) * d.ch * 2 * d.ch + d.ch * d.ch + d.ch * c)
flop += 2 * N * T * d.n_mel * d.up_k * d.n_mel
for _ in range(WARMUP):
    w = eng.train_step(audio, mel)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(STEPS):
    w = eng.train_step(audio, mel)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / STEPS
s = eng.scalars(w)
print("waveglow train step, batch %d x %d samples (%d frames), reference widths: %.1f ms/step, %.0f samples/s, %.1f TFLOP/s "
      "(%.2f TFLOP/step counted as 3 x forward); loss %.4f, global norm %.3g, peak memory %.1f GB"
      % (N, La, T, dt * 1e3, N * La / dt, 3 * flop / dt / 1e12, 3 * flop / 1e12, s["Loss"], s["Global_Norm"], torch.cuda.max_memory_allocated() / 1e9))
