"""WaveGlow inference throughput at the reference sizes (BASELINE.json configs[4]: batch 4 chunks x 40 mel frames).

--arith-ab [--rounds R] [--out FILE]: the vocoder's arithmetic modes against each other in ONE process, at N = 4 and N = 16 chunks x 40 frames:
three legs - f32 | bf16 (resident bf16 operands, mstts_gemm_bf16_res) | bf16 with MSTTS_WG_BF16_RESIDENT=0 (mstts_gemm_bf16 on the fp32
buffers) - ALTERNATED (every round runs the legs in turn, so drift and neighbours on a shared machine hit all legs alike), R >= 7 rounds after
warm-up, each call timed by device events; median / min / max per leg, and for a fixed latent seed |wav_bf16 - wav_f32| / |wav_f32|.
Acceptance rule of a faster leg: its slowest round beats the other leg's fastest round."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from multi_speaker_tts_amd.waveglow import WaveGlowEngine, WGDims, random_values
dev = torch.device("cuda:0")
d = WGDims()
values = None
if "--arith-ab" in sys.argv:
    # the reference's initialiser zeroes every coupling's output conv (an identity coupling: no contraction reaches the samples, the two
    # arithmetics would give the same waveform); a trained network's are small but not zero
    values = random_values(d, 1234)
    g = np.random.default_rng(1)
    for k in values:
        if k.endswith("wavenet/conv1d/kernel"):
            values[k] = g.normal(0, 0.0025, values[k].shape).astype(np.float32)
eng = WaveGlowEngine(d, device=dev, values=values)
eng.split_in = int(os.environ.get("SPLIT_IN", 0))
N, T = int(os.environ.get("N", 4)), 40


def arith_ab(rounds, out_path):
    legs = [("f32", "f32", "1"), ("bf16", "bf16", "1"), ("bf16 RESIDENT=0", "bf16", "0")]
    lines = []

    def run(mel, arith, resident, seed):
        os.environ["MSTTS_WG_BF16_RESIDENT"] = resident
        return eng.infer(mel, seed=seed, arith=arith)
    for n in (4, 16):
        mel = torch.tensor(np.clip(np.random.default_rng(0).normal(0, 1.5, (n, T, d.n_mel)), -4, 4).astype(np.float32), device=dev)
        samples = n * ((T - 1) * d.up_stride + d.up_k)
        for _ in range(2):                                   # warm-up: every leg, every shape
            for _, arith, res in legs:
                run(mel, arith, res, 0)
        torch.cuda.synchronize()
        ms = {name: [] for name, _, _ in legs}
        for r in range(rounds):
            for name, arith, res in legs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(mel, arith, res, r)
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1))
        for name, _, _ in legs:
            v = np.array(ms[name])
            lines.append("N = %2d x %d frames (%d samples), %-16s median %7.2f ms  min %7.2f  max %7.2f  (%d alternated rounds)  %.2f M samples/s"
                         % (n, T, samples, name + ":", np.median(v), v.min(), v.max(), rounds, samples / np.median(v) / 1e3))
        for a, b in (("bf16", "f32"), ("bf16", "bf16 RESIDENT=0")):
            lines.append("N = %2d: slowest %s round %.2f ms %s fastest %s round %.2f ms" % (
                n, a, max(ms[a]), "<" if max(ms[a]) < min(ms[b]) else ">= (NO non-overlapping win)", b, min(ms[b])))
        w32, w16 = run(mel, "f32", "1", 5).double(), run(mel, "bf16", "1", 5).double()
        lines.append("N = %2d, latent seed 5: |wav_bf16 - wav_f32| / |wav_f32| = %.3e" % (n, float((w16 - w32).norm() / w32.norm())))
    text = "\n".join(lines)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


if "--arith-ab" in sys.argv:
    arg = lambda flag, default: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else default
    arith_ab(max(7, int(arg("--rounds", 7))), arg("--out", None))
    sys.exit(0)
mel = np.clip(np.random.default_rng(0).normal(0, 1.5, (N, T, d.n_mel)), -4, 4).astype(np.float32)
L = (T - 1) * d.up_stride + d.up_k
rows = N * L // d.groups
flop = 0
for f in range(d.flows):
    c = d.channels(f)
    per_row = 2 * (c // 2) * d.ch + 2 * d.groups * d.n_mel * d.layers * 2 * d.ch + d.layers * 2 * d.k * d.ch * 2 * d.ch \
              + (d.layers - 1) * 2 * d.ch * 2 * d.ch + 2 * d.ch * d.ch + 2 * d.ch * c
    flop += per_row * rows
for it in range(3):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    w = eng.infer(mel, seed=it)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    print("batch %d x %d frames -> %d samples: %.1f ms, %.0f samples/s (%.1fx real time at 22.05 kHz), %.1f TFLOP/s"
          % (N, T, N * L, dt * 1e3, N * L / dt, N * L / dt / 22050, flop / dt / 1e12))
