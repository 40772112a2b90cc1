"""One train step with the persistent launches switched off, so the launch-per-step loop drivers (csrc/decoder.hip) and their host-side
launch rate are on the clock: reference widths, B = 32 x 128 tokens x a short mel.  usage: launch_per_step_bench.py [L=40] [steps=20]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from multi_speaker_tts_amd.engine import TrainEngine
from multi_speaker_tts_amd.params import Dims

L = int(sys.argv[1]) if len(sys.argv) > 1 else 40
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
dev, d, g, B, Te = torch.device("cuda:0"), Dims(), np.random.default_rng(0), 32, 128
eng = TrainEngine(d, device=dev, seed=1234)
tok = g.integers(2, d.n_tok, size=(B, Te)).astype(np.int32)
tok[:, 0] = 0
tok[:, -1] = 1
mel = np.clip(g.normal(0, 1.5, size=(B, L, d.n_mel)), -4, 4).astype(np.float32)
spk = g.normal(0, 1, size=(B, d.spk))
spk = (spk / np.sqrt((spk ** 2).sum())).astype(np.float32)
t = lambda a: torch.from_numpy(a).to(dev).contiguous()
batch = {"Token": t(tok), "Token_Length": t(np.full(B, Te, np.int32)), "Mel": t(mel), "Mel_Length": t(np.full(B, L, np.int32)), "Speaker_Embedding": t(spk)}
w = eng.plan(B, Te, L)
w.persist = w.persist_bwd = False
for i in range(3 + steps):
    if i == 3:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
    eng.train_step(batch)
torch.cuda.synchronize()
print("launch-per-step train step B=%d Te=%d L=%d : %.3f ms" % (B, Te, L, (time.perf_counter() - t0) / steps * 1e3))
