"""Batched DTW on the GPU (dtw.dtw_batch -> mstts_dtw_batch) against the vectorised fp64 host checker (dtw.dtw_host) in one process, legs
alternated, median of --rounds: 16 pairs of about 700 x 720 frames, K = 13 (an evaluation batch of Tacotron2.Evaluate), and one such pair alone.
  * device by HIP events on tensors already on the device (the launch alone, enqueue included), without and with the path, and the same
    divided by the longest pair's n + m - 1 anti-diagonals - one workgroup barrier each: the price of a step,
  * device end to end by the host clock, host arrays in, host arrays out (one upload, one launch, one download),
  * mcd_dtw_batch end to end from 80-band mels (cepstra and DTW with no host round trip in between),
  * the two-pass form at K = 80, by events,
  * dtw_host on the same pairs, one after the other.
Prints one line per figure and a JSON line per leg, and writes the same text to --out (default profiles/dtw_bench.txt)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from multi_speaker_tts_amd import dtw as D

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--host-rounds", type=int, default=2)
ap.add_argument("--pairs", type=int, default=16)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dtw_bench.txt"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("dtw_bench: no GPU")
dev = torch.device("cuda:0")
med = lambda xs: float(np.median(xs))
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def launcher(a_List, b_List, want_path):
    """The launch alone on resident tensors -> a callable."""
    n_List, m_List = [x.shape[0] for x in a_List], [x.shape[0] for x in b_List]
    a_off, b_off, offs, hosts = D._offsets(n_List, m_List)
    offs_d, a_d, b_d = D._upload([offs, np.concatenate(a_List), np.concatenate(b_List)], dev)
    pairs = len(a_List)
    cost, length = torch.zeros(pairs, device=dev), torch.zeros(pairs, dtype=torch.int32, device=dev)
    path = torch.zeros((int(a_off[-1] + b_off[-1]) - pairs, 2), dtype=torch.int32, device=dev) if want_path else None
    return lambda: D.dtw_launch(a_d, b_d, offs_d, hosts, a_List[0].shape[1], "symmetric1", cost, length, path)


g = np.random.default_rng(0)
shapes = [(int(700 + g.integers(-40, 41)), int(720 + g.integers(-40, 41))) for _ in range(a.pairs)]
say("GPU: %s; %d pairs, frames %s" % (torch.cuda.get_device_name(0), a.pairs, " ".join("%dx%d" % s for s in shapes)))
for label, todo in (("%d pairs" % a.pairs, shapes), ("1 pair", [(700, 720)])):
    mels_a = [np.clip(g.normal(0, 1.5, (n, 80)), -4, 4).astype(np.float32) for n, _ in todo]
    mels_b = [np.clip(g.normal(0, 1.5, (m, 80)), -4, 4).astype(np.float32) for _, m in todo]
    A = [D.mel_cepstra_host(x, 13).astype(np.float32) for x in mels_a]
    B = [D.mel_cepstra_host(x, 13).astype(np.float32) for x in mels_b]
    diagonals = max(n + m - 1 for n, m in todo)
    D.dtw_batch(A, B, return_path=True, device=dev)            # warm-up: code objects, allocator
    D.mcd_dtw_batch(mels_a, mels_b, device=dev)
    plain, with_path, wide = launcher(A, B, False), launcher(A, B, True), launcher(mels_a, mels_b, False)
    wide()
    ev, evp, evw, wall, wallp, wallm, host = [], [], [], [], [], [], []
    for r in range(a.rounds):
        ev.append(events(plain, 10))
        evp.append(events(with_path, 10))
        evw.append(events(wide, 3))
        for store, fn in ((wall, lambda: D.dtw_batch(A, B, device=dev)), (wallp, lambda: D.dtw_batch(A, B, return_path=True, device=dev)),
                          (wallm, lambda: D.mcd_dtw_batch(mels_a, mels_b, device=dev))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            store.append(1e3 * (time.perf_counter() - t0))
        if r < a.host_rounds:
            t0 = time.perf_counter()
            ref = [D.dtw_host(x, y) for x, y in zip(A, B)]
            host.append(1e3 * (time.perf_counter() - t0))
    worst = max(abs(float(c) - h["cost"]) / h["cost"] for c, h in zip(D.dtw_batch(A, B, device=dev)["cost"], ref))
    say("%s, K = 13, symmetric1 (longest pair: %d anti-diagonals):" % (label, diagonals))
    say("  device by events, fused launch, no path: %.3f ms = %.3f us per anti-diagonal; with the path: %.3f ms" % (med(ev), 1e3 * med(ev) / diagonals, med(evp)))
    say("  device end to end, host arrays to host arrays: %.3f ms (%.3f - %.3f); with the path %.3f ms; median of %d"
        % (med(wall), min(wall), max(wall), med(wallp), a.rounds))
    say("  mcd_dtw_batch end to end from 80-band mels: %.3f ms" % med(wallm))
    say("  two-pass form on the same frames at K = 80, by events: %.3f ms" % med(evw))
    say("  dtw_host (fp64, vectorised over anti-diagonals), the pairs one after the other: %.1f ms; device end to end / that: %.5f"
        % (med(host), med(wall) / med(host)))
    say("  largest relative cost difference device / host: %.2e" % worst)
    if med(wall) >= med(host):
        say("  THE DEVICE BATCH DOES NOT BEAT THE HOST CHECKER HERE")
    say(json.dumps({"leg": label, "k": 13, "diagonals": diagonals, "event_ms": med(ev), "event_path_ms": med(evp), "us_per_diagonal": 1e3 * med(ev) / diagonals,
                    "wall_ms": med(wall), "wall_path_ms": med(wallp), "mcd_wall_ms": med(wallm), "two_pass_k80_event_ms": med(evw), "host_ms": med(host),
                    "rounds": a.rounds, "gpu": torch.cuda.get_device_name(0)}))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
