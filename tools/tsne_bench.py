"""Exact t-SNE on the GPU (tsne.tsne -> mstts_tsne_affinities, mstts_tsne_iterate) against scikit-learn on the host in one process, legs
alternated, median of --rounds: N = 653, D = 256 (the reference's in-training inference list: 11 labels of unequal sizes; here synthetic
clustered unit vectors) and N = 4096 (the envelope's edge), 1 000 iterations, perplexity 30.
  * device end to end by the host clock, host array in, host array out (upload, stage A, 2 000 launches, one read-back),
  * device stage A and stage B apart by HIP events on preallocated device tensors, stage B also per iteration,
  * scikit-learn's default TSNE (Barnes-Hut, an approximation) and TSNE(method='exact') with init='random', random_state=0 -
    the exact leg runs once at N = 4096 and is skipped there when one round at N = 653 already took longer than --exact-budget seconds,
  * the final KL of every leg (each leg's own figure).
Prints one line per figure and a JSON line per shape; exits non-zero if the device is not faster than scikit-learn's default."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from multi_speaker_tts_amd import tsne as T

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=1000)
ap.add_argument("--sizes", type=int, nargs="*", default=[653, 4096])
ap.add_argument("--exact-budget", type=float, default=60.0, help="skip scikit-learn exact at the larger sizes if it is expected to take longer (s)")
ap.add_argument("--no-sklearn", action="store_true")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("tsne_bench: no GPU")
dev = torch.device("cuda:0")
med = lambda xs: float(np.median(xs))


def clustered(n, dim, labels, seed):
    g = np.random.default_rng(seed)
    cuts = np.sort(g.choice(np.arange(1, n), labels - 1, replace=False))
    sizes = np.diff(np.concatenate([[0], cuts, [n]]))
    centres = g.normal(size=(labels, dim))
    x = np.concatenate([centres[i] + 0.35 * g.normal(size=(s, dim)) for i, s in enumerate(sizes)])
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32), sizes


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


exact_rate = None                                   # seconds per (n^2 * iteration) of scikit-learn exact, from the first size
ok = True
for n in a.sizes:
    X, sizes = clustered(n, 256, 11, 0)
    lr = T.auto_learning_rate(n, 12.0)
    res = {"n": n, "dim": 256, "labels": 11, "iters": a.iters, "perplexity": 30, "gpu": torch.cuda.get_device_name(0)}
    T.tsne(X, max_iter=60, device=dev)              # warm-up: code objects, allocator
    Xd = torch.from_numpy(X).to(dev)
    wall, ta, tb, sk_bh, sk_ex, kl = [], [], [], [], [], {}
    for r in range(a.rounds):                       # the legs alternate
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        Y, info = T.tsne(X, max_iter=a.iters, device=dev, return_info=True)
        wall.append(1e3 * (time.perf_counter() - t0))
        kl["device"] = info["kl_divergence"]
        (P, beta), ms = events(lambda: T.affinities_device(Xd, 30.0, dev))
        ta.append(ms)
        Yd = torch.from_numpy(T.random_init(n, 0)).to(dev)
        state = (Yd, torch.zeros_like(Yd), torch.ones_like(Yd))
        _, ms = events(lambda: T.iterate_device(state, P, 0, a.iters, 12.0, 250, lr))
        tb.append(ms)
        if a.no_sklearn:
            continue
        from sklearn.manifold import TSNE
        t0 = time.perf_counter()
        m = TSNE(n_components=2, random_state=0, init="random", max_iter=a.iters).fit(X)
        sk_bh.append(time.perf_counter() - t0)
        kl["sklearn_default"] = float(m.kl_divergence_)
        expect = None if exact_rate is None else exact_rate * n * n * a.iters
        if (expect is None or expect <= a.exact_budget) and not (sk_ex and n > 1024):
            t0 = time.perf_counter()
            m = TSNE(n_components=2, random_state=0, init="random", method="exact", max_iter=a.iters).fit(X)
            sk_ex.append(time.perf_counter() - t0)
            kl["sklearn_exact"] = float(m.kl_divergence_)
            res["sklearn_exact_n_iter"] = int(m.n_iter_) + 1
    if sk_ex and exact_rate is None:
        exact_rate = med(sk_ex) / (n * n * a.iters)
    res.update(device_wall_ms=med(wall), device_wall_ms_min=min(wall), device_wall_ms_max=max(wall), stage_a_ms=med(ta), stage_b_ms=med(tb),
               stage_b_us_per_iter=1e3 * med(tb) / a.iters, kl=kl)
    print("n %d (label sizes %s), %d iterations:" % (n, " ".join(str(s) for s in sizes), a.iters))
    print("  device end to end, host array to host array: %.1f ms (%.1f - %.1f), median of %d" % (med(wall), min(wall), max(wall), a.rounds))
    print("  device by events: stage A %.3f ms, stage B %.1f ms = %.1f us per iteration (two launches; enqueue included); P is %.1f MB"
          % (med(ta), med(tb), 1e3 * med(tb) / a.iters, 4e-6 * n * n))
    if sk_bh:
        res.update(sklearn_default_s=med(sk_bh), sklearn_exact_s=med(sk_ex) if sk_ex else None, sklearn_exact_rounds=len(sk_ex))
        print("  scikit-learn default (Barnes-Hut): %.2f s; device end to end / that: %.4f" % (med(sk_bh), 1e-3 * med(wall) / med(sk_bh)))
        if sk_ex:
            print("  scikit-learn method='exact': %.2f s (%d round%s, %d iterations run); device end to end / that: %.5f"
                  % (med(sk_ex), len(sk_ex), "" if len(sk_ex) == 1 else "s", res["sklearn_exact_n_iter"], 1e-3 * med(wall) / med(sk_ex)))
        else:
            print("  scikit-learn method='exact': skipped, expected %.0f s from the smaller size (budget %.0f s)" % (exact_rate * n * n * a.iters, a.exact_budget))
        ok = ok and 1e-3 * med(wall) < med(sk_bh)
    print("  final KL: " + ", ".join("%s %.4f" % kv for kv in kl.items()))
    print(json.dumps(res))
if not ok:
    sys.exit("tsne_bench: the device is not faster than scikit-learn's default")
