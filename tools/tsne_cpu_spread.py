"""How far apart do correct t-SNE runs end?  CPU only.  For the cases and seeds of the whole-run test of tests/test_gpu_tsne.py: the final
KL(P || Q) and the Embedding_Value of the 2-D map against the true labels of (a) the fp64 checker tsne.tsne_host, (b) its fp32 emulation
(the same iteration with state AND gradient arithmetic in float32, the pair sums in NumPy's pairwise order), (c) scikit-learn's
TSNE(method='exact', init=random_init(n, seed), learning_rate='auto').  Trajectories of correct runs diverge within 100 iterations
(second table: checker against scikit-learn's _gradient_descent on the same P and state), so only the results can be compared; the
largest excess KL_x / KL_y - 1 over any two of the three runs of one (case, seed) is the ruler the device's final KL is capped by.

    python tools/tsne_cpu_spread.py            # prints the tables; the figures are quoted in tests/test_gpu_tsne.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from multi_speaker_tts_amd import tsne as T                                    # noqa: E402
from multi_speaker_tts_amd.Speaker_Embedding import Embedding_Value            # noqa: E402
import tsne_cases as TC                                                        # noqa: E402


def gradient_f32(Y, P, e):
    """gradient_host's formulas in float32, in the split form the device uses: g = 4 (a - b / Z)."""
    f = np.float32
    dx, dy = Y[:, 0][:, None] - Y[:, 0][None, :], Y[:, 1][:, None] - Y[:, 1][None, :]
    num = f(1) / (f(1) + (dx * dx + dy * dy))
    np.fill_diagonal(num, f(0))
    Z = num.sum(dtype=f)
    w, n2 = (f(e) * P) * num, num * num
    a = np.stack([np.sum(w * dx, axis=1, dtype=f), np.sum(w * dy, axis=1, dtype=f)], axis=1)
    b = np.stack([np.sum(n2 * dx, axis=1, dtype=f), np.sum(n2 * dy, axis=1, dtype=f)], axis=1)
    return f(4) * (a - b / Z)


def run_f32(P64, Y0, n_iters, lr, e=12.0, ex=250):
    f = np.float32
    P, Y = P64.astype(f), Y0.astype(f)
    U, G = np.zeros_like(Y), np.ones_like(Y)
    for it in range(n_iters):
        early = it < ex
        if it == ex:
            U, G = np.zeros_like(Y), np.ones_like(Y)
        g = gradient_f32(Y, P, e if early else 1.0)
        G = np.maximum(np.where(U * g < 0, G + f(0.2), G * f(0.8)), f(0.01))
        U = f(0.5 if early else 0.8) * U - f(lr) * (G * g)
        Y = Y + U
    return Y


def main():
    from scipy.spatial.distance import squareform
    from sklearn.manifold import TSNE, _t_sne
    worst = 0.0
    print("case seed |  KL: fp64 checker, fp32 emulation, scikit-learn exact | Embedding_Value of the map: the same three | largest excess")
    for name in ("A", "B"):
        X, perplexity = TC.case(name)
        n, lab = X.shape[0], TC.labels(name)
        P, _ = TC.host_affinities(name)
        lr = TC.learning_rate(name)
        for seed in (0, 1, 2):
            Y0 = T.random_init(n, seed)
            (Ya, _, _), hist = T.iterate_host(T.initial_state(Y0), P, 0, 1000, 12.0, 250, lr)
            Yb = run_f32(P, Y0, 1000, lr)
            sk = TSNE(method="exact", init=Y0.copy(), learning_rate="auto", perplexity=perplexity, max_iter=1000)
            Yc = sk.fit_transform(X)
            kls = [hist[-1][1], T.gradient_host(Yb.astype(np.float64), P)[0], T.gradient_host(Yc.astype(np.float64), P)[0]]
            vals = [float(Embedding_Value(Y, lab)) for Y in (Ya, Yb, Yc)]
            excess = max(a / b - 1.0 for a in kls for b in kls)
            worst = max(worst, excess)
            print("%s    %d    | %.4f %.4f %.4f (scikit-learn's own figure %.4f, %d iterations) | %.1f %.1f %.1f | %.4f"
                  % (name, seed, kls[0], kls[1], kls[2], sk.kl_divergence_, sk.n_iter_ + 1, vals[0], vals[1], vals[2], excess))
    print("largest excess between any two correct runs of one case and seed: %.4f" % worst)
    print()
    print("case iterations | max |Y - Y_sklearn| / max |Y_sklearn|: fp64 state, float32 state (scikit-learn's _gradient_descent, same P, same start)")
    for name in ("C", "D", "A"):
        X, _ = TC.case(name)
        n = X.shape[0]
        P, _ = TC.host_affinities(name)
        Pc = squareform(P, checks=False) * 12.0
        lr = TC.learning_rate(name)
        for iters in (10, 50, 100, 250):
            errs = []
            for dt in (np.float64, np.float32):
                Y0 = T.random_init(n, 0).astype(dt)
                p, _, _ = _t_sne._gradient_descent(_t_sne._kl_divergence, Y0.ravel().copy(), it=0, max_iter=iters, momentum=0.5, learning_rate=lr,
                                                   n_iter_check=50, min_grad_norm=0.0, n_iter_without_progress=10 ** 9, args=[Pc, 1.0, n, 2],
                                                   kwargs=dict(skip_num_points=0))
                (Y, _, _), _ = T.iterate_host(T.initial_state(Y0, dt), P, 0, iters, 12.0, 250, lr, dt)
                errs.append(float(np.abs(Y.ravel() - p).max() / np.abs(p).max()))
            print("%s    %4d       | %.3e %.3e" % (name, iters, errs[0], errs[1]))


if __name__ == "__main__":
    main()
