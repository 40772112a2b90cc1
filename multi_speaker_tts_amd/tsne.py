"""Exact t-SNE into two dimensions (van der Maaten & Hinton 2008) with the schedule of scikit-learn's ``TSNE(method='exact',
init='random')``: `tsne` runs it on the GPU (csrc/tsne.hip: mstts_tsne_affinities, mstts_tsne_iterate; fp32), `tsne_host` is the fp64
statement of the same algorithm in NumPy, its stages callable alone (`affinities_host`, `joint_from_beta_host`, `gradient_host`,
`iterate_host`) - the checker every device stage is judged against (tests/test_gpu_tsne.py), itself pinned to the installed scikit-learn
(tests/test_cpu_tsne.py).

The algorithm.  Stage A: squared Euclidean distances d_ij; per row i the precision beta_i whose conditional row c_ij = exp(-beta_i d_ij) /
sum_{j != i} exp(-beta_i d_ij) has entropy ln(perplexity), found as scikit-learn's `_binary_search_perplexity` finds it (beta = 1, doubled
or halved until bracketed, then bisected, at most 100 evaluations, done at |H - ln perplexity| <= 1e-5, a zero sum replaced by 1e-8); P =
max((C + C^T) / sum, 2.220446e-16).  Stage B: `max_iter` iterations of gradient descent on KL(P || Q), q_ij = num_ij / Z, num_ij = 1 / (1 +
|y_i - y_j|^2), Z = sum_{i != j} num_ij: g_i = 4 sum_j (e p_ij - q_ij) num_ij (y_i - y_j); gains += 0.2 where update g < 0, else gains *= 0.8,
floor 0.01; update = momentum update - learning_rate gains g; Y += update.  Iterations below `exaggeration_iters` use e = early_exaggeration
and momentum 0.5, the others e = 1 and momentum 0.8, and iteration `exaggeration_iters` starts from update = 0, gains = 1: scikit-learn runs
its two stages as two calls of its descent, each of which begins that way.  There is no recentring (scikit-learn does none).

scikit-learn's early stop (no progress for 300 iterations, or a gradient norm below 1e-7, looked at every 50 iterations) is NOT built: it can
only end a run earlier, and the run length here is always `max_iter`.  scikit-learn clamps q_ij from below at 2.220446e-16; `gradient_host`
does too, the device does not - the clamp acts only where num_ij / Z < 2.2e-16, a map more than ten million units across.
"""
from __future__ import annotations

import numpy as np

FLOOR = 2.220446e-16          # scikit-learn's MACHINE_EPSILON (np.finfo(np.double).eps), the value csrc/tsne.hip uses
MAX_N, MAX_DIM = 4096, 1024
SEARCH_STEPS, SEARCH_TOL, CHECK_EVERY = 100, 1e-5, 50


def tsne_supported(n, dim, perplexity):
    """The device envelope: 4 <= n <= 4096, 1 <= dim <= 1024, 1 <= perplexity < n (mstts_tsne_supported says the same)."""
    return 4 <= int(n) <= MAX_N and 1 <= int(dim) <= MAX_DIM and 1.0 <= float(perplexity) < int(n)


def auto_learning_rate(n, early_exaggeration):
    """scikit-learn's learning_rate='auto'."""
    return max(n / early_exaggeration / 4.0, 50.0)


def random_init(n, seed):
    """What ``TSNE(init='random', random_state=seed)`` starts from: 1e-4 * RandomState(seed).standard_normal((n, 2)) as float32."""
    return (1e-4 * np.random.RandomState(seed).standard_normal((n, 2))).astype(np.float32)


def reports(it, last):
    """Does iteration `it` of a run whose last iteration is `last` append to the history?"""
    return (it + 1) % CHECK_EVERY == 0 or it == last


def distances_host(X):
    """Squared Euclidean distances [n, n] from the differences themselves (duplicate rows give an exact 0), fp64."""
    X = np.asarray(X, np.float64)
    return np.stack([np.sum((X - x) ** 2, axis=1) for x in X])


def _rows(D, beta):
    """Unnormalised conditional rows exp(-beta_i d_ij), the diagonal 0, and their sums (a zero sum replaced by 1e-8)."""
    E = np.exp(-D * beta[:, None])
    np.fill_diagonal(E, 0.0)
    s = E.sum(axis=1)
    return E, np.where(s == 0.0, 1e-8, s)


def entropy_host(D, beta):
    """H_i = ln sum_j p_j + beta_i sum_j d_ij p_j / sum_j p_j of the rows with the precisions `beta`."""
    E, s = _rows(np.asarray(D, np.float64), np.asarray(beta, np.float64))
    return np.log(s) + beta * np.sum(D * E, axis=1) / s


def conditional_host(D, perplexity):
    """The search of stage A on squared distances D [n, n] -> (C, beta): every row is searched at once, a row that has met the
    tolerance keeps the beta it met it with."""
    D = np.asarray(D, np.float64)
    n = D.shape[0]
    want = np.log(perplexity)
    beta, lo, hi = np.ones(n), np.full(n, -np.inf), np.full(n, np.inf)
    live = np.ones(n, bool)
    for _ in range(SEARCH_STEPS):
        diff = entropy_host(D, beta) - want
        live &= np.abs(diff) > SEARCH_TOL
        if not live.any():
            break
        up, down = live & (diff > 0), live & (diff <= 0)
        lo[up] = beta[up]
        hi[down] = beta[down]
        new = beta.copy()
        new[up] = np.where(np.isinf(hi[up]), beta[up] * 2.0, (beta[up] + hi[up]) / 2.0)
        new[down] = np.where(np.isinf(lo[down]), beta[down] / 2.0, (beta[down] + lo[down]) / 2.0)
        beta_evaluated, beta = beta, new
    else:
        beta = np.where(live, beta_evaluated, beta)          # out of steps: the row of the last EVALUATED beta, as scikit-learn leaves it
    E, s = _rows(D, beta)
    return E / s[:, None], beta


def _joint(C):
    S = C + C.T
    return np.maximum(S / max(S.sum(), FLOOR), FLOOR)


def joint_from_beta_host(X, beta):
    """P of stage A for GIVEN precisions (no search): what the device's P must be, given the device's beta."""
    E, s = _rows(distances_host(X), np.asarray(beta, np.float64))
    return _joint(E / s[:, None])


def affinities_host(X, perplexity):
    """Stage A -> (P [n, n], beta [n]); the diagonal of P is at the floor."""
    C, beta = conditional_host(distances_host(X), perplexity)
    return _joint(C), beta


def gradient_host(Y, P, exaggeration=1.0, want_kl=True):
    """KL(eP || Q) over i != j (None unless want_kl) and its gradient [n, 2] at the map Y: fp64 arithmetic, the gradient returned in Y's
    precision when that is float32 (scikit-learn keeps its map and gradient in float32)."""
    Y = np.asarray(Y)
    out = np.float32 if Y.dtype == np.float32 else np.float64
    Y = Y.astype(np.float64)
    P = np.asarray(P, np.float64) * exaggeration
    dx, dy = Y[:, 0][:, None] - Y[:, 0][None, :], Y[:, 1][:, None] - Y[:, 1][None, :]
    num = 1.0 / (1.0 + (dx * dx + dy * dy))
    np.fill_diagonal(num, 0.0)
    Z = max(num.sum(), FLOOR)
    Q = np.maximum(num / Z, FLOOR)
    kl = None
    if want_kl:
        T = P * np.log(np.maximum(P, FLOOR) / Q)
        np.fill_diagonal(T, 0.0)
        kl = float(T.sum())
    w = (P - Q) * num                                        # (the diagonal: num = 0)
    g = 4.0 * np.stack([np.sum(w * dx, axis=1), np.sum(w * dy, axis=1)], axis=1)
    return kl, g.astype(out)


def initial_state(Y0, dtype=np.float64):
    Y = np.array(Y0, dtype)
    return Y, np.zeros_like(Y), np.ones_like(Y)


def iterate_host(state, P, first_iter, n_iters, early_exaggeration=12.0, exaggeration_iters=250, learning_rate=200.0, dtype=np.float64):
    """Iterations first_iter ... first_iter + n_iters - 1 of stage B from state = (Y, update, gains) -> (state, history), history a list of
    (iteration, KL, |g|_2) for every iteration `reports` names.  The state is kept in `dtype` (scikit-learn keeps it in float32; the
    gradient itself is fp64 on either)."""
    Y, U, G = (np.array(a, dtype) for a in state)
    last, history = first_iter + n_iters - 1, []
    for it in range(first_iter, first_iter + n_iters):
        early = it < exaggeration_iters
        if it == exaggeration_iters:
            U, G = np.zeros_like(Y), np.ones_like(Y)
        kl, g = gradient_host(Y, P, early_exaggeration if early else 1.0, want_kl=reports(it, last))
        inc = U * g < 0.0
        G = np.maximum(np.where(inc, G + 0.2, G * 0.8), 0.01).astype(dtype)
        U = ((0.5 if early else 0.8) * U - learning_rate * (G * g)).astype(dtype)
        Y = (Y + U).astype(dtype)
        if reports(it, last):
            history.append((it, kl, float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))))
    return (Y, U, G), history


def _checked(X, perplexity):
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError("X must be [n, dim]")
    if not float(perplexity) < X.shape[0]:
        raise ValueError("perplexity (%g) must be less than the number of rows (%d)" % (perplexity, X.shape[0]))
    if not float(perplexity) > 0:
        raise ValueError("perplexity must be positive (%g)" % perplexity)
    return X


def _initial(X, init, seed):
    Y0 = random_init(X.shape[0], seed) if init is None else np.asarray(init, np.float32)
    if Y0.shape != (X.shape[0], 2):
        raise ValueError("init must be [n, 2]")
    return Y0


def _info(history, beta, max_iter):
    return {"kl_divergence": history[-1][1], "kl_history": [(it, kl) for it, kl, _ in history],
            "grad_norm_history": [(it, gn) for it, _, gn in history], "beta": np.asarray(beta), "n_iter": int(max_iter)}


def tsne_host(X, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", max_iter=1000, exaggeration_iters=250, seed=0, init=None,
              return_info=False, dtype=np.float64):
    """The whole algorithm on the host, fp64 (state in `dtype`) -> Y [n, 2] float32, with return_info also the dict `tsne` returns."""
    X = _checked(X, perplexity)
    lr = auto_learning_rate(X.shape[0], early_exaggeration) if learning_rate == "auto" else float(learning_rate)
    Y0 = _initial(X, init, seed)
    P, beta = affinities_host(X, perplexity)
    state, history = iterate_host(initial_state(Y0, dtype), P, 0, int(max_iter), early_exaggeration, exaggeration_iters, lr,
                                  dtype)
    Y = state[0].astype(np.float32)
    return (Y, _info(history, beta, max_iter)) if return_info else Y


# ---- device ----

def affinities_device(X, perplexity, device="cuda"):
    """Stage A on the GPU: X [n, dim] (array or device tensor) -> (P [n, n], beta [n]) as device tensors."""
    import torch
    from . import lib
    x = (X if torch.is_tensor(X) else torch.from_numpy(np.array(X, np.float32, order="C"))).to(torch.device(device), torch.float32).contiguous()
    n, dim = x.shape
    ws = torch.empty(int(lib.load().mstts_tsne_affinities_ws_floats(n)), dtype=torch.float32, device=x.device)
    P = torch.empty((n, n), dtype=torch.float32, device=x.device)
    beta = torch.empty(n, dtype=torch.float32, device=x.device)
    lib.call("mstts_tsne_affinities", lib.ptr(x), dim, n, dim, float(perplexity), lib.ptr(ws), lib.ptr(P), lib.ptr(beta))
    return P, beta


def iterate_device(state, P, first_iter, n_iters, early_exaggeration=12.0, exaggeration_iters=250, learning_rate=200.0, grad=None):
    """Stage B on the GPU, in place on state = (Y, update, gains), contiguous float32 device tensors [n, 2]; P [n, n] on the same device
    -> history [slots, 2] (KL, |g|_2) as a device tensor, one row per iteration `reports` names.  grad: a tensor like Y that receives the
    last iteration's gradient.  Nothing synchronises."""
    import torch
    from . import lib
    Y, U, G = state
    n = int(P.shape[0])
    for t in (Y, U, G) + (() if grad is None else (grad,)):
        if t.dtype != torch.float32 or tuple(t.shape) != (n, 2) or not t.is_contiguous() or t.device != P.device:
            raise ValueError("the state must be contiguous float32 [n, 2] tensors on P's device")
    if P.dtype != torch.float32 or tuple(P.shape) != (n, n) or not P.is_contiguous():
        raise ValueError("P must be a contiguous float32 [n, n] tensor")
    L = lib.load()
    slots = int(L.mstts_tsne_history_slots(int(first_iter), int(n_iters)))
    ws = torch.empty(int(L.mstts_tsne_iterate_ws_floats(n)), dtype=torch.float32, device=P.device)
    hist = torch.zeros((max(slots, 1), 2), dtype=torch.float32, device=P.device)
    lib.call("mstts_tsne_iterate", lib.ptr(P), n, lib.ptr(Y), lib.ptr(U), lib.ptr(G), int(first_iter), int(n_iters), int(exaggeration_iters),
             float(early_exaggeration), float(learning_rate), lib.ptr(ws), lib.ptr(hist), slots, lib.ptr(grad))
    return hist


def tsne(X, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", max_iter=1000, exaggeration_iters=250, seed=0, init=None,
         device="cuda", return_info=False):
    """Exact t-SNE of X [n, dim] on the GPU -> Y [n, 2] float32 (NumPy).  learning_rate "auto" is scikit-learn's max(n / early_exaggeration / 4,
    50); init None is `random_init(n, seed)`, made on the host - what ``TSNE(init='random', random_state=seed)`` starts from (PCA initialisation
    is not offered).  The run is always `max_iter` iterations long: scikit-learn's early stop is not built (module docstring).  The host
    reads the device once, after the run.  With return_info also a dict: kl_divergence (of the last iteration), kl_history and
    grad_norm_history (lists of (iteration, value): every 50th iteration and the last), beta [n], n_iter.
    Outside the device envelope (`tsne_supported`) one line is printed and `tsne_host` runs; perplexity >= n is a ValueError."""
    X = _checked(X, perplexity)
    n, dim = X.shape
    if not tsne_supported(n, dim, perplexity):
        print("tsne: n %d, dim %d, perplexity %g is outside the device envelope - running on the host" % (n, dim, perplexity))
        return tsne_host(X, perplexity, early_exaggeration, learning_rate, max_iter, exaggeration_iters, seed, init, return_info)
    import torch
    lr = auto_learning_rate(n, early_exaggeration) if learning_rate == "auto" else float(learning_rate)
    Y0 = _initial(X, init, seed)
    P, beta = affinities_device(X, perplexity, device)
    Y = torch.from_numpy(Y0.copy()).to(P.device).contiguous()
    state = (Y, torch.zeros_like(Y), torch.ones_like(Y))
    hist = iterate_device(state, P, 0, int(max_iter), early_exaggeration, exaggeration_iters, lr)
    out = Y.cpu().numpy()
    if not return_info:
        return out
    last = int(max_iter) - 1
    its = [it for it in range(int(max_iter)) if reports(it, last)]
    h = hist.cpu().numpy().astype(np.float64)
    return out, _info([(it, float(k), float(g)) for it, (k, g) in zip(its, h)], beta.cpu().numpy(), max_iter)
