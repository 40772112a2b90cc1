"""The inputs of the t-SNE tests (test_cpu_tsne.py, test_gpu_tsne.py): clustered unit vectors - S centres ~ N(0, I) in `dim` dimensions plus
0.35 N(0, I) noise, rows normalised, float32, default_rng(seed) - and the reference results that more than one test needs, computed once per
process and handed out read-only."""
import functools

import numpy as np

# name: (cluster sizes, dim, perplexity, seed)
CASES = {
    "A": ((16,) * 6, 256, 10, 1),             # N = 96
    "B": ((11,) * 7, 256, 5, 2),              # N = 77, no multiple of 64; row 5 is overwritten by row 3: a zero distance
    "C": ((13,) * 5, 3, 3, 3),                # N = 65: one past a wave, a narrow input
    "D": ((2, 2), 8, 1, 4),                   # N = 4: the lower edge
    "E": ((103,) * 10, 64, 30, 6),            # N = 1030: crosses 1024
}


def clustered(sizes, dim, seed):
    g = np.random.default_rng(seed)
    centres = g.normal(size=(len(sizes), dim))
    x = np.concatenate([centres[i] + 0.35 * g.normal(size=(s, dim)) for i, s in enumerate(sizes)])
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def labels(name):
    return [i for i, s in enumerate(CASES[name][0]) for _ in range(s)]


@functools.lru_cache(maxsize=None)
def case(name):
    sizes, dim, perplexity, seed = CASES[name]
    X = clustered(sizes, dim, seed)
    if name == "B":
        X[5] = X[3]
    X.setflags(write=False)
    return X, perplexity


@functools.lru_cache(maxsize=None)
def host_affinities(name):
    """(P, beta) of the fp64 checker."""
    from multi_speaker_tts_amd import tsne as T
    X, perplexity = case(name)
    P, beta = T.affinities_host(X, perplexity)
    P.setflags(write=False)
    beta.setflags(write=False)
    return P, beta


def learning_rate(name):
    from multi_speaker_tts_amd import tsne as T
    return T.auto_learning_rate(case(name)[0].shape[0], 12.0)


@functools.lru_cache(maxsize=None)
def host_state(name, iters, seed=0):
    """The fp64 checker's (Y, update, gains) after `iters` iterations from random_init(n, seed), and its history."""
    from multi_speaker_tts_amd import tsne as T
    n = case(name)[0].shape[0]
    if iters > 300:                                        # one descent serves both stops (iteration 299 reports either way)
        state, hist = host_state(name, 300, seed)
        state, more = T.iterate_host(state, host_affinities(name)[0], 300, iters - 300, 12.0, 250, learning_rate(name))
        hist = hist + more
    else:
        state, hist = T.iterate_host(T.initial_state(T.random_init(n, seed)), host_affinities(name)[0], 0, iters, 12.0, 250, learning_rate(name))
    for a in state:
        a.setflags(write=False)
    return state, hist
