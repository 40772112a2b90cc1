"""Cases shared by tests/test_cpu_dtw.py and tests/test_gpu_dtw.py: the hand-worked DTW cases on 1-D integer features (every distance an
exact integer, so the host and the device must agree exactly, path included), the random pairs and the derived cost bound."""
import numpy as np


def col(values):
    return np.asarray(values, np.float32)[:, None]


def _diagonal(n):
    return [(i, i) for i in range(n)]


# name -> (a, b, {step: (cost, path)}), every cost and path worked by hand from the recurrence and the tie order of dtw.py's docstring.
#
# "doubled": a = [1, 4, 2], b = [1, 1, 4, 4, 2, 2].  d rows: [0 0 3 3 1 1], [3 3 0 0 2 2], [1 1 2 2 0 0].  D row 0: 0 0 3 6 7 8.  Row 1: 3,
#   then (1,1) = min(0+3, 0+3, 3+3) = 3, (1,2) = min(D01+0, D02+0, D11+0) = 0 by the diagonal, (1,3) = min(3, 6, D12+0 = 0) = 0 from the left,
#   2, 4.  Row 2: 4, 4, 2, (2,3) = 2, (2,4) = min(D13+0, D14+0, D23+0) = min(0, 2, 2) = 0 by the diagonal, (2,5) = min(2, 4, D24+0) = 0 from the
#   left.  Back from (2,5): (2,4), (1,3), (1,2), (0,1), (0,0): every frame of a meets its two copies, 2N cells.  Weight 2 multiplies zeros only.
# "two_three": a = [0, 3], b = [0, 1, 3], d = [0 1 3], [3 2 0].  Row 0: 0 1 4.  symmetric1: (1,0) = 3, (1,1) = min(0+2, 1+2, 3+2) = 2,
#   (1,2) = min(D01+0, D02+0, D11+0) = min(1, 4, 2) = 1 by the diagonal.  symmetric2: (1,1) = min(0+4, 1+2, 3+2) = 3 from above, (1,2) =
#   min(1, 4, 3) = 1.  "two_two" is its first two columns, where the weight changes the chosen cost AND the path: 2 by the diagonal, 3 around it.
# "all_tie": a = b = [5, 5, 5]: every d is 0, every candidate 0 - the diagonal is taken each time, 3 cells and not 5.
KATS = {
    "equal": (col([1, 4, 2, 7, 3]), col([1, 4, 2, 7, 3]), {s: (0.0, _diagonal(5)) for s in ("symmetric1", "symmetric2")}),
    "doubled": (col([1, 4, 2]), col([1, 1, 4, 4, 2, 2]),
                {s: (0.0, [(0, 0), (0, 1), (1, 2), (1, 3), (2, 4), (2, 5)]) for s in ("symmetric1", "symmetric2")}),
    "doubled5": (col([1, 4, 2, 7, 3]), col([1, 1, 4, 4, 2, 2, 7, 7, 3, 3]),
                 {s: (0.0, [(0, 0), (0, 1), (1, 2), (1, 3), (2, 4), (2, 5), (3, 6), (3, 7), (4, 8), (4, 9)]) for s in ("symmetric1", "symmetric2")}),
    "row": (col([2]), col([0, 1, 2, 3, 4, 5, 6]), {s: (13.0, [(0, j) for j in range(7)]) for s in ("symmetric1", "symmetric2")}),
    "column": (col([0, 1, 2, 3, 4, 5, 6]), col([2]), {s: (13.0, [(i, 0) for i in range(7)]) for s in ("symmetric1", "symmetric2")}),
    "two_three": (col([0, 3]), col([0, 1, 3]), {s: (1.0, [(0, 0), (0, 1), (1, 2)]) for s in ("symmetric1", "symmetric2")}),
    "two_two": (col([0, 3]), col([0, 1]), {"symmetric1": (2.0, [(0, 0), (1, 1)]), "symmetric2": (3.0, [(0, 0), (0, 1), (1, 1)])}),
    "all_tie": (col([5, 5, 5]), col([5, 5, 5]), {s: (0.0, _diagonal(3)) for s in ("symmetric1", "symmetric2")}),
}
STEPS = ("symmetric1", "symmetric2")


def pair(n, m, k, seed=0):
    """A random float32 pair a [n, k], b [m, k]."""
    g = np.random.default_rng([seed, n, m, k])
    return g.normal(size=(n, k)).astype(np.float32), g.normal(size=(m, k)).astype(np.float32)


def cost_bound(n, m, k):
    """The relative bound on an fp32 DTW cost against the fp64 one: every local distance carries at most k + 3 roundings (k differences
    folded into k fused multiply-adds and a square root, with room), a path sum of non-negative terms at most n + m more, and a relative
    perturbation eps of every path's cost moves the minimum over paths by at most eps."""
    return (k + n + m + 8) * 2.0 ** -24


def assert_valid_path(path, n, m, length):
    path = np.asarray(path)
    assert path.dtype == np.int32 and path.shape == (length, 2)
    assert tuple(path[0]) == (0, 0) and tuple(path[-1]) == (n - 1, m - 1)
    steps = {tuple(s) for s in np.diff(path, axis=0).tolist()}
    assert steps <= {(1, 1), (1, 0), (0, 1)}, steps
