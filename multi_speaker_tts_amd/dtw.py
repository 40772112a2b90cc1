"""Dynamic time warping of feature sequences, batched, and the MCD-DTW figure of Tacotron2.Evaluate: `dtw_batch`, `mel_cepstra_batch` and
`mcd_dtw_batch` run on the GPU (csrc/dtw.hip: mstts_dtw_batch, mstts_mel_cepstra; fp32), `dtw_host`, `mel_cepstra_host` and `mcd_dtw_host`
are the fp64 statements of the same algorithms in NumPy - the checkers every device result is judged against (tests/test_gpu_dtw.py),
themselves pinned by hand-worked cases (tests/test_cpu_dtw.py).

The algorithm, the same in the checker and in the kernel.  Two sequences a [N, K] and b [M, K], float32.  Local distance d[i,j] =
sqrt(sum_k (a[i,k] - b[j,k])^2), from the differences themselves (not |a|^2 + |b|^2 - 2ab): identical frames give an exact 0.  D[0,0] =
d[0,0]; D[i,j] = min(D[i-1,j-1] + w d[i,j], D[i-1,j] + d[i,j], D[i,j-1] + d[i,j]), a neighbour that does not exist left out of the
minimum.  step="symmetric1": w = 1; step="symmetric2": w = 2, the Sakoe-Chiba form whose normaliser N + M does not depend on the path.
Ties go to the first minimum in the order diagonal, (i-1, j), (i, j-1).  L[i,j], the number of cells on the chosen path, is carried
through the same recurrence (L[0,0] = 1), so the path mean needs no backtrack.  Per pair: cost = D[N-1,M-1], length = L[N-1,M-1], mean =
cost / length, normalized = cost / (N + M) (meaningful for symmetric2) and, on request, path [length, 2], int32 cells (i, j) from (0,0) to
(N-1, M-1).  No band constraint, no other step pattern, no subsequence (open-ended) matching.

The cepstra.  A normalised mel row x in [-max_abs, max_abs]^n_mel goes back to decibels by the inverse of Audio._symmetric_normalize, dB =
(x + max_abs) (-min_level_db) / (2 max_abs) + min_level_db, and f_k = (1 / sqrt 2) sum_m dB_m sqrt(2 / n_mel) cos(pi k (m + 1/2) / n_mel), k =
1 ... n_cep: rows 1 ... n_cep of the orthonormal DCT-II (row 0, the energy, is left out) over sqrt 2.  With that scale the Euclidean
distance of two feature rows IS the frame's mel-cepstral distortion in dB, (10 / ln 10) sqrt(2 sum_k dc_k^2) on natural-log amplitudes.
The device multiplies x by the table `cepstra_table` (the slope folded in, fp64, rounded once); the constant of the dB map meets DCT rows
that sum to zero and is left out there.  These are cepstra of THIS model's 80-band mels, not WORLD mel-cepstra: the figure compares
checkpoints of this model with each other and is not comparable with other papers' tables.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import Hyper_Parameters as hp

MAX_LEN, MAX_K, MAX_CEP, MAX_MEL = 1024, 128, 40, 128
STEP_WEIGHT = {"symmetric1": 1.0, "symmetric2": 2.0}


def dtw_supported(n, m, k):
    """The device envelope: 1 <= n, m <= 1024 frames, 1 <= k <= 128 features (mstts_dtw_supported says the same)."""
    return 1 <= int(n) <= MAX_LEN and 1 <= int(m) <= MAX_LEN and 1 <= int(k) <= MAX_K


def _weight(step):
    if step not in STEP_WEIGHT:
        raise ValueError("step must be 'symmetric1' or 'symmetric2' (%r)" % (step,))
    return STEP_WEIGHT[step]


def _pair(a, b, dtype=np.float64):
    a, b = np.asarray(a, dtype), np.asarray(b, dtype)
    if a.ndim != 2 or b.ndim != 2:
        raise ValueError("a sequence must be [frames, features]")
    if a.shape[0] == 0 or b.shape[0] == 0 or a.shape[1] == 0:
        raise ValueError("empty sequence")
    if a.shape[1] != b.shape[1]:
        raise ValueError("the sequences have %d and %d features" % (a.shape[1], b.shape[1]))
    return a, b


def _root_sum(A, B):
    """sqrt(sum_k (A[..., k] - B[..., k])^2), the squares added for k ascending (one order for `distances_host` and `path_cost_host`)."""
    s = 0.0
    for k in range(A.shape[-1]):
        s = s + (A[..., k] - B[..., k]) ** 2
    return np.sqrt(s)


def distances_host(a, b):
    """d [N, M] of the module docstring, fp64."""
    a, b = _pair(a, b)
    return _root_sum(a[:, None, :], b[None, :, :])


def dtw_host(a, b, step="symmetric1", return_path=False):
    """The algorithm of the module docstring in fp64 -> {"cost", "length", "mean", "normalized"} and, with return_path, "path" [length, 2]
    int32.  One NumPy pass per anti-diagonal i + j = t, whose cells depend on diagonals t - 1 and t - 2 only."""
    w = _weight(step)
    d = distances_host(a, b)
    n, m = d.shape
    T = n + m - 1
    skew = np.zeros((T, n))                                    # skew[i + j, i] = d[i, j]
    ii, jj = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
    skew[ii + jj, ii] = d
    # diagonals as arrays over i, shifted by one so that row -1 reads +inf; cells outside a diagonal's range stay +inf
    D1, D2 = np.full(n + 1, np.inf), np.full(n + 1, np.inf)
    L1, L2 = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    codes = np.full((T, n), 3, np.uint8) if return_path else None
    for t in range(T):
        lo, hi = max(0, t - m + 1), min(n - 1, t)
        i = np.arange(lo, hi + 1)
        dt = skew[t, lo:hi + 1]
        D0, L0 = np.full(n + 1, np.inf), np.zeros(n + 1, np.int64)
        if t == 0:
            D0[1], L0[1] = dt[0], 1
        else:
            cand = np.stack([D2[i] + w * dt, D1[i] + dt, D1[i + 1] + dt])           # (i-1, j-1), (i-1, j), (i, j-1)
            pick = np.argmin(cand, axis=0)                                       # the first minimum
            D0[i + 1] = cand[pick, np.arange(i.size)]
            L0[i + 1] = np.stack([L2[i], L1[i], L1[i + 1]])[pick, np.arange(i.size)] + 1
            if return_path:
                codes[t, lo:hi + 1] = pick
        D2, L2, D1, L1 = D1, L1, D0, L0
    cost, length = float(D1[n]), int(L1[n])
    res = {"cost": cost, "length": length, "mean": cost / length, "normalized": cost / (n + m)}
    if return_path:
        path = np.zeros((length, 2), np.int32)
        pi, pj = n - 1, m - 1
        for pos in range(length - 1, -1, -1):
            path[pos] = (pi, pj)
            c = codes[pi + pj, pi]
            pi, pj = pi - (c != 2), pj - (c != 1)
        res["path"] = path
    return res


def path_cost_host(a, b, path, step="symmetric1"):
    """The cost of a GIVEN path [length, 2], recomputed in fp64: d of its first cell plus, per later cell, w d after a diagonal step and d
    after any other, added in path order."""
    w = _weight(step)
    a, b = _pair(a, b)
    path = np.asarray(path, np.int64)
    d = _root_sum(a[path[:, 0]], b[path[:, 1]])
    diagonal = np.concatenate([[False], (np.diff(path[:, 0]) == 1) & (np.diff(path[:, 1]) == 1)])
    return float(np.cumsum(np.where(diagonal, w * d, d))[-1])


def _dct_rows(n_cep, n_mel):
    k, mm = np.arange(1, n_cep + 1, dtype=np.float64)[:, None], np.arange(n_mel, dtype=np.float64)[None, :]
    return np.sqrt(0.5) * np.sqrt(2.0 / n_mel) * np.cos(np.pi * k * (mm + 0.5) / n_mel)


def _check_cep(n_cep, n_mel):
    if not 1 <= int(n_cep) < int(n_mel):
        raise ValueError("n_cep must lie in 1 ... n_mel - 1 (n_cep %d, n_mel %d)" % (n_cep, n_mel))


def cepstra_table(n_cep=13, n_mel=None, max_abs=None, min_level_db=-100):
    """The weights the device multiplies a normalised mel row by, [n_cep, n_mel] fp64: the DCT rows of the module docstring times the slope
    (-min_level_db) / (2 max_abs) of the inverse normalisation."""
    n_mel = hp.Sound.Mel_Dim if n_mel is None else int(n_mel)
    max_abs = hp.Sound.Max_Abs_Mel if max_abs is None else max_abs
    _check_cep(n_cep, n_mel)
    return _dct_rows(int(n_cep), n_mel) * (-float(min_level_db) / (2.0 * float(max_abs)))


def mel_cepstra_host(mel, n_cep=13, max_abs=None, min_level_db=-100):
    """mel [T, n_mel] (normalised as Audio.melspectrogram leaves it) -> the features f [T, n_cep] of the module docstring, fp64."""
    max_abs = hp.Sound.Max_Abs_Mel if max_abs is None else max_abs
    mel = np.asarray(mel, np.float64)
    if mel.ndim != 2 or mel.shape[0] == 0:
        raise ValueError("a mel must be [frames, bands] with at least one frame")
    _check_cep(n_cep, mel.shape[1])
    dB = (mel + max_abs) * (-float(min_level_db)) / (2.0 * max_abs) + float(min_level_db)
    return dB @ _dct_rows(int(n_cep), mel.shape[1]).T


def _figure(res, step):
    return res["mean"] if step == "symmetric1" else res["normalized"]


def mcd_dtw_host(mel_a, mel_b, n_cep=13, step="symmetric1"):
    """The MCD-DTW figure of two mels in dB, fp64: DTW on their cepstra, the path mean for symmetric1, cost / (N + M) for symmetric2."""
    _weight(step)
    return _figure(dtw_host(mel_cepstra_host(mel_a, n_cep), mel_cepstra_host(mel_b, n_cep), step), step)


# ---- device ----

def _checked_lists(a_List, b_List):
    if len(a_List) != len(b_List):
        raise ValueError("the two lists hold %d and %d sequences" % (len(a_List), len(b_List)))
    if len(a_List) == 0:
        raise ValueError("at least one pair is needed")
    pairs = [_pair(a, b, np.float32) for a, b in zip(a_List, b_List)]
    if len({a.shape[1] for a, _ in pairs}) != 1:
        raise ValueError("every pair must have the same number of features")
    return [a for a, _ in pairs], [b for _, b in pairs]


def _upload(parts, dev):
    """NumPy arrays -> device tensors of the same shapes and dtypes, through ONE host buffer and one copy (every part 16-byte aligned)."""
    import torch
    parts = [np.ascontiguousarray(p) for p in parts]
    starts = np.cumsum([0] + [(p.nbytes + 15) // 16 * 16 for p in parts])
    blob = np.zeros(int(starts[-1]), np.uint8)
    for p, s in zip(parts, starts):
        blob[s:s + p.nbytes] = p.reshape(-1).view(np.uint8)
    d = torch.from_numpy(blob).to(dev)
    return [d[int(s):int(s) + p.nbytes].view(torch.from_numpy(np.zeros(1, p.dtype)).dtype).view(p.shape) for p, s in zip(parts, starts)]


def _offsets(n_List, m_List):
    """The layout of a packed batch, as Audio._packed_offsets lays one out: the two int64 offset arrays (pairs + 1 entries, in frames), their
    stack [2, pairs + 1] for the device and the two ctypes arrays the entry point checks every shape from."""
    from .Audio import _offsets as cum
    a_off, b_off = cum(n_List), cum(m_List)
    hosts = tuple((ctypes.c_int64 * o.size)(*o.tolist()) for o in (a_off, b_off))
    return a_off, b_off, np.stack([a_off, b_off]), hosts


def dtw_launch(a, b, offs, hosts, k, step, cost, length, path=None):
    """mstts_dtw_batch on packed device tensors a [sum n, k], b [sum m, k], offs [2, pairs + 1] int64 (hosts: the same offsets as the two
    ctypes arrays of `_offsets`) into the device tensors cost (float32), length (int32) and, where given, path (int32 [sum (n + m - 1), 2]).
    Nothing synchronises; the workspace is allocated here and freed to torch's caching allocator behind the launch (stream-ordered)."""
    import torch
    from . import lib
    pairs = len(hosts[0]) - 1
    n_max = max(hosts[0][p + 1] - hosts[0][p] for p in range(pairs))
    m_max = max(hosts[1][p + 1] - hosts[1][p] for p in range(pairs))
    need = int(lib.load().mstts_dtw_ws_bytes(pairs, n_max, m_max, int(k), int(path is not None)))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=a.device)
    lib.call("mstts_dtw_batch", lib.ptr(a), lib.ptr(b), hosts[0], hosts[1], lib.ptr(offs), pairs, int(k), float(_weight(step)), lib.ptr(ws), need,
             lib.ptr(cost), lib.ptr(length), lib.ptr(path))


def _dtw_packed(a, b, offs, a_off, b_off, hosts, k, step, return_path, return_tensor):
    """The DTW of a packed device batch -> the result dict of `dtw_batch`; the results leave the device in one buffer, one copy."""
    import torch
    pairs = a_off.size - 1
    rows = int(a_off[-1] + b_off[-1] - pairs) if return_path else 0
    out = torch.full((2 * pairs + 2 * rows,), -1, dtype=torch.int32, device=a.device)         # cost bits | length | path slots
    cost, length = out[:pairs].view(torch.float32), out[pairs:2 * pairs]
    path = out[2 * pairs:].view(rows, 2) if return_path else None
    dtw_launch(a, b, offs, hosts, k, step, cost, length, path)
    slot = a_off[:-1] + b_off[:-1] - np.arange(pairs)
    sizes = np.diff(a_off) + np.diff(b_off)                                                 # n + m
    if return_tensor:
        lf, total = length.to(torch.float32), torch.as_tensor(sizes.astype(np.float32)).to(a.device)
        res = {"cost": cost, "length": length, "mean": cost / lf, "normalized": cost / total}
        if return_path:                      # (no read-back here: the whole slot, of which the first length[p] rows are the path)
            res["path"] = [path[int(s):int(s) + int(z) - 1] for s, z in zip(slot, sizes)]
        return res
    h = out.cpu().numpy()
    cost_h, length_h = h[:pairs].view(np.float32).copy(), h[pairs:2 * pairs].copy()
    res = {"cost": cost_h, "length": length_h, "mean": cost_h / length_h.astype(np.float32), "normalized": cost_h / sizes.astype(np.float32)}
    if return_path:
        ph = h[2 * pairs:].reshape(rows, 2)
        res["path"] = [ph[int(s):int(s) + int(l)].copy() for s, l in zip(slot, length_h)]
    return res


def _host_batch(a_List, b_List, step, return_path):
    each = [dtw_host(a, b, step, return_path) for a, b in zip(a_List, b_List)]
    res = {"cost": np.array([e["cost"] for e in each], np.float32), "length": np.array([e["length"] for e in each], np.int32),
           "mean": np.array([e["mean"] for e in each], np.float32), "normalized": np.array([e["normalized"] for e in each], np.float32)}
    if return_path:
        res["path"] = [e["path"] for e in each]
    return res


def dtw_batch(a_List, b_List, step="symmetric1", return_path=False, device="cuda", return_tensor=False):
    """DTW of the pairs (a_List[p] [n_p, k], b_List[p] [m_p, k]), ragged, in one device call: one upload (offsets and both packed lists in
    one buffer), one launch (two for k > 16), one download -> {"cost" float32 [pairs], "length" int32 [pairs], "mean" = cost / length,
    "normalized" = cost / (n + m), both float32} and, with return_path, "path": a list of int32 [length_p, 2] arrays.  return_tensor: device
    tensors and no read-back ("path" then holds each pair's whole slot [n + m - 1, 2], its first length_p rows the path, the rest -1).
    Outside the device envelope (`dtw_supported`) one line is printed and `dtw_host` runs.  ValueError: an empty sequence, pairs or lists that
    disagree in their number of features, lists of different lengths, no pair at all."""
    _weight(step)
    a_List, b_List = _checked_lists(a_List, b_List)
    k = a_List[0].shape[1]
    n_List, m_List = [a.shape[0] for a in a_List], [b.shape[0] for b in b_List]
    if not dtw_supported(max(n_List), max(m_List), k):
        print("dtw_batch: %d x %d frames of %d features is outside the device envelope - running on the host" % (max(n_List), max(m_List), k))
        return _host_batch(a_List, b_List, step, return_path)
    a_off, b_off, offs, hosts = _offsets(n_List, m_List)
    offs_d, a_d, b_d = _upload([offs, np.concatenate(a_List), np.concatenate(b_List)], device)
    return _dtw_packed(a_d, b_d, offs_d, a_off, b_off, hosts, k, step, return_path, return_tensor)


def _checked_mels(mel_List):
    mels = [np.asarray(m, np.float32) for m in mel_List]
    if not mels:
        raise ValueError("at least one mel is needed")
    if any(m.ndim != 2 or m.shape[0] == 0 for m in mels):
        raise ValueError("a mel must be [frames, bands] with at least one frame")
    if len({m.shape[1] for m in mels}) != 1:
        raise ValueError("every mel must have the same number of bands")
    return mels


def cepstra_supported(n_cep, n_mel):
    return 2 <= int(n_mel) <= MAX_MEL and 1 <= int(n_cep) <= min(MAX_CEP, int(n_mel) - 1)


def _cepstra_packed(mel, table, n_cep):
    """mstts_mel_cepstra on a packed device tensor mel [rows, n_mel] -> [rows, n_cep]."""
    import torch
    from . import lib
    out = torch.empty((mel.shape[0], int(n_cep)), dtype=torch.float32, device=mel.device)
    lib.call("mstts_mel_cepstra", lib.ptr(mel), int(mel.shape[0]), int(mel.shape[1]), int(n_cep), lib.ptr(table), lib.ptr(out))
    return out


def mel_cepstra_batch(mel_List, n_cep=13, device="cuda", return_tensor=False):
    """The features of `mel_cepstra_host` for a ragged list of mels [T_i, n_mel] on the GPU: one upload, one launch, one download -> a list of
    float32 [T_i, n_cep] arrays (return_tensor: views of the packed device result).  Outside 1 <= n_cep <= min(40, n_mel - 1), n_mel <= 128
    one line is printed and the host runs."""
    mels = _checked_mels(mel_List)
    n_mel = mels[0].shape[1]
    _check_cep(n_cep, n_mel)
    if not cepstra_supported(n_cep, n_mel):
        print("mel_cepstra_batch: n_cep %d of %d bands is outside the device envelope - running on the host" % (n_cep, n_mel))
        return [mel_cepstra_host(m, n_cep).astype(np.float32) for m in mels]
    from .Audio import _offsets as cum
    off = cum([m.shape[0] for m in mels])
    table, packed = _upload([cepstra_table(n_cep, n_mel).astype(np.float32), np.concatenate(mels)], device)
    out = _cepstra_packed(packed, table, n_cep)
    if not return_tensor:
        out = out.cpu().numpy()
    return [out[int(s):int(e)] for s, e in zip(off[:-1], off[1:])]


def mcd_dtw_batch(mel_a_List, mel_b_List, n_cep=13, step="symmetric1", device="cuda", return_path=False):
    """The MCD-DTW figure of the pairs (mel_a_List[p], mel_b_List[p]): one upload, the cepstra of every mel in one launch, the DTW on them
    where they lie (no host round trip in between), one download -> the dict of `dtw_batch` plus "mcd" float32 [pairs]: `mean` for
    symmetric1, `normalized` for symmetric2.  Outside the device envelopes one line is printed and the host runs."""
    _weight(step)
    if len(mel_a_List) != len(mel_b_List):
        raise ValueError("the two lists hold %d and %d mels" % (len(mel_a_List), len(mel_b_List)))
    A, B = _checked_mels(mel_a_List), _checked_mels(mel_b_List)
    n_mel = A[0].shape[1]
    if B[0].shape[1] != n_mel:
        raise ValueError("the mels have %d and %d bands" % (n_mel, B[0].shape[1]))
    _check_cep(n_cep, n_mel)
    n_List, m_List = [a.shape[0] for a in A], [b.shape[0] for b in B]
    if not (cepstra_supported(n_cep, n_mel) and dtw_supported(max(n_List), max(m_List), n_cep)):
        print("mcd_dtw_batch: %d x %d frames, n_cep %d of %d bands is outside the device envelope - running on the host"
              % (max(n_List), max(m_List), n_cep, n_mel))
        res = _host_batch([mel_cepstra_host(a, n_cep) for a in A], [mel_cepstra_host(b, n_cep) for b in B], step, return_path)
    else:
        a_off, b_off, offs, hosts = _offsets(n_List, m_List)
        offs_d, table, packed = _upload([offs, cepstra_table(n_cep, n_mel).astype(np.float32), np.concatenate(A + B)], device)
        cep = _cepstra_packed(packed, table, n_cep)
        res = _dtw_packed(cep[:int(a_off[-1])], cep[int(a_off[-1]):], offs_d, a_off, b_off, hosts, n_cep, step, return_path, False)
    res["mcd"] = _figure(res, step)
    return res
