"""The fp64 statements of multi_speaker_tts_amd/dtw.py (the checkers tests/test_gpu_dtw.py judges the device against): hand-worked cases,
path properties on random inputs, the cepstral MCD identity, the envelope, the refusals, the hosted half of the C ABI and the part of
Tacotron2.Evaluate that needs no engine."""
import math
import types

import numpy as np
import pytest

from multi_speaker_tts_amd import dtw as D
from dtw_cases import KATS, STEPS, assert_valid_path, pair


@pytest.mark.parametrize("name", sorted(KATS))
def test_hand_worked_cases(name):
    a, b, want = KATS[name]
    for step in STEPS:
        cost, path = want[step]
        r = D.dtw_host(a, b, step, return_path=True)
        assert r["cost"] == cost and r["path"].tolist() == [list(c) for c in path] and r["length"] == len(path), (step, r)
        assert r["mean"] == cost / len(path) and r["normalized"] == cost / (a.shape[0] + b.shape[0])
        assert D.path_cost_host(a, b, r["path"], step) == cost
        assert D.dtw_host(a, b, step)["cost"] == cost and "path" not in D.dtw_host(a, b, step)


def test_cases_say_what_the_issue_asks_of_them():
    """Doubling every frame costs nothing and takes 2N cells; a single row or column has one path, whose cost is the sum of the distances
    under both step patterns; the diagonal weight changes the chosen cost where a diagonal step competes; an all-way tie takes the diagonal."""
    assert len(KATS["doubled5"][2]["symmetric1"][1]) == 2 * 5
    a, b, _ = KATS["row"]
    assert D.dtw_host(a, b, "symmetric1")["cost"] == D.dtw_host(a, b, "symmetric2")["cost"] == float(D.distances_host(a, b).sum()) == 13.0
    assert KATS["two_two"][2]["symmetric1"][0] != KATS["two_two"][2]["symmetric2"][0]
    assert len(KATS["all_tie"][2]["symmetric1"][1]) == 3


def _naive(a, b, w):
    d = D.distances_host(a, b)
    n, m = d.shape
    table = np.full((n, m), np.inf)
    table[0, 0] = d[0, 0]
    for i in range(n):
        for j in range(m):
            if i or j:
                table[i, j] = min(table[i - 1, j - 1] + w * d[i, j] if i and j else np.inf, table[i - 1, j] + d[i, j] if i else np.inf,
                                  table[i, j - 1] + d[i, j] if j else np.inf)
    return table[-1, -1]


@pytest.mark.parametrize("shape", [(1, 1, 3), (9, 14, 2), (31, 17, 13), (40, 40, 1)])
def test_random_pairs_properties(shape):
    n, m, k = shape
    a, b = pair(n, m, k, seed=1)
    for step in STEPS:
        r = D.dtw_host(a, b, step, return_path=True)
        assert r["cost"] == _naive(a, b, D.STEP_WEIGHT[step])                  # the anti-diagonal sweep is the plain double loop
        assert_valid_path(r["path"], n, m, r["length"])                        # monotone, contiguous, length == len(path)
        assert D.path_cost_host(a, b, r["path"], step) == r["cost"]
        assert max(n, m) <= r["length"] <= n + m - 1
    assert D.dtw_host(a, b, "symmetric1")["cost"] == D.dtw_host(b, a, "symmetric1")["cost"]          # (the same sums in the same order, transposed)


def test_the_checker_is_quick_at_the_envelope_edge():
    """It is the reference of every GPU test: a 1024 x 1024 pair must not take long (no time is asserted: the sweep is vectorised over
    anti-diagonals, 2047 NumPy passes instead of a million Python iterations)."""
    a, b = pair(1024, 1024, 13)
    r = D.dtw_host(a, b, "symmetric2", return_path=True)
    assert_valid_path(r["path"], 1024, 1024, r["length"])
    assert D.path_cost_host(a, b, r["path"], "symmetric2") == r["cost"]


def test_distances_come_from_the_differences():
    a = np.array([[1e4, 1.0, -3.0], [2.0, 2.0, 2.0]], np.float32)
    d = D.distances_host(a, a)
    assert d[0, 0] == 0.0 and d[1, 1] == 0.0 and d[0, 1] == d[1, 0] == math.sqrt((1e4 - 2) ** 2 + 1 + 25)


def test_feature_distance_is_the_mel_cepstral_distortion():
    """Two ways to one number: the Euclidean distance of two feature rows, and (10 / ln 10) sqrt(2 sum_k dc_k^2) on the orthonormal DCT-II of
    the natural-log amplitudes, coefficients 1 ... 13 (the DCT written out here, not taken from dtw.py).  1e-12 relative."""
    from multi_speaker_tts_amd import Hyper_Parameters as hp
    g = np.random.default_rng(5)
    x = np.clip(g.normal(0, 1.5, (2, 80)), -4, 4)
    f = D.mel_cepstra_host(x, 13)
    assert f.shape == (2, 13) and f.dtype == np.float64
    ours = float(np.linalg.norm(f[0] - f[1]))
    dB = (x + hp.Sound.Max_Abs_Mel) * 100.0 / (2 * hp.Sound.Max_Abs_Mel) - 100.0          # the inverse of Audio._symmetric_normalize
    ln_amp = dB * math.log(10.0) / 20.0
    c = np.array([[math.sqrt(2.0 / 80) * sum(row[m] * math.cos(math.pi * k * (m + 0.5) / 80) for m in range(80)) for k in range(1, 14)]
                  for row in ln_amp])
    mcd = 10.0 / math.log(10.0) * math.sqrt(2.0 * float(np.sum((c[0] - c[1]) ** 2)))
    print("cepstra: feature distance %.12f, MCD %.12f dB" % (ours, mcd))
    assert abs(ours - mcd) <= 1e-12 * mcd
    # the table the device multiplies by says the same thing (the constant of the dB map meets rows that sum to zero)
    assert np.abs(x @ D.cepstra_table(13).T - f).max() < 1e-11
    assert np.abs(D.cepstra_table(13).sum(axis=1)).max() < 1e-12


def test_a_level_offset_leaves_the_features_unchanged():
    g = np.random.default_rng(6)
    x = np.clip(g.normal(0, 1.0, (7, 80)), -3, 3)
    f0, f1 = D.mel_cepstra_host(x, 13), D.mel_cepstra_host(x + 0.75, 13)          # the 0th coefficient, left out, carries it
    assert np.abs(f0 - f1).max() < 1e-11
    assert D.mcd_dtw_host(x, x) == 0.0 and D.mcd_dtw_host(x, x[::-1].copy(), step="symmetric2") > 0.0


def test_envelope_rule():
    assert D.dtw_supported(1, 1, 1) and D.dtw_supported(1024, 1024, 128)
    for bad in ((0, 5, 13), (5, 0, 13), (1025, 5, 13), (5, 1025, 13), (5, 5, 0), (5, 5, 129)):
        assert not D.dtw_supported(*bad), bad
    assert D.cepstra_supported(13, 80) and D.cepstra_supported(40, 80) and not D.cepstra_supported(41, 80) and not D.cepstra_supported(13, 129)


def test_refusals():
    a, b = pair(4, 5, 3)
    for fn in (lambda: D.dtw_host(a[:0], b), lambda: D.dtw_host(a, b[:, :2]), lambda: D.dtw_host(a, b, step="itakura"),
               lambda: D.dtw_batch([a[:0]], [b], device="cpu"), lambda: D.dtw_batch([a], [b[:, :2]], device="cpu"),
               lambda: D.dtw_batch([a, a], [b], device="cpu"), lambda: D.dtw_batch([], [], device="cpu"),
               lambda: D.dtw_batch([a, a[:, :2]], [b, b[:, :2]], device="cpu"), lambda: D.dtw_batch([a], [b], step="x", device="cpu"),
               lambda: D.path_cost_host(a, b, [[0, 0]], step="x"), lambda: D.mel_cepstra_host(np.zeros((3, 80)), 80),
               lambda: D.mel_cepstra_host(np.zeros((0, 80))), lambda: D.mcd_dtw_batch([np.zeros((3, 80))], [], device="cpu"),
               lambda: D.mcd_dtw_batch([np.zeros((3, 80))], [np.zeros((3, 40))], device="cpu"),
               lambda: D.mel_cepstra_batch([], device="cpu")):
        with pytest.raises(ValueError):
            fn()


def test_outside_the_envelope_the_host_runs(capsys):
    a, b = pair(3, 1025, 2)
    r = D.dtw_batch([a], [b], return_path=True, device="cpu")          # (never reaches a device)
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "outside the device envelope" in out
    h = D.dtw_host(a, b, return_path=True)
    assert r["cost"].dtype == np.float32 and r["cost"][0] == np.float32(h["cost"]) and r["length"][0] == h["length"]
    assert np.array_equal(r["path"][0], h["path"])


def test_c_abi_hosted_half():
    """mstts_dtw_supported and mstts_dtw_ws_bytes answer on a host without a device; the workspace is the diagonal-major planes: pairs x
    (max_n + max_m - 1) x max_n cells, a float each for k > 16, a direction byte each when a path is asked for."""
    from multi_speaker_tts_amd import lib
    L = lib.load()
    assert L.mstts_dtw_supported(1, 1, 1) == 1 and L.mstts_dtw_supported(1024, 1024, 128) == 1
    for bad in ((0, 5, 13), (1025, 5, 13), (5, 1025, 13), (5, 5, 0), (5, 5, 129), (-1, 5, 13)):
        assert L.mstts_dtw_supported(*bad) == 0, bad
    cells = 3 * (96 + 70 - 1) * 96
    assert cells == 47520
    assert L.mstts_dtw_ws_bytes(3, 96, 70, 13, 0) == 0 and L.mstts_dtw_ws_bytes(3, 96, 70, 13, 1) == cells
    assert L.mstts_dtw_ws_bytes(3, 96, 70, 80, 0) == 4 * cells and L.mstts_dtw_ws_bytes(3, 96, 70, 80, 1) == 5 * cells
    assert L.mstts_dtw_ws_bytes(1, 5, 3, 13, 1) == 48                      # 35 direction bytes, rounded up to 16
    assert L.mstts_dtw_ws_bytes(0, 96, 70, 13, 1) == 0 and L.mstts_dtw_ws_bytes(3, 1025, 70, 13, 1) == 0


def test_evaluate_without_files_says_so_and_returns_none(tmp_path, monkeypatch, capsys):
    """No METADATA.PICKLE and no file_List: one line, None - before any engine is touched (the method runs here on a bare object)."""
    from multi_speaker_tts_amd import Hyper_Parameters as hp
    from multi_speaker_tts_amd.MSTTS_SV import Tacotron2
    monkeypatch.setattr(hp.Train, "Pattern_Path", str(tmp_path / "nothing"))
    bare = types.SimpleNamespace(rank=0)
    assert Tacotron2.Evaluate(bare) is None
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "evaluation skipped" in out and "METADATA.PICKLE" in out
    assert Tacotron2.Evaluate(bare, pattern_path=str(tmp_path)) is None and "evaluation skipped" in capsys.readouterr().out
    assert Tacotron2.Evaluate(types.SimpleNamespace(rank=1)) is None and capsys.readouterr().out == ""
    with pytest.raises(ValueError):
        Tacotron2.Evaluate(bare, step="itakura")
    import inspect
    assert list(inspect.signature(Tacotron2.Evaluate).parameters)[1:9] == ["file_List", "max_files", "batch_Size", "seed", "n_cep", "step",
                                                                            "pattern_path", "max_steps"]
