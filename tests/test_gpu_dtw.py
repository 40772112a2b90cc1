"""csrc/dtw.hip on the GPU against the fp64 statements of multi_speaker_tts_amd/dtw.py, and Tacotron2.Evaluate end to end.

The cost bound is derived, not measured (dtw_cases.cost_bound): relative (K + N + M + 8) 2^-24 of the fp64 cost.  `length` and `path` are
not compared with the host's on random data - a near-tie may legitimately fall the other way; the device's own path must be valid and its
cost, recomputed in fp64, no more than (1 + 2 eps) times the fp64 minimum.  On the integer cases the device must equal the host exactly.
Every figure is printed before it is asserted (run with -s to read them)."""
import functools
import os
import pickle

import numpy as np
import pytest
import torch

from multi_speaker_tts_amd import dtw as D
from dtw_cases import KATS, STEPS, assert_valid_path, cost_bound, pair

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 13), (1, 7, 13), (7, 1, 13), (65, 64, 13), (64, 65, 1), (96, 70, 13), (64, 129, 80)]
EDGE = [(1024, 1024, 13), (1024, 3, 16)]


@functools.lru_cache(maxsize=None)
def host_cost(n, m, k, step):
    return D.dtw_host(*pair(n, m, k), step)["cost"]


def check_pair(r, p, a, b, step, want):
    """Entry p of a device result against the fp64 minimum `want`."""
    n, m, k = a.shape[0], b.shape[0], a.shape[1]
    eps = cost_bound(n, m, k)
    cost, length, path = float(r["cost"][p]), int(r["length"][p]), r["path"][p]
    own = D.path_cost_host(a, b, path, step)
    print("dtw %s %4d x %4d x %3d: cost %.9g host %.9g, relative %.2e (bound %.2e); own path %d cells, its fp64 cost over the minimum %.2e"
          % (step, n, m, k, cost, want, abs(cost - want) / max(want, 1e-300), eps, length, own / max(want, 1e-300) - 1))
    assert abs(cost - want) <= eps * want
    assert_valid_path(path, n, m, length)
    assert own <= (1 + 2 * eps) * want
    assert r["mean"][p] == np.float32(cost) / np.float32(length) and r["normalized"][p] == np.float32(cost) / np.float32(n + m)


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("shape", SHAPES + EDGE, ids=lambda s: "x".join(map(str, s)))
def test_cost_and_path_against_the_host(dev, shape, step):
    a, b = pair(*shape)
    r = D.dtw_batch([a], [b], step, return_path=True, device=dev)
    assert r["cost"].dtype == np.float32 and r["length"].dtype == np.int32 and r["cost"].shape == r["length"].shape == (1,)
    check_pair(r, 0, a, b, step, host_cost(*shape, step))


@pytest.mark.parametrize("step", STEPS)
def test_integer_cases_equal_the_host_exactly(dev, step):
    names = sorted(KATS)
    r = D.dtw_batch([KATS[n][0] for n in names], [KATS[n][1] for n in names], step, return_path=True, device=dev)       # one ragged batch
    for p, name in enumerate(names):
        cost, path = KATS[name][2][step]
        assert r["cost"][p] == cost and r["length"][p] == len(path) and r["path"][p].tolist() == [list(c) for c in path], (name, step)
        h = D.dtw_host(KATS[name][0], KATS[name][1], step, return_path=True)
        assert np.array_equal(r["path"][p], h["path"])


def _raw(dev, a_List, b_List, step, want_path=True, guard=5):
    """mstts_dtw_batch on guarded buffers -> (cost bits, length, path rows, slot starts) as host arrays, the guards included."""
    n_List, m_List = [a.shape[0] for a in a_List], [b.shape[0] for b in b_List]
    a_off, b_off, offs, hosts = D._offsets(n_List, m_List)
    offs_d, a_d, b_d = D._upload([offs, np.concatenate(a_List), np.concatenate(b_List)], dev)
    pairs, rows = len(a_List), int(a_off[-1] + b_off[-1]) - len(a_List)
    cost = torch.full((pairs + guard,), -7.0, dtype=torch.float32, device=dev)
    length = torch.full((pairs + guard,), -7, dtype=torch.int32, device=dev)
    path = torch.full((rows + guard, 2), -7, dtype=torch.int32, device=dev)
    D.dtw_launch(a_d, b_d, offs_d, hosts, a_List[0].shape[1], step, cost[:pairs], length[:pairs], path[:rows] if want_path else None)
    torch.cuda.synchronize()
    return cost.cpu().numpy().view(np.int32), length.cpu().numpy(), path.cpu().numpy(), a_off[:-1] + b_off[:-1] - np.arange(pairs)


@pytest.mark.parametrize("k", [13, 80], ids=["fused", "two_pass"])
def test_ragged_batch_is_bit_equal_to_the_pairs_alone_and_guards_hold(dev, k):
    shapes = [(1, 1), (65, 64), (96, 70)]
    a_List, b_List = zip(*[pair(n, m, k) for n, m in shapes])
    for step in STEPS:
        cost, length, path, slot = _raw(dev, a_List, b_List, step)
        again = _raw(dev, a_List, b_List, step)
        assert all(np.array_equal(x, y) for x, y in zip((cost, length, path), again[:3]))                # the same bits on a second run
        assert np.all(cost[3:] == np.float32(-7).view(np.int32)) and np.all(length[3:] == -7)            # guards behind cost and length
        quiet = _raw(dev, a_List, b_List, step, want_path=False)
        assert np.array_equal(quiet[0], cost) and np.array_equal(quiet[1], length) and np.all(quiet[2] == -7)   # no path asked for: none written, the same cost and length bits
        for p, (n, m) in enumerate(shapes):
            c1, l1, p1, _ = _raw(dev, [a_List[p]], [b_List[p]], step)
            assert c1[0] == cost[p] and l1[0] == length[p]                                               # alone == inside the batch, bit for bit
            mine = path[slot[p]:slot[p] + n + m - 1]
            assert np.array_equal(mine[:length[p]], p1[:l1[0]])
            assert np.all(mine[length[p]:] == -7)                                                        # the rest of the pair's slot is not written
            assert_valid_path(mine[:length[p]].copy(), n, m, int(length[p]))
        assert np.all(path[slot[-1] + sum(shapes[-1]) - 1:] == -7)


def test_dict_forms_agree(dev):
    """return_path=False gives the cost and length bits of True; return_tensor gives device tensors with the same bits."""
    for shape in [(96, 70, 13), (64, 129, 80)]:
        a, b = pair(*shape)
        with_path = D.dtw_batch([a, b[:40]], [b, a[:33]], "symmetric2", return_path=True, device=dev)
        without = D.dtw_batch([a, b[:40]], [b, a[:33]], "symmetric2", device=dev)
        assert "path" not in without
        for key in ("cost", "length", "mean", "normalized"):
            assert np.array_equal(with_path[key], without[key]), key
        t = D.dtw_batch([a, b[:40]], [b, a[:33]], "symmetric2", return_path=True, device=dev, return_tensor=True)
        assert t["cost"].is_cuda and t["path"][0].shape == (shape[0] + shape[1] - 1, 2)
        for key in ("cost", "length"):
            assert np.array_equal(t[key].cpu().numpy(), with_path[key]), key
        for key in ("mean", "normalized"):
            assert np.allclose(t[key].cpu().numpy(), with_path[key], rtol=1e-6, atol=0), key
        for p in range(2):
            assert np.array_equal(t["path"][p].cpu().numpy()[:with_path["length"][p]], with_path["path"][p])


def _mels(frames, seed=0):
    g = np.random.default_rng(seed)
    return [np.clip(g.normal(0, 1.5, (f, 80)), -4, 4).astype(np.float32) for f in frames]


def test_cepstra_against_the_host(dev):
    """(80 + 4) 2^-24 max|f| absolute: an 80-term fp32 dot product with a table built in fp64 and rounded once."""
    mels = _mels([1, 64, 130])
    got = D.mel_cepstra_batch(mels, 13, device=dev)
    want = [D.mel_cepstra_host(m, 13) for m in mels]
    for g, w in zip(got, want):
        peak = float(np.abs(w).max())
        bound = (80 + 4) * 2.0 ** -24 * peak
        assert g.dtype == np.float32 and g.shape == w.shape
        err = float(np.abs(g - w).max())
        print("cepstra %3d frames: %.3e absolute (bound %.3e, peak %.2f)" % (w.shape[0], err, bound, peak))
        assert err <= bound
    wide, want40 = D.mel_cepstra_batch(mels[1:2], 40, device=dev)[0], D.mel_cepstra_host(mels[1], 40)
    assert np.abs(wide - want40).max() <= (80 + 4) * 2.0 ** -24 * np.abs(want40).max() and np.array_equal(wide[:, :13], got[1])


def test_mcd_dtw_batch(dev):
    A, B = _mels([50, 64, 3], seed=1), _mels([47, 90, 1], seed=2)
    for step in STEPS:
        r = D.mcd_dtw_batch(A, B, 13, step, device=dev, return_path=True)
        two = D.dtw_batch(D.mel_cepstra_batch(A, 13, device=dev), D.mel_cepstra_batch(B, 13, device=dev), step, return_path=True, device=dev)
        for key in ("cost", "length", "mean", "normalized"):
            assert np.array_equal(r[key], two[key]), key                       # no host round trip in between, the same bits
        assert all(np.array_equal(x, y) for x, y in zip(r["path"], two["path"]))
        assert np.array_equal(r["mcd"], r["mean"] if step == "symmetric1" else r["normalized"])
        for p in range(3):                                                      # the check the issue sets for Evaluate's figure: the cost bound
            want = D.mcd_dtw_host(A[p], B[p], 13, step)
            eps = cost_bound(A[p].shape[0], B[p].shape[0], 13)
            print("mcd %s pair %d: %.6f dB, host %.6f dB, relative %.2e (bound %.2e)" % (step, p, r["mcd"][p], want, abs(r["mcd"][p] - want) / want, eps))
            assert abs(r["mcd"][p] - want) <= eps * want
        same = D.mcd_dtw_batch(A, A, 13, step, device=dev)
        assert np.all(same["cost"] == 0.0) and np.all(same["mcd"] == 0.0)       # a mel against itself: exactly 0, along the diagonal
        assert np.array_equal(same["length"], [50, 64, 3])


def _write_patterns(root, n_files=5):
    """Five pattern pickles and a METADATA.PICKLE as Pattern_Generate leaves them."""
    from multi_speaker_tts_amd import Feeder as F, Hyper_Parameters as hp
    os.makedirs(root)
    g = np.random.default_rng(11)
    tokens = F.load_token_dict()
    md = {"Token_Index_Dict": tokens, "Spectrogram_Dim": hp.Sound.Spectrogram_Dim, "Mel_Dim": hp.Sound.Mel_Dim, "Frame_Shift": hp.Sound.Frame_Shift,
          "Frame_Length": hp.Sound.Frame_Length, "Sample_Rate": hp.Sound.Sample_Rate, "File_List": [], "Dataset_Dict": {}, "Mel_Length_Dict": {},
          "Token_Length_Dict": {}}
    mels = {}
    for i in range(n_files):
        name = "LJ.LJ001-%04d.PICKLE" % i
        token = g.integers(2, len(tokens), size=5 + 2 * i).astype(np.int32)
        mel = np.clip(g.normal(0, 1.5, (41 + 3 * i, hp.Sound.Mel_Dim)), -4, 4).astype(np.float32)
        with open(os.path.join(root, name), "wb") as f:
            pickle.dump({"Token": token, "Mel": mel, "Text": "X" * token.size, "Dataset": "LJ"}, f, protocol=2)
        md["File_List"].append(name)
        md["Dataset_Dict"][name], md["Mel_Length_Dict"][name], md["Token_Length_Dict"][name] = "LJ", mel.shape[0], token.size
        mels[name] = mel
    with open(os.path.join(root, hp.Train.Metadata_File.upper()), "wb") as f:
        pickle.dump(md, f, protocol=2)
    return mels


def test_tacotron2_evaluate_end_to_end(dev, tmp_path, monkeypatch, capsys):
    from multi_speaker_tts_amd import Hyper_Parameters as hp
    from multi_speaker_tts_amd.MSTTS_SV import Tacotron2
    from multi_speaker_tts_amd.params import Dims
    monkeypatch.setattr(hp, "Checkpoint_Path", str(tmp_path / "ckpt"))
    monkeypatch.setattr(hp, "Inference_Path", str(tmp_path / "inf"))
    monkeypatch.setattr(hp.Train, "Pattern_Path", str(tmp_path / "empty"))            # the feeder itself finds no pattern set
    monkeypatch.setattr(hp.Train, "Main_Train_Dataset_List", ["LJ"])
    root = str(tmp_path / "patterns")
    recorded = _write_patterns(root)
    max_inf = 12
    dims = Dims(emb=32, enc_conv_ch=32, enc_lstm=16, spk=256, prenet=16, dec_lstm=32, post_ch=16, bank_ch=8, proj1_ch=16, birnn=8, n_spec=20,
                spk_lstm=256, max_inf=max_inf)
    t = Tacotron2(is_Training=True, device=dev, dims=dims, allow_random_init=True)
    capsys.readouterr()
    res = t.Evaluate(batch_Size=2, seed=3, pattern_path=root, return_mels=True)
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert line.startswith("Global step: 0    Evaluation: 5 files    MCD-DTW: ") and "Duration ratio: " in line and "Not stopped: " in line
    assert set(res) == {"Files", "MCD", "Mean_MCD", "Frames", "Target_Frames", "Duration_Ratio", "Stopped", "Path_Length", "Global_Step", "Cut"}
    assert res["Files"] == sorted(recorded) and res["Global_Step"] == 0
    assert res["MCD"].dtype == np.float32 and res["MCD"].shape == (5,) and np.isfinite(res["MCD"]).all() and (res["MCD"] > 0).all()
    assert res["Mean_MCD"] == pytest.approx(float(res["MCD"].astype(np.float64).mean()))
    assert res["Stopped"].dtype == bool and res["Frames"].shape == res["Target_Frames"].shape == res["Path_Length"].shape == res["Stopped"].shape == (5,)
    assert np.array_equal(res["Target_Frames"], [recorded[f].shape[0] for f in res["Files"]])
    assert np.all(res["Frames"] >= 1) and np.all(res["Frames"] <= max_inf + 1)
    assert np.all(res["Frames"][~res["Stopped"]] == max_inf + 1) and np.all(res["Frames"][res["Stopped"]] <= max_inf)
    assert np.allclose(res["Duration_Ratio"], res["Frames"] / res["Target_Frames"])
    assert int(line.rsplit("Not stopped: ", 1)[1]) == int((~res["Stopped"]).sum())
    for i, name in enumerate(res["Files"]):
        cut = res["Cut"][i]
        assert cut.shape == (res["Frames"][i], 80) and max(cut.shape[0], recorded[name].shape[0]) <= res["Path_Length"][i]
        want = D.mcd_dtw_host(cut, recorded[name], 13, "symmetric1")
        eps = cost_bound(cut.shape[0], recorded[name].shape[0], 13)
        print("evaluate %s: %d frames against %d, MCD %.6f dB, host %.6f dB (relative %.2e)"
              % (name, cut.shape[0], recorded[name].shape[0], res["MCD"][i], want, abs(res["MCD"][i] - want) / want))
        assert abs(res["MCD"][i] - want) <= eps * want
    again = t.Evaluate(batch_Size=2, seed=3, pattern_path=root, return_mels=True)
    assert np.array_equal(again["MCD"], res["MCD"]) and all(np.array_equal(x, y) for x, y in zip(again["Cut"], res["Cut"]))     # the same seed: the same bits
    other = t.Evaluate(batch_Size=2, seed=4, pattern_path=root, return_mels=True)
    assert "Cut" in other and not all(np.array_equal(x, y) for x, y in zip(other["Cut"], res["Cut"]))                       # prenet dropout: the seed is part of the result
    named = t.Evaluate(file_List=res["Files"][3:1:-1], batch_Size=16, seed=3, pattern_path=root, step="symmetric2")
    assert named["Files"] == res["Files"][3:1:-1] and "Cut" not in named and np.isfinite(named["MCD"]).all()
    # the object still trains and synthesises afterwards
    r = t.Train_Step(t.feeder.Get_Train_Pattern(batch_Size=2, token_Length=9, mel_Length=200))
    assert r["Global_Step"] == 0 and np.isfinite(r["Loss"])
    mels = [np.clip(np.random.default_rng(i).normal(0, 1.5, (230, 80)), -4, 4).astype(np.float32) for i in range(2)]
    out = t.Inference(None, ["Please call Stella.", "Who knows?"], speaker_Mel_List=mels, export=False)
    assert out["Mel"].shape[0] == 2 and np.isfinite(out["Mel"]).all()
