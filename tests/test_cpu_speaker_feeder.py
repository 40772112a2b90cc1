"""Host side of the speaker encoder's corpus path, no GPU: the batch planner's rules (Speaker_Embedding/Feeder.py:47-101 as integers),
the table check, the embedding value, the loss-method switch, and the presence of the two new entry points in header, library and binding."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _index():
    """9 speakers; speakers 3 and 7 hold fewer than 3 files.  Lengths straddle the frame range (20, 24)."""
    from multi_speaker_tts_amd.speaker_feeder import BankIndex
    g = np.random.default_rng(0)
    counts = [5, 3, 4, 2, 6, 3, 3, 1, 4]
    lengths, files, n = [], [], 0
    for c in counts:
        files.append(np.arange(n, n + c))
        lengths += [int(v) for v in g.integers(1, 60, c)]
        n += c
    lengths[0:5] = [20, 22, 24, 19, 25]              # equal-length hits for every T in range, and both neighbours
    return BankIndex(np.asarray(lengths, np.int64), files), counts


def test_plan_batch_invariants():
    from multi_speaker_tts_amd.speaker_feeder import check_table, epoch_groups, plan_batch
    idx, counts = _index()
    P, S, fr = 3, 3, (20, 24)
    speaker_of = np.concatenate([np.full(c, k) for k, c in enumerate(counts)])
    seen_T, kinds = set(), set()
    for seed in range(200):
        rng = np.random.default_rng(seed)
        T, table = plan_batch(rng, idx, S, P, fr)
        seen_T.add(T)
        assert fr[0] <= T <= fr[1] and table.dtype == np.int32 and table.shape[1] == 4 and table.shape[0] % P == 0
        assert 2 <= table.shape[0] // P <= S
        check_table(table, idx.lengths, T)
        spk = speaker_of[table[:, 0]].reshape(-1, P)
        assert np.all(spk == spk[:, :1])                                           # speaker-major: P consecutive rows per speaker
        assert len(set(spk[:, 0])) == spk.shape[0]                                 # a speaker once per batch
        assert not set(spk[:, 0]) & {3, 7}                                         # under-stocked speakers never appear
        for rows in table.reshape(-1, P, 4):
            assert len(set(rows[:, 0])) == P                                       # no file twice within a speaker
        for f, src, dst, cnt in table:
            n = int(idx.lengths[f])
            if n > T:
                kinds.add("crop")
                assert dst == 0 and cnt == T and 0 <= src < n - T                  # exclusive upper bound: n - T is never drawn
            elif n == T:
                kinds.add("equal")
                assert (src, dst, cnt) == (0, 0, T)
            else:
                kinds.add("pad")
                assert src == 0 and cnt == n and 0 <= dst < T - n                  # exclusive upper bound: T - n is never drawn
    assert seen_T == set(range(fr[0], fr[1] + 1)) and kinds == {"crop", "equal", "pad"}
    # 7 eligible speakers in groups of 3: 3 + 3 + 1 - the singleton tail is dropped, every epoch
    for seed in range(200):
        groups = epoch_groups(np.random.default_rng(seed), idx, S, P)
        assert [len(g) for g in groups] == [3, 3]
        assert len(set(np.concatenate(groups))) == 6 and not set(np.concatenate(groups)) & {3, 7}
    # the same seed plans the same batch
    a, b = plan_batch(np.random.default_rng(5), idx, S, P, fr), plan_batch(np.random.default_rng(5), idx, S, P, fr)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    with pytest.raises(ValueError):
        epoch_groups(np.random.default_rng(0), idx, S, 6)                          # one speaker with 6 files: no batch of 2 speakers


def test_check_table_raises_on_each_kind_of_bad_row():
    from multi_speaker_tts_amd.speaker_feeder import check_table
    lengths, T = [10, 30], 20
    good = np.asarray([[0, 0, 5, 10], [1, 10, 0, 20], [1, 30, 20, 0]], np.int32)
    check_table(good, lengths, T)
    for bad in ([2, 0, 0, 1], [-1, 0, 0, 1], [0, -1, 0, 1], [0, 0, -1, 1], [0, 0, 0, -1], [0, 1, 0, 10], [1, 0, 1, 20], [1, 11, 0, 20],
                [0, 2 ** 31 - 1, 0, 2 ** 31 - 1]):
        t = good.copy()
        t[1] = bad
        with pytest.raises(ValueError):
            check_table(t, lengths, T)
    with pytest.raises(ValueError):
        check_table(np.zeros((3, 3), np.int32), lengths, T)


def test_embedding_value_is_the_reference_ratio():
    from multi_speaker_tts_amd.Speaker_Embedding import Embedding_Value
    g = np.random.default_rng(1)
    label_List = ["a", "b", "c", "a", "b", "a", "c", "c"]
    embedding_Array = g.normal(0, 1, (8, 16)).astype(np.float32)
    mean = {lab: np.mean([y for x, y in zip(label_List, embedding_Array) if x == lab], axis=0) for lab in set(label_List)}
    between = []
    for l1, m1 in mean.items():
        for l2, m2 in mean.items():
            if l1 == l2:
                continue
            between.append(np.sqrt(np.sum(np.power(m1 - m2, 2))))
    within = []
    for lab, e in zip(label_List, embedding_Array):
        within.append(np.sqrt(np.sum(np.power(e - mean[lab], 2))))
    assert Embedding_Value(embedding_Array, label_List) == pytest.approx(np.mean(between) / np.mean(within), rel=1e-6)


def test_engine_refuses_an_unknown_loss_calc_method(monkeypatch):
    from multi_speaker_tts_amd import Hyper_Parameters as hp
    from multi_speaker_tts_amd.speaker_trainer import SpeakerTrainEngine, loss_call
    assert hp.Speaker_Embedding.Train.Loss_Calc_Method == "Softmax"                # the shipped default
    assert loss_call() == loss_call("softmax") == "mstts_ge2e_loss_fwd_bwd" and loss_call("CONTRAST") == loss_call("Contrast") == "mstts_ge2e_contrast_fwd_bwd"
    with pytest.raises(ValueError, match="Unsupported loss calc method"):
        SpeakerTrainEngine(device="cpu", loss_method="Triplet")
    monkeypatch.setattr(hp.Speaker_Embedding.Train, "Loss_Calc_Method", "Hinge")
    with pytest.raises(ValueError, match="Unsupported loss calc method"):
        SpeakerTrainEngine(device="cpu")
    monkeypatch.setattr(hp.Speaker_Embedding.Train, "Loss_Calc_Method", "contrast")
    assert loss_call() == "mstts_ge2e_contrast_fwd_bwd"


def test_new_entry_points_in_header_library_and_binding():
    from multi_speaker_tts_amd import build, lib
    text = open(os.path.join(ROOT, "include", "mstts.h")).read()
    cdll = ctypes.CDLL(build.build())
    for name in ("mstts_mel_bank_gather", "mstts_ge2e_contrast_fwd_bwd"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(cdll, name) and name in lib.SIGNATURES
    assert lib.SIGNATURES["mstts_ge2e_contrast_fwd_bwd"] == lib.SIGNATURES["mstts_ge2e_loss_fwd_bwd"]
    assert "mel_bank.hip" in build.SOURCES
