"""What the device corpus feeders share (multi_speaker_tts_amd/device_bank.py), no GPU: the bank on device="cpu" under an explicit budget,
the row-check prelude, and the three planners' draws through `_Epochs` against tables recorded before the feeders were put on it."""
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "feeder_plans.json")


@pytest.mark.parametrize("width", [1, 5])
def test_device_bank_offsets_contents_and_budget(width):
    from multi_speaker_tts_amd.device_bank import BankBudgetError, DeviceBank, load_chunked
    lengths = [5, 7, 1, 4]
    g = np.random.default_rng(width)
    arrays = [g.normal(0, 1, (n,) if width == 1 else (n, width)).astype(np.float32) for n in lengths]
    need = sum(lengths) * width * 4
    bank = DeviceBank(lengths, width, "cpu", need, names="abcd")                   # an exact fit passes
    assert bank.bank.shape == ((17,) if width == 1 else (17, width)) and bank.bank.dtype.is_floating_point and bank.bank.element_size() == 4
    assert bank.offsets.tolist() == bank._offsets.tolist() == [0, 5, 12, 13, 17] and str(bank.offsets.dtype) == "torch.int64"
    assert bank.lengths.tolist() == lengths and bank.names == list("abcd") and bank.total == 17 and bank.bank_bytes == need
    bank._fill(0, arrays[:2])                                                       # two chunks, as load_chunked makes them
    bank._fill(2, arrays[2:])
    assert np.array_equal(bank.bank.numpy(), np.concatenate(arrays, axis=0))
    other = DeviceBank(lengths, width, "cpu", need)
    calls = []
    load_chunked(other, list(range(4)), lambda k: (calls.append(k), arrays[k])[1], workers=99, chunk=3)
    assert sorted(calls) == [0, 1, 2, 3] and np.array_equal(other.bank.numpy(), bank.bank.numpy()) and other.names is None
    with pytest.raises(BankBudgetError, match="%d bytes.*budget is %d bytes" % (need, need - 1)):
        DeviceBank(lengths, width, "cpu", need - 1)                                # one byte less raises
    assert issubclass(BankBudgetError, ValueError)
    tail = () if width == 1 else (width,)
    for wrong in ((4,) + tail, (5, width + 1), (5, 1) if width == 1 else (5,)):    # a row short; a column more; the other rank
        with pytest.raises(ValueError):
            bank._fill(0, [np.zeros(wrong, np.float32)])
    with pytest.raises(ValueError):
        bank._fill(1, [arrays[0]])                                                 # the right shape for another file
    for empty in ([], [0, 0]):
        with pytest.raises(ValueError, match="holds no"):
            DeviceBank(empty, width, "cpu", 1024)


def test_the_named_banks_are_device_banks():
    """The aliases the trainers, tools and tests use are the shared bank's own tensors, and an over-budget mel bank raises the same error."""
    import torch
    from multi_speaker_tts_amd.device_bank import BankBudgetError, DeviceBank
    from multi_speaker_tts_amd.speaker_feeder import MelBank
    from multi_speaker_tts_amd.taco1_feeder import SignalBank
    mels = {"a": [np.ones((3, 5), np.float32), np.full((2, 5), 2, np.float32)], "b": [np.full((4, 5), 3, np.float32)]}
    m = MelBank.from_mels(mels, device="cpu", bank_bytes=9 * 5 * 4)
    assert isinstance(m, DeviceBank) and m.frame_off is m.offsets and (m.total_frames, m.n_mel) == (9, 5) and m.bank.shape == (9, 5)
    assert m.speakers == ["a", "b"] and [f.tolist() for f in m.index.speaker_files] == [[0, 1], [2]] and m.index.lengths is m.lengths
    assert torch.equal(m.bank[:, 0], torch.tensor([1, 1, 1, 2, 2, 3, 3, 3, 3.0]))
    with pytest.raises(BankBudgetError):
        MelBank.from_mels(mels, device="cpu", bank_bytes=9 * 5 * 4 - 1)
    s = SignalBank.from_signals([np.arange(3), np.arange(4)], device="cpu", bank_bytes=28)
    assert isinstance(s, DeviceBank) and s.sig_off is s.offsets and s.total_samples == 7 and s.bank.shape == (7,)


def test_file_lengths():
    from multi_speaker_tts_amd.device_bank import file_lengths
    bad, n = file_lengths([0, 2, -1, 3, 2 ** 31 - 1, 1], [10, 20, 30])
    assert bad.tolist() == [False, False, True, True, True, False] and n[~bad].tolist() == [10, 30, 20] and n.dtype == np.int64
    bad, n = file_lengths(np.asarray([0, -1], np.int32), [])                       # no files: every row is bad, nothing is indexed
    assert bad.tolist() == [True, True] and n.tolist() == [0, 0]
    bad, n = file_lengths(np.zeros(0, np.int32), [4])
    assert bad.shape == n.shape == (0,)


def test_epochs_probe_and_refill():
    from multi_speaker_tts_amd.device_bank import _Epochs
    seen = []

    def draw(rng):
        seen.append(rng)
        return [int(rng.integers(0, 1000)), int(rng.integers(0, 1000))]
    e = _Epochs(9, draw)
    assert len(seen) == 1 and seen[0] is not e.rng                                 # the probe does not touch the seeded generator
    g = np.random.default_rng(9)
    assert [e.next() for _ in range(5)] == [int(g.integers(0, 1000)) for _ in range(6)][:5] and len(seen) == 4

    def none(rng):
        raise ValueError("no batch can be formed")
    with pytest.raises(ValueError):
        _Epochs(9, none)                                                           # raised at construction, by the probe


def test_planner_draws_are_frozen():
    """The first 6 planned tables of each feeder at a fixed seed, from the planning functions alone driven through `_Epochs`, equal the
    tables recorded (tests/golden/feeder_plans.json, with the synthetic corpus they were made on) from the three separate feeders."""
    from multi_speaker_tts_amd.device_bank import _Epochs
    from multi_speaker_tts_amd.speaker_feeder import BankIndex, epoch_groups, plan_batch
    from multi_speaker_tts_amd.taco1_feeder import epoch_batches
    from multi_speaker_tts_amd.waveglow_feeder import crop_plan
    with open(GOLDEN) as f:
        gold = json.load(f)
    seed, c = gold["corpus"]["seed"], gold["corpus"]

    s = c["speaker"]
    files, n = [], 0
    for k in s["counts"]:
        files.append(np.arange(n, n + k))
        n += k
    idx = BankIndex(np.asarray(s["lengths"], np.int64), files)
    S, P, fr = s["batch_speaker"], s["batch_per_speaker"], tuple(s["frame_range"])
    e = _Epochs(seed, lambda rng: epoch_groups(rng, idx, S, P))
    for want in gold["speaker"]:
        T, table = plan_batch(e.rng, idx, S, P, fr, speakers=e.next())
        assert T == want["T"] and table.dtype == np.int32 and table.tolist() == want["table"]

    t = c["taco1"]
    frames = np.asarray(t["frames"], np.int64)
    e = _Epochs(seed, lambda rng: epoch_batches(rng, range(len(frames)), frames, t["batch_size"], t["sort_by_length"]))
    for want in gold["taco1"]:
        group = e.next().astype(np.int32)
        assert int(frames[group].max()) == want["T"] and group.tolist() == want["table"]

    w = c["waveglow"]
    e = _Epochs(seed, lambda rng: epoch_batches(rng, range(len(w["lengths"])), w["lengths"], w["batch_size"], False))
    for want in gold["waveglow"]:
        assert crop_plan(e.rng, w["lengths"], e.next(), w["crop"]).tolist() == want["table"]
    assert len(gold["speaker"]) == len(gold["taco1"]) == len(gold["waveglow"]) == 6
