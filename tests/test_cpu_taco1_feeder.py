"""Host side of the Taco1 vocoder trainer's corpus path, no GPU: the epoch planner's rules (Taco1_Mel_to_Spect/Feeder.py:46-64 as integers),
the host feeder against a restatement of the padding rule, the metadata and row checks, the new entry point in header, library and binding
with its host checks, and which feeder Train() picks."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_epoch_batches_rules():
    from multi_speaker_tts_amd.taco1_feeder import epoch_batches
    g = np.random.default_rng(0)
    n, B = 23, 5
    names = ["F%02d" % i for i in range(n)]
    lengths = g.integers(10, 40, n)
    lengths[[3, 11, 17]] = 25                                                      # ties: the sort must be stable
    run = np.argsort(lengths, kind="stable")
    for seed in range(50):
        groups = epoch_batches(np.random.default_rng(seed), names, lengths, B, True)
        assert sorted(np.concatenate(groups).tolist()) == list(range(n))           # every file exactly once
        assert sorted(len(x) for x in groups) == [3, 5, 5, 5, 5]                   # the last group of the sorted list is short
        for x in groups:                                                           # each group is one run of the length-sorted list
            k = int(np.nonzero(run == x[0])[0][0])
            assert k % B == 0 and np.array_equal(x, run[k:k + B])
            assert lengths[x].max() - lengths[x].min() == lengths[run[min(k + B, n) - 1]] - lengths[run[k]]
    orders = {tuple(int(x[0]) for x in epoch_batches(np.random.default_rng(s), names, lengths, B, True)) for s in range(50)}
    assert len(orders) > 1                                                         # the groups are shuffled
    rng = np.random.default_rng(4)
    first, second = epoch_batches(rng, names, lengths, B, False), epoch_batches(rng, names, lengths, B, False)
    for groups in (first, second):
        assert sorted(np.concatenate(groups).tolist()) == list(range(n)) and sorted(len(x) for x in groups) == [3, 5, 5, 5, 5]
    assert not np.array_equal(np.concatenate(first), np.concatenate(second))       # without sorting two epochs differ
    assert {frozenset(x.tolist()) for x in first} != {frozenset(x.tolist()) for x in second}       # ... in their membership, not only their order
    for sort in (True, False):
        a, b = epoch_batches(np.random.default_rng(9), names, lengths, B, sort), epoch_batches(np.random.default_rng(9), names, lengths, B, sort)
        assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))            # the same seed, the same plan
    with pytest.raises(ValueError):
        epoch_batches(np.random.default_rng(0), [], [], B, True)
    with pytest.raises(ValueError):
        epoch_batches(np.random.default_rng(0), names, lengths[:-1], B, True)


def _pattern_set(root, with_signal, n=7, seed=1):
    """n hand-made pattern files of widths 80 and 1025 (+ a 'Signal' of the matching length) and their metadata."""
    from multi_speaker_tts_amd import Hyper_Parameters as hp
    g = np.random.default_rng(seed)
    md = {"Spectrogram_Dim": hp.Sound.Spectrogram_Dim, "Mel_Dim": hp.Sound.Mel_Dim, "Frame_Shift": hp.Sound.Frame_Shift,
          "Frame_Length": hp.Sound.Frame_Length, "Sample_Rate": hp.Sound.Sample_Rate, "File_List": [], "Mel_Length_Dict": {}}
    if with_signal:
        md["Signal_Length_Dict"] = {}
    data = {}
    for i in range(n):
        T = int(g.integers(6, 15))
        d = {"Mel": g.normal(0, 1, (T, 80)).astype(np.float32), "Spectrogram": g.uniform(0, 1, (T, 1025)).astype(np.float32)}
        if with_signal:
            d["Signal"] = g.normal(0, 0.1, (T - 1) * 200 + int(g.integers(0, 200))).astype(np.float32)
        name = "P%02d.PICKLE" % i
        with open(os.path.join(root, name), "wb") as f:
            pickle.dump(d, f, protocol=2)
        md["File_List"].append(name)
        md["Mel_Length_Dict"][name] = T
        if with_signal:
            md["Signal_Length_Dict"][name] = d["Signal"].shape[0]
        data[name] = d
    with open(os.path.join(root, "METADATA.PICKLE"), "wb") as f:
        pickle.dump(md, f, protocol=2)
    return md, data


def test_pattern_feeder_is_the_padding_rule_bit_for_bit(tmp_path, monkeypatch):
    from multi_speaker_tts_amd import Hyper_Parameters as hp
    from multi_speaker_tts_amd import taco1_feeder as TF
    tr = hp.Taco1_Mel_to_Spect.Train
    monkeypatch.setattr(tr, "Pattern_Path", str(tmp_path))
    monkeypatch.setattr(tr, "Batch_Size", 3)
    monkeypatch.setattr(tr, "Max_Pattern_Queue", 2)
    md, data = _pattern_set(str(tmp_path), with_signal=False)
    names = md["File_List"]
    lengths = [md["Mel_Length_Dict"][n] for n in names]
    for sort in (True, False):
        monkeypatch.setattr(tr, "Pattern_Sorting_by_Length", sort)
        f = TF.PatternFeeder(seed=5)
        try:
            got = [f.Get_Train_Pattern() for _ in range(7)]                        # more than two epochs of 3 batches
            assert f.queue.maxsize == 2 and 1 <= f.max_queued <= 2 and f.queue.qsize() <= 2        # never more than Max_Pattern_Queue ahead
            assert f.thread.is_alive()
        finally:
            f.close()
        assert not f.thread.is_alive()
        rng = np.random.default_rng(5)
        plan = TF.epoch_batches(rng, names, lengths, 3, sort) + TF.epoch_batches(rng, names, lengths, 3, sort) + TF.epoch_batches(rng, names, lengths, 3, sort)
        for group, pat in zip(plan, got):
            assert sorted(pat) == ["Mel", "Spectrogram"]
            T = max(lengths[i] for i in group)
            for key, width in (("Mel", 80), ("Spectrogram", 1025)):
                want = np.zeros((len(group), T, width), np.float32)
                for r, i in enumerate(group):
                    want[r, :lengths[i]] = data[names[i]][key]
                assert pat[key].dtype == np.float32 and pat[key].shape == want.shape
                assert np.array_equal(pat[key].view(np.int32), want.view(np.int32)), (sort, key)
    # a producer that cannot read a file hands its error to the consumer instead of going quiet
    os.remove(tmp_path / names[0])
    f = TF.PatternFeeder(seed=5)
    try:
        with pytest.raises(OSError):
            for _ in range(4):
                f.Get_Train_Pattern()
    finally:
        f.close()


def test_check_metadata_and_check_files():
    from multi_speaker_tts_amd import Hyper_Parameters as hp
    from multi_speaker_tts_amd.taco1_feeder import check_files, check_metadata
    s = hp.Sound
    md = {"Spectrogram_Dim": s.Spectrogram_Dim, "Mel_Dim": s.Mel_Dim, "Frame_Shift": s.Frame_Shift, "Frame_Length": s.Frame_Length,
          "Sample_Rate": s.Sample_Rate, "File_List": [], "Mel_Length_Dict": {}}
    check_metadata(md)
    for key in ("Spectrogram_Dim", "Mel_Dim", "Frame_Shift", "Frame_Length", "Sample_Rate"):
        with pytest.raises(ValueError, match="not consistent"):
            check_metadata({**md, key: md[key] + 1})
    lengths, n_fft, hop = [4000, 1024, 1025, 7400], 2048, 200
    check_files([0, 2, 3, 3], lengths, 38, n_fft, hop)                             # 7400 samples: 38 frames
    check_files(np.asarray([2], np.int32), lengths, 6, n_fft, hop)
    for bad, T in (([0, 4], 38), ([0, -1], 38), ([0, 1], 38), ([0, 3], 37), ([2], 5), ([2 ** 31 - 1], 38)):
        with pytest.raises(ValueError):
            check_files(bad, lengths, T, n_fft, hop)
    with pytest.raises(ValueError):
        check_files(np.zeros((2, 2), np.int32), lengths, 38, n_fft, hop)


def test_entry_point_in_header_library_and_binding_and_its_host_checks():
    """A null bank, n_fft = 1000, N = 0 (and T = 0, n_files = 0, both outputs null, N * T = 2^31) return MSTTS_ERR_SHAPE with the error
    text set before anything is launched; the pointers are dummies that are never dereferenced, so this runs without a GPU."""
    from multi_speaker_tts_amd import build, lib
    assert "stft_bank.hip" in build.SOURCES and os.path.join(build.CSRC, "stft_frame.h") in build.HEADERS
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mstts.h")).read(), flags=re.S)
    assert re.search(r"\bmstts_stft_bank_batch\s*\(", text)
    assert hasattr(ctypes.CDLL(build.build()), "mstts_stft_bank_batch") and "mstts_stft_bank_batch" in lib.SIGNATURES
    assert len(lib.SIGNATURES["mstts_stft_bank_batch"][1]) == 21
    assert lib.ABI_VERSION == 5 and lib.load().mstts_abi_version() == 5            # additions only
    L = lib.load()
    one = ctypes.c_void_p(16)

    def batch(bank=one, n_files=3, N=2, T=10, n_fft=2048, win=800, mel=one, spec=one, status=one, hop=200):
        return L.mstts_stft_bank_batch(bank, one, n_files, one, N, T, 0.97, one, one, one, one, n_fft, hop, win, 80, 4.0, 20.0, mel, spec, status, None)
    ERR_SHAPE = -1
    assert batch(bank=None) == ERR_SHAPE and b"null pointer" in L.mstts_last_error()
    assert batch(n_fft=1000) == ERR_SHAPE and b"power of two" in L.mstts_last_error()
    assert batch(N=0) == ERR_SHAPE and b"N, T, n_files" in L.mstts_last_error()
    assert batch(T=0) == ERR_SHAPE and batch(n_files=0) == ERR_SHAPE and batch(hop=0) == ERR_SHAPE
    assert batch(mel=None, spec=None) == ERR_SHAPE and batch(status=None) == ERR_SHAPE
    assert batch(n_fft=8192) == ERR_SHAPE and batch(win=4096) == ERR_SHAPE
    assert batch(N=2 ** 16, T=2 ** 15) == ERR_SHAPE and b"2^31" in L.mstts_last_error()


def test_the_frame_body_has_one_copy():
    """The transform lives in csrc/stft_frame.h; both kernels call it and neither keeps stages of its own."""
    csrc = os.path.join(ROOT, "multi_speaker_tts_amd", "csrc")
    header = open(os.path.join(csrc, "stft_frame.h")).read()
    assert "stft_frame_body" in header and "fft_stockham_stages(" in header
    for name in ("audio.hip", "stft_bank.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "stft_frame.h"' in text and "stft_frame_body(" in text
        assert "fft_stockham_stages" not in text and "fft_stages.h" not in text, name


class _Stub:
    """Stands in for SignalBank / Taco1Feeder on the GPU-less host."""
    made = []

    def __init__(self, *a, **kw):
        self.args, self.kw = a, kw
        _Stub.made.append(self)

    @classmethod
    def from_patterns(cls, *a, **kw):
        return cls(*a, **kw)

    def Get_Train_Pattern(self):
        return {"Mel": "bank", "Spectrogram": "bank"}

    def check_status(self):
        self.checked = getattr(self, "checked", 0) + 1


def test_train_picks_its_feeder(tmp_path, monkeypatch, capsys):
    from multi_speaker_tts_amd import Hyper_Parameters as hp
    from multi_speaker_tts_amd import taco1_feeder as TF
    from multi_speaker_tts_amd.Taco1_Mel_to_Spect import Mel_to_Spect
    from multi_speaker_tts_amd.params import Dims
    tr = hp.Taco1_Mel_to_Spect.Train
    monkeypatch.setattr(tr, "Batch_Size", 3)
    monkeypatch.setattr(tr, "Max_Pattern_Queue", 2)
    monkeypatch.setattr(tr, "Checkpoint_Save_Timing", 1000)
    monkeypatch.setattr(tr, "Inference_Timing", 1000)
    monkeypatch.setattr(TF, "SignalBank", _Stub)
    monkeypatch.setattr(TF, "Taco1Feeder", _Stub)
    dims = Dims(emb=32, enc_conv_ch=32, enc_lstm=16, spk=64, prenet=16, dec_lstm=32, post_ch=16, bank_ch=8, proj1_ch=16, birnn=8, spk_lstm=64, max_inf=4)

    def trainer():
        m = Mel_to_Spect(device="cpu", seed=3, dims=dims)
        m.fed = []

        def step(pattern=None):                                                     # the engine's step, stubbed
            m.fed.append(pattern)
            m.engine.global_step += 1
            return {"Global_Step": m.engine.global_step - 1, "Learning_Rate": 1e-3, "Loss": 0.5, "Train_OP": None}
        monkeypatch.setattr(m, "Train_Step", step)
        return m

    # no metadata file: as before, Train_Step(None) (the synthetic pattern)
    monkeypatch.setattr(tr, "Pattern_Path", str(tmp_path / "nothing"))
    m = trainer()
    m.Train(max_steps=2)
    assert m.feeder is None and m.fed == [None, None]
    m.Train(max_steps=3, pattern_fn=lambda: "mine")
    assert m.fed[-1] == "mine"

    # a set without 'Signal' (what the reference's generator writes): the host feeder, and one line saying why
    os.makedirs(tmp_path / "plain")
    os.makedirs(tmp_path / "signal")
    md, data = _pattern_set(str(tmp_path / "plain"), with_signal=False)
    monkeypatch.setattr(tr, "Pattern_Path", str(tmp_path / "plain"))
    capsys.readouterr()
    m = trainer()
    try:
        m.Train(max_steps=3)
        assert isinstance(m.feeder, TF.PatternFeeder) and not _Stub.made
        out = [line for line in capsys.readouterr().out.splitlines() if "PatternFeeder" in line]
        assert len(out) == 1 and "7 of 7" in out[0] and "'Signal'" in out[0]
        assert len(m.fed) == 3 and all(p["Mel"].shape[2] == 80 and p["Spectrogram"].shape[:2] == p["Mel"].shape[:2] for p in m.fed)
        m.Train(max_steps=4, pattern_fn=lambda: "mine")                             # a pattern_fn still wins
        assert m.fed[-1] == "mine"
    finally:
        m.feeder.close()

    # a set with it: the bank and the device feeder, check_status after every step
    _pattern_set(str(tmp_path / "signal"), with_signal=True)
    monkeypatch.setattr(tr, "Pattern_Path", str(tmp_path / "signal"))
    m = trainer()
    m.Train(max_steps=4)
    bank, feeder = _Stub.made
    assert m.feeder is feeder and feeder.args == (bank,) and feeder.kw == {"seed": 3} and feeder.checked == 4
    assert m.fed == [{"Mel": "bank", "Spectrogram": "bank"}] * 4
    assert "PatternFeeder" not in capsys.readouterr().out

    # ... over its budget: the host feeder again, and the line names the budget
    def over(*a, **kw):
        raise TF.BankBudgetError("the corpus needs 9 bytes of device memory, the signal bank's budget is 8 bytes")
    monkeypatch.setattr(_Stub, "from_patterns", over)
    m = trainer()
    try:
        m.Train(max_steps=1)
        assert isinstance(m.feeder, TF.PatternFeeder)
        out = [line for line in capsys.readouterr().out.splitlines() if "PatternFeeder" in line]
        assert len(out) == 1 and "budget" in out[0]
    finally:
        m.feeder.close()
    _Stub.made.clear()


def test_signal_bank_budget_and_shapes():
    from multi_speaker_tts_amd import taco1_feeder as TF
    sigs = [np.arange(5, dtype=np.float32), np.arange(7, dtype=np.float32) + 10]
    bank = TF.SignalBank.from_signals(sigs, device="cpu", bank_bytes=48)
    assert bank.bank.tolist() == list(range(5)) + list(range(10, 17)) and bank.sig_off.tolist() == [0, 5, 12] and bank.lengths.tolist() == [5, 7]
    with pytest.raises(TF.BankBudgetError):
        TF.SignalBank.from_signals(sigs, device="cpu", bank_bytes=47)
    assert issubclass(TF.BankBudgetError, ValueError)
    with pytest.raises(ValueError):
        bank._fill(0, [np.zeros(4, np.float32)])
