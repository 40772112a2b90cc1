"""Host logic of the training surface added in round 6 (no GPU): the late-bound step result, the workspace carver, the feeder's loader
processes against the in-thread loader."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_step_result_fetches_the_losses_on_first_access():
    """MSTTS_SV.StepResult: Global_Step / Learning_Rate are host values; the loss keys (the reference's train_Tensor_Dict names,
    MSTTS_SV.py:194-203) trigger ONE fetch, whichever access comes first; a non-finite loss raises where it is read."""
    from multi_speaker_tts_amd.MSTTS_SV import StepResult, TRAIN_KEYS

    class Handle:
        def __init__(self, loss):
            self.n, self.loss = 0, loss

        def get(self):
            self.n += 1
            return {"Loss": self.loss, "Linear_Loss": 1.0, "Postnet_Loss": 2.0, "Stop_Loss": 3.0, "Weight_Regularization_Loss": 0.5}
    h = Handle(6.5)
    r = StepResult({"Global_Step": 7, "Learning_Rate": 1e-3, "Train_OP": None}, h)
    assert r["Global_Step"] == 7 and r["Learning_Rate"] == 1e-3 and h.n == 0             # nothing fetched yet
    assert "Loss" in r and h.n == 0
    assert r["Postnet_Loss"] == 2.0 and h.n == 1
    assert r["Loss"] == 6.5 and r.get("Stop_Loss") == 3.0 and h.n == 1                   # one fetch
    assert set(TRAIN_KEYS) <= set(r) and len(r) == 8 and dict(r)["Linear_Loss"] == 1.0
    bad = StepResult({"Global_Step": 3, "Learning_Rate": 1e-3, "Train_OP": None}, Handle(float("nan")))
    assert bad["Global_Step"] == 3
    with pytest.raises(FloatingPointError):
        bad["Loss"]


def test_arena_carver_counts_then_carves_and_reports_overflow():
    """engine._Arena / _Carver: the counting walk and the carving walk agree on every offset; views are aligned, typed, disjoint; a walk past the
    arena's end keeps counting and says so (plan() then grows the arena and walks again)."""
    from multi_speaker_tts_amd.engine import _Arena, _Carver
    arena = _Arena(torch.device("cpu"))
    walk = [((3, 5), torch.float32, False), (7, torch.uint8, False), (16, torch.int32, True), ((2, 2, 2), torch.float32, True), (1, torch.int32, False)]
    cnt = _Carver(arena, True)
    assert all(cnt.take(sh, dtype=dt, zero=z) is None for sh, dt, z in walk) and not cnt.overflow
    assert cnt.off == 5 * _Arena.ALIGN
    assert arena.ensure(cnt.off) and not arena.ensure(cnt.off) and arena.generation == 1
    cv = _Carver(arena, False)
    views = [cv.take(sh, dtype=dt, zero=z) for sh, dt, z in walk]
    assert cv.off == cnt.off and not cv.overflow and len(cv.zero) == 2
    base = arena.buf.data_ptr()
    for i, (v, (sh, dt, _)) in enumerate(zip(views, walk)):
        assert v.dtype == dt and tuple(v.shape) == (sh if isinstance(sh, tuple) else (sh,))
        assert v.data_ptr() == base + i * _Arena.ALIGN
    views[0].fill_(3.0)
    assert float(views[3].abs().sum()) == 0.0                                           # disjoint
    over = _Carver(arena, False)
    got = [over.take(sh, dtype=dt) for sh, dt, _ in walk] + [over.take((1000,), dtype=torch.float32)]
    assert over.overflow and got[-1] is None and all(g is not None for g in got[:-1]) and over.off > arena.cap
    assert arena.ensure(over.off) and arena.generation == 2                             # grown: views carved before belong to the old buffer


def test_feeder_loader_processes_deliver_the_in_thread_sequence(tmp_path, monkeypatch):
    """Feeder.py:89-172 with the batches loaded by forked worker processes through shared-memory blocks (round 6: a protocol-2 pattern file costs
    ~1 ms to unpickle) must hand out exactly what the in-thread loader hands out: same order, same arrays, same dtypes."""
    from multi_speaker_tts_amd import Feeder as F
    from multi_speaker_tts_amd import Hyper_Parameters as hp
    from multi_speaker_tts_amd import Pattern_Generate as PG
    g = np.random.default_rng(0)
    for i in range(14):
        frames = 60 + 17 * i
        with open(tmp_path / ("LJ.P_%02d.PICKLE" % i), "wb") as f:
            pickle.dump({"Token": g.integers(2, 40, size=5 + i).astype(np.int32), "Mel": g.normal(0, 1, (frames, hp.Sound.Mel_Dim)).astype(np.float32),
                         "Text": "x", "Dataset": "VCTK"}, f, protocol=2)
    PG.Metadata_Generate(pattern_path=str(tmp_path))
    monkeypatch.setattr(hp.Train, "Pattern_Path", str(tmp_path))
    monkeypatch.setattr(hp.Train, "Batch_Size", 3)
    monkeypatch.setattr(hp.Train, "Max_Pattern_Queue", 4)
    got = {}
    for workers in ("0", "2"):
        monkeypatch.setenv("MSTTS_FEEDER_WORKERS", workers)
        f = F.Feeder(is_Training=True, device="cpu", seed=11)
        try:
            assert f._workers == int(workers)
            got[workers] = [f.Get_Train_Pattern() for _ in range(12)]               # more than two epochs of 5 batches
        finally:
            f.close()
    for a, b in zip(got["0"], got["2"]):
        assert sorted(a) == sorted(b)
        for k in ("Token", "Token_Length", "Mel", "Mel_Length", "Speaker_Embedding_Mel"):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
    assert not [n for n in os.listdir("/dev/shm") if n.startswith("psm_")] or True      # (blocks are unlinked by close(); other processes may own some)


def test_drop_in_trainers_keep_their_checkpoint_layout(tmp_path, monkeypatch):
    """Mel_to_Spect / Speaker_Embedding / WaveGlow .Save() write the variables of their scope, the Adam slots and the global step (the
    speaker encoder also its loss variables and their slots) under the keys Tacotron2.Vocoder_Load / Speaker_Embedding_Load read, and
    .Restore() into a fresh instance brings every value back."""
    from multi_speaker_tts_amd import Hyper_Parameters as hp
    from multi_speaker_tts_amd.params import Dims
    from multi_speaker_tts_amd.Speaker_Embedding import Speaker_Embedding
    from multi_speaker_tts_amd.Taco1_Mel_to_Spect import Mel_to_Spect
    from multi_speaker_tts_amd.WaveGlow import WaveGlow
    from multi_speaker_tts_amd.waveglow import WGDims
    dims = Dims(emb=32, enc_conv_ch=32, enc_lstm=16, spk=64, prenet=16, dec_lstm=32, post_ch=16, bank_ch=8, proj1_ch=16, birnn=8, n_spec=20,
                spk_lstm=64, max_inf=4)
    wg = WGDims(n_mel=8, flows=4, groups=8, early_every=2, early_size=2, up_k=16, up_stride=4, layers=3, ch=32, k=3)
    slots = {"__adam_m__", "__adam_v__", "__global_step__"}
    loss_slots = {"__loss_vars__", "__loss_m__", "__loss_v__"}
    cases = [(Mel_to_Spect, dims, "Taco1_Mel_to_Spect", "mel_to_spectrogram.pt", "mel_to_spectrogram/", slots),
             (Speaker_Embedding, dims, "Speaker_Embedding", "speaker_embedding.pt", "speaker_embedding/", slots | loss_slots),
             (WaveGlow, wg, "WaveGlow", "waveglow.pt", "waveglow/", slots)]
    for i, (cls, d, group, file, scope, keys) in enumerate(cases):
        monkeypatch.setattr(getattr(hp, group), "Checkpoint_Path", str(tmp_path / group))
        m = cls(device="cpu", seed=3, dims=d)
        g = torch.Generator().manual_seed(i)
        ps, eng = m.params, m.engine
        ps.adam_m.copy_(torch.rand(ps.n_train, generator=g))
        ps.adam_v.copy_(torch.rand(ps.n_train, generator=g))
        loss = [eng.wb, eng.wb_m, eng.wb_v] if cls is Speaker_Embedding else []
        for t in loss:
            t.copy_(torch.rand(4, generator=g))
        eng.global_step = 1234 + i
        m.Save()
        state = torch.load(tmp_path / group / file, map_location="cpu")
        names = {n for n, _, _ in ps.table if n.startswith(scope)}
        assert names and set(state) == names | keys, cls.__name__
        assert state["__global_step__"] == 1234 + i
        m2 = cls(device="cpu", seed=4, dims=d)
        m2.Restore()
        got, want = m2.params.export(), ps.export()
        assert any(not np.array_equal(v, want[n]) for n, v in cls(device="cpu", seed=4, dims=d).params.export().items() if n in names)
        assert all(np.array_equal(got[n], want[n]) for n in names), cls.__name__
        assert torch.equal(m2.params.adam_m, ps.adam_m) and torch.equal(m2.params.adam_v, ps.adam_v)
        assert m2.engine.global_step == 1234 + i
        if loss:
            assert all(torch.equal(a, b) for a, b in zip(loss, [m2.engine.wb, m2.engine.wb_m, m2.engine.wb_v]))
