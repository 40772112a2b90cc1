"""The speaker encoder on a corpus: the mel-bank gather kernel, the "Contrast" loss kernel and train step against the fp64 restatement,
and the way from a directory of wavs through the pattern generator, the device feeder and Train() to Inference on wav paths."""
import os

import numpy as np
import pytest
import torch

from multi_speaker_tts_amd import lib
from multi_speaker_tts_amd.speaker_trainer import SpeakerTrainEngine
from oracle import model as OM, train as OT
from tests.ge2e_ref import between_gap, ge2e_contrast
from tests.helpers import dims_pair, rel_err, t2n

pytestmark = pytest.mark.gpu

GAP = 1e-3          # least distance between a row's two largest between-speaker logits: a flipped arg-max cannot hide behind a tolerance


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _gather_rows(lengths, T):
    """Every placement rule at its edges: crop at the first and last legal start, the equal-length file whole, short files at dst_start 0
    and T - len, and count = 0 rows."""
    rows = []
    for f, n in enumerate(lengths):
        if n > T:
            rows += [(f, 0, 0, T), (f, n - T, 0, T)]
        elif n == T:
            rows.append((f, 0, 0, T))
        else:
            rows += [(f, 0, 0, n), (f, 0, T - n, n)]
    rows += [(2, 0, 0, 0), (len(lengths) - 1, lengths[-1], T, 0)]
    return np.asarray(rows, np.int32)


@pytest.mark.parametrize("T", [24, 70])                 # 70: three frame blocks per row, the last one partial
@pytest.mark.parametrize("n_mel", [80, 5])              # 5: the scalar path
def test_mel_bank_gather_bit_exact(dev, n_mel, T):
    from multi_speaker_tts_amd.speaker_feeder import check_table
    lengths = [1, 23, 24, 25, 60, 3, 100]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    bank = np.random.default_rng(3).normal(0, 1, (int(off[-1]), n_mel)).astype(np.float32)
    table = _gather_rows(lengths, T)
    check_table(table, lengths, T)                      # only valid tables go to the GPU
    N = table.shape[0]
    want = np.zeros((N, T, n_mel), np.float32)
    for r, (f, src, dst, cnt) in enumerate(table):
        want[r, dst:dst + cnt] = bank[off[f] + src:off[f] + src + cnt]
    guard = 1024
    buf = torch.full((N * T * n_mel + guard,), float("nan"), device=dev)
    buf[N * T * n_mel:] = 12345.0
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    bank_d, off_d, table_d = torch.tensor(bank, device=dev), torch.tensor(off, device=dev), torch.tensor(table, device=dev)
    lib.call("mstts_mel_bank_gather", lib.ptr(bank_d), lib.ptr(off_d), len(lengths), lib.ptr(table_d), N, T, n_mel, lib.ptr(buf), lib.ptr(status))
    got = buf.cpu().numpy()
    assert np.array_equal(got[:N * T * n_mel].view(np.int32), want.reshape(-1).view(np.int32))
    assert np.all(got[N * T * n_mel:] == 12345.0)
    assert int(status.item()) == 0


@pytest.mark.parametrize("S,P,D,seed", [(4, 3, 16, 4), (7, 5, 100, 4), (32, 10, 256, 5)])
def test_ge2e_contrast_kernel(dev, S, P, D, seed):
    """mstts_ge2e_contrast_fwd_bwd against the fp64 restatement, at the bounds of the Softmax kernel's test."""
    N, ld = S * P, D + 8
    xh = np.random.default_rng(seed).normal(0, 1, (N, D)).astype(np.float32)
    x64 = torch.tensor(xh).double().requires_grad_(True)
    w64, b64 = torch.tensor(10.0, dtype=torch.float64, requires_grad=True), torch.tensor(-5.0, dtype=torch.float64, requires_grad=True)
    gap = between_gap(x64, P, w64, b64)
    print("between-logit gap", gap)
    assert gap >= GAP
    x = torch.zeros(N, ld, device=dev); x[:, :D] = torch.tensor(xh)
    wb = torch.tensor([10.0, -5.0, 0, 0], device=dev)
    out, dx = torch.zeros(4, device=dev), torch.zeros(N, ld, device=dev)
    ws = torch.zeros(int(lib.load().mstts_ge2e_ws_floats(N, D, S)), device=dev)
    lib.call("mstts_ge2e_contrast_fwd_bwd", lib.ptr(x), ld, S, P, D, lib.ptr(wb), lib.ptr(out), lib.ptr(dx), ld, lib.ptr(ws))
    loss = ge2e_contrast(x64, P, w64, b64)
    loss.backward()
    L, gw, gb = float(loss.detach()), float(w64.grad), float(b64.grad)
    print("loss", float(out[0]), L, "dx rel", rel_err(t2n(dx[:, :D]), t2n(x64.grad)), "dw", float(out[1]), gw, "db", float(out[2]), gb)
    assert abs(float(out[0]) - L) < 1e-4 * max(1.0, abs(L))
    assert rel_err(t2n(dx[:, :D]), t2n(x64.grad)) < 1e-3
    assert abs(float(out[1]) - gw) < 1e-4 * max(1e-3, abs(gw)) + 1e-6
    assert abs(float(out[2]) - gb) < 1e-4 * max(1e-3, abs(gb)) + 1e-6
    assert float(dx[:, D:].abs().max()) == 0.0


def test_speaker_train_step_contrast_parity(dev, monkeypatch):
    """Two trainer steps under Loss_Calc_Method "Contrast": loss, every gradient (the loss's weight AND bias), the parameters after TF-Adam -
    the quantities and bounds of test_speaker_train_step_parity, the oracle's step run with the Contrast restatement as its loss."""
    monkeypatch.setattr(OT, "ge2e_loss", ge2e_contrast)
    S, P, T = 4, 3, 12
    pd, od = dims_pair(spk=64, spk_lstm=64, n_mel=80)
    values = OM.init_params(od, 9)
    g = np.random.default_rng(10)
    for k in values:
        if k.startswith(OM.P_S) and k.endswith("bias"):
            values[k] = g.normal(0, 0.1, values[k].shape)
    N = S * P
    mel = np.clip(g.normal(0, 1.5, (N, T, od.n_mel)), -4, 4).astype(np.float32)
    eng = SpeakerTrainEngine(pd, device=dev, values=values, loss_method="Contrast")
    params, lv, opt = values, {"loss/weight": 10.0, "loss/bias": -5.0}, None
    for step in range(2):
        masks = {}
        for i in range(od.spk_lstm_n):
            masks["s_zc_%d" % i] = torch.tensor(g.integers(0, 2, (T, N, od.spk_lstm)).astype(np.uint8))
            masks["s_zh_%d" % i] = torch.tensor(g.integers(0, 2, (T, N, od.spk_lstm)).astype(np.uint8))
        before = dict(lv)
        params, lv, opt, sc, grads, out = OT.speaker_train_step(params, lv, opt, od, torch.tensor(mel), P, masks, step, return_grads=True)
        gap = between_gap(out[:, -1, :], P, before["loss/weight"], before["loss/bias"])
        print("step", step, "between-logit gap", gap)
        assert gap >= GAP
        w = eng.plan(N, T)
        eng.forward(torch.tensor(mel, device=dev), w, masks={k: v.numpy() for k, v in masks.items()})
        assert rel_err(t2n(w.x[-1]), t2n(out)) < 1e-3
        eng.loss_and_backward(w, P)
        assert abs(float(w.out3[0]) - sc["Loss"]) < 1e-4 * max(1.0, abs(sc["Loss"]))
        gexp = eng.params.export(grads=True)
        bad = [(k, rel_err(gexp[k], t2n(grads[k]))) for k in gexp if k.startswith(OM.P_S) and rel_err(gexp[k], t2n(grads[k])) > 5e-3]
        assert not bad, bad
        assert abs(float(w.out3[1]) - float(grads["loss/weight"])) < 5e-3 * abs(float(grads["loss/weight"])) + 1e-7
        assert abs(float(w.out3[2]) - float(grads["loss/bias"])) < 5e-3 * abs(float(grads["loss/bias"])) + 1e-7
        eng.adam_step(w)
        now = eng.params.export()
        bad = [(k, rel_err(now[k], t2n(params[k]))) for k in now if k.startswith(OM.P_S) and rel_err(now[k], t2n(params[k])) > 2e-3]
        assert not bad, bad
        assert abs(float(eng.wb[0]) - lv["loss/weight"]) < 1e-4 and abs(float(eng.wb[1]) - lv["loss/bias"]) < 1e-4
        assert abs(lv["loss/bias"] - before["loss/bias"]) > 1e-4 and abs(float(eng.wb[1]) - before["loss/bias"]) > 1e-4      # the bias moved


def _write_corpus(root):
    """VCTK-shaped tree: 4 speakers x 3 wavs of tones + noise at 16 kHz, 0.6 - 1.0 s; one wav of 1 100 samples (shorter than any T)."""
    from scipy.io import wavfile
    g = np.random.default_rng(21)
    paths, labels = [], []
    for k, f0 in enumerate((110.0, 160.0, 230.0, 330.0)):
        d = os.path.join(root, "p%03d" % (225 + k))
        os.makedirs(d)
        for u in range(3):
            n = 1100 if (k, u) == (2, 1) else int(g.integers(9600, 16001))
            t = np.arange(n) / 16000.0
            y = sum(a * np.sin(2 * np.pi * f0 * h * t + g.uniform(0, 6.28)) for h, a in ((1, 0.3), (2, 0.2), (3, 0.1), (5 + k, 0.1)))
            y = y + g.normal(0, 0.02, n)
            p = os.path.join(d, "p%03d_%03d.wav" % (225 + k, u + 1))
            wavfile.write(p, 16000, np.clip(y * 32767, -32767, 32767).astype(np.int16))
            paths.append(p); labels.append("p%03d" % (225 + k))
    return paths, labels


def test_speaker_corpus_end_to_end(dev, tmp_path, monkeypatch):
    from multi_speaker_tts_amd import Hyper_Parameters as hp
    from multi_speaker_tts_amd import Speaker_Embedding_Pattern_Generate as PG
    from multi_speaker_tts_amd import speaker_feeder as SF
    from multi_speaker_tts_amd.Speaker_Embedding import Embedding_Value, Speaker_Embedding
    from multi_speaker_tts_amd.params import Dims
    tr = hp.Speaker_Embedding.Train
    monkeypatch.setattr(hp.Speaker_Embedding, "Checkpoint_Path", str(tmp_path / "se"))
    monkeypatch.setattr(tr, "Pattern_Path", str(tmp_path / "patterns"))
    monkeypatch.setattr(tr, "Frame_Range", (20, 24))
    monkeypatch.setattr(tr, "Batch_Speaker", 4)
    monkeypatch.setattr(tr, "Batch_per_Speaker", 3)
    paths, labels = _write_corpus(str(tmp_path / "wav48"))
    written = PG.Pattern_Generate_VCTK(str(tmp_path / "wav48"), device=dev)
    md = PG.Metadata_Generate()
    assert len(written) == 12 and written[0] == "VCTK.0000000.pickle"
    assert set(md) == {"Sample_Rate", "Spectrogram_Dim", "Mel_Dim", "Frame_Shift", "Frame_Length", "Speaker_File_List_Dict", "Speaker_Dict", "Mel_Length_Dict"}
    assert sorted(md["Speaker_File_List_Dict"]) == ["VCTK.p225", "VCTK.p226", "VCTK.p227", "VCTK.p228"]
    assert all(len(v) == 3 for v in md["Speaker_File_List_Dict"].values()) and min(md["Mel_Length_Dict"].values()) == 1 + 1100 // 200
    assert os.path.exists(SF.metadata_path())

    dims = Dims(emb=32, enc_conv_ch=32, enc_lstm=16, spk=64, prenet=16, dec_lstm=32, post_ch=16, bank_ch=8, proj1_ch=16, birnn=8, n_spec=20,
                spk_lstm=64, max_inf=4)
    m = Speaker_Embedding(device=dev, dims=dims)
    losses, step = [], m.Train_Step
    monkeypatch.setattr(m, "Train_Step", lambda pattern=None: (lambda r: (losses.append(r["Loss"]), r)[1])(step(pattern)))
    m.Train(max_steps=30)
    assert m.feeder is not None and len(losses) == 30 and m.engine.global_step == 30
    print("losses", losses[:5], losses[-5:])
    assert np.all(np.isfinite(losses)) and np.mean(losses[-5:]) < np.mean(losses[:5])

    a, b = SF.SpeakerFeeder(m.feeder.bank, seed=7), SF.SpeakerFeeder(m.feeder.bank, seed=7)
    for _ in range(4):
        pa, pb = a.Get_Train_Pattern(), b.Get_Train_Pattern()
        assert pa["Mel"].shape == pb["Mel"].shape and pa["Mel"].shape[0] == 12 and 20 <= pa["Mel"].shape[1] <= 24
        assert torch.equal(pa["Mel"], pb["Mel"]) and pa["Batch_per_Speaker"] == 3
    a.check_status(); b.check_status()

    emb = m.Inference(paths, label_List=labels)
    assert emb.shape == (12, 64) and np.all(np.isfinite(emb))
    means = {lab: emb[[x == lab for x in labels]].mean(axis=0) for lab in set(labels)}
    between = np.mean([np.linalg.norm(means[p] - means[q]) for p in means for q in means if p != q])
    within = np.mean([np.linalg.norm(e - means[lab]) for e, lab in zip(emb, labels)])
    value = Embedding_Value(emb, labels)
    assert np.isfinite(value) and abs(value - between / within) < 1e-6 * abs(value) and abs(m.embedding_Value - value) == 0.0
