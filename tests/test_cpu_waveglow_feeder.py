"""Host side of the WaveGlow trainer's corpus path, no GPU: the crop planner against WaveGlow.train_signal's draws, the row check, the new
entry point in header, library and binding with its host checks, the one copy of the frame body, which feeder Train() picks, and the
reference sizes against scipy."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_crop_plan_rules_and_train_signal_draws(monkeypatch):
    from multi_speaker_tts_amd import Feeder, WaveGlow as W
    from multi_speaker_tts_amd.waveglow_feeder import crop_plan
    L = 100
    lengths = np.asarray([40, 100, 101, 102, 250, 99, 1000, 101])
    files = [6, 0, 2, 2, 7, 4, 1, 3, 5, 6]
    for seed in range(40):
        table = crop_plan(np.random.default_rng(seed), lengths, files, L)
        assert table.dtype == np.int32 and table.shape == (len(files), 2) and table[:, 0].tolist() == files
        for f, start in table:
            n = lengths[f]
            assert (0 <= start < n - L) if n > L else start == 0
    assert len({tuple(crop_plan(np.random.default_rng(s), lengths, files, L)[:, 1]) for s in range(40)}) > 1
    # one seed: the draws train_signal makes for signals of the same lengths in the same order
    ramps = {"f%d" % f: np.arange(1, lengths[f] + 1, dtype=np.float64) for f in range(len(lengths))}
    monkeypatch.setattr(Feeder, "load_wav", lambda path, *a, **kw: ramps[path])
    rng = np.random.default_rng(17)
    table = crop_plan(np.random.default_rng(17), lengths, files, L)
    for f, start in table:
        sig = W.train_signal("f%d" % f, rng, L)                                    # ramp / peak * 0.99, cropped or padded
        want = np.zeros(L)
        piece = ramps["f%d" % f][start:start + L]
        want[:piece.shape[0]] = piece / lengths[f] * 0.99
        assert np.array_equal(sig, want.astype(np.float32)), (f, start)


def test_check_table():
    from multi_speaker_tts_amd.waveglow_feeder import check_table
    lengths = [50, 7, 300]
    check_table([[0, 0], [1, 6], [2, 299], [2, 0]], lengths)                       # start = len - 1 is a crop of one sample
    check_table(np.zeros((0, 2), np.int32), lengths)
    for bad in ([-1, 0], [3, 0], [1, -1], [1, 7], [0, 50], [2 ** 31 - 1, 0]):
        with pytest.raises(ValueError):
            check_table([[0, 0], bad, [2, 5]], lengths)
    with pytest.raises(ValueError):
        check_table([0, 1, 2], lengths)


def test_entry_point_in_header_library_and_binding_and_its_host_checks():
    """Every host check returns MSTTS_ERR_SHAPE with its text before anything is launched; the pointers are dummies that are never
    dereferenced, so this runs without a GPU."""
    from multi_speaker_tts_amd import build, lib
    assert "wg_crop.hip" in build.SOURCES
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mstts.h")).read(), flags=re.S)
    dll = ctypes.CDLL(build.build())
    for name in ("mstts_wg_crop_batch", "mstts_wg_crop_supported"):
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(dll, name) and name in lib.SIGNATURES
    assert len(lib.SIGNATURES["mstts_wg_crop_batch"][1]) == 24
    assert lib.ABI_VERSION == 5 and lib.load().mstts_abi_version() == 5            # additions only
    L = lib.load()
    one = ctypes.c_void_p(16)
    names = ("bank", "sig_off", "table", "phase", "window", "twiddle", "mel_basis", "mel_rng", "audio", "mel", "status")

    def batch(n_files=3, N=2, L_=8000, T=30, up=320, down=441, n_fft=2048, hop=200, win=800, **kw):
        p = {k: kw.get(k, one) for k in names}
        return L.mstts_wg_crop_batch(p["bank"], p["sig_off"], n_files, p["table"], N, L_, T, p["phase"], up, down, 0.97, p["window"], p["twiddle"],
                                     p["mel_basis"], p["mel_rng"], n_fft, hop, win, 80, 4.0, p["audio"], p["mel"], p["status"], None)
    ERR_SHAPE = -1
    for k in names:
        assert batch(**{k: None}) == ERR_SHAPE and b"null pointer" in L.mstts_last_error(), k
    for k in ("N", "L_", "T", "n_files"):
        assert batch(**{k: 0}) == ERR_SHAPE and b"N, L, T, n_files" in L.mstts_last_error(), k
    assert batch(N=2 ** 16, T=2 ** 15) == ERR_SHAPE and b"2^31" in L.mstts_last_error()
    assert batch(n_fft=1000) == ERR_SHAPE and b"power of two" in L.mstts_last_error()
    assert batch(n_fft=8192) == ERR_SHAPE and batch(win=4096) == ERR_SHAPE and batch(hop=0) == ERR_SHAPE
    assert batch(L_=1000) == ERR_SHAPE and b"726" in L.mstts_last_error() and b"reflect padding" in L.mstts_last_error()       # Lr = 726 <= 1024
    assert batch(T=29) == ERR_SHAPE and b"30 frames do not fit" in L.mstts_last_error()
    assert batch(up=640, down=882) == ERR_SHAPE and b"lowest terms" in L.mstts_last_error()
    assert batch(up=0) == ERR_SHAPE and batch(down=-1) == ERR_SHAPE
    assert batch(up=4099, down=4096) == ERR_SHAPE and b"not served" in L.mstts_last_error()
    assert L.mstts_wg_crop_supported(320, 441, 2048, 800) == 1 and L.mstts_wg_crop_supported(1, 1, 512, 400) == 1
    assert L.mstts_wg_crop_supported(2, 3, 4096, 4096) == 1                        # 32 KB + 16 KB of LDS
    assert L.mstts_wg_crop_supported(320, 441, 1000, 800) == 0 and L.mstts_wg_crop_supported(4099, 4096, 2048, 800) == 0
    assert L.mstts_wg_crop_supported(320, 441, 8192, 800) == 0


def test_the_frame_body_still_has_one_copy():
    csrc = os.path.join(ROOT, "multi_speaker_tts_amd", "csrc")
    header = open(os.path.join(csrc, "stft_frame.h")).read()
    assert "stft_frame_body(" in header and "fft_stockham_stages(" in header
    text = open(os.path.join(csrc, "wg_crop.hip")).read()
    assert '#include "stft_frame.h"' in text and "stft_frame_body(" in text
    assert "fft_stockham_stages" not in text and "fft_stages.h" not in text


class _Stub:
    """Stands in for the bank and for WaveGlowFeeder / WavFeeder on the GPU-less host."""
    made = []

    def __init__(self, *a, **kw):
        self.args, self.kw = a, kw
        _Stub.made.append(self)

    def Get_Train_Pattern(self):
        return "bank"

    def check_status(self):
        self.checked = getattr(self, "checked", 0) + 1


class _HostStub:
    made = []

    def __init__(self, *a, **kw):
        self.args, self.kw = a, kw
        _HostStub.made.append(self)

    def Get_Train_Pattern(self):
        return "host"


def test_train_picks_its_feeder(tmp_path, monkeypatch, capsys):
    from multi_speaker_tts_amd import Hyper_Parameters as hp
    from multi_speaker_tts_amd import WaveGlow as W
    from multi_speaker_tts_amd import waveglow_feeder as WF
    from multi_speaker_tts_amd.waveglow import WGDims
    tr = hp.WaveGlow.Train
    monkeypatch.setattr(tr, "Checkpoint_Save_Timing", 1000)
    monkeypatch.setattr(tr, "Pattern_Path", str(tmp_path))
    monkeypatch.setattr(WF, "bank_from_wavs", lambda paths, device: _Stub(paths, device=device))
    monkeypatch.setattr(WF, "WaveGlowFeeder", _Stub)
    monkeypatch.setattr(W, "WavFeeder", _HostStub)
    monkeypatch.delenv("MSTTS_WG_FEEDER", raising=False)
    _Stub.made.clear()
    _HostStub.made.clear()
    dims = WGDims(n_mel=8, flows=4, groups=8, early_every=2, early_size=2, up_k=16, up_stride=4, layers=3, ch=32, k=3)

    def trainer(**kw):
        m = W.WaveGlow(device="cpu", seed=3, dims=dims, **kw)
        m.fed = []

        def step(pattern=None):                                                     # the engine's step, stubbed
            m.fed.append(pattern)
            m.engine.global_step += 1
            return {"Global_Step": m.engine.global_step - 1, "Learning_Rate": 1e-3, "Log_S_Loss": 0.1, "Log_Det_W_Loss": 0.2, "Audio_Loss": 0.3, "Train_OP": None}
        monkeypatch.setattr(m, "Train_Step", step)
        return m

    for name in ("a.wav", "b.WAV", "c.txt"):
        open(tmp_path / name, "wb").close()
    wavs = [str(tmp_path / "a.wav").replace("\\", "/"), str(tmp_path / "b.WAV").replace("\\", "/")]

    # the default: the host feeder, as before
    m = trainer()
    m.Train(max_steps=2)
    assert m.feeder_mode == "host" and isinstance(m.feeder, _HostStub) and m.feeder.kw == {"device": "cpu"} and m.fed == ["host", "host"]
    assert not _Stub.made
    m.Train(max_steps=3, pattern_fn=lambda: "mine")                                # a pattern_fn still wins
    assert m.fed[-1] == "mine"

    # the argument, and the environment variable (the argument wins)
    for kw, env in (({"feeder": "device"}, None), ({}, "device"), ({"feeder": "device"}, "host")):
        _Stub.made.clear()
        if env is None:
            monkeypatch.delenv("MSTTS_WG_FEEDER", raising=False)
        else:
            monkeypatch.setenv("MSTTS_WG_FEEDER", env)
        m = trainer(**kw)
        m.Train(max_steps=4)
        bank, feeder = _Stub.made
        assert bank.args == (wavs,) and bank.kw == {"device": "cpu"}
        assert m.feeder is feeder and feeder.args == (bank,) and feeder.kw == {"seed": 3, "dims": dims} and feeder.checked == 4
        assert m.fed == ["bank"] * 4
    monkeypatch.setenv("MSTTS_WG_FEEDER", "device")
    assert trainer(feeder="host").feeder_mode == "host"
    monkeypatch.setenv("MSTTS_WG_FEEDER", "gpu")
    with pytest.raises(ValueError):
        trainer()
    monkeypatch.delenv("MSTTS_WG_FEEDER")
    with pytest.raises(ValueError):
        trainer(feeder="bank")

    # over the budget: the host feeder, and one line that names the budget
    def over(paths, device):
        raise WF.BankBudgetError("the corpus needs more than 9 bytes of device memory, the signal bank's budget is 8 bytes")
    monkeypatch.setattr(WF, "bank_from_wavs", over)
    capsys.readouterr()
    m = trainer(feeder="device")
    m.Train(max_steps=1)
    assert isinstance(m.feeder, _HostStub) and m.fed == ["host"]
    out = [line for line in capsys.readouterr().out.splitlines() if "WavFeeder" in line]
    assert len(out) == 1 and "budget" in out[0]

    # no wav files: WavFeeder's error
    monkeypatch.setattr(tr, "Pattern_Path", str(tmp_path / "nothing"))
    with pytest.raises(ValueError, match="no .wav files"):
        trainer(feeder="device").Train(max_steps=1)


def test_reference_sizes_against_scipy():
    from scipy.signal import resample_poly
    from multi_speaker_tts_amd import Audio, Hyper_Parameters as hp
    from multi_speaker_tts_amd import waveglow_feeder as WF
    up, down = Audio.resample_ratio(hp.WaveGlow.Export_Sample_Rate, hp.Sound.Sample_Rate)
    assert (up, down) == (320, 441) and hp.WaveGlow.Train.Max_Signal_Length == 8000
    assert resample_poly(np.zeros(8000), up, down).shape == (5805,)
    assert WF.crop_frames(8000, up, down, WF.hp_transform()) == (5805, 30)
    assert Audio.resample_taps(up, down) == 29 and Audio.resample_phase_table(up, down).shape == (320, 29)
    assert resample_poly(np.zeros(1000), up, down).shape == (726,)
