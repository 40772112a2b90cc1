"""The vocoder's config-3 mode (WaveGlowEngine.infer(arith="bf16")): the resident bf16 contraction and the three glue kernels op by op, the
engine stage by stage against tests/waveglow_bf16_ref.py (derived bounds, no trajectory), and the public surfaces."""
import ctypes as C

import numpy as np
import pytest
import torch

from multi_speaker_tts_amd import lib
from multi_speaker_tts_amd import waveglow as WG
from oracle import waveglow as OW
from tests import waveglow_bf16_ref as R

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _rn(dev, *shape, seed=0, scale=1.0):
    return torch.tensor(np.random.default_rng(seed).normal(0, scale, shape), dtype=torch.float32, device=dev)


def _nan(dev, *shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


# ------------------------------------------------------------------------------------------------------------ mstts_gemm_bf16_res
#        (batch, Lg, Cin, Cout, taps, dil) of a dilated 'same' convolution, or ("dense", M, N, K)
GEMM_CASES = [(2, 37, 32, 64, 3, 1),           # plain small case
              (3, 50, 32, 48, 3, 4),           # N not a multiple of 8
              (1, 20, 64, 32, 3, 16),          # taps almost all outside the sequence
              (2, 64, 32, 32, 5, 2),           # five taps
              (1, 300, 8, 264, 3, 128),        # smallest legal win_C; K = 24 below one K-tile; shift >= tile height; three N-tiles
              ("dense", 130, 136, 72)]         # one row and eight columns past a tile; K-tail
_gemm_memo = {}


def _gemm_case(dev, case):
    """Operands and the float64 reference of one case, computed once: (A, B, bias, M, N, K, lda, win, ref, mag), ref / mag WITHOUT bias."""
    if case not in _gemm_memo:
        if case[0] == "dense":
            _, M, N, K = case
            lda, win = K, None
            A = _rn(dev, M, K, seed=4).to(torch.bfloat16)
            Aref = A.double()
        else:
            n, Lg, Cin, N, taps, dil = case
            M, K, lda, win = n * Lg, taps * Cin, Cin, (Lg, Cin, (taps - 1) // 2, dil)
            A = _rn(dev, M, Cin, seed=4).to(torch.bfloat16)
            Aref = R.im2col(A.double(), n, Lg, taps, dil, (taps - 1) // 2)
        B = _rn(dev, N, K, seed=5, scale=0.2).to(torch.bfloat16)
        bias = _rn(dev, N, seed=6)
        _gemm_memo[case] = (A, B, bias, M, N, K, lda, win, Aref @ B.double().t(), Aref.abs() @ B.double().abs().t())
    return _gemm_memo[case]


@pytest.mark.parametrize("config", ["plain", "bias_accumulate_band", "split_k2", "twice"])
@pytest.mark.parametrize("case", GEMM_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_gemm_bf16_res(dev, case, config):
    """|C - ref64| <= 2 (K + 2) 2^-24 (|A| |B| + |bias| + |C0|): bf16 x bf16 products are exact in fp32, only the K + 2 additions round."""
    A, B, bias, M, N, K, lda, win, ref, mag = _gemm_case(dev, case)
    tol = 2 * (K + 2) * U
    if config == "plain":
        y = _nan(dev, M, N)
        lib.gemm_res(A, B, y, M, N, K, lda, K, N, win=win)
        err, bound = (y.double() - ref).abs(), tol * mag
    elif config == "bias_accumulate_band":
        ldc = N + 16
        base = _rn(dev, M, ldc, seed=7)
        y = base.clone()
        lib.gemm_res(A, B, y, M, N, K, lda, K, ldc, bias=bias, accumulate=True, win=win, c_off=8)
        assert torch.equal(y[:, :8].view(torch.int32), base[:, :8].view(torch.int32)) and torch.equal(y[:, 8 + N:].view(torch.int32), base[:, 8 + N:].view(torch.int32))
        err = (y[:, 8:8 + N].double() - (ref + bias.double() + base[:, 8:8 + N].double())).abs()
        bound = tol * (mag + bias.double().abs() + base[:, 8:8 + N].double().abs())
    elif config == "split_k2":
        y = torch.zeros(M, N, device=dev)
        lib.gemm_res(A, B, y, M, N, K, lda, K, N, bias=bias, split_k=2, win=win)
        err, bound = (y.double() - (ref + bias.double())).abs(), tol * (mag + bias.double().abs())
    else:
        y, y2 = _nan(dev, M, N), _nan(dev, M, N)
        lib.gemm_res(A, B, y, M, N, K, lda, K, N, bias=bias, win=win)
        lib.gemm_res(A, B, y2, M, N, K, lda, K, N, bias=bias, win=win)
        assert torch.equal(y.view(torch.int32), y2.view(torch.int32))
        err, bound = (y.double() - (ref + bias.double())).abs(), tol * (mag + bias.double().abs())
    assert bool(torch.isfinite(y).all())
    print("%s %s: worst error / bound %.3f" % (case, config, float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all()), float((err - bound).max())


@pytest.mark.parametrize("what", ["win_C=12", "K=20"])
def test_gemm_bf16_res_refuses(dev, what):
    """Shapes whose 8-element runs would straddle a tap or the end of K: mstts_gemm_bf16_res_supported says 0, the entry returns
    MSTTS_ERR_ALIGN, and nothing is launched (the NaN-filled output stays untouched)."""
    L = lib.load()
    if what == "win_C=12":
        M, N, K, lda, win = 40, 32, 36, 12, (20, 12, 1, 1)
    else:
        M, N, K, lda, win = 40, 32, 20, 24, None
    A, B, y = torch.ones(M, lda, device=dev, dtype=torch.bfloat16), torch.ones(N, 40, device=dev, dtype=torch.bfloat16), _nan(dev, M, N)
    assert L.mstts_gemm_bf16_res_supported(M, N, K, lda, 40, win[0] if win else 0, win[1] if win else 0) == 0
    d = lib.GemmResDesc()
    d.A, d.B, d.C = lib.ptr(A), lib.ptr(B), lib.ptr(y)
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc = M, N, K, lda, 40, N
    if win:
        d.win_T, d.win_C, d.win_pad, d.win_dil = win
    assert L.mstts_gemm_bf16_res(C.byref(d), lib.stream()) == -3 and L.mstts_last_error()          # MSTTS_ERR_ALIGN
    with pytest.raises(lib.MsttsError):
        lib.gemm_res(A, B, y, M, N, K, lda, 40, N, win=win)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())


# ------------------------------------------------------------------------------------------------------------ glue kernels
def test_round_bf16(dev):
    """Bit-equal to torch's round-to-nearest-even conversion: exact ties both ways, +-0, 1 +- 2^-9, large finite values below bf16 overflow."""
    edge = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 0.0, -0.0, 1 + 2.0 ** -9, 1 - 2.0 ** -9, 1 - 2.0 ** -10,
            3.3e38, -3.3e38, 3.389e38, 3.38e38, 1e-38, -1e-30, 65504.0]
    x = torch.cat([torch.tensor(edge, dtype=torch.float32, device=dev), _rn(dev, 4096 + 4, seed=1, scale=3.0)])
    assert x.numel() % 4 == 0
    y = torch.full((x.numel(),), float("nan"), dtype=torch.bfloat16, device=dev)
    lib.call("mstts_round_bf16", lib.ptr(x), lib.ptr(y), x.numel())
    ref = x.to(torch.bfloat16)
    assert bool(torch.isfinite(ref.float()).all()) and torch.equal(y.view(torch.int16), ref.view(torch.int16))
    assert y[:2].float().tolist() == [1.0, 1 + 2.0 ** -6]             # ties to even: down, then up


def test_gate_bf16(dev):
    """z bit-equal to mstts_wg_gate's on the same input, zb == bf(z) bit for bit.  Also the yardstick of the engine-level z check: the existing
    fp32 kernel's own error against the float64 gate on this input is printed and must stay within waveglow_bf16_ref.GATE_KERNEL_REL (the
    engine check allows twice that)."""
    for rows, Cc, lda in [(7, 8, 16), (130, 32, 80), (1000, 512, 1024)]:
        a = _rn(dev, rows, lda, seed=rows, scale=2.5)
        z0, z1, zb = _nan(dev, rows, Cc), _nan(dev, rows, Cc), _nan(dev, rows, Cc, dtype=torch.bfloat16)
        lib.call("mstts_wg_gate", lib.ptr(a), lda, lib.ptr(z0), rows, Cc)
        lib.call("mstts_wg_gate_bf16", lib.ptr(a), lda, lib.ptr(z1), lib.ptr(zb), rows, Cc)
        assert torch.equal(z0.view(torch.int32), z1.view(torch.int32)) and bool(torch.isfinite(z0).all())
        assert torch.equal(zb.view(torch.int16), z1.to(torch.bfloat16).view(torch.int16))
        z64 = R.gate64(a[:, :2 * Cc])
        rel = float(((z0.double() - z64).abs() / z64.abs().clamp_min(1e-30)).max())
        print("mstts_wg_gate against the float64 gate, %d x %d: worst relative error %.3e" % (rows, Cc, rel))
        assert rel <= R.GATE_KERNEL_REL, rel


@pytest.mark.parametrize("rows", [7, 130])
@pytest.mark.parametrize("Cc", [8, 32])
def test_res_skip_bf16(dev, rows, Cc):
    """out bit-equal to mstts_wg_res_skip's for first / last in all four combinations; xb == bf(z + rs[:, :C]) with the host's float32 add."""
    z = _rn(dev, rows, Cc, seed=2)
    for last in (0, 1):
        rs = _rn(dev, rows, Cc if last else 2 * Cc, seed=3 + last)
        for first in (0, 1):
            o0 = _rn(dev, rows, Cc, seed=5) if not first else _nan(dev, rows, Cc)
            o1 = o0.clone()
            x, xb = _nan(dev, rows, Cc), _nan(dev, rows, Cc, dtype=torch.bfloat16)
            lib.call("mstts_wg_res_skip", lib.ptr(z), lib.ptr(rs), lib.ptr(x), lib.ptr(o0), rows, Cc, last, first)
            lib.call("mstts_wg_res_skip_bf16", lib.ptr(z), lib.ptr(rs), lib.ptr(xb), lib.ptr(o1), rows, Cc, last, first)
            assert torch.equal(o0.view(torch.int32), o1.view(torch.int32)) and bool(torch.isfinite(o1).all())
            if last:
                assert bool(torch.isnan(xb.float()).all())
            else:
                ref = (z.cpu() + rs.cpu()[:, :Cc]).to(torch.bfloat16)
                assert torch.equal(xb.cpu().view(torch.int16), ref.view(torch.int16))
                assert torch.equal(x.cpu().to(torch.bfloat16).view(torch.int16), ref.view(torch.int16))


# ------------------------------------------------------------------------------------------------------------ engine, stage by stage
# CFGS[0] / CFGS[1] of tests/test_gpu_waveglow.py (copied by value), a ch = 20 variant that mstts_gemm_bf16_res refuses, one flow at the reference widths
CFG0 = dict(n_mel=8, flows=4, groups=8, early_every=2, early_size=2, up_k=16, up_stride=4, layers=3, ch=32, k=3)
CFG1 = dict(n_mel=16, flows=12, groups=8, early_every=4, early_size=2, up_k=32, up_stride=8, layers=4, ch=64, k=3)
CFG_CH20 = dict(CFG0, ch=20)
CFG_REF1 = dict(n_mel=80, flows=1, groups=8, early_every=4, early_size=2, up_k=1024, up_stride=256, layers=8, ch=512, k=3)
ENGINE_CASES = {"cfg0": (CFG0, 2, 5), "cfg1": (CFG1, 3, 6), "ch20": (CFG_CH20, 2, 5), "ref_width_160_rows": (CFG_REF1, 1, 2), "ref_width_832_rows": (CFG_REF1, 2, 10)}
_engines = {}


def _engine(dev, cfg):
    key = tuple(sorted(cfg.items()))
    if key not in _engines:
        od = OW.WGDims(**cfg)
        values = OW.init_params(od, seed=3)
        for k in values:                     # (as tests/test_gpu_waveglow.py: a trained network keeps the couplings' log-scales small)
            if cfg["ch"] == 512 and k.endswith("wavenet/conv1d/kernel"):
                values[k] = np.asarray(values[k]) * 0.05
        _engines[key] = (od, WG.WaveGlowEngine(WG.WGDims(**cfg), device=dev, values=values))
    return _engines[key]


def _inputs(od, N, T):
    mel = np.clip(np.random.default_rng(8).normal(0, 1.5, (N, T, od.n_mel)), -4, 4).astype(np.float32)
    L = (T - 1) * od.up_stride + od.up_k
    return mel, OW.make_noise(od, N, L // od.groups, seed=9), L


@pytest.mark.parametrize("resident", ["1", "0"])
@pytest.mark.parametrize("name", list(ENGINE_CASES))
def test_engine_stages(dev, monkeypatch, name, resident):
    """Every stage of one infer(arith="bf16") call judged from what the engine stored (waveglow_bf16_ref.check: contraction bound
    2 (K + 2) 2^-24 (|A| |B| + |bias| + |C0|); z to twice the fp32 gate kernel's own measured accuracy, GATE_KERNEL_REL = 2.8e-7 relative;
    zb / xb exact) - with the resident contraction and, MSTTS_WG_BF16_RESIDENT=0, on mstts_gemm_bf16 over the fp32 buffers."""
    cfg, N, T = ENGINE_CASES[name]
    od, eng = _engine(dev, cfg)
    mel, noise, L = _inputs(od, N, T)
    monkeypatch.setenv("MSTTS_WG_BF16_RESIDENT", resident)
    stages = {}
    wav = eng.infer(mel, noise=noise, sigma=0.8, arith="bf16", stages=stages)
    assert wav.shape == (N, L) and bool(torch.isfinite(wav).all())
    took = stages["resident"]
    if resident == "0":
        assert took == {"cond": False, "conv": False, "res_skip": False}
    elif name == "ch20":
        assert took == {"cond": True, "conv": False, "res_skip": False}             # K = ch = 20: the fallback
    else:
        assert took == {"cond": True, "conv": True, "res_skip": True}
    assert set(stages[(0, 0)]) == {"pre", "z", "zb", "rs", "xb"} and {"melg_b", "x", "ls_b"} <= set(stages[0])
    R.check(stages, eng, mel, noise, sigma=0.8, wav=wav)


@pytest.mark.parametrize("name", ["cfg0", "ref_width_832_rows"])
def test_engine_mode_properties(dev, monkeypatch, name):
    """One seed -> the same bits twice; the bf16 waveform is finite and NOT the fp32 one; arith="f32" is the call without the argument."""
    monkeypatch.delenv("MSTTS_WG_ARITH", raising=False)
    monkeypatch.delenv("MSTTS_WG_BF16_RESIDENT", raising=False)
    cfg, N, T = ENGINE_CASES[name]
    od, eng = _engine(dev, cfg)
    mel, _, L = _inputs(od, N, T)
    a, b = eng.infer(mel, seed=5, arith="bf16").clone(), eng.infer(mel, seed=5, arith="bf16").clone()
    assert a.shape == (N, L) and bool(torch.isfinite(a).all()) and torch.equal(a.view(torch.int32), b.view(torch.int32))
    f0, f1 = eng.infer(mel, seed=5).clone(), eng.infer(mel, seed=5, arith="f32").clone()
    assert torch.equal(f0.view(torch.int32), f1.view(torch.int32))
    assert not torch.equal(a, f0)
    rel = float((a.double() - f0.double()).norm() / f0.double().norm())
    print("%s: |wav_bf16 - wav_f32| / |wav_f32| = %.3e" % (name, rel))
    assert rel > 0
    with pytest.raises(ValueError):
        eng.infer(mel, seed=5, arith="fp16")
    monkeypatch.setenv("MSTTS_WG_ARITH", "bf16")
    assert torch.equal(eng.infer(mel, seed=5).view(torch.int32), a.view(torch.int32))         # the environment variable alone selects it


def test_vocode_arith(dev, monkeypatch):
    monkeypatch.delenv("MSTTS_WG_ARITH", raising=False)
    od, eng = _engine(dev, CFG0)
    g = np.random.default_rng(1)
    mels = [g.normal(0, 1, (t, od.n_mel)).astype(np.float32) for t in (7, 3)]
    w32, w16 = WG.vocode(eng, mels, split=3, batch=2, noise_seed=11), WG.vocode(eng, mels, split=3, batch=2, noise_seed=11, arith="bf16")
    assert [w.shape for w in w32] == [w.shape for w in w16] and all(np.isfinite(w).all() for w in w16)
    assert not np.array_equal(w32[0], w16[0])


def test_tacotron2_inference_waveglow_bf16_surface(dev, tmp_path, monkeypatch):
    """Tacotron2.Inference_WaveGlow(..., wg_arith="bf16") on the tiny dims of tests/test_gpu_waveglow.py's surface test: same shapes and cut
    points as fp32, finite, different samples; Inference forwards it; MSTTS_WG_ARITH alone selects it."""
    from multi_speaker_tts_amd import Hyper_Parameters as hp
    from multi_speaker_tts_amd.MSTTS_SV import Tacotron2
    from multi_speaker_tts_amd.params import Dims
    monkeypatch.delenv("MSTTS_WG_ARITH", raising=False)
    monkeypatch.setattr(hp, "Checkpoint_Path", str(tmp_path / "ckpt"))
    monkeypatch.setattr(hp, "Inference_Path", str(tmp_path / "inf"))
    monkeypatch.setattr(hp, "Use_Vocoder", "WaveGlow")
    for k, v in dict(Flows=4, Early_Every=2).items():
        monkeypatch.setattr(hp.WaveGlow, k, v)
    monkeypatch.setattr(hp.WaveGlow.WaveNet, "Channels", 32)
    monkeypatch.setattr(hp.WaveGlow.WaveNet, "Layers", 2)
    monkeypatch.setattr(hp.WaveGlow.Upsample, "Kernel_Size", 32)
    monkeypatch.setattr(hp.WaveGlow.Upsample, "Strides", 8)
    monkeypatch.setattr(hp.WaveGlow.Inference, "Mel_Split_Length", 3)
    monkeypatch.setattr(hp.WaveGlow, "Checkpoint_Path", str(tmp_path / "wg"))
    dims = Dims(emb=32, enc_conv_ch=32, enc_lstm=16, spk=256, prenet=16, dec_lstm=32, post_ch=16, bank_ch=8, proj1_ch=16, birnn=8, n_spec=20,
                spk_lstm=256, max_inf=6)
    t = Tacotron2(is_Training=False, device=dev, dims=dims, allow_random_init=True)
    # the reference's initialiser zeroes every coupling's output conv (an identity coupling: no contraction reaches the samples), so give the
    # vocoder the oracle's random values, whose output convs are not zero; load() also drops the packed bf16 weights of the old values
    import dataclasses
    t.waveglow.load(OW.init_params(OW.WGDims(**dataclasses.asdict(t.waveglow.d)), seed=4))
    mels = [np.clip(np.random.default_rng(i).normal(0, 1.5, (230, 80)), -4, 4).astype(np.float32) for i in range(2)]
    texts = ["Please call Stella.", "Who knows?"]
    run = lambda **kw: t.Inference_WaveGlow(None, texts, speaker_Mel_List=mels, export=False, noise_seed=3, **kw)
    r32, r16 = run(), run(wg_arith="bf16")
    for i in range(2):
        assert r16["Wav"][i].shape == r32["Wav"][i].shape and r16["Cut"][i]["Wav"].shape == r32["Cut"][i]["Wav"].shape
        assert np.isfinite(r16["Wav"][i]).all() and not np.array_equal(r16["Wav"][i], r32["Wav"][i])
    assert np.array_equal(run(wg_arith="f32")["Wav"][0], r32["Wav"][0])
    via = t.Inference(None, texts, speaker_Mel_List=mels, export=False, wg_arith="bf16")
    assert via["Wav"][0].shape == r16["Wav"][0].shape and np.isfinite(via["Wav"][0]).all()
    monkeypatch.setenv("MSTTS_WG_ARITH", "bf16")
    assert np.array_equal(run()["Wav"][0], r16["Wav"][0]) and np.array_equal(run()["Wav"][1], r16["Wav"][1])
