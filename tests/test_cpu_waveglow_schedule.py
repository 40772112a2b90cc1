"""The launch schedule of WaveGlowEngine.infer per mode, without a GPU: `call`, `gemm` and `gemm_res` of multi_speaker_tts_amd.waveglow are
replaced by recorders that launch nothing, then infer runs on an engine built with device="cpu".  (lib.load() and lib.deterministic_gemm
need no device: they load the library and flip a host-side switch.)"""
import numpy as np
import pytest

from multi_speaker_tts_amd import waveglow as WG
from oracle import waveglow as OW

CFG0 = dict(n_mel=8, flows=4, groups=8, early_every=2, early_size=2, up_k=16, up_stride=4, layers=3, ch=32, k=3)      # = tests/test_gpu_waveglow.py CFGS[0]
N, T = 2, 5
RESIDENT_ONLY = ("mstts_gemm_bf16_res", "mstts_round_bf16", "mstts_wg_gate_bf16", "mstts_wg_res_skip_bf16")
BF16_ENTRY_POINTS = RESIDENT_ONLY + ("mstts_gemm_bf16",)


def run(monkeypatch, cfg=CFG0, N=N, T=T, arith="f32", resident=None, two=False):
    """[(entry point, args, kwargs)] of one infer: every `call` by its name, `gemm` as mstts_gemm_bf16 / mstts_gemm_f32, `gemm_res`."""
    if resident is None:
        monkeypatch.delenv("MSTTS_WG_BF16_RESIDENT", raising=False)
    else:
        monkeypatch.setenv("MSTTS_WG_BF16_RESIDENT", resident)
    eng = WG.WaveGlowEngine(WG.WGDims(**cfg), device="cpu", values=OW.init_params(OW.WGDims(**cfg), seed=3))
    eng.conv_two_pieces = two
    rec = []
    monkeypatch.setattr(WG, "call", lambda name, *a: rec.append((name, a, {})))
    monkeypatch.setattr(WG, "gemm", lambda *a, **k: rec.append(("mstts_gemm_bf16" if k.get("bf16") else "mstts_gemm_f32", a, k)))
    monkeypatch.setattr(WG, "gemm_res", lambda *a, **k: rec.append(("mstts_gemm_bf16_res", a, k)))
    mel = np.zeros((N, T, cfg["n_mel"]), np.float32)
    wav = eng.infer(mel, seed=5, arith=arith)
    assert wav.shape == (N, (T - 1) * cfg["up_stride"] + cfg["up_k"])
    return rec


def count(rec, name):
    return sum(1 for r in rec if r[0] == name)


def test_fp32_issues_no_bf16_entry_point(monkeypatch):
    rec = run(monkeypatch)
    flows, layers = CFG0["flows"], CFG0["layers"]
    assert not [r[0] for r in rec if r[0] in BF16_ENTRY_POINTS]
    assert all("bf16" not in r[2] or r[2]["bf16"] is False for r in rec)
    assert count(rec, "mstts_gemm_f32") == 1 + flows * (2 + 2 * layers + 1)
    assert count(rec, "mstts_wg_gate") == flows * layers == count(rec, "mstts_wg_res_skip") and count(rec, "mstts_wg_gate_add") == 0


def test_bf16_resident(monkeypatch):
    rec = run(monkeypatch, arith="bf16")
    flows, layers = CFG0["flows"], CFG0["layers"]
    assert count(rec, "mstts_gemm_bf16_res") == flows * (1 + 2 * layers)
    assert count(rec, "mstts_round_bf16") == 1 + flows
    assert count(rec, "mstts_wg_gate_bf16") == flows * layers == count(rec, "mstts_wg_res_skip_bf16")
    assert count(rec, "mstts_gemm_f32") == 0 and count(rec, "mstts_wg_gate") == 0 and count(rec, "mstts_wg_res_skip") == 0
    assert count(rec, "mstts_gemm_bf16") == 1 + 2 * flows                  # the upsampler, the initial and the output conv
    for r in rec:                       # the transposed packed weight: ldb = K, not N
        if r[0] == "mstts_gemm_bf16_res":
            A, B, C, M, Nn, K, lda, ldb, ldc = r[1]
            assert ldb == K and tuple(B.shape) == (Nn, K)


def test_bf16_resident_switched_off(monkeypatch):
    rec = run(monkeypatch, arith="bf16", resident="0")
    flows, layers = CFG0["flows"], CFG0["layers"]
    assert not [r[0] for r in rec if r[0] in RESIDENT_ONLY]
    assert count(rec, "mstts_gemm_f32") == 0 and count(rec, "mstts_gemm_bf16") == 1 + flows * (2 + 2 * layers + 1)
    assert all(r[2].get("bf16") is True for r in rec if r[0].startswith("mstts_gemm"))


def test_bf16_ch36(monkeypatch):
    """ch = 36: mstts_gemm_bf16_res refuses every product whose K or pitch is ch-derived (K = 3 * 36 and K = 36 are no multiples of 8) - the
    dilated convolution and the res/skip product - while the vector glue (C % 4 == 0) would still be legal: neither bf16 glue kernel may
    run, since its consumer is not resident.  The conditioning product's K, lda and ldb are groups * n_mel = 64 whatever ch is, so it
    alone stays resident (once per flow, with the one rounding of melg): as at the parent commit, and unlike the issue's "none of the four",
    which holds for the two ch-dependent products."""
    cfg = dict(CFG0, ch=36)
    rec = run(monkeypatch, cfg=cfg, arith="bf16")
    flows, layers = cfg["flows"], cfg["layers"]
    assert count(rec, "mstts_wg_gate_bf16") == 0 and count(rec, "mstts_wg_res_skip_bf16") == 0
    assert count(rec, "mstts_wg_gate") == flows * layers == count(rec, "mstts_wg_res_skip")
    res = [r for r in rec if r[0] == "mstts_gemm_bf16_res"]
    assert len(res) == flows and all(r[1][5] == cfg["groups"] * cfg["n_mel"] for r in res)          # K = G * n_mel: the conditioning product
    assert count(rec, "mstts_round_bf16") == 1
    assert count(rec, "mstts_gemm_f32") == 0 and count(rec, "mstts_gemm_bf16") == 1 + flows * (1 + 2 * layers + 1)
    assert all(r[2].get("bf16") is True for r in rec if r[0] in ("mstts_gemm_bf16", "mstts_gemm_f32"))


def test_fp32_two_pieces(monkeypatch):
    """conv_two_pieces forced on at 160 rows x 1024 (pinned True in tests/test_cpu_policy.py): each layer issues a split_k = 2 product into the
    convolution's own buffer and mstts_wg_gate_add."""
    cfg = dict(n_mel=80, flows=1, groups=8, early_every=4, early_size=2, up_k=1024, up_stride=256, layers=8, ch=512, k=3)
    assert WG._conv_two_pieces(160, 1024)
    rec = run(monkeypatch, cfg=cfg, N=1, T=2, two=True)                    # L = 1280, rows = 160
    layers = cfg["layers"]
    assert count(rec, "mstts_wg_gate_add") == layers and count(rec, "mstts_wg_gate") == 0
    split2 = [r for r in rec if r[0] == "mstts_gemm_f32" and r[2].get("split_k") == 2]
    assert len(split2) == layers and all(not r[2].get("accumulate") and r[1][3:6] == (160, 1024, 3 * 512) for r in split2)
    assert not [r[0] for r in rec if r[0] in BF16_ENTRY_POINTS]
    # ... and the same engine in bf16 mode takes one piece: the two-piece form is fp32 only
    rec = run(monkeypatch, cfg=cfg, N=1, T=2, arith="bf16", two=True)
    assert count(rec, "mstts_wg_gate_add") == 0 and not [r for r in rec if r[2].get("split_k", 1) != 1]
