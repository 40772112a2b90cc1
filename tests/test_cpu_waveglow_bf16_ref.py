"""Pins the judge of the vocoder's bf16 mode (tests/waveglow_bf16_ref.py) without a GPU: a float32 torch emulation of the mode passes it, and
every planted fault is reported at its own stage and layer with nothing earlier over its bound.  Also the new C ABI symbols and the
host-only shape check of mstts_gemm_bf16_res."""
import os
import re

import numpy as np
import pytest
import torch

from multi_speaker_tts_amd import lib
from multi_speaker_tts_amd import waveglow as WG
from oracle import waveglow as OW
from tests import waveglow_bf16_ref as R

CFG0 = dict(n_mel=8, flows=4, groups=8, early_every=2, early_size=2, up_k=16, up_stride=4, layers=3, ch=32, k=3)      # = tests/test_gpu_waveglow.py CFGS[0]
N, T = 2, 5
AT = (1, 1)           # where the faults are planted: flow 1, layer 1 (dilation 2)


@pytest.fixture(scope="module")
def case():
    od, pd = OW.WGDims(**CFG0), WG.WGDims(**CFG0)
    eng = WG.WaveGlowEngine(pd, device="cpu", values=OW.init_params(od, seed=3))
    mel = np.clip(np.random.default_rng(8).normal(0, 1.5, (N, T, od.n_mel)), -4, 4).astype(np.float32)
    L = (T - 1) * od.up_stride + od.up_k
    noise = OW.make_noise(od, N, L // od.groups, seed=9)
    return eng, mel, noise


def test_emulation_passes_the_judge(case):
    eng, mel, noise = case
    wav, stages = R.emulate(eng, mel, noise, sigma=0.8)
    assert wav.shape == (N, (T - 1) * CFG0["up_stride"] + CFG0["up_k"]) and bool(torch.isfinite(wav).all())
    assert R.check(stages, eng, mel, noise, sigma=0.8, wav=wav) == []
    assert set(stages[AT]) == {"pre", "z", "zb", "rs", "xb"} and {"melg_b", "x", "ls_b"} <= set(stages[AT[0]])


@pytest.mark.parametrize("fault,stage", [("truncate", "xb"), ("xb_unrounded", "xb"), ("round_before_add", "xb"), ("conv_fp32_x", "pre"),
                                         ("weight_other_rounding", "pre"), ("tap_shift", "pre")])
def test_planted_fault_is_reported_at_its_stage(case, fault, stage):
    """operands truncated instead of rounded to nearest even | xb left unrounded | x = zb + res (rounded before the residual add) | the conv
    multiplying the fp32 x | the weight rounded to another value than the packed fp32 fold's | tap 0 shifted by dil - 1.  The judge follows
    no trajectory, so the FIRST finding is the planted stage at the planted layer, and it is the only one."""
    eng, mel, noise = case
    _, stages = R.emulate(eng, mel, noise, sigma=0.8, fault=fault, at=AT)
    found = R.check(stages, eng, mel, noise, sigma=0.8, raise_=False)
    assert found and found[0][:3] == (stage, AT[0], AT[1]), found
    assert len(found) == 1, found
    with pytest.raises(AssertionError):
        R.check(stages, eng, mel, noise, sigma=0.8)


def test_bf_is_round_to_nearest_even():
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -9, 1.0 - 2.0 ** -9, -0.0])
    assert R.bf(x).tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0, 1.0, -0.0]             # ties to even both ways; below half an ulp: down
    assert not torch.equal(R._truncate(torch.tensor([1.0 + 3 * 2.0 ** -8])), R.bf(torch.tensor([1.0 + 3 * 2.0 ** -8])))


def test_new_symbols_and_shape_check():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "mstts.h")).read()
    L = lib.load()
    for name in ("mstts_gemm_bf16_res", "mstts_gemm_bf16_res_supported", "mstts_round_bf16", "mstts_wg_gate_bf16", "mstts_wg_res_skip_bf16"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in lib.SIGNATURES and hasattr(L, name), name
    assert "mstts_gemm_res_desc" in header and lib.ABI_VERSION == 5 and L.mstts_abi_version() == 5          # additions only
    ok = L.mstts_gemm_bf16_res_supported
    assert ok(130, 136, 72, 72, 72, 0, 0) == 1 and ok(300, 264, 24, 8, 24, 300, 8) == 1 and ok(5504, 1024, 1536, 512, 1536, 1376, 512) == 1
    assert ok(40, 32, 36, 12, 36, 20, 12) == 0           # win_C = 12
    assert ok(40, 32, 20, 20, 20, 0, 0) == 0             # K = 20
    assert ok(40, 32, 24, 28, 24, 0, 0) == 0 and ok(40, 32, 24, 24, 28, 0, 0) == 0          # lda / ldb not multiples of 8
    assert ok(40, 32, 48, 16, 48, 20, 8) == 0            # window: lda != win_C
    assert lib.gemm_res_supported(40, 32, 48, 16, 48, win=(20, 16)) and not lib.gemm_res_supported(40, 32, 60, 20, 60, win=(20, 20))


def test_arith_resolution(monkeypatch):
    monkeypatch.delenv("MSTTS_WG_ARITH", raising=False)
    assert WG.resolve_arith(None) == "f32" and WG.resolve_arith(None, "bf16") == "bf16" and WG.resolve_arith("f32", "bf16") == "f32"
    monkeypatch.setenv("MSTTS_WG_ARITH", "bf16")
    assert WG.resolve_arith(None) == "bf16" and WG.resolve_arith(None, "f32") == "f32" and WG.resolve_arith("f32") == "f32"
    monkeypatch.setenv("MSTTS_WG_ARITH", "fp8")
    with pytest.raises(ValueError):
        WG.resolve_arith(None)
    with pytest.raises(ValueError):
        WG.resolve_arith("half")
    with pytest.raises(ValueError):
        WG.WaveGlowEngine(WG.WGDims(**CFG0), device="cpu", arith="half")
