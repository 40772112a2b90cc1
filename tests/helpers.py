"""Shared helpers of the parity tests (the oracle is only ever the checker)."""
import numpy as np
import torch

from oracle import model as OM
from multi_speaker_tts_amd.params import Dims


def small_dims(**kw):
    """Reduced widths (attention dims stay at the kernels' built sizes A=128, CH=32)."""
    base = dict(emb=32, enc_conv_ch=32, enc_lstm=16, spk=16, prenet=16, dec_lstm=32, n_mel=8, post_ch=16,
                bank_ch=8, proj1_ch=16, birnn=8, n_spec=20, spk_lstm=16, att_k=31)
    base.update(kw)
    return base


def dims_pair(**kw):
    cfg = small_dims(**kw)
    return Dims(**cfg), OM.Dims(**cfg)


def rel_err(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def to_dev(batch, dev):
    return {k: v.to(dev).contiguous() for k, v in batch.items()}


def t2n(t):
    return t.detach().cpu().numpy()


def taco1_problem(B, S, kw):
    """The Taco1 trainer parity problem of one case (tests/test_gpu_taco1_trainer.py; its CPU side in tests/test_cpu_oracle.py): (engine dims,
    oracle dims, variables, mel [B,S,n_mel], spectrogram [B,S,n_spec], the generator, from which the zoneout masks of every step are drawn next)."""
    pd, od = dims_pair(**kw)
    values = OM.init_params(od, 5)
    g = np.random.default_rng(6)
    for k in values:
        if k.startswith(OM.P_V) and k.endswith(("bias", "beta")) and "highway" not in k:
            values[k] = g.normal(0, 0.1, values[k].shape)
        if k.startswith(OM.P_V) and k.endswith("moving_variance"):
            values[k] = 0.5 + np.abs(g.normal(0, 0.5, values[k].shape))
    mel = np.clip(g.normal(0, 1.5, (B, S, od.n_mel)), -4, 4).astype(np.float32)
    spec = g.uniform(0, 1, (B, S, od.n_spec)).astype(np.float32)
    return pd, od, values, mel, spec, g


def taco1_zoneout_masks(g, B, S, od):
    return {k: torch.tensor(g.integers(0, 2, (S, B, od.birnn)).astype(np.uint8)) for k in ("v_zc_fw", "v_zh_fw", "v_zc_bw", "v_zh_bw")}


# the Taco1 parity cases whose convolutions all run on the kernels long sequences reach (T >= 32, K cin >= 160 for K >= 2, a 165-row reduction)
# and the reference's CBHG widths; at their ~500 000 ReLU outputs and ~200 000 L1 terms the engine's kink patterns are injected into the oracle
TACO1_LONG = [(5, 33, dict(n_mel=80, bank_ch=32, proj1_ch=64, birnn=32, n_spec=129)), (2, 97, dict(n_mel=80, bank_ch=128, proj1_ch=256, birnn=128, n_spec=1025))]
