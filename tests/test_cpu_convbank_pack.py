"""The packed conv bank (mstts_convbank_pack, params.bank_groups, tests/convbank_ref.py): the bank's 'same' convolutions of widths 1..bank_k as
one window product per group of widths.  Checked in fp64 on the CPU: the packing rule entry by entry, and the products of the packed groups
against the bank_k separate convolutions, column for column."""
import numpy as np
import pytest
import torch

from multi_speaker_tts_amd.params import bank_groups
from tests.convbank_ref import bank_pack_reference

BANK_K, CIN, COUT = 8, 5, 3


def _bank(seed=0):
    rng = np.random.default_rng(seed)
    kernels = [rng.standard_normal((k, CIN, COUT)) for k in range(1, BANK_K + 1)]
    biases = [rng.standard_normal(COUT) for _ in range(BANK_K)]
    return kernels, biases


def test_groups_of_the_reference_bank():
    assert bank_groups(8, 4) == [(1, 4, 4, 1), (5, 8, 8, 3)]          # (lo, hi, window, pad): offsets -1..+2 and -3..+4
    assert bank_groups(8, 8) == [(1, 8, 8, 3)]
    assert bank_groups(1, 1) == [(1, 1, 1, 0)]
    for bank_k, ks in ((8, 4), (8, 8), (8, 3), (5, 2)):
        for lo, hi, win, pad in bank_groups(bank_k, ks):
            for k in range(lo, hi + 1):                                # every width's offsets -(k-1)//2 .. k-1-(k-1)//2 lie inside the window's
                assert -pad <= -((k - 1) // 2) and k - 1 - (k - 1) // 2 <= win - 1 - pad


@pytest.mark.parametrize("k_split", [4, 8, 3])
def test_packing_rule(k_split):
    """Conv k's tap j sits at window tap j + pad - (k-1)//2 of its group, in the columns (k - lo) * cout; everything else is zero; the bias is in
    bank order."""
    kernels, biases = _bank()
    mats, bias = bank_pack_reference(kernels, biases, k_split)
    groups = bank_groups(BANK_K, k_split)
    assert len(mats) == len(groups)
    for m, (lo, hi, win, pad) in zip(mats, groups):
        assert m.shape == (win * CIN, (hi - lo + 1) * COUT)
        seen = np.zeros(m.shape, bool)
        for k in range(lo, hi + 1):
            for j in range(k):
                tap = j + pad - (k - 1) // 2
                assert 0 <= tap < win
                blk = (slice(tap * CIN, (tap + 1) * CIN), slice((k - lo) * COUT, (k - lo + 1) * COUT))
                assert np.array_equal(m[blk], kernels[k - 1][j])
                seen[blk] = True
        assert not m[~seen].any()
    assert np.array_equal(bias, np.concatenate(biases))


def _same_conv(x, kernel, bias):
    """tf.layers.conv1d(padding='same') of x [B, S, cin] with kernel [k, cin, cout]: output frame t reads the frames t - (k-1)//2 .. t + k-1-(k-1)//2."""
    k = kernel.shape[0]
    xp = torch.nn.functional.pad(x.permute(0, 2, 1), ((k - 1) // 2, k - 1 - (k - 1) // 2))
    return torch.nn.functional.conv1d(xp, kernel.permute(2, 1, 0), bias).permute(0, 2, 1)


def _window_product(x, mat, win, pad):
    """The implicit im2col view mstts_gemm_f32's window mode forms (A(m, tap * cin + c) = x[m - pad + tap][c], zero outside the batch row's own S
    frames) times the packed matrix."""
    B, S, cin = x.shape
    a = torch.zeros(B, S, win, cin, dtype=x.dtype)
    for t in range(S):
        for tap in range(win):
            if 0 <= t - pad + tap < S:
                a[:, t, tap] = x[:, t - pad + tap]
    return a.reshape(B * S, win * cin) @ mat


@pytest.mark.parametrize("k_split", [4, 8])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S", [1, 2, 9])
def test_packed_groups_equal_the_separate_convolutions(S, B, k_split):
    kernels, biases = _bank(1)
    mats, bias = bank_pack_reference(kernels, biases, k_split)
    x = torch.from_numpy(np.random.default_rng(10 * S + B).standard_normal((B, S, CIN)))
    got = torch.cat([_window_product(x, torch.from_numpy(m), win, pad) for m, (_, _, win, pad) in zip(mats, bank_groups(BANK_K, k_split))], dim=1)
    got = (got + torch.from_numpy(bias)).reshape(B, S, BANK_K * COUT)
    for k in range(1, BANK_K + 1):
        ref = _same_conv(x, torch.from_numpy(kernels[k - 1]), torch.from_numpy(biases[k - 1]))
        d = (got[:, :, (k - 1) * COUT:k * COUT] - ref).abs()
        assert float(d.max()) <= 1e-12, (k, float(d.max()))
        assert float(d[:, 0].max()) <= 1e-12 and float(d[:, -1].max()) <= 1e-12         # the first and the last frame of every batch row
