"""mstts_convbank_pack's rule in NumPy: what tests/test_cpu_convbank_pack.py checks against the separate convolutions in fp64 and
tests/test_gpu_voc_chain.py holds the native launch to, bit for bit."""
import numpy as np

from multi_speaker_tts_amd.params import bank_groups


def bank_pack_reference(kernels, biases, k_split):
    """kernels[k-1] [k, cin, cout], biases[k-1] [cout] -> ([one [window * cin, n * cout]
    matrix per group], bias [bank_k * cout]); conv k's tap j sits at window tap j + pad - (k-1)//2 of its group, in columns (k-lo) * cout."""
    bank_k = len(kernels)
    cin, cout = kernels[0].shape[1:]
    out = []
    for lo, hi, win, pad in bank_groups(bank_k, k_split):
        m = np.zeros((win, cin, hi - lo + 1, cout), kernels[0].dtype)
        for k in range(lo, hi + 1):
            for j in range(k):
                m[j + pad - (k - 1) // 2, :, k - lo, :] = kernels[k - 1][j]
        out.append(m.reshape(win * cin, (hi - lo + 1) * cout))
    return out, np.concatenate([np.asarray(b).reshape(cout) for b in biases])
