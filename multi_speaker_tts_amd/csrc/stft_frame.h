// One STFT frame by a 256-thread workgroup, shared by stft_fft_kernel (csrc/audio.hip: frames of packed waveforms, back to back) and
// stft_bank_batch_kernel (csrc/stft_bank.hip: frames of bank signals, straight into padded batch tensors).  The kernels differ only in
// how a workgroup finds its waveform, its frame and its output rows; the arithmetic is this one body, so both give the same bits.
#pragma once
#include "common.h"
#include "stft_parts.h"

namespace mstts {

//   x[i] = window[i - off] * preemph(reflect(f*hop + i - n_fft/2))   (0 outside the window)       Audio.py:42-48,62-64
//   z[m] = x[2m] + i x[2m+1]  ->  Stockham radix-4 FFT of n_fft/2 complex points (ping-pong LDS buffers, twiddles from a table
//   built in fp64 on the host)  ->  X[k] = E[k] + e^{-2 pi i k / n_fft} O[k]  ->  |X[k]|, k = 0 .. n_fft/2
//   spec_row = clip((20 log10(max(1e-5, |X|)) - ref_db + 100) / 100, 0, 1)                          Audio.py:19-22,91-92
//   mel_row  = symmetric-normalised dB of mel_basis . |X| over each filter's non-zero bin range     Audio.py:29-32,78-80,94-96
// fft_lds: n_fft float2 of LDS.  x / n: the waveform and its length (n > n_fft / 2), f: the frame.  mel_row [n_mel] / spec_row
// [n_fft/2+1]: this frame's output rows, either may be null.  mag_row != null: no transform, the magnitudes are read from it and
// sub[k] * sub_scale is subtracted (clipped at 0).  flags & 1: the [0, 1] mel normalisation; flags & 2: spec_row gets raw magnitudes.
__device__ __forceinline__ void stft_frame_body(float2* fft_lds, const float* __restrict__ x, long n, long f, float coef,
                                                const float* __restrict__ window, const float2* __restrict__ tw,
                                                const float* __restrict__ mel_basis, const int* __restrict__ mel_rng, int n_fft, int hop,
                                                int win, int n_mel, float max_abs, float ref_db, float* __restrict__ mel_row,
                                                float* __restrict__ spec_row, const float* __restrict__ mag_row,
                                                const float* __restrict__ sub, float sub_scale, int flags) {
    const int N2 = n_fft >> 1, tid = threadIdx.x;
    float2* bufa = fft_lds;
    float2* bufb = fft_lds + N2;
    const int off = (n_fft - win) >> 1, pad = n_fft >> 1;
    auto sample = [&](int i) -> float {                  // windowed, pre-emphasised, reflect-padded sample i of this frame
        if (i < off || i >= off + win) return 0.f;
        const long j = stft_reflect_once(f * hop + i - pad, n);
        const float prev = j > 0 ? x[j - 1] : 0.f;
        return window[i - off] * (x[j] - coef * prev);
    };
    const int NB = N2 + 1;
    float* mag = reinterpret_cast<float*>(bufb);
    if (mag_row) {
        // second pass of the spectral-subtraction form (Audio.py:45-46): magnitudes of the first pass minus sub[k], clipped at 0
        for (int k = tid; k < NB; k += 256) {
            const float m = fmaxf(mag_row[k] - (sub ? sub[k] * sub_scale : 0.f), 0.f);
            mag[k] = m;
            if (spec_row) {
                const float db = 20.f * log10f(fmaxf(1e-5f, m)) - ref_db;
                spec_row[k] = fminf(fmaxf((db + 100.f) * 0.01f, 0.f), 1.f);
            }
        }
        __syncthreads();
    } else {
    for (int m = tid; m < N2; m += 256) bufa[m] = make_float2(sample(2 * m), sample(2 * m + 1));
    __syncthreads();
    // Stockham radix-4 stages (csrc/fft_stages.h); the spectrum ends up in bufa, bufb is the other buffer
    {
        float2* z = fft_stockham_stages(bufa, bufb, tw, N2, n_fft, tid);
        if (z != bufa) { bufb = bufa; bufa = z; }
    }
    // real-input post-processing -> magnitudes in LDS (bufb is free).  rfft_split's rule (csrc/stft_parts.h has the derivation) in a text
    // of its own: one bin per thread, and E + W^k O summed left to right, not rfft_split's E + (W^k O) - this body's bits are pinned.
    mag = reinterpret_cast<float*>(bufb);
    for (int k = tid; k < NB; k += 256) {
        const float2 zk = bufa[k & (N2 - 1)], zc = bufa[(N2 - k) & (N2 - 1)];
        const float er = 0.5f * (zk.x + zc.x), ei = 0.5f * (zk.y - zc.y);           // E = (Z[k] + conj(Z[N2-k])) / 2
        const float orr = 0.5f * (zk.y + zc.y), oi = -0.5f * (zk.x - zc.x);         // O = -i (Z[k] - conj(Z[N2-k])) / 2
        const float2 t = k < N2 ? tw[k] : make_float2(-1.f, 0.f);
        const float re = er + orr * t.x - oi * t.y, im = ei + orr * t.y + oi * t.x;
        const float m = sqrtf(re * re + im * im);
        mag[k] = m;
        if (spec_row) {
            if (flags & 2) spec_row[k] = m;                             // raw magnitudes (first pass of the spectral-subtraction form)
            else {
                const float db = 20.f * log10f(fmaxf(1e-5f, m)) - ref_db;
                spec_row[k] = fminf(fmaxf((db + 100.f) * 0.01f, 0.f), 1.f);
            }
        }
    }
    __syncthreads();
    }
    if (!mel_row) return;
    // mel: three threads per filter, each sums every third bin of the filter's non-zero range; the three partial sums are
    // combined in fixed order (bit-reproducible).  No wave reductions: twenty dependent shuffle chains per wave cost more than
    // the transform itself.
    float* part = reinterpret_cast<float*>(bufa);             // the spectrum has been consumed
    for (int c0 = 0; c0 < n_mel; c0 += 85) {                   // 85 filters x 3 threads per pass
        const int c = c0 + tid / 3, q = tid - (tid / 3) * 3;
        if (tid < 255 && c < n_mel) {
            const int lo = mel_rng[2 * c], hi = mel_rng[2 * c + 1];
            const float* row = mel_basis + (long)c * NB;
            float acc = 0.f;
            for (int b = lo + q; b < hi; b += 3) acc = fmaf(row[b], mag[b], acc);
            part[tid] = acc;
        }
        __syncthreads();
        if (tid < 85 && c0 + tid < n_mel) {
            const int cc = c0 + tid;
            const float m = (part[3 * tid] + part[3 * tid + 1]) + part[3 * tid + 2];
            const float db = 20.f * log10f(fmaxf(1e-5f, m));
            if (flags & 1) mel_row[cc] = fminf(fmaxf((db + 100.f) * 0.01f, 0.f), 1.f);          // Audio._normalize
            else {
                const float v = (2.f * max_abs) * ((db + 100.f) * 0.01f) - max_abs;            // Audio._symmetric_normalize
                mel_row[cc] = fminf(fmaxf(v, -max_abs), max_abs);
            }
        }
        __syncthreads();
    }
}

}  // namespace mstts
