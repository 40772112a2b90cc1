// The in-LDS FFT of every STFT kernel: stft_frame_body (csrc/stft_frame.h: stft_fft_kernel, stft_bank_batch_kernel, wg_crop_batch_kernel)
// and the round trips built from csrc/stft_parts.h, griffin_lim_kernel (csrc/griffin_lim.hip) and wg_denoise_frames_kernel (csrc/wg_denoise.hip).
#pragma once
#include "common.h"

namespace mstts {

// Forward FFT of N2 = n_fft / 2 complex points by a 256-thread workgroup: Stockham autosort, radix 4 while it fits and one radix-2 stage
// for the odd power (N2 = 512, 2048), ping-pong between two LDS buffers, a barrier after every stage.  bufa holds the input (written and
// barriered by the caller); the result is in the returned buffer (bufa or bufb).  Stage with sub-transform size p: thread i takes
// x[i + m t], m < radix, t = N2 / radix, twiddles e^{-2 pi i m k / (radix p)} = tw[m k n_fft / (radix p)] (tw has n_fft entries;
// 3 m k n_fft / (4 p) < 3 n_fft / 4).  The inverse transform is this one on conjugated input, conjugated again.
__device__ __forceinline__ float2* fft_stockham_stages(float2* bufa, float2* bufb, const float2* __restrict__ tw, int N2, int n_fft, int tid) {
    int p = 1;
    for (; p * 4 <= N2; p <<= 2) {
        const int t4 = N2 >> 2, tmul = n_fft / (4 * p);
        for (int i = tid; i < t4; i += 256) {
            const int k = i & (p - 1), m = k * tmul;
            const float2 w1 = tw[m], w2 = tw[2 * m], w3 = tw[3 * m];
            const float2 x0 = bufa[i], x1 = bufa[i + t4], x2 = bufa[i + 2 * t4], x3 = bufa[i + 3 * t4];
            const float2 u1 = make_float2(x1.x * w1.x - x1.y * w1.y, x1.x * w1.y + x1.y * w1.x);
            const float2 u2 = make_float2(x2.x * w2.x - x2.y * w2.y, x2.x * w2.y + x2.y * w2.x);
            const float2 u3 = make_float2(x3.x * w3.x - x3.y * w3.y, x3.x * w3.y + x3.y * w3.x);
            const float2 v0 = make_float2(x0.x + u2.x, x0.y + u2.y), v1 = make_float2(x0.x - u2.x, x0.y - u2.y);
            const float2 v2 = make_float2(u1.x + u3.x, u1.y + u3.y), v3 = make_float2(u1.y - u3.y, u3.x - u1.x);   // (u1 - u3) * (-i)
            const int j0 = ((i - k) << 2) + k;
            bufb[j0] = make_float2(v0.x + v2.x, v0.y + v2.y);
            bufb[j0 + p] = make_float2(v1.x + v3.x, v1.y + v3.y);
            bufb[j0 + 2 * p] = make_float2(v0.x - v2.x, v0.y - v2.y);
            bufb[j0 + 3 * p] = make_float2(v1.x - v3.x, v1.y - v3.y);
        }
        __syncthreads();
        float2* t_ = bufa; bufa = bufb; bufb = t_;
    }
    if (p < N2) {                                            // p == N2 / 2: the last radix-2 stage
        const int tmul = n_fft / (2 * p);
        for (int i = tid; i < (N2 >> 1); i += 256) {
            const int k = i & (p - 1);
            const float2 a = bufa[i], b = bufa[i + (N2 >> 1)], t = tw[k * tmul];
            const float2 bt = make_float2(b.x * t.x - b.y * t.y, b.x * t.y + b.y * t.x);
            const int j0 = ((i - k) << 1) + k;
            bufb[j0] = make_float2(a.x + bt.x, a.y + bt.y);
            bufb[j0 + p] = make_float2(a.x - bt.x, a.y - bt.y);
        }
        __syncthreads();
        float2* t_ = bufa; bufa = bufb; bufb = t_;
    }
    return bufa;
}

}  // namespace mstts
