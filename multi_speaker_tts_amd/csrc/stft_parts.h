// The frame toolkit of the STFT round trips, each rule stated once: griffin_lim_kernel (csrc/griffin_lim.hip) and
// wg_denoise_frames_kernel (csrc/wg_denoise.hip) are one skeleton - stft_owner, fill the frame, fft_stockham_stages, rfft_split / their
// own map of the bin pair / rfft_merge, stft_frame_tail - and their gathers are stft_ola.  The kernels promise bit-reproducibility, so
// the statement order of every piece is part of its contract.  stft_frame_body (csrc/stft_frame.h) and stft_fft_kernel (csrc/audio.hip)
// have pinned instruction text: they keep the split and the lookup as text of their own (profiles/stft_parts_refactor_codegen.txt).
#pragma once
#include "common.h"
#include "fft_stages.h"

namespace mstts {

// Index w with key(w) <= v < key(w + 1), key non-decreasing over 0 .. nw: uniform binary search, every lane of a workgroup (or every
// thread, in the gathers) takes the same number of steps.  w follows lo inside the loop, so nw = 1 returns 0 without a comparison.
template <class Key>
__device__ __forceinline__ int stft_owner_by(Key key, int nw, long v) {
    int w = 0;
    for (int lo = 0, hi = nw; hi - lo > 1;) {
        const int mid = (lo + hi) >> 1;
        if (key(mid) <= v) lo = mid; else hi = mid;
        w = lo;
    }
    return w;
}

// the usual key: an offset table, off[w] <= v < off[w + 1]
__device__ __forceinline__ int stft_owner(const long* __restrict__ off, int nw, long v) {
    return stft_owner_by([&](int m) { return off[m]; }, nw, v);
}

// np.pad(mode='reflect') index of a signal of n samples when one reflection is enough (|overhang| < n; callers require n > n_fft / 2)
__device__ __forceinline__ long stft_reflect_once(long j, long n) {
    if (j < 0) j = -j;
    if (j >= n) j = 2 * (n - 1) - j;
    if (j < 0) j = 0;
    return j;
}

// Sample of istft's overlap-add at position q >= 0 of the padded signal, shifted by the window's offset in the frame (q = j + pad - off,
// j the index in the trimmed signal), of a waveform with T frames whose windowed frames [T, win] start at F: entries of the frames
// fh - 3 .. fh that exist and cover q, summed in frame order, divided by the window-square sum of exactly those frames where that
// exceeds float32 tiny (Audio._istft).  fh = q / hop; four frames are all there are while win <= 4 hop.
__device__ __forceinline__ float stft_ola(const float* __restrict__ F, const float* __restrict__ window, int q, int fh, int T, int hop, int win) {
    float v[4], ww[4];
    const int i0 = q - fh * hop;                             // < hop
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int f = fh - 3 + c, idx = i0 + (3 - c) * hop;
        const bool ok = f >= 0 && f < T && idx < win;
        v[c] = ok ? F[(long)f * win + idx] : 0.f;
        ww[c] = ok ? window[idx] : 0.f;
    }
    const float num = ((v[0] + v[1]) + v[2]) + v[3];
    const float den = ((ww[0] * ww[0] + ww[1] * ww[1]) + ww[2] * ww[2]) + ww[3] * ww[3];
    return den > 1.17549435e-38f ? num / den : num;
}

// The real transform of n_fft samples through the complex one of N2 = n_fft / 2 points, z[m] = x[2m] + i x[2m+1], W = e^{-2 pi i / n_fft}
// (tw[k] = W^k).  Bin pairs (k, N2 - k), 1 <= k <= N2 / 2, stay in one thread:
//   split:  X[k] = E + W^k O,  X[N2 - k] = conj(E - W^k O)   with  E = (Z[k] + conj Z[N2-k]) / 2,  O = -i (Z[k] - conj Z[N2-k]) / 2
//   merge:  Z'[k] = E' + i O',  Z'[N2-k] = conj E' + i conj O'  with  E' = (Y[k] + conj Y[N2-k]) / 2,  O' = conj(W^k) (Y[k] - conj Y[N2-k]) / 2
// The inverse transform runs the forward stages on conjugated input, so the merge returns conj Z'.  k = 0 and the Nyquist bin are real
// (irfft ignores their imaginary parts) and share Z[0]: X[0] = Re + Im, X[N2] = Re - Im, and back conj Z'[0] = ((Y0 + Yn) - i (Y0 - Yn)) / 2.
__device__ __forceinline__ void rfft_split(float2 zk, float2 zc, float2 t, float2& xk, float2& xc) {
    const float er = 0.5f * (zk.x + zc.x), ei = 0.5f * (zk.y - zc.y);
    const float orr = 0.5f * (zk.y + zc.y), oi = -0.5f * (zk.x - zc.x);
    const float tr = orr * t.x - oi * t.y, ti = orr * t.y + oi * t.x;
    xk = make_float2(er + tr, ei + ti);
    xc = make_float2(er - tr, -(ei - ti));
}

__device__ __forceinline__ void rfft_merge(float2 yk, float2 yc, float2 t, float2& zk, float2& zc) {
    const float e2r = 0.5f * (yk.x + yc.x), e2i = 0.5f * (yk.y - yc.y);
    const float t2r = 0.5f * (yk.x - yc.x), t2i = 0.5f * (yk.y + yc.y);
    const float o2r = t2r * t.x + t2i * t.y, o2i = t2i * t.x - t2r * t.y;
    zk = make_float2(e2r - o2i, -(e2i + o2r));
    zc = make_float2(e2r + o2i, -(o2r - e2i));
}

__device__ __forceinline__ float2 rfft_split_dc(float2 z0) { return make_float2(z0.x + z0.y, z0.x - z0.y); }       // (X[0], X[N2])
__device__ __forceinline__ float2 rfft_merge_dc(float y0, float yn) { return make_float2(0.5f * (y0 + yn), -0.5f * (y0 - yn)); }

// The tail of a round-trip frame: inverse transform of the conj-packed input in Y (the forward stages; `other` is the second LDS
// buffer), the 1 / N2 scale, and the `win` samples under the window (frame positions off .. off + win) stored windowed to out[win].
__device__ __forceinline__ void stft_frame_tail(float2* Y, float2* other, const float2* __restrict__ tw, int N2, int n_fft, int tid,
                                                const float* __restrict__ window, int off, int win, float* __restrict__ out) {
    float2* R = fft_stockham_stages(Y, other, tw, N2, n_fft, tid);                        // conj of the packed frame, times N2
    const float scale = 1.0f / (float)N2;
    for (int iw = tid; iw < win; iw += 256) {
        const int i = iw + off;
        const float2 z = R[i >> 1];
        out[iw] = window[iw] * (((i & 1) ? -z.y : z.x) * scale);
    }
}

}  // namespace mstts
