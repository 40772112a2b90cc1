// WaveGlow denoiser on gfx950: bias-spectrum subtraction for a whole batch of waveforms (Audio.spectral_denoise is the fp64 statement).
//
//   X_t    = rfft(window * reflect_pad(x)[t hop : t hop + n_fft])                 librosa's stft, center=True, as Audio._stft_samples
//   Y_t[k] = max(|X_t[k]| - strength bias[k], 0) X_t[k] / |X_t[k]|                 (0 where X_t[k] = 0: bias, strength >= 0)
//   y[j]   = sum_t (window * irfft(Y_t))[j + pad - t hop] / sum_t window^2[j + pad - t hop]     the frames that exist there, j < n
//
// Two launches.  A: a workgroup per frame, every waveform of the batch in the same grid (frame g belongs to waveform w with
// frame_off[w] <= g < frame_off[w + 1]): reflect-padded framing as stft_frame_body (csrc/stft_frame.h), the half-size complex FFT in
// LDS (csrc/fft_stages.h), the real-FFT split with the bin pair (k, n_fft/2 - k) in one thread, magnitude / subtract / clamp / rescale
// on the pair, the inverse merge and the inverse FFT as griffin_lim_kernel (csrc/griffin_lim.hip) does them - the spectrum never
// leaves registers and LDS - and the `win` windowed samples stored to the workspace [total_frames, win].  B: y[j] for every sample of
// every waveform, a gather of the at most four workspace entries that cover it, summed in frame order and divided by the window-square
// sum of exactly those frames: no atomics, one fixed summation order, so a waveform gives the same bits alone and in any batch.
// The pieces shared in spirit with audio.hip / griffin_lim.hip are restated here: those two files stay byte-identical.
#include "common.h"
#include "fft_stages.h"

namespace mstts {

// index w with off[w] <= v < off[w + 1] (uniform binary search, as stft_fft_kernel)
__device__ __forceinline__ int dn_owner(const long* __restrict__ off, int nw, long v) {
    int w = 0;
    for (int lo = 0, hi = nw; hi - lo > 1;) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= v) lo = mid; else hi = mid;
        w = lo;
    }
    return w;
}

// max(|X| - sb, 0) / |X|, the factor X is scaled by; 0 where |X| = 0 (the direction (1, 0) times max(-sb, 0) = 0)
__device__ __forceinline__ float dn_gain(float re, float im, float sb) {
    const float m = sqrtf(re * re + im * im);
    return m > 0.f ? fmaxf(m - sb, 0.f) / m : 0.f;
}

__global__ __launch_bounds__(256) void wg_denoise_frames_kernel(const float* __restrict__ wav, const long* __restrict__ wav_off,
                                                                const long* __restrict__ frame_off, int nw, const float* __restrict__ bias,
                                                                float strength, const float* __restrict__ window,
                                                                const float2* __restrict__ tw, int n_fft, int hop, int win,
                                                                float* __restrict__ F) {
    extern __shared__ __attribute__((aligned(16))) float2 dn_lds[];
    const int N2 = n_fft >> 1, tid = threadIdx.x;
    float2* bufa = dn_lds;
    float2* bufb = dn_lds + N2;
    const long g = blockIdx.x;
    const int w = dn_owner(frame_off, nw, g);
    const long f = g - frame_off[w], n = wav_off[w + 1] - wav_off[w];
    const float* x = wav + wav_off[w];
    const int off = (n_fft - win) >> 1, pad = n_fft >> 1;
    auto sample = [&](int i) -> float {                      // windowed, reflect-padded sample i of this frame (n > pad: one reflection)
        if (i < off || i >= off + win) return 0.f;
        long j = f * hop + i - pad;
        if (j < 0) j = -j;
        if (j >= n) j = 2 * (n - 1) - j;
        if (j < 0) j = 0;
        return window[i - off] * x[j];
    };
    for (int m = tid; m < N2; m += 256) bufa[m] = make_float2(sample(2 * m), sample(2 * m + 1));
    __syncthreads();
    float2* Z = fft_stockham_stages(bufa, bufb, tw, N2, n_fft, tid);
    float2* Y = Z == bufa ? bufb : bufa;                     // conj of the packed inverse input
    // bin pairs (k, N2 - k), 1 <= k <= N2 / 2:  X[k] = E + W^k O,  X[N2 - k] = conj(E - W^k O)  with  E = (Z[k] + conj Z[N2-k]) / 2,
    // O = -i (Z[k] - conj Z[N2-k]) / 2;  Y = gain X  and back:  Z'[k] = E' + i O',  Z'[N2-k] = conj E' + i conj O'  with
    // E' = (Y[k] + conj Y[N2-k]) / 2,  O' = conj(W^k) (Y[k] - conj Y[N2-k]) / 2
    for (int k = 1 + tid; k <= (N2 >> 1); k += 256) {
        const int kc = N2 - k;
        const float2 t = tw[k];
        const float2 zk = Z[k], zc = Z[kc];
        const float er = 0.5f * (zk.x + zc.x), ei = 0.5f * (zk.y - zc.y);
        const float orr = 0.5f * (zk.y + zc.y), oi = -0.5f * (zk.x - zc.x);
        const float tr = orr * t.x - oi * t.y, ti = orr * t.y + oi * t.x;
        const float xkr = er + tr, xki = ei + ti, xcr = er - tr, xci = -(ei - ti);
        const float gk = dn_gain(xkr, xki, strength * bias[k]), gc = dn_gain(xcr, xci, strength * bias[kc]);
        const float2 yk = make_float2(gk * xkr, gk * xki), yc = make_float2(gc * xcr, gc * xci);
        const float e2r = 0.5f * (yk.x + yc.x), e2i = 0.5f * (yk.y - yc.y);
        const float t2r = 0.5f * (yk.x - yc.x), t2i = 0.5f * (yk.y + yc.y);
        const float o2r = t2r * t.x + t2i * t.y, o2i = t2i * t.x - t2r * t.y;
        Y[k] = make_float2(e2r - o2i, -(e2i + o2r));
        if (kc != k) Y[kc] = make_float2(e2r + o2i, -(o2r - e2i));
    }
    if (tid == 0) {                                          // k = 0 and the Nyquist bin: real
        const float2 z0 = Z[0];
        const float x0 = z0.x + z0.y, xn = z0.x - z0.y;
        const float y0 = x0 * dn_gain(x0, 0.f, strength * bias[0]), yn = xn * dn_gain(xn, 0.f, strength * bias[N2]);
        Y[0] = make_float2(0.5f * (y0 + yn), -0.5f * (y0 - yn));
    }
    __syncthreads();
    float2* R = fft_stockham_stages(Y, Y == bufa ? bufb : bufa, tw, N2, n_fft, tid);       // conj of the packed frame, times N2
    const float scale = 1.0f / (float)N2;
    float* out = F + g * win;
    for (int iw = tid; iw < win; iw += 256) {
        const int i = iw + off;
        const float2 z = R[i >> 1];
        out[iw] = window[iw] * (((i & 1) ? -z.y : z.x) * scale);
    }
}

// istft with length = n: sample j of waveform w sits at q = j + pad - off of the overlap-add; the frames fh - 3 .. fh (fh = q / hop)
// that exist and cover q are summed in frame order and divided by the window-square sum of exactly those frames where that exceeds
// float32 tiny (gl_ola of csrc/griffin_lim.hip, restated).
__global__ __launch_bounds__(256) void wg_denoise_gather_kernel(const float* __restrict__ F, const long* __restrict__ wav_off,
                                                                const long* __restrict__ frame_off, int nw,
                                                                const float* __restrict__ window, int n_fft, int hop, int win, long first,
                                                                long total, float* __restrict__ y) {
    const int off = (n_fft - win) >> 1, pad = n_fft >> 1;
    for (long r = blockIdx.x * 256L + threadIdx.x; r < total; r += gridDim.x * 256L) {
        const long i = first + r;
        const int w = dn_owner(wav_off, nw, i);
        const long f0 = frame_off[w];
        const int T = (int)(frame_off[w + 1] - f0), q = (int)(i - wav_off[w]) + pad - off, fh = q / hop;
        const float* Fw = F + f0 * win;
        const int i0 = q - fh * hop;                         // < hop
        float v[4], ww[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int f = fh - 3 + c, idx = i0 + (3 - c) * hop;
            const bool ok = f >= 0 && f < T && idx < win;
            v[c] = ok ? Fw[(long)f * win + idx] : 0.f;
            ww[c] = ok ? window[idx] : 0.f;
        }
        const float num = ((v[0] + v[1]) + v[2]) + v[3];
        const float den = ((ww[0] * ww[0] + ww[1] * ww[1]) + ww[2] * ww[2]) + ww[3] * ww[3];
        y[i] = den > 1.17549435e-38f ? num / den : num;
    }
}

}  // namespace mstts
using namespace mstts;

// The gather takes four frames per sample (win <= 4 hop); with 2 hop <= win every one of the n samples lies under at least one window
// (the last frame is centred at most hop - 1 < win / 2 samples before the end of the signal).
extern "C" int mstts_wg_denoise_supported(int32_t n_fft, int32_t hop, int32_t win) {
    return mstts_stft_fft_supported(n_fft, win) && hop >= 1 && 2 * (int64_t)hop <= win && win <= 4 * (int64_t)hop;
}

extern "C" int64_t mstts_wg_denoise_ws_floats(int64_t total_frames, int32_t win) {
    if (total_frames < 0 || win < 0) return 0;
    return total_frames * win;
}

extern "C" int mstts_wg_denoise(const float* wav, const int64_t* wav_off_host, const int64_t* wav_off, const int64_t* frame_off, int32_t nw,
                                const float* bias, float strength, const float* window, const float* twiddle, int32_t n_fft, int32_t hop,
                                int32_t win, float* ws, float* out, mstts_stream_t s) {
    MSTTS_REQUIRE(wav && wav_off_host && wav_off && frame_off && bias && window && twiddle && ws && out, MSTTS_ERR_SHAPE,
                  "wg_denoise: null pointer");
    MSTTS_REQUIRE(mstts_wg_denoise_supported(n_fft, hop, win), MSTTS_ERR_SHAPE,
                  "wg_denoise: n_fft must be a power of two in [512, 4096] and 2 hop <= win <= 4 hop (n_fft %d, hop %d, win %d)", (int)n_fft,
                  (int)hop, (int)win);
    MSTTS_REQUIRE(strength >= 0.f && strength <= 3.0e38f, MSTTS_ERR_SHAPE, "wg_denoise: strength %g is negative or not finite", (double)strength);
    MSTTS_REQUIRE(nw >= 1 && wav_off_host[0] >= 0, MSTTS_ERR_SHAPE, "wg_denoise: waveform count / first offset");
    int64_t frames = 0;
    for (int w = 0; w < nw; ++w) {
        const int64_t n = wav_off_host[w + 1] - wav_off_host[w];
        // one reflection at either end (n > n_fft / 2), and the int arithmetic of the gather (n + n_fft < 2^31)
        MSTTS_REQUIRE(n > n_fft / 2 && n < (1LL << 30), MSTTS_ERR_SHAPE,
                      "wg_denoise: waveform %d has %lld samples (more than n_fft / 2 = %d, fewer than 2^30)", w, (long long)n, (int)(n_fft / 2));
        frames += 1 + n / hop;
    }
    MSTTS_REQUIRE(frames < (1LL << 31) / win, MSTTS_ERR_SHAPE, "wg_denoise: frame count");
    hipStream_t st = (hipStream_t)s;
    hipLaunchKernelGGL(wg_denoise_frames_kernel, dim3((unsigned)frames), dim3(256), sizeof(float2) * (size_t)n_fft, st, wav, (const long*)wav_off,
                       (const long*)frame_off, (int)nw, bias, strength, window, (const float2*)twiddle, (int)n_fft, (int)hop, (int)win, ws);
    MSTTS_CHECK_LAUNCH("wg_denoise frames");
    const long first = (long)wav_off_host[0], samples = (long)(wav_off_host[nw] - wav_off_host[0]);
    long blocks = (samples + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(wg_denoise_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)ws, (const long*)wav_off,
                       (const long*)frame_off, (int)nw, window, (int)n_fft, (int)hop, (int)win, first, samples, out);
    MSTTS_CHECK_LAUNCH("wg_denoise gather");
    return MSTTS_OK;
}
