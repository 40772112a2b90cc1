// WaveGlow denoiser on gfx950: bias-spectrum subtraction for a whole batch of waveforms (Audio.spectral_denoise is the fp64 statement).
//
//   X_t    = rfft(window * reflect_pad(x)[t hop : t hop + n_fft])                 librosa's stft, center=True, as Audio._stft_samples
//   Y_t[k] = max(|X_t[k]| - strength bias[k], 0) X_t[k] / |X_t[k]|                 (0 where X_t[k] = 0: bias, strength >= 0)
//   y[j]   = sum_t (window * irfft(Y_t))[j + pad - t hop] / sum_t window^2[j + pad - t hop]     the frames that exist there, j < n
//
// Two launches.  A: a workgroup per frame, every waveform of the batch in the same grid (frame g belongs to waveform w with
// frame_off[w] <= g < frame_off[w + 1]), the skeleton griffin_lim_kernel (csrc/griffin_lim.hip) has too, from the pieces of
// csrc/stft_parts.h: stft_owner, fill the frame (here: the window times the reflect-padded waveform, stft_reflect_once),
// fft_stockham_stages, rfft_split / rfft_merge with the bin pair (k, n_fft/2 - k) in one thread (between them, here: magnitude /
// subtract / clamp / rescale, dn_gain) - the spectrum never leaves registers and LDS - and stft_frame_tail, which stores the `win`
// windowed samples to the workspace [total_frames, win].  B: y[j] for every sample of every waveform, stft_ola: a gather of the at
// most four workspace entries that cover it, summed in frame order and divided by the window-square sum of exactly those frames: no
// atomics, one fixed summation order, so a waveform gives the same bits alone and in any batch.
#include "common.h"
#include "stft_parts.h"

namespace mstts {

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
    const int w = stft_owner(frame_off, nw, g);
    const long f = g - frame_off[w], n = wav_off[w + 1] - wav_off[w];
    const float* x = wav + wav_off[w];
    const int off = (n_fft - win) >> 1, pad = n_fft >> 1;
    auto sample = [&](int i) -> float {                      // windowed, reflect-padded sample i of this frame (n > pad: one reflection)
        if (i < off || i >= off + win) return 0.f;
        return window[i - off] * x[stft_reflect_once(f * hop + i - pad, n)];
    };
    for (int m = tid; m < N2; m += 256) bufa[m] = make_float2(sample(2 * m), sample(2 * m + 1));
    __syncthreads();
    float2* Z = fft_stockham_stages(bufa, bufb, tw, N2, n_fft, tid);
    float2* Y = Z == bufa ? bufb : bufa;                     // conj of the packed inverse input
    for (int k = 1 + tid; k <= (N2 >> 1); k += 256) {        // Y = gain X on the bin pair (k, N2 - k)
        const int kc = N2 - k;
        const float2 t = tw[k];
        float2 xk, xc, zk, zc;
        rfft_split(Z[k], Z[kc], t, xk, xc);
        const float gk = dn_gain(xk.x, xk.y, strength * bias[k]), gc = dn_gain(xc.x, xc.y, strength * bias[kc]);
        rfft_merge(make_float2(gk * xk.x, gk * xk.y), make_float2(gc * xc.x, gc * xc.y), t, zk, zc);
        Y[k] = zk;
        if (kc != k) Y[kc] = zc;
    }
    if (tid == 0) {                                          // k = 0 and the Nyquist bin: real
        const float2 x = rfft_split_dc(Z[0]);
        Y[0] = rfft_merge_dc(x.x * dn_gain(x.x, 0.f, strength * bias[0]), x.y * dn_gain(x.y, 0.f, strength * bias[N2]));
    }
    __syncthreads();
    stft_frame_tail(Y, Y == bufa ? bufb : bufa, tw, N2, n_fft, tid, window, off, win, F + g * win);
}

// istft with length = n: sample j of waveform w sits at q = j + pad - off of the overlap-add (stft_ola, fh = q / hop)
__global__ __launch_bounds__(256) void wg_denoise_gather_kernel(const float* __restrict__ F, const long* __restrict__ wav_off,
                                                                const long* __restrict__ frame_off, int nw,
                                                                const float* __restrict__ window, int n_fft, int hop, int win, long first,
                                                                long total, float* __restrict__ y) {
    const int off = (n_fft - win) >> 1, pad = n_fft >> 1;
    for (long r = blockIdx.x * 256L + threadIdx.x; r < total; r += gridDim.x * 256L) {
        const long i = first + r;
        const int w = stft_owner(wav_off, nw, i);
        const long f0 = frame_off[w];
        const int T = (int)(frame_off[w + 1] - f0), q = (int)(i - wav_off[w]) + pad - off;
        y[i] = stft_ola(F + f0 * win, window, q, q / hop, T, hop, win);
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
