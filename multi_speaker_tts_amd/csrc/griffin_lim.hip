// Griffin-Lim on gfx950: normalised spectrogram -> waveform for a whole batch (Audio.py:15-27,50-60; librosa's stft / istft
// conventions as Audio._stft / _istft of this package restate them).
//
//   A          = (10 ^ ((clip(s, 0, 1) * 100 - 100 + ref_db) / 20)) ^ power                                       Audio.py:24-27,91-99
//   Y_0[k]     = A[k] e^{2 pi i u[k]}                                                                              Audio.py:52-54
//   frame_t    = window * irfft(Y_t)                         only the `win` samples under the window are kept
//   y_t[j]     = sum_f frame_t[f][j + pad - f hop] / sum_f window^2[j + pad - f hop]   (the frames that exist there)  istft
//   Y_{t+1}[k] = A[k] X[k] / |X[k]|,  X = rfft(window * reflect_pad(y_t))                                            Audio.py:56-59
//   wav        = lfilter([1], [1, -preemph], y_iters)                                                               Audio.py:15-16
//
// One launch per iteration, a workgroup per frame, every utterance of the batch in the same grid (frame g belongs to utterance w
// with frame_off[w] <= g < frame_off[w + 1]; its samples start at hop (frame_off[w] - w)).  The overlap-add of istft is a GATHER in
// the consumer: a workgroup sums, in frame order, the at most four entries of the previous iteration's windowed frames that cover
// each of the `win` samples its own window touches - no atomics, one fixed summation order, bit-reproducible.  Both transforms are
// the half-size complex FFT in LDS of stft_fft_kernel (csrc/audio.hip): Stockham radix 4 (+ one radix-2 stage), ping-pong buffers,
// fp64-built twiddles; the inverse runs the same forward stages on conjugated input.  Bin pairs (k, n_fft/2 - k) stay in one thread
// from the forward real-FFT split through phase, magnitude and the inverse merge, so the spectrum never leaves registers.
// A frame is the skeleton wg_denoise_frames_kernel (csrc/wg_denoise.hip) has too, from the pieces of csrc/stft_parts.h: stft_owner,
// fill the frame (here: stft_ola of the previous frames), fft_stockham_stages, rfft_split / rfft_merge (between them, here: phase
// times amplitude), stft_frame_tail.  What this file keeps is its own: the periodic reflection, gl_phase, the amplitudes and the initial phase.
#include "common.h"
#include "stft_parts.h"

namespace mstts {

// X / |X| with (1, 0) for X = 0 (exp(i angle(0))); the components are scaled by a power of two first, so tiny and huge bins keep
// their direction
__device__ __forceinline__ float2 gl_phase(float re, float im) {
    const float s = fmaxf(fabsf(re), fabsf(im));
    if (!(s > 0.f)) return make_float2(1.f, 0.f);
    int e;
    frexpf(s, &e);
    re = ldexpf(re, -e); im = ldexpf(im, -e);
    const float m = sqrtf(re * re + im * im);
    return make_float2(re / m, im / m);
}

__device__ __forceinline__ void gl_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// FIRST: the prepare launch.  A from the normalised spectrogram (stored for the iterations), initial phase from the uniforms
// phase_u [total_frames, NB] or, when that is null, from Philox4x32-10 keyed by the utterance's seed with counter (bin, frame of
// the utterance): 24-bit uniforms, independent of where the utterance sits in the batch.
// !FIRST: one Griffin-Lim iteration, Fin -> Fout.
template <bool FIRST>
__global__ __launch_bounds__(256) void griffin_lim_kernel(const float* __restrict__ spec, const float* __restrict__ phase_u,
                                                          const unsigned long long* __restrict__ seeds, const long* __restrict__ frame_off, int nu,
                                                          const float* __restrict__ window, const float2* __restrict__ tw, int n_fft, int hop,
                                                          int win, float power, float ref_db, float* __restrict__ A,
                                                          const float* __restrict__ Fin, float* __restrict__ Fout) {
    extern __shared__ __attribute__((aligned(16))) float2 gl_lds[];
    const int N2 = n_fft >> 1, NB = N2 + 1, tid = threadIdx.x;
    float2* bufa = gl_lds;
    float2* bufb = gl_lds + N2;
    const long g = blockIdx.x;
    const int w = stft_owner(frame_off, nu, g);
    const long f0 = frame_off[w];
    const int f = (int)(g - f0), T = (int)(frame_off[w + 1] - f0);
    const int off = (n_fft - win) >> 1, pad = n_fft >> 1;
    float* Ag = A + g * NB;
    float2* Z = bufa;                                        // forward transform of the packed frame (!FIRST)
    if (!FIRST) {
        const float* Fu = Fin + f0 * win;
        const int n = hop * (T - 1);                         // samples of the utterance (>= 2)
        auto sample = [&](int i) -> float {                  // windowed sample i of this frame of reflect_pad(istft(previous frames))
            if (i < off || i >= off + win) return 0.f;
            const int iw = i - off;
            int j = f * hop + i - pad, q, fh;
            if (j >= 0 && j < n) {
                q = j + pad - off;
                fh = f + (iw >= hop) + (iw >= 2 * hop) + (iw >= 3 * hop);       // (f hop + iw) / hop, iw < win <= 4 hop
            } else {                                         // np.pad(mode='reflect'): period 2 (n - 1), not stft_reflect_once: n may be 2
                const int per = 2 * (n - 1);
                j %= per;
                if (j < 0) j += per;
                if (j >= n) j = per - j;
                q = j + pad - off;
                fh = q / hop;
            }
            return window[iw] * stft_ola(Fu, window, q, fh, T, hop, win);
        };
        for (int m = tid; m < N2; m += 256) bufa[m] = make_float2(sample(2 * m), sample(2 * m + 1));
        __syncthreads();
        Z = fft_stockham_stages(bufa, bufb, tw, N2, n_fft, tid);
    }
    float2* Y = Z == bufa ? bufb : bufa;                     // conj of the packed inverse input
    // amplitude of bin k of this frame
    auto amp = [&](int k) -> float {
        if (!FIRST) return Ag[k];
        const double s = fmin(fmax((double)spec[g * NB + k], 0.0), 1.0);
        const float a = (float)pow(pow(10.0, (s * 100.0 - 100.0 + (double)ref_db) * 0.05), (double)power);
        Ag[k] = a;
        return a;
    };
    auto initial = [&](int k) -> float2 {                    // e^{2 pi i u}
        float u;
        if (phase_u) u = phase_u[g * NB + k];
        else {
            uint32_t r[4];
            const unsigned long long sd = seeds[w];
            gl_philox((uint32_t)(k >> 2), (uint32_t)f, 0x474c494du, 0u, (uint32_t)sd, (uint32_t)(sd >> 32), r);
            u = (float)(r[k & 3] >> 8) * (1.0f / 16777216.0f);
        }
        float s, c;
        sincospif(2.f * u, &s, &c);
        return make_float2(c, s);
    };
    for (int k = 1 + tid; k <= (N2 >> 1); k += 256) {        // Y = A X / |X| (the prepare launch: A e^{2 pi i u}) on the bin pair (k, N2 - k)
        const int kc = N2 - k;
        const float2 t = tw[k];
        float2 pk, pc, zk, zc;
        if (FIRST) { pk = initial(k); pc = initial(kc); }
        else {
            float2 xk, xc;
            rfft_split(Z[k], Z[kc], t, xk, xc);
            pk = gl_phase(xk.x, xk.y); pc = gl_phase(xc.x, xc.y);
        }
        const float ak = amp(k), ac = amp(kc);
        rfft_merge(make_float2(ak * pk.x, ak * pk.y), make_float2(ac * pc.x, ac * pc.y), t, zk, zc);
        Y[k] = zk;
        if (kc != k) Y[kc] = zc;
    }
    if (tid == 0) {                                          // k = 0 and the Nyquist bin: real
        float p0, pn;
        if (FIRST) { p0 = initial(0).x; pn = initial(N2).x; }
        else {
            const float2 x = rfft_split_dc(Z[0]);
            p0 = gl_phase(x.x, 0.f).x; pn = gl_phase(x.y, 0.f).x;
        }
        Y[0] = rfft_merge_dc(amp(0) * p0, amp(N2) * pn);
    }
    __syncthreads();
    stft_frame_tail(Y, Y == bufa ? bufb : bufa, tw, N2, n_fft, tid, window, off, win, Fout + g * win);
}

// istft of the last frames: y[j] for every sample of every utterance
__global__ __launch_bounds__(256) void gl_overlap_add_kernel(const float* __restrict__ F, const long* __restrict__ frame_off, int nu,
                                                             const float* __restrict__ window, int n_fft, int hop, int win, long total,
                                                             float* __restrict__ y) {
    const int off = (n_fft - win) >> 1, pad = n_fft >> 1;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
        const int w = stft_owner_by([&](int m) { return (frame_off[m] - m) * hop; }, nu, i);       // sample offset of utterance m
        const long f0 = frame_off[w];
        const int T = (int)(frame_off[w + 1] - f0), j = (int)(i - (f0 - w) * hop), q = j + pad - off;
        y[i] = stft_ola(F + f0 * win, window, q, q / hop, T, hop, win);
    }
}

// inv_preemphasis in place, y[n] = x[n] + c y[n-1]: a workgroup per utterance, tiles of 256 x 8 samples.  A thread filters its 8
// samples from a zero state; the states at the ends of the threads' pieces are combined by a Kogge-Stone scan over the lanes
// (y_end = piece_end + c^8 y_before), the waves' ends and the carry of the previous tile in wave order - every sum in a fixed order.
constexpr int GL_SCAN = 8;
__global__ __launch_bounds__(256) void gl_deemphasis_kernel(float* __restrict__ y, const long* __restrict__ frame_off, int hop, float c) {
    __shared__ float lane_pow[64];                           // c^(8 lane)
    __shared__ float wave_end[4];
    const int w = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long f0 = frame_off[w];
    const long n = (frame_off[w + 1] - f0 - 1) * hop;
    float* x = y + (f0 - w) * hop;
    if (tid < 64) lane_pow[tid] = (float)pow((double)c, (double)(GL_SCAN * tid));
    const float c8 = (float)pow((double)c, (double)GL_SCAN), c512 = (float)pow((double)c, 64.0 * GL_SCAN);
    __syncthreads();
    float carry = 0.f;                                       // y just before the tile
    for (long base = 0; base < n; base += 256 * GL_SCAN) {
        const long p0 = base + (long)tid * GL_SCAN;
        float v[GL_SCAN];
        float run = 0.f;
#pragma unroll
        for (int i = 0; i < GL_SCAN; ++i) {
            const float xi = p0 + i < n ? x[p0 + i] : 0.f;
            run = xi + c * run;
            v[i] = run;
        }
        float agg = run, pw = c8;                            // state at the end of lanes [lane - d + 1, lane] from a zero state
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const float o = __shfl_up(agg, d, 64);
            if (lane >= d) agg = agg + pw * o;
            pw *= pw;
        }
        float before = __shfl_up(agg, 1, 64);                // state just before this lane's piece, zero state at the wave's start
        if (lane == 0) before = 0.f;
        if (lane == 63) wave_end[wv] = agg;
        __syncthreads();
        float cw = carry, tile_end = carry;                  // state at the start of this wave / at the end of the tile
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            tile_end = wave_end[k] + c512 * tile_end;
            if (k + 1 == wv) cw = tile_end;
        }
        const float in = before + lane_pow[lane] * cw;
        float pc = c;
#pragma unroll
        for (int i = 0; i < GL_SCAN; ++i) {
            if (p0 + i < n) x[p0 + i] = v[i] + pc * in;
            pc *= c;
        }
        carry = tile_end;
        __syncthreads();
    }
}

}  // namespace mstts
using namespace mstts;

// The gather takes four frames per sample (win <= 4 hop) and assumes no gaps between windows (hop <= win).
extern "C" int mstts_griffin_lim_supported(int32_t n_fft, int32_t hop, int32_t win) {
    return mstts_stft_fft_supported(n_fft, win) && hop >= 1 && hop <= win && win <= 4 * hop;
}

extern "C" int64_t mstts_griffin_lim_ws_floats(int64_t total_frames, int32_t n_fft, int32_t win) {
    if (total_frames < 0 || n_fft < 2 || win < 0) return 0;
    return total_frames * (n_fft / 2 + 1) + 2 * total_frames * win;
}

extern "C" int mstts_griffin_lim(const float* spec, const float* phase_u, const uint64_t* seeds, const int64_t* frame_off_host,
                                 const int64_t* frame_off, int32_t nu, const float* window, const float* twiddle, int32_t n_fft,
                                 int32_t hop, int32_t win, float power, float ref_level_db, float preemph, int32_t iters, float* ws,
                                 float* wav_out, mstts_stream_t s) {
    MSTTS_REQUIRE(spec && (phase_u || seeds) && frame_off_host && frame_off && window && twiddle && ws && wav_out, MSTTS_ERR_SHAPE,
                  "griffin_lim: null pointer");
    MSTTS_REQUIRE(mstts_griffin_lim_supported(n_fft, hop, win), MSTTS_ERR_SHAPE,
                  "griffin_lim: n_fft must be a power of two in [512, 4096] and hop <= win <= 4 hop");
    MSTTS_REQUIRE(nu >= 1 && iters >= 0 && frame_off_host[0] == 0, MSTTS_ERR_SHAPE, "griffin_lim: utterance / iteration count");
    for (int w = 0; w < nu; ++w) {
        const int64_t T = frame_off_host[w + 1] - frame_off_host[w];
        // two samples at least for the reflect padding, and the int arithmetic of the kernels (hop (T - 1) + n_fft < 2^31)
        MSTTS_REQUIRE(T >= 2 && (T - 1) * hop >= 2 && (T - 1) * (int64_t)hop < (1LL << 30), MSTTS_ERR_SHAPE,
                      "griffin_lim: utterance %d has %lld frames (2 frames and 2 samples at least)", w, (long long)T);
    }
    const int64_t total = frame_off_host[nu];
    MSTTS_REQUIRE(total < (1LL << 31) / (win > n_fft / 2 + 1 ? win : n_fft / 2 + 1), MSTTS_ERR_SHAPE, "griffin_lim: frame count");
    hipStream_t st = (hipStream_t)s;
    const int NB = n_fft / 2 + 1;
    float* A = ws;
    float* F[2] = {ws + total * NB, ws + total * NB + total * win};
    const size_t lds = sizeof(float2) * (size_t)n_fft;
    hipLaunchKernelGGL(griffin_lim_kernel<true>, dim3((unsigned)total), dim3(256), lds, st, spec, phase_u, (const unsigned long long*)seeds,
                       (const long*)frame_off, (int)nu, window, (const float2*)twiddle, (int)n_fft, (int)hop, (int)win, power, ref_level_db, A,
                       (const float*)nullptr, F[0]);
    MSTTS_CHECK_LAUNCH("griffin_lim prepare");
    int cur = 0;
    for (int it = 0; it < iters; ++it, cur ^= 1) {
        hipLaunchKernelGGL(griffin_lim_kernel<false>, dim3((unsigned)total), dim3(256), lds, st, (const float*)nullptr, (const float*)nullptr,
                           (const unsigned long long*)nullptr, (const long*)frame_off, (int)nu, window, (const float2*)twiddle, (int)n_fft, (int)hop,
                           (int)win, power, ref_level_db, A, (const float*)F[cur], F[cur ^ 1]);
        MSTTS_CHECK_LAUNCH("griffin_lim iteration");
    }
    const long samples = (long)(total - nu) * hop;
    long blocks = (samples + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(gl_overlap_add_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)F[cur], (const long*)frame_off, (int)nu,
                       window, (int)n_fft, (int)hop, (int)win, samples, wav_out);
    MSTTS_CHECK_LAUNCH("griffin_lim overlap-add");
    hipLaunchKernelGGL(gl_deemphasis_kernel, dim3((unsigned)nu), dim3(256), 0, st, wav_out, (const long*)frame_off, (int)hop, preemph);
    MSTTS_CHECK_LAUNCH("griffin_lim deemphasis");
    return MSTTS_OK;
}
