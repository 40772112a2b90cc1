// Waveform front end on gfx950: what Feeder.load_wav does to decoded samples - polyphase rate conversion, silence trim, scale -
// for a whole batch of waveforms, packed so that the result goes straight into mstts_stft_fft (csrc/audio.hip).
//
//   resample   y[m] = sum_j h[half + m down - j up] x[j]            scipy.signal.resample_poly(x, up, down), zero padding
//   trim       frames [i hop, i hop + frame), kept when 20 log10(max(rms_i, 1e-10) / max(max_i rms_i, 1e-10)) > -top_db;
//              the result is [first hop, min(len, (last + 1) hop))                                   Feeder.load_wav
//   gather     out[off'[w] + i] = x[off[w] + start_w + i] * scale   (scale, or scale / peak_w), off' and the STFT's frame offsets
//              from a scan over the kept lengths
//
// Waveforms lie back to back with device offset arrays, as mstts_stft_fft takes them.  Every output sample and every frame's mean
// square is one sum in one fixed order by one thread (or one wave), nothing is accumulated with atomics: a waveform gives the same
// bits alone or anywhere in a batch.  The only atomics are integer min / max (on frame indices in LDS, on the bit patterns of the
// non-negative mean squares in memory), whose result has no order.
#include "common.h"

namespace mstts {

constexpr int WAV_TILE = 1024;                               // outputs of one waveform per workgroup (4 per thread)
constexpr int WAV_LDS_FLOATS = 16384;                        // 64 KB: phase table + staged input span

// taps per output sample, as the host lays the phase table out: ceil((2 half + 1) / up) made odd (the row stride in LDS: odd =
// the rows of the 32 lanes of a ds_read_b32 group fall on 32 different banks when their phases differ mod 32)
static inline long wav_taps(long up, long down) {
    const long half = 10 * (up > down ? up : down);
    return ((2 * half + 1 + up - 1) / up) | 1;
}
static inline long wav_span(long up, long down) { return ((long)(WAV_TILE - 1) * down) / up + 1 + wav_taps(up, down); }

// Phase table tab[up][T]: tab[p][i] = h[p + (T - 1 - i) up] (0 beyond the filter), so that output m with q = half + m down,
// p = q mod up, jm = q / up is  sum_{i < T} tab[p][i] x[jm - (T - 1) + i]  - ascending j, x = 0 outside [0, n).
__global__ __launch_bounds__(256) void wav_resample_kernel(const float* __restrict__ x, const long* __restrict__ in_off,
                                                           const long* __restrict__ out_off, const float* __restrict__ tab, int up,
                                                           int down, int T, float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float wav_lds[];
    const int w = blockIdx.y, tid = threadIdx.x;
    const long n = in_off[w + 1] - in_off[w], n_out = out_off[w + 1] - out_off[w];
    const long m0 = (long)blockIdx.x * WAV_TILE;
    if (m0 >= n_out) return;                                 // (uniform: the grid is sized for the longest waveform)
    const long m1 = m0 + WAV_TILE < n_out ? m0 + WAV_TILE : n_out;
    const long half = 10L * (up > down ? up : down);
    float* tl = wav_lds;
    float* xs = wav_lds + up * T;
    for (int i = tid; i < up * T; i += 256) tl[i] = tab[i];
    const long j_lo = (half + m0 * down) / up - (T - 1), j_hi = (half + (m1 - 1) * down) / up;
    const int span = (int)(j_hi - j_lo + 1);
    const float* xw = x + in_off[w];
    for (int s = tid; s < span; s += 256) {
        const long j = j_lo + s;
        xs[s] = j >= 0 && j < n ? xw[j] : 0.f;
    }
    __syncthreads();
    float* yw = y + out_off[w];
    for (long m = m0 + tid; m < m1; m += 256) {
        const long q = half + m * down, jm = q / up;
        const int p = (int)(q - jm * up);
        const float* c = tl + p * T;
        const float* v = xs + (int)(jm - (T - 1) - j_lo);
        float acc = 0.f;
        for (int i = 0; i < T; ++i) acc = fmaf(c[i], v[i], acc);
        yw[m] = acc;
    }
}

// mean square of frame i of x: in index order by one thread (frame < 256), or - a wave per frame - lane l sums the elements
// l, l + 64, ... in index order and the 64 partial sums are combined by wave_sum's fixed tree
__device__ __forceinline__ float wav_frame_ms(const float* __restrict__ x, long i, int frame, int hop) {
    const float* f = x + i * hop;
    float a = 0.f;
    for (int k = 0; k < frame; ++k) a = fmaf(f[k], f[k], a);
    return a / (float)frame;
}
__device__ __forceinline__ float wav_frame_ms_wave(const float* __restrict__ x, long i, int frame, int hop, int lane) {
    const float* f = x + i * hop;
    float a = 0.f;
    for (int k = lane; k < frame; k += 64) a = fmaf(f[k], f[k], a);
    return wave_sum(a) / (float)frame;
}

__device__ __forceinline__ bool wav_kept(float ms, float ref, float top_db) {
    const float rms = fmaxf(sqrtf(ms), 1e-10f);
    return 20.f * log10f(rms / ref) > -top_db;
}

// Trim, launch 1: the mean square of every frame.  Workgroup (c, w) owns WAV_TRIM_FRAMES (a wave per frame: WAV_TRIM_WAVE_FRAMES)
// consecutive frames of waveform w, writes them to ms[off[w] - off[0] + i] (a waveform has no more frames than samples) and folds
// their maximum into maxbits[w]: integer atomic max on the bit patterns of non-negative floats, which has no order.
constexpr int WAV_TRIM_FRAMES = 256, WAV_TRIM_WAVE_FRAMES = 16;
__global__ __launch_bounds__(256) void wav_frame_ms_kernel(const float* __restrict__ x, const long* __restrict__ off, int frame, int hop,
                                                           float* __restrict__ ms, unsigned* __restrict__ maxbits) {
    __shared__ float red[16];
    const int w = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long n = off[w + 1] - off[w];
    if (n < frame) return;
    const long nf = 1 + (n - frame) / hop;
    const bool by_wave = frame >= 256;
    const long i0 = (long)blockIdx.x * (by_wave ? WAV_TRIM_WAVE_FRAMES : WAV_TRIM_FRAMES);
    if (i0 >= nf) return;                                    // (uniform)
    const float* xw = x + off[w];
    float* mw = ms + (off[w] - off[0]);
    float mx = 0.f;
    if (by_wave) {
        for (long i = i0 + wv; i < i0 + WAV_TRIM_WAVE_FRAMES && i < nf; i += 4) {
            const float v = wav_frame_ms_wave(xw, i, frame, hop, lane);
            if (lane == 0) mw[i] = v;
            mx = fmaxf(mx, v);
        }
    } else if (i0 + tid < nf) {
        mx = wav_frame_ms(xw, i0 + tid, frame, hop);
        mw[i0 + tid] = mx;
    }
    mx = block_max(mx, red);                                 // (fmaxf drops a NaN frame here; it is never kept below)
    if (tid == 0) atomicMax(&maxbits[w], __float_as_uint(mx));
}

// Trim, launch 2: a workgroup per waveform - the first and last kept frame from the stored mean squares, then max |x| over the kept
// range.  bounds[w] = (start, end) relative to the waveform's first sample.
__global__ __launch_bounds__(1024) void wav_trim_kernel(const float* __restrict__ x, const long* __restrict__ off, int frame, int hop,
                                                        float top_db, const float* __restrict__ ms, const unsigned* __restrict__ maxbits,
                                                        long* __restrict__ bounds, float* __restrict__ peak) {
    __shared__ float red[16];
    __shared__ int first_last[2];
    const int w = blockIdx.x, tid = threadIdx.x;
    const long n = off[w + 1] - off[w];
    const float* xw = x + off[w];
    long start = 0, end = n;
    if (n >= frame) {                                        // (uniform)
        const long nf = 1 + (n - frame) / hop;
        const float* mw = ms + (off[w] - off[0]);
        const float ref = fmaxf(sqrtf(__uint_as_float(maxbits[w])), 1e-10f);
        if (tid == 0) { first_last[0] = 0x7fffffff; first_last[1] = -1; }
        __syncthreads();
        int lo = 0x7fffffff, hi = -1;
        for (long i = tid; i < nf; i += 1024)
            if (wav_kept(mw[i], ref, top_db)) { lo = lo < (int)i ? lo : (int)i; hi = (int)i; }
        if (hi >= 0) { atomicMin(&first_last[0], lo); atomicMax(&first_last[1], hi); }
        __syncthreads();
        if (first_last[1] >= 0) {
            start = (long)first_last[0] * hop;
            end = ((long)first_last[1] + 1) * hop;
            if (end > n) end = n;
        }
    }
    float pk = 0.f;
    for (long j = start + tid; j < end; j += 1024) pk = fmaxf(pk, fabsf(xw[j]));
    pk = block_max(pk, red);
    if (tid == 0) {
        bounds[2 * w] = start;
        bounds[2 * w + 1] = end;
        peak[w] = pk;
    }
}

// One workgroup: exclusive scan over the kept lengths -> sample offsets and STFT frame offsets (1 + len / stft_hop frames each).
// A thread owns a contiguous run of waveforms; the 256 run totals are scanned in LDS.
__global__ __launch_bounds__(256) void wav_offsets_kernel(const long* __restrict__ bounds, int nw, int stft_hop, long* __restrict__ out_off,
                                                          long* __restrict__ frame_off) {
    __shared__ long tot[2][256];
    const int tid = threadIdx.x, per = (nw + 255) / 256;
    const int w0 = tid * per, w1 = w0 + per < nw ? w0 + per : nw;
    long s = 0, f = 0;
    for (int w = w0; w < w1; ++w) {
        const long len = bounds[2 * w + 1] - bounds[2 * w];
        s += len;
        f += 1 + len / stft_hop;
    }
    tot[0][tid] = s; tot[1][tid] = f;
    __syncthreads();
    long bs = 0, bf = 0;
    for (int t = 0; t < tid; ++t) { bs += tot[0][t]; bf += tot[1][t]; }
    for (int w = w0; w < w1; ++w) {
        out_off[w] = bs; frame_off[w] = bf;
        const long len = bounds[2 * w + 1] - bounds[2 * w];
        bs += len;
        bf += 1 + len / stft_hop;
    }
    if (w1 == nw && w0 < nw) { out_off[nw] = bs; frame_off[nw] = bf; }
}

__global__ __launch_bounds__(256) void wav_gather_kernel(const float* __restrict__ x, const long* __restrict__ in_off,
                                                         const long* __restrict__ bounds, const float* __restrict__ peak, float scale,
                                                         int peak_normalize, const long* __restrict__ out_off, float* __restrict__ y) {
    const int w = blockIdx.y;
    const long start = bounds[2 * w], len = bounds[2 * w + 1] - start;
    const long i0 = (long)blockIdx.x * WAV_TILE;
    if (i0 >= len) return;
    float sc = scale;
    if (peak_normalize && peak[w] > 0.f) sc = scale / peak[w];
    const float* src = x + in_off[w] + start;
    float* dst = y + out_off[w];
    const long i1 = i0 + WAV_TILE < len ? i0 + WAV_TILE : len;
    for (long i = i0 + threadIdx.x; i < i1; i += 256) dst[i] = src[i] * sc;
}

}  // namespace mstts
using namespace mstts;

// The phase table and the input span of a tile of WAV_TILE outputs must fit the 64 KB of LDS a workgroup gets by default.
extern "C" int mstts_wav_resample_supported(int32_t up, int32_t down) {
    if (up < 1 || down < 1 || up > 4096 || down > 4096) return 0;
    return (long)up * wav_taps(up, down) + wav_span(up, down) <= WAV_LDS_FLOATS;
}

extern "C" int32_t mstts_wav_resample_taps(int32_t up, int32_t down) {
    return up >= 1 && down >= 1 && up <= 4096 && down <= 4096 ? (int32_t)wav_taps(up, down) : 0;
}

extern "C" int mstts_wav_resample(const float* wav, const int64_t* in_off, const int64_t* out_off, int32_t nw, int64_t max_out,
                                  const float* phase_table, int32_t up, int32_t down, float* out, mstts_stream_t s) {
    MSTTS_REQUIRE(nw >= 1 && nw <= 65535, MSTTS_ERR_SHAPE, "wav_resample: %d waveforms (1 .. 65535)", (int)nw);
    MSTTS_REQUIRE(up >= 1 && down >= 1, MSTTS_ERR_SHAPE, "wav_resample: up = %d, down = %d must be positive", (int)up, (int)down);
    MSTTS_REQUIRE(mstts_wav_resample_supported(up, down), MSTTS_ERR_SHAPE, "wav_resample: %d / %d is outside the supported envelope", (int)up,
                  (int)down);
    MSTTS_REQUIRE(max_out >= 0 && max_out < (1LL << 31), MSTTS_ERR_SHAPE, "wav_resample: longest output");
    MSTTS_REQUIRE(wav && in_off && out_off && phase_table && out, MSTTS_ERR_SHAPE, "wav_resample: null pointer");
    if (max_out == 0) return MSTTS_OK;
    const int T = (int)wav_taps(up, down);
    const size_t lds = sizeof(float) * (size_t)((long)up * T + wav_span(up, down));
    hipLaunchKernelGGL(wav_resample_kernel, dim3((unsigned)cdiv(max_out, WAV_TILE), (unsigned)nw), dim3(256), lds, (hipStream_t)s, wav,
                       (const long*)in_off, (const long*)out_off, phase_table, (int)up, (int)down, T, out);
    MSTTS_CHECK_LAUNCH("wav_resample");
    return MSTTS_OK;
}

// floats of workspace for waveforms of total_samples samples in all: a mean square per frame (no more frames than samples) and the
// largest one per waveform
extern "C" int64_t mstts_wav_trim_ws_floats(int64_t total_samples, int32_t nw) {
    return total_samples < 0 || nw < 0 ? 0 : total_samples + nw;
}

extern "C" int mstts_wav_trim(const float* wav, const int64_t* off, int32_t nw, int64_t total_samples, int64_t max_len, int32_t frame,
                              int32_t hop, float top_db, float* ws, int64_t* bounds, float* peak, mstts_stream_t s) {
    MSTTS_REQUIRE(nw >= 1 && nw <= 65535, MSTTS_ERR_SHAPE, "wav_trim: %d waveforms (1 .. 65535)", (int)nw);
    MSTTS_REQUIRE(frame >= 1 && hop >= 1, MSTTS_ERR_SHAPE, "wav_trim: frame = %d, hop = %d must be positive", (int)frame, (int)hop);
    MSTTS_REQUIRE(max_len >= 0 && max_len <= total_samples && total_samples < (1LL << 40) && max_len < (1LL << 31), MSTTS_ERR_SHAPE,
                  "wav_trim: sample counts");
    MSTTS_REQUIRE(wav && off && ws && bounds && peak, MSTTS_ERR_SHAPE, "wav_trim: null pointer");
    hipStream_t st = (hipStream_t)s;
    unsigned* maxbits = reinterpret_cast<unsigned*>(ws + total_samples);
    if (hipMemsetAsync(maxbits, 0, sizeof(unsigned) * (size_t)nw, st) != hipSuccess)
        return mstts::set_err(MSTTS_ERR_LAUNCH, "wav_trim: clearing the workspace failed");
    if (max_len >= frame) {
        const long nf = 1 + (max_len - frame) / hop;
        hipLaunchKernelGGL(wav_frame_ms_kernel, dim3((unsigned)cdiv(nf, frame >= 256 ? WAV_TRIM_WAVE_FRAMES : WAV_TRIM_FRAMES), (unsigned)nw),
                           dim3(256), 0, st, wav, (const long*)off, (int)frame, (int)hop, ws, maxbits);
        MSTTS_CHECK_LAUNCH("wav_frame_ms");
    }
    hipLaunchKernelGGL(wav_trim_kernel, dim3((unsigned)nw), dim3(1024), 0, st, wav, (const long*)off, (int)frame, (int)hop, top_db,
                       (const float*)ws, (const unsigned*)maxbits, (long*)bounds, peak);
    MSTTS_CHECK_LAUNCH("wav_trim");
    return MSTTS_OK;
}

extern "C" int mstts_wav_gather_scale(const float* wav, const int64_t* in_off, const int64_t* bounds, const float* peak, int32_t nw,
                                      int64_t max_len, float scale, int32_t peak_normalize, int32_t stft_hop, float* out, int64_t* out_off,
                                      int64_t* frame_off, mstts_stream_t s) {
    MSTTS_REQUIRE(nw >= 1 && nw <= 65535, MSTTS_ERR_SHAPE, "wav_gather_scale: %d waveforms (1 .. 65535)", (int)nw);
    MSTTS_REQUIRE(stft_hop >= 1, MSTTS_ERR_SHAPE, "wav_gather_scale: stft_hop = %d must be positive", (int)stft_hop);
    MSTTS_REQUIRE(max_len >= 0 && max_len < (1LL << 31), MSTTS_ERR_SHAPE, "wav_gather_scale: longest waveform");
    MSTTS_REQUIRE(wav && in_off && bounds && out && out_off && frame_off && (peak || !peak_normalize), MSTTS_ERR_SHAPE,
                  "wav_gather_scale: null pointer");
    hipStream_t st = (hipStream_t)s;
    hipLaunchKernelGGL(wav_offsets_kernel, dim3(1), dim3(256), 0, st, (const long*)bounds, (int)nw, (int)stft_hop, (long*)out_off, (long*)frame_off);
    MSTTS_CHECK_LAUNCH("wav_offsets");
    if (max_len == 0) return MSTTS_OK;
    hipLaunchKernelGGL(wav_gather_kernel, dim3((unsigned)cdiv(max_len, WAV_TILE), (unsigned)nw), dim3(256), 0, st, wav, (const long*)in_off,
                       (const long*)bounds, peak, scale, (int)peak_normalize, (const long*)out_off, out);
    MSTTS_CHECK_LAUNCH("wav_gather_scale");
    return MSTTS_OK;
}
