// Waveform front end by librosa's rules on gfx950 (the second rule set of Feeder.load_wav, rule = "librosa"): a polyphase FIR with a
// host-supplied phase table of any size - resampy's kaiser_best has 130 .. 386 taps and up to 320 rows, 228 KB - and the centred,
// reflect-indexed, power-thresholded silence trim of librosa.effects.trim.  The gather / scale launch of wav_front_end.hip is reused.
//
//   resample   q = origin + m down, p = q mod up, jm = q div up:  y[m] = sum_{i < taps} table[p][i] x[jm - (taps - 1) + i]  (x = 0
//              outside [0, n)) for m < n_valid[w], y[m] = 0 for n_valid[w] <= m < n_out[w]
//   trim       frame i covers x[i hop - pad, i hop - pad + frame), pad = frame / 2, reflect-indexed outside [0, n); kept when
//              10 log10(max(1e-10, ms_i)) - 10 log10(max(1e-10, max_i ms_i)) > -top_db; the result is [first hop, min(n, (last + 1) hop))
//
// Two tilings of the resampler, chosen on the host (mstts_wav_resample_fir_supported):
//   phase-major  a workgroup owns C <= 32 residues of m mod up - which all read the same C rows - over K periods of up outputs: the C rows
//                (row stride taps | 1: the rows of 32 lanes fall on 32 banks) and the input span (K - 1) down + C down / up + taps are
//                staged in LDS once and every row is reused K times.  Serves every table whose C rows and one period's span fit in 64 KB.
//   row-major    a workgroup owns 1024 consecutive outputs; rows and input come from memory through L1 / L2.  Serves everything else of
//                the envelope (up, down <= 4096, up taps <= 2^22), where a single row may be longer than LDS.
// Under either, an output is ONE fmaf chain over i ascending from 0 by one thread, with out-of-range inputs as 0.f and no atomics: a
// waveform gives the same bits alone, anywhere in a batch, and under either tiling.
#include "common.h"

namespace mstts {

constexpr int FIR_LDS_FLOATS = 16384;                        // 64 KB: C rows + the staged input span
constexpr int FIR_C = 32;                                    // residues per workgroup (one per bank of a ds_read_b32 group)
constexpr int FIR_MAX_OUT = 1024;                            // outputs per workgroup (4 per thread)
constexpr int FIR_TILE = 1024;                               // row-major: outputs per workgroup

struct FirPlan { int C, K, span; };                          // K = 0: the phase-major tiling cannot serve this table

// C = min(up, 32) residues, K = the most periods whose span fits beside the rows, at most FIR_MAX_OUT outputs.  The span of K periods
// and C residues is at most (K - 1) down + ceil((C - 1) down / up) + taps inputs (see the kernel); one more is kept for the rounding.
static inline FirPlan fir_plan(long up, long down, long taps) {
    FirPlan p{(int)(up < FIR_C ? up : FIR_C), 0, 0};
    const long rows = (long)p.C * (taps | 1);
    const long one = ((long)(p.C - 1) * down + up - 1) / up + 1 + taps;                    // span of one period
    if (rows + one > FIR_LDS_FLOATS) return p;
    long K = 1 + (FIR_LDS_FLOATS - rows - one) / down;
    if (K > FIR_MAX_OUT / p.C) K = FIR_MAX_OUT / p.C;
    p.K = (int)K;
    p.span = (int)(one + (K - 1) * down);
    return p;
}

// Phase-major.  blockIdx.x = period tile * chunks + chunk; the workgroup owns residues c0 .. c0 + C - 1 of m mod up (chunk) and the periods
// k0 .. k0 + K - 1 (tile): outputs m = (k0 + k) up + c0 + c.  With e_c = origin + (c0 + c) down, output (k, c) reads row e_c mod up
// against the inputs ending at jm = (k0 + k) down + e_c div up.
__global__ __launch_bounds__(256) void wav_fir_phase_kernel(const float* __restrict__ x, const long* __restrict__ in_off,
                                                            const long* __restrict__ out_off, const long* __restrict__ n_valid,
                                                            const float* __restrict__ tab, int up, int down, int T, long origin, int C, int K,
                                                            int chunks, float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float fir_lds[];
    const int w = blockIdx.y, tid = threadIdx.x;
    const long n = in_off[w + 1] - in_off[w], n_out = out_off[w + 1] - out_off[w];
    const long nv = n_valid[w] < n_out ? n_valid[w] : n_out;
    const int c0 = (int)(blockIdx.x % chunks) * C;
    const long k0 = (long)(blockIdx.x / chunks) * K;
    if (k0 * up + c0 >= n_out) return;                       // (uniform: the grid is sized for the longest waveform)
    const int Cw = c0 + C <= up ? C : up - c0;
    const int Ts = T | 1;
    float* tl = fir_lds;
    float* xs = fir_lds + C * Ts;
    for (int c = 0; c < Cw; ++c) {
        const float* row = tab + ((origin + (long)(c0 + c) * down) % up) * T;
        for (int i = tid; i < T; i += 256) tl[c * Ts + i] = row[i];
    }
    const long j_lo = k0 * down + (origin + (long)c0 * down) / up - (T - 1);
    const long j_hi = (k0 + K - 1) * down + (origin + (long)(c0 + Cw - 1) * down) / up;
    const int span = (int)(j_hi - j_lo + 1);                 // <= the plan's span
    const float* xw = x + in_off[w];
    for (int s = tid; s < span; s += 256) {
        const long j = j_lo + s;
        xs[s] = j >= 0 && j < n ? xw[j] : 0.f;
    }
    __syncthreads();
    float* yw = y + out_off[w];
    // thread = (residue c, period group g): the 256 threads form G = 256 / Cp groups (Cp = Cw rounded up to a power of two), group g owns the
    // periods g, g + G, ...; four of them at a time share every row element read from LDS (four independent chains, each ascending in i)
    const int Cp = Cw <= 1 ? 1 : Cw <= 2 ? 2 : Cw <= 4 ? 4 : Cw <= 8 ? 8 : Cw <= 16 ? 16 : 32;
    const int c = tid & (Cp - 1), g = tid / Cp, G = 256 / Cp;
    if (c >= Cw) return;
    const float* r = tl + c * Ts;
    const int base = (int)((origin + (long)(c0 + c) * down) / up - (T - 1) - (j_lo - k0 * down));      // xs index of tap 0 of period k0
    for (int k = g; k < K; k += 4 * G) {
        int kq[4];
        const float* v[4];
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            kq[u] = k + u * G < K ? k + u * G : k;           // (past the tile: recompute period k, store nothing)
            v[u] = xs + base + kq[u] * down;
        }
        for (int i = 0; i < T; ++i) {
            const float ri = r[i];
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = fmaf(ri, v[u][i], acc[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long m = (k0 + kq[u]) * up + c0 + c;
            if ((u == 0 || k + u * G < K) && m < n_out) yw[m] = m < nv ? acc[u] : 0.f;
        }
    }
}

// Row-major: thread t of workgroup (b, w) owns outputs b FIR_TILE + t, + 256, ...; neighbouring lanes read neighbouring inputs and
// each walks its own row.
__global__ __launch_bounds__(256) void wav_fir_row_kernel(const float* __restrict__ x, const long* __restrict__ in_off,
                                                          const long* __restrict__ out_off, const long* __restrict__ n_valid,
                                                          const float* __restrict__ tab, int up, int down, int T, long origin,
                                                          float* __restrict__ y) {
    const int w = blockIdx.y;
    const long n = in_off[w + 1] - in_off[w], n_out = out_off[w + 1] - out_off[w];
    const long nv = n_valid[w] < n_out ? n_valid[w] : n_out;
    const long m0 = (long)blockIdx.x * FIR_TILE;
    if (m0 >= n_out) return;
    const long m1 = m0 + FIR_TILE < n_out ? m0 + FIR_TILE : n_out;
    const float* xw = x + in_off[w];
    float* yw = y + out_off[w];
    for (long m = m0 + threadIdx.x; m < m1; m += 256) {
        float acc = 0.f;
        if (m < nv) {
            const long q = origin + m * down, jm = q / up;
            const float* r = tab + (q - jm * up) * T;
            const long j0 = jm - (T - 1);
            for (int i = 0; i < T; ++i) {
                const long j = j0 + i;
                acc = fmaf(r[i], j >= 0 && j < n ? xw[j] : 0.f, acc);
            }
        }
        yw[m] = acc;
    }
}

__device__ __forceinline__ long wav_reflect(long j, long n) { return j < 0 ? -j : j >= n ? 2 * (n - 1) - j : j; }

// mean square of the centred frame i (n > pad, so that every reflected index lies inside the waveform): in index order by one thread, or -
// a wave per frame - lane l sums the elements l, l + 64, ... in index order and wave_sum's fixed tree combines the 64 partial sums
__device__ __forceinline__ float wav_centred_ms(const float* __restrict__ x, long n, long i, int frame, int hop) {
    const long j0 = i * hop - frame / 2;
    float a = 0.f;
    for (int k = 0; k < frame; ++k) {
        const float v = x[wav_reflect(j0 + k, n)];
        a = fmaf(v, v, a);
    }
    return a / (float)frame;
}
__device__ __forceinline__ float wav_centred_ms_wave(const float* __restrict__ x, long n, long i, int frame, int hop, int lane) {
    const long j0 = i * hop - frame / 2;
    float a = 0.f;
    for (int k = lane; k < frame; k += 64) {
        const float v = x[wav_reflect(j0 + k, n)];
        a = fmaf(v, v, a);
    }
    return wave_sum(a) / (float)frame;
}

__device__ __forceinline__ long wav_centred_frames(long n, int frame, int hop) { return 1 + (n + 2 * (long)(frame / 2) - frame) / hop; }

// Centred trim, launch 1: the mean square of every frame.  Workgroup (c, w) owns 256 (a wave per frame: 16) consecutive frames of
// waveform w, writes them to ms[off[w] - off[0] + w + i] (a waveform of n samples has at most n + 1 frames) and folds their maximum into
// maxbits[w] by integer atomic max on the bit patterns of non-negative floats.
constexpr int WAVC_FRAMES = 256, WAVC_WAVE_FRAMES = 16;
__global__ __launch_bounds__(256) void wav_centred_ms_kernel(const float* __restrict__ x, const long* __restrict__ off, int frame, int hop,
                                                             float* __restrict__ ms, unsigned* __restrict__ maxbits) {
    __shared__ float red[16];
    const int w = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long n = off[w + 1] - off[w];
    if (n <= frame / 2) return;                              // (uniform) nothing to reflect on: launch 2 keeps the whole waveform
    const long nf = wav_centred_frames(n, frame, hop);
    const bool by_wave = frame >= 256;
    const long i0 = (long)blockIdx.x * (by_wave ? WAVC_WAVE_FRAMES : WAVC_FRAMES);
    if (i0 >= nf) return;                                    // (uniform)
    const float* xw = x + off[w];
    float* mw = ms + (off[w] - off[0]) + w;
    float mx = 0.f;
    if (by_wave) {
        for (long i = i0 + wv; i < i0 + WAVC_WAVE_FRAMES && i < nf; i += 4) {
            const float v = wav_centred_ms_wave(xw, n, i, frame, hop, lane);
            if (lane == 0) mw[i] = v;
            mx = fmaxf(mx, v);
        }
    } else if (i0 + tid < nf) {
        mx = wav_centred_ms(xw, n, i0 + tid, frame, hop);
        mw[i0 + tid] = mx;
    }
    mx = block_max(mx, red);                                 // (fmaxf drops a NaN frame here; it is never kept below)
    if (tid == 0) atomicMax(&maxbits[w], __float_as_uint(mx));
}

__device__ __forceinline__ float wav_power_db(float ms) { return 10.f * log10f(fmaxf(1e-10f, ms)); }

// Centred trim, launch 2: a workgroup per waveform - first and last kept frame, then max |x| over the kept range.  n = 0 -> (0, 0);
// 0 < n <= pad -> (0, n); no frame kept -> (0, 0).
__global__ __launch_bounds__(1024) void wav_trim_centred_kernel(const float* __restrict__ x, const long* __restrict__ off, int frame, int hop,
                                                                float top_db, const float* __restrict__ ms,
                                                                const unsigned* __restrict__ maxbits, long* __restrict__ bounds,
                                                                float* __restrict__ peak) {
    __shared__ float red[16];
    __shared__ int first_last[2];
    const int w = blockIdx.x, tid = threadIdx.x;
    const long n = off[w + 1] - off[w];
    const float* xw = x + off[w];
    long start = 0, end = n;
    if (n > frame / 2) {                                     // (uniform)
        const long nf = wav_centred_frames(n, frame, hop);
        const float* mw = ms + (off[w] - off[0]) + w;
        const float ref = wav_power_db(__uint_as_float(maxbits[w]));
        if (tid == 0) { first_last[0] = 0x7fffffff; first_last[1] = -1; }
        __syncthreads();
        int lo = 0x7fffffff, hi = -1;
        for (long i = tid; i < nf; i += 1024)
            if (wav_power_db(mw[i]) - ref > -top_db) { lo = lo < (int)i ? lo : (int)i; hi = (int)i; }
        if (hi >= 0) { atomicMin(&first_last[0], lo); atomicMax(&first_last[1], hi); }
        __syncthreads();
        if (first_last[1] >= 0) {
            start = (long)first_last[0] * hop;
            end = ((long)first_last[1] + 1) * hop;
            if (end > n) end = n;
        } else {
            start = end = 0;
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

}  // namespace mstts
using namespace mstts;

// 0: outside the envelope; 1: served by the row-major tiling only; 2: the phase-major tiling serves it (and is what tiling = 0 takes)
extern "C" int mstts_wav_resample_fir_supported(int32_t up, int32_t down, int32_t taps) {
    if (up < 1 || down < 1 || taps < 1 || up > 4096 || down > 4096 || (long)up * taps > (1L << 22)) return 0;
    return fir_plan(up, down, taps).K > 0 ? 2 : 1;
}

extern "C" int mstts_wav_resample_fir(const float* wav, const int64_t* in_off, const int64_t* out_off, const int64_t* n_valid, int32_t nw,
                                      int64_t max_out, const float* table, int32_t up, int32_t down, int32_t taps, int64_t origin,
                                      int32_t tiling, float* out, mstts_stream_t s) {
    MSTTS_REQUIRE(nw >= 1 && nw <= 65535, MSTTS_ERR_SHAPE, "wav_resample_fir: %d waveforms (1 .. 65535)", (int)nw);
    MSTTS_REQUIRE(up >= 1 && down >= 1 && taps >= 1, MSTTS_ERR_SHAPE, "wav_resample_fir: up = %d, down = %d, taps = %d must be positive", (int)up,
                  (int)down, (int)taps);
    const int can = mstts_wav_resample_fir_supported(up, down, taps);
    MSTTS_REQUIRE(can, MSTTS_ERR_SHAPE, "wav_resample_fir: %d / %d with %d taps is outside the supported envelope", (int)up, (int)down, (int)taps);
    MSTTS_REQUIRE(tiling >= 0 && tiling <= 2 && (tiling != 2 || can == 2), MSTTS_ERR_SHAPE,
                  "wav_resample_fir: tiling = %d (0 = chosen here, 1 = row-major, 2 = phase-major where the table allows it)", (int)tiling);
    MSTTS_REQUIRE(origin >= 0 && origin < (1LL << 40), MSTTS_ERR_SHAPE, "wav_resample_fir: origin");
    MSTTS_REQUIRE(max_out >= 0 && max_out < (1LL << 31), MSTTS_ERR_SHAPE, "wav_resample_fir: longest output");
    MSTTS_REQUIRE(wav && in_off && out_off && n_valid && table && out, MSTTS_ERR_SHAPE, "wav_resample_fir: null pointer");
    if (max_out == 0) return MSTTS_OK;
    if (tiling == 2 || (tiling == 0 && can == 2)) {
        const FirPlan p = fir_plan(up, down, taps);
        const int chunks = cdiv(up, p.C);
        const long tiles = cdiv(cdiv(max_out, up), p.K);
        MSTTS_REQUIRE(tiles * chunks < (1LL << 31), MSTTS_ERR_SHAPE, "wav_resample_fir: grid");
        const size_t lds = sizeof(float) * (size_t)((long)p.C * (taps | 1) + p.span);
        hipLaunchKernelGGL(wav_fir_phase_kernel, dim3((unsigned)(tiles * chunks), (unsigned)nw), dim3(256), lds, (hipStream_t)s, wav,
                           (const long*)in_off, (const long*)out_off, (const long*)n_valid, table, (int)up, (int)down, (int)taps, (long)origin,
                           p.C, p.K, chunks, out);
    } else {
        hipLaunchKernelGGL(wav_fir_row_kernel, dim3((unsigned)cdiv(max_out, FIR_TILE), (unsigned)nw), dim3(256), 0, (hipStream_t)s, wav,
                           (const long*)in_off, (const long*)out_off, (const long*)n_valid, table, (int)up, (int)down, (int)taps, (long)origin,
                           out);
    }
    MSTTS_CHECK_LAUNCH("wav_resample_fir");
    return MSTTS_OK;
}

// floats of workspace: a mean square per frame (a waveform of n samples has at most n + 1 centred frames: hop = 1) and the largest one
// per waveform
extern "C" int64_t mstts_wav_trim_centred_ws_floats(int64_t total_samples, int32_t nw) {
    return total_samples < 0 || nw < 0 ? 0 : total_samples + 2 * (int64_t)nw;
}

extern "C" int mstts_wav_trim_centred(const float* wav, const int64_t* off, int32_t nw, int64_t total_samples, int64_t max_len, int32_t frame,
                                      int32_t hop, float top_db, float* ws, int64_t* bounds, float* peak, mstts_stream_t s) {
    MSTTS_REQUIRE(nw >= 1 && nw <= 65535, MSTTS_ERR_SHAPE, "wav_trim_centred: %d waveforms (1 .. 65535)", (int)nw);
    MSTTS_REQUIRE(frame >= 1 && hop >= 1, MSTTS_ERR_SHAPE, "wav_trim_centred: frame = %d, hop = %d must be positive", (int)frame, (int)hop);
    MSTTS_REQUIRE(max_len >= 0 && max_len <= total_samples && total_samples < (1LL << 40) && max_len < (1LL << 31) - 1, MSTTS_ERR_SHAPE,
                  "wav_trim_centred: sample counts");
    MSTTS_REQUIRE(wav && off && ws && bounds && peak, MSTTS_ERR_SHAPE, "wav_trim_centred: null pointer");
    hipStream_t st = (hipStream_t)s;
    unsigned* maxbits = reinterpret_cast<unsigned*>(ws + total_samples + nw);
    if (hipMemsetAsync(maxbits, 0, sizeof(unsigned) * (size_t)nw, st) != hipSuccess)
        return mstts::set_err(MSTTS_ERR_LAUNCH, "wav_trim_centred: clearing the workspace failed");
    if (max_len > frame / 2) {
        const long nf = 1 + (max_len + 2 * (long)(frame / 2) - frame) / hop;
        hipLaunchKernelGGL(wav_centred_ms_kernel, dim3((unsigned)cdiv(nf, frame >= 256 ? WAVC_WAVE_FRAMES : WAVC_FRAMES), (unsigned)nw), dim3(256),
                           0, st, wav, (const long*)off, (int)frame, (int)hop, ws, maxbits);
        MSTTS_CHECK_LAUNCH("wav_centred_ms");
    }
    hipLaunchKernelGGL(wav_trim_centred_kernel, dim3((unsigned)nw), dim3(1024), 0, st, wav, (const long*)off, (int)frame, (int)hop, top_db,
                       (const float*)ws, (const unsigned*)maxbits, (long*)bounds, peak);
    MSTTS_CHECK_LAUNCH("wav_trim_centred");
    return MSTTS_OK;
}
