// Waveform front end on gfx950: what Feeder.load_wav does to decoded samples - polyphase rate conversion, silence trim, scale -
// for a whole batch of waveforms, packed so that the result goes straight into mstts_stft_fft (csrc/audio.hip).  Both rule sets
// of Feeder.load_wav: "scipy" (resample_poly, uncentred RMS trim) and "librosa" (kaiser_best, centred power trim).  The trim is one
// pipeline under two rule structs, the gather is shared, and the resampler is one sum with three kernels: the two FIR tilings below and
// the default rule's own (wav_resample_kernel), which all give the same bits where more than one serves a table.
//
//   resample   q = origin + m down, p = q mod up, jm = q div up:  y[m] = sum_{i < taps} table[p][i] x[jm - (taps - 1) + i]  (x = 0
//              outside [0, n)) for m < n_valid[w], y[m] = 0 for n_valid[w] <= m < n_out[w]; the table [up][taps] comes from the host.
//              scipy.signal.resample_poly(x, up, down) is this at origin = half = 10 max(up, down), table[p][i] = h[p + (taps - 1 - i) up],
//              every output valid; resampy's kaiser_best at origin = L up, taps = 2 L
//   trim       frame i covers x[i hop - pad, i hop - pad + frame); the result is [first hop, min(len, (last + 1) hop)) of the kept frames
//              uncentred RMS (Feeder.load_wav): pad = 0, kept when 20 log10(max(rms_i, 1e-10) / max(max_i rms_i, 1e-10)) > -top_db
//              centred power (librosa.effects.trim): pad = frame / 2, reflect-indexed outside [0, n), kept when
//              10 log10(max(1e-10, ms_i)) - 10 log10(max(1e-10, max_i ms_i)) > -top_db
//   gather     out[off'[w] + i] = x[off[w] + start_w + i] * scale   (scale, or scale / peak_w), off' and the STFT's frame offsets
//              from a scan over the kept lengths
//
// Two tilings of mstts_wav_resample_fir, chosen on the host (mstts_wav_resample_fir_supported):
//   phase-major  a workgroup owns C <= 32 residues of m mod up - which all read the same C rows - over K periods of up outputs: the C rows
//                (row stride taps | 1: the rows of 32 lanes fall on 32 banks) and the input span (K - 1) down + C down / up + taps are
//                staged in LDS once and every row is reused K times.  Serves every table whose C rows and one period's span fit in 64 KB.
//   row-major    a workgroup owns 1024 consecutive outputs; rows and input come from memory through L1 / L2.  Serves everything else of
//                the envelope (up, down <= 4096, up taps <= 2^22), where a single row may be longer than LDS.
//
// Waveforms lie back to back with device offset arrays, as mstts_stft_fft takes them.  Every output sample is ONE fmaf chain over i
// ascending from 0 by one thread, with out-of-range inputs as 0.f, and every frame's mean square is one sum in one fixed order by one
// thread (or one wave); nothing is accumulated with atomics: a waveform gives the same bits alone, anywhere in a batch, and under either
// tiling.  The only atomics are integer min / max (on frame indices in LDS, on the bit patterns of the non-negative mean squares in
// memory), whose result has no order.
#include "common.h"

namespace mstts {

constexpr int WAV_TILE = 1024;                               // outputs of one waveform per workgroup (4 per thread)
constexpr int WAV_LDS_FLOATS = 16384;                        // 64 KB: (phase table or C rows of it) + the staged input span
constexpr int FIR_C = 32;                                    // residues per workgroup (one per bank of a ds_read_b32 group)

// taps per output sample of the default rule, as the host lays its phase table out: ceil((2 half + 1) / up) made odd (the row stride
// in LDS: odd = the rows of the 32 lanes of a ds_read_b32 group fall on 32 different banks when their phases differ mod 32)
static inline long wav_taps(long up, long down) {
    const long half = 10 * (up > down ? up : down);
    return ((2 * half + 1 + up - 1) / up) | 1;
}
static inline long wav_span(long up, long down) { return ((long)(WAV_TILE - 1) * down) / up + 1 + wav_taps(up, down); }

// The default rule's own kernel: the FIR below at origin = half = 10 max(up, down), T = wav_taps, every output valid, with the WHOLE
// phase table tab[up][T] (tab[p][i] = h[p + (T - 1 - i) up], 0 beyond the filter) staged beside the input span of a tile of WAV_TILE
// consecutive outputs.  Output m with q = half + m down, p = q mod up, jm = q / up is  sum_{i < T} tab[p][i] x[jm - (T - 1) + i]  -
// the same fmaf chain, hence the same bits, as either FIR tiling; its short tables (T <= 61) are cheaper staged whole than by residue.
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

struct FirPlan { int C, K, span; };                          // K = 0: the phase-major tiling cannot serve this table

// C = min(up, 32) residues, K = the most periods whose span fits beside the rows, at most WAV_TILE outputs.  The span of K periods
// and C residues is at most (K - 1) down + ceil((C - 1) down / up) + taps inputs (see the kernel); one more is kept for the rounding.
static inline FirPlan fir_plan(long up, long down, long taps) {
    FirPlan p{(int)(up < FIR_C ? up : FIR_C), 0, 0};
    const long rows = (long)p.C * (taps | 1);
    const long one = ((long)(p.C - 1) * down + up - 1) / up + 1 + taps;                    // span of one period
    if (rows + one > WAV_LDS_FLOATS) return p;
    long K = 1 + (WAV_LDS_FLOATS - rows - one) / down;
    if (K > WAV_TILE / p.C) K = WAV_TILE / p.C;
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

// Row-major: thread t of workgroup (b, w) owns outputs b WAV_TILE + t, + 256, ...; neighbouring lanes read neighbouring inputs and
// each walks its own row.
__global__ __launch_bounds__(256) void wav_fir_row_kernel(const float* __restrict__ x, const long* __restrict__ in_off,
                                                          const long* __restrict__ out_off, const long* __restrict__ n_valid,
                                                          const float* __restrict__ tab, int up, int down, int T, long origin,
                                                          float* __restrict__ y) {
    const int w = blockIdx.y;
    const long n = in_off[w + 1] - in_off[w], n_out = out_off[w + 1] - out_off[w];
    const long nv = n_valid[w] < n_out ? n_valid[w] : n_out;
    const long m0 = (long)blockIdx.x * WAV_TILE;
    if (m0 >= n_out) return;
    const long m1 = m0 + WAV_TILE < n_out ? m0 + WAV_TILE : n_out;
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

// The two trim rules: what the mean-square and the bounds kernel below do not share.
struct TrimUncentredRms {                                    // Feeder.load_wav
    static constexpr const char* ms_name = "wav_frame_ms";
    static constexpr const char* name = "wav_trim";
    static constexpr int slots = 0;                          // a waveform has no more frames than samples
    static constexpr bool none_kept_keeps_all = true;
    __host__ __device__ static bool framed(long n, int frame) { return n >= frame; }       // else: no frame pass, the whole waveform is kept
    __host__ __device__ static long frames(long n, int frame, int hop) { return 1 + (n - frame) / hop; }
    __device__ static int pad(int) { return 0; }
    __device__ static long at(long j, long) { return j; }
    __device__ static float ref(float max_ms) { return fmaxf(sqrtf(max_ms), 1e-10f); }
    __device__ static bool kept(float ms, float ref, float top_db) { return 20.f * log10f(fmaxf(sqrtf(ms), 1e-10f) / ref) > -top_db; }
};
struct TrimCentredPower {                                    // librosa.effects.trim
    static constexpr const char* ms_name = "wav_centred_ms";
    static constexpr const char* name = "wav_trim_centred";
    static constexpr int slots = 1;                          // a waveform of n samples has at most n + 1 frames (hop = 1)
    static constexpr bool none_kept_keeps_all = false;       // (0, 0)
    __host__ __device__ static bool framed(long n, int frame) { return n > frame / 2; }    // else: nothing to reflect on
    __host__ __device__ static long frames(long n, int frame, int hop) { return 1 + (n + 2 * (long)(frame / 2) - frame) / hop; }
    __device__ static int pad(int frame) { return frame / 2; }
    __device__ static long at(long j, long n) { return j < 0 ? -j : j >= n ? 2 * (n - 1) - j : j; }      // n > pad: inside the waveform
    __device__ static float db(float ms) { return 10.f * log10f(fmaxf(1e-10f, ms)); }
    __device__ static float ref(float max_ms) { return db(max_ms); }
    __device__ static bool kept(float ms, float ref, float top_db) { return db(ms) - ref > -top_db; }
};

// sum of squares of the elements k0, k0 + step, ... of frame i, in index order
template <class Rule>
__device__ __forceinline__ float wav_frame_squares(const float* __restrict__ x, long n, long i, int frame, int hop, int k0, int step) {
    const long j0 = i * hop - Rule::pad(frame);
    float a = 0.f;
    for (int k = k0; k < frame; k += step) {
        const float v = x[Rule::at(j0 + k, n)];
        a = fmaf(v, v, a);
    }
    return a;
}

// Trim, launch 1: the mean square of every frame.  Workgroup (c, w) owns WAV_TRIM_FRAMES consecutive frames of waveform w, a thread per
// frame - or, from 256 samples a frame on, WAV_TRIM_WAVE_FRAMES of them, a wave per frame: lane l sums the elements l, l + 64, ... and
// wave_sum's fixed tree combines the 64 partial sums.  It writes them to ms[off[w] - off[0] + slots w + i] and folds their maximum into
// maxbits[w]: integer atomic max on the bit patterns of non-negative floats, which has no order.
constexpr int WAV_TRIM_FRAMES = 256, WAV_TRIM_WAVE_FRAMES = 16;
template <class Rule>
__global__ __launch_bounds__(256) void wav_frame_ms_kernel(const float* __restrict__ x, const long* __restrict__ off, int frame, int hop,
                                                           float* __restrict__ ms, unsigned* __restrict__ maxbits) {
    __shared__ float red[16];
    const int w = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long n = off[w + 1] - off[w];
    if (!Rule::framed(n, frame)) return;                     // (uniform)
    const long nf = Rule::frames(n, frame, hop);
    const bool by_wave = frame >= 256;
    const long i0 = (long)blockIdx.x * (by_wave ? WAV_TRIM_WAVE_FRAMES : WAV_TRIM_FRAMES);
    if (i0 >= nf) return;                                    // (uniform)
    const float* xw = x + off[w];
    float* mw = ms + (off[w] - off[0]) + Rule::slots * w;
    float mx = 0.f;
    if (by_wave) {
        for (long i = i0 + wv; i < i0 + WAV_TRIM_WAVE_FRAMES && i < nf; i += 4) {
            const float v = wave_sum(wav_frame_squares<Rule>(xw, n, i, frame, hop, lane, 64)) / (float)frame;
            if (lane == 0) mw[i] = v;
            mx = fmaxf(mx, v);
        }
    } else if (i0 + tid < nf) {
        mx = wav_frame_squares<Rule>(xw, n, i0 + tid, frame, hop, 0, 1) / (float)frame;
        mw[i0 + tid] = mx;
    }
    mx = block_max(mx, red);                                 // (fmaxf drops a NaN frame here; it is never kept below)
    if (tid == 0) atomicMax(&maxbits[w], __float_as_uint(mx));
}

// Trim, launch 2: a workgroup per waveform - the first and last kept frame from the stored mean squares, then max |x| over the kept
// range.  bounds[w] = (start, end) relative to the waveform's first sample; a waveform without frames is kept whole.
template <class Rule>
__global__ __launch_bounds__(1024) void wav_trim_kernel(const float* __restrict__ x, const long* __restrict__ off, int frame, int hop,
                                                        float top_db, const float* __restrict__ ms, const unsigned* __restrict__ maxbits,
                                                        long* __restrict__ bounds, float* __restrict__ peak) {
    __shared__ float red[16];
    __shared__ int first_last[2];
    const int w = blockIdx.x, tid = threadIdx.x;
    const long n = off[w + 1] - off[w];
    const float* xw = x + off[w];
    long start = 0, end = n;
    if (Rule::framed(n, frame)) {                            // (uniform)
        const long nf = Rule::frames(n, frame, hop);
        const float* mw = ms + (off[w] - off[0]) + Rule::slots * w;
        const float ref = Rule::ref(__uint_as_float(maxbits[w]));
        if (tid == 0) { first_last[0] = 0x7fffffff; first_last[1] = -1; }
        __syncthreads();
        int lo = 0x7fffffff, hi = -1;
        for (long i = tid; i < nf; i += 1024)
            if (Rule::kept(mw[i], ref, top_db)) { lo = lo < (int)i ? lo : (int)i; hi = (int)i; }
        if (hi >= 0) { atomicMin(&first_last[0], lo); atomicMax(&first_last[1], hi); }
        __syncthreads();
        if (first_last[1] >= 0) {
            start = (long)first_last[0] * hop;
            end = ((long)first_last[1] + 1) * hop;
            if (end > n) end = n;
        } else if (!Rule::none_kept_keeps_all) {
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

// Both trim entries end here, their arguments checked.  Workspace: total_samples + slots nw mean squares, then the largest one per waveform.
template <class Rule>
static int trim_launch(const float* wav, const int64_t* off, int nw, int64_t total_samples, int64_t max_len, int frame, int hop, float top_db,
                       float* ws, int64_t* bounds, float* peak, mstts_stream_t s) {
    hipStream_t st = (hipStream_t)s;
    unsigned* maxbits = reinterpret_cast<unsigned*>(ws + total_samples + Rule::slots * nw);
    if (hipMemsetAsync(maxbits, 0, sizeof(unsigned) * (size_t)nw, st) != hipSuccess)
        return set_err(MSTTS_ERR_LAUNCH, "%s: clearing the workspace failed", Rule::name);
    if (Rule::framed(max_len, frame)) {
        const long nf = Rule::frames(max_len, frame, hop);
        hipLaunchKernelGGL(wav_frame_ms_kernel<Rule>, dim3((unsigned)cdiv(nf, frame >= 256 ? WAV_TRIM_WAVE_FRAMES : WAV_TRIM_FRAMES), (unsigned)nw),
                           dim3(256), 0, st, wav, (const long*)off, frame, hop, ws, maxbits);
        MSTTS_CHECK_LAUNCH(Rule::ms_name);
    }
    hipLaunchKernelGGL(wav_trim_kernel<Rule>, dim3((unsigned)nw), dim3(1024), 0, st, wav, (const long*)off, frame, hop, top_db,
                       (const float*)ws, (const unsigned*)maxbits, (long*)bounds, peak);
    MSTTS_CHECK_LAUNCH(Rule::name);
    return MSTTS_OK;
}

}  // namespace mstts
using namespace mstts;

// The phase table and the input span of a tile of WAV_TILE outputs must fit the 64 KB of LDS a workgroup gets by default.  Every other
// ratio is converted on the host, so this answer decides results.
extern "C" int mstts_wav_resample_supported(int32_t up, int32_t down) {
    if (up < 1 || down < 1 || up > 4096 || down > 4096) return 0;
    return (long)up * wav_taps(up, down) + wav_span(up, down) <= WAV_LDS_FLOATS;
}

extern "C" int32_t mstts_wav_resample_taps(int32_t up, int32_t down) {
    return up >= 1 && down >= 1 && up <= 4096 && down <= 4096 ? (int32_t)wav_taps(up, down) : 0;
}

// 0: outside the envelope; 1: served by the row-major tiling only; 2: the phase-major tiling serves it (and is what tiling = 0 takes)
extern "C" int mstts_wav_resample_fir_supported(int32_t up, int32_t down, int32_t taps) {
    if (up < 1 || down < 1 || taps < 1 || up > 4096 || down > 4096 || (long)up * taps > (1L << 22)) return 0;
    return fir_plan(up, down, taps).K > 0 ? 2 : 1;
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
        hipLaunchKernelGGL(wav_fir_row_kernel, dim3((unsigned)cdiv(max_out, WAV_TILE), (unsigned)nw), dim3(256), 0, (hipStream_t)s, wav,
                           (const long*)in_off, (const long*)out_off, (const long*)n_valid, table, (int)up, (int)down, (int)taps, (long)origin,
                           out);
    }
    MSTTS_CHECK_LAUNCH("wav_resample_fir");
    return MSTTS_OK;
}

// floats of workspace for waveforms of total_samples samples in all: a mean square per frame and the largest one per waveform
extern "C" int64_t mstts_wav_trim_ws_floats(int64_t total_samples, int32_t nw) {
    return total_samples < 0 || nw < 0 ? 0 : total_samples + nw;
}
extern "C" int64_t mstts_wav_trim_centred_ws_floats(int64_t total_samples, int32_t nw) {
    return total_samples < 0 || nw < 0 ? 0 : total_samples + 2 * (int64_t)nw;
}

extern "C" int mstts_wav_trim(const float* wav, const int64_t* off, int32_t nw, int64_t total_samples, int64_t max_len, int32_t frame,
                              int32_t hop, float top_db, float* ws, int64_t* bounds, float* peak, mstts_stream_t s) {
    MSTTS_REQUIRE(nw >= 1 && nw <= 65535, MSTTS_ERR_SHAPE, "wav_trim: %d waveforms (1 .. 65535)", (int)nw);
    MSTTS_REQUIRE(frame >= 1 && hop >= 1, MSTTS_ERR_SHAPE, "wav_trim: frame = %d, hop = %d must be positive", (int)frame, (int)hop);
    MSTTS_REQUIRE(max_len >= 0 && max_len <= total_samples && total_samples < (1LL << 40) && max_len < (1LL << 31), MSTTS_ERR_SHAPE,
                  "wav_trim: sample counts");
    MSTTS_REQUIRE(wav && off && ws && bounds && peak, MSTTS_ERR_SHAPE, "wav_trim: null pointer");
    return trim_launch<TrimUncentredRms>(wav, off, nw, total_samples, max_len, frame, hop, top_db, ws, bounds, peak, s);
}

extern "C" int mstts_wav_trim_centred(const float* wav, const int64_t* off, int32_t nw, int64_t total_samples, int64_t max_len, int32_t frame,
                                      int32_t hop, float top_db, float* ws, int64_t* bounds, float* peak, mstts_stream_t s) {
    MSTTS_REQUIRE(nw >= 1 && nw <= 65535, MSTTS_ERR_SHAPE, "wav_trim_centred: %d waveforms (1 .. 65535)", (int)nw);
    MSTTS_REQUIRE(frame >= 1 && hop >= 1, MSTTS_ERR_SHAPE, "wav_trim_centred: frame = %d, hop = %d must be positive", (int)frame, (int)hop);
    MSTTS_REQUIRE(max_len >= 0 && max_len <= total_samples && total_samples < (1LL << 40) && max_len < (1LL << 31) - 1, MSTTS_ERR_SHAPE,
                  "wav_trim_centred: sample counts");
    MSTTS_REQUIRE(wav && off && ws && bounds && peak, MSTTS_ERR_SHAPE, "wav_trim_centred: null pointer");
    return trim_launch<TrimCentredPower>(wav, off, nw, total_samples, max_len, frame, hop, top_db, ws, bounds, peak, s);
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
