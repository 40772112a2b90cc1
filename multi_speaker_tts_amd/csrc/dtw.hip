// Batched dynamic time warping and the cepstra of the model's mels on gfx950; dtw.dtw_host / dtw.mel_cepstra_host are the fp64 statements.
// fp32, explicit fmaf, every sum in one fixed order, no atomics: the same inputs give the same bits, for a pair alone or inside any batch
// (a cell's arithmetic depends on neither the block size nor the pair's place in the batch).
//
//   d[i,j] = sqrt(sum_k (a[i,k] - b[j,k])^2), the sum over k = 0 ... K - 1 in that order (identical frames: an exact 0)
//   D[0,0] = d[0,0];  D[i,j] = min(D[i-1,j-1] + w d[i,j], D[i-1,j] + d[i,j], D[i,j-1] + d[i,j]), a missing neighbour left out (+inf here),
//   the first minimum in that order wins; L[i,j] = 1 + L of the chosen neighbour, L[0,0] = 1.
//
// dtw_kernel: ONE workgroup owns one pair from start to finish, thread i owns row i, step t works on the anti-diagonal i + j = t.  A
//   row's left neighbour D[i,j-1] is the thread's own previous value and its diagonal neighbour D[i-1,j-1] is the "up" value it read one
//   step earlier, so a step costs one LDS read (D, L of row i - 1 on diagonal t - 1), one LDS write and one __syncthreads() - two rotating
//   diagonals of (D, L), 16 KB; the NEXT step's distance is computed in front of the barrier.  Nothing waits on another workgroup, there is no flag and no spin; every trip count is n, m or k.
//   K <= 16 (the cepstral case) is FUSED: a_i sits in 16 registers, b lies k-major in LDS (64 KB, both padded with zeros to 16 features;
//   lane i reads b[k][t - i], consecutive banks) and no distance plane exists.  Wider K takes two passes: dtw_dist_kernel writes the distances DIAGONAL-MAJOR, plane[t * n + i],
//   so that the lanes of diagonal t read consecutive floats (a row-major [N, M] plane would be read with stride M - 1).
//   The direction bytes, written only when a path is asked for, are diagonal-major as well.  The backtrack is the last row's thread alone:
//   at most n + m - 1 steps whatever the bytes hold, its indices clamped to the pair's rectangle, rows written back to front into the
//   pair's slot from the known length.
// mel_cepstra_kernel: 16 mel rows per workgroup, the weight table [n_cep, n_mel] (built on the host in fp64: orthonormal DCT-II rows
//   1 ... n_cep over sqrt(2), times the slope of the inverse normalisation; the constant of that map meets rows that sum to zero) in LDS.
#include "common.h"

namespace mstts {

constexpr int DTW_MAX_LEN = 1024, DTW_MAX_K = 128, DTW_FUSED_K = 16, DTW_MAX_PAIRS = 65535;
constexpr int CEP_MAX_MEL = 128, CEP_MAX_CEP = 40, CEP_ROWS = 16;

__global__ __launch_bounds__(256) void dtw_dist_kernel(const float* __restrict__ a, const float* __restrict__ b, const int64_t* __restrict__ offs,
                                                       int pairs, int k, float* __restrict__ dist, long plane) {
    const int p = blockIdx.x, tid = threadIdx.x;
    const long a0 = offs[p], b0 = offs[pairs + 1 + p];
    const int n = min((int)(offs[p + 1] - a0), DTW_MAX_LEN), m = min((int)(offs[pairs + 2 + p] - b0), DTW_MAX_LEN);
    float* out = dist + (long)p * plane;
    for (int t = blockIdx.y; t < n + m - 1; t += gridDim.y) {
        const int lo = max(0, t - m + 1), hi = min(n - 1, t);
        for (int i = lo + tid; i <= hi; i += 256) {
            const float* ai = a + (a0 + i) * k;
            const float* bj = b + (b0 + (t - i)) * k;
            float s = 0.f;
            for (int kk = 0; kk < k; ++kk) {
                const float x = ai[kk] - bj[kk];
                s = fmaf(x, x, s);
            }
            out[(long)t * n + i] = sqrtf(s);
        }
    }
}

template <bool FUSED>
__global__ __launch_bounds__(1024) void dtw_kernel(const float* __restrict__ a, const float* __restrict__ b, const int64_t* __restrict__ offs,
                                                   int pairs, int k, float w, const float* __restrict__ dist, uint8_t* __restrict__ dir, long plane,
                                                   float* __restrict__ cost, int32_t* __restrict__ length, int32_t* __restrict__ path) {
    __shared__ float2 sDL[2][DTW_MAX_LEN];                                // (D, the bits of L) of the last two diagonals, by row
    __shared__ float sB[FUSED ? DTW_FUSED_K * DTW_MAX_LEN : 1];          // b, k-major: sB[kk * 1024 + j], rows k ... 15 zero
    const int p = blockIdx.x, i = threadIdx.x;
    const long a0 = offs[p], b0 = offs[pairs + 1 + p];
    const int n = min((int)(offs[p + 1] - a0), DTW_MAX_LEN), m = min((int)(offs[pairs + 2 + p] - b0), DTW_MAX_LEN);
    float ar[DTW_FUSED_K];
    if (FUSED) {
        // a and b are padded with zeros to 16 features: (0 - 0)^2 adds an exact 0 to a sum that is never negative, so the padded
        // sum has the bits of the k-term one, and the 16 LDS reads of a cell are issued back to back with no branch between them
#pragma unroll
        for (int kk = 0; kk < DTW_FUSED_K; ++kk) ar[kk] = (i < n && kk < k) ? a[(a0 + i) * k + kk] : 0.f;
        for (int idx = i; idx < m * k; idx += blockDim.x) sB[(idx % k) * DTW_MAX_LEN + idx / k] = b[b0 * k + idx];
        for (int idx = i; idx < m * (DTW_FUSED_K - k); idx += blockDim.x) sB[(k + idx / m) * DTW_MAX_LEN + idx % m] = 0.f;
    }
    __syncthreads();
    const float* dp = FUSED ? nullptr : dist + (long)p * plane;
    uint8_t* dirp = dir ? dir + (long)p * plane : nullptr;
    auto local = [&](int t) -> float {          // d[i, t - i] where that cell exists
        const int j = t - i;
        if (!(i < n && j >= 0 && j < m)) return 0.f;
        if (!FUSED) return dp[(long)t * n + i];
        float s = 0.f;
#pragma unroll
        for (int kk = 0; kk < DTW_FUSED_K; ++kk) {
            const float x = ar[kk] - sB[kk * DTW_MAX_LEN + j];
            s = fmaf(x, x, s);
        }
        return sqrtf(s);
    };
    float own = 0.f, up_prev = 0.f;          // D[i, j - 1] and D[i - 1, j - 1] of the step to come
    int own_l = 0, up_prev_l = 0;
    const int steps = n + m - 1;
    float d = local(0);
    for (int t = 0; t < steps; ++t) {
        const int j = t - i, cur = t & 1;
        if (i < n && j >= 0 && j < m) {
            float up = INFINITY;
            int up_l = 0;
            if (i > 0) {
                const float2 v = sDL[cur ^ 1][i - 1];
                up = v.x, up_l = __float_as_int(v.y);
            }
            float D = d;
            int L = 1, code = 3;
            if (t > 0) {
                const float c0 = (i > 0 && j > 0) ? fmaf(w, d, up_prev) : INFINITY;
                const float c1 = up + d;
                const float c2 = j > 0 ? own + d : INFINITY;
                D = c0, L = up_prev_l, code = 0;
                if (c1 < D) D = c1, L = up_l, code = 1;
                if (c2 < D) D = c2, L = own_l, code = 2;
                L += 1;
            }
            sDL[cur][i] = make_float2(D, __int_as_float(L));
            if (dirp) dirp[(long)t * n + i] = (uint8_t)code;
            up_prev = up, up_prev_l = up_l, own = D, own_l = L;
        }
        d = local(t + 1);          // the next cell's distance needs nothing from this step: it is on its way while the barrier is waited for
        __syncthreads();
    }
    if (i != n - 1) return;
    cost[p] = own;
    length[p] = own_l;
    if (!path) return;
    // the direction bytes were written by this workgroup, in front of the loop's last barrier
    int32_t* slot = path + 2 * (a0 + b0 - p);          // pair p owns n + m - 1 rows behind those of the pairs in front of it
    const int len = min(max(own_l, 1), steps);
    int pi = n - 1, pj = m - 1;
    for (int s = 0; s < steps; ++s) {
        const int pos = len - 1 - s;
        if (pos < 0) break;
        slot[2 * pos] = pi;
        slot[2 * pos + 1] = pj;
        const int code = dirp[(long)(pi + pj) * n + pi];
        if (code != 2) pi = max(pi - 1, 0);
        if (code != 1) pj = max(pj - 1, 0);
    }
}

__global__ __launch_bounds__(256) void mel_cepstra_kernel(const float* __restrict__ mel, long rows, int n_mel, int n_cep, const float* __restrict__ table,
                                                          float* __restrict__ out) {
    __shared__ float sT[CEP_MAX_CEP * (CEP_MAX_MEL + 1)];
    __shared__ float sX[CEP_ROWS * CEP_MAX_MEL];
    const int tid = threadIdx.x, pitch = n_mel | 1;          // odd: lanes over the coefficients read distinct banks
    const long r0 = (long)blockIdx.x * CEP_ROWS;
    const int nr = (int)min((long)CEP_ROWS, rows - r0);
    for (int idx = tid; idx < n_cep * n_mel; idx += 256) sT[(idx / n_mel) * pitch + idx % n_mel] = table[idx];
    for (int idx = tid; idx < nr * n_mel; idx += 256) sX[idx] = mel[r0 * n_mel + idx];
    __syncthreads();
    for (int o = tid; o < nr * n_cep; o += 256) {
        const int r = o / n_cep, c = o % n_cep;
        float s = 0.f;
        for (int mm = 0; mm < n_mel; ++mm) s = fmaf(sX[r * n_mel + mm], sT[c * pitch + mm], s);
        out[r0 * n_cep + o] = s;
    }
}

static inline int64_t dtw_plane(int64_t max_n, int64_t max_m) { return (max_n + max_m - 1) * max_n; }

}  // namespace mstts
using namespace mstts;

extern "C" int mstts_dtw_supported(int64_t n, int64_t m, int64_t k) {
    return n >= 1 && n <= DTW_MAX_LEN && m >= 1 && m <= DTW_MAX_LEN && k >= 1 && k <= DTW_MAX_K;
}

extern "C" int64_t mstts_dtw_ws_bytes(int64_t pairs, int64_t max_n, int64_t max_m, int64_t k, int32_t want_path) {
    if (pairs < 1 || pairs > DTW_MAX_PAIRS || !mstts_dtw_supported(max_n, max_m, k)) return 0;
    const int64_t cells = pairs * dtw_plane(max_n, max_m);
    return (k > DTW_FUSED_K ? cells * (int64_t)sizeof(float) : 0) + (want_path ? (cells + 15) / 16 * 16 : 0);
}

extern "C" int mstts_dtw_batch(const float* a, const float* b, const int64_t* a_off_host, const int64_t* b_off_host, const int64_t* offs,
                               int32_t pairs, int32_t k, float diag_weight, void* ws, int64_t ws_bytes, float* cost, int32_t* length,
                               int32_t* path, mstts_stream_t s) {
    MSTTS_REQUIRE(a && b && a_off_host && b_off_host && offs && cost && length, MSTTS_ERR_SHAPE, "dtw_batch: null pointer");
    MSTTS_REQUIRE(pairs >= 1 && pairs <= DTW_MAX_PAIRS && k >= 1 && k <= DTW_MAX_K, MSTTS_ERR_SHAPE,
                  "dtw_batch: 1 <= pairs <= 65535, 1 <= k <= 128 (pairs %d, k %d)", (int)pairs, (int)k);
    MSTTS_REQUIRE(diag_weight > 0.f && diag_weight <= 3.0e38f, MSTTS_ERR_SHAPE, "dtw_batch: diagonal weight %g", (double)diag_weight);
    MSTTS_REQUIRE(a_off_host[0] == 0 && b_off_host[0] == 0, MSTTS_ERR_SHAPE, "dtw_batch: the offsets start at 0");
    int64_t max_n = 0, max_m = 0;
    for (int32_t p = 0; p < pairs; ++p) {
        const int64_t n = a_off_host[p + 1] - a_off_host[p], m = b_off_host[p + 1] - b_off_host[p];
        MSTTS_REQUIRE(mstts_dtw_supported(n, m, k), MSTTS_ERR_SHAPE, "dtw_batch: pair %d is %lld x %lld frames, 1 <= n, m <= 1024", (int)p,
                      (long long)n, (long long)m);
        max_n = n > max_n ? n : max_n;
        max_m = m > max_m ? m : max_m;
    }
    const int64_t need = mstts_dtw_ws_bytes(pairs, max_n, max_m, k, path != nullptr);
    MSTTS_REQUIRE(need == 0 || (ws && ws_bytes >= need), MSTTS_ERR_SHAPE, "dtw_batch: the workspace holds %lld bytes, the call needs %lld",
                  (long long)ws_bytes, (long long)need);
    MSTTS_REQUIRE(need == 0 || aligned16(ws), MSTTS_ERR_ALIGN, "dtw_batch: ws must be 16-byte aligned");
    hipStream_t st = (hipStream_t)s;
    const long plane = (long)dtw_plane(max_n, max_m);
    const bool fused = k <= DTW_FUSED_K;
    float* dist = fused ? nullptr : (float*)ws;
    uint8_t* dir = path ? (uint8_t*)ws + (fused ? 0 : (size_t)pairs * plane * sizeof(float)) : nullptr;
    const unsigned threads = (unsigned)((max_n + 63) / 64 * 64);
    if (fused) {
        hipLaunchKernelGGL(dtw_kernel<true>, dim3((unsigned)pairs), dim3(threads), 0, st, a, b, offs, (int)pairs, (int)k, diag_weight,
                           (const float*)nullptr, dir, plane, cost, length, path);
    } else {
        const unsigned slices = (unsigned)(max_n + max_m - 1 < 512 ? max_n + max_m - 1 : 512);
        hipLaunchKernelGGL(dtw_dist_kernel, dim3((unsigned)pairs, slices), dim3(256), 0, st, a, b, offs, (int)pairs, (int)k, dist, plane);
        MSTTS_CHECK_LAUNCH("dtw distances");
        hipLaunchKernelGGL(dtw_kernel<false>, dim3((unsigned)pairs), dim3(threads), 0, st, a, b, offs, (int)pairs, (int)k, diag_weight,
                           (const float*)dist, dir, plane, cost, length, path);
    }
    MSTTS_CHECK_LAUNCH("dtw");
    return MSTTS_OK;
}

extern "C" int mstts_mel_cepstra(const float* mel, int64_t rows, int32_t n_mel, int32_t n_cep, const float* table, float* out, mstts_stream_t s) {
    MSTTS_REQUIRE(mel && table && out, MSTTS_ERR_SHAPE, "mel_cepstra: null pointer");
    MSTTS_REQUIRE(rows >= 1 && rows < (1LL << 31) * CEP_ROWS && n_mel >= 2 && n_mel <= CEP_MAX_MEL && n_cep >= 1 && n_cep <= CEP_MAX_CEP && n_cep < n_mel,
                  MSTTS_ERR_SHAPE, "mel_cepstra: rows >= 1, 2 <= n_mel <= 128, 1 <= n_cep <= min(40, n_mel - 1) (rows %lld, n_mel %d, n_cep %d)",
                  (long long)rows, (int)n_mel, (int)n_cep);
    hipLaunchKernelGGL(mel_cepstra_kernel, dim3((unsigned)cdiv(rows, CEP_ROWS)), dim3(256), 0, (hipStream_t)s, mel, (long)rows, (int)n_mel,
                       (int)n_cep, table, out);
    MSTTS_CHECK_LAUNCH("mel cepstra");
    return MSTTS_OK;
}
