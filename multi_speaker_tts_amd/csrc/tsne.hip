// Exact t-SNE on gfx950 (van der Maaten & Hinton 2008, with the schedule of scikit-learn's TSNE(method='exact')); tsne.tsne_host is the
// fp64 statement, stage by stage.  fp32 throughout, plain expf / logf / division, every reduction in one fixed order and no
// floating-point atomic: the same inputs give the same bits.  No kernel waits on another workgroup; what a stage needs from every row
// goes through a kernel boundary.
//
// Stage A, affinities (two launches):
//   tsne_cond_kernel    a workgroup per row i: d_j = |x_i - x_j|^2 into LDS (a thread per j, x_i read from LDS), then the search for the
//                       precision beta_i with entropy H = ln sum_j p_j + beta sum_j d_j p_j / sum_j p_j = ln(perplexity), p_j =
//                       exp(-beta d_j), j != i: beta = 1, doubled or halved until it is bracketed, then bisected, at most 100 evaluations,
//                       done when |H - ln(perplexity)| <= 1e-5; a zero sum is replaced by 1e-8 (it cannot arise here: d is taken relative to
//                       the row's smallest distance).  The row C[i, :] = p / sum p of the LAST EVALUATED beta, beta_i and the row's sum go
//                       out.  Every thread sees the same block sums, so the search's control flow is uniform.
//   tsne_joint_kernel   64 x 64 tiles: P[i, j] = max((C[i, j] + C[j, i]) / (2 sum of the row sums), 2.220446e-16), the mirrored tile
//                       through LDS.  a + b = b + a, so P is symmetric bit for bit; the diagonal is at the floor.
// Stage B, one descent iteration (two launches):
//   tsne_pair_kernel    a wave per row i, lanes over j != i: num = 1 / (1 + |y_i - y_j|^2) and the row's sums z = sum num,
//                       a = sum e p num (y_i - y_j), b = sum num^2 (y_i - y_j) - on reporting iterations also sum e p ln(e p),
//                       sum e p ln num and sum e p - to R[i, 0..7].
//   tsne_update_kernel  one workgroup: Z = sum_i z_i, g_i = 4 (a_i - b_i / Z), the gain rule, the momentum step, Y += update; on reporting
//                       iterations KL = sum ep ln ep - sum ep ln num + ln Z sum ep and |g|_2 into the history buffer.
#include "common.h"

namespace mstts {

constexpr float TSNE_FLOOR = 2.220446e-16f;            // scikit-learn's MACHINE_EPSILON
constexpr int TSNE_MAX_N = 4096, TSNE_MAX_D = 1024, TSNE_SEARCH_STEPS = 100, TSNE_CHECK_EVERY = 50, TSNE_ROW_SUMS = 8;

__global__ __launch_bounds__(256) void tsne_cond_kernel(const float* __restrict__ X, long pitch, int N, int D, float want_h,
                                                        float* __restrict__ Cm, float* __restrict__ beta_out, float* __restrict__ row_sum) {
    extern __shared__ __attribute__((aligned(16))) float tsne_lds[];
    float* xi = tsne_lds;                         // [D] rounded up to 4
    float* d = tsne_lds + ((D + 3) & ~3);         // [N]
    float* scratch = d + ((N + 3) & ~3);          // [16]
    const int i = blockIdx.x, tid = threadIdx.x;
    for (int k = tid; k < D; k += 256) xi[k] = X[i * pitch + k];
    __syncthreads();
    for (int j = tid; j < N; j += 256) {
        const float* xj = X + j * pitch;
        float s = 0.f, lost = 0.f;                        // compensated: an error e in d_j is a relative error beta e in p_j, beta ~ 10 ... 100
        for (int k = 0; k < D; ++k) {
            const float t = xi[k] - xj[k];
            const float term = t * t - lost, next = s + term;
            lost = (next - s) - term;
            s = next;
        }
        d[j] = s;
    }
    __syncthreads();
    // The row is the same with d - min_j d in place of d (numerator and sum both carry the factor exp(beta min d)), and so is H; shifted,
    // the nearest neighbour's term is exp(0) at any beta, where float32's exp(-beta d) would leave a row of zeros from beta d > 87 on.
    float dmin = INFINITY;
    for (int j = tid; j < N; j += 256)
        if (j != i) dmin = fminf(dmin, d[j]);
    dmin = -block_max(-dmin, scratch);
    for (int j = tid; j < N; j += 256) d[j] -= dmin;       // (each thread shifts the entries it alone reads below)
    float beta = 1.f, lo = -INFINITY, hi = INFINITY, used = 1.f, sum_p = 1.f;
    for (int step = 0; step < TSNE_SEARCH_STEPS; ++step) {
        float sp = 0.f, sdp = 0.f;
        for (int j = tid; j < N; j += 256) {
            if (j == i) continue;
            const float e = expf(-d[j] * beta);
            sp += e;
            sdp += d[j] * e;
        }
        sum_p = block_sum(sp, scratch);
        const float sum_dp = block_sum(sdp, scratch);
        if (sum_p == 0.f) sum_p = 1e-8f;
        used = beta;
        const float diff = logf(sum_p) + beta * (sum_dp / sum_p) - want_h;
        if (fabsf(diff) <= 1e-5f) break;
        if (diff > 0.f) {
            lo = beta;
            beta = hi == INFINITY ? beta * 2.f : (beta + hi) * 0.5f;
        } else {
            hi = beta;
            beta = lo == -INFINITY ? beta * 0.5f : (beta + lo) * 0.5f;
        }
    }
    float rs = 0.f;
    for (int j = tid; j < N; j += 256) {
        const float c = j == i ? 0.f : expf(-d[j] * used) / sum_p;
        Cm[(long)i * N + j] = c;
        rs += c;
    }
    rs = block_sum(rs, scratch);
    if (tid == 0) {
        beta_out[i] = used;
        row_sum[i] = rs;
    }
}

__global__ __launch_bounds__(256) void tsne_joint_kernel(const float* __restrict__ Cm, const float* __restrict__ row_sum, int N,
                                                         float* __restrict__ P) {
    __shared__ float mirror[64][65];
    __shared__ float scratch[16];
    const int tid = threadIdx.x, c = tid & 63, r0 = tid >> 6;
    const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
    float t = 0.f;
    for (int k = tid; k < N; k += 256) t += row_sum[k];
    const float total = fmaxf(2.f * block_sum(t, scratch), TSNE_FLOOR);
    for (int r = r0; r < 64; r += 4)                       // C[j0 + r, i0 + c]: the mirrored tile, rows read coalesced
        mirror[r][c] = (j0 + r < N && i0 + c < N) ? Cm[(long)(j0 + r) * N + i0 + c] : 0.f;
    __syncthreads();
    for (int r = r0; r < 64; r += 4) {
        const int i = i0 + r, j = j0 + c;
        if (i < N && j < N) P[(long)i * N + j] = fmaxf((Cm[(long)i * N + j] + mirror[c][r]) / total, TSNE_FLOOR);
    }
}

__global__ __launch_bounds__(256) void tsne_pair_kernel(const float* __restrict__ P, const float2* __restrict__ Y, int N, float exaggeration,
                                                        int report, float* __restrict__ R) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;                                    // whole waves leave; the kernel has no workgroup barrier
    const float2 yi = Y[i];
    const float* p = P + (long)i * N;
    float z = 0.f, ax = 0.f, ay = 0.f, bx = 0.f, by = 0.f, k1 = 0.f, k2 = 0.f, k3 = 0.f;
    for (int j = lane; j < N; j += 64) {
        if (j == i) continue;
        const float2 yj = Y[j];
        const float dx = yi.x - yj.x, dy = yi.y - yj.y;
        const float num = 1.f / (1.f + (dx * dx + dy * dy));
        const float pe = exaggeration * p[j];
        const float w = pe * num, n2 = num * num;
        z += num;
        ax += w * dx;
        ay += w * dy;
        bx += n2 * dx;
        by += n2 * dy;
        if (report) {
            k1 += pe * logf(fmaxf(pe, TSNE_FLOOR));
            k2 += pe * logf(num);
            k3 += pe;
        }
    }
    z = wave_sum(z);
    ax = wave_sum(ax);
    ay = wave_sum(ay);
    bx = wave_sum(bx);
    by = wave_sum(by);
    if (report) {
        k1 = wave_sum(k1);
        k2 = wave_sum(k2);
        k3 = wave_sum(k3);
    }
    if (lane == 0) {
        float4* out = reinterpret_cast<float4*>(R + (long)i * TSNE_ROW_SUMS);
        out[0] = make_float4(z, ax, ay, bx);
        out[1] = make_float4(by, k1, k2, k3);
    }
}

__global__ __launch_bounds__(512) void tsne_update_kernel(const float* __restrict__ R, int N, float2* __restrict__ Y, float2* __restrict__ U,
                                                          float2* __restrict__ G, float momentum, float lr, int reset, int slot,
                                                          float* __restrict__ hist, float2* __restrict__ grad) {
    __shared__ float scratch[16];
    const int tid = threadIdx.x;
    float t = 0.f;
    for (int i = tid; i < N; i += 512) t += R[(long)i * TSNE_ROW_SUMS];
    const float Z = block_sum(t, scratch);
    float gn = 0.f, k1 = 0.f, k2 = 0.f, k3 = 0.f;
    for (int i = tid; i < N; i += 512) {
        const float4 a = reinterpret_cast<const float4*>(R + (long)i * TSNE_ROW_SUMS)[0];
        const float4 b = reinterpret_cast<const float4*>(R + (long)i * TSNE_ROW_SUMS)[1];
        const float gx = 4.f * (a.y - a.w / Z), gy = 4.f * (a.z - b.x / Z);
        float2 u = reset ? make_float2(0.f, 0.f) : U[i], g = reset ? make_float2(1.f, 1.f) : G[i], y = Y[i];
        g.x = fmaxf(u.x * gx < 0.f ? g.x + 0.2f : g.x * 0.8f, 0.01f);
        g.y = fmaxf(u.y * gy < 0.f ? g.y + 0.2f : g.y * 0.8f, 0.01f);
        u.x = momentum * u.x - lr * (g.x * gx);
        u.y = momentum * u.y - lr * (g.y * gy);
        y.x += u.x;
        y.y += u.y;
        G[i] = g;
        U[i] = u;
        Y[i] = y;
        if (grad) grad[i] = make_float2(gx, gy);
        gn += gx * gx + gy * gy;
        k1 += b.y;
        k2 += b.z;
        k3 += b.w;
    }
    if (slot >= 0) {                                       // (uniform: a kernel argument)
        gn = block_sum(gn, scratch);
        k1 = block_sum(k1, scratch);
        k2 = block_sum(k2, scratch);
        k3 = block_sum(k3, scratch);
        if (tid == 0) {
            hist[2 * slot] = k1 - k2 + logf(Z) * k3;
            hist[2 * slot + 1] = sqrtf(gn);
        }
    }
}

static bool tsne_reports(int64_t it, int64_t last) { return (it + 1) % TSNE_CHECK_EVERY == 0 || it == last; }

}  // namespace mstts
using namespace mstts;

extern "C" int mstts_tsne_supported(int64_t n, int64_t dim, double perplexity) {
    return n >= 4 && n <= TSNE_MAX_N && dim >= 1 && dim <= TSNE_MAX_D && perplexity >= 1.0 && perplexity < (double)n;
}

extern "C" int64_t mstts_tsne_affinities_ws_floats(int64_t n) { return n < 0 ? 0 : n * n + n; }

extern "C" int64_t mstts_tsne_iterate_ws_floats(int64_t n) { return n < 0 ? 0 : n * TSNE_ROW_SUMS; }

extern "C" int32_t mstts_tsne_history_slots(int32_t first_iter, int32_t n_iters) {
    if (first_iter < 0 || n_iters < 1 || (int64_t)first_iter + n_iters > INT32_MAX) return 0;
    int32_t slots = 0;
    const int64_t last = (int64_t)first_iter + n_iters - 1;
    for (int64_t it = first_iter; it <= last; ++it) slots += tsne_reports(it, last);
    return slots;
}

extern "C" int mstts_tsne_affinities(const float* X, int64_t pitch, int32_t n, int32_t dim, float perplexity, float* ws, float* P, float* beta,
                                     mstts_stream_t s) {
    MSTTS_REQUIRE(X && ws && P && beta, MSTTS_ERR_SHAPE, "tsne_affinities: null pointer");
    MSTTS_REQUIRE(mstts_tsne_supported(n, dim, perplexity), MSTTS_ERR_SHAPE,
                  "tsne_affinities: 4 <= n <= 4096, 1 <= dim <= 1024, 1 <= perplexity < n (n %d, dim %d, perplexity %g)", (int)n, (int)dim,
                  (double)perplexity);
    MSTTS_REQUIRE(pitch >= dim && pitch < (1LL << 31), MSTTS_ERR_SHAPE, "tsne_affinities: row pitch %lld below dim %d", (long long)pitch, (int)dim);
    hipStream_t st = (hipStream_t)s;
    float* Cm = ws;
    float* row_sum = ws + (size_t)n * n;
    const size_t lds = sizeof(float) * (size_t)(((dim + 3) & ~3) + ((n + 3) & ~3) + 16);
    hipLaunchKernelGGL(tsne_cond_kernel, dim3((unsigned)n), dim3(256), lds, st, X, (long)pitch, (int)n, (int)dim, logf(perplexity), Cm, beta,
                       row_sum);
    MSTTS_CHECK_LAUNCH("tsne conditional rows");
    const unsigned tiles = (unsigned)cdiv(n, 64);
    hipLaunchKernelGGL(tsne_joint_kernel, dim3(tiles, tiles), dim3(256), 0, st, (const float*)Cm, (const float*)row_sum, (int)n, P);
    MSTTS_CHECK_LAUNCH("tsne joint probabilities");
    return MSTTS_OK;
}

extern "C" int mstts_tsne_iterate(const float* P, int32_t n, float* Y, float* update, float* gains, int32_t first_iter, int32_t n_iters,
                                  int32_t exaggeration_iters, float early_exaggeration, float learning_rate, float* ws, float* history,
                                  int32_t history_slots, float* grad, mstts_stream_t s) {
    MSTTS_REQUIRE(P && Y && update && gains && ws && history, MSTTS_ERR_SHAPE, "tsne_iterate: null pointer");
    MSTTS_REQUIRE(n >= 4 && n <= TSNE_MAX_N, MSTTS_ERR_SHAPE, "tsne_iterate: 4 <= n <= 4096 (n %d)", (int)n);
    MSTTS_REQUIRE(aligned16(ws) && ((uintptr_t)Y & 7u) == 0 && ((uintptr_t)update & 7u) == 0 && ((uintptr_t)gains & 7u) == 0 &&
                      ((uintptr_t)grad & 7u) == 0,
                  MSTTS_ERR_ALIGN,
                  "tsne_iterate: ws must be 16-byte, the state and grad 8-byte aligned");
    const int32_t slots = mstts_tsne_history_slots(first_iter, n_iters);
    MSTTS_REQUIRE(slots >= 1, MSTTS_ERR_SHAPE, "tsne_iterate: first_iter %d >= 0 and n_iters %d >= 1", (int)first_iter, (int)n_iters);
    MSTTS_REQUIRE(history_slots >= slots, MSTTS_ERR_SHAPE, "tsne_iterate: the history buffer holds %d entries, the run reports %d",
                  (int)history_slots, (int)slots);
    MSTTS_REQUIRE(exaggeration_iters >= 0 && early_exaggeration > 0.f && early_exaggeration <= 3.0e38f && learning_rate > 0.f &&
                      learning_rate <= 3.0e38f,
                  MSTTS_ERR_SHAPE, "tsne_iterate: exaggeration_iters %d, early_exaggeration %g, learning_rate %g", (int)exaggeration_iters,
                  (double)early_exaggeration, (double)learning_rate);
    hipStream_t st = (hipStream_t)s;
    const int64_t last = (int64_t)first_iter + n_iters - 1;
    int slot = 0;
    for (int64_t it = first_iter; it <= last; ++it) {
        const bool early = it < exaggeration_iters, report = tsne_reports(it, last);
        hipLaunchKernelGGL(tsne_pair_kernel, dim3((unsigned)cdiv(n, 4)), dim3(256), 0, st, P, (const float2*)Y, (int)n,
                           early ? early_exaggeration : 1.f, (int)report, ws);
        MSTTS_CHECK_LAUNCH("tsne pair sums");
        hipLaunchKernelGGL(tsne_update_kernel, dim3(1), dim3(512), 0, st, (const float*)ws, (int)n, (float2*)Y, (float2*)update, (float2*)gains,
                           early ? 0.5f : 0.8f, learning_rate, (int)(it == exaggeration_iters), report ? slot : -1, history, (float2*)grad);
        MSTTS_CHECK_LAUNCH("tsne update");
        slot += report;
    }
    return MSTTS_OK;
}
