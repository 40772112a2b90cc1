// bf16-operand GEMM on the gfx950 matrix cores (v_mfma_f32_32x32x16_bf16, fp32 accumulate) - BASELINE config 3
// ("bf16 with fp32 master"): the SAME contractions mstts_gemm_f32 covers (dense, conv1d 'same' as implicit im2col, data and
// weight gradients, split-K, batches), same descriptor, but both operands are rounded to bf16 (round-to-nearest-even) on their
// way into LDS.  Inputs and outputs stay fp32 in memory - master weights, activations, gradients and the accumulators never
// leave fp32; only the multiplicands are 8-bit-mantissa.  16x the fp32 MFMA rate, so these launches become memory/LDS-bound.
//
// The 128 x 128 x 64 tile is gemm_tile128_kernel (gemm_tile.h); here are its loaders for fp32 operands.  The LDS image is k CONTIGUOUS
// per row whatever the operand's memory layout; the transposition this needs for operands that are contiguous along their M/N index is
// done in registers: a thread loads a 4 (k) x 4 (rows) block as four float4 and writes four 8-byte k-runs.
#include "gemm_tile.h"
#include <type_traits>
#include <cstdlib>

namespace mstts {

typedef __bf16 gb_bf16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ gb_bf16x4 gb_round4(float a, float b, float c, float d) {
    return (gb_bf16x4){(__bf16)a, (__bf16)b, (__bf16)c, (__bf16)d};
}
// staging policy of gemm_bf16_big_kernel (gemm_tile.h): four values -> one round-to-nearest-even bf16 plane
struct RoundPlane {
    static __device__ __forceinline__ void put(__bf16* __restrict__ p, float a, float b, float c, float d) {
        *reinterpret_cast<gb_bf16x4*>(p) = gb_round4(a, b, c, d);
    }
};

// operand contiguous along k in memory (A row-major, or B given as [N,K]): thread (k4 = tid & 15, r = tid >> 4) takes the float4
// k-run k4 of rows r, r + 16, .., r + 112.  Window arithmetic is hoisted like in gemm.hip: prepare() once, then load() for
// k0, k0 + GT_BK, ... (a thread's rows are fixed, its k advances by GT_BK per call).
template <bool VEC>
struct GbLoaderKC {
    float4 reg[8];
    int t_row[8], tap, kc;
    __device__ __forceinline__ void prepare(int row0, int k0, int wT, int wC) {
        if (wT > 0) {
            const int k4 = threadIdx.x & 15, r = threadIdx.x >> 4;
#pragma unroll
            for (int i = 0; i < 8; ++i) t_row[i] = (row0 + r + i * 16) % wT;
            const int k = k0 + k4 * 4;
            tap = k / wC; kc = k - tap * wC;
        }
    }
    __device__ __forceinline__ void load(const float* __restrict__ base, long ld, int row0, int k0, int rows, int kmax,
                                         int wT, int wC, int wpad, int wdil) {
        const int k4 = threadIdx.x & 15, r = threadIdx.x >> 4;
        const int k = k0 + k4 * 4;
        const int sh = wT > 0 ? (tap - wpad) * wdil : 0;     // tap j = k / C of a dilated 'same' conv: source row = row + (j - pad) * dil
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int row = row0 + r + i * 16;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            bool ok = row < rows && k < kmax;
            long off = (long)row * ld + k;
            if (wT > 0) {
                const int t = t_row[i] + sh;
                ok = ok && t >= 0 && t < wT;
                off = ((long)row + sh) * ld + kc;
            }
            if (ok) {
                if (VEC) v = *reinterpret_cast<const float4*>(base + off);
                else {
                    v.x = base[off];
                    if (k + 1 < kmax) v.y = base[off + 1];
                    if (k + 2 < kmax) v.z = base[off + 2];
                    if (k + 3 < kmax) v.w = base[off + 3];
                }
            }
            reg[i] = v;
        }
        if (wT > 0) {
            kc += GT_BK;
            while (kc >= wC) { kc -= wC; ++tap; }
        }
    }
    __device__ __forceinline__ void store(__bf16* __restrict__ s) const {
        const int k4 = threadIdx.x & 15, r = threadIdx.x >> 4;
#pragma unroll
        for (int i = 0; i < 8; ++i)
            *reinterpret_cast<gb_bf16x4*>(s + (r + i * 16) * GT_LD + k4 * 4) = gb_round4(reg[i].x, reg[i].y, reg[i].z, reg[i].w);
    }
};

// operand contiguous along its M/N index (B row-major [K,N], or A given as [K,M]): thread (c4 = tid & 31, kq = tid >> 5) takes, in
// each of the two 32-k halves, the 4 x 4 block of k rows 4 kq .. 4 kq + 3 x columns 4 c4 .. 4 c4 + 3 and writes it transposed
template <bool VEC>
struct GbLoaderMC {
    float4 reg[8];
    int sh, cm, t_k[8];
    __device__ __forceinline__ void prepare(int col0, int k0, int wT, int wC, int wpad, int wdil) {
        if (wT > 0) {
            const int c4 = threadIdx.x & 31, kq = threadIdx.x >> 5;
            const int col = col0 + c4 * 4;
            const int tp = col / wC;
            sh = (tp - wpad) * wdil; cm = col - tp * wC;
#pragma unroll
            for (int i = 0; i < 8; ++i) t_k[i] = (k0 + (i >> 2) * 32 + kq * 4 + (i & 3)) % wT;
        }
    }
    __device__ __forceinline__ void load(const float* __restrict__ base, long ld, int col0, int k0, int cols, int kmax,
                                         int wT, int wC, int wpad, int wdil) {
        const int c4 = threadIdx.x & 31, kq = threadIdx.x >> 5;
        const int col = col0 + c4 * 4;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = k0 + (i >> 2) * 32 + kq * 4 + (i & 3);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            bool ok = k < kmax && col < cols;
            long off = (long)k * ld + col;
            if (wT > 0) {                  // window (A only): element (m, kk) with kk = (b, t) row index, m = (tap, c)
                const int t = t_k[i] + sh;
                ok = ok && t >= 0 && t < wT;
                off = ((long)k + sh) * ld + cm;
                t_k[i] += GT_BK;
                while (t_k[i] >= wT) t_k[i] -= wT;
            }
            if (ok) {
                if (VEC) v = *reinterpret_cast<const float4*>(base + off);
                else {
                    v.x = base[off];
                    if (col + 1 < cols) v.y = base[off + 1];
                    if (col + 2 < cols) v.z = base[off + 2];
                    if (col + 3 < cols) v.w = base[off + 3];
                }
            }
            reg[i] = v;
        }
    }
    __device__ __forceinline__ void store(__bf16* __restrict__ s) const {
        const int c4 = threadIdx.x & 31, kq = threadIdx.x >> 5;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            __bf16* p = s + (c4 * 4) * GT_LD + h * 32 + kq * 4;
            const float4 *q = reg + 4 * h;
            *reinterpret_cast<gb_bf16x4*>(p) = gb_round4(q[0].x, q[1].x, q[2].x, q[3].x);
            *reinterpret_cast<gb_bf16x4*>(p + GT_LD) = gb_round4(q[0].y, q[1].y, q[2].y, q[3].y);
            *reinterpret_cast<gb_bf16x4*>(p + 2 * GT_LD) = gb_round4(q[0].z, q[1].z, q[2].z, q[3].z);
            *reinterpret_cast<gb_bf16x4*>(p + 3 * GT_LD) = gb_round4(q[0].w, q[1].w, q[2].w, q[3].w);
        }
    }
};

// the loader pair of gemm_tile128_kernel (gemm_tile.h) for fp32 operands in any of the four layouts
template <bool TA, bool TB, bool VEC>
struct GbLoaders {
    using Args = GemmTileArgs;
    using LA = typename std::conditional<TA, GbLoaderMC<VEC>, GbLoaderKC<VEC>>::type;
    using LB = typename std::conditional<TB, GbLoaderKC<VEC>, GbLoaderMC<VEC>>::type;
    static constexpr bool BATCHED = true;
    static __device__ __forceinline__ const GemmTileArgs& tile(const Args& g) { return g; }
    static __device__ __forceinline__ const float* a(const Args& g) { return g.A; }
    static __device__ __forceinline__ const float* b(const Args& g) { return g.B; }
    static __device__ __forceinline__ void prepare(const GemmTileArgs& g, LA& la, LB&, int m0, int, int kbeg) {
        if constexpr (TA) la.prepare(m0, kbeg, g.win_T, g.win_C, g.win_pad, g.win_dil);
        else la.prepare(m0, kbeg, g.win_T, g.win_C);
    }
    static __device__ __forceinline__ void load(const GemmTileArgs& g, LA& la, LB& lb, const float* A, const float* B, int m0, int n0, int k0, int kend) {
        la.load(A, g.lda, m0, k0, g.M, kend, g.win_T, g.win_C, g.win_pad, g.win_dil);
        lb.load(B, g.ldb, n0, k0, g.N, kend, 0, 1, 0, 1);
    }
};

// (in a profile: gemm_tile128_kernel<GbLoaders<TA, TB, VEC>>)
template <bool TA, bool TB, bool VEC> constexpr auto gemm_bf16_kernel = &gemm_tile128_kernel<GbLoaders<TA, TB, VEC>>;

struct GemmBf16 {                 // no WIN flag (run-time window), static LDS
    using Args = GemmTileArgs;
    static constexpr int THREADS = 256;
    static constexpr size_t LDS_BYTES = 0;
    template <bool TA, bool TB, bool VEC, bool WIN> static constexpr auto kernel() { return gemm_bf16_kernel<TA, TB, VEC>; }
};


// ---------------------------------------------------------------------------------------------------------------------------------------
// Big-tile form (round 5): 256 x 256 x 32 per 512-thread workgroup, one workgroup per CU.  The 128 x 128 kernel above moves 32 KB of fp32
// operands per 1.05 MFLOP through the CU's vector-memory path; with one bf16 product per element (not six, as in the fp32 split kernel) the
// matrix cores need 512 cycles for what the loads need ~1 000 for, and the kernel sat at 11-16 % of the bf16 peak.  A 256 x 256 tile
// halves the bytes per flop (64 KB per 4.2 MFLOP).  Eight waves as 2 x 4, each 128 x 64 = 4 x 2 MFMA tiles (128 accumulator registers); every
// wave loads, converts, stages and multiplies; two LDS buffers (2 x 40 KB), ONE raw barrier per K-tile:
//     k-step 0 of tile t   |  registers of tile t + 1 -> bf16 -> buffer (t + 1) & 1  |  loads of tile t + 2 issued  |  k-step 1 of tile t  |  barrier
// (buffer (t + 1) & 1 was last read as tile t - 1, i.e. before the previous barrier).  Loaders shared with the split kernels (gemm_tile.h): uniform base + 32-bit
// per-thread offsets fixed at prepare(), unconditional loads (out-of-range lanes read a zero block), branch-free conv-window bookkeeping
// (template flag; needs win_C >= 32 and win_T >= 32 - anything smaller stays on the kernel above).
constexpr int GX_BM = 256, GX_BN = 256, GX_BK = 32, GX_LD = 40, GX_THREADS = 512;     // LDS row stride 80 B: conflict-free b128 fragment reads
constexpr int GX_PLANE = 256 * GX_LD;                                                   // bf16 elements of one operand's tile
constexpr size_t GX_LDS_BYTES = 2 * 2 * GX_PLANE * sizeof(__bf16);
// operand contiguous along k: thread (k4 = tid & 7, r = tid >> 3 in 0..63) takes the float4 k-run k4 of rows r, r + 64, r + 128, r + 192
template <bool VEC, bool WIN> using GxLoaderKC = TileLoaderKC<8, 4, 64, GX_LD, RoundPlane, VEC, WIN>;
// operand contiguous along its M/N index: thread (kq = tid & 7, c4 = tid >> 3 in 0..63) takes the 4 x 4 block of k rows 4 kq .. + 3 x columns
// 4 c4 .. + 3 as four float4 and writes it transposed (four 8-byte k-runs)
template <bool VEC, bool WIN> using GxLoaderMC = TileLoaderMC<8, GX_LD, RoundPlane, VEC, WIN>;

template <bool TA, bool TB, bool VEC, bool WIN>
__global__ __launch_bounds__(GX_THREADS) void gemm_bf16_big_kernel(GemmTileArgs g) {
    extern __shared__ __attribute__((aligned(16))) __bf16 gx_lds[];           // [buffer 2][A | B][256 rows][GX_LD]
    const int tiles_n = (g.N + GX_BN - 1) / GX_BN;
    const int tile = gemm_xcd_tile(blockIdx.x, gridDim.x);
    const int tile_m = tile / tiles_n, tile_n = tile % tiles_n;
    const int batch = blockIdx.z / g.split_k, split = blockIdx.z % g.split_k;
    float* C = g.C + (long)batch * g.stride_c;
    const int m0 = tile_m * GX_BM, n0 = tile_n * GX_BN;
    const int kbeg = split * g.k_per_split;
    const int kend = min(g.K, kbeg + g.k_per_split);
    const int nt = kend > kbeg ? (kend - kbeg + GX_BK - 1) / GX_BK : 0;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wrow = (wave >> 2) * 128, wcol = (wave & 3) * 64;
    const int l31 = lane & 31, kg = lane >> 5;

    using LA = typename std::conditional<TA, GxLoaderMC<VEC, WIN>, GxLoaderKC<VEC, WIN>>::type;
    using LB = typename std::conditional<TB, GxLoaderKC<VEC, false>, GxLoaderMC<VEC, false>>::type;
    LA la; LB lb;
    la.prepare(tid, g.A + (long)batch * g.stride_a, g.lda, m0, kbeg, g.M, g.win_T, g.win_C, g.win_pad, g.win_dil);
    lb.prepare(tid, g.B + (long)batch * g.stride_b, g.ldb, n0, kbeg, g.N, 0, 1, 0, 1);
    float4 ra[4], rb[4];
    auto load = [&](int k) {
        la.load(tid, ra, k, kend, g.lda, g.win_T, g.win_C, g.win_pad, g.win_dil);
        lb.load(tid, rb, k, kend, g.ldb, 0, 1, 0, 1);
    };
    auto store = [&](int buf) {
        la.store(tid, ra, gx_lds + buf * 2 * GX_PLANE);
        lb.store(tid, rb, gx_lds + buf * 2 * GX_PLANE + GX_PLANE);
    };

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int aoff = (wrow + l31) * GX_LD + kg * 8, boff = GX_PLANE + (wcol + l31) * GX_LD + kg * 8;
    auto kstep = [&](const __bf16* buf, int ks) {
        gemm_bf16x8 a[4], b[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const gemm_bf16x8*>(buf + aoff + i * 32 * GX_LD + ks * 16);
#pragma unroll
        for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const gemm_bf16x8*>(buf + boff + j * 32 * GX_LD + ks * 16);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    };
    // (Measured and not kept: two fragment register sets with the barrier between a tile's two k-steps, as in gemm_split.inc - 554 instead of
    //  714 TFLOP/s on 8192^3, 416 instead of 500 on the 25 632-row weight gradient; and two operand register sets, i.e. loads issued two
    //  iterations ahead - no change.  With two waves per SIMD the hardware interleaves one wave's fragment reads / staging with the other's MFMAs.)
    if (nt > 0) {
        load(kbeg);
        store(0);
        load(kbeg + GX_BK);                 // (past the end: the loaders read the zero block)
        gemm_barrier();
        for (int t = 0; t < nt; ++t) {
            const __bf16* buf = gx_lds + (t & 1) * 2 * GX_PLANE;
            kstep(buf, 0);
            store((t + 1) & 1);             // tile t + 1 (loaded one iteration ago) -> the buffer tile t - 1 was read from
            load(kbeg + (t + 2) * GX_BK);
            kstep(buf, 1);
            gemm_barrier();
        }
    }

    gemm_store_tile<4, 2>(g, acc, C, m0 + wrow, n0 + wcol, lane, split == 0, g.split_k > 1);
}

struct GemmBf16Big {
    using Args = GemmTileArgs;
    static constexpr int THREADS = GX_THREADS;
    static constexpr size_t LDS_BYTES = GX_LDS_BYTES;
    template <bool TA, bool TB, bool VEC, bool WIN> static constexpr auto kernel() { return &gemm_bf16_big_kernel<TA, TB, VEC, WIN>; }
};

}  // namespace mstts

using namespace mstts;

// Process-global development switches (A/B runs, tests), set through the entry points below - the library reads no environment variable
// (multi_speaker_tts_amd/lib.py maps its MSTTS_GEMM_* variables onto these setters when it loads the library).
static int g_bf16_big = 1;
extern "C" int mstts_gemm_bf16_big(int32_t on) { g_bf16_big = on != 0; return MSTTS_OK; }
static int g_bf16_big_min = 160;         // (measured: 180 workgroups of the 256 x 256 kernel beat 720 of the small one by 1.3 x, 101 lose to 404 by 1.2 x)
namespace mstts { void gemm_bf16_set_big_min(int n) { if (n > 0) g_bf16_big_min = n; } }       // (mstts_gemm_big_min_workgroups, csrc/gemm.hip)
static int g_bf16_autocut = 1;           // 0: no K-cut of the library's own (A/B)
extern "C" int mstts_gemm_bf16_autocut(int32_t on) { g_bf16_autocut = on != 0; return MSTTS_OK; }

namespace mstts { int gemm_deterministic_now(); }
extern "C" int mstts_gemm_bf16(const mstts_gemm_desc* d, mstts_stream_t stream) {
    GemmTileArgs g;
    bool vec;
    const int rc = gemm_args_from(d, "gemm_bf16", GT_BK, 0, &g, &vec);
    if (rc != MSTTS_OK || g.M == 0 || g.N == 0) return rc;
    const int batch = d->batch > 0 ? (int)d->batch : 1;
    int split = g.split_k;
    hipStream_t st = (hipStream_t)stream;
    const bool ta = d->trans_a != 0, tb = d->trans_b != 0, win = g.win_T > 0;
    // the 256 x 256 tile where the operand is large enough to fill the chip with such tiles (at least ~3/4 of a round of 256 workgroups) and the
    // strides fit its 32-bit tile-relative offsets; MSTTS_GEMM_BF16_BIG=0 / mstts_gemm_bf16_big(0) keeps the 128 x 128 kernel (A/B, tests)
    const long big_wgs = (long)cdiv(d->M, GX_BM) * cdiv(d->N, GX_BN) * batch * split;
    const bool big = g_bf16_big && d->M >= 192 && d->N >= 192 && big_wgs >= g_bf16_big_min && d->lda < (1 << 22) && d->ldb < (1 << 22) &&
                     (d->win_T <= 0 || (d->win_T >= GX_BK && d->win_C >= GX_BK)) && gemm_ready<GemmBf16Big>();
    if (big) {
        g.k_per_split = gemm_k_per_split(g.K, split, GX_BK);
        dim3 gridb(cdiv(d->M, GX_BM) * cdiv(d->N, GX_BN), 1, batch * split);
        gemm_launch<GemmBf16Big>(g, ta, tb, vec, win, gridb, st);
        MSTTS_CHECK_LAUNCH("gemm_bf16 (256 x 256 tile)");
        return MSTTS_OK;
    }
    // The 128 x 128 kernel runs two workgroups per CU: 512 slots.  A contraction whose tile list is far from a multiple of that - the encoder's
    // 4 096-row convolutions (128 tiles), the 80 / 84-column products (14 - 201 tiles) - and whose caller asked for NO cut (split_k <= 1) is cut
    // along K so that it fills one round: pieces of at least 128 contraction steps, cost model rounds x (K per piece + 300) x (1 + 2 % per piece
    // for its atomics), fitted to a sweep of every such call of a train step (tools/gemm_split_sweep.py --config3: 0.31 ms per step against
    // cuts chosen for the fp32 kernel's tiles).  Only without a fused activation, for one batch, and not under mstts_gemm_deterministic; without
    // `accumulate` the output's N columns (not its row pitch: C may be a column band of a wider matrix) are cleared here first.  A caller's own
    // split_k > 1 is honoured exactly - as mstts_gemm_f32 does - so a caller that reasons about the number of pieces (0 + p + q) gets that number.
    if (g_bf16_autocut && split == 1 && d->act == MSTTS_ACT_NONE && batch == 1 && !gemm_deterministic_now()) {
        const long tiles = (long)cdiv(d->M, GT_BM) * cdiv(d->N, GT_BN);
        int best = 1;
        double best_cost = 0.0;
        for (int sk = 1; sk <= 64; ++sk) {
            if (sk > 1 && g.K / sk < 128) break;
            const double cost = (double)cdiv(tiles * sk, 512) * ((double)g.K / sk + 300.0) * (1.0 + 0.02 * sk);
            if (sk == 1 || cost < best_cost * 0.97) { best = sk; best_cost = cost; }      // (a cut has to win by 3 %)
        }
        if (best > 1) {
            if (!d->accumulate) {
                if (hipMemset2DAsync(d->C, (size_t)d->ldc * 4, 0, (size_t)d->N * 4, (size_t)d->M, st) != hipSuccess)
                    MSTTS_REQUIRE(false, MSTTS_ERR_LAUNCH, "gemm_bf16: clearing the output of a K-cut contraction failed");
            }
            split = best;
            g.split_k = split;
            g.k_per_split = gemm_k_per_split(g.K, split, GT_BK);
        }
    }
    dim3 grid(cdiv(d->M, GT_BM) * cdiv(d->N, GT_BN), 1, batch * split);
    gemm_launch<GemmBf16>(g, ta, tb, vec, win, grid, st);
    MSTTS_CHECK_LAUNCH("gemm_bf16");
    return MSTTS_OK;
}
