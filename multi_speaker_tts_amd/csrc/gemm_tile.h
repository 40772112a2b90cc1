// What the GEMM kernels of gemm.hip (+ gemm_split.inc) and gemm_bf16.hip share: the kernel-argument block, the tile loaders of the
// LDS-staged bf16 kernels, the epilogue, the XCD-aware tile order, and on the host the descriptor check and the launch path.
// Each kernel keeps its own K loop and fragment schedule; a kernel family says how a float4 is staged (its `Stage` policy) and with
// which geometry, everything about addressing and the conv window lives here once.  The two 128 x 128 x 64 bf16 forms (gemm_bf16.hip:
// fp32 operands rounded on the way into LDS; gemm_bf16_res.hip: operands that are bf16 in memory) differ in their loaders only and are one
// kernel template, gemm_tile128_kernel.
#pragma once
#include "common.h"
#include <utility>

namespace mstts {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// Kernel arguments of every GEMM kernel (gemm_kernel and the split kernels append their tile schedule: GemmArgs, gemm.hip)
struct GemmTileArgs {
    const float* A; const float* B; float* C; const float* bias;
    int M, N, K;
    long lda, ldb, ldc;
    int win_T, win_C, win_pad, win_dil;
    int act, accumulate, split_k;
    long stride_a, stride_b, stride_c;
    float alpha;
    int k_per_split;
};

__device__ __forceinline__ float apply_act(float v, int act) {
    if (act == MSTTS_ACT_RELU) return fmaxf(v, 0.f);
    if (act == MSTTS_ACT_TANH) return tanhf_(v);
    if (act == MSTTS_ACT_SIGMOID) return sigmoidf_(v);
    return v;
}

// ---- tile loaders -------------------------------------------------------------------------
// "KC": operand contiguous along k in memory (A row-major, or B given as [N,K]); rows = the M (or N) index.
// "MC": operand contiguous along its M/N index (B row-major [K,N], or A given as [K,M]).
// Out-of-range elements are read from this zero block instead of being skipped: the loads stay unconditional (no exec-mask
// branches in the K loop, the scheduler can hide them behind the MFMAs) and the padding is zero without a select on the data.
static __device__ __attribute__((aligned(16))) const float gemm_zero16[4] = {0.f, 0.f, 0.f, 0.f};
// ... and they go through an explicit GLOBAL-address-space pointer: the select between the operand and the zero block otherwise degrades to
// a flat pointer, flat loads count in lgkmcnt as well as vmcnt, and every s_waitcnt lgkmcnt(0) in front of an MFMA group (placed for the
// LDS fragment reads) would then also wait for the K-tile prefetch issued just before - the whole global latency exposed once per K-tile.
typedef float gemm_f32x4 __attribute__((ext_vector_type(4)));
typedef const gemm_f32x4 __attribute__((address_space(1)))* gemm_gptr4;
__device__ __forceinline__ float4 gemm_ld4(const float* p) {
    const gemm_f32x4 v = *(gemm_gptr4)p;
    return make_float4(v[0], v[1], v[2], v[3]);
}

// The workgroup barrier of the kernels that keep loads in flight across K-tiles: LDS traffic of the wave drained, then s_barrier.  NOT
// __syncthreads(): its fence also drains vmcnt, and such a wave always has the loads of the next K-tiles in flight - every barrier would wait
// out a full global-memory latency (measured on gemm_split_kernel: 2.3 us per K-tile instead of 0.7).
__device__ __forceinline__ void gemm_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// The loaders of the kernels that stage bf16 in LDS with k contiguous per row (gemm_split_kernel, gemm_split_big_kernel,
// gemm_bf16_big_kernel).  Geometry: KQ float4 k-quads per tile row (BKT = 4 KQ), LD = LDS row stride in bf16 elements.  Stage::put(p, a, b, c, d)
// says what becomes of four fp32 values bound for LDS address p .. p + 3 (three split planes, or one rounded plane).
// Addressing: every load is  uniform base (SGPRs, advanced once per K-tile)  +  a 32-bit per-thread offset fixed at prepare()  - no 64-bit
// address arithmetic and no bounds arithmetic beyond one compare in the K loop (it cost 9 % of the matrix-core time).
// WIN (conv window mode) is a template parameter and the window bookkeeping is branch-free (one conditional subtract per K-tile: needs
// win_C >= BKT and win_T >= BKT, the entry points send anything smaller to gemm_kernel / gemm_bf16_kernel): a loop that stages must be ONE
// basic block - with branches inside the loaders the register allocator put copies behind the loads of the loop-carried register sets, and a
// copy waits for its load.
// The thread mapping is mask and shift of the caller's signed `tid`, written exactly so: as tid % KQ, tid / KQ the same template compiles to
// different register allocation in the 256-VGPR kernels (profiles/gemm_codegen_after.txt is the record to compare against).
constexpr int gemm_log2(int v) { return v <= 1 ? 0 : 1 + gemm_log2(v >> 1); }

// window: element (row, k) is tap j = k / C of a dilated 'same' conv: source row = row + (j - pad) * dil, valid iff it stays inside the
// row's length-T sequence.  A thread's rows never change (t_row = row % T once) and k advances by BKT per load (tap / kc kept
// incrementally): prepare() once, then load() for k0, k0 + BKT, ...
// Thread (k4 = tid & (KQ - 1), r = tid >> log2 KQ) takes the float4 k-run k4 of the NV rows r, r + RSTEP, ...
template <int KQ, int NV, int RSTEP, int LD, class Stage, bool VEC, bool WIN>
struct TileLoaderKC {
    static constexpr int BKT = 4 * KQ, KSH = gemm_log2(KQ);
    const float* ubase;                               // non-window: base + row0 ld + k0 ; window: base + (row0 - pad dil) ld (for the
                                                      // first tile that is in front of the operand: only ever added to offsets of valid taps)
    unsigned voff[NV], rmask;                         // (r + RSTEP i) ld (+ 4 k4 without window); bit i: row inside the operand
    int t_row[NV], tap, kc, ld_;
    __device__ __forceinline__ void prepare(int tid, const float* __restrict__ base, long ld, int row0, int k0, int rows, int wT, int wC, int wpad, int wdil) {
        const int k4 = tid & (KQ - 1), r = tid >> KSH;
        rmask = 0; ld_ = (int)ld;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int row = row0 + r + i * RSTEP;
            if (row < rows) rmask |= 1u << i;
            voff[i] = (unsigned)((r + i * RSTEP) * (int)ld) + (WIN ? 0u : (unsigned)(k4 * 4));
            if (WIN) t_row[i] = row % wT;
        }
        if (WIN) {
            const int k = k0 + k4 * 4;
            tap = k / wC; kc = k - tap * wC;
            ubase = base + ((long)row0 - (long)wpad * wdil) * ld;
        } else {
            ubase = base + (long)row0 * ld + k0;
        }
    }
    __device__ __forceinline__ void load(int tid, float4 (&reg)[4], int k0, int kmax, long, int wT, int wC, int wpad, int wdil) {
        const int k4 = tid & (KQ - 1);
        const int k = k0 + k4 * 4;
        const bool kok = k < kmax;
        const int sh = WIN ? (tap - wpad) * wdil : 0;
        const unsigned wadd = WIN ? (unsigned)(tap * wdil * ld_ + kc) : 0u;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            bool ok = kok && ((rmask >> i) & 1u);
            if (WIN) {
                const int t = t_row[i] + sh;
                ok = ok && t >= 0 && t < wT;
            }
            if (VEC) {
                v = gemm_ld4(ok ? ubase + (voff[i] + wadd) : gemm_zero16);
            } else if (ok) {
                const float* p = ubase + (voff[i] + wadd);
                v.x = p[0];
                if (k + 1 < kmax) v.y = p[1];
                if (k + 2 < kmax) v.z = p[2];
                if (k + 3 < kmax) v.w = p[3];
            }
            reg[i] = v;
        }
        if (WIN) {                                     // next call is for k0 + BKT
            kc += BKT;
            const bool wrap = kc >= wC;
            kc -= wrap ? wC : 0; tap += wrap ? 1 : 0;
        } else {
            ubase += BKT;
        }
    }
    __device__ __forceinline__ void store(int tid, const float4 (&reg)[4], __bf16* __restrict__ s) const {
        const int k4 = tid & (KQ - 1), r = tid >> KSH;
#pragma unroll
        for (int i = 0; i < NV; ++i) Stage::put(s + (r + i * RSTEP) * LD + k4 * 4, reg[i].x, reg[i].y, reg[i].z, reg[i].w);
    }
};

// window (A only): element (m, kk) with kk = (b, t) row index, m = (tap, c): valid iff 0 <= (kk % T) + m / C - pad < T; address =
// base[(kk + (tap - pad) dil) * ld + c].  A thread's column (tap, c) is fixed, its k-rows advance by BKT per load.
// Thread (kq = tid & (KQ - 1), c4 = tid >> log2 KQ) takes the 4 x 4 block of k rows 4 kq .. 4 kq + 3 x columns 4 c4 .. 4 c4 + 3 as four
// float4 and writes it transposed (four 8-byte k-runs per plane).
// kq in the LOW lane bits: with KQ = 8 a wave reads 8 float4 = 128 contiguous bytes from each of 32 k-rows, and its transposed 8-byte LDS
// writes walk along k inside a row (16 words) over 8 rows - at an 80-byte row stride 4 lanes per bank pair instead of the 32 that
// c4-in-the-low-bits gives (rows 4 apart are 80 words = 16 banks apart: every lane of a wave landed on two bank groups, a 16-way conflict on
// each of the 24 stores per K-tile of gemm_split_kernel).
template <int KQ, int LD, class Stage, bool VEC, bool WIN>
struct TileLoaderMC {
    static constexpr int BKT = 4 * KQ, KSH = gemm_log2(KQ);
    const float* ubase;                               // base + k0 ld + col0 (window: base + (k0 - pad dil) ld), advanced by BKT ld per load
    unsigned voff[4];
    int sh, t_k[4], cols_left;                        // cols_left: columns of the operand from this thread's first one (<= 0: none)
    __device__ __forceinline__ void prepare(int tid, const float* __restrict__ base, long ld, int col0, int k0, int cols, int wT, int wC, int wpad, int wdil) {
        const int kq = tid & (KQ - 1), c4 = tid >> KSH;
        const int col = col0 + c4 * 4;
        cols_left = cols - col;
        if (WIN) {
            const int tp = col / wC, cm = col - tp * wC;
            sh = (tp - wpad) * wdil;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                t_k[i] = (k0 + kq * 4 + i) % wT;
                voff[i] = (unsigned)((kq * 4 + i + tp * wdil) * (int)ld + cm);
            }
            ubase = base + ((long)k0 - (long)wpad * wdil) * ld;
        } else {
            sh = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) voff[i] = (unsigned)((kq * 4 + i) * (int)ld + c4 * 4);
            ubase = base + (long)k0 * ld + col0;
        }
    }
    __device__ __forceinline__ void load(int tid, float4 (&reg)[4], int k0, int kmax, long ld, int wT, int, int, int) {
        const int kq = tid & (KQ - 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = k0 + kq * 4 + i;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            bool ok = k < kmax && cols_left > 0;
            if (WIN) {
                const int t = t_k[i] + sh;
                ok = ok && t >= 0 && t < wT;
                t_k[i] += BKT;                         // next call is for k0 + BKT
                t_k[i] -= (t_k[i] >= wT) ? wT : 0;     // one wrap at most (win_T >= BKT)
            }
            if (VEC) {
                v = gemm_ld4(ok ? ubase + voff[i] : gemm_zero16);
            } else if (ok) {
                const float* p = ubase + voff[i];
                v.x = p[0];
                if (cols_left > 1) v.y = p[1];
                if (cols_left > 2) v.z = p[2];
                if (cols_left > 3) v.w = p[3];
            }
            reg[i] = v;
        }
        ubase += BKT * ld;
    }
    __device__ __forceinline__ void store(int tid, const float4 (&reg)[4], __bf16* __restrict__ s) const {
        const int kq = tid & (KQ - 1), c4 = tid >> KSH;
        __bf16* p = s + (c4 * 4) * LD + kq * 4;
        Stage::put(p, reg[0].x, reg[1].x, reg[2].x, reg[3].x);
        Stage::put(p + LD, reg[0].y, reg[1].y, reg[2].y, reg[3].y);
        Stage::put(p + 2 * LD, reg[0].z, reg[1].z, reg[2].z, reg[3].z);
        Stage::put(p + 3 * LD, reg[0].w, reg[1].w, reg[2].w, reg[3].w);
    }
};

// XCD-aware tile order: block b runs on XCD b % 8 and every XCD has its own L2, so give each XCD a contiguous range of the (tile_m-major)
// list of nb tiles - a band of A rows it re-reads from its own L2 - instead of every eighth tile.
__device__ __forceinline__ int gemm_xcd_tile(int tile, int nb) {
    const int q = nb >> 3, r = nb & 7, xcd = tile & 7, idx = tile >> 3;
    if (nb >= 64) tile = xcd * q + (xcd < r ? xcd : r) + idx;
    return tile;
}

// epilogue of one wave's WM x WN grid of 32 x 32 MFMA tiles: C/D layout col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
template <int WM, int WN>
__device__ __forceinline__ void gemm_store_tile(const GemmTileArgs& g, const f32x16 (&acc)[WM][WN], float* __restrict__ C, int row0, int col0,
                                                int lane, bool with_bias, bool atomic) {
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            const int col = col0 + j * 32 + (lane & 31);
            if (col >= g.N) continue;
            const float bv = (g.bias != nullptr && with_bias) ? g.bias[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = row0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (row >= g.M) continue;
                float v = g.alpha * acc[i][j][r] + bv;
                float* dst = C + (long)row * g.ldc + col;
                if (atomic) {
                    atomicAdd(dst, v);
                } else {
                    v = apply_act(v, g.act);
                    if (g.accumulate) v += *dst;
                    *dst = v;
                }
            }
        }
}

// ---- the 128 x 128 x 64 bf16 tile (gemm_bf16.hip, gemm_bf16_res.hip) ------------------------
// 256 threads = 4 wave64 as 2 x 2, each 64 x 64 = 2 x 2 MFMA tiles.  LDS image of an operand: [128 rows][64 k] bf16, k contiguous per row
// at a row stride of 144 B = 36 words (36 mod 32 = 4): 16-byte aligned rows, an MFMA fragment (lane l: row l & 31, k = 8 (l >> 5) .. + 7)
// is one conflict-free ds_read_b128.
typedef __bf16 gemm_bf16x8 __attribute__((ext_vector_type(8)));
constexpr int GT_BM = 128, GT_BN = 128, GT_BK = 64, GT_LD = 72;

// The kernel, for a loader pair L (GbLoaders: fp32 operands rounded on the way into LDS, gemm_bf16.hip; GrLoaders: operands that are bf16
// in memory, gemm_bf16_res.hip).  L names the kernel's argument (L::Args; L::tile(args) = its GemmTileArgs, L::a / L::b(args) = the operands),
// whether blockIdx.z also counts batches (L::BATCHED), the two loader types (L::LA, L::LB: their registers are the kernel's own locals) and
// how they are called: prepare(g, la, lb, m0, n0, kbeg) once, load(g, la, lb, A, B, m0, n0, k0, kend) = fetch the K-tile at k0 of both
// operands into the loaders' registers; la.store(As) / lb.store(Bs) write those registers to LDS as bf16.  The next K-tile is loaded under the
// current one's MFMAs.  An output element is ONE sum over the K-tiles of its split in ascending order, whatever M, N or the grid are.
// One __global__ template and not a shared __device__ body called from two kernels: behind a function boundary, however it is inlined, the
// same statements get another schedule and register allocation (profiles/waveglow_refactor_codegen.txt), and these kernels are tuned.
template <class L>
__global__ __launch_bounds__(256) void gemm_tile128_kernel(typename L::Args args) {
    __shared__ __attribute__((aligned(16))) __bf16 As[GT_BM * GT_LD];
    __shared__ __attribute__((aligned(16))) __bf16 Bs[GT_BN * GT_LD];
    const GemmTileArgs& g = L::tile(args);

    const int tiles_n = (g.N + GT_BN - 1) / GT_BN;
    const int tile = gemm_xcd_tile(blockIdx.x, gridDim.x);
    const int tile_m = tile / tiles_n, tile_n = tile % tiles_n;
    const int batch = L::BATCHED ? blockIdx.z / g.split_k : 0, split = L::BATCHED ? blockIdx.z % g.split_k : blockIdx.z;
    const auto* A = L::a(args) + (long)batch * g.stride_a;
    const auto* B = L::b(args) + (long)batch * g.stride_b;
    float* C = g.C + (long)batch * g.stride_c;
    const int m0 = tile_m * GT_BM, n0 = tile_n * GT_BN;
    const int kbeg = split * g.k_per_split;
    const int kend = min(g.K, kbeg + g.k_per_split);

    typename L::LA la; typename L::LB lb;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wrow = (wave >> 1) * 64, wcol = (wave & 1) * 64;
    const int l31 = lane & 31, kg = lane >> 5;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    L::prepare(g, la, lb, m0, n0, kbeg);
    if (kbeg < kend) L::load(g, la, lb, A, B, m0, n0, kbeg, kend);
    for (int k0 = kbeg; k0 < kend; k0 += GT_BK) {
        __syncthreads();                       // previous tile fully consumed
        la.store(As);
        lb.store(Bs);
        __syncthreads();
        if (k0 + GT_BK < kend) L::load(g, la, lb, A, B, m0, n0, k0 + GT_BK, kend);      // prefetch next tile while this one is multiplied
#pragma unroll
        for (int ks = 0; ks < GT_BK / 16; ++ks) {
            gemm_bf16x8 a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const gemm_bf16x8*>(As + (wrow + i * 32 + l31) * GT_LD + ks * 16 + kg * 8);
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const gemm_bf16x8*>(Bs + (wcol + j * 32 + l31) * GT_LD + ks * 16 + kg * 8);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }

    gemm_store_tile<2, 2>(g, acc, C, m0 + wrow, n0 + wcol, lane, split == 0, g.split_k > 1);
}

// ---- host side ----------------------------------------------------------------------------
// K range of one of `split` pieces: whole K-tiles of depth bk, at least one
static inline int gemm_k_per_split(int K, int split, int bk) {
    const int kps = ((K + split - 1) / split + bk - 1) / bk * bk;
    return kps < bk ? bk : kps;
}

// What every descriptor (mstts_gemm_desc, mstts_gemm_res_desc) is checked for first, for the entry point `who` (the prefix of its error
// texts): it is there, its dims are non-negative and fit an int, its operands are there.  Fills g->M, N, K; an empty product (M or N zero)
// returns MSTTS_OK with g->M = g->N = 0 and nothing else filled: the caller returns.
template <class Desc>
static inline int gemm_desc_dims(const Desc* d, const char* who, GemmTileArgs* g) {
    MSTTS_REQUIRE(d != nullptr, MSTTS_ERR_SHAPE, "%s: null descriptor", who);
    MSTTS_REQUIRE(d->M >= 0 && d->N >= 0 && d->K >= 0, MSTTS_ERR_SHAPE, "%s: negative dims", who);
    if (d->M == 0 || d->N == 0) { g->M = g->N = 0; return MSTTS_OK; }
    MSTTS_REQUIRE(d->A && d->B && d->C, MSTTS_ERR_SHAPE, "%s: null operand", who);
    MSTTS_REQUIRE(d->M < (1LL << 31) && d->N < (1LL << 31) && d->K < (1LL << 31), MSTTS_ERR_SHAPE, "%s: dims exceed int32", who);
    g->M = (int)d->M; g->N = (int)d->N; g->K = (int)d->K;
    return MSTTS_OK;
}

// Validates a descriptor for the entry point `who` ("gemm" / "gemm_bf16": the prefix of its error texts) and fills the common argument block
// (k_per_split for K-tiles of depth bk).  max_ld > 0: the entry point's kernels address rows with 32-bit tile-relative offsets.  An empty
// product is gemm_desc_dims's.
// *vec: every float4 the loaders form is 16-byte aligned and does not straddle a conv tap or the end of a row.
static inline int gemm_args_from(const mstts_gemm_desc* d, const char* who, int bk, long max_ld, GemmTileArgs* g, bool* vec) {
    const int rc = gemm_desc_dims(d, who, g);
    if (rc != MSTTS_OK || g->M == 0 || g->N == 0) return rc;
    MSTTS_REQUIRE(max_ld <= 0 || (d->lda >= 0 && d->ldb >= 0 && d->lda < max_ld && d->ldb < max_ld), MSTTS_ERR_SHAPE,
                  "%s: row strides must be below 2^24 elements (tile-relative offsets are 32-bit)", who);
    const int split = d->split_k > 1 ? d->split_k : 1;
    MSTTS_REQUIRE(split == 1 || (d->act == MSTTS_ACT_NONE), MSTTS_ERR_SHAPE,
                  "%s: split_k needs act=none (output must be pre-zeroed or accumulated into)", who);
    if (d->win_T > 0) {
        MSTTS_REQUIRE(d->win_C > 0 && d->lda == d->win_C, MSTTS_ERR_SHAPE, "%s: window mode needs lda == win_C", who);
        MSTTS_REQUIRE(d->win_C % 4 == 0, MSTTS_ERR_SHAPE, "%s: window mode needs win_C %% 4 == 0", who);
    }
    g->A = d->A; g->B = d->B; g->C = d->C; g->bias = d->bias;
    g->lda = d->lda; g->ldb = d->ldb; g->ldc = d->ldc;
    g->win_T = d->win_T; g->win_C = d->win_C > 0 ? d->win_C : 1; g->win_pad = d->win_pad; g->win_dil = d->win_dil > 0 ? d->win_dil : 1;
    g->act = d->act; g->accumulate = d->accumulate; g->split_k = split;
    g->stride_a = d->stride_a; g->stride_b = d->stride_b; g->stride_c = d->stride_c;
    g->alpha = d->alpha;
    g->k_per_split = gemm_k_per_split(g->K, split, bk);
    bool v = aligned16(d->A) && aligned16(d->B) && (d->lda % 4 == 0) && (d->ldb % 4 == 0) &&
             (d->stride_a % 4 == 0) && (d->stride_b % 4 == 0);
    v = v && (d->trans_a ? (d->M % 4 == 0) : (d->K % 4 == 0));
    v = v && (d->trans_b ? (d->K % 4 == 0) : (d->N % 4 == 0));
    if (d->win_T > 0) v = v && (d->win_C % 4 == 0);
    *vec = v;
    return MSTTS_OK;
}

// One launch path.  A kernel family F names its instantiations - F::Args, F::THREADS, F::LDS_BYTES (dynamic LDS) and
// F::template kernel<TA, TB, VEC, WIN>() - and the run-time (trans_a, trans_b, vec, win) index one table of the 16 kernel pointers, which
// serves both the attribute call and the launch.
template <class F> using GemmKernelFn = void (*)(typename F::Args);
template <class F, size_t... I>
static const GemmKernelFn<F>* gemm_kernel_table(std::index_sequence<I...>) {
    static const GemmKernelFn<F> table[16] = {F::template kernel<(I & 8) != 0, (I & 4) != 0, (I & 2) != 0, (I & 1) != 0>()...};
    return table;
}
template <class F>
static const GemmKernelFn<F>* gemm_kernel_table() { return gemm_kernel_table<F>(std::make_index_sequence<16>()); }
// raises the family's dynamic-LDS limit on the current device, once per device; 0: the device refuses (the caller takes a smaller kernel)
template <class F>
static int gemm_ready() {
    static int memo[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    if (!memo[dev]) {
        bool ok = true;
        for (int i = 0; i < 16; ++i)
            ok = ok && hipFuncSetAttribute((const void*)gemm_kernel_table<F>()[i], hipFuncAttributeMaxDynamicSharedMemorySize, (int)F::LDS_BYTES) == hipSuccess;
        if (!ok) (void)hipGetLastError();
        memo[dev] = ok ? 2 : 1;
    }
    return memo[dev] == 2;
}
template <class F>
static void gemm_launch(const typename F::Args& g, bool ta, bool tb, bool vec, bool win, dim3 grid, hipStream_t st) {
    const int variant = (ta ? 8 : 0) + (tb ? 4 : 0) + (vec ? 2 : 0) + (win ? 1 : 0);
    hipLaunchKernelGGL(gemm_kernel_table<F>()[variant], grid, dim3(F::THREADS), F::LDS_BYTES, st, g);
}

}  // namespace mstts
