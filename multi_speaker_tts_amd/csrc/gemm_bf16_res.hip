// Contraction on operands that ALREADY ARE bf16 in memory (v_mfma_f32_32x32x16_bf16, fp32 accumulate, fp32 C): the resident form of
// gemm_bf16_kernel (gemm_bf16.hip).  That kernel reads fp32 operands and rounds them on the way into LDS - 4 bytes of HBM / L2 traffic per
// multiplicand and a conversion (plus, for a [K, N] weight, a register transposition) per element.  Here A is bf16 [M, lda] and B is bf16
// [N, ldb], BOTH k-contiguous (the weight stored transposed, packed once at load), so staging is a copy: a thread moves 16-byte runs
// (8 elements) from global memory to their LDS rows with one global_load_dwordx4 and one ds_write_b128 each - half the bytes, no VALU.
//
// Same tile and fragment layout as gemm_bf16_kernel: 128 x 128 x 64 per 256-thread workgroup (4 wave64 as 2 x 2, each 64 x 64 = 2 x 2 MFMA
// tiles), LDS image [128 rows][64 k] bf16 at a row stride of 144 B (fragment reads are conflict-free ds_read_b128), the same epilogue
// (gemm_store_tile: bias, accumulate, split-k atomics, ldc).  The next K-tile is prefetched into registers under the current one's MFMAs.
// An output element is ONE sum over the K-tiles of its split in ascending order, whatever M, N or the grid are.
//
// Window mode (win_T > 0: A is the implicit im2col view of X[rows, win_C], see mstts_gemm_desc at trans_a = 0): win_C % 8 == 0, so a run
// never straddles a tap - it is loaded whole, or zeroed whole when m % win_T + (tap - win_pad) * win_dil leaves [0, win_T).  Rows past M,
// rows of B past N and runs at or past the split's kend read as zero (from the loaders' zero block: the loads stay unconditional).
#include "gemm_tile.h"

namespace mstts {

typedef __bf16 gr_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned gr_u32x4 __attribute__((ext_vector_type(4)));
typedef const gr_u32x4 __attribute__((address_space(1)))* gr_gptr;       // explicit global loads (see gemm_ld4, gemm_tile.h)

constexpr int GR_BM = 128, GR_BN = 128, GR_BK = 64;
constexpr int GR_LD = 72;                 // LDS row stride in bf16 elements (144 B), as in gemm_bf16_kernel

struct GemmResArgs {
    GemmTileArgs t;                       // what the shared epilogue reads (A / B unused there: the operands are the two below)
    const __bf16* A; const __bf16* B;
};

// Thread (k8 = tid & 7, r = tid >> 3 in 0..31) takes the 16-byte k-run k8 of rows r, r + 32, r + 64, r + 96: a wave reads 128 contiguous
// bytes from each of 8 rows.  prepare() once, then load() for k0, k0 + GR_BK, ... (window: tap / kc kept incrementally).
template <bool WIN>
struct GrLoader {
    gr_u32x4 reg[4];
    long roff[4];                         // row * ld
    int t_row[4], rows_left[4];           // row % win_T ; rows - row (> 0: the row is inside the operand)
    int tap, kc;
    __device__ __forceinline__ void prepare(int row0, int k0, int rows, long ld, int wT, int wC) {
        const int k8 = threadIdx.x & 7, r = threadIdx.x >> 3;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = row0 + r + i * 32;
            rows_left[i] = rows - row;
            roff[i] = (long)row * ld;
            t_row[i] = WIN ? row % wT : 0;
        }
        tap = 0; kc = 0;
        if (WIN) {
            const int k = k0 + k8 * 8;
            tap = k / wC; kc = k - tap * wC;
        }
    }
    __device__ __forceinline__ void load(const __bf16* __restrict__ base, int k0, int kend, long ld, int wT, int wC, int wpad, int wdil) {
        const int k = k0 + (threadIdx.x & 7) * 8;
        const bool kok = k < kend;
        const int sh = WIN ? (tap - wpad) * wdil : 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bool ok = kok && rows_left[i] > 0;
            long off = roff[i] + k;
            if (WIN) {
                const int t = t_row[i] + sh;
                ok = ok && t >= 0 && t < wT && sh < rows_left[i];        // (the last: a final sequence shorter than win_T)
                off = roff[i] + (long)sh * ld + kc;
            }
            reg[i] = *(gr_gptr)(ok ? (const void*)(base + off) : (const void*)gemm_zero16);
        }
        if (WIN) {                                  // next call is for k0 + GR_BK
            kc += GR_BK;
            while (kc >= wC) { kc -= wC; ++tap; }
        }
    }
    __device__ __forceinline__ void store(__bf16* __restrict__ s) const {
        const int k8 = threadIdx.x & 7, r = threadIdx.x >> 3;
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<gr_u32x4*>(s + (r + i * 32) * GR_LD + k8 * 8) = reg[i];
    }
};

template <bool WIN>
__global__ __launch_bounds__(256) void gemm_bf16_res_kernel(GemmResArgs a) {
    __shared__ __attribute__((aligned(16))) __bf16 As[GR_BM * GR_LD];
    __shared__ __attribute__((aligned(16))) __bf16 Bs[GR_BN * GR_LD];
    const GemmTileArgs& g = a.t;

    const int tiles_n = (g.N + GR_BN - 1) / GR_BN;
    const int tile = gemm_xcd_tile(blockIdx.x, gridDim.x);
    const int tile_m = tile / tiles_n, tile_n = tile % tiles_n;
    const int split = blockIdx.z;
    const int m0 = tile_m * GR_BM, n0 = tile_n * GR_BN;
    const int kbeg = split * g.k_per_split;
    const int kend = min(g.K, kbeg + g.k_per_split);

    GrLoader<WIN> la; GrLoader<false> lb;

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

    la.prepare(m0, kbeg, g.M, g.lda, g.win_T, g.win_C);
    lb.prepare(n0, kbeg, g.N, g.ldb, 0, 1);
    if (kbeg < kend) {
        la.load(a.A, kbeg, kend, g.lda, g.win_T, g.win_C, g.win_pad, g.win_dil);
        lb.load(a.B, kbeg, kend, g.ldb, 0, 1, 0, 1);
    }
    for (int k0 = kbeg; k0 < kend; k0 += GR_BK) {
        __syncthreads();                       // previous tile fully consumed
        la.store(As);
        lb.store(Bs);
        __syncthreads();
        if (k0 + GR_BK < kend) {               // prefetch next tile while this one is multiplied
            la.load(a.A, k0 + GR_BK, kend, g.lda, g.win_T, g.win_C, g.win_pad, g.win_dil);
            lb.load(a.B, k0 + GR_BK, kend, g.ldb, 0, 1, 0, 1);
        }
#pragma unroll
        for (int ks = 0; ks < GR_BK / 16; ++ks) {
            gr_bf16x8 fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const gr_bf16x8*>(As + (wrow + i * 32 + l31) * GR_LD + ks * 16 + kg * 8);
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[j] = *reinterpret_cast<const gr_bf16x8*>(Bs + (wcol + j * 32 + l31) * GR_LD + ks * 16 + kg * 8);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
    }

    gemm_store_tile<2, 2>(g, acc, g.C, m0 + wrow, n0 + wcol, lane, split == 0, g.split_k > 1);
}

static bool gemm_res_strides_ok(int64_t K, int64_t lda, int64_t ldb, int32_t win_T, int32_t win_C) {
    return K % 8 == 0 && lda % 8 == 0 && ldb % 8 == 0 && (win_T <= 0 || (win_C > 0 && win_C % 8 == 0));
}

}  // namespace mstts

using namespace mstts;

extern "C" int mstts_gemm_bf16_res_supported(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int32_t win_T, int32_t win_C) {
    const int64_t lim = 1LL << 31;
    if (M < 0 || N < 0 || K < 0 || M >= lim || N >= lim || K >= lim || lda < 0 || ldb < K) return 0;
    if (!gemm_res_strides_ok(K, lda, ldb, win_T, win_C)) return 0;
    return win_T > 0 ? lda == win_C : lda >= K;
}

extern "C" int mstts_gemm_bf16_res(const mstts_gemm_res_desc* d, mstts_stream_t stream) {
    MSTTS_REQUIRE(d != nullptr, MSTTS_ERR_SHAPE, "gemm_bf16_res: null descriptor");
    MSTTS_REQUIRE(d->M >= 0 && d->N >= 0 && d->K >= 0, MSTTS_ERR_SHAPE, "gemm_bf16_res: negative dims");
    if (d->M == 0 || d->N == 0) return MSTTS_OK;
    MSTTS_REQUIRE(d->A && d->B && d->C, MSTTS_ERR_SHAPE, "gemm_bf16_res: null operand");
    MSTTS_REQUIRE(d->M < (1LL << 31) && d->N < (1LL << 31) && d->K < (1LL << 31), MSTTS_ERR_SHAPE, "gemm_bf16_res: dims exceed int32");
    MSTTS_REQUIRE(gemm_res_strides_ok(d->K, d->lda, d->ldb, d->win_T, d->win_C), MSTTS_ERR_ALIGN,
                  "gemm_bf16_res: K, lda, ldb and win_C must be multiples of 8 (operands move as 16-byte runs of 8 bf16)");
    MSTTS_REQUIRE(aligned16(d->A) && aligned16(d->B), MSTTS_ERR_ALIGN, "gemm_bf16_res: A and B must be 16-byte aligned");
    MSTTS_REQUIRE((reinterpret_cast<uintptr_t>(d->C) & 3u) == 0 && (reinterpret_cast<uintptr_t>(d->bias) & 3u) == 0, MSTTS_ERR_ALIGN,
                  "gemm_bf16_res: C and bias must be 4-byte aligned");
    if (d->win_T > 0) MSTTS_REQUIRE(d->lda == d->win_C, MSTTS_ERR_SHAPE, "gemm_bf16_res: window mode needs lda == win_C");
    else MSTTS_REQUIRE(d->lda >= d->K, MSTTS_ERR_SHAPE, "gemm_bf16_res: lda < K");
    MSTTS_REQUIRE(d->ldb >= d->K && d->ldc >= d->N, MSTTS_ERR_SHAPE, "gemm_bf16_res: ldb < K or ldc < N");
    const int split = d->split_k > 1 ? d->split_k : 1;
    const long tiles = (long)cdiv(d->M, GR_BM) * cdiv(d->N, GR_BN);
    MSTTS_REQUIRE(tiles < (1LL << 31) && split <= 65535, MSTTS_ERR_SHAPE, "gemm_bf16_res: grid too large");

    GemmResArgs a;
    GemmTileArgs& g = a.t;
    a.A = (const __bf16*)d->A; a.B = (const __bf16*)d->B;
    g.A = nullptr; g.B = nullptr; g.C = d->C; g.bias = d->bias;
    g.M = (int)d->M; g.N = (int)d->N; g.K = (int)d->K;
    g.lda = d->lda; g.ldb = d->ldb; g.ldc = d->ldc;
    g.win_T = d->win_T > 0 ? d->win_T : 0; g.win_C = d->win_C > 0 ? d->win_C : 1; g.win_pad = d->win_pad; g.win_dil = d->win_dil > 0 ? d->win_dil : 1;
    g.act = MSTTS_ACT_NONE; g.accumulate = d->accumulate; g.split_k = split;
    g.stride_a = g.stride_b = g.stride_c = 0;
    g.alpha = 1.f;
    g.k_per_split = gemm_k_per_split(g.K, split, GR_BK);
    dim3 grid((unsigned)tiles, 1, split);
    if (g.win_T > 0) hipLaunchKernelGGL(gemm_bf16_res_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(gemm_bf16_res_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
    MSTTS_CHECK_LAUNCH("gemm_bf16_res");
    return MSTTS_OK;
}
