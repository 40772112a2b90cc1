// Contraction on operands that ALREADY ARE bf16 in memory (v_mfma_f32_32x32x16_bf16, fp32 accumulate, fp32 C): the resident form of
// gemm_bf16_kernel (gemm_bf16.hip).  That kernel reads fp32 operands and rounds them on the way into LDS - 4 bytes of HBM / L2 traffic per
// multiplicand and a conversion (plus, for a [K, N] weight, a register transposition) per element.  Here A is bf16 [M, lda] and B is bf16
// [N, ldb], BOTH k-contiguous (the weight stored transposed, packed once at load), so staging is a copy: a thread moves 16-byte runs
// (8 elements) from global memory to their LDS rows with one global_load_dwordx4 and one ds_write_b128 each - half the bytes, no VALU.
//
// Everything but the loaders is shared with the fp32-operand form: gemm_tile128_kernel (gemm_tile.h) - LDS image, K loop with its register
// prefetch, fragment reads, MFMA block, the gemm_store_tile epilogue with bias, accumulate, split-k atomics and ldc.
//
// Window mode (win_T > 0: A is the implicit im2col view of X[rows, win_C], see mstts_gemm_desc at trans_a = 0): win_C % 8 == 0, so a run
// never straddles a tap - it is loaded whole, or zeroed whole when m % win_T + (tap - win_pad) * win_dil leaves [0, win_T).  Rows past M,
// rows of B past N and runs at or past the split's kend read as zero (from the loaders' zero block: the loads stay unconditional).
#include "gemm_tile.h"

namespace mstts {

typedef unsigned gr_u32x4 __attribute__((ext_vector_type(4)));
typedef const gr_u32x4 __attribute__((address_space(1)))* gr_gptr;       // explicit global loads (see gemm_ld4, gemm_tile.h)

struct GemmResArgs {
    GemmTileArgs t;                       // what the shared epilogue reads (A / B unused there: the operands are the two below)
    const __bf16* A; const __bf16* B;
};

// Thread (k8 = tid & 7, r = tid >> 3 in 0..31) takes the 16-byte k-run k8 of rows r, r + 32, r + 64, r + 96: a wave reads 128 contiguous
// bytes from each of 8 rows.  prepare() once, then load() for k0, k0 + GT_BK, ... (window: tap / kc kept incrementally).
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
        if (WIN) {                                  // next call is for k0 + GT_BK
            kc += GT_BK;
            while (kc >= wC) { kc -= wC; ++tap; }
        }
    }
    __device__ __forceinline__ void store(__bf16* __restrict__ s) const {
        const int k8 = threadIdx.x & 7, r = threadIdx.x >> 3;
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<gr_u32x4*>(s + (r + i * 32) * GT_LD + k8 * 8) = reg[i];
    }
};

// the loader pair of gemm_tile128_kernel (gemm_tile.h): A through the window when WIN, B plain
template <bool WIN>
struct GrLoaders {
    using Args = GemmResArgs;
    using LA = GrLoader<WIN>;
    using LB = GrLoader<false>;
    static constexpr bool BATCHED = false;
    static __device__ __forceinline__ const GemmTileArgs& tile(const Args& a) { return a.t; }
    static __device__ __forceinline__ const __bf16* a(const Args& a) { return a.A; }
    static __device__ __forceinline__ const __bf16* b(const Args& a) { return a.B; }
    static __device__ __forceinline__ void prepare(const GemmTileArgs& g, LA& la, LB& lb, int m0, int n0, int kbeg) {
        la.prepare(m0, kbeg, g.M, g.lda, g.win_T, g.win_C);
        lb.prepare(n0, kbeg, g.N, g.ldb, 0, 1);
    }
    static __device__ __forceinline__ void load(const GemmTileArgs& g, LA& la, LB& lb, const __bf16* A, const __bf16* B, int, int, int k0, int kend) {
        la.load(A, k0, kend, g.lda, g.win_T, g.win_C, g.win_pad, g.win_dil);
        lb.load(B, k0, kend, g.ldb, 0, 1, 0, 1);
    }
};

// (in a profile: gemm_tile128_kernel<GrLoaders<WIN>>)
template <bool WIN> constexpr auto gemm_bf16_res_kernel = &gemm_tile128_kernel<GrLoaders<WIN>>;

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
    GemmResArgs a;
    GemmTileArgs& g = a.t;
    const int rc = gemm_desc_dims(d, "gemm_bf16_res", &g);
    if (rc != MSTTS_OK || g.M == 0 || g.N == 0) return rc;
    MSTTS_REQUIRE(gemm_res_strides_ok(d->K, d->lda, d->ldb, d->win_T, d->win_C), MSTTS_ERR_ALIGN,
                  "gemm_bf16_res: K, lda, ldb and win_C must be multiples of 8 (operands move as 16-byte runs of 8 bf16)");
    MSTTS_REQUIRE(aligned16(d->A) && aligned16(d->B), MSTTS_ERR_ALIGN, "gemm_bf16_res: A and B must be 16-byte aligned");
    MSTTS_REQUIRE((reinterpret_cast<uintptr_t>(d->C) & 3u) == 0 && (reinterpret_cast<uintptr_t>(d->bias) & 3u) == 0, MSTTS_ERR_ALIGN,
                  "gemm_bf16_res: C and bias must be 4-byte aligned");
    if (d->win_T > 0) MSTTS_REQUIRE(d->lda == d->win_C, MSTTS_ERR_SHAPE, "gemm_bf16_res: window mode needs lda == win_C");
    else MSTTS_REQUIRE(d->lda >= d->K, MSTTS_ERR_SHAPE, "gemm_bf16_res: lda < K");
    MSTTS_REQUIRE(d->ldb >= d->K && d->ldc >= d->N, MSTTS_ERR_SHAPE, "gemm_bf16_res: ldb < K or ldc < N");
    const int split = d->split_k > 1 ? d->split_k : 1;
    const long tiles = (long)cdiv(d->M, GT_BM) * cdiv(d->N, GT_BN);
    MSTTS_REQUIRE(tiles < (1LL << 31) && split <= 65535, MSTTS_ERR_SHAPE, "gemm_bf16_res: grid too large");

    a.A = (const __bf16*)d->A; a.B = (const __bf16*)d->B;
    g.A = nullptr; g.B = nullptr; g.C = d->C; g.bias = d->bias;
    g.lda = d->lda; g.ldb = d->ldb; g.ldc = d->ldc;
    g.win_T = d->win_T > 0 ? d->win_T : 0; g.win_C = d->win_C > 0 ? d->win_C : 1; g.win_pad = d->win_pad; g.win_dil = d->win_dil > 0 ? d->win_dil : 1;
    g.act = MSTTS_ACT_NONE; g.accumulate = d->accumulate; g.split_k = split;
    g.stride_a = g.stride_b = g.stride_c = 0;
    g.alpha = 1.f;
    g.k_per_split = gemm_k_per_split(g.K, split, GT_BK);
    dim3 grid((unsigned)tiles, 1, split);
    if (g.win_T > 0) hipLaunchKernelGGL(gemm_bf16_res_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(gemm_bf16_res_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
    MSTTS_CHECK_LAUNCH("gemm_bf16_res");
    return MSTTS_OK;
}
