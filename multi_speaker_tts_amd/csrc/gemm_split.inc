// fp32 GEMM on the gfx950 bf16 matrix cores: every fp32 operand element is split EXACTLY into three bf16 terms
//     x = hi + mid + lo,   hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid)      (round-to-nearest-even; both differences are exact in fp32)
// and a product a.b is evaluated as the six bf16 x bf16 products (each exact in fp32: 8 + 8 significand bits)
//     hi.hi + hi.mid + mid.hi + mid.mid + hi.lo + lo.hi
// accumulated in fp32 by v_mfma_f32_32x32x16_bf16.  What is dropped - mid.lo + lo.mid + lo.lo - is at most 2^-26 |a||b| (|mid| <= 2^-9 |x|,
// |lo| <= 2^-18 |x| with nearest rounding), a quarter of the 2^-24 unit roundoff every fp32 accumulation of that product incurs anyway: the
// result is an fp32 GEMM (fp32 in memory, fp32 accumulators, error against fp64 equal to the v_mfma_f32_32x32x2_f32 kernel's - measured in
// tests/test_gpu_ops.py::test_gemm_split_is_fp32_accurate), at 6/16 of the fp32 matrix-core time: the f32-input MFMA runs at 1/16 of the
// bf16 rate on this chip (157 vs 2 500 TFLOP/s).  This is NOT config 3's bf16 arithmetic (gemm_bf16.hip: one bf16 term, 2^-9 per product).
//
// Tile 128 x 128 x 32 per 768-thread workgroup, one workgroup per CU, the twelve waves SPECIALISED, three per SIMD: waves 0-3 are consumers
// (2 x 2, each 64 x 64 = 2 x 2 MFMA tiles x 2 k-steps x 6 products per K-tile) that only read fragments and issue MFMAs; waves 4-7 stage
// operand A and waves 8-11 operand B - they load the fp32 K-tiles two tiles ahead into registers, split every element once and write the
// three bf16 planes into the LDS buffer the consumers read next.  A SIMD therefore always holds one wave whose stream is MFMA/LDS-read and two
// whose stream is VALU/LDS-write/global-load, and the hardware interleaves them - no hand-built software pipeline.  (The first form - every
// wave doing both, two workgroups per CU - ran the phases of both workgroups in lockstep: 160 TFLOP/s-equivalent, the sum of MFMA + LDS +
// VALU time per K-tile.)  164-166 VGPRs: three waves per SIMD fit.
// Measured on the eight-wave form (one producer quartet staging both operands; tools/gemm_stamp_probe.py, -DGS_STAMP): per K-tile a producer
// is busy 2 490 cycles and waits 60, a consumer is busy 2 120 and waits 440, against 1 536 cycles of MFMA issue; the loads are never waited
// for (8 cycles per tile).  Halving each producer's work (this form) buys 2-5 %, not 30: per SIMD the tile time (2 540 cycles) is the SUM of
// the matrix-core time and the vector time of its waves (1 536 + ~1 000) - they do not overlap - so the rate is set by MFMA time + split
// arithmetic: 176-191 TFLOP/s-equivalent on the 25 632-row weight gradients and 8192^3 (f32-input MFMA: 131-133).  The lever that is left is
// fewer vector instructions per MFMA: split every element once per GEMM instead of once per tile that reads it, or larger tiles.
// Two LDS buffers (2 x 60 KB), ONE barrier per K-tile: it says "tile t + 1 is written, tile t is consumed".
// LDS image of an operand: three planes [128 rows][32 k] bf16, row stride 80 B, k CONTIGUOUS per row whatever the operand's memory layout,
// so an MFMA fragment (lane l: row l & 31, k = 8 (l >> 5) .. + 7) is one conflict-free ds_read_b128.  Same descriptor, loaders (dense / conv
// window / transposed), body + tail schedule and epilogue semantics as gemm_kernel above.
// Included by gemm.hip (not a translation unit).

typedef __bf16 gs_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 gs_bf16x4 __attribute__((ext_vector_type(4)));
constexpr int GS_BM = 128, GS_LD = 40;            // LDS row stride in bf16 elements (80 B = 20 words: 8 consecutive rows cover the 32 banks once)
constexpr int GS_PLANE = 128 * GS_LD;             // bf16 elements per plane

struct Split3 { gs_bf16x4 hi, mid, lo; };
// one pair: ONE v_cvt_pk_bf16_f32 per term, the bf16 pair widened back with a shift and a mask, remainders exact.  Written as single
// instructions: left to itself the compiler converts every element twice (once alone for the remainder, once paired for the plane) and
// SLP-packs the subtractions into v_pk_add_f32, whose operands must be adjacent register pairs - for the transposing loader that means a
// copy of every loaded register, placed right behind the load, i.e. a wait for the whole prefetch at the top of every K-tile.
__device__ __forceinline__ uint32_t gs_cvt_pk(float a, float b) {
    uint32_t r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float gs_sub(float a, uint32_t b_bits) {
    float r;
    asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b_bits));
    return r;
}
__device__ __forceinline__ void gs_split2(float x0, float x1, uint32_t& hi, uint32_t& mid, uint32_t& lo) {
    hi = gs_cvt_pk(x0, x1);
    x0 = gs_sub(x0, hi << 16); x1 = gs_sub(x1, hi & 0xffff0000u);
    mid = gs_cvt_pk(x0, x1);
    x0 = gs_sub(x0, mid << 16); x1 = gs_sub(x1, mid & 0xffff0000u);
    lo = gs_cvt_pk(x0, x1);
}
__device__ __forceinline__ Split3 gs_split4(float a, float b, float c, float d) {
    uint2 h, m, l;
    gs_split2(a, b, h.x, m.x, l.x);
    gs_split2(c, d, h.y, m.y, l.y);
    Split3 s;
    s.hi = __builtin_bit_cast(gs_bf16x4, h); s.mid = __builtin_bit_cast(gs_bf16x4, m); s.lo = __builtin_bit_cast(gs_bf16x4, l);
    return s;
}
// staging policy of the split kernels (gemm_tile.h): four values -> the hi / mid / lo planes, PLANE bf16 elements apart
template <int PLANE>
struct SplitPlanes {
    static __device__ __forceinline__ void put(__bf16* __restrict__ p, float a, float b, float c, float d) {
        const Split3 s = gs_split4(a, b, c, d);
        *reinterpret_cast<gs_bf16x4*>(p) = s.hi;
        *reinterpret_cast<gs_bf16x4*>(p + PLANE) = s.mid;
        *reinterpret_cast<gs_bf16x4*>(p + 2 * PLANE) = s.lo;
    }
};

// operand contiguous along k in memory: thread (k4 = tid & 7, r = tid >> 3) takes the float4 k-run k4 of rows r, r + 32, r + 64, r + 96
template <bool VEC, bool WIN> using GsLoaderKC = TileLoaderKC<8, 4, 32, GS_LD, SplitPlanes<GS_PLANE>, VEC, WIN>;
// operand contiguous along its M/N index: thread (kq = tid & 7, c4 = tid >> 3) takes the 4 x 4 block of k rows 4 kq .. x columns 4 c4 ..
template <bool VEC, bool WIN> using GsLoaderMC = TileLoaderMC<8, GS_LD, SplitPlanes<GS_PLANE>, VEC, WIN>;

#ifdef GS_STAMP
// dev only: wave 0 (a consumer) of block 0 accumulates the time it spends inside the barrier (arrival -> release) and in the whole loop
// into g.bias (used as 3 x uint64)
#define GS_BAR(slot) do { if (stamp) { const unsigned long long t0_ = __builtin_readcyclecounter(); gemm_barrier(); acc_wait += __builtin_readcyclecounter() - t0_; } else gemm_barrier(); } while (0)
#else
#define GS_BAR(slot) gemm_barrier()
#endif

__device__ __forceinline__ int tiles_m_of(const GemmArgs& g) { return (g.M + GS_BM - 1) / GS_BM; }
constexpr int GS_NPROD = 6;
constexpr int GS_BUF = 6 * GS_PLANE;                 // bf16 elements of one LDS buffer: A planes hi/mid/lo, then B planes
constexpr size_t GS_LDS_BYTES = 2 * GS_BUF * sizeof(__bf16);

constexpr int GS_THREADS = 768;
// one operand's producer loop (12-wave form: waves 4-7 stage A, waves 8-11 stage B): tile t + 1 (register set (t + 1) & 1) is split and written
// into buffer (t + 1) & 1 between barrier t and barrier t + 1, the freed set is re-issued for tile t + 3.  Straight-line, see below.
template <class LoadFn, class StoreFn>
__device__ __forceinline__ void gs_produce(LoadFn load, StoreFn store, __bf16* lds0, int kbeg, int nt2) {
    float4 r[2][4];
    load(r[0], kbeg);
    load(r[1], kbeg + BK);
    store(r[0], lds0);
    load(r[0], kbeg + 2 * BK);
    gemm_barrier();
    for (int t = 0; t < nt2; t += 2) {
        store(r[1], lds0 + GS_BUF);
        load(r[1], kbeg + (t + 3) * BK);
        gemm_barrier();
        store(r[0], lds0);
        load(r[0], kbeg + (t + 4) * BK);
        gemm_barrier();
    }
}

template <bool TA, bool TB, bool VEC, bool WIN>
__global__ __launch_bounds__(GS_THREADS) void gemm_split_kernel(GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) __bf16 gs_lds[];

    const int tiles_n = (g.N + BN - 1) / BN;
    int tile = blockIdx.x, piece = -1;             // XCD-aware tile order and the body + tail schedule of gemm_kernel
    if (tile < g.body) {
        tile = gemm_xcd_tile(tile, g.body);
    } else {
        const int u = tile - g.body;
        tile = g.body + u / g.tail_s;
        piece = u % g.tail_s;
    }
    int tile_m = tile / tiles_n, tile_n = tile % tiles_n;
    if (g.band > 0) {
        // wide outputs: the tile list runs down column bands of `band` tiles, so the 32 tiles an XCD works on at one time form a 4 x 8
        // block (per K-tile 4 A slices + 8 B slices through its L2) instead of 1 x 32 (1 + 32): at this kernel's rate the row-major order
        // asks the memory side for 6 TB/s on the 4096-column weight gradients
        const int per_band = g.band * tiles_m_of(g), b = tile / per_band, r = tile - b * per_band;
        const int w = min(g.band, tiles_n - b * g.band);
        tile_m = r / w; tile_n = b * g.band + r - tile_m * w;
    }
    const int batch = blockIdx.z / g.split_k, split = blockIdx.z % g.split_k;
    const int m0 = tile_m * GS_BM, n0 = tile_n * BN;
    const int kbeg = piece >= 0 ? piece * g.tail_kps : split * g.k_per_split;
    const int kend = min(g.K, kbeg + (piece >= 0 ? g.tail_kps : g.k_per_split));
    const int nt = kend > kbeg ? (kend - kbeg + BK - 1) / BK : 0, nt2 = (nt + 1) & ~1;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
#ifdef GS_STAMP
    const bool stamp = blockIdx.x == 0 && blockIdx.z == 0 && wave == 0 && g.bias != nullptr;
    unsigned long long acc_wait = 0, t_begin = __builtin_readcyclecounter(), w_begin = wall_clock64();
#endif

    if (wave >= 4) {
        // ---- producers, one operand per wave quartet (three waves per SIMD: a consumer, an A producer, a B producer)
        using LA = typename std::conditional<TA, GsLoaderMC<VEC, WIN>, GsLoaderKC<VEC, WIN>>::type;
        using LB = typename std::conditional<TB, GsLoaderKC<VEC, false>, GsLoaderMC<VEC, false>>::type;
        if (wave < 8) {
            const int tid = threadIdx.x - 256;
            LA la;
            la.prepare(tid, g.A + (long)batch * g.stride_a, g.lda, m0, kbeg, g.M, g.win_T, g.win_C, g.win_pad, g.win_dil);
            gs_produce([&](float4 (&r)[4], int k) { la.load(tid, r, k, kend, g.lda, g.win_T, g.win_C, g.win_pad, g.win_dil); },
                       [&](const float4 (&r)[4], __bf16* dst) { la.store(tid, r, dst); }, gs_lds, kbeg, nt2);
        } else {
            const int tid = threadIdx.x - 512;
            LB lb;
            lb.prepare(tid, g.B + (long)batch * g.stride_b, g.ldb, n0, kbeg, g.N, 0, 1, 0, 1);
            gs_produce([&](float4 (&r)[4], int k) { lb.load(tid, r, k, kend, g.ldb, 0, 1, 0, 1); },
                       [&](const float4 (&r)[4], __bf16* dst) { lb.store(tid, r, dst); }, gs_lds + 3 * GS_PLANE, kbeg, nt2);
        }
        return;
    }

    // ---- consumers
    float* C = g.C + (long)batch * g.stride_c;
    const int lane = threadIdx.x & 63;
    const int wrow = (wave >> 1) * 64, wcol = (wave & 1) * 64;
    const int l31 = lane & 31, kg = lane >> 5;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int aoff = (wrow + l31) * GS_LD + kg * 8, boff = 3 * GS_PLANE + (wcol + l31) * GS_LD + kg * 8;
    // One consumer wave per SIMD: nobody else hides its LDS latency, so the fragments of k-step s + 1 are requested before the 24 MFMAs of
    // k-step s issue (two fragment sets, the scheduler pinned with sched_barrier), across the K-tile barrier too: the barrier sits between
    // the two k-steps of a tile - by then every read of tile t has landed (tile t is "consumed"), tile t + 1 has been written during the
    // first k-step, and its first fragments are requested behind the barrier, under the second k-step's MFMAs.
    gs_bf16x8 fa[2][2][3], fb[2][2][3];                // [set][tile row / column][plane]
    auto frags = [&](int set, const __bf16* buf, int ks) {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[set][i][p] = *reinterpret_cast<const gs_bf16x8*>(buf + aoff + p * GS_PLANE + i * 32 * GS_LD + ks * 16);
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[set][j][p] = *reinterpret_cast<const gs_bf16x8*>(buf + boff + p * GS_PLANE + j * 32 * GS_LD + ks * 16);
        }
    };
    auto products = [&](int set) {
#pragma unroll
        for (int tt = 0; tt < GS_NPROD; ++tt) {
            const int pa = (tt == 0) ? 0 : (tt == 1) ? 1 : (tt == 2) ? 0 : (tt == 3) ? 1 : (tt == 4) ? 2 : 0;
            const int pb = (tt == 0) ? 0 : (tt == 1) ? 0 : (tt == 2) ? 1 : (tt == 3) ? 1 : (tt == 4) ? 0 : 2;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[set][i][pa], fb[set][j][pb], acc[i][j], 0, 0, 0);
        }
    };
    GS_BAR(0);                                      // tile 0 is in buffer 0
    frags(0, gs_lds, 0);
    for (int t = 0; t < nt2; ++t) {
        const __bf16* buf = gs_lds + (t & 1) * GS_BUF;
        frags(1, buf, 1);
        __builtin_amdgcn_sched_barrier(0);
        products(0);                                   // (the padding tile of an odd count is all zeros: the producers wrote it from the zero block)
        __builtin_amdgcn_sched_barrier(0);
        GS_BAR(0);                                  // tile t consumed, tile t + 1 written
        frags(0, gs_lds + ((t + 1) & 1) * GS_BUF, 0);
        __builtin_amdgcn_sched_barrier(0);
        products(1);
        __builtin_amdgcn_sched_barrier(0);
    }
#ifdef GS_STAMP
    if (stamp && (threadIdx.x & 63) == 0) { unsigned long long* o = (unsigned long long*)g.bias; o[0] = acc_wait; o[1] = __builtin_readcyclecounter() - t_begin; o[2] = nt2; o[3] = wall_clock64() - w_begin; }
    if (stamp) return;
#endif
    gemm_store_tile<2, 2>(g, acc, C, m0 + wrow, n0 + wcol, lane, split == 0 && piece <= 0, g.split_k > 1 || piece >= 0);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Big-tile form of the same six-product split (round 5): 256 x 256 x 16 per 512-thread workgroup, one workgroup per CU, eight waves as 2 x 4,
// each 128 x 64 = 4 x 2 MFMA tiles (128 accumulator registers), and EVERY wave loads, splits, stages and multiplies - no producer / consumer
// split.  Per K-tile a wave issues 48 MFMAs (1 536 cycles of matrix-core time, as a consumer of the 12-wave kernel does) but splits only 16
// elements and reads 18 fragments for them: half the split arithmetic and global-load bytes and three quarters of the LDS traffic per MFMA of
// the 128 x 128 x 32 form, and two MFMA-issuing waves per SIMD, so that one wave's staging / fragment reads run under the other's matrix-core
// time (what carried the 256 x 256 bf16 kernel of gemm_bf16.hip from 430 to 714 TFLOP/s).  Two LDS buffers of 72 KB (three planes x two
// operands x 256 rows x 16 k, row stride 48 B: conflict-free b128 fragment reads), one raw barrier per K-tile:
//     k-step of tile t: fragments + first half of the products | registers of tile t + 1 -> split -> buffer (t + 1) & 1 | loads of tile t + 2 | second half | barrier
constexpr int GSB_BM = 256, GSB_BN = 256, GSB_BK = 16, GSB_LD = 24, GSB_THREADS = 512;
constexpr int GSB_PLANE = 256 * GSB_LD;                           // bf16 elements per plane
constexpr int GSB_BUF = 6 * GSB_PLANE;                            // A planes hi / mid / lo, then B planes
constexpr size_t GSB_LDS_BYTES = 2 * GSB_BUF * sizeof(__bf16);
// operand contiguous along k: thread (k4 = tid & 3, r = tid >> 2 in 0..127) takes the float4 k-run k4 of rows r and r + 128 (all 512 threads)
template <bool VEC, bool WIN> using GsbLoaderKC = TileLoaderKC<4, 2, 128, GSB_LD, SplitPlanes<GSB_PLANE>, VEC, WIN>;
// operand contiguous along its M/N index: 64 column quads x 4 k-quads = 256 blocks of 4 x 4, so ONE half of the workgroup takes a block each
// (thread u = tid & 255 of the half: kq = u & 3, c4 = u >> 2) as four float4 and writes it transposed
template <bool VEC, bool WIN> using GsbLoaderMC = TileLoaderMC<4, GSB_LD, SplitPlanes<GSB_PLANE>, VEC, WIN>;

// who stages an operand: all 512 threads one that is contiguous along k, ONE half of the workgroup (threads HALF * 256 ..) a transposed one -
// operand A on waves 0..3, operand B on waves 4..7, so that two such operands (the weight gradients) load every thread equally
template <bool TRANSPOSED, int HALF>
__device__ __forceinline__ bool gsb_stages(int tid) {
    if (TRANSPOSED) return (tid >> 8) == HALF;
    return true;
}

template <bool TA, bool TB, bool VEC, bool WIN>
__global__ __launch_bounds__(GSB_THREADS) void gemm_split_big_kernel(GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) __bf16 gs_lds[];
    const int tiles_n = (g.N + GSB_BN - 1) / GSB_BN;
    const int tile = gemm_xcd_tile(blockIdx.x, gridDim.x);
    const int tile_m = tile / tiles_n, tile_n = tile % tiles_n;
    const int batch = blockIdx.z / g.split_k, split = blockIdx.z % g.split_k;
    float* C = g.C + (long)batch * g.stride_c;
    const int m0 = tile_m * GSB_BM, n0 = tile_n * GSB_BN;
    const int kbeg = split * g.k_per_split;
    const int kend = min(g.K, kbeg + g.k_per_split);
    const int nt = kend > kbeg ? (kend - kbeg + GSB_BK - 1) / GSB_BK : 0;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wrow = (wave >> 2) * 128, wcol = (wave & 3) * 64;
    const int l31 = lane & 31, kg = lane >> 5;

    using LA = typename std::conditional<TA, GsbLoaderMC<VEC, WIN>, GsbLoaderKC<VEC, WIN>>::type;
    using LB = typename std::conditional<TB, GsbLoaderKC<VEC, false>, GsbLoaderMC<VEC, false>>::type;
    LA la; LB lb;
    const bool a_mine = gsb_stages<TA, 0>(tid), b_mine = gsb_stages<!TB, 1>(tid);              // (wave-uniform)
    const int tid_a = TA ? (tid & 255) : tid, tid_b = TB ? tid : (tid & 255);                 // index within the threads that stage the operand
    if (a_mine) la.prepare(tid_a, g.A + (long)batch * g.stride_a, g.lda, m0, kbeg, g.M, g.win_T, g.win_C, g.win_pad, g.win_dil);
    if (b_mine) lb.prepare(tid_b, g.B + (long)batch * g.stride_b, g.ldb, n0, kbeg, g.N, 0, 1, 0, 1);
    float4 ra[4], rb[4];
    auto load = [&](int k) {
        if (a_mine) la.load(tid_a, ra, k, kend, g.lda, g.win_T, g.win_C, g.win_pad, g.win_dil);
        if (b_mine) lb.load(tid_b, rb, k, kend, g.ldb, 0, 1, 0, 1);
    };
    auto store = [&](int buf) {
        if (a_mine) la.store(tid_a, ra, gs_lds + buf * GSB_BUF);
        if (b_mine) lb.store(tid_b, rb, gs_lds + buf * GSB_BUF + 3 * GSB_PLANE);
    };

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int aoff = (wrow + l31) * GSB_LD + kg * 8, boff = 3 * GSB_PLANE + (wcol + l31) * GSB_LD + kg * 8;
    // Fragments: all three B planes of the wave's two column blocks (24 registers) and TWO A-plane sets (2 x 16) that take turns - A.hi and
    // A.mid first, A.lo into the hi set once its three products have issued - instead of all 18 fragments at once (72 registers: with the
    // 128 accumulators that spilled).  Product order hi.hi, hi.mid, hi.lo | mid.hi, mid.mid | lo.hi: the same six terms as gemm_split_kernel.
    gs_bf16x8 fb[2][3], fa0[4], fa1[4];
    auto ldA = [&](gs_bf16x8 (&f)[4], const __bf16* buf, int p) {
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = *reinterpret_cast<const gs_bf16x8*>(buf + aoff + p * GSB_PLANE + i * 32 * GSB_LD);
    };
    auto ldB = [&](const __bf16* buf) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[j][p] = *reinterpret_cast<const gs_bf16x8*>(buf + boff + p * GSB_PLANE + j * 32 * GSB_LD);
    };
    auto mm = [&](const gs_bf16x8 (&f)[4], int pb) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[i], fb[j][pb], acc[i][j], 0, 0, 0);
    };

    if (nt > 0) {
        load(kbeg);
        store(0);
        load(kbeg + GSB_BK);                // (past the end: the loaders read the zero block)
        gemm_barrier();
        for (int t = 0; t < nt; ++t) {
            const __bf16* buf = gs_lds + (t & 1) * GSB_BUF;
            ldB(buf); ldA(fa0, buf, 0); ldA(fa1, buf, 1);
            mm(fa0, 0); mm(fa0, 1); mm(fa0, 2);
            ldA(fa0, buf, 2);
            store((t + 1) & 1);             // tile t + 1 (loaded one iteration ago) -> the buffer tile t - 1 was read from
            load(kbeg + (t + 2) * GSB_BK);
            mm(fa1, 0); mm(fa1, 1);
            mm(fa0, 0);
            gemm_barrier();
        }
    }
    gemm_store_tile<4, 2>(g, acc, C, m0 + wrow, n0 + wcol, lane, split == 0, g.split_k > 1);
}

struct GemmSplit {
    using Args = GemmArgs;
    static constexpr int THREADS = GS_THREADS;
    static constexpr size_t LDS_BYTES = GS_LDS_BYTES;
    template <bool TA, bool TB, bool VEC, bool WIN> static constexpr auto kernel() { return &gemm_split_kernel<TA, TB, VEC, WIN>; }
};
struct GemmSplitBig {
    using Args = GemmArgs;
    static constexpr int THREADS = GSB_THREADS;
    static constexpr size_t LDS_BYTES = GSB_LDS_BYTES;
    template <bool TA, bool TB, bool VEC, bool WIN> static constexpr auto kernel() { return &gemm_split_big_kernel<TA, TB, VEC, WIN>; }
};
