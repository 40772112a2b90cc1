// Batch gather out of a device-resident mel bank: the speaker-encoder trainer's feeder (Speaker_Embedding/Feeder.py:66-100 cuts
// Batch_Speaker x Batch_per_Speaker utterances to one random frame count per batch, by a random crop or a random zero-padded placement).
// Every utterance's mel lies back to back in `bank` [total_frames, n_mel], file f at frames frame_off[f] .. frame_off[f + 1]; the host
// draws one table row (file, src_start, dst_start, count) per output row and ONE launch writes the whole batch:
//   out[r, t, :] = bank[frame_off[file] + src_start + (t - dst_start), :]   for dst_start <= t < dst_start + count,   0 elsewhere.
// Every element of out is stored exactly once (the caller never clears it).  A workgroup owns FRAMES consecutive frames of one row: they
// are contiguous in out and - inside the copied range - in the bank, so the body is one linear index with two bounds, no division.
// A row that would read outside its file or write outside its T frames (file outside [0, n_files), a negative field, src_start + count
// beyond the file, dst_start + count beyond T) copies nothing: it is written as zeros and bit 0 of *status is set.
#include "common.h"

namespace mstts {

typedef float mel_v4 __attribute__((ext_vector_type(4)));      // (a native vector: the select below stays in registers)
constexpr int MEL_BANK_FRAMES = 32;          // frames per workgroup: 320 x 180 x 80 -> 320 x 6 = 1 920 workgroups, 7.5 per CU

template <typename V>                        // V = mel_v4 (n_mel % 4 == 0, both pointers 16-byte aligned) or float; W = n_mel in units of V
__global__ __launch_bounds__(256) void mel_bank_gather_kernel(const V* __restrict__ bank, const long long* __restrict__ frame_off, int n_files,
                                                              const int4* __restrict__ table, int T, int W, int blocks_per_row,
                                                              V* __restrict__ out, int* __restrict__ status) {
    const int r = blockIdx.x / blocks_per_row, blk = blockIdx.x - r * blocks_per_row;
    const int4 row = table[r];
    const int file = row.x, src = row.y, dst = row.z;
    int count = row.w;
    bool ok = file >= 0 && file < n_files && src >= 0 && dst >= 0 && count >= 0;
    long base = 0;
    if (ok) {
        const long f0 = frame_off[file], f1 = frame_off[file + 1];
        ok = (long)src + count <= f1 - f0 && (long)dst + count <= T;
        base = f0 + src;
    }
    if (!ok) {
        count = 0;
        if (blk == 0 && threadIdx.x == 0) atomicOr(status, 1);
    }
    const int t0 = blk * MEL_BANK_FRAMES;
    const int n = min(MEL_BANK_FRAMES, T - t0) * W;                 // elements of this workgroup
    const long lo = ((long)dst - t0) * W, hi = lo + (long)count * W;     // ... of which [lo, hi) are copied
    const long shift = base * W - lo;                                    // bank index of element e; read only at lo <= e < hi: frames base .. base + count
    V* to = out + ((long)r * T + t0) * W;
    for (int e = threadIdx.x; e < n; e += 256) {
        V v = V(0.f);
        if (e >= lo && e < hi) v = bank[shift + e];
        to[e] = v;
    }
}

}  // namespace mstts
using namespace mstts;

/* bank [total_frames, n_mel] fp32, frame_off int64 [n_files + 1], table int32 [N, 4] = (file, src_start, dst_start, count) per row,
 * out [N, T, n_mel] fp32, status int32 [1] (bit 0 is OR-ed in when a row is invalid; the caller zeroes it once) - all on the device */
extern "C" int mstts_mel_bank_gather(const float* bank, const int64_t* frame_off, int64_t n_files, const int32_t* table, int64_t N, int64_t T,
                                     int64_t n_mel, float* out, int32_t* status, mstts_stream_t s) {
    MSTTS_REQUIRE(bank && frame_off && table && out && status, MSTTS_ERR_SHAPE, "mel_bank_gather: null pointer");
    MSTTS_REQUIRE(N >= 1 && T >= 1 && n_mel >= 1 && n_files >= 1, MSTTS_ERR_SHAPE, "mel_bank_gather: need N, T, n_mel, n_files >= 1");
    MSTTS_REQUIRE(aligned16(table), MSTTS_ERR_SHAPE, "mel_bank_gather: the table must be 16-byte aligned");
    const int64_t bpr = (T + MEL_BANK_FRAMES - 1) / MEL_BANK_FRAMES;
    MSTTS_REQUIRE(n_files < (1ll << 31) && T * n_mel < (1ll << 31) && N * bpr < (1ll << 31), MSTTS_ERR_SHAPE, "mel_bank_gather: batch too large");
    const dim3 grid((unsigned)(N * bpr)), block(256);
    if (n_mel % 4 == 0 && aligned16(bank) && aligned16(out))
        hipLaunchKernelGGL(mel_bank_gather_kernel<mel_v4>, grid, block, 0, (hipStream_t)s, (const mel_v4*)bank, (const long long*)frame_off, (int)n_files,
                           (const int4*)table, (int)T, (int)(n_mel / 4), (int)bpr, (mel_v4*)out, (int*)status);
    else
        hipLaunchKernelGGL(mel_bank_gather_kernel<float>, grid, block, 0, (hipStream_t)s, bank, (const long long*)frame_off, (int)n_files,
                           (const int4*)table, (int)T, (int)n_mel, (int)bpr, out, (int*)status);
    MSTTS_CHECK_LAUNCH("mel_bank_gather");
    return MSTTS_OK;
}
