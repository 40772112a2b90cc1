// Batch features out of a device-resident bank of waveforms: the Taco1 vocoder trainer's feeder (Taco1_Mel_to_Spect/Feeder.py:46-105 pads
// Batch_Size pickled (mel, spectrogram) pairs to the batch's longest).  Both features are one STFT of the trimmed waveform, and the waveform
// is 800 B per frame where the pickled pair is 4 420 B, so the bank holds the WAVEFORMS back to back (file f at samples sig_off[f] ..
// sig_off[f + 1]) and ONE launch computes a batch's mel and spectrogram straight into the padded batch tensors:
//   F_r = 1 + len(files[r]) / hop
//   mel_out[r, t, :], spec_out[r, t, :] = frame t of mstts_stft_fft on that waveform   for t < F_r,   0 for F_r <= t < T.
// A workgroup per (row, frame); the frame's arithmetic is stft_frame_body (csrc/stft_frame.h), the code stft_fft_kernel runs, so a valid
// frame has the bits of mstts_stft_fft.  Every element of both outputs is stored exactly once (the caller never clears them).  A row whose
// file lies outside [0, n_files), whose waveform is not longer than the reflect padding (len <= n_fft / 2) or has more than T frames reads
// nothing from the bank: it is written as zeros and bit 0 of *status is set.  Pad frames and invalid rows leave before touching LDS.
#include "common.h"
#include "stft_frame.h"

namespace mstts {

__global__ __launch_bounds__(256) void stft_bank_batch_kernel(const float* __restrict__ bank, const long* __restrict__ sig_off, int n_files,
                                                              const int* __restrict__ files, int T, float coef,
                                                              const float* __restrict__ window, const float2* __restrict__ tw,
                                                              const float* __restrict__ mel_basis, const int* __restrict__ mel_rng, int n_fft,
                                                              int hop, int win, int n_mel, float max_abs, float ref_db,
                                                              float* __restrict__ mel_out, float* __restrict__ spec_out, int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) float2 fft_lds[];
    const int r = blockIdx.x / T, t = blockIdx.x - r * T;          // (the host checked N * T < 2^31)
    const int file = files[r];
    const int NB = (n_fft >> 1) + 1;
    long s0 = 0, n = 0, F = 0;
    bool ok = file >= 0 && file < n_files;
    if (ok) {
        s0 = sig_off[file];
        n = sig_off[file + 1] - s0;
        F = 1 + n / hop;
        ok = n > (n_fft >> 1) && F <= T;
    }
    if (!ok) {
        F = 0;
        if (t == 0 && threadIdx.x == 0) atomicOr(status, 1);
    }
    const long g = blockIdx.x;
    float* mel_row = mel_out ? mel_out + g * n_mel : nullptr;
    float* spec_row = spec_out ? spec_out + g * NB : nullptr;
    if (t >= F) {                                                    // (uniform per workgroup) padding: the reference's 0.0
        if (mel_row) for (int c = threadIdx.x; c < n_mel; c += 256) mel_row[c] = 0.f;
        if (spec_row) for (int k = threadIdx.x; k < NB; k += 256) spec_row[k] = 0.f;
        return;
    }
    stft_frame_body(fft_lds, bank + s0, n, (long)t, coef, window, tw, mel_basis, mel_rng, n_fft, hop, win, n_mel, max_abs, ref_db, mel_row,
                    spec_row, nullptr, nullptr, 0.f, 0);
}

}  // namespace mstts
using namespace mstts;

/* bank fp32 = the waveforms back to back, sig_off int64 [n_files + 1], files int32 [N], the tables of mstts_stft_fft, mel_out [N, T, n_mel],
 * spec_out [N, T, n_fft/2+1] (either may be NULL), status int32 [1] (bit 0 is OR-ed in when a row is invalid; the caller zeroes it once) -
 * all on the device */
extern "C" int mstts_stft_bank_batch(const float* bank, const int64_t* sig_off, int64_t n_files, const int32_t* files, int64_t N, int64_t T,
                                     float preemph, const float* window, const float* twiddle, const float* mel_basis, const int32_t* mel_rng,
                                     int32_t n_fft, int32_t hop, int32_t win, int32_t n_mel, float max_abs, float ref_level_db,
                                     float* mel_out, float* spec_out, int32_t* status, mstts_stream_t s) {
    MSTTS_REQUIRE(bank && sig_off && files && window && twiddle && status && (mel_out || spec_out), MSTTS_ERR_SHAPE, "stft_bank_batch: null pointer");
    MSTTS_REQUIRE(!mel_out || (mel_basis && mel_rng && n_mel >= 1), MSTTS_ERR_SHAPE, "stft_bank_batch: mel output needs the filterbank and its ranges");
    MSTTS_REQUIRE(mstts_stft_fft_supported(n_fft, win) && hop >= 1, MSTTS_ERR_SHAPE, "stft_bank_batch: n_fft must be a power of two in [512, 4096]");
    MSTTS_REQUIRE(N >= 1 && T >= 1 && n_files >= 1 && n_files < (1LL << 31), MSTTS_ERR_SHAPE, "stft_bank_batch: need N, T, n_files >= 1");
    MSTTS_REQUIRE(N < (1LL << 31) && T < (1LL << 31) && N * T < (1LL << 31), MSTTS_ERR_SHAPE, "stft_bank_batch: N * T must be below 2^31");
    hipLaunchKernelGGL(stft_bank_batch_kernel, dim3((unsigned)(N * T)), dim3(256), sizeof(float2) * (size_t)n_fft, (hipStream_t)s, bank,
                       (const long*)sig_off, (int)n_files, (const int*)files, (int)T, preemph, window, (const float2*)twiddle, mel_basis,
                       (const int*)mel_rng, (int)n_fft, (int)hop, (int)win, (int)n_mel, max_abs, ref_level_db, mel_out, spec_out, (int*)status);
    MSTTS_CHECK_LAUNCH("stft_bank_batch");
    return MSTTS_OK;
}
