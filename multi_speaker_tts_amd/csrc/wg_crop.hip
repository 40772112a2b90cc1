// Training batches of the WaveGlow trainer out of a device-resident bank of waveforms (WaveGlow/Feeder.py:55-105 loads, trims, scales,
// crops, resamples and transforms Batch_Size files per batch on the host).  The bank holds every file's trimmed, peak-scaled waveform at
// Export_Sample_Rate back to back (file f at samples sig_off[f] .. sig_off[f + 1]); a batch is a table of (file, start) pairs and ONE
// launch writes both tensors of the pattern.  For row r, with len = the file's length and c = min(L, len - start):
//   x[i]  = bank[sig_off[file] + start + i]  for 0 <= i < c,   0 elsewhere              audio_out[r, :] = x[0 .. L)
//   y[m]  = sum_{i < taps} phase_table[q mod up][i] x[q div up - (taps - 1) + i],  q = 10 max(up, down) + m down,   m < Lr = ceil(L up / down)
//           (mstts_wav_resample's sum: one fmaf chain over i ascending, out-of-range inputs as 0.f; y = x when up = down = 1)
//   mel_out[r, t, :] = frame t of mstts_stft_fft on y   for t < F = 1 + Lr / hop,   0 for F <= t < T.
// A workgroup per (row, frame).  A frame touches at most win + 1 samples of y (win window positions after the reflection at the ends of
// y, and the pre-emphasis neighbour of the lowest): the workgroup forms exactly those, one thread per sample, straight from the bank - the
// phase rows and the bank come through the caches - and stages them in LDS behind the FFT buffers.  stft_frame_body (csrc/stft_frame.h)
// then reads them through a pointer shifted by the first staged index, so the frame has the bits of mstts_wav_resample followed by
// mstts_stft_fft on a host-made crop.  LDS: 8 n_fft bytes of FFT buffers + 4 (win + 1) bytes of samples (19.6 KB at 2048 / 800).  Samples
// of the bank before `start` or behind the crop are never read.  The row's L audio samples are copied by its T workgroups, ceil(L / T)
// each.  Every element of both outputs is stored exactly once.  A row whose file lies outside [0, n_files), with start < 0 or start >= len
// reads nothing from the bank: it is written as zeros and bit 0 of *status is set.  Pad frames and invalid rows leave before touching LDS.
// spec_out (the frames' [0, 1] spectrogram rows [N, T, n_fft/2+1]) is NULL from the entry point - the WaveGlow pattern has no spectrogram -
// and is a run-time argument on purpose: with the spectrogram store compiled in, the compiler keeps the magnitude loop of stft_frame_body
// in the scalar form it has in stft_fft_kernel and stft_bank_batch_kernel (re^2 + im^2 as one multiply and one fused multiply-add); with
// the store compiled out it packs the two squares into one v_pk_mul_f32 and adds them, and 0.5 % of the mel values differ in the last
// bits (measured).  tests/test_gpu_waveglow_corpus.py pins the bits.
#include "common.h"
#include "stft_frame.h"

namespace mstts {

__global__ __launch_bounds__(256) void wg_crop_batch_kernel(const float* __restrict__ bank, const long* __restrict__ sig_off, int n_files,
                                                            const int* __restrict__ table, int L, int T, int Lr,
                                                            const float* __restrict__ tab, int up, int down, int taps, float coef,
                                                            const float* __restrict__ window, const float2* __restrict__ tw,
                                                            const float* __restrict__ mel_basis, const int* __restrict__ mel_rng, int n_fft,
                                                            int hop, int win, int n_mel, float max_abs, float* __restrict__ audio_out,
                                                            float* __restrict__ mel_out, float* __restrict__ spec_out,
                                                            int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) float2 fft_lds[];
    const int r = blockIdx.x / T, t = blockIdx.x - r * T, tid = threadIdx.x;          // (the host checked N * T < 2^31)
    const int file = table[2 * r], start = table[2 * r + 1];
    long s0 = 0;
    int c = 0;                                                       // samples of the crop that lie in the bank: x[0 .. c)
    bool ok = file >= 0 && file < n_files && start >= 0;
    if (ok) {
        s0 = sig_off[file];
        const long len = sig_off[file + 1] - s0;
        ok = start < len;
        if (ok) {
            c = len - start < L ? (int)(len - start) : L;
            s0 += start;
        }
    }
    if (!ok && t == 0 && tid == 0) atomicOr(status, 1);
    const float* __restrict__ x = bank + s0;
    // this workgroup's share of the row's audio
    {
        const long per = ((long)L + T - 1) / T, a0 = (long)t * per;
        const long a1 = a0 + per < L ? a0 + per : L;
        float* arow = audio_out + (long)r * L;
        for (long i = a0 + tid; i < a1; i += 256) arow[i] = i < c ? x[i] : 0.f;
    }
    const int F = ok ? 1 + Lr / hop : 0;
    float* mel_row = mel_out + (long)blockIdx.x * n_mel;
    float* spec_row = spec_out ? spec_out + (long)blockIdx.x * ((n_fft >> 1) + 1) : nullptr;
    if (t >= F) {                                                    // (uniform per workgroup) padding: the reference's 0.0
        for (int k = tid; k < n_mel; k += 256) mel_row[k] = 0.f;
        if (spec_row) for (int k = tid; k <= n_fft >> 1; k += 256) spec_row[k] = 0.f;
        return;
    }
    // The indices of y this frame reads: window position i reads reflect(t hop + i - n_fft / 2) for off <= i < off + win, and its
    // predecessor.  Reflected indices fold back onto the run next to the end they crossed, so the set is one run [lo, hi].
    const int off = (n_fft - win) >> 1;
    const long a = (long)t * hop + off - (n_fft >> 1), b = a + win - 1;
    long lo = a < 0 ? (b < 0 ? -b : 0) : a;
    if (b >= Lr) {
        long m = 2L * (Lr - 1) - b;
        if (m < 0) m = 0;
        if (m < lo) lo = m;
    }
    lo = lo > 0 ? lo - 1 : 0;
    long hi = b < Lr ? b : Lr - 1;
    if (a < 0 && -a > hi) hi = -a;
    if (hi > Lr - 1) hi = Lr - 1;
    if (hi > lo + win) hi = lo + win;                                // (at most win + 1 samples: the staging area's size)
    float* ys = reinterpret_cast<float*>(fft_lds + n_fft);
    const int count = (int)(hi - lo + 1);
    if (up == 1 && down == 1) {
        for (int s = tid; s < count; s += 256) {
            const long m = lo + s;
            ys[s] = m < c ? x[m] : 0.f;
        }
    } else {
        const long half = 10L * (up > down ? up : down);
        for (int s = tid; s < count; s += 256) {
            const long q = half + (lo + s) * down, jm = q / up;
            const float* __restrict__ row = tab + (q - jm * up) * taps;
            const long j0 = jm - (taps - 1);
            float acc = 0.f;
            for (int i = 0; i < taps; ++i) {
                const long j = j0 + i;
                acc = fmaf(row[i], j >= 0 && j < c ? x[j] : 0.f, acc);
            }
            ys[s] = acc;
        }
    }
    __syncthreads();
    stft_frame_body(fft_lds, ys - lo, (long)Lr, (long)t, coef, window, tw, mel_basis, mel_rng, n_fft, hop, win, n_mel, max_abs, 20.f, mel_row,
                    spec_row, nullptr, nullptr, 0.f, 0);
}

static inline long wg_gcd(long a, long b) {
    while (b) {
        const long r = a % b;
        a = b;
        b = r;
    }
    return a;
}

}  // namespace mstts
using namespace mstts;

// The LDS plan (FFT buffers + the frame's win + 1 resampled samples) fits the 64 KB a workgroup gets by default, the transform is one
// mstts_stft_fft serves and the ratio one mstts_wav_resample serves (whose sum this kernel restates).
extern "C" int mstts_wg_crop_supported(int32_t up, int32_t down, int32_t n_fft, int32_t win) {
    if (!mstts_stft_fft_supported(n_fft, win) || !mstts_wav_resample_supported(up, down)) return 0;
    return sizeof(float2) * (size_t)n_fft + sizeof(float) * ((size_t)win + 1) <= 65536;
}

/* bank, sig_off, the tables of mstts_stft_fft and mstts_wav_resample's phase_table [up][taps] (may be NULL when up = down = 1), table int32
 * [N][2] = (file, start), audio_out [N, L], mel_out [N, T, n_mel], status int32 [1] (bit 0 is OR-ed in when a row is invalid; the caller
 * zeroes it once) - all on the device */
extern "C" int mstts_wg_crop_batch(const float* bank, const int64_t* sig_off, int64_t n_files, const int32_t* table, int64_t N, int64_t L,
                                   int64_t T, const float* phase_table, int32_t up, int32_t down, float preemph, const float* window,
                                   const float* twiddle, const float* mel_basis, const int32_t* mel_rng, int32_t n_fft, int32_t hop,
                                   int32_t win, int32_t n_mel, float max_abs, float* audio_out, float* mel_out, int32_t* status,
                                   mstts_stream_t s) {
    MSTTS_REQUIRE(bank && sig_off && table && window && twiddle && mel_basis && mel_rng && audio_out && mel_out && status, MSTTS_ERR_SHAPE,
                  "wg_crop_batch: null pointer");
    MSTTS_REQUIRE(N >= 1 && L >= 1 && T >= 1 && n_files >= 1 && n_files < (1LL << 31) && L < (1LL << 31), MSTTS_ERR_SHAPE,
                  "wg_crop_batch: need N, L, T, n_files >= 1");
    MSTTS_REQUIRE(N < (1LL << 31) && T < (1LL << 31) && N * T < (1LL << 31), MSTTS_ERR_SHAPE, "wg_crop_batch: N * T must be below 2^31");
    MSTTS_REQUIRE(mstts_stft_fft_supported(n_fft, win) && hop >= 1 && n_mel >= 1, MSTTS_ERR_SHAPE,
                  "wg_crop_batch: n_fft must be a power of two in [512, 4096]");
    MSTTS_REQUIRE(up >= 1 && down >= 1 && wg_gcd(up, down) == 1, MSTTS_ERR_SHAPE, "wg_crop_batch: up = %d, down = %d must be in lowest terms",
                  (int)up, (int)down);
    MSTTS_REQUIRE(mstts_wg_crop_supported(up, down, n_fft, win), MSTTS_ERR_SHAPE, "wg_crop_batch: %d / %d with n_fft = %d, win = %d is not served",
                  (int)up, (int)down, (int)n_fft, (int)win);
    MSTTS_REQUIRE(phase_table || (up == 1 && down == 1), MSTTS_ERR_SHAPE, "wg_crop_batch: null pointer (the phase table)");
    const int64_t Lr = (L * up + down - 1) / down;
    MSTTS_REQUIRE(Lr < (1LL << 31), MSTTS_ERR_SHAPE, "wg_crop_batch: resampled length");
    MSTTS_REQUIRE(Lr > n_fft / 2, MSTTS_ERR_SHAPE, "wg_crop_batch: %lld resampled samples are not longer than the reflect padding (%d)",
                  (long long)Lr, (int)(n_fft / 2));
    MSTTS_REQUIRE(1 + Lr / hop <= T, MSTTS_ERR_SHAPE, "wg_crop_batch: %lld frames do not fit T = %lld", (long long)(1 + Lr / hop), (long long)T);
    const size_t lds = sizeof(float2) * (size_t)n_fft + sizeof(float) * ((size_t)win + 1);
    hipLaunchKernelGGL(wg_crop_batch_kernel, dim3((unsigned)(N * T)), dim3(256), lds, (hipStream_t)s, bank, (const long*)sig_off, (int)n_files,
                       (const int*)table, (int)L, (int)T, (int)Lr, phase_table, (int)up, (int)down, (int)mstts_wav_resample_taps(up, down), preemph,
                       window, (const float2*)twiddle, mel_basis, (const int*)mel_rng, (int)n_fft, (int)hop, (int)win, (int)n_mel, max_abs,
                       audio_out, mel_out, (float*)nullptr, (int*)status);
    MSTTS_CHECK_LAUNCH("wg_crop_batch");
    return MSTTS_OK;
}
