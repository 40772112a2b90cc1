// Audio.melspectrogram on gfx950 (Audio.py:12-13,29-32,42-48,62-96).
// The reference zero-pads an 800-tap Hann window to n_fft = 2048, so each STFT frame touches only
// 800 samples: the windowed DFT is a [frames, 800] x [800, 2*1025] contraction and goes through the
// fp32 MFMA GEMM (overlapping frames are just rows with stride hop), followed by the 1025 -> 80 mel
// filterbank GEMM and a fused dB / normalise pass.
#include "common.h"
#include "stft_frame.h"

namespace mstts {

__global__ void preemph_pad_kernel(const float* __restrict__ x, long n, float coef, int pad, float* __restrict__ out) {
    const long total = n + 2L * pad;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        long j = i - pad;
        if (j < 0) j = -j;                       // np.pad(mode='reflect')
        if (j >= n) j = 2 * (n - 1) - j;
        if (j < 0) j = 0;
        const float prev = j > 0 ? x[j - 1] : 0.f;
        out[i] = x[j] - coef * prev;
    }
}

__global__ void magnitude_kernel(const float* __restrict__ spec, float* __restrict__ mag, long frames, int NB) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < frames * NB; i += (long)gridDim.x * blockDim.x) {
        const long f = i / NB; const int k = (int)(i % NB);
        const float re = spec[f * 2 * NB + k], im = spec[f * 2 * NB + NB + k];
        mag[i] = sqrtf(re * re + im * im);
    }
}

__global__ void db_normalize_kernel(float* __restrict__ mel, long n, float max_abs) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float db = 20.f * log10f(fmaxf(1e-5f, mel[i]));
        const float v = (2.f * max_abs) * ((db + 100.f) / 100.f) - max_abs;
        mel[i] = fminf(fmaxf(v, -max_abs), max_abs);
    }
}

// ---------------------------------------------------------------------------------------------
// The same transform as ONE launch: a workgroup per frame, real FFT in LDS (the frame's arithmetic: stft_frame_body, csrc/stft_frame.h).
// Several waveforms per launch: frame g belongs to waveform w with frame_off[w] <= g < frame_off[w + 1].
// Algorithmic bytes per frame: hop new samples in, n_mel (+ n_fft/2 + 1) floats out; 5 N log2 N flops - the kernel is bound by
// LDS round trips (log4(N/2) stages), a few microseconds per workgroup, 4+ workgroups resident per CU.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stft_fft_kernel(const float* __restrict__ wav, const long* __restrict__ wav_off,
                                                       const long* __restrict__ frame_off, int nw, float coef,
                                                       const float* __restrict__ window, const float2* __restrict__ tw,
                                                       const float* __restrict__ mel_basis, const int* __restrict__ mel_rng, int n_fft, int hop,
                                                       int win, int n_mel, float max_abs, float ref_db, float* __restrict__ mel_out,
                                                       float* __restrict__ spec_out, const float* __restrict__ mag_in,
                                                       const float* __restrict__ sub, float sub_scale, int flags) {
    extern __shared__ __attribute__((aligned(16))) float2 fft_lds[];
    const long g = blockIdx.x;
    int w = 0;
    for (int lo = 0, hi = nw; hi - lo > 1;) {            // = stft_owner (csrc/stft_parts.h), kept as text: any call moves this kernel's code
        const int mid = (lo + hi) >> 1;
        if (frame_off[mid] <= g) lo = mid; else hi = mid;
        w = lo;
    }
    const long f = g - frame_off[w], n = wav_off[w + 1] - wav_off[w];
    const long NB = (n_fft >> 1) + 1;
    stft_frame_body(fft_lds, wav + wav_off[w], n, f, coef, window, tw, mel_basis, mel_rng, n_fft, hop, win, n_mel, max_abs, ref_db,
                    mel_out ? mel_out + g * n_mel : nullptr, spec_out ? spec_out + g * NB : nullptr, mag_in ? mag_in + g * NB : nullptr, sub,
                    sub_scale, flags);
}

}  // namespace mstts
using namespace mstts;

extern "C" int mstts_stft_fft_supported(int32_t n_fft, int32_t win) {
    return n_fft >= 512 && n_fft <= 4096 && (n_fft & (n_fft - 1)) == 0 && win >= 2 && win <= n_fft;
}

extern "C" int mstts_stft_fft(const float* wav, const int64_t* wav_off, const int64_t* frame_off, int32_t nw, float preemph,
                              const float* window, const float* twiddle, const float* mel_basis, const int32_t* mel_rng, int32_t n_fft,
                              int32_t hop, int32_t win, int32_t n_mel, float max_abs, float ref_level_db, float* mel_out, float* spec_out,
                              int64_t total_frames, const float* mag_in, const float* sub, float sub_scale, int32_t flags, mstts_stream_t s) {
    MSTTS_REQUIRE(wav && wav_off && frame_off && window && twiddle && (mel_out || spec_out), MSTTS_ERR_SHAPE, "stft_fft: null pointer");
    MSTTS_REQUIRE(!mel_out || (mel_basis && mel_rng && n_mel >= 1), MSTTS_ERR_SHAPE, "stft_fft: mel output needs the filterbank and its ranges");
    MSTTS_REQUIRE(mstts_stft_fft_supported(n_fft, win) && hop >= 1 && nw >= 1, MSTTS_ERR_SHAPE, "stft_fft: n_fft must be a power of two in [512, 4096]");
    MSTTS_REQUIRE(total_frames >= 0 && total_frames < (1LL << 31), MSTTS_ERR_SHAPE, "stft_fft: frame count");
    if (total_frames == 0) return MSTTS_OK;
    hipLaunchKernelGGL(stft_fft_kernel, dim3((unsigned)total_frames), dim3(256), sizeof(float2) * (size_t)n_fft, (hipStream_t)s, wav,
                       (const long*)wav_off, (const long*)frame_off, (int)nw, preemph, window, (const float2*)twiddle, mel_basis,
                       (const int*)mel_rng, (int)n_fft, (int)hop, (int)win, (int)n_mel, max_abs, ref_level_db, mel_out, spec_out, mag_in, sub, sub_scale, (int)flags);
    MSTTS_CHECK_LAUNCH("stft_fft");
    return MSTTS_OK;
}

static inline long nb_of(int n_fft) { return ((n_fft / 2 + 1) + 3) / 4 * 4; }

extern "C" int64_t mstts_stft_mel_ws_floats(int64_t n, int32_t n_fft, int64_t frames) {
    const long NB = nb_of(n_fft);
    return ((n + n_fft + 3) / 4 * 4) + frames * 2 * NB + frames * NB;
}

extern "C" int mstts_stft_mel(const float* wav, int64_t n, float preemph, const float* dft_basis, const float* mel_basis_t,
                              int32_t n_fft, int32_t hop, int32_t win, int32_t n_mel, float max_abs, float* ws, float* mel_out,
                              int64_t frames, mstts_stream_t s) {
    MSTTS_REQUIRE(wav && dft_basis && mel_basis_t && ws && mel_out, MSTTS_ERR_SHAPE, "stft_mel: null pointer");
    MSTTS_REQUIRE(n >= 2 && frames == 1 + n / hop, MSTTS_ERR_SHAPE, "stft_mel: frames must be 1 + n / hop");
    MSTTS_REQUIRE(win <= n_fft && n > n_fft / 2, MSTTS_ERR_SHAPE, "stft_mel: signal shorter than the reflect pad");
    hipStream_t st = (hipStream_t)s;
    const long NB = nb_of(n_fft);
    const int pad = n_fft / 2;
    float* padded = ws;
    float* spec = ws + ((n + n_fft + 3) / 4 * 4);
    float* mag = spec + frames * 2 * NB;
    long tot = n + 2L * pad;
    hipLaunchKernelGGL(preemph_pad_kernel, dim3((unsigned)((tot + 255) / 256 > 2048 ? 2048 : (tot + 255) / 256)), dim3(256), 0, st,
                       wav, (long)n, preemph, pad, padded);
    MSTTS_CHECK_LAUNCH("preemph_pad");
    // frame f, tap i  ->  padded[f*hop + (n_fft - win)/2 + i]
    mstts_gemm_desc g;
    memset(&g, 0, sizeof(g));
    g.A = padded + (n_fft - win) / 2; g.lda = hop;
    g.B = dft_basis; g.ldb = 2 * NB; g.C = spec; g.ldc = 2 * NB;
    g.M = frames; g.N = 2 * NB; g.K = win; g.alpha = 1.f; g.split_k = 1; g.batch = 1;
    int rc = mstts_gemm_f32(&g, s);
    if (rc) return rc;
    long nm = frames * NB;
    hipLaunchKernelGGL(magnitude_kernel, dim3((unsigned)((nm + 255) / 256 > 2048 ? 2048 : (nm + 255) / 256)), dim3(256), 0, st,
                       (const float*)spec, mag, (long)frames, (int)NB);
    MSTTS_CHECK_LAUNCH("magnitude");
    memset(&g, 0, sizeof(g));
    g.A = mag; g.lda = NB; g.B = mel_basis_t; g.ldb = n_mel; g.C = mel_out; g.ldc = n_mel;
    g.M = frames; g.N = n_mel; g.K = NB; g.alpha = 1.f; g.split_k = 1; g.batch = 1;
    rc = mstts_gemm_f32(&g, s);
    if (rc) return rc;
    long ne = frames * n_mel;
    hipLaunchKernelGGL(db_normalize_kernel, dim3((unsigned)((ne + 255) / 256 > 2048 ? 2048 : (ne + 255) / 256)), dim3(256), 0, st,
                       mel_out, ne, max_abs);
    MSTTS_CHECK_LAUNCH("db_normalize");
    return MSTTS_OK;
}
