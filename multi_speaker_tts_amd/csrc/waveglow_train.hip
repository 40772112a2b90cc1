// WaveGlow vocoder, training direction (WaveGlow/WaveGlow.py:37-85; WaveGlow/Modules.py:9-34,135-175,210-352,373-385;
// WaveGlow/Inv1x1.py:9-41) - the flow-specific pieces around the contractions.  Every contraction of the step (transposed-conv
// taps and their weight gradient, the dilated K=3 convs in both directions, the 1x1 convs, the conditioning product) runs on
// mstts_gemm_f32; what is left is here, all fp32 with [rows, channels] row-major activations:
//   weight_norm_fwd / _bwd : w = g v rsqrt(max(sum v^2, 1e-5)) per output column for EVERY weight-normed conv of the model in one
//                            launch, driven by a device table of mstts_wg_wn_desc (:9-34), and its gradient
//   coupling_fwd / _bwd    : [a0 | exp(min(log_s, 8)) a1 + b] with the early chunk routed to z, sum min(log_s, 8) into the loss
//                            (:222-238, :329-352, :373-376), and its gradient (tf.minimum passes where log_s <= 8)
//   inv1x1_logdet          : fp64 LU of 1e3 W_f per flow -> log(det + 1e-6) - c log(1e3) into the loss, det/(det+1e-6) W^-T into
//                            the gradient (Inv1x1.py:21-27)
//   gate_bwd / res_skip_bwd: backward of z = tanh(t) sigmoid(s) and of the residual / skip routing (:286-311)
//   overlap_add_bwd        : gather of the transposed-conv tap gradients from the (sliced) upsampled-mel gradient (:135-175,198-208)
//   bias_fold              : the conditioning GEMM's bias, mel_cond_i/bias + audio_in_i/bias, formed on the device every step
//   adam_tf_clip           : TF-Adam with tf.clip_by_global_norm's factor read from a device sum of squares (WaveGlow.py:53-73)
#include "common.h"

namespace mstts {

// ---- weight norm: one workgroup = one descriptor x 64 columns; 4 row groups of 64 lanes (a lane owns one column: coalesced rows)
constexpr int WN_COLS = 64, WN_RG = 4;

__global__ __launch_bounds__(256) void wg_weight_norm_fwd_kernel(const mstts_wg_wn_desc* __restrict__ table) {
    const mstts_wg_wn_desc d = table[blockIdx.y];
    const long col = (long)blockIdx.x * WN_COLS + (threadIdx.x & (WN_COLS - 1));
    const int rg = threadIdx.x / WN_COLS;
    if ((long)blockIdx.x * WN_COLS >= d.cols) return;                  // whole workgroup out of this descriptor's columns
    __shared__ float part[WN_RG][WN_COLS];
    const bool on = col < d.cols;
    float ss = 0.f;
    if (on)
        for (long r = rg; r < d.rows; r += WN_RG) { const float v = d.v[r * d.cols + col]; ss += v * v; }
    part[rg][threadIdx.x & (WN_COLS - 1)] = ss;
    __syncthreads();
    if (!on) return;
    const int c = threadIdx.x & (WN_COLS - 1);
    ss = part[0][c] + part[1][c] + part[2][c] + part[3][c];
    const float scale = d.g[col] * rsqrtf(fmaxf(ss, 1e-5f));
    for (long r = rg; r < d.rows; r += WN_RG) d.w[r * d.ldw + col] = d.v[r * d.cols + col] * scale;
}

__global__ __launch_bounds__(256) void wg_weight_norm_bwd_kernel(const mstts_wg_wn_desc* __restrict__ table) {
    const mstts_wg_wn_desc d = table[blockIdx.y];
    const long col = (long)blockIdx.x * WN_COLS + (threadIdx.x & (WN_COLS - 1));
    const int rg = threadIdx.x / WN_COLS;
    if ((long)blockIdx.x * WN_COLS >= d.cols) return;
    __shared__ float part[2][WN_RG][WN_COLS];
    const bool on = col < d.cols;
    const float* __restrict__ dw = d.w;                                // backward: the effective kernel's gradient, same layout
    float ss = 0.f, dot = 0.f;
    if (on)
        for (long r = rg; r < d.rows; r += WN_RG) {
            const float v = d.v[r * d.cols + col];
            ss += v * v; dot += v * dw[r * d.ldw + col];
        }
    const int c = threadIdx.x & (WN_COLS - 1);
    part[0][rg][c] = ss; part[1][rg][c] = dot;
    __syncthreads();
    if (!on) return;
    ss = part[0][0][c] + part[0][1][c] + part[0][2][c] + part[0][3][c];
    dot = part[1][0][c] + part[1][1][c] + part[1][2][c] + part[1][3][c];
    const float rn = rsqrtf(fmaxf(ss, 1e-5f)), g = d.g[col];
    const float dg = dot * rn;                                          // sum dw * v_hat
    if (rg == 0) d.dg[col] = dg;
    const float a = g * rn, b = ss > 1e-5f ? g * rn * rn * dg : 0.f;    // dv = g r dw - g r^2 dg v  (clamped: g r dw)
    for (long r = rg; r < d.rows; r += WN_RG) d.dv[r * d.cols + col] = a * dw[r * d.ldw + col] - b * d.v[r * d.cols + col];
}

// ---- affine coupling, one thread per row (c <= 16)
__global__ __launch_bounds__(256) void wg_coupling_fwd_kernel(const float* __restrict__ y, const float* __restrict__ lsb, float* __restrict__ next,
                                                              float* __restrict__ z, long ldz, int zcol, int ce, float* __restrict__ loss, long rows, int c) {
    __shared__ float scratch[16];
    const long r = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const int h = c / 2, cn = c - ce;
    float acc = 0.f;
    if (r < rows) {
        float o[16];
        for (int i = 0; i < h; ++i) o[i] = y[r * c + i];
        for (int i = 0; i < h; ++i) {
            const float ls = fminf(lsb[r * c + i], 8.f);
            acc += ls;
            o[h + i] = expf(ls) * y[r * c + h + i] + lsb[r * c + h + i];
        }
        for (int j = 0; j < ce; ++j) z[r * ldz + zcol + j] = o[j];
        for (int j = 0; j < cn; ++j) next[r * cn + j] = o[ce + j];
    }
    acc = block_sum(acc, scratch);
    if (threadIdx.x == 0 && loss) atomicAdd(loss, acc);
}

__global__ __launch_bounds__(256) void wg_coupling_bwd_kernel(const float* __restrict__ y, const float* __restrict__ lsb, const float* __restrict__ z, long ldz,
                                                              int zcol, int ce, const float* __restrict__ d_next, float inv_size,
                                                              float* __restrict__ d_y, float* __restrict__ d_lsb, long rows, int c) {
    const long r = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const int h = c / 2, cn = c - ce;
    float dout[16];
    for (int j = 0; j < ce; ++j) dout[j] = z[r * ldz + zcol + j] * inv_size;       // d Audio_Loss / d z = z / size
    for (int j = 0; j < cn; ++j) dout[ce + j] = d_next[r * cn + j];
    for (int i = 0; i < h; ++i) d_y[r * c + i] = dout[i];                           // a0 passes straight through
    for (int i = 0; i < h; ++i) {
        const float ls_raw = lsb[r * c + i], ls = fminf(ls_raw, 8.f), e = expf(ls), g = dout[h + i];
        d_y[r * c + h + i] = g * e;
        d_lsb[r * c + h + i] = g;                                                   // d b
        d_lsb[r * c + i] = ls_raw <= 8.f ? g * y[r * c + h + i] * e - inv_size : 0.f;   // d log_s (+ Log_S_Loss), zero where clamped
    }
}

// ---- log-determinant of the invertible 1x1 convolutions: one workgroup per flow, lane 0 does the fp64 LU (c <= 16)
__global__ __launch_bounds__(64) void wg_inv1x1_logdet_kernel(const float* __restrict__ params, float* __restrict__ grad, const int64_t* __restrict__ table,
                                                              float grad_scale, float* __restrict__ loss) {
    __shared__ double a[16 * 16], inv[16 * 16];
    __shared__ int perm[16];
    if (threadIdx.x != 0) return;
    const long off = table[2 * blockIdx.x];
    const int c = (int)table[2 * blockIdx.x + 1];
    for (int i = 0; i < c * c; ++i) a[i] = 1e3 * (double)params[off + i];
    for (int i = 0; i < c; ++i) perm[i] = i;
    double det = 1.0;
    for (int k = 0; k < c; ++k) {                                       // LU with partial pivoting, in place
        int p = k;
        for (int i = k + 1; i < c; ++i) if (fabs(a[i * c + k]) > fabs(a[p * c + k])) p = i;
        if (p != k) {
            for (int j = 0; j < c; ++j) { const double t = a[k * c + j]; a[k * c + j] = a[p * c + j]; a[p * c + j] = t; }
            const int t = perm[k]; perm[k] = perm[p]; perm[p] = t;
            det = -det;
        }
        const double piv = a[k * c + k];
        det *= piv;
        for (int i = k + 1; i < c; ++i) {
            const double m = a[i * c + k] / piv;
            a[i * c + k] = m;
            for (int j = k + 1; j < c; ++j) a[i * c + j] -= m * a[k * c + j];
        }
    }
    // inverse of 1e3 W, column by column: L U x = P e_j
    for (int j = 0; j < c; ++j) {
        double x[16];
        for (int i = 0; i < c; ++i) {
            double s = perm[i] == j ? 1.0 : 0.0;
            for (int k = 0; k < i; ++k) s -= a[i * c + k] * x[k];
            x[i] = s;
        }
        for (int i = c - 1; i >= 0; --i) {
            double s = x[i];
            for (int k = i + 1; k < c; ++k) s -= a[i * c + k] * x[k];
            x[i] = s / a[i * c + i];
        }
        for (int i = 0; i < c; ++i) inv[i * c + j] = x[i];
    }
    // loss: (float)log(det + 1e-6) - c log(1e3) (a negative determinant gives NaN, as tf.log does)
    const float ld = (float)log(det + 1e-6) - (float)c * logf(1e3f);
    atomicAdd(loss, ld);
    // gradient: det / (det + 1e-6) * W^-T = det / (det + 1e-6) * 1e3 * inv(1e3 W)^T
    const double f = (double)grad_scale * det / (det + 1e-6) * 1e3;
    for (int i = 0; i < c; ++i)
        for (int j = 0; j < c; ++j) grad[off + i * c + j] += (float)(f * inv[j * c + i]);
}

// ---- gated tanh backward: a = [t | s] pre-activations (row pitch lda), dz [rows, C] -> dpre [rows, 2C] (+ an optional copy at dpre2, pitch ld2)
__device__ __forceinline__ void gate_grad(float t, float s, float g, float& dt, float& ds) {
    const float th = tanhf(t), sg = sigmoid_acc(s);
    dt = g * sg * (1.f - th * th);
    ds = g * th * sg * (1.f - sg);
}
__global__ __launch_bounds__(256) void wg_gate_bwd_kernel(const float* __restrict__ a, long lda, const float* __restrict__ dz, float* __restrict__ dpre,
                                                          float* __restrict__ dpre2, long ld2, long rows, int C) {
    const long n = rows * C;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long r = i / C; const int c = (int)(i - r * C);
        float dt, ds;
        gate_grad(a[r * lda + c], a[r * lda + C + c], dz[i], dt, ds);
        dpre[r * 2 * C + c] = dt; dpre[r * 2 * C + C + c] = ds;
        if (dpre2) { dpre2[r * ld2 + c] = dt; dpre2[r * ld2 + C + c] = ds; }
    }
}
__global__ __launch_bounds__(256) void wg_gate_bwd4_kernel(const float* __restrict__ a, long lda, const float* __restrict__ dz, float* __restrict__ dpre,
                                                           float* __restrict__ dpre2, long ld2, long rows, int C) {
    const int c4n = C >> 2;
    const long n4 = rows * c4n;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const long r = i / c4n; const int c = (int)(i - r * c4n) * 4;
        const float4 t = *reinterpret_cast<const float4*>(a + r * lda + c), s = *reinterpret_cast<const float4*>(a + r * lda + C + c);
        const float4 g = *reinterpret_cast<const float4*>(dz + r * C + c);
        float4 dt, ds;
        gate_grad(t.x, s.x, g.x, dt.x, ds.x); gate_grad(t.y, s.y, g.y, dt.y, ds.y);
        gate_grad(t.z, s.z, g.z, dt.z, ds.z); gate_grad(t.w, s.w, g.w, dt.w, ds.w);
        *reinterpret_cast<float4*>(dpre + r * 2 * C + c) = dt; *reinterpret_cast<float4*>(dpre + r * 2 * C + C + c) = ds;
        if (dpre2) { *reinterpret_cast<float4*>(dpre2 + r * ld2 + c) = dt; *reinterpret_cast<float4*>(dpre2 + r * ld2 + C + c) = ds; }
    }
}

// ---- residual / skip routing backward: !last: drs = [dx_next | dskip], dz = dx_next; last: drs = dskip, dz = 0
__global__ __launch_bounds__(256) void wg_res_skip_bwd_kernel(const float* __restrict__ dxn, const float* __restrict__ dskip, float* __restrict__ drs,
                                                              float* __restrict__ dz, long rows, int C, int last) {
    const long n = rows * C;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long r = i / C; const int c = (int)(i - r * C);
        if (last) { drs[i] = dskip[i]; dz[i] = 0.f; }
        else { const float g = dxn[i]; drs[r * 2 * C + c] = g; drs[r * 2 * C + C + c] = dskip[i]; dz[i] = g; }
    }
}

// ---- transposed-conv tap gradients: dY[n, t, k, c] = d_up[n, t*S + k, c] where t*S + k < L (the slice to the audio length), else 0
__global__ __launch_bounds__(256) void wg_overlap_add_bwd_kernel(const float* __restrict__ dup, float* __restrict__ dY, long N, long T, long K, long S, long C, long L) {
    const long n_el = N * T * K * C;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n_el; i += (long)gridDim.x * blockDim.x) {
        const long c = i % C, k = (i / C) % K, t = (i / (C * K)) % T, n = i / (C * K * T);
        const long l = t * S + k;
        dY[i] = l < L ? dup[(n * L + l) * C + c] : 0.f;
    }
}

// ---- out[b, j] = base[table[2b] + j] + base[table[2b+1] + j]
__global__ __launch_bounds__(256) void wg_bias_fold_kernel(const float* __restrict__ base, const int64_t* __restrict__ table, float* __restrict__ out, long nb, long width) {
    const long n = nb * width;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long b = i / width, j = i - b * width;
        out[i] = base[table[2 * b] + j] + base[table[2 * b + 1] + j];
    }
}

// ---- TF-Adam with the clip_by_global_norm factor from a device sum of squares (gn = sqrt(sumsq_scale * sumsq[0]))
__global__ __launch_bounds__(256) void adam_tf_clip_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                           const float* __restrict__ sumsq, float sumsq_scale, float clip, float lr_t, float b1, float b2,
                                                           float eps, long n) {
    const float gn = sqrtf(sumsq_scale * sumsq[0]);
    const float gs = clip / fmaxf(gn, clip);
    const long n4 = n >> 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        float4 pv = reinterpret_cast<float4*>(p)[i], mv = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
        const float4 gv = reinterpret_cast<const float4*>(g)[i];
        float* pp = &pv.x; float* mp = &mv.x; float* vp = &vv.x; const float* gp = &gv.x;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float gg = gp[q] * gs;
            mp[q] = b1 * mp[q] + (1.f - b1) * gg;
            vp[q] = b2 * vp[q] + (1.f - b2) * gg * gg;
            pp[q] = pp[q] - lr_t * mp[q] / (sqrtf(vp[q]) + eps);
        }
        reinterpret_cast<float4*>(p)[i] = pv; reinterpret_cast<float4*>(m)[i] = mv; reinterpret_cast<float4*>(v)[i] = vv;
    }
    for (long i = n4 * 4 + blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float gg = g[i] * gs;
        const float mv = b1 * m[i] + (1.f - b1) * gg, vv = b2 * v[i] + (1.f - b2) * gg * gg;
        m[i] = mv; v[i] = vv;
        p[i] = p[i] - lr_t * mv / (sqrtf(vv) + eps);
    }
}

}  // namespace mstts
using namespace mstts;
#define ST(s) ((hipStream_t)(s))
static unsigned wgt_grid(long n) { long b = (n + 255) / 256; if (b > 8192) b = 8192; if (b < 1) b = 1; return (unsigned)b; }

extern "C" int mstts_wg_weight_norm_fwd(const mstts_wg_wn_desc* table, int64_t n, int64_t max_cols, mstts_stream_t s) {
    MSTTS_REQUIRE(table && n >= 0 && n <= 65535 && max_cols >= 1, MSTTS_ERR_SHAPE, "wg_weight_norm_fwd: bad arguments");
    if (n == 0) return MSTTS_OK;
    hipLaunchKernelGGL(wg_weight_norm_fwd_kernel, dim3((unsigned)((max_cols + WN_COLS - 1) / WN_COLS), (unsigned)n), dim3(256), 0, ST(s), table);
    MSTTS_CHECK_LAUNCH("wg_weight_norm_fwd");
    return MSTTS_OK;
}
extern "C" int mstts_wg_weight_norm_bwd(const mstts_wg_wn_desc* table, int64_t n, int64_t max_cols, mstts_stream_t s) {
    MSTTS_REQUIRE(table && n >= 0 && n <= 65535 && max_cols >= 1, MSTTS_ERR_SHAPE, "wg_weight_norm_bwd: bad arguments");
    if (n == 0) return MSTTS_OK;
    hipLaunchKernelGGL(wg_weight_norm_bwd_kernel, dim3((unsigned)((max_cols + WN_COLS - 1) / WN_COLS), (unsigned)n), dim3(256), 0, ST(s), table);
    MSTTS_CHECK_LAUNCH("wg_weight_norm_bwd");
    return MSTTS_OK;
}
extern "C" int mstts_wg_coupling_fwd(const float* y, const float* log_s_b, float* next, float* z, int64_t ldz, int64_t z_col, int64_t c_out,
                                     float* loss, int64_t rows, int64_t c, mstts_stream_t s) {
    MSTTS_REQUIRE(y && log_s_b && z && c >= 2 && c <= 16 && c % 2 == 0 && c_out >= 0 && c_out <= c && (c_out == c || next) && z_col >= 0 &&
                  z_col + c_out <= ldz, MSTTS_ERR_SHAPE, "wg_coupling_fwd: 2 <= c <= 16 (even), 0 <= c_out <= c, next when c_out < c");
    if (rows == 0) return MSTTS_OK;
    hipLaunchKernelGGL(wg_coupling_fwd_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, ST(s), y, log_s_b, next, z, (long)ldz, (int)z_col,
                       (int)c_out, loss, (long)rows, (int)c);
    MSTTS_CHECK_LAUNCH("wg_coupling_fwd");
    return MSTTS_OK;
}
extern "C" int mstts_wg_coupling_bwd(const float* y, const float* log_s_b, const float* z, int64_t ldz, int64_t z_col, int64_t c_out, const float* d_next,
                                     float inv_size, float* d_y, float* d_log_s_b, int64_t rows, int64_t c, mstts_stream_t s) {
    MSTTS_REQUIRE(y && log_s_b && z && d_y && d_log_s_b && c >= 2 && c <= 16 && c % 2 == 0 && c_out >= 0 && c_out <= c && (c_out == c || d_next) &&
                  z_col >= 0 && z_col + c_out <= ldz, MSTTS_ERR_SHAPE, "wg_coupling_bwd: 2 <= c <= 16 (even), 0 <= c_out <= c, d_next when c_out < c");
    if (rows == 0) return MSTTS_OK;
    hipLaunchKernelGGL(wg_coupling_bwd_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, ST(s), y, log_s_b, z, (long)ldz, (int)z_col, (int)c_out,
                       d_next, inv_size, d_y, d_log_s_b, (long)rows, (int)c);
    MSTTS_CHECK_LAUNCH("wg_coupling_bwd");
    return MSTTS_OK;
}
extern "C" int mstts_wg_inv1x1_logdet(const float* params, float* grad, const int64_t* table, int64_t n_flows, float grad_scale, float* loss, mstts_stream_t s) {
    MSTTS_REQUIRE(params && grad && table && loss && n_flows >= 0, MSTTS_ERR_SHAPE, "wg_inv1x1_logdet: bad arguments");
    if (n_flows == 0) return MSTTS_OK;
    hipLaunchKernelGGL(wg_inv1x1_logdet_kernel, dim3((unsigned)n_flows), dim3(64), 0, ST(s), params, grad, table, grad_scale, loss);
    MSTTS_CHECK_LAUNCH("wg_inv1x1_logdet");
    return MSTTS_OK;
}
extern "C" int mstts_wg_gate_bwd(const float* a, int64_t lda, const float* dz, float* dpre, float* dpre2, int64_t ld2, int64_t rows, int64_t C, mstts_stream_t s) {
    MSTTS_REQUIRE(a && dz && dpre && rows >= 0 && C >= 1 && lda >= 2 * C && (!dpre2 || ld2 >= 2 * C), MSTTS_ERR_SHAPE, "wg_gate_bwd: bad arguments");
    if (rows == 0) return MSTTS_OK;
    const bool v4 = C % 4 == 0 && lda % 4 == 0 && (!dpre2 || ld2 % 4 == 0) && aligned16(a) && aligned16(dz) && aligned16(dpre) && (!dpre2 || aligned16(dpre2));
    if (v4) hipLaunchKernelGGL(wg_gate_bwd4_kernel, dim3(wgt_grid(rows * C / 4)), dim3(256), 0, ST(s), a, (long)lda, dz, dpre, dpre2, (long)ld2, (long)rows, (int)C);
    else hipLaunchKernelGGL(wg_gate_bwd_kernel, dim3(wgt_grid(rows * C)), dim3(256), 0, ST(s), a, (long)lda, dz, dpre, dpre2, (long)ld2, (long)rows, (int)C);
    MSTTS_CHECK_LAUNCH("wg_gate_bwd");
    return MSTTS_OK;
}
extern "C" int mstts_wg_res_skip_bwd(const float* d_x_next, const float* d_skip, float* d_rs, float* d_z, int64_t rows, int64_t C, int32_t last, mstts_stream_t s) {
    MSTTS_REQUIRE(d_skip && d_rs && d_z && (last || d_x_next) && rows >= 0 && C >= 1, MSTTS_ERR_SHAPE, "wg_res_skip_bwd: bad arguments");
    if (rows == 0) return MSTTS_OK;
    hipLaunchKernelGGL(wg_res_skip_bwd_kernel, dim3(wgt_grid(rows * C)), dim3(256), 0, ST(s), d_x_next, d_skip, d_rs, d_z, (long)rows, (int)C, (int)last);
    MSTTS_CHECK_LAUNCH("wg_res_skip_bwd");
    return MSTTS_OK;
}
extern "C" int mstts_wg_overlap_add_bwd(const float* d_up, float* dY, int64_t N, int64_t T, int64_t K, int64_t S, int64_t C, int64_t L, mstts_stream_t s) {
    MSTTS_REQUIRE(d_up && dY && N >= 1 && T >= 1 && K >= 1 && S >= 1 && C >= 1 && L >= 1 && L <= (T - 1) * S + K, MSTTS_ERR_SHAPE,
                  "wg_overlap_add_bwd: bad arguments (L must not exceed the upsampled length)");
    hipLaunchKernelGGL(wg_overlap_add_bwd_kernel, dim3(wgt_grid(N * T * K * C)), dim3(256), 0, ST(s), d_up, dY, (long)N, (long)T, (long)K, (long)S, (long)C, (long)L);
    MSTTS_CHECK_LAUNCH("wg_overlap_add_bwd");
    return MSTTS_OK;
}
extern "C" int mstts_wg_bias_fold(const float* base, const int64_t* table, float* out, int64_t n_blocks, int64_t width, mstts_stream_t s) {
    MSTTS_REQUIRE(base && table && out && n_blocks >= 0 && width >= 1, MSTTS_ERR_SHAPE, "wg_bias_fold: bad arguments");
    if (n_blocks == 0) return MSTTS_OK;
    hipLaunchKernelGGL(wg_bias_fold_kernel, dim3(wgt_grid(n_blocks * width)), dim3(256), 0, ST(s), base, table, out, (long)n_blocks, (long)width);
    MSTTS_CHECK_LAUNCH("wg_bias_fold");
    return MSTTS_OK;
}
extern "C" int mstts_adam_tf_clip(float* p, const float* grad, float* m, float* v, const float* sumsq, float sumsq_scale, float clip_norm,
                                  float lr_t, float beta1, float beta2, float eps, int64_t n, mstts_stream_t s) {
    MSTTS_REQUIRE(p && grad && m && v && sumsq && n >= 0 && clip_norm > 0.f, MSTTS_ERR_SHAPE, "adam_tf_clip: bad arguments");
    MSTTS_REQUIRE(aligned16(p) && aligned16(grad) && aligned16(m) && aligned16(v), MSTTS_ERR_ALIGN, "adam_tf_clip: 16-byte aligned slabs required");
    if (n == 0) return MSTTS_OK;
    hipLaunchKernelGGL(adam_tf_clip_kernel, dim3(wgt_grid((n + 3) / 4)), dim3(256), 0, ST(s), p, grad, m, v, sumsq, sumsq_scale, clip_norm, lr_t, beta1, beta2, eps, (long)n);
    MSTTS_CHECK_LAUNCH("adam_tf_clip");
    return MSTTS_OK;
}
