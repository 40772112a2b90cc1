// Native time-loop drivers: they enqueue the dependent per-step kernels of the recurrent parts of
// the graph on one HIP stream (no host round trips, capturable into a hipGraph by the caller).
//   mstts_lstm_seq_fwd/bwd        - tf.nn.dynamic_rnn over a ZoneoutLSTMCell (encoder BiLSTM, Taco1
//                                   BiRNN, speaker encoder)          [Modules.py:49-73]
//   mstts_decoder_train_fwd/bwd   - the teacher-forced attention decoder loop and its BPTT
//                                   [Modules.py:76-119,323-472 + TF AttentionWrapper]
//   mstts_decoder_infer_steps     - the free-running loop            [Modules.py:212-237]
//
// A step is the same chain in every driver - cell product, cell update, (query, attention, projection) - and each link has tiers,
// chosen per call from the optional derived copies in the descriptor and the *_supported predicates:
//   cell, forward     fused cell (mstts_cell_fwd: product + update in one launch): packed kernel and packed activation block
//                     given (w0p / w1p / act_p, wh_p / h_p, w0sp; bf16: w0p16 / w1p16) and mstts_cell_fwd[_bf16]_supported;
//                     else recurrent_fwd + mstts_lstm_point_fwd.
//   recurrent_fwd     bf16 packed product (all six bf_* copies given and mstts_decoder_bf16_splits) > skinny K-split product
//                     (mstts_skinny_fwd_splits > 0, float4-aligned operands) > tiled GEMM.
//   attention         fused query (mstts_lsa_step_fwd_q: mstts_lsa_step_q_supported, lsa.loc_kt, A == 128, granule workspace large
//                     enough) > query product + mstts_lsa_step_fwd.  Free-running loop only, on top of the fused query and the fused
//                     cells: fused query + projection (mstts_lsa_step_fwd_qp: wp_own, vp, mstts_lsa_step_qp_supported), and with it
//                     the next step's prenet (mstts_lsa_step_prenet_supported); else project_step (skinny product + proj_finish).
//   attention, BPTT   single launch (mstts_lsa_step_bwd) when H + M and H are multiples of 4, else d_align + d_energy launches.
//   recurrent_bwd     bf16 packed product > packed fp32 product (w0f_bp / w1_bp / wq_bp given, R % 32 == 0) > skinny N-split
//                     product (mstts_skinny_bwd_splits > 0) > tiled GEMM.
//   query gradient    folded into cell 1's pointwise backward (wq_t given, A == 128, H % 128 == 0, 1 / 2 / 4 / 8 slabs), else a
//                     recurrent_bwd of its own.
#include "common.h"
#include "prenet_body.h"

using namespace mstts;

#define RC(call) do { int rc__ = (call); if (rc__ != MSTTS_OK) return rc__; } while (0)

// ---------------------------------------------------------------------------------------------
// Profiling probes (bench.py only): HIP events bracketing every launch of one selected kernel kind
// inside the loop drivers, on the stream the kernel is launched on.  Process-global and not
// thread-safe by design - never armed on the product path.
// ---------------------------------------------------------------------------------------------
#include <vector>
namespace {
struct Probe {
    int kind = 0;
    std::vector<hipEvent_t> ev;
    size_t used = 0;
} g_probe;
inline bool probe_on(int kind) { return g_probe.kind == kind && g_probe.used + 3 <= g_probe.ev.size(); }
inline void probe_mark(mstts_stream_t s) { hipEventRecord(g_probe.ev[g_probe.used++], (hipStream_t)s); }
}  // namespace
// three events per launch: e0 | launch | e1 | e2 - (e1 - e0) is the bracketed launch, (e2 - e1) an empty bracket on the same stream
// in the same place, i.e. what the event pair itself costs
#define PROBED(kind, s, call) do { const bool pr__ = probe_on(kind); if (pr__) probe_mark(s); RC(call); if (pr__) { probe_mark(s); probe_mark(s); } } while (0)

extern "C" int mstts_probe_begin(int32_t kind, int64_t max_launches) {
    for (hipEvent_t e : g_probe.ev) hipEventDestroy(e);
    g_probe.ev.clear();
    g_probe.used = 0;
    g_probe.kind = kind;
    if (kind == 0) return MSTTS_OK;
    g_probe.ev.resize((size_t)max_launches * 3);
    for (auto& e : g_probe.ev)
        if (hipEventCreate(&e) != hipSuccess) return set_err(MSTTS_ERR_LAUNCH, "probe: hipEventCreate failed");
    return MSTTS_OK;
}
/* after a stream synchronise: number of bracketed launches and their summed duration (ms) */
extern "C" int64_t mstts_probe_result(double* total_ms, double* empty_total_ms) {
    double tot = 0.0, emp = 0.0;
    for (size_t i = 0; i + 2 < g_probe.used; i += 3) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, g_probe.ev[i], g_probe.ev[i + 1]) == hipSuccess) tot += ms;
        if (hipEventElapsedTime(&ms, g_probe.ev[i + 1], g_probe.ev[i + 2]) == hipSuccess) emp += ms;
    }
    if (total_ms) *total_ms = tot;
    if (empty_total_ms) *empty_total_ms = emp;
    return (int64_t)(g_probe.used / 3);
}

static int gemm(const float* A, long lda, const float* B, long ldb, int trans_b, float* C, long ldc, long M, long N, long K,
                const float* bias, int act, int accumulate, mstts_stream_t s) {
    mstts_gemm_desc g;
    memset(&g, 0, sizeof(g));
    g.A = A; g.B = B; g.C = C; g.bias = bias;
    g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc;
    g.trans_a = 0; g.trans_b = trans_b; g.act = act; g.accumulate = accumulate; g.split_k = 1; g.batch = 1; g.alpha = 1.f;
    return mstts_gemm_f32(&g, s);
}

static int zero(float* p, long n, mstts_stream_t s) {
    hipError_t e = hipMemsetAsync(p, 0, n * sizeof(float), (hipStream_t)s);
    if (e != hipSuccess) return set_err(MSTTS_ERR_LAUNCH, "memset: %s", hipGetErrorString(e));
    return MSTTS_OK;
}

// ---------------------------------------------------------------------------------------------
// One cell's per-step slots.  State slot k of c sits at c + k * B * H, of h at h + k * h_step (rows of stride h_ld: the decoder keeps
// h inside the next product's input rows); the masks and the BPTT saves of step st at st * B * H (acts: 4 * B * H), NULL = none.
// ---------------------------------------------------------------------------------------------
struct CellSlots {
    long B, H;
    float* c;
    float* h; long h_ld, h_step;
    const uint8_t* zc; const uint8_t* zh; float zoneout;
    float* acts; float* c_raw;
};
// what the BPTT reads of them
struct CellSaved {
    long B, H;
    const float* c;
    const uint8_t* zc; const uint8_t* zh; float zoneout;
    const float* acts; const float* c_raw;
};
static CellSaved saved(const CellSlots& k) { return CellSaved{k.B, k.H, k.c, k.zc, k.zh, k.zoneout, k.acts, k.c_raw}; }
#define SLOT(ptr, n) ((ptr) ? (ptr) + (n) : nullptr)

// pointwise cell update of step st: state slot rd -> slot wr, gates = sum of `parts` slabs; the caller adds xw / bias / out (and the sequence fields)
static void fill_point_fwd(mstts_lstm_point_fwd_desc* p, const CellSlots& k, long st, long rd, long wr, const float* gates, int parts) {
    const long BH = k.B * k.H;
    memset(p, 0, sizeof(*p));
    p->B = k.B; p->H = k.H; p->gates_h = gates; p->gates_parts = parts; p->gates_pstride = 4 * BH;
    p->c_prev = k.c + rd * BH; p->h_prev = k.h + rd * k.h_step; p->h_prev_ld = k.h_ld;
    p->zc = SLOT(k.zc, st * BH); p->zh = SLOT(k.zh, st * BH); p->zoneout = k.zoneout;
    p->c_next = k.c + wr * BH; p->h_next = k.h + wr * k.h_step; p->h_next_ld = k.h_ld;
    p->acts_out = SLOT(k.acts, st * 4 * BH); p->c_raw = SLOT(k.c_raw, st * BH);
}
// the same slots of a fused cell step (product + cell update, cell.hip); the caller adds the operands, xw / bias / out and the packed destinations
static void fill_cell_fwd(mstts_cell_fwd_desc* q, const CellSlots& k, long st, long rd, long wr) {
    const long BH = k.B * k.H;
    memset(q, 0, sizeof(*q));
    q->B = k.B; q->H = k.H;
    q->c_prev = k.c + rd * BH; q->h_prev = k.h + rd * k.h_step; q->h_prev_ld = k.h_ld;
    q->zc = SLOT(k.zc, st * BH); q->zh = SLOT(k.zh, st * BH); q->zoneout = k.zoneout;
    q->c_next = k.c + wr * BH; q->h_next = k.h + wr * k.h_step; q->h_next_ld = k.h_ld;
    q->acts = SLOT(k.acts, st * 4 * BH); q->c_raw = SLOT(k.c_raw, st * BH);
}
// pointwise backward of step st: ds = the cell's state gradients [d_c 2][d_h 2][B][H], ping-pong (read `cur`, write the other); the
// caller adds the output-gradient addends
static void fill_point_bwd(mstts_lstm_point_bwd_desc* p, const CellSaved& k, long st, float* ds, int cur, float* dgates) {
    const long BH = k.B * k.H;
    memset(p, 0, sizeof(*p));
    p->B = k.B; p->H = k.H;
    p->d_c_state = ds + cur * BH; p->d_h_state = ds + (2 + cur) * BH; p->d_c_prev = ds + (cur ^ 1) * BH; p->d_h_prev = ds + (2 + (cur ^ 1)) * BH;
    p->acts = k.acts + st * 4 * BH; p->c_raw = k.c_raw + st * BH; p->c_prev = k.c + st * BH;
    p->zc = SLOT(k.zc, st * BH); p->zh = SLOT(k.zh, st * BH); p->zoneout = k.zoneout;
    p->dgates = dgates;
}

static mstts_cell_packed_dst packed(float* base, long K, long col0, int bf16) {
    mstts_cell_packed_dst o = {base, K, col0, bf16};
    return o;
}
// one fused cell step; out_p / hn_p: packed blocks of the cells that consume m / h' next
static int cell_step(const CellSlots& k, long st, long rd, long wr, const float* Xp, const float* Wp, long K, const float* xw, const float* bias,
                     float* out, long out_ld, mstts_cell_packed_dst out_p, mstts_cell_packed_dst hn_p, int bf16, mstts_stream_t s) {
    mstts_cell_fwd_desc q;
    fill_cell_fwd(&q, k, st, rd, wr);
    q.bf16 = bf16; q.K = K; q.Xp = Xp; q.Wp = Wp; q.xw = xw; q.xw_ld = xw ? 4 * k.H : 0; q.bias = bias;
    q.out = out; q.out_ld = out_ld; q.out_p = out_p; q.h_next_p = hn_p;
    return mstts_cell_fwd(&q, s);
}

// One kernel of a recurrent product: row-major [rows, cols] (row stride ld), its split count for the direction it is used in (0: the
// tiled GEMM) and its optional derived copies
struct Weights {
    const float* W; long ld, rows, cols; int splits;
    const float* Wp;                    // data-gradient product only: fp32 copy packed for exactly `splits` slices, or NULL
    const void* Wbf; int bsplit;        // bf16 copy packed for `bsplit` slices, or NULL (fp32 products)
};
// X[M,rows] . W -> *parts slabs [M,cols] in P: the bf16 packed product, else the skinny K-split kernel when the shape fits, else the tiled GEMM
static int recurrent_fwd(const Weights& w, const float* X, long ldx, float* P, long M, int* parts, mstts_stream_t s) {
    if (w.Wbf) {
        *parts = w.bsplit;
        return mstts_skinny_fwd_bf16(X, ldx, w.Wbf, P, 0, M, w.cols, w.rows, w.bsplit, s);
    }
    if (w.splits > 0 && ldx % 4 == 0 && w.ld % 4 == 0 && aligned16(X) && aligned16(w.W)) {
        *parts = w.splits;
        return mstts_skinny_fwd(X, ldx, w.W, w.ld, P, 0, M, w.cols, w.rows, w.splits, s);
    }
    *parts = 1;
    return gemm(X, ldx, w.W, w.ld, 0, P, w.cols, M, w.cols, w.rows, nullptr, 0, 0, s);
}
// dG[M,cols] . W^T -> *parts slabs [M,rows] in P (stride pstride, 0 = M * rows): the bf16 packed product, else the packed fp32 product,
// else the skinny N-split kernel, else the tiled GEMM
static int recurrent_bwd(const Weights& w, const float* dG, long ldg, float* P, long pstride, long M, int* parts, mstts_stream_t s) {
    if (w.Wbf) {
        *parts = w.bsplit;
        return mstts_skinny_bwd_bf16(dG, ldg, w.Wbf, P, pstride, M, w.rows, w.cols, w.bsplit, s);
    }
    if (w.Wp && w.splits > 0 && w.rows % 32 == 0 && ldg % 4 == 0 && aligned16(dG) && aligned16(w.Wp)) {
        *parts = w.splits;
        return mstts_skinny_bwd_packed(dG, ldg, w.Wp, P, pstride, M, w.rows, w.cols, w.splits, s);
    }
    if (w.splits > 0 && ldg % 4 == 0 && w.ld % 4 == 0 && aligned16(dG) && aligned16(w.W)) {
        *parts = w.splits;
        return mstts_skinny_bwd(dG, ldg, w.W, w.ld, P, pstride, M, w.rows, w.cols, w.splits, s);
    }
    *parts = 1;
    return gemm(dG, ldg, w.W, w.ld, 1, P, w.rows, M, w.rows, w.cols, nullptr, 0, 0, s);
}

// ---- bf16 recurrent products (BASELINE config 3): split counts capped by the fp32 path's, so every workspace / slab count the
// caller sized for fp32 also holds the bf16 path; the counts are baked into the packed kernels, hence exported.
/* out = {fwd cell0, fwd cell1, fwd query, bwd cell0, bwd cell1, bwd query}; returns 1 when the bf16 decoder path can run */
extern "C" int32_t mstts_decoder_bf16_splits(int64_t H, int64_t M, int64_t A, int32_t* out) {
    const long W0 = M + H, W1 = 2 * H;
    const int c0 = mstts_skinny_fwd_splits(4 * H, W0), c1 = mstts_skinny_fwd_splits(4 * H, W1), cq = mstts_skinny_fwd_splits(A, H);
    const int d0 = mstts_skinny_bwd_splits(W0, 4 * H), d1 = mstts_skinny_bwd_splits(W1, 4 * H), dq = mstts_skinny_bwd_splits(H, A);
    int v[6] = {skinny_bf16_fwd_split(4 * H, W0, c0), skinny_bf16_fwd_split(4 * H, W1, c1), skinny_bf16_fwd_split(A, H, cq),
                d0 > 0 ? skinny_bf16_bwd_split(W0, 4 * H, d0) : 0, skinny_bf16_bwd_split(W1, 4 * H, d1), skinny_bf16_bwd_split(H, A, dq > 1 ? dq : 1)};
    // the d_in0 slabs are counted by the caller (mstts_decoder_train_bwd_parts): the bf16 product must write exactly as many
    if (v[3] != d0) v[3] = (d0 > 0 && (4 * H) % (64L * d0) == 0 && 4 * H / d0 <= 1024 && W0 % 32 == 0) ? d0 : 0;
    int ok = 1;
    for (int i = 0; i < 6; ++i) { if (out) out[i] = v[i]; if (v[i] < 1) ok = 0; }
    return ok;
}

// ---------------------------------------------------------------------------------------------
// sequence loops (tf.nn.dynamic_rnn)
// ---------------------------------------------------------------------------------------------
extern "C" int64_t mstts_lstm_seq_ws_floats(int64_t B, int64_t H, int32_t backward) {
    int p = backward ? mstts_skinny_bwd_splits(H, 4 * H) : mstts_skinny_fwd_splits(4 * H, H);
    if (p < 1) p = 1;
    return backward ? 4 * B * H + (int64_t)p * B * H : (int64_t)p * B * 4 * H;
}

static CellSlots seq_slots(const mstts_lstm_seq_fwd_desc* d) {
    return CellSlots{d->B, d->H, d->c_hist, d->h_hist, d->H, d->B * d->H, d->zc, d->zh, d->zoneout, d->acts, d->c_raw};
}
// ---- fused sequence steps: one mstts_cell_fwd launch per step (recurrent product + cell update), h carried in packed blocks
static bool seq_fused_ok(const mstts_lstm_seq_fwd_desc* d) {
    return d->wh_p && d->h_p && !d->residual && mstts_cell_fwd_supported(d->H, d->H);
}
static void seq_cell_desc(const mstts_lstm_seq_fwd_desc* d, long t, mstts_cell_fwd_desc* q) {
    const long T = d->T, H = d->H, blk = mstts_cell_act_floats(d->B, H);
    fill_cell_fwd(q, seq_slots(d), t, t, t + 1);
    q->K = H; q->Xp = d->h_p + (t & 1) * blk; q->Wp = d->wh_p;
    q->xw = d->xw; q->xw_ld = T * 4 * H; q->xw_st = 4 * H;
    q->out = d->out; q->out_ld = d->out_sb; q->out_st = d->out_st;
    q->h_next_p = packed(d->h_p + ((t + 1) & 1) * blk, H, 0, 0);
    q->lengths = d->lengths; q->step = (int)t; q->reverse = d->reverse;
}
static int seq_fused_begin(const mstts_lstm_seq_fwd_desc* d, mstts_stream_t s) {
    MSTTS_REQUIRE(d->xw && d->c_hist && d->h_hist && d->out, MSTTS_ERR_SHAPE, "lstm_seq_fwd: null pointer");
    MSTTS_REQUIRE(!(d->reverse && !d->lengths), MSTTS_ERR_SHAPE, "lstm_seq_fwd: reverse needs a lengths array (pass T for every row)");
    RC(zero(d->c_hist, d->B * d->H, s));
    RC(zero(d->h_hist, d->B * d->H, s));
    return zero(d->h_p, 2 * mstts_cell_act_floats(d->B, d->H), s);
}

extern "C" int mstts_lstm_seq_fwd(const mstts_lstm_seq_fwd_desc* d, mstts_stream_t s) {
    MSTTS_REQUIRE(d && d->xw && d->wh && d->c_hist && d->h_hist && d->gates_ws, MSTTS_ERR_SHAPE, "lstm_seq_fwd: null pointer");
    MSTTS_REQUIRE(!(d->reverse && !d->lengths), MSTTS_ERR_SHAPE, "lstm_seq_fwd: reverse needs a lengths array (pass T for every row)");
    const long B = d->B, T = d->T, H = d->H, BH = B * H;
    if (seq_fused_ok(d)) {
        RC(seq_fused_begin(d, s));
        for (long t = 0; t < T; ++t) {
            mstts_cell_fwd_desc q;
            seq_cell_desc(d, t, &q);
            RC(mstts_cell_fwd(&q, s));
        }
        return MSTTS_OK;
    }
    const Weights wh = {d->wh, d->wh_ld, H, 4 * H, mstts_skinny_fwd_splits(4 * H, H), nullptr, nullptr, 0};
    const CellSlots k = seq_slots(d);
    RC(zero(d->c_hist, BH, s));
    RC(zero(d->h_hist, BH, s));
    for (long t = 0; t < T; ++t) {
        int parts = 1;
        RC(recurrent_fwd(wh, d->h_hist + t * BH, H, d->gates_ws, B, &parts, s));
        mstts_lstm_point_fwd_desc p;
        fill_point_fwd(&p, k, t, t, t + 1, d->gates_ws, parts);
        p.xw = d->xw; p.xw_sb = T * 4 * H; p.xw_st = 4 * H;
        p.lengths = d->lengths; p.step = (int)t; p.reverse = d->reverse;
        p.residual = d->residual; p.res_sb = T * H; p.res_st = H;
        p.out = d->out; p.out_sb = d->out_sb; p.out_st = d->out_st;
        RC(mstts_lstm_point_fwd(&p, s));
    }
    return MSTTS_OK;
}

extern "C" int mstts_lstm_seq_fwd_pair(const mstts_lstm_seq_fwd_desc* a, const mstts_lstm_seq_fwd_desc* b, mstts_stream_t s) {
    MSTTS_REQUIRE(a && b, MSTTS_ERR_SHAPE, "lstm_seq_fwd_pair: null descriptor");
    if (!(a->B == b->B && a->T == b->T && a->H == b->H && seq_fused_ok(a) && seq_fused_ok(b))) {
        RC(mstts_lstm_seq_fwd(a, s));
        return mstts_lstm_seq_fwd(b, s);
    }
    RC(seq_fused_begin(a, s));
    RC(seq_fused_begin(b, s));
    for (long t = 0; t < a->T; ++t) {
        mstts_cell_fwd_desc qa, qb;
        seq_cell_desc(a, t, &qa);
        seq_cell_desc(b, t, &qb);
        RC(mstts_cell_fwd_pair(&qa, &qb, s));
    }
    return MSTTS_OK;
}

// BPTT step t of a sequence.  ws = [d_c 2][d_h 2][B][H] ping-pong, then dgates . Wh^T of the later step in `parts` slabs [parts][B][H]
static void seq_point_bwd_desc(const mstts_lstm_seq_bwd_desc* d, long t, int cur, int parts, mstts_lstm_point_bwd_desc* p) {
    const long B = d->B, T = d->T, H = d->H, BH = B * H;
    const CellSaved k = {B, H, d->c_hist, d->zc, d->zh, d->zoneout, d->acts, d->c_raw};
    fill_point_bwd(p, k, t, d->ws, cur, d->dgates_step + t * 4 * BH);
    p->d_out = d->d_out; p->dout_sb = d->dout_sb; p->dout_st = d->dout_st;
    p->d_h_state2 = (t == T - 1) ? nullptr : d->ws + 4 * BH; p->dhs2_ld = H; p->dhs2_parts = parts; p->dhs2_pstride = BH;
    p->lengths = d->lengths; p->step = (int)t; p->reverse = d->reverse;
    p->dgates_pos = d->dgates_pos; p->dgp_sb = T * 4 * H; p->dgp_st = 4 * H;
}

extern "C" int mstts_lstm_seq_bwd(const mstts_lstm_seq_bwd_desc* d, mstts_stream_t s) {
    MSTTS_REQUIRE(d && d->wh && d->d_out && d->c_hist && d->acts && d->c_raw && d->dgates_step && d->ws, MSTTS_ERR_SHAPE,
                  "lstm_seq_bwd: null pointer");
    MSTTS_REQUIRE(!(d->reverse && !d->lengths), MSTTS_ERR_SHAPE, "lstm_seq_bwd: reverse needs a lengths array");
    const long B = d->B, T = d->T, H = d->H, BH = B * H;
    const Weights wh = {d->wh, d->wh_ld, H, 4 * H, mstts_skinny_bwd_splits(H, 4 * H), nullptr, nullptr, 0};
    RC(zero(d->ws, 4 * BH, s));
    int cur = 0, parts = 1;
    for (long t = T - 1; t >= 0; --t, cur ^= 1) {
        mstts_lstm_point_bwd_desc p;
        seq_point_bwd_desc(d, t, cur, parts, &p);
        RC(mstts_lstm_point_bwd(&p, s));
        // recurrent part of d_h_prev = dgates . Wh^T (slabs, consumed by the next iteration)
        RC(recurrent_bwd(wh, p.dgates, 4 * H, d->ws + 4 * BH, 0, B, &parts, s));
    }
    return MSTTS_OK;
}

extern "C" int mstts_lstm_seq_bwd_pair(const mstts_lstm_seq_bwd_desc* a, const mstts_lstm_seq_bwd_desc* b, mstts_stream_t s) {
    MSTTS_REQUIRE(a && b, MSTTS_ERR_SHAPE, "lstm_seq_bwd_pair: null descriptor");
    const long B = a->B, T = a->T, H = a->H, BH = B * H;
    const int sp = mstts_skinny_bwd_splits(H, 4 * H);
    const bool pair_ok = a->B == b->B && a->T == b->T && a->H == b->H && sp > 0 && a->wh_ld == b->wh_ld && a->wh_ld % 4 == 0 && aligned16(a->wh) &&
                         aligned16(b->wh) && (sp == 1 || sp == 2 || sp == 4 || sp == 8) && a->dgates_step && b->dgates_step;
    if (!pair_ok) {
        RC(mstts_lstm_seq_bwd(a, s));
        return mstts_lstm_seq_bwd(b, s);
    }
    for (const mstts_lstm_seq_bwd_desc* d : {a, b}) {
        MSTTS_REQUIRE(d->wh && d->d_out && d->c_hist && d->acts && d->c_raw && d->ws, MSTTS_ERR_SHAPE, "lstm_seq_bwd_pair: null pointer");
        MSTTS_REQUIRE(!(d->reverse && !d->lengths), MSTTS_ERR_SHAPE, "lstm_seq_bwd_pair: reverse needs a lengths array");
        RC(zero(d->ws, 4 * BH, s));
    }
    int cur = 0;
    for (long t = T - 1; t >= 0; --t, cur ^= 1) {
        mstts_lstm_point_bwd_desc pa, pb;
        seq_point_bwd_desc(a, t, cur, sp, &pa);
        seq_point_bwd_desc(b, t, cur, sp, &pb);
        RC(mstts_lstm_point_bwd_pair(&pa, &pb, s));
        RC(mstts_skinny_bwd_pair(pa.dgates, pb.dgates, 4 * H, a->wh, b->wh, a->wh_ld, a->ws + 4 * BH, b->ws + 4 * BH, 0, B, H, 4 * H, sp, s));
    }
    return MSTTS_OK;
}

// ---------------------------------------------------------------------------------------------
// teacher-forced decoder loop
// ---------------------------------------------------------------------------------------------
extern "C" int mstts_decoder_train_ws_floats(int64_t B, int64_t H, int64_t M, int64_t A, int64_t* gates, int64_t* q) {
    int p0 = mstts_skinny_fwd_splits(4 * H, M + H), p1 = mstts_skinny_fwd_splits(4 * H, 2 * H), pq = mstts_skinny_fwd_splits(A, H);
    int pg = p0 > p1 ? p0 : p1;
    if (pg < 1) pg = 1;
    if (pq < 1) pq = 1;
    if (gates) *gates = (int64_t)pg * B * 4 * H;
    if (q) *q = (int64_t)pq * B * A;
    return MSTTS_OK;
}

// the two decoder cells' slots in the histories of the train descriptor: h0 behind the context in in0's rows, h1 behind m0 in in1's
static CellSlots train_cell0(const mstts_decoder_train_desc* d) {
    const long W0 = d->lsa.M + d->H;
    return CellSlots{d->B, d->H, d->c0, d->in0 + d->lsa.M, W0, d->B * W0, d->zc0, d->zh0, d->zoneout, d->acts0, d->craw0};
}
static CellSlots train_cell1(const mstts_decoder_train_desc* d) {
    return CellSlots{d->B, d->H, d->c1, d->in1 + d->H, 2 * d->H, d->B * 2 * d->H, d->zc1, d->zh1, d->zoneout, d->acts1, d->craw1};
}

extern "C" int mstts_decoder_train_fwd(const mstts_decoder_train_desc* d, mstts_stream_t s) {
    MSTTS_REQUIRE(d && d->xw0 && d->w0f && d->w1 && d->b1 && d->wq && d->in0 && d->in1 && d->pj && d->c0 && d->c1 &&
                  d->acts0 && d->acts1 && d->craw0 && d->craw1 && d->q_hist && d->align_hist && d->cum_hist && d->gates_ws &&
                  d->energy_ws && d->q_ws, MSTTS_ERR_SHAPE, "decoder_train_fwd: null pointer");
    const long B = d->B, S = d->S, H = d->H, M = d->lsa.M, A = d->lsa.A, T = d->lsa.T;
    MSTTS_REQUIRE(d->lsa.B == B, MSTTS_ERR_SHAPE, "decoder_train_fwd: lsa.B != B");
    const long BH = B * H, W0 = M + H, W1 = 2 * H, WP = H + M;
    const int sp0 = mstts_skinny_fwd_splits(4 * H, W0), sp1 = mstts_skinny_fwd_splits(4 * H, W1), spq = mstts_skinny_fwd_splits(A, H);
    int32_t bfs[6] = {0, 0, 0, 0, 0, 0};
    const bool bf = d->bf_w0f_f && d->bf_w1_f && d->bf_wq_f && mstts_decoder_bf16_splits(H, M, A, bfs);
    const Weights w0 = {d->w0f, 4 * H, W0, 4 * H, sp0, nullptr, bf ? d->bf_w0f_f : nullptr, bfs[0]}, w1 = {d->w1, 4 * H, W1, 4 * H, sp1, nullptr, bf ? d->bf_w1_f : nullptr, bfs[1]},
                  wq = {d->wq, A, H, A, spq, nullptr, bf ? d->bf_wq_f : nullptr, bfs[2]};
    // fused cell steps: the attention step writes the context into cell 0's packed block
    const bool fused_cells = d->act_p && M % 4 == 0 &&
                             (bf ? (d->w0p16 && d->w1p16 && mstts_cell_fwd_bf16_supported(H, W0) && mstts_cell_fwd_bf16_supported(H, W1))
                                 : (d->w0p && d->w1p && mstts_cell_fwd_supported(H, W0) && mstts_cell_fwd_supported(H, W1)));
    const float* w0pk = bf ? (const float*)d->w0p16 : d->w0p;
    const float* w1pk = bf ? (const float*)d->w1p16 : d->w1p;
    const long p0n = mstts_cell_act_floats(B, W0), p1n = mstts_cell_act_floats(B, W1);
    if (fused_cells) RC(zero(d->act_p, 2 * (p0n + p1n), s));          // step-0 state: zero context / hidden states
    RC(zero(d->in0, B * W0, s));
    RC(zero(d->in1, B * W1, s));
    RC(zero(d->c0, BH, s));
    RC(zero(d->c1, BH, s));
    RC(zero(d->cum_hist, B * T, s));
    // query projection inside the attention launch: geometry supported, by-unit filter given, granule buffer large enough
    const bool fused_q = mstts_lsa_step_q_supported(T, M, H) && d->lsa.loc_kt && A == 128 &&
                         d->energy_ws_floats >= mstts_lsa_step_q_ws_bytes(B, T) / 4 && WP % 4 == 0;
    RC(zero(d->energy_ws, 2 * (fused_q ? LsaGranules(nullptr, B, T).words_q() : LsaGranules(nullptr, B, T).words()), s));   // 8-byte granules + time-out counter
    const CellSlots k0 = train_cell0(d), k1 = train_cell1(d);
    unsigned long long* gran = (unsigned long long*)d->energy_ws;
    for (long st = 0; st < S; ++st) {
        const float* xw0 = d->xw0 + st * B * 4 * H;
        const float* in0 = d->in0 + st * B * W0; float* in0n = d->in0 + (st + 1) * B * W0;   // rows [ctx | h0]
        float* in1 = d->in1 + st * B * W1;                                                   // rows [m0 | h1]
        float* pj = d->pj + st * B * WP;                                                     // rows [m1 | ctx]
        mstts_cell_packed_dst ctx_p = packed(nullptr, 0, 0, 0);
        int parts = 1;
        if (fused_cells) {
            // packed activation blocks, ping-pong by step parity: P0 = [ctx | h0] of cell 0, P1 = [m0 | h1] of cell 1.
            // cell 0 (step st) reads P0[st&1], writes m0 -> P1[st&1] and h0' -> P0[~st&1]; cell 1 reads P1[st&1], writes
            // h1' -> P1[~st&1]; the attention step writes ctx -> P0[~st&1].
            float* P0c = d->act_p + (st & 1) * p0n; float* P0n = d->act_p + ((st + 1) & 1) * p0n;
            float* P1c = d->act_p + 2 * p0n + (st & 1) * p1n; float* P1n = d->act_p + 2 * p0n + ((st + 1) & 1) * p1n;
            PROBED(MSTTS_PROBE_CELL0_GEMM, s, cell_step(k0, st, st, st + 1, P0c, w0pk, W0, xw0, nullptr, in1, W1, packed(P1c, W1, 0, bf), packed(P0n, W0, M, bf), bf, s));
            PROBED(MSTTS_PROBE_CELL1_GEMM, s, cell_step(k1, st, st, st + 1, P1c, w1pk, W1, nullptr, d->b1, pj, WP, packed(nullptr, 0, 0, bf), packed(P1n, W1, H, bf), bf, s));
            ctx_p = packed(P0n, W0, 0, bf);
        } else {
            mstts_lstm_point_fwd_desc p;
            // ---- cell 0: gates = [ctx | h0] . w0f + xw0[st]
            PROBED(MSTTS_PROBE_CELL0_GEMM, s, recurrent_fwd(w0, in0, W0, d->gates_ws, B, &parts, s));
            fill_point_fwd(&p, k0, st, st, st + 1, d->gates_ws, parts);
            p.xw = xw0; p.xw_sb = 4 * H; p.out = in1; p.out_sb = W1;
            RC(mstts_lstm_point_fwd(&p, s));
            // ---- cell 1: gates = [m0 | h1] . w1 + b1
            PROBED(MSTTS_PROBE_CELL1_GEMM, s, recurrent_fwd(w1, in1, W1, d->gates_ws, B, &parts, s));
            fill_point_fwd(&p, k1, st, st, st + 1, d->gates_ws, parts);
            p.bias = d->b1; p.out = pj; p.out_sb = WP;
            RC(mstts_lstm_point_fwd(&p, s));
        }
        // ---- query (partials summed inside the attention kernel, which also saves q) + attention
        float* q_hist = d->q_hist + st * B * A; float* align = d->align_hist + st * B * T;
        const float* cum = d->cum_hist + st * B * T; float* cum_n = d->cum_hist + (st + 1) * B * T;
        if (fused_q) {              // one launch: the eight slices of a row compute and exchange the query themselves
            PROBED(MSTTS_PROBE_LSA_ENERGY, s, mstts_lsa_step_fwd_q(&d->lsa, pj, WP, d->wq, H, bf, q_hist, cum, align, cum_n, in0n, W0, pj + H, WP,
                                                                    fused_cells ? &ctx_p : nullptr, gran, (uint32_t)(st + 1), -1, s));
            continue;
        }
        RC(recurrent_fwd(wq, pj, WP, d->q_ws, B, &parts, s));
        PROBED(MSTTS_PROBE_LSA_ENERGY, s, mstts_lsa_step_fwd(&d->lsa, d->q_ws, parts, B * A, q_hist, cum, align, cum_n, in0n, W0, pj + H, WP,
                                                              fused_cells ? &ctx_p : nullptr, gran, (uint32_t)(st + 1), s));
    }
    return MSTTS_OK;
}

extern "C" int32_t mstts_decoder_train_bwd_parts(int64_t H, int64_t M) {
    const int p = mstts_skinny_bwd_splits(M + H, 4 * H);
    return p > 0 ? p : 1;
}

extern "C" int64_t mstts_decoder_train_bwd_ws_floats(int64_t B, int64_t H, int64_t M, int64_t A, int64_t T, int64_t CH) {
    int p1 = mstts_skinny_bwd_splits(2 * H, 4 * H), pq = mstts_skinny_bwd_splits(H, A);
    if (p1 < 1) p1 = 1;
    if (pq < 1) pq = 1;
    return 8 * B * H + 2 * B * T + 2 * B * T * CH + B * T + (int64_t)p1 * B * 2 * H + (int64_t)pq * B * H;
}

extern "C" int mstts_decoder_train_bwd(const mstts_decoder_train_bwd_desc* bd, mstts_stream_t s) {
    MSTTS_REQUIRE(bd && bd->fwd && bd->d_pj && bd->dg0 && bd->dg1 && bd->dq_hist && bd->de_hist && bd->d_in0 && bd->ws,
                  MSTTS_ERR_SHAPE, "decoder_train_bwd: null pointer");
    const mstts_decoder_train_desc* d = bd->fwd;
    const long B = d->B, S = d->S, H = d->H, M = d->lsa.M, A = d->lsa.A, T = d->lsa.T, CH = d->lsa.CH;
    MSTTS_REQUIRE((bd->ctx_dead == 0 || bd->ctx_dead == 256) && bd->ctx_dead <= M, MSTTS_ERR_SHAPE, "decoder_train_bwd: ctx_dead must be 0 or 256");
    const long BH = B * H, BT = B * T, W0 = M + H, W1 = 2 * H, WP = H + M;
    const int sp1 = mstts_skinny_bwd_splits(W1, 4 * H), sp0 = mstts_skinny_bwd_splits(W0, 4 * H), spq = mstts_skinny_bwd_splits(H, A);
    const int np1 = sp1 > 0 ? sp1 : 1, npq = spq > 0 ? spq : 1;
    int32_t bfs[6] = {0, 0, 0, 0, 0, 0};
    const bool bf = d->bf_w0f_b && d->bf_w1_b && d->bf_wq_b && mstts_decoder_bf16_splits(H, M, A, bfs);
    const Weights w0 = {d->w0f, 4 * H, W0, 4 * H, sp0, d->w0f_bp, bf ? d->bf_w0f_b : nullptr, bfs[3]}, w1 = {d->w1, 4 * H, W1, 4 * H, sp1, d->w1_bp, bf ? d->bf_w1_b : nullptr, bfs[4]},
                  wq = {d->wq, A, H, A, spq, d->wq_bp, bf ? d->bf_wq_b : nullptr, bfs[5]};
    const long d_in0_slab = S * B * W0;
    // single-launch attention backward: its granules (B*ceil(T/8)+1 8-byte words) live in the d_align block (B*T floats)
    const bool fused_lsa = WP % 4 == 0 && H % 4 == 0;            // (the single-launch backward reads the forward context rows as float4)
    // query-layer data gradient inside cell 1's pointwise kernel: fp32 mode, A == 128, slab counts the lean kernel is built for
    // (bf16 mode: the kernel rounds both operands to bf16 first - the same products as the bf16 product launch it replaces)
    const int np1_eff = bf ? bfs[4] : np1;
    const bool fuse_q = d->wq_t && A == 128 && H % 128 == 0 && (np1_eff == 8 || np1_eff == 4 || np1_eff == 2 || np1_eff == 1) && B * H * 4 < (1LL << 30);
    // workspace: the two cells' state gradients, then the attention's carried gradients and the product slabs
    float* w = bd->ws;
    RC(zero(w, 8 * BH + 2 * BT + 2 * BT * CH + BT + (long)np1 * B * W1 + (long)npq * BH, s));
    float* ds0 = w;                                 w += 4 * BH;
    float* ds1 = w;                                 w += 4 * BH;
    float* G[2] = {w, w + BT};                      w += 2 * BT;
    float* df[2] = {w, w + BT * CH};                w += 2 * BT * CH;
    float* d_align = w;                             w += BT;
    float* tmp1 = w;                                w += (long)np1 * B * W1;      // [parts1][B][m0 | h1 state]
    float* dqm = w;                                                               // [partsq][B][H]
    const CellSaved k0 = saved(train_cell0(d)), k1 = saved(train_cell1(d));
    int cur = 0, parts0 = 1, parts1 = 1, partsq = 1;
    for (long st = S - 1; st >= 0; --st, cur ^= 1) {
        const int nxt = cur ^ 1;
        const bool last = (st == S - 1);
        float* dpj = bd->d_pj + st * B * WP;
        float* dq = bd->dq_hist + st * B * A; float* de = bd->de_hist + st * B * T;
        const float* align = d->align_hist + st * B * T; const float* q_hist = d->q_hist + st * B * A; const float* cum = d->cum_hist + st * B * T;
        const float* d_in0_next = last ? nullptr : bd->d_in0 + (st + 1) * B * W0;
        // ---- attention backward
        if (fused_lsa) {        // d_align stays on chip
            PROBED(MSTTS_PROBE_LSA_DALIGN, s, mstts_lsa_step_bwd(&d->lsa, dpj + H, WP, d_in0_next, W0, parts0, d_in0_slab, last ? nullptr : G[cur],
                                                                  last ? nullptr : df[cur], G[nxt], align, q_hist, cum, d->pj + st * B * WP + H, WP, de, dq, df[nxt], s));
        } else {
            PROBED(MSTTS_PROBE_LSA_DALIGN, s, mstts_lsa_dalign_bwd(&d->lsa, dpj + H, WP, d_in0_next, W0, parts0, d_in0_slab, last ? nullptr : G[cur],
                                                                    last ? nullptr : df[cur], G[nxt], d_align, s));
            PROBED(MSTTS_PROBE_LSA_DENERGY, s, mstts_lsa_denergy_bwd(&d->lsa, align, d_align, q_hist, cum, de, dq, df[nxt], s));
        }
        // ---- cell 1 backward; d_m1 (query path) = dq . Wq^T: folded into the pointwise kernel, or slabs it consumes
        mstts_lstm_point_bwd_desc p;
        fill_point_bwd(&p, k1, st, ds1, cur, bd->dg1 + st * B * 4 * H);
        p.d_out = dpj; p.dout_sb = WP;
        if (fuse_q) { p.dq = dq; p.wq_t = d->wq_t; p.A = A; p.dq_bf16 = bf; }
        else {
            RC(recurrent_bwd(wq, dq, A, dqm, 0, B, &partsq, s));
            p.d_out2 = dqm; p.dout2_parts = partsq; p.dout2_pstride = BH;
        }
        p.d_h_state2 = last ? nullptr : tmp1 + H; p.dhs2_ld = W1; p.dhs2_parts = parts1; p.dhs2_pstride = B * W1;
        RC(mstts_lstm_point_bwd(&p, s));
        // [d_m0 | d_h1 state] = dg1 . w1^T
        PROBED(MSTTS_PROBE_CELL1_DGEMM, s, recurrent_bwd(w1, p.dgates, 4 * H, tmp1, 0, B, &parts1, s));
        // ---- cell 0 backward
        fill_point_bwd(&p, k0, st, ds0, cur, bd->dg0 + st * B * 4 * H);
        p.d_out = tmp1; p.dout_sb = W1; p.dout_parts = parts1; p.dout_pstride = B * W1;
        p.d_h_state2 = last ? nullptr : d_in0_next + M; p.dhs2_ld = W0; p.dhs2_parts = parts0; p.dhs2_pstride = d_in0_slab;
        RC(mstts_lstm_point_bwd(&p, s));
        // [d_ctx_{st-1} | d_h0 state] = dg0 . w0f^T   (slabs at stride S*B*W0)
        PROBED(MSTTS_PROBE_CELL0_DGEMM, s, recurrent_bwd(w0, p.dgates, 4 * H, bd->d_in0 + st * B * W0, d_in0_slab, B, &parts0, s));
    }
    if (bd->ctx_dead > 0 && S * B > 0) {
        // the dead context columns of every slab: computed above like the others (the attention backward read them, where their constant
        // cancels), handed to the caller as the zeros the persistent launch leaves there
        const long slabs = mstts_decoder_train_bwd_parts(H, M);
        MSTTS_REQUIRE(hipMemset2DAsync(bd->d_in0 + (M - bd->ctx_dead), (size_t)W0 * 4, 0, (size_t)bd->ctx_dead * 4, (size_t)(slabs * S * B), (hipStream_t)s) == hipSuccess,
                      MSTTS_ERR_LAUNCH, "decoder_train_bwd: clearing the dead context columns failed");
    }
    return MSTTS_OK;
}

// ---------------------------------------------------------------------------------------------
// free-running decoder steps
// ---------------------------------------------------------------------------------------------
namespace mstts {
// Two-layer prenet of one decoder step for B <= 32 rows in ONE launch (prenet_body.h), the frame read from memory
__global__ __launch_bounds__(256) void prenet_step_kernel(const float* __restrict__ frame, int NM, const float* __restrict__ w0,
                                                          const float* __restrict__ b0, const float* __restrict__ w1, const float* __restrict__ b1,
                                                          const uint8_t* __restrict__ m0, const uint8_t* __restrict__ m1, float inv_keep,
                                                          int B, int P, float* __restrict__ out, long out_ld, PackedDst out_p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    PnFramePlain src{frame};
    prenet_body(src, (int)blockIdx.x * PN_COLS, NM, w0, b0, w1, b1, m0, m1, inv_keep, B, P, out, out_ld, out_p, sm);
}
// [parts][B][NP] projection partial slabs + bias -> linear[B][NM], stop[B] (column NM)
__global__ void proj_finish_kernel(const float* __restrict__ P_, int parts, long pstride, const float* __restrict__ bias, int B, int NP, int NM,
                                   float* __restrict__ linear, float* __restrict__ stop) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * (NM + 1)) return;
    const int b = i / (NM + 1), c = i % (NM + 1);
    float v = bias ? bias[c] : 0.f;
    for (int pp = 0; pp < parts; ++pp) v += P_[pp * pstride + (long)b * NP + c];
    if (c < NM) linear[(long)b * NM + c] = v; else stop[b] = v;
}
}  // namespace mstts

/* 1 when mstts_decoder_infer_steps can take its weight-streaming path (stacked cell-0 kernel w0s = [wx0 ; w0f] and the padded
 * projection kernel wp_pad must then be supplied in the descriptor). */
extern "C" int32_t mstts_decoder_infer_fast(int64_t B, int64_t H, int64_t P, int64_t M, int64_t A, int64_t n_mel) {
    const long NP = (n_mel + 1 + 3) / 4 * 4;
    if (B < 1 || B > PN_MAXB || M % 4 != 0) return 0;
    if (P % 64 != 0 || P / 64 > PN_MAXTPW || P / 16 > PN_MAXK1 || n_mel % 4 != 0 || n_mel / 4 > PN_MAXNM4) return 0;     // prenet_step_kernel tiles
    return mstts_skinny_fwd_splits(4 * H, P + M + H) > 0 && mstts_skinny_fwd_splits(4 * H, 2 * H) > 0 &&
           mstts_skinny_fwd_splits(A, H) > 0 && mstts_skinny_fwd_splits(NP, H + M) > 0;
}

// the two cells' slots of the free-running loop: two state slots each, ping-pong by step parity; h0 sits `h0_col` columns into in0's rows
static CellSlots infer_cell0(const mstts_decoder_infer_desc* d, long W0, long h0_col) {
    return CellSlots{d->B, d->H, d->c0, d->in0 + h0_col, W0, d->B * W0, nullptr, nullptr, d->zoneout, nullptr, nullptr};
}
static CellSlots infer_cell1(const mstts_decoder_infer_desc* d) {
    return CellSlots{d->B, d->H, d->c1, d->in1 + d->H, 2 * d->H, d->B * 2 * d->H, nullptr, nullptr, d->zoneout, nullptr, nullptr};
}
// projection of step st through the padded kernel: [m1 | ctx] . wp_pad in slabs at pp, then bias, linear and stop
static int project_step(const mstts_decoder_infer_desc* d, long st, float* pp, const Weights& wp, mstts_stream_t s) {
    const long B = d->B, NM = d->n_mel, NP = wp.cols;
    int parts = 1;
    RC(recurrent_fwd(wp, d->pj, wp.rows, pp, B, &parts, s));
    hipLaunchKernelGGL(proj_finish_kernel, dim3((unsigned)((B * (NM + 1) + 255) / 256)), dim3(256), 0, (hipStream_t)s, pp, parts, B * NP, d->bproj,
                       (int)B, (int)NP, (int)NM, d->linear + st * B * NM, d->stop + st * B);
    MSTTS_CHECK_LAUNCH("proj_finish");
    return MSTTS_OK;
}

static int infer_steps_fast(const mstts_decoder_infer_desc* d, int64_t step0, int64_t n, mstts_stream_t s) {
    const long B = d->B, H = d->H, P = d->P, NM = d->n_mel, M = d->lsa.M, A = d->lsa.A, T = d->lsa.T;
    const long BH = B * H, W0 = P + M + H, W1 = 2 * H, WP = H + M, BT = B * T, NP = (NM + 1 + 3) / 4 * 4;
    const Weights w0 = {d->w0s, 4 * H, W0, 4 * H, mstts_skinny_fwd_splits(4 * H, W0), nullptr, nullptr, 0}, w1 = {d->w1, 4 * H, W1, 4 * H, mstts_skinny_fwd_splits(4 * H, W1), nullptr, nullptr, 0},
                  wq = {d->wq, A, H, A, mstts_skinny_fwd_splits(A, H), nullptr, nullptr, 0}, wp = {d->wp_pad, NP, WP, NP, mstts_skinny_fwd_splits(NP, WP), nullptr, nullptr, 0};
    float* w = d->pre_ws;
    float* gates = w;       w += (long)MSTTS_MAX_PARTS * 4 * BH;
    const long gran_n = mstts_lsa_step_qp_ws_bytes(B, T) / 4;       // energy granules + counter, then the query and the frame granules
    float* gran = w;        w += gran_n;
    float* q = w;           w += (long)MSTTS_MAX_PARTS * B * A;
    float* pp = w;          w += (long)MSTTS_MAX_PARTS * B * NP;
    float* zero_frame = w;  w += B * NM;
    if (step0 == 0) {
        RC(zero(d->in0, 2 * B * W0, s));
        RC(zero(d->in1, 2 * B * W1, s));
        RC(zero(d->c0, 2 * BH, s));
        RC(zero(d->c1, 2 * BH, s));
        RC(zero(d->cum, 2 * BT, s));
        RC(zero(zero_frame, B * NM, s));
        RC(zero(gran, gran_n, s));
    }
    // query projection inside the attention launch, and the output projection too where the slice count allows
    const bool fused_q = mstts_lsa_step_q_supported(T, M, H) && d->lsa.loc_kt && A == 128 && WP % 4 == 0;
    const bool fused_qp = fused_q && d->wp_own && d->vp && mstts_lsa_step_qp_supported(T, M, H, NP);
    // ... and the next step's prenet too (the frame leaves its owners before their context phase): 3 launches per frame
    const bool fused_pre = fused_qp && mstts_lsa_step_prenet_supported(P, NM);
    const size_t pn_lds = sizeof(float) * (size_t)(PN_MAXB * (NM + 1) + PN_MAXB * (P + 1) + 4 * 32 * 17);
    // fused cell steps (cell.hip): packed kernels given and shapes covered -> 7 launches per frame instead of 9
    const bool fused = d->w0sp && d->w1p && d->act_p && mstts_cell_fwd_supported(H, W0) && mstts_cell_fwd_supported(H, W1);
    const long p0n = mstts_cell_act_floats(B, W0), p1n = mstts_cell_act_floats(B, W1);
    if (fused && step0 == 0) RC(zero(d->act_p, 2 * (p0n + p1n), s));
    const CellSlots k0 = infer_cell0(d, W0, P + M), k1 = infer_cell1(d);
    for (long st = step0; st < step0 + n; ++st) {
        const int par = (int)(st & 1), nx = par ^ 1;
        const float* frame = (st == 0) ? zero_frame : d->linear + (st - 1) * B * NM;
        float* in0c = d->in0 + par * B * W0; float* in0n = d->in0 + nx * B * W0;      // rows [prenet P | ctx M | h0 H]
        float* in1c = d->in1 + par * B * W1;                                          // rows [m0 H | h1 H]
        float* cum = d->cum + par * BT; float* cum_n = d->cum + nx * BT; float* align = d->align_hist + st * BT;
        float* P0c = fused ? d->act_p + par * p0n : nullptr; float* P0n = fused ? d->act_p + nx * p0n : nullptr;
        float* P1c = fused ? d->act_p + 2 * p0n + par * p1n : nullptr; float* P1n = fused ? d->act_p + 2 * p0n + nx * p1n : nullptr;
        PackedDst pre_p;
        pre_p.base = P0c; pre_p.nit = (int)(W0 / 64); pre_p.col0 = 0; pre_p.bf = 0;
        const bool pre_here = fused && fused_pre;        // the previous step's attention launch has left this step's prenet in in0c / P0c
        if (!pre_here || st == 0) {
            hipLaunchKernelGGL(prenet_step_kernel, dim3((unsigned)((P + PN_COLS - 1) / PN_COLS)), dim3(256), pn_lds, (hipStream_t)s, frame, (int)NM,
                               d->pw0, d->pb0, d->pw1, d->pb1, d->pm0 + st * B * P, d->pm1 + st * B * P, 1.f / d->prenet_keep, (int)B, (int)P, in0c, W0, pre_p);
            MSTTS_CHECK_LAUNCH("prenet_step");
        }
        int parts = 1;
        if (fused) {
            RC(cell_step(k0, 0, par, nx, P0c, d->w0sp, W0, nullptr, d->b0, in1c, W1, packed(P1c, W1, 0, 0), packed(P0n, W0, P + M, 0), 0, s));
            RC(cell_step(k1, 0, par, nx, P1c, d->w1p, W1, nullptr, d->b1, d->pj, WP, packed(nullptr, 0, 0, 0), packed(P1n, W1, H, 0), 0, s));
            mstts_cell_packed_dst ctx_p = packed(P0n, W0, P, 0);
            if (fused_qp) {
                mstts_lsa_prenet pn;
                memset(&pn, 0, sizeof(pn));
                const bool pre_next = fused_pre && st + 1 < d->Smax;           // (the masks hold Smax steps)
                if (pre_next) {
                    pn.w0 = d->pw0; pn.b0 = d->pb0; pn.w1 = d->pw1; pn.b1 = d->pb1; pn.m0 = d->pm0 + (st + 1) * B * P; pn.m1 = d->pm1 + (st + 1) * B * P;
                    pn.inv_keep = 1.f / d->prenet_keep; pn.P = (int32_t)P; pn.out = in0n; pn.out_ld = W0;
                    pn.out_p = packed(P0n, W0, 0, 0);
                }
                RC(mstts_lsa_step_fwd_qp(&d->lsa, d->pj, WP, d->wq, H, d->wp_own, d->vp, d->bproj, NP, NM, d->linear + st * B * NM, d->stop + st * B,
                                         cum, align, cum_n, in0n + P, W0, d->pj + H, WP, &ctx_p, pre_next ? &pn : nullptr, gran, (uint32_t)(st + 1), -1, s));
                continue;
            }
            if (fused_q) {
                RC(mstts_lsa_step_fwd_q(&d->lsa, d->pj, WP, d->wq, H, 0, nullptr, cum, align, cum_n, in0n + P, W0, d->pj + H, WP, &ctx_p, gran,
                                        (uint32_t)(st + 1), -1, s));
            } else {
                RC(recurrent_fwd(wq, d->pj, WP, q, B, &parts, s));
                RC(mstts_lsa_step_fwd(&d->lsa, q, parts, B * A, nullptr, cum, align, cum_n, in0n + P, W0, d->pj + H, WP, &ctx_p, gran, (uint32_t)(st + 1), s));
            }
            RC(project_step(d, st, pp, wp, s));
            continue;
        }
        mstts_lstm_point_fwd_desc p;
        RC(recurrent_fwd(w0, in0c, W0, gates, B, &parts, s));
        fill_point_fwd(&p, k0, 0, par, nx, gates, parts);
        p.bias = d->b0; p.out = in1c; p.out_sb = W1;
        RC(mstts_lstm_point_fwd(&p, s));
        RC(recurrent_fwd(w1, in1c, W1, gates, B, &parts, s));
        fill_point_fwd(&p, k1, 0, par, nx, gates, parts);
        p.bias = d->b1; p.out = d->pj; p.out_sb = WP;
        RC(mstts_lstm_point_fwd(&p, s));
        RC(recurrent_fwd(wq, d->pj, WP, q, B, &parts, s));
        RC(mstts_lsa_step_fwd(&d->lsa, q, parts, B * A, nullptr, cum, align, cum_n, in0n + P, W0, d->pj + H, WP, nullptr, gran, (uint32_t)(st + 1), s));
        RC(project_step(d, st, pp, wp, s));
    }
    return MSTTS_OK;
}

extern "C" int64_t mstts_decoder_infer_ws_floats(int64_t B, int64_t H, int64_t P, int64_t T, int64_t A, int64_t n_mel) {
    const long np = (n_mel + 1 + 3) / 4 * 4;
    const long slow = 2 * B * P + 8 * B * H + 2 * LsaGranules(nullptr, B, T).words() + B * A + B * n_mel;
    const long fast = (long)MSTTS_MAX_PARTS * (4 * B * H + B * A + B * np) + mstts_lsa_step_qp_ws_bytes(B, T) / 4 + B * n_mel;
    return slow > fast ? slow : fast;
}

extern "C" int mstts_decoder_infer_steps(const mstts_decoder_infer_desc* d, int64_t step0, int64_t n, mstts_stream_t s) {
    MSTTS_REQUIRE(d && d->pw0 && d->pw1 && d->wx0 && d->w0f && d->w1 && d->wq && d->wproj && d->in0 && d->in1 && d->pj &&
                  d->c0 && d->c1 && d->cum && d->pre_ws && d->linear && d->stop && d->align_hist && d->pm0 && d->pm1,
                  MSTTS_ERR_SHAPE, "decoder_infer_steps: null pointer");
    MSTTS_REQUIRE(step0 >= 0 && step0 + n <= d->Smax, MSTTS_ERR_SHAPE, "decoder_infer_steps: step range exceeds Smax");
    if (d->w0s && d->wp_pad && mstts_decoder_infer_fast(d->B, d->H, d->P, d->lsa.M, d->lsa.A, d->n_mel)) return infer_steps_fast(d, step0, n, s);
    // any other shape: every product on the tiled GEMM, the prenet as separate launches
    const long B = d->B, H = d->H, P = d->P, NM = d->n_mel, M = d->lsa.M, A = d->lsa.A, T = d->lsa.T;
    const long BH = B * H, W0 = M + H, W1 = 2 * H, WP = H + M, BT = B * T;
    float* w = d->pre_ws;
    float* pa = w;          w += B * P;
    float* pb = w;          w += B * P;
    float* xw = w;          w += 4 * BH;
    float* gates = w;       w += 4 * BH;
    float* gran = w;        w += 2 * LsaGranules(nullptr, B, T).words();          // the 8-byte granules (+ counter) of the single-launch attention step
    float* q = w;           w += B * A;
    float* zero_frame = w;  w += B * NM;
    if (step0 == 0) {
        RC(zero(d->in0, B * W0, s));
        RC(zero(d->in1, B * W1, s));
        RC(zero(d->c0, BH, s));
        RC(zero(d->c1, BH, s));
        RC(zero(d->cum, BT, s));
        RC(zero(zero_frame, B * NM, s));
        RC(zero(gran, 2 * LsaGranules(nullptr, B, T).words(), s));
    }
    const CellSlots k0 = infer_cell0(d, W0, M), k1 = infer_cell1(d);
    for (long st = step0; st < step0 + n; ++st) {
        const int par = (int)(st & 1), nx = par ^ 1;
        const float* frame = (st == 0) ? zero_frame : d->linear + (st - 1) * B * NM;
        // prenet (dropout always on, Modules.py:248-253)
        RC(gemm(frame, NM, d->pw0, P, 0, pa, P, B, P, NM, d->pb0, MSTTS_ACT_RELU, 0, s));
        RC(mstts_dropout(pa, d->pm0 + st * B * P, d->prenet_keep, pb, B * P, s));
        RC(gemm(pb, P, d->pw1, P, 0, pa, P, B, P, P, d->pb1, MSTTS_ACT_RELU, 0, s));
        RC(mstts_dropout(pa, d->pm1 + st * B * P, d->prenet_keep, pb, B * P, s));
        RC(gemm(pb, P, d->wx0, 4 * H, 0, xw, 4 * H, B, 4 * H, P, d->b0, 0, 0, s));
        mstts_lstm_point_fwd_desc p;
        float* in0c = d->in0 + par * B * W0; float* in0n = d->in0 + nx * B * W0;
        float* in1c = d->in1 + par * B * W1;
        // cell 0
        RC(gemm(in0c, W0, d->w0f, 4 * H, 0, gates, 4 * H, B, 4 * H, W0, nullptr, 0, 0, s));
        fill_point_fwd(&p, k0, 0, par, nx, gates, 1);
        p.xw = xw; p.xw_sb = 4 * H; p.out = in1c; p.out_sb = W1;
        RC(mstts_lstm_point_fwd(&p, s));
        // cell 1
        RC(gemm(in1c, W1, d->w1, 4 * H, 0, gates, 4 * H, B, 4 * H, W1, nullptr, 0, 0, s));
        fill_point_fwd(&p, k1, 0, par, nx, gates, 1);
        p.bias = d->b1; p.out = d->pj; p.out_sb = WP;
        RC(mstts_lstm_point_fwd(&p, s));
        // attention
        RC(gemm(d->pj, WP, d->wq, A, 0, q, A, B, A, H, nullptr, 0, 0, s));
        RC(mstts_lsa_step_fwd(&d->lsa, q, 1, 0, nullptr, d->cum + par * BT, d->align_hist + st * BT, d->cum + nx * BT,
                              in0n, W0, d->pj + H, WP, nullptr, gran, (uint32_t)(st + 1), s));
        // projection: [m1 | ctx] . Wp + b -> linear (n_mel) and stop (1)
        RC(gemm(d->pj, WP, d->wproj, NM + 1, 0, d->linear + st * B * NM, NM, B, NM, WP, d->bproj, 0, 0, s));
        RC(gemm(d->pj, WP, d->wproj + NM, NM + 1, 0, d->stop + st * B, 1, B, 1, WP, d->bproj ? d->bproj + NM : nullptr, 0, 0, s));
    }
    return MSTTS_OK;
}
