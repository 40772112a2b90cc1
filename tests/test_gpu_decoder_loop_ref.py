"""The teacher-forced decoder loop drivers and their BPTT against the fp64 checker tests/decoder_loop_ref.py (oracle.model.decoder's training
loop written out around zoneout_lstm_cell and lsa_step, gradients by autograd), every form on its own - never one form against another:
    launch-per-step, full     mstts_decoder_train_fwd + mstts_decoder_train_bwd with the descriptor as engine.py builds it: packed cell kernels
                              and activation blocks (fused cell steps), the by-unit location filter and the granule room (query projection inside
                              the attention launch), packed BPTT kernels, the transposed query kernel (query gradient folded into cell 1's
                              pointwise backward) - whatever the shape admits, asserted with the *_supported / *_splits queries
    launch-per-step, nulled   the same with every optional derived-copy pointer NULL (NULLED of test_gpu_loop_tiers.py, and lsa.loc_kt)
    persistent, xw0           mstts_decoder_train_fwd_persistent reading xw0, opk = NULL: row-major histories
    persistent, pre + opk     the same launch forming the prenet rows' product itself (pre / b0) and packing the cell operands (opk), then
                              mstts_persist_unpack_history, then mstts_decoder_train_bwd_persistent behind it (its first d_in0 slab carries only
                              the context columns of slots 1 .. S-1: exactly those are compared)
This is the base the "A equals B" comparisons of test_gpu_loop_tiers.py and test_gpu_persist.py stand on.  The bf16 forms of the same drivers
are held stage by stage to the same oracle in tests/test_gpu_decoder_bf16_ref.py, which builds its descriptors with the helpers below.

Inputs: the descriptors are built by hand from the case data of tests/decoder_loop_ref.py (packs through mstts_pack_cell_fwd,
mstts_pack_skinny_bwd, mstts_transpose01, mstts_persist_pack, mstts_persist_bwd_pack, mstts_lsa_fold_location, mstts_lsa_filter_by_unit, as
engine.py makes them), not taken from a TrainEngine: the loop's inputs are then float32 arrays drawn once on the host, the reference reads the
very arrays that are uploaded (no read-back, nothing upstream of the loop with atomics in it), the CPU test can pin the same cases and their
e32 without a GPU, and no encoder, prenet or postnet runs per case.

Cases (tests/decoder_loop_ref.py CASES), the smallest that reach each path; row 0 has token length Te, row 1 length 1:
  two_steps       defaults (H 32, M 48)  B 1  Te 7   S 2   smallest batch; one live BPTT hand-over; no fused cells, cell 0's product on the tiled GEMM
  plain_h32       defaults               B 3  Te 9   S 4   tiled-GEMM forward product, one-slab backward products
  fused_h64       MID (H 64, M 128)      B 5  Te 18  S 5   fused cell steps without the fused query, skinny K-splits, two d_in0 slabs
  two_pass_t140   MID                    B 2  Te 140 S 3   more tokens than one attention pass
  wide_one_tile   WIDE (H 1024, M 768)   B 3  Te 7   S 4   fused query, folded query gradient, eight d_in0 slabs; persistent launches
  wide_two_tiles  WIDE                   B 17 Te 12  S 4   both MFMA row tiles live
  wide_full       WIDE                   B 32 Te 128 S 3   full batch at the 128-token geometry
  wide_t131       WIDE                   B 5  Te 131 S 3   the 256-position persistent instantiation

Compared per (step, row) slice on the slice's own scale: in0, in1, pj, c0, c1, acts0/1, craw0/1, q_hist, align_hist, cum_hist, dg0, dg1, dq_hist,
de_hist, d_in0 (slabs summed), d_ctx, and - formed on the host in fp64 from the returned tensors, no GEMM kernel - dW0f, dW1, db1, dWq and
d_values (decoder_loop_ref.host_grads).  Every buffer a form writes in full is NaN-filled before the call and must be finite afterwards; the
forms of a case share no output buffer.  Exactly: align_hist, de_hist and the increments of cum_hist are 0 past a row's token length; slot 0 of
in0, c0, c1, cum_hist and the state half of in1 slot 0 are 0; d_pj is bit-identical after either BPTT form (both only read it).

Bound per quantity: MARGIN (8) x e32, e32 = the worst slice error of the same checker evaluated in float32 on the CPU; floor 1e-6.
Measured on an MI355X, the form with the largest error / bound per case and quantity, in units of 1e-7, e32 -> kernel (q, align, cum, dq, de:
the *_hist tensors; e32 is the float32 evaluation on that machine's CPU and differs from machine to machine by the draw of the worst slice):
  case           in0        in1        pj         c0         c1         acts0      acts1      craw0      craw1      q          align      cum
  two_steps      0.9->1.1   0.9->1.8   0.9->1.1   1.7->1.1   0.8->1.3   1.8->1.4   0.7->0.7   1.6->1.4   0.6->1.0   1.9->2.0   0.7->0.7   0.8->0.7
  plain_h32      2.0->1.7   2.6->2.7   2.0->1.7   3.5->3.0   1.5->1.9   3.3->2.3   1.5->1.5   3.0->2.4   1.7->2.9   2.7->3.4   1.7->1.3   1.1->1.2
  fused_h64      1.8->2.3   6.6->3.9   1.7->2.3   4.7->3.9   3.1->2.5   6.9->2.4   2.4->1.5   4.8->2.8   3.0->2.5   3.3->4.3   1.7->3.2   1.4->1.8
  two_pass_t140  1.4->3.0   2.8->3.2   1.4->3.0   2.4->1.8   2.0->1.8   3.8->1.5   2.4->1.1   2.4->1.6   2.0->1.8   3.3->3.4   1.2->1.3   0.8->1.3
  wide_one_tile  3.0->2.3   13.0->9.0  1.9->1.6   13.0->5.6  14.0->3.7  23.0->9.1  16.0->3.6  13.0->5.8  14.0->4.0  13.0->5.8  1.1->1.1   1.7->1.5
  wide_two_tiles 3.2->2.9   10.0->7.8  2.2->2.9   9.1->6.2   9.5->4.3   16.0->11.0 9.6->4.7   9.4->6.3   9.7->4.3   10.0->5.2  2.0->2.5   1.4->2.5
  wide_full      2.9->4.7   4.4->7.0   2.7->3.8   3.9->6.1   3.0->3.7   8.2->7.6   2.6->2.9   3.9->6.1   2.8->3.7   5.4->5.1   3.0->3.1   2.9->2.9
  wide_t131      3.3->3.7   5.4->7.2   2.1->3.1   5.3->4.4   5.5->3.2   7.5->8.5   5.2->2.5   5.5->4.8   5.8->3.2   10.0->4.4  1.9->3.4   1.9->1.9
  case           dg0        dg1        dq         de         d_in0      d_ctx      dw0f       dw1        db1        dwq        d_values
  two_steps      2.7->2.0   1.6->1.5   2.1->2.9   1.0->3.2   2.7->2.5   2.7->2.5   1.5->1.3   0.9->1.0   1.2->1.3   1.4->1.2   1.2->1.5
  plain_h32      3.1->3.3   2.6->1.9   3.8->4.8   2.8->3.1   3.1->2.8   3.2->2.6   0.7->0.4   0.8->0.6   1.0->1.1   0.9->1.1   2.1->2.1
  fused_h64      4.4->3.3   2.1->2.6   5.5->13.0  3.6->3.5   6.2->3.4   6.2->3.4   0.7->0.4   0.7->0.4   1.0->1.1   0.6->0.6   2.6->1.8
  two_pass_t140  4.9->2.7   1.7->1.8   6.0->6.0   2.3->2.2   3.4->2.7   3.3->2.7   1.4->0.8   1.2->1.0   1.2->1.1   1.9->1.2   2.6->1.9
  wide_one_tile  25.0->5.8  5.5->2.7   5.8->10.0  2.2->3.0   15.0->4.9  15.0->4.9  3.5->1.6   2.7->2.5   2.6->1.6   1.7->1.5   1.9->2.2
  wide_two_tiles 11.0->6.8  3.0->2.7   8.3->21.0  5.0->9.2   10.0->5.4  11.0->6.2  0.8->0.4   0.3->0.4   1.3->1.3   0.5->0.8   2.0->2.4
  wide_full      5.6->6.1   2.4->2.9   7.2->13.0  3.3->5.7   5.3->5.6   5.3->5.6   0.6->0.6   0.1->0.2   1.3->1.0   0.3->0.6   3.1->3.6
  wide_t131      7.5->4.3   2.1->2.7   4.9->9.6   2.5->3.4   11.0->4.7  11.0->4.7  0.8->0.8   1.0->1.2   1.4->1.4   1.1->1.7   2.4->3.7
No form of any case needs more than 3.2 x e32 (de_hist of two_steps, launch-per-step: 3.2e-7 against e32 1.0e-7, its bound being the floor
1e-6); the worst error / bound is 0.32.  dw0f, dw1 and dwq are judged with the magnitude of the sum's terms in the scale
(decoder_loop_ref.TERM_SCALED, where the reason is written down); every test also prints them on the rows' own scale, where the same run
gave at most 2.3 x e32 everywhere except dw0f of two_steps - ONE live outer product - at 8.5 x e32 (6.7e-6 against 0.79e-6), both launch-per-step
tiers alike.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.helpers import small_dims, t2n
from multi_speaker_tts_amd import lib
from multi_speaker_tts_amd.persist import near_xcd
from tests import decoder_loop_ref as R
from tests.test_gpu_loop_tiers import MID, NULLED
from tests.test_gpu_persist import WIDE

pytestmark = pytest.mark.gpu
A, CH, KS = R.A, R.CH, R.KS
FWD_BUFS = R.FORWARD_Q
LPS_Q = R.FORWARD_Q + R.BACKWARD_Q + R.HOST_Q
PERSIST_BWD_Q = ("dg0", "dg1", "dq_hist", "de_hist", "d_ctx") + R.HOST_Q


def test_widths_are_the_suites():
    """tests/decoder_loop_ref.py restates the widths (it imports from the oracle only): they are small_dims' with the overrides of the other
    loop tests."""
    for name, kw in (("defaults", {}), ("MID", MID), ("WIDE", WIDE)):
        cfg = small_dims(**kw)
        assert {k: cfg[k] for k in R.WIDTHS[name]} == R.WIDTHS[name], name
        assert (cfg["att_k"], cfg.get("att", A), cfg.get("att_ch", CH)) == (KS, A, CH)


def _nan(dev, *s):
    return torch.full(s, float("nan"), device=dev)


def _zeros(dev, n):
    return torch.zeros(int(n), device=dev)


@pytest.fixture(scope="module")
def wcache():
    cache = {}
    yield cache
    cache.clear()


BF_COPIES = ("w0f_f", "w1_f", "wq_f", "w0f_b", "w1_b", "wq_b")


def _bf16_copies(dev, w, widths):
    """The bf16 copies engine.py makes for recurrent_dtype "bf16": the six mstts_pack_bf16_fwd / _bwd copies with the counts of
    mstts_decoder_bf16_splits (where it admits the widths; zero-filled buffers where it does not - a driver that read them would multiply
    zeros) and the mstts_pack_cell_fwd_bf16 copies of the fused bf16 cell steps where both cells are supported."""
    L = lib.load()
    dm = R.dims_of(widths)
    H, M = dm["H"], dm["M"]
    sp = (C.c_int32 * 6)()
    w["bf_ok"], w["bf_splits"] = bool(L.mstts_decoder_bf16_splits(H, M, A, sp)), list(sp)
    i16 = lambda n: torch.zeros(n, dtype=torch.int16, device=dev)
    w["bf"] = {k: i16(n) for k, n in zip(BF_COPIES, ((M + H) * 4 * H, 2 * H * 4 * H, H * A) * 2)}
    if w["bf_ok"]:
        for i, (k, src, ld, rows, cols) in enumerate((("w0f_f", "w0f", 4 * H, M + H, 4 * H), ("w1_f", "w1", 4 * H, 2 * H, 4 * H), ("wq_f", "wq", A, H, A),
                                                      ("w0f_b", "w0f", 4 * H, M + H, 4 * H), ("w1_b", "w1", 4 * H, 2 * H, 4 * H), ("wq_b", "wq", A, H, A))):
            lib.call("mstts_pack_bf16_fwd" if i < 3 else "mstts_pack_bf16_bwd", lib.ptr(w[src]), ld, lib.ptr(w["bf"][k]), rows, cols, w["bf_splits"][i])
    w["w0p16"] = w["w1p16"] = None
    if L.mstts_cell_fwd_bf16_supported(H, M + H) and L.mstts_cell_fwd_bf16_supported(H, 2 * H):
        w["w0p16"], w["w1p16"] = i16((M + H) * 4 * H), i16(2 * H * 4 * H)
        lib.call("mstts_pack_cell_fwd_bf16", lib.ptr(w["w0f"]), 4 * H, lib.ptr(w["w0p16"]), M + H, H)
        lib.call("mstts_pack_cell_fwd_bf16", lib.ptr(w["w1"]), 4 * H, lib.ptr(w["w1p16"]), 2 * H, H)
    torch.cuda.synchronize()


def _weights(dev, cache, widths, bf16=False):
    """The variables of a set of widths on the device with every derived copy engine.py makes of them (refresh_derived, _ensure_fallback_packs);
    bf16: also the copies of its config-3 mode (_bf16_copies)."""
    if widths in cache:
        if bf16 and "bf" not in cache[widths]:
            _bf16_copies(dev, cache[widths], widths)
        return cache[widths]
    L = lib.load()
    dm = R.dims_of(widths)
    H, M = dm["H"], dm["M"]
    w = {k: v.to(dev).contiguous() for k, v in R.weights(widths).items()}
    f = lambda *s: torch.empty(*s, device=dev)
    w["loc_k"], w["loc_b"], w["loc_kt"] = f(KS, A), f(A), f(A, 36)
    lib.call("mstts_lsa_fold_location", lib.ptr(w["conv_k"]), lib.ptr(w["conv_b"]), lib.ptr(w["dense_k"]), lib.ptr(w["loc_k"]), lib.ptr(w["loc_b"]), KS, CH, A)
    lib.call("mstts_lsa_filter_by_unit", lib.ptr(w["loc_k"]), lib.ptr(w["loc_kt"]), KS, A)
    w["fused_cells"] = bool(L.mstts_cell_fwd_supported(H, M + H)) and bool(L.mstts_cell_fwd_supported(H, 2 * H))
    w["w0p"] = w["w1p"] = None
    if w["fused_cells"]:
        w["w0p"], w["w1p"] = f((M + H) * 4 * H), f(2 * H * 4 * H)
        lib.call("mstts_pack_cell_fwd", lib.ptr(w["w0f"]), 4 * H, lib.ptr(w["w0p"]), M + H, H)
        lib.call("mstts_pack_cell_fwd", lib.ptr(w["w1"]), 4 * H, lib.ptr(w["w1p"]), 2 * H, H)
    w["bwd_splits"] = (int(L.mstts_skinny_bwd_splits(M + H, 4 * H)), int(L.mstts_skinny_bwd_splits(2 * H, 4 * H)), int(L.mstts_skinny_bwd_splits(H, A)))
    for k, src, ld, rows, cols, sp in (("w0f_bp", "w0f", 4 * H, M + H, 4 * H, w["bwd_splits"][0]), ("w1_bp", "w1", 4 * H, 2 * H, 4 * H, w["bwd_splits"][1]),
                                       ("wq_bp", "wq", A, H, A, w["bwd_splits"][2])):
        w[k] = None
        if sp > 0 and rows % 32 == 0:
            w[k] = f(rows * cols)
            lib.call("mstts_pack_skinny_bwd", lib.ptr(w[src]), ld, lib.ptr(w[k]), rows, cols, sp)
    w["wq_t"] = f(A * H)
    lib.call("mstts_transpose01", lib.ptr(w["wq"]), lib.ptr(w["wq_t"]), H, A // 4, 4)
    w["persist"] = bool(L.mstts_persist_fwd_supported(1, H, M, A, 1, KS))
    w["persist_bwd"] = w["persist"] and bool(L.mstts_persist_bwd_supported(1, H, M, A, 1, KS))
    if w["persist"]:
        w["pk"] = [f(int(L.mstts_persist_pack_floats(i))) for i in range(3)]
        lib.call("mstts_persist_pack", lib.ptr(w["w0f"]), lib.ptr(w["w1"]), lib.ptr(w["wq"]), lib.ptr(w["wx0"]), *(lib.ptr(t) for t in w["pk"]))
    if w["persist_bwd"]:
        w["pkb"] = [f(int(L.mstts_persist_bwd_pack_floats(i))) for i in range(3)]
        lib.call("mstts_persist_bwd_pack", lib.ptr(w["w0f"]), lib.ptr(w["w1"]), lib.ptr(w["wq"]), *(lib.ptr(t) for t in w["pkb"]))
    torch.cuda.synchronize()
    if bf16:
        _bf16_copies(dev, w, widths)
    cache[widths] = w
    return w


def _upload(dev, cd):
    return {k: cd[k].to(dev).contiguous() for k in ("keys", "values", "lens", "xw0", "pre", "d_pj") + R.MASKS}


def _fwd_desc(dev, cd, w, u, tier, packed=False, bf16=None):
    """A forward descriptor with output buffers of its own.  tier: "full" (every derived copy engine.py passes), "nulled", "persistent" (the
    launch-per-step path's packed blocks and workspaces are not touched: none given).  Buffers written in full are NaN-filled; in1's slot S
    has no m0 half and, in the packed persistent form, c0 / c1 have no slot S (decoder_loop_ref.exclude_unwritten): zeroed, as engine.py does.
    bf16 (w from _weights(bf16=True)): "products" = the six bf_* copies, "full" = also the packed bf16 cell kernels where there are any."""
    B, T, S, H, M, P = cd["B"], cd["Te"], cd["S"], cd["H"], cd["M"], cd["P"]
    L = lib.load()
    t = dict(in0=_nan(dev, S + 1, B, M + H), in1=_nan(dev, S + 1, B, 2 * H), pj=_nan(dev, S, B, H + M), c0=_nan(dev, S + 1, B, H), c1=_nan(dev, S + 1, B, H),
             acts0=_nan(dev, S, B, 4 * H), acts1=_nan(dev, S, B, 4 * H), craw0=_nan(dev, S, B, H), craw1=_nan(dev, S, B, H),
             q_hist=_nan(dev, S, B, A), align_hist=_nan(dev, S, B, T), cum_hist=_nan(dev, S + 1, B, T))
    t["in1"][S, :, :H] = 0.0
    if packed:
        t["c0"][S] = 0.0
        t["c1"][S] = 0.0
    d = lib.DecoderTrain()
    d.B, d.S, d.H, d.P = B, S, H, P
    ls = d.lsa
    ls.B, ls.T, ls.A, ls.M, ls.KS, ls.CH = B, T, A, M, KS, CH
    ls.keys, ls.values, ls.lengths = lib.ptr(u["keys"]), lib.ptr(u["values"]), lib.ptr(u["lens"])
    for k in R.LSA_NAMES + ("loc_k", "loc_b"):
        setattr(ls, k, lib.ptr(w[k]))
    ls.loc_kt = lib.ptr(w["loc_kt"]) if tier != "nulled" else None
    d.xw0, d.w0f, d.w1, d.b1, d.wq = lib.ptr(u["xw0"]), lib.ptr(w["w0f"]), lib.ptr(w["w1"]), lib.ptr(w["b1"]), lib.ptr(w["wq"])
    d.zc0, d.zh0, d.zc1, d.zh1 = (lib.ptr(u[k]) for k in R.MASKS)
    d.zoneout = R.RATE
    for k in FWD_BUFS:
        setattr(d, k, lib.ptr(t[k]))
    d.chains = 1
    if tier != "persistent":
        ng, nq = C.c_int64(0), C.c_int64(0)
        L.mstts_decoder_train_ws_floats(B, H, M, A, C.byref(ng), C.byref(nq))
        t["energy_ws_floats"] = max(int(L.mstts_lsa_step_q_ws_bytes(B, T)) // 4 + 2, 2 * B * T + 2)
        t["gates_ws"], t["energy_ws"], t["q_ws"] = _zeros(dev, ng.value), _zeros(dev, t["energy_ws_floats"]), _zeros(dev, nq.value)
        d.gates_ws, d.energy_ws, d.q_ws = lib.ptr(t["gates_ws"]), lib.ptr(t["energy_ws"]), lib.ptr(t["q_ws"])
        d.energy_ws_floats = t["energy_ws_floats"]
    if tier == "full":
        d.w0f_bp, d.w1_bp, d.wq_bp, d.wq_t = lib.ptr(w["w0f_bp"]), lib.ptr(w["w1_bp"]), lib.ptr(w["wq_bp"]), lib.ptr(w["wq_t"])
        if w["fused_cells"]:
            t["act_p"] = _zeros(dev, 2 * int(L.mstts_cell_act_floats(B, M + H) + L.mstts_cell_act_floats(B, 2 * H)))
            d.w0p, d.w1p, d.act_p = lib.ptr(w["w0p"]), lib.ptr(w["w1p"]), lib.ptr(t["act_p"])
    if tier == "nulled":
        assert not any(getattr(d, k) for k in NULLED) and not d.lsa.loc_kt
    if bf16:
        for k in BF_COPIES:
            setattr(d, "bf_" + k, lib.ptr(w["bf"][k]))
        if bf16 == "full" and w["w0p16"] is not None:
            d.w0p16, d.w1p16 = lib.ptr(w["w0p16"]), lib.ptr(w["w1p16"])
    return d, t


def _bwd_desc(dev, cd, u, fwd, persistent):
    """A BPTT descriptor with NaN-filled outputs of its own and its own copy of d_pj.  dq_hist is zeroed for mstts_decoder_train_bwd, as
    include/mstts.h demands; the persistent launch needs no pre-zeroing."""
    B, T, S, H, M = cd["B"], cd["Te"], cd["S"], cd["H"], cd["M"]
    L = lib.load()
    parts = int(L.mstts_decoder_train_bwd_parts(H, M))
    t = dict(d_pj=u["d_pj"].clone(), dg0=_nan(dev, S, B, 4 * H), dg1=_nan(dev, S, B, 4 * H), de_hist=_nan(dev, S, B, T),
             dq_hist=_nan(dev, S, B, A) if persistent else torch.zeros(S, B, A, device=dev), d_in0=_nan(dev, parts, S, B, M + H),
             ws=_zeros(dev, L.mstts_decoder_train_bwd_ws_floats(B, H, M, A, T, CH)), parts=parts)
    b = lib.DecoderTrainBwd()
    b.fwd = C.pointer(fwd)
    b.d_pj, b.dg0, b.dg1, b.dq_hist, b.de_hist, b.d_in0, b.ws = (lib.ptr(t[k]) for k in ("d_pj", "dg0", "dg1", "dq_hist", "de_hist", "d_in0", "ws"))
    return b, t


def _collect(cd, u, f, b=None, persistent=False):
    """The compared quantities as numpy arrays; d_in0's slabs summed in fp64, d_ctx = its context columns of slots 1 .. S-1 (the persistent BPTT:
    its first slab's), the host-formed gradients from them."""
    M = cd["M"]
    got = {k: t2n(f[k]) for k in FWD_BUFS}
    notes = []
    if b is None:
        return got, notes
    for k in ("dg0", "dg1", "dq_hist", "de_hist"):
        got[k] = t2n(b[k])
    slabs = t2n(b["d_in0"]).astype(np.float64)
    if persistent:
        got["d_ctx"] = slabs[0, 1:, :, :M]
    else:
        got["d_in0"] = slabs.sum(0)
        got["d_ctx"] = got["d_in0"][1:, :, :M]
    if not torch.equal(b["d_pj"], u["d_pj"]):
        notes.append("d_pj is not bit-identical after the BPTT")
    got.update(R.host_grads(cd, got))
    return got, notes


def _judge(name, label, ref_form, got, notes, quantities, failures, packed=False):
    cd = R.case_data(name)
    for k in quantities:
        if not np.isfinite(got[k]).all():
            failures.append((label, k, "not finite: a buffer the form writes in full kept its NaN fill"))
    for msg in notes + R.exact_failures(cd, got):
        failures.append((label, msg))
    rows = R.judge(name, ref_form, got, quantities, packed=packed)
    print("%-15s %-28s %s" % (name, label, "  ".join("%s %.1e/%.1e%s" % (k, err, e32, "" if err <= bound else " FAIL") for k, e32, err, bound in rows)))
    ref, r32 = R.evaluations(name, ref_form)
    own = ["%s %.1e/%.1e" % (k, R.slice_err(got[k], ref[k]).max(), R.slice_err(r32[k], ref[k]).max()) for k in R.TERM_SCALED if k in quantities]
    if own:
        print("%-15s %-28s on the rows' own scale (reported, not judged: decoder_loop_ref.TERM_SCALED): %s" % (name, label, "  ".join(own)))
    for k, e32, err, bound in rows:
        if not err <= bound:
            failures.append((label, k, "err %.3e" % err, "e32 %.3e" % e32, "bound %.3e" % bound))


def _assert_tier(cd, w, full):
    """The full descriptor really selects the tier the case is there for - else the case would judge another path under its name."""
    L = lib.load()
    B, T, H, M = cd["B"], cd["Te"], cd["H"], cd["M"]
    widths = cd["widths"]
    if widths == "defaults":
        assert not w["fused_cells"] and not full.act_p and L.mstts_skinny_fwd_splits(4 * H, M + H) == 0          # product + pointwise launches, tiled GEMM for cell 0
        assert w["bwd_splits"] == (1, 1, 1) and L.mstts_decoder_train_bwd_parts(H, M) == 1                         # one-slab backward products
        assert L.mstts_lsa_step_q_supported(T, M, H) == 0
        return
    assert w["fused_cells"] and M % 4 == 0 and full.act_p and full.w0p and full.w1p and full.w0f_bp and full.w1_bp and full.wq_bp
    assert min(w["bwd_splits"]) >= 1
    assert min(L.mstts_skinny_fwd_splits(4 * H, M + H), L.mstts_skinny_fwd_splits(4 * H, 2 * H), L.mstts_skinny_fwd_splits(A, H)) >= 1
    assert L.mstts_lsa_step_q_supported(T, M, H) == int(widths == "WIDE")
    if widths == "WIDE":
        assert full.lsa.loc_kt and full.energy_ws_floats >= L.mstts_lsa_step_q_ws_bytes(B, T) // 4                  # fused query
        assert full.wq_t and H % 128 == 0 and w["bwd_splits"][1] in (1, 2, 4, 8) and B * H * 4 < 1 << 30            # fused query gradient
        assert (H + M) % 4 == 0 and H % 4 == 0 and L.mstts_decoder_train_bwd_parts(H, M) > 1                        # several d_in0 slabs
    else:
        assert L.mstts_decoder_train_bwd_parts(H, M) == 2


@pytest.mark.parametrize("name", list(R.CASES))
def test_launch_per_step_forms_against_the_oracle(dev, wcache, name):
    cd = R.case_data(name)
    w, u = _weights(dev, wcache, cd["widths"]), _upload(dev, cd)
    failures = []
    for tier in ("full", "nulled"):
        d, f = _fwd_desc(dev, cd, w, u, tier)
        if tier == "full":
            _assert_tier(cd, w, d)
        b, g = _bwd_desc(dev, cd, u, d, persistent=False)
        lib.call("mstts_decoder_train_fwd", C.byref(d))
        lib.call("mstts_decoder_train_bwd", C.byref(b))
        torch.cuda.synchronize()
        got, notes = _collect(cd, u, f, g)
        _judge(name, "launch-per-step, " + tier, "xw0", got, notes, LPS_Q, failures)
    assert not failures, failures


def _pdesc(dev, packs, xch_bytes, recurrent_bf16=0):
    """A persistent-launch descriptor with an exchange buffer and control words of its own; opk / pre / b0 are the caller's to set."""
    t = dict(xch=_zeros(dev, xch_bytes // 4), ctrl=torch.zeros(272, dtype=torch.int32, device=dev))
    p = lib.PersistDesc()
    p.w0pk, p.w1pk, p.wqpk, p.xch, p.ctrl = lib.ptr(packs[0]), lib.ptr(packs[1]), lib.ptr(packs[2]), lib.ptr(t["xch"]), lib.ptr(t["ctrl"])
    p.stamps, p.opk, p.pre, p.b0 = None, None, None, None
    p.selftest_fail_step, p.near_xcd, p.recurrent_bf16 = 0, near_xcd(), recurrent_bf16
    return p, t


def _ran_to_its_end(t, what):
    torch.cuda.synchronize()
    c = t["ctrl"].cpu().numpy()
    assert c[1] == 0 and c[2] == 256, (what, c[:4])


@pytest.mark.parametrize("name", [n for n in R.CASES if R.CASES[n]["widths"] == "WIDE"])
def test_persistent_forms_against_the_oracle(dev, wcache, name):
    cd = R.case_data(name)
    B, T, S, H, M = cd["B"], cd["Te"], cd["S"], cd["H"], cd["M"]
    L = lib.load()
    if not L.mstts_persist_fwd_supported(B, H, M, A, T, KS):
        pytest.skip("persistent loop not available on this device (needs 256 CUs and one workgroup per CU)")
    w, u = _weights(dev, wcache, cd["widths"]), _upload(dev, cd)
    failures = []
    pdesc = lambda packs, xch_bytes: _pdesc(dev, packs, xch_bytes)
    ran_to_its_end = _ran_to_its_end
    # ---- forward reading xw0, row-major histories
    d, f = _fwd_desc(dev, cd, w, u, "persistent")
    p, pt = pdesc(w["pk"], int(L.mstts_persist_fwd_ws_bytes()))
    lib.call("mstts_decoder_train_fwd_persistent", C.byref(d), C.byref(p))
    ran_to_its_end(pt, "forward, xw0")
    got, notes = _collect(cd, u, f)
    _judge(name, "persistent fwd, xw0", "xw0", got, notes, R.FORWARD_Q, failures)
    # ---- forward forming the prenet rows' product itself, cell operands packed; xw0 is ignored in this form: it points at NaN
    d, f = _fwd_desc(dev, cd, w, u, "persistent", packed=True)
    f["xw0_unused"] = _nan(dev, S, B, 4 * H)
    d.xw0 = lib.ptr(f["xw0_unused"])
    p, pt = pdesc(w["pk"], int(L.mstts_persist_fwd_ws_bytes()))
    opk = _nan(dev, int(L.mstts_persist_opk_floats(S)))
    p.opk, p.pre, p.b0 = lib.ptr(opk), lib.ptr(u["pre"]), lib.ptr(w["b0"])
    lib.call("mstts_decoder_train_fwd_persistent", C.byref(d), C.byref(p))
    ran_to_its_end(pt, "forward, pre + opk")
    bwd = w["persist_bwd"] and bool(L.mstts_persist_bwd_supported(B, H, M, A, T, KS))
    g = None
    if bwd:
        b, g = _bwd_desc(dev, cd, u, d, persistent=True)
        pb, pbt = pdesc(w["pkb"], int(L.mstts_persist_bwd_ws_bytes()))
        pb.opk = lib.ptr(opk)
        lib.call("mstts_decoder_train_bwd_persistent", C.byref(b), C.byref(pb))
        ran_to_its_end(pbt, "BPTT")
    lib.call("mstts_persist_unpack_history", lib.ptr(opk), C.byref(d))
    torch.cuda.synchronize()
    got, notes = _collect(cd, u, f, g, persistent=True)
    _judge(name, "persistent fwd, pre + opk" + (" + BPTT" if bwd else ""), "pre", got, notes, R.FORWARD_Q + (PERSIST_BWD_Q if bwd else ()), failures, packed=True)
    assert not failures, failures
