"""The sequence-LSTM drivers and their BPTT against oracle.model.run_lstm in fp64 (tests/lstm_seq_ref.py), every form on its own - never one
form against another: the launch-per-step drivers mstts_lstm_seq_fwd (product + pointwise launches, and the fused steps wh_p / h_p),
mstts_lstm_seq_fwd_pair, mstts_lstm_seq_bwd, mstts_lstm_seq_bwd_pair, and where the shape admits them the persistent launches
(mstts_lstm_seq_{fwd,bwd}_pair_persistent, mstts_lstm_seq_{fwd,bwd}_persistent).  This is the base the "A equals B" comparisons of
test_gpu_persist_lstm.py and test_gpu_ops.py::test_lstm_seq_fused_and_pair_forms stand on.

Cases (tests/lstm_seq_ref.py CASES), the smallest that reach each path:
  single_step    (1,1,64)     one step: the d_h slabs are absent at t == T - 1 only, which is the only step
  fused_h64      (5,9,64)     fused steps available; H % 128 != 0: pointwise kernels without the row-per-block grid; every row but row 0
                              shorter than T - 1: the state gradient crosses several dead steps
  unfused_h24    (7,5,24)     no fused steps, no K-split forward product (H % 32 != 0): tiled GEMM forward, one-slab skinny product backward
  pair_h256      (32,12,256)  reference width: persistent pair, split products (several d_h slabs)
  groups_h256    (33,6,256)   single sequences, both directions: two row groups of the persistent single-sequence launch
  residual_h256  (7,5,256)    residual wrapper (product + pointwise launches only): d_x = dgates_pos . Wx^T + d_out, dWx, bias gradient
  inference_h64  (5,9,64)     training = False, NULL masks (state' = 0.9 new + 0.1 old)
  no_lengths_h64 (5,9,64)     lengths = NULL, reverse = 0
Row 0 has length T, row 1 length 1; both directions; uint8 keep-masks at rate 0.1 in processing order.

Compared per (row, step) slice on the slice's own scale: out at the caller's strides (BiLSTM layout: both directions into one [B,T,2H]
buffer), c_hist[1:], h_hist[1:], acts, c_raw, dgates_step, dgates_pos, and - formed on the host in fp64 from the returned tensors, no GEMM
kernel - dWh = sum_t h_hist[t]^T . dgates_step[t], the bias gradient, and in the residual case dWx and d_x.  Exactly 0: out and dgates_pos
past a row's length, dgates_step rows of dead steps.  Slot T of the histories = the state after the row's own last live step, bit for bit.

Bound per quantity: MARGIN (8) x e32, e32 = the worst slice error of the same oracle function evaluated in float32 on the CPU; floor 1e-6.
Measured on an MI355X, worst over forms and directions, in units of 1e-7, e32 -> kernel:
  case            out       c_hist    h_hist    acts      c_raw     dgs       dgp       dwh       db        dx        dwx
  single_step     1.3->1.3  1.2->1.2  1.3->1.5  0.7->1.0  0.8->1.4  1.6->0.8  1.6->0.8  0 -> 0    1.6->0.8
  fused_h64       3.3->2.6  2.4->2.4  2.9->3.0  3.1->1.3  2.5->2.3  3.3->2.3  3.3->2.3  5.3->5.6  2.0->1.4
  unfused_h24     3.9->2.9  2.1->2.6  2.4->3.4  1.9->1.5  1.9->2.6  4.7->2.8  4.7->2.8  4.9->3.7  2.1->1.9
  pair_h256       2.8->3.5  2.5->2.9  3.0->3.5  3.0->2.1  2.4->2.9  3.4->4.7  3.4->4.7  3.8->3.8  1.7->1.4
  groups_h256     3.1->3.0  2.1->2.8  2.9->3.6  2.7->2.0  1.9->2.8  3.3->2.8  3.3->2.8  3.8->4.5  1.3->1.3
  residual_h256   1.5->0.8  8.0->2.2  10.->2.6  14.->1.5  8.0->2.1  10.->2.6  10.->2.6  16.->4.2  3.2->1.6  2.1->0.6  8.7->3.5
  inference_h64   2.5->2.6  2.1->2.5  2.9->2.6  1.9->1.4  2.2->2.5  4.8->3.5  4.8->3.5  4.8->4.5  1.6->1.8
  no_lengths_h64  3.0->3.2  2.1->2.2  2.6->3.3  3.3->1.5  2.2->2.1  2.5->7.6  2.5->7.6  4.8->3.6  1.2->1.0
No form needs more than 3.0 x e32 of its own direction (dgates of no_lengths_h64, product + pointwise launches); the worst error / bound is
0.38.  dWh of single_step is identically 0 (the state before the only step is 0) and is held to exact zeros.  residual_h256's e32 is larger
because the float32 oracle also forms x . Wx in float32, while the driver receives that product formed in fp64 and rounded once.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from multi_speaker_tts_amd import lib
from tests import lstm_seq_ref as R
from tests.helpers import t2n
from tests.test_gpu_persist_lstm import H as PERSIST_H, _run_bwd, _run_fwd      # they build buffers / descriptors with that file's _fwd_bufs / _fwd_descs

pytestmark = pytest.mark.gpu
DIRN = ("fw", "bw")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _nan(dev, *s):
    return torch.full(s, float("nan"), device=dev)


def _upload(dev, cd):
    """The case on the device.  BiLSTM layout: out / d_out are [B, T, 2H] with direction d at column d * H."""
    B, T, H, dirs = cd["B"], cd["T"], cd["H"], cd["dirs"]
    up = lambda t: None if t is None else t.to(dev).contiguous()
    u = {k: {d: up(cd[k][d]) for d in dirs} for k in ("wh", "xw", "zc", "zh")}
    u["lens"] = up(cd["lens"])
    u["x"] = {d: up(cd["x"].get(d)) for d in dirs}
    W = len(dirs) * H if cd["layout"] == "bilstm" else H
    u["W"] = W
    if cd["layout"] == "bilstm":
        u["dout_all"] = torch.cat([cd["dout"][d] for d in dirs], dim=2).to(dev).contiguous()
        u["dout"] = {d: (u["dout_all"], d * H) for d in dirs}
    else:
        u["dout"] = {d: (up(cd["dout"][d]), 0) for d in dirs}
    return u


def _fwd_desc(dev, cd, u, d, out, col, fused):
    """One direction's forward descriptor with fresh NaN-filled histories; returns (descriptor, tensors)."""
    B, T, H = cd["B"], cd["T"], cd["H"]
    L = lib.load()
    t = dict(c_hist=_nan(dev, T + 1, B, H), h_hist=_nan(dev, T + 1, B, H), acts=_nan(dev, T, B, 4 * H), c_raw=_nan(dev, T, B, H),
             gates=torch.empty(int(L.mstts_lstm_seq_ws_floats(B, H, 0)), device=dev), out=out, col=col)
    q = lib.LstmSeqFwd()
    q.B, q.T, q.H = B, T, H
    q.xw, q.wh, q.wh_ld = lib.ptr(u["xw"][d]), lib.ptr(u["wh"][d]), 4 * H
    q.lengths, q.reverse, q.zoneout = lib.ptr(u["lens"]), d, R.RATE
    q.zc, q.zh = lib.ptr(u["zc"][d]), lib.ptr(u["zh"][d])
    q.residual = lib.ptr(u["x"][d]) if cd["residual"] else None
    q.out, q.out_sb, q.out_st = lib.ptr(out, col), T * u["W"], u["W"]
    q.c_hist, q.h_hist, q.acts, q.c_raw, q.gates_ws = lib.ptr(t["c_hist"]), lib.ptr(t["h_hist"]), lib.ptr(t["acts"]), lib.ptr(t["c_raw"]), lib.ptr(t["gates"])
    if fused:
        t["whp"] = torch.empty(H * 4 * H, device=dev)
        lib.call("mstts_pack_cell_fwd", lib.ptr(u["wh"][d]), 4 * H, lib.ptr(t["whp"]), H, H)
        t["hp"] = torch.empty(2 * int(L.mstts_cell_act_floats(B, H)), device=dev)
        q.wh_p, q.h_p = lib.ptr(t["whp"]), lib.ptr(t["hp"])
    return q, t


def _bwd_desc(dev, cd, u, d, f):
    B, T, H = cd["B"], cd["T"], cd["H"]
    L = lib.load()
    t = dict(dgs=_nan(dev, T, B, 4 * H), dgp=_nan(dev, B, T, 4 * H), ws=torch.empty(int(L.mstts_lstm_seq_ws_floats(B, H, 1)), device=dev))
    q = lib.LstmSeqBwd()
    q.B, q.T, q.H = B, T, H
    q.wh, q.wh_ld, q.lengths, q.reverse, q.zoneout = lib.ptr(u["wh"][d]), 4 * H, lib.ptr(u["lens"]), d, R.RATE
    q.zc, q.zh = lib.ptr(u["zc"][d]), lib.ptr(u["zh"][d])
    dout, col = u["dout"][d]
    q.d_out, q.dout_sb, q.dout_st = lib.ptr(dout, col), T * u["W"], u["W"]
    q.c_hist, q.acts, q.c_raw = lib.ptr(f["c_hist"]), lib.ptr(f["acts"]), lib.ptr(f["c_raw"])
    q.dgates_step, q.dgates_pos, q.ws = lib.ptr(t["dgs"]), lib.ptr(t["dgp"]), lib.ptr(t["ws"])
    return q, t


def _collect(cd, d, f, b):
    H = cd["H"]
    got = {k: t2n(f[k]) for k in ("c_hist", "h_hist", "acts", "c_raw")}
    got["out"] = t2n(f["out"])[:, :, f["col"]:f["col"] + H]
    got["dgs"], got["dgp"] = t2n(b["dgs"]), t2n(b["dgp"])
    return got


def _launch_per_step(dev, cd, u, fwd, bwd):
    """fwd: 'plain' (product + pointwise launches), 'fused' (wh_p / h_p, one sequence per call), 'pair' (mstts_lstm_seq_fwd_pair, fused where
    the shape has fused steps); bwd: 'single' / 'pair'.  Every run has its own NaN-filled buffers."""
    B, T, H, dirs = cd["B"], cd["T"], cd["H"], cd["dirs"]
    shared = _nan(dev, B, T, u["W"]) if cd["layout"] == "bilstm" else None
    fused = fwd != "plain" and lib.load().mstts_cell_fwd_supported(H, H) == 1 and not cd["residual"]
    fd = {d: _fwd_desc(dev, cd, u, d, shared if shared is not None else _nan(dev, B, T, H), d * H if shared is not None else 0, fused) for d in dirs}
    if fwd == "pair":
        lib.call("mstts_lstm_seq_fwd_pair", C.byref(fd[0][0]), C.byref(fd[1][0]))
    else:
        for d in dirs:
            lib.call("mstts_lstm_seq_fwd", C.byref(fd[d][0]))
    bd = {d: _bwd_desc(dev, cd, u, d, fd[d][1]) for d in dirs}
    if bwd == "pair":
        lib.call("mstts_lstm_seq_bwd_pair", C.byref(bd[0][0]), C.byref(bd[1][0]))
    else:
        for d in dirs:
            lib.call("mstts_lstm_seq_bwd", C.byref(bd[d][0]))
    torch.cuda.synchronize()
    return {d: _collect(cd, d, fd[d][1], bd[d][1]) for d in dirs}


def _persistent_pair(dev, cd, u):
    """mstts_lstm_seq_{fwd,bwd}_pair_persistent through test_gpu_persist_lstm.py's descriptor / buffer builders (which also assert that the
    launches ran to their end), on this case's inputs."""
    B, T, H = cd["B"], cd["T"], cd["H"]
    st = {"B": B, "T": T, "lens": u["lens"], "zoneout": R.RATE}
    for d in cd["dirs"]:
        for k in ("wh", "xw", "zc", "zh"):
            st[k + "_" + DIRN[d]] = u[k][d]
        st["dout_" + DIRN[d]] = cd["dout"][d].to(dev).contiguous()
    o = _run_fwd(dev, st, True)
    r = _run_bwd(dev, st, o, True)
    res = {}
    for d in cd["dirs"]:
        n = DIRN[d]
        f = dict(c_hist=o["c_" + n], h_hist=o["h_" + n], acts=o["acts_" + n], c_raw=o["craw_" + n], out=o["out"], col=d * H)
        res[d] = _collect(cd, d, f, dict(dgs=r["dgs_" + n], dgp=r["dgp_" + n]))
    return res


def _persistent_single(dev, cd, u):
    """mstts_lstm_seq_{fwd,bwd}_persistent, one call per direction (a direction is a sequence of its own here), as
    test_gpu_persist_lstm.py::test_persistent_single_sequence_row_groups drives them: a launch that did not run to its end fails the test."""
    B, T, H = cd["B"], cd["T"], cd["H"]
    L = lib.load()
    groups = (B + 31) // 32
    res = {}
    for d in cd["dirs"]:
        q, f = _fwd_desc(dev, cd, u, d, _nan(dev, B, T, H), 0, False)
        qb, b = _bwd_desc(dev, cd, u, d, f)
        n = L.mstts_persist_lstm_pack_floats()
        pk, pkt = torch.empty(n, device=dev), torch.empty(n, device=dev)
        lib.call("mstts_persist_lstm_pack", lib.ptr(u["wh"][d]), 4 * H, lib.ptr(pk), lib.ptr(pkt))
        xch = torch.empty(L.mstts_persist_lstm_ws_bytes_n(B, 1) // 4, device=dev)
        ctrl = torch.zeros(16, dtype=torch.int32, device=dev)
        hist = torch.empty(L.mstts_persist_lstm_hist_floats_n(T, B, 1), device=dev)
        bws = torch.empty(L.mstts_persist_lstm_bwd_floats_n(T, B, 1), device=dev)
        lib.call("mstts_lstm_seq_fwd_persistent", C.byref(q), lib.ptr(pk), lib.ptr(xch), lib.ptr(ctrl), lib.ptr(hist))
        torch.cuda.synchronize()
        c = ctrl.cpu().numpy()
        assert c[1] == 0 and c[2] == 32 * groups, c[:4]
        lib.call("mstts_lstm_seq_bwd_persistent", C.byref(qb), lib.ptr(pkt), lib.ptr(xch), lib.ptr(ctrl), lib.ptr(hist), lib.ptr(bws))
        torch.cuda.synchronize()
        c = ctrl.cpu().numpy()
        assert c[1] == 0 and c[2] == 16 * groups, c[:4]
        res[d] = _collect(cd, d, f, b)
    return res


def _runs(dev, cd, u):
    """(name, results per direction) of every form the case's shape admits."""
    L = lib.load()
    B, H = cd["B"], cd["H"]
    fusable = L.mstts_cell_fwd_supported(H, H) == 1 and not cd["residual"]
    yield "plain fwd + single bwd", _launch_per_step(dev, cd, u, "plain", "single")
    if cd["layout"] == "bilstm":
        if fusable:
            yield "fused fwd + pair bwd", _launch_per_step(dev, cd, u, "fused", "pair")
        yield "pair fwd + pair bwd", _launch_per_step(dev, cd, u, "pair", "pair")
        if cd["training"] and H == PERSIST_H and L.mstts_persist_lstm_supported(B, H):
            yield "persistent pair", _persistent_pair(dev, cd, u)
    else:
        if fusable:
            yield "fused fwd + single bwd", _launch_per_step(dev, cd, u, "fused", "single")
        if cd["training"] and not cd["residual"] and cd["lens"] is not None and L.mstts_persist_lstm_supported_n(B, H, 1):
            yield "persistent single", _persistent_single(dev, cd, u)


@pytest.mark.parametrize("name", list(R.CASES))
def test_every_form_against_run_lstm(dev, name):
    cd = R.case_data(name)
    T = cd["T"]
    u = _upload(dev, cd)
    lens = R.live_mask(cd).sum(1)
    failures, forms = [], []
    for form, res in _runs(dev, cd, u):
        forms.append(form)
        for d in cd["dirs"]:
            ref, e32, bound = R.reference(name, d)
            got = dict(res[d])
            # slot 0 of the histories is the zero state the drivers write themselves
            if np.any(got["c_hist"][0] != 0.0) or np.any(got["h_hist"][0] != 0.0):
                failures.append((form, d, "slot 0 of the histories is not 0"))
            for k in ("c_hist", "h_hist"):
                full = got[k]
                if not all(np.array_equal(full[T, b], full[lens[b], b]) for b in range(cd["B"])):
                    failures.append((form, d, k + ": slot T is not the state after the row's last live step"))
            got.update(R.host_grads(cd, d, got["h_hist"], got["dgs"], got["dgp"]))
            got["c_hist"], got["h_hist"] = got["c_hist"][1:], got["h_hist"][1:]
            for k in R.dead_is_zero(cd, d, out=got["out"], dgs=got["dgs"], dgp=got["dgp"]):
                failures.append((form, d, k + ": not exactly 0 past a row's length"))
            for k in R.quantities(cd):
                err = float(R.slice_err(got[k], ref[k]).max())
                print("%-15s %-24s dir %d %-7s e32 %.2e  err %.2e  bound %.2e  (%.1f x e32)%s"
                      % (name, form, d, k, e32[k], err, bound[k], err / e32[k] if e32[k] else 0.0, "  FAIL" if not err <= bound[k] else ""))
                if not err <= bound[k]:
                    failures.append((form, d, k, err, bound[k]))
    expect = {"single_step": 3, "fused_h64": 3, "unfused_h24": 2, "residual_h256": 1, "inference_h64": 3, "no_lengths_h64": 2}
    if name in expect:
        assert len(forms) == expect[name], forms
    assert not failures, failures
