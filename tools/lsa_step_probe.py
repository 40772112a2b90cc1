"""Timing of the single-launch attention step: graph replay (frozen epoch = no waiting) and eager with fresh epochs."""
import ctypes as C, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from multi_speaker_tts_amd import lib
from tools.microbench import timeit
dev = torch.device("cuda:0")
B, T, M, A, CH, KS = 32, 128, 768, 128, 32, 31
rn = lambda *sh: torch.randn(*sh, device=dev)
keys, values = rn(B, T, A), rn(B, T, M)
conv_k, conv_b, dense_k, sw, sb = rn(KS, 1, CH) * .3, rn(CH) * .1, rn(CH, A) * .3, rn(A) * .5, rn(A) * .1
loc_k, loc_b = torch.zeros(KS, A, device=dev), torch.zeros(A, device=dev)
c = lib.LsaConst()
c.B, c.T, c.A, c.M, c.KS, c.CH = B, T, A, M, KS, CH
c.keys, c.values, c.lengths = lib.ptr(keys), lib.ptr(values), None
c.conv_k, c.conv_b, c.dense_k, c.score_w, c.score_b = lib.ptr(conv_k), lib.ptr(conv_b), lib.ptr(dense_k), lib.ptr(sw), lib.ptr(sb)
lib.call("mstts_lsa_fold_location", c.conv_k, c.conv_b, c.dense_k, lib.ptr(loc_k), lib.ptr(loc_b), KS, CH, A)
c.loc_k, c.loc_b = lib.ptr(loc_k), lib.ptr(loc_b)
q = rn(8, B, A); cum = torch.rand(B, T, device=dev); al = torch.zeros(B, T, device=dev); cn = torch.zeros(B, T, device=dev); cx = torch.zeros(B, M, device=dev)
en = torch.zeros(B, T, device=dev)
gran = torch.zeros(B * T + 1, dtype=torch.int64, device=dev)
ep = [0]
def step():
    ep[0] += 1
    lib.call("mstts_lsa_step_fwd", C.byref(c), lib.ptr(q), 8, B * A, None, lib.ptr(cum), lib.ptr(al), lib.ptr(cn), lib.ptr(cx), M, None, 0, None, lib.ptr(gran), ep[0])
def two():
    lib.call("mstts_lsa_energy_fwd", C.byref(c), lib.ptr(q), 8, B * A, None, lib.ptr(cum), lib.ptr(en))
    lib.call("mstts_lsa_context_fwd", C.byref(c), lib.ptr(en), lib.ptr(cum), lib.ptr(al), lib.ptr(cn), lib.ptr(cx), M, None, 0)
print("dbg=%s" % os.environ.get("MSTTS_LSA_STEP_DEBUG", "0"))
print("  fused, graph replay (frozen epoch): %.2f us" % timeit(step, 500, graph=True))
print("  fused, eager fresh epochs          : %.2f us" % timeit(step, 2000, graph=False))
print("  two launches, graph replay         : %.2f us" % timeit(two, 500, graph=True))
print("  two launches, eager                : %.2f us" % timeit(two, 2000, graph=False))
print("  time-outs:", int(gran[-1]))
# the other forms of the step kernel (graph replay), each on a granule buffer of its own, and the single-launch backward
L = lib.load()
H, NM, NP, PN = 1024, 80, 84, 256
loc_kt = torch.zeros(A, 36, device=dev)
lib.call("mstts_lsa_filter_by_unit", lib.ptr(loc_k), lib.ptr(loc_kt), KS, A)
cu = lib.LsaConst.from_buffer_copy(c)
cu.loc_kt = lib.ptr(loc_kt)
pj, wq = rn(B, H + M), rn(H, A) * .05
wp, bias = rn(H + M, NP) * .05, rn(NM + 1) * .1
wp_own = torch.zeros(int(L.mstts_lsa_proj_pack_floats()), device=dev)
lib.call("mstts_lsa_proj_pack", lib.ptr(wp), NP, H, NP, lib.ptr(wp_own))
vp = (values.reshape(B * T, M) @ wp[H:]).contiguous()
lin, stop, pre_out = torch.zeros(B, NM, device=dev), torch.zeros(B, device=dev), torch.zeros(B, PN, device=dev)
pw0, pb0, pw1, pb1 = rn(NM, PN) * .2, rn(PN) * .1, rn(PN, PN) * .1, rn(PN) * .1
pm0, pm1 = torch.ones(B, PN, dtype=torch.uint8, device=dev), torch.ones(B, PN, dtype=torch.uint8, device=dev)
pn = lib.LsaPrenet()
pn.w0, pn.b0, pn.w1, pn.b1, pn.m0, pn.m1 = lib.ptr(pw0), lib.ptr(pb0), lib.ptr(pw1), lib.ptr(pb1), lib.ptr(pm0), lib.ptr(pm1)
pn.inv_keep, pn.P, pn.out, pn.out_ld = 2.0, PN, lib.ptr(pre_out), PN
gran_u = torch.zeros(int(L.mstts_lsa_step_ws_bytes(B, T)) // 8, dtype=torch.int64, device=dev)
gran_q = torch.zeros(int(L.mstts_lsa_step_q_ws_bytes(B, T)) // 8, dtype=torch.int64, device=dev)
gran_p = torch.zeros(int(L.mstts_lsa_step_qp_ws_bytes(B, T)) // 8, dtype=torch.int64, device=dev)
def next_epoch():
    ep[0] += 1
    return ep[0]
def by_unit():
    lib.call("mstts_lsa_step_fwd", C.byref(cu), lib.ptr(q), 8, B * A, None, lib.ptr(cum), lib.ptr(al), lib.ptr(cn), lib.ptr(cx), M, None, 0, None, lib.ptr(gran_u), next_epoch())
def with_query():
    lib.call("mstts_lsa_step_fwd_q", C.byref(cu), lib.ptr(pj), H + M, lib.ptr(wq), H, 0, None, lib.ptr(cum), lib.ptr(al), lib.ptr(cn), lib.ptr(cx), M, None, 0, None,
             lib.ptr(gran_q), next_epoch(), -1)
def with_projection_prenet():
    lib.call("mstts_lsa_step_fwd_qp", C.byref(cu), lib.ptr(pj), H + M, lib.ptr(wq), H, lib.ptr(wp_own), lib.ptr(vp), lib.ptr(bias), NP, NM, lib.ptr(lin), lib.ptr(stop),
             lib.ptr(cum), lib.ptr(al), lib.ptr(cn), lib.ptr(cx), M, None, 0, None, C.byref(pn), lib.ptr(gran_p), next_epoch(), -1)
dctx, Gn, hn = rn(B, M), rn(B, T), rn(B, T, 32)
G, de, dq, hh = torch.zeros(B, T, device=dev), torch.zeros(B, T, device=dev), torch.zeros(B, A, device=dev), torch.zeros(B, T, 32, device=dev)
def bwd():
    lib.call("mstts_lsa_step_bwd", C.byref(c), lib.ptr(dctx), M, None, 0, 0, 0, lib.ptr(Gn), lib.ptr(hn), lib.ptr(G), lib.ptr(al), lib.ptr(q), lib.ptr(cum), lib.ptr(cx), M,
             lib.ptr(de), lib.ptr(dq), lib.ptr(hh))
print("  by-unit filter, graph replay       : %.2f us" % timeit(by_unit, 500, graph=True))
print("  + query, graph replay              : %.2f us" % timeit(with_query, 500, graph=True))
print("  + projection + prenet, graph replay: %.2f us" % timeit(with_projection_prenet, 500, graph=True))
print("  backward, single launch, graph     : %.2f us" % timeit(bwd, 500, graph=True))
print("  time-outs:", int(gran_u[B * T]) + int(gran_q[B * T]) + int(gran_p[B * T]))
