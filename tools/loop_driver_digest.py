"""SHA-256 of every output tensor of the launch-per-step loop drivers (csrc/decoder.hip) and the skinny products they launch, on seeded
inputs generated on the host: run it on two builds of the library and compare the lines.  Every tier of the drivers is reached by nulling
the optional derived-copy pointers of a descriptor copy; fp32 and bf16.  Tiled-GEMM tiers run inside lib.deterministic_gemm().
usage: python tools/loop_driver_digest.py [--dump out.npz]      (the dump holds the tensors, for a max-abs comparison of lines that differ)"""
import ctypes as C, hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
from helpers import dims_pair, to_dev
from oracle import model as OM, train as OT
from multi_speaker_tts_amd import inference, lib
from multi_speaker_tts_amd.engine import TrainEngine

dev, L_, OUT = torch.device("cuda:0"), lib.load(), {}
WIDE = dict(emb=64, enc_conv_ch=64, enc_lstm=256, spk=256, prenet=256, dec_lstm=1024, n_mel=16, post_ch=32)
HIST = ("in0", "in1", "pj", "c0", "c1", "acts0", "acts1", "craw0", "craw1", "q_hist", "align_hist", "cum_hist")


def put(name, t):
    torch.cuda.synchronize()
    OUT[name] = t.detach().cpu().numpy().copy()
    print("%s  %s" % (hashlib.sha256(OUT[name].tobytes()).hexdigest(), name), flush=True)


def host(shape, seed, scale=1.0):
    return torch.from_numpy(np.random.default_rng(seed).normal(0, scale, tuple(shape)).astype(np.float32)).to(dev)


def variant(desc, nulls):
    d = type(desc)()
    C.memmove(C.byref(d), C.byref(desc), C.sizeof(desc))
    for n in nulls:
        setattr(d.lsa if n == "loc_kt" else d, n, None)
    return d


def train(tag, dims, B, Te, L, **kw):
    pd, od = dims_pair(**dims)
    eng = TrainEngine(pd, device=dev, values=OM.init_params(od, 3), **kw)
    w = eng.plan(B, Te, L)
    w.persist = w.persist_bwd = False
    eng.forward(to_dev(OT.synthetic_batch(od, B, Te, L, seed=5, ragged=True), dev), w, seed=7)      # fills the descriptors and the derived copies
    eng.loss_and_backward(w)
    for i, k in enumerate(("xw0", "keys", "values", "d_pj")):                                      # ... whose inputs are then replaced
        getattr(w, k).copy_(host(getattr(w, k).shape, 100 + i, 0.3))
    for name, nulls in (("cells+query", ()), ("cells", ("loc_kt",)), ("query", ("act_p",)), ("products", ("act_p", "loc_kt"))):
        for k in HIST:
            getattr(w, k).zero_()
        lib.call("mstts_decoder_train_fwd", C.byref(variant(w.dec, nulls)))
        for k in HIST:
            put("train_fwd %s %s %s" % (tag, name, k), getattr(w, k))
    for name, nulls in (("packed+dq", ()), ("packed", ("wq_t",)), ("rowmajor", ("wq_t", "w0f_bp", "w1_bp", "wq_bp"))):
        dec, db = variant(w.dec, nulls), variant(w.dec_b, ())
        w.dq_hist.zero_()                                # (the attention backward adds into it)
        db.fwd = C.pointer(dec)
        lib.call("mstts_decoder_train_bwd", C.byref(db))
        for k in ("dg0", "dg1", "dq_hist", "de_hist", "d_in0"):
            put("train_bwd %s %s %s" % (tag, name, k), getattr(w, k))


def infer(B, Te, steps):
    pd, od = dims_pair(max_inf=steps - 1, dec_lstm=1024, prenet=256, enc_lstm=256, spk=256, n_mel=80)
    eng = inference.InferEngine(pd, device=dev, values=OM.init_params(od, 3))
    eng.persist_infer, seen, call = False, [], inference.call
    inference.call = lambda name, *a: (seen.append(a[0]._obj) if name == "mstts_decoder_infer_steps" else None, call(name, *a))[1]
    lengths = torch.tensor([Te] + [Te - 1 - b % 3 for b in range(B - 1)], dtype=torch.int32, device=dev)
    lin, stop, align, _ = eng.decode(host((B, Te, pd.mem), 1, 0.3), host((B, Te, pd.att), 2, 0.3), lengths, seed=9)
    inference.call = call
    for name, nulls in (("query+projection+prenet", ()), ("query", ("wp_own",)), ("cells", ("wp_own", "loc_kt")), ("products", ("w0sp",)), ("gemm", ("w0s",))):
        lib.call("mstts_decoder_infer_steps", C.byref(variant(seen[0], nulls)), 0, steps)
        for k, t in (("linear", lin), ("stop", stop), ("align", align)):
            put("infer %s %s" % (name, k), t[:steps])


def seq(B, T, H):
    lengths = torch.tensor([T] + [1 + (5 * b) % T for b in range(B - 1)], dtype=torch.int32, device=dev)
    def make(direction, fused):
        t = dict(xw=host((B, T, 4 * H), 10 + direction), wh=host((H, 4 * H), 20 + direction, H ** -0.5), out=torch.zeros(B, T, 2 * H, device=dev),
                 zc=torch.from_numpy(np.random.default_rng(30 + direction).integers(0, 2, (T, B, H)).astype(np.uint8)).to(dev),
                 zh=torch.from_numpy(np.random.default_rng(40 + direction).integers(0, 2, (T, B, H)).astype(np.uint8)).to(dev),
                 c=torch.zeros(T + 1, B, H, device=dev), h=torch.zeros(T + 1, B, H, device=dev), acts=torch.zeros(T, B, 4 * H, device=dev),
                 craw=torch.zeros(T, B, H, device=dev), ws=torch.zeros(int(L_.mstts_lstm_seq_ws_floats(B, H, 0)), device=dev), whp=torch.zeros(H * 4 * H, device=dev),
                 hp=torch.zeros(2 * int(L_.mstts_cell_act_floats(B, H)), device=dev), dout=host((B, T, 2 * H), 50 + direction),
                 dgs=torch.zeros(T, B, 4 * H, device=dev), dgp=torch.zeros(B, T, 4 * H, device=dev), bws=torch.zeros(int(L_.mstts_lstm_seq_ws_floats(B, H, 1)), device=dev))
        q, b, p = lib.LstmSeqFwd(), lib.LstmSeqBwd(), lib.ptr
        q.B, q.T, q.H, b.B, b.T, b.H = B, T, H, B, T, H
        q.xw, q.wh, q.wh_ld, q.lengths, q.reverse, q.zoneout, q.zc, q.zh = p(t["xw"]), p(t["wh"]), 4 * H, p(lengths), direction, 0.1, p(t["zc"]), p(t["zh"])
        q.out, q.out_sb, q.out_st = p(t["out"], direction * H), T * 2 * H, 2 * H
        q.c_hist, q.h_hist, q.acts, q.c_raw, q.gates_ws = p(t["c"]), p(t["h"]), p(t["acts"]), p(t["craw"]), p(t["ws"])
        if fused:
            lib.call("mstts_pack_cell_fwd", p(t["wh"]), 4 * H, p(t["whp"]), H, H)
            q.wh_p, q.h_p = p(t["whp"]), p(t["hp"])
        b.wh, b.wh_ld, b.lengths, b.reverse, b.zoneout, b.zc, b.zh = q.wh, 4 * H, q.lengths, direction, 0.1, q.zc, q.zh
        b.d_out, b.dout_sb, b.dout_st = p(t["dout"], direction * H), T * 2 * H, 2 * H
        b.c_hist, b.acts, b.c_raw, b.dgates_step, b.dgates_pos, b.ws = q.c_hist, q.acts, q.c_raw, p(t["dgs"]), p(t["dgp"]), p(t["bws"])
        return q, b, t
    for form in ("products", "fused", "pair"):
        (qa, ba, ta), (qb, bb, tb) = make(0, form != "products"), make(1, form != "products")
        if form == "pair":
            lib.call("mstts_lstm_seq_fwd_pair", C.byref(qa), C.byref(qb))
            lib.call("mstts_lstm_seq_bwd_pair", C.byref(ba), C.byref(bb))
        else:
            for q, b in ((qa, ba), (qb, bb)):
                lib.call("mstts_lstm_seq_fwd", C.byref(q))
                lib.call("mstts_lstm_seq_bwd", C.byref(b))
        for dr, t in (("fw", ta), ("bw", tb)):
            for k in ("out", "c", "h", "acts", "craw", "dgs", "dgp"):
                put("seq B%d H%d %s %s %s" % (B, H, form, dr, k), t[k])


def skinny(M, N, K):
    X, W, dG, dG2, W2, p = host((M, K), 1), host((K, N), 2, 0.05), host((M, N), 3), host((M, N), 4), host((K, N), 5, 0.05), lib.ptr
    ks, ns, ks16, ns16 = L_.mstts_skinny_fwd_splits(N, K), L_.mstts_skinny_bwd_splits(K, N), L_.mstts_skinny_bf16_fwd_splits(N, K), L_.mstts_skinny_bf16_bwd_splits(K, N)
    Pf, Pb, Wp, W16 = torch.zeros(16, M, N, device=dev), torch.zeros(2, 16, M, K, device=dev), torch.zeros(K * N, device=dev), torch.zeros(K * N, dtype=torch.int16, device=dev)
    tag = "skinny %dx%dx%d " % (M, N, K)
    lib.call("mstts_skinny_fwd", p(X), K, p(W), N, p(Pf), 0, M, N, K, ks); put(tag + "fwd", Pf[:ks])
    lib.call("mstts_skinny_bwd", p(dG), N, p(W), N, p(Pb), 0, M, K, N, ns); put(tag + "bwd", Pb[0, :ns])
    lib.call("mstts_skinny_bwd_pair", p(dG), p(dG2), N, p(W), p(W2), N, p(Pb[0]), p(Pb[1]), 0, M, K, N, ns); put(tag + "bwd_pair", Pb[:, :ns])
    lib.call("mstts_pack_skinny_bwd", p(W), N, p(Wp), K, N, ns)
    lib.call("mstts_skinny_bwd_packed", p(dG), N, p(Wp), p(Pb), 0, M, K, N, ns); put(tag + "bwd_packed", Pb[0, :ns])
    lib.call("mstts_pack_bf16_fwd", p(W), N, p(W16), K, N, ks16)
    lib.call("mstts_skinny_fwd_bf16", p(X), K, p(W16), p(Pf), 0, M, N, K, ks16); put(tag + "fwd_bf16", Pf[:ks16])
    lib.call("mstts_pack_bf16_bwd", p(W), N, p(W16), K, N, ns16)
    lib.call("mstts_skinny_bwd_bf16", p(dG), N, p(W16), p(Pb), 0, M, K, N, ns16); put(tag + "bwd_bf16", Pb[0, :ns16])


with lib.deterministic_gemm():
    for M, N, K in ((32, 4096, 1792), (17, 4096, 2048), (5, 128, 1024), (32, 256, 64)):
        skinny(M, N, K)
    seq(5, 9, 64)
    seq(32, 6, 256)
    train("wide", WIDE, 17, 40, 3)
    train("wide-bf16", WIDE, 17, 40, 3, recurrent_dtype="bf16", gemm_dtype="bf16")
    train("mid", dict(dec_lstm=64, enc_lstm=32, spk=64, prenet=32), 5, 18, 4)
    train("small", {}, 5, 18, 4)
    infer(17, 40, 4)
if "--dump" in sys.argv:
    np.savez(sys.argv[sys.argv.index("--dump") + 1], **OUT)
