"""SHA-256 of every output tensor of the Python engines (inference.InferEngine, taco1_trainer.Taco1TrainEngine,
speaker_trainer.SpeakerTrainEngine, engine.TrainEngine) on seeded inputs: run it on two trees that share a library and compare the
lines.  The InferEngine lines are taken with the persistent launches on ("persist") and off ("stepwise"); the `#` lines carry the
launch / fallback counters, so a line is compared only where both trees took the same path.  The trainers run inside
lib.deterministic_gemm(); their loss words and the auxiliary trainers' gradients are still summed with atomics, so those lines are
compared by max-abs difference over the dumps.  The "smoke" cases are the widths of __graft_entry__.smoke except spk_lstm, which is
set to spk (see SMOKE below); the "reference" cases are Dims().
usage: python tools/engine_digest.py [--dump out.npz] [--only 'infer smoke']      (the dump holds the tensors)"""
import argparse, hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
from helpers import to_dev
from oracle import model as OM, train as OT
from multi_speaker_tts_amd import lib
from multi_speaker_tts_amd.engine import TrainEngine
from multi_speaker_tts_amd.inference import InferEngine
from multi_speaker_tts_amd.params import Dims
from multi_speaker_tts_amd.speaker_trainer import SpeakerTrainEngine
from multi_speaker_tts_amd.taco1_trainer import Taco1TrainEngine

dev, OUT = torch.device("cuda:0"), {}
# the widths of __graft_entry__.smoke, but spk_lstm = spk: smoke() is handed its speaker embeddings and never runs the speaker stack, whose
# residual wrappers and layer-to-layer buffers hold ONE width (at spk_lstm = 16 under spk = 64 its second layer reads past its input)
SMOKE = dict(emb=32, enc_conv_ch=32, enc_lstm=32, spk=64, prenet=32, dec_lstm=64, n_mel=8, post_ch=16, bank_ch=8, proj1_ch=16, birnn=8, n_spec=20,
             spk_lstm=64)


def put(name, t):
    torch.cuda.synchronize()
    OUT[name] = (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).copy()
    print("%s  %s" % (hashlib.sha256(OUT[name].tobytes()).hexdigest(), name), flush=True)


def normal(g, shape):
    return np.clip(g.normal(0, 1.5, shape), -4, 4).astype(np.float32)


def infer(tag, cfg, B, Te, max_steps):
    pd, od = Dims(**cfg), OM.Dims(**cfg)
    values, g = OM.init_params(od, 3), np.random.default_rng(4)
    tok = g.integers(2, od.n_tok, size=(B, Te)).astype(np.int32)
    lens = np.array([Te] + [Te - 1 - b % 3 for b in range(B - 1)], np.int32)
    spk_mel = normal(g, (B * od.spk_samples, od.spk_frames, od.n_mel))
    t = lambda a: torch.from_numpy(a).to(dev).contiguous()
    for mode in ("persist", "stepwise"):
        eng = InferEngine(pd, device=dev, values=values)
        eng.persist_infer = eng.persist_lstm = mode == "persist"
        name = "infer %s %s " % (tag, mode)
        spk = eng.speaker_embedding(t(spk_mel))
        put(name + "speaker_embedding", spk)
        mem, keys = eng.encoder(t(tok), t(lens), spk)
        put(name + "encoder values", mem)
        put(name + "encoder keys", keys)
        lin, stop, align, S = eng.decode(mem, keys, t(lens), seed=9, max_steps=max_steps)
        for k, v in (("linear", lin), ("stop", stop), ("align", align)):
            put(name + "decode " + k, v)
        mel = eng.postnet(lin.transpose(0, 1).contiguous(), B, S)
        put(name + "postnet", mel)
        put(name + "mel_to_spectrogram", eng.mel_to_spectrogram(mel, B, S))
        res = eng.forward({"Token": tok, "Token_Length": lens, "Speaker_Embedding_Mel": spk_mel}, seed=9, max_steps=max_steps)
        for k in sorted(res):
            put(name + "forward " + k, res[k])
        print("#  %scounters: decode steps %d, persist_infer launches %d fallbacks %d, non_persistent_decodes %d, persist_disabled_decodes %d, "
              "persist_lstm launches %d fallbacks %d" % (name, S, eng.persist_infer_launches, eng.persist_infer_fallbacks, eng.non_persistent_decodes,
                                                         eng.persist_disabled_decodes, eng.persist_lstm_launches, eng.persist_lstm_fallbacks), flush=True)


def slabs(name, ps):
    put(name + "trainable slab after Adam", ps.train)
    put(name + "frozen slab", ps.frozen)


def taco1(tag, cfg, B, S):
    pd, od = Dims(**cfg), OM.Dims(**cfg)
    g, name = np.random.default_rng(6), "taco1 %s " % tag
    eng = Taco1TrainEngine(pd, device=dev, values=OM.init_params(od, 5))
    mel, spec = torch.from_numpy(normal(g, (B, S, od.n_mel))).to(dev), torch.from_numpy(g.uniform(0, 1, (B, S, od.n_spec)).astype(np.float32)).to(dev)
    with lib.deterministic_gemm():
        w = eng.train_step(mel, spec, seed=7)
    put(name + "prediction", w.pred)
    put(name + "gradient slab", eng.params.grad)
    slabs(name, eng.params)
    put(name + "loss words", w.scalars)


def speaker(tag, cfg, n_speakers):
    pd, od = Dims(**cfg), OM.Dims(**cfg)
    g, name = np.random.default_rng(8), "speaker %s " % tag
    eng = SpeakerTrainEngine(pd, device=dev, values=OM.init_params(od, 5))
    mel = torch.from_numpy(normal(g, (n_speakers * od.spk_samples, od.spk_frames, od.n_mel))).to(dev)
    with lib.deterministic_gemm():
        w = eng.train_step(mel, od.spk_samples, seed=7)
    put(name + "embedding", w.x[-1])
    put(name + "gradient slab", eng.params.grad)
    slabs(name, eng.params)
    put(name + "loss words", w.out3)
    print("#  %scounters: persist_lstm fallbacks %d" % (name, eng.persist_lstm_fallbacks), flush=True)


def train(tag, cfg, B, Te, L):
    pd, od = Dims(**cfg), OM.Dims(**cfg)
    name = "train %s " % tag
    eng = TrainEngine(pd, device=dev, values=OM.init_params(od, 3), deterministic=True)
    w = eng.plan(B, Te, L)
    with lib.deterministic_gemm():
        eng.forward(to_dev(OT.synthetic_batch(od, B, Te, L, seed=5, ragged=True), dev), w, seed=7)
        eng.loss_and_backward(w)
        put(name + "mel_out", w.mel_out)
        put(name + "gradient slab", eng.params.grad)
        eng.adam_step()
    slabs(name, eng.params)
    put(name + "loss words", w.scalars)


ap = argparse.ArgumentParser()
ap.add_argument("--dump", metavar="out.npz")
ap.add_argument("--only", metavar="WORDS", help="run the cases whose name holds every word, e.g. 'infer smoke'")
args = ap.parse_args()
for tag, cfg, B, Te, L, steps in (("smoke", SMOKE, 2, 8, 5, 5), ("reference", {}, 2, 16, 12, 8)):
    for case, fn, a in (("infer", infer, (B, Te, steps)), ("taco1", taco1, (B, L)), ("speaker", speaker, (B,)), ("train", train, (B, Te, L))):
        if all(word in (case, tag) for word in (args.only or "").split()):
            fn(tag, cfg, *a)
if args.dump:
    np.savez(args.dump, **OUT)
