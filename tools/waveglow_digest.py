"""Evidence that a refactor of the WaveGlow schedule changed nothing: run this file UNCHANGED in a checkout of the parent commit and in the
branch and compare the two outputs line by line (profiles/waveglow_refactor_digests.txt is such a record).  It uses only
WaveGlowEngine.infer(mel, noise=, seed=, sigma=, arith=, stages=), the attributes split_in / conv_two_pieces, the environment switches and
WaveGlowTrainEngine.plan / forward.

  --trace   (no GPU needed) every library call of one infer / one training forward, in order, with every integer and float argument
            (descriptor fields included); each pointer is replaced by the ordinal of its first appearance in that call's trace, so aliasing
            and buffer reuse are compared and allocation order is not.  Nothing is launched: the binding's library handle is replaced by a
            recorder.  One line per leg: the number of calls, per-entry-point counts and the SHA-256 of the trace text; --dump DIR keeps the text.
  --digest  (GPU) SHA-256 of the waveform of each leg, of every tensor of the bf16 `stages` hook, and of the training forward's z, cond[f],
            lsb[f] and skip[f].

Legs: fp32 with the dilated convolution in one piece | in two pieces | bf16 resident | bf16 with MSTTS_WG_BF16_RESIDENT=0 | bf16 at ch = 36
(every resident product refused, the vector glue still legal)."""
import argparse
import collections
import ctypes
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from multi_speaker_tts_amd import lib                                    # noqa: E402
from multi_speaker_tts_amd import waveglow as WG                         # noqa: E402
from multi_speaker_tts_amd import waveglow_trainer as WT                 # noqa: E402
from oracle import waveglow as OW                                        # noqa: E402

CFGS = [dict(n_mel=8, flows=4, groups=8, early_every=2, early_size=2, up_k=16, up_stride=4, layers=3, ch=32, k=3),          # = tests/test_gpu_waveglow.py
        dict(n_mel=16, flows=12, groups=8, early_every=4, early_size=2, up_k=32, up_stride=8, layers=4, ch=64, k=3),
        dict(n_mel=8, flows=6, groups=4, early_every=3, early_size=2, up_k=8, up_stride=4, layers=8, ch=32, k=3)]
REF_WG = dict(n_mel=80, flows=12, groups=8, early_every=4, early_size=2, up_k=1024, up_stride=256, layers=8, ch=512, k=3)
CASES = {"cfg0": (CFGS[0], 2, 5), "cfg1": (CFGS[1], 3, 6), "cfg2": (CFGS[2], 1, 9), "ref_4x40": (REF_WG, 4, 40)}
TRACE_CASES = dict(CASES, ref_4x40=(dict(REF_WG, flows=1), 4, 40))       # (one coupling at the reference widths: the trace of the others is the same but for c)
# leg -> (arith, conv_two_pieces, MSTTS_WG_BF16_RESIDENT, ch override)
LEGS = {"f32_one_piece": ("f32", False, "1", None), "f32_two_pieces": ("f32", True, "1", None), "bf16_resident": ("bf16", True, "1", None),
        "bf16_resident_off": ("bf16", True, "0", None), "bf16_ch36": ("bf16", True, "1", 36)}
TRAIN_CASE = (CFGS[0], 2, 13)                                            # the small config of tests/test_gpu_waveglow_trainer.py; La = 64


def values_of(cfg, seed=3):
    v = OW.init_params(OW.WGDims(**cfg), seed=seed)
    if cfg["ch"] >= 512:                 # a trained network keeps the couplings' log-scales small (as tests/test_gpu_waveglow.py)
        for k in v:
            if k.endswith("wavenet/conv1d/kernel"):
                v[k] = np.asarray(v[k]) * 0.05
    return v


def sha(t):
    t = t.detach().contiguous().cpu()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes() if t.dtype == torch.bfloat16 else t.numpy().tobytes()).hexdigest()[:16]


def sha_all(pairs):
    h = hashlib.sha256()
    for key, t in pairs:
        h.update(("%s %s %s\n" % (key, tuple(t.shape), sha(t))).encode())
    return h.hexdigest()[:16]


# ---------------------------------------------------------------------------------------------------------------- the recorder
class Recorder:
    """Stands in for the loaded library: records (entry point, arguments) and launches nothing.  The host-only entry points go through."""
    REAL = ("mstts_gemm_bf16_res_supported", "mstts_gemm_deterministic", "mstts_last_error", "mstts_abi_version")

    def __init__(self, real):
        self.real, self.lines, self.ordinal = real, [], {}

    def reset(self):
        self.lines, self.ordinal = [], {}

    def _ptr(self, v):
        v = getattr(v, "value", v)
        if not v:
            return "null"
        return "p%d" % self.ordinal.setdefault(int(v), len(self.ordinal))

    def _arg(self, ctype, v):
        if ctype is ctypes.c_void_p:
            return self._ptr(v)
        if hasattr(v, "_obj"):           # byref(descriptor)
            d = v._obj
            return "{%s}" % " ".join("%s=%s" % (n, self._arg(t, getattr(d, n))) for n, t in d._fields_)
        return repr(float(v)) if ctype is ctypes.c_float else repr(int(v))

    def __getattr__(self, name):
        if name in self.REAL:
            return getattr(self.real, name)
        types = lib.SIGNATURES[name][1]

        def record(*args):
            self.lines.append("%s %s" % (name, " ".join(self._arg(t, a) for t, a in zip(types[:-1], args[:-1]))))      # (the last one is the stream)
            return 0
        return record

    def summary(self):
        counts = collections.Counter(l.split(" ", 1)[0] for l in self.lines)
        text = "\n".join(self.lines) + "\n"
        return "%d calls sha %s  %s" % (len(self.lines), hashlib.sha256(text.encode()).hexdigest()[:16],
                                         " ".join("%s:%d" % (k.replace("mstts_", ""), counts[k]) for k in sorted(counts))), text


# ---------------------------------------------------------------------------------------------------------------- the legs
_engines = {}


def run_leg(case, cfg, N, T, leg, dev):
    """(engine, mel) set up for one leg; the engine of a (case, ch) is built once and only its switches change between legs."""
    arith, two, resident, ch = LEGS[leg]
    cfg = dict(cfg, ch=ch) if ch else cfg
    os.environ["MSTTS_WG_BF16_RESIDENT"] = resident
    if (case, ch) not in _engines:
        _engines.clear()                 # (one engine at a time: the reference widths are 268 M parameters)
        _engines[(case, ch)] = WG.WaveGlowEngine(WG.WGDims(**cfg), device=dev, values=values_of(cfg))
    eng = _engines[(case, ch)]
    eng.conv_two_pieces = two
    mel = np.clip(np.random.default_rng(8).normal(0, 1.5, (N, T, cfg["n_mel"])), -4, 4).astype(np.float32)
    return eng, mel


def train_forward(dev):
    cfg, N, T = TRAIN_CASE
    d = WG.WGDims(**cfg)
    eng = WT.WaveGlowTrainEngine(d, device=dev, values=values_of(cfg, seed=5))
    La = (T - 1) * d.up_stride + d.up_k
    g = np.random.default_rng(2)
    audio = torch.tensor(g.normal(0, 0.3, (N, La)), dtype=torch.float32, device=dev)
    mel = torch.tensor(np.clip(g.normal(0, 1.5, (N, T, d.n_mel)), -4, 4), dtype=torch.float32, device=dev)
    w = eng.plan(N, T, La)
    return eng, audio, mel, w


def trace(dump):
    real = lib.load()
    rec = lib._lib = Recorder(real)
    lib.stream = lambda: None            # (no device: the recorder drops the stream argument anyway)

    def emit(name, text_of):
        rec.reset()
        text_of()
        line, text = rec.summary()
        print("trace %-28s %s" % (name, line))
        if dump:
            os.makedirs(dump, exist_ok=True)
            with open(os.path.join(dump, name.replace(" ", "_") + ".txt"), "w") as f:
                f.write(text)
    for case, (cfg, N, T) in TRACE_CASES.items():
        for leg in LEGS:
            eng, mel = run_leg(case, cfg, N, T, leg, "cpu")
            emit("%s %s" % (case, leg), lambda: eng.infer(mel, seed=5, sigma=0.8, arith=LEGS[leg][0]))
    eng, audio, mel, w = train_forward("cpu")
    emit("train_forward cfg0", lambda: eng.forward(audio, mel, w))


def digest():
    dev = torch.device("cuda:0")
    for case, (cfg, N, T) in CASES.items():
        for leg in LEGS:
            eng, mel = run_leg(case, cfg, N, T, leg, dev)
            bf16 = LEGS[leg][0] == "bf16"
            stages = {} if bf16 else None
            wav = eng.infer(mel, seed=5, sigma=0.8, arith=LEGS[leg][0], stages=stages)
            torch.cuda.synchronize()
            print("digest %-10s %-18s wav %s finite %d" % (case, leg, sha(wav), int(torch.isfinite(wav).all())))
            if bf16:
                pairs = [("%s/%s" % (k, n), t) for k in sorted((k for k in stages if k != "resident"), key=str) for n, t in sorted(stages[k].items())]
                print("digest %-10s %-18s stages %s tensors %d resident %s" % (case, leg, sha_all(pairs), len(pairs), sorted(stages["resident"].items())))
    eng, audio, mel, w = train_forward(dev)
    z = eng.forward(audio, mel, w)
    torch.cuda.synchronize()
    print("digest train_fwd  z %s finite %d" % (sha(z), int(torch.isfinite(z).all())))
    for name in ("cond", "lsb", "skip"):
        print("digest train_fwd  %s %s" % (name, sha_all([(str(f), t) for f, t in enumerate(getattr(w, name))])))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--digest", action="store_true")
    ap.add_argument("--dump", default=None, help="--trace: keep the full trace text of every leg in this directory")
    a = ap.parse_args()
    if a.trace:
        trace(a.dump)
    if a.digest:
        digest()
