"""The host-side schedule of the train step, recorded at the ctypes boundary and at torch's event / stream calls, as text and as one SHA-256.

For each configuration below three optimizer steps run over the shapes (4, 33, 21), (3, 40, 12), (4, 33, 21) at the dims of
tests/test_gpu_model.py::test_side_chains_change_nothing (the reference widths with small emb / conv / post channels: the smallest at which
the persistent launches run), deterministic=True.  One line per event: the entry name, the stream it was enqueued on (main / encoder /
side), its scalar arguments, its pointer arguments replaced by the index of their first appearance, descriptors passed by reference
field by field in the same way; Event.record, Stream.wait_event and Stream.wait_stream likewise.  Then the SHA-256 of the trace and of
params.train / adam_m / adam_v / frozen / grad.  Two trees that print the same trace digests issue the same calls in the same order on the
same streams.

Configurations (1n and 5b: trace only): 1 default (1n: the same, not deterministic); 2 every *_OVERLAP switch off; 3 VOC_FUSED off; 4 = 3 with bf16
recurrent and contraction products; 5 the sets' persistent flags cleared (launch-per-step loops; 5b: the same in bf16); 6 / 7 / 8 a forward /
BPTT / encoder re-run through the self-test hooks, once in the first step; 9 train_step with a stand-in all_reduce whose calls go into the trace.

usage: python tools/train_step_trace.py [--tree DIR] [--configs 1,2,...] [--dump FILE] [--save DIR] [--against DIR]
  --tree DIR      import multi_speaker_tts_amd from DIR instead of this checkout (another revision of the package)
  --dump FILE     write the full traces there
  --save DIR      keep the final tensors of every configuration there (torch.save)
  --against DIR   print, per configuration and tensor, max |difference| / max |value| against the tensors saved there
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=ROOT)
ap.add_argument("--configs", default="1,1n,2,3,4,5,5b,6,7,8,9")
ap.add_argument("--dump")
ap.add_argument("--save")
ap.add_argument("--against")
args = ap.parse_args()
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.abspath(args.tree))

import torch
import multi_speaker_tts_amd
from multi_speaker_tts_amd import engine as E, inference, lib, training
from oracle import model as OM, train as OT
from tests.helpers import dims_pair, to_dev

dev = torch.device("cuda:0")
SHAPES = [(4, 33, 21), (3, 40, 12), (4, 33, 21)]
TENSORS = ("train", "adam_m", "adam_v", "frozen", "grad")
TRACE_ONLY = ("1n", "5b")    # no tensor digests: atomics in every cut product / bf16 roundings on top of the loops' atomics (two runs of one tree differ by 1e-1)
POINTER_MIN = 1 << 40        # device and host addresses lie far above every size, count, offset and step number of these shapes


class Trace:
    def __init__(self, eng):
        self.eng, self.lines, self.index, self.keep = eng, [], {}, []

    def stream(self, s=None):
        s = torch.cuda.current_stream() if s is None else s
        return "encoder" if s == self.eng._enc_stream else "side" if s == self.eng._side else "main"

    def ref(self, kind, key):
        return "%s%d" % (kind, self.index.setdefault((kind, key), len(self.index)))

    def obj(self, kind, o):
        self.keep.append(o)                  # (kept alive: an id is never handed out twice within one trace)
        return self.ref(kind, id(o))

    def value(self, v, depth=0):
        if v is None:
            return "null"
        if isinstance(v, bool):
            return str(int(v))
        if isinstance(v, int):
            return self.ref("p", v) if abs(v) >= POINTER_MIN else str(v)
        if isinstance(v, float):
            return repr(v)
        if isinstance(v, bytes):
            return repr(v)
        if isinstance(v, C.c_void_p):
            return self.value(v.value)
        if isinstance(v, C._SimpleCData):
            return self.value(v.value)
        if isinstance(v, C.Structure):
            return "{" + " ".join("%s=%s" % (f[0], self.value(getattr(v, f[0]), depth + 1)) for f in v._fields_) + "}"
        if isinstance(v, C.Array):
            return "[" + " ".join(self.value(x, depth + 1) for x in v) + "]"
        if isinstance(v, C._Pointer):
            return "null" if not v else ("->" + self.value(v.contents, depth + 1) if depth < 3 else "->...")
        if hasattr(v, "_obj"):               # ctypes.byref(descriptor)
            return "&" + self.value(v._obj, depth + 1)
        return type(v).__name__

    def add(self, name, s, *vals):
        self.lines.append(" ".join([name, "[" + s + "]"] + list(vals)))


def spied(trace):
    """Context: every `call` binding of the package and torch's Event.record / Stream.wait_event / Stream.wait_stream report to `trace`."""
    import contextlib

    @contextlib.contextmanager
    def cm():
        real_call = lib.call
        mods = [m for n, m in list(sys.modules.items()) if n.startswith("multi_speaker_tts_amd") and getattr(m, "call", None) is real_call]
        assert all(m in mods for m in (lib, E, training)), [m.__name__ for m in mods]     # (masks, params and lib.gemm go through lib.call or bind nothing)
        rec, wev, wst = torch.cuda.Event.record, torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream

        def call(name, *a):
            trace.add(name, trace.stream(), *[trace.value(x) for x in a])
            return real_call(name, *a)

        def record(self, stream=None):
            trace.add("Event.record", trace.stream(stream), trace.obj("e", self))
            return rec(self, stream) if stream is not None else rec(self)

        def wait_event(self, event):
            trace.add("Stream.wait_event", trace.stream(self), trace.obj("e", event))
            return wev(self, event)

        def wait_stream(self, other):
            trace.add("Stream.wait_stream", trace.stream(self), trace.stream(other))
            return wst(self, other)
        for m in mods:
            m.call = call
        torch.cuda.Event.record, torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream = record, wait_event, wait_stream
        try:
            yield
        finally:
            for m in mods:
                m.call = real_call
            torch.cuda.Event.record, torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream = rec, wev, wst
    return cm()


class StandInAllReduce:
    """What train_step asks of a gradient all-reduce, on one rank: every call goes into the trace, agree returns its argument."""

    def __init__(self, trace):
        self.trace = trace

    def start(self, g, lo, hi):
        self.trace.add("all_reduce.start", self.trace.stream(), str(lo), str(hi))

    def finish(self, g):
        self.trace.add("all_reduce.finish", self.trace.stream())

    def agree(self, ok):
        self.trace.add("all_reduce.agree", self.trace.stream(), str(int(bool(ok))))
        return ok


SWITCHES = {"VOC_OVERLAP": E, "POSTNET_WGRAD_OVERLAP": E, "ENC_OVERLAP": E, "ENC_TAIL_OVERLAP": E, "SPK_OVERLAP": inference, "VOC_FUSED": E}
pd, od = dims_pair(emb=64, enc_conv_ch=64, enc_lstm=256, spk=256, prenet=256, dec_lstm=1024, n_mel=80, post_ch=64)
values = OM.init_params(od, 6)
batches = [to_dev(OT.synthetic_batch(od, B, Te, L, seed=40 + i, ragged=True), dev) for i, (B, Te, L) in enumerate(SHAPES)]


def run(cfg):
    saved = {n: getattr(m, n) for n, m in SWITCHES.items()}
    try:
        if cfg == "2":
            for n, m in SWITCHES.items():
                if n.endswith("_OVERLAP"):
                    setattr(m, n, False)
        if cfg in ("3", "4", "5b"):
            E.VOC_FUSED = False
        dt = "bf16" if cfg in ("4", "5b") else "f32"
        eng = E.TrainEngine(pd, device=dev, values=values, seed=12, deterministic=cfg != "1n", recurrent_dtype=dt, gemm_dtype=dt)
        trace = Trace(eng)
        red = StandInAllReduce(trace) if cfg == "9" else None
        with spied(trace):
            for i, b in enumerate(batches):
                trace.add("step", "main", str(i))
                if cfg in ("5", "5b"):
                    w = eng.plan(*SHAPES[i])
                    w.persist = w.persist_bwd = w.persist_enc = False
                if i == 0 and cfg == "6":
                    eng.persist_selftest = 4
                if i == 0 and cfg == "7":
                    eng.persist_bwd_selftest = 3
                if i == 0 and cfg == "8":
                    eng.persist_enc_selftest = 1
                eng.train_step(b, all_reduce=red)
                eng.persist_selftest = eng.persist_bwd_selftest = 0
            torch.cuda.synchronize()
        trace.add("counters", "main", *[str(getattr(eng, n)) for n in ("persist_fallbacks", "persist_bwd_fallbacks", "persist_enc_fallbacks",
                                                                         "collective_redos", "persist_disabled_steps", "non_persistent_plans")])
        ps = eng.params
        return trace.lines, {"train": ps.train, "adam_m": ps.adam_m, "adam_v": ps.adam_v, "frozen": ps.frozen, "grad": ps.grad}
    finally:
        for n, m in SWITCHES.items():
            setattr(m, n, saved[n])


sha = lambda b: hashlib.sha256(b).hexdigest()
dump = open(args.dump, "w") if args.dump else None
assert os.path.dirname(os.path.dirname(os.path.abspath(multi_speaker_tts_amd.__file__))) == os.path.abspath(args.tree), multi_speaker_tts_amd.__file__
for cfg in args.configs.split(","):
    lines, tensors = run(cfg)
    text = "\n".join(lines) + "\n"
    print("config %-2s trace  %s  (%d events)  %s" % (cfg, sha(text.encode()), len(lines), lines[-1]))
    if dump:
        dump.write("==== config %s\n%s" % (cfg, text))
    if cfg in TRACE_ONLY:
        continue
    host = {k: v.detach().cpu() for k, v in tensors.items()}
    for k in TENSORS:
        print("config %-2s %-6s %s" % (cfg, k, sha(host[k].numpy().tobytes())))
    if args.save:
        os.makedirs(args.save, exist_ok=True)
        torch.save(host, os.path.join(args.save, "config_%s.pt" % cfg))
    if args.against:
        other = torch.load(os.path.join(args.against, "config_%s.pt" % cfg))
        for k in TENSORS:
            a, b = host[k].double(), other[k].double()
            print("config %-2s %-6s against %s: max|d|/max|v| = %.3e" % (cfg, k, os.path.basename(os.path.normpath(args.against)), float((a - b).abs().max() / (b.abs().max() + 1e-300))))
if dump:
    dump.close()
