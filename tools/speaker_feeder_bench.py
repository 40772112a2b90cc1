"""What feeding the GE2E speaker-encoder trainer costs, at the reference batch shape (32 speakers x 10 utterances, 140-180 frames, 80 mels)
on a seeded synthetic corpus.  Four legs in ONE process, alternated round by round so that they share the machine's mood:

  resident   Train_Step on one device-resident pattern (what tools/aux_trainers_bench.py times, minus its per-step upload)
  varied     Train_Step on 16 device-resident patterns cut beforehand, whose frame counts vary like the feeder's: what a varying batch
             shape alone costs the step (the engine keeps three workspace sets and builds the others anew)
  feeder     Train_Step fed by speaker_feeder.SpeakerFeeder: host integer planning, one pinned table upload, one gather launch
  host       Train_Step fed by a host loop shaped like the reference's feeder (Speaker_Embedding/Feeder.py:66-100): per batch it unpickles
             Batch_Speaker x Batch_per_Speaker protocol-2 files, crops / pads them into a NumPy batch, and the step uploads it

and the gather kernel alone, by device events over many launches, beside its byte floor 2 N T n_mel 4 bytes over the HBM rate (each output
byte is written once and - for a batch without padding - read once).  Writes one JSON object to --out (default
profiles/speaker_feeder_bench.json) and prints it.  A run without a GPU fails: there is no figure to report from a host.

    python tools/speaker_feeder_bench.py [--rounds 4] [--steps 8] [--speakers 64] [--files 12] [--out PATH]
"""
import argparse
import json
import os
import pickle
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12          # bytes/s: the MI355X's specified rate; the rate a float4 copy kernel reaches on it


def synthetic_corpus(speakers, files, n_mel, seed):
    """{speaker: [mel [T_i, n_mel]]}: a per-speaker offset pattern plus noise (like Speaker_Embedding.Synthetic_Pattern), 100 - 400 frames."""
    g = np.random.default_rng(seed)
    out = {}
    for k in range(speakers):
        base = g.normal(0, 1.0, (1, n_mel))
        out["SYN.%04d" % k] = [np.clip(base + g.normal(0, 1.0, (int(g.integers(100, 401)), n_mel)), -4, 4).astype(np.float32) for _ in range(files)]
    return out


def write_patterns(corpus, root):
    """The corpus as the reference's pattern set (one protocol-2 pickle per file) -> {speaker: [file names]}."""
    names, index = {}, 0
    for spk, mels in corpus.items():
        names[spk] = []
        for mel in mels:
            name = "SYN.{:07d}.pickle".format(index)
            with open(os.path.join(root, name), "wb") as f:
                pickle.dump({"Speaker": spk, "Mel": mel}, f, protocol=2)
            names[spk].append(name)
            index += 1
    return names


class HostLoop:
    """The reference's Train_Pattern_Generate, one batch per call, synchronous (its thread only hides this time while it is below the step's)."""

    def __init__(self, root, names, S, P, frame_range, n_mel, seed):
        self.root, self.names, self.S, self.P, self.fr, self.n_mel = root, names, S, P, frame_range, n_mel
        self.rng = np.random.default_rng(seed)
        self.groups = []

    def __call__(self):
        if not self.groups:
            spk = list(self.names)
            self.rng.shuffle(spk)
            self.groups = [spk[x:x + self.S] for x in range(0, len(spk), self.S)]
            self.groups = [g for g in self.groups if len(g) >= 2]
        group = self.groups.pop(0)
        T = int(self.rng.integers(self.fr[0], self.fr[1] + 1))
        batch = np.zeros((len(group), self.P, T, self.n_mel), np.float32)
        for i, s in enumerate(group):
            for j, name in enumerate(self.rng.choice(self.names[s], self.P, replace=False)):
                with open(os.path.join(self.root, name), "rb") as f:
                    mel = pickle.load(f)["Mel"]
                n = mel.shape[0]
                if n > T:
                    a = int(self.rng.integers(0, n - T))
                    batch[i, j] = mel[a:a + T]
                elif n == T:
                    batch[i, j] = mel
                else:
                    a = int(self.rng.integers(0, T - n))
                    batch[i, j, a:a + n] = mel
        return {"Mel": batch.reshape(-1, T, self.n_mel), "Batch_per_Speaker": self.P}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--speakers", type=int, default=64)
    ap.add_argument("--files", type=int, default=12)
    ap.add_argument("--gather-launches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "speaker_feeder_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("speaker_feeder_bench: no GPU - nothing is measured on a host")
    from multi_speaker_tts_amd import Hyper_Parameters as hp
    from multi_speaker_tts_amd import lib
    from multi_speaker_tts_amd.Speaker_Embedding import Speaker_Embedding
    from multi_speaker_tts_amd.speaker_feeder import MelBank, SpeakerFeeder
    dev = "cuda:0"
    tr = hp.Speaker_Embedding.Train
    S, P, fr, n_mel = tr.Batch_Speaker, tr.Batch_per_Speaker, tuple(tr.Frame_Range), hp.Sound.Mel_Dim
    corpus = synthetic_corpus(a.speakers, a.files, n_mel, seed=11)
    m = Speaker_Embedding(device=dev)
    bank = MelBank.from_mels(corpus, device=dev)
    feeder = SpeakerFeeder(bank, seed=3)
    with tempfile.TemporaryDirectory() as root:
        host = HostLoop(root, write_patterns(corpus, root), S, P, fr, n_mel, seed=3)
        resident = {"Mel": torch.as_tensor(m.Synthetic_Pattern(seed=1)["Mel"]).to(dev), "Batch_per_Speaker": P}
        pre, cut = SpeakerFeeder(bank, seed=4), []
        for _ in range(16):
            cut.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in pre.Get_Train_Pattern().items()})
        turn = iter(range(10 ** 9))
        legs = {"resident": lambda: resident, "varied": lambda: cut[next(turn) % len(cut)], "feeder": feeder.Get_Train_Pattern, "host": host}
        # warm-up: every frame count of the range plans its own workspace set; a few steps per leg load code objects and page-lock buffers
        for fn in legs.values():
            for _ in range(3):
                m.Train_Step(fn())
        times = {k: [] for k in legs}
        for _ in range(a.rounds):
            for name, fn in legs.items():
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(a.steps):
                    r = m.Train_Step(fn())                 # (ends in the loss read: a device synchronisation)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / a.steps * 1e3)
        feeder.check_status()
        # the feeder's own host + launch share, without a step behind it
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(50):
            feeder.Get_Train_Pattern()
        torch.cuda.synchronize(); feed_ms = (time.perf_counter() - t0) / 50 * 1e3
        t0 = time.perf_counter()
        for _ in range(5):
            host()
        host_ms = (time.perf_counter() - t0) / 5 * 1e3
    # the gather kernel alone at the largest batch of the range (N x T_max), one fixed table, by events
    N, T = S * P, fr[1]
    rng = np.random.default_rng(5)
    from multi_speaker_tts_amd.speaker_feeder import check_table, epoch_groups, plan_batch
    table = plan_batch(rng, bank.index, S, P, (T, T), speakers=epoch_groups(rng, bank.index, S, P)[0])[1]
    check_table(table, bank.lengths, T)
    table_d = torch.tensor(table, device=dev)
    out = torch.empty(N, T, n_mel, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    launch = lambda: lib.call("mstts_mel_bank_gather", lib.ptr(bank.bank), lib.ptr(bank.frame_off), bank.lengths.shape[0], lib.ptr(table_d), N, T, n_mel,
                              lib.ptr(out), lib.ptr(status))
    for _ in range(20):
        launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.gather_launches):
        launch()
    e1.record(); torch.cuda.synchronize()
    gather_us = e0.elapsed_time(e1) / a.gather_launches * 1e3
    assert int(status.item()) == 0
    copied = int(table[:, 3].sum()) * n_mel * 4
    floor_bytes = 2 * N * T * n_mel * 4
    res = {
        "what": "GE2E speaker-encoder trainer: step time by feeding leg, ms/step (median and all rounds), %d steps per round" % a.steps,
        "device": torch.cuda.get_device_name(0),
        "batch": {"speakers": S, "per_speaker": P, "frame_range": list(fr), "n_mel": n_mel},
        "corpus": {"speakers": a.speakers, "files_per_speaker": a.files, "bank_bytes": bank.total_frames * n_mel * 4},
        "step_ms": {k: {"median": float(np.median(v)), "rounds": [round(x, 3) for x in v]} for k, v in times.items()},
        "feeder_alone_ms_per_batch": round(feed_ms, 4),
        "host_loop_alone_ms_per_batch": round(host_ms, 3),
        "gather_kernel": {"N": N, "T": T, "us_per_launch_back_to_back": round(gather_us, 3), "bytes_written": N * T * n_mel * 4, "bytes_read": copied,
                          "floor_bytes": floor_bytes, "floor_us_at_8.0TBps_spec": round(floor_bytes / HBM_SPEC * 1e6, 3),
                          "floor_us_at_6.29TBps_copy": round(floor_bytes / HBM_COPY * 1e6, 3),
                          "note": "launches back to back on one stream: the figure includes the launch-to-launch boundary; the output and the bank rows it reads fit the 256 MB last-level cache, so this is no HBM measurement"},
        "last_loss": float(r["Loss"]),
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
