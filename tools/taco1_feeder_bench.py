"""What feeding the Taco1 vocoder trainer costs, at the reference batch (128 files, 80 mels, 1025 bins) on a seeded synthetic corpus of
tone-plus-noise signals of 1 - 5 s, written as wavs and turned into a pattern set by Taco1_Mel_to_Spect_Pattern_Generate's own code (so
every pickle holds 'Mel', 'Spectrogram' and 'Signal').  Legs of ONE process, alternated round by round so that they share the machine's
mood; a round of a leg is one epoch (every length-sorted group once), so every feeding leg sees the same set of batch shapes:

  resident   Train_Step on one device-resident 128 x 400-frame pattern (the shape tools/aux_trainers_bench.py times; one workspace set)
  precut     Train_Step on the epoch's batches cut beforehand and held on the device: what the varying batch shape alone costs the step
             (the engine keeps three workspace sets and builds the others anew)
  feeder     Train_Step fed by taco1_feeder.Taco1Feeder: host integer planning, one pinned upload of the files table, one
             mstts_stft_bank_batch launch
  host       Train_Step fed by taco1_feeder.PatternFeeder, the reference's loop (Taco1_Mel_to_Spect/Feeder.py:46-110): its thread unpickles
             and pads 128 files per batch, the step uploads the two arrays.  The feeder is started inside the timed region and closed after
             it, so no producer thread runs under the other legs; a loop bound by its producer runs at the producer's rate from the start

The timed region of a leg is `steps` x (get the pattern + Train_Step), between two device synchronisations; Train_Step ends in the loss read.
Beside them: the feeder's own host + launch share without a step behind it, the host loop alone per batch (unpickle + pad, synchronous),
and the feeder launch alone by device events over back-to-back launches of the longest group.  Writes one JSON object to --out (default
profiles/taco1_feeder_bench.json) and prints it.  A run without a GPU fails: there is no figure to report from a host.

    python tools/taco1_feeder_bench.py [--files 2048] [--rounds 3] [--launches 50] [--out PATH]
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def write_wavs(root, files, seed):
    """`files` 16-bit wavs at the trainer's sample rate: three harmonics of a per-file pitch plus noise, 1 - 5 s."""
    from scipy.io import wavfile
    from multi_speaker_tts_amd import Hyper_Parameters as hp
    g = np.random.default_rng(seed)
    sr = hp.Sound.Sample_Rate
    os.makedirs(root)
    for k in range(files):
        n = int(g.integers(sr, 5 * sr + 1))
        t = np.arange(n) / float(sr)
        f0 = g.uniform(90.0, 300.0)
        y = sum(a * np.sin(2 * np.pi * f0 * h * t + g.uniform(0, 6.28)) for h, a in ((1, 0.3), (2, 0.2), (3, 0.1))) + g.normal(0, 0.03, n)
        wavfile.write(os.path.join(root, "syn_%05d.wav" % k), sr, np.clip(y * 32767, -32767, 32767).astype(np.int16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "taco1_feeder_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("taco1_feeder_bench: no GPU - nothing is measured on a host")
    import contextlib
    import io
    from multi_speaker_tts_amd import Hyper_Parameters as hp
    from multi_speaker_tts_amd import Taco1_Mel_to_Spect_Pattern_Generate as PG
    from multi_speaker_tts_amd import taco1_feeder as TF
    from multi_speaker_tts_amd.Taco1_Mel_to_Spect import Mel_to_Spect
    dev = "cuda:0"
    tr = hp.Taco1_Mel_to_Spect.Train
    B = tr.Batch_Size
    with tempfile.TemporaryDirectory() as tmp:
        wav_root, root = os.path.join(tmp, "wav"), os.path.join(tmp, "patterns")
        t0 = time.perf_counter()
        write_wavs(wav_root, a.files, seed=11)
        with contextlib.redirect_stdout(io.StringIO()):                       # (one line per file)
            written = PG._generate("SYN", PG.VCTK_Info_Load(wav_root), dev, None, root, PG.BATCH)
            md = PG.Metadata_Generate(root)
        generate_s = time.perf_counter() - t0
        print("pattern set of %d files written in %.1f s" % (a.files, generate_s), file=sys.stderr, flush=True)
        assert len(written) == a.files == len(md["Signal_Length_Dict"])
        t0 = time.perf_counter()
        bank = TF.SignalBank.from_patterns(root, device=dev, md=md)
        torch.cuda.synchronize(); bank_fill_s = time.perf_counter() - t0
        feeder = TF.Taco1Feeder(bank, seed=3)
        epoch = -(-a.files // B)                                               # batches per epoch
        m = Mel_to_Spect(device=dev)
        resident = {k: torch.as_tensor(v).to(dev) for k, v in m.Synthetic_Pattern(batch_Size=B, length=400).items()}
        pre, cut = TF.Taco1Feeder(bank, seed=4), []
        for _ in range(epoch):
            cut.append({k: v.clone() for k, v in pre.Get_Train_Pattern().items()})
        pre.check_status()
        del pre
        turn = iter(range(10 ** 9))
        host = [None]

        def host_pattern():
            if host[0] is None:
                host[0] = TF.PatternFeeder(root, seed=3, md=md)
            return host[0].Get_Train_Pattern()

        def host_close():
            if host[0] is not None:
                host[0].close()
                host[0] = None
        legs = {"resident": lambda: resident, "precut": lambda: cut[next(turn) % len(cut)], "feeder": feeder.Get_Train_Pattern, "host": host_pattern}
        # warm-up: code objects, page-locked slots, the allocator's blocks for every batch shape of the epoch
        for name, fn in legs.items():
            for _ in range(3 if name in ("resident", "host") else epoch):
                m.Train_Step(fn())
        host_close()
        print("warm-up done", file=sys.stderr, flush=True)
        times = {k: [] for k in legs}
        for _ in range(a.rounds):
            for name, fn in legs.items():
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(epoch):
                    r = m.Train_Step(fn())                 # (ends in the loss read: a device synchronisation)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / epoch * 1e3)
                host_close()
        feeder.check_status()
        # the feeder's own host + launch share, without a step behind it (one epoch)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(epoch):
            feeder.Get_Train_Pattern()
        torch.cuda.synchronize(); feed_ms = (time.perf_counter() - t0) / epoch * 1e3
        # the host loop alone: unpickle + pad of one epoch's batches, synchronous, nothing uploaded
        import pickle
        names = md["File_List"]
        plan = TF.epoch_batches(np.random.default_rng(3), names, [md["Mel_Length_Dict"][n] for n in names], B, tr.Pattern_Sorting_by_Length)
        t0 = time.perf_counter()
        host_bytes = 0
        for group in plan:
            pairs = []
            for i in group:
                with open(os.path.join(root, names[i]), "rb") as f:
                    d = pickle.load(f)
                pairs.append((d["Mel"], d["Spectrogram"]))
            pat = TF.pad_batch([p[0] for p in pairs], [p[1] for p in pairs])
            host_bytes += pat["Mel"].nbytes + pat["Spectrogram"].nbytes
        host_ms = (time.perf_counter() - t0) / len(plan) * 1e3
        # the feeder launch alone: the group of the longest files, one fixed table, back to back, by events
        order = np.argsort(feeder.frames, kind="stable")[-B:].astype(np.int32)
        T, N = int(feeder.frames[order].max()), len(order)
        feeder.check_files(order, T)
        files_d = torch.tensor(order, device=dev)
        mel, spec = torch.empty(N, T, feeder.n_mel, device=dev), torch.empty(N, T, feeder.n_spec, device=dev)
        for _ in range(10):
            feeder.launch(files_d, N, T, mel, spec)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            feeder.launch(files_d, N, T, mel, spec)
        e1.record(); torch.cuda.synchronize()
        launch_us = e0.elapsed_time(e1) / a.launches * 1e3
        feeder.check_status()
        valid = int(feeder.frames[order].sum())
    frames = feeder.frames
    res = {
        "what": "Taco1 vocoder trainer: step time by feeding leg, ms/step (median and all rounds); a round = one epoch of %d batches" % epoch,
        "device": torch.cuda.get_device_name(0),
        "timed_region": "epoch x (get the pattern + Train_Step) between two device synchronisations; Train_Step ends in the loss read",
        "batch": {"files": B, "n_mel": feeder.n_mel, "n_spec": feeder.n_spec, "sorted_by_length": bool(tr.Pattern_Sorting_by_Length)},
        "corpus": {"files": a.files, "frames_min_median_max": [int(frames.min()), int(np.median(frames)), int(frames.max())],
                   "signal_bank_bytes": bank.total_samples * 4, "feature_bytes": int(frames.sum()) * (feeder.n_mel + feeder.n_spec) * 4,
                   "generate_s": round(generate_s, 1), "bank_fill_s": round(bank_fill_s, 2)},
        "step_ms": {k: {"median": float(np.median(v)), "rounds": [round(x, 3) for x in v]} for k, v in times.items()},
        "feeder_alone_ms_per_batch": round(feed_ms, 4),
        "host_loop_alone_ms_per_batch": round(host_ms, 2),
        "host_loop_bytes_per_batch": host_bytes // len(plan),
        "feeder_launch": {"N": N, "T": T, "valid_frames": valid, "us_per_launch_back_to_back": round(launch_us, 2),
                          "us_per_1000_workgroups": round(launch_us / (N * T) * 1e3, 3),
                          "note": "launches back to back on one stream: the figure includes the launch-to-launch boundary"},
        "last_loss": float(r["Loss"]),
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
