"""What feeding the WaveGlow trainer costs, at the reference widths (batch 4, crops of 8 000 samples at 22 050 Hz, 30 frames of 80 mels, 12
flows of 512 channels) on a seeded synthetic corpus of tone-plus-noise wavs (48 kHz int16, 2 - 6 s) written to a temporary directory.  Legs
of ONE process, alternated round by round so that they share the machine's mood:

  device     Train_Step fed by waveglow_feeder.WaveGlowFeeder: host integer planning, one pinned upload of the (file, start) table, one
             mstts_wg_crop_batch launch
  host       Train_Step fed by WaveGlow.WavFeeder, the reference's loop (WaveGlow/Feeder.py:30-114): its thread decodes, resamples, trims,
             crops, resamples again and transforms 4 files per batch, the step uploads the two arrays.  The feeder is started inside the
             timed region and stopped after it, so no producer thread runs under the other legs; a loop bound by its producer runs at the
             producer's rate from the start
  resident   Train_Step on one device-resident synthetic pattern of the same shape (the figure tools/aux_trainers_bench.py times)

The timed region of a leg is `steps` x (get the pattern + Train_Step), between two device synchronisations; Train_Step ends in the loss read.
Beside them: the device feeder's own host + launch share without a step behind it, and the launch alone by device events over back-to-back
launches of one fixed table.  Writes one JSON object to --out (default profiles/waveglow_feeder_bench.json) and prints it.  A run without
a GPU fails: there is no figure to report from a host.

    python tools/waveglow_feeder_bench.py [--files 64] [--steps 20] [--rounds 3] [--launches 50] [--out PATH]
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
    """`files` 16-bit wavs at 48 kHz: three harmonics of a per-file pitch plus noise, 2 - 6 s, 0.1 s of near silence on either side."""
    from scipy.io import wavfile
    g = np.random.default_rng(seed)
    sr = 48000
    os.makedirs(root)
    for k in range(files):
        n = int(g.integers(2 * sr, 6 * sr + 1))
        t = np.arange(n) / float(sr)
        f0 = g.uniform(90.0, 300.0)
        y = sum(a * np.sin(2 * np.pi * f0 * h * t + g.uniform(0, 6.28)) for h, a in ((1, 0.3), (2, 0.2), (3, 0.1))) + g.normal(0, 0.03, n)
        y = np.concatenate([np.zeros(4800), y, np.zeros(4800)]) + g.normal(0, 1e-4, n + 9600)
        wavfile.write(os.path.join(root, "syn_%05d.wav" % k), sr, np.clip(y * 32767, -32767, 32767).astype(np.int16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "waveglow_feeder_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("waveglow_feeder_bench: no GPU - nothing is measured on a host")
    from multi_speaker_tts_amd import Hyper_Parameters as hp
    from multi_speaker_tts_amd import WaveGlow as W
    from multi_speaker_tts_amd import waveglow_feeder as WF
    dev = "cuda:0"
    tr = hp.WaveGlow.Train
    B, L = tr.Batch_Size, tr.Max_Signal_Length
    with tempfile.TemporaryDirectory() as tmp:
        wav_root = os.path.join(tmp, "wav48")
        write_wavs(wav_root, a.files, seed=11)
        paths = W.wav_paths(wav_root)
        t0 = time.perf_counter()
        bank = WF.bank_from_wavs(paths, device=dev)
        torch.cuda.synchronize(); bank_fill_s = time.perf_counter() - t0
        feeder = WF.WaveGlowFeeder(bank, seed=3)
        m = W.WaveGlow(device=dev)
        resident = {"Audio": torch.empty(B, L, device=dev), "Mel": torch.empty(B, feeder.F, hp.Sound.Mel_Dim, device=dev)}
        for k, v in feeder.Get_Train_Pattern().items():                        # (a real batch's values: the flow's losses stay finite)
            resident[k].copy_(v)
        host = [None]

        def host_pattern():
            if host[0] is None:
                host[0] = W.WavFeeder(wav_root, device=dev, seed=3)
            return host[0].Get_Train_Pattern()

        def host_close():
            if host[0] is not None:
                host[0].stop()
                host[0].thread.join()
                host[0] = None
        legs = {"device": feeder.Get_Train_Pattern, "host": host_pattern, "resident": lambda: resident}
        for name, fn in legs.items():                                          # warm-up: code objects, page-locked slots, the workspace
            for _ in range(3):
                m.Train_Step(fn())
            host_close()
        print("warm-up done", file=sys.stderr, flush=True)
        times = {k: [] for k in legs}
        for _ in range(a.rounds):
            for name, fn in legs.items():
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(a.steps):
                    r = m.Train_Step(fn())                 # (ends in the loss read: a device synchronisation)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / a.steps * 1e3)
                host_close()
        feeder.check_status()
        # the device feeder's own host + launch share, without a step behind it
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(a.steps):
            feeder.Get_Train_Pattern()
        torch.cuda.synchronize(); feed_ms = (time.perf_counter() - t0) / a.steps * 1e3
        # the host loop alone: one batch at a time, synchronous (decode, resample, trim, crop, resample, mel), nothing queued
        rng = np.random.default_rng(3)
        t0 = time.perf_counter()
        n_host = max(2, min(5, a.files // B))
        for k in range(n_host):
            W.train_batch(paths[k * B:(k + 1) * B], rng, dev)
        host_ms = (time.perf_counter() - t0) / n_host * 1e3
        # the launch alone: one fixed table, back to back, by events
        table = feeder.plan()
        N = table.shape[0]
        table_d = torch.tensor(table, device=dev)
        audio, mel = torch.empty(N, L, device=dev), torch.empty(N, feeder.F, hp.Sound.Mel_Dim, device=dev)
        for _ in range(10):
            feeder.launch(table_d, N, audio, mel)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            feeder.launch(table_d, N, audio, mel)
        e1.record(); torch.cuda.synchronize()
        launch_us = e0.elapsed_time(e1) / a.launches * 1e3
        feeder.check_status()
    res = {
        "what": "WaveGlow trainer: step time by feeding leg, ms/step (median and all rounds); a round = %d steps" % a.steps,
        "device": torch.cuda.get_device_name(0),
        "timed_region": "steps x (get the pattern + Train_Step) between two device synchronisations; Train_Step ends in the loss read",
        "batch": {"files": B, "audio_samples": L, "mel_frames": feeder.F, "n_mel": int(hp.Sound.Mel_Dim), "up": feeder.up, "down": feeder.down},
        "corpus": {"files": a.files, "wav": "48 kHz int16, 2 - 6 s", "bank_files": int(len(bank.lengths)), "signal_bank_bytes": bank.total_samples * 4,
                   "bank_fill_s": round(bank_fill_s, 2)},
        "step_ms": {k: {"median": float(np.median(v)), "rounds": [round(x, 3) for x in v]} for k, v in times.items()},
        "device_feeder_alone_ms_per_batch": round(feed_ms, 4),
        "host_loop_alone_ms_per_batch": round(host_ms, 2),
        "feeder_launch": {"N": N, "T": feeder.F, "workgroups": N * feeder.F, "us_per_launch_back_to_back": round(launch_us, 2),
                          "note": "launches back to back on one stream: the figure includes the launch-to-launch boundary"},
        "last_loss": float(r["Log_S_Loss"] + r["Log_Det_W_Loss"] + r["Audio_Loss"]),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
