"""SHA-256 of every tensor of the first batches of the three device corpus feeders (speaker_feeder.SpeakerFeeder, taco1_feeder.Taco1Feeder,
waveglow_feeder.WaveGlowFeeder) on seeded synthetic corpora, at two seeds: the figure two trees are compared by when a change must leave
the batches as they are.  Only the feeders' public surface is used (MelBank.from_mels, SignalBank.from_signals, the feeder classes,
Get_Train_Pattern), so the same file runs on either tree.  One line per tensor: feeder, seed, batch, key, shape, digest.  A run without a
GPU fails: there is nothing to digest on a host.

    python tools/feeder_digest.py [--batches 8] [--out PATH]
"""
import argparse
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEEDS = (1234, 7)


def corpora():
    """5 speakers x 3 mels of 12 - 40 frames (the frame range 20 - 24 lies inside), and 8 signals of 0.2 - 0.9 s at 22 050 Hz, one of them
    shorter than a WaveGlow crop."""
    g = np.random.default_rng(11)
    mels = {"s%d" % k: [g.normal(0, 1, (int(g.integers(12, 41)), 80)).astype(np.float32) for _ in range(3)] for k in range(5)}
    signals = [(0.3 * np.sin(2 * np.pi * (110 + 30 * k) * np.arange(n) / 22050.0) + 0.05 * g.normal(size=n)).astype(np.float32)
               for k, n in enumerate([5000] + [int(v) for v in g.integers(9000, 19845, 7)])]
    return mels, signals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("feeder_digest: no GPU - nothing is digested on a host")
    from multi_speaker_tts_amd.speaker_feeder import MelBank, SpeakerFeeder
    from multi_speaker_tts_amd.taco1_feeder import SignalBank, Taco1Feeder
    from multi_speaker_tts_amd.waveglow_feeder import WaveGlowFeeder
    mels, signals = corpora()
    mel_bank, sig_bank = MelBank.from_mels(mels, device="cuda:0"), SignalBank.from_signals(signals, device="cuda:0")
    make = {"speaker": lambda seed: SpeakerFeeder(mel_bank, seed=seed, batch_speaker=3, batch_per_speaker=2, frame_range=(20, 24)),
            "taco1_sorted": lambda seed: Taco1Feeder(sig_bank, seed=seed, batch_size=3, sort_by_length=True),
            "taco1_shuffled": lambda seed: Taco1Feeder(sig_bank, seed=seed, batch_size=3, sort_by_length=False),
            "waveglow": lambda seed: WaveGlowFeeder(sig_bank, seed=seed, batch_size=3)}
    lines = []
    for name, ctor in make.items():
        for seed in SEEDS:
            feeder = ctor(seed)
            for k in range(a.batches):
                for key, v in sorted(feeder.Get_Train_Pattern().items()):
                    if torch.is_tensor(v):
                        h = v.cpu().contiguous().numpy()             # (read before the next draw: the ring reuses the buffer)
                        lines.append("%s seed %d batch %d %s %s %s" % (name, seed, k, key, tuple(h.shape), hashlib.sha256(h.tobytes()).hexdigest()))
            feeder.check_status()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
