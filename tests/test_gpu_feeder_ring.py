"""The promise of device_bank.TableFeeder, for each of the three feeders on it: a batch stays valid until `ring` - 1 further batches were
drawn - across the short last group of an epoch (fewer rows than the slot holds) and the first batch of the next epoch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _speaker():
    """5 speakers x 3 mels of 12 - 40 frames, groups of 3 speakers x 2 files: an epoch is a batch of 6 rows and one of 4."""
    from multi_speaker_tts_amd.speaker_feeder import MelBank, SpeakerFeeder
    g = np.random.default_rng(2)
    mels = {"s%d" % k: [g.normal(0, 1, (int(g.integers(12, 41)), 80)).astype(np.float32) for _ in range(3)] for k in range(5)}
    return SpeakerFeeder(MelBank.from_mels(mels, device=DEV), seed=5, batch_speaker=3, batch_per_speaker=2, frame_range=(20, 24)), [4, 6]


def _signals():
    """8 signals of 0.3 - 0.9 s at 22 050 Hz; in groups of 3 an epoch is 3 + 3 + 2."""
    g = np.random.default_rng(3)
    return [(0.3 * np.sin(2 * np.pi * (110 + 30 * k) * np.arange(n) / 22050.0) + 0.05 * g.normal(size=n)).astype(np.float32)
            for k, n in enumerate(int(v) for v in g.integers(6600, 19801, 8))]


def _taco1():
    from multi_speaker_tts_amd.taco1_feeder import SignalBank, Taco1Feeder
    return Taco1Feeder(SignalBank.from_signals(_signals(), device=DEV), seed=5, batch_size=3, sort_by_length=False), [2, 3, 3]


def _waveglow():
    from multi_speaker_tts_amd.taco1_feeder import SignalBank
    from multi_speaker_tts_amd.waveglow_feeder import WaveGlowFeeder
    return WaveGlowFeeder(SignalBank.from_signals(_signals(), device=DEV), seed=5, batch_size=3), [2, 3, 3]


@pytest.mark.parametrize("make,ring", [(_speaker, 3), (_taco1, 2), (_waveglow, 2)], ids=["speaker", "taco1", "waveglow"])
def test_a_batch_outlives_ring_minus_one_further_draws(make, ring):
    feeder, epoch_rows = make()
    assert len(feeder._slots) == ring
    window, rows = [], []                                    # (the batch's tensors, their clones) of the last `ring` draws
    for _ in range(2 * len(epoch_rows) + ring):              # two whole epochs and on into the third
        batch = {k: v for k, v in feeder.Get_Train_Pattern().items() if torch.is_tensor(v)}
        assert batch and all(v.is_cuda for v in batch.values())
        rows.append(next(iter(batch.values())).shape[0])
        window = window[-(ring - 1):] + [(batch, {k: v.clone() for k, v in batch.items()})]
        for age, (live, kept) in enumerate(reversed(window)):                      # age = the batches drawn since
            for k in live:
                assert torch.equal(live[k], kept[k]), (len(rows) - 1, age, k)
    feeder.check_status()
    n = len(epoch_rows)
    assert sorted(rows[:n]) == sorted(rows[n:2 * n]) == epoch_rows and min(epoch_rows) < max(epoch_rows)      # a short group in every epoch
    short = rows.index(min(epoch_rows))
    assert short + ring - 1 < len(rows) and len(rows) > 2 * n                      # ... outlived, and an epoch boundary crossed after it
