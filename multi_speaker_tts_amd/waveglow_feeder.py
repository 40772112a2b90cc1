"""Corpus feeder of the WaveGlow trainer (reference: WaveGlow/Feeder.py:30-114).

The reference decodes Batch_Size wav files per batch, resamples each whole file to Export_Sample_Rate, trims it, scales it to a peak of 0.99,
crops Max_Signal_Length samples, resamples the crop to Sound.Sample_Rate and transforms it: `WaveGlow.WavFeeder` is that loop.  Everything
before the crop depends on the file alone, so `bank_from_wavs` does it once (Audio.wav_front_end, `chunk` files per call) into a
`taco1_feeder.SignalBank`; a batch is planned on the host as integers only (`taco1_feeder.epoch_batches` without sorting, `crop_plan`: the
reference's shuffles and its crop rule) and ONE launch of mstts_wg_crop_batch (csrc/wg_crop.hip) turns the table of (file, start) pairs into
{'Audio': [N, L], 'Mel': [N, F, Mel_Dim]} on the device (`WaveGlowFeeder`).  `crop_batch_host` is its checker: the crops made on the host,
then the existing Audio.resample_poly_batch and Audio.stft_features; the kernel gives the same bits.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from . import Hyper_Parameters as hp
from .device_bank import MAX_WORKERS, BankBudgetError, TableFeeder, _Epochs, default_bank_bytes, file_lengths, pooled_chunks
from .taco1_feeder import SignalBank, epoch_batches

PREEMPHASIS = 0.97                               # Audio.stft_features' constant


class Transform(NamedTuple):
    """The mel transform of a crop, as Audio.stft_features takes it."""
    num_freq: int
    frame_shift_ms: float
    frame_length_ms: float
    num_mels: int
    sample_rate: int
    max_abs: float


def hp_transform():
    s = hp.Sound
    return Transform(s.Spectrogram_Dim, s.Frame_Shift, s.Frame_Length, s.Mel_Dim, s.Sample_Rate, s.Max_Abs_Mel)


def _decode(path):
    from .Feeder import decode_wav
    return decode_wav(path, "scipy")


def bank_from_wavs(paths, device="cuda", bank_bytes=None, chunk=256, workers=MAX_WORKERS):
    """Every file of `paths` as WaveGlow/Feeder.py:59-64 prepares it - at Export_Sample_Rate, trimmed (top_db 15, frame 32, hop 16), scaled
    to a peak of 0.99 - in a SignalBank (`names` = the paths kept, in order).  Decoding on the host with at most 16 worker threads; one
    Audio.wav_front_end call per `chunk` files, whose result stays on the device and is copied straight into the bank.  A file that trims
    to nothing is left out with one printed line.  bank_bytes: the bank's budget (default: half of the free device memory now); the
    corpus going over it raises BankBudgetError as soon as it does."""
    import torch
    from . import Audio
    dev = torch.device(device)
    paths = list(paths)
    if bank_bytes is None:
        bank_bytes = default_bank_bytes(dev)
    pieces, lengths, names, total = [], [], [], 0
    for first, decoded in pooled_chunks(paths, _decode, workers, chunk):
        sigs = Audio.wav_front_end([d for _, d in decoded], [r for r, _ in decoded], hp.WaveGlow.Export_Sample_Rate, top_db=15, frame=32,
                                   hop=16, scale=0.99, peak_normalize=True, device=dev, return_tensor=True, rule="scipy")
        kept = []
        for p, x in zip(paths[first:first + len(sigs)], sigs):
            if x.numel() == 0:
                print("'{}' trims to nothing: left out of the signal bank.".format(p))
                continue
            kept.append(x)
            names.append(p)
            lengths.append(int(x.numel()))
        total += sum(int(x.numel()) for x in kept)
        if total * 4 > bank_bytes:
            raise BankBudgetError("the corpus needs more than %d bytes of device memory, the signal bank's budget is %d bytes" % (total * 4, bank_bytes))
        if kept:
            pieces.append(torch.cat(kept))                           # (a copy: the front end's packed buffer, untrimmed, is let go)
    bank = SignalBank(lengths, dev, bank_bytes, names)
    at = 0
    for x in pieces:
        bank._fill_device(at, x)
        at += int(x.numel())
    return bank


def crop_plan(rng, lengths, files, L):
    """The crop of each row (Feeder.py:66-68, WaveGlow.train_signal): int32 [N, 2] of (file, start), drawn row by row in order -
    start = rng.integers(0, len - L) when len > L, else 0 (no draw)."""
    lengths = np.asarray(lengths, np.int64)
    table = np.zeros((len(files), 2), np.int32)
    for r, f in enumerate(files):
        n = int(lengths[int(f)])
        table[r] = (int(f), int(rng.integers(0, n - L)) if n > L else 0)
    return table


def check_table(table, lengths):
    """Raise ValueError on any row mstts_wg_crop_batch would flag: a file outside [0, n_files), start < 0, start >= the file's length."""
    t = np.asarray(table)
    if t.ndim != 2 or t.shape[1] != 2:
        raise ValueError("table must be [N, 2], not %s" % (t.shape,))
    bad, n = file_lengths(t[:, 0], lengths)
    bad |= (t[:, 1] < 0) | (t[:, 1] >= n)
    if bad.any():
        r = int(np.nonzero(bad)[0][0])
        raise ValueError("row %d (file %d, start %d) is invalid for %d files" % (r, int(t[r, 0]), int(t[r, 1]), len(lengths)))


def crop_frames(L, up, down, transform):
    """(Lr, F): samples of a crop of L after the conversion, and its mel frames."""
    from . import Audio
    hop = Audio._stft_parameters(transform.num_freq, transform.frame_shift_ms, transform.frame_length_ms, transform.sample_rate)[1]
    Lr = Audio.resample_out_len(L, up, down)
    return Lr, 1 + Lr // hop


def crop_supported(up, down, transform):
    from . import Audio, lib
    n_fft, _, win = Audio._stft_parameters(transform.num_freq, transform.frame_shift_ms, transform.frame_length_ms, transform.sample_rate)
    return bool(lib.load().mstts_wg_crop_supported(int(up), int(down), int(n_fft), int(win)))


def crop_batch(bank, sig_off, n_files, table_dev, N, L, T, up, down, transform, audio, mel, status):
    """One mstts_wg_crop_batch launch on the current stream: table_dev device int32 [N, 2] -> audio [N, L], mel [N, T, num_mels]."""
    from . import Audio
    from .lib import call, ptr
    n_fft, hop, win, hann, tw, fb, rng = Audio._fft_constants(transform.num_freq, transform.frame_shift_ms, transform.frame_length_ms,
                                                             transform.num_mels, transform.sample_rate, str(bank.device))
    phase = Audio._device_table("scipy", int(up), int(down), str(bank.device))[0] if (up, down) != (1, 1) else None
    call("mstts_wg_crop_batch", ptr(bank), ptr(sig_off), int(n_files), ptr(table_dev), int(N), int(L), int(T), ptr(phase) if phase is not None else None,
         int(up), int(down), PREEMPHASIS, ptr(hann), ptr(tw), ptr(fb), ptr(rng), n_fft, hop, win, int(transform.num_mels), float(transform.max_abs),
         ptr(audio), ptr(mel), ptr(status))


def crop_batch_host(bank_host, offsets, table, L, up, down, T=None, transform=None, device="cuda"):
    """What mstts_wg_crop_batch must equal bit for bit, composed of existing kernels on host-made crops: each row's crop, zero-padded to L,
    with NumPy; Audio.resample_poly_batch on the crops; Audio.stft_features on the result.  -> (audio [N, L], mel [N, T, num_mels]) host
    float32, T = the crop's frame count when None.  The table must pass `check_table`."""
    from . import Audio
    transform = transform or hp_transform()
    bank_host = np.asarray(bank_host, np.float32)
    offsets = np.asarray(offsets, np.int64)
    table = np.asarray(table)
    check_table(table, np.diff(offsets))
    audio = np.zeros((table.shape[0], L), np.float32)
    for r, (f, start) in enumerate(table):
        piece = bank_host[offsets[f] + start:min(offsets[f] + start + L, offsets[f + 1])]
        audio[r, :piece.shape[0]] = piece
    ys = Audio.resample_poly_batch(list(audio), up, down, device=device, return_tensor=True)
    feats = Audio.stft_features(ys, transform.num_freq, transform.frame_shift_ms, transform.frame_length_ms, transform.sample_rate,
                                num_mels=transform.num_mels, max_abs_value=transform.max_abs, device=device)
    F = crop_frames(L, up, down, transform)[1]
    mel = np.zeros((table.shape[0], F if T is None else T, transform.num_mels), np.float32)
    for r, (m, _) in enumerate(feats):
        mel[r, :F] = m.cpu().numpy()
    return audio, mel


class WaveGlowFeeder(TableFeeder):
    """`Get_Train_Pattern()` -> {'Audio': device tensor [N, L], 'Mel': device tensor [N, F, Mel_Dim]}, L = Max_Signal_Length, F = the mel
    frames of L samples after the conversion Export_Sample_Rate -> Sound.Sample_Rate: a TableFeeder (ring of 2) whose table is the
    (file, start) pairs of `crop_plan` and whose launch is mstts_wg_crop_batch.  The plan is the reference's: files shuffled, grouped by
    Batch_Size, the groups shuffled, then a crop per row as each batch is drawn, all from one Generator(seed).  dims: the trainer's
    WGDims, whose `restructure` must accept (L, F)."""
    KERNEL = "mstts_wg_crop_batch"

    def __init__(self, bank, seed=1234, batch_size=None, max_length=None, dims=None, transform=None, ring=2):
        from . import Audio
        from .waveglow import WGDims
        from .waveglow_trainer import restructure
        tr = hp.WaveGlow.Train
        self.bank = bank
        self.transform = transform or hp_transform()
        self.L = int(max_length or tr.Max_Signal_Length)
        self.up, self.down = Audio.resample_ratio(hp.WaveGlow.Export_Sample_Rate, self.transform.sample_rate)
        if not crop_supported(self.up, self.down, self.transform):
            raise ValueError("mstts_wg_crop_batch does not serve the conversion %d / %d with this transform" % (self.up, self.down))
        self.n_fft = Audio._stft_parameters(*self.transform[:3], self.transform.sample_rate)[0]
        self.Lr, self.F = crop_frames(self.L, self.up, self.down, self.transform)
        if self.Lr <= self.n_fft // 2:
            raise ValueError("crops of %d samples (%d after the conversion) are not longer than the transform's reflect padding (%d)"
                             % (self.L, self.Lr, self.n_fft // 2))
        B = int(batch_size or tr.Batch_Size)
        restructure(dims or WGDims.from_hp(hp), B, self.L, self.F)                 # (raises what the train step would)
        n = len(bank.lengths)
        self._epochs = _Epochs(seed, lambda rng: epoch_batches(rng, range(n), bank.lengths, B, False))
        n_max = min(B, n)
        self._make_ring(bank.device, n_max, 2, [n_max * self.L, n_max * self.F * int(self.transform.num_mels)], ring)

    def plan(self):
        """The next batch as its table, int32 [N, 2]."""
        return crop_plan(self._epochs.rng, self.bank.lengths, self._epochs.next(), self.L)

    def table(self, plan):
        check_table(plan, self.bank.lengths)
        return plan

    def launch(self, table_dev, N, audio, mel):
        b = self.bank
        crop_batch(b.bank, b.sig_off, b.lengths.shape[0], table_dev, N, self.L, self.F, self.up, self.down, self.transform, audio, mel, self.status)

    def batch(self, plan, table_dev, N, bufs):
        audio = bufs[0][:N * self.L].view(N, self.L)
        mel = bufs[1][:N * self.F * self.transform.num_mels].view(N, self.F, self.transform.num_mels)
        self.launch(table_dev, N, audio, mel)
        return {"Audio": audio, "Mel": mel}
