"""Training feeders of the Taco1 vocoder trainer (reference: Taco1_Mel_to_Spect/Feeder.py:32-110).

The reference unpickles Batch_Size files of {'Mel': [T, 80], 'Spectrogram': [T, 1025]} per batch on the host and pads them to the batch's
longest: 4 420 B per frame to read, pad and upload.  `PatternFeeder` is that loop, and the checker of the other one.  Both features are
one STFT of the trimmed waveform, which is 800 B per frame, so `SignalBank` holds every file's WAVEFORM on the device (the 'Signal' key
Taco1_Mel_to_Spect_Pattern_Generate writes), a batch is planned on the host as integers only (`epoch_batches`: the reference's sorting,
grouping and shuffles) and one launch of mstts_stft_bank_batch (csrc/stft_bank.hip) computes the batch's mel and spectrogram straight into
the padded batch tensors (`Taco1Feeder`).  With one seed both feeders deliver the same batches bit for bit.
"""
from __future__ import annotations

import os
import pickle
import queue
import threading

import numpy as np

from . import Hyper_Parameters as hp
from .device_bank import MAX_WORKERS, BankBudgetError, DeviceBank, TableFeeder, _Epochs, check_metadata, file_lengths, load_chunked  # noqa: F401

PREEMPHASIS, REF_LEVEL_DB = 0.97, 20.0          # Audio.stft_features' constants


def metadata_path(pattern_path=None):
    tr = hp.Taco1_Mel_to_Spect.Train
    return os.path.join(pattern_path or tr.Pattern_Path, tr.Metadata_File.upper()).replace("\\", "/")


def load_metadata(pattern_path=None):
    with open(metadata_path(pattern_path), "rb") as f:
        md = pickle.load(f)
    check_metadata(md)
    return md


def epoch_batches(rng, file_list, mel_lengths, batch_size, sort_by_length):
    """One epoch's batches (Feeder.py:46-64) as integers: a list of int64 arrays of positions in file_list.  With sorting: a stable sort
    by mel length, consecutive groups of batch_size, the groups shuffled.  Without: the files shuffled, then grouped, then the groups
    shuffled.  The last group may be short.  rng: numpy Generator."""
    n = len(file_list)
    lengths = np.asarray(mel_lengths, np.int64)
    if lengths.shape != (n,):
        raise ValueError("one mel length per file: %d files, lengths of shape %s" % (n, lengths.shape))
    if n < 1 or batch_size < 1:
        raise ValueError("no batch can be formed from %d files at batch size %d" % (n, batch_size))
    order = np.argsort(lengths, kind="stable") if sort_by_length else rng.permutation(n)
    groups = [order[x:x + batch_size].astype(np.int64) for x in range(0, n, batch_size)]
    return [groups[i] for i in rng.permutation(len(groups))]


def check_files(files, lengths, T, n_fft, hop):
    """Raise ValueError on any row mstts_stft_bank_batch would flag: a file outside [0, n_files), a signal not longer than the reflect
    padding (n_fft / 2), more frames (1 + len / hop) than T."""
    f = np.asarray(files)
    if f.ndim != 1:
        raise ValueError("files must be [N], not %s" % (f.shape,))
    bad, n = file_lengths(f, lengths)
    bad |= (n <= n_fft // 2) | (1 + n // hop > T)
    if bad.any():
        r = int(np.nonzero(bad)[0][0])
        raise ValueError("row %d (file %d) is invalid for %d files, n_fft = %d, hop = %d and T = %d" % (r, int(f[r]), len(lengths), n_fft, hop, T))


def _train_epochs(seed, mel_lengths, batch_size, sort_by_length):
    """(batch size, the epochs of `epoch_batches` over files 0 .. len(mel_lengths) - 1 that both feeders draw from); None: the
    trainer's hyper parameter."""
    tr = hp.Taco1_Mel_to_Spect.Train
    B, sort = int(batch_size or tr.Batch_Size), bool(tr.Pattern_Sorting_by_Length if sort_by_length is None else sort_by_length)
    lengths = np.asarray(mel_lengths, np.int64)
    return B, _Epochs(seed, lambda rng: epoch_batches(rng, range(len(lengths)), lengths, B, sort))


def pad_batch(mels, specs):
    """Feeder.py:83-97: zero-padded to the group's longest -> {'Mel': [N, T, n_mel], 'Spectrogram': [N, T, n_spec]} float32."""
    mel = np.zeros((len(mels), max(m.shape[0] for m in mels), mels[0].shape[1]), np.float32)
    spec = np.zeros((len(specs), max(s.shape[0] for s in specs), specs[0].shape[1]), np.float32)
    for i, (m, s) in enumerate(zip(mels, specs)):
        mel[i, :m.shape[0]] = m
        spec[i, :s.shape[0]] = s
    return {"Mel": mel, "Spectrogram": spec}


class PatternFeeder:
    """The reference's host loop: a producer thread unpickles a group, pads it and queues {'Mel', 'Spectrogram'} host arrays, at most
    Max_Pattern_Queue ahead (`max_queued` is the queue's high-water mark).  Works on pattern sets made by the reference (no 'Signal').
    `Get_Train_Pattern()` blocks until a batch is there; `close()` ends the thread."""

    def __init__(self, pattern_path=None, seed=1234, batch_size=None, sort_by_length=None, max_queue=None, md=None):
        self.root = pattern_path or hp.Taco1_Mel_to_Spect.Train.Pattern_Path
        md = md if md is not None else load_metadata(self.root)
        check_metadata(md)
        self.names = list(md["File_List"])
        self._epochs = _train_epochs(seed, [md["Mel_Length_Dict"][n] for n in self.names], batch_size, sort_by_length)[1]
        self.max_queue = int(max_queue or hp.Taco1_Mel_to_Spect.Train.Max_Pattern_Queue)
        self.queue = queue.Queue(maxsize=self.max_queue)
        self.max_queued = 0
        self._stop = threading.Event()
        self.thread = threading.Thread(target=self._produce, daemon=True)
        self.thread.start()

    def _load(self, name):
        with open(os.path.join(self.root, name).replace("\\", "/"), "rb") as f:
            d = pickle.load(f)
        return d["Mel"], d["Spectrogram"]

    def _put(self, item):
        while not self._stop.is_set():
            try:
                self.queue.put(item, timeout=0.05)
                self.max_queued = max(self.max_queued, self.queue.qsize())
                return
            except queue.Full:
                pass

    def _produce(self):
        try:
            while not self._stop.is_set():
                pairs = [self._load(self.names[i]) for i in self._epochs.next()]
                self._put(pad_batch([m for m, _ in pairs], [s for _, s in pairs]))
        except Exception as e:                                   # (handed to the consumer: a dead producer must not look like a slow one)
            self._put(e)

    def Get_Train_Pattern(self):
        item = self.queue.get()
        if isinstance(item, Exception):
            raise item
        return item

    def close(self):
        self._stop.set()
        self.thread.join()


def _load_signal(args):
    root, name, n = args
    with open(os.path.join(root, name).replace("\\", "/"), "rb") as f:
        sig = np.ascontiguousarray(pickle.load(f)["Signal"], np.float32).reshape(-1)
    if sig.shape[0] != n:
        raise ValueError("file %s: signal of %d samples, the metadata says %d" % (name, sig.shape[0], n))
    return sig


class SignalBank(DeviceBank):
    """Every file's trimmed waveform on the device: a DeviceBank of width 1 (`bank` fp32 [total_samples], `sig_off` = its offsets,
    `lengths` in samples)."""
    NAME, UNIT = "signal bank", "samples"

    def __init__(self, lengths, device="cuda", bank_bytes=None, names=None):
        super().__init__(lengths, 1, device, bank_bytes, names)
        self.sig_off, self.total_samples = self.offsets, self.total

    @classmethod
    def from_signals(cls, signals, device="cuda", bank_bytes=None):
        """A list of waveforms -> bank (files in list order)."""
        sigs = [np.ascontiguousarray(x, np.float32).reshape(-1) for x in signals]
        self = cls([x.shape[0] for x in sigs], device, bank_bytes)
        self._fill(0, sigs)
        return self

    @classmethod
    def from_patterns(cls, pattern_path=None, device="cuda", bank_bytes=None, workers=MAX_WORKERS, chunk=1024, md=None):
        """Read METADATA.PICKLE and the 'Signal' of every pattern pickle under pattern_path (default hp.Taco1_Mel_to_Spect.Train.Pattern_Path)
        once (`load_chunked`).  Files in 'File_List' order."""
        root = pattern_path or hp.Taco1_Mel_to_Spect.Train.Pattern_Path
        md = md if md is not None else load_metadata(root)
        check_metadata(md)
        names = list(md["File_List"])
        missing = [n for n in names if n not in md.get("Signal_Length_Dict", {})]
        if missing:
            raise ValueError("%d of %d pattern files carry no 'Signal' (the first: %s)" % (len(missing), len(names), missing[0]))
        self = cls([md["Signal_Length_Dict"][n] for n in names], device, bank_bytes, names)
        self.mel_lengths = np.asarray([md["Mel_Length_Dict"][n] for n in names], np.int64)
        load_chunked(self, [(root, n, int(k)) for n, k in zip(names, self.lengths)], _load_signal, workers, chunk)
        return self


class Taco1Feeder(TableFeeder):
    """`Get_Train_Pattern()` -> {'Mel': device tensor [N, T, n_mel], 'Spectrogram': device tensor [N, T, n_spec]}, T = the group's longest:
    a TableFeeder (ring of 2, its buffers sized for the largest possible group) whose table is the group's `files` and whose launch is
    mstts_stft_bank_batch.  The same seed gives the same batches as PatternFeeder's, bit for bit."""
    KERNEL = "mstts_stft_bank_batch"

    def __init__(self, bank, seed=1234, batch_size=None, sort_by_length=None, ring=2):
        from . import Audio
        s = hp.Sound
        self.bank = bank
        self.consts = Audio._fft_constants(s.Spectrogram_Dim, s.Frame_Shift, s.Frame_Length, s.Mel_Dim, s.Sample_Rate, str(bank.device))
        self.n_fft, self.hop, self.win = self.consts[:3]
        self.n_mel, self.n_spec, self.max_abs = int(s.Mel_Dim), self.n_fft // 2 + 1, float(s.Max_Abs_Mel)
        self.frames = 1 + bank.lengths // self.hop
        mel_lengths = getattr(bank, "mel_lengths", None)
        if mel_lengths is not None and not np.array_equal(mel_lengths, self.frames):
            raise ValueError("the metadata's mel lengths are not 1 + signal length / hop: the pattern set was not made from these signals")
        B, self._epochs = _train_epochs(seed, self.frames, batch_size, sort_by_length)
        n_max = min(B, len(self.frames))
        rows = n_max * int(self.frames.max())
        self._make_ring(bank.device, n_max, 1, [rows * self.n_mel, rows * self.n_spec], ring)

    def check_files(self, files, T):
        check_files(files, self.bank.lengths, T, self.n_fft, self.hop)

    def plan(self):
        """The next batch as (T, files int32 [N])."""
        files = self._epochs.next().astype(np.int32)
        return int(self.frames[files].max()), files

    def table(self, plan):
        self.check_files(plan[1], plan[0])
        return plan[1]

    def launch(self, files_dev, N, T, mel, spec):
        """One mstts_stft_bank_batch launch on the current stream: files_dev device int32 [N] -> mel [N, T, n_mel], spec [N, T, n_spec]
        (either may be None)."""
        from .lib import call, ptr
        _, _, _, hann, tw, fb, rng = self.consts
        b = self.bank
        call(self.KERNEL, ptr(b.bank), ptr(b.sig_off), b.lengths.shape[0], ptr(files_dev), N, T, PREEMPHASIS, ptr(hann), ptr(tw),
             ptr(fb), ptr(rng), self.n_fft, self.hop, self.win, self.n_mel, self.max_abs, REF_LEVEL_DB,
             ptr(mel) if mel is not None else None, ptr(spec) if spec is not None else None, ptr(self.status))

    def batch(self, plan, files_dev, N, bufs):
        T = plan[0]
        mel = bufs[0][:N * T * self.n_mel].view(N, T, self.n_mel)
        spec = bufs[1][:N * T * self.n_spec].view(N, T, self.n_spec)
        self.launch(files_dev, N, T, mel, spec)
        return {"Mel": mel, "Spectrogram": spec}
