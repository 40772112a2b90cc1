"""What the device corpus feeders (speaker_feeder, taco1_feeder, waveglow_feeder) share: the corpus in one device tensor (`DeviceBank`,
filled by `load_chunked`), the endless sequence of an rng's epochs (`_Epochs`), the prelude of a host row check (`file_lengths`), the
pattern sets' sound-parameter check (`check_metadata`) and the ring that turns one planned integer table into one launch per batch
(`TableFeeder`).  A feeder module keeps the reference's planning rules, its row semantics and its one launch.
"""
from __future__ import annotations

import numpy as np

from . import Hyper_Parameters as hp

MAX_WORKERS = 16                                 # host threads that read or decode a corpus


class BankBudgetError(ValueError):
    """The corpus does not fit the bank's budget."""


def check_metadata(md):
    """Speaker_Embedding/Feeder.py:37-45, Taco1_Mel_to_Spect/Feeder.py:36-44: the pattern set must have been made with the current sound
    hyper parameters."""
    s = hp.Sound
    if not all([md["Spectrogram_Dim"] == s.Spectrogram_Dim, md["Mel_Dim"] == s.Mel_Dim, md["Frame_Shift"] == s.Frame_Shift,
                md["Frame_Length"] == s.Frame_Length, md["Sample_Rate"] == s.Sample_Rate]):
        raise ValueError("The metadata information and hyper parameter setting are not consistent.")


def default_bank_bytes(device):
    """A bank's budget when none is given: half of the free device memory now."""
    import torch
    return torch.cuda.mem_get_info(device)[0] // 2


def file_lengths(files, lengths):
    """The prelude of a row check: (bad, file_len) for a column of file indices - bad where the file is outside [0, n_files), file_len
    the file's length (some valid file's where bad, zeros when there are no files: never indexed by a bad file)."""
    f, lengths = np.asarray(files, np.int64), np.asarray(lengths, np.int64)
    bad = (f < 0) | (f >= lengths.shape[0])
    return bad, lengths[np.where(bad, 0, f)] if lengths.shape[0] else np.zeros(f.shape[0], np.int64)


class DeviceBank:
    """Every file of a corpus in ONE device tensor: `bank` fp32 [total] (width 1) or [total, width], file k in rows offsets[k] to
    offsets[k + 1]; `offsets` int64 [n_files + 1] on the device, `_offsets` its host copy, `lengths` (host int64, rows per file), `names`,
    `total`.  bank_bytes is a budget (default: `default_bank_bytes`); a corpus over it raises BankBudgetError (a ValueError)."""
    NAME, UNIT = "device bank", "rows"           # a subclass's words for its error texts

    def __init__(self, lengths, width=1, device="cuda", bank_bytes=None, names=None):
        import torch
        self.device = torch.device(device)
        self.lengths = np.asarray(lengths, np.int64)
        self.width = int(width)
        self.names = list(names) if names is not None else None
        self._offsets = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)
        self.total = int(self._offsets[-1])
        need = self.total * self.width * 4
        if bank_bytes is None:
            bank_bytes = default_bank_bytes(self.device)
        if need > bank_bytes:
            raise BankBudgetError("the corpus needs %d bytes of device memory, the %s's budget is %d bytes" % (need, self.NAME, bank_bytes))
        if self.total < 1:
            raise ValueError("the corpus holds no %s" % self.UNIT)
        self.bank_bytes = int(bank_bytes)
        self.bank = torch.empty((self.total,) if self.width == 1 else (self.total, self.width), dtype=torch.float32, device=self.device)
        self.offsets = torch.as_tensor(self._offsets).to(self.device)

    def _fill(self, first, arrays):
        """arrays: host arrays of files first, first + 1, ...: one upload."""
        import torch
        tail = () if self.width == 1 else (self.width,)
        for k, x in enumerate(arrays):
            want = (int(self.lengths[first + k]),) + tail
            if x.shape != want:
                raise ValueError("file %d: an array of shape %s, the %s expects %s" % (first + k, x.shape, self.NAME, want))
        self._fill_device(int(self._offsets[first]), torch.as_tensor(np.concatenate(arrays, axis=0)))

    def _fill_device(self, at, x):
        """x: a tensor (host or device) of whole rows, copied to rows at, at + 1, ..."""
        self.bank[at:at + x.shape[0]].copy_(x)


def pooled_chunks(jobs, load_one, workers=MAX_WORKERS, chunk=1024):
    """(first, [load_one(job) for the jobs first .. first + chunk]) chunk after chunk, loaded by at most MAX_WORKERS threads."""
    from concurrent.futures import ThreadPoolExecutor
    chunk = max(1, int(chunk))
    with ThreadPoolExecutor(max_workers=max(1, min(int(workers), MAX_WORKERS))) as pool:
        for first in range(0, len(jobs), chunk):
            yield first, list(pool.map(load_one, jobs[first:first + chunk]))


def load_chunked(bank, jobs, load_one, workers=MAX_WORKERS, chunk=1024):
    """Fill `bank` with load_one(job) of every job (one per file, in file order): `chunk` files per upload."""
    for first, arrays in pooled_chunks(jobs, load_one, workers, chunk):
        bank._fill(first, arrays)


class _Epochs:
    """The endless sequence of groups a feeder draws from: `draw(rng)` is one epoch's list of groups, drawn anew from Generator(seed)
    when the last one is used up.  `rng` is also where a feeder takes its per-batch draws from."""

    def __init__(self, seed, draw):
        self.rng = np.random.default_rng(seed)
        self.draw = draw
        self._groups = []
        draw(np.random.default_rng(0))                                       # (raises now when no batch can be formed)

    def next(self):
        if not self._groups:
            self._groups = self.draw(self.rng)
        return self._groups.pop(0)


class TableFeeder:
    """A ring of `ring` slots, each a page-locked int32 table, its device copy, the output buffers and an event.  `Get_Train_Pattern()`
    plans a batch on the host, checks its rows, waits for the next slot's event (its upload and launch `ring` batches ago), uploads the
    table from the page-locked copy, has the subclass cut the batch out of its bank with one launch on the current stream and records the
    event.  Nothing is allocated per batch, and a returned batch stays valid until `ring` - 1 further batches were drawn.  `status`
    (device int32 [1]) has bit 0 set once the kernel met an invalid row; `check_status()` reads it (a synchronisation) and raises.

    A subclass sets KERNEL, calls `_make_ring`, and supplies `plan()` (the next batch's plan), `table(plan)` (its int32 table after the
    host row check) and `batch(plan, table_dev, N, bufs)` (views of the slot's buffers, the launch, the dict returned)."""
    KERNEL = None

    def _make_ring(self, device, n_max, cols, out_sizes, ring):
        """n_max: the most rows a batch can have; cols: the table's columns (1: a vector); out_sizes: floats of each output buffer."""
        import torch
        shape = (n_max,) if cols == 1 else (n_max, cols)
        self.status = torch.zeros(1, dtype=torch.int32, device=device)
        self._slots = [(torch.empty(shape, dtype=torch.int32, pin_memory=True), torch.empty(shape, dtype=torch.int32, device=device),
                        [torch.empty(n, dtype=torch.float32, device=device) for n in out_sizes], torch.cuda.Event())
                       for _ in range(max(2, int(ring)))]
        self._next = 0

    def Get_Train_Pattern(self):
        import torch
        plan = self.plan()
        table = self.table(plan)
        N = table.shape[0]
        host, dev, bufs, done = self._slots[self._next]
        self._next = (self._next + 1) % len(self._slots)
        done.synchronize()                                   # the slot's previous upload and launch (ring batches ago)
        host[:N].copy_(torch.from_numpy(table))
        dev[:N].copy_(host[:N], non_blocking=True)
        out = self.batch(plan, dev, N, bufs)
        done.record()
        return out

    def check_status(self):
        if int(self.status.item()) != 0:
            raise RuntimeError("%s met an invalid row (status %d)" % (self.KERNEL, int(self.status.item())))
