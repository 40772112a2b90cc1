"""Training feeder of the speaker encoder (reference: Speaker_Embedding/Feeder.py:33-101) with the corpus resident on the device.

The reference unpickles Batch_Speaker x Batch_per_Speaker files per batch on the host.  Here every utterance's mel is read ONCE into one
device tensor (`MelBank`: VCTK's mels are about 4 GB in fp32), a batch is planned on the host as integers only (`plan_batch`: the
reference's shuffles, frame count, sampling and crop / pad placement as a table of (file, src_start, dst_start, count) rows), and one
launch of mstts_mel_bank_gather (csrc/mel_bank.hip) cuts the batch out of the bank (`SpeakerFeeder`).

The one departure from the reference's batches: a trailing group of a single speaker is dropped, because the loss needs at least 2
speakers (the reference feeds such a group to a loss with an empty between-speaker set).
"""
from __future__ import annotations

import os
import pickle
from collections import namedtuple

import numpy as np

from . import Hyper_Parameters as hp

# lengths: int64 [n_files] frames per file; speaker_files: one int array of file indices per speaker
BankIndex = namedtuple("BankIndex", ["lengths", "speaker_files"])

MAX_WORKERS = 16


def metadata_path(pattern_path=None):
    tr = hp.Speaker_Embedding.Train
    return os.path.join(pattern_path or tr.Pattern_Path, tr.Metadata_File.upper()).replace("\\", "/")


def check_metadata(md):
    """Feeder.py:37-45: the pattern set must have been made with the current sound hyper parameters."""
    s = hp.Sound
    if not all([md["Spectrogram_Dim"] == s.Spectrogram_Dim, md["Mel_Dim"] == s.Mel_Dim, md["Frame_Shift"] == s.Frame_Shift,
                md["Frame_Length"] == s.Frame_Length, md["Sample_Rate"] == s.Sample_Rate]):
        raise ValueError("The metadata information and hyper parameter setting are not consistent.")


def epoch_groups(rng, bank_index, batch_speaker, batch_per_speaker):
    """One epoch's speaker groups (Feeder.py:48-60): the speakers with at least batch_per_speaker files, shuffled, cut into groups of
    batch_speaker, the groups shuffled; a group of one speaker (the tail) is dropped.  Returns a list of int arrays of speaker indices."""
    eligible = np.asarray([k for k, files in enumerate(bank_index.speaker_files) if len(files) >= batch_per_speaker], np.int64)
    rng.shuffle(eligible)
    groups = [eligible[x:x + batch_speaker] for x in range(0, len(eligible), batch_speaker)]
    order = rng.permutation(len(groups))
    groups = [groups[i] for i in order if len(groups[i]) >= 2]
    if not groups:
        raise ValueError("fewer than 2 speakers have at least %d files: no batch can be formed" % batch_per_speaker)
    return groups


def plan_batch(rng, bank_index, batch_speaker, batch_per_speaker, frame_range, speakers=None):
    """One batch by the reference's rules (Feeder.py:62-93) as integers: returns (T, table) with table int32 [N, 4] of
    (file, src_start, dst_start, count) rows, speaker-major, N = len(group) * batch_per_speaker.  rng: numpy Generator.
    speakers: the group (speaker indices, e.g. one of `epoch_groups`); None draws an epoch's groups and takes the first.
    T is uniform in the inclusive frame_range; each speaker gives batch_per_speaker files without replacement; a file longer than T is
    cropped at randint(0, len - T), a shorter one placed at randint(0, T - len), both with numpy.random.randint's EXCLUSIVE upper bound
    as in the reference (the last legal start is never drawn); a file of exactly T frames goes whole."""
    if speakers is None:
        speakers = epoch_groups(rng, bank_index, batch_speaker, batch_per_speaker)[0]
    T = int(rng.integers(frame_range[0], frame_range[1] + 1))
    table = np.zeros((len(speakers) * batch_per_speaker, 4), np.int32)
    r = 0
    for k in speakers:
        for f in rng.choice(bank_index.speaker_files[k], batch_per_speaker, replace=False):
            n = int(bank_index.lengths[f])
            if n > T:
                table[r] = (f, rng.integers(0, n - T), 0, T)
            elif n == T:
                table[r] = (f, 0, 0, T)
            else:
                table[r] = (f, 0, rng.integers(0, T - n), n)
            r += 1
    return T, table


def check_table(table, lengths, T):
    """Raise ValueError on any row mstts_mel_bank_gather would flag: file outside [0, n_files), a negative field, src_start + count
    beyond the file, dst_start + count beyond T."""
    t = np.asarray(table)
    if t.ndim != 2 or t.shape[1] != 4:
        raise ValueError("the table must be [N, 4], not %s" % (t.shape,))
    t = t.astype(np.int64)
    lengths = np.asarray(lengths, np.int64)
    bad = (t < 0).any(axis=1) | (t[:, 0] >= lengths.shape[0])
    file_len = lengths[np.where(bad, 0, t[:, 0])] if lengths.shape[0] else np.zeros(t.shape[0], np.int64)
    bad |= (t[:, 1] + t[:, 3] > file_len) | (t[:, 2] + t[:, 3] > T)
    if bad.any():
        r = int(np.nonzero(bad)[0][0])
        raise ValueError("table row %d %s is invalid for %d files and T = %d" % (r, tuple(int(v) for v in t[r]), lengths.shape[0], T))


def _load_pattern(args):
    root, name, speaker = args
    with open(os.path.join(root, name).replace("\\", "/"), "rb") as f:
        d = pickle.load(f)
    if d["Speaker"] != speaker:
        raise ValueError("The speaker labeling of pattern is wrong.\nPattern: {}".format(name))
    return np.ascontiguousarray(d["Mel"], np.float32)


class MelBank:
    """Every utterance's mel on the device: `bank` fp32 [total_frames, n_mel], `frame_off` int64 [n_files + 1] (device), `lengths`
    (host int64), `speakers` (names) and `index` (BankIndex: host lengths and speaker -> file lists).  bank_bytes is a budget (default:
    half of the free device memory at construction); a corpus over it raises ValueError."""

    def __init__(self, lengths, speakers, speaker_files, n_mel, device="cuda", bank_bytes=None):
        import torch
        self.device = torch.device(device)
        self.lengths = np.asarray(lengths, np.int64)
        self.speakers = list(speakers)
        self.index = BankIndex(self.lengths, [np.asarray(f, np.int64) for f in speaker_files])
        self.n_mel = int(n_mel)
        offsets = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)
        self.total_frames = int(offsets[-1])
        need = self.total_frames * self.n_mel * 4
        if bank_bytes is None:
            bank_bytes = torch.cuda.mem_get_info(self.device)[0] // 2
        if need > bank_bytes:
            raise ValueError("the corpus needs %d bytes of device memory, the mel bank's budget is %d bytes" % (need, bank_bytes))
        if self.total_frames < 1:
            raise ValueError("the corpus holds no frames")
        self.bank_bytes = int(bank_bytes)
        self.bank = torch.empty(self.total_frames, self.n_mel, dtype=torch.float32, device=self.device)
        self.frame_off = torch.as_tensor(offsets).to(self.device)
        self._offsets = offsets

    def _fill(self, first, mels):
        """mels: host arrays of files first, first + 1, ...: one upload."""
        import torch
        for k, m in enumerate(mels):
            if m.shape != (self.lengths[first + k], self.n_mel):
                raise ValueError("file %d: mel of shape %s, expected %s" % (first + k, m.shape, (int(self.lengths[first + k]), self.n_mel)))
        a, b = int(self._offsets[first]), int(self._offsets[first + len(mels)])
        self.bank[a:b].copy_(torch.as_tensor(np.concatenate(mels, axis=0)))

    @classmethod
    def from_mels(cls, speaker_to_mel_list, device="cuda", bank_bytes=None):
        """{speaker: [mel [T_i, n_mel], ...]} -> bank (speakers in the mapping's order, files in list order)."""
        speakers = list(speaker_to_mel_list)
        mels = [np.ascontiguousarray(m, np.float32) for s in speakers for m in speaker_to_mel_list[s]]
        files, n = [], 0
        for s in speakers:
            files.append(np.arange(n, n + len(speaker_to_mel_list[s])))
            n += len(speaker_to_mel_list[s])
        self = cls([m.shape[0] for m in mels], speakers, files, mels[0].shape[1], device, bank_bytes)
        self._fill(0, mels)
        return self

    @classmethod
    def from_patterns(cls, pattern_path=None, device="cuda", bank_bytes=None, workers=MAX_WORKERS, chunk=1024):
        """Read METADATA.PICKLE and every pattern pickle under pattern_path (default hp.Speaker_Embedding.Train.Pattern_Path) once, with at
        most 16 worker threads, `chunk` files per upload.  Speakers and their files in sorted order."""
        from concurrent.futures import ThreadPoolExecutor
        root = pattern_path or hp.Speaker_Embedding.Train.Pattern_Path
        with open(metadata_path(root), "rb") as f:
            md = pickle.load(f)
        check_metadata(md)
        speakers = sorted(md["Speaker_File_List_Dict"])
        jobs, files = [], []
        for s in speakers:
            names = sorted(md["Speaker_File_List_Dict"][s])
            files.append(np.arange(len(jobs), len(jobs) + len(names)))
            jobs += [(root, name, s) for name in names]
        self = cls([md["Mel_Length_Dict"][name] for _, name, _ in jobs], speakers, files, md["Mel_Dim"], device, bank_bytes)
        self.names = [name for _, name, _ in jobs]
        with ThreadPoolExecutor(max_workers=max(1, min(int(workers), MAX_WORKERS))) as pool:
            for first in range(0, len(jobs), chunk):
                self._fill(first, list(pool.map(_load_pattern, jobs[first:first + chunk])))
        return self


class SpeakerFeeder:
    """`Get_Train_Pattern()` -> {'Mel': device tensor [N, T, n_mel], 'Batch_per_Speaker': P}: per batch one pinned upload of the table and
    one gather launch, into a ring of `ring` output buffers (a returned 'Mel' stays valid until `ring` - 1 further batches were drawn).
    The same seed gives the same batches bit for bit.  `status` (device int32 [1]) has bit 0 set once the kernel met an invalid row;
    `check_status()` reads it (a synchronisation) and raises."""

    def __init__(self, bank, seed=1234, batch_speaker=None, batch_per_speaker=None, frame_range=None, ring=3):
        import torch
        tr = hp.Speaker_Embedding.Train
        self.bank = bank
        self.S = int(batch_speaker or tr.Batch_Speaker)
        self.P = int(batch_per_speaker or tr.Batch_per_Speaker)
        self.frame_range = tuple(int(v) for v in (frame_range or tr.Frame_Range))
        self.rng = np.random.default_rng(seed)
        self._groups = []
        n_max = self.S * self.P
        dev = bank.device
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self._slots = [(torch.empty(n_max, 4, dtype=torch.int32, pin_memory=True), torch.empty(n_max, 4, dtype=torch.int32, device=dev),
                        torch.empty(n_max * self.frame_range[1] * bank.n_mel, dtype=torch.float32, device=dev), torch.cuda.Event())
                       for _ in range(max(2, int(ring)))]
        self._next = 0
        epoch_groups(np.random.default_rng(0), bank.index, self.S, self.P)          # (raises now when no batch can be formed)

    def plan(self):
        """The next batch of the epoch as (T, table); a new epoch's groups are drawn when the last one is used up."""
        if not self._groups:
            self._groups = epoch_groups(self.rng, self.bank.index, self.S, self.P)
        return plan_batch(self.rng, self.bank.index, self.S, self.P, self.frame_range, speakers=self._groups.pop(0))

    def Get_Train_Pattern(self):
        import torch
        from .lib import call, ptr
        T, table = self.plan()
        check_table(table, self.bank.lengths, T)
        N, b = table.shape[0], self.bank
        host, dev, out, done = self._slots[self._next]
        self._next = (self._next + 1) % len(self._slots)
        done.synchronize()                                   # the slot's previous upload and launch (ring batches ago)
        host[:N].copy_(torch.from_numpy(table))
        dev[:N].copy_(host[:N], non_blocking=True)
        mel = out[:N * T * b.n_mel].view(N, T, b.n_mel)
        call("mstts_mel_bank_gather", ptr(b.bank), ptr(b.frame_off), b.lengths.shape[0], ptr(dev), N, T, b.n_mel, ptr(mel), ptr(self.status))
        done.record()
        return {"Mel": mel, "Batch_per_Speaker": self.P}

    def check_status(self):
        if int(self.status.item()) != 0:
            raise RuntimeError("mstts_mel_bank_gather met an invalid table row (status %d)" % int(self.status.item()))
