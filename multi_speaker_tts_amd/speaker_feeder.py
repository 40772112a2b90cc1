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
from .device_bank import MAX_WORKERS, DeviceBank, TableFeeder, _Epochs, check_metadata, file_lengths, load_chunked

# lengths: int64 [n_files] frames per file; speaker_files: one int array of file indices per speaker
BankIndex = namedtuple("BankIndex", ["lengths", "speaker_files"])


def metadata_path(pattern_path=None):
    tr = hp.Speaker_Embedding.Train
    return os.path.join(pattern_path or tr.Pattern_Path, tr.Metadata_File.upper()).replace("\\", "/")


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
    bad, file_len = file_lengths(t[:, 0], lengths)
    bad |= (t < 0).any(axis=1) | (t[:, 1] + t[:, 3] > file_len) | (t[:, 2] + t[:, 3] > T)
    if bad.any():
        r = int(np.nonzero(bad)[0][0])
        raise ValueError("table row %d %s is invalid for %d files and T = %d" % (r, tuple(int(v) for v in t[r]), len(lengths), T))


def _load_pattern(args):
    root, name, speaker = args
    with open(os.path.join(root, name).replace("\\", "/"), "rb") as f:
        d = pickle.load(f)
    if d["Speaker"] != speaker:
        raise ValueError("The speaker labeling of pattern is wrong.\nPattern: {}".format(name))
    return np.ascontiguousarray(d["Mel"], np.float32)


class MelBank(DeviceBank):
    """Every utterance's mel on the device: a DeviceBank of width n_mel (`bank` fp32 [total_frames, n_mel], `frame_off` = its offsets)
    with `speakers` (names) and `index` (BankIndex: host lengths and speaker -> file lists)."""
    NAME, UNIT = "mel bank", "frames"

    def __init__(self, lengths, speakers, speaker_files, n_mel, device="cuda", bank_bytes=None):
        super().__init__(lengths, n_mel, device, bank_bytes)
        self.speakers = list(speakers)
        self.index = BankIndex(self.lengths, [np.asarray(f, np.int64) for f in speaker_files])
        self.n_mel, self.frame_off, self.total_frames = self.width, self.offsets, self.total

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
        """Read METADATA.PICKLE and every pattern pickle under pattern_path (default hp.Speaker_Embedding.Train.Pattern_Path) once
        (`load_chunked`).  Speakers and their files in sorted order."""
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
        load_chunked(self, jobs, _load_pattern, workers, chunk)
        return self


class SpeakerFeeder(TableFeeder):
    """`Get_Train_Pattern()` -> {'Mel': device tensor [N, T, n_mel], 'Batch_per_Speaker': P}: a TableFeeder (ring of 3) whose table is
    `plan_batch`'s and whose launch is mstts_mel_bank_gather.  The same seed gives the same batches bit for bit."""
    KERNEL = "mstts_mel_bank_gather"

    def __init__(self, bank, seed=1234, batch_speaker=None, batch_per_speaker=None, frame_range=None, ring=3):
        tr = hp.Speaker_Embedding.Train
        self.bank = bank
        self.S = int(batch_speaker or tr.Batch_Speaker)
        self.P = int(batch_per_speaker or tr.Batch_per_Speaker)
        self.frame_range = tuple(int(v) for v in (frame_range or tr.Frame_Range))
        self._epochs = _Epochs(seed, lambda rng: epoch_groups(rng, bank.index, self.S, self.P))
        n_max = self.S * self.P
        self._make_ring(bank.device, n_max, 4, [n_max * self.frame_range[1] * bank.n_mel], ring)

    def plan(self):
        """The next batch of the epoch as (T, table); a new epoch's groups are drawn when the last one is used up."""
        return plan_batch(self._epochs.rng, self.bank.index, self.S, self.P, self.frame_range, speakers=self._epochs.next())

    def table(self, plan):
        check_table(plan[1], self.bank.lengths, plan[0])
        return plan[1]

    def batch(self, plan, table_dev, N, bufs):
        from .lib import call, ptr
        T, b = plan[0], self.bank
        mel = bufs[0][:N * T * b.n_mel].view(N, T, b.n_mel)
        call(self.KERNEL, ptr(b.bank), ptr(b.frame_off), b.lengths.shape[0], ptr(table_dev), N, T, b.n_mel, ptr(mel), ptr(self.status))
        return {"Mel": mel, "Batch_per_Speaker": self.P}
