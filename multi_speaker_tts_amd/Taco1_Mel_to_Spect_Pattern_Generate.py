"""The Taco1 vocoder trainer's pattern generator (reference: Taco1_Mel_to_Spect/Pattern_Generate.py:12-136, as it was meant to work: its
`__main__` never parses its arguments and its `*_Info_Load` functions return nothing): one pickle (protocol 2) per audio file, named
'<BASENAME>.PICKLE' in upper case, holding the reference's {'Spectrogram': float32 [frames, Spectrogram_Dim], 'Mel': float32 [frames,
Mel_Dim]} and a third key 'Signal': the float32 trimmed x 0.99 waveform both were computed from (the reference's feeder ignores extra
keys; taco1_feeder.SignalBank keeps these waveforms on the device and recomputes the features per batch).  METADATA.PICKLE carries the
reference's keys - the five sound parameters, 'File_List', 'Mel_Length_Dict' - and 'Signal_Length_Dict' for the files with a signal.
The `-vctk / -ls` command line.

The waveform is what Feeder.load_wav gives (top_db 15, frames 32 / 16, x 0.99), made for a batch of files on the GPU: decoding on the
host (Feeder.decode_wav), Audio.wav_front_end, one STFT launch for both features (Audio.stft_features).  A file that cannot be decoded,
whose trimmed waveform is not longer than the STFT's reflect padding, or whose mel is longer than
hp.Taco1_Mel_to_Spect.Train.Max_Mel_Length is reported and skipped.  The corpus walk is sorted.
"""
from __future__ import annotations

import os
import pickle

import numpy as np

from . import Hyper_Parameters as hp
from . import Feeder as _Feeder
from .Pattern_Generate import _audio_files, _slash, using_Extension      # noqa: F401  (using_Extension: the reference's module attribute)

BATCH = 64          # files per GPU batch


def _pattern_path(pattern_path=None):
    return pattern_path or hp.Taco1_Mel_to_Spect.Train.Pattern_Path


def Feature_Generate_Batch(paths, device="cuda", rule=None):
    """One (signal [n], mel [frames, Mel_Dim], spectrogram [frames, Spectrogram_Dim]) triple of float32 host arrays, or None (skipped,
    with a printed reason), per path."""
    from . import Audio
    rule = _Feeder.wav_rule(rule)
    s = hp.Sound
    n_fft = Audio._stft_parameters(s.Spectrogram_Dim, s.Frame_Shift, s.Frame_Length, s.Sample_Rate)[0]
    decoded = []
    for i, path in enumerate(paths):
        try:
            decoded.append((i,) + _Feeder.decode_wav(path, rule))
        except Exception as e:                                   # (an undecodable file must not stop a corpus run)
            print("Skipped '{}': {}".format(path, e))
    out = [None] * len(paths)
    if not decoded:
        return out
    sigs = Audio.wav_front_end([d for _, _, d in decoded], [r for _, r, _ in decoded], s.Sample_Rate, top_db=15, frame=32, hop=16, scale=0.99,
                               device=device, return_tensor=True, rule=rule)
    keep = []
    for (i, _, _), sig in zip(decoded, sigs):
        if int(sig.shape[0]) <= n_fft // 2:
            print("Skipped '{}': {} samples are not longer than the STFT's reflect padding ({})".format(paths[i], int(sig.shape[0]), n_fft // 2))
        else:
            keep.append((i, sig))
    if not keep:
        return out
    feats = Audio.stft_features([sig for _, sig in keep], s.Spectrogram_Dim, s.Frame_Shift, s.Frame_Length, s.Sample_Rate, num_mels=s.Mel_Dim,
                                max_abs_value=s.Max_Abs_Mel, want_mel=True, want_spec=True, device=device)
    mels = _Feeder.mels_to_host([m for m, _ in feats])
    specs = _Feeder.mels_to_host([sp for _, sp in feats])
    signals = _Feeder.mels_to_host([sig for _, sig in keep])     # (one copy back each)
    for (i, _), sig, mel, spec in zip(keep, signals, mels, specs):
        if hp.Taco1_Mel_to_Spect.Train.Max_Mel_Length < mel.shape[0]:
            print("File '{}' has too long. This file is ignored.".format(paths[i]))
            continue
        out[i] = (sig, mel, spec)
    return out


def Pickle_Write(path, signal, mel, spec, pattern_path=None):
    """Pattern_Generate.py:41-49, + 'Signal'."""
    name = "{}.PICKLE".format(os.path.splitext(os.path.basename(path))[0]).upper()
    with open(_slash(_pattern_path(pattern_path), name), "wb") as f:
        pickle.dump({"Spectrogram": np.asarray(spec, np.float32), "Mel": np.asarray(mel, np.float32), "Signal": np.asarray(signal, np.float32)},
                    f, protocol=2)
    return name


def _generate(prefix, file_List, device, rule, pattern_path, batch):
    os.makedirs(_pattern_path(pattern_path), exist_ok=True)
    written = []
    for first in range(0, len(file_List), batch):
        chunk = file_List[first:first + batch]
        for k, feat in enumerate(Feature_Generate_Batch(chunk, device=device, rule=rule)):
            if feat is None:
                continue
            name = Pickle_Write(chunk[k], *feat, pattern_path=pattern_path)
            written.append(name)
            print("[{} {}/{}]".format(prefix, first + k, len(file_List)), chunk[k], "->", name)
    return written


def VCTK_Info_Load(vctk_Path):
    """Pattern_Generate.py:54-61, returning its list."""
    return [_slash(root, name) for root, name in _audio_files(vctk_Path)]


def LS_Info_Load(ls_Path):
    """Pattern_Generate.py:64-71, returning its list."""
    return [_slash(root, name) for root, name in _audio_files(ls_Path)]


def Metadata_Generate(pattern_path=None):
    """Pattern_Generate.py:73-95: every pickle under the pattern path is read back.  'File_List' is sorted and does not list the metadata
    file itself; 'Signal_Length_Dict' holds the sample count of every file that carries a 'Signal'."""
    root_dir = _pattern_path(pattern_path)
    md = {"Spectrogram_Dim": hp.Sound.Spectrogram_Dim, "Mel_Dim": hp.Sound.Mel_Dim, "Frame_Shift": hp.Sound.Frame_Shift,
          "Frame_Length": hp.Sound.Frame_Length, "Sample_Rate": hp.Sound.Sample_Rate, "File_List": [], "Mel_Length_Dict": {},
          "Signal_Length_Dict": {}}
    meta = hp.Taco1_Mel_to_Spect.Train.Metadata_File.upper()
    for root, dirs, files in os.walk(root_dir):
        dirs.sort()
        for name in sorted(files):
            if name.upper() == meta:
                continue
            try:
                with open(_slash(root, name), "rb") as f:
                    d = pickle.load(f)
                md["Mel_Length_Dict"][name] = d["Mel"].shape[0]
                md["File_List"].append(name)
            except Exception:
                print("File '{}' is not correct pattern file. This file is ignored.".format(name))
                continue
            if "Signal" in d:
                md["Signal_Length_Dict"][name] = int(np.asarray(d["Signal"]).shape[0])
    md["File_List"].sort()
    with open(_slash(root_dir, meta), "wb") as f:
        pickle.dump(md, f, protocol=2)
    return md


def main(argv=None, device="cuda"):
    """The reference's command line (Pattern_Generate.py:97-136)."""
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("-vctk", "--vctk_path", required=False)
    ap.add_argument("-ls", "--ls_path", required=False)
    ap.add_argument("-batch", "--batch", type=int, default=BATCH)                         # files per GPU batch
    ap.add_argument("-rule", "--wav_rule", choices=("scipy", "librosa"), default=None)   # the waveform rule (Feeder.wav_rule)
    a = ap.parse_args(argv)
    lists = [(prefix, load(path)) for prefix, load, path in (("VCTK", VCTK_Info_Load, a.vctk_path), ("LS", LS_Info_Load, a.ls_path))
             if path is not None]
    if sum(len(file_List) for _, file_List in lists) == 0:
        raise ValueError("Total pattern count is zero.")
    for prefix, file_List in lists:
        _generate(prefix, file_List, device, a.wav_rule, None, max(1, a.batch))
    return Metadata_Generate()


if __name__ == "__main__":
    main()
