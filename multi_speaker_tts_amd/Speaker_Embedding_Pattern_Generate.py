"""The speaker-encoder trainer's pattern generator (reference: Speaker_Embedding/Pattern_Generate.py:19-163): one pickle (protocol 2) per
audio file holding {'Speaker': '<LEXICON>.<speaker directory>', 'Mel': float32 [frames, Mel_Dim]}, named '<LEXICON>.<index:07d>.pickle'
by the file's position in its corpus' list, plus METADATA.PICKLE with the sound hyper parameters, 'Speaker_File_List_Dict',
'Speaker_Dict' and 'Mel_Length_Dict'; the `-vctk / -ls / -vox1 / -vox2` command line.  speaker_feeder.MelBank.from_patterns reads the set.

As in the reference's Pickle_Generate the waveform is only brought to hp.Sound.Sample_Rate: no silence trim and no 0.99 scale.  The mels
are computed in batches on the GPU: decoding on the host (Feeder.decode_wav), the rate conversion of the chosen waveform rule for a whole
batch (Audio.resample_poly_batch / resample_kaiser_best_batch), one STFT launch per batch (Audio.stft_features).  A file that cannot be
decoded here (.m4a / .flac without the optional `soundfile` module) or that is not longer than the STFT's reflect padding is reported and
skipped; its index stays unused.  The corpus walk is sorted, so the numbering does not depend on the file system's order.
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
    return pattern_path or hp.Speaker_Embedding.Train.Pattern_Path


def Mel_Generate_Batch(paths, device="cuda", rule=None):
    """One mel [frames, Mel_Dim] (float32, host) or None (skipped, with a printed reason) per path."""
    from . import Audio
    rule = _Feeder.wav_rule(rule)
    s = hp.Sound
    n_fft = Audio._stft_parameters(s.Spectrogram_Dim, s.Frame_Shift, s.Frame_Length, s.Sample_Rate)[0]
    sigs, by_rate = {}, {}
    for i, path in enumerate(paths):
        try:
            rate, data = _Feeder.decode_wav(path, rule)
        except Exception as e:                                   # (an undecodable file must not stop a corpus run)
            print("Skipped '{}': {}".format(path, e))
            continue
        if rate == s.Sample_Rate:
            sigs[i] = data
        else:
            by_rate.setdefault(rate, []).append((i, data))
    for rate, members in by_rate.items():                        # one resample launch per source rate
        wavs = [d for _, d in members]
        if rule == "librosa":
            res = Audio.resample_kaiser_best_batch(wavs, rate, s.Sample_Rate, device=device, return_tensor=True)
        else:
            res = Audio.resample_poly_batch(wavs, *Audio.resample_ratio(rate, s.Sample_Rate), device=device, return_tensor=True)
        sigs.update({i: r for (i, _), r in zip(members, res)})
    keep = []
    for i in sorted(sigs):
        if int(sigs[i].shape[0]) <= n_fft // 2:
            print("Skipped '{}': {} samples are not longer than the STFT's reflect padding ({})".format(paths[i], int(sigs[i].shape[0]), n_fft // 2))
        else:
            keep.append(i)
    out = [None] * len(paths)
    if keep:
        feats = Audio.stft_features([sigs[i] for i in keep], s.Spectrogram_Dim, s.Frame_Shift, s.Frame_Length, s.Sample_Rate, num_mels=s.Mel_Dim,
                                    max_abs_value=s.Max_Abs_Mel, device=device)
        for i, mel in zip(keep, _Feeder.mels_to_host([m for m, _ in feats])):
            out[i] = mel
    return out


def Pickle_Write(lexicon_Name, pattern_Index, speaker, mel, pattern_path=None):
    """Pattern_Generate.py:35-42."""
    name = "{}.{:07d}.pickle".format(lexicon_Name, pattern_Index)
    with open(_slash(_pattern_path(pattern_path), name), "wb") as f:
        pickle.dump({"Speaker": speaker, "Mel": np.asarray(mel, np.float32)}, f, protocol=2)
    return name


def _generate(lexicon_Name, file_List, device, rule, pattern_path, batch):
    os.makedirs(_pattern_path(pattern_path), exist_ok=True)
    written = []
    for first in range(0, len(file_List), batch):
        chunk = file_List[first:first + batch]
        for k, mel in enumerate(Mel_Generate_Batch([p for _, p in chunk], device=device, rule=rule)):
            if mel is None:
                continue
            name = Pickle_Write(lexicon_Name, first + k, chunk[k][0], mel, pattern_path)
            written.append(name)
            print("{}    {}    ->    {}".format(lexicon_Name, chunk[k][1], name))
    return written


def _file_list(root_dir, speaker_fn):
    return [(speaker_fn(root), _slash(root, name)) for root, name in _audio_files(root_dir)]


def Pattern_Generate_VCTK(wav_Path, device="cuda", rule=None, pattern_path=None, batch=BATCH):
    """Pattern_Generate.py:46-62: the speaker is the file's directory."""
    print("VCTK raw file list generating...")
    file_List = _file_list(wav_Path, lambda root: "VCTK.{}".format(root.split("/")[-1]))
    print("VCTK raw file list generating...Done")
    return _generate("VCTK", file_List, device, rule, pattern_path, batch)


def Pattern_Generate_LS(data_Path, device="cuda", rule=None, pattern_path=None, batch=BATCH):
    """Pattern_Generate.py:64-81: <speaker>/<chapter>/<file>."""
    print("LS raw file list generating...")
    file_List = _file_list(data_Path, lambda root: "LS.{}".format(root.split("/")[-2]))
    print("LS raw file list generating...Done")
    return _generate("LS", file_List, device, rule, pattern_path, batch)


def Pattern_Generate_VC(lexicon_Suffix, wav_Path, device="cuda", rule=None, pattern_path=None, batch=BATCH):
    """Pattern_Generate.py:83-99 (VoxCeleb 1 / 2): <speaker>/<video>/<file>."""
    print("VC{} raw file list generating...".format(lexicon_Suffix))
    file_List = _file_list(wav_Path, lambda root: "VC{}.{}".format(lexicon_Suffix, root.split("/")[-2]))
    print("VC{} raw file list generating...Done".format(lexicon_Suffix))
    return _generate("VC{}".format(lexicon_Suffix), file_List, device, rule, pattern_path, batch)


def Metadata_Generate(pattern_path=None):
    """Pattern_Generate.py:101-131: every pickle under the pattern path is read back."""
    root_dir = _pattern_path(pattern_path)
    md = {"Sample_Rate": hp.Sound.Sample_Rate, "Spectrogram_Dim": hp.Sound.Spectrogram_Dim, "Mel_Dim": hp.Sound.Mel_Dim,
          "Frame_Shift": hp.Sound.Frame_Shift, "Frame_Length": hp.Sound.Frame_Length,
          "Speaker_File_List_Dict": {}, "Speaker_Dict": {}, "Mel_Length_Dict": {}}
    meta = hp.Speaker_Embedding.Train.Metadata_File.upper()
    print("Pickle data check...")
    for root, dirs, files in os.walk(root_dir):
        dirs.sort()
        for index, name in enumerate(sorted(files)):
            if name.upper() == meta:
                continue
            with open(_slash(root, name), "rb") as f:
                d = pickle.load(f)
            md["Speaker_File_List_Dict"].setdefault(d["Speaker"], []).append(name)
            md["Speaker_Dict"][name] = d["Speaker"]
            md["Mel_Length_Dict"][name] = d["Mel"].shape[0]
            print("{}/{}    {}    Done".format(index + 1, len(files), name))
    print("Pickle data check...Done")
    with open(_slash(root_dir, meta), "wb") as f:
        pickle.dump(md, f, protocol=2)
    return md


def main(argv=None, device="cuda"):
    """The reference's command line (Pattern_Generate.py:134-163)."""
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("-vctk", "--vctk_path", required=False)
    ap.add_argument("-ls", "--ls_path", required=False)
    ap.add_argument("-vox1", "--vox1_path", required=False)
    ap.add_argument("-vox2", "--vox2_path", required=False)
    ap.add_argument("-rule", "--wav_rule", choices=("scipy", "librosa"), default=None)   # the waveform rule (Feeder.wav_rule)
    a = ap.parse_args(argv)
    if all(v is None for v in (a.vctk_path, a.ls_path, a.vox1_path, a.vox2_path)):
        raise ValueError("At least, the path of one dataset should be assigned.")
    if a.vctk_path is not None:
        Pattern_Generate_VCTK(a.vctk_path, device=device, rule=a.wav_rule)
    if a.ls_path is not None:
        Pattern_Generate_LS(a.ls_path, device=device, rule=a.wav_rule)
    if a.vox1_path is not None:
        Pattern_Generate_VC("1", a.vox1_path, device=device, rule=a.wav_rule)
    if a.vox2_path is not None:
        Pattern_Generate_VC("2", a.vox2_path, device=device, rule=a.wav_rule)
    return Metadata_Generate()


if __name__ == "__main__":
    main()
