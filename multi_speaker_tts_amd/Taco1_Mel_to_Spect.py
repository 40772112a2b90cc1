"""Drop-in for the reference's vocoder trainer class ``Taco1_Mel_to_Spect.Taco1_Mel_to_Spect.Mel_to_Spect``
(Taco1_Mel_to_Spect/Taco1_Mel_to_Spect.py:15-205): ``Mel_to_Spect().Restore() / .Train() / .Train_Step(pattern)``.

The saved file (`mel_to_spectrogram.pt` under hp.Taco1_Mel_to_Spect.Checkpoint_Path) is exactly what
``MSTTS_SV.Tacotron2.Vocoder_Load`` reads, as in the reference where the TTS model restores the vocoder scope from the
vocoder trainer's checkpoint directory (MSTTS_SV.py:229-234).  Patterns are dicts {'Mel': [B,T,80], 'Spectrogram': [B,T,1025]}
(the reference's Taco1 feeder pads pickled (mel, spectrogram) pairs to the batch maximum).  ``Train()`` feeds itself from the pattern
set under hp.Taco1_Mel_to_Spect.Train.Pattern_Path when its metadata file exists: from a device bank of the set's waveforms
(taco1_feeder.SignalBank / Taco1Feeder: one STFT launch per batch; Taco1_Mel_to_Spect_Pattern_Generate writes such a set) when every
file carries its 'Signal' and the bank fits its budget, else from the reference's host loop (taco1_feeder.PatternFeeder); without a
metadata file a synthetic pattern of the trainer's batch shape is used.
"""
from __future__ import annotations

import os

import numpy as np

from . import Hyper_Parameters as hp
from .params import Dims
from .taco1_trainer import Taco1TrainEngine, learning_rate
from .training import DropIn

TRAIN_KEYS = ("Global_Step", "Learning_Rate", "Loss", "Train_OP")
INFERENCE_IN_TRAIN_FILE = "Mel_to_Spect_Inference_in_Train.txt"           # one wav path per line (Taco1_Mel_to_Spect.py:111-116)


class Mel_to_Spect(DropIn):
    HP, FILE, SCOPE = "Taco1_Mel_to_Spect", "mel_to_spectrogram.pt", "mel_to_spectrogram"
    COLUMNS = (("Learning rate: {:0.5f}", "Learning_Rate"), ("Loss: {:0.5f}", "Loss"))

    def __init__(self, device="cuda", seed=1234, dims: Dims = None):
        self.device = device
        self.seed = seed
        self.engine = Taco1TrainEngine(dims, device=device, seed=seed)
        self.params = self.engine.params
        self.train_Tensor_Dict = {k: k for k in TRAIN_KEYS}
        self.inference_Tensor_Dict = {k: k for k in ("Global_Step", "Mel", "Spectrogram")}

    def Synthetic_Pattern(self, batch_Size=None, length=200, seed=1234):
        g = np.random.default_rng(seed)
        B = batch_Size or hp.Taco1_Mel_to_Spect.Train.Batch_Size
        d = self.engine.d
        return {"Mel": np.clip(g.normal(0, 1.5, (B, length, d.n_mel)), -4, 4).astype(np.float32),
                "Spectrogram": g.uniform(0, 1, (B, length, d.n_spec)).astype(np.float32)}

    def Train_Step(self, pattern=None):
        """One iteration of the reference's `while True` body (:118-124)."""
        pattern = pattern or self.Synthetic_Pattern()
        step = self.engine.global_step
        w = self.engine.train_step(self._upload(pattern["Mel"]), self._upload(pattern["Spectrogram"]))
        res = self.engine.scalars(w)
        res.update({"Global_Step": step, "Learning_Rate": learning_rate(step), "Train_OP": None})
        return res

    def _corpus_feeder(self):
        """When the metadata file of hp.Taco1_Mel_to_Spect.Train.Pattern_Path exists: the device feeder when every file of the pattern set
        carries its 'Signal' and the bank fits its budget; else one line saying which of the two failed, and the host feeder."""
        from . import taco1_feeder as TF
        if not os.path.exists(TF.metadata_path()):
            return None
        md = TF.load_metadata()
        names, signals = md["File_List"], md.get("Signal_Length_Dict", {})
        missing = sum(1 for n in names if n not in signals)
        if missing:
            print("{} of {} pattern files carry no 'Signal': feeding from the host (PatternFeeder).".format(missing, len(names)))
            return TF.PatternFeeder(seed=self.seed, md=md)
        try:
            bank = TF.SignalBank.from_patterns(device=self.device, md=md)
        except TF.BankBudgetError as e:
            print("The signal bank does not fit ({}): feeding from the host (PatternFeeder).".format(e))
            return TF.PatternFeeder(seed=self.seed, md=md)
        return TF.Taco1Feeder(bank, seed=self.seed)

    def _after_step(self, result):
        """Taco1_Mel_to_Spect.py:108-135: the periodic inference on the wav paths of Mel_to_Spect_Inference_in_Train.txt."""
        super()._after_step(result)
        if (result["Global_Step"] + 1) % hp.Taco1_Mel_to_Spect.Train.Inference_Timing == 0 and os.path.exists(INFERENCE_IN_TRAIN_FILE):
            with open(INFERENCE_IN_TRAIN_FILE, "r") as f:
                paths = [line.strip() for line in f.readlines() if line.strip()]
            if paths:
                self.Inference(paths)

    def Inference(self, speaker_Wav_Paths, export=True, griffin_lim_seed=0):
        """Taco1_Mel_to_Spect.py:137-178 (the feeder's Get_Inference_Pattern, Feeder.py:114-147, included): wav files -> trimmed
        signals x 0.99 -> mels on the GPU (one launch) -> the vocoder graph in inference mode from THIS trainer's variables,
        hp.Taco1_Mel_to_Spect.Train.Inference.Batch_Size wavs at a time, zero-padded to the longest of the group -> one batched
        Griffin-Lim on the GPU for all of them -> <Inference.Path>/WAV/GS_<step>.IDX_<i>.WAV.  Returns {'Global_Step', 'Mel': list of
        [frames_i, n_mel], 'Spectrogram': list of [frames_i, n_spec], 'Wav': list of float32 waveforms (None where Griffin-Lim
        could not run: one frame, an export error)}.  The reference exports from a thread and returns nothing; its PLOT files are
        out of scope here."""
        import os

        import torch

        from . import Audio, Feeder as F
        from .inference import InferEngine
        if isinstance(speaker_Wav_Paths, str):
            speaker_Wav_Paths = [speaker_Wav_Paths]
        d, dev = self.engine.d, self.engine.device
        sigs = [F.load_wav(p, top_db=60.0) for p in speaker_Wav_Paths]          # librosa.effects.trim's default threshold
        feats = Audio.stft_features(sigs, hp.Sound.Spectrogram_Dim, hp.Sound.Frame_Shift, hp.Sound.Frame_Length, hp.Sound.Sample_Rate,
                                    num_mels=hp.Sound.Mel_Dim, max_abs_value=hp.Sound.Max_Abs_Mel, device=dev)
        mels = [m for m, _ in feats]
        if getattr(self, "_infer", None) is None:
            self._infer = InferEngine(d, device=dev, params=self.params)
        specs = []
        bs = hp.Taco1_Mel_to_Spect.Train.Inference.Batch_Size
        for b0 in range(0, len(mels), bs):
            group = mels[b0:b0 + bs]
            S = max(m.shape[0] for m in group)
            x = torch.zeros(len(group), S, d.n_mel, dtype=torch.float32, device=dev)
            for i, m in enumerate(group):
                x[i, :m.shape[0]] = m
            y = self._infer.mel_to_spectrogram(x.view(len(group) * S, d.n_mel), len(group), S)
            specs.extend(y[i, :m.shape[0]].contiguous() for i, m in enumerate(group))
        prefix = "GS_{}".format(self.engine.global_step)
        names = ["{}.IDX_{}.WAV".format(prefix, i) for i in range(len(specs))]
        wavs = [None] * len(specs)
        todo = []
        for i, s in enumerate(specs):
            if s.shape[0] <= 1:
                print("WAV '{}' exporting failed. The exported spectrogram is too short.".format(names[i]))
            else:
                todo.append(i)
        try:
            if todo:
                for i, y in zip(todo, Audio.Griffin_Lim_Batch([specs[i] for i in todo], seed=[griffin_lim_seed + i for i in todo], device=dev)):
                    wavs[i] = y
            if export:
                from scipy.io import wavfile
                wav_dir = os.path.join(hp.Taco1_Mel_to_Spect.Train.Inference.Path, "WAV").replace("\\", "/")
                os.makedirs(wav_dir, exist_ok=True)
                for i in todo:
                    wavfile.write(os.path.join(wav_dir, names[i]), hp.Sound.Sample_Rate, wavs[i])
        except Exception as e:           # the reference swallows and reports every export error
            print("Wav exporting failed: {}".format(e))
        out = {"Global_Step": self.engine.global_step, "Mel": [m.cpu().numpy() for m in mels], "Spectrogram": [s.cpu().numpy() for s in specs],
               "Wav": wavs}
        self._infer._keep = []           # (the copies above synchronised: the forward's temporaries may go)
        return out
