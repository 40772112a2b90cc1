"""Drop-in for the reference's vocoder trainer class ``Taco1_Mel_to_Spect.Taco1_Mel_to_Spect.Mel_to_Spect``
(Taco1_Mel_to_Spect/Taco1_Mel_to_Spect.py:15-205): ``Mel_to_Spect().Restore() / .Train() / .Train_Step(pattern)``.

The saved file (`mel_to_spectrogram.pt` under hp.Taco1_Mel_to_Spect.Checkpoint_Path) is exactly what
``MSTTS_SV.Tacotron2.Vocoder_Load`` reads, as in the reference where the TTS model restores the vocoder scope from the
vocoder trainer's checkpoint directory (MSTTS_SV.py:229-234).  Patterns are dicts {'Mel': [B,T,80], 'Spectrogram': [B,T,1025]}
(the reference's Taco1 feeder pads pickled (mel, spectrogram) pairs to the batch maximum); without one a synthetic pattern
of the trainer's batch shape is used.
"""
from __future__ import annotations

import numpy as np

from . import Hyper_Parameters as hp
from .params import Dims
from .taco1_trainer import Taco1TrainEngine, learning_rate
from .training import DropIn

TRAIN_KEYS = ("Global_Step", "Learning_Rate", "Loss", "Train_OP")


class Mel_to_Spect(DropIn):
    HP, FILE, SCOPE = "Taco1_Mel_to_Spect", "mel_to_spectrogram.pt", "mel_to_spectrogram"
    COLUMNS = (("Learning rate: {:0.5f}", "Learning_Rate"), ("Loss: {:0.5f}", "Loss"))

    def __init__(self, device="cuda", seed=1234, dims: Dims = None):
        self.device = device
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
