"""Drop-in for the reference's vocoder trainer class ``WaveGlow.WaveGlow`` (WaveGlow/WaveGlow.py:17-205):
``WaveGlow().Restore() / .Train() / .Train_Step(pattern) / .Inference(path_List)``.

The saved file (`waveglow.pt` under hp.WaveGlow.Checkpoint_Path) holds the variables under their `waveglow/...` names - exactly
what ``MSTTS_SV.Tacotron2.Vocoder_Load`` reads - plus the Adam slots and the global step under `__...__` keys, which the inference
engine ignores.  Patterns are dicts {'Audio': [N, L], 'Mel': [N, T, 80]}; without one a synthetic pattern of the reference's batch
shape is used.  The wav feeder follows WaveGlow/Feeder.py:30-114 (Feeder.load_wav's trim stands in for librosa's); with
feeder="device" the batches come from a device-resident bank of the corpus instead (waveglow_feeder.py).
"""
from __future__ import annotations

import collections
import os
import threading
import time

import numpy as np

from . import Hyper_Parameters as hp
from .training import DropIn
from .waveglow import P_WG, WaveGlowEngine, WGDims, vocode
from .waveglow_trainer import WaveGlowTrainEngine, learning_rate

TRAIN_KEYS = ("Global_Step", "Learning_Rate", "Log_S_Loss", "Log_Det_W_Loss", "Audio_Loss", "Train_OP")


# ---- Feeder (WaveGlow/Feeder.py:30-114) ---------------------------------------------------------------------------------------------
def train_signal(path, rng, max_length=None):
    """A training waveform: loaded at Export_Sample_Rate, trimmed (top_db 15, frame 32, hop 16), scaled to a peak of 0.99, then a random
    crop of Max_Signal_Length samples or zero padding to that length."""
    from .Feeder import load_wav
    max_length = max_length or hp.WaveGlow.Train.Max_Signal_Length
    sig = load_wav(path, hp.WaveGlow.Export_Sample_Rate, top_db=15.0, frame=32, hop=16).astype(np.float64)
    peak = np.abs(sig).max() if sig.size else 0.0
    if peak > 0:
        sig = sig / peak * 0.99
    if sig.shape[0] > max_length:
        start = int(rng.integers(0, sig.shape[0] - max_length))
        sig = sig[start:start + max_length]
    else:
        sig = np.concatenate([sig, np.zeros(max_length - sig.shape[0])])
    return sig.astype(np.float32)


def resample_for_mel(sig):
    """The reference resamples the (padded) signal to Sound.Sample_Rate for the mel ONLY; the audio target stays at Export_Sample_Rate."""
    from scipy.signal import resample_poly
    a, b = int(hp.WaveGlow.Export_Sample_Rate), int(hp.Sound.Sample_Rate)
    if a == b:
        return np.asarray(sig, np.float32)
    g = np.gcd(a, b)
    return resample_poly(np.asarray(sig, np.float64), b // g, a // g).astype(np.float32)


def mel_frames(n_samples):
    """Frames of Audio.melspectrogram for n samples at Sound.Sample_Rate (1 + n / hop)."""
    hop = int(hp.Sound.Frame_Shift / 1000 * hp.Sound.Sample_Rate)
    return 1 + n_samples // hop


def signal_mel(sig, device="cuda"):
    from . import Audio
    s = hp.Sound
    return np.transpose(Audio.melspectrogram(resample_for_mel(sig), num_freq=s.Spectrogram_Dim, frame_shift_ms=s.Frame_Shift,
                                             frame_length_ms=s.Frame_Length, num_mels=s.Mel_Dim, sample_rate=s.Sample_Rate,
                                             max_abs_value=s.Max_Abs_Mel, device=device))


def train_batch(paths, rng, device="cuda", mel_fn=None):
    """{'Audio': [N, max L], 'Mel': [N, max T, Mel_Dim]}, every item zero-padded to the batch's longest."""
    sigs = [train_signal(p, rng) for p in paths]
    mel_fn = mel_fn or (lambda s: signal_mel(s, device))
    mels = [mel_fn(s) for s in sigs]
    audio = np.zeros((len(sigs), max(s.shape[0] for s in sigs)), np.float32)
    mel = np.zeros((len(mels), max(m.shape[0] for m in mels), hp.Sound.Mel_Dim), np.float32)
    for i, (s, m) in enumerate(zip(sigs, mels)):
        audio[i, :s.shape[0]] = s
        mel[i, :m.shape[0]] = m
    return {"Audio": audio, "Mel": mel}


def wav_paths(root):
    out = []
    for r, _, files in os.walk(root):
        out += [os.path.join(r, f).replace("\\", "/") for f in files if os.path.splitext(f)[1].upper() == ".WAV"]
    return sorted(out)


class WavFeeder:
    """Train_Pattern_Generate (Feeder.py:30-114) in a producer thread: shuffled batches of Batch_Size files, at most Max_Pattern_Queue ahead."""

    def __init__(self, root=None, device="cuda", seed=None, mel_fn=None):
        self.paths = wav_paths(root or hp.WaveGlow.Train.Pattern_Path)
        if not self.paths:
            raise ValueError("no .wav files under '%s'" % (root or hp.WaveGlow.Train.Pattern_Path))
        self.rng = np.random.default_rng(seed)
        self.device, self.mel_fn = device, mel_fn
        self.queue = collections.deque()
        self._stop = False
        self.thread = threading.Thread(target=self._run, daemon=True)
        self.thread.start()

    def _run(self):
        bs = hp.WaveGlow.Train.Batch_Size
        while not self._stop:
            paths = list(self.paths)
            self.rng.shuffle(paths)
            batches = [paths[x:x + bs] for x in range(0, len(paths), bs)]
            self.rng.shuffle(batches)
            for b in batches:
                while len(self.queue) >= hp.WaveGlow.Train.Max_Pattern_Queue and not self._stop:
                    time.sleep(0.1)
                if self._stop:
                    return
                self.queue.append(train_batch(b, self.rng, self.device, self.mel_fn))

    def Get_Train_Pattern(self):
        while not self.queue:
            time.sleep(0.01)
        return self.queue.popleft()

    def stop(self):
        self._stop = True


def feeder_mode(feeder=None):
    """"device" or "host": the argument, else the environment variable MSTTS_WG_FEEDER, else "host" (WavFeeder resamples with scipy in
    fp64; the device resampler cannot promise its last bit, so the bank path is opt-in as front_end="device" is)."""
    mode = feeder if feeder is not None else os.environ.get("MSTTS_WG_FEEDER", "host")
    if mode not in ("device", "host"):
        raise ValueError("feeder must be 'device' or 'host', not {!r}".format(mode))
    return mode


# ---- the trainer class ----------------------------------------------------------------------------------------------------------------
class WaveGlow(DropIn):
    HP, FILE, SCOPE = "WaveGlow", "waveglow.pt", P_WG
    COLUMNS = (("Learning rate: {:0.5f}", "Learning_Rate"), ("Log S Loss: {:0.5f}", "Log_S_Loss"),
               ("Log Det W Loss: {:0.5f}", "Log_Det_W_Loss"), ("Audio Loss: {:0.5f}", "Audio_Loss"))

    def __init__(self, device="cuda", seed=1234, dims: WGDims = None, values=None, feeder=None):
        self.device = device
        self.seed = seed
        self.feeder_mode = feeder_mode(feeder)
        self.engine = WaveGlowTrainEngine(dims or WGDims.from_hp(hp), device=device, seed=seed, values=values)
        self.params = self.engine.params
        self.train_Tensor_Dict = {k: k for k in TRAIN_KEYS}
        self.inference_Tensor_Dict = {k: k for k in ("Global_Step", "Audio")}

    def Synthetic_Pattern(self, batch_Size=None, length=None, seed=1234):
        """Audio of `length` samples (default Max_Signal_Length) and the fewest mel frames whose upsampled length covers it."""
        g = np.random.default_rng(seed)
        d = self.engine.d
        N = batch_Size or hp.WaveGlow.Train.Batch_Size
        L = length or hp.WaveGlow.Train.Max_Signal_Length
        T = max(1, -(-(L - d.up_k) // d.up_stride) + 1)
        return {"Audio": np.clip(g.normal(0, 0.3, (N, L)), -0.99, 0.99).astype(np.float32),
                "Mel": np.clip(g.normal(0, 1.5, (N, T, d.n_mel)), -4, 4).astype(np.float32)}

    def Train_Step(self, pattern=None):
        """One iteration of the reference's `while True` body (WaveGlow.py:117-129)."""
        pattern = pattern or self.Synthetic_Pattern()
        step = self.engine.global_step
        w = self.engine.train_step(self._upload(pattern["Audio"]), self._upload(pattern["Mel"]))
        res = self.engine.scalars(w)
        res.update({"Global_Step": step, "Learning_Rate": learning_rate(step), "Train_OP": None})
        return res

    def _corpus_feeder(self):
        """"host": the reference's loop (WavFeeder).  "device": the signal bank of the wavs under hp.WaveGlow.Train.Pattern_Path and the
        one-launch feeder on it; when the bank does not fit its budget, one line saying so and the host feeder."""
        if self.feeder_mode == "host":
            return WavFeeder(device=self.device)
        from . import waveglow_feeder as WF
        paths = wav_paths(hp.WaveGlow.Train.Pattern_Path)
        if not paths:
            raise ValueError("no .wav files under '%s'" % hp.WaveGlow.Train.Pattern_Path)
        try:
            bank = WF.bank_from_wavs(paths, device=self.device)
        except WF.BankBudgetError as e:
            print("The signal bank does not fit ({}): feeding from the host (WavFeeder).".format(e))
            return WavFeeder(device=self.device)
        return WF.WaveGlowFeeder(bank, seed=self.seed, dims=self.engine.d)

    def Inference(self, path_List, file_Prefix=None, wg_arith=None, denoiser_strength=None):
        """wav -> mel -> WaveGlowEngine (built from the current values) -> WAV files under hp.WaveGlow.Inference.Path/WAV (WaveGlow.py:144-205).
        wg_arith: the vocoder's arithmetic, "f32" | "bf16" (None: MSTTS_WG_ARITH, else "f32"; WaveGlowEngine.infer).
        denoiser_strength: the WaveGlow denoiser (WaveGlowEngine.denoise) on the stitched waveforms, before the peak normalisation; None:
        MSTTS_WG_DENOISE, else off."""
        from scipy.io.wavfile import write
        from .Feeder import load_wav
        mels = []
        for path in path_List:
            sig = load_wav(path, hp.WaveGlow.Export_Sample_Rate, top_db=15.0, frame=32, hop=16)
            peak = np.abs(sig).max()
            sig = sig / peak * 0.99 if peak > 0 else sig
            mels.append(signal_mel(sig, self.device).astype(np.float32))
        eng = WaveGlowEngine(self.engine.d, device=self.device, values=self.engine.values())
        wavs = vocode(eng, mels, hp.WaveGlow.Inference.Mel_Split_Length, hp.WaveGlow.Inference.Batch_Size, arith=wg_arith,
                      denoise=denoiser_strength)
        out_dir = os.path.join(hp.WaveGlow.Inference.Path, "WAV").replace("\\", "/")
        os.makedirs(out_dir, exist_ok=True)
        prefix = file_Prefix or "GS_{}".format(self.engine.global_step)
        for i, wav in enumerate(wavs):
            peak = np.abs(wav).max()
            wav = wav / peak if peak > 0 else wav                  # librosa.util.normalize (WaveGlow.py:186)
            write(os.path.join(out_dir, "{}.IDX_{}.WAV".format(prefix, i)), hp.WaveGlow.Export_Sample_Rate, wav.astype(np.float32))
        return wavs
