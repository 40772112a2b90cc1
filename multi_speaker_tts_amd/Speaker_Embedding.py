"""Drop-in for the reference's speaker-encoder trainer class ``Speaker_Embedding.Speaker_Embedding.Speaker_Embedding``
(Speaker_Embedding/Speaker_Embedding.py:16-160): ``Speaker_Embedding(is_Training).Restore() / .Train() / .Train_Step(pattern) /
.Inference(mel_List)``.  `speaker_embedding.pt` under hp.Speaker_Embedding.Checkpoint_Path is exactly what
``MSTTS_SV.Tacotron2.Speaker_Embedding_Load`` reads (MSTTS_SV.py:223-227).  A training pattern is {'Mel': [Batch_Speaker *
Batch_per_Speaker, frames, 80]} speaker-major with one random frame count from hp.Speaker_Embedding.Train.Frame_Range per batch
(Speaker_Embedding/Feeder.py:66-100).  ``Train()`` feeds itself from the pattern set under hp.Speaker_Embedding.Train.Pattern_Path
when its metadata file exists (speaker_feeder.MelBank / SpeakerFeeder: the corpus resident on the device, one gather launch per batch;
Speaker_Embedding_Pattern_Generate writes such a set); without one a synthetic pattern of that shape is used.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import Hyper_Parameters as hp
from . import Feeder as _Feeder
from .params import Dims
from .speaker_trainer import SpeakerTrainEngine, learning_rate
from .training import DropIn

TRAIN_KEYS = ("Global_Step", "Learning_Rate", "Loss", "Train_OP")
INFERENCE_IN_TRAIN_FILE = "Speaker_Embedding_Inference_in_Train.txt"       # lines `label<TAB>wav path` (Speaker_Embedding.py:99-102)


def Embedding_Value(embeddings, labels):
    """The figure the reference judges an encoder by (Export_TSNE, Speaker_Embedding.py:155-170): mean distance between the per-label mean
    embeddings (over ordered pairs of different labels) / mean distance of every embedding to its label's mean."""
    emb = np.asarray(embeddings)
    labels = list(labels)
    means = {lab: np.mean([e for x, e in zip(labels, emb) if x == lab], axis=0) for lab in set(labels)}
    between = [np.sqrt(np.sum(np.power(m1 - m2, 2))) for l1, m1 in means.items() for l2, m2 in means.items() if l1 != l2]
    within = [np.sqrt(np.sum(np.power(e - means[lab], 2))) for lab, e in zip(labels, emb)]
    return np.mean(between) / np.mean(within)


TSNE_COLORS = ("r", "g", "b", "c", "m", "y", "k", "w", "orange", "purple")      # one per displayed label: at most ten
TSNE_PERPLEXITY = 30.0                                                           # scikit-learn's default, what the reference's TSNE() ran with


def export_tsne(embedding_Array, label_List, global_Step, out_Dir, file_Name="TSNE", tsne_fn=None):
    """The part of `Speaker_Embedding.Export_TSNE` that needs no engine: `Embedding_Value` of the embeddings, their 2-D t-SNE map by
    tsne_fn(X, perplexity=..., seed=0, return_info=True) -> (Y, info) (`tsne.tsne`, or `tsne.tsne_host` where there is no GPU),
    out_Dir/<file_Name>.npz (Y, labels, value, kl_divergence, global_Step) always and, when matplotlib imports, the reference's picture
    out_Dir/<file_Name>.PNG: a 10 x 10 inch scatter of the map, the first ten labels in SORTED order (the reference takes the first ten of
    a set(), an order that changes from process to process) in its colours with black edges, a legend, and the title "Global step: ...
    t-SNE Result    V: ...".  The perplexity is 30, or min(30, (N - 1) / 3) where 30 >= N (printed; scikit-learn would raise).  Returns
    {"value", "title", "perplexity", "kl_divergence", "npz", "png"} (png None without matplotlib), or None when the directory or a file
    cannot be written (an OSError: "export skipped", printed)."""
    X = np.asarray(embedding_Array, np.float32)
    labels = [str(x) for x in label_List]
    n = X.shape[0]
    if len(labels) != n:
        raise ValueError("%d labels for %d embeddings" % (len(labels), n))
    value = float(Embedding_Value(X, labels))
    perplexity = TSNE_PERPLEXITY
    if n < 4 or perplexity >= n:
        perplexity = min(TSNE_PERPLEXITY, (n - 1) / 3.0)
        print("Export_TSNE: %d embeddings, perplexity %g instead of %g" % (n, perplexity, TSNE_PERPLEXITY))
    if n >= 2:
        Y, info = tsne_fn(X, perplexity=perplexity, seed=0, return_info=True)
        kl = float(info["kl_divergence"])
    else:
        Y, kl = np.zeros((n, 2), np.float32), float("nan")
    title = "Global step: {}    t-SNE Result    V: {:0.5f}".format(global_Step, value)
    result = {"value": value, "title": title, "perplexity": perplexity, "kl_divergence": kl, "npz": None, "png": None}
    try:
        os.makedirs(out_Dir, exist_ok=True)
        result["npz"] = os.path.join(out_Dir, "{}.npz".format(file_Name)).replace("\\", "/")
        np.savez(result["npz"], Y=Y, labels=np.asarray(labels), value=value, kl_divergence=kl, global_Step=int(global_Step))
        try:
            from matplotlib.backends.backend_agg import FigureCanvasAgg
            from matplotlib.figure import Figure
        except ImportError:
            print("Export_TSNE: matplotlib is not installed, no picture; the map is in %s" % result["npz"])
            return result
        fig = Figure(figsize=(10, 10))
        FigureCanvasAgg(fig)
        ax = fig.add_subplot(111)
        for speaker, color in zip(sorted(set(labels)), TSNE_COLORS):
            mask = np.asarray([x == speaker for x in labels])
            ax.scatter(Y[mask, 0], Y[mask, 1], c=color, edgecolors="k", label=speaker)
        ax.set_title(title)
        fig.tight_layout()
        ax.legend()
        result["png"] = os.path.join(out_Dir, "{}.PNG".format(file_Name)).replace("\\", "/")
        fig.savefig(result["png"], format="png")
    except OSError as e:
        print("Export_TSNE: export skipped (%s)" % e)
        return None
    return result


class Speaker_Embedding(DropIn):
    HP, FILE, SCOPE = "Speaker_Embedding", "speaker_embedding.pt", "speaker_embedding"
    COLUMNS = (("Learning rate: {:0.6f}", "Learning_Rate"), ("Loss: {:0.5f}", "Loss"))

    def __init__(self, is_Training=True, device="cuda", seed=1234, dims: Dims = None, loss_method=None):
        self.is_Training = is_Training
        self.device = device
        self.seed = seed
        self.engine = SpeakerTrainEngine(dims, device=device, seed=seed, loss_method=loss_method)
        self.embedding_Value = None
        self.params = self.engine.params
        self.train_Tensor_Dict = {k: k for k in TRAIN_KEYS} if is_Training else None
        self.inference_Tensor_Dict = {k: k for k in ("Global_Step", "Embedding")}
        self._infer = None

    def _slots(self):
        e = self.engine
        return {**super()._slots(), "__loss_vars__": e.wb, "__loss_m__": e.wb_m, "__loss_v__": e.wb_v}

    def Synthetic_Pattern(self, speakers=None, per_speaker=None, seed=1234):
        """Speaker-dependent synthetic mels (a per-speaker offset pattern plus noise), so the loss has something to learn."""
        tr = hp.Speaker_Embedding.Train
        S, P = speakers or tr.Batch_Speaker, per_speaker or tr.Batch_per_Speaker
        g = np.random.default_rng(seed)
        T = int(g.integers(tr.Frame_Range[0], tr.Frame_Range[1] + 1))
        d = self.engine.d
        base = g.normal(0, 1.0, (S, 1, 1, d.n_mel))
        mel = np.clip(base + g.normal(0, 1.0, (S, P, T, d.n_mel)), -4, 4).astype(np.float32)
        return {"Mel": mel.reshape(S * P, T, d.n_mel), "Batch_per_Speaker": P}

    def Train_Step(self, pattern=None):
        pattern = pattern or self.Synthetic_Pattern()
        mel = self._upload(pattern["Mel"])
        step = self.engine.global_step
        w = self.engine.train_step(mel, int(pattern.get("Batch_per_Speaker", hp.Speaker_Embedding.Train.Batch_per_Speaker)))
        return {"Global_Step": step, "Learning_Rate": learning_rate(step), "Loss": float(w.out3[0]), "Train_OP": None}

    def _corpus_feeder(self):
        """When training and the metadata file of hp.Speaker_Embedding.Train.Pattern_Path exists: the corpus goes into a device mel bank
        once and every step's batch comes from a SpeakerFeeder on it."""
        from . import speaker_feeder as SF
        if self.is_Training and os.path.exists(SF.metadata_path()):
            return SF.SpeakerFeeder(SF.MelBank.from_patterns(device=self.device), seed=self.seed)

    def _after_step(self, result):
        super()._after_step(result)
        if (result["Global_Step"] + 1) % hp.Speaker_Embedding.Train.Inference_Timing == 0 and os.path.exists(INFERENCE_IN_TRAIN_FILE):
            with open(INFERENCE_IN_TRAIN_FILE, "r") as f:
                label_List, path_List = list(zip(*[line.strip().split("\t") for line in f.readlines() if line.strip()]))
            self.Inference(list(path_List), export_TSNE=True, label_List=list(label_List))
            print("Global step: {}    Embedding value: {:0.5f}".format(result["Global_Step"] + 1, self.embedding_Value))

    def _wav_mels(self, path_List):
        """Feeder.py:130-144: wav -> trimmed (top_db 15, frames 32 / 16), scaled waveform -> mel [frames, Mel_Dim]."""
        from . import Audio
        s = hp.Sound
        return [np.transpose(Audio.melspectrogram(y=_Feeder.load_wav(path), num_freq=s.Spectrogram_Dim, frame_shift_ms=s.Frame_Shift,
                                                  frame_length_ms=s.Frame_Length, num_mels=s.Mel_Dim, sample_rate=s.Sample_Rate,
                                                  max_abs_value=s.Max_Abs_Mel, device=self.device)).astype(np.float32) for path in path_List]

    def Inference(self, path_or_mel_List, export_TSNE=False, label_List=None):
        """Embeddings of whole utterances: 5 windows of 64 frames each, mean of the last-frame outputs, whole-tensor l2
        normalisation (Speaker_Embedding/Modules.py:127-137; Feeder.py:105-160).  path_or_mel_List: [T_i, 80] mel arrays - one forward
        for all, as ever - or wav paths (Speaker_Embedding.py:127-150): hp.Speaker_Embedding.Inference.Max_Embedding_per_Batch files per
        forward, each batch normalised as a whole like in the reference, the results stacked.  With a label_List the between / within
        ratio of the result is left in `embedding_Value` (`Embedding_Value`).  export_TSNE (needs a label_List: ValueError without) also
        draws the reference's picture of them, `Export_TSNE` with file_Name 'GS_<global step>'; the returned array and `embedding_Value`
        are the same with and without it."""
        from .inference import InferEngine
        if export_TSNE and label_List is None:
            raise ValueError("export_TSNE needs a label_List")
        if self._infer is None:
            self._infer = InferEngine(self.engine.d, device=self.device, params=self.params)
        items = list(path_or_mel_List)
        if items and all(isinstance(x, str) for x in items):
            n = hp.Speaker_Embedding.Inference.Max_Embedding_per_Batch
            batches = [self._wav_mels(items[x:x + n]) for x in range(0, len(items), n)]
        else:
            batches = [items]
        out = []
        for mel_List in batches:
            self._infer._keep = []
            win = torch.as_tensor(_Feeder.speaker_windows(mel_List)).to(torch.device(self.device), torch.float32).contiguous()
            out.append(self._infer.speaker_embedding(win).cpu().numpy())
        result = np.vstack(out)
        if label_List is not None:
            self.embedding_Value = Embedding_Value(result, label_List)
        if export_TSNE:
            self.Export_TSNE(result, label_List, self.engine.global_step, "GS_{}".format(self.engine.global_step))
        return result

    def Export_TSNE(self, embedding_Array, label_List, global_Step, file_Name="TSNE"):
        """The reference's Export_TSNE (Speaker_Embedding.py:152-193): `embedding_Value` of the embeddings and their exact t-SNE map
        (tsne.tsne on this object's device, seed 0: csrc/tsne.hip) as hp.Speaker_Embedding.Train.Inference_Path/PLOT/<file_Name>.npz and,
        with matplotlib, .PNG - `export_tsne`, which says what the picture holds.  Synchronous: the reference's thread hid the host's
        t-SNE, which here is a device call."""
        from . import tsne as _tsne
        out_Dir = os.path.join(hp.Speaker_Embedding.Train.Inference_Path, "PLOT").replace("\\", "/")
        result = export_tsne(embedding_Array, label_List, global_Step, out_Dir, file_Name,
                             lambda X, **kw: _tsne.tsne(X, device=self.device, **kw))
        if result is not None:
            self.embedding_Value = result["value"]
        return result
