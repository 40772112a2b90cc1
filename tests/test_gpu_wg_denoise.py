"""The WaveGlow denoiser on the GPU (mstts_wg_denoise through Audio.spectral_denoise_batch) against its fp64 statement
Audio.spectral_denoise (which tests/test_cpu_wg_denoise.py pins against torch's stft / istft), the bias-spectrum plumbing of
WaveGlowEngine, `vocode(denoise=...)` and the surfaces.  Every parity figure is printed before it is asserted (run with -s to read them).
Errors are max |device - host| relative to the host INPUT's peak."""
import ctypes

import numpy as np
import pytest
import torch

from multi_speaker_tts_amd import Audio, lib
from multi_speaker_tts_amd import waveglow as WG
from oracle import waveglow as OW

pytestmark = pytest.mark.gpu

PARAMS = [(1024, 256, 1024), (512, 128, 512), (2048, 200, 800)]           # the last: a window shorter than n_fft
STRENGTHS = (0.0, 0.1, 1.0)
# Bound: four times the figure measured on the MI355X (profiles/wg_denoise_parity.txt) - room for another order of the FFT factorisation
# between builds, not for a defect.  The ruler is Griffin-Lim's one-iteration figure for the same stft / istft pair, 5.4e-7 of the peak
# (tests/test_gpu_griffin_lim.py); a figure above ten times that would be a defect to be found.
MEASURED = 3.282e-07      # the largest figure of test_op_parity (n_fft 512, strength 0)
BOUND = 4 * MEASURED
RULER = 5.4e-7


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def lengths(n_fft, hop):
    return (n_fft // 2 + 1, 37 * hop + 19, 121 * hop)                      # the shortest admitted, no multiple of hop, a multiple of hop


def tone_plus_noise(n, seed):
    """A tone of amplitude 0.3 (its frequency depends on the seed) in white noise of deviation 0.05."""
    g = np.random.default_rng(seed)
    f = 0.01 + 0.02 * (seed % 7)
    return (0.3 * np.sin(2 * np.pi * f * np.arange(n) + seed) + 0.05 * g.normal(size=n)).astype(np.float32)


@pytest.fixture(scope="module")
def sets():
    """Per parameter set: nine waveforms (three lengths x three seeds), the bias = the per-bin median of their own |X| over all their
    frames (fp64), and the host results per strength - computed once, shared by the tests below, never written to."""
    out = {}
    for n_fft, hop, win in PARAMS:
        wavs = [tone_plus_noise(n, 10 * i + s) for i, n in enumerate(lengths(n_fft, hop)) for s in range(3)]
        mags = [np.abs(Audio._stft_samples(w.astype(np.float64), n_fft, hop, win)) for w in wavs]
        bias = np.median(np.concatenate(mags, axis=1), axis=1).astype(np.float32)
        clamped = float(np.mean(np.concatenate(mags, axis=1) < bias.astype(np.float64)[:, None]))
        want = {s: [Audio.spectral_denoise(w.astype(np.float64), bias.astype(np.float64), s, n_fft, hop, win) for w in wavs] for s in STRENGTHS}
        for v in want.values():
            for y in v:
                y.setflags(write=False)
        out[(n_fft, hop, win)] = (wavs, bias, want, clamped)
    return out


@pytest.mark.parametrize("n_fft,hop,win", PARAMS)
def test_op_parity(dev, sets, n_fft, hop, win):
    """Nine waveforms in one call per strength (0, 0.1, 1) against Audio.spectral_denoise.  At strength 1 both branches of the clamp
    run: the share of clamped bins on the fp64 side lies in [0.2, 0.8] (0.50 by construction of the bias).
    Measured on the MI355X, the largest of the nine, of the input's peak, at strengths 0 / 0.1 / 1: n_fft 1024: 3.000e-07, 2.732e-07,
    2.574e-07; n_fft 512: 3.282e-07, 2.837e-07, 2.511e-07; n_fft 2048 (win 800): 2.668e-07, 2.754e-07, 2.219e-07 - all below the ruler
    (profiles/wg_denoise_parity.txt)."""
    wavs, bias, want, clamped = sets[(n_fft, hop, win)]
    print("wg_denoise parity: n_fft %d hop %d win %d: share of clamped bins at strength 1: %.3f" % (n_fft, hop, win, clamped))
    assert 0.2 <= clamped <= 0.8
    worst = {}
    for s in STRENGTHS:
        got = Audio.spectral_denoise_batch(wavs, bias, s, n_fft, hop, win, device=dev)
        assert len(got) == len(wavs)
        errs = []
        for x, y, w in zip(wavs, got, want[s]):
            assert y.dtype == np.float32 and y.shape == x.shape == w.shape and np.isfinite(y).all()
            errs.append(float(np.abs(y - w).max() / np.abs(x).max()))
        worst[s] = max(errs)
        print("wg_denoise parity: n_fft %d hop %d win %d strength %.1f: %s -> %.3e of the peak"
              % (n_fft, hop, win, s, " ".join("%.2e" % e for e in errs), worst[s]))
    # the subtraction does something: strength 1 moves the signal by far more than the parity bound
    assert max(float(np.abs(a - b).max()) for a, b in zip(want[1.0], want[0.0])) > 0.01
    for s in STRENGTHS:
        assert worst[s] < 10 * RULER, ("a defect, not a bound to be widened", s, worst[s])
        assert worst[s] < BOUND, (s, worst[s], BOUND)


def test_batch_equals_singles(dev, sets):
    """Each waveform alone and in the batch: equal bits; the output is as long as the input, also where that is no multiple of hop;
    device tensors in, device tensors out."""
    for (n_fft, hop, win), (wavs, bias, _, _) in sets.items():
        pick = [0, 4, 8]                                                   # one of each length
        both = Audio.spectral_denoise_batch([wavs[i] for i in pick], bias, 1.0, n_fft, hop, win, device=dev)
        assert [y.shape[0] for y in both] == list(lengths(n_fft, hop)) and both[1].shape[0] % hop != 0
        for k, i in enumerate(pick):
            alone, = Audio.spectral_denoise_batch([wavs[i]], bias, 1.0, n_fft, hop, win, device=dev)
            assert np.array_equal(alone, both[k]), (n_fft, i)
        t_out = Audio.spectral_denoise_batch([torch.as_tensor(wavs[i]).to(dev) for i in pick], torch.as_tensor(bias).to(dev), 1.0, n_fft, hop, win,
                                             device=dev, return_tensor=True)
        assert all(torch.is_tensor(y) and y.is_cuda and np.array_equal(y.cpu().numpy(), b) for y, b in zip(t_out, both))


def test_refusals_by_return_code(dev):
    """Nothing is launched: the C entry returns MSTTS_ERR_SHAPE (lib.MsttsError) naming the cause, and the Python surface raises before it
    gets there."""
    buf = torch.zeros(4096, device=dev)
    off = torch.tensor([0, 1024, 1536, 0, 5, 8], dtype=torch.int64, device=dev)

    def raw(host, nw, strength, n_fft, hop, win):
        lib.call("mstts_wg_denoise", lib.ptr(buf), (ctypes.c_int64 * len(host))(*host), lib.ptr(off), lib.ptr(off, 3), nw, lib.ptr(buf), strength,
                 lib.ptr(buf), lib.ptr(buf), n_fft, hop, win, lib.ptr(buf), lib.ptr(buf))
    with pytest.raises(lib.MsttsError, match="waveform 1 has 512 samples"):          # n = n_fft / 2
        raw([0, 1024, 1536], 2, 1.0, 1024, 256, 1024)
    with pytest.raises(lib.MsttsError, match="2 hop <= win"):                          # win < 2 hop
        raw([0, 1024, 2048], 2, 1.0, 1024, 513, 1024)
    with pytest.raises(lib.MsttsError, match=r"n_fft must be a power of two in \[512, 4096\]"):
        raw([0, 1024, 2048], 2, 1.0, 256, 64, 256)
    with pytest.raises(lib.MsttsError, match="strength -0.5 is negative"):
        raw([0, 1024, 2048], 2, -0.5, 1024, 256, 1024)
    x = np.zeros(2000, np.float32)
    with pytest.raises(ValueError, match="waveform 1: 512 samples"):
        Audio.spectral_denoise_batch([x, x[:512]], np.zeros(513, np.float32), 1.0, device=dev)
    with pytest.raises(ValueError, match="negative"):
        Audio.spectral_denoise_batch([x], np.zeros(513, np.float32), -1.0, device=dev)
    with pytest.raises(ValueError, match="513"):
        Audio.spectral_denoise_batch([x], np.zeros(512, np.float32), 1.0, device=dev)
    # outside the device envelope the host function answers, waveform by waveform
    assert not Audio.spectral_denoise_supported(256, 64, 256)
    y, = Audio.spectral_denoise_batch([x + 0.5], np.ones(129, np.float32), 0.0, 256, 64, 256, device=dev)
    assert y.dtype == np.float32 and np.abs(y - 0.5).max() < 1e-6


# The engine tests run the dims of tests/test_gpu_waveglow.py's CFGS[0] with a wider upsampler (kernel 192, stride 64 instead of 16 / 4):
# the denoiser's smallest transform is n_fft = 512, which needs waveforms of more than 256 samples, and CFGS[0] itself makes 24 samples
# out of a 3-frame chunk and 44 out of 8 bias frames.  With 192 / 64 a 3-frame chunk has 320 samples and the 8-frame bias waveform 640.
CFG = dict(n_mel=8, flows=4, groups=8, early_every=2, early_size=2, up_k=192, up_stride=64, layers=3, ch=32, k=3)
DN = dict(n_fft=512, hop=128, win=512, frames=8)


def small_values(seed=4):
    """The oracle's trained-like variables: a non-zero output conv, so the flow is not the identity and has a bias signal."""
    return OW.init_params(OW.WGDims(**CFG), seed=seed)


@pytest.fixture(scope="module")
def engine(dev):
    return WG.WaveGlowEngine(WG.WGDims(**CFG), device=dev, values=small_values())


def test_engine_bias_spectrum(dev, engine):
    """bias_spectrum() = |rfft| of frame 0 of the device's own bias waveform (fp64 on the host) within the parity bound scaled to the
    spectrum's peak (the transform's error grows with the sum of the windowed samples as the spectrum does); cached per argument tuple
    and arithmetic; load() drops the cache.  Measured: 1.153e-07 (f32), 6.775e-08 (bf16) of the spectrum's peak."""
    d = engine.d
    L = (DN["frames"] - 1) * d.up_stride + d.up_k
    zeros = lambda width: np.zeros((1, L // d.groups, width), np.float32)
    noise = {"z": zeros(d.z_channels), "early_2": zeros(d.early_size)}
    got = {}
    for arith in WG.ARITHS:
        b = engine.bias_spectrum(arith=arith, **DN)
        assert torch.is_tensor(b) and b.is_cuda and b.shape == (DN["n_fft"] // 2 + 1,) and b.dtype == torch.float32
        assert engine.bias_spectrum(arith=arith, **DN) is b                                            # the cached tensor
        wav = engine.infer(np.zeros((1, DN["frames"], d.n_mel), np.float32), noise=noise, arith=arith).cpu().numpy().reshape(-1).astype(np.float64)
        assert wav.shape == (L,) and np.abs(wav).max() > 0
        want = np.abs(Audio._stft_samples(wav, DN["n_fft"], DN["hop"], DN["win"]))[:, 0]
        e = float(np.abs(b.cpu().numpy() - want).max() / want.max())
        print("wg_denoise bias spectrum (%s): %.3e of the spectrum's peak (peak %.3e, waveform peak %.3e)" % (arith, e, want.max(), np.abs(wav).max()))
        assert e < BOUND, (arith, e)
        got[arith] = b
    assert got["f32"] is not got["bf16"]                                                               # per arithmetic
    assert engine.bias_spectrum(**DN) is got["f32"]                                                    # None resolves to the engine's default
    other = engine.bias_spectrum(arith="f32", n_fft=512, hop=128, win=512, frames=8, mel_value=0.5)
    assert other is not got["f32"] and not torch.equal(other, got["f32"])                              # per argument tuple
    engine.load(small_values())
    again = engine.bias_spectrum(arith="f32", **DN)
    assert again is not got["f32"] and torch.equal(again, got["f32"])                                  # recomputed from the same values
    with pytest.raises(ValueError, match="reflect padding"):
        engine.bias_spectrum(n_fft=2048, hop=512, win=2048, frames=8)                                  # 640 samples <= 1024


def test_vocode_denoise(dev, engine, monkeypatch):
    """The workload of test_vocode_chunking (mels of 7, 3 and 10 frames, split 3, batch 2, one seed): denoise None / 0.0 / no argument give
    equal bits; 0.5 is Audio.spectral_denoise of the undenoised result with the engine's bias, within the parity bound.  Measured: 2.141e-07,
    1.349e-07, 1.702e-07 of the peak, where the denoiser itself moves the waveforms by 1e-2 of it."""
    monkeypatch.delenv("MSTTS_WG_DENOISE", raising=False)
    g = np.random.default_rng(1)
    mels = [g.normal(0, 1, (t, engine.d.n_mel)).astype(np.float32) for t in (7, 3, 10)]
    args = {k: DN[k] for k in ("n_fft", "hop", "win", "frames")}
    run = lambda **kw: WG.vocode(engine, mels, split=3, batch=2, noise_seed=11, **kw)
    plain = run()
    per_chunk = (3 - 1) * engine.d.up_stride + engine.d.up_k
    assert [w.shape[0] for w in plain] == [3 * per_chunk, 1 * per_chunk, 4 * per_chunk]
    for other in (run(denoise=None), run(denoise=0.0), run(denoise=0.0, denoise_args=args)):
        assert all(np.array_equal(a, b) for a, b in zip(plain, other))
    got = run(denoise=0.5, denoise_args=args)
    bias = engine.bias_spectrum(**DN).cpu().numpy().astype(np.float64)
    assert bias.max() > 0
    for i, (x, y) in enumerate(zip(plain, got)):
        assert y.dtype == np.float32 and y.shape == x.shape and np.isfinite(y).all() and not np.array_equal(x, y)
        want = Audio.spectral_denoise(x.astype(np.float64), bias, 0.5, DN["n_fft"], DN["hop"], DN["win"])
        e = float(np.abs(y - want).max() / np.abs(x).max())
        moved = float(np.abs(want - x).max() / np.abs(x).max())
        print("wg_denoise vocode: utterance %d (%d samples): %.3e of the peak (the denoiser moved it by %.3e)" % (i, x.shape[0], e, moved))
        assert e < BOUND, (i, e)
    monkeypatch.setenv("MSTTS_WG_DENOISE", "0.5")                                                      # the environment stands in for the argument
    assert all(np.array_equal(a, b) for a, b in zip(got, run(denoise_args=args)))
    assert all(np.array_equal(a, b) for a, b in zip(plain, run(denoise=0.0)))
    # engine.denoise on host arrays is the same call
    again = engine.denoise(plain, 0.5, **DN)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))


def _wg_hp(monkeypatch, hp, tmp_path):
    """hp of test_tacotron2_inference_waveglow_surface, with an upsampler (kernel 512, stride 64) whose chunks are longer than the
    reflect padding of the denoiser's own transform (n_fft 1024: more than 512 samples)."""
    monkeypatch.setattr(hp, "Use_Vocoder", "WaveGlow")
    for k, v in dict(Flows=4, Early_Every=2).items():
        monkeypatch.setattr(hp.WaveGlow, k, v)
    monkeypatch.setattr(hp.WaveGlow.WaveNet, "Channels", 32)
    monkeypatch.setattr(hp.WaveGlow.WaveNet, "Layers", 2)
    monkeypatch.setattr(hp.WaveGlow.Upsample, "Kernel_Size", 512)
    monkeypatch.setattr(hp.WaveGlow.Upsample, "Strides", 64)
    monkeypatch.setattr(hp.WaveGlow.Inference, "Mel_Split_Length", 3)
    monkeypatch.setattr(hp.WaveGlow, "Checkpoint_Path", str(tmp_path / "wg"))


def _unzero_output_convs(eng, seed=7):
    """A randomly initialised WaveGlow has zero output convs and no bias signal: give it one."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    for F in eng.flow:
        for k in ("w_out", "b_out"):
            F[k].copy_((0.05 * torch.randn(F[k].shape, generator=g)).to(F[k].device))
    eng._bias = {}


def test_tacotron2_surface(dev, tmp_path, monkeypatch):
    """Tacotron2.Inference_WaveGlow(denoiser_strength=0.5): finite waveforms of unchanged lengths, Cut taken from them, the WAV written;
    MSTTS_WG_DENOISE=0.5 gives the same arrays; without either the result is the call's as it was before the argument existed."""
    from scipy.io import wavfile
    from multi_speaker_tts_amd import Hyper_Parameters as hp
    from multi_speaker_tts_amd.MSTTS_SV import Tacotron2
    from multi_speaker_tts_amd.params import Dims
    monkeypatch.delenv("MSTTS_WG_DENOISE", raising=False)
    monkeypatch.setattr(hp, "Checkpoint_Path", str(tmp_path / "ckpt"))
    monkeypatch.setattr(hp, "Inference_Path", str(tmp_path / "inf"))
    _wg_hp(monkeypatch, hp, tmp_path)
    dims = Dims(emb=32, enc_conv_ch=32, enc_lstm=16, spk=256, prenet=16, dec_lstm=32, post_ch=16, bank_ch=8, proj1_ch=16, birnn=8, n_spec=20,
                spk_lstm=256, max_inf=6)
    t = Tacotron2(is_Training=False, device=dev, dims=dims, allow_random_init=True)
    _unzero_output_convs(t.waveglow)
    mels = [np.clip(np.random.default_rng(i).normal(0, 1.5, (230, 80)), -4, 4).astype(np.float32) for i in range(2)]
    texts = ["Please call Stella.", "Who knows?"]
    run = lambda **kw: t.Inference_WaveGlow(None, texts, speaker_Mel_List=mels, noise_seed=3, **kw)
    plain = run(export=False)
    res = run(file_Prefix="dn", denoiser_strength=0.5)
    assert len(res["Wav"]) == 2
    for i in range(2):
        w = res["Wav"][i]
        assert w.dtype == np.float32 and w.shape == plain["Wav"][i].shape and np.isfinite(w).all() and not np.array_equal(w, plain["Wav"][i])
        n = res["Cut"][i]["Wav"].shape[0]
        assert n == plain["Cut"][i]["Wav"].shape[0] and np.array_equal(res["Cut"][i]["Wav"], w[:n])
        rate, back = wavfile.read(str(tmp_path / "inf" / "WAV" / ("dn.IDX_%d.WAV" % i)))
        assert rate == hp.WaveGlow.Export_Sample_Rate and np.array_equal(back, w[:n])
    direct = t.waveglow.denoise(plain["Wav"], 0.5)
    assert all(np.array_equal(a, b) for a, b in zip(direct, res["Wav"]))
    via = t.Inference(None, texts, speaker_Mel_List=mels, export=False, denoiser_strength=0.0)          # passes the argument through
    assert via["Wav"][0].shape == plain["Wav"][0].shape
    monkeypatch.setenv("MSTTS_WG_DENOISE", "0.5")
    env = run(export=False)
    assert all(np.array_equal(a, b) for a, b in zip(env["Wav"], res["Wav"]))
    monkeypatch.delenv("MSTTS_WG_DENOISE")
    # the call on the parent commit's signature: Inference_WaveGlow's body before the argument existed, restated
    from multi_speaker_tts_amd import waveglow as W
    chunks, index = W.split_mels(list(plain["Mel"]), 3)
    pat = np.zeros((len(chunks), max(c.shape[0] for c in chunks), 80), np.float32)
    for i, c in enumerate(chunks):
        pat[i, :c.shape[0]] = c
    B = hp.WaveGlow.Inference.Batch_Size
    old = np.concatenate([t.waveglow.infer(pat[b0:b0 + B], seed=3 + b0).cpu().numpy() for b0 in range(0, len(chunks), B)], axis=0)
    again = run(export=False)
    for i, (a, b) in enumerate(index):
        assert np.array_equal(old[a:b].reshape(-1), again["Wav"][i]) and np.array_equal(plain["Wav"][i], again["Wav"][i])


def test_waveglow_inference_surface(dev, tmp_path, monkeypatch):
    """WaveGlow.Inference(denoiser_strength=...): the denoiser runs before the peak normalisation - the files' peak is 1 - and the
    returned waveforms are the denoised ones."""
    from scipy.io import wavfile
    from multi_speaker_tts_amd import Hyper_Parameters as hp
    from multi_speaker_tts_amd.WaveGlow import WaveGlow
    monkeypatch.delenv("MSTTS_WG_DENOISE", raising=False)
    _wg_hp(monkeypatch, hp, tmp_path)
    monkeypatch.setattr(hp.WaveGlow.Inference, "Path", str(tmp_path / "out"))
    pd = WG.WGDims.from_hp(hp)
    values = WG.random_values(pd, seed=2)
    g = np.random.default_rng(5)
    for k in list(values):
        if "wavenet/conv1d/" in k:
            values[k] = (values[k] + g.normal(0, 0.05, values[k].shape)).astype(np.float32)
    rate = hp.WaveGlow.Export_Sample_Rate
    paths = []
    for i, sec in enumerate((0.3, 0.2)):
        n = int(rate * sec)
        y = 0.4 * np.sin(2 * np.pi * (180 + 60 * i) * np.arange(n) / rate) + 0.02 * g.normal(size=n)
        paths.append(str(tmp_path / ("v%d.wav" % i)))
        wavfile.write(paths[-1], rate, (y * 32767).astype(np.int16))
    m = WaveGlow(device=dev, dims=pd, values=values)
    plain = m.Inference(paths, file_Prefix="p")
    got = m.Inference(paths, file_Prefix="d", denoiser_strength=0.5)
    for i in range(2):
        assert got[i].shape == plain[i].shape and np.isfinite(got[i]).all() and not np.array_equal(got[i], plain[i])
        _, back = wavfile.read(str(tmp_path / "out" / "WAV" / ("d.IDX_%d.WAV" % i)))
        assert back.dtype == np.float32 and abs(float(np.abs(back).max()) - 1.0) < 1e-6
        assert np.array_equal(back, (got[i] / np.abs(got[i]).max()).astype(np.float32))
