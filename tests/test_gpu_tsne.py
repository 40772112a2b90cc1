"""Exact t-SNE on the GPU (csrc/tsne.hip through multi_speaker_tts_amd/tsne.py) against its fp64 statement (tsne.affinities_host,
joint_from_beta_host, gradient_host, iterate_host, which tests/test_cpu_tsne.py pins to scikit-learn), stage by stage, then the whole run
and the Export_TSNE surface.  Every parity figure is printed before it is asserted (run with -s to read them; profiles/tsne_parity.txt
keeps the figures of the MI355X).  The inputs are the cases of tests/tsne_cases.py.

Bounds: four times the figure measured on the MI355X - room for another summation order between builds, not for a defect - and beside each
one the ceiling above which a figure is a defect to be found, whatever was measured.

The whole-run cap: correct runs of this chaotic iteration end at different KL.  On the CPU, for the cases and seeds used here, the fp64
checker, its fp32 emulation and scikit-learn's TSNE(method='exact') ended at (python tools/tsne_cpu_spread.py, profiles/tsne_cpu_spread.txt)
    A seed 0: 0.1778 0.1846 0.1823   seed 1: 0.1786 0.1839 0.1841   seed 2: 0.1828 0.1818 0.1766
    B seed 0: 0.2044 0.2054 0.1953   seed 1: 0.2096 0.2072 0.2173   seed 2: 0.2088 0.2068 0.2108
the largest excess of one over another of the same case and seed being 5.15 % (B seed 0); the device's final KL may exceed the checker's
by twice that.  The maps' Embedding_Value against the true labels were 32.8 ... 33.6 (A) and 25.1 ... 25.6 (B)."""
import os

import numpy as np
import pytest
import torch

from multi_speaker_tts_amd import tsne as T
from multi_speaker_tts_amd.Speaker_Embedding import Embedding_Value
import tsne_cases as TC

pytestmark = pytest.mark.gpu

# measured on the MI355X (profiles/tsne_parity.txt), the largest figure over the cases of each test
MEASURED_H_SLACK = 2.030e-7     # test_affinities, E: how far past 1e-5 the fp64 entropy of a row lies that the fp32 evaluation accepted
MEASURED_P = 4.233e-7           # test_affinities, B
MEASURED_GRAD = 1.455e-6        # test_gradient_at_a_developed_state, B at e = 1 (n 4096: 2.2e-7)
MEASURED_KL = 3.002e-6          # the same test, A at e = 1
MEASURED_SCHEDULE = 7.634e-5    # test_schedule from iteration 0, B, the update (Y 3.3e-5)
MEASURED_SCHEDULE_SWITCH = 4.342e-5     # from iteration 245, B, the update (Y 7.9e-6)
DEFECT_P, DEFECT_GRAD, DEFECT_SCHEDULE = 1e-5, 4.5e-5, 1e-3
CPU_SPREAD = 0.0515


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def up(a, dev):
    return torch.from_numpy(np.array(a, np.float32, order="C")).to(dev)


def f64(t):
    return t.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("name", list(TC.CASES))
def test_affinities(dev, name):
    """Stage A.  The search stops at a threshold, so an fp32 evaluation of H may stop a step earlier or later than fp64 and P is not
    compared with affinities_host's; instead (1) the entropy recomputed in fp64 from the device's beta lies within 1e-5 + slack of
    ln(perplexity) in every row, the slack being the error of the fp32 evaluation of H; (2) P agrees with joint_from_beta_host(X,
    beta_device), of max P; (3) P is symmetric bit for bit, its diagonal at the floor, its sum within 1e-5 of 1, everything finite -
    the duplicate rows of B included, whose mutual entry is the largest of their rows."""
    X, perplexity = TC.case(name)
    n = X.shape[0]
    P, beta = T.affinities_device(X, perplexity, dev)
    assert P.shape == (n, n) and beta.shape == (n,) and P.dtype == beta.dtype == torch.float32
    Pd, bd = f64(P), f64(beta)
    assert np.isfinite(Pd).all() and np.isfinite(bd).all() and (bd > 0).all()
    D = T.distances_host(X)
    excess = float(np.abs(T.entropy_host(D, bd) - np.log(perplexity)).max()) - T.SEARCH_TOL
    beta_host = TC.host_affinities(name)[1]
    want = T.joint_from_beta_host(X, bd)
    err = float(np.abs(Pd - want).max() / want.max())
    print("tsne gpu: affinities %s (n %d): |H(beta_device) - ln perplexity| - 1e-5 = %.3e; beta against the fp64 search %.3e relative; "
          "P against joint_from_beta_host %.3e of max P; sum P - 1 = %.3e"
          % (name, n, excess, float(np.abs(bd / beta_host - 1).max()), err, Pd.sum() - 1.0))
    assert excess <= 4 * MEASURED_H_SLACK
    assert err < DEFECT_P, ("a defect, not a bound to be widened", err)
    assert err < 4 * MEASURED_P
    assert torch.equal(P, P.t()) and bool((torch.diagonal(P) == np.float32(T.FLOOR)).all()) and float(P.min()) == np.float32(T.FLOOR)
    assert abs(Pd.sum() - 1.0) < 1e-5
    if name == "B":
        assert D[3, 5] == 0.0 and Pd[3, 5] == Pd[3].max() and Pd[5, 3] == Pd[5].max()


def _one_gradient(dev, P32, Y32, exaggeration):
    """The device's gradient and KL at the map Y32 for the joint probabilities P32 (float32 arrays): one iteration of mstts_tsne_iterate
    numbered past every switch (or before, for an exaggerated P), its gradient output and its history entry."""
    P, Y = up(P32, dev), up(Y32, dev)
    state = (Y, torch.zeros_like(Y), torch.ones_like(Y))
    g = torch.empty_like(Y)
    first = 0 if exaggeration != 1.0 else 1000
    hist = T.iterate_device(state, P, first, 1, exaggeration, 250, 1.0, grad=g)
    h = f64(hist)
    assert h.shape == (1, 2)
    return f64(g), h[0, 0], h[0, 1], f64(state[0]), f64(state[1]), f64(state[2])


@pytest.mark.parametrize("name", ["A", "B", "E"])
def test_gradient_at_a_developed_state(dev, name):
    """One gradient where the map has structure: the fp64 checker's Y after 300 iterations, rounded to float32 like P, uploaded.  Device
    gradient, KL and |g|_2 against gradient_host on the same rounded inputs, the gradient relative to max |g|; at an exaggerated P too.
    The ruler: an fp32 evaluation on the CPU differs from fp64 by 1.5e-6 ... 4.5e-6 of max |g|.  The state after that one step (update =
    -0.8 lr g, gains 0.8, Y + update) is checked against the device's own gradient."""
    (Y300, _, _), _ = TC.host_state(name, 300)
    P32, Y32 = TC.host_affinities(name)[0].astype(np.float32), Y300.astype(np.float32)
    for e in (1.0, 12.0):
        g, kl, gn, Y1, U1, G1 = _one_gradient(dev, P32, Y32, e)
        kl_want, g_want = T.gradient_host(Y32.astype(np.float64), P32.astype(np.float64), e)
        eg = float(np.abs(g - g_want).max() / np.abs(g_want).max())
        ek, en = abs(kl - kl_want) / abs(kl_want), abs(gn - np.linalg.norm(g_want)) / np.linalg.norm(g_want)
        print("tsne gpu: gradient %s (n %d) e %g: gradient %.3e of max |g| = %.3e; KL %.6f against %.6f: %.3e relative; |g|_2 %.3e relative"
              % (name, Y32.shape[0], e, eg, np.abs(g_want).max(), kl, kl_want, ek, en))
        assert eg < DEFECT_GRAD, ("a defect, not a bound to be widened", eg)
        assert eg < 4 * MEASURED_GRAD and ek < 4 * MEASURED_KL and en < 4 * MEASURED_GRAD
        assert np.all(G1 == np.float32(0.8)) and np.allclose(U1, -0.8 * g, rtol=1e-6, atol=0) and np.allclose(Y1, Y32 + U1, rtol=1e-6, atol=0)


def test_gradient_at_the_envelope_edge(dev):
    """n = 4096, once: a synthetic symmetric normalised P (no search) and a random map of scale 10."""
    n = T.MAX_N
    g = np.random.default_rng(12)
    S = g.random((n, n)) ** 4
    S = S + S.T
    np.fill_diagonal(S, 0.0)
    P32 = np.maximum(S / S.sum(), T.FLOOR).astype(np.float32)
    Y32 = (10.0 * g.normal(size=(n, 2))).astype(np.float32)
    got, kl, gn, _, _, _ = _one_gradient(dev, P32, Y32, 1.0)
    kl_want, g_want = T.gradient_host(Y32.astype(np.float64), P32.astype(np.float64), 1.0)
    eg, ek = float(np.abs(got - g_want).max() / np.abs(g_want).max()), abs(kl - kl_want) / abs(kl_want)
    print("tsne gpu: gradient at n 4096: %.3e of max |g| = %.3e; KL %.6f against %.6f: %.3e relative" % (eg, np.abs(g_want).max(), kl, kl_want, ek))
    assert eg < DEFECT_GRAD, ("a defect, not a bound to be widened", eg)
    assert eg < 4 * MEASURED_GRAD and ek < 4 * MEASURED_KL


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("first", [0, 245])
def test_schedule(dev, name, first):
    """Ten iterations from the fp64 checker's state (Y, update, gains) at iteration 0 and at iteration 245 - across the switch of exaggeration
    and momentum and the fresh update / gains at 250 - against iterate_host from the same float32-rounded state and P: Y, update and gains,
    each of its own largest magnitude.  A switch at the wrong iteration, a wrong momentum or gain rule or a missing factor 4 moves these by
    orders of magnitude; the ruler for rounding alone is 6e-6 ... 1.2e-4 of max |Y| on the CPU, growing with every iteration."""
    state, _ = TC.host_state(name, first) if first else (T.initial_state(T.random_init(TC.case(name)[0].shape[0], 0)), None)
    P32 = TC.host_affinities(name)[0].astype(np.float32)
    s32 = [np.asarray(a, np.float32) for a in state]
    lr = TC.learning_rate(name)
    want, hist_want = T.iterate_host([a.astype(np.float64) for a in s32], P32.astype(np.float64), first, 10, 12.0, 250, lr)
    P = up(P32, dev)
    got = tuple(up(a, dev) for a in s32)
    hist = f64(T.iterate_device(got, P, first, 10, 12.0, 250, lr))
    errs = [float(np.abs(f64(a) - w).max() / np.abs(w).max()) for a, w in zip(got, want)]
    assert hist.shape == (len(hist_want), 2) and hist.shape[0] == (2 if first else 1)
    ek = max(abs(h[0] - w[1]) / abs(w[1]) for h, w in zip(hist, hist_want))
    print("tsne gpu: schedule %s, iterations %d ... %d: Y %.3e, update %.3e, gains %.3e of their largest; KL %s against %s: %.3e relative"
          % (name, first, first + 9, errs[0], errs[1], errs[2], " ".join("%.5f" % h[0] for h in hist), " ".join("%.5f" % w[1] for w in hist_want), ek))
    assert max(errs) < DEFECT_SCHEDULE, ("a defect, not a bound to be widened", errs)
    assert max(errs) < 4 * (MEASURED_SCHEDULE_SWITCH if first else MEASURED_SCHEDULE) and ek < DEFECT_SCHEDULE


@pytest.mark.parametrize("name", ["A", "B"])
def test_whole_run(dev, name):
    """1 000 iterations, three seeds.  Trajectories are not comparable (fp32 and fp64 have diverged by iteration 50 on the CPU too), the
    results are: the device's final KL is at most the fp64 checker's times 1 + twice the largest excess between correct CPU runs (module
    docstring); its own KL figure agrees with the fp64 KL of its map; the map's Embedding_Value against the true labels is at least half
    the checker map's; the KL history does not rise by more than 1 % from iteration 300 on."""
    X, perplexity = TC.case(name)
    labels = TC.labels(name)
    P64 = TC.host_affinities(name)[0]
    for seed in (0, 1, 2):
        (Yh, _, _), hist_h = TC.host_state(name, 1000, seed)
        Y, info = T.tsne(X, perplexity, seed=seed, device=dev, return_info=True)
        assert Y.shape == Yh.shape and Y.dtype == np.float32 and np.isfinite(Y).all() and info["n_iter"] == 1000
        its = [it for it, _ in info["kl_history"]]
        assert its == [it for it, _, _ in hist_h] == list(range(49, 1000, 50))
        kl, kl_h = info["kl_divergence"], hist_h[-1][1]
        kl64 = T.gradient_host(Y.astype(np.float64), P64)[0]
        v, v_h = float(Embedding_Value(Y, labels)), float(Embedding_Value(Yh, labels))
        late = [k for it, k in info["kl_history"] if it >= 299]
        rise = max(b / a for a, b in zip(late[:-1], late[1:]))
        print("tsne gpu: whole run %s seed %d: KL %.4f (fp64 of the device map, host P: %.4f) against the checker's %.4f, cap %.4f; "
              "Embedding_Value %.1f against %.1f; largest KL ratio between reports from 300 on %.4f; KL at 50 / 250 / 300: %.3f %.3f %.3f"
              % (name, seed, kl, kl64, kl_h, kl_h * (1 + 2 * CPU_SPREAD), v, v_h, rise, info["kl_history"][0][1], info["kl_history"][4][1],
                 info["kl_history"][5][1]))
        assert kl <= kl_h * (1 + 2 * CPU_SPREAD)
        # KL = sum p ln p - sum p ln num + ln Z sum p: three terms of magnitude ~10 that leave ~0.2, each an fp32 sum good to ~1e-6 of
        # itself, and a P whose rows met the entropy to 1e-5 at another beta than the host's: a few 1e-5 of 10, 1e-3 of the result
        assert abs(kl - kl64) < 1e-3 * kl64
        assert v >= 0.5 * v_h
        assert rise <= 1.01
        assert len(info["grad_norm_history"]) == 20 and all(np.isfinite(g) and g > 0 for _, g in info["grad_norm_history"])


def test_reproducible(dev):
    """The same call twice: the same bits, map and history; another seed: another map."""
    X, perplexity = TC.case("B")
    a, ia = T.tsne(X, perplexity, max_iter=300, device=dev, return_info=True)
    b, ib = T.tsne(X, perplexity, max_iter=300, device=dev, return_info=True)
    c = T.tsne(X, perplexity, max_iter=300, seed=1, device=dev)
    assert np.array_equal(a, b) and ia["kl_history"] == ib["kl_history"] and ia["grad_norm_history"] == ib["grad_norm_history"]
    assert np.array_equal(ia["beta"], ib["beta"]) and not np.array_equal(a, c)
    d = T.tsne(X, perplexity, max_iter=300, init=T.random_init(X.shape[0], 0), device=dev)
    assert np.array_equal(a, d)


def test_device_refusals(dev):
    """What the host refuses before any launch (MSTTS_ERR_SHAPE through lib.call): shapes outside the envelope, a history buffer too short."""
    from multi_speaker_tts_amd import lib
    X, _ = TC.case("D")
    for bad in (dict(X=X[:3], perplexity=1.0), dict(X=X, perplexity=4.0), dict(X=X, perplexity=0.5)):
        with pytest.raises(lib.MsttsError):
            T.affinities_device(bad["X"], bad["perplexity"], dev)
    P = up(TC.host_affinities("D")[0], dev)
    Y = up(T.random_init(4, 0), dev)
    ws, hist = torch.empty(32, device=dev), torch.zeros(2, device=dev)
    with pytest.raises(lib.MsttsError):
        lib.call("mstts_tsne_iterate", lib.ptr(P), 4, lib.ptr(Y), lib.ptr(Y), lib.ptr(Y), 0, 100, 250, 12.0, 50.0, lib.ptr(ws), lib.ptr(hist), 1, None)
    with pytest.raises(lib.MsttsError):
        lib.call("mstts_tsne_iterate", lib.ptr(P), 4, lib.ptr(Y), lib.ptr(Y), lib.ptr(Y), 0, 0, 250, 12.0, 50.0, lib.ptr(ws), lib.ptr(hist), 1, None)
    with pytest.raises(ValueError):
        T.iterate_device((Y, Y, Y[:2]), P, 0, 1)


def test_surface(dev, tmp_path, monkeypatch):
    """Speaker_Embedding.Inference(mel_List, export_TSNE=True, label_List=...): PLOT/GS_<step>.npz (and .PNG with matplotlib) under
    Inference_Path; without export_TSNE the same embeddings bit for bit and no file."""
    from multi_speaker_tts_amd import Hyper_Parameters as hp
    from multi_speaker_tts_amd.Speaker_Embedding import Speaker_Embedding
    from multi_speaker_tts_amd.params import Dims
    monkeypatch.setattr(hp.Speaker_Embedding.Train, "Inference_Path", str(tmp_path / "out"))
    dims = Dims(emb=32, enc_conv_ch=32, enc_lstm=16, spk=64, prenet=16, dec_lstm=32, post_ch=16, bank_ch=8, proj1_ch=16, birnn=8, n_spec=20,
                spk_lstm=64, max_inf=4)
    m = Speaker_Embedding(is_Training=False, device=dev, dims=dims)
    g = np.random.default_rng(3)
    base = g.normal(size=(4, 1, 80))
    labels = ["s%d" % (i % 4) for i in range(12)]
    mels = [np.clip(base[i % 4] + 0.5 * g.normal(size=(70 + 5 * i, 80)), -4, 4).astype(np.float32) for i in range(12)]
    plain = m.Inference(mels, label_List=labels)
    value = m.embedding_Value
    assert plain.shape == (12, 64) and not os.path.exists(str(tmp_path / "out"))
    with pytest.raises(ValueError):
        m.Inference(mels, export_TSNE=True)
    emb = m.Inference(mels, export_TSNE=True, label_List=labels)
    assert np.array_equal(emb, plain) and m.embedding_Value == value
    stem = str(tmp_path / "out" / "PLOT" / "GS_{}".format(m.engine.global_step))
    with np.load(stem + ".npz") as z:
        assert z["Y"].shape == (12, 2) and np.isfinite(z["Y"]).all() and list(z["labels"]) == labels
        assert float(z["value"]) == float(value) and float(z["kl_divergence"]) > 0 and int(z["global_Step"]) == m.engine.global_step
    try:
        import matplotlib      # noqa: F401
    except ImportError:
        assert not os.path.exists(stem + ".PNG")
    else:
        assert os.path.getsize(stem + ".PNG") > 0
    assert sorted(os.listdir(str(tmp_path / "out" / "PLOT"))) == sorted(os.path.basename(stem) + e for e in (".npz", ".PNG") if os.path.exists(stem + e))
