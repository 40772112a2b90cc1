"""The fp64 statement of exact t-SNE (multi_speaker_tts_amd/tsne.py: the checker the device stages are judged against in
tests/test_gpu_tsne.py) pinned stage by stage to the installed scikit-learn, the refusals, and the engine-free half of Export_TSNE.
Every parity figure is printed before it is asserted (run with -s to read them)."""
import os

import numpy as np
import pytest

from multi_speaker_tts_amd import tsne as T
from tsne_cases import CASES, case


def _sk():
    pytest.importorskip("sklearn")
    from scipy.spatial.distance import squareform
    from sklearn.manifold import _t_sne, _utils
    return squareform, _t_sne, _utils


@pytest.mark.parametrize("name", ["A", "B"])
def test_conditional_rows_match_scikit_learn(name):
    """conditional_host (the rows affinities_host symmetrises) against scikit-learn's float32 search on the float32 distances.  Bound 1e-6
    absolute (rows peak at 0.34 / 0.58); measured 1.7e-7 on A, 4.1e-7 on B.  The joint P against _joint_probabilities, of its peak:
    3.6e-7 / 4.0e-7, bound 1e-6."""
    squareform, _t_sne, _utils = _sk()
    X, perplexity = case(name)
    D = T.distances_host(X)
    C, beta = T.conditional_host(D, perplexity)
    ref = _utils._binary_search_perplexity(D.astype(np.float32), float(perplexity), 0)
    err = float(np.abs(C - ref).max())
    print("tsne cpu: case %s conditional rows: %.3e absolute (peak %.3f)" % (name, err, ref.max()))
    assert np.all(np.diag(C) == 0.0) and np.allclose(C.sum(axis=1), 1.0, atol=1e-12) and np.all(beta > 0)
    assert np.abs(T.entropy_host(D, beta) - np.log(perplexity)).max() <= T.SEARCH_TOL
    assert err < 1e-6
    P, beta2 = T.affinities_host(X, perplexity)
    assert np.array_equal(beta, beta2) and np.array_equal(P, P.T) and np.all(np.diag(P) == T.FLOOR) and abs(P.sum() - 1.0) < 1e-9
    assert np.array_equal(P, T.joint_from_beta_host(X, beta))
    Pref = _t_sne._joint_probabilities(D.astype(np.float32), perplexity, 0)
    errj = float(np.abs(squareform(P, checks=False) - Pref).max() / Pref.max())
    print("tsne cpu: case %s joint P: %.3e of its peak" % (name, errj))
    assert errj < 1e-6
    if name == "B":                                  # the duplicate pair: distance exactly 0, the largest entry of both rows
        assert D[3, 5] == 0.0 and C[3, 5] == C[3].max() and np.isfinite(P).all()


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
@pytest.mark.parametrize("exaggeration", [1.0, 12.0])
def test_gradient_matches_scikit_learn(name, exaggeration):
    """gradient_host against _kl_divergence (exact) at a random map of scale 1, plain and exaggerated P: 1e-10 relative (measured:
    below 1e-15)."""
    squareform, _t_sne, _ = _sk()
    X, perplexity = case(name)
    n = X.shape[0]
    P, _ = T.affinities_host(X, perplexity)
    Y = np.random.default_rng(5).normal(size=(n, 2))
    kl, g = T.gradient_host(Y, P, exaggeration)
    kl_ref, g_ref = _t_sne._kl_divergence(Y.ravel().copy(), squareform(P, checks=False) * exaggeration, 1.0, n, 2)
    ek, eg = abs(kl - kl_ref) / abs(kl_ref), float(np.abs(g.ravel() - g_ref).max() / np.abs(g_ref).max())
    print("tsne cpu: case %s e %g: KL %.3e, gradient %.3e relative" % (name, exaggeration, ek, eg))
    assert ek < 1e-10 and eg < 1e-10
    assert T.gradient_host(Y, P, exaggeration, want_kl=False)[0] is None


def _sk_descent(_t_sne, squareform, P, Y0, n_total, lr, early_exaggeration, exaggeration_iters):
    """scikit-learn's two stages through _gradient_descent, called the way TSNE._tsne calls it (its early stops switched off)."""
    n = Y0.shape[0]
    Pc = squareform(P, checks=False)
    kw = dict(n_iter_check=50, min_grad_norm=0.0, learning_rate=lr, verbose=0, kwargs=dict(skip_num_points=0), n_iter_without_progress=10 ** 9)
    p, kl, it = _t_sne._gradient_descent(_t_sne._kl_divergence, Y0.ravel().copy(), it=0, max_iter=min(exaggeration_iters, n_total), momentum=0.5,
                                         args=[Pc * early_exaggeration, 1.0, n, 2], **kw)
    if n_total > exaggeration_iters:
        p, kl, it = _t_sne._gradient_descent(_t_sne._kl_divergence, p, it=it + 1, max_iter=n_total, momentum=0.8, args=[Pc, 1.0, n, 2], **kw)
    return p.reshape(n, 2), kl


@pytest.mark.parametrize("name", ["C", "D"])
def test_trajectory_matches_scikit_learn(name):
    """iterate_host against scikit-learn's descent.  The whole ``TSNE(method='exact', init=Y0, learning_rate='auto', max_iter=250)`` run
    cannot be the ruler: the dynamics are chaotic, and at 250 iterations two correct runs have diverged completely - measured here, the
    fp64 checker against scikit-learn's own _gradient_descent on the SAME fp64 P and fp64 state (tools/tsne_cpu_spread.py,
    profiles/tsne_cpu_spread.txt): D 1.3e-16 of max |Y| after 10 iterations, 2.0e-6 after 50, 0.78 after 100, 1.6 at 250; C 4.7e-14, 0.55,
    1.4, 0.83 (with scikit-learn's float32 state: 1.4e-7 / 6.3e-6 at 10, order 1 from 50 on).  So the
    comparison is through _gradient_descent directly, as TSNE._tsne calls it, where nothing has diverged yet: (a) 10 iterations of
    the early stage, (b) 5 early iterations + 7 late ones with exaggeration_iters = 5, which crosses the switch of exaggeration and
    momentum and the fresh update / gains scikit-learn enters its second stage with.  Bound 1e-9 of max |Y| (sixteen digits less the
    growth seen over 50 iterations); measured (a) 4.7e-14 (C), 1.3e-16 (D), (b) 9.1e-15 (C), 1.9e-16 (D)."""
    squareform, _t_sne, _ = _sk()
    X, perplexity = case(name)
    n = X.shape[0]
    P, _ = T.affinities_host(X, perplexity)
    lr = T.auto_learning_rate(n, 12.0)
    assert lr == 50.0
    Y0 = T.random_init(n, 0).astype(np.float64)
    for n_total, ex in ((10, 250), (12, 5)):
        want, kl_want = _sk_descent(_t_sne, squareform, P, Y0, n_total, lr, 12.0, ex)
        (Y, U, G), hist = T.iterate_host(T.initial_state(Y0), P, 0, n_total, 12.0, ex, lr)
        err = float(np.abs(Y - want).max() / np.abs(want).max())
        print("tsne cpu: case %s, %d iterations (switch at %d): %.3e of max |Y|, KL %.6f / %.6f" % (name, n_total, ex, err, hist[-1][1], kl_want))
        assert err < 1e-9
        assert hist[-1][0] == n_total - 1 and abs(hist[-1][1] - kl_want) < 1e-9 * abs(kl_want)
    # a run cut in two gives the same state as the run in one piece: the state is everything the iteration needs
    mid, _ = T.iterate_host(T.initial_state(Y0), P, 0, 5, 12.0, 5, lr)
    (Y2, U2, G2), _ = T.iterate_host(mid, P, 5, 7, 12.0, 5, lr)
    assert np.array_equal(Y2, Y) and np.array_equal(U2, U) and np.array_equal(G2, G)


def test_history_and_info():
    X, perplexity = case("D")
    Y, info = T.tsne_host(X, perplexity, max_iter=120, return_info=True)
    assert Y.shape == (4, 2) and Y.dtype == np.float32 and np.isfinite(Y).all()
    assert [it for it, _ in info["kl_history"]] == [49, 99, 119] == [it for it, _ in info["grad_norm_history"]]
    assert info["kl_divergence"] == info["kl_history"][-1][1] and info["n_iter"] == 120 and info["beta"].shape == (4,)
    assert np.array_equal(Y, T.tsne_host(X, perplexity, max_iter=120)) and not np.array_equal(Y, T.tsne_host(X, perplexity, max_iter=120, seed=1))
    assert np.array_equal(T.random_init(4, 0), (1e-4 * np.random.RandomState(0).standard_normal((4, 2))).astype(np.float32))


def test_refusals(capsys):
    assert T.tsne_supported(4, 1, 1) and T.tsne_supported(4096, 1024, 4095.5)
    assert not T.tsne_supported(3, 8, 1) and not T.tsne_supported(4097, 8, 30) and not T.tsne_supported(64, 0, 5)
    assert not T.tsne_supported(64, 1025, 5) and not T.tsne_supported(64, 8, 0.5) and not T.tsne_supported(64, 8, 64)
    from multi_speaker_tts_amd import lib
    L = lib.load()
    for n, dim, p in ((4, 1, 1), (4096, 1024, 4095.5), (3, 8, 1), (4097, 8, 30), (64, 0, 5), (64, 1025, 5), (64, 8, 0.5), (64, 8, 64)):
        assert bool(L.mstts_tsne_supported(n, dim, p)) == T.tsne_supported(n, dim, p)
    assert L.mstts_tsne_history_slots(0, 1000) == 20 and L.mstts_tsne_history_slots(245, 10) == 2 and L.mstts_tsne_history_slots(0, 10) == 1
    assert L.mstts_tsne_history_slots(0, 0) == 0 and L.mstts_tsne_history_slots(-1, 5) == 0
    assert L.mstts_tsne_affinities_ws_floats(653) == 653 * 654 and L.mstts_tsne_iterate_ws_floats(653) == 8 * 653
    X = case("D")[0]
    for fn in (T.tsne, T.tsne_host):
        with pytest.raises(ValueError):
            fn(X, perplexity=4)
        with pytest.raises(ValueError):
            fn(X, perplexity=0)
        with pytest.raises(ValueError):
            fn(X[0], perplexity=1)
        with pytest.raises(ValueError):
            fn(X, perplexity=1, init=np.zeros((3, 2)))
    # outside the envelope (three rows): one line, then the host path - no device is touched
    capsys.readouterr()
    Y = T.tsne(X[:3], perplexity=1, max_iter=20)
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "outside the device envelope" in out
    assert np.array_equal(Y, T.tsne_host(X[:3], perplexity=1, max_iter=20))


def _embeddings():
    g = np.random.default_rng(11)
    centres = g.normal(size=(3, 16))
    labels = ["p%d" % (i % 3) for i in range(24)]
    emb = np.stack([centres[i % 3] + 0.2 * g.normal(size=16) for i in range(24)]).astype(np.float32)
    return emb / np.linalg.norm(emb, axis=1, keepdims=True), labels


def test_export(tmp_path, capsys):
    """The module-level export with tsne_host: 24 embeddings of 3 labels, 60 iterations."""
    from multi_speaker_tts_amd.Speaker_Embedding import Embedding_Value, export_tsne
    emb, labels = _embeddings()
    seen = {}

    def short(X, **kw):
        seen.update(kw)
        return T.tsne_host(X, max_iter=60, **kw)
    out = str(tmp_path / "PLOT")
    r = export_tsne(emb, labels, 1234, out, "GS_1234", short)
    text = capsys.readouterr().out
    V = float(Embedding_Value(emb, labels))
    assert seen == {"perplexity": 23 / 3.0, "seed": 0, "return_info": True} and "perplexity 7.66667" in text        # 30 >= 24
    assert r["value"] == V and r["title"] == "Global step: 1234    t-SNE Result    V: {:0.5f}".format(V) and r["perplexity"] == 23 / 3.0
    assert r["npz"] == os.path.join(out, "GS_1234.npz")
    with np.load(r["npz"]) as z:
        assert z["Y"].shape == (24, 2) and np.isfinite(z["Y"]).all() and list(z["labels"]) == labels
        assert float(z["value"]) == V and int(z["global_Step"]) == 1234 and float(z["kl_divergence"]) == r["kl_divergence"] > 0
    try:
        import matplotlib      # noqa: F401
    except ImportError:
        assert r["png"] is None and "matplotlib is not installed" in text
    else:
        from PIL import Image
        assert r["png"] == os.path.join(out, "GS_1234.PNG") and os.path.getsize(r["png"]) > 0
        with Image.open(r["png"]) as im:
            assert im.size == (1000, 1000) and im.format == "PNG"
    with pytest.raises(ValueError):
        export_tsne(emb, labels[:-1], 0, out, "X", short)


def test_export_survives_an_unwritable_path(tmp_path, capsys):
    from multi_speaker_tts_amd.Speaker_Embedding import export_tsne
    emb, labels = _embeddings()
    blocker = tmp_path / "file"
    blocker.write_text("not a directory")
    r = export_tsne(emb, labels, 0, str(blocker / "PLOT"), "TSNE", lambda X, **kw: T.tsne_host(X, max_iter=5, **kw))
    assert r is None and "export skipped" in capsys.readouterr().out


def test_export_of_very_few_embeddings(tmp_path, capsys):
    """Three embeddings: perplexity (3 - 1) / 3, below the device envelope, still a map."""
    from multi_speaker_tts_amd.Speaker_Embedding import export_tsne
    emb, labels = _embeddings()
    r = export_tsne(emb[:3], ["a", "a", "b"], 7, str(tmp_path), "T3", lambda X, **kw: T.tsne_host(X, max_iter=5, **kw))
    assert r is not None and abs(r["perplexity"] - 2 / 3.0) < 1e-12 and np.load(r["npz"])["Y"].shape == (3, 2)


def test_inference_refuses_export_without_labels():
    import inspect
    from multi_speaker_tts_amd.Speaker_Embedding import Speaker_Embedding
    assert list(inspect.signature(Speaker_Embedding.Export_TSNE).parameters) == ["self", "embedding_Array", "label_List", "global_Step", "file_Name"]
    assert inspect.signature(Speaker_Embedding.Export_TSNE).parameters["file_Name"].default == "TSNE"
    src = inspect.getsource(Speaker_Embedding.Inference)
    assert src.index("export_TSNE needs a label_List") < src.index("InferEngine(")       # refused before any engine is made


def test_cases_are_what_they_say():
    for name, (sizes, dim, perplexity, seed) in CASES.items():
        X, p = case(name)
        assert X.shape == (sum(sizes), dim) and X.dtype == np.float32 and p == perplexity and not X.flags.writeable
        assert np.allclose(np.linalg.norm(X.astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert np.array_equal(case("B")[0][5], case("B")[0][3]) and case("B")[0].shape[0] % 64 and case("E")[0].shape[0] > 1024
