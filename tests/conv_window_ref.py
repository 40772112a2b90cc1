"""fp64 checker of the conv-window GEMMs (tests/test_gpu_conv_window_ref.py; pinned without a GPU by tests/test_cpu_conv_window_ref.py).

Every convolution of the four trainers is mstts_gemm_f32 / mstts_gemm_bf16 in window mode (include/mstts.h, win_T > 0); one conv block issues
three such products (training.conv_fwd / conv_bn_bwd, waveglow_trainer).  Here they are stated in plain NumPy with the window view as an
explicit per-tap slice copy - tap j of output frame t reads frame t + (j - pad) * dil of the SAME sequence, zero outside its length T; no
unfold, no conv1d - on float32 arrays x [B, T, cin], w [K, cin, cout], bias [cout], dz [B, T, cout], dw0 [K, cin, cout], dx0 [B, T, cin] drawn
once per case from a fixed seed:
    y      = act(win(x, pad) . w + bias)                 pad = (K - 1) // 2: SAME padding, left (K-1)//2, right K-1-left (quirk Q12)
    dw     = dw0 + win(x, pad)^T . dz                    the weight gradient lands on a pre-filled slab (split_k >= 2: atomic adds)
    dx     = win(dz, K - 1 - pad) . flip(w)              flip(w)[K-1-k][o][c] = w[k][c][o]: what mstts_conv_kernel_flip writes
    dx_acc = dx0 + dx                                    the `accumulate` form
evaluate(..., dtype=np.float32) evaluates the same statements in float32 (its worst slice error is e32); rounded=True rounds both operands of
every product to bf16 (round to nearest even) before the product, the reference of the mstts_gemm_bf16 forms (as _bf does in test_gpu_ops.py).

Judging (slice_err, MARGIN, FLOOR of tests/lstm_seq_ref.py): every slice on its own scale - y, dx, dx_acc: each output row (b, t); dw: each
tap's [cin, cout] block - scale = max|ref slice| + 1e-3 max|ref|; the bound of a quantity is 8 x e32, never less than 1e-6."""
import functools

import numpy as np

from tests.lstm_seq_ref import FLOOR, MARGIN, slice_err      # noqa: F401  (the project's constants, not copies)

ACTS = {"none": 0, "relu": 1, "tanh": 2}                      # lib.ACT_* (asserted by the GPU test)
QUANTITIES = ("y", "dw", "dx", "dx_acc")

# B, T, cin -> cout, K, dil, act: each the smallest shape that reaches its path (rows = B T).  only: the quantities the case is there for.
CASES = {}
for _k in range(1, 9):
    # 165 rows: a second, ragged row tile, the sequence seams 33 / 66 / 99 / 132 inside the tiles; win_C = 80 is no multiple of the 32-deep
    # K-tile, so a K-tile straddles a tap boundary; the weight-gradient reduction is five K-tiles + five rows in two split_k pieces
    CASES["bank_k%d" % _k] = dict(B=5, T=33, cin=80, cout=128, K=_k, dil=1, act="relu", why=(
        "CBHG bank, K = 1: K cin = 80 < 160 stays on the fallback kernel" if _k == 1 else
        "CBHG bank, K = 2: K cin = 160 exactly on the split kernel's threshold; even K: asymmetric SAME padding, mirrored in the data gradient" if _k == 2 else
        "CBHG bank, %s K = %d on win_C = 80 on the fast kernels" % ("even (asymmetric padding)" if _k % 2 == 0 else "odd", _k)))
CASES.update({
    "t32": dict(B=6, T=32, cin=32, cout=48, K=5, dil=1, act="none", why="win_T = win_C = 32: the first window the fast kernels take; t_k wraps every K-tile"),
    "t31": dict(B=6, T=31, cin=32, cout=48, K=5, dil=1, act="none", why="win_T = 31: the last window sent to the fallback kernel"),
    "t_below_k": dict(B=4, T=3, cin=80, cout=128, K=8, dil=1, act="relu", why="more taps than frames: fallback kernel, 32-row tile, windows mostly padding"),
    "t_one": dict(B=1, T=1, cin=80, cout=128, K=8, dil=1, act="relu", why="one frame: one live tap of eight, a one-row product"),
    "proj1": dict(B=2, T=97, cin=1024, cout=256, K=3, dil=1, act="relu", why="rows 194 and N 256 >= 192: big-tile eligible once the workgroup minimum is lowered; "
                  "otherwise every tile cut along K with the tail activation kernel"),
    "proj2": dict(B=2, T=97, cin=256, cout=80, K=3, dil=1, act="none", why="80-column output: one ragged column tile"),
    "enc_post": dict(B=3, T=67, cin=512, cout=512, K=5, dil=1, act="tanh", why="encoder / postnet geometry at few rows (201: two row tiles)"),
    "enc_post_out": dict(B=3, T=67, cin=512, cout=80, K=5, dil=1, act="tanh", why="the postnet's last layer, 512 -> 80"),
    "enc_post_in": dict(B=3, T=67, cin=80, cout=512, K=5, dil=1, act="tanh", why="the postnet's first layer, 80 -> 512: win_C = 80 in the forward, 512 in the data gradient"),
    "wn_d1": dict(B=2, T=140, cin=256, cout=512, K=3, dil=1, act="none", why="WaveGlow in-layer, dilation 1"),
    "wn_d4": dict(B=2, T=140, cin=256, cout=512, K=3, dil=4, act="none", why="WaveGlow in-layer, dilation 4"),
    "wn_d128": dict(B=2, T=140, cin=256, cout=512, K=3, dil=128, act="none", why="dilation 128: only 12 frames per sequence see an outer tap"),
    "wn_d256": dict(B=2, T=140, cin=256, cout=512, K=3, dil=256, act="none", why="dilation 256 > T: no frame sees an outer tap (their dw blocks are the slab's own values)"),
    "bank_long_k1": dict(B=41, T=401, cin=80, cout=128, K=1, dil=1, act="relu", only=("dw",), why="dw over 16 441 rows >= 16 384: the long-reduction branch of training._split_k, one tile"),
    "bank_long_k8": dict(B=41, T=401, cin=80, cout=128, K=8, dil=1, act="relu", only=("dw",), why="... and five row tiles of the slab"),
})
del _k
# the cases the wrong implementations of the CPU test are named on
EVEN_K = ("bank_k2", "bank_k4", "bank_k6", "bank_k8")
DILATED = ("wn_d4", "wn_d128", "wn_d256")


def quantities(name):
    return CASES[name].get("only", QUANTITIES)


def pad_of(K):
    """Left SAME padding in taps (the win_pad of the forward and weight-gradient products; the data gradient runs with K - 1 - pad)."""
    return (K - 1) // 2


def bf16_round(a):
    """float32 -> the nearest bf16 value (ties to even), as float32: the rounding mstts_gemm_bf16 applies on the way into LDS."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def win(x, K, pad, dil=1, fault=None):
    """The window view of x [B, T, C] as [B T, K C]: column block j = frame t + (j - pad) dil of the row's own sequence, 0 outside it.
    fault (negative controls of the CPU test only): "no_seams" - the rows as ONE sequence of length B T; "pad_unscaled" - tap j reads frame
    t + j dil - pad."""
    B, T, C = x.shape
    if fault == "no_seams":
        return win(x.reshape(1, B * T, C), K, pad, dil)
    out = np.zeros((B, T, K, C), x.dtype)
    for j in range(K):
        s = j * dil - pad if fault == "pad_unscaled" else (j - pad) * dil
        lo, hi = max(0, -s), min(T, T - s)
        if lo < hi:
            out[:, lo:hi, j] = x[:, lo + s:hi + s]
    return out.reshape(B * T, K * C)


def flip(w):
    """mstts_conv_kernel_flip (include/mstts.h): wt[K-1-k][o][c] = w[k][c][o], [K, cout, cin]."""
    return np.ascontiguousarray(w[::-1].transpose(0, 2, 1))


def act_fn(v, act):
    if act == "relu":
        return np.maximum(v, 0)
    if act == "tanh":
        return np.tanh(v)
    assert act == "none", act
    return v


@functools.lru_cache(maxsize=None)
def case_data(name):
    """The inputs of a case as float32 arrays - the very arrays that are uploaded and that the reference reads; never modified."""
    cd = dict(CASES[name], name=name)
    B, T, cin, cout, K = cd["B"], cd["T"], cd["cin"], cd["cout"], cd["K"]
    g = np.random.default_rng(list(CASES).index(name) + 31)
    f32 = lambda a: np.asarray(a, np.float32)
    cd["x"] = f32(g.normal(0, 1, (B, T, cin)))
    cd["w"] = f32(g.normal(0, 1.0 / np.sqrt(K * cin), (K, cin, cout)))
    cd["bias"] = f32(g.normal(0, 0.3, cout))
    cd["dz"] = f32(g.normal(0, 1, (B, T, cout)))
    cd["dw0"] = f32(g.normal(0, 1, (K, cin, cout)))
    cd["dx0"] = f32(g.normal(0, 1, (B, T, cin)))
    for k in ("x", "w", "bias", "dz", "dw0", "dx0"):
        cd[k].setflags(write=False)
    return cd


def evaluate(cd, dtype=np.float64, rounded=False, fault=None, only=None):
    """The quantities of a case in `dtype`, as float64 arrays in the judged layout: y [B T, cout], dw [K, cin cout], dx / dx_acc [B T, cin].
    fault: the wrong implementations tests/test_cpu_conv_window_ref.py holds the judge against (win's, and "sym_pad", "dx_unflipped",
    "dx_fwd_pad", "dw_whole_tiles")."""
    B, T, cin, cout, K, dil = cd["B"], cd["T"], cd["cin"], cd["cout"], cd["K"], cd["dil"]
    rows = B * T
    rnd = (lambda a: bf16_round(a)) if rounded else (lambda a: a)
    x, w, dz = (rnd(cd[k]).astype(dtype) for k in ("x", "w", "dz"))
    bias, dw0, dx0 = (cd[k].astype(dtype) for k in ("bias", "dw0", "dx0"))
    pad = K // 2 if fault == "sym_pad" else pad_of(K)
    wfault = fault if fault in ("no_seams", "pad_unscaled") else None
    want = only or quantities(cd["name"])
    q = {}
    if "y" in want or "dw" in want:
        W = win(x, K, pad, dil, wfault)
    if "y" in want:
        q["y"] = act_fn(W @ w.reshape(K * cin, cout) + bias, cd["act"])
    if "dw" in want:
        n = rows // 32 * 32 if fault == "dw_whole_tiles" else rows
        q["dw"] = (dw0.reshape(K * cin, cout) + W[:n].T @ dz.reshape(rows, cout)[:n]).reshape(K, cin * cout)
    if "dx" in want or "dx_acc" in want:
        wf = w.transpose(0, 2, 1) if fault == "dx_unflipped" else flip(w)
        dx = win(dz, K, pad if fault == "dx_fwd_pad" else K - 1 - pad, dil, wfault) @ wf.reshape(K * cout, cin)
        if "dx" in want:
            q["dx"] = dx
        if "dx_acc" in want:
            q["dx_acc"] = dx0.reshape(rows, cin) + dx
    return {k: np.asarray(v, np.float64) for k, v in q.items()}


@functools.lru_cache(maxsize=None)
def evaluations(name, rounded=False):
    """(the fp64 evaluation, the float32 evaluation) of a case; computed once per process, never modified."""
    cd = case_data(name)
    ref, r32 = evaluate(cd, np.float64, rounded), evaluate(cd, np.float32, rounded)
    for v in list(ref.values()) + list(r32.values()):
        v.setflags(write=False)
    return ref, r32


@functools.lru_cache(maxsize=None)
def reference(name, rounded=False):
    """(fp64 quantities, e32 per quantity) of a case; rounded: the bf16-operand statements, reference and float32 evaluation alike."""
    ref, r32 = evaluations(name, rounded)
    return ref, {k: float(slice_err(r32[k], ref[k]).max()) for k in ref}


def bound_of(e32):
    return max(MARGIN * e32, FLOOR)


def judge(name, got, ref, e32):
    """(worst slice error, bound) of quantity `name`: got against ref slice by slice on the slice's own scale; bound = MARGIN x e32, at least FLOOR.
    got: anything that reshapes to ref's judged layout."""
    got = np.asarray(got, np.float64).reshape(ref.shape)
    return float(slice_err(got, ref).max()), bound_of(e32)


# ---- which kernel the dispatch conditions select (csrc/gemm.hip mstts_gemm_f32, csrc/gemm_bf16.hip mstts_gemm_bf16): documentation printed
# beside every measured figure, restated here so that it can be tabulated without a GPU.  form: FORMS of the GPU test.
def products(name):
    """{quantity: (M, N, K, win_T, win_C, act, split_k)} of a case as the trainers build them (dx and dx_acc are the same product)."""
    from multi_speaker_tts_amd.training import _split_k
    c = CASES[name]
    rows, cin, cout, K, T = c["B"] * c["T"], c["cin"], c["cout"], c["K"], c["T"]
    p = {"y": (rows, cout, K * cin, T, cin, c["act"], 1), "dw": (K * cin, cout, rows, T, cin, "none", max(2, _split_k(K * cin, cout, rows))),
         "dx": (rows, cin, K * cout, T, cout, "none", 1)}
    return {k: v for k, v in p.items() if k in quantities(name)}


def selected_kernel(form, M, N, K, win_T, win_C, act, split):
    cdiv = lambda a, b: -(-a // b)
    if form.startswith("bf16"):
        big = form == "bf16_big" and M >= 192 and N >= 192 and win_T >= 32 and win_C >= 32
        return "bf16 256x256" if big else "bf16 128x128" + ("" if split > 1 or act != "none" else ", library K-cut possible")
    if M <= 32:
        return "f32 MFMA, 32-row tile"
    split3 = form != "f32_mfma" and K >= 160 and win_T >= 32 and win_C >= 32
    if not split3:
        return "f32 MFMA"
    if form in ("split_big", "default_det") and M >= 192 and N >= 192 and (act == "none" or split == 1):
        if cdiv(M, 256) * cdiv(N, 256) * split >= (1 if form == "split_big" else 160):
            return "split 256x256"
    tiles = cdiv(M, 128) * cdiv(N, 128)
    cut = form != "default_det" and split == 1 and tiles <= 128 and min(16, 256 // tiles, cdiv(K, 32) // 8) >= 2
    return "split 128x128" + (", every tile K-cut" + (" + tail act" if act != "none" else "") if cut else "")
