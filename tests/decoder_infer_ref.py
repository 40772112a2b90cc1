"""fp64 checker of the free-running (inference) decoder drivers (tests/test_gpu_decoder_infer_ref.py; pinned without a GPU by
tests/test_cpu_decoder_infer_ref.py).

The reference is `unrolled_free_decoder`: the inference branch of oracle.model.decoder's loop written out around oracle.model.prenet / dropout,
zoneout_lstm_cell(training=False) and lsa_step, on the inputs the drivers take - the prenet kernels and biases, wx0, b0, the folded w0f, w1, b1,
wq, the five attention variables, wproj, bproj, keys, values, token lengths, the two prenet keep-masks [Smax, B, P]; zoneout 0.1 applied
deterministically.  It returns what the drivers store, step-major (linear [n, B, n_mel], stop [n, B], align_hist [n, B, T], n = the loop length),
and the states after the last step.  Two algebraic forms:
    plain    frame -> prenet, projection of [m1 | ctx]: what mstts_decoder_infer_steps computes
    folded   what csrc/persist_infer.hip computes - the frame is never formed: vp = values . Wp_c, u = vp[:, :n_mel] . W1p,
             wfm = Wp_m[:, :n_mel] . W1p, bf = bp[:n_mel] . W1p + b1p; first prenet layer = relu(m1 . wfm + sum_t a[t] u[t] + bf), outputs =
             m1 . Wp_m + sum_t a[t] vp[t] + bp, pre0 = the prenet of the zero start frame
In fp64, on unrounded folded operands, the two agree to 1e-12 (CPU test).  The folded operands that are uploaded are formed in fp64 and rounded
once (`folded_operands`), like the keys: the float32 evaluation reads the very arrays the kernel reads and no GEMM kernel sits upstream of the loop.

Stops: the trajectory does not depend on the stop column of wproj (only linear is fed back).  A "designed" case takes the [m1 | ctx] rows of the
fp64 trajectory over all Smax steps (Smax . B rows, fewer than H + M) and solves the minimum-norm least-squares problem for a stop column (stop
bias 0) with targets -1 before the row's chosen stop step, +1 at it and -1 after it (a row that "un-finishes" changes the loop length); the column is
rounded to float32 and re-evaluated: min |stop| >= 0.99 and the designed loop length are pinned by the CPU test.  A "forced" case draws the stop
column and sets the stop bias to -100: nobody stops, the forced stop at Smax - 1 ends the loop.

Judging (slice_err, MARGIN, FLOOR, SLICE_EPS of tests/lstm_seq_ref.py): every (step, row) slice of linear and align_hist and every step of stop on
its own scale; the final states one slice per row; bound = MARGIN x e32, at least FLOOR, e32 = the worst slice error of THIS checker evaluated in
float32 on the CPU in the algebra of the form under test ("plain"; "persistent" = the worse of plain and folded)."""
import functools
import types

import numpy as np
import torch

from oracle import model as OM
from tests import decoder_loop_ref as R
from tests.lstm_seq_ref import FLOOR, MARGIN, SLICE_EPS, slice_err      # noqa: F401  (the project's constants, not copies)

RATE = R.RATE
PRENET_DROP = 0.5
A, CH, KS = R.A, R.CH, R.KS
PRENET = types.SimpleNamespace(prenet_n=2, prenet_drop=PRENET_DROP)      # what oracle.model.prenet reads of its Dims
P_PRE = "decoder/decoder/prenet_%d/dense/"
P_PROJ = "decoder/decoder/linear_projection/dense/"
# Row 0 has token length Te, row 1 length 1.  stops: "designed" (rows stop at chosen steps, row 0 last, at Smax - 2 or before) or "forced" (nobody stops).
# forms: G generic path | F0 skinny products, pointwise cells | F1 fused cell steps | F2 fused query | F3 fused query + projection |
# F4 the same with the next step's prenet inside the attention launch | P the persistent launch
CASES = {
    "two_steps": dict(widths="defaults", n_mel=8, B=1, Te=7, Smax=2, stops="forced", forms=("G",)),
    "plain_h32": dict(widths="defaults", n_mel=8, B=3, Te=9, Smax=6, stops="designed", forms=("G",)),
    "fused_h64": dict(widths="h64_p64", n_mel=20, B=5, Te=18, Smax=6, stops="designed", forms=("G", "F0", "F1")),
    "two_pass_t140": dict(widths="h64_p64", n_mel=20, B=2, Te=140, Smax=3, stops="forced", forms=("G", "F0", "F1")),
    "wide16_one_tile": dict(widths="WIDE", n_mel=16, B=3, Te=7, Smax=4, stops="forced", forms=("G", "F0", "F1", "F2", "F3")),
    "wide16_two_tiles": dict(widths="WIDE", n_mel=16, B=17, Te=12, Smax=4, stops="forced", forms=("F0", "F1", "F2", "F3")),
    "wide80_one_tile": dict(widths="WIDE", n_mel=80, B=3, Te=7, Smax=7, stops="designed", forms=("F4", "P")),
    "wide80_two_tiles": dict(widths="WIDE", n_mel=80, B=17, Te=12, Smax=6, stops="designed", forms=("F4", "P")),
    "wide80_full": dict(widths="WIDE", n_mel=80, B=32, Te=128, Smax=3, stops="forced", forms=("F4", "P")),
    "wide80_t131": dict(widths="WIDE", n_mel=80, B=5, Te=131, Smax=4, stops="designed", forms=("F4", "P")),              # 256 positions, one row tile
    "wide80_t256_two_tiles": dict(widths="WIDE", n_mel=80, B=17, Te=256, Smax=3, stops="forced", forms=("F4", "P")),     # 256 positions, two row tiles
    "wide80_b33": dict(widths="WIDE", n_mel=80, B=33, Te=9, Smax=2, stops="forced", forms=("G",)),                       # B > 32: neither fast nor persistent
}
OUTPUTS = ("linear", "stop", "align_hist")
STATES = ("c0", "c1", "h0", "h1", "ctx", "cum", "m1")       # after the last step (m1: the last step's cell-1 output, the m1 half of pj)
QUANTITIES = OUTPUTS + STATES
ALGEBRAS = {"plain": ("plain",), "persistent": ("plain", "folded")}
FAULTS = ("masks_of_previous_step", "context_once", "no_zoneout", "cum_not_accumulated", "bf_without_b1p", "row_unfinishes")
FOLDED = ("vp", "u", "wfm", "bf", "pre0")
VARIABLES = ("pw0", "pb0", "pw1", "pb1", "wx0", "b0", "w0f", "w1", "b1", "wq", "wproj", "bproj", "k0b") + R.LSA_NAMES


@functools.lru_cache(maxsize=None)
def weights(widths, n_mel):
    """decoder_loop_ref.weights(widths) - cells, query layer, attention, memory layer - plus what only the free-running loop has, in the same
    style (weights N(0, 1 / sqrt(fan_in)), biases N(0, 0.1)): the prenet, the projection (its stop column: see case_data) and k0b, the SECOND
    context block of the unfolded cell-0 kernel (the first being w0f's context rows minus it), for the context_once control and for building the
    kernel oracle.model.decoder folds."""
    dm = R.dims_of(widths)
    H, M, P = dm["H"], dm["M"], dm["P"]
    g = np.random.default_rng(1000 * sorted(R.WIDTHS).index(widths) + n_mel + 7)
    n = lambda fan_in, *s: g.normal(0, 1.0 / np.sqrt(fan_in), s).astype(np.float32)
    b = lambda *s: g.normal(0, 0.1, s).astype(np.float32)
    w = dict(R.weights(widths))
    w.update(pw0=R._f32(n(n_mel, n_mel, P)), pb0=R._f32(b(P)), pw1=R._f32(n(P, P, P)), pb1=R._f32(b(P)), wproj=R._f32(n(H + M, H + M, n_mel + 1)),
             bproj=R._f32(b(n_mel + 1)), k0b=R._f32(n(P + 2 * M + H, M, 4 * H)))
    return w


def stop_steps(cd):
    """The designed stop step of every row: row 0 at last = max(Smax - 3, 2), after every other row (where Smax allows, the persistent launch's
    one step more is then not the last of the buffer: a step it must leave untouched remains); row b >= 1 at (b - 1) mod last - row 1 at step 0."""
    last = max(cd["Smax"] - 3, 2)
    assert last <= cd["Smax"] - 2
    return np.array([last] + [(b - 1) % last for b in range(1, cd["B"])])


def designed_length(cd):
    return int(stop_steps(cd)[0]) + 1 if cd["stops"] == "designed" else cd["Smax"]


@functools.lru_cache(maxsize=None)
def case_data(name):
    """The inputs of a case as float32 / uint8 / int32 CPU tensors - the very arrays that are uploaded and that the reference reads: values and
    keys as decoder_loop_ref.case_data makes them, the prenet keep-masks, the variables with the case's stop column in wproj / bproj, and the
    folded operands of the persistent launch formed in fp64 and rounded once."""
    c = CASES[name]
    cd = dict(c, name=name, **R.dims_of(c["widths"]))
    B, T, S, H, M, P, NM = cd["B"], cd["Te"], cd["Smax"], cd["H"], cd["M"], cd["P"], cd["n_mel"]
    g = np.random.default_rng(sorted(CASES).index(name) + 211)
    w = weights(c["widths"], NM)
    lens = g.integers(1, T + 1, B)
    lens[0] = T
    if B > 1:
        lens[1] = 1
    cd["lens"] = torch.tensor(lens.astype(np.int32))
    live = np.arange(T)[None, :] < lens[:, None]
    cd["values"] = R._f32(g.normal(0, 1, (B, T, M)).astype(np.float32) * live[:, :, None])
    cd["keys"] = (cd["values"].double() @ w["wmem"].double()).float()
    for k in ("pm0", "pm1"):
        cd[k] = torch.tensor((g.random((S, B, P)) > PRENET_DROP).astype(np.uint8))
    for k in VARIABLES:
        cd[k] = w[k]
    wproj, bproj = w["wproj"].clone(), w["bproj"].clone()
    if c["stops"] == "forced":
        bproj[NM] = -100.0
    else:
        # the stop column: minimum-norm least squares on the [m1 | ctx] rows of the fp64 trajectory over all Smax steps
        bproj[NM] = 0.0
        cd["wproj"], cd["bproj"] = wproj, bproj
        with torch.no_grad():
            x = unrolled_free_decoder(operands(cd, torch.float64), cd["lens"], cd["pm0"], cd["pm1"], RATE, S, run_all=True)["pj_hist"]
        assert S * B < H + M
        first = stop_steps(cd)
        y = np.where(np.arange(S)[:, None] == first[None, :], 1.0, -1.0).reshape(-1)
        col = np.linalg.lstsq(x.numpy().reshape(S * B, H + M), y, rcond=None)[0]
        wproj[:, NM] = torch.tensor(col.astype(np.float32))
    cd["wproj"], cd["bproj"] = wproj, bproj
    cd.update(folded_operands(cd, rounded=True))
    return cd


def folded_operands(cd, rounded, fault=None):
    """vp [B, T, n_mel + 1], u [B, T, P], wfm [H, P], bf [P] and pre0 [B, P] in fp64 from the case's float32 arrays; rounded: to float32, once.
    fault "bf_without_b1p": the negative control."""
    H, NM = cd["H"], cd["n_mel"]
    d = lambda k: cd[k].double()
    vp = d("values") @ d("wproj")[H:]
    bf = d("bproj")[:NM] @ d("pw0") + (0.0 if fault == "bf_without_b1p" else d("pb0"))
    lv = {k: d(k) for k in ("pw0", "pb0", "pw1", "pb1")}
    pre0 = _prenet(lv, torch.zeros(cd["B"], NM, dtype=torch.float64), cd["pm0"], cd["pm1"], 0)
    o = dict(vp=vp, u=vp[:, :, :NM] @ d("pw0"), wfm=d("wproj")[:H, :NM] @ d("pw0"), bf=bf, pre0=pre0)
    return {k: v.float() for k, v in o.items()} if rounded else o


def operands(cd, dtype, folded=None, fault=None):
    """What unrolled_free_decoder reads, in `dtype`.  folded: None, "rounded" (the uploaded float32 arrays) or "exact" (unrounded fp64)."""
    lv = {k: cd[k].to(dtype) for k in VARIABLES + ("keys", "values")}
    if folded is not None:
        src = folded_operands(cd, rounded=(folded == "rounded"), fault=fault)
        lv.update({k: src[k].to(dtype) for k in FOLDED})
    return lv


def _prenet(lv, frame, pm0, pm1, step):
    p = {P_PRE % 0 + "kernel": lv["pw0"], P_PRE % 0 + "bias": lv["pb0"], P_PRE % 1 + "kernel": lv["pw1"], P_PRE % 1 + "bias": lv["pb1"]}
    return OM.prenet(p, PRENET, frame, {"prenet_drop_0": pm0, "prenet_drop_1": pm1}, step)


def unrolled_free_decoder(lv, lens, pm0, pm1, rate, Smax, form="plain", fault=None, run_all=False):
    """The inference branch of oracle.model.decoder's loop.  lv: pw0 [n_mel, P], pb0, pw1 [P, P], pb1, wx0 [P, 4H], b0, w0f [M + H, 4H], w1, b1,
    wq, the five attention variables, wproj [H + M, n_mel + 1], bproj, keys [B, T, A], values [B, T, M] and, for form "folded", vp, u, wfm, bf,
    pre0; pm0 / pm1 [Smax, B, P] keep-masks, row s = the prenet that feeds step s.  The forced stop fires at step Smax - 1.  run_all: every one
    of the Smax steps whatever the stop logits say (the stop design).  fault: the negative controls of the CPU test (FAULTS; "bf_without_b1p"
    lives in folded_operands).  Returns linear [n, B, n_mel], stop [n, B], align_hist [n, B, T], pj_hist [n, B, H + M], n, and the states after
    step n - 1."""
    keys, values, w0f, w1, wproj = lv["keys"], lv["values"], lv["w0f"], lv["w1"], lv["wproj"]
    B, T, _ = keys.shape
    H, M, NM = w1.shape[0] // 2, values.shape[2], wproj.shape[1] - 1
    p = R.lsa_params(lv)
    lmask = torch.arange(T)[None, :] < lens.long()[:, None]
    z = lambda n: keys.new_zeros(B, n)
    c0, h0, c1, h1, ctx, cum = z(H), z(H), z(H), z(H), z(M), z(T)
    if fault == "context_once":          # the unfolded kernel's first context block alone
        w0f = torch.cat([w0f[:M] - lv["k0b"], w0f[M:]])
    cell_rate = 0.0 if fault == "no_zoneout" else rate
    finished = torch.zeros(B, dtype=torch.bool)
    pre = lv["pre0"] if form == "folded" else _prenet(lv, z(NM), pm0, pm1, 0)
    o = {k: [] for k in ("linear", "stop", "align_hist", "pj_hist")}
    t = 0
    while True:
        g0 = OM.gmm(pre, lv["wx0"]) + lv["b0"] + OM.rmm(torch.cat([ctx, h0], dim=1), w0f)
        m0, c0, h0 = OM.zoneout_lstm_cell(None, c0, h0, None, None, None, None, cell_rate, False, gates=g0)
        g1 = OM.rmm(torch.cat([m0, h1], dim=1), w1) + lv["b1"]
        m1, c1, h1 = OM.zoneout_lstm_cell(None, c1, h1, None, None, None, None, cell_rate, False, gates=g1)
        align, cum_n, ctx = OM.lsa_step(p, None, keys, values, lmask, m1, cum)
        if fault != "cum_not_accumulated":
            cum = cum_n
        if form == "folded":
            proj = m1 @ wproj[:H] + (align[:, :, None] * lv["vp"]).sum(dim=1) + lv["bproj"]
        else:
            proj = OM.gmm(torch.cat([m1, ctx], dim=1), wproj) + lv["bproj"]
        lin, st = proj[:, :NM], proj[:, NM]
        for k, v in (("linear", lin), ("stop", st), ("align_hist", align), ("pj_hist", torch.cat([m1, ctx], dim=1))):
            o[k].append(v)
        nf = (st >= 0.0) | torch.tensor(t >= Smax - 1)
        finished = nf if fault == "row_unfinishes" else finished | nf
        t += 1
        if t == Smax or (bool(finished.all()) and not run_all):
            break
        mt = t - 1 if fault == "masks_of_previous_step" else t
        if form == "folded":
            l1 = OM.dropout(torch.relu(m1 @ lv["wfm"] + (align[:, :, None] * lv["u"]).sum(dim=1) + lv["bf"]), pm0[mt], PRENET_DROP)
            pre = OM.dropout(torch.relu(OM.gmm(l1, lv["pw1"]) + lv["pb1"]), pm1[mt], PRENET_DROP)
        else:
            pre = _prenet(lv, lin, pm0, pm1, mt)
    out = {k: torch.stack(v) for k, v in o.items()}
    out.update(n=t, c0=c0, c1=c1, h0=h0, h1=h1, ctx=ctx, cum=cum, m1=m1)
    return out


def evaluate(cd, form, dtype, fault=None):
    """Every compared quantity of the checker in `dtype` and algebra `form`, as float64 arrays, and the loop length "n"."""
    lv = operands(cd, dtype, folded="rounded" if form == "folded" else None, fault=fault)
    with torch.no_grad():
        o = unrolled_free_decoder(lv, cd["lens"], cd["pm0"], cd["pm1"], RATE, cd["Smax"], form=form, fault=fault)
    q = {k: o[k].double().numpy() for k in QUANTITIES}
    q["n"] = o["n"]
    return q


@functools.lru_cache(maxsize=None)
def evaluations(name):
    """(the fp64 evaluation in the plain form, {form: the float32 evaluation}) of a case; computed once per process, never modified."""
    cd = case_data(name)
    ref, r32 = evaluate(cd, "plain", torch.float64), {f: evaluate(cd, f, torch.float32) for f in ("plain", "folded")}
    for q in [ref] + list(r32.values()):
        for v in q.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return ref, r32


def judged_err(k, got, ref):
    """The error of every slice of quantity k: (step, row) slices of linear and align_hist, steps of stop, rows of a final state.  `got` may
    hold more steps than the reference (a launch that ran on): the reference's steps are judged."""
    r = ref[k]
    got = np.asarray(got, np.float64)
    if k in OUTPUTS:
        assert got.shape[0] >= r.shape[0], (k, got.shape, r.shape)
        got = got[:r.shape[0]]
    return slice_err(got, r)


@functools.lru_cache(maxsize=None)
def reference(name, algebra="plain"):
    """(fp64 quantities, e32 per quantity, bound per quantity) of a case for the forms of an algebra ("plain" or "persistent")."""
    ref, r32 = evaluations(name)
    for f in ALGEBRAS[algebra]:
        assert r32[f]["n"] == ref["n"], (name, f, r32[f]["n"], ref["n"])
    e32 = {k: max(float(judged_err(k, r32[f][k], ref).max()) for f in ALGEBRAS[algebra]) for k in QUANTITIES}
    bound = {k: max(MARGIN * e32[k], FLOOR) for k in e32}
    return ref, e32, bound


def exact_failures(cd, align_hist):
    """Names of the exact conditions align_hist [n, B, T] breaks: 0 past a row's length; exactly 1.0 at position 0 of a row of length 1."""
    a = np.asarray(align_hist)
    lens = cd["lens"].numpy()
    dead = np.arange(cd["Te"])[None, :] >= lens[:, None]
    bad = []
    if np.any(a[:, dead] != 0.0):
        bad.append("align_hist: not exactly 0 past a row's length")
    if np.any(a[:, lens == 1, 0] != 1.0):
        bad.append("align_hist: a row of length 1 does not have alignment exactly 1.0 at position 0")
    return bad


def judge(name, algebra, got, quantities):
    """[(quantity, e32, worst slice error, bound)] of `got` (the steps 0 .. n - 1 of the outputs, any of the final states) against the reference."""
    ref, e32, bound = reference(name, algebra)
    return [(k, e32[k], float(judged_err(k, got[k], ref).max()), bound[k]) for k in quantities]
