"""Sharpness-aware minimisation (nsd_sam, include/nsd.h) on the host: the numpy restatement (tests/sam_ref.py) against the sequence in
stock torch -- gradient, e = rho g / (|g| + 1e-12), weights + e, second gradient, weights restored, torch.optim.Adam -- on a tiny
nn.Linear problem; the fp32 ascent against its float64 formula; ops.Sam; --sam-rho / --grid sam_rho= and the best-configuration
arguments; through ctypes every refusal of the three entry points (all refused before a launch); and the step recipe: one prepare, two
passes with the same rng, counted on stand-ins for the launches.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import nsd_amd
from nsd_amd import _lib, grid, ops, train
from nsd_amd import step_recipe as sr
from tests import sam_ref
from tests.optim_ref import grad_norm

FAKE = 1 << 20                                                      # never dereferenced
E_INVALID, E_WORKSPACE = -1, -3
SAM_SYMBOLS = {"nsd_sam_state_bytes", "nsd_sam_state_init", "nsd_sam_ascend", "nsd_multi_sam_ascend", "nsd_sam_ascend_flat"}


def _err(L):
    return L.nsd_last_error().decode()


# ---- the restatement against stock torch -------------------------------------------------------------------------------------------
def _linear_problem():
    g = torch.Generator().manual_seed(3)
    x = torch.randn((16, 5), generator=g, dtype=torch.float64)
    y = torch.randint(0, 3, (16,), generator=g)
    lin = torch.nn.Linear(5, 3).double()
    return lin, x, y


def _flat(lin):
    return torch.cat([lin.weight.detach().reshape(-1), lin.bias.detach().reshape(-1)]).numpy().copy()


def _grad_fn(x, y):
    """the gradient of the same loss at a flat parameter vector, through a Linear of its own"""
    probe = torch.nn.Linear(5, 3).double()

    def fn(p):
        with torch.no_grad():
            probe.weight.copy_(torch.from_numpy(np.asarray(p[:15])).view(3, 5))
            probe.bias.copy_(torch.from_numpy(np.asarray(p[15:])))
        probe.zero_grad()
        torch.nn.functional.cross_entropy(probe(x), y).backward()
        return torch.cat([probe.weight.grad.reshape(-1), probe.bias.grad.reshape(-1)]).numpy().copy()
    return fn


@pytest.mark.parametrize("rho,wd", [(0.05, 0.0), (0.2, 0.0), (0.0, 0.0), (0.05, 1e-2)])
def test_restatement_equals_the_sequence_in_stock_torch(rho, wd):
    """20 steps; float64 on both sides, so the bound is the association of a few operations: 1e-12 on values below 1"""
    lin, x, y = _linear_problem()
    adam = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=wd)
    ref = sam_ref.SamAdam(_flat(lin), rho, **adam)
    fn = _grad_fn(x, y)
    opt = torch.optim.Adam(lin.parameters(), lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    params = [lin.weight, lin.bias]
    for _ in range(20):
        opt.zero_grad()
        torch.nn.functional.cross_entropy(lin(x), y).backward()                       # 1. the gradient
        norm = torch.sqrt(sum((p.grad ** 2).sum() for p in params))
        es = [rho * p.grad / (norm + 1e-12) for p in params]                          # 2. e = rho g / (|g| + 1e-12)
        with torch.no_grad():
            for p, e in zip(params, es):
                p.add_(e)                                                             # 3. the weights moved
        opt.zero_grad()
        torch.nn.functional.cross_entropy(lin(x), y).backward()                       # 4. the second gradient
        with torch.no_grad():
            for p, e in zip(params, es):
                p.sub_(e)                                                             # 5. the weights restored
        opt.step()
        ref.step(fn)
    err = float(np.abs(ref.p - _flat(lin)).max())
    print(f"[sam_ref vs torch] rho {rho} wd {wd}: max |p_ref - p_torch| {err:.2e}")
    assert err < 1e-12


def test_rho_zero_is_plain_adam():
    lin, x, y = _linear_problem()
    fn = _grad_fn(x, y)
    a, b = sam_ref.SamAdam(_flat(lin), 0.0, lr=1e-2), sam_ref.ClippedAdam(_flat(lin), lr=1e-2, fp32_fields=False)
    for _ in range(5):
        a.step(fn)
        b.step(fn(b.p))
    assert np.array_equal(a.p, b.p)


@pytest.mark.parametrize("n", [1, 257, 31764])
@pytest.mark.parametrize("gscale", [1.0, 0.25, 1.0 / 3.0])
def test_the_fp32_ascent_follows_its_formula(n, gscale):
    """ascend() in fp32 against p + rho g~ / (|g~| + 1e-12) in float64: two roundings of the step (the length, the product) and one of
    the sum: 2^-23 of the step's size twice over plus half an ulp of the result"""
    rs = np.random.RandomState(n)
    p, g, rho = rs.uniform(-1, 1, n).astype(np.float32), rs.standard_normal(n).astype(np.float32), 0.05
    row, rec = sam_ref.ascend(p, g, rho, gscale)
    gt = (g * np.float32(gscale)).astype(np.float64)
    S, norm = grad_norm(g, gscale)
    want = p.astype(np.float64) + float(np.float32(rho)) * gt / (norm + 1e-12)
    bound = 2.0 ** -22 * np.abs(want - p) + 2.0 ** -24 * np.abs(want) + 1e-45
    assert row.dtype == np.float32 and (np.abs(row - want) <= bound).all()
    assert rec["nonfinite"] == 0 and rec["norm"] == float(np.float32(norm)) and rec["scale"] == float(np.float32(float(np.float32(rho)) / (norm + 1e-12)))
    # the length of the move is rho, to fp32
    assert abs(math.sqrt(float(np.sum((row.astype(np.float64) - p) ** 2))) - rho) < 1e-6 * max(1.0, math.sqrt(n))


def test_the_copies_of_the_ascent():
    p = np.array([1.5, -0.0, 0.0, -2.25], np.float32)
    g = np.array([1.0, 2.0, -3.0, 0.5], np.float32)
    row, rec = sam_ref.ascend(p, g, 0.0)
    assert np.array_equal(row.view(np.uint32), p.view(np.uint32)) and rec["scale"] == 0.0 and rec["nonfinite"] == 0
    assert np.signbit(row[1]) and not np.signbit(row[2])
    for bad in (np.inf, -np.inf, np.nan):
        gb = g.copy()
        gb[2] = bad
        row, rec = sam_ref.ascend(p, gb, 0.05)
        assert np.array_equal(row.view(np.uint32), p.view(np.uint32)) and rec["nonfinite"] == 1 and not math.isfinite(rec["norm"])
    big = np.full(4, 3e38, np.float32)            # finite elements, finite S in double (the squares do not overflow there)
    row, rec = sam_ref.ascend(p, big, 0.05)
    assert rec["nonfinite"] == 0 and rec["norm"] == float("inf") and np.isfinite(row).all()          # (the fp32 record overflows, S does not)
    # a zero gradient: S = 0, es = rho / 1e-12, the products are zero and p + 0 is p in value (the sign of a zero may go)
    row, rec = sam_ref.ascend(p, np.zeros(4, np.float32), 0.05)
    assert np.array_equal(row, p) and rec["norm"] == 0.0 and rec["scale"] == float(np.float32(float(np.float32(0.05)) / 1e-12))


# ---- ops.Sam and the C ABI's refusals ------------------------------------------------------------------------------------------------
def test_python_settings():
    for bad in (-0.1, math.nan, math.inf, "0.05", None):
        with pytest.raises(ValueError, match="rho"):
            ops.Sam(bad)
    assert ops.Sam().rho == 0.05 and ops.Sam(0.0).struct().rho == 0.0 and ops.Sam(0.2).struct().rho == np.float32(0.2)
    assert ops._sam_struct(None).rho == 0.0 and nsd_amd.Sam is ops.Sam and "Sam" in nsd_amd.__all__
    a, b = ops.Sam(0.05), ops.Sam(0.2)
    assert ops._per_model([a, ops.Sam(0.05)], 2, "sam") == (a, None) and ops._per_model([a, None, b], 3, "sam") == (None, [a, None, b])
    r = sr.StepRecipe(nsd_amd.EEG_LSTM(), True, None, None, "cpu", sam=a)
    assert r.sam == a and r.sam_args("state") == dict(sam=a, sam_state="state")
    assert sr.StepRecipe(nsd_amd.EEG_LSTM(), False, None, None, "cpu", sam=a).sam == a          # not one of the stochastic parts
    off = sr.StepRecipe(nsd_amd.EEG_LSTM(), True, None, None, "cpu")
    assert off.sam is None and off.sam_args(None) == {}
    models = [nsd_amd.EEG_LSTM() for _ in range(3)]
    each = sr.StepRecipe(models[0], True, None, None, "cpu", models=models, sam=[a, None, b])
    assert each.sam == [a, None, b]
    assert sr.StepRecipe(models[0], True, None, None, "cpu", models=models, sam=[a, a, ops.Sam(0.05)]).sam == a
    assert sr.StepRecipe(models[0], True, None, None, "cpu", models=models, sam=[None] * 3).sam is None
    with pytest.raises(ValueError, match="an ops.Sam or None"):
        sr.StepRecipe(models[0], True, None, None, "cpu", sam=0.05)


def test_the_feature_is_detected_by_its_symbols_and_the_size_function():
    L = nsd_amd.load_library()
    assert L.nsd_version() == 301 and SAM_SYMBOLS <= set(_lib.SYMBOLS) and all(hasattr(L, s) for s in SAM_SYMBOLS)
    assert C.sizeof(_lib.Sam) == 4 and C.sizeof(_lib.SamRecord) == 16
    assert L.nsd_sam_state_bytes(31764, 1) == 16 + 4 * 31764 and L.nsd_sam_state_bytes(10, 3) == 48 + 120 and L.nsd_sam_state_bytes(0, 2) == 32
    assert L.nsd_sam_state_bytes(-1, 1) == E_INVALID and L.nsd_sam_state_bytes(5, 0) == E_INVALID and L.nsd_sam_state_bytes(5, 33) == E_INVALID
    assert L.nsd_sam_state_init(None, 64, None) == E_INVALID and L.nsd_sam_state_init(FAKE, 15, None) == E_INVALID


BAD_RHO = [(-0.5, "rho -0.5 negative or NaN"), (float("nan"), "rho nan negative or NaN")]


def test_refusals_of_the_flat_route():
    L = nsd_amd.load_library()
    who, n = "sam_ascend_flat", 1000
    ob, sb = L.nsd_opt_state_bytes(n, 1), L.nsd_sam_state_bytes(n, 1)
    P_, G_, O_, S_ = FAKE, 2 * FAKE, 3 * FAKE, 4 * FAKE

    def call(rho=0.05, n=n, p=P_, g=G_, sam=True, ost=O_, o_bytes=ob, sst=S_, s_bytes=sb):
        return L.nsd_sam_ascend_flat(n, p, g, C.byref(_lib.Sam(rho)) if sam else None, 1.0, ost, o_bytes, sst, s_bytes, None)
    assert call(p=None) == E_INVALID and _err(L) == f"{who}: null pointer or n<0"
    assert call(g=None) == E_INVALID and call(n=-1) == E_INVALID and _err(L) == f"{who}: null pointer or n<0"
    assert call(sam=False) == E_INVALID and _err(L) == f"{who}: sam is NULL"
    for rho, text in BAD_RHO:
        assert call(rho=rho) == E_INVALID and _err(L) == f"{who}: {text}"
    assert call(ost=None) == E_INVALID and call(sst=None) == E_INVALID and _err(L) == f"{who}: opt_state or sam_state is NULL"
    assert call(o_bytes=ob - 8) == E_WORKSPACE and _err(L).startswith(f"{who}: opt_state of {ob - 8} bytes is smaller")
    assert call(s_bytes=sb - 4) == E_WORKSPACE and _err(L) == f"{who}: sam_state of {sb - 4} bytes is smaller than nsd_sam_state_bytes() = {sb}"
    # the rows (from byte 16 of sam_state) against p and g: the first and the last word of either
    for base in (P_, G_):
        for sst in (base - 16, base - 16 - 4 * (n - 1), base - 16 + 4 * (n - 1)):
            assert call(sst=sst) == E_INVALID and _err(L) == f"{who}: the rows of sam_state overlap p or grads", (base, sst)
    assert call(n=0) == 0 and call(n=0, rho=0.0) == 0           # nothing to do: returns before a launch


@pytest.mark.parametrize("sym,M,each", [("nsd_sam_ascend", 1, 0), ("nsd_multi_sam_ascend", 3, 0), ("nsd_multi_sam_ascend", 3, 1),
                                        ("nsd_multi_sam_ascend", 1, 1)])
def test_refusals_of_the_routes_from_the_slabs(sym, M, each):
    L = nsd_amd.load_library()
    who, multi = sym[4:], "multi" in sym
    d = _lib.Dims(4, 10, 8, 48, 2, 3, 32)
    need = L.nsd_multi_workspace_bytes(C.byref(d), M, None) if multi else L.nsd_workspace_bytes(C.byref(d), None)
    P = L.nsd_param_count(8, 48, 2, 3, 32)
    ob, sb = L.nsd_opt_state_bytes(P, M), L.nsd_sam_state_bytes(P, M)
    span = 4 * M * P
    W_, G_, P_, O_, S_ = FAKE, 64 * FAKE, 128 * FAKE, 192 * FAKE, 256 * FAKE
    assert span < 64 * FAKE
    gs = (C.c_float * M)(*[1.0] * M)

    def call(rhos=None, ws=W_, bytes_=need - 4, grads=G_, p=P_, sam=True, ost=O_, o_bytes=ob, sst=S_, s_bytes=sb):
        arr = (_lib.Sam * M)(*[_lib.Sam(r) for r in (rhos or [0.05] * M)])
        sp = C.cast(arr, C.c_void_p) if sam else None
        if multi:
            return L.nsd_multi_sam_ascend(C.byref(d), M, ws, bytes_, grads, p, sp, each, C.cast(gs, C.c_void_p), ost, o_bytes, sst, s_bytes, None)
        return L.nsd_sam_ascend(C.byref(d), ws, bytes_, grads, p, sp, 1.0, ost, o_bytes, sst, s_bytes, None)
    assert call(grads=None) == E_INVALID and call(p=None) == E_INVALID and _err(L) == f"{who}: null pointer"
    assert call(sam=False) == E_INVALID and _err(L) == f"{who}: sam is NULL"
    for rho, text in BAD_RHO:                         # (one nsd_sam for all models: ONE entry is read)
        assert call(rhos=[0.05] * (M - 1) + [rho]) == (E_INVALID if each or M == 1 else E_WORKSPACE)
        if each or M == 1:
            assert _err(L) == (f"{who}: sam[{M - 1}]: {text}" if each else f"{who}: {text}")
    assert call(ost=None) == E_INVALID and call(sst=None) == E_INVALID and _err(L) == f"{who}: opt_state or sam_state is NULL"
    assert call(o_bytes=ob - 8) == E_WORKSPACE and _err(L).startswith(f"{who}: opt_state of {ob - 8} bytes is smaller")
    assert call(s_bytes=sb - 4) == E_WORKSPACE and _err(L) == f"{who}: sam_state of {sb - 4} bytes is smaller than nsd_sam_state_bytes() = {sb}"
    for base in (P_, G_):
        for sst in (base - 16 * M, base - 16 * M - (span - 4), base - 16 * M + (span - 4)):
            assert call(sst=sst) == E_INVALID and _err(L) == f"{who}: the rows of sam_state overlap p or grads", (base, sst)
    assert call(ws=None) == E_INVALID and _err(L) == (f"{who}: workspace is NULL" if multi else f"{who}: null pointer")
    assert call() == E_WORKSPACE and _err(L).startswith(f"{who}: workspace of {need - 4} bytes is smaller than ")
    if multi:
        assert L.nsd_multi_sam_ascend(C.byref(d), 0, W_, need, G_, P_, None, each, None, O_, ob, S_, sb, None) == E_INVALID
        assert L.nsd_multi_sam_ascend(C.byref(d), M, W_, need, G_, P_, C.cast((_lib.Sam * M)(), C.c_void_p), each, None, O_, ob, S_, sb, None) == E_INVALID
        assert _err(L) == f"{who}: null pointer"


# ---- the command lines -------------------------------------------------------------------------------------------------------------------
def test_train_and_grid_options():
    ap = train.build_parser()
    base = ["--synthetic", "64"]
    a = ap.parse_args(base + ["--sam-rho", "0.05"])
    assert a.sam_rho == 0.05 and train.sam_for(a) == ops.Sam(0.05)
    assert train.sam_for(ap.parse_args(base)) is None and ap.parse_args(base).sam_rho is None
    assert train.sam_for(ap.parse_args(base + ["--sam-rho", "0"])) is None                     # 0 is off
    for bad in ("-0.1", "nan", "inf"):
        with pytest.raises(ValueError, match="--sam-rho"):
            train.sam_for(ap.parse_args(base + ["--sam-rho", bad]))
    a = ap.parse_args(base + ["--kfold", "5", "--concurrent", "--sam-rho", "0.1", "--avg", "ema", "--avg-decay", "0.99"])
    assert train.sam_for(a) == ops.Sam(0.1) and a.concurrent and a.kfold == 5
    # the grid axis: 0 is a configuration without SAM; the best-configuration line carries train's own option
    assert "sam_rho" in grid.ALL_KEYS and "sam_rho" not in grid.GRID_KEYS
    g = grid.parse_grid(["sam_rho=0,0.02,0.05,0.1,0.2", "lr=1e-3,3e-3"])
    assert g == [("sam_rho", [0.0, 0.02, 0.05, 0.1, 0.2]), ("lr", [1e-3, 3e-3])]
    assert grid.parse_grid(["sam-rho=0.05"]) == [("sam_rho", [0.05])]
    with pytest.raises(ValueError, match="sam_rho"):
        grid.parse_grid(["sam_rho=big"])
    args = grid.train_args({"sam_rho": 0.05, "lr": 3e-3})
    assert args == ["--sam-rho", "0.05", "--lr", "0.003"]
    back = ap.parse_args(base + args)
    assert back.sam_rho == 0.05 and back.lr == 3e-3 and train.sam_for(back) == ops.Sam(0.05)
    assert train.sam_for(ap.parse_args(base + grid.train_args({"sam_rho": 0.0}))) is None
    gp = grid.build_parser().parse_args(base + ["--grid", "sam_rho=0,0.05"])
    assert gp.grid == ["sam_rho=0,0.05"] and gp.sam_rho is None


# ---- the step recipe: one prepare, two passes with the same rng ---------------------------------------------------------------------------
@pytest.fixture
def launches(monkeypatch):
    """the library calls of ops as recorded stand-ins on CPU tensors: (name, arguments) with every struct passed by reference replaced by
    its bytes; ops.augment / ops.mixup / ops.zscore count as ("augment" | "mixup" | "zscore", None)"""
    rec = []

    def plain(a):
        obj = getattr(a, "_obj", None)              # C.byref(struct)
        return bytes(obj) if obj is not None else a

    def call(name, dev, *args):
        rec.append((name, tuple(plain(a) for a in args)))

    monkeypatch.setattr(ops, "_call", call)
    monkeypatch.setattr(ops, "_dev_f32", lambda t, name, shape=None: None if t is None else t.data_ptr())
    monkeypatch.setattr(ops, "_labels_ptr", lambda t: t.data_ptr())
    monkeypatch.setattr(ops, "augment", lambda x, aug, rngs, **kw: (rec.append(("augment", None)), x + 1.0)[1])
    monkeypatch.setattr(ops, "zscore", lambda x, out=None: (rec.append(("zscore", None)), x + 1.0)[1])
    monkeypatch.setattr(ops, "mixup", lambda x, labels, K, rngs, **kw: (rec.append(("mixup", None)),
                                                                         (None if x is None else x * 0.5, torch.zeros((labels.numel(), K))))[1])
    return rec


AUG = nsd_amd.Augment(max_shift=3, scale_range=0.1, p_channel=0.2, noise_std=0.3)
LOSS = nsd_amd.Loss(label_smoothing=0.1, mixup=0.5)


def _passes(rec, fwd, bwd):
    f = [a for n, a in rec if n == fwd]
    b = [a for n, a in rec if n == bwd]
    return f, b


@pytest.mark.parametrize("masks", [False, True])
def test_a_single_model_step_prepares_once_and_repeats_its_passes(launches, masks):
    """the step as Trainer._local_grads issues it: recipe.prepare, recipe.rng, ops.train_step_grads with recipe.sam_args -- one
    augmentation, one mixup, and the two forward/backward calls differ in the parameter pointer alone"""
    sam = ops.Sam(0.05)
    model = nsd_amd.EEG_LSTM(dropout=0.4)
    r = sr.StepRecipe(model, True, AUG, LOSS, "cpu", sam=sam)
    spec, B, T = model.spec, 4, 5
    P = spec.param_count
    x, y = torch.randn(B, T, 8), torch.randint(0, 3, (B,), dtype=torch.int32)
    flat, grads, ws, logits = torch.zeros(P), torch.zeros(P), torch.zeros(64), torch.zeros(B, 3)
    sstate, ostate = torch.zeros(16 + 4 * P, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)
    xo, lab, tg = r.prepare(x, y, [77], 3)
    rng = r.rng(77, 3)
    mk = dict(drop_lstm=torch.ones(1, B, T, 48), rrelu_slope=torch.ones(B, 32), drop_head=torch.ones(B, 32)) if masks else {}
    adam = dict(m=torch.zeros(P), v=torch.zeros(P), opt=ops.opt_struct(lr=1e-3), opt_state=ostate, step=3)
    ops.train_step_grads(spec, flat, xo, ws, lab, logits, grads, rng=None if masks else rng, adam=adam, targets=tg, **mk, **r.sam_args(sstate))
    names = [n for n, _ in launches]
    fwd, bwd = ("nsd_lstm_head_train_soft", "nsd_lstm_bwd") if masks else ("nsd_lstm_head_train_soft", "nsd_lstm_bwd_rng")
    assert names == ["augment", "mixup", fwd, bwd, "nsd_sam_ascend", fwd, bwd, "nsd_grad_reduce_clip_adam"]
    f, b = _passes(launches, fwd, bwd)
    row = ops.sam_rows(sstate, 1, P)[0].data_ptr()
    for one, two in (f, b):
        assert one[1] == flat.data_ptr() and two[1] == row and one[0] == two[0] and one[2:] == two[2:]
    if not masks:
        want = bytes(ops._rng_struct(sr.step_rng(77, 3, 0.4, 0.4)))
        assert want in f[0] and want in b[0]                                   # the step's streams, in both passes of both launches
    asc = [a for n, a in launches if n == "nsd_sam_ascend"][0]
    tail = [a for n, a in launches if n == "nsd_grad_reduce_clip_adam"][0]
    assert asc[3] == grads.data_ptr() and asc[4] == flat.data_ptr() and asc[5] == bytes(_lib.Sam(0.05)) and asc[9] == sstate.data_ptr()
    assert tail[4] == flat.data_ptr() and tail[3] == grads.data_ptr()          # the update is on the real parameters
    # without sam: today's calls
    del launches[:]
    ops.train_step_grads(spec, flat, xo, ws, lab, logits, grads, rng=None if masks else rng, adam=adam, targets=tg, **mk,
                         **sr.StepRecipe(model, True, AUG, LOSS, "cpu").sam_args(None))
    assert [n for n, _ in launches] == [fwd, bwd, "nsd_grad_reduce_clip_adam"]


def test_the_data_parallel_form_ascends_from_the_flat_gradient(launches):
    """adam=None (the all-reduce comes between gradient and update): nsd_grad_reduce, nsd_sam_ascend_flat, pass 2, nsd_grad_reduce; an
    empty shard issues what it issues without sam"""
    model = nsd_amd.EEG_LSTM(dropout=0.4)
    spec, B, T = model.spec, 4, 5
    P = spec.param_count
    r = sr.StepRecipe(model, True, None, None, "cpu", sam=ops.Sam(0.1))
    flat, grads, ws, logits = torch.zeros(P), torch.zeros(P), torch.zeros(64), torch.zeros(B, 3)
    sstate, ostate = torch.zeros(16 + 4 * P, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)
    x, y = torch.randn(B, T, 8), torch.randint(0, 3, (B,), dtype=torch.int32)
    ops.train_step_grads(spec, flat, x, ws, y, logits, grads, rng=r.rng(5, 1), opt_state=ostate, **r.sam_args(sstate))
    assert [n for n, _ in launches] == ["nsd_lstm_head_train_rng", "nsd_lstm_bwd_rng", "nsd_grad_reduce", "nsd_sam_ascend_flat",
                                        "nsd_lstm_head_train_rng", "nsd_lstm_bwd_rng", "nsd_grad_reduce"]
    del launches[:]
    x0, y0, l0 = torch.zeros(0, T, 8), torch.zeros(0, dtype=torch.int32), torch.zeros(0, 3)
    ops.train_step_grads(spec, flat, x0, ws, y0, l0, grads, rng=r.rng(5, 1), opt_state=ostate, **r.sam_args(sstate))
    assert [n for n, _ in launches] == ["nsd_lstm_head_train_rng", "nsd_lstm_bwd_rng", "nsd_grad_reduce"]
    with pytest.raises(nsd_amd.NsdError, match="needs an opt_state"):
        ops.train_step_grads(spec, flat, x, ws, y, logits, grads, rng=r.rng(5, 1), **r.sam_args(sstate))
    with pytest.raises(nsd_amd.NsdError, match="needs sam_state"):
        ops.train_step_grads(spec, flat, x, ws, y, logits, grads, rng=r.rng(5, 1), sam=ops.Sam(0.1))


@pytest.mark.parametrize("sams", [[0.05, None, 0.2], [0.05, 0.05, 0.05]])
def test_a_model_batched_step_prepares_once_and_repeats_its_passes(launches, sams):
    M, B, T = 3, 4, 5
    models = [nsd_amd.EEG_LSTM(dropout=0.4) for _ in range(M)]
    sams = [None if s is None else ops.Sam(s) for s in sams]
    r = sr.StepRecipe(models[0], True, AUG, LOSS, "cpu", models=models, sam=sams)
    spec = models[0].spec
    P = spec.param_count
    x, y = torch.randn(M, B, T, 8), torch.randint(0, 3, (M * B,), dtype=torch.int32)
    params, grads, ws = torch.zeros(M, P), torch.zeros(M, P), torch.zeros(64)
    sstate, ostate = torch.zeros(16 * M + 4 * M * P, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)
    xo, lab, tg = r.prepare(x, y, [7, 8, 9], 2, M=M)
    rngs = r.rngs([7, 8, 9], 2)
    ops.multi_train_step(spec, params, xo, lab, ws, grads, rngs=rngs, logits=torch.zeros(M * B, 3), m=torch.zeros(M, P), v=torch.zeros(M, P),
                         step=2, targets=tg, opt=ops.opt_struct(lr=1e-3), opt_state=ostate, **r.sam_args(sstate))
    fwd, bwd = "nsd_multi_train_fwd_soft", "nsd_multi_train_bwd"
    assert [n for n, _ in launches] == ["augment", "mixup", fwd, bwd, "nsd_multi_sam_ascend", fwd, bwd, "nsd_multi_grad_reduce_clip_adam"]
    f, b = _passes(launches, fwd, bwd)
    rows = ops.sam_rows(sstate, M, P).data_ptr()
    for one, two in (f, b):
        assert one[2] == params.data_ptr() and two[2] == rows and one[:2] == two[:2] and one[3:] == two[3:]
    asc = [a for n, a in launches if n == "nsd_multi_sam_ascend"][0]
    each = sams[1] is None
    assert asc[1] == M and asc[4] == grads.data_ptr() and asc[5] == params.data_ptr() and asc[7] == (1 if each else 0)


def test_passes_of_a_trainer_that_issues_them_itself():
    """StepRecipe.passes (the bf16 sequence path): forward_backward(params), ascend(), forward_backward(the row) -- one callable, so
    one batch, one rng; without SAM, or for an empty shard (no state), the one pass of today"""
    P = nsd_amd.EEG_LSTM().spec.param_count
    flat, state = torch.zeros(P), torch.zeros(16 + 4 * P, dtype=torch.uint8)
    seen = []
    r = sr.StepRecipe(nsd_amd.EEG_LSTM(), True, None, None, "cpu", sam=ops.Sam(0.05))
    r.passes(flat, state, lambda p: seen.append(("fb", p.data_ptr(), p.numel())), lambda: seen.append(("ascend",)))
    assert seen == [("fb", flat.data_ptr(), P), ("ascend",), ("fb", state.data_ptr() + 16, P)]
    del seen[:]
    r.passes(flat, None, lambda p: seen.append(("fb", p.data_ptr())), lambda: seen.append(("ascend",)))
    sr.StepRecipe(nsd_amd.EEG_LSTM(), True, None, None, "cpu").passes(flat, state, lambda p: seen.append(("fb", p.data_ptr())),
                                                                      lambda: seen.append(("ascend",)))
    assert seen == [("fb", flat.data_ptr())] * 2


def test_trainers_refuse_before_they_need_a_gpu():
    from nsd_amd.multimodel import ModelBatchTrainer
    from nsd_amd.trainer import Trainer
    with pytest.raises(nsd_amd.NsdError, match="needs the model on the MI355X"):
        Trainer(nsd_amd.EEG_LSTM(), sam=ops.Sam(0.05))
    with pytest.raises(nsd_amd.NsdError):
        ModelBatchTrainer([nsd_amd.EEG_LSTM(), nsd_amd.EEG_LSTM()], sam=[ops.Sam(0.05), None])
