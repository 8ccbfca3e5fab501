"""The composed front-end reference and its case table (tests/pipeline_ref.py), the parts that need no GPU:

  * the table is a pairwise cover of its factors over the allowed combinations (by enumeration against refused()), and each refusal
    is the documented error of the package;
  * prepare_ref with every stage off returns its input bits, with exactly one stage on that stage's own restatement, and in every row
    every enabled stage changes the bits of its input (the assertions that condition the inputs);
  * StepRecipe.prepare / gather, driven for every row the way its mode drives them with recording stand-ins for the ops stages: the
    documented stage order, no stage writing the caller's inputs, static modes writing static buffers only, and two stages sharing an
    output only where the later one is documented as in place."""
import itertools
import types

import numpy as np
import pytest
import torch

import nsd_amd
from nsd_amd import ops
from nsd_amd import step_recipe as sr
from nsd_amd.data import BatchSchedule, DeviceTrialSet
from nsd_amd.multimodel import ModelBatchTrainer
from nsd_amd.trainer import Trainer
from tests import align_ref, augment_ref, crop_ref, gate_ref, gather_ref, mixup_ref, prep_ref
from tests import pipeline_ref as pl
from tests.small_kernels_ref import zscore_ref

IDS = [pl.case_id(c) for c in pl.CASES]


def zscore_host(x):
    """the CPU stand-in of the z-score link (pipeline_ref's docstring): float64, rounded once"""
    return zscore_ref(x).astype(np.float32)


# ---- the table --------------------------------------------------------------------------------------------------------------------
def _pairs(c):
    names = list(pl.FACTORS)
    return {((a, c[a]), (b, c[b])) for i, a in enumerate(names) for b in names[i + 1:]}


def test_the_table_covers_every_allowed_pair():
    names = list(pl.FACTORS)
    for f, levels in pl.FACTORS.items():
        assert len(set(levels)) == len(levels), f
    rows = [dict(zip(names, v)) for v in itertools.product(*pl.FACTORS.values())]
    allowed = [r for r in rows if pl.refused(r) is None]
    need = set().union(*(_pairs(r) for r in allowed))
    table = [{f: getattr(c, f) for f in names} for c in pl.CASES]
    for c, r in zip(pl.CASES, table):
        assert all(r[f] in pl.FACTORS[f] for f in names) and pl.refused(r) is None, c
    uncovered = sorted(need - set().union(*(_pairs(r) for r in table)), key=repr)
    print(f"{len(pl.CASES)} rows; {len(allowed)} allowed combinations of {len(rows)}; {len(need)} allowed pairs; uncovered: {uncovered}")
    assert uncovered == []
    assert 25 <= len(pl.CASES) <= 35 and [c.id for c in pl.CASES] == list(range(len(pl.CASES)))
    # every pair that no allowed combination holds is one a refusal names
    every = {((a, la), (b, lb)) for i, a in enumerate(names) for b in names[i + 1:] for la in pl.FACTORS[a] for lb in pl.FACTORS[b]}
    assert len(every - need) == 11, sorted(every - need, key=repr)
    # the two full-chain blocks
    full = [c for c in pl.CASES if c.id in pl.FULL_CHAIN_IDS]
    assert sorted(c.mode for c in full) == sorted(pl.FACTORS["mode"])
    for c in full:
        assert (c.augment, c.gate, c.prep, c.align, c.crop, c.loss, c.targets, c.normalize, c.tail) == (1, 1, 1, 1, "drawn", "mix", "int", 0, "all"), c
    n = pl.CASES[pl.NORMALIZE_ROW_ID]
    assert (n.normalize, n.augment, n.crop, n.loss, n.tail, n.source) == (1, 1, "drawn", "mix", "all", "bound")
    # model-batched rows see both shared and per-model inputs
    assert {c.xin for c in pl.CASES if c.mode in ("multi", "each")} == {"shared", "per"}
    assert all(c.xin == "per" for c in pl.CASES if c.mode in ("multi", "each") and c.source == "bound")
    assert all(c.xin == "-" for c in pl.CASES if c.mode not in ("multi", "each"))
    # mode "each" runs the _each launches somewhere: differing augment and loss lists both appear
    assert any(c.mode == "each" and c.augment for c in pl.CASES) and any(c.mode == "each" and c.loss == "mix" for c in pl.CASES)


def test_each_refusal_is_the_documented_error():
    G, P, A = nsd_amd.SignalGate(**pl.GATE), nsd_amd.CausalPrep.design(**pl.PREP), nsd_amd.SessionAlign()
    for kw, word in ((dict(gate=G), "gate together with normalize"), (dict(prep=P), "prep together with normalize"),
                     (dict(align=A), "align together with normalize")):
        with pytest.raises(ValueError, match=word):
            nsd_amd.EEG_LSTM(normalize=True, **kw)
    # the trainers' own refusals come before anything touches the device: the methods run on stand-ins of the trainer
    model = nsd_amd.EEG_LSTM()
    x, q = torch.zeros((pl.B, pl.T, pl.C)), torch.zeros((pl.B, pl.K))
    me = types.SimpleNamespace(loss=nsd_amd.Loss(label_smoothing=0.1), spec=model.spec, world=1, _crops=1, step_count=0)
    with pytest.raises(nsd_amd.NsdError, match="float targets together with loss="):
        Trainer.step.__wrapped__(me, x, q)
    soft_set = DeviceTrialSet(np.zeros((pl.N, pl.T, pl.C), np.float32), np.zeros((pl.N, pl.K), np.float32), "cpu")
    bound = dict(trials=soft_set, first=1, taken=0, S=pl.S, B=pl.B, T=pl.T)
    me = types.SimpleNamespace(_bound=bound, step_count=0, model=model)
    with pytest.raises(nsd_amd.NsdError, match="the static inputs hold int32 labels"):
        Trainer.step_scheduled.__wrapped__(me, static=True)
    me = types.SimpleNamespace(_bound=None, step_count=0, model=model)
    with pytest.raises(nsd_amd.NsdError, match="no batches bound"):
        Trainer.step_scheduled.__wrapped__(me, static=True)
    sched = BatchSchedule(np.zeros((pl.M, pl.S, pl.B), np.int32), pl.S)
    with pytest.raises(nsd_amd.NsdError, match="the trial set holds target rows"):
        ModelBatchTrainer.bind_batches(types.SimpleNamespace(), soft_set, sched)
    # the two refusals that leave no level in the table
    with pytest.raises(nsd_amd.NsdError, match="stochastic=False with drawn crop offsets"):
        sr.StepRecipe(model, False, None, None, "cpu", crop=nsd_amd.Crop(pl.CROP_W, pl.CROP_R, 0))
    models = [nsd_amd.EEG_LSTM() for _ in range(pl.M)]
    with pytest.raises(nsd_amd.NsdError, match="different crop settings"):
        sr.StepRecipe(models[0], True, None, None, "cpu", models=models, crop=[nsd_amd.Crop(16, 3), nsd_amd.Crop(16, 3), nsd_amd.Crop(8, 3)])
    for c in pl.CASES:
        assert pl.refused(c._asdict()) is None


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)


@pytest.fixture(scope="module")
def batch():
    rs = np.random.RandomState(5)
    x = pl._trials(pl.M * pl.B, rs).reshape(pl.M, pl.B, pl.T, pl.C)
    y = rs.randint(0, pl.K, (pl.M, pl.B)).astype(np.int32)
    return x, y, [sr.trainer_seed(s) for s in pl.SEEDS]


def test_reference_with_every_stage_off_returns_its_input(batch):
    x, y, seeds = batch
    w, lab, tg = pl.prepare_ref(x, y, seeds, 2, M=pl.M)
    assert _same(w, x) and _same(lab, y) and tg is None
    w, lab, tg = pl.prepare_ref(x[0], y[0], seeds[:1], 2)
    assert _same(w, x[:1]) and _same(lab, y[:1]) and tg is None
    q = pl._soft_rows(pl.B, np.random.RandomState(1))
    w, lab, tg = pl.prepare_ref(x[0], q, seeds[:1], 2)
    assert _same(w, x[:1]) and lab is None and _same(tg, q[None])
    w, lab, tg = pl.prepare_ref(x[0], y[0], seeds, 2, M=pl.M)             # shared by M: each model its copy
    assert all(_same(w[m], x[0]) and _same(lab[m], y[0]) for m in range(pl.M))


def test_reference_with_one_stage_on_is_that_stages_own_restatement(batch):
    x, y, seeds = batch
    step, bs = 3, sr.base_stream(3)
    one = lambda **kw: pl.prepare_ref(x, y, seeds, step, M=pl.M, **kw)
    models = range(pl.M)
    a = pl.AUGMENTS[0]
    w, lab, _ = one(augment=a)
    assert _same(w, augment_ref.augment_models(x, [(s, bs) for s in seeds], **a)) and _same(lab, y)
    w, _, _ = one(augment=list(pl.AUGMENTS))
    assert _same(w[1], x[1]) and _same(w[2], augment_ref.augment(x[2], seeds[2], bs, **pl.AUGMENTS[2])) and not _same(w[0], x[0])
    G = nsd_amd.SignalGate(**pl.GATE).to_dict()
    w, _, _ = one(gate=G)
    for m in models:
        held, mask = gate_ref.gate_ref(x[m], G)
        assert mask.any() and (gate_ref.popcount(mask) > G["max_bad"]).any()          # the three-channel pop: rejected outside a training step
        assert _same(w[m], gate_ref.apply_ref(held, mask, dict(G, max_bad=pl.C))) and np.isfinite(w[m]).all()
        assert np.isnan(gate_ref.apply_ref(held, mask, G)).any()
    P = nsd_amd.CausalPrep.design(**pl.PREP)
    kw = dict(sections=P.sections, alpha=P.alpha, var0=P.var0, baseline=P.baseline, car=P.car)
    w, _, _ = one(prep=kw)
    assert all(_same(w[m], prep_ref.prep_ref(x[m], **kw)) for m in models)
    W = pl._matrices(pl.M, np.random.RandomState(2))
    assert not np.array_equal(W[0], W[0].T) and not np.array_equal(W[0], W[1])
    w, _, _ = one(align=W)
    assert all(_same(w[m], align_ref.apply_ref(x[m], W[m])) for m in models)
    for hop in (0, pl.GRID_HOP):
        w, lab, _ = one(crop=dict(window=pl.CROP_W, crops=pl.CROP_R, hop=hop))
        cw, cl, _, off = crop_ref.crop_models(x, pl.CROP_W, pl.CROP_R, [(s, bs) for s in seeds], hop=hop, labels=y)
        assert _same(w, cw) and _same(lab, cl) and w.shape == (pl.M, pl.B * pl.CROP_R, pl.CROP_W, pl.C)
        assert (hop == 0) == bool((off[0] != off[1]).any())
    assert (pl.CROP_R - 1) * pl.GRID_HOP + pl.CROP_W == pl.T                            # the grid reaches the last sample
    q = pl._soft_rows(pl.B, np.random.RandomState(1))
    w, lab, tg = pl.prepare_ref(x[0], q, seeds[:1], step, crop=dict(window=pl.CROP_W, crops=pl.CROP_R, hop=0))
    assert lab is None and _same(tg[0], np.repeat(q, pl.CROP_R, axis=0))
    lo = pl.LOSSES["smooth"][0]
    w, lab, tg = one(loss=lo)
    assert _same(w, x) and lab is None and _same(tg, mixup_ref.mixup_models(None, y, pl.K, [(s, bs) for s in seeds], eps=lo["eps"], weights=lo["weights"])[1])
    lo = pl.LOSSES["mix"][0]
    w, lab, tg = one(loss=lo)
    mw, mt = mixup_ref.mixup_models(x, y, pl.K, [(s, bs) for s in seeds], **lo)
    assert _same(w, mw) and _same(tg, mt) and not _same(w, x)
    w, lab, tg = one(loss=list(pl.LOSSES["mix"]))                       # a model without a loss beside ones with: copied windows, one-hot rows
    assert _same(w[1], x[1]) and _same(tg[1], np.eye(pl.K, dtype=np.float32)[y[1]]) and not _same(w[2], x[2])
    w, _, _ = one(normalize=True, zscore=zscore_host)
    assert _same(w, zscore_host(x.reshape(-1, pl.T, pl.C)).reshape(x.shape))
    # gather: bits, the row rule, and no stream -- the same draws as the host-fed step on the gathered batch
    rs = np.random.RandomState(9)
    xa, ya = pl._trials(pl.N, rs), rs.randint(0, pl.K, pl.N).astype(np.int32)
    table = np.stack([np.stack([rs.permutation(pl.N)[:pl.B] for _ in range(pl.S)]) for _ in range(pl.M)]).astype(np.int32)
    for s, first in ((2, 2), (3, 2), (5, 2), (1, 1)):
        w, lab, _ = pl.prepare_ref(None, None, seeds, s, M=pl.M, bound=dict(x=xa, y=ya, table=table, first=first))
        r = gather_ref.row(s, first, pl.S)
        assert r == (s - first) % pl.S and _same(w, xa[table[:, r]]) and _same(lab, ya[table[:, r]])
        a1 = pl.prepare_ref(None, None, seeds, s, M=pl.M, augment=a, bound=dict(x=xa, y=ya, table=table, first=first))[0]
        assert _same(a1, pl.prepare_ref(xa[table[:, r]], ya[table[:, r]], seeds, s, M=pl.M, augment=a)[0])


@pytest.mark.parametrize("c", pl.CASES, ids=IDS)
def test_in_every_row_every_enabled_stage_changes_its_input(c):
    ref = pl.reference(c, zscore=zscore_host)
    n, each = pl.models_of(c), c.mode == "each"
    want = pl.expected_stages(c)
    rows, W = (pl.B * pl.CROP_R, pl.CROP_W) if c.crop != "off" else (pl.B, pl.T)
    for s in pl.STEPS:
        w, lab, tg, trace = ref[s]
        assert w.shape == (n, rows, W, pl.C) and w.dtype == np.float32 and np.isfinite(w).all()
        assert [k for k in pl.STAGES if k in trace] == want, (s, trace)
        for stage in want:
            acts = [True] * n
            if each and stage == "augment":
                acts = [a is not None for a in pl.AUGMENTS]
            if each and stage == "mixup":
                acts = [lo is not None for lo in pl.LOSSES["mix"]]
            assert trace[stage] == acts, (s, stage, trace[stage])
        if c.targets == "float" or c.loss != "off":
            assert lab is None and tg.shape == (n, rows, pl.K) and tg.dtype == np.float32
        else:
            assert tg is None and lab.shape == (n, rows) and lab.dtype == np.int32
        if c.loss != "off":
            assert trace["targets"] == ([lo is not None for lo in pl.LOSSES[c.loss]] if each else [True] * n)
    # the batches of the three steps differ, and so do the alignment matrices of steps 2 and 3
    assert not np.array_equal(ref[1][0], ref[2][0]) and not np.array_equal(ref[2][0], ref[3][0])
    if c.align:
        inp = pl.inputs(c)
        assert np.array_equal(inp["align"][1], inp["align"][2]) and not np.array_equal(inp["align"][2], inp["align"][3])


# ---- the buffers of StepRecipe.prepare / gather -------------------------------------------------------------------------------------
def _ptr(t):
    return t.untyped_storage().data_ptr()


@pytest.fixture
def stages(monkeypatch):
    """every ops stage of the step as a stand-in on CPU tensors: records (name, its window input, its named outputs, the other
    arguments) and returns the `out` it was given or a new tensor of the launch's shape"""
    rec = []

    def new(shape, dtype=torch.float32):
        return torch.zeros(tuple(shape), dtype=dtype)

    def windows(x, M):
        return tuple(x.shape) if x.dim() == 4 or M == 1 else (M,) + tuple(x.shape)

    def augment(x, aug, rngs, *, M=1, zscore=False, step_dev=None, out=None):
        res = out if out is not None else new(windows(x, M))
        rec.append(dict(name="augment", x=x, outs=dict(out=out), res=res, aug=aug, rngs=rngs, M=M, zscore=zscore, step_dev=step_dev))
        return res

    def zscore(x, out=None):
        res = out if out is not None else new(x.shape)
        rec.append(dict(name="zscore", x=x, outs=dict(out=out), res=res))
        return res

    def gate_step(x, gate, state=None, *, slots=None, out=None, mask=None):
        res = out if out is not None else new(x.shape)
        mk = mask if mask is not None else new(x.shape[:-1], torch.int32)
        rec.append(dict(name="gate_step", x=x, outs=dict(out=out, mask=mask), res=res, state=state))
        return res, mk

    def prep_step(x, prep, state=None, *, slots=None, out=None):
        res = out if out is not None else new(x.shape)
        rec.append(dict(name="prep_step", x=x, outs=dict(out=out), res=res, state=state))
        return res

    def gate_apply(v, gate, mask, *, out=None, max_bad=None):
        res = out if out is not None else new(v.shape)
        rec.append(dict(name="gate_apply", x=v, outs=dict(out=out), res=res, max_bad=max_bad, mask=mask))
        return res

    def spatial_apply(v, W, *, sel=None, out=None):
        res = out if out is not None else new(v.shape)
        rec.append(dict(name="spatial_apply", x=v, outs=dict(out=out), res=res, W=W, sel=sel))
        return res

    def crop(x, cfg, rngs=None, *, M=1, labels=None, targets=None, step_dev=None, out=None, labels_out=None, targets_out=None, offsets=None):
        shape = windows(x, M)
        rows = shape[-3] * cfg.crops
        res = out if out is not None else new(shape[:-3] + (rows, cfg.window, shape[-1]))
        n = (M if len(shape) == 4 else 1) * rows
        lo = None if labels is None else labels_out if labels_out is not None else new((n,), torch.int32)
        to = None if targets is None else targets_out if targets_out is not None else new((n, targets.shape[1]))
        rec.append(dict(name="crop", x=x, outs=dict(out=out, labels_out=labels_out, targets_out=targets_out), res=res, rngs=rngs, M=M,
                        step_dev=step_dev, labels=labels, targets=targets))
        return res, lo, to

    def mixup(x, labels, K, rngs, *, label_smoothing=0.0, mix=0.0, class_weights=None, M=1, step_dev=None, out=None, targets=None):
        res = None if x is None else out if out is not None else new(windows(x, M))
        tg = targets if targets is not None else new((labels.numel(), K))
        rec.append(dict(name="mixup", x=x, outs=dict(out=out if x is not None else None, targets=targets), res=res, rngs=rngs, M=M, step_dev=step_dev,
                        labels=labels, mix=mix, label_smoothing=label_smoothing, class_weights=class_weights))
        return res, tg

    def gather_batch(x_all, table, *, step=0, step_base=0, step_dev=None, labels_all=None, targets_all=None, out=None, labels_out=None,
                     targets_out=None, status=None):
        rec.append(dict(name="gather_batch", x=x_all, outs=dict(out=out, labels_out=labels_out, targets_out=targets_out), res=out, table=table,
                        step=step, step_base=step_base, step_dev=step_dev, labels_all=labels_all, targets_all=targets_all))
        return out, labels_out, targets_out

    for f in (augment, zscore, gate_step, prep_step, gate_apply, spatial_apply, crop, mixup, gather_batch):
        monkeypatch.setattr(ops, f.__name__, f)
    return rec


OPS_OF = dict(gather="gather_batch", augment="augment", zscore="zscore", gate="gate_step", prep="prep_step", apply="gate_apply",
              align="spatial_apply", crop="crop", zscore_crops="zscore", mixup="mixup")
# the stages documented as in place (StepRecipe: nsd_prep_step "on the augmented windows in place, else into the same buffer"; the gate's
# two stages around it in that buffer; nsd_spatial_apply "in place in the buffer the front end wrote"; nsd_zscore_fwd "on the crops in
# place").  augment, crop, mixup and gather never are: each reads rows it has not yet written.
IN_PLACE = {"gate_step", "prep_step", "gate_apply", "spatial_apply", "zscore"}


def _recipe_of(c):
    st = pl.settings(c)
    n = pl.models_of(c)
    models = [nsd_amd.EEG_LSTM(dropout=p, **st["model"]) for p in st["dropouts"]]
    tr = st["trainer"]
    if n == 1:
        return sr.StepRecipe(models[0], True, tr["augment"], tr["loss"], "cpu", sam=tr.get("sam"), crop=tr["crop"])
    sam = tr.get("sam")
    return sr.StepRecipe(models[0], True, tr["augment"], tr["loss"], "cpu", models=models, sam=sam if isinstance(sam, list) else [sam] * n, crop=tr["crop"])


@pytest.mark.parametrize("c", pl.CASES, ids=IDS)
def test_prepare_writes_where_its_mode_allows_in_the_documented_order(stages, c):
    recipe, inp, n = _recipe_of(c), pl.inputs(c), pl.models_of(c)
    seeds = [sr.trainer_seed(s) for s in pl.SEEDS[:n]]
    static = c.mode in ("static", "sched")
    step = 2
    step_dev = torch.full((1,), step, dtype=torch.int64) if static else None
    mine, bufs, bound = [], None, None                 # mine: the caller's tensors, which no stage may be given to write
    if c.source == "bound":
        xa, ya = inp["trials"]
        trials = DeviceTrialSet(xa, ya, "cpu")
        bound, kept = sr.StepRecipe.bind(None, trials, BatchSchedule(inp["schedules"][0], pl.S), n, 1, "test")
        assert not kept
        mine += [trials.x, trials.y, bound["table"]]
    if static:
        x, y = torch.zeros((pl.B, pl.T, pl.C)), torch.zeros((pl.B,), dtype=torch.int32)
        bufs = dict(x=x, y=y, **recipe.static_buffers(x))
        if c.mode == "sched":
            gx, gy = recipe.gather(bound, 0, step_dev=step_dev, x=x, y=y)
            assert gx is x and gy is y
        else:
            mine += [x, y]
        out = recipe.prepare(x, y, seeds, 0, step_dev=step_dev, bufs=bufs)
    else:
        if bound is not None:
            x, y = recipe.gather(bound, step)
            assert x is bound["x"] and y is bound["y"]
            if n > 1:
                x, y = x.view(n, pl.B, pl.T, -1), y.view(n, pl.B)
        else:
            x, y = torch.from_numpy(inp["x"][step]), torch.from_numpy(inp["y"][step])
        mine += [x, y]
        if n > 1:                                     # as ModelBatchTrainer.step hands them over
            y = (y.unsqueeze(0).expand(n, pl.B) if y.dim() == 1 else y).contiguous().view(-1)
            mine.append(y)
        out = recipe.prepare(x, y, seeds, step, M=n)
    # the documented order
    # (behind an augmentation the whole-window z-score rides in nsd_augment's launch; smoothing alone still launches nsd_mixup, for the rows)
    want = [OPS_OF[s] for s in pl.expected_stages(c) if not (s == "zscore" and c.augment)] + (["mixup"] if c.loss == "smooth" else [])
    assert [r["name"] for r in stages] == want
    by = {}
    for r in stages:
        by.setdefault(r["name"], []).append(r)
    # what the stages are told
    if c.augment:
        assert by["augment"][0]["zscore"] is bool(c.normalize and c.crop == "off") and by["augment"][0]["M"] == n
    if c.gate:
        assert by["gate_apply"][0]["max_bad"] == pl.C and by["gate_step"][0]["state"] is None
        assert tuple(by["gate_apply"][0]["mask"].shape) == tuple(by["gate_step"][0]["x"].shape[:-1])      # the detector's words reach the apply stage
        assert not static or by["gate_step"][0]["outs"]["mask"] is bufs["gm"] is by["gate_apply"][0]["mask"]
    if c.align:                                        # one matrix per model: model m's rows name matrix m
        a = by["spatial_apply"][0]
        assert a["W"] is recipe.align_W and tuple(a["W"].shape) == ((pl.C, pl.C) if n == 1 else (n, pl.C, pl.C))
        assert a["sel"] is None if n == 1 else a["sel"].tolist() == np.repeat(np.arange(n), pl.B).tolist()
    if c.crop != "off":
        assert (by["crop"][0]["rngs"] is not None) == (c.crop == "drawn") and by["crop"][0]["M"] == n
    if c.loss != "off":
        assert (by["mixup"][0]["x"] is not None) == (c.loss == "mix") and by["mixup"][0]["M"] == n
    for r in stages:
        if r.get("rngs") is not None:
            assert [g["seed"] for g in r["rngs"]] == seeds and {g["base_stream"] for g in r["rngs"]} == {0 if static else sr.base_stream(step)}
            assert r["step_dev"] is step_dev
    if c.source == "bound":
        g = by["gather_batch"][0]
        assert g["x"] is trials.x and g["table"] is bound["table"] and g["step_base"] == 1
        assert (g["step"], g["step_dev"]) == ((0, step_dev) if static else (step, None))
    # no stage is given the caller's inputs to write
    mine_ptrs = {_ptr(t) for t in mine}
    for r in stages:
        held = {_ptr(t) for t in (trials.x, trials.y, bound["table"])} if r["name"] == "gather_batch" else mine_ptrs   # (the gather fills the step's x / y)
        for k, t in r["outs"].items():
            assert t is None or _ptr(t) not in held, (r["name"], k)
    # the static modes write static buffers only: nothing is allocated inside a capture
    if static:
        own = {_ptr(t): k for k, t in bufs.items() if t is not None and k not in ("x", "y")}
        for r in stages:
            if r["name"] == "gather_batch":
                assert r["outs"]["out"] is x and r["outs"]["labels_out"] is y
                continue
            outs = dict(r["outs"])
            if r["name"] == "mixup" and r["x"] is None:
                outs.pop("out")                        # mixup off: the launch builds the target rows alone
            if r["name"] == "crop":
                outs.pop("targets_out")                # (int32 labels only in the static modes)
            for k, t in outs.items():
                assert t is not None and _ptr(t) in own, (r["name"], k, "not a static buffer")
        assert all(t is None or _ptr(t) in own or t is x or t is y for t in out), "the step's kernels are handed a tensor made inside the capture"
        if c.loss == "off":
            assert out[1] is (bufs["yc"] if c.crop != "off" else y)
    # two stages share an output only where the later one is documented as in place, and then it is its own input
    written = {}
    for r in stages:
        t = r["outs"].get("out")
        if t is None:
            t = r["res"] if r["name"] != "gather_batch" else None
        if t is None:
            continue
        if r["name"] not in IN_PLACE:
            assert _ptr(t) != _ptr(r["x"]), (r["name"], "writes its own input")
        if _ptr(t) in written:
            assert r["name"] in IN_PLACE and _ptr(t) == _ptr(r["x"]), (r["name"], "shares its output with", written[_ptr(t)])
        written[_ptr(t)] = r["name"]
    for k in ("mask", "labels_out", "targets"):
        seen = [_ptr(r["outs"][k]) for r in stages if r["outs"].get(k) is not None]
        assert len(seen) == len(set(seen)), k
    # and the shapes the kernels are handed
    rows, W = (pl.B * pl.CROP_R, pl.CROP_W) if c.crop != "off" else (pl.B, pl.T)
    per_model = n > 1 and (c.xin == "per" or c.augment or c.align or c.crop != "off" or c.loss == "mix")
    assert tuple(out[0].shape) == ((n, rows, W, pl.C) if per_model else (rows, W, pl.C)) and recipe.dims(pl.B, pl.T) == (rows, W)
