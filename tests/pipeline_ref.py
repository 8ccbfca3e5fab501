"""The composed reference of a training step's front end, and the table of rows the pipeline tests run.

prepare_ref() states what the model kernels of step `step` must see -- windows [rows, W, C] and int32 labels or fp32 target rows, per
model -- for a given batch, seeds and stage settings.  It is built ONLY by calling the per-stage restatements under tests/
(gather_ref, augment_ref, gate_ref, prep_ref, align_ref, crop_ref, mixup_ref) in the order the StepRecipe docstring states,

    gather -> augment (+ fused z-score) -> gate -> prep -> gate-apply -> align -> crop (+ z-score on the crops) -> mixup / target rows,

with the stream ids of step_recipe.base_stream and the slot constants (every drawing stage uses base_stream + SLOT_AUGMENT, on index
slots of its own).  The rules it encodes are the documented ones (StepRecipe, include/nsd.h):
  * the apply stage of a training step never rejects (max_bad = C);
  * with a crop, augment runs without its fused z-score and the z-score is taken on the crops;
  * labels and float target rows are repeated per crop, and mixup pairs crops;
  * a model with no augment / loss beside one that has them gets bit-copied windows and one-hot rows, and a row of ones for weights;
  * gather copies bits and moves no stream.

The z-score link.  nsd_zscore_fwd has no bitwise restatement: tests/test_gpu_small_kernels.py holds it to float64 within 2e-5, and its
fused form is held bit-equal to ops.zscore by tests/test_gpu_augment.py.  In rows with normalize=True the z-score link of the chain is
therefore THE KERNEL ITSELF: prepare_ref takes `zscore=`, a callable on [n, T, C] float32 numpy windows, and calls it once, on all
models' pre-z-score windows; the GPU tests pass a function that uploads them and calls ops.zscore.  The CPU tests pass the float64
restatement of tests/small_kernels_ref.py (they check order, shapes and which stage acts, not those bits).  Every other link is numpy.

CASES is the table: two full-chain blocks (every compatible stage on, in each of the five modes; one normalize row with everything
compatible with it) and a pairwise cover of the factors below over the allowed combinations; tests/test_pipeline_cpu.py proves the
cover by enumeration.  Imports without a GPU.
"""
from collections import namedtuple

import numpy as np

from nsd_amd.step_recipe import SLOT_AUGMENT, base_stream, trainer_seed
from tests import align_ref, augment_ref, crop_ref, gate_ref, gather_ref, mixup_ref, prep_ref

assert augment_ref.AUG_STREAM == SLOT_AUGMENT        # the restatements draw on base_stream + SLOT_AUGMENT, as the kernels do

F32 = np.float32
STAGES = ("gather", "augment", "zscore", "gate", "prep", "apply", "align", "crop", "zscore_crops", "mixup")      # the documented order


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _differs(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape != b.shape or not np.array_equal(_bits(a), _bits(b))


def _entries(v, M):
    """a setting given once (or None) or per model -> its M entries"""
    return list(v) if isinstance(v, (list, tuple)) else [v] * M


def prepare_ref(x, y, seeds, step, *, M=1, K=3, augment=None, gate=None, prep=None, align=None, crop=None, loss=None, normalize=False,
                zscore=None, bound=None, trace=None):
    """What the model kernels of step `step` (1-based) see.

    x        host windows [B,T,C] (one model, or shared by M) or [M,B,T,C]; None with bound=
    y        int labels [B] (shared) or [M,B] / [M*B], or float32 target rows [B,K] (one model)
    bound    dict(x [N,T,C], y [N] int or [N,K] float, table int [M,S,B], first: the step that reads row 0) -- the resident trial set
             and the schedule's index table, in place of x and y
    seeds    the per-model seeds AS THE KERNELS SEE THEM (trainer_seed)
    augment  None, a dict of augment_ref.augment's keywords, or a list of M (None: that model's windows are copied)
    gate     None or the gate's fields (SignalGate.to_dict());  prep: None or prep_ref's keywords
    align    None, a matrix [C,C] (one model) or [M,C,C]
    crop     None or dict(window, crops, hop)
    loss     None, dict(eps, weights, mix), or a list of M (None: one-hot rows, unit weights, windows copied)
    zscore   with normalize: the callable that IS the z-score link (module docstring)
    trace    a dict that receives, per stage that ran, one bool per model: did the stage change the bits of its input

    -> (windows float32 [M, rows, W, C], labels int32 [M, rows] or None, targets float32 [M, rows, K] or None)"""
    seeds = [int(s) for s in seeds]
    assert len(seeds) == M
    bs = base_stream(step)
    trace = {} if trace is None else trace

    def note(stage, before, after):
        trace[stage] = [bool(_differs(b, a)) for b, a in zip(before, after)]

    # gather: a bitwise copy of the named trials and their labels / rows; no stream moves
    if bound is not None:
        assert x is None and y is None
        xa, ya, table = np.asarray(bound["x"], F32), np.asarray(bound["y"]), np.asarray(bound["table"], np.int32)
        soft = ya.dtype.kind == "f"
        xo, lo, to, status = gather_ref.gather(xa, table, step, step_base=bound["first"], labels_all=None if soft else ya.astype(np.int32),
                                               targets_all=ya.astype(F32) if soft else None)
        assert not status.any()
        Bn = table.shape[2]
        v = [xo[m].view(F32) for m in range(M)]
        ys = [to.view(F32).reshape(M, Bn, -1)[m] if soft else lo.reshape(M, Bn)[m] for m in range(M)]
        note("gather", [xa[:Bn]] * M, v)
    else:
        x, y = np.asarray(x, F32), np.asarray(y)
        soft = y.dtype.kind == "f"
        v = [x if x.ndim == 3 else x[m] for m in range(M)]
        Bn = v[0].shape[0]
        if soft:
            assert M == 1 and y.shape == (Bn, K)
            ys = [y.astype(F32)]
        else:
            yy = y.astype(np.int32).reshape(-1)
            ys = [yy if yy.size == Bn else yy.reshape(M, Bn)[m] for m in range(M)]
    Cc = v[0].shape[-1]

    def zs(ws, stage):
        out = zscore(np.ascontiguousarray(np.stack(ws).reshape((-1,) + ws[0].shape[1:]), dtype=F32)).reshape((M,) + ws[0].shape)
        note(stage, ws, list(out))
        return [np.ascontiguousarray(o, dtype=F32) for o in out]

    # augment, the whole-window z-score fused behind it -- unless a crop follows: then the z-score is of the crops
    augs = _entries(augment, M)
    if any(a is not None for a in augs):
        w = [augment_ref.augment(v[m], seeds[m], bs, **augs[m]) if augs[m] is not None else v[m].copy() for m in range(M)]
        note("augment", v, w)
        v = w
    if normalize and crop is None:
        v = zs(v, "zscore")
    # gate -> prep -> apply: the detector sees the raw (augmented) samples; inside a training step nothing is rejected
    if gate is not None:
        held, masks = zip(*[gate_ref.gate_ref(v[m], gate) for m in range(M)])
        note("gate", v, held)
        v = list(held)
    if prep is not None:
        w = [prep_ref.prep_ref(v[m], **prep) for m in range(M)]
        note("prep", v, w)
        v = w
    if gate is not None:
        w = [gate_ref.apply_ref(v[m], masks[m], dict(gate, max_bad=Cc)) for m in range(M)]
        note("apply", v, w)
        v = w
    if align is not None:
        A = np.asarray(align, F32)
        assert A.shape == ((Cc, Cc) if M == 1 and A.ndim == 2 else (M, Cc, Cc))
        w = [align_ref.apply_ref(v[m], A if A.ndim == 2 else A[m]) for m in range(M)]
        note("align", v, w)
        v = w
    # crop: windows, labels and rows repeated per crop; each model with its own offsets
    if crop is not None:
        cut = [crop_ref.crop(v[m], crop["window"], crop["crops"], crop["hop"], seeds[m], bs, labels=None if soft else ys[m],
                             targets=ys[m] if soft else None) for m in range(M)]
        w = [c[0] for c in cut]
        note("crop", v, w)
        v, ys = w, [c[2] if soft else c[1] for c in cut]
        if normalize:
            v = zs(v, "zscore_crops")
    v = [np.ascontiguousarray(a, dtype=F32) for a in v]
    losses = _entries(loss, M)
    if soft:
        assert all(lo is None for lo in losses)                      # float rows are used as they are
        return np.stack(v), None, np.stack(ys).astype(F32)
    if all(lo is None for lo in losses):
        return np.stack(v), np.stack(ys).astype(np.int32), None
    # mixup / target rows: on what the model would otherwise see; the windows are mixed (or copied) as soon as one model mixes
    off = dict(eps=0.0, weights=None, mix=0.0)
    losses = [dict(off, **lo) if lo is not None else dict(off) for lo in losses]
    if any(lo["weights"] is not None for lo in losses):
        for lo in losses:
            lo["weights"] = lo["weights"] if lo["weights"] is not None else (1.0,) * K
    mixing = any(lo["mix"] > 0 for lo in losses)
    out = [mixup_ref.mixup(v[m] if mixing else None, ys[m], K, seeds[m], bs, mix=losses[m]["mix"], eps=losses[m]["eps"],
                           weights=losses[m]["weights"]) for m in range(M)]
    if mixing:
        w = [o[0] for o in out]
        note("mixup", v, w)
        v = w
    onehot = [mixup_ref.base_rows(ys[m], K) for m in range(M)]
    trace["targets"] = [bool(_differs(onehot[m], out[m][1])) for m in range(M)]
    return np.stack(v), None, np.stack([o[1] for o in out]).astype(F32)


# ------------------------------------------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------------------------------------------
# The default model (C = 8, H = 48, L = 2, K = 3, F = 32): the only shape all three trainers and the model-batched path share.
# B = 5 trials (odd: mixup's partner rotation has an odd cycle), T = 40, crops of 16 x 3 (drawn: hop 0; grid: hop 12, 16 + 2 * 12 = 40
# reaches the last sample), a resident set of N = 11 trials with schedules of S = 3 rows, M = 3 models.
B, T, C, K, M, N, S = 5, 40, 8, 3, 3, 11, 3
CROP_W, CROP_R, GRID_HOP = 16, 3, 12
STEPS = (1, 2, 3)
SEEDS = (11, 12, 13)                 # the callers' seeds; the kernels see trainer_seed(seed)
DROPOUT = (0.6, 0.3, 0.5)            # mode "each": the models' own probabilities (the other modes: 0.6, the model's default)

FACTORS = dict(
    source=("host", "bound"),        # host-fed; bound (bind_batches + step_scheduled)
    augment=(0, 1), gate=(0, 1), prep=(0, 1), align=(0, 1),
    crop=("off", "grid", "drawn"),
    loss=("off", "smooth", "mix"),   # off; smoothing + weights; mixup + smoothing + weights
    targets=("int", "float"),
    normalize=(0, 1),
    tail=("plain", "clip", "avg", "sam", "all"),       # clip: global-norm clipping + LR schedule; all: the four together
    mode=("eager", "static", "sched", "multi", "each"))
# eager: Trainer.step (bound: step_scheduled());  static: Trainer.step_static;  sched: Trainer.step_scheduled(static=True);
# multi: ModelBatchTrainer with one setting for all models;  each: ModelBatchTrainer with per-model augment / loss / sam / dropout lists
# (whichever of them the row has on), so that nsd_augment_each / nsd_mixup_each and the per-model SAM rows run.


def refused(c):
    """Why a combination of levels is not a step this package takes (None: it is one).  Each reason names the line that refuses it;
    tests/test_pipeline_cpu.py constructs the refused arguments and expects that error."""
    if c["normalize"] and c["gate"]:
        return "EEG_LSTM.__init__: gate together with normalize=True"
    if c["normalize"] and c["prep"]:
        return "EEG_LSTM.__init__: prep together with normalize=True"
    if c["normalize"] and c["align"]:
        return "EEG_LSTM.__init__: align together with normalize=True"
    if c["targets"] == "float" and c["loss"] != "off":
        return "Trainer.step: float targets together with loss="
    if c["targets"] == "float" and c["mode"] in ("static", "sched"):
        return "Trainer.static_inputs holds int32 labels; Trainer.step_scheduled(static=True): a trial set of target rows steps with static=False"
    if c["targets"] == "float" and c["mode"] in ("multi", "each"):
        return "ModelBatchTrainer.step: y.to(torch.int32); ModelBatchTrainer.bind_batches: the trial set holds target rows"
    if c["mode"] == "sched" and c["source"] != "bound":
        return "Trainer.step_scheduled: no batches bound"
    if c["mode"] == "static" and c["source"] != "host":
        return "Trainer.step_static steps on the static inputs its caller fills (the bound form of it is mode sched)"
    return None
# Two further refusals leave no level in the table: drawn crop offsets with stochastic=False (StepRecipe.__init__; every row here trains
# with stochastic=True, which the graph step needs anyway) and a per-model crop (StepRecipe.__init__: the models have different crop
# settings).


Case = namedtuple("Case", "id source augment gate prep align crop loss targets normalize tail mode xin")
# xin: "shared" -- the model-batched step is fed one [B,T,C] batch and one [B] label vector for all models; "per" -- [M,B,T,C] / [M,B]
# (bound rows gather per model; single-model rows: "-").  Rows with float targets run in mode eager: the model-batched trainer and the
# static inputs take int32 labels only (refused() above), so a single Trainer is the mode that can express them.
_ROWS = [
    # every compatible stage on, in each of the five modes
    (0,  "host",  1, 1, 1, 1, "drawn", "mix",    "int",   0, "all",   "eager",  "-"),
    (1,  "host",  1, 1, 1, 1, "drawn", "mix",    "int",   0, "all",   "static", "-"),
    (2,  "bound", 1, 1, 1, 1, "drawn", "mix",    "int",   0, "all",   "sched",  "-"),
    (3,  "bound", 1, 1, 1, 1, "drawn", "mix",    "int",   0, "all",   "multi",  "per"),
    (4,  "host",  1, 1, 1, 1, "drawn", "mix",    "int",   0, "all",   "each",   "shared"),
    # normalize with everything compatible with it
    (5,  "bound", 1, 0, 0, 0, "drawn", "mix",    "int",   1, "all",   "eager",  "-"),
    # the pairwise cover
    (6,  "host",  0, 1, 0, 0, "grid",  "off",    "float", 0, "avg",   "eager",  "-"),
    (7,  "bound", 0, 0, 1, 1, "off",   "smooth", "int",   0, "clip",  "each",   "per"),
    (8,  "host",  1, 0, 0, 0, "grid",  "smooth", "int",   1, "sam",   "multi",  "per"),
    (9,  "bound", 1, 0, 0, 0, "off",   "off",    "int",   1, "plain", "sched",  "-"),
    (10, "bound", 0, 1, 1, 1, "off",   "off",    "float", 0, "sam",   "eager",  "-"),
    (11, "host",  0, 0, 0, 0, "drawn", "off",    "int",   1, "clip",  "static", "-"),
    (12, "bound", 0, 1, 1, 1, "grid",  "mix",    "int",   0, "plain", "sched",  "-"),
    (13, "bound", 1, 0, 0, 0, "off",   "mix",    "int",   1, "avg",   "each",   "per"),
    (14, "host",  0, 1, 1, 0, "drawn", "smooth", "int",   0, "plain", "static", "-"),
    (15, "host",  0, 1, 0, 1, "off",   "off",    "int",   0, "all",   "multi",  "shared"),
    (16, "bound", 1, 0, 0, 0, "grid",  "off",    "float", 1, "clip",  "eager",  "-"),
    (17, "bound", 0, 1, 1, 1, "drawn", "smooth", "int",   0, "avg",   "sched",  "-"),
    (18, "host",  1, 1, 0, 1, "drawn", "mix",    "int",   0, "clip",  "multi",  "shared"),
    (19, "host",  0, 0, 1, 1, "drawn", "mix",    "int",   0, "sam",   "static", "-"),
    (20, "bound", 0, 1, 1, 0, "grid",  "smooth", "int",   0, "all",   "each",   "per"),
    (21, "bound", 0, 1, 1, 0, "drawn", "off",    "float", 0, "plain", "eager",  "-"),
    (22, "host",  0, 0, 1, 0, "off",   "smooth", "int",   0, "avg",   "static", "-"),
    (23, "host",  0, 1, 1, 1, "grid",  "off",    "int",   0, "plain", "each",   "per"),
    (24, "bound", 1, 1, 1, 0, "drawn", "mix",    "int",   0, "clip",  "sched",  "-"),
    (25, "host",  1, 0, 0, 0, "grid",  "mix",    "int",   1, "plain", "multi",  "shared"),
    (26, "host",  1, 1, 1, 1, "drawn", "off",    "int",   0, "avg",   "multi",  "per"),
    (27, "host",  1, 0, 1, 0, "off",   "smooth", "int",   0, "all",   "eager",  "-"),
    (28, "host",  1, 0, 0, 0, "grid",  "smooth", "int",   1, "clip",  "static", "-"),
    (29, "host",  0, 1, 1, 1, "drawn", "off",    "float", 0, "all",   "eager",  "-"),
    (30, "bound", 0, 0, 0, 0, "off",   "smooth", "int",   1, "sam",   "each",   "per"),
    (31, "bound", 0, 1, 0, 0, "grid",  "off",    "int",   0, "sam",   "sched",  "-"),
    # beyond the pairs: the align stage and the mixing as the FIRST stage of a step, where the buffer they read is the caller's own
    (32, "host",  0, 0, 0, 1, "off",   "off",    "int",   0, "plain", "eager",  "-"),
    (33, "host",  0, 0, 0, 1, "grid",  "off",    "int",   0, "plain", "static", "-"),
    (34, "host",  0, 0, 0, 0, "off",   "mix",    "int",   0, "plain", "static", "-"),
]
CASES = [Case(*r) for r in _ROWS]
FULL_CHAIN_IDS, NORMALIZE_ROW_ID = (0, 1, 2, 3, 4), 5


def case_id(c):
    on = "".join(ch for ch, f in zip("AGPL", (c.augment, c.gate, c.prep, c.align)) if f) or "none"
    return (f"{c.id:02d}-{c.mode}-{c.source}-{on}-crop_{c.crop}-loss_{c.loss}-{c.targets}{'-norm' if c.normalize else ''}-{c.tail}"
            + ("" if c.xin == "-" else f"-{c.xin}"))


def models_of(c):
    return M if c.mode in ("multi", "each") else 1


# ------------------------------------------------------------------------------------------------------------------------------------
# the settings of a row: the package's objects (for the trainers) and the restatements' keywords (for prepare_ref)
# ------------------------------------------------------------------------------------------------------------------------------------
AUGMENTS = (dict(max_shift=3, scale_range=0.1, p_channel=0.2, noise_std=0.3), None, dict(max_shift=2, scale_range=0.05, noise_std=0.5))
LOSSES = {"smooth": (dict(eps=0.1, weights=(1.0, 2.0, 0.5)), None, dict(eps=0.2)),
          "mix": (dict(eps=0.1, weights=(1.0, 2.0, 0.5), mix=0.5), None, dict(eps=0.2, weights=(0.5, 1.0, 2.0), mix=1.0))}
GATE = dict(rail=100.0, hold_samples=2, max_bad=2)       # max_bad = 2: the three-channel pop below would be rejected outside a training step
PREP = dict(highpass=1.0, lowpass=40.0, zscore_seconds=0.4, var0=250.0, car=True)          # CausalPrep.design's keywords
SAMS = (0.05, None, 0.1)
TAILS = {"plain": (), "clip": ("clip",), "avg": ("avg",), "sam": ("sam",), "all": ("clip", "avg", "sam")}


def settings(c):
    """-> dict(model: EEG_LSTM keywords (without the alignment matrix), trainer: the trainer's keywords beside lr / seed(s), dropouts: one
    per model, ref: prepare_ref's stage keywords (without align=, which changes during a run))"""
    import nsd_amd
    n, each = models_of(c), c.mode == "each"
    gate = nsd_amd.SignalGate(**GATE) if c.gate else None
    prep = nsd_amd.CausalPrep.design(**PREP) if c.prep else None
    model = dict(normalize=bool(c.normalize), gate=gate, prep=prep, align=nsd_amd.SessionAlign() if c.align else None)
    crop = None if c.crop == "off" else dict(window=CROP_W, crops=CROP_R, hop=GRID_HOP if c.crop == "grid" else 0)
    augs = (list(AUGMENTS) if each else AUGMENTS[0]) if c.augment else None
    losses = (list(LOSSES[c.loss]) if each else LOSSES[c.loss][0]) if c.loss != "off" else None
    as_aug = lambda a: None if a is None else nsd_amd.Augment(**a)
    as_loss = lambda lo: None if lo is None else nsd_amd.Loss(label_smoothing=lo.get("eps", 0.0), class_weights=lo.get("weights"), mixup=lo.get("mix", 0.0))
    tail, parts = {}, TAILS[c.tail]
    if "clip" in parts:
        tail.update(clip_grad_norm=0.5, lr_schedule=nsd_amd.LrSchedule(kind="cosine", warmup_steps=2, total_steps=10, min_ratio=0.1))
    if "avg" in parts:
        tail.update(average=nsd_amd.Average(kind="ema", decay=0.9))
    sams = None
    if "sam" in parts:
        sams = [None if r is None else nsd_amd.Sam(rho=r) for r in SAMS] if each else nsd_amd.Sam(rho=SAMS[0])
        tail.update(sam=sams)
    trainer = dict(tail, augment=[as_aug(a) for a in augs] if isinstance(augs, list) else as_aug(augs),
                   loss=[as_loss(lo) for lo in losses] if isinstance(losses, list) else as_loss(losses),
                   crop=None if crop is None else nsd_amd.Crop(**crop))
    ref = dict(M=n, K=K, augment=augs, gate=gate.to_dict() if gate else None,
               prep=dict(sections=prep.sections, alpha=prep.alpha, var0=prep.var0, baseline=prep.baseline, car=prep.car) if prep else None,
               crop=crop, loss=losses, normalize=bool(c.normalize))
    return dict(model=model, trainer=trainer, dropouts=list(DROPOUT) if each else [0.6] * n, ref=ref, sams=sams)


def plain_tail(c, m):
    """the tail keywords of the plain Trainer that shadows model m of row c"""
    st = settings(c)
    tail = {k: v for k, v in st["trainer"].items() if k in ("clip_grad_norm", "lr_schedule", "average")}
    sam = st["sams"][m] if isinstance(st["sams"], list) else st["sams"]
    if sam is not None:
        tail["sam"] = sam
    return tail


# ------------------------------------------------------------------------------------------------------------------------------------
# the inputs of a row: made so that every enabled stage visibly acts
# ------------------------------------------------------------------------------------------------------------------------------------
def _trials(n, rs):
    """n trials of clean noise of 10 units; trial i rails channel i % C at sample (5 + 3 i) % T (so the gate fires in every trial), and
    every B-th trial pops three channels at once at sample 30 (more than the gate's max_bad: rejected outside a training step)"""
    x = np.clip(10.0 * rs.standard_normal((n, T, C)), -40, 40).astype(F32)
    for i in range(n):
        x[i, (5 + 3 * i) % T, i % C] = 300.0 if i % 2 == 0 else -300.0
    x[::B, 30, 1:4] = 500.0
    return x


def _soft_rows(n, rs):
    """non-negative rows with sums != 1 and a zero row"""
    q = (1.5 * rs.rand(n, K)).astype(F32)
    q[1] = 0.0
    return q


def _matrices(n, rs):
    """non-identity, non-symmetric alignment matrices near the identity: [C,C] for n = 1, else [n,C,C]"""
    W = (np.eye(C) + 0.15 * rs.standard_normal((n, C, C))).astype(F32)
    return W[0] if n == 1 else W


def inputs(c):
    """-> dict: host rows: x[step], y[step];  bound rows: trials (x [N,T,C], y), tables {step: (table [M',S,B], first)} -- schedule A is
    bound before step 1 and schedule B, of the same shape, before step 2, and the first step after a binding reads row 0;  align[step]:
    the alignment matrices of the step (a new set is written in front of step 3)"""
    rs = np.random.RandomState(1000 + c.id)
    n = models_of(c)
    soft = c.targets == "float"
    out = dict(align={})
    if c.source == "host":
        out["x"], out["y"] = {}, {}
        for s in STEPS:
            per = n > 1 and c.xin == "per"
            x = _trials(n * B if per else B, rs)
            out["x"][s] = x.reshape(n, B, T, C) if per else x
            out["y"][s] = _soft_rows(B, rs) if soft else rs.randint(0, K, (n, B) if per else (B,)).astype(np.int32)
    else:
        out["trials"] = (_trials(N, rs), _soft_rows(N, rs) if soft else rs.randint(0, K, N).astype(np.int32))
        tabA = np.stack([np.stack([rs.permutation(N)[:B] for _ in range(S)]) for _ in range(n)]).astype(np.int32)
        tabB = np.stack([np.stack([rs.permutation(N)[:B] for _ in range(S)]) for _ in range(n)]).astype(np.int32)
        out["schedules"] = (tabA, tabB)
        out["tables"] = {1: (tabA, 1), 2: (tabB, 2), 3: (tabB, 2)}
    if c.align:
        W1, W2 = _matrices(n, rs), _matrices(n, rs)
        out["align"] = {1: W1, 2: W1, 3: W2}
    return out


def reference(c, zscore=None):
    """prepare_ref for the three steps of row c -> {step: (windows [M', rows, W, C], labels or None, targets or None, trace)}"""
    st, inp = settings(c), inputs(c)
    seeds = [trainer_seed(s) for s in SEEDS[:models_of(c)]]
    out = {}
    for s in STEPS:
        trace = {}
        kw = dict(st["ref"], align=inp["align"].get(s), zscore=zscore, trace=trace)
        if c.source == "host":
            w, lab, tg = prepare_ref(inp["x"][s], inp["y"][s], seeds, s, **kw)
        else:
            table, first = inp["tables"][s]
            w, lab, tg = prepare_ref(None, None, seeds, s, bound=dict(x=inp["trials"][0], y=inp["trials"][1], table=table, first=first), **kw)
        out[s] = (w, lab, tg, trace)
    return out


def expected_stages(c):
    """the stages of STAGES that row c has on, in the documented order"""
    on = dict(gather=c.source == "bound", augment=c.augment, zscore=c.normalize and c.crop == "off", gate=c.gate, prep=c.prep, apply=c.gate,
              align=c.align, crop=c.crop != "off", zscore_crops=c.normalize and c.crop != "off", mixup=c.loss == "mix")
    return [s for s in STAGES if on[s]]
