"""The one recipe of a training step: which random streams it draws and what the kernels see of (windows, labels, seed, step).
Trainer.step (eager), Trainer.step_static (hipGraph replay), ModelBatchTrainer.step and EEG_LSTM's train-mode surface take their stream
numbering from here, and the three trainer steps prepare their inputs through StepRecipe.prepare -- so "the replayed step is the eager
step" and "model m of the batched step is Trainer(model_m, seed=seeds[m])'s step" follow from the structure.
A step owns four consecutive streams of its seed, base_stream(step) + SLOT_* (the slots are named beside the launches, in ops.py).
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import ops
from .ops import SLOT_AUGMENT, SLOT_HEAD_DROPOUT, SLOT_LSTM_DROPOUT, SLOT_RRELU          # noqa: F401 (re-exported)


def trainer_seed(seed: int, rank: int = 0) -> int:
    """The seed a trainer's kernels see: the caller's seed moved by a golden-ratio multiple of (rank + 1), so ranks draw apart."""
    return (int(seed) + 0x9E3779B97F4A7C15 * (rank + 1)) & 0xFFFFFFFFFFFFFFFF


def base_stream(step: int) -> int:
    """First stream id of optimisation step `step`, as a uint32 (what nsd_*_dev form from the device step counter)."""
    return (int(step) & 0x3FFFFFFF) * 4


def step_rng(seed: int, step: int, p_lstm: float = 0.0, p_head: float = 0.0) -> dict:
    """The rng= / rngs= argument of the ops for step `step` of `seed`."""
    return dict(seed=seed, base_stream=base_stream(step), p_lstm=p_lstm, p_head=p_head)


def refuse_resample(models, who: str) -> None:
    """A trainer's batches are at the model's rate: prepare() runs no stage 0, so a model with a rate conversion would be trained on
    unconverted windows and evaluated on converted ones.  Refused where the trainer is built."""
    if any(getattr(m, "resample", None) is not None for m in models):
        raise ops.NsdError(f"{who}: the model has a rate conversion (EEG_LSTM(resample=...)), and a training step converts no rate: train "
                           "a resample-free model on converted trials (ops.resample_trials(x, resample)) and hand resample= to "
                           "save_reference_checkpoint, which writes the conversion into the checkpoint")


class StepRecipe:
    """What a trainer does to a batch before the step's kernels, and with which streams.  `model`: an EEG_LSTM (spec, dropout_p,
    head_dropout_p, normalize, prep).  augment / loss are the EFFECTIVE ones: augmentation and mixup belong to the stochastic parts, so
    stochastic=False strips them (smoothing and class weights, which draw nothing, stay); None -- also for an Augment / Loss with every
    part off -- is the plain step, launch for launch.

    models (ModelBatchTrainer): the M models of a model-batched step.  Each model then drops with its own dropout_p / head_dropout_p
    (rngs()), and augment / loss may be sequences of M, one per model (a hyper-parameter grid in one launch).  Sequences whose
    effective entries are all equal are the single setting, launch for launch.  Where they differ, self.augment / self.loss are lists
    of M (an Augment() / Loss() with every part off for a model without one: its windows are copied bit for bit and its target rows
    are one-hot), the launches are nsd_augment_each / nsd_mixup_each, and class weights go as [M, K] (a row of ones -- an exact
    product -- for a model without weights).

    sam (ops.Sam; with models a sequence of M, None for a model without it): sharpness-aware minimisation.  What it changes in a step
    is said here and nowhere else: the step's forward/backward launches are issued TWICE, on the parameters and then on the perturbed
    rows the ascent leaves in the trainer's sam_state, and everything around them once -- prepare() runs once (one augmentation, one
    mixup), the step counter advances once, and both passes get the same rng() / rngs() dicts or the same explicit mask tensors, so
    pass 2 sees pass 1's draws (the streams are counter-based).  The tail is the step's usual one, on the real parameters.  SAM is
    not one of the stochastic parts: stochastic=False keeps it.  self.sam is None (off: today's calls), one Sam, or where the models
    differ a list of M (None: that model's second pass runs on a copy of its parameters); passes() drives the two passes.

    crop (ops.Crop): cropped training.  The step's kernels then see B * R windows of W samples in place of B trials of T: prepare()
    cuts them (nsd_crop) behind the front end and in front of the mixing, augment -> prep -> crop -> mixup -- the front end has run
    over the whole trial before a window begins, as a stream's filter has, and mixup pairs crops.  With normalize the whole-window
    z-score is of what the model sees: nsd_augment runs without its fused z-score and nsd_zscore_fwd runs on the crops.  Labels and
    float target rows are repeated per crop.  W and R set the launch dimensions, so cropping is not one of the per-model axes: a
    sequence must hold equal entries.  Drawn offsets (hop = 0) are a stochastic part, but a deterministic trainer cannot simply drop
    them -- the step's dimensions hang on the crop -- so stochastic=False with hop = 0 is refused; a regular grid draws nothing and
    stays.  None: today's step, launch for launch.  dims() gives the dimensions the step's kernels see.

    Bound batches (bind() / take() / gather() / check_gather(), behind the trainers' bind_batches and step_scheduled): the trials and
    the run's index schedule stay on the device and nsd_gather forms each step's batch there, as the stage in front of prepare():
    gather -> augment -> prep -> crop -> mixup.  It draws nothing and copies bit for bit, so the step behind it is the host-fed step.

    A model with a signal-quality gate (EEG_LSTM(gate=...)) adds its two stages around the front end, in window mode: gather -> augment
    -> gate -> prep -> apply -> crop -> mixup.  The apply stage of a training step never rejects (max_bad = C), so the loss stays finite;
    bad trials are dropped at the data-set level (data.screen_trials).

    A model with session alignment (EEG_LSTM(align=...)) adds the stage behind the front end and in front of the crop: gather ->
    augment -> gate -> prep -> apply -> align -> crop -> mixup.  One nsd_spatial_apply, in place in the buffer the front end wrote (or
    into bufs["xn"]); it draws nothing and moves no stream.  One model uses its own matrix (sel = NULL); with models= the recipe holds
    one matrix per model ([M,C,C], a copy of the models' at construction: set_alignment() writes both) and a static int32 selection
    [M*B], model m's rows naming matrix m.

    A model with a rate conversion (EEG_LSTM(resample=...)) is refused: prepare() has no stage 0, the batches are at the model's rate."""

    def __init__(self, model, stochastic: bool, augment, loss, device, models: Optional[Sequence] = None, sam=None, crop=None):
        refuse_resample([model] if models is None else models, "StepRecipe")
        self.spec, self.stochastic, self.normalize, self.prep = model.spec, stochastic, model.normalize, model.prep
        self.gate = getattr(model, "gate", None)
        self.align = getattr(model, "align", None)
        self.align_W, self._align_models, self._align_sel = None, models, {}
        if self.align is not None:
            self.align_W = model.align_matrix if models is None else torch.stack([m.align_matrix for m in models]).contiguous()
        self.p_lstm, self.p_head = model.dropout_p, model.head_dropout_p
        self.probs = [(m.dropout_p, m.head_dropout_p) for m in models] if models is not None else None
        M = len(models) if models is not None else 1
        augs = [self._effective_augment(a) for a in self._entries(augment, M, "augment")]
        losses = [self._effective_loss(lo) for lo in self._entries(loss, M, "loss")]
        if all(a == augs[0] for a in augs):
            self.augment = augs[0]
        else:
            self.augment = [a if a is not None else ops.Augment() for a in augs]
        if all(lo == losses[0] for lo in losses):
            self.loss = losses[0]
            self.class_weights = None if self.loss is None else self.loss.weights_tensor(device)
        else:
            self.loss = [lo if lo is not None else ops.Loss() for lo in losses]
            rows = [lo.class_weights for lo in self.loss]
            self.class_weights = None if all(r is None for r in rows) else torch.tensor(
                [r if r is not None else (1.0,) * self.spec.K for r in rows], dtype=torch.float32, device=device)

        sams = self._entries(sam, M, "sam")
        for e in sams:
            if e is not None and not isinstance(e, ops.Sam):
                raise ValueError(f"StepRecipe: sam {e!r}: an ops.Sam or None")
        self.sam = sams[0] if all(e == sams[0] for e in sams) else sams

        crops = self._entries(crop, M, "crop")
        for e in crops:
            if e is not None and not isinstance(e, ops.Crop):
                raise ValueError(f"StepRecipe: crop {e!r}: an ops.Crop or None")
        if any(e != crops[0] for e in crops):
            raise ops.NsdError("StepRecipe: the models have different crop settings: window and crops set the dimensions of the launch, "
                               "so cropping is not a per-model setting (train models of different windows in different trainers)")
        self.crop = crops[0]
        if self.crop is not None and self.crop.hop == 0 and not stochastic:
            raise ops.NsdError("StepRecipe: stochastic=False with drawn crop offsets (hop = 0): a deterministic trainer draws nothing; "
                               "give the crop a regular grid (hop > 0)")

    def dims(self, B: int, T: int):
        """(rows, samples) the step's kernels see for B trials of T samples: (B * crops, window) with a crop, else (B, T)"""
        if self.crop is None:
            return B, T
        self.crop.check_trial(T)
        return B * self.crop.crops, self.crop.window

    def sam_args(self, sam_state: Optional[torch.Tensor]) -> dict:
        """sam= / sam_state= of ops.train_step_grads / ops.multi_train_step (empty without SAM: the calls are today's)"""
        return {} if self.sam is None else dict(sam=self.sam, sam_state=sam_state)

    def passes(self, params: torch.Tensor, sam_state: Optional[torch.Tensor], forward_backward, ascend) -> None:
        """The forward/backward passes of a step whose trainer issues them itself (the bf16 sequence path; the fp32 ops take sam_args()
        and do the same inside): forward_backward(params) once, and with SAM ascend() and forward_backward(perturbed row) -- the
        callable is the same, so the batch, targets, rng and workspace of the two passes are."""
        forward_backward(params)
        if self.sam is not None and sam_state is not None:
            ascend()
            forward_backward(ops.sam_rows(sam_state, 1, params.numel())[0])

    @staticmethod
    def _entries(v, M: int, name: str) -> list:
        if not isinstance(v, (list, tuple)):
            return [v] * M
        if len(v) != M:
            raise ops.NsdError(f"StepRecipe: {len(v)} {name} entries for {M} models")
        return list(v)

    def _effective_augment(self, augment: Optional[ops.Augment]) -> Optional[ops.Augment]:
        return augment if augment is not None and augment.enabled and self.stochastic else None

    def _effective_loss(self, loss: Optional[ops.Loss]) -> Optional[ops.Loss]:
        if loss is not None and loss.mixup and not self.stochastic:
            loss = ops.Loss(label_smoothing=loss.label_smoothing, class_weights=loss.class_weights)
        if loss is None or not loss.enabled:
            return None
        loss.check_classes(self.spec.K)
        return loss

    def rng(self, seed: int, step: int) -> Optional[dict]:
        """The in-kernel streams of the step (None for a deterministic trainer)."""
        return step_rng(seed, step, self.p_lstm, self.p_head) if self.stochastic else None

    def rngs(self, seeds: Sequence[int], step: int) -> Optional[list]:
        """The in-kernel streams of a model-batched step: model m's with its own dropout probabilities (None: deterministic)."""
        if not self.stochastic:
            return None
        probs = self.probs if self.probs is not None else [(self.p_lstm, self.p_head)] * len(seeds)
        return [step_rng(s, step, pl, ph) for s, (pl, ph) in zip(seeds, probs)]

    def gather(self, bound: dict, step: int, *, step_dev: Optional[torch.Tensor] = None, x: Optional[torch.Tensor] = None,
               y: Optional[torch.Tensor] = None):
        """The stage in front of prepare() for a trainer with bound batches (bind_batches): gather -> augment -> prep -> crop -> mixup.
        One nsd_gather forms the batch of step `step` (1-based, or the device counter step_dev) of all models of the bound table from
        the resident trials -> (x [M,B,T,C] or [B,T,C], labels [M*B] or target rows [M*B,K]), into the bound buffers or into x / y (a
        static step's inputs).  The gather draws nothing: no stream moves, and the step behind it is the step on these windows."""
        trials = bound["trials"]
        soft = trials.labels is None
        xo, lo, to = ops.gather_batch(trials.x, bound["table"], step=step, step_base=bound["base"], step_dev=step_dev,
                                      labels_all=trials.labels, targets_all=trials.targets, out=x if x is not None else bound["x"],
                                      labels_out=None if soft else (y if y is not None else bound["y"]),
                                      targets_out=(y if y is not None else bound["y"]) if soft else None, status=bound["status"])
        return xo, (to if soft else lo)

    @staticmethod
    def bind(bound: Optional[dict], trials, schedule, M: int, next_step: int, who: str):
        """The bound-batches record of a trainer of M models whose next step is `next_step` -> (record, kept).  A schedule of the
        bound shape on the bound trials is copied into the device table in place (kept: captured graphs hold its address and
        step_base, so the rows are rotated to put row 0 at next_step); anything else gets new buffers."""
        import numpy as np
        if schedule.M != M:
            raise ops.NsdError(f"{who}: the schedule holds {schedule.M} models' batches, the trainer {M}")
        try:
            schedule.check_trials(len(trials))
        except ValueError as e:
            raise ops.NsdError(f"{who}: {e}") from None
        S, B = schedule.steps, schedule.batch
        N, T, Cc = (int(v) for v in trials.x.shape)
        if not ops.gather_path(B, T, Cc, M, N, S):
            raise ops.NsdError(f"{who}: M = {M}, N = {N}, S = {S}, B = {B}, T = {T}, C = {Cc} are outside nsd_gather (nsd_gather_path)")
        kept = bound is not None and bound["trials"] is trials and (bound["M"], bound["S"], bound["B"]) == (M, S, B)
        if kept:
            shift = (next_step - bound["base"]) % S
            bound["table"].copy_(torch.from_numpy(np.roll(schedule.table, shift, axis=1)).view(bound["table"].shape))
            bound["status"].zero_()
            bound.update(first=next_step, taken=0)
            return bound, True
        dev = trials.x.device
        one = M == 1
        y = (torch.empty((M * B, trials.targets.shape[1]), dtype=torch.float32, device=dev) if trials.labels is None
             else torch.empty((M * B,), dtype=torch.int32, device=dev))
        return dict(trials=trials, table=torch.from_numpy(schedule.table).to(dev).view((S, B) if one else (M, S, B)), base=next_step,
                    first=next_step, taken=0, M=M, S=S, B=B, T=T, status=torch.zeros(M, dtype=torch.int32, device=dev),
                    x=torch.empty((B, T, Cc) if one else (M, B, T, Cc), dtype=torch.float32, device=dev), y=y), False

    @staticmethod
    def take(bound: Optional[dict], who: str) -> dict:
        """The host's count of the bound schedule's steps: NsdError without a schedule or past its last row."""
        if bound is None:
            raise ops.NsdError(f"{who}: no batches bound (bind_batches(trials, schedule) first)")
        if bound["taken"] >= bound["S"]:
            raise ops.NsdError(f"{who}: the bound schedule's {bound['S']} steps are taken; bind the next schedule")
        bound["taken"] += 1
        return bound

    @staticmethod
    def check_gather(bound: Optional[dict], who: str) -> None:
        """NsdError naming the models whose gather met a trial index outside the set (nsd_gather's status; synchronises)."""
        if bound is None:
            return
        bad = [m for m, s in enumerate(bound["status"].cpu().tolist()) if s]
        if bad:
            raise ops.NsdError(f"{who}: the batch schedule of model(s) {bad} named a trial outside the resident set of "
                               f"{len(bound['trials'])}: those rows were NaN and their steps skipped or spoilt.  Results are invalid")

    def set_alignment(self, W) -> None:
        """Write the alignment matrices ([C,C] for one model, [M,C,C] with models=) into the recipe's table and the models' buffers, in
        place: a captured step reads the new matrices at its next replay."""
        if self.align is None:
            raise ops.NsdError("StepRecipe.set_alignment: the model was built without align=SessionAlign(...)")
        W = torch.as_tensor(W, dtype=torch.float32)
        if tuple(W.shape) != tuple(self.align_W.shape):
            raise ValueError(f"set_alignment: expected matrices of shape {tuple(self.align_W.shape)}, got {tuple(W.shape)}")
        with torch.no_grad():
            self.align_W.copy_(W)
            for m, mdl in enumerate(self._align_models or ()):
                mdl.align_matrix.copy_(self.align_W[m])

    def align_apply(self, x: torch.Tensor, *, fresh: bool, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The align stage on x [B,T,C] or [M,B,T,C] (no-op without align): in place where x is a buffer of this step's own (fresh),
        else into out (or a new buffer).  With one matrix per model a shared [B,T,C] becomes [M,B,T,C]."""
        if self.align is None:
            return x
        W = self.align_W
        if W.dim() == 2:
            return ops.spatial_apply(x, W, out=x if fresh else out)
        M, B = int(W.shape[0]), int(x.shape[-3])
        if x.dim() == 3:
            x, fresh = x.unsqueeze(0).expand(M, *x.shape).contiguous(), True
        key = (B, x.device)
        if key not in self._align_sel:
            self._align_sel[key] = torch.arange(M, dtype=torch.int32, device=x.device).repeat_interleave(B).contiguous()
        return ops.spatial_apply(x, W, sel=self._align_sel[key], out=x if fresh else out)

    def static_buffers(self, x: torch.Tensor) -> dict:
        """The outputs of prepare() for the static windows x [B,T,C] of a hipGraph step: nothing is allocated inside a capture."""
        buf = {}
        if (self.augment is not None or self.prep is not None or self.gate is not None or self.align is not None
                or (self.normalize and self.crop is None)):
            buf["xn"] = torch.empty_like(x)
        if self.gate is not None:                    # the mask words of the signal-quality gate, one per (trial, step)
            buf["gm"] = torch.empty(tuple(x.shape[:-1]), dtype=torch.int32, device=x.device)
        if self.crop is not None:                    # the crops (z-scored in place with normalize) and their labels
            rows, W = self.dims(int(x.shape[0]), int(x.shape[1]))
            buf["xc"] = x = torch.empty((rows, W, x.shape[2]), dtype=torch.float32, device=x.device)
            buf["yc"] = torch.empty((rows,), dtype=torch.int32, device=x.device)
        if self.loss is not None:                    # (a single-model trainer's: self.loss is one Loss)
            buf["tg"] = torch.empty((x.shape[0], self.spec.K), dtype=torch.float32, device=x.device)
            buf["xm"] = torch.empty_like(x) if self.loss.mixup > 0 else None
        return buf

    def prepare(self, x: torch.Tensor, y: torch.Tensor, seeds: Sequence[int], step: int, *, M: int = 1,
                step_dev: Optional[torch.Tensor] = None, bufs: Optional[dict] = None):
        """(windows, labels, targets) of step `step`: exactly one of labels / targets is None.  x [B,T,C] (one model, or shared by M)
        or [M,B,T,C]; y int32 labels [M*B], or float32 target rows that are used as they are; seeds: one per model.
        Launches nsd_augment (with the z-score fused behind it; without augmentation nsd_zscore_fwd, or nothing), then for a model with
        a causal front end nsd_prep_step in window mode (on the augmented windows in place, else into the same buffer), then with loss=
        nsd_mixup on the windows the model would otherwise see (mixup off: it only builds the target rows).  An empty shard launches
        nothing.  step_dev (device step counter, with bufs = the trainer's static buffers): the stream ids come from the counter and
        the outputs go to bufs' xn / xc / yc / xm / tg.
        With crop: nsd_augment (never z-scoring), nsd_prep_step, nsd_crop -- windows [B*R,W,C] per model, labels or float target
        rows repeated per crop -- then with normalize nsd_zscore_fwd on the crops in place, then nsd_mixup as above, on crops."""
        bufs = bufs or {}
        x = x.contiguous().float()
        B, T, Cc = x.shape[-3:]
        if B == 0:
            return (x, None, y) if y.is_floating_point() else (x, y, None)
        drawn_crop = self.crop is not None and self.crop.hop == 0
        if self.augment is not None or self.loss is not None or drawn_crop:
            rngs = [step_rng(s, 0 if step_dev is not None else step) for s in seeds]
        if self.augment is not None:       # a shared [B,T,C] becomes [M,B,T,C], each model with its own draws
            x = ops.augment(x, self.augment, rngs, M=M, zscore=self.normalize and self.crop is None, step_dev=step_dev, out=bufs.get("xn"))
        elif self.normalize and self.crop is None:   # as EEG_LSTM.forward: the model is trained on what it is evaluated on
            x = ops.zscore(x.reshape(-1, T, Cc), out=bufs.get("xn")).view(x.shape)
        mask = None
        if self.gate is not None:          # augment -> gate -> prep -> apply: the detector sees the raw (augmented) samples
            x, mask = ops.gate_step(x, self.gate, out=x if self.augment is not None else bufs.get("xn"), mask=bufs.get("gm"))
        if self.prep is not None:          # augment -> prep -> mixup: the front end sees the raw (augmented) samples, as a stream's does
            x = ops.prep_step(x, self.prep, out=x if (self.augment is not None or mask is not None) else bufs.get("xn"))
        if mask is not None:               # a bad channel is zeroed; inside a training step nothing is rejected (the loss stays finite)
            x = ops.gate_apply(x, self.gate, mask, out=x, max_bad=int(Cc))
        if self.align is not None:         # ... -> apply -> align -> crop: in place in the buffer the front end wrote, or into xn
            x = self.align_apply(x, fresh=self.augment is not None or mask is not None or self.prep is not None, out=bufs.get("xn"))
        if self.crop is not None:          # ... -> prep -> crop -> mixup: the step's dimensions become (B * R, W) here
            self.crop.check_trial(T)
            soft = y.is_floating_point()
            x, yl, yt = ops.crop(x, self.crop, rngs if drawn_crop else None, M=M, labels=None if soft else y, targets=y if soft else None,
                                 step_dev=step_dev if drawn_crop else None, out=bufs.get("xc"), labels_out=bufs.get("yc"))
            y = yt if soft else yl
            if self.normalize:
                ops.zscore(x.view(-1, self.crop.window, Cc), out=x.view(-1, self.crop.window, Cc))
        if y.is_floating_point() or self.loss is None:
            return (x, None, y) if y.is_floating_point() else (x, y, None)
        lo = self.loss
        if isinstance(lo, list):                     # per model: the windows are mixed (or copied) as soon as one model mixes
            smooth, mix = [e.label_smoothing for e in lo], [e.mixup for e in lo]
            mixing = any(v > 0 for v in mix)
        else:
            smooth, mix, mixing = lo.label_smoothing, lo.mixup, lo.mixup > 0
        xm, tg = ops.mixup(x if mixing else None, y, self.spec.K, rngs, M=M, label_smoothing=smooth, mix=mix,
                           class_weights=self.class_weights, step_dev=step_dev, out=bufs.get("xm"), targets=bufs.get("tg"))
        return (xm if mixing else x), None, tg
