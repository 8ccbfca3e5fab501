"""Several H = 48 models per launch: folds, seed sweeps and ensembles (include/nsd.h, nsd_multi_*).

ModelBatchTrainer steps M same-shaped EEG_LSTM models together: one forward, one backward and one reduction + Adam launch for all
of them.  Model m's step is the step `Trainer(model_m, seed=seeds[m])` would take on its batch: the same recipe and random
streams (step_recipe.py, where a step's streams are defined), the same mean cross-entropy over its own B trials, the same Adam
update.  EnsemblePredictor averages the class probabilities of M checkpoints computed in one inference launch, behind
SimplePredictor's surface and preprocessing.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from . import ops
from ._lib import NsdError
from .lstm_eeg_model import EEG_LSTM, SimplePredictor
from .step_recipe import StepRecipe, refuse_resample, trainer_seed


def _check_models(models: Sequence[EEG_LSTM], what: str) -> None:
    M = len(models)
    if M < 1:
        raise NsdError(f"{what}: no models")
    sp = models[0].spec
    if len({id(m) for m in models}) != M:
        raise NsdError(f"{what}: the same module is passed more than once (each model needs its own parameters)")
    for i, mdl in enumerate(models):
        if (mdl.spec != sp or mdl.residual != models[0].residual or mdl.precision != models[0].precision
                or mdl.normalize != models[0].normalize or mdl.prep != models[0].prep or mdl.gate != models[0].gate
                or getattr(mdl, "align", None) != getattr(models[0], "align", None)
                or getattr(mdl, "resample", None) != getattr(models[0], "resample", None)):
            raise NsdError(f"{what}: model {i} has another shape / options than model 0 (mixed shapes: one launch runs one shape)")
    if models[0].residual or models[0].precision != "fp32" or sp.D != 1:
        raise NsdError(f"{what}: the model-batched path runs the plain fp32 stack (no residual extension, no bf16)")
    if not ops.multi_path(sp, M):
        raise NsdError(f"{what}: {M} models of {sp} are outside the model-batched path (nsd_multi_path: H = 48, L = 2, C <= 8, "
                       f"F <= 64, K <= 8, 1 <= M <= 32)")


class ModelBatchTrainer:
    """Trains M same-shaped EEG_LSTM models in the launches one model uses (single GPU).

    The models' parameters are packed into one [M, P] buffer and each model's parameters are re-pointed as views into its row, so
    every model stays an ordinary module (forward, state_dict, save_reference_checkpoint work as before).  step(x, y) takes
    x [M,B,T,C] (per-model windows) or a shared [B,T,C], and y [M,B] or a shared [B].  augment: ops.Augment, applied per model as
    Trainer does.  loss: ops.Loss (label smoothing, class weights, mixup), applied per model as Trainer(model_m, seed=seeds[m], loss=loss)
    does: nsd_augment (if any) -> nsd_mixup -> the step with targets, each one launch for all models; the scale stays 1 / B per model.
    clip_grad_norm / lr_schedule: as Trainer's, the norm taken per model.

    A hyper-parameter grid in one launch: lr, betas, eps, weight_decay, clip_grad_norm, lr_schedule, augment and loss each take a scalar
    or object (one setting for all models, as above) or a sequence of length M, one per model (betas: M pairs); a wrong length raises
    NsdError.  Model m then takes the step a ModelBatchTrainer of the same models and seeds with setting m for everybody would give it,
    bit for bit (nsd_augment_each, nsd_mixup_each, nsd_multi_grad_reduce_clip_adam_each).  Sequences of equal entries, like scalars,
    issue exactly the calls of the single setting.  One model's loss=None beside another model's loss trains on one-hot target rows
    through the soft-target entry point: the hard-label gradient up to the summation order over the classes (the same bits for K <= 3).

    average: an ops.Average, or a sequence of M with None for a model that does not average -- a grid axis like lr.  The update launch
    then also keeps each model's averaged row (weight averaging as Trainer's: the guarded tail is on, nothing is clipped by it, a
    skipped step does not average; no extra launch).  averaged_models() are modules on those rows; evaluate / track_best take
    weights="average" to score -- and snapshot -- the averaged rows instead of the last iterates.

    sam: an ops.Sam, or a sequence of M with None for a model without it -- a grid axis like average.  Sharpness-aware minimisation as
    Trainer's: every step runs forward and backward twice for all models, the ascent of all models (nsd_multi_sam_ascend, each with its
    own rho) between them, then the usual tail; the guarded tail is on.  A model without SAM beside one with it also takes both passes,
    the second on a bitwise copy of its parameters, and is bit for bit the model trained without SAM.  last_sams() reads the records;
    last_losses() are then the second pass's.

    crop: an ops.Crop -- cropped training as Trainer's: every model's trials are cut into crop.crops windows of crop.window samples in one
    launch (each model with its own offsets), the step's kernels see (B * crops, window) and each model's loss is the mean over its
    crops.  One setting for all models: window and crops set the launch dimensions, so a sequence of differing entries is refused.
    evaluate / track_best take crop=ops.Crop(W, R, hop > 0) to score trials by their pooled windows.

    Dropout comes from each model's own dropout_p / head_dropout_p (NSD_FLAG_MODEL_P is passed only where they differ).  This corrects
    earlier behaviour: models with different probabilities were all, silently, trained with model 0's."""

    def __init__(self, models: Sequence[EEG_LSTM], lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0, seeds: Optional[Sequence[int]] = None, stochastic: bool = True, group=None,
                 augment=None, loss=None, clip_grad_norm=None, lr_schedule=None, average=None, sam=None, crop=None):
        import torch.distributed as dist
        self.models: List[EEG_LSTM] = list(models)
        _check_models(self.models, "ModelBatchTrainer")
        refuse_resample(self.models, "ModelBatchTrainer")
        if group is not None or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            raise NsdError("ModelBatchTrainer: world size > 1 is not supported (model batching is single-GPU; use Trainer for data parallel)")
        M = len(self.models)
        self.M, self.spec = M, self.models[0].spec
        dev = self.models[0].flat_parameters().device
        if not self.models[0].flat_parameters().is_cuda:
            raise NsdError("ModelBatchTrainer needs the models on the MI355X (model.to('cuda')); there is no CPU training path")
        P = self.spec.param_count
        self.params = torch.empty((M, P), dtype=torch.float32, device=dev)
        offs = self.spec.offsets()
        with torch.no_grad():
            for i, mdl in enumerate(self.models):
                if mdl.flat_parameters().device != dev:
                    raise NsdError("ModelBatchTrainer: all models must live on one device")
                self.params[i].copy_(mdl.flat_parameters())
                for n, p in mdl._named_in_order():
                    p.data = self.params[i, offs[n]:offs[n] + p.numel()].view(p.shape)
                mdl._flat = self.params[i]
        seeds = list(seeds) if seeds is not None else [1234] * M
        if len(seeds) != M:
            raise NsdError(f"ModelBatchTrainer: {len(seeds)} seeds for {M} models")
        self.seeds = [trainer_seed(s) for s in seeds]      # the streams of model m are those of Trainer(model_m, seed=seeds[m])
        # optimizer settings: one for all models (scalars: today's calls) or one per model (self._each: lists of M)
        per = {"lr": self._per_model(lr, "lr"), "eps": self._per_model(eps, "eps"), "weight_decay": self._per_model(weight_decay, "weight_decay"),
               "betas": self._per_model(betas, "betas", pair=True), "clip_grad_norm": self._per_model(clip_grad_norm, "clip_grad_norm"),
               "lr_schedule": self._per_model(lr_schedule, "lr_schedule")}
        for c in per["clip_grad_norm"]:
            if c is not None and not c >= 0.0:
                raise ValueError(f"ModelBatchTrainer: clip_grad_norm {c!r} negative or NaN")
        self._each = per if any(any(e != v[0] for e in v[1:]) for v in per.values()) else None
        lr, eps, weight_decay, betas, clip_grad_norm, lr_schedule = (per[k][0] for k in ("lr", "eps", "weight_decay", "betas", "clip_grad_norm",
                                                                                           "lr_schedule"))
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay          # (model 0's where they are per model)
        self.stochastic = stochastic
        # Trainer's recipe (step_recipe.py), applied per model with its own seed and dropout, each launch for all models
        self.recipe = StepRecipe(self.models[0], stochastic, augment, loss, dev, models=self.models, sam=self._per_model(sam, "sam"),
                                 crop=crop)
        self.crop = self.recipe.crop
        for mdl in self.models:
            if self.crop is not None and mdl.crop is None:
                mdl.crop = self.crop     # as Trainer: the models and their checkpoints carry the trained window
        self.sam = self.recipe.sam                                               # None: off; one Sam; or a list of M
        self.augment, self.loss = self.recipe.augment, self.recipe.loss
        self.m = torch.zeros_like(self.params)
        self.v = torch.zeros_like(self.params)
        self.grads = torch.zeros_like(self.params)
        # clipping and schedule as in Trainer: one global norm, one record and one skip decision PER MODEL (nsd_multi_grad_reduce_clip_adam)
        self.clip_grad_norm, self.lr_schedule = clip_grad_norm, lr_schedule
        self.average = self._per_model(average, "average")
        for a in self.average:
            if a is not None and not isinstance(a, ops.Average):
                raise ValueError(f"ModelBatchTrainer: average {a!r}: an ops.Average or None")
        self._avg_on = any(a is not None for a in self.average)
        self._opt_on = self._each is not None or clip_grad_norm is not None or lr_schedule is not None or self._avg_on or self.sam is not None
        self._sam_state = ops.sam_state(P, M, dev) if self.sam is not None else None
        self._opt_state = ops.opt_state(P, M, dev) if self._opt_on else None
        self._avg_state = ops.avg_state(P, M, dev) if self._avg_on else None
        self._avg_models = None
        self.step_count = 0
        self._bufs = {}
        self._last = None
        self._bound = None               # bind_batches: the resident trials, the device schedule and the host's count of its steps
        self._sel_buf, self._sel_state, self._sel_rule = None, None, None      # early stopping: allocated by the first track_best

    def _per_model(self, v, name: str, pair: bool = False) -> list:
        """A setting given once or per model -> its M entries (pair: the single setting is itself a pair, per model is M pairs)."""
        seq = isinstance(v, (list, tuple)) and (not pair or (len(v) > 0 and isinstance(v[0], (list, tuple))))
        if not seq:
            return [v] * self.M
        if len(v) != self.M:
            raise NsdError(f"ModelBatchTrainer: {name} has {len(v)} entries for {self.M} models")
        return [tuple(e) for e in v] if pair else list(v)

    def _buffers(self, B: int, T: int):
        key = (B, T)
        if key not in self._bufs:
            dev = self.params.device
            self._bufs = {key: {"ws": ops.multi_workspace(self.spec, self.M, B, T, dev),
                                "logits": torch.empty((self.M * B, self.spec.K), dtype=torch.float32, device=dev)}}
        return self._bufs[key]

    def step(self, x: torch.Tensor, y: torch.Tensor) -> None:
        M = self.M
        if x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[0] != M):
            raise NsdError(f"ModelBatchTrainer.step: x must be [M={M},B,T,C] or [B,T,C], got {tuple(x.shape)}")
        B, T = int(x.shape[-3]), int(x.shape[-2])
        if B == 0:
            raise NsdError("ModelBatchTrainer.step: empty batch")
        B, T = self.recipe.dims(B, T)        # (with crop=: the crops the kernels see)
        if not ops.multi_path(self.spec, M, B, T):
            raise NsdError(f"ModelBatchTrainer.step: T = {T} is outside the model-batched path (nsd_multi_path: T <= 1024)")
        y = y.to(torch.int32)
        Bt = int(x.shape[-3])                # trials
        if y.dim() == 1:
            if y.shape[0] != Bt:
                raise NsdError(f"ModelBatchTrainer.step: y has {y.shape[0]} labels for {Bt} trials")
            y = y.unsqueeze(0).expand(M, Bt)
        if tuple(y.shape) != (M, Bt):
            raise NsdError(f"ModelBatchTrainer.step: y must be [M,B] or [B], got {tuple(y.shape)}")
        self.step_count += 1
        x, y, tg = self.recipe.prepare(x, y.contiguous().view(-1), self.seeds, self.step_count, M=M)
        rngs = self.recipe.rngs(self.seeds, self.step_count)
        buf = self._buffers(B, T)
        ops.multi_train_step(self.spec, self.params, x, y, buf["ws"], self.grads, rngs=rngs, logits=buf["logits"], m=self.m, v=self.v,
                             step=self.step_count, lr=self.lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps,
                             weight_decay=self.weight_decay, targets=tg, opt=self._opt() if self._opt_on else None, opt_state=self._opt_state,
                             avg=self.average if self._avg_on else None, avg_state=self._avg_state, **self.recipe.sam_args(self._sam_state))
        self._last = (B, T)

    def set_alignment(self, W) -> None:
        """The M alignment matrices [M,C,C] of models built with align=SessionAlign(...) (SessionAlign.fit(model, trials, groups) forms
        them, one group per fold): written into the step's table and each model's buffer."""
        self.recipe.set_alignment(W)

    # ---- device-resident batches --------------------------------------------------------------------------------------------------
    def bind_batches(self, trials, schedule) -> None:
        """Keep the trials (a data.DeviceTrialSet with labels) and the M models' index schedule (a data.BatchSchedule, e.g.
        BatchSchedule.for_runs) on the device: step_scheduled() then forms all models' batches of a step in one launch (nsd_gather)
        instead of the host indexing and stacking them.  The first step after binding reads row 0; a schedule of the bound shape is
        copied into the device table in place."""
        if trials.labels is None:
            raise NsdError("ModelBatchTrainer.bind_batches: the model-batched step takes int32 labels; the trial set holds target rows")
        self._bound, _ = StepRecipe.bind(self._bound, trials, schedule, self.M, self.step_count + 1, "ModelBatchTrainer.bind_batches")

    def step_scheduled(self) -> None:
        """One step of all models on the next row of the bound schedule: one nsd_gather into [M,B,T,C] / [M*B], then step() on them.
        Stepping past the schedule's last row raises."""
        who = "ModelBatchTrainer.step_scheduled"
        b = self._bound
        if b is not None and self.step_count + 1 != b["first"] + b["taken"]:
            raise NsdError(f"{who}: other steps were taken since the batches were bound (the row is named by the step count); bind again")
        b = StepRecipe.take(b, who)
        x, y = self.recipe.gather(b, self.step_count + 1)
        self.step(x.view(self.M, b["B"], b["T"], -1), y.view(self.M, b["B"]))

    def _opt(self):
        """nsd_opt of the step: one, or with per-model settings a list of M"""
        if self._each is None:
            return ops.opt_struct(lr=self.lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, weight_decay=self.weight_decay,
                                  max_norm=self.clip_grad_norm, schedule=self.lr_schedule)
        e = self._each
        return [ops.opt_struct(lr=e["lr"][i], beta1=e["betas"][i][0], beta2=e["betas"][i][1], eps=e["eps"][i], weight_decay=e["weight_decay"][i],
                               max_norm=e["clip_grad_norm"][i], schedule=e["lr_schedule"][i]) for i in range(self.M)]

    # ---- weight averaging -------------------------------------------------------------------------------------------------------
    def averaged_params(self) -> torch.Tensor:
        """The averaged rows [M, P], a view of the device buffer the update launch writes.  The row of a model without averaging, or
        before its first averaged step, holds nothing of use (averaged_counts())."""
        if not self._avg_on:
            raise NsdError("ModelBatchTrainer: no weight averaging (pass average=ops.Average(...))")
        return ops.avg_rows(self._avg_state, self.M, self.spec.param_count)

    def averaged_counts(self) -> List[int]:
        """Per model: how many steps its average holds (synchronises)."""
        return [r["n_avg"] for r in ops.avg_records(self._avg_state, self.M)] if self._avg_on else [0] * self.M

    def averaged_models(self) -> List[EEG_LSTM]:
        """One EEG_LSTM (eval mode) per model whose parameters are views of its averaged row; they follow later steps."""
        if self._avg_models is None:
            rows = self.averaged_params()
            self._avg_models = [mdl.view_of(rows[i]) for i, mdl in enumerate(self.models)]
        return self._avg_models

    def _weights(self, weights: str, who: str) -> torch.Tensor:
        if weights not in ("last", "average"):
            raise NsdError(f"ModelBatchTrainer.{who}: weights {weights!r}: 'last' or 'average'")
        return self.params if weights == "last" else self.averaged_params()

    def last_sams(self) -> Optional[List[dict]]:
        """Per model the record of the last ascent (sam=): {norm, scale, nonfinite} as Trainer.last_sam(); None without sam= or before
        a step.  Synchronises."""
        if self.sam is None or self._last is None:
            return None
        return ops.sam_records(self._sam_state, self.M)

    def last_grad_norms(self) -> List[float]:
        """Each model's global gradient norm of the last step, before clipping (synchronises; NaN with both options off or before a step)."""
        if not self._opt_on or self._last is None:
            return [float("nan")] * self.M
        return [r["norm"] for r in ops.opt_records(self._opt_state, self.M)]

    def last_lr(self) -> float:
        """Learning rate of the last update (one lr and schedule for all models; synchronises).  Where the models have their own:
        last_lrs()."""
        if self._each is not None and any(e != v[0] for k in ("lr", "lr_schedule") for v in (self._each[k],) for e in v[1:]):
            raise NsdError("ModelBatchTrainer.last_lr: the models have their own lr / lr_schedule: use last_lrs()")
        return self.last_lrs()[0]

    def last_lrs(self) -> List[float]:
        """Each model's learning rate of the last update (synchronises)."""
        if self._opt_on and self._last is not None:
            return [r["lr"] for r in ops.opt_records(self._opt_state, self.M)]
        opts = self._opt()
        opts = opts if isinstance(opts, list) else [opts] * self.M
        return [float(torch.tensor(float(o.lr) * ops.lr_factor(o, max(self.step_count, 1)), dtype=torch.float32)) for o in opts]

    def skipped_steps(self) -> List[int]:
        """Per model: updates skipped on the device because its gradient norm was not finite (sticky; synchronises)."""
        return [r["skipped"] for r in ops.opt_records(self._opt_state, self.M)] if self._opt_on else [0] * self.M

    def last_losses(self) -> List[float]:
        """Mean loss (CE, or the soft-target loss with loss=) of each model's last step (synchronises)."""
        if self._last is None:
            return [float("nan")] * self.M
        B, T = self._last
        StepRecipe.check_gather(self._bound, "ModelBatchTrainer.last_losses")
        s = ops.multi_loss_sum(self.spec, self._bufs[(B, T)]["ws"], self.M, B, T)
        return [float(v) / B for v in s.cpu().tolist()]

    # ---- held-out metrics and early stopping for all models (nsd_multi_eval of include/nsd.h) --------------------------------------
    # A trainer on which none of these is called allocates nothing for them and issues exactly the calls it issued without them.

    def _held_out(self, x: torch.Tensor, y: torch.Tensor, counts, select, who: str, weights: str = "last", crop=None) -> List[dict]:
        """nsd_multi_infer on the windows (behind the models' front end, as EEG_LSTM.forward), nsd_multi_eval on its logits, ONE read of
        the records: with selection the eval records lie directly in front of the select state in one allocation, so one copy brings
        both kinds.  crop (a regular grid): the trials are cut as a cropped step cuts them (front end, nsd_crop, z-score of the
        crops), nsd_multi_infer decides the B * R windows, nsd_crop_pool pools each trial's R decisions and nsd_multi_eval reads the
        logarithms of the pooled probabilities as its logits: the loss is -log of the pooled probability of the label, the
        prediction the pooled decision, and n, counts and the confusion matrix count TRIALS."""
        if crop is not None and (not isinstance(crop, ops.Crop) or crop.hop < 1):
            raise NsdError(f"ModelBatchTrainer.{who}: crop {crop!r}: an ops.Crop with a regular grid (hop > 0), so that an evaluation "
                           f"draws nothing and is the sliding decoder's")
        M = self.M
        params = self._weights(weights, who)
        if x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[0] != M):
            raise NsdError(f"ModelBatchTrainer.{who}: x must be [M={M},B,T,C] or [B,T,C], got {tuple(x.shape)}")
        B, T, Cc = (int(v) for v in x.shape[-3:])
        if B == 0:
            raise NsdError(f"ModelBatchTrainer.{who}: no windows")
        y = y.to(torch.int32)
        if y.dim() == 1 and y.shape[0] == B:
            y = y.unsqueeze(0).expand(M, B)
        if tuple(y.shape) != (M, B):
            raise NsdError(f"ModelBatchTrainer.{who}: y must be [M,B] = [{M},{B}] or [B], got {tuple(y.shape)}")
        x = x.contiguous().float()
        if self.models[0].prep is not None or self.models[0].gate is not None:
            x = self.recipe.align_apply(self.models[0]._gate_prep(x), fresh=True)
        elif self.recipe.align is not None:
            x = self.recipe.align_apply(x, fresh=False)
        elif self.models[0].normalize and crop is None:
            x = ops.zscore(x.reshape(-1, T, Cc)).view(x.shape)
        if crop is None:
            logits, _ = ops.multi_infer(self.spec, params, x, want_probs=False)
        else:
            crop.check_trial(T)
            x, _, _ = ops.crop(x, crop, M=M if x.dim() == 4 else 1)      # (shared trials are cut once: a regular grid draws nothing)
            if self.models[0].normalize:
                ops.zscore(x.view(-1, crop.window, Cc), out=x.view(-1, crop.window, Cc))
            _, probs = ops.multi_infer(self.spec, params, x)                       # [M, B*R, K]
            _, logits = ops.crop_pool(probs.view(M * B, crop.crops, self.spec.K))
            logits = logits.view(M, B, self.spec.K)
        if select is None:
            return ops.eval_records(ops.multi_eval(logits, y.contiguous(), counts=counts), M, self.spec.K)
        lead = (M * ops.EVAL_RECORD_BYTES + 15) // 16 * 16
        if self._sel_state is None:
            self._sel_buf = torch.empty(lead + ops.select_state_bytes(M, self.spec.param_count), dtype=torch.uint8, device=self.params.device)
            self._sel_state = ops.select_state(M, self.spec.param_count, self.params.device, out=self._sel_buf[lead:])
        ops.multi_eval(logits, y.contiguous(), counts=counts, out=self._sel_buf[:M * ops.EVAL_RECORD_BYTES], select=select, params=params,
                       state=self._sel_state)
        raw = self._sel_buf[:lead + M * ops.SELECT_RECORD_BYTES].cpu()
        recs = ops.eval_records(raw, M, self.spec.K)
        for r, s in zip(recs, ops.select_records(raw[lead:], M)):
            r.update(best_eval=s["best_eval"], bad=s["bad"], stopped=bool(s["stopped"]))
        return recs

    def evaluate(self, x: torch.Tensor, y: torch.Tensor, counts=None, weights: str = "last", crop=None) -> List[dict]:
        """Held-out metrics of all M models in two launches and one read: x [M,B,T,C] (each model's own windows) or a shared [B,T,C], y
        [M,B] or [B] class indices.  counts: None, or M ints -- only model m's first counts[m] windows count, the rest is padding
        (folds differ in size by one; the padding may hold anything).  Returns M dicts: loss (mean cross-entropy, summed in double),
        acc, n, nonfinite (windows whose logits were not finite: they count nowhere else and make the loss NaN) and confusion, a
        [K,K] numpy array indexed [label, prediction].  Synchronises.  weights="average": the metrics of the averaged rows
        (average=) instead of the last iterates.  crop=ops.Crop(W, R, hop > 0): x holds whole trials and every trial is decided by
        the mean of the class probabilities of its R windows (offsets 0, hop, ...: the decisions a sliding decoder with (W, hop) takes
        on it); loss is then -log of the pooled probability of the label, and n, counts and confusion count trials.  A trial with a
        non-finite window is non-finite, and no other."""
        return self._held_out(x, y, counts, None, "evaluate", weights, crop)

    def track_best(self, x: torch.Tensor, y: torch.Tensor, counts=None, metric: str = "loss", patience: int = 0,
                   min_delta: float = 0.0, weights: str = "last", crop=None) -> List[dict]:
        """evaluate(), and in the same launch early stopping per model: is this the model's best evaluation so far (metric "loss": the
        mean loss fell by more than min_delta; "acc": the accuracy rose by more than min_delta, or stayed with a lower loss), if so copy
        its parameter row into a snapshot on the device, else count one more bad evaluation and, with patience > 0, mark the model
        stopped after `patience` of them in a row (patience = 0 tracks the best and never stops).  A non-finite evaluation is a bad
        one.  Returns evaluate()'s dicts extended by best_eval (1-based number of the best evaluation, 0: none yet), bad and stopped.
        One rule per trainer: another metric, patience or min_delta on a later call raises.  weights="average": the averaged rows are
        what is evaluated AND what is snapshotted, so restore_best() puts the best averaged weights into the models.

        A stopped model STILL TRAINS: step() keeps updating its parameters until the caller's loop ends (the step kernels know nothing
        of this).  Its snapshot and its record are frozen, so restore_best() gives what stopping it would have given; all_stopped()
        lets the loop end early.  crop: as evaluate()'s -- the rule then runs on the trial-level (pooled) metrics."""
        if metric not in ("loss", "acc"):
            raise NsdError(f"ModelBatchTrainer.track_best: metric {metric!r}: 'loss' or 'acc'")
        if int(patience) < 0 or not float(min_delta) >= 0.0:
            raise NsdError(f"ModelBatchTrainer.track_best: patience {patience} / min_delta {min_delta}: both >= 0")
        self._weights(weights, "track_best")
        rule = dict(metric=metric, patience=int(patience), min_delta=float(min_delta))
        if self._sel_rule is not None and (rule, weights) != self._sel_rule:
            raise NsdError(f"ModelBatchTrainer.track_best: the rule was {self._sel_rule}, now {(rule, weights)}: one rule per trainer")
        recs = self._held_out(x, y, counts, rule, "track_best", weights, crop)
        self._sel_rule = (rule, weights)
        return recs

    def _select_records(self) -> List[dict]:
        if self._sel_state is None:
            return [dict(best_loss=float("nan"), best_correct=0, best_n=0, best_eval=0, evals=0, bad=0, stopped=0, status=0)] * self.M
        return ops.select_records(self._sel_state, self.M)

    def stopped(self) -> List[bool]:
        """Per model: has track_best marked it stopped (synchronises)."""
        return [bool(r["stopped"]) for r in self._select_records()]

    def all_stopped(self) -> bool:
        return all(self.stopped())

    def best_evals(self) -> List[int]:
        """Per model: the 1-based number of its best track_best call, 0 where it has none yet (synchronises)."""
        return [r["best_eval"] for r in self._select_records()]

    def best_state_dict(self, m: int) -> dict:
        """The state_dict of model m at its best evaluation, from the snapshot (copies; the model itself is not touched)."""
        if self._sel_state is None or self.best_evals()[m] == 0:
            raise NsdError(f"ModelBatchTrainer.best_state_dict: model {m} has no best evaluation yet (call track_best)")
        row = ops.select_snapshot(self._sel_state, self.M, self.spec.param_count)[m]
        offs = self.spec.offsets()
        return {n: row[offs[n]:offs[n] + p.numel()].view(p.shape).clone() for n, p in self.models[m]._named_in_order()}

    def restore_best(self) -> List[int]:
        """Copy the snapshot row of every model that has a best evaluation back into self.params; returns best_evals().  The modules
        stay views of their rows, so state_dict() and save_reference_checkpoint see the restored model.  Adam's m and v rows of a
        restored model are zeroed: training on from a restored model restarts its moments (the snapshot holds parameters only)."""
        best = self.best_evals()
        if self._sel_state is not None:
            snap = ops.select_snapshot(self._sel_state, self.M, self.spec.param_count)
            with torch.no_grad():
                for i, b in enumerate(best):
                    if b > 0:
                        self.params[i].copy_(snap[i])
                        self.m[i].zero_()
                        self.v[i].zero_()
        return best


class _EnsembleModel:
    """What SimplePredictor calls on its model: predict_proba -> the mean of the M models' class probabilities (one launch)."""

    def __init__(self, models: Sequence[EEG_LSTM]):
        _check_models(models, "EnsemblePredictor")
        self.models = list(models)
        self.spec, self.precision, self.normalize, self.prep = models[0].spec, "fp32", models[0].normalize, models[0].prep
        self.gate = models[0].gate
        self.resample = getattr(models[0], "resample", None)
        self.align = getattr(models[0], "align", None)      # (the front end is shared: member 0's matrix is the ensemble's)
        self.params = torch.stack([m.flat_parameters() for m in self.models]).contiguous()

    @property
    def align_matrix(self):
        return self.models[0].align_matrix

    @property
    def align_record(self):
        return self.models[0].align_record

    def set_alignment(self, W, record=None) -> None:
        for m in self.models:
            m.set_alignment(W, record=record)

    def enable_alignment(self, align=None):
        """Every member gains the alignment stage at the identity where it has none (EEG_LSTM.enable_alignment), and so does the shared
        front end: the start of align.EnsembleSpatialFit."""
        for m in self.models:
            m.enable_alignment(align if align is not None else self.models[0].align)
        self.align = self.models[0].align
        return self

    def predict_proba(self, x: torch.Tensor) -> torch.Tensor:
        x = x.contiguous().float()
        x = self.models[0]._front_end(x)
        _, probs = ops.multi_infer(self.spec, self.params, x)
        return probs.mean(0)


class EnsemblePredictor(SimplePredictor):
    """SimplePredictor over M checkpoints of one shape: predict / predict_windows return the mean of the models' class probabilities
    (and its argmax label), computed for all models in one nsd_multi_infer launch on the shared windows.  Arguments are those of
    SimplePredictor, with a list of .pth paths in place of one."""

    def __init__(self, pth_paths: Sequence[str], sr: int, **kw):
        paths = list(pth_paths)
        if not paths:
            raise NsdError("EnsemblePredictor: no checkpoints")
        super().__init__(paths[0], sr, **kw)
        models = [self.model]
        for p in paths[1:]:
            models.append(SimplePredictor(p, sr, **{**kw, "preprocess": "identity"}).model)
        self.members = models
        self.model = _EnsembleModel(models)

    def input_gradient(self, trials, labels, reduce: str = "mean") -> np.ndarray:
        """The ensemble's saliency: dL/dx of the members' mean cross-entropy on `trials` [N,T,C] with `labels` [N] class indices, all
        members in the launches one model uses (ops.multi_train_dx on the shared windows, eval-mode noise; the members are read, never
        written).  reduce="mean" -> [N,T,C], the gradient of (1/M) sum_m mean_n CE_m (the serial fp32 mean over the members,
        align.mean_over_models); "per_model" -> [M,N,T,C].  The gradient is with respect to what the LSTM is fed, behind the z-score or
        the alignment matrix where the members have one; members with a signal-quality gate or a causal front end are refused, as
        EEG_LSTM.forward refuses x.requires_grad through them."""
        em = self.model
        if em.gate is not None or em.prep is not None or em.resample is not None:
            raise NsdError("EnsemblePredictor.input_gradient: dx through the rate conversion / the signal-quality gate / the causal front end is not offered; "
                           "differentiate gate- and prep-free members on the front end's output (ops.gate_step, ops.prep_step)")
        x = torch.as_tensor(np.asarray(trials, dtype=np.float32)).to(self.gpu).contiguous()
        sp, M = em.spec, len(em.models)
        if x.dim() != 3 or x.shape[-1] != sp.C or x.shape[0] < 1:
            raise ValueError(f"EnsemblePredictor.input_gradient: trials must be [N >= 1, T, {sp.C}], got {tuple(x.shape)}")
        N, T = int(x.shape[0]), int(x.shape[1])
        y = torch.as_tensor(np.asarray(labels).astype(np.int32).reshape(-1)).to(self.gpu)
        if int(y.numel()) != N:
            raise ValueError(f"EnsemblePredictor.input_gradient: {int(y.numel())} labels for {N} trials")
        with torch.no_grad():
            x = em.models[0]._front_end(x)
            x = x.contiguous()
            ws = ops.multi_workspace(sp, M, N, T, x.device)
            logits = torch.empty((M * N, sp.K), dtype=torch.float32, device=x.device)
            dx = torch.empty((N, T, sp.C) if reduce == "mean" else (M, N, T, sp.C), dtype=torch.float32, device=x.device)
            ops.multi_train_dx(sp, em.params, x, ws, logits, dx, labels=y.repeat(M).contiguous(), reduce=reduce)
        return dx.cpu().numpy()
