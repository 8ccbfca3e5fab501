"""Training loop for EEG_LSTM on MI355X: fused step through the C ABI + data-parallel gradient all-reduce.

The reference's training notebook (DeepLearning/lstm_trainer.ipynb) is not part of the reference tree
(.MISSING_LARGE_BLOBS:1), so this trainer defines the step itself:
    zero_grad -> CE(model(x), y) -> backward -> Adam(lr=1e-3)
with the reference model's train-mode stochastic parts (inter-layer dropout p, RReLU noise, head dropout p).

Per step and per GPU the stream sees, for the reference model's shape, three launches: LSTM forward + attention
pooling + head + CE + head backward (nsd_lstm_head_train_rng, the dropout / RReLU streams drawn in the kernel), BPTT
(nsd_lstm_bwd_rng), slab reduction + Adam (nsd_grad_reduce_adam); with more than one rank the last becomes
nsd_grad_reduce -> ONE all-reduce of the flat fp32 gradient over RCCL -> nsd_adam_step.  Other shapes run the unfused
equivalents (ops.train_step_grads).  With clip_grad_norm= / lr_schedule= the last launch becomes nsd_grad_reduce_clip_adam (one rank) or
nsd_grad_norm + nsd_adam_step_clip behind the all-reduce: global-norm clipping and the schedule are evaluated by the update kernel
(DESIGN.md 4.4).  Nothing synchronises the host.  What the kernels see of (windows, labels, seed, step) and the
step's four random-stream slots are defined in one place, step_recipe.py, for this trainer's eager and hipGraph steps and ModelBatchTrainer.

Data parallelism: trials are independent, so the global batch is split contiguously over ranks
(shard_range; shards may differ by one trial and may be EMPTY); every rank scales its CE gradient by 1/B_global, the flat
gradient vector (31 764 floats = 127 KB for the reference model) is summed with ONE all-reduce, and every rank applies
the same Adam update.  Every rank enters the collective in every step -- a rank without trials contributes a zero
gradient -- and the parameters are broadcast from rank 0 once at construction, so identical replicas do not rest on
identical seeding.
"""
from __future__ import annotations

import math
import os
from typing import Optional, Tuple

import torch
import torch.distributed as dist

from . import ops
from .lstm_eeg_model import EEG_LSTM
from .step_recipe import StepRecipe, base_stream, refuse_resample, trainer_seed


def shard_range(n: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous shard [lo, hi) of n trials for `rank`; sizes differ by at most one."""
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


class FlatGradAllReducer:
    """Sum one flat gradient vector over the data-parallel group with a single collective.
    backend 'nccl' is RCCL over xGMI on ROCm; 'gloo' is used by the CPU tests."""

    def __init__(self, group=None):
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1

    def __call__(self, flat_grad: torch.Tensor) -> torch.Tensor:
        if self.world > 1:
            dist.all_reduce(flat_grad, op=dist.ReduceOp.SUM, group=self.group)
        return flat_grad


def _on_own_device(method):
    """Run a Trainer method with the trainer's GPU as the current device (the C ABI enqueues on the current device)."""
    import functools

    @functools.wraps(method)
    def wrapped(self, *a, **kw):
        with torch.cuda.device(self.flat.device):
            return method(self, *a, **kw)
    return wrapped


class DataParallelStep:
    """The rank-level control flow of one optimisation step, separated from how the numbers are produced so that the
    CPU tests (gloo, world_size 2 and 3, uneven and empty shards) drive exactly this code with an injected gradient
    function.  `local_grads(x, y, scale)` must leave this rank's share of the gradient of sum_b CE_b * scale in the
    flat buffer `grads`; `zero_grads()` clears it; `apply_update()` consumes it."""

    def __init__(self, grads: torch.Tensor, reducer: FlatGradAllReducer, local_grads, zero_grads, apply_update):
        self.grads, self.reducer = grads, reducer
        self.local_grads, self.zero_grads, self.apply_update = local_grads, zero_grads, apply_update

    def __call__(self, x, y, global_batch: int) -> None:
        if global_batch < 1:
            raise ValueError("global_batch must be >= 1 (the number of trials of the step over all ranks)")
        if int(x.shape[0]) > 0:
            self.local_grads(x, y, 1.0 / float(global_batch))
        else:
            self.zero_grads()              # empty shard: still take part in the collective, with a zero gradient
        self.reducer(self.grads)           # EVERY rank, EVERY step
        self.apply_update()


def broadcast_parameters(flat: torch.Tensor, group=None, src: int = 0) -> None:
    """Make every replica start from rank `src`'s parameters (one collective on the flat vector)."""
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.broadcast(flat, src=src, group=group)


class Trainer:
    average: Optional[ops.Average] = None        # weight averaging is off unless __init__ turns it on
    _avg_state: Optional[torch.Tensor] = None
    sam: Optional[ops.Sam] = None                # so is sharpness-aware minimisation
    _sam_state: Optional[torch.Tensor] = None

    def __init__(self, model: EEG_LSTM, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, seed: int = 1234, stochastic: bool = True, group=None,
                 augment: Optional[ops.Augment] = None, loss: Optional[ops.Loss] = None,
                 clip_grad_norm: Optional[float] = None, lr_schedule: Optional[ops.LrSchedule] = None,
                 average: Optional[ops.Average] = None, sam: Optional[ops.Sam] = None, crop: Optional[ops.Crop] = None):
        """crop: an ops.Crop -- cropped training: every trial of a step is shown to the model as crop.crops windows of crop.window
        samples, cut on the device behind the front end (StepRecipe: augment -> prep -> crop -> mixup).  The step's kernels, workspaces,
        captured graphs and path checks then see (B * crops, window); the loss scale is 1 / (global_batch * crops), and last_loss() is
        the mean over the crops.  World > 1: each rank draws its own offsets (trainer_seed), as it augments.  None: today's step.
        sam: an ops.Sam -- sharpness-aware minimisation: every step runs its forward/backward twice on the same batch with the same
        random draws, at the parameters and at the parameters moved rho uphill along the normalised gradient (formed on the device,
        nsd_sam_ascend), and updates the real parameters with the second gradient; about twice the step's time.  It switches the guarded
        tail on, as average= does: a non-finite second gradient is skipped and counted in skipped_steps().  World > 1: each rank ascends
        along its own shard's gradient (no extra collective; the paper's per-replica form).  last_sam() reads the ascent's record.
        average: an ops.Average -- the update launch also keeps an exponential moving average or a running mean (SWA) of the
        parameters (averaged_model()); no extra launch.  Averaging switches the guarded tail on, as clip_grad_norm=0.0 does: it does
        not clip, and a step whose gradient norm is not finite is skipped and counted (skipped_steps()); a skipped step does not
        average.  World > 1: every rank averages its identical replica, with no communication.  None: today's calls, launch for launch."""
        refuse_resample([model], "Trainer")
        self.model = model
        self.spec = model.spec
        self.flat = model.flat_parameters()
        if not self.flat.is_cuda:
            raise ops.NsdError("Trainer needs the model on the MI355X (model.to('cuda')); there is no CPU training path")
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.m = torch.zeros_like(self.flat)
        self.v = torch.zeros_like(self.flat)
        # global-norm clipping (clip_grad_norm: the threshold; 0.0: report the norm and skip non-finite steps without clipping) and the
        # learning-rate schedule, both evaluated by the update kernel (nsd_opt, include/nsd.h).  Both None: the plain step, launch for launch.
        if clip_grad_norm is not None and not clip_grad_norm >= 0.0:
            raise ValueError(f"Trainer: clip_grad_norm {clip_grad_norm!r} negative or NaN")
        self.clip_grad_norm, self.lr_schedule = clip_grad_norm, lr_schedule
        if average is not None and not isinstance(average, ops.Average):
            raise ValueError(f"Trainer: average {average!r}: an ops.Average or None")
        self.average = average
        if sam is not None and not isinstance(sam, ops.Sam):
            raise ValueError(f"Trainer: sam {sam!r}: an ops.Sam or None")
        self.sam = sam
        self._opt_on = clip_grad_norm is not None or lr_schedule is not None or average is not None or sam is not None
        self._sam_state = ops.sam_state(self.flat.numel(), 1, self.flat.device) if sam is not None else None
        self._opt_state = ops.opt_state(self.flat.numel(), 1, self.flat.device) if self._opt_on else None
        self._avg_state = ops.avg_state(self.flat.numel(), 1, self.flat.device) if average is not None else None
        self._avg_model = None
        # the flat gradient with ONE extra element behind it: the bf16 path's failure flag (ops.seq_guard).  The whole buffer is
        # what the ranks all-reduce, so a scan time-out on ANY rank makes EVERY rank skip the update (guarded Adam) -- still
        # one collective per step.  Always 0 on the fp32 path.
        self._grads_ext = torch.zeros(self.flat.numel() + 1, dtype=torch.float32, device=self.flat.device)
        self.grads = self._grads_ext[:self.flat.numel()]
        self._skip = self._grads_ext[self.flat.numel():]
        self.reducer = FlatGradAllReducer(group)
        self.rank = dist.get_rank(group) if self.reducer.world > 1 else 0
        self.world = self.reducer.world
        broadcast_parameters(self.flat, group)     # identical replicas by construction, not by seeding
        self.fused_head = True           # nsd_lstm_head_train (one launch) where the shape allows; False: two launches
        self.in_kernel_rng = True        # dropout / RReLU streams generated inside the kernels where the shape allows
        self.seed = trainer_seed(seed, self.rank)
        self.stochastic = stochastic
        # what a step does to (windows, labels) before its kernels: step_recipe.py, shared with step_static and ModelBatchTrainer.
        # Each rank augments / mixes inside its own shard with its own seed; the scale stays 1 / global_batch (torch's weighted
        # `mean` divides by the weight sum).
        self.recipe = StepRecipe(model, stochastic, augment, loss, self.flat.device, sam=sam, crop=crop)
        self.augment, self.loss = self.recipe.augment, self.recipe.loss          # the effective ones (None: off)
        self.crop = self.recipe.crop
        self._crops = self.crop.crops if self.crop is not None else 1            # rows of a step per trial
        if self.crop is not None and model.crop is None:
            model.crop = self.crop       # the model and its checkpoints carry the window it is trained on (predict_trials, open_stream)
        self.step_count = 0
        self._bufs = {}
        self._loss = torch.zeros(1, dtype=torch.float32, device=self.flat.device)
        self._last_B = 0
        self._carried_failure = ""       # bf16 path, world > 1: message of a time-out found in a workspace that was replaced
        # hipGraph replay of the step (static-input path): everything that varies per step lives on the device
        self._step_dev = torch.zeros(1, dtype=torch.int64, device=self.flat.device)
        self._graphs = {}
        self._bound = None               # bind_batches: the resident trials, the device schedule and the host's count of its steps

    # buffers that depend on the batch shape are created once and reused every step.  (B, T): what the step's kernels see -- with
    # crop= the crops (recipe.dims), not the trials
    def _buffers(self, B: int, T: int):
        key = (B, T)
        if key not in self._bufs:
            sp, dev = self.spec, self.flat.device
            buf = {"ws": ops.new_workspace(sp, B, T, dev),
                   "logits": torch.empty((B, sp.K), dtype=torch.float32, device=dev), "rng_ok": ops.rng_path(sp, B, T)}
            if self.stochastic:
                if self.model.dropout_p > 0 and sp.L > 1:
                    buf["drop_lstm"] = torch.empty((sp.L - 1, B, T, sp.H), dtype=torch.float32, device=dev)
                buf["rrelu"] = torch.empty((B, sp.F), dtype=torch.float32, device=dev)
                if self.model.head_dropout_p > 0:
                    buf["drop_head"] = torch.empty((B, sp.F), dtype=torch.float32, device=dev)
            self._bufs = {key: buf}      # keep only the current shape (workspaces are large)
        return self._bufs[key]

    @_on_own_device
    def step(self, x: torch.Tensor, y: torch.Tensor, global_batch: Optional[int] = None) -> None:
        """One optimisation step on this rank's shard: x [B,T,C] fp32, y [B] int32 (device tensors).  `global_batch`: trials
        of this step over ALL ranks (default B * world, i.e. equal shards); the CE gradient is scaled by 1/global_batch so
        that the all-reduced sum is the global mean whatever the shard sizes.  B may be 0 when world > 1.
        y may also be a float32 [B,K] tensor: the trials' target rows, used as they are (distillation, sample weights; loss_b =
        - sum_k y[b,k] log softmax_k) -- an error together with an enabled loss=, which builds the targets from labels."""
        B = int(x.shape[0])
        if y.is_floating_point():
            if self.loss is not None:
                raise ops.NsdError("Trainer.step: float targets together with loss=: the trainer's Loss builds the targets from int32 labels")
            if y.dtype != torch.float32 or tuple(y.shape) != (B, self.spec.K):
                raise ops.NsdError(f"Trainer.step: float targets must be float32 [B,K] = [{B},{self.spec.K}], got {y.dtype} {tuple(y.shape)}")
            y = y.contiguous()
        if global_batch is None:
            global_batch = B * self.world
        global_batch *= self._crops      # the step's rows over all ranks: with crop= every trial is crops windows
        self.step_count += 1
        if self.world == 1:
            if B == 0:
                raise ops.NsdError("Trainer.step: empty batch")
            # no exchange step between reduction and update: one launch does both
            self._local_grads(x, y, 1.0 / float(global_batch), fuse_adam=True)
        else:
            DataParallelStep(self._grads_ext, self.reducer, self._local_grads, self._grads_ext.zero_, self._adam)(x, y, global_batch)
        if B > 0:
            self._last_B, self._last_T = self.recipe.dims(B, int(x.shape[1]))

    def _hyper(self) -> dict:
        return dict(step=self.step_count, lr=self.lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps,
                    weight_decay=self.weight_decay)

    def _opt(self):
        """nsd_opt of this trainer (clipping / schedule on)"""
        return ops.opt_struct(lr=self.lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, weight_decay=self.weight_decay,
                              max_norm=self.clip_grad_norm, schedule=self.lr_schedule)

    def _fused_tail(self, step_dev: Optional[torch.Tensor] = None) -> dict:
        """adam= of ops.train_step_grads: the update in the reduction's tail (with clipping / a schedule: nsd_grad_reduce_clip_adam)"""
        if not self._opt_on:
            return dict(m=self.m, v=self.v, **self._hyper())
        return dict(m=self.m, v=self.v, opt=self._opt(), opt_state=self._opt_state, step=self.step_count, step_dev=step_dev,
                    avg=self.average, avg_state=self._avg_state)

    def _adam(self, step_dev: Optional[torch.Tensor] = None) -> None:
        # bf16 path: skipped on the device when any rank's scan timed out (self._skip, summed over ranks by the all-reduce)
        skip = self._skip if self.model.precision == "bf16" else None
        if self._opt_on:
            # flat route: every rank forms the norm of the same all-reduced bits, hence the same coef
            opt = self._opt()
            ops.grad_norm(self.grads, self._opt_state, opt.grad_scale)
            if self.average is not None:
                ops.adam_step_clip_avg(self.flat, self.grads, self.m, self.v, opt, self._opt_state, self.average, self._avg_state,
                                       step=self.step_count, step_dev=step_dev, skip=skip)
                return
            ops.adam_step_clip(self.flat, self.grads, self.m, self.v, opt, self._opt_state, step=self.step_count, step_dev=step_dev, skip=skip)
            return
        ops.adam_step(self.flat, self.grads, self.m, self.v, skip=skip, step_dev=step_dev, **self._hyper())

    def _masks(self, buf: dict, step_dev: Optional[torch.Tensor] = None):
        """Fill the step's explicit mask tensors (those the model needs) from its streams -> (drop_lstm, rrelu, drop_head)."""
        masks = (buf.get("drop_lstm"), buf.get("rrelu"), buf.get("drop_head"))
        stream = base_stream(self.step_count) if step_dev is None else step_dev      # graph step: the device counter alone
        ops.train_masks(self.seed, stream, self.recipe.p_lstm, self.recipe.p_head, *masks)
        return masks

    def _local_grads(self, x: torch.Tensor, y: torch.Tensor, scale: float, fuse_adam: bool = False) -> None:
        """Launches that leave this shard's gradient (scaled) in self.grads; fuse_adam: the update rides in the last one."""
        sp = self.spec
        x, y, tg = self.recipe.prepare(x, y, [self.seed], self.step_count)
        B, T, _ = x.shape                # (with crop=: the crops)
        rng = self.recipe.rng(self.seed, self.step_count)
        if self.model.precision == "bf16":
            # sequence-batched path: forward (+ head, CE, head backward), backward (+ all parameter gradients), Adam
            key = ("seq", B, T)
            if key not in self._bufs:
                # a reported time-out must not vanish with the buffer.  One rank: raise here.  Several ranks: raising on this rank
                # alone would leave the others waiting in the step's all-reduce, so the old status is carried into the failure
                # flag that rides that all-reduce (below) and every rank raises in check().
                if self.world == 1:
                    self._check_old_workspaces("Trainer.step")
                else:
                    try:
                        self._check_old_workspaces("Trainer.step")
                    except ops.NsdError as e:
                        self._carried_failure = str(e)
                self._bufs = {key: {"ws": ops.seq_workspace(sp, B, T, self.flat.device),
                                    "logits": torch.empty((B, sp.K), dtype=torch.float32, device=self.flat.device)}}
            buf = self._bufs[key]
            def forward_backward(params):
                ops.seq_train_fwd(sp, params, x, y, buf["ws"], rng=rng, scale=scale, logits=buf["logits"], targets=tg)
                ops.seq_train_bwd(sp, params, buf["ws"], B, T, rng=rng, grads=self.grads)

            # (with sam=: twice, the flat ascent between them -- StepRecipe.passes; an empty shard takes the one pass it takes today)
            self.recipe.passes(self.flat, self._sam_state if B > 0 else None, forward_backward,
                               lambda: ops.sam_ascend_flat(self.flat, self.grads, self.sam, self._opt_state, self._sam_state))
            ops.seq_guard(buf["ws"], self._skip)
            if self._carried_failure:                          # (seq_guard overwrites the flag with this workspace's status)
                self._skip.add_(1.0)
            if fuse_adam:
                self._adam()
            return
        buf = self._buffers(B, T)
        if self.in_kernel_rng and buf["rng_ok"] and all(k in buf for k in ("drop_lstm", "rrelu", "drop_head")):
            dl = sl = dh = None        # the three streams of the step are generated inside the LSTM kernels (same values as nsd_train_masks)
        else:
            (dl, sl, dh), rng = self._masks(buf), None
        ops.train_step_grads(sp, self.flat, x, buf["ws"], y, buf["logits"], self.grads, scale=scale, drop_lstm=dl,
                             rrelu_slope=sl, drop_head=dh, residual=self.model.residual, fused_head=self.fused_head, rng=rng,
                             adam=self._fused_tail() if fuse_adam else None, targets=tg, opt_state=self._opt_state,
                             **self.recipe.sam_args(self._sam_state))

    # ---- hipGraph path ------------------------------------------------------------------------------------
    def static_inputs(self, B: int, T: int):
        """(x [B,T,C] fp32, y [B] int32) device buffers owned by the trainer.  Fill them in place (copy_, index_select
        with out=...) and call step_static(B, T): the whole step is then ONE hipGraph replay per segment instead of
        seven launches, with no host-side argument that changes from step to step."""
        if self.model.precision == "bf16":
            raise ops.NsdError("Trainer.static_inputs / step_static (hipGraph replay) exist for the fp32 path only; "
                               "precision='bf16' trains through Trainer.step")
        buf = self._buffers(*self.recipe.dims(B, T))
        if "x" in buf and tuple(buf["x"].shape[:2]) != (B, T):     # (crop=: other trials with the same crops)
            self._bufs, self._graphs = {}, {}
            buf = self._buffers(*self.recipe.dims(B, T))
        if "x" not in buf:
            dev = self.flat.device
            buf["x"] = torch.zeros((B, T, self.spec.C), dtype=torch.float32, device=dev)
            buf["y"] = torch.zeros((B,), dtype=torch.int32, device=dev)
            buf.update(self.recipe.static_buffers(buf["x"]))       # xn / xm / tg: what the step makes of x and y
        return buf["x"], buf["y"]

    def _issue_segment_a(self, B: int, T: int, scheduled: bool = False) -> None:
        """step counter, random streams, lstm fwd, fused head, lstm bwd, slab reduce -> self.grads (one rank with clipping / a schedule:
        the clipped tail rides here as in the eager step, reading the device counter, and segment B is empty).  scheduled: the gather
        of the bound batches fills the static inputs right behind the counter, reading its row from it."""
        buf = self._buffers(*self.recipe.dims(B, T))
        ops.step_counter_inc(self._step_dev)
        if scheduled:
            self.recipe.gather(self._bound, 0, step_dev=self._step_dev, x=buf["x"], y=buf["y"])
        if self.stochastic and not all(k in buf for k in ("drop_lstm", "rrelu", "drop_head")):
            raise ops.NsdError("graph step needs all three random streams (dropout > 0, num_layers > 1) or stochastic=False")
        dl, sl, dh = self._masks(buf, step_dev=self._step_dev)
        # static buffers throughout, and every stream id from the device step counter: the graph replays it
        xin, y, tg = self.recipe.prepare(buf["x"], buf["y"], [self.seed], 0, step_dev=self._step_dev, bufs=buf)
        ops.train_step_grads(self.spec, self.flat, xin, buf["ws"], y, buf["logits"], self.grads,
                             scale=1.0 / (B * self._crops * self.world), drop_lstm=dl, rrelu_slope=sl, drop_head=dh,
                             residual=self.model.residual,
                             adam=self._fused_tail(self._step_dev) if self._opt_on and self.world == 1 else None, targets=tg,
                             opt_state=self._opt_state, **self.recipe.sam_args(self._sam_state))

    def _issue_segment_b(self) -> None:
        if not (self._opt_on and self.world == 1):
            self._adam(step_dev=self._step_dev)

    @_on_own_device
    def step_static(self, B: int, T: int) -> None:
        """One optimisation step on the trainer's static input buffers, replayed from captured hipGraphs.
        world == 1: one graph.  world > 1: graph A, the eager RCCL all-reduce of the flat gradient, graph B (Adam)."""
        self._replay_static(B, T, False)

    def _replay_static(self, B: int, T: int, scheduled: bool) -> None:
        """step_static, or with scheduled the same graph with nsd_gather of the bound batches as its first node behind the counter"""
        key = ("scheduled", B, T) if scheduled else (B, T)
        if self.model.precision == "bf16":
            raise ops.NsdError("Trainer.step_static (hipGraph replay) exists for the fp32 path only; precision='bf16' trains "
                               "through Trainer.step")
        if key not in self._graphs:
            self.static_inputs(B, T)
            self._step_dev.fill_(self.step_count)
            # warm up eagerly on a side stream (lazy module loading, hipFuncSetAttribute), then capture
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                snap = (self.flat.clone(), self.m.clone(), self.v.clone())
                avg_snap = self._avg_state.clone() if self._avg_state is not None else None
                self._issue_segment_a(B, T, scheduled)
                self._issue_segment_b()
                self.flat.copy_(snap[0]); self.m.copy_(snap[1]); self.v.copy_(snap[2])     # the warm-up step does not count
                if avg_snap is not None:
                    self._avg_state.copy_(avg_snap)
                self._step_dev.fill_(self.step_count)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            ga = torch.cuda.CUDAGraph()
            with torch.cuda.graph(ga):
                self._issue_segment_a(B, T, scheduled)
                if self.world == 1:
                    self._issue_segment_b()
            gb = None
            if self.world > 1:
                gb = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gb):
                    self._issue_segment_b()
            self._graphs = {key: (ga, gb)}
        ga, gb = self._graphs[key]
        self.step_count += 1
        ga.replay()
        if gb is not None:
            self.reducer(self.grads)
            gb.replay()
        self._last_B, self._last_T = self.recipe.dims(B, T)

    # ---- device-resident batches ------------------------------------------------------------------------------------------
    @_on_own_device
    def bind_batches(self, trials, schedule) -> None:
        """Keep the run's trials (a data.DeviceTrialSet) and index schedule (a data.BatchSchedule of one model) on the device:
        step_scheduled() then forms every step's batch there (nsd_gather, the first stage of the step) instead of the host indexing
        it.  The first step after binding reads row 0.  A schedule of the bound shape on the bound trials is copied into the device
        table in place, so the captured graphs of step_scheduled(static=True) survive; another shape drops them.  One rank only."""
        if self.world > 1:
            raise ops.NsdError("Trainer.bind_batches: world size > 1 is not supported (a sharded schedule is a separate piece of work); "
                               "feed the shards through Trainer.step")
        self._bound, kept = StepRecipe.bind(self._bound, trials, schedule, 1, self.step_count + 1, "Trainer.bind_batches")
        if not kept:
            self._graphs = {k: g for k, g in self._graphs.items() if k[0] != "scheduled"}

    @_on_own_device
    def step_scheduled(self, static: bool = False) -> None:
        """One optimisation step on the next row of the bound schedule.  Eager: nsd_gather, then step() on the gathered buffers.
        static=True (fp32 path, int32 labels): one hipGraph replay -- step_static's graph with the gather as its first node behind the
        step counter, which names the row; precision='bf16' takes the eager route.  Stepping past the schedule's last row raises."""
        who = "Trainer.step_scheduled"
        b = self._bound
        if b is not None and self.step_count + 1 != b["first"] + b["taken"]:
            raise ops.NsdError(f"{who}: other steps were taken since the batches were bound (the row is named by the step count); bind again")
        b = StepRecipe.take(b, who)
        if static and self.model.precision != "bf16":
            if b["trials"].labels is None:
                raise ops.NsdError(f"{who}: the static inputs hold int32 labels; a trial set of target rows steps with static=False")
            self._replay_static(b["B"], b["T"], True)
            return
        x, y = self.recipe.gather(b, self.step_count + 1)
        self.step(x, y)

    @_on_own_device
    def scan_status(self) -> int:
        """precision='bf16' only: 0 unless a scan group timed out in any step on the current workspace (the status is sticky:
        nsd_seq_status).  Synchronises."""
        for key, buf in self._bufs.items():
            if key[0] == "seq":
                return ops.seq_status(buf["ws"])
        return 0

    def _check_old_workspaces(self, what: str) -> None:
        for key, buf in self._bufs.items():
            if key[0] == "seq":
                ops.seq_raise_on_timeout(buf["ws"], what, nonfinite=True)

    @_on_own_device
    def check(self) -> None:
        """Raise NsdError if a scan group of the bf16 path timed out on ANY rank since the workspaces were created
        (synchronises this rank's stream; no collective: the flag read here was summed over the ranks by the step's own
        all-reduce, so every rank raises in the same step).  nsd_amd.train calls it on every rank at every log interval."""
        StepRecipe.check_gather(self._bound, "Trainer")
        if self.model.precision != "bf16":
            return
        if float(self._skip.item()) != 0.0:
            if self._carried_failure:
                raise ops.NsdError(self._carried_failure)
            self._check_old_workspaces("Trainer")              # this rank's own status, with the stage in the message
            raise ops.NsdError("Trainer: a scan group of the sequence-batched path timed out, or met non-finite activations, on another "
                               "rank; every rank has skipped the guarded Adam update of that step (and, after a time-out, of every "
                               "step since).  Results are invalid")
        self._check_old_workspaces("Trainer")

    @_on_own_device
    def last_loss(self) -> float:
        """Mean loss of this rank's shard in the most recent step: CE on the labels or, with loss= / float targets, the soft-target
        loss sum_b loss_b / B (synchronises).  With sam= this is the loss of the step's SECOND pass, at the perturbed weights."""
        if not self._last_B:
            return float("nan")
        StepRecipe.check_gather(self._bound, "Trainer.last_loss")
        if self.model.precision == "bf16":
            ws = self._bufs[("seq", self._last_B, self._last_T)]["ws"]
            ops.seq_loss_sum(self.spec, ws, self._last_B, self._last_T, out=self._loss)
            loss = float(self._loss.item()) / self._last_B
            if loss != loss:                                   # NaN: the head poisons its outputs when a scan timed out
                ops.seq_raise_on_timeout(ws, "Trainer.last_loss")
            return loss
        ws = self._buffers(self._last_B, self._last_T)["ws"]
        ops.loss_sum(self.spec, ws, self._last_B, self._last_T, out=self._loss)
        return float(self._loss.item()) / self._last_B

    # ---- clipping / schedule readouts (all synchronise) ---------------------------------------------------------------
    def _record(self) -> Optional[dict]:
        """The device record of the last clipped / scheduled update; None with both options off or before the first step."""
        if not self._opt_on or not self._last_B:
            return None
        with torch.cuda.device(self.flat.device):
            return ops.opt_records(self._opt_state)[0]

    def last_grad_norm(self) -> float:
        """Global L2 norm of the last step's gradient before clipping (NaN with clip_grad_norm / lr_schedule off, or before a step)."""
        rec = self._record()
        return float("nan") if rec is None else rec["norm"]

    def last_lr(self) -> float:
        """Learning rate of the last update, as the kernel formed it; before the first step or with both options off, lr * f(step)
        from the host."""
        rec = self._record()
        if rec is not None:
            return rec["lr"]
        opt = self._opt()
        return float(torch.tensor(float(opt.lr) * ops.lr_factor(opt, max(self.step_count, 1)), dtype=torch.float32))

    def skipped_steps(self) -> int:
        """Updates skipped on the device because the gradient norm was not finite (sticky; 0 with both options off)."""
        return ops.opt_records(self._opt_state)[0]["skipped"] if self._opt_on else 0

    def last_sam(self) -> Optional[dict]:
        """The record of the last ascent (sam=): {norm: the first pass's gradient norm, scale: rho / (norm + 1e-12) as the kernel formed
        it, nonfinite: ascents whose norm was not finite (sticky; the row was then a copy of the parameters)}.  None without sam= or
        before a step.  Synchronises."""
        if self.sam is None or not self._last_B:
            return None
        with torch.cuda.device(self.flat.device):
            return ops.sam_records(self._sam_state)[0]

    # ---- weight averaging ----------------------------------------------------------------------------------------------
    def averaged_weights(self) -> torch.Tensor:
        """The averaged parameter row, a flat fp32 view of the device buffer the update launch writes (it follows later steps)."""
        if self.average is None:
            raise ops.NsdError("Trainer: no weight averaging (pass average=ops.Average(...))")
        return ops.avg_rows(self._avg_state, 1, self.flat.numel())[0]

    def averaged_count(self) -> int:
        """How many steps the average holds (n_avg; synchronises).  0: no step has averaged yet and the row holds nothing of use."""
        return ops.avg_records(self._avg_state)[0]["n_avg"] if self.average is not None else 0

    def averaged_model(self) -> EEG_LSTM:
        """An EEG_LSTM (eval mode) whose parameters are views of the averaged row: forward, state_dict, save_reference_checkpoint and
        SimplePredictor-style consumers work on it, and it follows later steps.  Before the first averaged step its weights are
        whatever the row held (zeros from the allocation): see averaged_count()."""
        if self._avg_model is None:
            self._avg_model = self.model.view_of(self.averaged_weights())
        return self._avg_model

    def state_dict(self):
        sd = {"model": {k: v.detach().cpu() for k, v in self.model.state_dict().items()},
              "adam_m": self.m.cpu(), "adam_v": self.v.cpu(), "step": self.step_count, "skipped": self.skipped_steps()}
        if self.average is not None:
            sd["avg_row"], sd["avg_n"] = self.averaged_weights().cpu(), self.averaged_count()
        return sd

    def load_state_dict(self, sd):
        self.model.load_state_dict(sd["model"], strict=True)
        self.flat = self.model.flat_parameters()
        self.m.copy_(sd["adam_m"]); self.v.copy_(sd["adam_v"]); self.step_count = int(sd["step"])
        # the schedule resumes with the step (f depends on it alone); the sticky counter goes back into the device record
        if self._opt_on:
            self._opt_state[12:16].view(torch.int32).fill_(int(sd.get("skipped", 0)))
            self._step_dev.fill_(self.step_count)            # a captured graph reads the step, and with it the schedule, from here
        if self.average is not None and "avg_row" in sd:
            self.averaged_weights().copy_(sd["avg_row"])
            self._avg_state[:4].view(torch.int32).fill_(int(sd["avg_n"]))


def save_reference_checkpoint(model: EEG_LSTM, path: str, resample=None) -> None:
    """Write a .pth the reference's SimplePredictor loads unchanged (raw state_dict with the reference's
    key names on CPU; lstm_eeg_model.py:77-81).  A model with a causal front end is written in the dict form both loaders accept,
    {"state_dict": ..., "nsd_prep": prep.to_dict()}: the reference's loader reads the weights, SimplePredictor here rebuilds the prep too.
    A model trained on crops (model.crop) adds "nsd_crop" = {window, crops, hop} to that dict, one with a signal-quality gate
    "nsd_gate" = gate.to_dict(), one with session alignment "nsd_align" = {config, matrix [C,C], record of its fit or None}, one with a
    rate conversion "nsd_resample" = resample.to_dict() (L, M, P and the tap table); a model with none of them is written as before.  resample=: the conversion to
    write for a model that was trained without the stage on trials already brought to its rate (train --input-rate)."""
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    crop, gate = getattr(model, "crop", None), getattr(model, "gate", None)
    align, resample = getattr(model, "align", None), resample if resample is not None else getattr(model, "resample", None)
    if model.prep is None and crop is None and gate is None and align is None and resample is None:
        torch.save(sd, path)
        return
    extra = {} if model.prep is None else {"nsd_prep": model.prep.to_dict()}
    if resample is not None:
        extra["nsd_resample"] = resample.to_dict()
    if gate is not None:
        extra["nsd_gate"] = gate.to_dict()
    if align is not None:
        extra["nsd_align"] = {"config": align.to_dict(), "matrix": model.align_matrix.detach().cpu().clone(),
                              "record": None if model.align_record is None else dict(model.align_record)}
    if crop is not None:
        extra["nsd_crop"] = {"window": int(crop.window), "crops": int(crop.crops), "hop": int(crop.hop)}
    torch.save({"state_dict": sd, **extra}, path)


def init_distributed(backend: Optional[str] = None) -> Tuple[int, int, int]:
    """Join the process group described by torchrun's environment; returns (rank, local_rank, world)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # NSD_DIST_BACKEND=gloo: rehearsal of the multi-rank code path where RCCL cannot run (several ranks on one GPU)
        backend = backend or os.environ.get("NSD_DIST_BACKEND") or ("nccl" if torch.cuda.is_available() else "gloo")
        if backend == "nccl":
            torch.cuda.set_device(local)
            dist.init_process_group(backend, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    return rank, local, world
