"""Session alignment (nsd_cov_step / nsd_whiten_fit / nsd_spatial_apply of include/nsd.h, csrc/nsd_align.hip): every session is whitened
by the inverse square root of its mean channel second moment, y = R^(-1/2) x (Euclidean alignment) -- label-free, a fixed C x C matrix at
serve time.  Host side: the configuration, the numpy restatements for host use, and `fit`, which runs a model's own front end over
trials and forms the matrices on the device.

An extension: the reference never mixes channels.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from . import _lib

MAX_CHANNELS = 32                # the gate's range: the mask words of nsd_gate_step travel with the samples


@dataclass(frozen=True)
class SessionAlign:
    """R' = (1 - shrinkage) R + shrinkage (tr R / C) I;  eigenvalues below floor * lambda_max are raised to it;  a group of fewer than
    min_steps used steps keeps the identity (None: 4 * C)."""
    shrinkage: float = 0.0
    floor: float = 1e-4
    min_steps: Optional[int] = None

    def __post_init__(self):
        s, f = float(np.float32(self.shrinkage)), float(np.float32(self.floor))
        if not (math.isfinite(s) and 0.0 <= s <= 1.0):
            raise ValueError(f"SessionAlign: shrinkage {self.shrinkage!r} must lie in [0, 1]")
        if not (math.isfinite(f) and 0.0 < f <= 1.0):
            raise ValueError(f"SessionAlign: floor {self.floor!r} must lie in (0, 1]")
        object.__setattr__(self, "shrinkage", s)
        object.__setattr__(self, "floor", f)
        if self.min_steps is not None:
            if int(self.min_steps) != self.min_steps or int(self.min_steps) < 1:
                raise ValueError(f"SessionAlign: min_steps {self.min_steps!r} must be an integer >= 1 (or None: 4 * C)")
            object.__setattr__(self, "min_steps", int(self.min_steps))

    def steps_needed(self, C: int) -> int:
        return 4 * int(C) if self.min_steps is None else self.min_steps

    def struct(self, C: int = 1) -> "_lib.Whiten":
        """nsd_whiten for C channels: the two ratios as fp32"""
        return _lib.Whiten(self.shrinkage, self.floor, self.steps_needed(C))

    def to_dict(self) -> dict:
        return {"shrinkage": self.shrinkage, "floor": self.floor, "min_steps": self.min_steps}

    @classmethod
    def from_dict(cls, d: dict) -> "SessionAlign":
        return cls(**{k: d[k] for k in ("shrinkage", "floor", "min_steps") if k in d})

    # ---- the numpy restatements, for host use ----
    @staticmethod
    def cov_reference(v, mask=None, init=None) -> Tuple[np.ndarray, np.ndarray]:
        """v [B,T,C] (or [T,C]) fp32, mask [B,T] uint32 or None -> (sums [B,C,C] float64, counts [B,2] int64: used, skipped), bit for
        bit what nsd_cov_step writes.  init: the (sums, counts) the streams start from (default: zero, window mode)."""
        x = np.asarray(v, np.float32)
        x = x[None] if x.ndim == 2 else x
        if x.ndim != 3 or not 1 <= x.shape[2] <= MAX_CHANNELS:
            raise ValueError(f"SessionAlign.cov_reference: v must be [B,T,C] or [T,C] with C in [1, {MAX_CHANNELS}], got {x.shape}")
        B, T, Cc = x.shape
        used = np.isfinite(x).all(axis=2)
        if mask is not None:
            used &= np.asarray(mask).reshape(B, T).astype(np.uint32) == 0
        sums = np.zeros((B, Cc, Cc), np.float64) if init is None else np.array(init[0], np.float64).reshape(B, Cc, Cc)
        counts = np.zeros((B, 2), np.int64) if init is None else np.array(init[1], np.int64).reshape(B, 2)
        x64 = np.where(used[:, :, None], x, np.float32(0)).astype(np.float64)
        for t in range(T):                                     # one serial chain per (i, j): the product is exact, the sum rounds once
            u = used[:, t]
            sums[u] = sums[u] + x64[u, t, :, None] * x64[u, t, None, :]
        counts[:, 0] += used.sum(axis=1)
        counts[:, 1] += T - used.sum(axis=1)
        return sums, counts

    def fit_reference(self, sums, counts, groups=None, G: int = 1) -> Tuple[np.ndarray, List[dict]]:
        """sums [N,C,C] float64, counts [N,2] int64, groups None or N indices -> (W [G,C,C] fp32, G records) as nsd_whiten_fit forms
        them, with numpy.linalg.eigh (float64) where the kernel runs its Jacobi sweeps (the records carry no sweep count)."""
        sums, counts = np.asarray(sums, np.float64), np.asarray(counts, np.int64).reshape(-1, 2)
        N = counts.shape[0]
        if N == 0:
            raise ValueError("SessionAlign.fit_reference: no accumulator (the channel count is unknown)")
        Cc = int(round(math.sqrt(sums.size // N)))
        groups = np.zeros(N, np.int64) if groups is None else np.asarray(groups, np.int64).reshape(N)
        sums = sums.reshape(N, Cc, Cc)
        ignored = int(((groups < 0) | (groups >= G)).sum())
        Ws, recs = np.empty((G, Cc, Cc), np.float32), []
        shrink, floor = float(self.shrinkage), float(self.floor)
        for g in range(G):
            S, n, skipped, nacc = np.zeros((Cc, Cc), np.float64), 0, 0, 0
            for a in np.flatnonzero(groups == g):
                S, n, skipped, nacc = S + sums[a], n + int(counts[a, 0]), skipped + int(counts[a, 1]), nacc + 1
            rec = dict(steps=n, skipped=skipped, trace_mean=0.0, eig_min=0.0, eig_max=0.0, status=0, accumulators=nacc, ignored=ignored)
            if n < self.steps_needed(Cc):
                rec["status"] = _lib.NSD_WHITEN_FEW
            elif not np.isfinite(S).all() or not np.trace(S) > 0:
                rec["status"] = _lib.NSD_WHITEN_NONFINITE
            else:
                R = S / float(n)
                tm = np.trace(R) / Cc
                lam, V = np.linalg.eigh((1.0 - shrink) * R + shrink * tm * np.eye(Cc))
                thr = floor * lam.max()
                if lam.min() < thr:
                    rec["status"] |= _lib.NSD_WHITEN_CLIPPED
                W = (V * (1.0 / np.sqrt(np.maximum(lam, thr)))) @ V.T
                Ws[g] = (0.5 * (W + W.T)).astype(np.float32)
                rec.update(trace_mean=float(tm), eig_min=float(lam.min()), eig_max=float(lam.max()))
            if rec["status"] & (_lib.NSD_WHITEN_FEW | _lib.NSD_WHITEN_NONFINITE):
                Ws[g] = np.eye(Cc, dtype=np.float32)
            recs.append(rec)
        return Ws, recs

    @staticmethod
    def apply_reference(v, W, sel=None) -> np.ndarray:
        """v [B,T,C] fp32, W [C,C] or [n_mat,C,C] fp32, sel None or B indices -> what nsd_spatial_apply writes, bit for bit: the sum over
        the input channel serially, every product and every sum rounded to fp32."""
        x = np.asarray(v, np.float32)
        W = np.asarray(W, np.float32)
        W = W[None] if W.ndim == 2 else W
        B, T, Cc = x.shape
        sel = np.zeros(B, np.int64) if sel is None else np.asarray(sel, np.int64).reshape(B)
        ok = (sel >= 0) & (sel < W.shape[0])
        Wb = W[np.where(ok, sel, 0)]                           # [B,C,C]
        with np.errstate(invalid="ignore", over="ignore"):
            acc = Wb[:, None, :, 0] * x[:, :, None, 0]
            for j in range(1, Cc):
                acc = acc + Wb[:, None, :, j] * x[:, :, None, j]
        acc = acc.astype(np.float32)
        acc[~ok] = np.nan
        return acc

    # ---- the fit on the device ----
    def fit(self, model, trials, groups=None):
        """The alignment matrices of `trials` [N,T,C] as `model` sees them: the model's own gate -> prep -> apply over whole windows
        (eval mode: a rejected step is left out of the moment), then nsd_cov_step and nsd_whiten_fit.  groups: None (one matrix from all
        trials) or N group indices in [0, G) -> (W float32 [G,C,C] on the device, the G records as dicts).  Label-free."""
        import torch
        from . import ops
        x = torch.as_tensor(trials, dtype=torch.float32)
        dev = next(model.parameters()).device
        x = x.to(dev).contiguous()
        if x.dim() != 3 or x.shape[-1] != model.spec.C:
            raise ValueError(f"SessionAlign.fit: trials must be [N, T, {model.spec.C}], got {tuple(x.shape)}")
        if getattr(model, "resample", None) is not None:    # stage 0 of the model's front end: the trials are at the amplifier's rate
            x = ops.resample_trials(x, model.resample)
        G, group = 1, None
        if groups is not None:
            g = np.asarray(groups, np.int64).reshape(-1)
            if g.size != x.shape[0] or (g.size and g.min() < 0):
                raise ValueError(f"SessionAlign.fit: groups must be {x.shape[0]} indices >= 0")
            G = int(g.max()) + 1 if g.size else 1
            group = torch.as_tensor(g, dtype=torch.int32).to(dev)
        with torch.no_grad():
            was = model.training
            model.eval()
            try:
                v, mask = model._gate_prep(x, want_mask=True)
            finally:
                model.train(was)
            sums, counts = ops.cov_step(v, mask=mask)
            W, rec = ops.whiten_fit(model.spec.C, self, sums, counts, group=group, G=G)
        return W, ops.whiten_records(rec, G)


def mean_over_models(d) -> np.ndarray:
    """The numpy restatement of NSD_DX_MEAN and nsd_multi_loss_mean (include/nsd.h): d [M, ...] fp32 -> (((d[0] + d[1]) + ...) + d[M-1])
    / float32(M) -- a serial fp32 sum over m ascending, every addition rounded on its own, then one division.  M = 1 returns d[0]'s
    bits; a non-finite value stays in its own element."""
    d = np.asarray(d, np.float32)
    if d.ndim < 1 or d.shape[0] < 1:
        raise ValueError(f"mean_over_models: expected [M >= 1, ...], got {d.shape}")
    with np.errstate(invalid="ignore", over="ignore"):
        s = d[0].copy()
        for m in range(1, d.shape[0]):
            s = (s + d[m]).astype(np.float32)
        return (s / np.float32(d.shape[0])).astype(np.float32)


def check_spatial_fit(epochs, lr, decay, betas, eps) -> None:
    """The configuration nsd_spatial_fit_step would refuse, refused on the host with the field's name."""
    if isinstance(epochs, bool) or int(epochs) != epochs or int(epochs) < 1:
        raise ValueError(f"SpatialFit: epochs {epochs!r} must be an integer >= 1")
    for name, v in (("lr", lr), ("decay", decay)):
        if not (math.isfinite(float(v)) and float(v) >= 0.0):
            raise ValueError(f"SpatialFit: {name} {v!r} must be finite and >= 0")
    if len(tuple(betas)) != 2 or not all(0.0 <= float(b) < 1.0 for b in betas):
        raise ValueError(f"SpatialFit: betas {betas!r} must be two values in [0, 1)")
    if not (math.isfinite(float(eps)) and float(eps) > 0.0):
        raise ValueError(f"SpatialFit: eps {eps!r} must be finite and > 0")


class SpatialFit:
    """Supervised session alignment: fit the model's alignment matrix A [C,C] on a few labelled trials of the new session by gradient
    descent THROUGH the frozen model (nsd_spatial_bwd / nsd_spatial_fit_step of include/nsd.h), everything on the device.  Whitening
    restores the second moment and leaves a rotation open; the labels close it.

      fit(trials, labels) -> losses [E]   trials [N,T,C], labels [N] class indices.  The model's own gate -> prep -> apply runs over
                                          the trials ONCE, in eval mode: these inputs v are frozen.  Every epoch then runs, full batch:
                                          nsd_spatial_apply(v, A) -> nsd_lstm_head_train[_soft] -> nsd_lstm_bwd with dx -> nsd_loss_sum ->
                                          nsd_spatial_bwd (dA) -> nsd_spatial_fit_step (Adam on A with g = dA + decay * (A - A0)).  The
                                          forward takes eval-mode noise (no dropout, the eval RReLU slope) through the explicit mask
                                          arguments, as dx needs.  The model's parameters are read and never written.  Epoch 1 runs
                                          eagerly; epochs 2 .. E replay one captured graph where capture works (graph=None), the same
                                          launches eagerly where it does not (or with graph=False): the bits are the same.  losses[e]: the
                                          mean loss before epoch e's update, copied on the device.  The fitted matrix is written with
                                          model.set_alignment; its record gains "spatial_fit".  A second call continues the run (Adam's
                                          moments and step live in the state): 2 + 3 epochs leave the bits 5 leave.
      reset()                             forget the moments, the step and the status (the matrix stays as it is)
      status()                            [status word]: 1 where an epoch's gradient was not finite -- those epochs left A untouched
      check()                             raises NsdError where the status is set

    A0, the prior the fit starts from and is pulled towards, is the matrix the model holds at construction: the whitening matrix of a
    label-free refit, or the identity (a model without align= gains the stage through EEG_LSTM.enable_alignment()).
    epochs = 50, lr = 1e-2 and decay = 1e-2 are CHOICES, not measurements: nothing here has tuned them on held-out data.
    loss: an nsd_amd.Loss -- label smoothing and class weights build the target rows as HeadFit.targets does; mixup is refused (the
    inputs are frozen whole trials)."""

    def __init__(self, model, *, epochs: int = 50, lr: float = 1e-2, decay: float = 1e-2, betas=(0.9, 0.999), eps: float = 1e-8,
                 loss=None, graph: Optional[bool] = None):
        from . import ops
        from .lstm_eeg_model import EEG_LSTM
        if not isinstance(model, EEG_LSTM):
            raise _lib.NsdError("SpatialFit: expected an EEG_LSTM (an ensemble is fitted member by member)")
        check_spatial_fit(epochs, lr, decay, betas, eps)
        sp = model.spec
        if model.precision != "fp32" or sp.D != 1 or not ops.dx_path(sp, 1, 1) or not (sp.H == 48 and sp.L == 2 and sp.C <= 8):
            raise _lib.NsdError(f"SpatialFit: model shape {sp} is outside nsd_dx_path's fast path -- the input gradient the fit descends "
                                "along is formed for fp32 models of hidden size 48, 2 layers and <= 8 channels")
        if loss is not None and loss.mixup:
            raise _lib.NsdError("SpatialFit: mixup is refused -- the inputs are frozen whole trials; label smoothing and class weights apply")
        if loss is not None:
            loss.check_classes(sp.K)
        flat = model.flat_parameters()
        if not flat.is_cuda:
            raise _lib.NsdError("SpatialFit runs only on the MI355X HIP path: move the model to the GPU first; there is no CPU fallback")
        model.enable_alignment()
        self.model, self.spec, self.device = model, sp, flat.device
        self.epochs, self.lr, self.decay, self.betas, self.eps = int(epochs), float(lr), float(decay), (float(betas[0]), float(betas[1])), float(eps)
        self.loss, self.graph = loss, graph
        self.A0 = model.align_matrix.detach().to(self.device).clone().contiguous()
        self.A = self.A0.clone()
        self.state = ops.spatial_fit_state(sp.C, 1, self.device)
        self.replayed = False                                  # whether the last fit() replayed a captured graph
        self.capture_error = None                              # the last failed capture's error (graph=None falls back to eager)
        self._losses = []                                      # the mean losses of every epoch since the reset

    def targets(self, labels, N: int):
        """(int32 labels [N] on the device, target rows [N,K] or None): the rows where a Loss asks for them, one nsd_mixup launch at mix = 0"""
        import torch
        from . import ops
        y = labels if torch.is_tensor(labels) else torch.from_numpy(np.ascontiguousarray(labels))
        y = y.to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
        if int(y.numel()) != N:
            raise _lib.NsdError(f"SpatialFit.fit: {int(y.numel())} labels for {N} trials")
        return y, (None if self.loss is None else ops.target_rows(y, self.spec.K, 1, self.loss))

    def fit(self, trials, labels, epochs: Optional[int] = None):
        import torch
        from . import ops
        sp, dev, model = self.spec, self.device, self.model
        E = self.epochs if epochs is None else int(epochs)
        if E < 1:
            raise ValueError(f"SpatialFit.fit: epochs {epochs!r} must be >= 1")
        x = torch.as_tensor(trials, dtype=torch.float32).to(dev).contiguous()
        if x.dim() != 3 or x.shape[-1] != sp.C or x.shape[0] < 1:
            raise ValueError(f"SpatialFit.fit: trials must be [N >= 1, T, {sp.C}], got {tuple(x.shape)}")
        if getattr(model, "resample", None) is not None:    # stage 0 of the model's front end: the trials are at the amplifier's rate
            x = ops.resample_trials(x, model.resample)
        N, T = int(x.shape[0]), int(x.shape[1])
        if not ops.dx_path(sp, N, T):
            raise _lib.NsdError(f"SpatialFit.fit: {N} trials of {T} steps for {sp} are outside nsd_dx_path (hidden size 48, 2 layers, <= 8 channels)")
        with torch.no_grad():
            y, q = self.targets(labels, N)
            was = model.training
            model.eval()
            try:
                v = model._gate_prep(x)                        # the frozen inputs: the model's own front end, once
            finally:
                model.train(was)
            v = v.clone() if v is x else v
            flat = model.flat_parameters()
            xa, dx = torch.empty_like(v), torch.empty_like(v)
            ws = ops.new_workspace(sp, N, T, dev)
            logits = torch.empty((N, sp.K), dtype=torch.float32, device=dev)
            dA = torch.empty((1, sp.C, sp.C), dtype=torch.float32, device=dev)
            counts = torch.empty(2, dtype=torch.int64, device=dev)
            scratch = torch.empty(N * sp.C * sp.C, dtype=torch.float64, device=dev)
            loss1 = torch.zeros(1, dtype=torch.float32, device=dev)
            losses = torch.full((E,), float("nan"), dtype=torch.float32, device=dev)
            self.state[-8:].zero_()                            # the call counter indexes this call's losses

            def epoch():
                ops.spatial_apply(v, self.A, out=xa)
                ops.train_dx(sp, flat, xa, ws, logits, dx, labels=y, targets=q, rrelu_slope=None, residual=model.residual, loss_out=loss1)
                ops.spatial_bwd(v, dx, self.A, want_dv=False, dW=dA, counts=counts, scratch=scratch)
                ops.spatial_fit_step(self.A, dA, self.state, A0=self.A0, lr=self.lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps,
                                     decay=self.decay, loss_in=loss1, loss_out=losses)

            epoch()
            g = self._capture(epoch) if E > 1 and self.graph is not False else None
            self.replayed = g is not None
            for _ in range(E - 1):
                if g is not None:
                    g.replay()
                else:
                    epoch()
            mean = losses / float(N)
            host = [float(l) for l in mean.cpu()]
            self._losses.extend(host)
            rec = dict(model.align_record or {})
            rec["spatial_fit"] = dict(epochs=len(self._losses), lr=self.lr, decay=self.decay, loss_first=self._losses[0],
                                      loss_last=self._losses[-1], status=self.status()[0])
            model.set_alignment(self.A, record=rec)
        return mean

    def _capture(self, epoch):
        """One epoch as a captured graph, or None where capture does not work (graph=True: the error is raised).  Capture runs nothing:
        the state is as the eager epochs left it."""
        import torch
        try:
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                epoch()
            return g
        except Exception as e:                                 # (graph=None: eager is the fallback and leaves the same bits -- but say so)
            if self.graph:
                raise
            import warnings
            self.capture_error = repr(e)
            warnings.warn(f"SpatialFit: capturing the epoch as a graph failed ({e!r}); the remaining epochs run eagerly", RuntimeWarning)
            torch.cuda.synchronize(self.device)
            return None

    def reset(self) -> None:
        self.state.zero_()
        self._losses = []

    def _records(self):
        from . import ops
        return ops.spatial_fit_records(self.spec.C, 1, self.state)

    def epochs_done(self) -> int:
        return self._records()[0]["step"]

    def status(self) -> list:
        return [int(r["status"]) for r in self._records()]

    def check(self) -> None:
        if any(self.status()):
            raise _lib.NsdError("SpatialFit: an epoch's gradient of the alignment matrix was not finite (a non-finite input step, or a loss "
                                "that overflowed); those epochs left the matrix untouched.  reset() clears the status")


class EnsembleSpatialFit(SpatialFit):
    """SpatialFit for the object the ensemble decoders serve: ONE alignment matrix A [C,C] fitted through M frozen models at once, on
    the objective (1/M) sum_m mean_n CE_m -- the members share one front end (member 0's gate -> prep -> apply -> A), so M matrices
    fitted member by member could not be served.

      models    a sequence of EEG_LSTM of one shape, or the ensemble an EnsemblePredictor holds (`predictor.model`), as HeadFit takes them
      fit(trials, labels) -> losses [E]   member 0's gate -> prep -> apply runs over the trials ONCE, in eval mode.  Every epoch is
                                          nsd_spatial_apply(v, A) -> nsd_multi_train_fwd[_soft] (x_model_stride = 0, rng NULL: eval-mode
                                          noise) -> nsd_multi_train_bwd_dx(NSD_DX_MEAN) -> nsd_multi_loss_mean -> nsd_spatial_bwd ->
                                          nsd_spatial_fit_step: the launches of a single model's epoch, whatever M.  dx is the serial
                                          fp32 mean over the members (mean_over_models), losses[e] the same mean of the members' mean
                                          losses before epoch e's update.  Epoch 1 runs eagerly, epochs 2 .. E replay one captured graph
                                          (graph=, replayed, capture_error: SpatialFit's).  The members' parameters are read, never
                                          written.  The fitted matrix is written to EVERY member with set_alignment; the record's
                                          "spatial_fit" carries members = M and shared = True.
      reset / status / check / epochs_done, continuation (2 + 3 epochs leave the bits of 5) and the refusals are SpatialFit's.

    A0 is the matrix the members share at construction; members without the stage gain it at the identity (enable_alignment()),
    members that hold different matrices are refused.  One member, or two copies of one model, leave SpatialFit's bits.
    The defaults are SpatialFit's: choices, not measurements."""

    def __init__(self, models, *, epochs: int = 50, lr: float = 1e-2, decay: float = 1e-2, betas=(0.9, 0.999), eps: float = 1e-8,
                 loss=None, graph: Optional[bool] = None):
        import torch
        from . import ops
        from .lstm_eeg_model import EEG_LSTM
        from .multimodel import _check_models
        self._ensemble = None
        if hasattr(models, "models") and hasattr(models, "params"):
            self._ensemble, members = models, list(models.models)
        elif isinstance(models, EEG_LSTM):
            members = [models]
        else:
            try:
                members = list(models)
            except TypeError:
                members = [models]
        if not members or not all(isinstance(m, EEG_LSTM) for m in members):
            raise _lib.NsdError("EnsembleSpatialFit: expected a sequence of EEG_LSTM, or the ensemble an EnsemblePredictor holds")
        _check_models(members, "EnsembleSpatialFit")
        check_spatial_fit(epochs, lr, decay, betas, eps)
        sp, M = members[0].spec, len(members)
        if not ops.multi_dx_path(sp, M):
            raise _lib.NsdError(f"EnsembleSpatialFit: {M} models of shape {sp} are outside nsd_multi_dx_path -- the input gradient the fit "
                                "descends along is formed for fp32 models of hidden size 48, 2 layers and <= 8 channels")
        if loss is not None and loss.mixup:
            raise _lib.NsdError("EnsembleSpatialFit: mixup is refused -- the inputs are frozen whole trials; label smoothing and class weights apply")
        if loss is not None:
            loss.check_classes(sp.K)
        if members[0].align is not None:
            for i, m in enumerate(members[1:], 1):
                if not torch.equal(m.align_matrix.detach().cpu(), members[0].align_matrix.detach().cpu()):
                    raise _lib.NsdError(f"EnsembleSpatialFit: member {i} holds another alignment matrix than member 0 -- the members share "
                                        "one front end and the fit starts from ONE matrix; set_alignment the same matrix on all first")
        flats = [m.flat_parameters() for m in members]
        if not all(f.is_cuda for f in flats):
            raise _lib.NsdError("EnsembleSpatialFit runs only on the MI355X HIP path: move the models to the GPU first; there is no CPU fallback")
        if self._ensemble is not None:
            self._ensemble.enable_alignment()
        else:
            for m in members:
                m.enable_alignment()
        self.members, self.model, self.spec, self.device = members, members[0], sp, flats[0].device
        self.epochs, self.lr, self.decay, self.betas, self.eps = int(epochs), float(lr), float(decay), (float(betas[0]), float(betas[1])), float(eps)
        self.loss, self.graph = loss, graph
        self.A0 = members[0].align_matrix.detach().to(self.device).clone().contiguous()
        self.A = self.A0.clone()
        self.state = ops.spatial_fit_state(sp.C, 1, self.device)
        self.replayed = False
        self.capture_error = None
        self._losses = []

    @property
    def M(self) -> int:
        return len(self.members)

    def _params(self):
        """[M,P]: the ensemble's own stacked buffer (what its decoders read), or a gathered copy of the members' vectors"""
        import torch
        if self._ensemble is not None:
            return self._ensemble.params
        return torch.stack([m.flat_parameters() for m in self.members]).contiguous()

    def targets(self, labels, N: int):
        """(int32 labels [M*N] on the device -- the same N for every member --, target rows [M*N,K] or None)"""
        import torch
        from . import ops
        y = labels if torch.is_tensor(labels) else torch.from_numpy(np.ascontiguousarray(labels))
        y = y.to(device=self.device, dtype=torch.int32).reshape(-1)
        if int(y.numel()) != N:
            raise _lib.NsdError(f"EnsembleSpatialFit.fit: {int(y.numel())} labels for {N} trials")
        y = y.repeat(self.M).contiguous()
        return y, (None if self.loss is None else ops.target_rows(y, self.spec.K, self.M, self.loss))

    def fit(self, trials, labels, epochs: Optional[int] = None):
        import torch
        from . import ops
        sp, dev, M = self.spec, self.device, self.M
        E = self.epochs if epochs is None else int(epochs)
        if E < 1:
            raise ValueError(f"EnsembleSpatialFit.fit: epochs {epochs!r} must be >= 1")
        x = torch.as_tensor(trials, dtype=torch.float32).to(dev).contiguous()
        if x.dim() != 3 or x.shape[-1] != sp.C or x.shape[0] < 1:
            raise ValueError(f"EnsembleSpatialFit.fit: trials must be [N >= 1, T, {sp.C}], got {tuple(x.shape)}")
        if getattr(self.members[0], "resample", None) is not None:    # stage 0 of the shared front end
            x = ops.resample_trials(x, self.members[0].resample)
        N, T = int(x.shape[0]), int(x.shape[1])
        if not ops.multi_dx_path(sp, M, N, T):
            raise _lib.NsdError(f"EnsembleSpatialFit.fit: {N} trials of {T} steps for {M} models of {sp} are outside nsd_multi_dx_path "
                                "(hidden size 48, 2 layers, <= 8 channels, T <= 1024)")
        with torch.no_grad():
            y, q = self.targets(labels, N)
            front = self.members[0]
            was = front.training
            front.eval()
            try:
                v = front._gate_prep(x)                        # the frozen inputs: the shared front end (member 0's), once
            finally:
                front.train(was)
            v = v.clone() if v is x else v
            params = self._params()
            xa, dx = torch.empty_like(v), torch.empty_like(v)
            ws = ops.multi_workspace(sp, M, N, T, dev)
            logits = torch.empty((M * N, sp.K), dtype=torch.float32, device=dev)
            dA = torch.empty((1, sp.C, sp.C), dtype=torch.float32, device=dev)
            counts = torch.empty(2, dtype=torch.int64, device=dev)
            scratch = torch.empty(N * sp.C * sp.C, dtype=torch.float64, device=dev)
            loss1 = torch.zeros(1, dtype=torch.float32, device=dev)
            losses = torch.full((E,), float("nan"), dtype=torch.float32, device=dev)
            self.state[-8:].zero_()                            # the call counter indexes this call's losses

            def epoch():
                ops.spatial_apply(v, self.A, out=xa)
                ops.multi_train_dx(sp, params, xa, ws, logits, dx, labels=y, targets=q, reduce="mean", loss_out=loss1)
                ops.spatial_bwd(v, dx, self.A, want_dv=False, dW=dA, counts=counts, scratch=scratch)
                ops.spatial_fit_step(self.A, dA, self.state, A0=self.A0, lr=self.lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps,
                                     decay=self.decay, loss_in=loss1, loss_out=losses)

            epoch()
            g = self._capture(epoch) if E > 1 and self.graph is not False else None
            self.replayed = g is not None
            for _ in range(E - 1):
                if g is not None:
                    g.replay()
                else:
                    epoch()
            mean = losses / float(N)
            host = [float(l) for l in mean.cpu()]
            self._losses.extend(host)
            rec = dict(self.members[0].align_record or {})
            rec["spatial_fit"] = dict(epochs=len(self._losses), lr=self.lr, decay=self.decay, loss_first=self._losses[0],
                                      loss_last=self._losses[-1], status=self.status()[0], members=M, shared=True)
            for m in self.members:
                m.set_alignment(self.A, record=rec)
        return mean

    def check(self) -> None:
        if any(self.status()):
            raise _lib.NsdError("EnsembleSpatialFit: an epoch's gradient of the alignment matrix was not finite (a non-finite input step, or "
                                "a loss that overflowed); those epochs left the matrix untouched.  reset() clears the status")
