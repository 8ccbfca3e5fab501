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

