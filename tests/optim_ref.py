"""float64 restatement of the clipped / scheduled Adam step of include/nsd.h (nsd_opt): the schedule factor f(s), the global-norm clip
coefficient of torch.nn.utils.clip_grad_norm_(norm_type=2) and torch.optim.Adam's update with weight decay applied after clipping.
tests/test_optim_cpu.py pins it to torch (CosineAnnealingLR, StepLR, clip_grad_norm_ + Adam); the GPU tests compare the kernels with it.
numpy and the math module only; nothing here calls the library."""
import math

import numpy as np

KINDS = ("constant", "cosine", "step")


def f32(v) -> float:
    """the value a float field of nsd_opt holds"""
    return float(np.float32(v))


def lr_factor(kind: str, s: int, warmup_steps: int = 0, total_steps: int = 0, min_ratio: float = 0.0, step_size: int = 1,
              gamma: float = 1.0) -> float:
    """f(s), s the 1-based step; min_ratio and gamma as the fp32 fields hold them; libm's cos / pow in double, in the header's order"""
    e, W = s - 1, warmup_steps
    if e < W:
        return (e + 1) / W
    ep = e - W
    if kind == "cosine":
        Np, r = total_steps - W, f32(min_ratio)
        return r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * min(ep, Np) / Np))
    if kind == "step":
        return math.pow(f32(gamma), float(ep // step_size))
    return 1.0


def grad_norm(g, grad_scale: float = 1.0, fp32_product: bool = True):
    """(S, sqrt(S)) of g~ = g * grad_scale in float64; fp32_product: g~ rounded to fp32 first, as the kernels form it"""
    g = np.asarray(g)
    gt = (g.astype(np.float32) * np.float32(grad_scale)).astype(np.float64) if fp32_product else g.astype(np.float64) * grad_scale
    with np.errstate(over="ignore", invalid="ignore"):
        S = float(np.sum(gt * gt))
    return S, math.sqrt(S)


def clip_coef(norm: float, max_norm: float) -> float:
    return min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0


class ClippedAdam:
    """State (p, m, v, step s, skipped) in float64.  step(g) follows the header: norm, skip when not finite, coef, schedule, Adam."""

    def __init__(self, p0, *, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_scale=1.0, max_norm=0.0,
                 schedule=None, fp32_fields: bool = True, step: int = 0):
        c = f32 if fp32_fields else float
        self.p = np.asarray(p0, dtype=np.float64).copy()
        self.m, self.v = np.zeros_like(self.p), np.zeros_like(self.p)
        self.lr, self.b1, self.b2, self.eps, self.wd = c(lr), c(beta1), c(beta2), c(eps), c(weight_decay)
        self.gscale, self.max_norm, self.fp32 = c(grad_scale), c(max_norm), fp32_fields
        self.schedule = dict(schedule or dict(kind="constant"))
        self.s, self.skipped = int(step), 0

    def step(self, g) -> dict:
        self.s += 1
        S, norm = grad_norm(g, self.gscale, self.fp32)
        lr_eff = self.lr * lr_factor(s=self.s, **self.schedule)
        if self.fp32:
            lr_eff = f32(lr_eff)
        if not math.isfinite(S):
            self.skipped += 1
            return dict(norm=norm, coef=0.0, lr=lr_eff, skipped=True)
        coef = clip_coef(norm, self.max_norm)
        if self.fp32:
            coef = f32(coef)
        g = np.asarray(g, dtype=np.float64)
        gt = (np.asarray(g, dtype=np.float32) * np.float32(self.gscale)).astype(np.float64) if self.fp32 else g * self.gscale
        gi = gt * coef + self.wd * self.p
        self.m = self.b1 * self.m + (1.0 - self.b1) * gi
        self.v = self.b2 * self.v + (1.0 - self.b2) * gi * gi
        bc1, bc2 = 1.0 - self.b1 ** self.s, 1.0 - self.b2 ** self.s
        self.p = self.p - (lr_eff / bc1) * (self.m / (np.sqrt(self.v) / math.sqrt(bc2) + self.eps))
        return dict(norm=norm, coef=coef, lr=lr_eff, skipped=False)
