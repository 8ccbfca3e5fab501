"""Sharpness-aware minimisation restated in numpy (the rule of include/nsd.h, nsd_sam).  ascend() is the ascent with the kernel's
roundings: S in float64 from the fp32 products (optim_ref.grad_norm, the tail's definition), the step length formed in double and rounded
once to fp32, then one rounded fp32 product and one rounded fp32 sum per element.  SamAdam is a float64 SAM + Adam step on
optim_ref.ClippedAdam, which tests/test_sam_cpu.py pins to stock torch.  numpy and the math module only; nothing here calls the library."""
import math

import numpy as np

from tests.optim_ref import ClippedAdam, grad_norm


def step_length(rho, S):
    """es = (float)((double)rho / (sqrt(S) + 1e-12)) with rho as the fp32 field holds it; 0 where the row is a copy"""
    rho = float(np.float32(rho))
    if rho == 0.0 or not math.isfinite(S):
        return np.float32(0.0)
    return np.float32(rho / (math.sqrt(S) + 1e-12))


def ascend(p, g, rho, grad_scale=1.0):
    """-> (p_adv fp32, record dict(norm, scale, nonfinite: 0 or 1)).  rho == 0 or S not finite: p_adv is p, word for word."""
    p, g = np.asarray(p, dtype=np.float32), np.asarray(g, dtype=np.float32)
    S, norm = grad_norm(g, grad_scale)
    es = step_length(rho, S)
    with np.errstate(over="ignore", invalid="ignore"):
        rec = dict(norm=float(np.float32(norm)), scale=float(es), nonfinite=0 if math.isfinite(S) else 1)
    if float(np.float32(rho)) == 0.0 or not math.isfinite(S):
        return p.copy(), rec
    gt = g * np.float32(grad_scale)              # fp32(grads[e] * grad_scale)
    up = es * gt                                 # one rounded product ...
    return (p + up).astype(np.float32), rec      # ... and one rounded sum


class SamAdam:
    """float64 SAM + Adam: step(grad_fn) takes g = grad_fn(p), e = rho g / (|g| + 1e-12), g2 = grad_fn(p + e), and gives g2 to
    ClippedAdam (p itself is never moved by e)."""

    def __init__(self, p0, rho, **adam):
        self.rho = float(rho)
        self.opt = ClippedAdam(p0, fp32_fields=False, **adam)

    @property
    def p(self):
        return self.opt.p

    def step(self, grad_fn) -> dict:
        g = np.asarray(grad_fn(self.opt.p), dtype=np.float64)
        e = self.rho * g / (math.sqrt(float(np.sum(g * g))) + 1e-12)
        g2 = np.asarray(grad_fn(self.opt.p + e), dtype=np.float64)
        return self.opt.step(g2)
