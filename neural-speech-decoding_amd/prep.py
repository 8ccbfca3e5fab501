"""The configuration of the causal front end (nsd_prep of include/nsd.h, csrc/nsd_prep.hip): what a live stream goes through chunk by
chunk in front of the model, and what the trainers therefore run over whole windows.  Host side only: the sections are designed here in
float64 and handed to the kernels as fp32 coefficients; ops.prep_step runs them.

An extension: the reference filters whole windows with a non-causal third-party filter (preprocessor.py:21-36), which a stream cannot use.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import numpy as np

from . import _lib

Section = Tuple[float, float, float, float, float]      # b0 b1 b2 a1 a2 (a0 = 1)


def _butter2(kind: str, fc: float, fs: float) -> Section:
    """Second-order Butterworth section by the bilinear transform with pre-warping: K = tan(pi fc / fs), Q = 1 / sqrt(2),
    n = 1 / (1 + K / Q + K^2); low-pass b = n K^2 (1, 2, 1), high-pass b = n (1, -2, 1); a1 = 2 n (K^2 - 1), a2 = n (1 - K / Q + K^2)
    (scipy.signal.butter(2, fc, kind, fs=fs))."""
    if not 0.0 < fc < fs / 2:
        raise ValueError(f"CausalPrep.design: {kind} corner {fc!r} Hz outside (0, fs / 2 = {fs / 2})")
    K = math.tan(math.pi * fc / fs)
    rq = math.sqrt(2.0)
    n = 1.0 / (1.0 + K * rq + K * K)
    a1, a2 = 2.0 * n * (K * K - 1.0), n * (1.0 - K * rq + K * K)
    if kind == "lowpass":
        return (n * K * K, 2.0 * n * K * K, n * K * K, a1, a2)
    return (n, -2.0 * n, n, a1, a2)


def _notch(f0: float, q: float, fs: float) -> Section:
    """scipy.signal.iirnotch(f0, q, fs): w0 = 2 pi f0 / fs, bw = w0 / q, beta = tan(bw / 2), g = 1 / (1 + beta);
    b = g (1, -2 cos w0, 1), a = (1, -2 g cos w0, 2 g - 1)."""
    if not 0.0 < f0 < fs / 2 or not q > 0:
        raise ValueError(f"CausalPrep.design: notch at {f0!r} Hz (Q = {q!r}) outside (0, fs / 2 = {fs / 2})")
    w0 = 2.0 * math.pi * f0 / fs
    g = 1.0 / (1.0 + math.tan(w0 / q / 2.0))
    return (g, -2.0 * g * math.cos(w0), g, -2.0 * g * math.cos(w0), 2.0 * g - 1.0)


@dataclass(frozen=True)
class CausalPrep:
    """Causal per-channel front end, in this order (include/nsd.h has the arithmetic): baseline removal (the slot's first sample),
    common-average reference, `sections` (up to 4 second-order IIR sections (b0, b1, b2, a1, a2), the same for all channels) and a
    running z-score (alpha > 0: exponential mean / variance with that weight, started at the first sample and `var0`)."""
    sections: Tuple[Section, ...] = ()
    alpha: float = 0.0
    var0: float = 1.0
    baseline: bool = True
    car: bool = False

    def __post_init__(self):
        secs = tuple(tuple(float(v) for v in s) for s in self.sections)
        object.__setattr__(self, "sections", secs)
        if len(secs) > _lib.NSD_PREP_MAX_SECTIONS or any(len(s) != 5 for s in secs):
            raise ValueError(f"CausalPrep: at most {_lib.NSD_PREP_MAX_SECTIONS} sections of 5 coefficients (b0 b1 b2 a1 a2), got {secs!r}")
        for s in secs:
            a1, a2 = float(np.float32(s[3])), float(np.float32(s[4]))
            if not all(math.isfinite(float(np.float32(v))) for v in s) or not (abs(a2) < 1.0 and abs(a1) < 1.0 + a2):
                raise ValueError(f"CausalPrep: section {s!r} is not finite or not stable (|a2| < 1 and |a1| < 1 + a2)")
        if not 0.0 <= self.alpha < 1.0:
            raise ValueError(f"CausalPrep: alpha {self.alpha!r} outside [0, 1)")
        if not math.isfinite(self.var0) or (self.alpha > 0 and not self.var0 > 0):
            raise ValueError(f"CausalPrep: var0 {self.var0!r} must be finite, and positive with the running z-score")

    @classmethod
    def design(cls, fs: float = 125.0, highpass: Optional[float] = None, lowpass: Optional[float] = None, notch: Optional[float] = None,
               notch_q: float = 30.0, zscore_seconds: Optional[float] = None, var0: float = 1.0, baseline: bool = True,
               car: bool = False) -> "CausalPrep":
        """Sections formed in float64, in the order high-pass, low-pass, notch; corners in Hz at the sampling rate fs.
        High-pass / low-pass: the bilinear second-order Butterworth section (scipy.signal.butter(2, fc, fs=fs)).
        Notch: scipy.signal.iirnotch's formula -- w0 = 2 pi f0 / fs, beta = tan(w0 / (2 Q)), g = 1 / (1 + beta),
        b = g (1, -2 cos w0, 1), a = (1, -2 g cos w0, 2 g - 1).  zscore_seconds: alpha = 1 / (zscore_seconds * fs)."""
        secs = []
        if highpass is not None:
            secs.append(_butter2("highpass", float(highpass), float(fs)))
        if lowpass is not None:
            secs.append(_butter2("lowpass", float(lowpass), float(fs)))
        if notch is not None:
            secs.append(_notch(float(notch), float(notch_q), float(fs)))
        alpha = 0.0
        if zscore_seconds is not None:
            if not zscore_seconds * fs > 1.0:
                raise ValueError(f"CausalPrep.design: zscore_seconds {zscore_seconds!r} must span more than one sample")
            alpha = 1.0 / (float(zscore_seconds) * float(fs))
        return cls(sections=tuple(secs), alpha=alpha, var0=float(var0), baseline=bool(baseline), car=bool(car))

    @property
    def flags(self) -> int:
        return (_lib.NSD_PREP_BASELINE if self.baseline else 0) | (_lib.NSD_PREP_CAR if self.car else 0)

    def struct(self) -> "_lib.Prep":
        """nsd_prep: the coefficients rounded to fp32"""
        p = _lib.Prep(self.flags, len(self.sections))
        for s, sec in enumerate(self.sections):
            for k, v in enumerate(sec):
                p.sos[s][k] = v
        p.alpha, p.var0 = self.alpha, self.var0
        return p

    def filtered(self, windows) -> np.ndarray:
        """Host float64: windows [B,T,C] (or [T,C]) through baseline, common average and the sections (fp32-rounded coefficients), each
        window from rest -- everything in front of the running z-score."""
        x = np.asarray(windows, np.float64)
        x = x[None] if x.ndim == 2 else x
        if x.ndim != 3:
            raise ValueError(f"CausalPrep: windows must be [B,T,C] or [T,C], got {x.shape}")
        v = x - x[:, :1] if self.baseline else x.copy()
        if self.car:
            v = v - v.mean(axis=2, keepdims=True)
        for sec in self.sections:
            b0, b1, b2, a1, a2 = (float(np.float32(c)) for c in sec)
            z1, z2 = np.zeros_like(v[:, 0]), np.zeros_like(v[:, 0])
            for t in range(v.shape[1]):
                u = v[:, t].copy()
                y = b0 * u + z1
                z1 = (b1 * u - a1 * y) + z2
                z2 = b2 * u - a2 * y
                v[:, t] = y
        return v

    def calibrate(self, windows) -> "CausalPrep":
        """A copy whose var0 is the mean variance of the filtered windows (over time, averaged over windows and channels; host
        float64): the level the running variance starts from, so that the first samples of a stream are scaled like the rest."""
        v = self.filtered(windows)
        var0 = float(v.var(axis=1).mean())
        if not (math.isfinite(var0) and var0 > 0):
            raise ValueError(f"CausalPrep.calibrate: the filtered windows have variance {var0!r}")
        return replace(self, var0=float(np.float32(var0)))

    def to_dict(self) -> dict:
        return {"sections": [list(s) for s in self.sections], "alpha": float(self.alpha), "var0": float(self.var0),
                "baseline": bool(self.baseline), "car": bool(self.car)}

    @classmethod
    def from_dict(cls, d: dict) -> "CausalPrep":
        return cls(sections=tuple(tuple(s) for s in d.get("sections", ())), alpha=float(d.get("alpha", 0.0)), var0=float(d.get("var0", 1.0)),
                   baseline=bool(d.get("baseline", True)), car=bool(d.get("car", False)))
