"""The configuration of the signal-quality gate (nsd_gate of include/nsd.h, csrc/nsd_gate.hip): a causal per-channel detector of railed,
jumping, flat and high-amplitude spans that holds a bad channel through the front end, zeroes it in front of the model and turns a step
that is bad on too many channels into "no decision".  Host side only: ops.gate_step / ops.gate_apply run the kernels; `reference` is
the numpy restatement for host use.

An extension: the reference has no notion of a bad channel or an artefact.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import _lib

MAX_CHANNELS = 32                # one mask bit per channel


def _samples(seconds: float, fs: float) -> int:
    """seconds at the sampling rate fs, rounded to the nearest sample (halves up)"""
    return int(math.floor(float(seconds) * float(fs) + 0.5))


@dataclass(frozen=True)
class SignalGate:
    """The detectors of include/nsd.h, each off at 0: `rail` (|x| >= rail), `jump` (|x - prev| >= jump), `flat_samples` equal samples in
    a row (a pair is equal within `flat_eps`), `pp` peak to peak over the last `pp_samples` samples.  A channel stays bad for
    `hold_samples` samples after its last raw-bad one.  A step with more than `max_bad` bad channels is rejected (NaN in front of the
    model; max_bad >= C: never).  zero: a bad channel is 0 in front of the model, else its held value passes."""
    rail: float = 0.0
    jump: float = 0.0
    flat_eps: float = 0.0
    flat_samples: int = 0
    pp: float = 0.0
    pp_samples: int = 0
    hold_samples: int = 0
    max_bad: int = MAX_CHANNELS
    zero: bool = True

    def __post_init__(self):
        for name in ("rail", "jump", "flat_eps", "pp"):
            v = float(np.float32(getattr(self, name)))
            if not (math.isfinite(v) and v >= 0.0):
                raise ValueError(f"SignalGate: {name} {getattr(self, name)!r} must be finite and >= 0")
            object.__setattr__(self, name, v)
        for name in ("flat_samples", "pp_samples", "hold_samples", "max_bad"):
            v = getattr(self, name)
            if int(v) != v or int(v) < 0:
                raise ValueError(f"SignalGate: {name} {v!r} must be an integer >= 0")
            object.__setattr__(self, name, int(v))
        if self.pp_samples > _lib.NSD_GATE_MAX_SPAN:
            raise ValueError(f"SignalGate: pp_samples {self.pp_samples} outside [0, {_lib.NSD_GATE_MAX_SPAN}]")
        object.__setattr__(self, "zero", bool(self.zero))

    @classmethod
    def design(cls, fs: float = 125.0, rail: Optional[float] = None, jump: Optional[float] = None, flat_seconds: Optional[float] = None,
               flat_eps: float = 0.0, pp: Optional[float] = None, pp_seconds: float = 0.5, hold_seconds: float = 0.0,
               max_bad_channels: Optional[int] = None, zero: bool = True) -> "SignalGate":
        """Thresholds in the units of the samples, spans in seconds at the sampling rate fs, rounded to the nearest sample.  A detector
        left at None is off.  flat_seconds must span at least two samples, pp_seconds 1 .. 64 samples (0.5 s at 125 Hz: 63).
        max_bad_channels None: no step is ever rejected."""
        flat_samples = pp_samples = 0
        if flat_seconds is not None:
            flat_samples = _samples(flat_seconds, fs)
            if flat_samples < 2:
                raise ValueError(f"SignalGate.design: flat_seconds {flat_seconds!r} must span at least two samples at fs = {fs}")
        if pp is not None:
            pp_samples = _samples(pp_seconds, fs)
            if not 1 <= pp_samples <= _lib.NSD_GATE_MAX_SPAN:
                raise ValueError(f"SignalGate.design: pp_seconds {pp_seconds!r} is {pp_samples} samples at fs = {fs}, "
                                 f"outside [1, {_lib.NSD_GATE_MAX_SPAN}]")
        if hold_seconds < 0:
            raise ValueError(f"SignalGate.design: hold_seconds {hold_seconds!r} < 0")
        return cls(rail=0.0 if rail is None else float(rail), jump=0.0 if jump is None else float(jump), flat_eps=float(flat_eps),
                   flat_samples=flat_samples, pp=0.0 if pp is None else float(pp), pp_samples=pp_samples,
                   hold_samples=_samples(hold_seconds, fs), max_bad=MAX_CHANNELS if max_bad_channels is None else int(max_bad_channels),
                   zero=bool(zero))

    @property
    def flags(self) -> int:
        return _lib.NSD_GATE_ZERO if self.zero else 0

    def struct(self) -> "_lib.Gate":
        """nsd_gate: the thresholds as fp32"""
        return _lib.Gate(self.rail, self.jump, self.flat_eps, self.flat_samples, self.pp, self.pp_samples, self.hold_samples,
                         self.max_bad, self.flags)

    def to_dict(self) -> dict:
        return {"rail": self.rail, "jump": self.jump, "flat_eps": self.flat_eps, "flat_samples": self.flat_samples, "pp": self.pp,
                "pp_samples": self.pp_samples, "hold_samples": self.hold_samples, "max_bad": self.max_bad, "zero": self.zero}

    @classmethod
    def from_dict(cls, d: dict) -> "SignalGate":
        return cls(**{k: d[k] for k in ("rail", "jump", "flat_eps", "flat_samples", "pp", "pp_samples", "hold_samples", "max_bad", "zero")
                      if k in d})

    # ---- the numpy restatement, for host use ----
    def reference(self, windows) -> Tuple[np.ndarray, np.ndarray]:
        """Window mode on the host: windows [B,T,C] (or [T,C]) fp32, every window from a reset state -> (y [B,T,C] fp32, mask [B,T]
        uint32), bit for bit what nsd_gate_step writes."""
        x = np.asarray(windows, np.float32)
        x = x[None] if x.ndim == 2 else x
        if x.ndim != 3 or not 1 <= x.shape[2] <= MAX_CHANNELS:
            raise ValueError(f"SignalGate.reference: windows must be [B,T,C] or [T,C] with C in [1, {MAX_CHANNELS}], got {x.shape}")
        B, T, Cc = x.shape
        fin = np.isfinite(x)
        with np.errstate(invalid="ignore", over="ignore"):
            raw = ~fin
            if self.rail > 0:
                raw |= np.abs(x) >= np.float32(self.rail)
            d = np.abs(x[:, 1:] - x[:, :-1])                   # fp32: one rounding
            pair = fin[:, 1:] & fin[:, :-1]
            if self.jump > 0:
                raw[:, 1:] |= pair & (d >= np.float32(self.jump))
            if self.pp_samples > 0:
                hi, lo = np.where(fin, x, -np.inf).astype(np.float32), np.where(fin, x, np.inf).astype(np.float32)
                for t in range(T):
                    t0 = max(0, t - self.pp_samples + 1)
                    h, l = hi[:, t0:t + 1].max(axis=1), lo[:, t0:t + 1].min(axis=1)
                    raw[:, t] |= (h >= l) & ((h - l) >= np.float32(self.pp))
            flat = np.zeros((B, T, Cc), bool)
            if self.flat_samples > 0:
                flat[:, 1:] = pair & (d <= np.float32(self.flat_eps))
        y, mask = np.empty_like(x), np.zeros((B, T), np.uint32)
        held = np.zeros((B, Cc), np.float32)
        run, hang = np.zeros((B, Cc), np.int64), np.zeros((B, Cc), np.int64)
        weights = (np.uint32(1) << np.arange(Cc, dtype=np.uint32))
        for t in range(T):
            run = np.where(flat[:, t], np.minimum(run + 1, self.flat_samples), 0)
            r = raw[:, t] | ((run >= self.flat_samples - 1) if self.flat_samples > 0 else False)
            bad = r | (hang > 0)
            hang = np.where(r, self.hold_samples, np.maximum(hang - 1, 0))
            held = np.where(bad, held, x[:, t])
            y[:, t] = held
            mask[:, t] = (bad * weights).sum(axis=1, dtype=np.uint32)
        return y, mask

    def apply_reference(self, v, mask, max_bad: Optional[int] = None) -> np.ndarray:
        """The apply stage on the host: v [..., T, C] fp32 and mask [..., T] uint32 -> what nsd_gate_apply writes."""
        v, mask = np.asarray(v, np.float32), np.asarray(mask).astype(np.uint32)
        Cc = v.shape[-1]
        bits = ((mask[..., None] >> np.arange(Cc, dtype=np.uint32)) & 1).astype(bool)
        count = np.zeros(mask.shape, np.int64)
        for c in range(32):
            count += (mask >> np.uint32(c)) & 1
        out = v.copy()
        if self.zero:
            out[bits] = 0.0
        out[count > (self.max_bad if max_bad is None else int(max_bad))] = np.nan
        return out
