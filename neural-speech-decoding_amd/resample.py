"""The configuration of the rate converter (nsd_resample of include/nsd.h, csrc/nsd_resample.hip): stage 0 of the front end, which
brings a stream at any amplifier rate to the rate the models were trained at.  Host side only: the prototype filter is designed here in
float64 and handed to the kernel as an fp32 polyphase table [L][P]; ops.resample_step / ops.resample_trials run it.

An extension: the reference's board and every recorded trial run at 125 Hz, and nothing in it converts a rate.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

MAX_RATIO, MAX_TAPS_PER_PHASE, MAX_TAPS = 1024, 256, 65536      # the ranges of nsd_resample_step


@dataclass(frozen=True, eq=False)
class Resample:
    """A causal polyphase FIR rate converter: out / in rate = L / M (reduced), P taps per phase, taps float32 [L][P] with
    taps[ph][i] = h[ph + i*L] of the prototype filter h.  Output j is sum_i taps[(j*M) % L][i] * x[(j*M) // L - i], in fp32, in that
    order (include/nsd.h has the arithmetic)."""
    L: int
    M: int
    P: int
    taps: np.ndarray

    def __post_init__(self):
        L, M, P = int(self.L), int(self.M), int(self.P)
        object.__setattr__(self, "L", L)
        object.__setattr__(self, "M", M)
        object.__setattr__(self, "P", P)
        if not (1 <= L <= MAX_RATIO and 1 <= M <= MAX_RATIO):
            raise ValueError(f"Resample: L / M = {L} / {M} outside [1, {MAX_RATIO}]")
        if math.gcd(L, M) != 1:
            raise ValueError(f"Resample: L / M = {L} / {M} is not reduced")
        if not 1 <= P <= MAX_TAPS_PER_PHASE or L * P > MAX_TAPS:
            raise ValueError(f"Resample: P = {P} taps per phase outside [1, {MAX_TAPS_PER_PHASE}], or L * P = {L * P} > {MAX_TAPS}")
        taps = np.ascontiguousarray(np.asarray(self.taps, dtype=np.float32))
        if taps.shape != (L, P):
            raise ValueError(f"Resample: taps of shape {taps.shape}, expected [L][P] = {(L, P)}")
        if not np.isfinite(taps).all():
            raise ValueError("Resample: a tap is not finite")
        taps.setflags(write=False)
        object.__setattr__(self, "taps", taps)
        object.__setattr__(self, "_device", {})

    # (the table is an array: equality and the hash are spelled out)
    def __eq__(self, other):
        return (isinstance(other, Resample) and (self.L, self.M, self.P) == (other.L, other.M, other.P)
                and np.array_equal(self.taps.view(np.uint32), other.taps.view(np.uint32)))

    def __hash__(self):
        return hash((self.L, self.M, self.P, self.taps.tobytes()))

    @classmethod
    def from_prototype(cls, h, L: int, M: int) -> "Resample":
        """The polyphase table of a prototype filter h at the L-fold rate, zero-padded to a multiple of L."""
        h = np.asarray(h, np.float64).ravel()
        P = max(1, -(-len(h) // int(L)))
        hp = np.zeros(P * int(L), np.float64)
        hp[:len(h)] = h
        return cls(L=L, M=M, P=P, taps=hp.reshape(P, int(L)).T.astype(np.float32))

    @classmethod
    def design(cls, fs_in: float, fs_out: float, zeros: int = 10, beta: float = 8.6, rolloff: float = 0.9) -> "Resample":
        """A Kaiser-windowed sinc in float64: L / M = the reduced fraction fs_out / fs_in, half = ceil(zeros * max(L, M) / rolloff),
        N = 2 half + 1 taps at k = -half .. half, fc = rolloff / max(L, M), h = L fc sinc(fc k) kaiser(N, beta).  The group delay is
        half / M output samples (about 11 at the defaults)."""
        fr = Fraction(fs_out).limit_denominator(1 << 20) / Fraction(fs_in).limit_denominator(1 << 20)
        L, M = fr.numerator, fr.denominator
        if not (fs_in > 0 and fs_out > 0) or max(L, M) > MAX_RATIO:
            raise ValueError(f"Resample.design: {fs_in!r} Hz -> {fs_out!r} Hz is L / M = {L} / {M}, outside [1, {MAX_RATIO}]")
        if not (zeros >= 1 and 0.0 < rolloff <= 1.0):
            raise ValueError(f"Resample.design: zeros = {zeros!r} (>= 1), rolloff = {rolloff!r} (in (0, 1])")
        q = max(L, M)
        half = int(math.ceil(zeros * q / rolloff))
        N = 2 * half + 1
        k = np.arange(N, dtype=np.float64) - half
        fc = rolloff / q
        h = L * fc * np.sinc(fc * k) * np.kaiser(N, beta)
        return cls.from_prototype(h, L, M)

    @property
    def delay(self) -> float:
        """The group delay in output samples: the prototype's centre of mass over M (design()'s filters: half / M)."""
        return self.prototype_delay() / self.M

    def prototype_delay(self) -> float:
        """The centre of mass of the prototype filter in samples at the L-fold rate (half, for design()'s filters)."""
        h = self.prototype()
        return float((np.arange(len(h)) * h).sum() / h.sum())

    def prototype(self) -> np.ndarray:
        """The prototype filter h[ph + i*L] = taps[ph][i] in float64 (zero padding included)."""
        return self.taps.astype(np.float64).T.reshape(-1)

    def out_steps(self, n_in: int, T: int) -> int:
        """Outputs a push of T samples emits from a stream that holds n_in: ceil((n_in+T) L / M) - ceil(n_in L / M)."""
        return -((-(int(n_in) + int(T)) * self.L) // self.M) - -((-int(n_in) * self.L) // self.M)

    def struct(self):
        from . import _lib
        return _lib.Resample(self.L, self.M, self.P)

    def device_taps(self, device):
        """The table on `device` (cached per device)."""
        import torch
        key = str(torch.device(device))
        t = self._device.get(key)
        if t is None:
            t = self._device[key] = torch.from_numpy(self.taps.copy()).to(device)
        return t

    def to_dict(self) -> dict:
        return {"L": self.L, "M": self.M, "P": self.P, "taps": [[float(v) for v in row] for row in self.taps]}

    @classmethod
    def from_dict(cls, d: dict) -> "Resample":
        return cls(L=int(d["L"]), M=int(d["M"]), P=int(d["P"]), taps=np.asarray(d["taps"], np.float32))
