"""Helpers that hold a launch to the buffer promises of include/nsd.h ("the CALLER owns every buffer"): nothing outside the stated extent
of an output or workspace is written, nothing the caller left in them beforehand shows in a result, inputs stay as they were.  Used by
tests/test_buffer_contract_cpu.py (the helpers themselves, on CPU tensors) and tests/test_gpu_buffer_contract.py (the library).

  guarded(shape, dtype, device, fill)  one allocation [guard | payload | guard]; the guards hold the byte 0xA5 and are as long as the larger
                                       of 4 KiB and one leading-dimension slice of the payload (one trial's row), rounded up to 256 bytes,
                                       so the payload keeps a 256-byte aligned pointer.  torch's caching allocator rounds an allocation up
                                       to 512 bytes and hands out neighbours of the same pool: a row spilled past a plain tensor lands in
                                       slack or in another test's buffer and nobody sees it; here it lands in a guard.
                                       -> (payload view, check); check() raises, naming the first changed byte and its side.
  FILLS                                what the payload holds before the call, as bit patterns (see fill_payload)
  snapshot(*tensors).unchanged()       bitwise immutability of inputs
  Arena                                the named buffers of one evaluation of a route, all guarded with one fill; with fill "stale" each
                                       buffer lies inside the allocation an earlier, larger evaluation used under the same name, at the
                                       same payload address, and keeps what that evaluation left there
  *_bytes                              the exact sizes nsd_workspace_bytes & co. return (a workspace is never rounded up here)
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import torch

GUARD_BYTE = 0xA5
GUARD_MIN = 4096
ALIGN = 256
# zeros: every bf16 half has the ring slots' step tag (bit 14) clear.  ones: 0xFF bytes -- every half has bit 14 set and is a NaN, as
# fp32 and as bf16.  nan32: 0x7FC00000 per word -- asymmetric: the high half is a NaN with bit 14 set, the low half zero.  stale: what
# an earlier complete evaluation of the same route (larger shape, other parameters) left in the same allocation.
FILLS = ("zeros", "ones", "nan32", "stale")
NAN32 = 0x7FC00000


def _round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def guard_bytes(shape, dtype) -> int:
    """larger of 4 KiB and one leading-dimension slice of the payload, rounded up to a multiple of 256 bytes"""
    row = torch.empty(0, dtype=dtype).element_size()
    for v in tuple(shape)[1:]:
        row *= int(v)
    return _round_up(max(GUARD_MIN, row), ALIGN)


def fill_payload(raw: torch.Tensor, fill: str) -> None:
    """raw: the payload as a 1-D uint8 view.  "stale" leaves it as it is."""
    if fill == "zeros":
        raw.zero_()
    elif fill == "ones":
        raw.fill_(0xFF)
    elif fill == "nan32":
        n = raw.numel()
        word = torch.tensor([NAN32 & 0xFF, (NAN32 >> 8) & 0xFF, (NAN32 >> 16) & 0xFF, NAN32 >> 24], dtype=torch.uint8, device=raw.device)
        raw.copy_(word.repeat((n + 3) // 4)[:n])                  # little-endian words; a tail shorter than a word takes their first bytes
    elif fill != "stale":
        raise ValueError(f"unknown fill {fill!r}: one of {FILLS}")


class Guarded:
    """[guard | payload | guard] in one uint8 allocation.  within: an earlier Guarded whose allocation and payload address this one
    takes over (its extent must cover this one's guards); the payload is then left as that one's user left it unless `fill` says
    otherwise."""

    def __init__(self, shape, dtype, device, fill: str = "zeros", within: Optional["Guarded"] = None):
        if fill not in FILLS:
            raise ValueError(f"unknown fill {fill!r}: one of {FILLS}")
        if fill == "stale" and within is None:
            raise ValueError("fill 'stale' needs the allocation of the earlier evaluation (within=)")
        self.shape, self.dtype = tuple(int(v) for v in shape), dtype
        n = torch.empty(0, dtype=dtype).element_size()
        for v in self.shape:
            n *= v
        self.nbytes, self.guard = n, guard_bytes(self.shape, dtype)
        if within is None:
            store = torch.empty(2 * self.guard + n + ALIGN, dtype=torch.uint8, device=device)
            self.store, self.off = store, (-store.data_ptr()) % ALIGN + self.guard
        else:
            self.store, self.off = within.store, within.off
            lo, hi = within.off - within.guard, within.off + within.nbytes + within.guard
            if self.off - self.guard < lo or self.off + n + self.guard > hi:
                raise ValueError(f"{self.shape} with guards of {self.guard} bytes does not fit the earlier allocation "
                                 f"({within.shape}, guards of {within.guard} bytes)")
        raw = self.store[self.off:self.off + n]
        fill_payload(raw, fill)
        self.store[self.off - self.guard:self.off].fill_(GUARD_BYTE)
        self.store[self.off + n:self.off + n + self.guard].fill_(GUARD_BYTE)
        self.payload = raw.view(dtype).view(self.shape)
        assert self.payload.is_contiguous() and (n == 0 or self.payload.data_ptr() % ALIGN == 0)

    def violation(self) -> Optional[Tuple[str, int]]:
        """None, or (side, offset) of the first changed guard byte: side "before" with offset < 0 or "after" with offset >= nbytes,
        both in bytes from the payload's first byte"""
        for side, lo in (("before", self.off - self.guard), ("after", self.off + self.nbytes)):
            bad = (self.store[lo:lo + self.guard] != GUARD_BYTE).nonzero()
            if bad.numel():
                return side, lo + int(bad[0, 0]) - self.off
        return None

    def check(self, name: str = "buffer") -> None:
        v = self.violation()
        if v is not None:
            side, at = v
            where = f"{-at} bytes before its first byte" if side == "before" else f"{at - self.nbytes} bytes past its last byte (offset {at})"
            raise AssertionError(f"{name} {self.shape} {self.dtype}: written outside the payload of {self.nbytes} bytes, {side} it: "
                                 f"first changed byte {where}")


def guarded(shape, dtype, device, fill: str = "zeros"):
    """-> (contiguous payload view of `shape`, check)"""
    g = Guarded(shape, dtype, device, fill)
    return g.payload, g.check


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().view(-1).view(torch.uint8).clone()


class Snapshot:
    def __init__(self, tensors):
        self.tensors = [t for t in tensors if t is not None]
        self.bits = [_bits(t) for t in self.tensors]

    def changed(self):
        """indices (in the order given, None left out) of the tensors whose bits differ from the snapshot"""
        return [i for i, (t, b) in enumerate(zip(self.tensors, self.bits)) if not torch.equal(_bits(t), b)]

    def unchanged(self) -> bool:
        return not self.changed()


def snapshot(*tensors) -> Snapshot:
    return Snapshot(tensors)


class Arena:
    """The caller-owned outputs and workspaces of one evaluation, by name, every one guarded and pre-filled.  prior: the Arena of the
    earlier evaluation whose allocations fill "stale" takes over.  A second request for a name returns the same buffer untouched (a
    captured launch sequence runs twice on one set of buffers)."""

    def __init__(self, device, fill: str, prior: Optional["Arena"] = None):
        self.device, self.fill, self.prior, self.bufs = device, fill, prior, {}          # type: Dict[str, Guarded]

    def buf(self, name: str, shape, dtype=torch.float32) -> torch.Tensor:
        shape = tuple(int(v) for v in shape)
        if name in self.bufs:
            g = self.bufs[name]
            assert g.shape == shape and g.dtype == dtype, (name, g.shape, shape)
            return g.payload
        within = self.prior.bufs[name] if self.fill == "stale" else None
        self.bufs[name] = g = Guarded(shape, dtype, self.device, self.fill, within)
        return g.payload

    def check(self) -> None:
        for name, g in self.bufs.items():
            g.check(name)


# ---- exact sizes -------------------------------------------------------------------------------------------------------------------
def workspace_bytes(spec, B: int, T: int) -> int:
    from nsd_amd import ops
    return ops.workspace_layout(spec, B, T)[0]


def multi_workspace_bytes(spec, M: int, B: int, T: int) -> int:
    from nsd_amd import _lib
    d, w = spec.dims(B, T), _lib.WsLayout()
    n = int(_lib.lib().nsd_multi_workspace_bytes(C.byref(d), int(M), C.byref(w)))
    assert n > 0, n
    return n


def seq_workspace_bytes(spec, B: int, T: int) -> int:
    from nsd_amd import _lib
    d = spec.dims(B, T)
    n = int(_lib.lib().nsd_seq_workspace_bytes(C.byref(d), spec.seq_flags))
    assert n > 0, n
    return n


def infer_scratch_bytes(spec, B: int, T: int) -> int:
    from nsd_amd import _lib
    d = spec.dims(B, T)
    n = int(_lib.lib().nsd_infer_scratch_bytes(C.byref(d)))
    assert n >= 0, n
    return n


def multi_infer_scratch_bytes(spec, M: int, B: int, T: int) -> int:
    from nsd_amd import _lib
    d = spec.dims(B, T)
    n = int(_lib.lib().nsd_multi_infer_scratch_bytes(C.byref(d), int(M)))
    assert n >= 0, n
    return n
