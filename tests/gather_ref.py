"""nsd_gather restated in numpy (include/nsd.h): the row rule, the bitwise copy and the NaN rows.  All data travels as uint32 words, so
NaN payloads and signed zeros are compared as bits."""
from __future__ import annotations

from typing import Optional

import numpy as np

NAN32 = np.uint32(0x7FC00000)


def row(c: int, step_base: int, S: int) -> int:
    """r = (c - step_base) mod S, taken non-negative (python's % on ints is that)"""
    return (int(c) - int(step_base)) % int(S)


def gather(x_all: np.ndarray, table: np.ndarray, c: int, step_base: int = 0, labels_all: Optional[np.ndarray] = None,
           targets_all: Optional[np.ndarray] = None, x: Optional[np.ndarray] = None, labels: Optional[np.ndarray] = None,
           targets: Optional[np.ndarray] = None, status: Optional[np.ndarray] = None):
    """x_all [N,T,C] fp32, table int32 [M,S,B], c the counter -> (x [M,B,T,C] as uint32 words, labels int32 [M*B] or None, targets
    [M*B,K] as uint32 words or None, status int32 [M]).  x / labels / targets / status: what the outputs held before the call (a copy
    is updated; B = 0 leaves them as they were)."""
    N, T, Cc = x_all.shape
    M, S, B = table.shape
    r = row(c, step_base, S)
    xa = np.ascontiguousarray(x_all, dtype=np.float32).view(np.uint32)
    xo = np.zeros((M, B, T, Cc), np.uint32) if x is None else np.ascontiguousarray(x).view(np.uint32).reshape(M, B, T, Cc).copy()
    lo = to = None
    if labels_all is not None:
        lo = np.zeros(M * B, np.int32) if labels is None else np.asarray(labels, np.int32).reshape(-1).copy()
    if targets_all is not None:
        K = targets_all.shape[1]
        ta = np.ascontiguousarray(targets_all, dtype=np.float32).view(np.uint32)
        to = np.zeros((M * B, K), np.uint32) if targets is None else np.ascontiguousarray(targets).view(np.uint32).reshape(M * B, K).copy()
    st = np.zeros(M, np.int32) if status is None else np.asarray(status, np.int32).copy()
    for m in range(M):
        for b in range(B):
            i = int(table[m, r, b])
            ok = 0 <= i < N
            xo[m, b] = xa[i] if ok else NAN32
            if lo is not None:
                lo[m * B + b] = labels_all[i] if ok else 0
            if to is not None:
                to[m * B + b] = ta[i] if ok else NAN32
            if not ok:
                st[m] |= 1
    return xo, lo, to, st
