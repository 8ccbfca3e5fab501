"""The numpy float32 restatement of the rate converter's definition (include/nsd.h, "rate conversion"): for one stream, output j has
p = j*M, ph = p mod L, q = p div L and y[j] = (((+0 + taps[ph][0]*xa[q]) + taps[ph][1]*xa[q-1]) + ...) over the P taps in ascending
order, every product and every sum rounded to float32 on its own; xa[k] = 0 before the slot's reset.  A call that adds T samples to a
slot holding n_in emits j in [ceil(n_in L / M), ceil((n_in + T) L / M)).  The state is the last P - 1 samples, chronological, and n_in.

Shared by tests/test_resample_cpu.py and tests/test_gpu_resample.py; nothing here touches the library under test.
"""
from __future__ import annotations

import numpy as np


def ceil_div(a: int, b: int) -> int:
    return -((-int(a)) // int(b))


def out_steps(L: int, M: int, n_in: int, T: int) -> int:
    return ceil_div((n_in + T) * L, M) - ceil_div(n_in * L, M)


def step(x, taps, L: int, M: int, n_in: int = 0, hist=None):
    """One stream's chunk x [T,C] (float32) on top of a slot (n_in, hist [P-1,C]; None: a reset slot)
    -> (y [cnt,C] float32, cnt, n_in + T, the new hist [P-1,C])."""
    x = np.asarray(x, np.float32)
    taps = np.asarray(taps, np.float32)
    assert taps.ndim == 2 and taps.shape[0] == L and x.ndim == 2
    P, (T, C) = taps.shape[1], x.shape
    hist = np.zeros((P - 1, C), np.float32) if hist is None else np.asarray(hist, np.float32)
    assert hist.shape == (P - 1, C)
    ext = np.concatenate([hist, x], axis=0)                    # ext[P-1 + (k - n_in)] = xa[k]
    j = np.arange(ceil_div(n_in * L, M), ceil_div((n_in + T) * L, M), dtype=np.int64)
    p = j * M
    ph, q = p % L, p // L
    assert len(j) == 0 or (q.min() >= n_in and q.max() <= n_in + T - 1)
    row = (P - 1) + (q - n_in)
    acc = np.zeros((len(j), C), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(P):
            acc = acc + taps[ph, i][:, None] * ext[row - i]   # float32 product, float32 sum: one rounding each
    assert acc.dtype == np.float32
    return acc, len(j), n_in + T, ext[len(ext) - (P - 1):].copy() if P > 1 else np.zeros((0, C), np.float32)


def step_batch(x, taps, L: int, M: int, To: int, n_in=None, hist=None):
    """Streams x [B,T,C] with per-stream n_in [B] and hist [B,P-1,C] -> (y [B,To,C] with NaN behind each row's outputs, cnt [B] int32,
    n_in' [B] int64, hist' [B,P-1,C]): what nsd_resample_step leaves."""
    x = np.asarray(x, np.float32)
    B, T, C = x.shape
    P = np.asarray(taps).shape[1]
    n_in = np.zeros(B, np.int64) if n_in is None else np.asarray(n_in, np.int64)
    hist = np.zeros((B, P - 1, C), np.float32) if hist is None else np.asarray(hist, np.float32)
    y = np.full((B, To, C), np.nan, np.float32)
    cnt, n_out, h_out = np.zeros(B, np.int32), n_in.copy(), hist.copy()
    for b in range(B):
        yb, cnt[b], n_out[b], h_out[b] = step(x[b], taps, L, M, int(n_in[b]), hist[b])
        y[b, :cnt[b]] = yb
    return y, cnt, n_out, h_out


def trials(x, taps, L: int, M: int):
    """Window mode: whole trials x [B,T,C], each from rest -> [B, ceil(T L / M), C]."""
    x = np.asarray(x, np.float32)
    return step_batch(x, taps, L, M, ceil_div(x.shape[1] * L, M))[0]


def state_words(n_in, hist, layout_n_in: int, stride: int):
    """The slots' image in 4-byte words, as nsd_resample_state_layout lays them out: hist flat from word 0, the int64 n_in at word
    `layout_n_in`, zeros elsewhere -> uint32 [B, stride]."""
    hist = np.asarray(hist, np.float32)
    B = hist.shape[0]
    w = np.zeros((B, stride), np.uint32)
    flat = hist.reshape(B, -1)
    w[:, :flat.shape[1]] = flat.view(np.uint32)
    w[:, layout_n_in:layout_n_in + 2] = np.asarray(n_in, np.int64).reshape(B, 1).view(np.uint32)
    return w


def poisoned_outputs(L: int, M: int, P: int, n: int, n_total: int):
    """The outputs j (of a stream of n_total samples from rest) that a non-finite sample at index n makes non-finite: q in [n, n+P-1]."""
    j = np.arange(ceil_div(n_total * L, M), dtype=np.int64)
    q = (j * M) // L
    return j[(q >= n) & (q <= n + P - 1)]


def same_bits(a, b) -> bool:
    """Finite values bit for bit, NaNs by position."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(np.uint32)[~na] == b.view(np.uint32)[~nb]).all())
