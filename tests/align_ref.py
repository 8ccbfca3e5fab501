"""Numpy restatements of session alignment (nsd_cov_step / nsd_whiten_fit / nsd_spatial_apply of include/nsd.h) for the tests, written
sample by sample from the header's words and kept apart from the package's own (nsd_amd.align), which the CPU tests hold against these.

  cov_ref      the second-moment accumulator: one serial chain per (i, j) in double, exact products -- bit for bit
  whiten_ref   S -> R -> R' -> float64 eigh -> clip -> W, rounded once to fp32, and the record
  apply_ref    out[i] = ((W[i][0]*v[0] + W[i][1]*v[1]) + ...) with every fp32 operation rounding on its own -- bit for bit
  constructed  the accumulators of the fit tests: n * Q diag(lambda) Q^T with a chosen condition number, symmetric bit for bit
"""
import numpy as np

FEW, NONFINITE, CLIPPED, NOT_CONVERGED = 1, 2, 4, 8
RECORD_BYTES = 64


def cov_ref(v, mask=None, sums=None, counts=None):
    """v [B,T,C] fp32, mask [B,T] uint32 or None; sums [B,C,C] float64 / counts [B,2] int64 to continue from (updated copies are
    returned) -> (sums, counts)"""
    v = np.asarray(v, np.float32)
    B, T, C = v.shape
    sums = np.zeros((B, C, C), np.float64) if sums is None else np.array(sums, np.float64)
    counts = np.zeros((B, 2), np.int64) if counts is None else np.array(counts, np.int64)
    for b in range(B):
        for t in range(T):
            row = v[b, t]
            if np.isfinite(row).all() and (mask is None or int(mask[b, t]) == 0):
                d = row.astype(np.float64)
                sums[b] = sums[b] + np.outer(d, d)             # (the product of two fp32 values is exact in double)
                counts[b, 0] += 1
            else:
                counts[b, 1] += 1
    return sums, counts


def whiten_ref(sums, counts, shrinkage=0.0, floor=1e-4, min_steps=1, groups=None, G=1):
    """sums [N,C,C] float64, counts [N,2] int64 -> (W [G,C,C] fp32, records: G dicts)"""
    sums, counts = np.asarray(sums, np.float64), np.asarray(counts, np.int64)
    N, C = sums.shape[0], sums.shape[-1]
    groups = np.zeros(N, np.int64) if groups is None else np.asarray(groups, np.int64)
    shrinkage, floor = float(np.float32(shrinkage)), float(np.float32(floor))
    W, recs = np.zeros((G, C, C), np.float32), []
    ignored = int(sum(1 for g in groups if not 0 <= g < G))
    for g in range(G):
        S, n, skipped, nacc = np.zeros((C, C)), 0, 0, 0
        for a in range(N):
            if groups[a] == g:
                S, n, skipped, nacc = S + sums[a], n + int(counts[a, 0]), skipped + int(counts[a, 1]), nacc + 1
        rec = dict(steps=n, skipped=skipped, trace_mean=0.0, eig_min=0.0, eig_max=0.0, status=0, accumulators=nacc, ignored=ignored)
        W[g] = np.eye(C, dtype=np.float32)
        if n < min_steps:
            rec["status"] = FEW
        elif not np.isfinite(S).all() or not np.trace(S) > 0:
            rec["status"] = NONFINITE
        else:
            R = S / n
            tm = np.trace(R) / C
            Rp = (1.0 - shrinkage) * R + shrinkage * tm * np.eye(C)
            lam, V = np.linalg.eigh(Rp)
            thr = floor * lam[-1]
            if lam[0] < thr:
                rec["status"] = CLIPPED
            Wd = (V / np.sqrt(np.maximum(lam, thr))) @ V.T
            W[g] = (0.5 * (Wd + Wd.T)).astype(np.float32)
            rec.update(trace_mean=tm, eig_min=lam[0], eig_max=lam[-1])
        recs.append(rec)
    return W, recs


def apply_ref(v, W, sel=None):
    """v [B,T,C], W [n_mat,C,C] (or [C,C]) fp32, sel None or [B] -> out [B,T,C] fp32"""
    v, W = np.asarray(v, np.float32), np.asarray(W, np.float32)
    W = W[None] if W.ndim == 2 else W
    B, T, C = v.shape
    out = np.empty_like(v)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            m = 0 if sel is None else int(sel[b])
            if not 0 <= m < W.shape[0]:
                out[b] = np.nan
                continue
            acc = W[m][None, :, 0] * v[b][:, None, 0]           # [T,C] fp32: one rounding per product
            for j in range(1, C):
                acc = acc + W[m][None, :, j] * v[b][:, None, j]  # one per product, one per sum
            out[b] = acc
    return out


def constructed(C, cond, seed, n=4096):
    """One accumulator whose R = S / n has eigenvalues log-spaced over [1 / cond, 1] times a scale of EEG size in a random orthogonal
    basis -> (sums [C,C] float64, symmetric bit for bit; counts [2] int64: n used, 3 skipped)"""
    rs = np.random.RandomState(seed + 131 * C + int(np.log10(cond)))
    Q, _ = np.linalg.qr(rs.standard_normal((C, C)))
    lam = 25.0 * np.logspace(0.0, -np.log10(cond), C) if C > 1 else np.array([25.0])
    R = (Q * lam) @ Q.T
    S = 0.5 * (R + R.T) * n
    return S, np.array([n, 3], np.int64)


def same_bits(a, b):
    """equal shapes, dtypes and bit patterns, except that a NaN matches any NaN at the same place"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    ua = a.view(np.uint32 if a.dtype == np.float32 else np.uint64)
    ub = b.view(ua.dtype)
    return bool(((ua == ub) | (np.isnan(a) & np.isnan(b))).all())
