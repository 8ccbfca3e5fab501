"""Numpy restatements of the supervised session alignment (nsd_spatial_bwd / nsd_spatial_fit_step of include/nsd.h) for the tests,
written from the header's words and kept apart from the package's own.

  bwd_ref      dv: out[j] = ((W[0][j]*dy[0] + W[1][j]*dy[1]) + ...) with every fp32 operation rounding on its own -- bit for bit;
               dW: p[b][i][j] one serial double chain over t (exact products), then one serial double chain over the rows b with
               sel[b] == m, rounded once to fp32 -- bit for bit;  counts {rows used, rows left out}
  FitRef       nsd_spatial_fit_step's state and arithmetic: g = dW + decay * (A - A0) in fp32, then nsd_adam_step's operations in their
               order with the bias corrections in double (the power by repeated squaring) -- bit for bit
"""
import numpy as np

NONFINITE = 1
F32 = np.float32


def bwd_ref(v, dy, W, sel=None):
    """v, dy [B,T,C], W [n_mat,C,C] (or [C,C]) fp32, sel None or [B] -> (dv [B,T,C] fp32, dW [n_mat,C,C] fp32, counts [2] int64)"""
    v, dy, W = np.asarray(v, F32), np.asarray(dy, F32), np.asarray(W, F32)
    W = W[None] if W.ndim == 2 else W
    B, T, C = v.shape
    n_mat = W.shape[0]
    dv = np.empty_like(v)
    p = np.zeros((B, C, C), np.float64)
    acc = np.zeros((n_mat, C, C), np.float64)
    used = left = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            m = 0 if sel is None else int(sel[b])
            if not 0 <= m < n_mat:
                dv[b] = np.nan
                left += 1
                continue
            used += 1
            a = W[m][None, 0, :] * dy[b][:, 0, None]               # [T,C] over j: W[0][j] * dy[t,0], one rounding per product
            for i in range(1, C):
                a = a + W[m][None, i, :] * dy[b][:, i, None]       # one per product, one per sum
            dv[b] = a
            y64, x64 = dy[b].astype(np.float64), v[b].astype(np.float64)
            for t in range(T):                                     # (the product of two fp32 values is exact in double)
                p[b] = p[b] + y64[t][:, None] * x64[t][None, :]
            acc[m] = acc[m] + p[b]
        dW = acc.astype(F32)
    return dv, dW, np.array([used, left], np.int64)


def pow_int(b, s):
    """b^s by squaring, in double: the products the kernel takes"""
    b, r, s = np.float64(b), np.float64(1.0), int(s)
    while s:
        if s & 1:
            r = r * b
        b = b * b
        s >>= 1
    return r


class FitRef:
    """The state of nsd_spatial_fit_step for n_mat matrices of C x C, and step()."""

    def __init__(self, C, n_mat=1):
        self.C, self.n_mat = int(C), int(n_mat)
        self.m = np.zeros((n_mat, C, C), F32)
        self.v = np.zeros((n_mat, C, C), F32)
        self.step_count = np.zeros(n_mat, np.int64)
        self.skipped = np.zeros(n_mat, np.int64)
        self.status = np.zeros(n_mat, np.uint32)
        self.calls = 0

    def step(self, A, dW, A0=None, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, decay=0.0, loss_in=None, loss_out=None):
        """A [n_mat,C,C] fp32 is updated in place (and returned); loss_out (a numpy array) takes loss_in at the call's index"""
        A = np.asarray(A)
        assert A.dtype == F32 and A.shape == self.m.shape
        dW = np.asarray(dW, F32).reshape(A.shape)
        lr, b1, b2, eps, decay = F32(lr), F32(beta1), F32(beta2), F32(eps), F32(decay)
        if loss_in is not None and self.calls < len(loss_out):
            loss_out[self.calls] = F32(loss_in)
        self.calls += 1
        one = F32(1.0)
        with np.errstate(invalid="ignore", over="ignore"):
            for k in range(self.n_mat):
                g = dW[k] if A0 is None else (dW[k] + decay * (A[k] - np.asarray(A0, F32).reshape(A.shape)[k])).astype(F32)
                if not np.isfinite(g).all():
                    self.status[k] |= NONFINITE
                    self.skipped[k] += 1
                    continue
                s = int(self.step_count[k]) + 1
                bc1, bc2 = np.float64(1.0) - pow_int(b1, s), np.float64(1.0) - pow_int(b2, s)
                lr_over_bc1, rsqrt_bc2 = F32(np.float64(lr) / bc1), F32(np.float64(1.0) / np.sqrt(bc2))
                mi = b1 * self.m[k] + (one - b1) * g
                vi = b2 * self.v[k] + ((one - b2) * g) * g
                self.m[k], self.v[k] = mi, vi
                denom = np.sqrt(vi) * rsqrt_bc2 + eps
                A[k] = A[k] - lr_over_bc1 * (mi / denom)
                self.step_count[k] = s
        return A


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
