"""numpy restatement of nsd_mixup (include/nsd.h): the specification the kernel is held to bit for bit.

Every fp32 operation is a numpy float32 operation (one rounding each, no FMA), in the order the header writes down; the draws are
tests/augment_ref.py's port of nsd_rand_u32 on the stream nsd_augment uses (base_stream + 3), at index slots it leaves alone.
dtype=np.float64 runs the same formulas in double (the same draws: U is exact in either), for the comparison with torch."""
import numpy as np

from tests.augment_ref import AUG_STREAM, TRIAL_BIT, rand_u32, trial_index, unit

ROT_INDEX = TRIAL_BIT | (np.uint64(1) << np.uint64(62))      # 2^63 | 2^62: the rotation of a model's batch
LAMBDA_SLOT = 1024                                            # P(b, 1024): the trial's mixing weight
F1 = np.float32(1.0)


def partner(B: int, seed: int, base_stream: int) -> np.ndarray:
    """p(b) = (b + r) mod B, r = 1 + R(2^63 | 2^62) mod (B - 1): a rotation of the batch (B >= 2), never b itself; B = 1: itself"""
    if B < 2:
        return np.arange(B)
    r = 1 + int(rand_u32(seed, base_stream + AUG_STREAM, np.array([ROT_INDEX], dtype=np.uint64))[0]) % (B - 1)
    return (np.arange(B) + r) % B


def lambdas(B: int, mix: float, seed: int, base_stream: int, dtype=np.float32):
    """(lambda_b, mu_b) [B]: lambda = 1 - mix * U(R(P(b, 1024))), mu = 1 - lambda"""
    u = unit(rand_u32(seed, base_stream + AUG_STREAM, trial_index(np.arange(B), LAMBDA_SLOT))).astype(dtype)
    lam = dtype(1.0) - dtype(np.float32(mix)) * u
    return lam, dtype(1.0) - lam


def base_rows(labels: np.ndarray, K: int, eps: float = 0.0, weights=None, dtype=np.float32) -> np.ndarray:
    """base(label_b)[k] = w_k * (k == label_b ? (1 - eps) + eps / K : eps / K), [B, K]"""
    eps = dtype(np.float32(eps))
    ek = eps / dtype(K)
    on = (dtype(1.0) - eps) + ek
    rows = np.where(np.arange(K)[None, :] == np.asarray(labels)[:, None], on, ek).astype(dtype)
    if weights is not None:
        rows = np.asarray(weights, dtype=np.float32).astype(dtype)[None, :] * rows
    assert rows.dtype == dtype
    return rows


def mixup(x, labels: np.ndarray, K: int, seed: int, base_stream: int, mix: float = 0.0, eps: float = 0.0, weights=None, dtype=np.float32):
    """One model: x [B,T,C] float32 (or None with mix = 0), labels [B] -> (y [B,T,C] or None, targets [B,K])."""
    labels = np.asarray(labels)
    B = labels.shape[0]
    base = base_rows(labels, K, eps, weights, dtype)
    if x is not None:
        x = np.ascontiguousarray(x, dtype=np.float32).astype(dtype)
    if np.float32(mix) == 0 or B < 2:
        return (None if x is None else x.copy()), base
    p = partner(B, seed, base_stream)
    lam, mu = lambdas(B, mix, seed, base_stream, dtype)
    tg = lam[:, None] * base + mu[:, None] * base[p]
    y = lam[:, None, None] * x + mu[:, None, None] * x[p]
    assert tg.dtype == dtype and y.dtype == dtype
    return y, tg


def mixup_models(x, labels: np.ndarray, K: int, rngs, **kw):
    """M models: x [B,T,C] (shared), [M,B,T,C] or None; labels [M,B]; rngs: M (seed, base_stream) pairs -> ([M,B,T,C] or None, [M,B,K])."""
    ys, tgs = [], []
    for m, (s, bs) in enumerate(rngs):
        xm = None if x is None else (x if x.ndim == 3 else x[m])
        y, tg = mixup(xm, labels[m], K, s, bs, **kw)
        ys.append(y); tgs.append(tg)
    return (None if x is None else np.stack(ys)), np.stack(tgs)


def soft_ce(logits: np.ndarray, q: np.ndarray, scale: float = 1.0):
    """float64: per-trial loss = - sum_k q_k log softmax_k and dlogits = scale (s p - q), s = sum_k q_k"""
    lg = np.asarray(logits, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    m = lg.max(-1, keepdims=True)
    lse = m + np.log(np.exp(lg - m).sum(-1, keepdims=True))
    logp = lg - lse
    loss = -(q * logp).sum(-1)
    dl = scale * (q.sum(-1, keepdims=True) * np.exp(logp) - q)
    return loss, dl
