"""numpy restatement of nsd_crop and nsd_crop_pool (include/nsd.h): the specification the kernels are held to bit for bit.

The draws are tests/augment_ref.py's port of nsd_rand_u32 on the stream nsd_augment uses (base_stream + 3), at index slots
2048 .. 2048 + NSD_CROP_MAX - 1, which neither nsd_augment (0, 1, 256..511) nor nsd_mixup (1024 and the index 2^63 | 2^62) touches.  A
crop is a copy, so the windows are compared as bits; the pool's sum is a chain of numpy float32 additions (one rounding each)."""
import numpy as np

from tests.augment_ref import AUG_STREAM, rand_u32, trial_index

CROP_SLOT0 = 2048
CROP_MAX = 64                      # NSD_CROP_MAX


def crop_slots():
    """every per-trial index slot nsd_crop may draw"""
    return set(range(CROP_SLOT0, CROP_SLOT0 + CROP_MAX))


def offsets(B: int, T: int, W: int, R: int, hop: int = 0, seed: int = 0, base_stream: int = 0) -> np.ndarray:
    """[B, R] int64: hop > 0: r * hop (no draws); hop == 0: R(P(b, 2048 + r)) mod (T - W + 1)"""
    assert 1 <= W <= T and 1 <= R <= CROP_MAX and hop >= 0
    if hop > 0:
        assert (R - 1) * hop + W <= T
        return np.broadcast_to(np.arange(R, dtype=np.int64) * hop, (B, R)).copy()
    b = np.arange(B)[:, None]
    idx = trial_index(b, 0) | (np.uint64(CROP_SLOT0) + np.arange(R, dtype=np.uint64)[None, :])
    r = rand_u32(seed, base_stream + AUG_STREAM, idx)
    return (r % np.uint32(T - W + 1)).astype(np.int64).reshape(B, R)


def crop(x: np.ndarray, W: int, R: int, hop: int = 0, seed: int = 0, base_stream: int = 0, labels=None, targets=None):
    """One model: x [B,T,C] float32 -> (y [B*R,W,C], labels [B*R] or None, targets [B*R,K] or None, offsets [B*R]); row b * R + r."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, T, C = x.shape
    o = offsets(B, T, W, R, hop, seed, base_stream)
    y = np.stack([x[b, o[b, r]:o[b, r] + W] for b in range(B) for r in range(R)]) if B else np.zeros((0, W, C), np.float32)
    lab = None if labels is None else np.repeat(np.asarray(labels, dtype=np.int32), R)
    tg = None if targets is None else np.repeat(np.asarray(targets, dtype=np.float32), R, axis=0)
    return y, lab, tg, o.reshape(-1).astype(np.int32)


def crop_models(x: np.ndarray, W: int, R: int, rngs, hop: int = 0, labels=None, targets=None):
    """M models: x [B,T,C] (shared) or [M,B,T,C]; rngs: M (seed, base_stream) pairs; labels [M,B] / targets [M,B,K] or None
    -> (y [M,B*R,W,C], labels [M,B*R] or None, targets [M,B*R,K] or None, offsets [M,B*R]).  Model m's draws are those of a
    single-model call with rngs[m]."""
    out = [crop(x if x.ndim == 3 else x[m], W, R, hop, s, bs, None if labels is None else labels[m], None if targets is None else targets[m])
           for m, (s, bs) in enumerate(rngs)]
    stack = lambda i: None if out[0][i] is None else np.stack([o[i] for o in out])
    return stack(0), stack(1), stack(2), stack(3)


def pool(probs: np.ndarray, counts=None):
    """probs [N,R,K] float32 -> (mean [N,K] float32, log [N,K] float64 of the mean).  The serial float32 sum over the first cnt windows
    from 0, divided by float32(cnt); a count outside [1, R] or a non-finite value in the counted rows gives a NaN row."""
    probs = np.asarray(probs, dtype=np.float32)
    N, R, K = probs.shape
    mean = np.full((N, K), np.nan, dtype=np.float32)
    for n in range(N):
        cnt = R if counts is None else int(counts[n])
        if cnt < 1 or cnt > R or not np.isfinite(probs[n, :cnt]).all():
            continue
        s = np.zeros(K, dtype=np.float32)
        for r in range(cnt):
            s = s + probs[n, r]
        mean[n] = s / np.float32(cnt)
    assert mean.dtype == np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        return mean, np.log(mean.astype(np.float64))
