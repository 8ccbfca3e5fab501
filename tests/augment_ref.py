"""numpy restatement of nsd_augment (include/nsd.h): the specification the kernel is held to bit for bit.

Every fp32 operation is a numpy float32 operation (one rounding each, no FMA); the random draws are a vectorised port of
nsd_rand_u32 (csrc/nsd_common.h), itself checked against oracle.nsd_oracle's nsd_oracle_rand_u32 by tests/test_augment_cpu.py."""
import numpy as np

AUG_STREAM = 3                      # base_stream + 3: the trainers use + {0, 1, 2}
TRIAL_BIT = np.uint64(1) << np.uint64(63)
_M32 = np.uint64(0xFFFFFFFF)


def _mix32(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    return x ^ (x >> np.uint32(16))


def rand_u32(seed: int, stream: int, index) -> np.ndarray:
    """nsd_rand_u32(seed, stream, index) for an array of 64-bit indices."""
    index = np.asarray(index, dtype=np.uint64)
    lo, hi = (index & _M32).astype(np.uint32), (index >> np.uint64(32)).astype(np.uint32)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    s0, s1 = np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32)
    k = np.uint32((0x9E3779B9 * ((int(stream) + 1) & 0xFFFFFFFF)) & 0xFFFFFFFF)
    with np.errstate(over="ignore"):
        h = _mix32(lo ^ s0)
        h = _mix32(h + k + hi)
        return _mix32(h ^ s1)


def trial_index(b, slot: int) -> np.ndarray:
    """P(b, slot) = 2^63 | (uint64(b) << 16) | slot"""
    return TRIAL_BIT | (np.asarray(b, dtype=np.uint64) << np.uint64(16)) | np.uint64(slot)


def drop_threshold(p: float) -> int:
    """nsd_drop_threshold of csrc/nsd_common.h, on the float the C ABI receives"""
    t = float(np.float32(p)) * 4294967296.0
    return int(min(t, 4294967295.0))


def unit(r) -> np.ndarray:
    """U(r) = float(r >> 8) * 2^-24"""
    return (r >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def shifts(B: int, S: int, seed: int, base_stream: int) -> np.ndarray:
    r = rand_u32(seed, base_stream + AUG_STREAM, trial_index(np.arange(B), 0))
    return (r % np.uint32(2 * S + 1)).astype(np.int64) - S


def scales(B: int, r: float, seed: int, base_stream: int) -> np.ndarray:
    u = unit(rand_u32(seed, base_stream + AUG_STREAM, trial_index(np.arange(B), 1)))
    w = np.float32(2.0) * u - np.float32(1.0)                     # exact
    return np.float32(1.0) + np.float32(r) * w


def noise_units(n: int, seed: int, base_stream: int, first: int = 0) -> np.ndarray:
    """The integer n of the noise (byte sum - 510) of the per-element indices first .. first + n - 1, as float32."""
    q = rand_u32(seed, base_stream + AUG_STREAM, np.arange(first, first + n, dtype=np.uint64))
    s = (q & np.uint32(255)) + ((q >> np.uint32(8)) & np.uint32(255)) + ((q >> np.uint32(16)) & np.uint32(255)) + (q >> np.uint32(24))
    return (s.astype(np.int64) - 510).astype(np.float32)


def noise_factor(sigma: float) -> np.float32:
    return np.float32(float(np.float32(sigma)) / np.sqrt(21845.0))


def dropped(B: int, C: int, p: float, seed: int, base_stream: int) -> np.ndarray:
    """[B, C] bool"""
    b = np.arange(B)[:, None]
    idx = trial_index(b, 0) | (np.uint64(256) + np.arange(C, dtype=np.uint64)[None, :])
    return rand_u32(seed, base_stream + AUG_STREAM, idx) < np.uint32(drop_threshold(p))


def augment(x: np.ndarray, seed: int, base_stream: int, max_shift: int = 0, scale_range: float = 0.0, p_channel: float = 0.0,
            noise_std: float = 0.0) -> np.ndarray:
    """One model: x [B,T,C] float32 -> y [B,T,C] float32.  Order: shift, scale, noise, channel drop; an operation at 0 is skipped."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, T, C = x.shape
    v = x.copy()
    if max_shift:
        s = shifts(B, max_shift, seed, base_stream)
        src = np.clip(np.arange(T)[None, :] - s[:, None], 0, T - 1)
        v = np.take_along_axis(x, src[:, :, None], axis=1)
    if scale_range:
        v = scales(B, scale_range, seed, base_stream)[:, None, None] * v
    if noise_std:
        n = noise_units(B * T * C, seed, base_stream).reshape(B, T, C)
        v = v + noise_factor(noise_std) * n
    if p_channel:
        v = np.where(dropped(B, C, p_channel, seed, base_stream)[:, None, :], np.float32(0.0), v)
    assert v.dtype == np.float32
    return v


def augment_models(x: np.ndarray, rngs, **aug) -> np.ndarray:
    """M models: x [B,T,C] (shared) or [M,B,T,C]; rngs: M (seed, base_stream) pairs -> [M,B,T,C].  Model m's draws are those of a
    single-model call with rngs[m]."""
    return np.stack([augment(x if x.ndim == 3 else x[m], s, bs, **aug) for m, (s, bs) in enumerate(rngs)])
