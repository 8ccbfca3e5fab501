"""Trial augmentation (nsd_augment), the parts that need no GPU: the exported symbols, the refusals of the C entry point, the numpy
restatement the kernel is held to (tests/augment_ref.py) and the command-line flags."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nsd_amd
from nsd_amd import _lib
from oracle import nsd_oracle as orc
from tests import augment_ref as ar
from tests.train_cli import parse_train_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1


def test_augment_symbols_are_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nsd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(nsd_[a-z0-9_]+)\s*\(", hdr))
    L = nsd_amd.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    for name in ("nsd_augment", "nsd_augment_path"):
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(L, name) and name in exported, name
    assert "#define NSD_AUG_ZSCORE 1u" in hdr and "typedef struct nsd_aug" in hdr
    assert L.nsd_version() == 301                                  # additive: the version stays


def _call(L, d, M=1, x=4096, stride=0, aug=None, rng=True, step_dev=None, flags=0, y=1 << 30):
    a = aug if aug is not None else _lib.Aug(0, 0.0, 0.0, 0.0)
    r = (_lib.Rng * 32)()
    return L.nsd_augment(C.byref(d), M, x, stride, C.byref(a) if aug is not False else None,
                         C.cast(r, C.c_void_p) if rng else None, step_dev, flags, y, None)


def test_augment_refusals_without_a_gpu():
    """Every refusal returns NSD_E_INVALID before any launch (the pointers are never dereferenced: no device here)."""
    L = nsd_amd.load_library()
    d = _lib.Dims(4, 10, 8, 48, 2, 3, 32)
    n = 4 * 10 * 8
    for M in (0, -1, _lib.NSD_MAX_MODELS + 1):
        assert _call(L, d, M=M) == E_INVALID and b"M =" in L.nsd_last_error()
    assert _call(L, d, x=None) == E_INVALID and b"null" in L.nsd_last_error()
    assert _call(L, d, y=None) == E_INVALID
    assert _call(L, d, aug=False) == E_INVALID
    assert _call(L, d, rng=False) == E_INVALID
    assert L.nsd_augment(None, 1, 4096, 0, None, None, None, 0, 1 << 30, None) == E_INVALID
    for S in (-1, 10, 11):
        assert _call(L, d, aug=_lib.Aug(S, 0.0, 0.0, 0.0)) == E_INVALID and b"max_shift" in L.nsd_last_error()
    for r in (-0.1, 1.0, 2.0, float("nan")):
        assert _call(L, d, aug=_lib.Aug(0, r, 0.0, 0.0)) == E_INVALID and b"scale_range" in L.nsd_last_error()
    for p in (-0.1, 1.0, float("nan")):
        assert _call(L, d, aug=_lib.Aug(0, 0.0, p, 0.0)) == E_INVALID and b"p_channel" in L.nsd_last_error()
    for s in (-1.0, float("inf"), float("nan")):
        assert _call(L, d, aug=_lib.Aug(0, 0.0, 0.0, s)) == E_INVALID and b"noise_std" in L.nsd_last_error()
    for Cc in (0, 257, -3):
        assert _call(L, _lib.Dims(4, 10, Cc, 48, 2, 3, 32)) == E_INVALID
    assert _call(L, _lib.Dims(4, 0, 8, 48, 2, 3, 32)) == E_INVALID
    assert _call(L, d, M=3, stride=-1) == E_INVALID and b"x_model_stride" in L.nsd_last_error()
    assert _call(L, d, M=3, stride=n - 1) == E_INVALID and b"x_model_stride" in L.nsd_last_error()
    # y overlapping x: the same buffer, y inside x, x inside the M outputs
    assert _call(L, d, x=4096, y=4096) == E_INVALID and b"overlaps" in L.nsd_last_error()
    assert _call(L, d, x=4096, y=4096 + 4 * (n - 1)) == E_INVALID
    assert _call(L, d, M=3, x=4096 + 4 * (3 * n - 1), y=4096) == E_INVALID
    assert _call(L, d, M=3, stride=n, x=4096, y=4096 + 4 * (3 * n - 1)) == E_INVALID
    assert _call(L, d, flags=2) == E_INVALID
    # only B, T, C of the dims are read; B = 0 is fine and launches nothing
    assert _call(L, _lib.Dims(0, 10, 8, -5, 99, 0, 0)) == 0
    assert _call(L, _lib.Dims(0, 10, 8, 48, 2, 3, 32), M=32, flags=1) == 0


def test_augment_path_answers():
    L = nsd_amd.load_library()
    for Cc, want in ((1, 1), (8, 1), (64, 1), (256, 1), (0, 0), (257, 0)):
        assert L.nsd_augment_path(C.byref(_lib.Dims(16, 625, Cc, 48, 2, 3, 32))) == want, Cc
    assert L.nsd_augment_path(C.byref(_lib.Dims(16, 0, 8, 48, 2, 3, 32))) == 0
    assert L.nsd_augment_path(None) == 0


# ---- the numpy restatement by itself --------------------------------------------------------------------------------------------------
def test_numpy_hash_is_the_oracles():
    f = orc.lib().nsd_oracle_rand_u32
    rs = np.random.RandomState(0)
    idx = np.concatenate([np.arange(40, dtype=np.uint64), rs.randint(0, 2 ** 62, 200).astype(np.uint64) * np.uint64(3),
                          ar.trial_index(np.arange(5), 0), ar.trial_index(np.array([70000]), 256 + 255)])
    for seed, stream in ((0, 0), (1234, 7), (0x9E3779B97F4A7C15 + 5, 4 * 0x3FFFFFFF + 3), (2 ** 64 - 1, 2 ** 32 - 1)):
        got = ar.rand_u32(seed, stream, idx)
        want = np.array([f(seed, stream, int(i)) for i in idx], dtype=np.uint32)
        assert np.array_equal(got, want), (seed, stream)


def _x(B, T, Cc, seed=0):
    return (2.7 * np.random.RandomState(seed).standard_normal((B, T, Cc))).astype(np.float32)


def test_all_off_is_the_identity_bitwise():
    x = _x(5, 30, 8)
    x[0, 0, 0], x[1, 2, 3], x[2, 0, 1] = -0.0, np.nan, np.inf
    y = ar.augment(x, 99, 4)
    assert y is not x and np.array_equal(y.view(np.uint32), x.view(np.uint32))


def test_shift_stays_in_range_and_repeats_edges():
    B, T, Cc, S = 400, 20, 3, 6
    x = np.broadcast_to(np.arange(T, dtype=np.float32)[None, :, None] + 100.0, (B, T, Cc)).copy()
    s = ar.shifts(B, S, 5, 8)
    assert s.min() >= -S and s.max() <= S and set(s) == set(range(-S, S + 1))
    y = ar.augment(x, 5, 8, max_shift=S)
    for b in range(B):
        want = np.clip(np.arange(T) - s[b], 0, T - 1) + 100.0
        assert np.array_equal(y[b, :, 0], want.astype(np.float32))
        if s[b] > 0:
            assert np.all(y[b, :s[b] + 1] == 100.0)                # the first sample repeated, no wrap, no zero fill
        if s[b] < 0:
            assert np.all(y[b, T + s[b] - 1:] == 100.0 + T - 1)
    s_full = ar.shifts(B, T - 1, 5, 8)
    assert s_full.min() >= -(T - 1) and s_full.max() <= T - 1


def test_scale_is_one_factor_per_trial():
    x = _x(50, 12, 4, 1)
    y = ar.augment(x, 3, 12, scale_range=0.25)
    a = ar.scales(50, 0.25, 3, 12)
    assert a.dtype == np.float32 and a.min() >= 0.75 and a.max() <= 1.25 and a.std() > 0.05
    assert np.array_equal(y, a[:, None, None] * x)


def test_dropped_channel_is_exactly_zero_noise_included():
    x = _x(60, 9, 8, 2)
    d = ar.dropped(60, 8, 0.3, 11, 16)
    assert 0.15 < d.mean() < 0.45
    y = ar.augment(x, 11, 16, max_shift=2, scale_range=0.1, p_channel=0.3, noise_std=0.5)
    keep = ar.augment(x, 11, 16, max_shift=2, scale_range=0.1, noise_std=0.5)
    for b in range(60):
        for c in range(8):
            if d[b, c]:
                assert np.all(y[b, :, c].view(np.uint32) == 0)
            else:
                assert np.array_equal(y[b, :, c], keep[b, :, c])   # no rescaling of the kept channels


def test_model_draws_do_not_depend_on_the_other_models():
    x = _x(7, 15, 8, 3)
    aug = dict(max_shift=4, scale_range=0.2, p_channel=0.2, noise_std=0.3)
    three = ar.augment_models(x, [(10, 4), (20, 4), (30, 4)], **aug)
    five = ar.augment_models(x, [(77, 4), (20, 4), (1, 8), (2, 4), (3, 4)], **aug)
    assert np.array_equal(three[1], five[1]) and np.array_equal(three[1], ar.augment(x, 20, 4, **aug))
    assert not np.array_equal(three[0], three[1])


def test_two_steps_differ():
    x = _x(7, 15, 8, 4)
    for aug in (dict(max_shift=4), dict(scale_range=0.2), dict(p_channel=0.5), dict(noise_std=0.3)):
        assert not np.array_equal(ar.augment(x, 5, 4, **aug), ar.augment(x, 5, 8, **aug)), aug


@pytest.mark.parametrize("seed,base", [(1234, 4), (0x9E3779B97F4A7C15, 400), (7, 4 * 0x3FFFFFFF)])
def test_noise_moments(seed, base):
    """n / sqrt(21845) over 2e6 elements: |mean| <= 3.5e-3 and |var - 1| <= 5e-3 (5 standard errors), bounded by +-3.45."""
    n = ar.noise_units(2_000_000, seed, base).astype(np.float64) / np.sqrt(21845.0)
    mean, var = n.mean(), n.var()
    print(f"noise seed={seed} base={base}: mean {mean:+.3e} var-1 {var - 1:+.3e} max|n| {np.abs(n).max():.3f}")
    assert abs(mean) <= 3.5e-3 and abs(var - 1.0) <= 5e-3
    assert np.abs(n).max() <= 510 / np.sqrt(21845.0) + 1e-12
    assert ar.noise_factor(0.3) == np.float32(float(np.float32(0.3)) / np.sqrt(21845.0))


def test_shift_counts_are_uniform():
    """S = 25 over 2e5 trials: each of the 51 values 3922 +- 313 times (5 standard errors)."""
    s = ar.shifts(200_000, 25, 4321, 4)
    counts = np.bincount(s + 25, minlength=51)
    print(f"shift counts: {counts.min()} .. {counts.max()}")
    assert len(counts) == 51 and np.all(np.abs(counts - 200_000 / 51) <= 313)


# ---- Python surface -------------------------------------------------------------------------------------------------------------------
def test_augment_dataclass():
    A = nsd_amd.Augment
    assert A().enabled is False and A(max_shift=0, scale_range=0.0, p_channel=0.0, noise_std=0.0) == A()
    for kw in (dict(max_shift=1), dict(scale_range=0.1), dict(p_channel=0.1), dict(noise_std=0.1)):
        assert A(**kw).enabled is True
    for kw in (dict(max_shift=-1), dict(scale_range=1.0), dict(scale_range=-0.1), dict(p_channel=1.0), dict(noise_std=-1.0),
               dict(noise_std=float("inf")), dict(noise_std=float("nan"))):
        with pytest.raises(ValueError):
            A(**kw)
    with pytest.raises(Exception):
        A().max_shift = 3                                          # frozen


def test_cli_flags_parse(monkeypatch):
    seen = parse_train_args(["--synthetic", "16", "--aug-shift", "12", "--aug-scale", "0.1", "--aug-channel-drop", "0.2", "--aug-noise", "0.3"],
                  monkeypatch)
    a = seen["args"]
    assert (a.aug_shift, a.aug_scale, a.aug_channel_drop, a.aug_noise) == (12, 0.1, 0.2, 0.3) and seen.get("reached_device")
    d = parse_train_args(["--synthetic", "16"], monkeypatch)["args"]
    assert (d.aug_shift, d.aug_scale, d.aug_channel_drop, d.aug_noise) == (0, 0.0, 0.0, 0.0)


@pytest.mark.parametrize("bad", [["--aug-scale", "1.0"], ["--aug-shift", "-1"], ["--aug-channel-drop", "1.5"], ["--aug-noise", "-0.5"],
                                 ["--aug-shift", "625"]])
def test_cli_out_of_range_is_an_argparse_error_before_any_device(bad, monkeypatch, capsys):
    with pytest.raises(SystemExit) as e:
        parse_train_args(["--synthetic", "16"] + bad, monkeypatch)
    assert e.value.code == 2 and "error:" in capsys.readouterr().err
