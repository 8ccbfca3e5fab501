"""The causal front end (nsd_prep_* of include/nsd.h, nsd_amd.CausalPrep), everything that can be held without a GPU: the ABI surface,
the public state layout, every host-side refusal, the kernel's code object (no private segment), the fp32 reference against a float64
filter, the section design against scipy, the prefix property, the configuration's round trip and StepRecipe's order with the ops
stubbed out."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import nsd_amd
from nsd_amd import _lib, ops
from nsd_amd import step_recipe as sr
from tests import prep_ref as pr
from tests.code_object import device_elf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREP_SYMBOLS = ("nsd_prep_path", "nsd_prep_state_bytes", "nsd_prep_state_layout", "nsd_prep_reset", "nsd_prep_step")
E_INVALID, E_WORKSPACE = -1, -3
PTR = 4096                       # stands for a device pointer: a refusal returns before anything looks at it
CHAIN = dict(highpass=1.0, lowpass=40.0, notch=50.0)        # 1-40 Hz band-pass + 50 Hz notch at 125 Hz: three sections


def test_prep_symbols_are_declared_bound_and_exported_and_the_version_stays():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nsd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(nsd_[a-z0-9_]+)\s*\(", hdr))
    for name in PREP_SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS, name
    L = nsd_amd.load_library()
    for name in PREP_SYMBOLS:
        assert hasattr(L, name), name
    assert "typedef struct nsd_prep {" in hdr and "typedef struct nsd_prep_layout" in hdr
    assert "#define NSD_PREP_MAX_SECTIONS 4" in hdr and "#define NSD_PREP_BASELINE 1u" in hdr and "#define NSD_PREP_CAR      2u" in hdr
    assert L.nsd_version() == 301
    assert "nsd_prep.hip" in open(os.path.join(ROOT, "neural-speech-decoding_amd", "csrc", "Makefile")).read()
    assert "CausalPrep" in nsd_amd.__all__
    assert C.sizeof(_lib.Prep) == 8 + 4 * 5 * 4 + 8 and C.sizeof(_lib.PrepLayout) == 48
    assert (_lib.NSD_PREP_MAX_SECTIONS, _lib.NSD_PREP_BASELINE, _lib.NSD_PREP_CAR) == (4, 1, 2)


@pytest.mark.parametrize("Cc", [1, 2, 3, 7, 8, 63, 64])
def test_state_layout_is_disjoint_aligned_and_sized(Cc):
    L = nsd_amd.load_library()
    lay = ops.prep_layout(Cc)
    regions = [(lay.x0, Cc), (lay.z, 4 * 2 * Cc), (lay.mu, Cc), (lay.var, Cc), (lay.steps, 2)]
    used = np.zeros(int(lay.stride), np.int32)
    for off, n in regions:
        assert 0 <= off and off + n <= lay.stride, (off, n)
        used[off:off + n] += 1
    assert used.max() == 1                                           # disjoint
    assert (lay.steps * 4) % 8 == 0 and (lay.stride * 4) % 8 == 0    # the int64 sample count of every slot is 8-byte aligned
    assert lay.stride - int(used.sum()) < 8                          # no more than alignment padding
    assert {k: getattr(lay, k) for k in ("x0", "z", "mu", "var", "steps", "stride")} == pr.layout(Cc)
    for S in (1, 2, 7, 100000):
        assert L.nsd_prep_state_bytes(Cc, S) == S * lay.stride * 4
    assert L.nsd_prep_state_bytes(Cc, 0) == E_INVALID and L.nsd_prep_state_layout(Cc, None) == E_INVALID


def test_layout_and_path_outside_the_channel_range():
    L = nsd_amd.load_library()
    lay = _lib.PrepLayout()
    for Cc in (0, -1, 65, 1000):
        assert L.nsd_prep_path(Cc, None) == 0 and L.nsd_prep_state_bytes(Cc, 1) == E_INVALID
        assert L.nsd_prep_state_layout(Cc, C.byref(lay)) == E_INVALID
    assert L.nsd_prep_path(1, None) == 1 and L.nsd_prep_path(64, None) == 1
    assert ops.prep_path(8) and ops.prep_path(8, nsd_amd.CausalPrep.design(**CHAIN, zscore_seconds=2.0)) and not ops.prep_path(65)
    with pytest.raises(nsd_amd.NsdError):
        ops.prep_layout(65)


def _prep(flags=3, n=1, sos=None, alpha=0.01, var0=1.0):
    p = _lib.Prep(flags, n)
    sos = [(0.5, 0.1, 0.2, -0.3, 0.4)] * 4 if sos is None else sos
    for s, sec in enumerate(sos):
        for k, v in enumerate(sec):
            p.sos[s][k] = v
    p.alpha, p.var0 = alpha, var0
    return p


def test_every_host_side_refusal_returns_its_code_without_a_gpu():
    L = nsd_amd.load_library()
    Cc, S = 8, 4
    d = _lib.Dims(3, 5, Cc, 1, 1, 1, 1)
    need = L.nsd_prep_state_bytes(Cc, S)
    err = lambda: L.nsd_last_error().decode()
    NO = object()

    def step(dd=d, p=NO, x=PTR, slots=None, state=PTR, nbytes=need, s=S, y=2 * PTR):
        p = _prep() if p is NO else p
        return L.nsd_prep_step(None if dd is None else C.byref(dd), None if p is None else C.cast(C.pointer(p), C.c_void_p), x, slots,
                               state, nbytes, s, y, None)

    path = lambda p: L.nsd_prep_path(Cc, C.cast(C.pointer(p), C.c_void_p))       # the configuration's verdict without a launch
    dims = lambda B=3, T=5, c=Cc: _lib.Dims(B, T, c, 1, 1, 1, 1)
    assert step(dd=None) == E_INVALID and step(p=None) == E_INVALID and step(x=None) == E_INVALID and step(y=None) == E_INVALID
    assert "null" in err()
    for c in (0, -1, 65):
        assert step(dd=dims(c=c), state=None) == E_INVALID and "[1, 64]" in err()
    assert step(dd=dims(T=0)) == E_INVALID and step(dd=dims(B=-1)) == E_INVALID
    assert step(dd=dims(B=5)) == E_INVALID and "B = 5" in err()                 # more streams than slots
    assert step(s=0) == E_INVALID
    assert step(slots=PTR, state=None) == E_INVALID and "slots without a state" in err()
    assert step(p=_prep(flags=4)) == E_INVALID and "flag" in err() and step(p=_prep(flags=0x80000001)) == E_INVALID
    assert step(p=_prep(n=-1)) == E_INVALID and step(p=_prep(n=5)) == E_INVALID and "n_sections" in err()
    ok = (0.5, 0.1, 0.2, -0.3, 0.4)
    for k in range(5):
        for bad in (float("nan"), float("inf"), -float("inf")):
            sec = list(ok)
            sec[k] = bad
            assert step(p=_prep(n=2, sos=[ok, sec])) == E_INVALID, (k, bad)
            assert path(_prep(n=2, sos=[ok, sec])) == 0 and path(_prep(n=1, sos=[ok, sec])) == 1    # an unused section is not looked at
    for a1, a2 in ((0.0, 1.0), (0.0, -1.0), (0.0, 1.5), (1.5, 0.5), (-1.5, 0.5), (2.0, 1.0), (0.5, -0.5), (-0.7, -0.3)):
        assert step(p=_prep(sos=[(1.0, 0.0, 0.0, a1, a2)])) == E_INVALID and "unstable" in err(), (a1, a2)
    for a1, a2 in ((0.0, 0.0), (1.49, 0.5), (-1.49, 0.5), (0.0, 0.99), (0.0, -0.99), (-1.9, 0.95)):
        assert path(_prep(sos=[(1.0, 0.0, 0.0, a1, a2)])) == 1, (a1, a2)
    for alpha in (-0.1, 1.0, 1.5, float("nan")):
        assert step(p=_prep(alpha=alpha)) == E_INVALID and "alpha" in err()
    for var0 in (float("nan"), float("inf"), 0.0, -1.0):
        assert step(p=_prep(var0=var0)) == E_INVALID and "var0" in err()
    assert path(_prep(alpha=0.0, var0=0.0)) == 1 and step(p=_prep(alpha=0.0, var0=float("inf"))) == E_INVALID
    assert path(_prep()) == 1 and path(_prep(flags=0, n=0, alpha=0.0)) == 1 and path(_prep(n=4)) == 1
    n = 3 * 5 * Cc * 4
    assert step(x=PTR, y=PTR + 4) == E_INVALID and "overlap" in err() and step(x=PTR + n - 4, y=PTR) == E_INVALID
    assert step(x=PTR + 4, y=PTR, state=None, s=0) == E_INVALID                # (window mode too; y == x is the GPU tests' in-place case)
    assert step(nbytes=need - 1) == E_WORKSPACE and "nsd_prep_state_bytes" in err() and step(nbytes=0) == E_WORKSPACE
    assert step(dd=dims(B=0)) == 0 and step(dd=dims(B=0), state=None, s=0) == 0    # nothing to do: accepted, nothing launched
    reset = lambda c=Cc, state=PTR, nbytes=need, s=S, slots=None, n=0: L.nsd_prep_reset(c, state, nbytes, s, slots, n, None)
    assert reset(c=0) == E_INVALID and reset(c=65) == E_INVALID and reset(state=None) == E_INVALID and reset(s=0) == E_INVALID
    assert reset(nbytes=need - 4) == E_WORKSPACE
    assert reset(slots=PTR, n=-1) == E_INVALID and reset(slots=PTR, n=S + 1) == E_INVALID
    assert reset(slots=PTR, n=0) == 0                                          # an empty list: accepted, nothing launched
    hdr = open(os.path.join(ROOT, "include", "nsd.h")).read()
    for words in ("its rows of y are NaN", "a partial overlap is refused", "stays NaN until its slot is reset", "No host synchronisation"):
        assert words in hdr, words


def test_prep_kernels_have_no_private_segment(tmp_path):
    notes = device_elf("nsd_prep", str(tmp_path))
    sizes = {}
    for block in re.split(r"^\s*- \.agpr_count:", notes, flags=re.M)[1:]:
        kv = dict(re.findall(r"^\s*(\.[a-z_]+):\s*(.+?)\s*$", block, re.M))
        sizes[kv[".name"]] = int(kv[".private_segment_fixed_size"], 0)
    # one instantiation per (sections 0 .. 4, z-score, staging width), and the reset
    assert len(sizes) == 21 and sum("prep_kernel" in k for k in sizes) == 20 and any("prep_reset_kernel" in k for k in sizes), sorted(sizes)
    assert all(v == 0 for v in sizes.values()), sizes


# ---- the fp32 arithmetic against float64 ---------------------------------------------------------------------------------------------
OFFSETS = (0.0, 50.0, 5000.0, 2e5)
# three times the worst value this test prints (the largest |fp32 - float64| over the largest |float64| output of a case, over all
# cases): measured 7.5e-6
FP64_BOUND = 3 * 7.5e-6


def _raw(T, Cc=8, seed=0):
    """One window per offset scale: noise of 20 units, a 10 Hz rhythm, and per-channel DC offsets of up to the scale"""
    rs = np.random.RandomState(seed)
    t = np.arange(T)[None, :, None] / 125.0
    sig = 20.0 * rs.standard_normal((len(OFFSETS), T, Cc)) + 15.0 * np.sin(2 * np.pi * 10.0 * t + rs.uniform(0, 6.28, (len(OFFSETS), 1, Cc)))
    dc = np.asarray(OFFSETS)[:, None, None] * rs.uniform(-1.0, 1.0, (len(OFFSETS), 1, Cc))
    return (sig + dc).astype(np.float32)


def _float64(x, prep):
    from scipy.signal import sosfilt
    v = x.astype(np.float64)
    v = v - v[:, :1]
    if prep.car:
        v = v - v.mean(axis=2, keepdims=True)
    sos = np.array([[np.float32(c) for c in s[:3]] + [1.0] + [np.float32(c) for c in s[3:]] for s in prep.sections], np.float64)
    v = sosfilt(sos, v, axis=1)
    if prep.alpha > 0:
        a = float(np.float32(prep.alpha))
        oma = float(np.float32(1.0) - np.float32(prep.alpha))
        mu, var = v[:, 0].copy(), np.full_like(v[:, 0], float(np.float32(prep.var0)))
        out = np.empty_like(v)
        out[:, 0] = 0.0
        for t in range(1, v.shape[1]):
            d = v[:, t] - mu
            mu = mu + a * d
            var = oma * (var + (a * d) * d)
            out[:, t] = (v[:, t] - mu) / (np.sqrt(var) + 1e-6)
        v = out
    return v


def test_the_fp32_reference_against_a_float64_filter():
    pytest.importorskip("scipy")
    worst = 0.0
    for T in (41, 625, 5000):
        x = _raw(T)
        for car in (False, True):
            for alpha in (0.0, 0.002, 0.01):
                prep = nsd_amd.CausalPrep(sections=nsd_amd.CausalPrep.design(**CHAIN).sections, alpha=alpha, var0=400.0, car=car)
                got = pr.prep_ref(x, sections=prep.sections, alpha=prep.alpha, var0=prep.var0, baseline=True, car=car)
                want = _float64(x, prep)
                # the same function of CausalPrep's own float64 filter, where there is no z-score
                if alpha == 0.0:
                    assert np.abs(prep.filtered(x) - want).max() <= 1e-9 * np.abs(want).max()
                for i, off in enumerate(OFFSETS):
                    e = float(np.abs(got[i] - want[i]).max() / np.abs(want[i]).max())
                    print(f"T={T} car={car} alpha={alpha} offset={off:g}: {e:.2e}")
                    worst = max(worst, e)
    print(f"worst fp32 vs float64, of the largest output: {worst:.2e}")
    assert worst < FP64_BOUND


def test_design_against_scipy():
    signal = pytest.importorskip("scipy.signal")
    for fs in (125.0, 250.0, 1000.0):
        for fc in (0.5, 1.0, 8.0, 40.0, 0.45 * fs):
            for kind, kw in (("highpass", dict(highpass=fc)), ("lowpass", dict(lowpass=fc))):
                b, a = signal.butter(2, fc, kind, fs=fs)
                (sec,) = nsd_amd.CausalPrep.design(fs=fs, **kw).sections
                assert np.abs(np.array(sec) - np.array([b[0], b[1], b[2], a[1], a[2]]) / a[0]).max() < 1e-12, (fs, fc, kind)
        for f0, q in ((50.0, 30.0), (60.0, 30.0), (50.0, 5.0), (10.0, 2.0)):
            b, a = signal.iirnotch(f0, q, fs=fs)
            (sec,) = nsd_amd.CausalPrep.design(fs=fs, notch=f0, notch_q=q).sections
            assert np.abs(np.array(sec) - np.array([b[0], b[1], b[2], a[1], a[2]]) / a[0]).max() < 1e-12, (fs, f0, q)
    p = nsd_amd.CausalPrep.design(**CHAIN, zscore_seconds=2.0)
    assert len(p.sections) == 3 and p.alpha == 1.0 / 250.0 and p.baseline and not p.car and p.var0 == 1.0
    assert p.sections[0][1] < 0 < p.sections[1][1]                   # high-pass, low-pass, notch: in this order
    for bad in (dict(highpass=0.0), dict(lowpass=62.5), dict(notch=70.0), dict(zscore_seconds=0.001), dict(notch=50.0, notch_q=0.0)):
        with pytest.raises(ValueError):
            nsd_amd.CausalPrep.design(**bad)


def test_prefix_property_of_the_reference():
    x = _raw(70, Cc=5, seed=3)
    p = nsd_amd.CausalPrep.design(**CHAIN, zscore_seconds=0.5, car=True)
    kw = dict(sections=p.sections, alpha=p.alpha, var0=p.var0, baseline=True, car=True)
    whole = pr.prep_ref(x, **kw)
    for t in (1, 2, 33, 69):
        assert pr.prep_ref(x[:, :t], **kw).tobytes() == whole[:, :t].tobytes(), t
    # ... and of the state: chunk by chunk ends where the whole window ends
    st, parts = pr.State(4, 5), []
    for lo, hi in ((0, 7), (7, 8), (8, 41), (41, 70)):
        parts.append(pr.prep_ref(x[:, lo:hi], state=st, **kw))
    whole_st = pr.State(4, 5)
    pr.prep_ref(x, state=whole_st, **kw)
    assert np.concatenate(parts, 1).tobytes() == whole.tobytes() and st.slot_rows().tobytes() == whole_st.slot_rows().tobytes()
    assert list(st.n) == [70] * 4
    # everything off: a copy
    assert pr.prep_ref(x, baseline=False).tobytes() == x.tobytes()
    assert pr.same_bits(np.array([1.0, np.nan], np.float32), np.array([1.0, -np.nan], np.float32))
    assert not pr.same_bits(np.array([0.0], np.float32), np.array([-0.0], np.float32))


def test_configuration_round_trip_and_refusals():
    p = nsd_amd.CausalPrep.design(**CHAIN, zscore_seconds=2.0, var0=3.5, car=True, baseline=False)
    d = p.to_dict()
    assert nsd_amd.CausalPrep.from_dict(d) == p and set(d) == {"sections", "alpha", "var0", "baseline", "car"}
    import io
    buf = io.BytesIO()
    torch.save({"state_dict": {}, "nsd_prep": d}, buf)               # plain lists and numbers: loads with weights_only
    buf.seek(0)
    assert nsd_amd.CausalPrep.from_dict(torch.load(buf, weights_only=True)["nsd_prep"]) == p
    s = p.struct()
    assert (s.flags, s.n_sections) == (_lib.NSD_PREP_CAR, 3) and s.sos[2][4] == np.float32(p.sections[2][4]) and s.var0 == 3.5
    assert nsd_amd.CausalPrep().struct().flags == _lib.NSD_PREP_BASELINE
    for bad in (dict(alpha=1.0), dict(alpha=-0.1), dict(alpha=0.1, var0=0.0), dict(var0=float("nan")), dict(sections=((1, 0, 0, 0, 1.0),)),
                dict(sections=((1, 0, 0, 2.0, 0.5),)), dict(sections=((1, 0, 0, 0),)), dict(sections=((1, 0, 0, 0, 0),) * 5),
                dict(sections=((float("inf"), 0, 0, 0, 0),))):
        with pytest.raises(ValueError):
            nsd_amd.CausalPrep(**bad)
    with pytest.raises(ValueError, match="normalize"):
        nsd_amd.EEG_LSTM(normalize=True, prep=p)
    with pytest.raises(ValueError):
        nsd_amd.EEG_LSTM(prep="highpass")
    assert nsd_amd.EEG_LSTM(prep=p).prep is p and nsd_amd.EEG_LSTM().prep is None
    # calibrate: var0 becomes the mean variance of the filtered windows
    x = _raw(625)[:2]
    q = nsd_amd.CausalPrep.design(**CHAIN, zscore_seconds=2.0).calibrate(x)
    assert q.var0 == float(np.float32(q.filtered(x).var(axis=1).mean())) and 100.0 < q.var0 < 2000.0 and q.alpha == 1.0 / 250.0
    # without a GPU the model says so, with or without a front end
    with pytest.raises(nsd_amd.NsdError, match="GPU"):
        nsd_amd.EEG_LSTM(prep=p).eval()(torch.zeros(1, 4, 8))
    # a checkpoint without a front end is the plain state_dict it always was; with one, the dict form both loaders accept
    from nsd_amd.trainer import save_reference_checkpoint
    plain, with_prep = io.BytesIO(), io.BytesIO()
    save_reference_checkpoint(nsd_amd.EEG_LSTM(), plain)
    save_reference_checkpoint(nsd_amd.EEG_LSTM(prep=p), with_prep)
    plain.seek(0); with_prep.seek(0)
    a, b = torch.load(plain, weights_only=True), torch.load(with_prep, weights_only=True)
    assert len(a) == 16 and all(torch.is_tensor(v) for v in a.values())
    assert set(b) == {"state_dict", "nsd_prep"} and list(b["state_dict"]) == list(a) and b["nsd_prep"] == d


# ---- StepRecipe: augment -> prep -> mixup, into the buffers the step already has -----------------------------------------------------
AUG = nsd_amd.Augment(max_shift=3, scale_range=0.1)
LOSS = nsd_amd.Loss(label_smoothing=0.1, mixup=0.5)
PREP = nsd_amd.CausalPrep.design(**CHAIN, zscore_seconds=2.0)


@pytest.fixture
def calls(monkeypatch):
    rec = []

    def augment(x, aug, rngs, *, M=1, zscore=False, step_dev=None, out=None):
        rec.append(("augment", dict(x=x, zscore=zscore, out=out, M=M)))
        shape = tuple(x.shape) if x.dim() == 4 or M == 1 else (M,) + tuple(x.shape)
        return out if out is not None else torch.full(shape, 7.0)

    def prep_step(x, prep, state=None, *, slots=None, out=None):
        rec.append(("prep", dict(x=x, prep=prep, state=state, slots=slots, out=out)))
        return out if out is not None else x + 2.0

    def zscore(x, out=None):
        rec.append(("zscore", dict(x=x, out=out)))
        return out if out is not None else x + 1.0

    def mixup(x, labels, K, rngs, *, label_smoothing=0.0, mix=0.0, class_weights=None, M=1, step_dev=None, out=None, targets=None):
        rec.append(("mixup", dict(x=x, out=out)))
        tg = targets if targets is not None else torch.zeros((labels.numel(), K))
        return (None if x is None else out if out is not None else x * 0.5), tg

    for name, fn in (("augment", augment), ("prep_step", prep_step), ("zscore", zscore), ("mixup", mixup)):
        monkeypatch.setattr(ops, name, fn)
    return rec


def _recipe(stochastic=True, augment=None, loss=None, **kw):
    return sr.StepRecipe(nsd_amd.EEG_LSTM(**kw), stochastic, augment, loss, "cpu")


def test_step_recipe_runs_augment_prep_mixup_in_this_order(calls):
    g = torch.Generator().manual_seed(0)
    x, y = torch.randn((4, 5, 8), generator=g), torch.randint(0, 3, (4,), generator=g, dtype=torch.int32)
    r = _recipe(augment=AUG, loss=LOSS, prep=PREP)
    assert r.prep is PREP and _recipe().prep is None
    xo, labels, tg = r.prepare(x, y, [77], 3)
    assert [n for n, _ in calls] == ["augment", "prep", "mixup"]
    a, p, m = (c[1] for c in calls)
    assert a["zscore"] is False and torch.equal(a["x"], x)
    assert torch.equal(p["x"], torch.full((4, 5, 8), 7.0)) and p["out"] is p["x"] and p["prep"] is PREP and p["state"] is None and p["slots"] is None
    assert m["x"] is p["x"] and torch.equal(xo, p["x"] * 0.5) and labels is None
    # prep alone: one launch, the labels untouched; no z-score launch
    del calls[:]
    xo, labels, tg = _recipe(prep=PREP).prepare(x, y, [77], 3)
    assert [n for n, _ in calls] == ["prep"] and calls[0][1]["out"] is None and torch.equal(xo, x + 2.0) and labels is y and tg is None
    # stochastic=False strips the augmentation and the mixup, never the front end
    del calls[:]
    xo, _, _ = _recipe(stochastic=False, augment=AUG, loss=LOSS, prep=PREP).prepare(x, y, [77], 3)
    assert [n for n, _ in calls] == ["prep", "mixup"] and calls[1][1]["x"] is None and torch.equal(xo, x + 2.0)
    # an empty shard launches nothing
    del calls[:]
    x0, y0 = torch.zeros((0, 5, 8)), torch.zeros((0,), dtype=torch.int32)
    assert r.prepare(x0, y0, [1], 2)[0].shape == x0.shape and calls == []


def test_step_recipe_prep_uses_the_static_buffers_the_step_has(calls):
    g = torch.Generator().manual_seed(0)
    x, y = torch.randn((4, 5, 8), generator=g), torch.randint(0, 3, (4,), generator=g, dtype=torch.int32)
    step_dev = torch.zeros(1, dtype=torch.int64)
    # with augmentation: augment -> xn, prep in place on xn, mixup xn -> xm
    r = _recipe(augment=AUG, loss=LOSS, prep=PREP)
    bufs = r.static_buffers(x)
    assert sorted(bufs) == ["tg", "xm", "xn"]
    xo, labels, tg = r.prepare(x, y, [77], 0, step_dev=step_dev, bufs=bufs)
    a, p, m = (c[1] for c in calls)
    assert a["out"] is bufs["xn"] and p["x"] is bufs["xn"] and p["out"] is bufs["xn"] and m["x"] is bufs["xn"] and m["out"] is bufs["xm"]
    assert xo is bufs["xm"] and tg is bufs["tg"]
    # prep alone: x -> xn, nothing else
    del calls[:]
    r = _recipe(prep=PREP)
    bufs = r.static_buffers(x)
    assert sorted(bufs) == ["xn"]
    xo, labels, tg = r.prepare(x, y, [77], 0, step_dev=step_dev, bufs=bufs)
    assert [n for n, _ in calls] == ["prep"] and calls[0][1]["x"] is x and calls[0][1]["out"] is bufs["xn"] and xo is bufs["xn"] and labels is y
    # model-batched, per-model windows: one launch over all of them, in the caller's shape
    del calls[:]
    x4 = torch.randn((3, 4, 5, 8), generator=g)
    xo, _, _ = _recipe(prep=PREP).prepare(x4, y.repeat(3), [5, 6, 7], 4, M=3)
    assert [n for n, _ in calls] == ["prep"] and calls[0][1]["x"] is x4 and xo.shape == x4.shape


def test_model_batch_needs_the_same_prep_on_all_models():
    from nsd_amd.multimodel import _check_models
    other = nsd_amd.CausalPrep.design(highpass=2.0)
    with pytest.raises(nsd_amd.NsdError, match="model 1"):
        _check_models([nsd_amd.EEG_LSTM(prep=PREP), nsd_amd.EEG_LSTM(prep=other)], "test")
    with pytest.raises(nsd_amd.NsdError, match="model 1"):
        _check_models([nsd_amd.EEG_LSTM(prep=PREP), nsd_amd.EEG_LSTM()], "test")
