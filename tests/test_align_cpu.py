"""Session alignment without a GPU: the package's numpy restatements (nsd_amd.SessionAlign.*_reference) against the tests' own
(tests/align_ref.py) and against straightforward float64 formulas, the configuration's validation, the ABI's declarations, checkpoint
keys, CLI parsing and the stage-order bookkeeping of StepRecipe.static_buffers."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import nsd_amd
from nsd_amd import _lib
from tests import align_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nsd_cov_state_bytes", "nsd_cov_state_layout", "nsd_cov_reset", "nsd_cov_step", "nsd_whiten_fit", "nsd_spatial_apply")


def test_the_abi_declares_binds_and_exports_the_symbols():
    text = open(os.path.join(ROOT, "include", "nsd.h")).read()
    declared = set(re.findall(r"\b(nsd_[a-z0-9_]+)\s*\(", text))
    L = _lib.lib()
    for name in SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS and hasattr(L, name), name
    assert C.sizeof(_lib.WhitenRecord) == 64 and C.sizeof(_lib.Whiten) == 12 and C.sizeof(_lib.CovLayout) == 32
    assert f"#define NSD_WHITEN_MAX_SWEEPS {_lib.NSD_WHITEN_MAX_SWEEPS}" in text
    for name in ("FEW", "NONFINITE", "CLIPPED", "NOT_CONVERGED"):
        assert re.search(rf"#define NSD_WHITEN_{name}\s+{getattr(_lib, 'NSD_WHITEN_' + name)}u", text), name
        assert getattr(ar, name) == getattr(_lib, "NSD_WHITEN_" + name)
    # host-side entry points answer without a device
    lay = _lib.CovLayout()
    assert L.nsd_cov_state_layout(8, C.byref(lay)) == 0 and (lay.sum, lay.count, lay.skipped, lay.stride) == (0, 64, 65, 66)
    assert L.nsd_cov_state_bytes(8, 3) == 3 * 66 * 8 and L.nsd_cov_state_bytes(33, 1) < 0 and L.nsd_cov_state_bytes(8, 0) < 0


def test_refusals_happen_before_any_launch():
    L = _lib.lib()
    d = _lib.Dims(2, 10, 8, 1, 1, 1, 1)
    fake = C.c_void_p(4096)                                                         # never dereferenced: every call below is refused
    w = _lib.Whiten(0.0, 1e-4, 1)
    INV = L.nsd_cov_step(None, fake, None, None, None, 0, 0, fake, fake, None)
    assert INV != 0
    assert L.nsd_cov_step(C.byref(d), fake, None, fake, None, 0, 0, fake, fake, None) == INV          # slots without a state
    assert L.nsd_cov_step(C.byref(d), fake, None, None, None, 0, 0, None, fake, None) == INV          # window mode without sums
    assert L.nsd_cov_step(C.byref(d), fake, None, None, fake, 1 << 20, 4, fake, fake, None) == INV    # sums with a state
    assert L.nsd_cov_step(C.byref(d), fake, None, None, fake, 1 << 20, 1, None, None, None) == INV    # B > S
    ws = L.nsd_cov_step(C.byref(d), fake, None, None, fake, 2 * 66 * 8 - 1, 2, None, None, None)
    assert ws not in (0, INV)                                                       # NSD_E_WORKSPACE
    assert b"nsd_cov_state_bytes" in L.nsd_last_error()
    assert L.nsd_cov_reset(8, fake, 66 * 8 - 1, 1, None, 0, None) == ws
    for bad in (_lib.Whiten(-0.1, 1e-4, 1), _lib.Whiten(1.5, 1e-4, 1), _lib.Whiten(0.0, 0.0, 1), _lib.Whiten(0.0, 2.0, 1),
                _lib.Whiten(0.0, 1e-4, 0), _lib.Whiten(float("nan"), 1e-4, 1)):
        assert L.nsd_whiten_fit(8, C.byref(bad), fake, 64, fake, 2, 1, None, 1, fake, fake, None) == INV
    assert L.nsd_whiten_fit(8, C.byref(w), fake, 63, fake, 2, 1, None, 1, fake, fake, None) == INV    # a stride below its row
    assert L.nsd_whiten_fit(8, C.byref(w), fake, 64, fake, 1, 1, None, 1, fake, fake, None) == INV
    assert L.nsd_whiten_fit(8, C.byref(w), fake, 64, fake, 2, 1, None, 0, fake, fake, None) == INV    # G < 1
    assert L.nsd_whiten_fit(33, C.byref(w), fake, 33 * 33, fake, 2, 1, None, 1, fake, fake, None) == INV
    assert L.nsd_spatial_apply(C.byref(d), fake, fake, 0, None, fake, None) == INV                    # n_mat < 1
    assert L.nsd_spatial_apply(C.byref(d), fake, fake, 1, None, C.c_void_p(4096 + 16), None) == INV   # a partial overlap
    assert b"overlaps" in L.nsd_last_error()
    empty = _lib.Dims(0, 10, 8, 1, 1, 1, 1)                                         # B = 0 launches nothing
    assert L.nsd_spatial_apply(C.byref(empty), fake, fake, 1, None, fake, None) == 0
    assert L.nsd_cov_step(C.byref(empty), fake, None, None, None, 0, 0, fake, fake, None) == 0


def test_config_validation_and_round_trip():
    A = nsd_amd.SessionAlign
    a = A(shrinkage=0.1, floor=1e-3, min_steps=40)
    assert A.from_dict(a.to_dict()) == a and A.from_dict({}) == A() and A().min_steps is None
    assert A().steps_needed(8) == 32 and a.steps_needed(8) == 40
    s = a.struct(8)
    assert (s.shrinkage, s.floor, s.min_steps) == (np.float32(0.1), np.float32(1e-3), 40) and A().struct(5).min_steps == 20
    for kw in (dict(shrinkage=-0.1), dict(shrinkage=1.1), dict(shrinkage=float("nan")), dict(floor=0.0), dict(floor=1.5), dict(min_steps=0),
               dict(min_steps=2.5)):
        with pytest.raises(ValueError):
            A(**kw)
    with pytest.raises(ValueError, match="SessionAlign"):
        nsd_amd.EEG_LSTM(align=dict(shrinkage=0.0))
    with pytest.raises(ValueError, match="normalize"):
        nsd_amd.EEG_LSTM(align=A(), normalize=True)
    with pytest.raises(ValueError, match="align_matrix without"):
        nsd_amd.EEG_LSTM(align_matrix=np.eye(8))
    with pytest.raises(ValueError, match="1 .. 32 channels"):
        nsd_amd.EEG_LSTM(input_size=33, align=A())


def _noisy(B, T, Cc, seed=0):
    rs = np.random.RandomState(seed)
    v = (10.0 * rs.standard_normal((B, T, Cc))).astype(np.float32)
    mask = np.zeros((B, T), np.uint32)
    if T > 4:
        v[0, 2, Cc - 1], v[B - 1, T - 1, 0], mask[B - 1, 1], mask[0, 3] = np.nan, np.inf, 6, 0x80000000
    return v, mask


@pytest.mark.parametrize("B,T,Cc", [(1, 1, 1), (3, 70, 3), (2, 65, 8), (2, 20, 32)])
def test_the_package_restatements_equal_the_tests_own_bitwise(B, T, Cc):
    A = nsd_amd.SessionAlign(floor=1e-6, min_steps=1)
    v, mask = _noisy(B, T, Cc)
    s1, c1 = A.cov_reference(v, mask)
    s2, c2 = ar.cov_ref(v, mask)
    assert ar.same_bits(s1, s2) and np.array_equal(c1, c2) and (c1.sum(axis=1) == T).all()
    # continuing from a state is the same chain: any cut gives the bits of the whole
    if T > 8:
        sa, ca = A.cov_reference(v[:, :7], mask[:, :7])
        sb, cb = A.cov_reference(v[:, 7:], mask[:, 7:], init=(sa, ca))
        assert ar.same_bits(sb, s1) and np.array_equal(cb, c1)
        sc, cc = ar.cov_ref(v[:, 7:], mask[:, 7:], sa, ca)
        assert ar.same_bits(sc, s1) and np.array_equal(cc, c1)
    clean = np.nan_to_num(v, nan=1.0, posinf=2.0)
    rs = np.random.RandomState(Cc)
    W = (rs.standard_normal((3, Cc, Cc)) / np.sqrt(Cc)).astype(np.float32)
    sel = [(2 * b + 1) % 4 for b in range(B)]                                       # (3 names a matrix outside the table)
    assert ar.same_bits(A.apply_reference(clean, W, sel), ar.apply_ref(clean, W, sel))
    assert ar.same_bits(A.apply_reference(v, W[0]), ar.apply_ref(v, W[0]))          # NaN steps by the arithmetic
    out = ar.apply_ref(v, W[0])
    assert np.isnan(out[np.isnan(v).any(axis=2)]).all() and np.isfinite(out[np.isfinite(v).all(axis=2)]).all()
    assert not np.isfinite(out[~np.isfinite(v).all(axis=2)]).any()                  # (an Inf sample: Inf or NaN on every channel)


@pytest.mark.parametrize("Cc", [1, 2, 8, 17, 32])
def test_the_fit_restatements_whiten_the_constructed_cases(Cc):
    for cond in (1.0, 1e2, 1e4):
        for shrink in (0.0, 0.25):
            A = nsd_amd.SessionAlign(shrinkage=shrink, floor=1e-6, min_steps=1)
            S, n = ar.constructed(Cc, cond, seed=5)
            assert np.array_equal(S, S.T)
            W1, r1 = A.fit_reference(S[None], n[None])
            W2, r2 = ar.whiten_ref(S[None], n[None], shrink, 1e-6, 1)
            assert np.abs(W1.astype(np.float64) - W2).max() <= 2.0 ** -23 * np.abs(W2).max()
            assert r1[0]["status"] == r2[0]["status"] == 0 and r1[0]["steps"] == 4096 and r1[0]["skipped"] == 3
            # the straightforward formula, in float64: W R' W = I
            R = S / n[0]
            Rp = (1.0 - np.float32(shrink)) * R + np.float32(shrink) * np.trace(R) / Cc * np.eye(Cc)
            lam, V = np.linalg.eigh(Rp)
            Wd = (V / np.sqrt(lam)) @ V.T
            assert np.abs(Wd @ Rp @ Wd - np.eye(Cc)).max() <= 1e-10
            assert np.abs(W2[0] - Wd).max() <= 2.0 ** -23 * np.abs(Wd).max()
            assert abs(r2[0]["eig_max"] - lam[-1]) <= 1e-12 * lam[-1] and abs(r2[0]["trace_mean"] - np.trace(R) / Cc) <= 1e-12 * lam[-1]


def test_the_fit_restatements_agree_on_every_status():
    Cc = 4
    A = nsd_amd.SessionAlign(min_steps=100)
    good = ar.constructed(Cc, 10.0, seed=1)
    flat = ar.constructed(Cc, 10.0, seed=2)
    flat[0][1, :] = 0.0
    flat[0][:, 1] = 0.0
    bad = (good[0].copy(), good[0 + 1].copy())
    bad[0][0, 0] = np.nan
    accs = [good, (good[0], np.array([50, 0])), bad, flat, (np.zeros((Cc, Cc)), np.array([500, 0]))]
    sums, counts = np.stack([a[0] for a in accs]), np.stack([a[1] for a in accs])
    groups = [0, 1, 2, 3, 4]
    W1, r1 = A.fit_reference(sums, counts, groups, 7)
    W2, r2 = ar.whiten_ref(sums, counts, 0.0, 1e-4, 100, groups, 7)
    assert [r["status"] for r in r1] == [r["status"] for r in r2] == [0, ar.FEW, ar.NONFINITE, ar.CLIPPED, ar.NONFINITE, ar.FEW, ar.FEW]
    eye = np.eye(Cc, dtype=np.float32)
    assert all(np.array_equal(W1[g], eye) and np.array_equal(W2[g], eye) for g in (1, 2, 4, 5, 6))
    assert np.abs(W1.astype(np.float64) - W2).max() <= 2.0 ** -23 * np.abs(W2).max()
    assert [r["accumulators"] for r in r1] == [1, 1, 1, 1, 1, 0, 0] and all(r["ignored"] == 0 for r in r1)
    _, r3 = A.fit_reference(sums, counts, [0, 9, -1, 3, 4], 5)
    assert all(r["ignored"] == 2 for r in r3) and r3[1]["status"] == ar.FEW


def test_checkpoint_keys_and_the_models_buffer(tmp_path):
    from nsd_amd.trainer import save_reference_checkpoint
    A = nsd_amd.SessionAlign(shrinkage=0.2)
    m = nsd_amd.EEG_LSTM(align=A)
    assert torch.equal(m.align_matrix, torch.eye(8)) and "align_matrix" not in m.state_dict() and m.align_record is None
    W = torch.eye(8) + 0.01 * torch.arange(64, dtype=torch.float32).view(8, 8)
    m.set_alignment(W, record={"steps": 10, "status": 0})
    with pytest.raises(ValueError):
        m.set_alignment(torch.eye(7))
    with pytest.raises(nsd_amd.NsdError, match="without align"):
        nsd_amd.EEG_LSTM().set_alignment(W)
    path = str(tmp_path / "a.pth")
    save_reference_checkpoint(m, path)
    state = torch.load(path, map_location="cpu", weights_only=True)
    assert set(state) == {"state_dict", "nsd_align"}
    assert state["nsd_align"]["config"] == A.to_dict() and torch.equal(state["nsd_align"]["matrix"], W)
    assert state["nsd_align"]["record"] == {"steps": 10, "status": 0}
    plain = str(tmp_path / "p.pth")
    save_reference_checkpoint(nsd_amd.EEG_LSTM(), plain)                            # a model without the stage: the raw state_dict, as before
    assert "nsd_align" not in torch.load(plain, map_location="cpu", weights_only=True)
    assert nsd_amd.EEG_LSTM(align=A, align_matrix=W.numpy()).align_matrix.equal(W)


def test_cli_parsing():
    from nsd_amd import calibrate, grid, train
    ap = train.build_parser()
    off = ap.parse_args(["--data", "d"])
    assert train.align_for(off) is None and not off.align
    on = ap.parse_args(["--data", "d", "--align", "--align-shrinkage", "0.1", "--align-floor", "0.001"])
    assert train.align_for(on) == nsd_amd.SessionAlign(shrinkage=0.1, floor=0.001)
    assert train.align_for(ap.parse_args(["--data", "d", "--align"])) == nsd_amd.SessionAlign()
    with pytest.raises(ValueError, match="without --align"):
        train.align_for(ap.parse_args(["--data", "d", "--align-floor", "0.001"]))
    with pytest.raises(ValueError):
        train.align_for(ap.parse_args(["--data", "d", "--align", "--align-shrinkage", "2"]))
    g = grid.build_parser().parse_args(["--data", "d", "--align", "--grid", "lr=1e-3,3e-3"])
    assert g.align and train.align_for(g) == nsd_amd.SessionAlign()
    c = calibrate.build_parser()
    assert c.parse_args(["--model", "m", "--data", "d", "--out", "o", "--align"]).align
    assert not c.parse_args(["--model", "m", "--data", "d", "--out", "o"]).align


def test_static_buffers_know_the_align_stage():
    from nsd_amd.step_recipe import StepRecipe
    x = torch.zeros((4, 32, 8))
    dev = torch.device("cpu")
    plain = StepRecipe(nsd_amd.EEG_LSTM(), True, None, None, dev)
    assert plain.align is None and plain.static_buffers(x) == {}                    # without the stage: nothing new
    m = nsd_amd.EEG_LSTM(align=nsd_amd.SessionAlign())
    r = StepRecipe(m, True, None, None, dev)
    bufs = r.static_buffers(x)
    assert set(bufs) == {"xn"} and tuple(bufs["xn"].shape) == (4, 32, 8) and r.align_W is m.align_matrix
    G = nsd_amd.SignalGate(rail=100.0)
    rg = StepRecipe(nsd_amd.EEG_LSTM(align=nsd_amd.SessionAlign(), gate=G), True, None, None, dev)
    assert set(rg.static_buffers(x)) == {"xn", "gm"}                                # the stage writes in place into the gate's xn
    from nsd_amd import ops
    rc = StepRecipe(m, True, None, None, dev, crop=ops.Crop(16, 2, 8))
    assert set(rc.static_buffers(x)) == {"xn", "xc", "yc"}                          # in front of the crop
    ms = [nsd_amd.EEG_LSTM(align=nsd_amd.SessionAlign()) for _ in range(3)]
    rm = StepRecipe(ms[0], True, None, None, dev, models=ms)
    assert tuple(rm.align_W.shape) == (3, 8, 8)
    W = torch.stack([torch.eye(8) * (k + 1) for k in range(3)])
    rm.set_alignment(W)
    assert all(torch.equal(ms[k].align_matrix, W[k]) for k in range(3))
    with pytest.raises(ValueError):
        rm.set_alignment(torch.eye(8))
