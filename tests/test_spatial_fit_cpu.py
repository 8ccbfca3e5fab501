"""Supervised session alignment without a GPU: the numpy restatements of nsd_spatial_bwd / nsd_spatial_fit_step (tests/spatial_fit_ref.py)
against an exact sum (math.fsum), float64 formulas and torch's Adam, the ABI's declarations and refusals, the configuration's validation, the
parser's new flags and the checkpoint round trip with and without the `spatial_fit` record.

Bounds, derived here:
  dW   every product (double)dy * (double)v of two fp32 values is exact; a serial chain of n additions in double is off by at most
       n * 2^-53 * sum|terms| (n - 1 roundings; the second-order terms fit into the spare one).  Stage 1 chains T terms, stage 2 at
       most B partial sums, so |s - exact| <= (T + B) * 2^-53 * sum|terms| for the double s that is then rounded once to fp32, which
       adds 2^-24 * |s|.  The reference is EXACT -- math.fsum over the exact products returns the correctly rounded sum -- so the bound
       stands as derived, with nothing added for the reference's own error.
  dv   C products and C - 1 sums, each rounded to fp32: |dv - exact| <= C * 2^-24 * sum_i |W[i][j] dy[i]| (first order, again with
       C + 1 for the second-order terms); the float64 product it is held to is exact to 2^-53 of that and does not show.
  Adam over n steps against torch.optim.Adam in float64: a step moves an entry by at most lr * max|m^ / sqrt(v^)| <= lr / (1 - beta1)
       (10 lr at beta1 = 0.9) and the fp32 evaluation of that update takes fewer than 16 roundings, so a step adds at most
       10 lr * 16 * 2^-24 plus the rounding of the entry itself, 2^-24 * |A|.  The moments feed back, so the sum over steps is doubled.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import nsd_amd
from nsd_amd import _lib
from nsd_amd.align import SpatialFit, check_spatial_fit
from tests import spatial_fit_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nsd_spatial_bwd_scratch_bytes", "nsd_spatial_bwd", "nsd_spatial_fit_state_bytes", "nsd_spatial_fit_state_layout",
           "nsd_spatial_fit_step")
SHAPES = [(1, 1, 1), (3, 5, 3), (5, 64, 4), (2, 65, 8), (4, 129, 7), (2, 3, 32)]


def _problem(B, T, Cc, n_mat=1, seed=0):
    rs = np.random.RandomState(seed + 100 * B + 10 * T + Cc)
    v = (10.0 * rs.standard_normal((B, T, Cc))).astype(np.float32)
    dy = (1e-3 * rs.standard_normal((B, T, Cc))).astype(np.float32)
    W = (np.eye(Cc) + 0.3 * rs.standard_normal((n_mat, Cc, Cc))).astype(np.float32)
    return v, dy, W


def test_the_abi_declares_binds_and_exports_the_symbols():
    text = open(os.path.join(ROOT, "include", "nsd.h")).read()
    declared = set(re.findall(r"\b(nsd_[a-z0-9_]+)\s*\(", text))
    L = _lib.lib()
    for name in SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS and hasattr(L, name), name
    assert C.sizeof(_lib.SpatialFitCfg) == 20 and C.sizeof(_lib.SpatialFitLayout) == 48
    assert re.search(rf"#define NSD_SPATIAL_FIT_NONFINITE\s+{_lib.NSD_SPATIAL_FIT_NONFINITE}u", text) and sr.NONFINITE == _lib.NSD_SPATIAL_FIT_NONFINITE
    lay = _lib.SpatialFitLayout()
    assert L.nsd_spatial_fit_state_layout(8, C.byref(lay)) == 0
    assert (lay.m, lay.v, lay.step, lay.skipped, lay.status, lay.stride) == (0, 256, 512, 520, 528, 536)
    assert L.nsd_spatial_fit_state_bytes(8, 3) == 3 * 536 + 8 and L.nsd_spatial_fit_state_bytes(33, 1) < 0 and L.nsd_spatial_fit_state_bytes(8, 0) < 0
    d = _lib.Dims(5, 20, 8, 1, 1, 1, 1)
    assert L.nsd_spatial_bwd_scratch_bytes(C.byref(d)) == 5 * 64 * 8
    assert L.nsd_spatial_bwd_scratch_bytes(C.byref(_lib.Dims(5, 20, 33, 1, 1, 1, 1))) < 0


def test_refusals_happen_before_any_launch():
    L = _lib.lib()
    d = _lib.Dims(2, 10, 8, 1, 1, 1, 1)
    fake = C.c_void_p(4096)                                                         # never dereferenced: every call below is refused
    INV = L.nsd_spatial_bwd(None, fake, fake, fake, 1, None, fake, None, None, None, 0, None)
    assert INV != 0
    assert L.nsd_spatial_bwd(C.byref(d), fake, fake, fake, 1, None, None, None, None, None, 0, None) == INV       # neither dv nor dW
    assert L.nsd_spatial_bwd(C.byref(d), fake, fake, fake, 0, None, fake, None, None, None, 0, None) == INV       # n_mat < 1
    assert L.nsd_spatial_bwd(C.byref(d), fake, fake, fake, 1, None, None, fake, None, None, 0, None) == INV       # dW without a scratch
    assert L.nsd_spatial_bwd(C.byref(d), fake, C.c_void_p(8192), fake, 1, None, C.c_void_p(8192 + 16), None, None, None, 0, None) == INV
    assert b"overlaps" in L.nsd_last_error()
    ws = L.nsd_spatial_bwd(C.byref(d), fake, fake, fake, 1, None, None, fake, None, fake, 2 * 64 * 8 - 1, None)
    assert ws not in (0, INV) and b"nsd_spatial_bwd_scratch_bytes" in L.nsd_last_error()                       # NSD_E_WORKSPACE
    bad33 = _lib.Dims(2, 10, 33, 1, 1, 1, 1)
    assert L.nsd_spatial_bwd(C.byref(bad33), fake, fake, fake, 1, None, fake, None, None, None, 0, None) == INV
    need = L.nsd_spatial_fit_state_bytes(8, 1)
    ok = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, decay=1e-2)
    for field, value in (("lr", -1.0), ("lr", float("nan")), ("lr", float("inf")), ("decay", -0.5), ("decay", float("nan")),
                         ("beta1", 1.0), ("beta1", -0.1), ("beta2", 1.0), ("beta2", float("nan")), ("eps", 0.0), ("eps", -1e-8),
                         ("eps", float("inf"))):
        cfg = _lib.SpatialFitCfg(**dict(ok, **{field: value}))
        assert L.nsd_spatial_fit_step(8, 1, fake, None, fake, C.byref(cfg), fake, need, None, None, 0, None) == INV, (field, value)
        assert field.encode() in L.nsd_last_error(), (field, L.nsd_last_error())
    cfg = _lib.SpatialFitCfg(**ok)
    assert L.nsd_spatial_fit_step(8, 1, fake, None, fake, C.byref(cfg), fake, need - 1, None, None, 0, None) == INV
    assert b"state" in L.nsd_last_error()
    assert L.nsd_spatial_fit_step(33, 1, fake, None, fake, C.byref(cfg), fake, 1 << 20, None, None, 0, None) == INV
    assert L.nsd_spatial_fit_step(8, 1, fake, None, fake, C.byref(cfg), fake, need, fake, None, 4, None) == INV      # loss_in without loss_out


@pytest.mark.parametrize("B,T,Cc", SHAPES)
def test_the_restated_dW_against_an_exact_sum(B, T, Cc):
    n_mat = 3
    v, dy, W = _problem(B, T, Cc, n_mat)
    sel = np.arange(B) % n_mat
    _, dW, counts = sr.bwd_ref(v, dy, W, sel)
    y64, x64 = dy.astype(np.float64), v.astype(np.float64)
    for m in range(n_mat):
        rows = np.flatnonzero(sel == m)
        terms = (y64[rows][:, :, :, None] * x64[rows][:, :, None, :]).reshape(-1, Cc, Cc)        # exact products, [rows * T, C, C]
        exact = np.array([[math.fsum(terms[:, i, j]) for j in range(Cc)] for i in range(Cc)])
        mass = np.abs(terms).sum(axis=0)
        chain = (T + B) * 2.0 ** -53 * mass
        bound = chain + 2.0 ** -24 * (np.abs(exact) + chain)
        err = np.abs(dW[m].astype(np.float64) - exact)
        print(f"dW m={m} {B, T, Cc}: worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert (err <= bound).all(), (m, float(err.max()))
    assert counts.tolist() == [B, 0]


@pytest.mark.parametrize("B,T,Cc", SHAPES)
def test_the_restated_dv_against_a_float64_product(B, T, Cc):
    v, dy, W = _problem(B, T, Cc)
    dv, _, _ = sr.bwd_ref(v, dy, W)
    exact = dy.astype(np.float64) @ W[0].astype(np.float64)                         # dv[t, j] = sum_i dy[t, i] W[i][j]
    mass = np.abs(dy.astype(np.float64)) @ np.abs(W[0].astype(np.float64))
    bound = (Cc + 1) * 2.0 ** -24 * mass
    assert (np.abs(dv.astype(np.float64) - exact) <= bound).all()


def test_rows_outside_the_table_and_nan_in_the_restatement():
    v, dy, W = _problem(5, 7, 4, n_mat=3)
    sel = np.array([0, -1, 2, 3, 0])
    dv, dW, counts = sr.bwd_ref(v, dy, W, sel)
    assert np.isnan(dv[1]).all() and np.isnan(dv[3]).all() and np.isfinite(dv[[0, 2, 4]]).all()
    assert counts.tolist() == [3, 2] and not dW[1].any()                            # no row selects matrix 1: zeros
    keep = [0, 2, 4]
    _, dW2, _ = sr.bwd_ref(v[keep], dy[keep], W, sel[keep])
    assert sr.same_bits(dW, dW2)
    dy2 = dy.copy()
    dy2[2, 3, 1] = np.nan
    dv3, dW3, _ = sr.bwd_ref(v, dy2, W, sel)
    nan_dv = np.isnan(dv3) & ~np.isnan(dv)
    assert nan_dv[2, 3].all() and nan_dv.sum() == 4                                 # exactly that step
    nan_dW = np.isnan(dW3)
    assert nan_dW[2, 1].all() and nan_dW.sum() == 4                                 # exactly row i = 1 of the matrix of trial 2


def test_the_restated_adam_against_torch_adam():
    rs = np.random.RandomState(5)
    Cc, n_mat, steps, lr = 8, 2, 6, 1e-2
    A0 = (np.eye(Cc)[None] + 0.1 * rs.standard_normal((n_mat, Cc, Cc))).astype(np.float32)
    grads = [(1e-2 * rs.standard_normal((n_mat, Cc, Cc))).astype(np.float32) for _ in range(steps)]
    ref = sr.FitRef(Cc, n_mat)
    A = A0.copy()
    p = torch.tensor(A0.astype(np.float64), requires_grad=True)
    opt = torch.optim.Adam([p], lr=float(np.float32(lr)), betas=(float(np.float32(0.9)), float(np.float32(0.999))), eps=float(np.float32(1e-8)))
    for s, g in enumerate(grads, 1):
        ref.step(A, g, None, lr=lr, decay=0.0)
        p.grad = torch.tensor(g.astype(np.float64))
        opt.step()
        bound = 2.0 * s * (10.0 * lr * 16 * 2.0 ** -24 + 2.0 ** -24 * np.abs(A0).max())
        err = float(np.abs(A.astype(np.float64) - p.detach().numpy()).max())
        print(f"adam step {s}: error {err:.3e} bound {bound:.3e}")
        assert err <= bound, (s, err, bound)
    assert ref.step_count.tolist() == [steps] * n_mat and ref.calls == steps
    # the first step moves every entry by lr against its gradient's sign (m^ / sqrt(v^) = sign(g) up to eps)
    ref1, A1 = sr.FitRef(Cc, n_mat), A0.copy()
    ref1.step(A1, grads[0], None, lr=lr)
    moved = A1.astype(np.float64) - A0
    assert (np.sign(moved) == -np.sign(grads[0])).all() and np.abs(np.abs(moved) - lr).max() < 1e-2 * lr


def test_the_restated_step_decay_skip_and_continuation():
    rs = np.random.RandomState(9)
    Cc, n_mat = 3, 3
    A0 = (np.eye(Cc)[None] + 0.1 * rs.standard_normal((n_mat, Cc, Cc))).astype(np.float32)
    prior = np.broadcast_to(np.eye(Cc, dtype=np.float32), A0.shape).copy()
    gs = [(1e-2 * rs.standard_normal((n_mat, Cc, Cc))).astype(np.float32) for _ in range(3)]
    a, A = sr.FitRef(Cc, n_mat), A0.copy()
    for g in gs:
        a.step(A, g, prior, decay=0.1)
    b, B_ = sr.FitRef(Cc, n_mat), A0.copy()
    for g in gs[:2]:
        b.step(B_, g, prior, decay=0.1)
    b.step(B_, gs[2], prior, decay=0.1)
    assert sr.same_bits(A, B_) and sr.same_bits(a.m, b.m) and sr.same_bits(a.v, b.v)
    nodecay, Cn = sr.FitRef(Cc, n_mat), A0.copy()
    nodecay.step(Cn, gs[0], prior, decay=0.0)
    plain, Cp = sr.FitRef(Cc, n_mat), A0.copy()
    plain.step(Cp, gs[0], None, decay=0.1)                                          # no prior: no pull, whatever the decay
    assert sr.same_bits(Cn, Cp)
    # a non-finite gradient of matrix 1: it stays, the others move
    bad = gs[0].copy()
    bad[1, 2, 0] = np.inf
    c, Cc_ = sr.FitRef(Cc, n_mat), A0.copy()
    losses = np.full(2, np.nan, np.float32)
    c.step(Cc_, bad, prior, decay=0.1, loss_in=1.5, loss_out=losses)
    c.step(Cc_, gs[1], prior, decay=0.1, loss_in=2.5, loss_out=losses)
    c.step(Cc_, gs[2], prior, decay=0.1, loss_in=3.5, loss_out=losses)              # past the cap: not written
    assert c.status.tolist() == [0, 1, 0] and c.skipped.tolist() == [0, 1, 0] and c.step_count.tolist() == [3, 2, 3] and c.calls == 3
    assert losses.tolist() == [1.5, 2.5]


def test_config_validation():
    check_spatial_fit(50, 1e-2, 1e-2, (0.9, 0.999), 1e-8)
    check_spatial_fit(1, 0.0, 0.0, (0.0, 0.0), 1e-12)
    for kw in (dict(epochs=0), dict(epochs=2.5), dict(epochs=True), dict(lr=-1e-3), dict(lr=float("nan")), dict(decay=-1.0),
               dict(decay=float("inf")), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(betas=(0.9,)), dict(eps=0.0),
               dict(eps=float("nan"))):
        args = dict(epochs=50, lr=1e-2, decay=1e-2, betas=(0.9, 0.999), eps=1e-8)
        args.update(kw)
        with pytest.raises(ValueError, match=next(iter(kw))):
            check_spatial_fit(**args)
    with pytest.raises(nsd_amd.NsdError, match="EEG_LSTM"):
        SpatialFit([nsd_amd.EEG_LSTM()])
    with pytest.raises(ValueError, match="lr"):
        SpatialFit(nsd_amd.EEG_LSTM(), lr=-1.0)
    with pytest.raises(nsd_amd.NsdError, match="hidden size 48, 2 layers"):        # the limit is named
        SpatialFit(nsd_amd.EEG_LSTM(hidden_size=32))
    with pytest.raises(nsd_amd.NsdError, match="mixup"):
        SpatialFit(nsd_amd.EEG_LSTM(), loss=nsd_amd.Loss(mixup=0.2))
    with pytest.raises(nsd_amd.NsdError, match="no CPU fallback"):
        SpatialFit(nsd_amd.EEG_LSTM())
    assert "CHOICES" in SpatialFit.__doc__


def test_enable_alignment_and_the_gradient_switch():
    m = nsd_amd.EEG_LSTM()
    assert m.align is None and not m.align_grad and not hasattr(m, "align_matrix")
    assert m.enable_alignment() is m and m.align == nsd_amd.SessionAlign() and torch.equal(m.align_matrix, torch.eye(8))
    assert "align_matrix" not in m.state_dict()
    W = torch.eye(8) + 0.5
    m.set_alignment(W)
    m.enable_alignment(nsd_amd.SessionAlign(shrinkage=0.3))                         # a model that has the stage keeps it, and its matrix
    assert m.align == nsd_amd.SessionAlign() and torch.equal(m.align_matrix, W)
    with pytest.raises(ValueError, match="normalize"):
        nsd_amd.EEG_LSTM(normalize=True).enable_alignment()
    assert nsd_amd.EEG_LSTM(align=nsd_amd.SessionAlign(), align_grad=True).align_grad


def test_cli_parsing():
    from nsd_amd import calibrate
    c = calibrate.build_parser()
    off = c.parse_args(["--model", "m", "--data", "d", "--out", "o"])
    assert not off.fit_spatial and (off.spatial_epochs, off.spatial_lr, off.spatial_decay) == (50, 1e-2, 1e-2)
    on = c.parse_args(["--model", "m", "--data", "d", "--out", "o", "--fit-spatial", "--spatial-epochs", "20", "--spatial-lr", "3e-3",
                       "--spatial-decay", "0"])
    assert on.fit_spatial and (on.spatial_epochs, on.spatial_lr, on.spatial_decay) == (20, 3e-3, 0.0) and not on.align


def test_checkpoint_round_trip_with_and_without_the_record(tmp_path):
    from nsd_amd.trainer import save_reference_checkpoint
    W = torch.eye(8) + 0.01 * torch.arange(64, dtype=torch.float32).view(8, 8)
    fit = dict(epochs=5, lr=1e-2, decay=1e-2, loss_first=1.25, loss_last=0.75, status=0)
    m = nsd_amd.EEG_LSTM().enable_alignment()
    m.set_alignment(W, record={"steps": 10, "status": 0, "spatial_fit": fit})
    path = str(tmp_path / "s.pth")
    save_reference_checkpoint(m, path)
    state = torch.load(path, map_location="cpu", weights_only=True)
    assert set(state) == {"state_dict", "nsd_align"} and torch.equal(state["nsd_align"]["matrix"], W)
    assert state["nsd_align"]["record"]["spatial_fit"] == fit and state["nsd_align"]["record"]["steps"] == 10
    # an older checkpoint: a record without the key, and no record at all, load unchanged
    for record in ({"steps": 10, "status": 0}, None):
        old = nsd_amd.EEG_LSTM(align=nsd_amd.SessionAlign(shrinkage=0.2), align_matrix=W)
        old.align_record = record
        p = str(tmp_path / "o.pth")
        save_reference_checkpoint(old, p)
        st = torch.load(p, map_location="cpu", weights_only=True)["nsd_align"]
        assert st["record"] == record and st["config"] == old.align.to_dict()
        back = nsd_amd.EEG_LSTM(align=nsd_amd.SessionAlign.from_dict(st["config"]))
        back.set_alignment(st["matrix"], record=st.get("record"))
        assert torch.equal(back.align_matrix, W) and back.align_record == record
