"""Head width F (fc.0) and class count K across the range include/nsd.h promises, on the host (no GPU): parameter and workspace
layouts over the (F, K) grid, the domain predicates at their documented edges with the refusals that go with them, and the CPU
oracle against a float64 torch restatement of the model at the shapes tests/test_gpu_head_dims.py compares the kernels at.

The rest of the suite runs at F = 32 and K <= 8 only; the reference the GPU tests of other head sizes rest on is pinned here.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import nsd_amd
from nsd_amd import _lib, ops
from oracle import nsd_oracle as orc
from oracle import seq_bf16_ref as sr
from oracle.torch_ref import TorchRefEEG
from tests.gpu_harness import BASE_SHAPES, KINK_MARGIN, head_inputs, kink_margin

F_GRID = (1, 7, 31, 32, 33, 48, 63, 64, 65)
K_GRID = (1, 2, 3, 8, 9, 33, 64, 65)
_FAKE = 4096                     # a pointer that is never dereferenced: every call it is passed to is refused before a launch


# ---- parameter count and layout ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", F_GRID)
def test_param_count_and_layout_over_the_head_grid(F):
    L = nsd_amd.load_library()
    for K in K_GRID:
        d = orc.Dims(C=8, H=48, L=2, K=K, F=F)
        spec = ops.ModelSpec(C=8, H=48, L=2, K=K, F=F)
        assert spec.param_count == orc.param_count(d) == 29952 + 3 * 48 + 1 + F * 48 + F + K * F + K, (F, K)
        assert spec.offsets() == orc.layout(d) and spec.shapes() == orc.param_shapes(d), (F, K)
        # the sequence path's layout: one direction and two, against oracle/seq_bf16_ref.py
        for Cs, Hs, Ls, D in ((8, 128, 2, 1), (24, 64, 3, 2)):
            ref = sr.param_layout(Cs, Hs, Ls, K, F, D)
            sspec = ops.ModelSpec(C=Cs, H=Hs, L=Ls, K=K, F=F, D=D)
            assert L.nsd_seq_param_count(Cs, Hs, Ls, K, F, D) == sr.param_count(Cs, Hs, Ls, K, F, D), (F, K, D)
            offs = (C.c_int64 * (4 * Ls * D + 8))()
            assert L.nsd_seq_param_layout(Cs, Hs, Ls, K, F, D, offs) == 0
            assert [int(o) for o in offs] == [o for o, _ in ref.values()], (F, K, D)
            assert sspec.names() == list(ref) and sspec.shapes() == {k: s for k, (_, s) in ref.items()}, (F, K, D)
    assert ops.ModelSpec(K=8, F=64).param_count == 33753 and ops.ModelSpec(K=64, F=1).param_count == 30274   # neither a multiple of 4


# ---- workspace layout -------------------------------------------------------------------------------------------------------------
_REGIONS = ["hseq", "cseq", "gact", "inseq", "top", "alpha", "pooled", "fc0_pre", "dscore", "dpooled", "loss", "adpack", "slabs", "hslabs",
            "da_seq", "din"]


def _check_ws(w, nbytes, trials, T, H, Ll, F, P, P_lstm, fast):
    """regions in ascending order, each at least the size the comments of nsd_ws_layout (include/nsd.h) state; total * 4 == bytes"""
    BT = trials * T
    need = {"hseq": Ll * BT * H, "cseq": Ll * BT * H, "gact": 4 * Ll * BT * H, "inseq": (Ll - 1) * BT * H, "top": BT * H, "alpha": BT,
            "pooled": trials * H, "fc0_pre": trials * F, "dscore": BT, "dpooled": trials * H, "loss": trials, "adpack": 4 * BT,
            "slabs": w.n_slabs * P_lstm, "hslabs": trials * (P - P_lstm),
            "da_seq": 0 if fast else Ll * BT * 4 * H, "din": 0 if fast else 2 * BT * H}
    offs = [getattr(w, r) for r in _REGIONS] + [w.total]
    assert offs[0] == 0 and nbytes == 4 * w.total and w.n_slabs >= 1
    for i, r in enumerate(_REGIONS):
        assert offs[i] % 4 == 0, r
        assert offs[i + 1] - offs[i] >= need[r], (r, offs[i + 1] - offs[i], need[r])


@pytest.mark.parametrize("F", F_GRID)
def test_workspace_layouts_over_the_head_grid(F):
    L = nsd_amd.load_library()
    for K in K_GRID:
        for H, B, T in ((48, 5, 33), (48, 300, 7), (40, 6, 17)):
            d = _lib.Dims(B, T, 8, H, 2, K, F)
            P, P_lstm = L.nsd_param_count(8, H, 2, K, F), orc.layout(orc.Dims(C=8, H=H, L=2, K=K, F=F))["ln.weight"]
            w = _lib.WsLayout()
            n = L.nsd_workspace_bytes(C.byref(d), C.byref(w))
            assert n > 0, (F, K, H)
            _check_ws(w, n, B, T, H, 2, F, P, P_lstm, fast=H == 48)
            if H != 48:
                continue
            for M in (1, 3, 17):
                wm = _lib.WsLayout()
                nm = L.nsd_multi_workspace_bytes(C.byref(d), M, C.byref(wm))
                if F <= 64 and K <= 8:
                    assert nm > 0, (F, K, M)
                    _check_ws(wm, nm, M * B, T, H, 2, F, P, P_lstm, fast=True)
                else:
                    assert nm == -1 and "F <= 64, K <= 8" in L.nsd_last_error().decode(), (F, K, M)


# ---- domain predicates and the refusals that go with them -------------------------------------------------------------------------
def _d48(F, K, B=4, T=10):
    return _lib.Dims(B, T, 8, 48, 2, K, F)


def test_rng_path_flips_at_its_documented_edge_and_the_entry_points_refuse_beyond_it():
    """nsd_rng_path: the single-launch H = 48 train step, F <= 64 and K <= 8 (TT_KMAX of csrc/nsd_lstm2_fwd48.hip)"""
    L = nsd_amd.load_library()
    for F, K, ok in ((64, 8, 1), (1, 1, 1), (65, 8, 0), (64, 9, 0), (65, 9, 0), (32, 64, 0)):
        d = _d48(F, K)
        assert L.nsd_rng_path(C.byref(d)) == ok, (F, K)
        assert ops.rng_path(ops.ModelSpec(K=K, F=F), 4, 10) == bool(ok)
        need = L.nsd_workspace_bytes(C.byref(d), None)
        rng = _lib.Rng(1, 4, 0.6, 0.6)
        if ok:
            continue
        rc = L.nsd_lstm_head_train_rng(C.byref(d), _FAKE, _FAKE, C.byref(rng), _FAKE, 1.0, 2, _FAKE, need, _FAKE, None)
        err = L.nsd_last_error().decode()
        assert rc == -1 and err.startswith("lstm_head_train_rng: shape outside the single-launch path") and "F <= 64, K <= 8" in err, err
        rc = L.nsd_lstm_bwd_rng(C.byref(d), _FAKE, _FAKE, C.byref(rng), 2, _FAKE, need, None)
        err = L.nsd_last_error().decode()
        assert rc == -1 and err.startswith("lstm_bwd_rng: shape outside the single-launch path") and "F <= 64, K <= 8" in err, err
    # the explicit-mask entry point takes the same shapes through its two-launch fallback: only the workspace size stands in its way here
    d = _d48(33, 9)
    need = L.nsd_workspace_bytes(C.byref(d), None)
    assert L.nsd_lstm_head_train(C.byref(d), _FAKE, _FAKE, None, None, None, _FAKE, 1.0, 2, _FAKE, need - 4, _FAKE, None) == -3


def test_multi_path_flips_at_its_documented_edge_and_every_entry_point_refuses_beyond_it():
    L = nsd_amd.load_library()
    adam = [1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1]
    for F, K, ok in ((64, 8, 1), (1, 1, 1), (65, 8, 0), (64, 9, 0), (32, 64, 0)):
        d = _d48(F, K)
        for M in (1, 3, 32):
            assert L.nsd_multi_path(C.byref(d), M) == ok, (F, K, M)
        assert ops.multi_path(ops.ModelSpec(K=K, F=F), 3) == bool(ok)
        if ok:
            continue
        M = 3
        rngs = (_lib.Rng * M)(*[_lib.Rng(1 + m, 4, 0.6, 0.6) for m in range(M)])
        rp = C.cast(rngs, C.c_void_p)
        big = 1 << 40
        calls = {
            "multi_train_fwd": lambda: L.nsd_multi_train_fwd(C.byref(d), M, _FAKE, _FAKE, 0, rp, _FAKE, 0, _FAKE, big, _FAKE, None),
            "multi_train_bwd": lambda: L.nsd_multi_train_bwd(C.byref(d), M, _FAKE, _FAKE, 0, rp, 0, _FAKE, big, None),
            "multi_grad_reduce": lambda: L.nsd_multi_grad_reduce(C.byref(d), M, _FAKE, big, _FAKE, None),
            "multi_grad_reduce_adam": lambda: L.nsd_multi_grad_reduce_adam(C.byref(d), M, _FAKE, big, _FAKE, _FAKE, _FAKE, _FAKE, *adam, None),
            "multi_loss_sum": lambda: L.nsd_multi_loss_sum(C.byref(d), M, _FAKE, big, _FAKE, None),
            "multi_infer": lambda: L.nsd_multi_infer(C.byref(d), M, _FAKE, _FAKE, 0, 0, _FAKE, None, _FAKE, None),
        }
        for who, call in calls.items():
            assert call() == -1, (who, F, K)
            assert L.nsd_last_error().decode() == (f"{who}: shape outside the model-batched path (nsd_multi_path: H = 48, L = 2, C <= 8, "
                                                   "T <= 1024, F <= 64, K <= 8)"), (who, F, K)
        assert L.nsd_multi_workspace_bytes(C.byref(d), M, None) == -1
        assert L.nsd_multi_infer_scratch_bytes(C.byref(d), M) == -1


def test_seq_supported_flips_at_its_documented_edge_and_every_entry_point_refuses_beyond_it():
    L = nsd_amd.load_library()
    rng = _lib.Rng(1, 4, 0.4, 0.4)
    rp = C.cast(C.pointer(rng), C.c_void_p)
    for F, K, ok in ((64, 64, 1), (1, 1, 1), (65, 64, 0), (64, 65, 0), (65, 65, 0)):
        for flags in (0, _lib.NSD_FLAG_BIDIR):
            d = _lib.Dims(32, 10, 8, 128, 2, K, F)
            assert L.nsd_seq_supported(C.byref(d), flags) == ok, (F, K, flags)
            assert ops.ModelSpec(H=128, K=K, F=F, D=2 if flags else 1).seq_path(32, 10) == bool(ok)
            if ok:
                assert L.nsd_seq_workspace_bytes(C.byref(d), flags) > 0
                continue
            big = 1 << 40
            calls = [
                lambda: L.nsd_seq_workspace_bytes(C.byref(d), flags),
                lambda: L.nsd_seq_infer(C.byref(d), _FAKE, _FAKE, flags, _FAKE, None, _FAKE, big, None),
                lambda: L.nsd_seq_train_fwd(C.byref(d), _FAKE, _FAKE, rp, _FAKE, 1.0, flags, _FAKE, big, _FAKE, None),
                lambda: L.nsd_seq_train_bwd(C.byref(d), _FAKE, rp, flags, _FAKE, big, _FAKE, None),
                lambda: L.nsd_seq_train_fwd_logits(C.byref(d), _FAKE, _FAKE, rp, flags, _FAKE, big, _FAKE, None),
                lambda: L.nsd_seq_head_bwd(C.byref(d), _FAKE, rp, _FAKE, flags, _FAKE, big, None),
                lambda: L.nsd_seq_train_bwd_dx(C.byref(d), _FAKE, rp, flags, _FAKE, big, _FAKE, _FAKE, None),
                lambda: L.nsd_seq_loss_sum(C.byref(d), flags, _FAKE, big, _FAKE, None),
            ]
            for i, call in enumerate(calls):
                assert call() == -1, (i, F, K)
                assert L.nsd_last_error().decode() == f"seq path: F={F} K={K} exceed 64", (i, F, K)


def test_inference_tail_and_dx_domains_do_not_depend_on_the_head_beyond_their_documented_limits():
    """nsd_fast_path / nsd_dx_path look at the LSTM's shape only; nsd_infer takes any F, K >= 1 (the H = 48 tail to 64, nsd_head.hip beyond)"""
    L = nsd_amd.load_library()
    for F, K in ((1, 1), (64, 64), (65, 65), (200, 300)):
        d = _d48(F, K)
        assert L.nsd_fast_path(C.byref(d)) == 1 and L.nsd_dx_path(C.byref(d)) == 1
        assert L.nsd_infer_scratch_bytes(C.byref(d)) == 4 * 4 * 10 * 48
        assert L.nsd_infer(C.byref(d), None, None, 0, None, None, None, None) == -1 and b"null" in L.nsd_last_error()
    for F, K in ((0, 3), (32, 0)):
        d = _d48(F, K)
        assert L.nsd_workspace_bytes(C.byref(d), None) == -1 and L.nsd_rng_path(C.byref(d)) == 0 and L.nsd_multi_path(C.byref(d), 2) == 0


# ---- the oracle itself, off the reference's head size -----------------------------------------------------------------------------
@pytest.mark.parametrize("Cc,H,K,F,B,T", BASE_SHAPES)
def test_oracle_matches_a_float64_restatement_of_the_model(Cc, H, K, F, B, T):
    """The CPU oracle (plain C, fp32) against the model of lstm_eeg_model.py:32-39 restated with stock torch in float64, train-mode
    masks on: logits within 1e-6, every gradient tensor within 5e-6 of its largest element (measured 2.4e-7 / 7.1e-7: what is left is
    the fp32 summation order of the oracle).  K = 1: the loss and every gradient are exactly zero on both sides."""
    d, flat, x, y, masks = head_inputs(Cc, H, K, F, B, T)
    loss, g, fw = orc.loss_and_grads(flat, x, y, d, **masks)
    margin = kink_margin(fw)
    m = TorchRefEEG(Cc, H, 2, K, F=F)
    m.load_reference_state({k: torch.from_numpy(v) for k, v in orc.unflatten(flat, d).items()})
    m = m.double()
    t = lambda a: torch.from_numpy(a).double()           # noqa: E731
    logits = m(t(x), t(masks["drop_lstm"]), t(masks["rrelu_slope"]), t(masks["drop_head"]))
    loss64 = torch.nn.functional.cross_entropy(logits, torch.from_numpy(y.astype(np.int64)))
    loss64.backward()
    loss64 = float(loss64.detach())
    lerr = float(np.abs(fw["logits"] - logits.detach().numpy()).max())
    ref = {k: v.detach().numpy() for k, v in m.reference_named_grads().items()}
    got = orc.unflatten(g, d)
    worst = 0.0
    for k in orc.param_names(d):
        scale = float(np.abs(ref[k]).max())
        err = float(np.abs(got[k] - ref[k].reshape(got[k].shape)).max())
        if K == 1:
            assert scale == 0.0 and err <= 1e-7, (k, scale, err)
            continue
        if k == "attn.bias":                               # analytically zero: both sides are round-off
            assert err < 2e-6, (k, err)
            continue
        worst = max(worst, err / scale)
        assert err <= 5e-6 * scale, (k, err, scale)
    print(f"oracle vs float64 C={Cc} H={H} K={K} F={F}: logits {lerr:.2e}  loss {abs(loss - loss64):.2e}  grads/max {worst:.2e}  "
          f"kink margin {margin:.1e}")
    assert lerr < 1e-6
    assert abs(loss - loss64) < 2e-6               # log-sum-exp and the label's logit each move by at most the logits' bound
    assert margin > KINK_MARGIN, margin
    if K == 1:
        assert abs(loss) < 1e-7
