"""The model-batched H = 48 path (nsd_multi_*) without a GPU: symbols, shape rules, workspace layout, refusals before any launch."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["nsd_multi_path", "nsd_multi_workspace_bytes", "nsd_multi_train_fwd", "nsd_multi_train_bwd", "nsd_multi_grad_reduce",
       "nsd_multi_grad_reduce_adam", "nsd_multi_loss_sum", "nsd_multi_infer_scratch_bytes", "nsd_multi_infer"]


@pytest.fixture(scope="module")
def L():
    import nsd_amd
    nsd_amd.build_library()
    from nsd_amd import _lib
    return _lib


def _d(L, B=32, T=40, C_=8, H=48, Ly=2, K=3, F=32):
    return L.Dims(B, T, C_, H, Ly, K, F)


def test_symbols_in_header_binding_and_library(L):
    hdr = open(os.path.join(ROOT, "include", "nsd.h")).read()
    assert re.search(r"#define NSD_MAX_MODELS 32\b", hdr)
    assert re.search(r"#define NSD_VERSION 301\b", hdr)
    lib = L.lib()
    for s in NEW:
        assert re.search(r"\b%s\(" % s, hdr), s
        assert s in L.SYMBOLS, s
        assert hasattr(lib, s), s
    import nsd_amd
    assert "ModelBatchTrainer" in nsd_amd.__all__ and "EnsemblePredictor" in nsd_amd.__all__


def test_multi_path_rules(L):
    lib = L.lib()
    assert lib.nsd_multi_path(C.byref(_d(L)), 1) == 1
    assert lib.nsd_multi_path(C.byref(_d(L)), 32) == 1
    for M in (0, 33, -1):
        assert lib.nsd_multi_path(C.byref(_d(L)), M) == 0
    for kw in (dict(H=32), dict(H=64), dict(Ly=3), dict(C_=9), dict(T=1025), dict(K=9), dict(F=65), dict(K=0), dict(T=0), dict(B=-1)):
        assert lib.nsd_multi_path(C.byref(_d(L, **kw)), 5) == 0, kw
    assert lib.nsd_multi_path(None, 5) == 0


@pytest.mark.parametrize("M,B,T", [(1, 32, 40), (5, 32, 625), (25, 32, 625), (3, 171, 9), (32, 64, 100)])
def test_workspace_covers_the_single_model_workspace_of_all_trials(L, M, B, T):
    lib = L.lib()
    w, ws = L.WsLayout(), L.WsLayout()
    n = lib.nsd_multi_workspace_bytes(C.byref(_d(L, B=B, T=T)), M, C.byref(w))
    n1 = lib.nsd_workspace_bytes(C.byref(_d(L, B=M * B, T=T)), C.byref(ws))
    assert n >= n1 > 0
    assert w.total * 4 == n
    names = ["hseq", "cseq", "gact", "inseq", "top", "alpha", "pooled", "fc0_pre", "dscore", "dpooled", "loss", "adpack", "slabs", "hslabs"]
    offs = [getattr(w, k) for k in names]
    assert all(o % 4 == 0 for o in offs) and offs == sorted(offs)
    P = lib.nsd_param_count(8, 48, 2, 3, 32)
    p_lstm = 4 * 48 * 8 + 4 * 48 * 48 + 8 * 48 + 4 * 48 * 48 * 2 + 8 * 48
    assert w.hslabs - w.slabs >= w.n_slabs * p_lstm
    assert w.total - w.hslabs >= M * B * (P - p_lstm)
    assert w.n_slabs >= ws.n_slabs
    assert lib.nsd_multi_workspace_bytes(C.byref(_d(L, B=B, T=T)), 0, None) < 0


def test_slab_counts_follow_the_launch_plan(L):
    """n_slabs of nsd_workspace_bytes (M = 1) and nsd_multi_workspace_bytes (M = 2 .. 32) against an independent restatement of the
    backward's grid rule (plan48, csrc/nsd_lstm2.hip): one trial per workgroup up to 512 trials in the launch, two beyond; one
    workgroup per CU, the CUs partitioned by model; never fewer slabs than the single-model workspace of all M*B trials.  Without a
    device the library assumes the MI355X's 256 CUs, as this restatement does."""
    import torch
    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the restatement is written for 256 CUs")
    lib = L.lib()

    def single(B):
        nb = 1 if B <= 512 else 2
        return min(-(-B // nb), 256)

    def multi(M, B):
        nb = 1 if M * B <= 512 else 2
        return max(M * min(-(-B // nb), max(256 // M, 1)), single(M * B))

    w = L.WsLayout()
    for B in list(range(1, 80)) + [127, 128, 129, 255, 256, 257, 300, 511, 512, 513, 575, 1024, 1025, 2100]:
        assert lib.nsd_workspace_bytes(C.byref(_d(L, B=B)), C.byref(w)) > 0
        assert w.n_slabs == single(B), B
        for M in range(2, 33):
            assert lib.nsd_multi_workspace_bytes(C.byref(_d(L, B=B)), M, C.byref(w)) > 0
            assert w.n_slabs == multi(M, B), (M, B)


def test_refusals_before_any_launch(L):
    """Every refusal returns its code before a launch: the pointers below are never dereferenced (no GPU here)."""
    lib = L.lib()
    d = _d(L)
    fake = 0x1000
    big = 1 << 40
    r2 = (L.Rng * 2)(L.Rng(1, 4, 0.6, 0.6), L.Rng(2, 4, 0.5, 0.6))
    ok_r = (L.Rng * 2)(L.Rng(1, 4, 0.6, 0.6), L.Rng(2, 4, 0.6, 0.6))
    fwd = lambda M, rng=None, params=fake, nbytes=big, flags=0, stride=0: lib.nsd_multi_train_fwd(
        C.byref(d), M, params, fake, stride, C.cast(rng, C.c_void_p) if rng is not None else None, fake, flags, fake, nbytes, fake, None)
    assert fwd(0) == -1 and b"M = 0" in lib.nsd_last_error()
    assert fwd(33) == -1
    assert fwd(2, params=None) == -1 and b"null" in lib.nsd_last_error()
    assert fwd(2, rng=r2) == -1 and b"share" in lib.nsd_last_error()
    assert fwd(2, rng=ok_r, nbytes=16) == -3
    assert fwd(2, flags=1) == -1 and b"residual" in lib.nsd_last_error()
    assert fwd(2, stride=7) == -1 and b"x_model_stride" in lib.nsd_last_error()
    assert lib.nsd_multi_train_fwd(C.byref(_d(L, H=64)), 2, fake, fake, 0, None, fake, 0, fake, big, fake, None) == -1
    assert lib.nsd_multi_train_bwd(C.byref(d), 2, fake, fake, 0, C.cast(r2, C.c_void_p), 0, fake, big, None) == -1
    assert lib.nsd_multi_train_bwd(C.byref(d), 2, None, fake, 0, None, 0, fake, big, None) == -1
    assert lib.nsd_multi_grad_reduce(C.byref(d), 2, fake, 16, fake, None) == -3
    assert lib.nsd_multi_grad_reduce(C.byref(d), 2, fake, big, None, None) == -1
    assert lib.nsd_multi_grad_reduce_adam(C.byref(d), 2, fake, big, fake, fake, None, fake, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1, None) == -1
    assert lib.nsd_multi_loss_sum(C.byref(d), 40, fake, big, fake, None) == -1
    assert lib.nsd_multi_infer(C.byref(d), 2, None, fake, 0, 0, fake, None, None, None) == -1
    assert lib.nsd_multi_infer(C.byref(_d(L, C_=9)), 2, fake, fake, 0, 0, fake, None, None, None) == -1
    assert lib.nsd_multi_infer_scratch_bytes(C.byref(d), 3) >= 0


def test_python_refusals_name_the_rule():
    import nsd_amd
    from nsd_amd import multimodel
    with pytest.raises(nsd_amd.NsdError, match="no models"):
        multimodel._check_models([], "ModelBatchTrainer")
    a, b = nsd_amd.EEG_LSTM(), nsd_amd.EEG_LSTM(hidden_size=32)
    with pytest.raises(nsd_amd.NsdError, match="mixed shapes"):
        multimodel._check_models([a, b], "ModelBatchTrainer")
    with pytest.raises(nsd_amd.NsdError, match="nsd_multi_path"):
        multimodel._check_models([nsd_amd.EEG_LSTM(hidden_size=64)], "ModelBatchTrainer")
    with pytest.raises(nsd_amd.NsdError, match="nsd_multi_path"):
        multimodel._check_models([nsd_amd.EEG_LSTM() for _ in range(33)], "ModelBatchTrainer")
    with pytest.raises(nsd_amd.NsdError, match="more than once"):
        multimodel._check_models([a, a], "ModelBatchTrainer")
    with pytest.raises(nsd_amd.NsdError, match="mixed shapes"):
        multimodel._check_models([nsd_amd.EEG_LSTM(), nsd_amd.EEG_LSTM(normalize=True)], "EnsemblePredictor")


# ---- train.py --kfold K --concurrent [--kfold-seeds N] ----------------------------------------------------------------------------
def _y(n=324, k=3):
    import numpy as np
    return (np.arange(n) % k).astype(np.int32)


def test_concurrent_runs_are_the_sequential_folds_and_seeds():
    import numpy as np
    from nsd_amd import data as D
    from nsd_amd.train import concurrent_runs
    y = _y()
    runs = concurrent_runs(y, 5, 2, 7, 32)
    assert len(runs) == 10
    for i in range(2):
        folds = D.stratified_folds(y, 5, 7 + i)
        for f in range(5):
            r = runs[5 * i + f]
            assert r["seed_run"] == 7 + i and r["fold"] == f and r["seed"] == 7 + i + 101 * f     # train.py's sequential fit() seed
            assert np.array_equal(r["va"], folds[f]) and np.array_equal(r["tr"], np.setdiff1d(np.arange(len(y)), folds[f]))


def test_concurrent_refusals():
    from nsd_amd.train import concurrent_runs
    with pytest.raises(ValueError, match="fewer than --batch"):
        concurrent_runs(_y(60), 3, 1, 0, 41)                    # 40 training windows per fold
    with pytest.raises(ValueError, match="batches of 10 per epoch"):
        concurrent_runs(_y(44), 3, 1, 0, 10)                    # 29 / 29 / 30 training windows: 2 / 2 / 3 batches
    with pytest.raises(ValueError, match="at most 32"):
        concurrent_runs(_y(), 3, 11, 0, 32)


def test_concurrent_epoch_draws_each_folds_sequential_batches():
    import numpy as np
    from nsd_amd import data as D
    from nsd_amd.train import concurrent_epoch, concurrent_runs
    runs = concurrent_runs(_y(), 5, 1, 3, 32)
    for epoch in range(3):
        seen = []
        n = concurrent_epoch(runs, 32, epoch, lambda idxs: seen.append([ix.copy() for ix in idxs]))
        for k, r in enumerate(runs):
            ref = list(D.epoch_batches(len(r["tr"]), 32, r["seed"], epoch, drop_last=True))
            assert n == len(ref) == len(r["tr"]) // 32
            assert all(np.array_equal(a[k], b) for a, b in zip(seen, ref))


@pytest.mark.parametrize("argv,msg", [
    (["--synthetic", "64", "--kfold", "3", "--kfold-seeds", "2"], "needs --kfold K --concurrent"),
    (["--synthetic", "64", "--concurrent"], "K >= 2"),
    (["--synthetic", "64", "--kfold", "5", "--concurrent", "--kfold-seeds", "7"], "1 .. 32"),
    (["--synthetic", "64", "--kfold", "3", "--concurrent", "--hidden", "64"], "H = 48 fp32"),
    (["--synthetic", "64", "--kfold", "3", "--concurrent", "--precision", "bf16", "--hidden", "64"], "H = 48 fp32"),
])
def test_train_cli_refuses_concurrent_misuse(argv, msg, capsys):
    from nsd_amd.train import main
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert e.value.code == 2 and msg in capsys.readouterr().err
