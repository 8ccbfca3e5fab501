"""Device-resident batches (nsd_gather), the parts that need no GPU: BatchSchedule against the host loops it restates, its refusals, the
row rule of the numpy restatement (tests/gather_ref.py), the refusals of the C entry point, the bound-schedule bookkeeping of
StepRecipe (on CPU tensors: nothing is launched) and the command-line flag."""
import ctypes as C

import numpy as np
import pytest
import torch

import nsd_amd
from nsd_amd import _lib, ops
from nsd_amd import data as D
from nsd_amd import step_recipe as sr
from nsd_amd.train import concurrent_epoch, concurrent_runs
from tests import gather_ref as gr
from tests.train_cli import parse_train_args

E_INVALID = -1


# ---- BatchSchedule restates the host loops --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 7])
@pytest.mark.parametrize("n,batch", [(37, 8), (40, 8), (9, 9)])
def test_for_run_is_the_fit_loop(seed, n, batch):
    epochs = 3
    tr_idx = np.sort(np.random.RandomState(5).permutation(100)[:n])
    s = D.BatchSchedule.for_run(tr_idx, batch, seed, epochs)
    want = [tr_idx[idx] for e in range(epochs) for idx in D.epoch_batches(n, batch, seed, e, drop_last=True)]
    assert s.table.dtype == np.int32 and s.table.shape == (1, len(want), batch)
    assert s.M == 1 and s.steps == len(want) and s.batch == batch and s.steps_per_epoch == n // batch and s.epochs == epochs
    for row, w in zip(s.table[0], want):
        assert np.array_equal(row, w)
    # the epochs differ, and so do the seeds
    assert not np.array_equal(s.table[0, :s.steps_per_epoch], s.table[0, s.steps_per_epoch:2 * s.steps_per_epoch])
    assert not np.array_equal(s.table, D.BatchSchedule.for_run(tr_idx, batch, seed + 1, epochs).table)


@pytest.mark.parametrize("seed", [0, 3])
def test_for_runs_is_concurrent_epoch(seed):
    """folds of unequal size (50 trials in 3 folds: 17 / 17 / 16 held out) that draw the same number of batches"""
    y = np.random.RandomState(1).randint(0, 3, 50)
    runs = concurrent_runs(y, 3, 1, seed, 8)
    assert len({len(r["tr"]) for r in runs}) > 1
    epochs = 3
    s = D.BatchSchedule.for_runs(runs, 8, epochs)
    seen = []
    per_epoch = [concurrent_epoch(runs, 8, e, lambda idxs: seen.append([r["tr"][ix] for r, ix in zip(runs, idxs)])) for e in range(epochs)]
    assert s.table.shape == (3, len(seen), 8) and s.steps_per_epoch == per_epoch[0] and len(set(per_epoch)) == 1
    for j, step in enumerate(seen):
        for m, idx in enumerate(step):
            assert np.array_equal(s.table[m, j], idx), (j, m)
    for m, r in enumerate(runs):                                   # a run trains on its own trials only
        assert set(s.table[m].ravel()) <= set(r["tr"].tolist())


def test_schedule_refusals():
    idx = np.arange(20)
    with pytest.raises(ValueError, match="fewer than one batch"):
        D.BatchSchedule.for_run(idx[:5], 8, 0, 2)
    with pytest.raises(ValueError, match="short tail batch of 4"):
        D.BatchSchedule.for_run(idx, 8, 0, 2, drop_last=False)
    assert D.BatchSchedule.for_run(idx, 5, 0, 2, drop_last=False).steps == 8          # 20 = 4 x 5: no tail to keep
    with pytest.raises(ValueError, match="batch 0"):
        D.BatchSchedule.for_run(idx, 0, 0, 2)
    with pytest.raises(ValueError, match="epochs 0"):
        D.BatchSchedule.for_run(idx, 4, 0, 0)
    with pytest.raises(ValueError, match="no runs"):
        D.BatchSchedule.for_runs([], 4, 1)
    with pytest.raises(ValueError, match="run 1.*fewer than one batch"):
        D.BatchSchedule.for_runs([dict(tr=idx, seed=0), dict(tr=idx[:3], seed=1)], 4, 1)
    with pytest.raises(ValueError, match="same count"):
        D.BatchSchedule.for_runs([dict(tr=idx, seed=0), dict(tr=idx[:9], seed=1)], 4, 1)
    with pytest.raises(ValueError, match=r"\[M,S,B\]"):
        D.BatchSchedule(np.zeros((4, 3), np.int32), 1)
    with pytest.raises(ValueError, match="not trial indices"):
        D.BatchSchedule(np.zeros((1, 4, 3), np.float32), 1)
    with pytest.raises(ValueError, match="negative"):
        D.BatchSchedule(np.full((1, 4, 3), -1), 1)
    with pytest.raises(ValueError, match="whole number of epochs"):
        D.BatchSchedule(np.zeros((1, 4, 3), np.int64), 3)
    s = D.BatchSchedule(np.full((1, 4, 3), 6), 2)
    s.check_trials(7)
    with pytest.raises(ValueError, match="trial index 6 for a set of 6"):
        s.check_trials(6)


def test_device_trial_set_forms():
    x = np.zeros((5, 4, 3), np.float64)
    t = D.DeviceTrialSet(x, np.arange(5, dtype=np.int64), "cpu")
    assert len(t) == 5 and t.x.dtype == torch.float32 and t.labels.dtype == torch.int32 and t.targets is None and t.y is t.labels
    t = D.DeviceTrialSet(torch.zeros(5, 4, 3), np.zeros((5, 2), np.float32), "cpu")
    assert t.labels is None and tuple(t.targets.shape) == (5, 2) and t.y is t.targets
    for bad in (lambda: D.DeviceTrialSet(np.zeros((5, 4)), np.zeros(5, np.int32), "cpu"),
                lambda: D.DeviceTrialSet(x, np.zeros(4, np.int32), "cpu"), lambda: D.DeviceTrialSet(x, np.zeros(5, np.float32), "cpu"),
                lambda: D.DeviceTrialSet(x, np.zeros((5, 2), np.int32), "cpu")):
        with pytest.raises(ValueError):
            bad()


# ---- the numpy restatement by itself ---------------------------------------------------------------------------------------------------
def test_row_rule_of_the_reference():
    S = 4
    assert [gr.row(c, 10, S) for c in range(10, 14)] == [0, 1, 2, 3]                  # inside the table
    assert [gr.row(c, 10, S) for c in (9, 8, 7, 6, 5, -1)] == [3, 2, 1, 0, 3, 1]      # below the base: non-negative
    assert [gr.row(c, 10, S) for c in (14, 17, 18, 21)] == [0, 3, 0, 3]               # one and two wraps past base + S
    assert gr.row(0, 0, 1) == 0 and gr.row(-5, 3, 1) == 0
    x_all = np.arange(3 * 2 * 2, dtype=np.float32).reshape(3, 2, 2)
    x_all[1, 0, 0] = np.array([0x7FA00001], np.uint32).view(np.float32)[0]            # a signalling NaN payload travels as bits
    table = np.array([[[0, 1], [2, 2]], [[1, 3], [-1, 0]]], np.int32)
    lab, tg = np.array([5, 6, 7], np.int32), np.arange(6, dtype=np.float32).reshape(3, 2)
    xo, lo, to, st = gr.gather(x_all, table, 4, 4, lab, tg)
    words = x_all.view(np.uint32)
    assert np.array_equal(xo[0], words[[0, 1]]) and np.array_equal(xo[1, 0], words[1]) and (xo[1, 1] == gr.NAN32).all()
    assert lo.tolist() == [5, 6, 6, 0] and (to[3] == gr.NAN32).all() and np.array_equal(to[:3], tg.view(np.uint32)[[0, 1, 1]])
    assert st.tolist() == [0, 1]
    xo, lo, _, st = gr.gather(x_all, table, 5, 4, lab)
    assert np.array_equal(xo[0], words[[2, 2]]) and (xo[1, 0] == gr.NAN32).all() and lo.tolist() == [7, 7, 0, 5] and st.tolist() == [0, 1]


# ---- the C entry point's refusals ------------------------------------------------------------------------------------------------------
def _gather(L, d, M=1, N=7, x_all=4096, labels_all=None, targets_all=None, table=1 << 20, S=4, x=1 << 30, labels=None, targets=None,
            status=None):
    return L.nsd_gather(C.byref(d) if d is not None else None, M, N, x_all, labels_all, targets_all, table, S, 0, None, 0, x, labels, targets,
                        status, None)


def test_gather_refusals_without_a_gpu():
    L = nsd_amd.load_library()
    d = _lib.Dims(3, 5, 3, 48, 2, 3, 32)
    err = lambda: L.nsd_last_error()
    assert _gather(L, None) == E_INVALID and b"dims" in err()
    for M in (0, -1, _lib.NSD_MAX_MODELS + 1):
        assert _gather(L, d, M=M) == E_INVALID and b"M =" in err()
    for kw in (dict(N=0), dict(N=-3), dict(S=0), dict(S=-1)):
        assert _gather(L, d, **kw) == E_INVALID and b"N =" in err(), kw
    for bad in (_lib.Dims(-1, 5, 3, 48, 2, 3, 32), _lib.Dims(3, 0, 3, 48, 2, 3, 32), _lib.Dims(3, 5, 0, 48, 2, 3, 32)):
        assert _gather(L, bad) == E_INVALID and b"shape" in err()
    for kw in (dict(x_all=None), dict(table=None), dict(x=None)):
        assert _gather(L, d, **kw) == E_INVALID and b"null" in err(), kw
    assert _gather(L, d, labels=1 << 29) == E_INVALID and b"labels without labels_all" in err()
    assert _gather(L, d, targets=1 << 29) == E_INVALID and b"targets without targets_all" in err()
    assert _gather(L, _lib.Dims(3, 5, 3, 48, 2, 0, 32), targets_all=1 << 28, targets=1 << 29) == E_INVALID and b"K =" in err()
    n_all, n_out = 7 * 15 * 4, 3 * 15 * 4                                               # bytes of x_all and of x
    assert _gather(L, d, x_all=4096, x=4096) == E_INVALID and b"overlaps" in err()
    assert _gather(L, d, x_all=4096, x=4096 + n_all - 4) == E_INVALID                   # x begins in x_all's last float
    assert _gather(L, d, x_all=4096 + n_out - 4, x=4096) == E_INVALID                   # x_all begins in x's last float
    assert _gather(L, _lib.Dims(0, 5, 3, 48, 2, 3, 32), x_all=4096, x=4096 + n_all) == 0   # ... and side by side is fine (B = 0: no launch)
    assert _gather(L, _lib.Dims(2 ** 20, 64, 8, 48, 2, 3, 32), M=4, x=1 << 50) == E_INVALID and b"M * B * T * C" in err()
    assert _gather(L, _lib.Dims(2 ** 16, 1, 1, 48, 2, 3, 32), M=2, S=2 ** 15, x=1 << 50) == E_INVALID and b"M * S * B" in err()
    # B = 0 launches nothing; an input without its output is ignored; only B, T, C are read
    assert _gather(L, _lib.Dims(0, 5, 3, -5, 99, 0, 0)) == 0
    assert _gather(L, _lib.Dims(0, 5, 3, 48, 2, 0, 32), labels_all=1 << 27, targets_all=1 << 28, M=32) == 0
    # the path query is the shape checks
    q = lambda dd, M=1, N=7, S=4: L.nsd_gather_path(C.byref(dd), M, N, S)
    assert q(d) == 1 and q(d, M=32) == 1 and q(_lib.Dims(0, 5, 3, 0, 0, 0, 0)) == 1
    assert q(d, M=0) == 0 and q(d, M=33) == 0 and q(d, N=0) == 0 and q(d, S=0) == 0 and q(_lib.Dims(3, 0, 3, 48, 2, 3, 32)) == 0
    assert q(_lib.Dims(2 ** 20, 64, 8, 48, 2, 3, 32), M=4) == 0 and q(_lib.Dims(2 ** 16, 1, 1, 48, 2, 3, 32), M=2, S=2 ** 15) == 0
    assert L.nsd_gather_path(None, 1, 7, 4) == 0
    assert L.nsd_version() == 301                                                      # additive: detected by the symbols


def test_gather_batch_refuses_bad_tensors_before_the_library():
    x_all, table = torch.zeros(7, 5, 3), torch.zeros(2, 4, 3, dtype=torch.int32)
    with pytest.raises(ops.NsdError, match=r"\[N,T,C\]"):
        ops.gather_batch(x_all[0], table)
    with pytest.raises(ops.NsdError, match="table must be int32"):
        ops.gather_batch(x_all, table[0, 0])
    with pytest.raises(ops.NsdError, match="table must be a contiguous int32 device tensor"):
        ops.gather_batch(x_all, table)                                                 # (a CPU tensor: there is no CPU path)


# ---- the bound schedule's bookkeeping (StepRecipe.bind / take) -------------------------------------------------------------------------
def test_bind_rotates_an_equal_shaped_schedule_in_place_and_counts_steps():
    trials = D.DeviceTrialSet(np.zeros((9, 4, 2), np.float32), np.arange(9, dtype=np.int32), "cpu")
    s1 = D.BatchSchedule(np.arange(8).reshape(1, 4, 2), 2)
    b, kept = sr.StepRecipe.bind(None, trials, s1, 1, 6, "t")
    assert not kept and b["base"] == 6 and tuple(b["table"].shape) == (4, 2) and tuple(b["x"].shape) == (2, 4, 2)
    for j in range(4):                                              # step 6 + j reads row j
        assert gr.row(6 + j, b["base"], 4) == j
        sr.StepRecipe.take(b, "t")
    with pytest.raises(ops.NsdError, match="4 steps are taken"):
        sr.StepRecipe.take(b, "t")
    with pytest.raises(ops.NsdError, match="no batches bound"):
        sr.StepRecipe.take(None, "t")
    # the next schedule, bound after only 3 more steps than a multiple of S: the rows are rotated, base and addresses stay
    addr = b["table"].data_ptr()
    s2 = D.BatchSchedule(8 - np.arange(8).reshape(1, 4, 2), 4)
    b2, kept = sr.StepRecipe.bind(b, trials, s2, 1, 13, "t")
    assert kept and b2 is b and b["base"] == 6 and b["table"].data_ptr() == addr and b["taken"] == 0 and b["first"] == 13
    for j in range(4):
        assert np.array_equal(b["table"][gr.row(13 + j, 6, 4)].numpy(), s2.table[0, j])
    # another shape, other trials, a wrong model count, an index outside the set
    assert not sr.StepRecipe.bind(b, trials, D.BatchSchedule(np.zeros((1, 2, 2), np.int32), 1), 1, 13, "t")[1]
    other = D.DeviceTrialSet(np.zeros((9, 4, 2), np.float32), np.arange(9, dtype=np.int32), "cpu")
    assert not sr.StepRecipe.bind(b, other, s2, 1, 13, "t")[1]
    with pytest.raises(ops.NsdError, match="holds 1 models' batches, the trainer 3"):
        sr.StepRecipe.bind(None, trials, s1, 3, 1, "t")
    with pytest.raises(ops.NsdError, match="trial index 9 for a set of 9"):
        sr.StepRecipe.bind(None, trials, D.BatchSchedule(np.full((1, 2, 2), 9), 1), 1, 1, "t")
    b3, _ = sr.StepRecipe.bind(None, trials, D.BatchSchedule(np.zeros((3, 2, 2), np.int32), 1), 3, 1, "t")
    assert tuple(b3["table"].shape) == (3, 2, 2) and tuple(b3["x"].shape) == (3, 2, 4, 2) and tuple(b3["y"].shape) == (6,)
    assert b3["status"].tolist() == [0, 0, 0]
    sr.StepRecipe.check_gather(b3, "t")
    b3["status"][1] = 1
    with pytest.raises(ops.NsdError, match=r"model\(s\) \[1\]"):
        sr.StepRecipe.check_gather(b3, "t")


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def test_cli_flag_parses_and_defaults_off(monkeypatch):
    seen = parse_train_args(["--synthetic", "32", "--T", "20"], monkeypatch)
    assert seen["args"].device_batches is False
    seen = parse_train_args(["--synthetic", "32", "--T", "20", "--device-batches"], monkeypatch)
    assert seen["args"].device_batches is True and seen.get("reached_device")
    from nsd_amd import grid
    assert grid.build_parser().parse_args(["--kfold", "2", "--device-batches"]).device_batches is True
