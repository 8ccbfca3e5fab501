"""Early stopping for model batches on the host: the float64 restatement of nsd_multi_eval (tests/eval_ref.py) against torch, the
early-stopping rule on written-down trajectories, the declarations of the new symbols, the library's refusals (they come before any
launch, so they are reachable without a device), the drivers' option checks and the inner split.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import nsd_amd
from nsd_amd import _lib, data as D, grid, ops, train
from tests import eval_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nsd_multi_eval_path", "nsd_select_state_bytes", "nsd_select_state_init", "nsd_multi_eval")


def scripted_logits(B, K, seed, scale=3.0):
    rs = np.random.RandomState(seed)
    return (scale * rs.standard_normal((B, K))).astype(np.float32), rs.randint(0, K, B).astype(np.int32)


@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("B", [1, 2, 255, 256, 257, 1025])
def test_restatement_loss_is_torch_cross_entropy_in_float64(B, K):
    lg, y = scripted_logits(B, K, seed=B * 10 + K)
    lg[0] *= 27.0                                                       # a row of magnitude ~80
    rec = er.eval_record(lg, y)
    want = torch.nn.functional.cross_entropy(torch.from_numpy(lg).double(), torch.from_numpy(y).long(), reduction="sum").item()
    assert rec["n"] == B and rec["nonfinite"] == 0
    assert abs(rec["loss_sum"] - want) <= 1e-12 * max(abs(want), 1e-300) or (K == 1 and rec["loss_sum"] == want == 0.0)


def test_restatement_argmax_and_confusion_are_torchs_ties_included():
    lg, y = scripted_logits(300, 5, seed=1)
    lg[::7, 3] = lg[::7, 1] = np.abs(lg[::7]).max(axis=1) + 1.0        # exact two-way ties at the maximum: index 1 wins
    lg[5] = 0.25                                                        # a row of equal logits: index 0
    rec = er.eval_record(lg, y)
    pred = torch.from_numpy(lg).double().argmax(-1).numpy()             # torch's argmax returns the first maximal index too
    assert (pred[::7] == 1).all() and pred[5] == 0
    conf = np.zeros((8, 8), dtype=np.int64)
    np.add.at(conf, (y, pred), 1)
    assert np.array_equal(rec["confusion"], conf) and rec["correct"] == int((pred == y).sum()) == int(np.trace(conf))


def test_restatement_counts_padding_and_nonfinite_rows():
    lg, y = scripted_logits(40, 3, seed=2)
    base = er.eval_record(lg[:30], y[:30])
    lg2, y2 = lg.copy(), y.copy()
    lg2[30:] = np.nan
    y2[30:35], y2[35:] = -7, 99
    assert er.pack_eval(er.eval_record(lg2, y2, count=30)) == er.pack_eval(base)
    lg2[4, 1] = np.inf
    y2[9] = 3                                                           # a label outside [0, K) among the counted rows
    rec = er.eval_record(lg2, y2, count=30)
    assert rec["nonfinite"] == 2 and rec["n"] == 28 and np.isnan(rec["loss_sum"]) and rec["confusion"].sum() == 28


def test_lane_tree_sum_is_the_documented_order():
    v = np.random.RandomState(3).rand(1025)
    lanes = [0.0] * 256
    for i, x in enumerate(v):
        lanes[i % 256] += float(x)
    s = 128
    while s:
        for i in range(s):
            lanes[i] += lanes[i + s]
        s //= 2
    assert er.lane_tree_sum(v) == lanes[0]


def ev(mean, n=10, correct=5):
    return dict(loss_sum=mean * n, n=n, correct=correct)


def test_rule_on_written_down_trajectories():
    s = er.Selector(1, "loss", patience=2, min_delta=0.01)
    got = [s.offer([ev(m)])[0] for m in (1.0, 0.8, 0.795, 0.7, 0.75, 0.72, 0.1)]
    #       first   better  within min_delta  better  bad 1  bad 2 -> stopped  ignored
    assert got == [True, True, False, True, False, False, False]
    r = s.records[0]
    assert (r["best_eval"], r["evals"], r["bad"], r["stopped"], s.held[0]) == (4, 6, 2, 1, 3) and r["best_loss"] == 0.7 * 10 / 10
    s = er.Selector(1, "loss", patience=0)
    assert [s.offer([ev(m)])[0] for m in (1.0, 2.0, 3.0, 4.0, 0.5)] == [True, False, False, False, True] and not s.records[0]["stopped"]
    s = er.Selector(1, "loss", patience=3)
    s.offer([ev(1.0)])
    assert s.offer([dict(loss_sum=float("nan"), n=9, correct=0)]) == [False]
    assert (s.records[0]["status"], s.records[0]["bad"], s.held[0]) == (1, 1, 0)
    s = er.Selector(1, "acc", patience=0, min_delta=0.05)
    got = [s.offer([ev(m, 20, c)])[0] for m, c in ((1.0, 10), (0.9, 10), (0.95, 10), (0.5, 11), (0.9, 12))]
    #       first           tie, lower loss  tie, higher loss  +0.05 is not MORE than 0.05   +0.10
    assert got == [True, True, False, False, True] and s.records[0]["best_correct"] == 12


def test_header_binding_and_makefile_declare_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "nsd.h")).read()
    assert int(re.search(r"#define NSD_VERSION (\d+)", hdr).group(1)) == 301              # additive: detected by the symbols
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(nsd_[a-z0-9_]+)\s*\(", code))
    L = nsd_amd.load_library()
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(L, name), name
    for macro, val in (("NSD_SELECT_LOSS", 0), ("NSD_SELECT_ACC", 1), ("NSD_EVAL_MAX_K", 8)):
        assert int(re.search(rf"#define {macro}\s+(\d+)", hdr).group(1)) == val == getattr(_lib, macro)
    assert C.sizeof(_lib.Select) == 12 and C.sizeof(_lib.EvalRecord) == er.EVAL_BYTES and C.sizeof(_lib.SelectRecord) == er.SELECT_BYTES
    assert "nsd_eval.hip" in open(os.path.join(ROOT, "neural-speech-decoding_amd", "csrc", "Makefile")).read()
    for name in ("evaluate", "track_best", "restore_best", "stopped", "all_stopped", "best_evals", "best_state_dict"):
        assert hasattr(nsd_amd.ModelBatchTrainer, name), name
    # the state: M records padded to 16 bytes, then [M][P] floats
    for M, P in ((1, 1), (2, 5), (3, 19875), (32, 7)):
        assert int(L.nsd_select_state_bytes(M, P)) == (40 * M + 15) // 16 * 16 + 4 * M * P == ops.select_records_bytes(M) + 4 * M * P
    assert int(L.nsd_select_state_bytes(0, 4)) < 0 and int(L.nsd_select_state_bytes(33, 4)) < 0 and int(L.nsd_select_state_bytes(2, 0)) < 0
    assert L.nsd_multi_eval_path(32, 1025, 8, 0) == 1 and L.nsd_multi_eval_path(1, 1, 1, 5) == 1
    assert not any(L.nsd_multi_eval_path(*a) for a in ((0, 4, 3, 0), (33, 4, 3, 0), (2, 0, 3, 0), (2, 4, 0, 0), (2, 4, 9, 0), (2, 4, 3, -1),
                                                       (32, 2 ** 31 // 64, 8, 0)))


def test_refusals_happen_on_the_host_without_a_gpu():
    """every refusal of nsd_multi_eval / nsd_select_state_init comes before any launch: reachable, and named, with no device"""
    L = nsd_amd.load_library()
    A = 0x1000                                                          # any non-null address: nothing is dereferenced before a launch
    M, B, K, P = 3, 16, 3, 10
    sbytes = int(L.nsd_select_state_bytes(M, P))
    good = _lib.Select(0, 2, 0.0)

    def call(M=M, B=B, K=K, logits=A, labels=A, counts=None, out=A, sel=good, params=A, P=P, state=A, nbytes=sbytes):
        cp = (C.c_int32 * len(counts))(*counts) if counts is not None else None
        return L.nsd_multi_eval(M, B, K, logits, labels, cp, out, C.byref(sel) if sel is not None else None, params, P, state, nbytes, None)

    def err():
        return L.nsd_last_error().decode()

    for kw, word in ((dict(M=0), "M = 0"), (dict(M=33), "M = 33"), (dict(K=0), "K = 0"), (dict(K=9), "K = 9"), (dict(B=0), "B = 0"),
                     (dict(counts=[16, 0, 16]), "counts[1] = 0"), (dict(counts=[16, 16, 17]), "counts[2] = 17"), (dict(counts=[-1, 1, 1]), "counts[0]"),
                     (dict(M=32, B=2 ** 31 // 64, K=8), "M * B * K"), (dict(logits=None), "logits"), (dict(labels=None), "labels"),
                     (dict(out=None), "out"), (dict(sel=_lib.Select(2, 0, 0.0)), "metric"), (dict(sel=_lib.Select(-1, 0, 0.0)), "metric"),
                     (dict(sel=_lib.Select(0, -1, 0.0)), "patience"), (dict(sel=_lib.Select(1, 0, -1e-3)), "min_delta"),
                     (dict(sel=_lib.Select(1, 0, float("nan"))), "min_delta"), (dict(params=None), "params"), (dict(state=None), "sel_state"),
                     (dict(P=0), "P = 0")):
        assert call(**kw) == -1 and word in err(), (kw, err())
    assert call(nbytes=sbytes - 1) == -3 and "nsd_select_state_bytes" in err()
    assert L.nsd_select_state_init(None, sbytes, M, P, None) == -1 and "sel_state" in err()
    assert L.nsd_select_state_init(A, sbytes, 0, P, None) == -1 and L.nsd_select_state_init(A, sbytes, M, 0, None) == -1
    assert L.nsd_select_state_init(A, sbytes - 1, M, P, None) == -3 and "nsd_select_state_bytes" in err()


def test_ops_argument_checks_raise_before_the_library_is_asked():
    lg, y = torch.zeros(2, 4, 3), torch.zeros(2, 4, dtype=torch.int32)
    with pytest.raises(_lib.NsdError, match=r"\[M,B,K\]"):
        ops.multi_eval(lg[0], y)
    with pytest.raises(_lib.NsdError, match="labels"):
        ops.multi_eval(lg, y)                                           # host tensors: there is no CPU path
    with pytest.raises(_lib.NsdError, match="bytes"):
        ops.eval_records(torch.zeros(10, dtype=torch.uint8), 2, 3)
    raw = torch.frombuffer(bytearray(er.pack_eval(er.eval_record(*scripted_logits(9, 3, 4))) * 2), dtype=torch.uint8)
    recs = ops.eval_records(raw, 2, 3)
    assert recs[0]["n"] == 9 and recs[1]["confusion"].shape == (3, 3) and recs[0]["loss"] == recs[0]["loss_sum"] / 9
    sel = dict(best_loss=0.5, best_correct=3, best_n=9, best_eval=2, evals=4, bad=2, stopped=1, status=1)
    raw = torch.frombuffer(bytearray(er.pack_select(sel) + er.pack_select(er.new_select_record())), dtype=torch.uint8)
    assert ops.select_records(raw, 2) == [sel, er.new_select_record()]


def run_main(main, argv, capsys):
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_driver_options_are_checked_before_anything_runs(capsys):
    base = ["--synthetic", "64", "--T", "12"]
    cc = base + ["--kfold", "3", "--concurrent"]
    assert "--kfold K --concurrent" in run_main(train.main, base + ["--early-stop-patience", "3"], capsys)
    assert "--kfold K --concurrent" in run_main(train.main, base + ["--kfold", "3", "--inner-fraction", "0.2"], capsys)
    assert "--kfold K --concurrent" in run_main(train.main, base + ["--early-stop-metric", "acc"], capsys)
    assert "needs --early-stop-patience" in run_main(train.main, cc + ["--early-stop-min-delta", "0.1"], capsys)
    assert "negative" in run_main(train.main, cc + ["--early-stop-patience", "-1"], capsys)
    assert "--early-stop-min-delta" in run_main(train.main, cc + ["--early-stop-patience", "2", "--early-stop-min-delta", "-0.5"], capsys)
    for f in ("0", "0.51", "-0.2", "nan"):
        assert "outside (0, 0.5]" in run_main(train.main, cc + ["--early-stop-patience", "2", "--inner-fraction", f], capsys)
        assert "outside (0, 0.5]" in run_main(grid.main, base + ["--kfold", "3", "--early-stop-patience", "2", "--inner-fraction", f], capsys)
    assert "invalid choice" in run_main(train.main, cc + ["--early-stop-patience", "2", "--early-stop-metric", "f1"], capsys)
    assert "negative" in run_main(grid.main, base + ["--kfold", "3", "--early-stop-patience", "-2"], capsys)
    ap = train.build_parser()
    assert train.early_stop_settings(ap.parse_args(cc), True) is None                      # nothing asked for: nothing changes
    es = train.early_stop_settings(ap.parse_args(cc + ["--early-stop-patience", "5"]), True)
    assert es == dict(metric="loss", patience=5, min_delta=0.0, inner_fraction=0.2)
    assert train.selection_text(es) == "inner split: early stopping on loss, patience 5"
    assert train.selection_text(None) == "none: fixed epoch count, last-epoch model"
    es = train.early_stop_settings(grid.build_parser().parse_args(["--early-stop-patience", "0", "--early-stop-metric", "acc", "--inner-fraction",
                                                                   "0.5", "--early-stop-min-delta", "0.01"]), True)
    assert es == dict(metric="acc", patience=0, min_delta=0.01, inner_fraction=0.5)


def test_inner_split_is_stratified_disjoint_from_the_outer_fold_and_reproducible():
    rs = np.random.RandomState(5)
    y = rs.permutation(np.repeat([0, 1, 2], [110, 105, 110])).astype(np.int32)
    plain = train.concurrent_runs(y, 5, 2, 7, 32)
    runs = train.concurrent_runs(y, 5, 2, 7, 32, inner_fraction=0.2)
    again = train.concurrent_runs(y, 5, 2, 7, 32, inner_fraction=0.2)
    assert len(runs) == 10
    for p, r, a in zip(plain, runs, again):
        assert np.array_equal(r["va"], p["va"]) and r["seed"] == p["seed"]                  # the outer folds are those of the plain runs
        assert np.array_equal(np.sort(np.concatenate([r["tr"], r["inner"]])), p["tr"])      # fit + inner = the fold's training trials
        assert not set(r["inner"]) & set(r["tr"]) and not set(r["inner"]) & set(r["va"]) and not set(r["tr"]) & set(r["va"])
        assert np.array_equal(r["tr"], a["tr"]) and np.array_equal(r["inner"], a["inner"])
        fit_rel, inner_rel = D.stratified_split(y[p["tr"]], 0.2, r["seed"])                   # the split is the run's seed's
        assert np.array_equal(r["inner"], p["tr"][inner_rel]) and np.array_equal(r["tr"], p["tr"][fit_rel])
        for cls in range(3):                                                                # every class gives round(0.2 * its count)
            assert int((y[r["inner"]] == cls).sum()) == int(round(0.2 * int((y[p["tr"]] == cls).sum())))
    assert any(not np.array_equal(runs[0]["inner"], r["inner"]) for r in runs[1:])
    with pytest.raises(ValueError, match="fewer than"):                                     # the checks apply to the fit part
        train.concurrent_runs(y, 5, 1, 0, 250, inner_fraction=0.2)
    train.concurrent_runs(y, 5, 1, 0, 250)
    x_all = torch.arange(20, dtype=torch.float32).view(20, 1, 1).expand(20, 2, 3).contiguous()
    xs, ys, counts = train.padded_parts(x_all, torch.arange(20, dtype=torch.int32), [np.array([3, 4, 5]), np.array([7, 9])])
    assert counts == [3, 2] and tuple(xs.shape) == (2, 3, 2, 3) and ys.tolist() == [[3, 4, 5], [7, 9, 7]] and xs[1, 2, 0, 0] == 7
