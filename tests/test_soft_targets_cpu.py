"""Soft targets (nsd_mixup and the `_soft` entry points), the parts that need no GPU: the exported symbols, every refusal of the C entry
points, the numpy restatement the mixing kernel is held to (tests/mixup_ref.py) against torch's cross-entropy, the Loss dataclass
and the command-line flags."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import nsd_amd
from nsd_amd import _lib, ops, train
from tests import augment_ref as ar
from tests import mixup_ref as mr
from tests.train_cli import parse_train_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_WS = -1, -3
SOFT = ("nsd_mixup", "nsd_head_train_soft", "nsd_lstm_head_train_soft", "nsd_multi_train_fwd_soft", "nsd_seq_train_fwd_soft")
fake = 4096                                                        # never dereferenced: every refusal comes before a launch


def test_soft_symbols_are_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nsd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(nsd_[a-z0-9_]+)\s*\(", hdr))
    L = nsd_amd.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    for name in SOFT:
        assert name in declared and name in _lib.SYMBOLS, name
        assert hasattr(L, name) and name in exported, name
    assert "typedef struct nsd_mix" in hdr
    assert L.nsd_version() == 301                                  # additive: the version stays


# ---- refusals of nsd_mixup ------------------------------------------------------------------------------------------------------------
def _mix(L, d, M=1, x=fake, stride=0, labels=fake, w=None, mix=None, rng=True, step_dev=None, y=1 << 30, targets=1 << 31):
    m = mix if mix is not None else _lib.Mix(0.5, 0.1)
    r = (_lib.Rng * 32)()
    return L.nsd_mixup(C.byref(d) if d is not None else None, M, x, stride, labels, w, C.byref(m) if mix is not False else None,
                       C.cast(r, C.c_void_p) if rng else None, step_dev, y, targets, None)


def test_mixup_refusals_without_a_gpu():
    L = nsd_amd.load_library()
    d = _lib.Dims(4, 10, 8, 48, 2, 3, 32)
    n = 4 * 10 * 8
    for M in (0, -1, _lib.NSD_MAX_MODELS + 1):
        assert _mix(L, d, M=M) == E_INVALID and b"M =" in L.nsd_last_error()
    assert _mix(L, None) == E_INVALID
    assert _mix(L, d, labels=None) == E_INVALID and b"null" in L.nsd_last_error()
    assert _mix(L, d, targets=None) == E_INVALID
    assert _mix(L, d, rng=False) == E_INVALID
    assert _mix(L, d, mix=False) == E_INVALID
    for eps in (-0.1, 1.0, 2.0, float("nan")):
        assert _mix(L, d, mix=_lib.Mix(0.0, eps)) == E_INVALID and b"smoothing" in L.nsd_last_error()
    for m in (-0.1, 1.5, float("nan")):
        assert _mix(L, d, mix=_lib.Mix(m, 0.0)) == E_INVALID and b"mix" in L.nsd_last_error()
    for K in (0, -1, 65):
        assert _mix(L, _lib.Dims(4, 10, 8, 48, 2, K, 32)) == E_INVALID and b"K =" in L.nsd_last_error()
    # the windows: needed with mix > 0, and given together
    assert _mix(L, d, x=None, y=None) == E_INVALID and b"needs the windows" in L.nsd_last_error()
    assert _mix(L, d, x=None, y=None, mix=_lib.Mix(1.0, 0.0)) == E_INVALID
    assert _mix(L, d, x=None, mix=_lib.Mix(0.0, 0.0)) == E_INVALID and b"together" in L.nsd_last_error()
    assert _mix(L, d, y=None, mix=_lib.Mix(0.0, 0.0)) == E_INVALID
    assert _mix(L, d, M=3, stride=-1) == E_INVALID and b"x_model_stride" in L.nsd_last_error()
    assert _mix(L, d, M=3, stride=n - 1) == E_INVALID and b"x_model_stride" in L.nsd_last_error()
    assert _mix(L, d, x=fake, y=fake) == E_INVALID and b"overlaps" in L.nsd_last_error()
    assert _mix(L, d, x=fake, y=fake + 4 * (n - 1)) == E_INVALID
    assert _mix(L, d, M=3, x=fake + 4 * (3 * n - 1), y=fake) == E_INVALID
    assert _mix(L, d, M=3, stride=n, x=fake, y=fake + 4 * (3 * n - 1)) == E_INVALID
    assert _mix(L, _lib.Dims(4, 0, 8, 48, 2, 3, 32)) == E_INVALID
    assert _mix(L, _lib.Dims(4, 10, 0, 48, 2, 3, 32)) == E_INVALID
    # only B, T, C, K are read; B = 0 launches nothing; mix = 0 without windows is the targets-only call
    assert _mix(L, _lib.Dims(0, 10, 8, -5, 99, 3, 0)) == 0
    assert _mix(L, _lib.Dims(0, 10, 8, 48, 2, 64, 32), M=32, x=None, y=None, mix=_lib.Mix(0.0, 0.5)) == 0
    assert _mix(L, _lib.Dims(0, 10, 8, 48, 2, 1, 32), mix=_lib.Mix(1.0, 0.0)) == 0


# ---- refusals of the `_soft` entry points: those of their hard-label twins ---------------------------------------------------------------
def test_soft_entry_points_refuse_like_their_twins_without_a_gpu():
    L = nsd_amd.load_library()
    d = _lib.Dims(8, 20, 8, 48, 2, 3, 32)
    need = L.nsd_workspace_bytes(C.byref(d), None)
    rng = _lib.Rng(1, 4, 0.5, 0.5)
    err = lambda: L.nsd_last_error().decode()
    # short workspace -> NSD_E_WORKSPACE before any launch, with the twin's text under the soft name
    assert L.nsd_head_train_soft(C.byref(d), fake, None, None, fake, 1.0, fake, need - 4, fake, None) == E_WS
    assert err() == f"head_train_soft: workspace of {need - 4} bytes is smaller than nsd_workspace_bytes() = {need}"
    assert L.nsd_lstm_head_train_soft(C.byref(d), fake, fake, None, None, None, None, fake, 1.0, 2, fake, need - 4, fake, None) == E_WS
    assert err().startswith("lstm_head_train_soft: workspace of")
    assert L.nsd_lstm_head_train_soft(C.byref(d), fake, fake, None, None, None, C.byref(rng), fake, 1.0, 2, fake, need - 4, fake, None) == E_WS
    # null pointers
    assert L.nsd_head_train_soft(C.byref(d), fake, None, None, None, 1.0, fake, need, fake, None) == E_INVALID and "null" in err()
    assert L.nsd_head_train_soft(C.byref(d), None, None, None, fake, 1.0, fake, need, fake, None) == E_INVALID
    assert L.nsd_head_train_soft(C.byref(d), fake, None, None, fake, 1.0, fake, need, None, None) == E_INVALID
    assert L.nsd_head_train_soft(None, fake, None, None, fake, 1.0, fake, need, fake, None) == E_INVALID
    assert L.nsd_lstm_head_train_soft(C.byref(d), fake, fake, None, None, None, None, None, 1.0, 2, fake, need, fake, None) == E_INVALID and "null" in err()
    assert L.nsd_lstm_head_train_soft(C.byref(d), fake, None, None, None, None, None, fake, 1.0, 2, fake, need, fake, None) == E_INVALID
    assert L.nsd_lstm_head_train_soft(C.byref(d), fake, fake, None, None, None, None, fake, 1.0, 2, None, need, fake, None) == E_INVALID
    # masks and rng exclude each other; rng probabilities are checked; rng outside the single-launch shape is refused
    assert L.nsd_lstm_head_train_soft(C.byref(d), fake, fake, fake, None, None, C.byref(rng), fake, 1.0, 2, fake, need, fake, None) == E_INVALID
    assert "not both" in err()
    assert L.nsd_lstm_head_train_soft(C.byref(d), fake, fake, None, fake, None, C.byref(rng), fake, 1.0, 2, fake, need, fake, None) == E_INVALID
    bad = _lib.Rng(1, 4, 1.0, 0.5)
    assert L.nsd_lstm_head_train_soft(C.byref(d), fake, fake, None, None, None, C.byref(bad), fake, 1.0, 2, fake, need, fake, None) == E_INVALID
    d40 = _lib.Dims(3, 4, 5, 40, 1, 3, 32)
    need40 = L.nsd_workspace_bytes(C.byref(d40), None)
    assert L.nsd_rng_path(C.byref(d40)) == 0
    assert L.nsd_lstm_head_train_soft(C.byref(d40), fake, fake, None, None, None, C.byref(rng), fake, 1.0, 2, fake, need40, fake, None) == E_INVALID
    assert "nsd_rng_path" in err()
    # an empty batch is accepted and launches nothing, as for the twins
    d0 = _lib.Dims(0, 20, 8, 48, 2, 3, 32)
    need0 = L.nsd_workspace_bytes(C.byref(d0), None)
    assert L.nsd_head_train_soft(C.byref(d0), fake, None, None, fake, 1.0, fake, need0, fake, None) == 0
    assert L.nsd_lstm_head_train_soft(C.byref(d0), fake, fake, None, None, None, None, fake, 1.0, 2, fake, need0, fake, None) == 0
    assert L.nsd_head_train_soft(C.byref(d0), fake, None, None, fake, 1.0, fake, need0 - 4, fake, None) == E_WS

    # model-batched
    M = 3
    needm = L.nsd_multi_workspace_bytes(C.byref(d), M, None)
    rngs = (_lib.Rng * M)(*[_lib.Rng(m, 4, 0.5, 0.5) for m in range(M)])
    rp = C.cast(rngs, C.c_void_p)
    assert L.nsd_multi_train_fwd_soft(C.byref(d), M, fake, fake, 0, rp, fake, 0, fake, needm - 4, fake, None) == E_WS
    assert err() == f"multi_train_fwd_soft: workspace of {needm - 4} bytes is smaller than nsd_multi_workspace_bytes() = {needm}"
    assert L.nsd_multi_train_fwd_soft(C.byref(d), M, fake, fake, 0, rp, None, 0, fake, needm, fake, None) == E_INVALID and "null" in err()
    assert L.nsd_multi_train_fwd_soft(C.byref(d), 0, fake, fake, 0, rp, fake, 0, fake, needm, fake, None) == E_INVALID
    assert L.nsd_multi_train_fwd_soft(C.byref(d), 33, fake, fake, 0, rp, fake, 0, fake, needm, fake, None) == E_INVALID
    assert L.nsd_multi_train_fwd_soft(C.byref(d), M, fake, fake, 0, rp, fake, 1, fake, needm, fake, None) == E_INVALID      # residual
    assert L.nsd_multi_train_fwd_soft(C.byref(d), M, fake, fake, 5, rp, fake, 0, fake, needm, fake, None) == E_INVALID      # stride
    assert L.nsd_multi_train_fwd_soft(C.byref(d40), M, fake, fake, 0, rp, fake, 0, fake, needm, fake, None) == E_INVALID    # shape
    rngs[1].p_head = 0.25
    assert L.nsd_multi_train_fwd_soft(C.byref(d), M, fake, fake, 0, rp, fake, 0, fake, needm, fake, None) == E_INVALID and "share" in err()

    # bf16 sequence path
    ds = _lib.Dims(37, 5, 8, 64, 2, 5, 32)
    needs = L.nsd_seq_workspace_bytes(C.byref(ds), 0)
    assert needs > 0
    rc = L.nsd_seq_train_fwd_soft(C.byref(ds), fake, fake, None, fake, 1.0, 0, fake, needs - 1, fake, None)
    rc_twin = L.nsd_seq_train_fwd(C.byref(ds), fake, fake, None, fake, 1.0, 0, fake, needs - 1, fake, None)
    assert rc == rc_twin == E_WS
    for args in ((None, fake, fake, fake), (fake, None, fake, fake), (fake, fake, None, fake), (fake, fake, fake, None)):
        p, x, tg, lg = args
        assert L.nsd_seq_train_fwd_soft(C.byref(ds), p, x, None, tg, 1.0, 0, fake, needs, lg, None) == E_INVALID, args
    assert L.nsd_seq_train_fwd_soft(C.byref(ds), fake, fake, None, fake, 1.0, 0, None, needs, fake, None) == E_INVALID
    assert L.nsd_seq_train_fwd_soft(C.byref(d), fake, fake, None, fake, 1.0, 0, fake, needs, fake, None) == E_INVALID       # H = 48
    assert L.nsd_seq_train_fwd_soft(C.byref(ds), fake, fake, None, fake, 1.0, 1 << 20, fake, needs, fake, None) == E_INVALID


# ---- the numpy restatement by itself --------------------------------------------------------------------------------------------------
def _x(B, T, Cc, seed=0):
    return (2.7 * np.random.RandomState(seed).standard_normal((B, T, Cc))).astype(np.float32)


@pytest.mark.parametrize("B", [2, 3, 5, 33])
def test_partner_map_is_a_bijection_without_fixed_points(B):
    for seed, base in ((1, 4), (0x9E3779B97F4A7C15, 400), (7, 4 * 0x3FFFFFFF), (99, 8), (100, 8), (101, 12)):
        p = mr.partner(B, seed, base)
        assert sorted(p) == list(range(B)) and np.all(p != np.arange(B)), (B, seed, base)
        assert np.array_equal(p, (np.arange(B) + (p[0] - 0) % B) % B)       # a rotation
    if B > 2:                                                               # the rotation depends on the draw
        assert len({int(mr.partner(B, s, 4)[0]) for s in range(40)}) > 1


def test_all_off_gives_exact_one_hot_rows_and_leaves_x_alone():
    x = _x(5, 7, 3)
    x[0, 0, 0], x[1, 2, 1] = -0.0, np.nan
    labels = np.array([0, 2, 1, 1, 0])
    y, tg = mr.mixup(x, labels, 3, 9, 4)
    assert tg.dtype == np.float32 and np.array_equal(tg, np.eye(3, dtype=np.float32)[labels])
    assert y is not x and np.array_equal(y.view(np.uint32), x.view(np.uint32))
    # B = 1 with mixing on, and mix = 0 with the other parts on: the windows stay, the row is base(label) exactly
    y1, tg1 = mr.mixup(x[:1], labels[:1], 3, 9, 4, mix=1.0, eps=0.1, weights=[1.0, 2.0, 0.5])
    assert np.array_equal(y1.view(np.uint32), x[:1].view(np.uint32)) and np.array_equal(tg1, mr.base_rows(labels[:1], 3, 0.1, [1.0, 2.0, 0.5]))
    y0, tg0 = mr.mixup(x, labels, 3, 9, 4, mix=0.0, eps=0.1, weights=[1.0, 2.0, 0.5])
    assert np.array_equal(y0.view(np.uint32), x.view(np.uint32)) and np.array_equal(tg0, mr.base_rows(labels, 3, 0.1, [1.0, 2.0, 0.5]))
    assert mr.mixup(None, labels, 3, 9, 4, eps=0.1)[0] is None


def test_lambda_range_and_model_independence():
    lam, mu = mr.lambdas(4000, 0.75, 5, 8)
    assert lam.dtype == np.float32 and lam.min() >= 0.25 and lam.max() <= 1.0 and 0.6 < lam.mean() < 0.65
    assert np.array_equal(mu, np.float32(1.0) - lam)
    x = _x(6, 5, 4, 2)
    lab = np.array([[0, 1, 2, 0, 1, 2]] * 3)
    y3, t3 = mr.mixup_models(x, lab, 3, [(10, 4), (20, 4), (30, 4)], mix=1.0, eps=0.1)
    y1, t1 = mr.mixup(x, lab[1], 3, 20, 4, mix=1.0, eps=0.1)
    assert np.array_equal(y3[1], y1) and np.array_equal(t3[1], t1) and not np.array_equal(y3[0], y3[1])
    # the slots are not nsd_augment's: shift (slot 0), scale (1), channel drops (256 + c), and the per-element indices have the top bit clear
    assert mr.LAMBDA_SLOT >= 256 + 256 and int(mr.ROT_INDEX) >> 62 == 3
    assert int(ar.trial_index(np.array([0xFFFF_FFFF]), 0xFFFF)[0]) >> 62 == 2       # no per-trial index reaches the rotation's


@pytest.mark.parametrize("K,B,eps,mix,weighted", [(3, 5, 0.0, 0.0, False), (3, 5, 0.1, 0.0, False), (3, 5, 0.0, 0.0, True), (3, 5, 0.0, 1.0, False),
                                                  (5, 33, 0.2, 0.7, True), (8, 6, 0.05, 1.0, True), (64, 6, 0.3, 0.5, True), (2, 1, 0.1, 1.0, True)])
def test_reference_targets_are_torchs_cross_entropy(K, B, eps, mix, weighted):
    """float64: the reference's target rows give the per-trial loss and dlogits of F.cross_entropy(logits, mixed one-hot rows,
    weight=w, label_smoothing=eps, reduction='none') to 1e-12."""
    rs = np.random.RandomState(K * 100 + B)
    logits = 3.0 * rs.standard_normal((B, K))
    labels = rs.randint(0, K, B)
    w = (0.25 + rs.rand(K)).astype(np.float32) if weighted else None
    if weighted:
        w[rs.randint(K)] = 0.0                                      # a class that does not count
    seed, base = 1234 + K, 8
    _, q = mr.mixup(np.zeros((B, 1, 1), np.float32), labels, K, seed, base, mix=mix, eps=eps, weights=w, dtype=np.float64)
    loss, dl = mr.soft_ce(logits, q)
    onehot = np.eye(K)[labels]
    if np.float32(mix) != 0 and B >= 2:
        lam, mu = mr.lambdas(B, mix, seed, base, np.float64)
        onehot = lam[:, None] * onehot + mu[:, None] * onehot[mr.partner(B, seed, base)]
    lt = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
    ref = torch.nn.functional.cross_entropy(lt, torch.tensor(onehot, dtype=torch.float64), weight=None if w is None else torch.tensor(w, dtype=torch.float64),
                                            label_smoothing=float(np.float32(eps)), reduction="none")
    ref.sum().backward()
    assert np.abs(loss - ref.detach().numpy()).max() <= 1e-12
    assert np.abs(dl - lt.grad.numpy()).max() <= 1e-12
    if eps == 0 and mix == 0 and not weighted:                      # hard labels: torch's index form too
        hard = torch.nn.functional.cross_entropy(torch.tensor(logits), torch.tensor(labels), reduction="none").numpy()
        assert np.abs(loss - hard).max() <= 1e-12
    # the fp32 rows the kernel is held to are these rows rounded
    _, q32 = mr.mixup(np.zeros((B, 1, 1), np.float32), labels, K, seed, base, mix=mix, eps=eps, weights=w)
    assert q32.dtype == np.float32 and np.abs(q32 - q).max() <= 4 * 2.0 ** -24 * max(1.0, float(np.abs(q).max()))


# ---- Python surface -------------------------------------------------------------------------------------------------------------------
def test_loss_dataclass():
    Ls = nsd_amd.Loss
    assert Ls().enabled is False and Ls(label_smoothing=0.0, class_weights=None, mixup=0.0) == Ls()
    for kw in (dict(label_smoothing=0.1), dict(mixup=0.5), dict(mixup=1.0), dict(class_weights=[1.0, 1.0, 1.0])):
        assert Ls(**kw).enabled is True
    assert Ls(class_weights=[1, 2, 0]).class_weights == (1.0, 2.0, 0.0)
    for kw in (dict(label_smoothing=-0.1), dict(label_smoothing=1.0), dict(label_smoothing=float("nan")), dict(mixup=-0.1), dict(mixup=1.5),
               dict(mixup=float("nan")), dict(class_weights=[1.0, -1.0]), dict(class_weights=[float("inf"), 1.0]),
               dict(class_weights=[float("nan")]), dict(class_weights=[])):
        with pytest.raises(ValueError):
            Ls(**kw)
    with pytest.raises(ValueError):
        Ls(class_weights=[1.0, 2.0]).check_classes(3)
    Ls(class_weights=[1.0, 2.0, 3.0]).check_classes(3)
    with pytest.raises(Exception):
        Ls().mixup = 0.5                                           # frozen
    assert ops.Loss is Ls


def test_trainers_still_refuse_on_the_cpu_with_a_loss():
    """No device here: the trainers raise their own NsdError (there is no CPU training path), loss= or not."""
    from nsd_amd.trainer import Trainer
    with pytest.raises(nsd_amd.NsdError, match="no CPU training path"):
        Trainer(nsd_amd.EEG_LSTM(), loss=nsd_amd.Loss(mixup=0.5))
    with pytest.raises(nsd_amd.NsdError):
        nsd_amd.ModelBatchTrainer([nsd_amd.EEG_LSTM(), nsd_amd.EEG_LSTM()], loss=nsd_amd.Loss(label_smoothing=0.1))


def test_balanced_weights_on_the_packed_three_class_fixture():
    from nsd_amd import data as D
    ts = D.load_trials_npz(os.path.join(ROOT, "tests", "golden", "recorded_trials.npz"), D.LABELS_3CLASS_CHECKPOINT)
    y = ts.y
    n = np.bincount(y, minlength=3)
    assert n.sum() == len(y) and np.all(n > 0)
    w = train.balanced_class_weights(y, 3)
    assert w == tuple(len(y) / (3 * int(c)) for c in n)
    assert abs(sum(wk * c for wk, c in zip(w, n)) - len(y)) < 1e-9          # the weighted trial count is the trial count
    tr, _ = D.stratified_split(y, 0.2, 0)
    a = train.loss_for(train.argparse.Namespace(label_smoothing=0.1, class_weights="balanced", mixup=0.0, classes=3), y[tr])
    assert a.class_weights == train.balanced_class_weights(y[tr], 3) and a.label_smoothing == 0.1
    assert train.balanced_class_weights(np.array([0, 0, 2]), 3) == (0.5, 0.0, 1.0)     # an absent class weighs nothing
    assert train.parse_class_weights("1,2.5,0", 3) == (1.0, 2.5, 0.0) and train.parse_class_weights(None, 3) is None
    for bad in ("1,2", "a,b,c", "1,-2,3", "1,2,inf"):
        with pytest.raises(ValueError):
            train.parse_class_weights(bad, 3)


def test_cli_loss_flags_parse(monkeypatch):
    seen = parse_train_args(["--synthetic", "16", "--label-smoothing", "0.1", "--class-weights", "balanced", "--mixup", "0.5"], monkeypatch)
    a = seen["args"]
    assert (a.label_smoothing, a.class_weights, a.mixup) == (0.1, "balanced", 0.5) and seen.get("reached_device")
    a = parse_train_args(["--synthetic", "16", "--class-weights", "1,2,0.5", "--kfold", "5", "--concurrent"], monkeypatch)["args"]
    assert a.class_weights == "1,2,0.5" and train.loss_for(a, np.array([0, 1, 2])).class_weights == (1.0, 2.0, 0.5)
    d = parse_train_args(["--synthetic", "16"], monkeypatch)["args"]
    assert (d.label_smoothing, d.class_weights, d.mixup) == (0.0, None, 0.0) and not train.loss_for(d, np.array([0, 1, 2])).enabled


@pytest.mark.parametrize("bad", [["--label-smoothing", "1.0"], ["--label-smoothing", "-0.1"], ["--mixup", "1.5"], ["--mixup", "-1"],
                                 ["--class-weights", "1,2"], ["--class-weights", "x"], ["--class-weights", "1,-1,1"]])
def test_cli_loss_out_of_range_is_an_argparse_error_before_any_device(bad, monkeypatch, capsys):
    with pytest.raises(SystemExit) as e:
        parse_train_args(["--synthetic", "16"] + bad, monkeypatch)
    assert e.value.code == 2 and "error:" in capsys.readouterr().err
