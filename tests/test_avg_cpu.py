"""Weight averaging in the step tail (nsd_avg, include/nsd.h) on the host: the numpy restatement of the rule (tests/avg_ref.py) against
torch.optim.swa_utils.AveragedModel in float64, its start / stride / skip bookkeeping, and through ctypes the size function and every
refusal of the `_avg` entry points with its text -- every call below is refused, or returns, before a launch.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

import nsd_amd
from nsd_amd import _lib, ops
from tests.avg_ref import EMA, SWA, AveragedWeights

FAKE = 4096                                                         # never dereferenced
E_INVALID, E_WORKSPACE = -1, -3
AVG_SYMBOLS = {"nsd_avg_state_bytes", "nsd_avg_state_init", "nsd_grad_reduce_clip_adam_avg", "nsd_multi_grad_reduce_clip_adam_avg",
               "nsd_multi_grad_reduce_clip_adam_avg_each", "nsd_adam_step_clip_avg"}


def _err(L):
    return L.nsd_last_error().decode()


def _opts(M):
    arr = (_lib.Opt * M)()
    for m in range(M):
        for k, v in dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_scale=1.0, max_norm=0.0, sched=0, warmup_steps=0,
                         total_steps=0, step_size=1, min_ratio=0.0, gamma=1.0).items():
            setattr(arr[m], k, v)
    return arr


def _avgs(M, last=None, **bad):
    """M valid EMA entries; the LAST one takes `bad` (or is `last`, a whole tuple)"""
    arr = (_lib.Avg * M)(*[_lib.Avg(1, 0.9, 1, 1) for _ in range(M)])
    if last is not None:
        arr[M - 1] = _lib.Avg(*last)
    for k, v in bad.items():
        setattr(arr[M - 1], k, v)
    return arr


# the refusals of one nsd_avg, as (fields, text); EMA-only decay checks included
BAD_AVG = [(dict(mode=3), "mode 3 unknown (NSD_AVG_EMA / NSD_AVG_SWA)"), (dict(mode=-1), "mode -1 unknown (NSD_AVG_EMA / NSD_AVG_SWA)"),
           (dict(decay=1.0), "decay 1 outside [0, 1) or NaN"), (dict(decay=-0.25), "decay -0.25 outside [0, 1) or NaN"),
           (dict(decay=float("nan")), "decay nan outside [0, 1) or NaN"), (dict(start_step=0), "start_step 0 must be >= 1"),
           (dict(every=0), "every 0 must be >= 1")]


@pytest.mark.parametrize("decay", [0.5, 0.9, 0.999, None])
def test_restatement_equals_torch_averaged_model_in_float64(decay):
    """40 updates of 1000 uniform(-1, 1) values: EMA through get_ema_multi_avg_fn(decay), SWA (decay None) through AveragedModel's
    default.  Bound 1e-12 (the two differ by the association of a handful of float64 operations on values below 1)."""
    rng = np.random.default_rng(7)
    holder = torch.nn.Module()
    holder.w = torch.nn.Parameter(torch.zeros(1000, dtype=torch.float64))
    am = AveragedModel(holder) if decay is None else AveragedModel(holder, multi_avg_fn=get_ema_multi_avg_fn(decay))
    ref = AveragedWeights(SWA if decay is None else EMA, decay=decay or 0.0, dtype=np.float64)
    worst = 0.0
    for s in range(1, 41):
        p = rng.uniform(-1.0, 1.0, 1000)
        with torch.no_grad():
            holder.w.copy_(torch.from_numpy(p))
        am.update_parameters(holder)
        assert ref.update(p, s)
        worst = max(worst, float(np.abs(am.module.w.detach().numpy() - ref.row).max()))
    print(f"decay {decay}: max |restatement - AveragedModel| = {worst:.3g}")
    assert ref.n == 40 and int(am.n_averaged) == 40 and worst <= 1e-12


def test_start_stride_and_skip_bookkeeping():
    a = AveragedWeights(SWA, start_step=3, every=2)
    ps = [np.full(4, float(s), np.float32) for s in range(8)]
    took = [s for s in range(1, 8) if a.update(ps[s], s, skipped=(s == 5))]
    assert took == [3, 7] and a.n == 2 and np.array_equal(a.row, np.full(4, 5.0, np.float32))          # mean of 3 and 7
    b = AveragedWeights(EMA, decay=0.75, start_step=2)
    assert not b.update(ps[1], 1) and b.row is None and b.n == 0
    assert b.update(ps[2], 2) and np.array_equal(b.row, ps[2]) and b.row is not ps[2]                     # the first one copies
    assert b.update(ps[6], 3) and np.array_equal(b.row, np.full(4, 3.0, np.float32)) and b.n == 2       # 2 + 0.25 * (6 - 2)
    # float32 runs round where the kernel rounds: w = 1.0f - decay
    assert AveragedWeights(EMA, decay=0.999).w == np.float32(1.0) - np.float32(0.999) != 1.0 - 0.999


def test_the_feature_is_detected_by_its_symbols_and_the_size_function():
    L = nsd_amd.load_library()
    assert L.nsd_version() == 301 and AVG_SYMBOLS <= set(_lib.SYMBOLS) and all(hasattr(L, s) for s in AVG_SYMBOLS)
    assert C.sizeof(_lib.Avg) == 16 and (_lib.NSD_AVG["ema"], _lib.NSD_AVG["swa"]) == (EMA, SWA) == (1, 2)
    for n, M in ((0, 1), (1, 1), (31764, 1), (31764, 25), ((1 << 20) + 1, 1), (31764, 32)):
        assert L.nsd_avg_state_bytes(n, M) == 16 * M + 4 * M * n == ops.avg_state_bytes(n, M)
    for n, M in ((-1, 1), (5, 0), (5, 33)):
        assert L.nsd_avg_state_bytes(n, M) == E_INVALID and _err(L).startswith("avg_state_bytes: n = ")
    assert L.nsd_avg_state_init(None, 64, 1, None) == E_INVALID and _err(L) == "avg_state_init: avg_state is NULL or shorter than 1 records"
    assert L.nsd_avg_state_init(FAKE, 47, 3, None) == E_INVALID and _err(L) == "avg_state_init: avg_state is NULL or shorter than 3 records"
    assert L.nsd_avg_state_init(FAKE, 64, 0, None) == E_INVALID and _err(L) == "avg_state_init: M = 0 (1 <= M <= 32)"


def test_refusals_of_the_flat_route():
    """the twin's refusals first, then avg's fields, then avg_state: NULL, short"""
    L = nsd_amd.load_library()
    who, n = "adam_step_clip_avg", 1000
    ob, ab = L.nsd_opt_state_bytes(n, 1), L.nsd_avg_state_bytes(n, 1)

    def call(avg, p=FAKE, step=1, state=FAKE, st_bytes=ob, astate=FAKE, a_bytes=ab - 4):
        return L.nsd_adam_step_clip_avg(n, p, FAKE, FAKE, FAKE, C.cast(_opts(1), C.c_void_p), step, None, None, state, st_bytes, None,
                                        C.cast(avg, C.c_void_p) if avg is not None else None, astate, a_bytes)
    assert call(_avgs(1), p=None) == E_INVALID and _err(L) == f"{who}: null pointer or n<0"
    assert call(_avgs(1), step=0) == E_INVALID and _err(L) == f"{who}: step 0 must be >= 1 (or pass step_dev)"
    assert call(_avgs(1), st_bytes=ob - 8) == E_WORKSPACE and _err(L).startswith(f"{who}: opt_state of {ob - 8} bytes is smaller")
    assert call(None) == E_INVALID and _err(L) == f"{who}: avg is NULL"
    for bad, text in BAD_AVG + [(dict(mode=0), "mode 0 unknown (NSD_AVG_EMA / NSD_AVG_SWA)")]:
        assert call(_avgs(1, **bad), astate=None) == E_INVALID and _err(L) == f"{who}: {text}", bad
    assert call(_avgs(1), astate=None) == E_INVALID and _err(L) == f"{who}: avg_state is NULL"
    assert call(_avgs(1)) == E_WORKSPACE and _err(L) == f"{who}: avg_state of {ab - 4} bytes is smaller than nsd_avg_state_bytes() = {ab}"
    # decay is EMA's alone: SWA with any decay passes the field checks and reaches the size check
    assert call(_avgs(1, last=(SWA, float("nan"), 1, 1))) == E_WORKSPACE


@pytest.mark.parametrize("sym,M", [("nsd_grad_reduce_clip_adam_avg", 1), ("nsd_multi_grad_reduce_clip_adam_avg", 3),
                                   ("nsd_multi_grad_reduce_clip_adam_avg_each", 3), ("nsd_multi_grad_reduce_clip_adam_avg_each", 1)])
def test_refusals_of_the_fused_tails(sym, M):
    """dims / shape and pointers as the twin, opt, the step, opt_state, then avg (entry by entry with the index named in `_each`, where
    mode 0 is allowed), avg_state, and last the workspace"""
    L = nsd_amd.load_library()
    who, each, multi = sym[4:], sym.endswith("_each"), "multi" in sym
    d = _lib.Dims(4, 10, 8, 48, 2, 3, 32)
    need = L.nsd_multi_workspace_bytes(C.byref(d), M, None) if multi else L.nsd_workspace_bytes(C.byref(d), None)
    P = L.nsd_param_count(8, 48, 2, 3, 32)
    ob, ab = L.nsd_opt_state_bytes(P, M), L.nsd_avg_state_bytes(P, M)

    def call(avg, grads=FAKE, step=1, state=FAKE, astate=FAKE, a_bytes=ab, ws=FAKE, bytes_=need - 4, opts=True):
        head = (C.byref(d),) + ((M,) if multi else ())
        return getattr(L, sym)(*head, ws, bytes_, grads, FAKE, FAKE, FAKE, C.cast(_opts(M), C.c_void_p) if opts else None, step, None, state, ob, None,
                               C.cast(avg, C.c_void_p) if avg is not None else None, astate, a_bytes)
    assert call(_avgs(M, mode=7), grads=None) == E_INVALID and _err(L) == f"{who}: null pointer"
    assert call(_avgs(M, mode=7), opts=False) == E_INVALID and _err(L) == f"{who}: opt is NULL"
    assert call(_avgs(M, mode=7), step=0) == E_INVALID and _err(L) == f"{who}: step 0 must be >= 1 (or pass step_dev)"
    assert call(_avgs(M, mode=7), state=None) == E_INVALID and _err(L) == f"{who}: opt_state is NULL"
    assert call(None) == E_INVALID and _err(L) == f"{who}: avg is NULL"
    for bad, text in BAD_AVG:                         # (one nsd_avg for all models: ONE entry is read)
        assert call(_avgs(M if each else 1, **bad), astate=None) == E_INVALID
        assert _err(L) == (f"{who}: avg[{M - 1}]: {text}" if each else f"{who}: {text}"), bad
    if not each:                                      # 0 is no mode outside `_each`
        assert call(_avgs(1, mode=0), astate=None) == E_INVALID and _err(L) == f"{who}: mode 0 unknown (NSD_AVG_EMA / NSD_AVG_SWA)"
    else:                                             # mode 0 in an entry: that model does not average, whatever its other fields say
        assert call(_avgs(M, last=(0, 5.0, -3, 0)), astate=None) == E_INVALID and _err(L) == f"{who}: avg_state is NULL"
    assert call(_avgs(M), astate=None) == E_INVALID and _err(L) == f"{who}: avg_state is NULL"
    assert call(_avgs(M), a_bytes=ab - 4) == E_WORKSPACE
    assert _err(L) == f"{who}: avg_state of {ab - 4} bytes is smaller than nsd_avg_state_bytes() = {ab}"
    # (the single-model twin counts the workspace among its pointers, as nsd_grad_reduce_clip_adam does)
    assert call(_avgs(M), ws=None) == E_INVALID and _err(L) == (f"{who}: workspace is NULL" if multi else f"{who}: null pointer")
    assert call(_avgs(M)) == E_WORKSPACE and _err(L).startswith(f"{who}: workspace of {need - 4} bytes is smaller than ")


def test_python_settings():
    with pytest.raises(ValueError, match="kind 'mean'"):
        ops.Average("mean")
    for kw, msg in ((dict(decay=1.0), "decay 1.0 outside"), (dict(decay=math.nan), "decay nan outside"), (dict(start_step=0), "start_step 0 must be"),
                    (dict(every=0), "every 0 must be"), (dict(every=1.5), "every 1.5 must be")):
        with pytest.raises(ValueError, match=msg):
            ops.Average("ema", **kw)
    assert ops.Average("swa", decay=7.0).struct().mode == SWA                        # decay is EMA's alone
    s = ops.Average("ema", 0.99, start_step=5, every=2).struct()
    assert (s.mode, s.start_step, s.every) == (EMA, 5, 2) and s.decay == np.float32(0.99)
    off = ops._avg_struct(None)
    assert (off.mode, off.start_step, off.every) == (0, 1, 1)
    # a grid axis like lr: once or per model, None entries allowed; equal entries take the single setting's route
    a, b = ops.Average("ema", 0.9), ops.Average("swa")
    assert ops._per_model([a, ops.Average("ema", 0.9)], 2, "avg") == (a, None) and ops._per_model([a, None, b], 3, "avg") == (None, [a, None, b])
    assert ops._per_model([None, None], 2, "avg") == (None, None)
    with pytest.raises(nsd_amd.NsdError, match="2 entries for 3 models"):
        ops._per_model([a, b], 3, "multi: avg")


def test_trainers_refuse_before_they_need_a_gpu():
    from nsd_amd.lstm_eeg_model import EEG_LSTM
    from nsd_amd.multimodel import ModelBatchTrainer
    from nsd_amd.trainer import Trainer
    with pytest.raises(nsd_amd.NsdError, match="needs the model on the MI355X"):
        Trainer(EEG_LSTM(), average=ops.Average("swa"))
    with pytest.raises(nsd_amd.NsdError):
        ModelBatchTrainer([EEG_LSTM(), EEG_LSTM()], average=[ops.Average("swa"), None])
    row = torch.zeros(EEG_LSTM().spec.param_count + 1)
    with pytest.raises(nsd_amd.NsdError, match="view_of: row must be"):
        EEG_LSTM().view_of(row)
    m = EEG_LSTM()
    twin = m.view_of(m.flat_parameters().clone())                 # a module on a row: same keys, the row's values, eval mode
    assert not twin.training and twin.state_dict().keys() == m.state_dict().keys()
    assert all(torch.equal(v, m.state_dict()[k]) for k, v in twin.state_dict().items())
    twin.flat_parameters().zero_()
    assert all(float(v.abs().max()) == 0.0 for v in twin.state_dict().values()) and float(m.flat_parameters().abs().max()) > 0.0
