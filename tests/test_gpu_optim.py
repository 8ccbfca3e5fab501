"""Global-norm clipping and learning-rate schedules in the step tail (nsd_opt of include/nsd.h) on the MI355X: the flat route
(nsd_grad_norm + nsd_adam_step_clip), the fused tail (nsd_grad_reduce_clip_adam), the model-batched tail, the non-finite guard, the
schedule evaluated from the device step counter, both trainers, the bf16 path, two ranks, and the buffer contract of the four
launching entry points.  Run with `pytest -m gpu -s`: every comparison prints its figures before it asserts.

References never come from the kernels: tests/optim_ref.py (float64; tests/test_optim_cpu.py pins it to torch) and, for the bitwise
claims, the existing entry points nsd_grad_reduce / nsd_grad_reduce_adam / nsd_adam_step.

Bounds:
  norm, coef, lr of a record    1 fp32 ulp of the float64 value formed from the same gradient: the squares are exact in double and the
                                sum of n <= 2^20 + 1 of them is good to ~1e-13 relative, so only the final rounding to fp32 can differ
  p, m, v against float64       1e-6 absolute, the bound of test_gpu_parity.py::test_adam_matches_oracle_and_torch (seven fp32 steps at
                                lr = 1e-3 on |p| <= 1: each step rounds p once, <= 6e-8); device- against host-step: the same 1e-6, the
                                bound of test_graph_replay_step_equals_eager_step for the device's pow against libm's
  bitwise                       wherever the header promises bits: unclipped constant-schedule steps against today's entry points, grads
                                against nsd_grad_reduce, a model of a batched launch against the single-model call on its slabs, ranks
                                against each other, side streams and graph replays against the plain call.
"""
import contextlib
import ctypes as C
import math
import os
import socket

import numpy as np
import pytest
import torch

from tests import buffer_contract as bc
from tests import optim_ref as ref
from tests.golden.make_goldens import synth_labels, synth_params, synth_x
from tests.gpu_harness import dev, head_inputs, nsd, to_dev  # noqa: F401  (dev, nsd: fixtures)

pytestmark = pytest.mark.gpu

TOL = 1e-6
LR = 1e-3


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """bit for bit (NaN payloads included)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _ulps(a: float, b: float) -> int:
    """distance of two fp32 values in units in the last place; NaN == NaN, Inf == Inf"""
    a, b = np.float32(a), np.float32(b)
    if np.isnan(a) or np.isnan(b):
        return 0 if np.isnan(a) and np.isnan(b) else 1 << 30
    ia, ib = int(a.view(np.int32)), int(b.view(np.int32))
    return abs(ia - ib)


def _lr32(f: float) -> float:
    """lr_eff as the header forms it: (float)((double)lr * f) with lr the fp32 field"""
    return float(np.float32(ref.f32(LR) * f))


def _records(ops, state, M=1):
    torch.cuda.synchronize()
    return ops.opt_records(state, M)


def _err(t: torch.Tensor, want: np.ndarray) -> float:
    return float(np.abs(t.detach().cpu().numpy().astype(np.float64) - want).max())


# ---- direct calls of the tails on a workspace that holds an evaluation's slabs -------------------------------------------------------
def _tail_clip(ops, spec, B, T, ws, grads, p, m, v, opt, state, step=1, step_dev=None):
    d = spec.dims(B, T)
    ops._call("nsd_grad_reduce_clip_adam", ws.device, C.byref(d), ws.data_ptr(), ops._nbytes(ws), grads.data_ptr(), p.data_ptr(), m.data_ptr(),
              v.data_ptr(), C.byref(opt), step, None if step_dev is None else step_dev.data_ptr(), state.data_ptr(), ops._nbytes(state), ops.STREAM)


def _tail_plain(ops, spec, B, T, ws, grads, p, m, v, step=1, lr=LR, wd=0.0):
    d = spec.dims(B, T)
    ops._call("nsd_grad_reduce_adam", ws.device, C.byref(d), ws.data_ptr(), ops._nbytes(ws), grads.data_ptr(), p.data_ptr(), m.data_ptr(),
              v.data_ptr(), lr, 0.9, 0.999, 1e-8, wd, 1.0, step, ops.STREAM)


def _multi_tail_clip(ops, spec, M, B, T, ws, grads, p, m, v, opt, state, step=1):
    d = spec.dims(B, T)
    ops._call("nsd_multi_grad_reduce_clip_adam", ws.device, C.byref(d), M, ws.data_ptr(), ops._nbytes(ws), grads.data_ptr(), p.data_ptr(),
              m.data_ptr(), v.data_ptr(), C.byref(opt), step, None, state.data_ptr(), ops._nbytes(state), ops.STREAM)


def _moments(n, seed):
    """Adam moments of a run in progress: m ~ 1e-3 N(0, 1), v ~ 1e-6 U(0, 1)"""
    rs = np.random.RandomState(seed)
    return (1e-3 * rs.standard_normal(n)).astype(np.float32), (1e-6 * rs.random_sample(n)).astype(np.float32)


def _ref_step(p0, m0, v0, g, step, **kw):
    R = ref.ClippedAdam(p0, lr=LR, step=step - 1, **kw)
    R.m, R.v = m0.astype(np.float64), v0.astype(np.float64)
    rec = R.step(g)
    return R, rec


# ---- 1. flat route -------------------------------------------------------------------------------------------------------------------
FLAT_N = [1, 3, 33, 31764, 2**20 + 1]


def _flat_problem(n):
    rs = np.random.RandomState(n % 9973)
    p0 = rs.uniform(-1, 1, n).astype(np.float32)
    gs = [rs.standard_normal(n).astype(np.float32) for _ in range(7)]
    return p0, gs, [ref.grad_norm(g)[1] for g in gs]


def _flat_run(ops, dev, p0, gs, opt, state, skip=None):
    p, m, v = to_dev(p0, dev), torch.zeros(len(p0), device=dev), torch.zeros(len(p0), device=dev)
    recs = []
    for s, g in enumerate(gs, 1):
        gt = to_dev(g, dev)
        ops.grad_norm(gt, state, opt.grad_scale)
        ops.adam_step_clip(p, gt, m, v, opt, state, step=s, skip=skip)
        recs.append(_records(ops, state)[0])
    return p, m, v, recs


@pytest.mark.parametrize("n", FLAT_N)
def test_flat_route_clipped_against_float64(nsd, dev, n):
    """max_norm = 0.1 |g_1|, seven steps, weight decay on: record within 1 ulp per step, p / m / v within 1e-6 of optim_ref"""
    from nsd_amd import ops
    p0, gs, norms = _flat_problem(n)
    kw = dict(weight_decay=1e-2, max_norm=0.1 * norms[0], grad_scale=0.5)
    opt, state = ops.opt_struct(lr=LR, **kw), ops.opt_state(n, 1, dev)
    p, m, v, recs = _flat_run(ops, dev, p0, gs, opt, state)
    R = ref.ClippedAdam(p0, lr=LR, **kw)
    worst = 0
    for g, rec in zip(gs, recs):
        want = R.step(g)
        u = (_ulps(rec["norm"], want["norm"]), _ulps(rec["coef"], want["coef"]), _ulps(rec["lr"], LR))
        worst = max(worst, *u)
        assert rec["skipped"] == 0
    errs = (_err(p, R.p), _err(m, R.m), _err(v, R.v))
    print(f"[flat clipped] n={n}: record ulps <= {worst}, coef_1 {recs[0]['coef']:.4f}, |dp| {errs[0]:.2e} |dm| {errs[1]:.2e} |dv| {errs[2]:.2e}")
    assert recs[0]["coef"] < 1.0                               # the first step clips by construction
    assert worst <= 1 and max(errs) <= TOL


@pytest.mark.parametrize("n", FLAT_N)
def test_flat_route_unclipped_is_adam_step_bitwise(nsd, dev, n):
    """max_norm = 10 max |g| and max_norm = 0 with a constant schedule: p, m, v bitwise what nsd_adam_step leaves, seven steps"""
    from nsd_amd import ops
    p0, gs, norms = _flat_problem(n)
    pa, ma, va = to_dev(p0, dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    for s, g in enumerate(gs, 1):
        ops.adam_step(pa, to_dev(g, dev), ma, va, step=s, lr=LR, weight_decay=1e-2, grad_scale=0.5)
    for max_norm in (10.0 * max(norms), 0.0):
        opt, state = ops.opt_struct(lr=LR, weight_decay=1e-2, grad_scale=0.5, max_norm=max_norm), ops.opt_state(n, 1, dev)
        p, m, v, recs = _flat_run(ops, dev, p0, gs, opt, state)
        assert all(r["coef"] == 1.0 and r["skipped"] == 0 for r in recs)
        assert _same(p, pa) and _same(m, ma) and _same(v, va), (n, max_norm)
        assert _ulps(recs[-1]["norm"], ref.grad_norm(gs[-1], 0.5)[1]) <= 1


def test_flat_route_honours_skip(nsd, dev):
    """skip[0] = 1: p, m, v and the record (its counter included) stay as they were; skip[0] = 0: the update runs"""
    from nsd_amd import ops
    n = 31764
    p0, gs, norms = _flat_problem(n)
    opt, state = ops.opt_struct(lr=LR, max_norm=0.1 * norms[0]), ops.opt_state(n, 1, dev)
    p, m, v, _ = _flat_run(ops, dev, p0, gs[:2], opt, state)
    before = (p.clone(), m.clone(), v.clone(), state[:16].clone())
    flag = torch.ones(1, device=dev)
    gt = to_dev(gs[2], dev)
    ops.grad_norm(gt, state)
    ops.adam_step_clip(p, gt, m, v, opt, state, step=3, skip=flag)
    torch.cuda.synchronize()
    assert _same(p, before[0]) and _same(m, before[1]) and _same(v, before[2]) and torch.equal(state[:16], before[3])
    flag.zero_()
    ops.adam_step_clip(p, gt, m, v, opt, state, step=3, skip=flag)
    assert not _same(p, before[0]) and _records(ops, state)[0]["skipped"] == 0


def test_flat_route_skips_non_finite_gradients(nsd, dev):
    """inf, then nan, in one gradient element: p, m, v bitwise untouched, skipped 1 then 2, the norm records the value; the next clean
    step updates as nsd_adam_step does and leaves the counter alone.  max_norm = 0: the guard works without clipping"""
    from nsd_amd import ops
    n = 33
    p0, gs, _ = _flat_problem(n)
    opt, state = ops.opt_struct(lr=LR, max_norm=0.0), ops.opt_state(n, 1, dev)
    p, m, v, _ = _flat_run(ops, dev, p0, gs[:2], opt, state)
    before = (p.clone(), m.clone(), v.clone())
    for k, bad in enumerate((float("inf"), float("nan")), 1):
        g = gs[2].copy()
        g[5] = bad
        gt = to_dev(g, dev)
        ops.grad_norm(gt, state)
        ops.adam_step_clip(p, gt, m, v, opt, state, step=3)
        rec = _records(ops, state)[0]
        print(f"[flat non-finite] {bad}: record {rec}")
        assert _same(p, before[0]) and _same(m, before[1]) and _same(v, before[2])
        assert rec["skipped"] == k and (math.isinf(rec["norm"]) if k == 1 else math.isnan(rec["norm"])) and rec["coef"] == 0.0
    pa, ma, va = (t.clone() for t in before)
    gt = to_dev(gs[2], dev)
    ops.adam_step(pa, gt, ma, va, step=3, lr=LR)
    ops.grad_norm(gt, state)
    ops.adam_step_clip(p, gt, m, v, opt, state, step=3)
    rec = _records(ops, state)[0]
    assert _same(p, pa) and _same(m, ma) and _same(v, va) and not _same(p, before[0])
    assert rec["skipped"] == 2 and rec["coef"] == 1.0 and _ulps(rec["norm"], ref.grad_norm(gs[2])[1]) <= 1


# ---- 2. fused tail -------------------------------------------------------------------------------------------------------------------
# H = 48: (1, 1) fewer slabs than slab groups, (5, 7) odd batch, (513, 3) the four-trial band's slab count; H = 40: the generic path (one
# slab); (K, F) = (2, 1), (8, 64): P no multiple of 32 (P % 32 = 6 and 25), so the last workgroup has idle lanes.  The LSTM block is
# 4H (C + 3H + 4) floats for L = 2, a multiple of 32 at H = 48 and H = 40 whatever C is, so at those shapes the LSTM / head boundary
# never falls inside a workgroup; the last case (C = 7, H = 20: 5680 = 177 * 32 + 16 floats) puts it there.
FUSED = [(8, 48, 2, 3, 32, 1, 1), (8, 48, 2, 3, 32, 5, 7), (8, 48, 2, 3, 32, 513, 3), (8, 40, 2, 3, 32, 5, 7), (8, 48, 2, 2, 1, 5, 7),
         (8, 48, 2, 8, 64, 5, 7), (7, 20, 2, 3, 32, 5, 7)]


def _evaluation(ops, dev, Cc, H, L, K, F, B, T):
    """a real forward + backward: the workspace holds the slabs, grads is nsd_grad_reduce's"""
    _, flat, x, y, _ = head_inputs(Cc, H, K, F, B, T, L=L)
    spec = ops.ModelSpec(C=Cc, H=H, L=L, K=K, F=F)
    flat_t, ws = to_dev(flat, dev), ops.new_workspace(spec, B, T, dev)
    logits, grads = torch.empty((B, K), device=dev), torch.full((spec.param_count,), float("nan"), device=dev)
    ops.train_step_grads(spec, flat_t, to_dev(x, dev), ws, to_dev(y, dev), logits, grads)
    return spec, flat_t, ws, grads


@pytest.mark.parametrize("shape", FUSED, ids=lambda s: "C%d-H%d-L%d-K%d-F%d-B%d-T%d" % s)
def test_fused_tail(nsd, dev, shape):
    from nsd_amd import ops
    Cc, H, L, K, F, B, T = shape
    spec, flat, ws, g_ref = _evaluation(ops, dev, *shape)
    P = spec.param_count
    print(f"[fused tail] {shape}: P % 32 = {P % 32}, LSTM / head boundary % 32 = {spec.offsets()['ln.weight'] % 32}")
    g64 = g_ref.cpu().numpy()
    norm = ref.grad_norm(g64)[1]
    assert np.isfinite(g64).all() and norm > 0
    m0, v0 = _moments(P, seed=B + T)
    p0 = flat.cpu().numpy()
    state = ops.opt_state(P, 1, dev)

    def run(tail, **kw):
        p, m, v, g = to_dev(p0, dev), to_dev(m0, dev), to_dev(v0, dev), torch.full((P,), float("nan"), device=dev)
        tail(ops, spec, B, T, ws, g, p, m, v, **kw)
        return p, m, v, g
    # clipped, weight decay on, step 3 of a run in progress
    kw = dict(weight_decay=1e-2, max_norm=0.1 * norm)
    p, m, v, g = run(_tail_clip, opt=ops.opt_struct(lr=LR, **kw), state=state, step=3)
    rec = _records(ops, state)[0]
    R, want = _ref_step(p0, m0, v0, g64, 3, **kw)
    u = (_ulps(rec["norm"], norm), _ulps(rec["coef"], want["coef"]))
    errs = (_err(p, R.p), _err(m, R.m), _err(v, R.v))
    print(f"[fused tail] {shape}: P={P} norm {norm:.4e} record ulps {u} coef {rec['coef']:.4f} |dp| {errs[0]:.2e} |dm| {errs[1]:.2e} |dv| {errs[2]:.2e}")
    assert _same(g, g_ref)                                     # grads: nsd_grad_reduce's bits
    assert max(u) <= 1 and rec["coef"] < 1.0 and rec["lr"] == float(np.float32(LR)) and rec["skipped"] == 0
    assert max(errs) <= TOL
    # unclipped, constant schedule: nsd_grad_reduce_adam's bits
    pa, ma, va, ga = run(_tail_plain, step=3, wd=1e-2)
    for max_norm in (10.0 * norm, 0.0):
        p, m, v, g = run(_tail_clip, opt=ops.opt_struct(lr=LR, weight_decay=1e-2, max_norm=max_norm), state=state, step=3)
        assert _same(g, ga) and _same(p, pa) and _same(m, ma) and _same(v, va), (shape, max_norm)
        assert _records(ops, state)[0]["coef"] == 1.0


# ---- 3. model-batched tail -----------------------------------------------------------------------------------------------------------
MB, BB, TB = 3, 5, 7


@pytest.fixture(scope="module")
def batched(nsd, dev):
    """M = 3 models on shared windows scaled by 1, 30 and 1e-3: one forward + backward, the workspace keeps the slabs"""
    from nsd_amd import _lib, ops
    spec = ops.ModelSpec()
    P = spec.param_count
    from oracle import nsd_oracle as orc
    d = orc.Dims()
    params = torch.stack([to_dev(orc.flatten_state(synth_params(8, 48, 2, 3, seed=70 + i), d), dev) for i in range(MB)]).contiguous()
    x0 = synth_x(BB, TB, seed=5)
    x = torch.stack([to_dev(x0 * np.float32(s), dev) for s in (1.0, 30.0, 1e-3)]).contiguous()
    y = to_dev(np.tile(synth_labels(BB, seed=5), MB), dev)
    ws = ops.multi_workspace(spec, MB, BB, TB, dev)
    grads = torch.empty((MB, P), device=dev)
    ops.multi_train_step(spec, params, x, y, ws, grads, fuse_adam=False)
    lay = _lib.WsLayout()
    dd = spec.dims(BB, TB)
    assert _lib.lib().nsd_multi_workspace_bytes(C.byref(dd), MB, C.byref(lay)) > 0
    torch.cuda.synchronize()
    return dict(spec=spec, P=P, params=params, ws=ws, grads=grads, lay=lay)


def _single_ws_of_model(ops, dev, batched, mdl):
    """a single-model workspace that holds model mdl's slabs: at B = 5 either launch writes one LSTM slab per trial"""
    from nsd_amd import _lib
    spec, lay, ws = batched["spec"], batched["lay"], batched["ws"]
    nb, one = ops.workspace_layout(spec, BB, TB)
    assert one.n_slabs == BB
    offs = spec.offsets()
    p_lstm = offs["ln.weight"]
    stride, ph = (p_lstm + 3) // 4 * 4, batched["P"] - p_lstm
    w1 = torch.full((nb // 4,), float("nan"), device=dev)
    w1[one.slabs:one.slabs + BB * stride] = ws[lay.slabs + mdl * BB * stride:lay.slabs + (mdl + 1) * BB * stride]
    w1[one.hslabs:one.hslabs + BB * ph] = ws[lay.hslabs + mdl * BB * ph:lay.hslabs + (mdl + 1) * BB * ph]
    return w1


def test_model_batched_tail_is_the_single_model_tail_per_model(nsd, dev, batched):
    """One max_norm between the models' norms: some clip, some do not; records per model; every model bitwise its single-model call"""
    from nsd_amd import ops
    spec, P, params, ws, g_ref = (batched[k] for k in ("spec", "P", "params", "ws", "grads"))
    norms = [ref.grad_norm(g_ref[i].cpu().numpy())[1] for i in range(MB)]
    max_norm = math.sqrt(sorted(norms)[1] * sorted(norms)[2])        # between the two largest norms: one model clips, two do not
    opt = ops.opt_struct(lr=LR, weight_decay=1e-2, max_norm=max_norm)
    m0, v0 = _moments(MB * P, seed=3)
    p, m, v = params.clone(), to_dev(m0, dev).view(MB, P).clone(), to_dev(v0, dev).view(MB, P).clone()
    g, state = torch.full((MB, P), float("nan"), device=dev), ops.opt_state(P, MB, dev)
    _multi_tail_clip(ops, spec, MB, BB, TB, ws, g, p, m, v, opt, state, step=3)
    recs = _records(ops, state, MB)
    print(f"[multi tail] norms {norms} max_norm {max_norm:.4e} coefs {[r['coef'] for r in recs]}")
    assert _same(g, g_ref)
    clipped = [r["coef"] < 1.0 for r in recs]
    assert any(clipped) and not all(clipped)                   # the mix
    for i in range(MB):
        assert _ulps(recs[i]["norm"], norms[i]) <= 1 and clipped[i] == (norms[i] > max_norm)
        w1, s1 = _single_ws_of_model(ops, dev, batched, i), ops.opt_state(P, 1, dev)
        p1, m1, v1 = params[i].clone(), to_dev(m0, dev).view(MB, P)[i].clone(), to_dev(v0, dev).view(MB, P)[i].clone()
        g1 = torch.full((P,), float("nan"), device=dev)
        _tail_clip(ops, spec, BB, TB, w1, g1, p1, m1, v1, opt, s1, step=3)
        r1 = _records(ops, s1)[0]
        assert _same(g1, g[i]) and _same(p1, p[i]) and _same(m1, m[i]) and _same(v1, v[i]), i
        assert r1 == recs[i], (i, r1, recs[i])
        R, want = _ref_step(params[i].cpu().numpy(), m0.reshape(MB, P)[i], v0.reshape(MB, P)[i], g_ref[i].cpu().numpy(), 3,
                            weight_decay=1e-2, max_norm=max_norm)
        assert _err(p[i], R.p) <= TOL and _ulps(recs[i]["coef"], want["coef"]) <= 1


def test_model_batched_tail_skips_the_non_finite_model_alone(nsd, dev, batched):
    """inf, then nan, in one slab element of model 1: its p, m, v bitwise untouched, its counter 1 then 2, models 0 and 2 updated as
    without the fault; the next clean step updates all three and leaves the counters alone"""
    from nsd_amd import ops
    spec, P, params, lay = (batched[k] for k in ("spec", "P", "params", "lay"))
    ws = batched["ws"].clone()
    opt, state = ops.opt_struct(lr=LR, max_norm=0.0), ops.opt_state(P, MB, dev)
    stride = (spec.offsets()["ln.weight"] + 3) // 4 * 4
    at = lay.slabs + 1 * BB * stride + 2 * stride + 77          # model 1, slab 2, LSTM column 77

    def run(w):
        p, m, v, g = params.clone(), torch.zeros_like(params), torch.zeros_like(params), torch.empty_like(params)
        _multi_tail_clip(ops, spec, MB, BB, TB, w, g, p, m, v, opt, state, step=1)
        return p, m, v
    clean = run(batched["ws"])
    assert [r["skipped"] for r in _records(ops, state, MB)] == [0, 0, 0]
    for k, bad in enumerate((float("inf"), float("nan")), 1):
        ws[at] = bad
        p, m, v = run(ws)
        recs = _records(ops, state, MB)
        print(f"[multi non-finite] {bad}: {recs}")
        assert [r["skipped"] for r in recs] == [0, k, 0]
        assert _same(p[1], params[1]) and float(m[1].abs().max()) == 0.0 and float(v[1].abs().max()) == 0.0
        assert math.isinf(recs[1]["norm"]) if k == 1 else math.isnan(recs[1]["norm"])
        for i in (0, 2):
            assert _same(p[i], clean[0][i]) and _same(m[i], clean[1][i]) and _same(v[i], clean[2][i]), i
    p, m, v = run(batched["ws"])
    assert all(_same(a, b) for a, b in zip((p, m, v), clean))
    assert [r["skipped"] for r in _records(ops, state, MB)] == [0, 2, 0]


# ---- 4. the schedule on the device ---------------------------------------------------------------------------------------------------
W_S, NP_S = 3, 8


@pytest.mark.parametrize("kind", ["cosine", "step"])
def test_schedule_from_the_device_step_counter(nsd, dev, kind):
    """step_dev in {1, W, W + 1, N', N' + 5}: the recorded lr within 1 ulp of float(lr * nsd_lr_factor), p / m / v within 1e-6 of the
    host-step call (device pow / cos against libm's)"""
    from nsd_amd import ops
    n = 31764
    p0, gs, norms = _flat_problem(n)
    sched = nsd.LrSchedule(kind, warmup_steps=W_S, total_steps=W_S + NP_S, min_ratio=0.1, step_size=2, gamma=0.5)
    opt = ops.opt_struct(lr=LR, max_norm=0.5 * norms[0], schedule=sched)
    m0, v0 = _moments(n, seed=1)
    gt, state, step_dev = to_dev(gs[0], dev), ops.opt_state(n, 1, dev), torch.zeros(1, dtype=torch.int64, device=dev)
    lrs = []
    for s in (1, W_S, W_S + 1, NP_S, NP_S + 5):
        out = []
        for on_device in (False, True):
            p, m, v = to_dev(p0, dev), to_dev(m0, dev), to_dev(v0, dev)
            step_dev.fill_(s)
            ops.grad_norm(gt, state)
            ops.adam_step_clip(p, gt, m, v, opt, state, step=0 if on_device else s, step_dev=step_dev if on_device else None)
            out.append((p, m, v, _records(ops, state)[0]["lr"]))
        want = _lr32(ops.lr_factor(opt, s))
        assert want == _lr32(ref.lr_factor(kind, s, W_S, W_S + NP_S, 0.1, 2, 0.5))
        d = [float((a - b).abs().max()) for a, b in zip(out[0][:3], out[1][:3])]
        print(f"[schedule on device] {kind} s={s}: lr host {out[0][3]:.9e} device {out[1][3]:.9e} want {want:.9e}; host vs device |dp| {d[0]:.2e}")
        assert out[0][3] == want and _ulps(out[1][3], want) <= 1
        assert max(d) <= TOL
        lrs.append(want)
    assert len(set(lrs)) >= 3                                  # the schedule moves over these steps


# ---- 5. trainers ---------------------------------------------------------------------------------------------------------------------
BT, TT = 16, 30


def _ref_model(nsd, dev, ref_state, **kw):
    m = nsd.EEG_LSTM(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in ref_state.items()}, strict=True)
    return m.to(dev).train()


def _xy(dev, seed=8):
    return to_dev(synth_x(BT, TT, seed=seed), dev), to_dev(synth_labels(BT, seed=seed), dev)


COSINE = dict(kind="cosine", warmup_steps=2, total_steps=10, min_ratio=0.1)


def test_trainer_graph_replay_equals_eager_with_clipping_and_schedule(nsd, dev, ref_state):
    from nsd_amd.trainer import Trainer
    x, y = _xy(dev)
    kw = dict(lr=LR, seed=5, clip_grad_norm=0.05, lr_schedule=nsd.LrSchedule(**COSINE))
    ta, tb = Trainer(_ref_model(nsd, dev, ref_state), **kw), Trainer(_ref_model(nsd, dev, ref_state), **kw)
    xs, ys = tb.static_inputs(BT, TT)
    xs.copy_(x); ys.copy_(y)
    for s in range(1, 4):
        ta.step(x, y)
        tb.step_static(BT, TT)
        print(f"[trainer graph] step {s}: lr {ta.last_lr():.9e} / {tb.last_lr():.9e} norm {ta.last_grad_norm():.6e} / {tb.last_grad_norm():.6e}")
        assert ta.last_lr() == tb.last_lr() == _lr32(ref.lr_factor(s=s, **COSINE))
        assert ta.last_grad_norm() > 0.05                      # the threshold bites
    assert tb.step_count == 3 and int(tb._step_dev.item()) == 3
    assert torch.equal(ta.grads, tb.grads)
    assert (ta.flat - tb.flat).abs().max().item() < TOL
    assert ta.skipped_steps() == tb.skipped_steps() == 0


def test_trainer_unclipped_constant_schedule_is_todays_trainer_bitwise(nsd, dev, ref_state):
    from nsd_amd.trainer import Trainer
    x, y = _xy(dev)
    ta = Trainer(_ref_model(nsd, dev, ref_state), lr=LR, seed=5, weight_decay=1e-2)
    tb = Trainer(_ref_model(nsd, dev, ref_state), lr=LR, seed=5, weight_decay=1e-2, clip_grad_norm=1e9, lr_schedule=nsd.LrSchedule())
    for _ in range(3):
        ta.step(x, y)
        tb.step(x, y)
    assert torch.equal(ta.flat, tb.flat) and torch.equal(ta.m, tb.m) and torch.equal(ta.v, tb.v) and torch.equal(ta.grads, tb.grads)
    assert tb.last_lr() == ta.last_lr() == float(np.float32(LR)) and math.isnan(ta.last_grad_norm()) and ta.skipped_steps() == 0


def test_trainer_trajectory_is_the_restatement_on_its_own_gradients(nsd, dev, ref_state):
    """small max_norm: last_grad_norm() is the norm of trainer.grads, and p follows optim_ref driven by the trainer's per-step grads"""
    from nsd_amd.trainer import Trainer
    x, y = _xy(dev)
    sched = dict(kind="step", warmup_steps=1, step_size=1, gamma=0.5)
    tr = Trainer(_ref_model(nsd, dev, ref_state), lr=LR, seed=5, weight_decay=1e-2, clip_grad_norm=0.02, lr_schedule=nsd.LrSchedule(**sched))
    R = ref.ClippedAdam(tr.flat.cpu().numpy(), lr=LR, weight_decay=1e-2, max_norm=0.02, schedule=sched)
    for s in range(1, 4):
        tr.step(x, y)
        want = R.step(tr.grads.cpu().numpy())
        print(f"[trainer trajectory] step {s}: norm {tr.last_grad_norm():.6e} want {want['norm']:.6e} lr {tr.last_lr():.4e} |dp| {_err(tr.flat, R.p):.2e}")
        assert _ulps(tr.last_grad_norm(), want["norm"]) <= 1 and want["coef"] < 1.0 and tr.last_lr() == want["lr"]
    assert _err(tr.flat, R.p) <= TOL and _err(tr.m, R.m) <= TOL and _err(tr.v, R.v) <= TOL


def test_trainer_resumes_the_schedule_from_its_state_dict(nsd, dev, ref_state):
    from nsd_amd.trainer import Trainer
    x, y = _xy(dev)
    kw = dict(lr=LR, seed=5, clip_grad_norm=0.05, lr_schedule=nsd.LrSchedule(**COSINE))
    ta, tb = Trainer(_ref_model(nsd, dev, ref_state), **kw), Trainer(_ref_model(nsd, dev, ref_state), **kw)
    assert ta.last_lr() == _lr32(0.5)                          # before any step: the host's f(1)
    for _ in range(3):
        ta.step(x, y)
    for _ in range(2):
        tb.step(x, y)
    sd = tb.state_dict()
    assert sd["skipped"] == 0 and sd["step"] == 2
    tc = Trainer(_ref_model(nsd, dev, ref_state), **kw)
    sd["skipped"] = 4                                          # the sticky counter travels with the checkpoint
    tc.load_state_dict(sd)
    assert tc.last_lr() == _lr32(ref.lr_factor(s=2, **COSINE))        # no record yet: lr * f(step) from the host
    tc.step(x, y)
    assert tc.last_lr() == ta.last_lr() and tc.skipped_steps() == 4
    assert torch.equal(tc.flat, ta.flat) and torch.equal(tc.m, ta.m) and torch.equal(tc.v, ta.v)


def _launches(fn, steps=3):
    from nsd_amd import ops
    names = []

    @contextlib.contextmanager
    def hook(name):
        names.append(name)
        yield
    ops.set_launch_hook(hook)
    try:
        for _ in range(steps):
            fn()
    finally:
        ops.set_launch_hook(None)
    return names


def test_options_off_issue_todays_launches(nsd, dev, ref_state):
    from nsd_amd.trainer import Trainer
    x, y = _xy(dev)
    today = ["nsd_lstm_head_train_rng", "nsd_lstm_bwd_rng", "nsd_grad_reduce_adam"]
    for kw in ({}, dict(clip_grad_norm=None, lr_schedule=None)):
        tr = Trainer(_ref_model(nsd, dev, ref_state), lr=LR, seed=5, **kw)
        assert _launches(lambda: tr.step(x, y)) == today * 3
    tr = Trainer(_ref_model(nsd, dev, ref_state), lr=LR, seed=5, clip_grad_norm=0.0)
    assert _launches(lambda: tr.step(x, y)) == (today[:2] + ["nsd_grad_reduce_clip_adam"]) * 3
    models = lambda: [_ref_model(nsd, dev, ref_state) for _ in range(2)]
    mt = nsd.ModelBatchTrainer(models(), lr=LR, seeds=[1, 2])
    assert _launches(lambda: mt.step(x, y)) == ["nsd_multi_train_fwd", "nsd_multi_train_bwd", "nsd_multi_grad_reduce_adam"] * 3
    mc = nsd.ModelBatchTrainer(models(), lr=LR, seeds=[1, 2], clip_grad_norm=0.05, lr_schedule=nsd.LrSchedule(**COSINE))
    assert _launches(lambda: mc.step(x, y)) == ["nsd_multi_train_fwd", "nsd_multi_train_bwd", "nsd_multi_grad_reduce_clip_adam"] * 3
    norms = mc.last_grad_norms()
    want = [ref.grad_norm(mc.grads[i].cpu().numpy())[1] for i in range(2)]
    print(f"[model batch trainer] norms {norms} want {want} lr {mc.last_lr():.6e}")
    assert all(_ulps(a, b) <= 1 for a, b in zip(norms, want)) and mc.skipped_steps() == [0, 0]
    assert mc.last_lr() == _lr32(ref.lr_factor(s=3, **COSINE))


# ---- 6. bf16 path --------------------------------------------------------------------------------------------------------------------
def test_bf16_path_takes_the_flat_route_and_keeps_its_guard(nsd, dev):
    from nsd_amd.trainer import Trainer
    torch.manual_seed(11)
    model = nsd.EEG_LSTM(8, 64, 2, 5, dropout=0.6, precision="bf16").to(dev).train()
    tr = Trainer(model, lr=LR, seed=3, clip_grad_norm=0.05)
    x, y = to_dev(synth_x(32, 5, seed=4), dev), to_dev(synth_labels(32, 5, seed=4), dev)
    names = _launches(lambda: tr.step(x, y), steps=2)
    assert names[-2:] == ["nsd_grad_norm", "nsd_adam_step_clip"] and "nsd_adam_step_guarded" not in names
    want = ref.grad_norm(tr.grads.cpu().numpy())[1]
    print(f"[bf16] norm {tr.last_grad_norm():.6e} want {want:.6e}")
    assert tr.scan_status() == 0 and _ulps(tr.last_grad_norm(), want) <= 1 and tr.last_lr() == float(np.float32(LR))
    before = (tr.flat.clone(), tr.m.clone(), tr.v.clone(), tr._opt_state[:16].clone())
    tr._skip.fill_(1.0)                                        # what nsd_seq_guard raises after a time-out on any rank
    tr._adam()
    torch.cuda.synchronize()
    assert _same(tr.flat, before[0]) and _same(tr.m, before[1]) and _same(tr.v, before[2]) and torch.equal(tr._opt_state[:16], before[3])
    tr._skip.zero_()
    tr._adam()
    assert not _same(tr.flat, before[0])


# ---- 7. two ranks --------------------------------------------------------------------------------------------------------------------
DDP_KW = dict(lr=LR, stochastic=False, clip_grad_norm=0.05, lr_schedule=dict(kind="cosine", warmup_steps=1, total_steps=6, min_ratio=0.1))


def _ddp_model():
    import nsd_amd
    torch.manual_seed(11)
    return nsd_amd.EEG_LSTM(8, 48, 2, 3, dropout=0.6)


def _ddp_batches():
    return [(synth_x(B, 20, seed=40 + i), synth_labels(B, 3, seed=40 + i)) for i, B in enumerate((7, 1, 6, 2))]


def _ddp_trainer(dev):
    import nsd_amd
    from nsd_amd.trainer import Trainer
    kw = dict(DDP_KW)
    kw["lr_schedule"] = nsd_amd.LrSchedule(**kw["lr_schedule"])
    return Trainer(_ddp_model().to(dev).train(), **kw)


def _ddp_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from nsd_amd.trainer import shard_range
        dev = torch.device("cuda:0")
        tr = _ddp_trainer(dev)
        recs = []
        for x, y in _ddp_batches():
            lo, hi = shard_range(len(y), rank, world)
            tr.step(torch.from_numpy(x[lo:hi]).to(dev), torch.from_numpy(y[lo:hi]).to(dev), global_batch=len(y))
            recs.append(tr._opt_state[:16].cpu().numpy().copy())
        torch.cuda.synchronize()
        np.save(os.path.join(out_dir, f"rank{rank}.npy"), tr.flat.cpu().numpy())
        np.save(os.path.join(out_dir, f"rec{rank}.npy"), np.stack(recs))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_clip_alike(tmp_path):
    """world = 2 over gloo on one GPU, as tests/test_gpu_ddp.py: nsd_grad_reduce -> one all-reduce -> nsd_grad_norm + nsd_adam_step_clip.
    Both ranks see the same all-reduced bits, hence the same norm, coef and parameters, bit for bit; against one rank on the full
    batches (the fused tail) within that file's bound"""
    import torch.multiprocessing as mp
    assert torch.cuda.is_available()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_ddp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    p0, p1 = np.load(tmp_path / "rank0.npy"), np.load(tmp_path / "rank1.npy")
    r0, r1 = np.load(tmp_path / "rec0.npy"), np.load(tmp_path / "rec1.npy")
    assert np.array_equal(p0, p1) and np.array_equal(r0, r1)
    dev = torch.device("cuda:0")
    tr = _ddp_trainer(dev)
    norms = []
    for x, y in _ddp_batches():
        tr.step(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev))
        norms.append(tr.last_grad_norm())
    got = r0.view(np.float32)[:, 0]
    print(f"[two ranks] norms per step: ranks {got.tolist()} one rank {norms}")
    assert np.allclose(got, norms, rtol=1e-3) and (got > 0.05).all()             # every step clips
    dp = np.abs(p0 - tr.flat.cpu().numpy())
    assert dp.max() <= 2 * 1e-3 * 4 and (dp > 2e-5).mean() < 0.02, (dp.max(), (dp > 2e-5).mean())


# ---- 8. buffer contract of the four launching entry points -----------------------------------------------------------------------------
def _contract(ops, dev, n_state, M, launch, inputs, outputs):
    """launch(state) on fresh copies of `outputs` -> their bits.  opt_state of exactly nsd_opt_state_bytes between guards, pre-filled
    with zeros / 0xFF / NaN words and then initialised: identical results; inputs unchanged; the same bits on a side stream and from a
    replayed graph"""
    nb = ops.opt_state_bytes(n_state, M)
    results = []

    def once(fill, mode):
        state, check = bc.guarded((nb,), torch.uint8, dev, fill)
        ops._call("nsd_opt_state_init", dev, state.data_ptr(), nb, ops.STREAM)
        bc.fill_payload(state[16 * M:], fill)                  # (the initialisation may clear the scratch too: the pattern goes back in)
        outs = [t.clone() for t in outputs]
        snap = bc.snapshot(*inputs)
        torch.cuda.synchronize()
        if mode == "plain":
            launch(state, *outs)
        elif mode == "side":
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                launch(state, *outs)
            torch.cuda.current_stream().wait_stream(side)
        else:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                launch(state, *outs)
            g.replay()
        torch.cuda.synchronize()
        check("opt_state")
        assert snap.unchanged(), (fill, mode, snap.changed())
        return [bc._bits(t) for t in outs] + [state[:16 * M].clone()]
    base = once("zeros", "plain")
    for fill, mode in (("ones", "plain"), ("nan32", "plain"), ("zeros", "side"), ("ones", "graph")):
        got = once(fill, mode)
        assert all(torch.equal(a, b) for a, b in zip(base, got)), (fill, mode)
    return base


def test_buffer_contract_flat_route(nsd, dev):
    """nsd_grad_norm + nsd_adam_step_clip, n = 31764 (125 partials) and n = 2^20 + 1 (the 2048-partial cap)"""
    from nsd_amd import ops
    for n in (31764, 2**20 + 1):
        p0, gs, norms = _flat_problem(n)
        g, p, m, v = to_dev(gs[0], dev), to_dev(p0, dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        opt = ops.opt_struct(lr=LR, max_norm=0.1 * norms[0])

        def launch(state, p, m, v):
            ops.grad_norm(g, state)
            ops.adam_step_clip(p, g, m, v, opt, state, step=1)
        _contract(ops, dev, n, 1, launch, [g], [p, m, v])


def test_buffer_contract_fused_and_model_batched_tails(nsd, dev, batched):
    from nsd_amd import ops
    spec, P, params, ws = (batched[k] for k in ("spec", "P", "params", "ws"))
    opt = ops.opt_struct(lr=LR, max_norm=1.0)
    z = torch.zeros_like(params)

    def multi(state, g, p, m, v):
        _multi_tail_clip(ops, spec, MB, BB, TB, ws, g, p, m, v, opt, state, step=1)
    _contract(ops, dev, P, MB, multi, [ws], [torch.empty_like(params), params, z, z])
    w1 = _single_ws_of_model(ops, dev, batched, 1)

    def single(state, g, p, m, v):
        _tail_clip(ops, spec, BB, TB, w1, g, p, m, v, opt, state, step=1)
    _contract(ops, dev, P, 1, single, [w1], [torch.empty(P, device=dev), params[1], z[1], z[1]])
