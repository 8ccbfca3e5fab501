"""The model-batched twins of the H = 48 kernels at the loop edges.  Needs the MI355X.

nsd_lstm2_multi_{fwd48,bwd48,fwd48x4,bwd48x4}.hip include the single-model role code but are translation units of their own, with
their own machine code: every role forms a ModelView and walks wg_id / wg_count instead of blockIdx.x / gridDim.x, the forward twin
is not LEAN, the backward twin keeps a private segment.  The single-model kernels are swept over every step count
(tests/test_gpu_h48_step_loops.py, tests/test_gpu_h48_bwd_edges.py); here the twins are, through ops.multi_train_step /
ops.multi_infer, against
  * the CPU oracle, each model's streams regenerated on the host from rngs[m] (as tests/test_gpu_multimodel.py does), and
  * the model's own single-model ops.train_step_grads / ops.infer run.
Bounds against the oracle are the project's (tests/gpu_harness.py): logits 1e-4, batch-mean loss 5e-5, FAST48 (LSTM weight
gradients 5e-5 of each tensor's largest element, the other tensors 2e-5 + 1e-7, attn.bias 2e-6 absolute), probabilities 1e-5.
The workspace and every output are NaN-filled before every call.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import nsd_oracle as orc
from tests.gpu_harness import (BWD_T, FAST48, INFER_T, KINK, LOGIT_TOL, PROB_TOL, assert_step_vs_oracle, dev, kink_margin, multi_grad_ok,  # noqa: F401
                               multi_problem, nsd, oracle_step, oracle_streams)

pytestmark = pytest.mark.gpu

EDGE_T = tuple(sorted(set(range(1, 49)) | set(BWD_T)))       # every step count up to 48, then the ring / x-chunk edges up to 65


def _spec(nsd, C=8, K=3):
    return nsd.ModelSpec(C=C, H=48, L=2, K=K, F=32)


def _multi(spec, params, x, y, rngs, dev, targets=None):
    """ops.multi_train_step (no Adam) into NaN-filled buffers -> logits [M,B,K], grads [M,P], loss sums [M] (fp32, device values)"""
    from nsd_amd import ops
    M = params.shape[0]
    B, T = (x.shape[-3], x.shape[-2])
    ws = ops.multi_workspace(spec, M, B, T, dev)
    ws.fill_(float("nan"))
    grads = torch.full_like(params, float("nan"))
    logits = torch.full((M * B, spec.K), float("nan"), device=dev)
    ops.multi_train_step(spec, params, x, None if y is None else y.contiguous().view(-1), ws, grads, rngs=rngs, logits=logits,
                         fuse_adam=False, targets=targets)
    return logits.view(M, B, spec.K).clone(), grads, ops.multi_loss_sum(spec, ws, M, B, T).clone()


def _single(spec, flat, x, y, rng, dev, targets=None):
    """the same model alone: ops.train_step_grads -> logits, grads, loss sum"""
    from nsd_amd import ops
    B, T, _ = x.shape
    ws = ops.new_workspace(spec, B, T, dev)
    ws.fill_(float("nan"))
    logits = torch.full((B, spec.K), float("nan"), device=dev)
    grads = torch.full_like(flat, float("nan"))
    ops.train_step_grads(spec, flat.contiguous(), x.contiguous(), ws, None if y is None else y.contiguous(), logits, grads, rng=rng,
                         targets=targets)
    return logits, grads, ops.loss_sum(spec, ws, B, T).clone()


def _streams(rng, B, T):
    """no rng: no dropout, the eval slope -- the oracle's defaults"""
    return {} if rng is None else oracle_streams(rng["seed"], rng["base_stream"], B, T, 48, 32)


# The inputs are drawn again (seed + 100000, ...) until every fc.0 pre-activation of the oracle is KINK (tests/gpu_harness.py) away
# from 0; with 3 x 171 trials at T = 16 the first draw has one at +6.5e-9 (model 1, trial 168, unit 14; +7.7e-9 in the float64 model,
# from which the oracle's pre-activations are at most 1.8e-7 away): the four-trial twin took the oracle's side, the single-model
# kernel the other.
def _kink_margin(spec, flat, x, rng):
    d = orc.Dims(C=spec.C, K=spec.K)
    return kink_margin(orc.forward(flat.cpu().numpy(), x.cpu().numpy(), d, saves=True, **_streams(rng, x.shape[0], x.shape[1])))


def _problem_off_kink(spec, M, B, T, dev, seed, with_streams=(True,)):
    """multi_problem, drawn again until no fc.0 pre-activation lies within KINK of the RReLU kink"""
    for k in range(50):
        params, x, y, rngs = multi_problem(spec, M, B, T, dev, seed=seed + 100000 * k)
        if all(_kink_margin(spec, params[m], x[m], rngs[m] if on else None) > KINK for m in range(M) for on in with_streams):
            return params, x, y, rngs
    raise AssertionError("no draw away from the RReLU kink")


def _vs_oracle(spec, flat, x, y, rng, lg, gr, loss_sum, targets=None, what=None):
    """one model of a launch against the oracle: logits, batch-mean loss, every gradient tensor (FAST48); the oracle asserts KINK on
    its own pre-activations (a condition on the inputs: _problem_off_kink)"""
    d = orc.Dims(C=spec.C, K=spec.K)
    B, T, _ = x.shape
    tgt = dict(labels=y.cpu().numpy()) if targets is None else dict(targets=targets.cpu().numpy())
    ref = oracle_step(d, flat.cpu().numpy(), x.cpu().numpy(), masks=_streams(rng, B, T), kink=KINK, **tgt)
    out = dict(logits=lg.cpu().numpy(), grads=gr.cpu().numpy(), mean_loss=float(loss_sum) / B)
    print(f"twin {what}: logits {float(np.abs(out['logits'] - ref['logits']).max()):.2e} loss {abs(out['mean_loss'] - ref['loss']):.2e}")
    assert_step_vs_oracle(out, ref, d, FAST48)


def _bit_equal_to_singles(spec, params, x, y, rngs, dev, got, targets=None):
    lg, gr, ls = got
    M, B = lg.shape[0], lg.shape[1]
    for m in range(M):
        xm = x if x.dim() == 3 else x[m]
        l1, g1, s1 = _single(spec, params[m], xm, None if y is None else y[m], None if rngs is None else rngs[m], dev,
                             targets=None if targets is None else targets[m * B:(m + 1) * B].contiguous())
        assert torch.isfinite(l1).all() and torch.isfinite(g1).all(), m
        assert torch.equal(lg[m], l1), (m, float((lg[m] - l1).abs().max()))
        assert torch.equal(gr[m], g1), (m, float((gr[m] - g1).abs().max()))
        assert torch.equal(ls[m:m + 1], s1), (m, float(ls[m]), float(s1))


def _close_to_singles(spec, params, x, y, rngs, dev, got, models=None):
    """test_models_equal_separate_runs' bounds (another kernel or slab partition than the single-model run): logits and loss 1e-6,
    gradients FAST48's figures"""
    lg, gr, ls = got
    B = lg.shape[1]
    for m in (range(lg.shape[0]) if models is None else models):
        l1, g1, s1 = _single(spec, params[m], x[m], y[m], rngs[m], dev)
        assert float((lg[m] - l1).abs().max()) <= 1e-6 * max(float(l1.abs().max()), 1.0), m
        multi_grad_ok(spec, gr[m], g1)
        a, b = float(ls[m]) / B, float(s1) / B
        assert abs(a - b) <= 1e-6 * max(1.0, abs(b)), (m, a, b)


# ---------------------------------------------------------------------------------------------------
# 1. one-trial twins at every step count
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", EDGE_T)
def test_one_trial_twins_at_every_step_count(nsd, dev, T):
    """M = 2, B = 3, distinct streams per model.  The rule behind the bit-equality: plan48 reads only the trials of the launch -- with
    M * B = 6 <= #CUs both the model-batched and the single-model launch take the one-trial forward and backward instantiations, and a
    model gets min(B, #CUs / M) = 3 workgroups = 3 slabs, as the single-model launch of its 3 trials does; so every sum runs in the
    same order.  Each model equals its single-model run bit for bit (logits, flat gradient, loss sum), model M - 1 is held to the
    oracle, and a second identical call gives the same bits."""
    spec, M, B = _spec(nsd), 2, 3
    params, x, y, rngs = _problem_off_kink(spec, M, B, T, dev, 3000 + T)
    got = _multi(spec, params, x, y, rngs, dev)
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()
    _bit_equal_to_singles(spec, params, x, y, rngs, dev, got)
    _vs_oracle(spec, params[M - 1], x[M - 1], y[M - 1], rngs[M - 1], got[0][M - 1], got[1][M - 1], got[2][M - 1], what=("T", T))
    again = _multi(spec, params, x, y, rngs, dev)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), T


# ---------------------------------------------------------------------------------------------------
# 2. stream and target variants
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [5, 13, 21, 29, 37])
def test_twins_without_streams_and_with_soft_targets(nsd, dev, T):
    """rngs=None: the `rng.on = false` instantiations of the dW duties and of layer 0's prep; targets=: the SOFT forward twin."""
    spec, M, B = _spec(nsd), 2, 3
    params, x, y, rngs = _problem_off_kink(spec, M, B, T, dev, 4000 + T, with_streams=(True, False))
    got = _multi(spec, params, x, y, None, dev)
    _bit_equal_to_singles(spec, params, x, y, None, dev, got)
    for m in range(M):
        _vs_oracle(spec, params[m], x[m], y[m], None, got[0][m], got[1][m], got[2][m], what=("no streams", T, m))
    q = (1.5 * torch.rand((M * B, spec.K), generator=torch.Generator().manual_seed(T))).to(dev)
    q[1] = 0.0                                                # a row without weight
    got = _multi(spec, params, x, None, rngs, dev, targets=q)
    _bit_equal_to_singles(spec, params, x, None, rngs, dev, got, targets=q)
    for m in range(M):
        _vs_oracle(spec, params[m], x[m], None, rngs[m], got[0][m], got[1][m], got[2][m], targets=q[m * B:(m + 1) * B], what=("soft", T, m))


# ---------------------------------------------------------------------------------------------------
# 3. fewer channels
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,K", [(1, 2), (3, 3), (5, 4)])
def test_twins_with_fewer_channels(nsd, dev, C, K):
    """Lanes of the x-rows duty past the last channel, and ModelView strides (the parameter count) of 3, 4 and 5 floats mod 8: a
    model's rows start at every alignment."""
    spec, M, B, T = _spec(nsd, C, K), 3, 3, 21
    params, x, y, rngs = _problem_off_kink(spec, M, B, T, dev, 5000 + C)
    got = _multi(spec, params, x, y, rngs, dev)
    _bit_equal_to_singles(spec, params, x, y, rngs, dev, got)
    for m in range(M):
        _vs_oracle(spec, params[m], x[m], y[m], rngs[m], got[0][m], got[1][m], got[2][m], what=(C, K, m))


# ---------------------------------------------------------------------------------------------------
# 4. two trials per CU
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [7, 21, 33, 48])
@pytest.mark.parametrize("M,extra", [(2, 2), (3, 15), (2, 3), (3, 16)])
def test_twins_with_two_trials_per_cu(nsd, dev, M, extra, T):
    """M * B in (#CUs, 2 #CUs]: B = #CUs / M + extra.  The forward is the two-trial twin, the backward the one-trial twin on
    cap = #CUs / M workgroups per model; B > cap, so workgroups of every model start a second trial with the first trial's
    accumulators and windows.  (2, 2) and (3, 15) are the shapes as specified -- even B at 256 CUs; (2, 3) and (3, 16) make B odd
    there: the last pair of the forward has one trial.  Every model against the oracle, and against its single-model run (another
    slab partition: FAST48's figures, logits 1e-6)."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    spec, B = _spec(nsd), cus // M + extra
    assert cus < M * B <= 2 * cus and B > cus // M
    params, x, y, rngs = _problem_off_kink(spec, M, B, T, dev, 6000 + 10 * M + T)
    got = _multi(spec, params, x, y, rngs, dev)
    for m in range(M):
        _vs_oracle(spec, params[m], x[m], y[m], rngs[m], got[0][m], got[1][m], got[2][m], what=(M, B, T, m))
    _close_to_singles(spec, params, x, y, rngs, dev, got)


# ---------------------------------------------------------------------------------------------------
# 5. four-trial twins
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", range(1, 41))
def test_four_trial_twins_at_every_step_count(nsd, dev, T):
    """The four-trial twins pinned through the diagnostic library (it contains them): M = 2, B = 6 and B = 5 (a partial trial group
    in every model; more workgroups than trial groups).  Every model against the oracle and against its single-model run under
    the same pin."""
    from nsd_amd import _lib, ops
    spec, M = _spec(nsd), 2
    with _lib.diagnostic_library():
        try:
            ops.force_fwd48(4)
            ops.force_bwd48(4)
            for B in (6, 5):
                params, x, y, rngs = _problem_off_kink(spec, M, B, T, dev, 7000 + 50 * B + T)
                got = _multi(spec, params, x, y, rngs, dev)
                for m in range(M):
                    _vs_oracle(spec, params[m], x[m], y[m], rngs[m], got[0][m], got[1][m], got[2][m], what=("x4", B, T, m))
                _close_to_singles(spec, params, x, y, rngs, dev, got)
        finally:
            ops.force_fwd48(0)
            ops.force_bwd48(0)


@pytest.mark.parametrize("M,B,T", [(3, 171, 1), (3, 171, 4), (3, 171, 15), (3, 171, 16), (3, 171, 17), (3, 171, 33), (25, 32, 17)])
def test_four_trial_twins_through_the_products_dispatch(nsd, dev, M, B, T):
    """513 and 800 trials: the product's own plan picks the four-trial twins.  3 x 171: partial groups in every model; 25 x 32: more
    workgroups than trial groups per model -- idle workgroups must leave zero slabs.  The single-model runs (171 / 32 trials) take
    the one-trial kernels: test_models_equal_separate_runs' bounds."""
    spec = _spec(nsd)
    params, x, y, rngs = _problem_off_kink(spec, M, B, T, dev, 8000 + M + T)
    got = _multi(spec, params, x, y, rngs, dev)
    for m in range(M):
        _vs_oracle(spec, params[m], x[m], y[m], rngs[m], got[0][m], got[1][m], got[2][m], what=(M, B, T, m))
    _close_to_singles(spec, params, x, y, rngs, dev, got)


# ---------------------------------------------------------------------------------------------------
# 6. nsd_multi_infer
# ---------------------------------------------------------------------------------------------------
def _multi_infer(spec, params, x, dev):
    from nsd_amd import _lib, ops
    M = params.shape[0]
    B, T = x.shape[-3], x.shape[-2]
    nscr = int(_lib.lib().nsd_multi_infer_scratch_bytes(ctypes.byref(spec.dims(B, T)), M))
    scratch = torch.full((max(nscr // 4, 1),), float("nan"), device=dev)
    logits, probs = torch.full((M, B, spec.K), float("nan"), device=dev), torch.full((M, B, spec.K), float("nan"), device=dev)
    ops.multi_infer(spec, params, x, logits=logits, probs=probs, scratch=scratch)
    return logits, probs


def _infer(spec, flat, x, dev):
    from nsd_amd import _lib, ops
    B, T = x.shape[0], x.shape[1]
    nscr = int(_lib.lib().nsd_infer_scratch_bytes(ctypes.byref(spec.dims(B, T))))
    scratch = torch.full((max(nscr // 4, 1),), float("nan"), device=dev)
    logits, probs = torch.full((B, spec.K), float("nan"), device=dev), torch.full((B, spec.K), float("nan"), device=dev)
    ops.infer(spec, flat.contiguous(), x.contiguous(), logits=logits, probs=probs, scratch=scratch)
    return logits, probs


@pytest.mark.parametrize("T", INFER_T)
def test_multi_infer_is_bit_equal_to_infer_at_every_step_count(nsd, dev, T):
    """M = 2, B = 3, own and shared windows, at the step counts of tests/test_gpu_h48_infer_edges.py; beyond the model-batched
    path's 1024 steps the call is refused."""
    from nsd_amd import ops
    spec, M, B = _spec(nsd), 2, 3
    params, x, _, _ = multi_problem(spec, M, B, T, dev, seed=9000 + T)
    if not ops.multi_path(spec, M, B, T):
        assert T > 1024
        with pytest.raises(nsd.NsdError):
            ops.multi_infer(spec, params, x)
        return
    for xs in (x, x[1].contiguous()):
        lg, pr = _multi_infer(spec, params, xs, dev)
        for m in range(M):
            l1, p1 = _infer(spec, params[m], xs if xs.dim() == 3 else xs[m], dev)
            assert torch.isfinite(l1).all() and torch.isfinite(p1).all()
            assert torch.equal(lg[m], l1) and torch.equal(pr[m], p1), (T, m, xs.dim())


@pytest.mark.parametrize("T", [7, 33, 41])
def test_multi_infer_when_a_workgroup_pools_a_second_trial(nsd, dev, T):
    """M = 2, B = #CUs / 2 + 3: three workgroups of each model reset the pooling state (pool_reset) and walk a second trial."""
    spec, M = _spec(nsd), 2
    B = torch.cuda.get_device_properties(dev).multi_processor_count // 2 + 3
    params, x, _, _ = multi_problem(spec, M, B, T, dev, seed=9500 + T)
    lg, pr = _multi_infer(spec, params, x, dev)
    d = orc.Dims()
    for m in range(M):
        l1, p1 = _infer(spec, params[m], x[m], dev)
        assert torch.equal(lg[m], l1) and torch.equal(pr[m], p1), (T, m)
        ref = orc.forward(params[m].cpu().numpy(), x[m].cpu().numpy(), d)
        e_l, e_p = float(np.abs(lg[m].cpu().numpy() - ref["logits"]).max()), float(np.abs(pr[m].cpu().numpy() - ref["probs"]).max())
        print(f"multi_infer B={B} T={T} model {m}: logits {e_l:.2e} probs {e_p:.2e}")
        assert e_l < LOGIT_TOL and e_p < PROB_TOL, (T, m, e_l, e_p)
