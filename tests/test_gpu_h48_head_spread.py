"""The fused train head's weight-gradient outer products, written by the helper waves.  Needs the MI355X.

In the one- and two-trial H = 48 forward (nsd_lstm2_fwd48.hip) the pooling wave runs the dense head of a trial alone; the K F entries
of d fc.3.weight and the F H entries of d fc.0.weight -- products of vectors it leaves in LDS -- are formed and stored by the three
helper waves (192 lanes) behind the barrier that publishes them (train_tail).  What can go wrong there is an entry that no lane
takes or that two index maps disagree on, so the shapes are the ones at which the two loops end differently: fewer entries than
lanes (F H = 48, K F = 2), a last trip that is partly filled (F = 7, 33, 63), whole trips only (F = 64, K = 8: 3072 = 16 x 192), in
the one-trial band (B = 3) and the two-trial band with a padding trial in the last workgroup (B = compute units + 3).  The gradient
buffer and the workspace (the per-trial head slabs in it) are full of NaN before the step (gpu_harness.train_step), so an entry that
is not written fails the finiteness check, and one written to the wrong place the comparison with the oracle at the bounds every
other H = 48 test uses.  The model-batched twin keeps the pooling wave's own loop in its two-trial kernels: a model-batched launch in
that band against the same models one at a time.
"""
import numpy as np
import pytest
import torch

from oracle import nsd_oracle as orc
from tests.gpu_harness import (FAST48, HEAD_SAVES, assert_step_vs_oracle, cus, dev, head_inputs, multi_grad_ok, multi_problem,  # noqa: F401
                               multi_single, multi_step, nsd, oracle_step, spec_of, train_step)

pytestmark = pytest.mark.gpu

HEADS = [(2, 1), (3, 32), (5, 7), (3, 33), (8, 63), (8, 64)]           # (K, F)
T = 5


def _check(dev, K, F, B, safe):
    d, flat, x, y, masks = head_inputs(8, 48, K, F, B, T, safe=safe)
    ref = oracle_step(d, flat, x, labels=y, masks=masks)
    out = train_step(dev, spec_of(d), flat, x, labels=y, masks=masks, fused=True, saves=HEAD_SAVES)
    assert_step_vs_oracle(out, ref, d, FAST48, tag=f"K={K} F={F} B={B}")
    got, want = orc.unflatten(out["grads"], d), orc.unflatten(ref["grads"], d)
    for name in ("fc.0.weight", "fc.3.weight"):
        assert got[name].shape == want[name].shape and np.isfinite(got[name]).all(), name
    return out


@pytest.mark.parametrize("K,F", HEADS)
def test_one_trial_band(nsd, dev, K, F):
    _check(dev, K, F, 3, safe=False)


@pytest.mark.parametrize("K,F", HEADS)
def test_two_trial_band_with_a_padding_trial(nsd, dev, cus, K, F):
    B = cus + 3 + (cus & 1)                  # odd: the last workgroup's second trial is padding
    _check(dev, K, F, B, safe=True)


def test_unfused_head_gives_the_same_head_gradients_within_its_bound(nsd, dev):
    """the separate head kernel (fused=False) forms the same two outer products: the fused step's stay within the project's bound
    between the two launch sequences (GRAD_RTOL_12 of tests/test_gpu_head_dims.py), tensor by tensor"""
    from tests.gpu_harness import GRAD_RTOL_12
    K, F = 8, 63
    d, flat, x, y, masks = head_inputs(8, 48, K, F, 3, T)
    a = train_step(dev, spec_of(d), flat, x, labels=y, masks=masks, fused=True)
    b = train_step(dev, spec_of(d), flat, x, labels=y, masks=masks, fused=False)
    ga, gb = orc.unflatten(a["grads"], d), orc.unflatten(b["grads"], d)
    for name in ("fc.0.weight", "fc.3.weight"):
        err, scale = float(np.abs(ga[name] - gb[name]).max()), float(np.abs(gb[name]).max())
        print(f"{name}: fused - unfused {err:.2e} of {scale:.2e}")
        assert err <= GRAD_RTOL_12 * scale + 1e-7, (name, err, scale)


def test_model_batched_two_trial_band_vs_single_models(nsd, dev, cus):
    """M = 2 models with M B trials in the two-trial band: the twin's two-trial kernels (the pooling wave's own store loop) against
    each model alone in the one-trial band (the helper waves'), at the bound of the model-batched tests"""
    spec, M = spec_of(orc.Dims()), 2
    B = cus // 2 + 3
    params, x, y, rngs = multi_problem(spec, M, B, T, dev, seed=5)
    lg, gr, ls = multi_step(nsd, spec, params, x, y, rngs, dev)
    for m in range(M):
        l1, g1, s1 = multi_single(nsd, spec, params[m].clone(), x[m], y[m], rngs[m], dev)
        assert torch.isfinite(gr[m]).all() and torch.isfinite(g1).all(), m
        multi_grad_ok(spec, gr[m], g1)
