"""The time loops of the one-trial H = 48 kernels at the sizes where a peeled loop block can go wrong.  Needs the MI355X.

The recurrence roles of nsd_lstm2_fwd48.hip / nsd_lstm2_bwd48.hip run the ring blocks that lie wholly inside their active window
without a test of the step index and the blocks that hold an end of the window with it (ring_block, nsd_ring_block.h); the saver wave of the
forward does the same per 8-step chunk.  The edges are the forward's ring (16 steps), x chunk (32), save chunk (8) and pipeline lag
(layer 1 runs 2 macro steps behind layer 0), and the backward's ring (8), four-step hand-off groups and five-step lag of layer 0.
Everything goes through the C ABI (ops.train_step_grads / ops.multi_train_step), at shapes that take a fraction of a second.
"""
import numpy as np
import pytest
import torch

from oracle import nsd_oracle as orc
from tests.golden.make_goldens import counter_masks, synth_labels, synth_x
from tests.gpu_harness import (BWD_T, FAST48, FWD_T, D, assert_step_vs_oracle, dev, multi_problem, multi_single, multi_step, nsd, oracle_step,  # noqa: F401
                               oracle_streams, soft_targets, spec_of, train_step)

pytestmark = pytest.mark.gpu

RNG = dict(seed=77, base_stream=8, p_lstm=0.6, p_head=0.6)


def _step(dev, flat_np, x, **kw):
    return train_step(dev, spec_of(D), flat_np, x, **kw)


# ---------------------------------------------------------------------------------------------------
# forward: what a step saves does not depend on how many steps follow it
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("residual", [False, True])
def test_forward_saves_of_a_prefix_are_bit_equal(nsd, dev, ref_state, residual, fused):
    """With explicit multipliers, h, c, the gates and the layer-1 input of the steps t < T' are the same bits in a launch on T
    steps and in one on its first T' steps, for T = T' + 1, + 2, + 17: the step that was the last of a tested block of the time
    loop (or of the saver's chunk) is a step of an untested one in the longer launch, or lies in another block of it."""
    B, tmax = 3, max(FWD_T) + 17
    flat_np = orc.flatten_state(ref_state, D)
    x, y = synth_x(B, tmax, seed=91), synth_labels(B, seed=91)
    dl, sl, dh = counter_masks(B, tmax, 48, 32, seed=92)
    regions = ("hseq", "cseq", "gact", "inseq")              # [layers, B, T, ...]

    def run(T):
        masks = dict(drop_lstm=np.ascontiguousarray(dl[:, :, :T]), rrelu_slope=sl, drop_head=dh)
        out = _step(dev, flat_np, np.ascontiguousarray(x[:, :T]), labels=y, masks=masks, fused=fused, residual=residual, saves=regions)
        assert all(np.isfinite(out[r]).all() for r in regions), T
        return out

    long_runs = {}
    for tp in FWD_T:
        short = run(tp)
        for d in (1, 2, 17):
            T = tp + d
            if T not in long_runs:
                long_runs[T] = run(T)
            for r in regions:
                a, b = short[r], long_runs[T][r][:, :, :tp]
                assert a.shape == b.shape and a.tobytes() == np.ascontiguousarray(b).tobytes(), (r, tp, T)


# ---------------------------------------------------------------------------------------------------
# backward and the whole step against the oracle
# ---------------------------------------------------------------------------------------------------
def _check_step_vs_oracle(dev, flat_np, B, T):
    """hard labels and soft targets; explicit multipliers with and without dx, and the same streams drawn in the kernels"""
    x, y, q = synth_x(B, T, seed=7 * B + T), synth_labels(B, seed=B + T), soft_targets(B, 3, seed=3 * B + T)
    masks = oracle_streams(RNG["seed"], RNG["base_stream"], B, T, 48, 32)           # the values the kernels draw from RNG
    for kind, tgt in (("hard", dict(labels=y)), ("soft", dict(targets=q))):
        ref = oracle_step(D, flat_np, x, masks=masks, want_dx=True, **tgt)
        plain = _step(dev, flat_np, x, masks=masks, **tgt)
        with_dx = _step(dev, flat_np, x, masks=masks, want_dx=True, **tgt)
        drawn = _step(dev, flat_np, x, rng=RNG, **tgt)
        for name, out in (("plain", plain), ("dx", with_dx), ("rng", drawn)):
            assert_step_vs_oracle(out, ref, D, FAST48)
        # the two mask modes run the same arithmetic on the same values
        for k in ("logits", "loss", "grads"):
            assert drawn[k].tobytes() == plain[k].tobytes(), (kind, k)


@pytest.mark.parametrize("T", BWD_T)
def test_step_vs_oracle_at_the_loop_edges(nsd, dev, ref_state, T):
    _check_step_vs_oracle(dev, orc.flatten_state(ref_state, D), 3, T)


@pytest.mark.parametrize("T", [7, 33])
def test_step_vs_oracle_when_a_workgroup_walks_a_second_trial(nsd, dev, ref_state, T):
    """Two trials more than the GPU has compute units: with dx the one-trial backward takes the batch, and two of its workgroups
    start their time loops a second time."""
    B = torch.cuda.get_device_properties(dev).multi_processor_count + 2
    _check_step_vs_oracle(dev, orc.flatten_state(ref_state, D), B, T)


# ---------------------------------------------------------------------------------------------------
# the model-batched twins include the same role code
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [15, 33])
def test_model_batched_launch_is_bit_equal_to_single_model_launches(nsd, dev, T):
    spec, M, B = spec_of(D), 2, 3
    params, x, y, rngs = multi_problem(spec, M, B, T, dev, seed=T)
    lg, gr, ls = multi_step(nsd, spec, params, x, y, rngs, dev)
    for m in range(M):
        l1, g1, s1 = multi_single(nsd, spec, params[m].clone(), x[m], y[m], rngs[m], dev)
        assert torch.equal(lg[m], l1), m
        assert torch.equal(gr[m], g1), m
        assert float(ls[m]) == s1, m
