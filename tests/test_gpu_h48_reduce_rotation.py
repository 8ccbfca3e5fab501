"""The rotated slot ownership of the H = 48 chain roles (quad_reduce_scatter, nsd_common.h) on the GPU.  Needs the MI355X.

Slot i of lane s of a quad holds gate (backward: output unit) i ^ s; the weights are loaded that way in front of the time loops of
nsd_lstm2_fwd48.hip, nsd_lstm2_bwd48.hip, nsd_stream48.hip and nsd_window48.hip (and of their model-batched twins).  A gate row that
lands in the wrong slot changes a lane's whole sum, so every case here runs on SEEDED weights without any symmetry between gates (the
generators of tests/golden/make_goldens.py), where a swapped row shows in every tensor: whole train steps against the CPU oracle at
the harness's bounds (tests/gpu_harness.py), and the inference kernels against the oracle's batch forward with the comparisons of
their own test files.  Each case takes a fraction of a second.
"""
import numpy as np
import pytest
import torch

from oracle import nsd_oracle as orc
from tests import test_gpu_h48_infer_edges as tie
from tests import test_gpu_stream as tgs
from tests import test_gpu_window as tgw
from tests.golden.make_goldens import counter_masks, synth_labels, synth_params, synth_x
from tests.gpu_harness import (FAST48, KINK, KINK_MARGIN, assert_step_vs_oracle, dev, kink_safe, multi_problem, multi_step, nsd,  # noqa: F401
                               oracle_step, oracle_streams, spec_of, sync_at_the_end, to_dev, train_step)

pytestmark = pytest.mark.gpu

RNG = dict(seed=2113, base_stream=12, p_lstm=0.6, p_head=0.6)


def _problem(C, B, T):
    """(dims, flat parameters, x, labels) with seeded weights: no two gate rows alike.  fc.0.bias = +-4 (kink_safe): no pre-activation
    of any batch size sits at the RReLU kink, where oracle and kernel may round to different sides"""
    d = orc.Dims(C=C)
    flat = orc.flatten_state(kink_safe(synth_params(C, 48, 2, 3, F=32, seed=100 + C), 32), d)
    return d, flat, synth_x(B, T, C=C, seed=10 * T + C + B), synth_labels(B, seed=T + B)


# ---------------------------------------------------------------------------------------------------
# whole train steps against the oracle
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("C", [8, 5])
@pytest.mark.parametrize("T", [5, 33])
def test_one_trial_step_vs_oracle_with_seeded_weights(nsd, dev, T, C, residual, fused):
    """B = 3: the one-trial kernels.  C = 5: the zero-padded x columns of the rotated w_ih0 rows.  Explicit multipliers, the same
    streams drawn in the kernels (fused head: the only route that draws them) and, at T = 33 with C = 5, the input gradient."""
    d, flat, x, y = _problem(C, 3, T)
    masks = oracle_streams(RNG["seed"], RNG["base_stream"], 3, T, 48, 32)               # the values the kernels draw from RNG
    want_dx = T == 33 and C == 5
    ref = oracle_step(d, flat, x, labels=y, masks=masks, residual=residual, want_dx=want_dx, kink=KINK_MARGIN)
    plain = train_step(dev, spec_of(d), flat, x, labels=y, masks=masks, residual=residual, fused=fused, want_dx=want_dx)
    assert_step_vs_oracle(plain, ref, d, FAST48, tag=("explicit", T, C, residual, fused))
    if fused:
        drawn = train_step(dev, spec_of(d), flat, x, labels=y, rng=RNG, residual=residual)
        assert_step_vs_oracle(drawn, ref, d, FAST48, tag=("drawn", T, C, residual))
        for k in ("logits", "loss", "grads"):                                           # the same arithmetic on the same values
            assert drawn[k].tobytes() == plain[k].tobytes(), k


@pytest.mark.parametrize("B,residual", [(258, False), (258, True), (514, True)])
def test_two_trial_kernels_vs_oracle_with_seeded_weights(nsd, dev, B, residual):
    """T = 5.  258 trials: more than one per compute unit, the two-trial forward (the backward walks them one by one).  514 trials with
    the residual stack, which the four-trial kernels do not take: the two-trial backward, its first-generation x1 role included."""
    T = 5
    assert B > torch.cuda.get_device_properties(dev).multi_processor_count
    d, flat, x, y = _problem(8, B, T)
    dl, sl, dh = counter_masks(B, T, 48, 32, seed=B + T)
    masks = dict(drop_lstm=dl, rrelu_slope=sl, drop_head=dh)
    ref = oracle_step(d, flat, x, labels=y, masks=masks, residual=residual, kink=KINK_MARGIN)
    for fused in (True, False):
        out = train_step(dev, spec_of(d), flat, x, labels=y, masks=masks, residual=residual, fused=fused)
        assert_step_vs_oracle(out, ref, d, FAST48, tag=("B", B, residual, fused))


def test_model_batched_twins_vs_oracle(nsd, dev):
    """M = 2 models at B = 3, T = 33, random parameters per model, streams drawn in the kernels: each model against the oracle."""
    d = orc.Dims()
    spec, M, B, T = spec_of(d), 2, 3, 33
    params, x, y, rngs = multi_problem(spec, M, B, T, dev, seed=3301)
    lg, gr, ls = multi_step(nsd, spec, params, x, y, rngs, dev)
    for m in range(M):
        masks = oracle_streams(rngs[m]["seed"], rngs[m]["base_stream"], B, T, 48, 32)
        ref = oracle_step(d, params[m].cpu().numpy(), x[m].cpu().numpy(), labels=y[m].cpu().numpy(), masks=masks, kink=KINK)
        out = dict(logits=lg[m].cpu().numpy(), grads=gr[m].cpu().numpy(), mean_loss=float(ls[m]))
        assert_step_vs_oracle(out, ref, d, FAST48, tag=("model", m))


# ---------------------------------------------------------------------------------------------------
# inference: the one-launch tail and the chunked decoders against the batch forward
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,residual", [(8, False), (8, True), (5, False)])
def test_inference_kernels_vs_the_batch_forward(nsd, dev, C, residual):
    """B = 2, T = 33, seeded weights: nsd_infer, nsd_stream_step in chunks and nsd_window_step (a window of the whole length and
    hopping windows of 16) against the oracle's forward, with the comparisons of their own test files."""
    B, T = 2, 33
    d, flat_np, xn, _ = _problem(C, B, T)
    spec, flat, x = spec_of(d), to_dev(flat_np, dev), to_dev(xn, dev)
    lg, pr = tie._infer(dev, spec, flat, x, residual=residual)
    ref = tie._check_vs_oracle(lg, pr, flat_np, xn, d, residual=residual, what=("infer", C, residual))
    # the stream decoder: one call, and chunks that end on both sides of the 32-step staging chunk
    ends = []
    for cut in ([33], [32, 1], [5, 11, 17]):
        state = tgs._new_state(dev, spec, B)
        slg, spr = tgs._run_cut(dev, spec, flat, x, cut, state, residual=residual)
        tgs._check_outputs(slg, spr, ref, ("stream", C, residual, cut))
        ends.append((state.cpu().numpy().tobytes(), slg.tobytes(), spr.tobytes()))
    assert ends[0] == ends[1] == ends[2]
    # the sliding-window decoder: the whole length as one window, then windows of 16 every 8 samples
    for W, Hp in ((33, 33), (16, 8)):
        for cut in ([33], [20, 13]):
            state = tgw._new_state(dev, spec, W, Hp, B)
            got = tgw._run(dev, spec, flat, x, cut, state, W, Hp, residual=residual)
            assert sorted(got) == list(range((T - W) // Hp + 1)), sorted(got)
            for k, (wlg, wpr) in got.items():
                xw = np.ascontiguousarray(xn[:, k * Hp:k * Hp + W])
                wref = ref if W == T else orc.forward(flat_np, xw, d, residual=residual)
                tgs._check_outputs(wlg, wpr, wref, ("window", C, residual, W, Hp, cut, k))
