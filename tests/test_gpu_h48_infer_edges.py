"""The single-launch inference tail of the H = 48 kernel at every loop edge.  Needs the MI355X.

ops.infer runs the `l0` / `l1` / `p` roles of nsd_lstm2_fwd48.hip instantiated WITHOUT saves plus pool_role: the online softmax over
8-step chunks of the save ring, one chunk behind the recurrence.  That instantiation received the ring blocks without a step test
as the training one did, but saves nothing, so the prefix comparison of tests/test_gpu_h48_step_loops.py cannot see it.  Here every
T of 1..100 -- the 8-step pool chunk, the 16-step ring, the 32-step x chunk with n_steps = ceil((T + 2) / 32) * 32 -- and the step
counts around 128, 256 and the fast path's limit of 1024 (1025 and 1026 leave it) go against the CPU oracle's eval-mode forward, at
the project's bounds: logits 1e-4, probabilities 1e-5, rows of probabilities summing to 1 within 1e-6, the same argmax wherever the
oracle's top two logits are more than 1e-3 apart; and each trial launched alone gives the bits of its row of the batch launch.
Outputs and scratch are NaN-filled before every call.  Each case takes a few milliseconds.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import nsd_oracle as orc
from tests.golden.make_goldens import synth_params, synth_x
from tests.gpu_harness import INFER_T, LOGIT_TOL, PROB_TOL, D, dev, nsd, to_dev  # noqa: F401  (dev, nsd: fixtures)

pytestmark = pytest.mark.gpu

ROW_SUM_TOL, ARGMAX_GAP = 1e-6, 1e-3


def _infer(dev, spec, flat, x, *, residual=False, want_probs=True):
    """ops.infer into NaN-filled logits / probs / scratch -> numpy logits, probs (None without want_probs)"""
    from nsd_amd import _lib, ops
    B, T, _ = x.shape
    dims = spec.dims(B, T)
    nscr = int(_lib.lib().nsd_infer_scratch_bytes(ctypes.byref(dims)))
    scratch = torch.full((max(nscr // 4, 1),), float("nan"), device=dev)
    logits = torch.full((B, spec.K), float("nan"), device=dev)
    probs = torch.full((B, spec.K), float("nan"), device=dev) if want_probs else None
    lg, pr = ops.infer(spec, flat, x, residual=residual, want_probs=want_probs, logits=logits, probs=probs, scratch=scratch)
    assert lg is logits and pr is probs
    return logits.cpu().numpy(), None if probs is None else probs.cpu().numpy()


def _check_vs_oracle(lg, pr, flat_np, x, d, residual=False, what=None):
    ref = orc.forward(flat_np, x, d, residual=residual)
    e_l = float(np.abs(lg - ref["logits"]).max())
    assert e_l < LOGIT_TOL, (what, e_l)                       # (a NaN left in an output fails here)
    if pr is not None:
        e_p, e_s = float(np.abs(pr - ref["probs"]).max()), float(np.abs(pr.astype(np.float64).sum(1) - 1.0).max())
        print(f"infer {what}: logits {e_l:.2e} probs {e_p:.2e} row sums {e_s:.2e}")
        assert e_p < PROB_TOL, (what, e_p)
        assert e_s < ROW_SUM_TOL, (what, e_s)
    top = np.sort(ref["logits"], axis=1)
    clear = (top[:, -1] - top[:, -2]) > ARGMAX_GAP
    assert np.array_equal(lg.argmax(1)[clear], ref["logits"].argmax(1)[clear]), what
    return ref


@pytest.mark.parametrize("T", INFER_T)
def test_inference_vs_oracle_at_every_step_count(nsd, dev, ref_state, T):
    """B = 3 with the reference checkpoint: against the oracle, and batch invariance -- each trial alone is bit-equal to its row."""
    from nsd_amd import ops
    spec, B = ops.ModelSpec(), 3
    flat_np = orc.flatten_state(ref_state, D)
    flat, xn = to_dev(flat_np, dev), synth_x(B, T, seed=500 + T)
    x = to_dev(xn, dev)
    lg, pr = _infer(dev, spec, flat, x)
    _check_vs_oracle(lg, pr, flat_np, xn, D, what=("T", T))
    for b in range(B):
        l1, p1 = _infer(dev, spec, flat, x[b:b + 1].contiguous())
        assert l1.tobytes() == lg[b:b + 1].tobytes() and p1.tobytes() == pr[b:b + 1].tobytes(), (T, b)
    # without probabilities: the same logits, and the absent output is not touched
    l0, p0 = _infer(dev, spec, flat, x, want_probs=False)
    assert p0 is None and l0.tobytes() == lg.tobytes(), T


@pytest.mark.parametrize("T", [1, 2, 6, 7, 14, 15, 30, 31, 62])
def test_inference_residual_flag_and_three_channels(nsd, dev, ref_state, T):
    """The residual stack with the reference checkpoint, and a C = 3 model (x rows shorter than the 8 floats the staging is laid
    out for), at the step counts one and two short of the pool chunk, the ring, the x chunk and two x chunks."""
    from nsd_amd import ops
    B = 3
    flat_np, xn = orc.flatten_state(ref_state, D), synth_x(B, T, seed=700 + T)
    lg, pr = _infer(dev, ops.ModelSpec(), to_dev(flat_np, dev), to_dev(xn, dev), residual=True)
    _check_vs_oracle(lg, pr, flat_np, xn, D, residual=True, what=("residual", T))
    d3, spec3 = orc.Dims(C=3), ops.ModelSpec(C=3)
    flat3, x3 = orc.flatten_state(synth_params(3, 48, 2, 3, seed=43), d3), synth_x(B, T, C=3, seed=800 + T)
    for residual in (False, True):
        lg, pr = _infer(dev, spec3, to_dev(flat3, dev), to_dev(x3, dev), residual=residual)
        _check_vs_oracle(lg, pr, flat3, x3, d3, residual=residual, what=("C=3", residual, T))


@pytest.mark.parametrize("T", [7, 33, 41])
def test_inference_when_a_workgroup_pools_a_second_trial(nsd, dev, ref_state, T):
    """Two trials more than the GPU has compute units: two workgroups reset the pooling state and walk the time loop again."""
    from nsd_amd import ops
    spec = ops.ModelSpec()
    B = torch.cuda.get_device_properties(dev).multi_processor_count + 2
    flat_np, xn = orc.flatten_state(ref_state, D), synth_x(B, T, seed=900 + T)
    flat, x = to_dev(flat_np, dev), to_dev(xn, dev)
    lg, pr = _infer(dev, spec, flat, x)
    _check_vs_oracle(lg, pr, flat_np, xn, D, what=("B", B, "T", T))
    for b in (0, 1, B - 2, B - 1):                            # first and second trial of the workgroups that loop
        l1, p1 = _infer(dev, spec, flat, x[b:b + 1].contiguous())
        assert l1.tobytes() == lg[b:b + 1].tobytes() and p1.tobytes() == pr[b:b + 1].tobytes(), (T, b)
    l0, p0 = _infer(dev, spec, flat, x, want_probs=False)
    assert p0 is None and l0.tobytes() == lg.tobytes(), T
