"""The helper waves of the one-trial H = 48 backward at the sizes where a block edge can go wrong.  Needs the MI355X.

The x1 waves and the dW waves of nsd_lstm2_bwd48.hip run the blocks of 8 macro steps that h48_bwd_sched
(nsd_ring_block.h) names without a test of the step index, each wave in the instantiation of its own duty; the trial's first 16
steps (no complete window, no hand-off before step 4, layer 0 five steps behind) and its last blocks (t <= 0, da outside the trial)
keep the tests.  The edges are the first hand-off group, one, two and three 16-step windows, step counts that are 0 and 8 mod 16,
and a workgroup's second trial (accumulators and windows carried across).  Everything goes through ops.train_step_grads -- the
trainer's launch sequence, fused head -- or the module, against the CPU oracle within the bounds of this path
(tests/gpu_harness.py): LSTM weight gradients within 5e-5 of each tensor's largest element, every other tensor 2e-5
(+1e-7; attn.bias 2e-6 absolute), logits 1e-4, batch-mean loss 5e-5, dL/dx 2e-5; against stock autograd 2e-4 as the existing
input-gradient test.  The whole file takes a few seconds."""
import numpy as np
import pytest
import torch

from oracle import nsd_oracle as orc
from tests.golden.make_goldens import counter_masks, synth_labels, synth_params, synth_x
from tests.gpu_harness import FAST48, D, assert_step_vs_oracle, dev, nsd, oracle_step, spec_of, to_dev, train_step  # noqa: F401  (dev, nsd: fixtures)

pytestmark = pytest.mark.gpu

RNG = dict(seed=123, base_stream=12, p_lstm=0.6, p_head=0.6)


def _step(dev, flat_np, x, y, *, spec=None, **kw):
    """the fused step of the reference model (or of spec)"""
    return train_step(dev, spec or spec_of(D), flat_np, x, labels=y, **kw)


def _streams(B, T):
    """the multipliers the kernels draw from RNG, as tensors"""
    s, sid, p = RNG["seed"], RNG["base_stream"], RNG["p_lstm"]
    return dict(drop_lstm=orc.dropout_mask(s, sid, p, (1, B, T, 48)), rrelu_slope=orc.rrelu_noise(s, sid + 1, (B, 32)),
                drop_head=orc.dropout_mask(s, sid + 2, p, (B, 32)))


def _against_oracle(out, flat_np, x, y, d, masks, residual=False, want_dx=False):
    assert_step_vs_oracle(out, oracle_step(d, flat_np, x, labels=y, masks=masks, residual=residual, want_dx=want_dx), d, FAST48)


@pytest.fixture(scope="module")
def flat_ref(ref_state):
    return orc.flatten_state(ref_state, D)


@pytest.mark.parametrize("T", range(1, 49))
def test_every_step_count_up_to_three_windows(nsd, dev, flat_ref, T):
    """B = 3, C = 8, the multipliers drawn in the kernels (the benchmark's instantiations): the first hand-off group, one, two and
    three 16-step windows, step counts 0 and 8 mod 16; the same call twice gives the same bits."""
    B = 3
    x, y = synth_x(B, T, seed=500 + T), synth_labels(B, seed=600 + T)
    out = _step(dev, flat_ref, x, y, rng=RNG)
    _against_oracle(out, flat_ref, x, y, D, _streams(B, T))
    again = _step(dev, flat_ref, x, y, rng=RNG)
    assert again["grads"].tobytes() == out["grads"].tobytes() and again["logits"].tobytes() == out["logits"].tobytes()


@pytest.mark.parametrize("streams", ["none", "masks", "in-kernel"])
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("T", [5, 13, 21, 29, 37])
def test_residual_and_stream_variants(nsd, dev, flat_ref, T, residual, streams):
    """every loop variant of the x1 waves (residual pass-through on / off) and of the dW waves (multipliers drawn in the kernel or
    not), and layer 0's prep without multipliers"""
    B = 3
    x, y = synth_x(B, T, seed=700 + T), synth_labels(B, seed=800 + T)
    masks = {} if streams == "none" else _streams(B, T)
    kw = dict(rng=RNG) if streams == "in-kernel" else dict(masks=masks)
    out = _step(dev, flat_ref, x, y, residual=residual, **kw)
    _against_oracle(out, flat_ref, x, y, D, masks, residual=residual)
    again = _step(dev, flat_ref, x, y, residual=residual, **kw)
    assert again["grads"].tobytes() == out["grads"].tobytes()


def test_three_channels(nsd, dev):
    """C = 3 at T = 21: the x-rows duty with lanes past the last channel (rp >= C)"""
    from nsd_amd import ops
    C, K, B, T = 3, 3, 3, 21
    d, spec = orc.Dims(C=C, H=48, L=2, K=K), ops.ModelSpec(C=C, H=48, L=2, K=K)
    flat_np = orc.flatten_state(synth_params(C, 48, 2, K, seed=51), d)
    x, y = synth_x(B, T, C=C, seed=52), synth_labels(B, K=K, seed=53)
    dl, sl, dh = counter_masks(B, T, 48, 32, seed=54)
    masks = dict(drop_lstm=dl, rrelu_slope=sl, drop_head=dh)
    out = _step(dev, flat_np, x, y, spec=spec, masks=masks)
    _against_oracle(out, flat_np, x, y, d, masks)


@pytest.mark.parametrize("T", [21, 37])
def test_input_gradient_against_stock_autograd(nsd, dev, ref_state, T):
    """nsd_lstm_bwd with a dx buffer (the x1 wave without a prep duty sends da0 out: its own loop variant), through the module, against
    stock PyTorch on the CPU for the reference module's structure: 2e-4 of the largest element, as
    tests/test_gpu_parity.py::test_input_gradient_matches_torch_autograd"""
    from oracle.torch_ref import StackedTorchEEG
    B = 5
    ref = StackedTorchEEG(C=8, H=48, L=2, K=3).eval()
    ref.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in ref_state.items()}, strict=True)
    m = nsd.EEG_LSTM(input_size=8, hidden_size=48, num_layers=2, num_classes=3)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in ref_state.items()}, strict=True)
    m = m.to(dev).eval()
    xn, yn = synth_x(B, T, seed=900 + T), synth_labels(B, seed=901 + T).astype(np.int64)
    xr = torch.from_numpy(xn).requires_grad_(True)
    torch.nn.functional.cross_entropy(ref(xr), torch.from_numpy(yn)).backward()
    xg = to_dev(xn, dev).requires_grad_(True)
    torch.nn.functional.cross_entropy(m(xg), to_dev(yn, dev)).backward()
    assert xg.grad is not None and torch.isfinite(xg.grad).all()
    err, scale = (xg.grad.cpu() - xr.grad).abs().max().item(), xr.grad.abs().max().item()
    print(f"dx T={T}: max error {err:.3e}, largest element {scale:.3e}")
    assert err <= 2e-4 * scale + 1e-9, (err, scale)
    for (k, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        assert (p.grad.cpu() - q.grad).abs().max().item() <= 3e-4 * max(q.grad.abs().max().item(), 1e-6) + 2e-6, k


def test_a_workgroup_walks_two_trials(nsd, dev, flat_ref):
    """B = 260, T = 21 with dx: the input gradient keeps the one-trial kernel whatever the batch, so on 256 compute units four
    workgroups start their time loops a second time with the accumulators and the row windows of their first trial (without dx a
    batch above the CU count takes the two-trial kernel, which this file is not about; with dx the multipliers are explicit
    tensors: the entry point that draws them in the kernel forms no input gradient)"""
    B, T = 260, 21
    x, y = synth_x(B, T, seed=41), synth_labels(B, seed=42)
    masks = _streams(B, T)
    out = _step(dev, flat_ref, x, y, masks=masks, want_dx=True)
    _against_oracle(out, flat_ref, x, y, D, masks, want_dx=True)
    again = _step(dev, flat_ref, x, y, masks=masks, want_dx=True)
    assert again["grads"].tobytes() == out["grads"].tobytes() and again["dx"].tobytes() == out["dx"].tobytes()
