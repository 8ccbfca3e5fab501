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
from tests import mixup_ref as mr
from tests.golden.make_goldens import counter_masks, synth_labels, synth_x
from tests.test_gpu_multimodel import _multi, _problem, _single, _spec
from tests.test_gpu_parity import DX_TOL, FAST48, LOGIT_TOL, D, _grad_close, _t, dev, nsd  # noqa: F401  (dev, nsd: fixtures)
from tests.test_gpu_soft_targets import LOSS_TOL, _oracle_streams, _targets

pytestmark = pytest.mark.gpu

# T' of the forward's prefix pairs: around the ring (16), the x chunk (32) and their multiples, +-2 for layer 1's lag
FWD_T = (1, 2, 3, 13, 14, 15, 16, 17, 18, 29, 30, 31, 32, 33, 34, 47, 48, 49, 63, 64, 65)
# ... and what the backward adds: its 8-step ring, the four-step hand-off groups and layer 0's five-step lag
BWD_T = tuple(sorted(set(FWD_T) | {4, 5, 6, 7, 8, 9, 11, 12, 20, 21, 24, 25}))
RNG = dict(seed=77, base_stream=8, p_lstm=0.6, p_head=0.6)


def _step(dev, flat_np, x, *, labels=None, targets=None, masks=None, rng=None, want_dx=False, fused=True, residual=False, saves=()):
    """ops.train_step_grads -> logits, per-trial loss, flat gradient (+ dx, + the named workspace regions)"""
    from nsd_amd import ops
    spec = ops.ModelSpec()
    B, T, _ = x.shape
    flat, xt = _t(flat_np, dev), _t(x, dev)
    ws = ops.new_workspace(spec, B, T, dev)
    ws.fill_(float("nan"))                                   # nothing may be left unwritten
    logits = torch.full((B, spec.K), float("nan"), device=dev)
    grads = torch.empty_like(flat)
    dx = torch.full_like(xt, float("nan")) if want_dx else None
    ops.train_step_grads(spec, flat, xt, ws, _t(labels, dev), logits, grads, residual=residual, fused_head=fused, rng=rng, dx=dx,
                         targets=_t(targets, dev), **{k: _t(v, dev) for k, v in (masks or {}).items()})
    out = dict(logits=logits.cpu().numpy(), grads=grads.cpu().numpy(), loss=ops.ws_view(ws, spec, B, T, "loss").cpu().numpy().copy())
    if want_dx:
        out["dx"] = dx.cpu().numpy()
    for r in saves:
        out[r] = ops.ws_view(ws, spec, B, T, r).cpu().numpy().copy()
    return out


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
def _oracle(flat_np, x, masks, labels=None, targets=None):
    fw = orc.forward(flat_np, x, D, saves=True, **masks)
    if targets is None:
        loss, dl = orc.ce_loss(fw["logits"], labels)
    else:
        loss, dl = mr.soft_ce(fw["logits"], targets, 1.0 / x.shape[0])
    g, dx = orc.backward(flat_np, x, D, fw, dl.astype(np.float32), want_dx=True, **masks)
    return fw["logits"], float(np.sum(loss)) / x.shape[0] if np.ndim(loss) else float(loss), g, dx      # (mean loss)


def _check_step_vs_oracle(dev, flat_np, B, T):
    """hard labels and soft targets; explicit multipliers with and without dx, and the same streams drawn in the kernels"""
    x, y, q = synth_x(B, T, seed=7 * B + T), synth_labels(B, seed=B + T), _targets(B, 3, seed=3 * B + T)
    masks = _oracle_streams(RNG["seed"], RNG["base_stream"], B, T, 48, 32)           # the values the kernels draw from RNG
    for kind, tgt in (("hard", dict(labels=y)), ("soft", dict(targets=q))):
        lg_ref, loss_ref, g_ref, dx_ref = _oracle(flat_np, x, masks, **tgt)
        plain = _step(dev, flat_np, x, masks=masks, **tgt)
        with_dx = _step(dev, flat_np, x, masks=masks, want_dx=True, **tgt)
        drawn = _step(dev, flat_np, x, rng=RNG, **tgt)
        for name, out in (("plain", plain), ("dx", with_dx), ("rng", drawn)):
            assert np.abs(out["logits"] - lg_ref).max() < LOGIT_TOL, (kind, name)
            assert abs(float(out["loss"].sum()) / B - loss_ref) < LOSS_TOL, (kind, name)
            _grad_close(out["grads"], g_ref, D, **FAST48)
        err, scale = float(np.abs(with_dx["dx"] - dx_ref).max()), float(np.abs(dx_ref).max())
        print(f"dx B={B} T={T} {kind}: max error / largest element {err / scale:.2e}")
        assert err <= DX_TOL * scale, (kind, err, scale)
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
    spec, M, B = _spec(nsd), 2, 3
    params, x, y, rngs = _problem(spec, M, B, T, dev, seed=T)
    lg, gr, ls = _multi(nsd, spec, params, x, y, rngs, dev)
    for m in range(M):
        l1, g1, s1 = _single(nsd, spec, params[m].clone(), x[m], y[m], rngs[m], dev)
        assert torch.equal(lg[m], l1), m
        assert torch.equal(gr[m], g1), m
        assert float(ls[m]) == s1, m
