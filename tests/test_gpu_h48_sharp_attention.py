"""Every attention path with PEAKED attention weights against the CPU oracle.  Needs the MI355X.

With the parameters the rest of the suite uses, alpha is within a few percent of 1 / T: the online softmax's rescale
scale = exp(mrun - mnew) and its -inf start, the numerators, the alpha-weighted terms of the attention backward (fused tail,
nsd_head.hip, and the part deferred to the four-trial backward kernel and closed by nsd_att_close) all run next to a no-op.  The
inputs of tests/sharp_attention.py multiply attn.weight by s: at s = 100 alpha spreads over e^5.6 .. e^16.6 and everything is compared,
gradients included; at s = 1000 alpha is exactly 0 / 1 in places and logits, probabilities and the loss are compared (the fp32 oracle's
own gradients are off by up to 2.8e-5 there).  tests/test_sharp_attention_cpu.py holds the oracle to a quarter of each bound against
the float64 model on these very inputs.

Bounds: the project's (tests/gpu_harness.py) -- logits 1e-4, probabilities 1e-5, batch-mean loss 5e-5, FAST48 (LSTM weight
gradients 5e-5 of each tensor's largest element, other tensors 2e-5 + 1e-7, attn.bias 2e-6 absolute), dL/dx 2e-5; FP32_EXACT on the
H = 32 kernels and the generic path.  Workspace and outputs are NaN-filled before every call.
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from oracle import nsd_oracle as orc
from tests import sharp_attention as sa
from tests.gpu_harness import (FAST48, FP32_EXACT, LOGIT_TOL, LOSS_TOL, PROB_TOL, D, assert_step_vs_oracle, dev, nsd, oracle_step,  # noqa: F401
                               to_dev, train_step)

pytestmark = pytest.mark.gpu


def _step(dev, spec, flat_np, x, **kw):
    """train_step with the batch-mean loss of ops.loss_sum, the kernel the trainers read it with"""
    out = train_step(dev, spec, flat_np, x, **kw)
    out["mean_loss"] = out["loss_sum"] / x.shape[0]
    return out


_REFS = {}


def _oracle(s, B, T, kind, H=48):
    """oracle forward + backward of the (s, B, T) case with hard labels or soft targets; computed once per session, never changed"""
    key = (s, B, T, kind, H)
    if key not in _REFS:
        d = orc.Dims(H=H)
        x, y, q, masks = sa.sharp_inputs(B, T, H=H)
        ref = oracle_step(d, orc.flatten_state(sa.sharp_state(s, H=H), d), x, masks=masks, want_dx=True,
                          **(dict(labels=y) if kind == "hard" else dict(targets=q)))
        for a in (ref["logits"], ref["grads"], ref["dx"]):
            a.setflags(write=False)
        _REFS[key] = dict(ref, spread=sa.spread(ref["fw"]["alpha"]))
    return _REFS[key]


def _check(out, ref, s, what, d=D, bounds=FAST48):
    e_l, e_s = float(np.abs(out["logits"] - ref["logits"]).max()), abs(out["mean_loss"] - ref["loss"])
    print(f"sharp {what} s={s:g}: spread {ref['spread']:.1f} logits {e_l:.2e} loss {e_s:.2e}")
    if s == sa.S_GRAD:
        assert_step_vs_oracle(out, ref, d, bounds)
        return
    assert e_l < LOGIT_TOL, (what, s, e_l)
    assert e_s < LOSS_TOL, (what, s, e_s)
    assert np.isfinite(out["grads"]).all(), (what, s)


@contextlib.contextmanager
def _forced(fwd=0, bwd=0):
    """the diagnostic twin of the library with the forward / backward instantiation pinned; the forces are reset on the way out"""
    from nsd_amd import _lib, ops
    if not (fwd or bwd):
        yield
        return
    with _lib.diagnostic_library():
        try:
            ops.force_fwd48(fwd)
            ops.force_bwd48(bwd)
            yield
        finally:
            ops.force_fwd48(0)
            ops.force_bwd48(0)


# ---------------------------------------------------------------------------------------------------
# inference
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [sa.S_GRAD, sa.S_SAT])
@pytest.mark.parametrize("T", sa.SHARP_T)
def test_inference_with_peaked_attention(nsd, dev, T, s):
    """ops.infer and ops.multi_infer (M = 2: parameter seeds 7 and 8, shared windows)"""
    from nsd_amd import _lib, ops
    spec, B = ops.ModelSpec(), sa.SHARP_B
    x = sa.sharp_inputs(B, T)[0]
    dims = spec.dims(B, T)
    nscr = max(int(_lib.lib().nsd_infer_scratch_bytes(ctypes.byref(dims))), int(_lib.lib().nsd_multi_infer_scratch_bytes(ctypes.byref(dims), 2)))
    flats = [orc.flatten_state(sa.sharp_state(s, seed=sa.PARAM_SEED + m), D) for m in range(2)]
    refs = [orc.forward(f, x, D) for f in flats]
    xt = to_dev(x, dev)
    logits, probs = torch.full((B, 3), float("nan"), device=dev), torch.full((B, 3), float("nan"), device=dev)
    ops.infer(spec, to_dev(flats[0], dev), xt, logits=logits, probs=probs, scratch=torch.full((max(nscr // 4, 1),), float("nan"), device=dev))
    lm, pm = torch.full((2, B, 3), float("nan"), device=dev), torch.full((2, B, 3), float("nan"), device=dev)
    ops.multi_infer(spec, to_dev(np.stack(flats), dev), xt, logits=lm, probs=pm, scratch=torch.full((max(nscr // 4, 1),), float("nan"), device=dev))
    got = [("infer", logits, probs, refs[0]), ("multi_infer[0]", lm[0], pm[0], refs[0]), ("multi_infer[1]", lm[1], pm[1], refs[1])]
    for name, lg, pr, ref in got:
        e_l, e_p = float(np.abs(lg.cpu().numpy() - ref["logits"]).max()), float(np.abs(pr.cpu().numpy() - ref["probs"]).max())
        print(f"sharp {name} T={T} s={s:g}: logits {e_l:.2e} probs {e_p:.2e}")
        assert e_l < LOGIT_TOL and e_p < PROB_TOL, (name, e_l, e_p)
    assert torch.equal(lm[0], logits) and torch.equal(pm[0], probs)


# ---------------------------------------------------------------------------------------------------
# the train step
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [sa.S_GRAD, sa.S_SAT])
@pytest.mark.parametrize("T", sa.SHARP_T)
def test_one_trial_step_with_peaked_attention(nsd, dev, T, s):
    """the fused step with hard labels, with soft targets and with dx; the unfused head (nsd_head.hip's train and backward kernels);
    the two-trial forward"""
    from nsd_amd import ops
    spec, B = ops.ModelSpec(), sa.SHARP_B
    flat = orc.flatten_state(sa.sharp_state(s), D)
    x, y, q, masks = sa.sharp_inputs(B, T)
    for kind, tgt in (("hard", dict(labels=y)), ("soft", dict(targets=q))):
        ref = _oracle(s, B, T, kind)
        _check(_step(dev, spec, flat, x, masks=masks, **tgt), ref, s, (T, kind, "fused"))
        _check(_step(dev, spec, flat, x, masks=masks, want_dx=True, **tgt), ref, s, (T, kind, "fused, dx"))
        _check(_step(dev, spec, flat, x, masks=masks, fused=False, **tgt), ref, s, (T, kind, "unfused head"))
        _check(_step(dev, spec, flat, x, masks=masks, fused=False, want_dx=True, **tgt), ref, s, (T, kind, "unfused head, dx"))
    with _forced(fwd=2):
        _check(_step(dev, spec, flat, x, labels=y, masks=masks), _oracle(s, B, T, "hard"), s, (T, "two-trial forward"))


@pytest.mark.parametrize("s", [sa.S_GRAD, sa.S_SAT])
@pytest.mark.parametrize("B", [6, 5])
@pytest.mark.parametrize("T", sa.SHARP_T)
def test_four_trial_kernels_with_peaked_attention(nsd, dev, T, B, s):
    """four-trial forward + backward: the forward leaves alpha and OPEN records, the backward kernel forms dL/dscore; with dx the
    records are closed by nsd_att_close and the one-trial backward runs.  B = 5: a padding trial in the second group."""
    from nsd_amd import ops
    spec = ops.ModelSpec()
    flat = orc.flatten_state(sa.sharp_state(s), D)
    x, y, q, masks = sa.sharp_inputs(B, T)
    with _forced(fwd=4, bwd=4):
        _check(_step(dev, spec, flat, x, labels=y, masks=masks), _oracle(s, B, T, "hard"), s, (T, B, "x4"))
        _check(_step(dev, spec, flat, x, labels=y, masks=masks, want_dx=True), _oracle(s, B, T, "hard"), s, (T, B, "x4, dx"))
        _check(_step(dev, spec, flat, x, targets=q, masks=masks), _oracle(s, B, T, "soft"), s, (T, B, "x4, soft"))


@pytest.mark.parametrize("T", sa.SHARP_T)
def test_model_batched_step_with_peaked_attention(nsd, dev, T):
    """M = 2 sharp models, own windows, streams drawn in the kernels, against the oracle with the streams of rngs[m] regenerated on
    the host (sharp_attention.multi_case)"""
    from nsd_amd import ops
    spec, M, B = ops.ModelSpec(), 2, sa.SHARP_B
    states, xs, ys, rngs, masks = sa.multi_case(T, M, B)
    flats = np.stack([orc.flatten_state(st, D) for st in states])
    ws = ops.multi_workspace(spec, M, B, T, dev)
    ws.fill_(float("nan"))
    grads = torch.full((M, spec.param_count), float("nan"), device=dev)
    logits = torch.full((M * B, spec.K), float("nan"), device=dev)
    ops.multi_train_step(spec, to_dev(flats, dev), to_dev(xs, dev), to_dev(ys.reshape(-1), dev), ws, grads, rngs=rngs, logits=logits, fuse_adam=False)
    losses = ops.multi_loss_sum(spec, ws, M, B, T).cpu().numpy() / B
    for m in range(M):
        loss_ref, g_ref, fw = orc.loss_and_grads(flats[m], xs[m], ys[m], D, **masks[m])
        out = dict(logits=logits.view(M, B, -1)[m].cpu().numpy(), grads=grads[m].cpu().numpy(), mean_loss=float(losses[m]))
        _check(out, dict(logits=fw["logits"], loss=loss_ref, grads=g_ref, spread=sa.spread(fw["alpha"])), sa.S_GRAD, (T, "model", m))


@pytest.mark.parametrize("H", [32, 40])
def test_exact_fp32_routes_with_peaked_attention(nsd, dev, H):
    """one case each on the first-generation H = 32 kernels and on the generic path (H = 40), fused and unfused head: FP32_EXACT"""
    from nsd_amd import ops
    B, T, d, spec = sa.SHARP_B, 64, orc.Dims(H=H), ops.ModelSpec(H=H)
    flat = orc.flatten_state(sa.sharp_state(sa.S_GRAD, H=H), d)
    x, y, _, masks = sa.sharp_inputs(B, T, H=H)
    ref = _oracle(sa.S_GRAD, B, T, "hard", H=H)
    assert ref["spread"] > 5.0
    for fused in (True, False):
        _check(_step(dev, spec, flat, x, labels=y, masks=masks, fused=fused), ref, sa.S_GRAD, (H, "fused" if fused else "unfused"), d=d,
               bounds=FP32_EXACT)
