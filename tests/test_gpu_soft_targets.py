"""Soft targets on the MI355X: nsd_mixup against its numpy restatement (tests/mixup_ref.py) bit for bit; the `_soft` entry points of
every fused head against the oracle (forward -> dlogits = scale (s p - q) in float64 from the oracle's logits -> backward), against
their hard-label twins on one-hot rows and against each other (explicit masks / in-kernel streams, one model / several); the
cancellation-free form of s p - q; both trainers with loss= against the step without it fed the restatement's windows and targets."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import nsd_oracle as orc
from tests import mixup_ref as mr
from tests.golden.make_goldens import synth_labels, synth_params, synth_x
from tests.gpu_harness import (FAST48, FP32_EXACT, GRAD_RTOL_12, GRAD_RTOL_X4, LOGIT_TOL, LOSS_TOL, dev, grad_close, model_from_state, nsd,  # noqa: F401
                               oracle_step, oracle_streams, soft_targets, sync_at_the_end, to_dev, train_step)

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(t: torch.Tensor, ref: np.ndarray) -> bool:
    return t.shape == ref.shape and np.array_equal(_bits(t.cpu().numpy()), _bits(ref))


# ---- 1. nsd_mixup bit for bit ------------------------------------------------------------------------------------------------------------
# T*C = 1, 3, 21 (scalar tail), 2000 and 320 (16-byte path); B = 1 (nothing to mix with), 33 > one wave; K = 64: the widest row
MIX_SHAPES = [(1, 1, 1, 2), (2, 3, 1, 3), (5, 7, 3, 5), (33, 250, 8, 3), (6, 5, 64, 64)]


def _mix_configs(K, seed):
    w = (0.25 + np.random.RandomState(seed).rand(K)).astype(np.float32)
    w[seed % K] = 0.0
    return [dict(weights=w), dict(eps=0.1), dict(mix=1.0), dict(mix=0.37), dict(mix=0.6, eps=0.2, weights=w), {}]


def _ops_mixup(ops, x, labels, K, rngs, dev, mix=0.0, eps=0.0, weights=None, **kw):
    return ops.mixup(x, labels, K, rngs, label_smoothing=eps, mix=mix, class_weights=to_dev(weights, dev), **kw)


@pytest.mark.parametrize("B,T,C,K", MIX_SHAPES)
def test_mixup_kernel_equals_numpy_bitwise(nsd, dev, B, T, C, K):
    from nsd_amd import ops
    x_np, lab_np = synth_x(B, T, C, seed=B + T + C), synth_labels(B, K, seed=B + K)
    x, lab = to_dev(x_np, dev), to_dev(lab_np, dev)
    for i, kw in enumerate(_mix_configs(K, B + K)):
        seed, base = 0x9E3779B97F4A7C15 + 31 * i, 4 * (i + 1)
        y, tg = _ops_mixup(ops, x, lab, K, dict(seed=seed, base_stream=base), dev, **kw)
        y_ref, tg_ref = mr.mixup(x_np, lab_np, K, seed, base, **kw)
        assert _same_bits(tg.view(B, K), tg_ref), kw
        assert y.data_ptr() != x.data_ptr() and _same_bits(y, y_ref), kw
        # the device step counter gives the stream id of the explicit form
        step_dev = torch.tensor([i + 1], dtype=torch.int64, device=dev)
        y2, tg2 = _ops_mixup(ops, x, lab, K, dict(seed=seed, base_stream=999), dev, step_dev=step_dev, **kw)
        assert torch.equal(y2, y) and torch.equal(tg2, tg), kw
        if not kw.get("mix"):                                       # targets-only call: NULL x / y
            none, tg3 = _ops_mixup(ops, None, lab, K, dict(seed=seed, base_stream=base), dev, **kw)
            assert none is None and torch.equal(tg3, tg), kw
    if B >= 2:
        assert not np.array_equal(mr.mixup(x_np, lab_np, K, 5, 4, mix=1.0)[0], x_np)      # (the mixing does something)


@pytest.mark.parametrize("B,T,C,K", [(5, 7, 3, 5), (33, 250, 8, 3), (1, 1, 1, 2)])
def test_mixup_models_in_one_launch(nsd, dev, B, T, C, K):
    """M = 3 with shared windows (stride 0) and with per-model windows: row m is the M = 1 call with rng[m], bitwise, and the restatement."""
    from nsd_amd import ops
    w = np.linspace(0.5, 1.5, K).astype(np.float32)
    kw = dict(mix=0.8, eps=0.1, weights=w)
    rngs = [dict(seed=1000 + 17 * m, base_stream=4 * (m + 2)) for m in range(3)]
    pairs = [(r["seed"], r["base_stream"]) for r in rngs]
    xs_np = synth_x(3 * B, T, C, seed=7).reshape(3, B, T, C)
    lab_np = synth_labels(3 * B, K, seed=9).reshape(3, B)
    xs, lab = to_dev(xs_np, dev), to_dev(lab_np.reshape(-1), dev)
    shared, tg_s = _ops_mixup(ops, xs[0].contiguous(), lab, K, rngs, dev, M=3, **kw)
    own, tg_o = _ops_mixup(ops, xs, lab, K, rngs, dev, **kw)
    ys_ref, tgs_ref = mr.mixup_models(xs_np[0], lab_np, K, pairs, **kw)
    yo_ref, tgo_ref = mr.mixup_models(xs_np, lab_np, K, pairs, **kw)
    assert _same_bits(shared, ys_ref) and _same_bits(own, yo_ref)
    assert _same_bits(tg_s.view(3, B, K), tgs_ref) and _same_bits(tg_o.view(3, B, K), tgo_ref)
    for m in range(3):
        one, tg1 = _ops_mixup(ops, xs[m].contiguous(), lab.view(3, B)[m].contiguous(), K, rngs[m], dev, **kw)
        assert torch.equal(own[m], one) and torch.equal(tg_o.view(3, B, K)[m], tg1), m


# ---- 2. the fused H = 48 step against the oracle -------------------------------------------------------------------------------------------
def _soft_step(dev, spec, flat_np, x, q=None, labels=None, fused_head=True, rng=None, **masks):
    """train_step with targets= (or labels) -> logits, per-trial loss, grads, loss_sum"""
    return train_step(dev, spec, flat_np, x, labels=labels, targets=q, fused=fused_head, rng=rng, masks=masks)


@pytest.mark.parametrize("K", [3, 8])
@pytest.mark.parametrize("B,T", [(5, 9), (259, 5), (515, 5)])
def test_fused_h48_soft_step_vs_oracle(nsd, dev, B, T, K):
    """Through the product's dispatch: one trial per workgroup (B = 5), the two-trial forward (259), the four-trial kernels with a
    padding trial in the last group (515).  Explicit masks from the oracle's streams and the in-kernel streams: bitwise equal."""
    from nsd_amd import ops
    d, spec = orc.Dims(K=K), ops.ModelSpec(K=K)
    flat_np = orc.flatten_state(synth_params(8, 48, 2, K, seed=5 + K), d)
    x, q = synth_x(B, T, seed=3 * B + T), soft_targets(B, K, seed=B + K)
    seed, sid = 77 + B, 8
    masks = oracle_streams(seed, sid, B, T, 48, 32)
    a = _soft_step(dev, spec, flat_np, x, q, **masks)
    r = _soft_step(dev, spec, flat_np, x, q, rng=dict(seed=seed, base_stream=sid, p_lstm=0.6, p_head=0.6))
    for k in ("logits", "loss", "grads"):
        assert np.isfinite(a[k]).all() and np.array_equal(_bits(a[k]), _bits(r[k])), k
    ref = oracle_step(d, flat_np, x, targets=q, masks=masks)
    e_lg, e_loss = np.abs(a["logits"] - ref["logits"]).max(), abs(a["loss_sum"] / B - ref["loss"])
    print(f"soft step B={B} T={T} K={K}: logits {e_lg:.2e} loss {e_loss:.2e} per-trial loss {np.abs(a['loss'] - ref['loss_per_trial']).max():.2e}")
    assert e_lg < LOGIT_TOL and e_loss < LOSS_TOL
    assert a["loss"][1] == 0.0                                      # a zero row contributes nothing
    grad_close(a["grads"], ref["grads"], d, rtol=GRAD_RTOL_X4 if B >= 513 else GRAD_RTOL_12)


# ---- 3. one-hot targets reproduce the hard-label entry point -----------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(5, 9), (259, 5), (515, 5)])
def test_one_hot_targets_reproduce_the_hard_label_step(nsd, dev, ref_state, B, T):
    from nsd_amd import ops
    d, spec = orc.Dims(), ops.ModelSpec()
    flat_np = orc.flatten_state(ref_state, d)
    x, y = synth_x(B, T, seed=B + T), synth_labels(B, seed=B)
    rng = dict(seed=5, base_stream=12, p_lstm=0.6, p_head=0.6)
    hard = _soft_step(dev, spec, flat_np, x, labels=y, rng=rng)
    soft = _soft_step(dev, spec, flat_np, x, q=np.eye(3, dtype=np.float32)[y], rng=rng)
    assert np.array_equal(_bits(hard["logits"]), _bits(soft["logits"]))
    print(f"one-hot B={B}: per-trial loss differs by {np.abs(hard['loss'] - soft['loss']).max():.2e}")
    assert np.abs(hard["loss"] - soft["loss"]).max() <= 1e-6
    grad_close(soft["grads"], hard["grads"], d, rtol=GRAD_RTOL_X4 if B >= 513 else GRAD_RTOL_12)


# ---- 4. cancellation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused_head", [True, False])
def test_soft_dlogits_have_no_cancellation(nsd, dev, ref_state, fused_head):
    """B = 1, the dense head's last layer scaled until the winning class has 1 - p_y in [1e-7, 1e-5] (asserted from a float64 softmax
    of the returned logits).  d fc.3.bias = dlogits at B = 1: against float64 from those logits to 1e-4 relative, every class.  A
    cancellation-free fp32 evaluation errs by a few ulp times K (~1e-6); p_y - 1 formed by subtraction errs by 2^-24 / (1 - p_y) >= 0.6 %."""
    from nsd_amd import ops
    d, spec = orc.Dims(), ops.ModelSpec()
    st = {k: np.array(v) for k, v in ref_state.items()}
    x = synth_x(1, 9, seed=4)
    lg0 = _soft_step(dev, spec, orc.flatten_state(st, d), x, q=np.eye(3, dtype=np.float32)[[0]], fused_head=fused_head)["logits"][0].astype(np.float64)
    y = int(lg0.argmax())
    gap = lambda a: np.exp(a * (lg0 - lg0[y]))[np.arange(3) != y].sum()           # ~ 1 - p_y of the logits a * lg0
    lo, hi = 1.0, 1.0
    while gap(hi) > 1e-6:
        hi *= 2.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if gap(mid) > 1e-6 else (lo, mid)
    st["fc.3.weight"] = (st["fc.3.weight"] * np.float32(hi)).astype(np.float32)
    st["fc.3.bias"] = (st["fc.3.bias"] * np.float32(hi)).astype(np.float32)
    off = spec.offsets()["fc.3.bias"]
    for q in (np.eye(3, dtype=np.float32)[[y]], np.float32(2.5) * np.eye(3, dtype=np.float32)[[y]]):
        out = _soft_step(dev, spec, orc.flatten_state(st, d), x, q=q, fused_head=fused_head)
        lg = out["logits"].astype(np.float64)
        p = np.exp(lg - lg.max()) / np.exp(lg - lg.max()).sum()
        assert 1e-7 <= 1.0 - p[0, y] <= 1e-5, 1.0 - p[0, y]
        _, dl = mr.soft_ce(lg, q, 1.0)
        # (1 - p_y itself, formed in float64 without cancellation: the sum of the others)
        others = np.exp(lg[0] - lg[0, y])[np.arange(3) != y].sum()
        dl[0, y] = -q[0, y] * others / (1.0 + others)
        got = out["grads"][off:off + 3].astype(np.float64)
        rel = np.abs(got - dl[0]) / np.abs(dl[0])
        print(f"cancellation fused_head={fused_head} q_y={q[0, y]}: 1 - p_y = {1.0 - p[0, y]:.3e}, dlogits {got}, rel err {rel}")
        assert np.all(rel <= 1e-4), rel


# ---- 5. the unfused fallback ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,L,K", [(5, 40, 1, 3), (8, 32, 2, 3)])
def test_lstm_head_train_soft_outside_the_single_launch_shape(nsd, dev, C, H, L, K):
    """nsd_lstm_head_train_soft runs nsd_lstm_fwd + nsd_head_train_soft: the generic path (H = 40, L = 1, C = 5) and the first-generation
    H = 32 kernels, against the oracle."""
    from nsd_amd import ops
    B, T = 3, 4
    d, spec = orc.Dims(C=C, H=H, L=L, K=K), ops.ModelSpec(C=C, H=H, L=L, K=K)
    assert not ops.rng_path(spec, B, T)
    flat_np = orc.flatten_state(synth_params(C, H, L, K, seed=H), d)
    x, q = synth_x(B, T, C, seed=H), soft_targets(B, K, seed=H)
    masks = dict(rrelu_slope=orc.rrelu_noise(3, 1, (B, 32)), drop_head=orc.dropout_mask(3, 2, 0.6, (B, 32)))
    if L > 1:
        masks["drop_lstm"] = orc.dropout_mask(3, 0, 0.6, (L - 1, B, T, H))
    a = _soft_step(dev, spec, flat_np, x, q, **masks)
    ref = oracle_step(d, flat_np, x, targets=q, masks=masks)
    assert np.abs(a["logits"] - ref["logits"]).max() < LOGIT_TOL and abs(a["loss_sum"] / B - ref["loss"]) < LOSS_TOL
    assert a["loss"][1] == 0.0
    grad_close(a["grads"], ref["grads"], d, **FP32_EXACT)
    b = _soft_step(dev, spec, flat_np, x, q, fused_head=False, **masks)          # the two calls made by hand: the same launches
    for k in ("logits", "loss", "grads"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    with pytest.raises(nsd.NsdError, match="nsd_rng_path"):
        _soft_step(dev, spec, flat_np, x, q, rng=dict(seed=1, base_stream=4, p_lstm=0.6, p_head=0.6))


# ---- 6. several models ---------------------------------------------------------------------------------------------------------------------
def test_multi_train_fwd_soft_is_the_single_model_call_per_model(nsd, dev):
    from nsd_amd import ops
    M, B, T, K = 3, 5, 9, 3
    d, spec = orc.Dims(), ops.ModelSpec()
    P = spec.param_count
    params_np = np.stack([orc.flatten_state(synth_params(8, 48, 2, K, seed=40 + m), d) for m in range(M)])
    xs_np = synth_x(M * B, T, seed=6).reshape(M, B, T, 8)
    q_np = soft_targets(M * B, K, seed=8)
    rngs = [dict(seed=100 + m, base_stream=4 * (m + 1), p_lstm=0.6, p_head=0.6) for m in range(M)]
    params, xs, q = to_dev(params_np, dev), to_dev(xs_np, dev), to_dev(q_np, dev)
    ws = ops.multi_workspace(spec, M, B, T, dev)
    grads = torch.empty((M, P), device=dev)
    logits = ops.multi_train_step(spec, params, xs, None, ws, grads, rngs=rngs, fuse_adam=False, targets=q)
    losses = ops.multi_loss_sum(spec, ws, M, B, T).cpu().numpy()
    for m in range(M):
        one = _soft_step(dev, spec, params_np[m], xs_np[m], q_np[m * B:(m + 1) * B], rng=rngs[m])
        assert np.array_equal(_bits(logits.view(M, B, K)[m].cpu().numpy()), _bits(one["logits"])), m
        assert np.array_equal(_bits(grads[m].cpu().numpy()), _bits(one["grads"])), m
        assert np.float32(losses[m]) == np.float32(one["loss_sum"]), m
    # and against the oracle, model 1
    ref = oracle_step(d, params_np[1], xs_np[1], targets=q_np[B:2 * B], masks=oracle_streams(101, 8, B, T, 48, 32))
    assert np.abs(logits.view(M, B, K)[1].cpu().numpy() - ref["logits"]).max() < LOGIT_TOL and abs(losses[1] / B - ref["loss"]) < LOSS_TOL
    grad_close(grads[1].cpu().numpy(), ref["grads"], d, rtol=GRAD_RTOL_12)


# ---- 7. the bf16 sequence path ---------------------------------------------------------------------------------------------------------------
# Of each tensor's largest element.  The project's clean bound for this path is 2.6e-3 (tests/test_gpu_seqpath_bf16ref.py's
# REF_GRAD_RTOL_CLEAN, against an emulation); here both sides run the SAME kernels on the same saved activations and differ only in how
# dlogits reach the dense backward (fp32 in the kernel against float64 rounded to fp32), and the measured worst tensor on the MI355X is
# 6.24e-7 (attn.weight; profiles/r07_soft_targets.md).  Held to about 3 x measured: 2e-6.
SEQ_SOFT_GRAD_RTOL = 2e-6


def test_seq_train_fwd_soft_vs_the_any_loss_sequence(nsd, dev):
    from nsd_amd import ops
    B, T, K = 37, 5, 5
    spec, d = ops.ModelSpec(C=8, H=64, L=2, K=K), orc.Dims(C=8, H=64, L=2, K=K)
    flat = to_dev(orc.flatten_state(synth_params(8, 64, 2, K, seed=1), d), dev)
    x, y = to_dev(synth_x(B, T, seed=2), dev), to_dev(synth_labels(B, K, seed=2), dev)
    q_np = soft_targets(B, K, seed=3)
    q = to_dev(q_np, dev)
    rng = dict(seed=11, base_stream=8, p_lstm=0.6, p_head=0.6)
    ws = ops.seq_workspace(spec, B, T, dev)
    lg_hard = ops.seq_train_fwd(spec, flat, x, y, ws, rng=rng).clone()
    lg_soft = ops.seq_train_fwd(spec, flat, x, None, ws, rng=rng, targets=q).clone()
    g_soft = ops.seq_train_bwd(spec, flat, ws, B, T, rng=rng).clone()
    loss = float(ops.seq_loss_sum(spec, ws, B, T).item()) / B
    assert ops.seq_status(ws) == 0 and torch.equal(lg_hard, lg_soft)
    # the any-loss sequence on the same workspace
    lg = ops.seq_train_fwd_logits(spec, flat, x, ws, rng=rng)
    assert torch.equal(lg, lg_soft)
    loss_ref, dl = mr.soft_ce(lg.cpu().numpy(), q_np, 1.0 / B)
    ops.seq_head_bwd(spec, flat, ws, to_dev(dl.astype(np.float32), dev), B, T, rng=rng)
    g_any = ops.seq_train_bwd(spec, flat, ws, B, T, rng=rng)
    print(f"bf16 soft loss {loss:.6f} vs float64 {loss_ref.sum() / B:.6f}")
    assert abs(loss - loss_ref.sum() / B) < LOSS_TOL
    offs, shapes = spec.offsets(), spec.shapes()
    worst = 0.0
    for name, o in offs.items():
        n = int(np.prod(shapes[name]))
        a, b = g_soft[o:o + n], g_any[o:o + n]
        if name == "attn.bias":                                     # analytically zero (the softmax over time does not see it): held as
            assert abs(float(a[0])) < 1e-4 and abs(float(b[0])) < 1e-4          # tests/test_gpu_seqpath_bf16ref.py holds it, absolutely
            continue
        scale = max(float(b.abs().max()), 1e-6)
        err = float((a - b).abs().max()) / scale
        print(f"  {name}: {err:.3e}")
        worst = max(worst, err)
        assert err <= SEQ_SOFT_GRAD_RTOL, (name, err)
    print(f"bf16 soft vs any-loss gradients: worst tensor {worst:.3e} of its largest element (bound {SEQ_SOFT_GRAD_RTOL})")
    assert float(g_soft.abs().max()) > 0


# ---- 8. the trainers ---------------------------------------------------------------------------------------------------------------------
W3 = (0.5, 1.75, 1.0)


def _model(nsd, dev, seed, *a, **kw):
    torch.manual_seed(seed)
    return nsd.EEG_LSTM(*a, **kw).to(dev).train()


def _batch(dev, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return (2.7 * torch.randn((B, T, 8), generator=g)).to(dev), torch.randint(0, 3, (B,), generator=g, dtype=torch.int32).to(dev)


def _ref_mix(x: torch.Tensor, y: torch.Tensor, loss, seed, step, dev):
    xm, tg = mr.mixup(x.cpu().numpy(), y.cpu().numpy(), 3, seed, 4 * step, mix=loss.mixup, eps=loss.label_smoothing, weights=loss.class_weights)
    return to_dev(xm, dev), to_dev(tg, dev)


@pytest.mark.parametrize("case", ["fp32", "fp32_normalize_augment", "bf16_h64"])
def test_trainer_step_with_loss_equals_the_step_on_reference_windows_and_targets(nsd, dev, case):
    """Trainer(loss=L).step(x, y) leaves bitwise the parameters, Adam moments and loss of a trainer without loss= stepping on
    (mixup_ref's windows, mixup_ref's targets as float y) -- the windows being what the model would otherwise see: after nsd_augment
    and its fused z-score in the second case (the order augment -> mixup)."""
    from nsd_amd import ops
    from nsd_amd.trainer import Trainer
    bf16 = case.startswith("bf16")
    args = (8, 64, 2, 3, 0.6) if bf16 else ()
    kw = dict(precision="bf16") if bf16 else {}
    aug = case.endswith("augment")
    A = nsd.Augment(max_shift=5, scale_range=0.15, p_channel=0.2, noise_std=0.4) if aug else None
    Ls = nsd.Loss(label_smoothing=0.1, class_weights=W3, mixup=0.8)
    ma, mb = _model(nsd, dev, 11, *args, normalize=aug, **kw), _model(nsd, dev, 11, *args, **kw)
    ta, tb = Trainer(ma, lr=1e-3, seed=9, augment=A, loss=Ls), Trainer(mb, lr=1e-3, seed=9)
    assert ta.loss == Ls and tb.loss is None and ta.seed == tb.seed
    for step in range(1, 4):
        x, y = _batch(dev, 32, 40, seed=step)
        ta.step(x, y)
        seen = ops.augment(x, A, dict(seed=tb.seed, base_stream=4 * step), zscore=True) if aug else x
        xm, tg = _ref_mix(seen, y, Ls, tb.seed, step, dev)
        tb.step(xm, tg)
        assert torch.equal(ta.flat, tb.flat) and torch.equal(ta.m, tb.m) and torch.equal(ta.v, tb.v), step
        assert ta.last_loss() == tb.last_loss(), step
    assert not torch.equal(ta.flat, _model(nsd, dev, 11, *args, **kw).flat_parameters())
    with pytest.raises(nsd.NsdError, match="float targets together with loss="):
        ta.step(x, tg)
    # like the augmentation, the mixing belongs to the stochastic parts: a deterministic trainer mixes nothing, smoothing / weights stay
    assert Trainer(mb, loss=nsd.Loss(mixup=0.5), stochastic=False).loss is None
    assert Trainer(mb, loss=nsd.Loss(mixup=0.5, label_smoothing=0.1), stochastic=False).loss == nsd.Loss(label_smoothing=0.1)
    with pytest.raises(ValueError, match="class_weights"):
        Trainer(mb, loss=nsd.Loss(class_weights=(1.0, 2.0)))


@pytest.mark.parametrize("shared", [False, True])
def test_model_batch_trainer_with_loss_equals_separate_trainers(nsd, dev, shared):
    from nsd_amd.trainer import Trainer
    M, B, T = 3, 32, 40
    A = nsd.Augment(max_shift=5, noise_std=0.4)
    Ls = nsd.Loss(label_smoothing=0.1, class_weights=W3, mixup=1.0)
    seeds = [3, 4, 5]
    batched = [_model(nsd, dev, 100 + m) for m in range(M)]
    singles = [_model(nsd, dev, 100 + m) for m in range(M)]
    tr = nsd.ModelBatchTrainer(batched, lr=1e-3, seeds=seeds, augment=A, loss=Ls)
    trs = [Trainer(singles[m], lr=1e-3, seed=seeds[m], augment=A, loss=Ls) for m in range(M)]
    for step in range(1, 4):
        g = torch.Generator().manual_seed(step)
        xs = torch.randn((M, B, T, 8), generator=g).to(dev)
        ys = torch.randint(0, 3, (M, B), generator=g, dtype=torch.int32).to(dev)
        if shared:
            tr.step(xs[0].contiguous(), ys[0].contiguous())
        else:
            tr.step(xs, ys)
        losses = tr.last_losses()
        for m in range(M):
            k = 0 if shared else m
            trs[m].step(xs[k].contiguous(), ys[k].contiguous())
            assert torch.equal(tr.params[m], trs[m].flat) and torch.equal(tr.m[m], trs[m].m) and torch.equal(tr.v[m], trs[m].v), (step, m)
            assert losses[m] == trs[m].last_loss(), (step, m)


@pytest.mark.parametrize("mix", [0.0, 0.7])
def test_graph_replay_step_equals_eager_step_with_loss(nsd, dev, mix):
    """As tests/test_gpu_augment.py's replay test, with loss= on: the replayed graph draws the step's mixing from the device step
    counter.  The target rows and the mixed windows of every replay are bitwise the explicit-stream launch, the gradients are
    bit-identical; the parameters differ by the parent's device-pow() vs host-pow() Adam bias corrections only (its bound: 1e-6)."""
    from nsd_amd import ops
    from nsd_amd.trainer import Trainer
    B, T = 16, 30
    A = nsd.Augment(max_shift=4, noise_std=0.3)
    Ls = nsd.Loss(label_smoothing=0.1, class_weights=W3, mixup=mix)
    x, y = _batch(dev, B, T, seed=8)
    ma, mb = _model(nsd, dev, 21, normalize=True), _model(nsd, dev, 21, normalize=True)
    ta, tb = Trainer(ma, lr=1e-3, seed=5, augment=A, loss=Ls), Trainer(mb, lr=1e-3, seed=5, augment=A, loss=Ls)
    xs, ys = tb.static_inputs(B, T)
    xs.copy_(x); ys.copy_(y)
    for step in range(1, 4):
        ta.step(x, y)
        tb.step_static(B, T)
        seen = ops.augment(x, A, dict(seed=tb.seed, base_stream=4 * step), zscore=True)
        xm, tg = _ref_mix(seen, y, Ls, tb.seed, step, dev)
        buf = tb._buffers(B, T)
        assert torch.equal(buf["tg"], tg), step
        if mix:
            assert torch.equal(buf["xm"], xm), step
    assert tb.step_count == 3 and int(tb._step_dev.item()) == 3
    assert torch.equal(ta.grads, tb.grads)
    diff = (ma.flat_parameters() - mb.flat_parameters()).abs().max().item()
    print(f"graph replay with loss (mix={mix}): parameters differ by {diff:.2e}")
    assert diff < 1e-6 and abs(ta.last_loss() - tb.last_loss()) < 1e-6


def test_trainer_step_with_loss_matches_oracle(nsd, dev, ref_state):
    """One Trainer.step with smoothing + weights + mixup == oracle forward / backward with the step's counter-based masks on the
    restatement's mixed windows and targets, + oracle Adam: the bounds of test_trainer_step_matches_oracle_with_its_own_streams."""
    from nsd_amd.trainer import Trainer
    d = orc.Dims()
    m = model_from_state(nsd, dev, ref_state).train()
    Ls = nsd.Loss(label_smoothing=0.1, class_weights=W3, mixup=1.0)
    tr = Trainer(m, lr=1e-3, seed=7, loss=Ls)
    B, T = 12, 40
    x, y = synth_x(B, T, seed=4), synth_labels(B, seed=4)
    flat0 = orc.flatten_state(ref_state, d)
    tr.step(to_dev(x, dev), to_dev(y, dev))
    xm, q = mr.mixup(x, y, 3, tr.seed, 4, mix=1.0, eps=0.1, weights=W3)
    masks = oracle_streams(tr.seed, 4, B, T, 48, 32)
    ref = oracle_step(d, flat0, xm, targets=q, masks=masks)
    assert abs(tr.last_loss() - ref["loss"]) < LOSS_TOL
    grad_close(tr.grads.cpu().numpy(), ref["grads"], d, **FAST48)
    p, mm, vv = flat0.copy(), np.zeros_like(flat0), np.zeros_like(flat0)
    orc.adam(p, tr.grads.cpu().numpy(), mm, vv, lr=1e-3, step=1)
    assert np.abs(m.flat_parameters().cpu().numpy() - p).max() < 2e-6


# ---- 9. the default path ---------------------------------------------------------------------------------------------------------------------
def _launches(trainer, x, y, steps=3):
    from nsd_amd import ops
    names = []

    @contextlib.contextmanager
    def hook(name):
        names.append(name)
        yield
    ops.set_launch_hook(hook)
    try:
        for _ in range(steps):
            trainer.step(x, y)
    finally:
        ops.set_launch_hook(None)
    return names


@pytest.mark.parametrize("normalize", [False, True])
def test_loss_off_is_the_parents_step(nsd, dev, normalize):
    """loss=None and a disabled Loss(): the launch sequence of a trainer built without the argument, name for name (three launches per
    step for this shape, + the z-score), and bitwise its parameters after three steps.  With loss= on: one nsd_mixup per step, in
    front of the step, whose forward is the `_soft` twin."""
    from nsd_amd.trainer import Trainer
    x, y = _batch(dev, 32, 40, seed=2)
    step3 = ["nsd_lstm_head_train_rng", "nsd_lstm_bwd_rng", "nsd_grad_reduce_adam"]

    def run(**kw):
        t = Trainer(_model(nsd, dev, 3, normalize=normalize), lr=1e-3, seed=4, **kw)
        return _launches(t, x, y), t.flat.clone()
    base, p_base = run()
    assert base == ((["nsd_zscore_fwd"] if normalize else []) + step3) * 3
    for kw in (dict(loss=None), dict(loss=nsd.Loss())):
        names, p = run(**kw)
        assert names == base and torch.equal(p, p_base), kw
    on, p_on = run(loss=nsd.Loss(label_smoothing=0.1))
    per_step = (["nsd_zscore_fwd"] if normalize else []) + ["nsd_mixup", "nsd_lstm_head_train_soft", "nsd_lstm_bwd_rng", "nsd_grad_reduce_adam"]
    assert on == per_step * 3 and not torch.equal(p_on, p_base)

    def run_multi(**kw):
        models = [_model(nsd, dev, 30 + m, normalize=normalize) for m in range(3)]
        t = nsd.ModelBatchTrainer(models, lr=1e-3, seeds=[1, 2, 3], **kw)
        return _launches(t, x, y), t.params.clone()
    mbase, mp = run_multi()
    for kw in (dict(loss=None), dict(loss=nsd.Loss())):
        names, p = run_multi(**kw)
        assert names == mbase and torch.equal(p, mp), kw
    mon, _ = run_multi(loss=nsd.Loss(mixup=0.5))
    assert mon.count("nsd_mixup") == 3 and mon.count("nsd_multi_train_fwd_soft") == 3 and len(mon) == len(mbase) + 3


def test_explicit_mask_step_equals_in_kernel_streams_with_augmentation_and_loss(nsd, dev):
    """Trainer.in_kernel_rng = False (explicit mask tensors, filled through ops.train_masks) against True, both with augmentation and
    loss= on, three steps: parameters, Adam moments, gradients and loss bitwise equal.  The kernels promise the identity
    (test_gpu_parity.py::test_in_kernel_random_streams_equal_explicit_masks); this holds the trainer's plumbing around them to it."""
    from nsd_amd.trainer import Trainer
    A = nsd.Augment(max_shift=3, scale_range=0.1, p_channel=0.2, noise_std=0.3)
    Ls = nsd.Loss(label_smoothing=0.1, mixup=0.5)
    ta, tb = (Trainer(_model(nsd, dev, 11), lr=1e-3, seed=9, augment=A, loss=Ls) for _ in range(2))
    tb.in_kernel_rng = False
    # model m of the model-batched trainer carries the seed of Trainer(model_m, seed=seeds[m]) on rank 0
    from nsd_amd.step_recipe import trainer_seed
    seeds = [3, 2**64 - 1]
    mbt = nsd.ModelBatchTrainer([_model(nsd, dev, 100 + m) for m in range(2)], seeds=seeds)
    assert mbt.seeds == [trainer_seed(s, 0) for s in seeds] == [Trainer(_model(nsd, dev, 1), seed=s).seed for s in seeds]
    for step in range(1, 4):
        x, y = _batch(dev, 32, 40, seed=step)
        names = [_launches(t, x, y, steps=1) for t in (ta, tb)]
        assert "nsd_train_masks" not in names[0] and names[1].count("nsd_train_masks") == 1, step
        assert [n for n in names[1] if n != "nsd_train_masks"][:2] == ["nsd_augment", "nsd_mixup"] == names[0][:2], step
        for a, b in ((ta.flat, tb.flat), (ta.m, tb.m), (ta.v, tb.v), (ta.grads, tb.grads)):
            assert torch.equal(a, b), step
        assert ta.last_loss() == tb.last_loss(), step
    assert not torch.equal(ta.flat, _model(nsd, dev, 11).flat_parameters())
