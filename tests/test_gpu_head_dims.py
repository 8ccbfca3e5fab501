"""Every path of the library at head widths F (fc.0) and class counts K other than the reference's 32 and 3, against the CPU oracle
(tests/test_head_dims_cpu.py pins it to a float64 restatement of the model at these shapes) and, for the bf16 sequence path, the
float64 emulation of oracle/seq_bf16_ref.py.  Needs a real MI355X: run with `pytest -m gpu -s` (every comparison prints its errors,
the last test of the file the worst of them per class).

Inputs come from the generators of tests/golden/make_goldens.py with the seeds of head_inputs (tests/gpu_harness.py).  Every
comparison of gradients against the oracle first asserts that the ORACLE's fc.0 pre-activations stay 1e-4 away from the RReLU kink
(100x the fp32 forward error measured on them), so that a slope flip is a property of the kernel and never of the data.  Batches of
hundreds of trials, where no seed keeps tens of thousands of pre-activations that far away, take fc.0.bias = +-4 (kink_safe).

Bounds are the suite's own (tests/gpu_harness.py), with the worst value measured on one MI355X over this whole file (its last
test prints them) beside each:
  logits, train forward        1e-4 (LOGIT_TOL)                       measured 3.8e-6
  logits / probs, inference    1e-4 / 1e-5                            measured 1.4e-6 / 2.4e-7
  mean loss                    5e-5                                   measured 3.8e-7
  gradients, H = 48 fast path  FAST48: LSTM weights 5e-5, others 2e-5 of each tensor's largest element (+1e-7)
                                                                      measured 5.1e-6 / 2.1e-6 (10x / 9x room: FAST48, first measured at
                                                                      F = 32, K = 3, holds at every head size here)
  gradients, other routes      FP32_EXACT: LSTM weights 1e-5, others 2e-5 of each tensor's largest element (+1e-7)
                                                                      measured 5.9e-7 / 2.4e-6 (exact fp32; the bounds are derived in
                                                                      tests/test_gpu_fp32_routes.py)
  attn.bias gradient           2e-6 absolute                          measured 3.7e-9
  dx                           2e-5 (DX_TOL)                          measured 6.1e-7
  model-batched vs single run  3e-4 (MULTI_RTOL; the same arithmetic twice) measured 1.1e-5
  Adam, seven steps            1e-6 absolute                          measured 3.0e-7 vs float64, 1.2e-7 vs torch
  bf16 path vs its emulation   REF_* of tests/test_gpu_seqpath_bf16ref.py: clean 2.6e-3, streams 4e-3, logits 2e-3; any-loss sequence
                               vs fused CE 3.5e-3 (EQUIV_RTOL)        measured 8.1e-4, 1.4e-3, 4.7e-4; 7.3e-4
  bitwise where the header promises bits (in-kernel streams, batch invariance, model isolation, fused reduce + Adam, accumulate).
K = 1: loss and gradients are exactly zero in the oracle, so |loss| < 1e-7 and every gradient entry <= 1e-7 absolute (measured 0).
Wall time of the file on the MI355X: 8 s (118 tests), the CPU oracle and emulations included.
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from oracle import nsd_oracle as orc
from tests.golden.make_goldens import synth_labels, synth_params, synth_x
from tests.gpu_harness import (BASE_SHAPES, FAST48, GRAD_RTOL_12, HEAD_SAVES, HEAD_TOL, KINK_MARGIN, LOGIT_TOL, MULTI_RTOL, NAN, PROB_TOL, assert_step_vs_oracle,  # noqa: F401
                               bounds_of, dev, forward_backward, grad_close, grad_errors, head_inputs, model_from_state, multi_problem, multi_single,
                               multi_step, nsd, oracle_step, spec_of, to_dev, train_step, worse)
from tests.seq_bf16_harness import EQUIV_RTOL, any_loss, case_inputs, check_case, compare, emulate, per_tensor, run_gpu

pytestmark = pytest.mark.gpu

WORST = {}                       # class of number -> worst value seen in this run (printed by the last test)
T_START = time.time()


def _note(key, value):
    WORST[key] = worse(WORST.get(key, 0.0), float(value))


def _oracle(d, flat, x, y, masks, want_dx=False):
    """the oracle's step; asserts the kink margin on ITS pre-activations first"""
    return oracle_step(d, flat, x, labels=y, masks=masks, want_dx=want_dx, kink=KINK_MARGIN)


def _vs_oracle(tag, d, out, ref):
    """logits, mean loss, every gradient tensor (and dx, where both have one) of a train evaluation against _oracle's, at the
    bounds of the shape's route (bounds_of); the errors go into the table the last test prints"""
    if d.K > 1 and np.isfinite(out["grads"]).all():
        fast48 = bounds_of(d) is FAST48
        worst = grad_errors(out["grads"], ref["grads"], d)[1]
        _note("grad attn.bias (abs)", worst.pop("attn.bias"))
        for cls, v in worst.items():
            _note(f"grad {cls} / max ({'H = 48 fast path' if fast48 else 'other routes'})", v)
    errs = assert_step_vs_oracle(out, ref, d, bounds_of(d), tag=tag)
    _note("logits (abs)", errs["logits"])
    _note("K=1 |loss|" if d.K == 1 else "loss (abs)", errs["loss"])
    for k, name in (("k1_grad", "K=1 max |grad|"), ("dx", "dx / max")):
        if k in errs:
            _note(name, errs[k])
    return errs


def _step(dev, d, flat_np, x, y, fused_head=True, want_dx=False, rng=None, **masks):
    return train_step(dev, spec_of(d), flat_np, x, labels=y, fused=fused_head, want_dx=want_dx, rng=rng, masks=masks, saves=HEAD_SAVES)


def _same_step(a, b, d):
    """two launch sequences of one step: the bounds of test_single_launch_lstm_plus_head_train between its fused and unfused head"""
    for k in ("logits", "alpha", "pooled", "fc0_pre", "loss"):
        assert np.isfinite(a[k]).all() and np.isfinite(b[k]).all(), k
        assert np.abs(a[k] - b[k]).max() <= 2e-5 * max(1.0, np.abs(b[k]).max()), k
    for k in ("dscore", "dpooled"):
        assert np.abs(a[k] - b[k]).max() <= 1e-4 * np.abs(b[k]).max() + 1e-9, k
    if d.K > 1:
        grad_close(a["grads"], b["grads"], d, rtol=GRAD_RTOL_12)
    else:
        assert np.abs(a["grads"]).max() <= 1e-7 and np.abs(b["grads"]).max() <= 1e-7


def _infer_vs_oracle(tag, dev, d, flat_np, x, batch_invariance=True):
    """ops.infer against the oracle's eval-mode forward: logits, argmax where the oracle's top-two gap is clear, probabilities, and a
    batch equal to its single-trial runs bit for bit"""
    from nsd_amd import ops
    spec, flat, xt = spec_of(d), to_dev(flat_np, dev), to_dev(x, dev)
    lg_t, pr_t = ops.infer(spec, flat, xt)
    lg, pr = lg_t.cpu().numpy(), pr_t.cpu().numpy()
    ref = orc.forward(flat_np, x, d)
    lerr, perr = float(np.abs(lg - ref["logits"]).max()), float(np.abs(pr - ref["probs"]).max())
    print(f"[{tag}] C={d.C} H={d.H} L={d.L} K={d.K} F={d.F} B={x.shape[0]}: infer logits {lerr:.2e}  probs {perr:.2e}")
    _note("infer logits (abs)", lerr)
    _note("infer probs (abs)", perr)
    assert np.isfinite(lg).all() and lerr < LOGIT_TOL, (tag, lerr)
    assert perr < PROB_TOL, (tag, perr)
    assert np.abs(pr.sum(1) - 1.0).max() < 1e-5
    if d.K > 1:
        srt = np.sort(ref["logits"], axis=1)
        clear = (srt[:, -1] - srt[:, -2]) > 2 * LOGIT_TOL
        assert np.array_equal(lg.argmax(1)[clear], ref["logits"].argmax(1)[clear]), tag
    if batch_invariance:
        for i in range(x.shape[0]):
            l1, p1 = ops.infer(spec, flat, xt[i:i + 1].contiguous())
            assert torch.equal(l1[0], lg_t[i]) and torch.equal(p1[0], pr_t[i]), (tag, i)


# ---------------------------------------------------------------------------------------------------------------------------------
# a. the product's fused step (nsd_lstm_head_train, one trial per workgroup) at other head sizes
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc,H,K,F,B,T", [s for s in BASE_SHAPES if s[1] == 48 and s[2] <= 8])
def test_fused_train_step_vs_oracle(nsd, dev, Cc, H, K, F, B, T):
    """ops.train_step_grads(fused_head=True) -- what Trainer.step and bench.py launch -- with explicit masks, without any, and the two
    launches it replaces (fused_head=False): each against the oracle, and all outputs of the head against each other"""
    from nsd_amd import ops
    d, flat, x, y, masks = head_inputs(Cc, H, K, F, B, T)
    assert ops.rng_path(spec_of(d), B, T)                    # the single-launch shape
    ref = _oracle(d, flat, x, y, masks)
    a = _step(dev, d, flat, x, y, True, **masks)
    b = _step(dev, d, flat, x, y, False, **masks)
    _vs_oracle("a fused masks", d, a, ref)
    _vs_oracle("a unfused masks", d, b, ref)
    _same_step(a, b, d)
    for k in ("alpha", "pooled", "fc0_pre"):
        assert np.abs(a[k] - ref["fw"][k]).max() < HEAD_TOL, k
    ref0 = _oracle(d, flat, x, y, {})
    e = _step(dev, d, flat, x, y, True)
    _vs_oracle("a fused eval", d, e, ref0)


# ---------------------------------------------------------------------------------------------------------------------------------
# b. the three batch bands of the H = 48 dispatch (one-, two-, four-trial kernels)
# ---------------------------------------------------------------------------------------------------------------------------------
BAND_SHAPES = [(256, 9), (257, 9), (513, 9), (1025, 5)]
BAND_HEADS = [(8, 64), (2, 63), (5, 1), (8, 33)]


@pytest.mark.parametrize("B,T", BAND_SHAPES)
@pytest.mark.parametrize("K,F", BAND_HEADS)
def test_batch_bands_of_the_dispatch_vs_oracle(nsd, dev, K, F, B, T):
    """up to 256 trials one per workgroup, 257 .. 512 the two-trial forward, from 513 the four-trial kernels: the fused and the unfused
    head with masks against the oracle (fc.0.bias = +-4: see the header)"""
    d, flat, x, y, masks = head_inputs(8, 48, K, F, B, T, safe=True)
    ref = _oracle(d, flat, x, y, masks)
    res = []
    for fused in (True, False):
        out = _step(dev, d, flat, x, y, fused, **masks)
        _vs_oracle(f"b B={B} T={T} fused={fused}", d, out, ref)
        res.append(out["grads"])
    assert np.abs(res[0] - res[1]).max() <= 2e-5 * np.abs(res[0]).max()


# ---------------------------------------------------------------------------------------------------------------------------------
# c. the K = 9 edge on H = 48: no single launch, no in-kernel streams
# ---------------------------------------------------------------------------------------------------------------------------------
def test_nine_classes_take_the_two_launch_fallback(nsd, dev):
    from nsd_amd import ops
    Cc, H, K, F, B, T = 8, 48, 9, 33, 5, 33
    d, flat, x, y, masks = head_inputs(Cc, H, K, F, B, T)
    spec = spec_of(d)
    assert not ops.rng_path(spec, B, T) and ops.rng_path(spec_of(orc.Dims(C=8, H=48, L=2, K=8, F=33)), B, T)
    ref = _oracle(d, flat, x, y, masks)
    a = _step(dev, d, flat, x, y, True, **masks)           # nsd_lstm_head_train: falls back to nsd_lstm_fwd + nsd_head_train
    b = _step(dev, d, flat, x, y, False, **masks)
    _vs_oracle("c K=9 lstm_head_train", d, a, ref)
    assert np.array_equal(a["logits"], b["logits"]) and np.array_equal(a["grads"], b["grads"])     # the same two launches
    # the in-kernel streams are refused before any launch: logits and workspace stay as they were
    flat_t, xt = to_dev(flat, dev), to_dev(x, dev)
    ws = ops.new_workspace(spec, B, T, dev)
    ws.fill_(NAN)
    logits, grads = torch.full((B, K), NAN, device=dev), torch.full_like(flat_t, NAN)
    with pytest.raises(nsd.NsdError, match=r"lstm_head_train_rng: shape outside the single-launch path .*K <= 8"):
        ops.train_step_grads(spec, flat_t, xt, ws, to_dev(y, dev), logits, grads, rng=dict(seed=3, base_stream=4, p_lstm=0.6, p_head=0.6))
    torch.cuda.synchronize()
    assert torch.isnan(logits).all() and torch.isnan(ws).all() and torch.isnan(grads).all()


@pytest.mark.parametrize("K", [9, 12])
def test_trainer_step_beyond_eight_classes_matches_oracle_with_its_own_streams(nsd, dev, K):
    """EEG_LSTM(num_classes=K > 8): Trainer.step finds nsd_rng_path == 0, fills explicit masks with nsd_train_masks and runs the
    two-launch forward; one step == the oracle's forward / backward with the same counter streams + the oracle's Adam"""
    from nsd_amd.trainer import Trainer
    d = orc.Dims(C=8, H=48, L=2, K=K, F=32)
    state = synth_params(8, 48, 2, K, F=32, seed=48 + 32 + K)
    m = model_from_state(nsd, dev, state).train()
    tr = Trainer(m, lr=1e-3, seed=7)
    B, T = 12, 40
    x, y = synth_x(B, T, seed=32), synth_labels(B, K=K, seed=K)
    flat0 = orc.flatten_state(state, d)
    tr.step(to_dev(x, dev), to_dev(y, dev))
    assert tr._bufs[(B, T)]["rng_ok"] is False
    masks = dict(drop_lstm=orc.dropout_mask(tr.seed, 4, 0.6, (1, B, T, 48)), rrelu_slope=orc.rrelu_noise(tr.seed, 5, (B, 32)),
                 drop_head=orc.dropout_mask(tr.seed, 6, 0.6, (B, 32)))
    ref = _oracle(d, flat0, x, y, masks)
    _vs_oracle(f"c trainer K={K}", d, dict(logits=tr._bufs[(B, T)]["logits"].cpu().numpy(), mean_loss=tr.last_loss(), grads=tr.grads.cpu().numpy()), ref)
    p, mm, vv = flat0.copy(), np.zeros_like(flat0), np.zeros_like(flat0)
    orc.adam(p, tr.grads.cpu().numpy(), mm, vv, lr=1e-3, step=1)
    assert np.abs(m.flat_parameters().cpu().numpy() - p).max() < 2e-6


# ---------------------------------------------------------------------------------------------------------------------------------
# d. the streams drawn inside the kernels (index b*F + f) equal explicit masks, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(12, 40), (300, 7), (600, 6)])
@pytest.mark.parametrize("K,F", [(5, 1), (8, 33), (2, 63), (8, 64)])
def test_in_kernel_streams_equal_explicit_masks_bitwise(nsd, dev, K, F, B, T):
    """ops.train_step_grads(rng=) == the same step with the three tensors of nsd_train_masks, in each band of the dispatch"""
    from nsd_amd import _lib, ops
    d, flat, x, y, _ = head_inputs(8, 48, K, F, B, T)
    seed, base, p = 0xC0FFEE + F, 8, 0.6
    dl, sl, dh = torch.empty((1, B, T, 48), device=dev), torch.empty((B, F), device=dev), torch.empty((B, F), device=dev)
    ops._call("nsd_train_masks", dev, seed, base, p, p, dl.numel(), dl.data_ptr(), sl.numel(), sl.data_ptr(), dh.data_ptr(), ops.STREAM)
    torch.cuda.synchronize()
    assert np.array_equal(sl.cpu().numpy(), orc.rrelu_noise(seed, base + 1, (B, F)))
    assert np.array_equal(dh.cpu().numpy(), orc.dropout_mask(seed, base + 2, p, (B, F)))
    a = _step(dev, d, flat, x, y, True, rng=dict(seed=seed, base_stream=base, p_lstm=p, p_head=p))
    b = _step(dev, d, flat, x, y, True, drop_lstm=dl.cpu().numpy(), rrelu_slope=sl.cpu().numpy(), drop_head=dh.cpu().numpy())
    for k in ("logits", "grads", "fc0_pre", "loss", "pooled", "dpooled"):
        assert np.isfinite(a[k]).all(), k
        assert np.array_equal(a[k], b[k]), k
    assert (dh.cpu().numpy() == 0).any() and (dh.cpu().numpy() != 0).any()      # the head's dropout is really on


# ---------------------------------------------------------------------------------------------------------------------------------
# e. inference: the H = 48 tail up to 64 classes / units, nsd_head.hip beyond
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,F", [(K, F) for K in (1, 9, 33, 64) for F in (1, 33, 64)] + [(65, 33), (9, 65), (65, 65)])
def test_inference_over_the_head_grid(nsd, dev, K, F):
    d = orc.Dims(C=8, H=48, L=2, K=K, F=F)
    flat = orc.flatten_state(synth_params(8, 48, 2, K, F=F, seed=48 + F + K), d)
    _infer_vs_oracle("e", dev, d, flat, synth_x(7, 33, seed=F))
    _infer_vs_oracle("e B=300", dev, d, flat, synth_x(300, 5, seed=F + 1), batch_invariance=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# f. the other fp32 routes
# ---------------------------------------------------------------------------------------------------------------------------------
# (C, H, L, K, F, B, T, kink_safe, route)
ROUTES = [(8, 32, 2, 5, 7, 6, 15, False, "fused H=32"), (8, 64, 2, 33, 48, 6, 15, False, "fused H=64"),
          (8, 48, 3, 2, 65, 5, 37, False, "generic L=3"), (3, 40, 1, 5, 7, 5, 37, False, "generic L=1"),
          (8, 128, 2, 33, 48, 20, 9, True, "batched H=128"), (8, 64, 2, 2, 65, 400, 3, True, "batched H=64")]


@pytest.mark.parametrize("Cc,H,L,K,F,B,T,safe,route", ROUTES, ids=[r[-1] for r in ROUTES])
def test_other_fp32_routes_vs_oracle(nsd, dev, Cc, H, L, K, F, B, T, safe, route):
    from nsd_amd import ops
    d, flat, x, y, masks = head_inputs(Cc, H, K, F, B, T, L=L, safe=safe)
    spec = spec_of(d)
    assert spec.fast_path() == (L == 2 and H in (32, 48, 64))      # (H = 64 leaves the fused kernels for the batched ones from 384 trials)
    ref = _oracle(d, flat, x, y, masks)
    loss, grads, logits = forward_backward(dev, flat, x, y, spec=spec, **masks)
    _vs_oracle("f " + route, d, dict(logits=logits, mean_loss=loss, grads=grads), ref)
    _infer_vs_oracle("f " + route, dev, d, flat, x, batch_invariance=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# g. the input gradient on H = 48
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(5, 33), (513, 9)])
@pytest.mark.parametrize("K,F", [(8, 64), (2, 7)])
def test_input_gradient_vs_oracle(nsd, dev, K, F, B, T):
    """dx after the fused head and after the two-launch forward against the oracle's; the parameter gradients of a backward call
    with dx are those of the call without it (to the 2e-5 the fused and the unfused step agree to: from 513 trials dx sends the
    backward to the one-trial kernel)"""
    d, flat, x, y, masks = head_inputs(8, 48, K, F, B, T, safe=B > 256)
    ref = _oracle(d, flat, x, y, masks, want_dx=True)
    for fused in (True, False):
        out = _step(dev, d, flat, x, y, fused, want_dx=True, **masks)
        plain = _step(dev, d, flat, x, y, fused, **masks)
        assert "dx" in _vs_oracle(f"g B={B} fused={fused}", d, out, ref)          # (dx held to DX_TOL there)
        print(f"dx B={B} T={T} K={K} F={F} fused={fused}: grads with dx == without: {np.array_equal(out['grads'], plain['grads'])}")
        assert np.abs(out["grads"] - plain["grads"]).max() <= 2e-5 * np.abs(plain["grads"]).max()
        assert np.array_equal(out["logits"], plain["logits"])


# ---------------------------------------------------------------------------------------------------------------------------------
# h. the model-batched path where the strides between models are no multiples of four floats
# ---------------------------------------------------------------------------------------------------------------------------------
# (K, F): P = 33753 (P % 4 = 1), 30156, 33312, and (4, 2): P = 30207 (P % 4 = 3); the head slabs' stride P - 29952 is 3801, 204, 3360, 255
MULTI_HEADS = [(8, 64), (5, 1), (2, 63), (4, 2)]


def _mspec(nsd, K, F):
    return nsd.ModelSpec(C=8, H=48, L=2, K=K, F=F)


def _multi_grad_ok(spec, got, ref, tag):
    offs, shapes = spec.offsets(), spec.shapes()
    for n, shp in shapes.items():
        n_el = int(np.prod(shp))
        a, b = got[offs[n]:offs[n] + n_el], ref[offs[n]:offs[n] + n_el]
        err = float((a - b).abs().max())
        if n == "attn.bias":
            _note("multi vs single: grad attn.bias (abs)", err)
            assert err < 2e-6, (tag, n, err)
            continue
        scale = max(float(b.abs().max()), 1e-6)
        _note("multi vs single: grad / max", err / scale)
        assert err <= MULTI_RTOL * scale + 1e-7, (tag, n, err, scale)


@pytest.mark.parametrize("M,B", [(3, 171), (17, 32)])
@pytest.mark.parametrize("K,F", MULTI_HEADS)
def test_models_equal_separate_runs_at_unaligned_strides(nsd, dev, K, F, M, B):
    spec = _mspec(nsd, K, F)
    assert (spec.param_count % 4, K, F) in ((1, 8, 64), (0, 5, 1), (0, 2, 63), (3, 4, 2))
    params, x, y, rngs = multi_problem(spec, M, B, 9, dev, seed=M * 1000 + B + F)
    lg, gr, ls = multi_step(nsd, spec, params, x, y, rngs, dev)
    assert torch.isfinite(lg).all() and torch.isfinite(gr).all()
    for m in range(M):
        l1, g1, s1 = multi_single(nsd, spec, params[m].clone(), x[m], y[m], rngs[m], dev)
        assert float((lg[m] - l1).abs().max()) <= 1e-6 * max(float(l1.abs().max()), 1.0), m
        _multi_grad_ok(spec, gr[m], g1, (K, F, m))
        assert abs(float(ls[m]) - s1) <= 1e-6 * max(1.0, abs(s1)), (m, float(ls[m]), s1)


@pytest.mark.parametrize("M,B", [(3, 32), (17, 32), (3, 171)])
@pytest.mark.parametrize("K,F", MULTI_HEADS[:3])
def test_models_are_isolated_at_unaligned_strides(nsd, dev, K, F, M, B):
    spec = _mspec(nsd, K, F)
    params, x, y, rngs = multi_problem(spec, M, B, 12, dev, seed=7 + F)
    lg, gr, _ = multi_step(nsd, spec, params, x, y, rngs, dev)
    p2, x2 = params.clone(), x.clone()
    p2[1] += 0.01
    x2[1] *= -1.5
    lg2, gr2, _ = multi_step(nsd, spec, p2, x2, y, rngs, dev)
    for m in range(M):
        if m == 1:
            assert not torch.equal(lg[m], lg2[m])
        else:
            assert torch.equal(lg[m], lg2[m]) and torch.equal(gr[m], gr2[m]), m


@pytest.mark.parametrize("M,B", [(3, 171), (17, 32)])
@pytest.mark.parametrize("K,F", MULTI_HEADS[:3])
def test_multi_infer_equals_infer_at_unaligned_strides(nsd, dev, K, F, M, B):
    from nsd_amd import ops
    spec = _mspec(nsd, K, F)
    params, x, _, _ = multi_problem(spec, M, B, 20, dev, seed=5 + F)
    lg, pr = ops.multi_infer(spec, params, x)
    lgs, prs = ops.multi_infer(spec, params, x[0].contiguous())
    for m in range(M):
        l1, p1 = ops.infer(spec, params[m].contiguous(), x[m].contiguous())
        assert torch.equal(lg[m], l1) and torch.equal(pr[m], p1), m
        l1, p1 = ops.infer(spec, params[m].contiguous(), x[0].contiguous())
        assert torch.equal(lgs[m], l1) and torch.equal(prs[m], p1), m


@pytest.mark.parametrize("K,F", MULTI_HEADS[:3])
def test_multi_fused_reduce_adam_equals_reduce_then_adam_at_unaligned_strides(nsd, dev, K, F):
    from nsd_amd import ops
    spec = _mspec(nsd, K, F)
    M, B, T = 3, 32, 20
    params, x, y, rngs = multi_problem(spec, M, B, T, dev, seed=3 + F)
    hyper = dict(step=3, lr=1e-3, weight_decay=1e-2, grad_scale=0.5)
    pa, ma, va = params.clone(), torch.rand_like(params) * 1e-3, torch.rand_like(params) * 1e-6
    pb, mb, vb = pa.clone(), ma.clone(), va.clone()
    ga, gb = torch.full_like(params, NAN), torch.full_like(params, NAN)
    ops.multi_train_step(spec, pa, x, y.view(-1), ops.multi_workspace(spec, M, B, T, dev), ga, rngs=rngs, fuse_adam=True, m=ma, v=va, **hyper)
    ops.multi_train_step(spec, pb, x, y.view(-1), ops.multi_workspace(spec, M, B, T, dev), gb, rngs=rngs, fuse_adam=False)
    ops.adam_step(pb.view(-1), gb.view(-1), mb.view(-1), vb.view(-1), **hyper)
    assert torch.isfinite(ga).all() and not torch.equal(pa, params)
    assert torch.equal(ga, gb) and torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb)


def _multi_oracle_problem(spec, M, B, T, seed):
    """multi_problem on the host, and model M-1's masks from its own streams"""
    params, x, y, rngs = multi_problem(spec, M, B, T, torch.device("cpu"), seed=seed)
    r, m = rngs[M - 1], M - 1
    masks = dict(drop_lstm=orc.dropout_mask(r["seed"], r["base_stream"], 0.6, (1, B, T, 48)),
                 rrelu_slope=orc.rrelu_noise(r["seed"], r["base_stream"] + 1, (B, spec.F)),
                 drop_head=orc.dropout_mask(r["seed"], r["base_stream"] + 2, 0.6, (B, spec.F)))
    return params, x, y, rngs, (params[m].numpy(), x[m].numpy(), y[m].numpy(), masks)


# (K, F, M, B, T, seed of multi_problem: the first from 250 on whose oracle margin from the RReLU kink exceeds 3e-4 -- 3.6e-4, 5.6e-4, 3.8e-2)
MULTI_ORACLE = [(8, 64, 3, 32, 20, 278), (2, 63, 17, 32, 9, 254), (4, 2, 3, 171, 9, 252)]


@pytest.mark.parametrize("K,F,M,B,T,seed", MULTI_ORACLE)
def test_last_model_of_a_batch_against_the_oracle(nsd, dev, K, F, M, B, T, seed):
    """model M-1 -- the one whose parameters, gradients and head slabs lie furthest from an aligned address -- against the oracle"""
    spec = _mspec(nsd, K, F)
    d = orc.Dims(C=8, H=48, L=2, K=K, F=F)
    params, x, y, rngs, (pm, xm, ym, masks) = _multi_oracle_problem(spec, M, B, T, seed)
    ref = _oracle(d, pm, xm, ym, masks)
    lg, gr, ls = multi_step(nsd, spec, params.to(dev), x.to(dev), y.to(dev), rngs, dev)
    _vs_oracle(f"h model {M - 1} of {M}", d, dict(logits=lg[M - 1].cpu().numpy(), mean_loss=float(ls[M - 1]), grads=gr[M - 1].cpu().numpy()), ref)


# ---------------------------------------------------------------------------------------------------------------------------------
# i. the gradient reduction and Adam
# ---------------------------------------------------------------------------------------------------------------------------------
def test_grad_reduce_accumulates_bitwise_at_an_odd_parameter_count(nsd, dev):
    from nsd_amd import ops
    d, flat, x, y, masks = head_inputs(8, 48, 8, 64, 37, 20)
    spec, B, T = spec_of(d), 37, 20
    assert spec.param_count == 33753
    ft, xt = to_dev(flat, dev), to_dev(x, dev)
    ws = ops.new_workspace(spec, B, T, dev)
    logits, g0 = torch.empty((B, 8), device=dev), torch.full_like(ft, NAN)
    ops.train_step_grads(spec, ft, xt, ws, to_dev(y, dev), logits, g0, **{k: to_dev(v, dev) for k, v in masks.items()})
    old = torch.from_numpy(np.random.RandomState(5).standard_normal(33753).astype(np.float32) * 1e-2).to(dev)
    acc = old.clone()
    dd = spec.dims(B, T)
    ops._call("nsd_grad_reduce", dev, C.byref(dd), ws.data_ptr(), ws.numel() * 4, acc.data_ptr(), 1, ops.STREAM)
    again = torch.full_like(ft, NAN)
    ops._call("nsd_grad_reduce", dev, C.byref(dd), ws.data_ptr(), ws.numel() * 4, again.data_ptr(), 0, ops.STREAM)
    torch.cuda.synchronize()
    assert torch.isfinite(g0).all() and g0.abs().max().item() > 0
    assert torch.equal(again, g0) and torch.equal(acc, old + g0)


def _adam64(p, g, m, v, step, lr, wd, gscale, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam (amsgrad off, L2 weight decay added to the gradient) restated in float64, in place"""
    g = np.asarray(g, np.float64) * gscale + wd * p
    m *= b1
    m += (1 - b1) * g
    v *= b2
    v += (1 - b2) * g * g
    p -= (lr / (1 - b1 ** step)) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** step) + eps)


@pytest.mark.parametrize("wd,gscale", [(0.0, 1.0), (1e-2, 1.0), (0.0, 0.5), (1e-2, 0.5)])
@pytest.mark.parametrize("n", [1, 3, 33753, 2 ** 20 + 1])
def test_adam_entry_points_match_a_float64_restatement_and_torch(nsd, dev, n, wd, gscale):
    """nsd_adam_step, nsd_adam_step_guarded (flag 0; flag 1 leaves p / m / v untouched) and nsd_adam_step_dev over seven steps against
    torch.optim.Adam restated in float64 and against torch itself, 1e-6 as test_adam_matches_oracle_and_torch.  Parameters are drawn
    from U(-1, 1): an fp32 parameter below 1 moves by at most half an ulp, 3e-8, per step by rounding, 2.1e-7 over seven steps, and
    the update itself (1e-3 at most) carries a relative 1e-6 at worst -- the bound leaves 4x room whatever the kernel's order."""
    from nsd_amd import ops
    rs = np.random.RandomState(n % 1000 + int(wd * 1e4) + int(gscale * 10))
    p0 = rs.uniform(-1, 1, n).astype(np.float32)
    lr = 1e-3
    names = ("plain", "guarded", "dev")
    P = {k: to_dev(p0.copy(), dev) for k in names}
    Mm = {k: torch.zeros(n, device=dev) for k in names}
    V = {k: torch.zeros(n, device=dev) for k in names}
    p64, m64, v64 = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    pt = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([pt], lr=lr, weight_decay=wd)
    flag0, flag1 = torch.zeros(1, device=dev), torch.ones(1, device=dev)
    step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    for step in range(1, 8):
        g = rs.standard_normal(n).astype(np.float32)
        gt = to_dev(g, dev)
        ops.adam_step(P["plain"], gt, Mm["plain"], V["plain"], step=step, lr=lr, weight_decay=wd, grad_scale=gscale)
        before = [t.clone() for t in (P["guarded"], Mm["guarded"], V["guarded"])]
        ops.adam_step(P["guarded"], gt, Mm["guarded"], V["guarded"], step=step, lr=lr, weight_decay=wd, grad_scale=gscale, skip=flag1)
        assert all(torch.equal(a, b) for a, b in zip(before, (P["guarded"], Mm["guarded"], V["guarded"])))     # flag raised: untouched
        ops.adam_step(P["guarded"], gt, Mm["guarded"], V["guarded"], step=step, lr=lr, weight_decay=wd, grad_scale=gscale, skip=flag0)
        step_dev.fill_(step)
        ops._call("nsd_adam_step_dev", dev, n, P["dev"].data_ptr(), gt.data_ptr(), Mm["dev"].data_ptr(), V["dev"].data_ptr(), lr, 0.9, 0.999,
                  1e-8, wd, gscale, step_dev.data_ptr(), ops.STREAM)
        _adam64(p64, g, m64, v64, step, lr, wd, gscale)
        pt.grad = torch.from_numpy(g * np.float32(gscale))
        opt.step()
    for k in names:
        got = P[k].cpu().numpy()
        e64, et = float(np.abs(got - p64).max()), float(np.abs(got - pt.detach().numpy()).max())
        print(f"adam {k} n={n} wd={wd} grad_scale={gscale}: vs float64 {e64:.2e}  vs torch {et:.2e}")
        _note("adam vs float64 (abs)", e64)
        _note("adam vs torch (abs)", et)
        assert e64 < 1e-6 and et < 1e-6, (k, e64, et)
        assert np.abs(Mm[k].cpu().numpy() - m64).max() < 1e-6 and np.abs(V[k].cpu().numpy() - v64).max() < 1e-6, k
    assert torch.equal(P["plain"], P["guarded"])
    assert n < 1000 or np.abs(p64 - p0).max() > 5e-3        # seven steps of about lr each: the parameters really moved


@pytest.mark.parametrize("wd,gscale", [(0.0, 1.0), (1e-2, 0.5)])
@pytest.mark.parametrize("K,F", [(8, 64), (2, 1)])
def test_fused_reduce_adam_matches_a_float64_restatement(nsd, dev, K, F, wd, gscale):
    """nsd_grad_reduce_adam at P = 33753 and P = 30150 (P % 4 = 1 and 2), seven train steps: the gradient it writes is nsd_grad_reduce's
    bit for bit, and p / m / v follow the float64 restatement of torch.optim.Adam fed with that gradient (1e-6; |parameters| < 1.5)"""
    from nsd_amd import ops
    B, T, lr = 16, 12, 1e-3
    d, flat, x, y, masks = head_inputs(8, 48, K, F, B, T)
    spec = spec_of(d)
    n = spec.param_count
    assert n == {64: 33753, 1: 30150}[F] and np.abs(flat).max() < 1.5
    p, xt, yt = to_dev(flat.copy(), dev), to_dev(x, dev), to_dev(y, dev)
    mk = {k: to_dev(v, dev) for k, v in masks.items()}
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    p64, m64, v64 = flat.astype(np.float64), np.zeros(n), np.zeros(n)
    ws = ops.new_workspace(spec, B, T, dev)
    logits = torch.empty((B, K), device=dev)
    dd = spec.dims(B, T)
    for step in range(1, 8):
        g0, g1 = torch.full_like(p, NAN), torch.full_like(p, NAN)
        ops.train_step_grads(spec, p, xt, ws, yt, logits, g0, **mk)                      # ... nsd_grad_reduce -> g0, slabs stay
        ops._call("nsd_grad_reduce_adam", dev, C.byref(dd), ws.data_ptr(), ws.numel() * 4, g1.data_ptr(), p.data_ptr(), m.data_ptr(),
                  v.data_ptr(), lr, 0.9, 0.999, 1e-8, wd, gscale, step, ops.STREAM)
        torch.cuda.synchronize()
        assert torch.isfinite(g0).all() and torch.equal(g0, g1), step
        _adam64(p64, g0.cpu().numpy(), m64, v64, step, lr, wd, gscale)
    e = float(np.abs(p.cpu().numpy() - p64).max())
    print(f"reduce+adam K={K} F={F} wd={wd} grad_scale={gscale}: p vs float64 {e:.2e}")
    _note("adam vs float64 (abs)", e)
    assert e < 1e-6
    assert np.abs(m.cpu().numpy() - m64).max() < 1e-6 and np.abs(v.cpu().numpy() - v64).max() < 1e-6
    assert np.abs(p64 - flat).max() > 5e-3


# ---------------------------------------------------------------------------------------------------------------------------------
# j. the bf16 sequence path (machinery and bounds of tests/test_gpu_seqpath_bf16ref.py, any-loss sequence of tests/test_gpu_seq_autograd.py)
# ---------------------------------------------------------------------------------------------------------------------------------
# name -> (C, H, L, K, D, B, T, p, route, bound kind, diag no-fused flag, F)
SEQ_CASES = {
    "fused_k64_f64":   (8, 64, 2, 64, 1, 40, 24, None, "fused2", "clean", False, 64),
    "general_k1_f1":   (8, 128, 2, 1, 1, 64, 20, None, "general", "clean", True, 1),
    "streams_k33_f17": (8, 256, 2, 33, 1, 96, 12, 0.4, "fused2", "streams", False, 17),
    "bidir_k9_f48":    (24, 128, 2, 9, 2, 64, 9, 0.5, "general", "streams", False, 48),
}


def _seq_spec(case):
    from nsd_amd import ops
    C_, H, L, K, D = case[:5]
    return ops.ModelSpec(C=C_, H=H, L=L, K=K, F=case[11], D=D)


@pytest.mark.parametrize("tag", [t for t in sorted(SEQ_CASES) if SEQ_CASES[t][3] > 1])
def test_seq_path_head_dims_match_bf16_emulation(nsd, dev, tag):
    """train forward / backward and inference against the emulation (REF_* bounds of the case's kind), then the any-loss sequence
    nsd_seq_train_fwd_logits -> nsd_seq_head_bwd -> nsd_seq_train_bwd_dx: the fused route's logits bit for bit, its gradients within
    EQUIV_RTOL, train_bwd_dx's gradients those of train_bwd bit for bit"""
    from nsd_amd import ops
    case = SEQ_CASES[tag]
    errs, out, ref = check_case(tag, case, dev)
    _note(f"bf16 {case[9]}: grad / max", max(v for k, v in errs.items() if k != "attn.bias"))
    _note("bf16 logits (abs)", np.abs(out["logits"] - ref["logits"]).max())
    spec = _seq_spec(case)
    flat, x, y, _, rng = case_inputs(case)
    B, T = case[5], case[6]
    ft, xt, yt = torch.from_numpy(flat).to(dev), torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    ws = out["ws"]
    lf = ops.seq_train_fwd(spec, ft, xt, yt, ws, rng=rng).clone()
    gf = ops.seq_train_bwd(spec, ft, ws, B, T, rng=rng).clone()
    ce = lambda lg: (torch.softmax(lg, 1) - torch.nn.functional.one_hot(yt.long(), spec.K).float()) / B      # noqa: E731
    la, _, ga, dx = any_loss(spec, ft, xt, ws, ce, rng)
    g_plain = ops.seq_train_bwd(spec, ft, ws, B, T, rng=rng)
    torch.cuda.synchronize()
    assert ops.seq_status(ws) == 0
    eq = per_tensor(spec, ga, gf)
    worst = max(eq.items(), key=lambda kv: kv[1])
    print(f"[{tag}] any-loss sequence vs fused CE: worst {worst[1]:.2e} ({worst[0]})  dx max {dx.abs().max().item():.2e}")
    _note("bf16 any-loss vs fused / max", worst[1])
    assert torch.equal(la, lf) and torch.equal(lf.cpu(), torch.from_numpy(out["logits"]))
    assert torch.equal(ga, g_plain)
    assert torch.isfinite(dx).all() and dx.abs().max().item() > 0
    assert worst[1] < EQUIV_RTOL, eq


def test_seq_path_one_class_one_unit(nsd, dev):
    """K = 1, F = 1 on the general route of a shape the product fuses (diagnostic library): train-forward logits and inference against
    the emulation; the loss and every gradient are exactly zero there, so |loss| < 1e-7 and gradients <= 1e-7 absolute"""
    from nsd_amd import _lib, ops
    case = SEQ_CASES["general_k1_f1"]
    flat, x, y, masks, rng = case_inputs(case)
    ref = emulate(case, flat, x, y, masks)
    assert abs(ref["loss"]) < 1e-12 and np.abs(ref["grads"]).max() < 1e-12
    with _lib.diagnostic_library():
        ops.set_seq_diag_flags(fused_layers=False)
        try:
            out = run_gpu(case, flat, x, y, rng, dev)
        finally:
            ops.set_seq_diag_flags()
    compare("general_k1_f1", case, out["logits"], None, ref)
    compare("general_k1_f1 infer", case, out["infer"], None, ref, got_probs=out["probs"])
    assert np.array_equal(out["probs"], np.ones_like(out["probs"]))
    _note("K=1 |loss|", abs(out["loss"]))
    _note("K=1 max |grad|", np.abs(out["grads"]).max())
    assert abs(out["loss"]) < 1e-7 and np.isfinite(out["grads"]).all() and np.abs(out["grads"]).max() <= 1e-7


@pytest.mark.parametrize("K,F", [(65, 64), (64, 65), (65, 65)])
def test_seq_path_refuses_heads_beyond_64(nsd, dev, K, F):
    from nsd_amd import ops
    ok, bad = ops.ModelSpec(H=128, K=64, F=64), ops.ModelSpec(H=128, K=K, F=F)
    assert ok.seq_path(32, 10) and not bad.seq_path(32, 10)
    with pytest.raises(nsd.NsdError, match=rf"rc=-1\): seq path: F={F} K={K} exceed 64"):
        ops.seq_workspace(bad, 32, 10, dev)
    ws = ops.seq_workspace(ok, 32, 10, dev)
    flat = torch.zeros(bad.param_count, device=dev)
    x, y = torch.zeros((32, 10, 8), device=dev), torch.zeros(32, dtype=torch.int32, device=dev)
    for call in (lambda: ops.seq_infer(bad, flat, x, ws), lambda: ops.seq_train_fwd(bad, flat, x, y, ws),
                 lambda: ops.seq_train_fwd_logits(bad, flat, x, ws), lambda: ops.seq_train_bwd(bad, flat, ws, 32, 10)):
        with pytest.raises(nsd.NsdError, match=rf"rc=-1\): seq path: F={F} K={K} exceed 64"):
            call()
    assert ops.seq_status(ws) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
def test_zz_worst_errors_of_this_file(nsd, dev):
    """prints the worst value of every class of number compared above (run the whole file with -s) and the file's wall time"""
    torch.cuda.synchronize()
    print("\nworst errors of tests/test_gpu_head_dims.py:")
    for k in sorted(WORST):
        print(f"  {k:44s} {WORST[k]:.2e}")
    print(f"  wall time since import: {time.time() - T_START:.0f} s")
