"""Session calibration on the MI355X (nsd_stream_features / nsd_head_fit of include/nsd.h, csrc/nsd_head_fit.hip) against the float64
restatement tests/head_fit_ref.py and against itself, bit for bit, wherever the header promises bits.  Needs the MI355X.

Bounds (none comes from the kernel):
  gradient   g = m / (1 - beta1) after one epoch from a zero state (no weight decay) against float64: every tensor within FP32_EXACT's
             rtol = 2e-5 of its largest element, the bound of the project's other exact-fp32 head gradients; fc.0's pre-activations
             of the REFERENCE stay KINK_MARGIN from zero for every trial (the feature seed is searched until they do)
  loss       loss_out (scale = 1/N: the mean loss) within LOSS_TOL of float64
  update     p, m, v within 1e-6 absolute of float64 after one epoch at lr 1e-3 on |p| <= 1: test_gpu_optim.py's bound (each step
             rounds p once, <= 6e-8)
  features   bit-equal to pool_acc / pool_den of the public slot layout; their numpy read-out within LOGIT_TOL of the stream's logits
  it learns  100 % accuracy and a final loss <= 1/100 of the first on three Gaussian clusters (float64 PyTorch reaches < 1e-6 from 1.1)
Every launch works on a few kilobytes; the whole file takes a few seconds."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from oracle import nsd_oracle as orc
from tests import head_fit_ref as hf
from tests.buffer_contract import guarded, snapshot
from tests.golden.make_goldens import synth_params, synth_x
from tests.gpu_harness import FP32_EXACT, KINK_MARGIN, LOGIT_TOL, LOSS_TOL, NAN, dev, nsd, soft_targets, sync_at_the_end, to_dev, write_pth  # noqa: F401

pytestmark = pytest.mark.gpu

H = 48
UPDATE_TOL = 1e-6
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------------
def _spec(F=32, K=3):
    from nsd_amd import ops
    return ops.ModelSpec(C=8, H=H, L=2, K=K, F=F)


def _flat(F, K, seed):
    d = orc.Dims(C=8, H=H, L=2, K=K, F=F)
    return orc.flatten_state(synth_params(8, H, 2, K, F=F, seed=seed), d)


def _tail(spec, flat):
    """the trainable tail of a flat parameter vector, in the state's order (float64)"""
    offs, shapes = spec.offsets(), spec.shapes()
    return np.concatenate([np.asarray(flat[offs[k]:offs[k] + int(np.prod(shapes[k]))], dtype=np.float64) for k in hf.TAIL])


def _theta(spec, flat):
    return hf.tail_dict(_tail(spec, flat), H, spec.F, spec.K)


def _tail_mask(spec):
    """boolean [P]: the flat positions of the trainable tail"""
    offs, shapes = spec.offsets(), spec.shapes()
    mask = np.zeros(spec.param_count, bool)
    for k in hf.TAIL:
        mask[offs[k]:offs[k] + int(np.prod(shapes[k]))] = True
    return mask


def _group_mask(spec, train):
    offs, shapes = spec.offsets(), spec.shapes()
    mask = np.zeros(spec.param_count, bool)
    for g in train:
        for k in hf.GROUPS[g]:
            mask[offs[k]:offs[k] + int(np.prod(shapes[k]))] = True
    return mask


def _feats(N, seed):
    rs = np.random.RandomState(seed)
    return (rs.standard_normal((N, H)) * (0.5 + rs.rand(N, 1))).astype(np.float32)


def _kink_free_feats(spec, flat, N, seed0):
    """features whose fc.0 pre-activations, in the float64 reference, all stay KINK_MARGIN from zero: the first seed that does it"""
    theta = _theta(spec, flat)
    q = np.ones((N, spec.K))
    for seed in range(seed0, seed0 + 200):
        x = _feats(N, seed)
        pre = hf.epoch(theta, x, q, 1.0)[2]
        if float(np.abs(pre).min()) >= KINK_MARGIN:
            return x
    raise AssertionError("no feature seed keeps the reference away from the RReLU kink")


def _fields(spec, state_np):
    """state [M, stride] (numpy float32) -> m [M,Pt], v [M,Pt], epochs [M] int64, status [M] int32"""
    from nsd_amd import ops
    lay, pt = ops.head_fit_layout(spec), hf.tail_count(H, spec.F, spec.K)
    raw = np.ascontiguousarray(state_np)
    return dict(m=raw[:, int(lay.m):int(lay.m) + pt], v=raw[:, int(lay.v):int(lay.v) + pt],
                epochs=np.ascontiguousarray(raw[:, int(lay.epochs):int(lay.epochs) + 2]).view(np.int64)[:, 0],
                status=raw.view(np.int32)[:, int(lay.status)])


def _make_state(spec, M, m=None, v=None, count=0):
    from nsd_amd import ops
    lay, pt = ops.head_fit_layout(spec), hf.tail_count(H, spec.F, spec.K)
    st = np.zeros((M, int(lay.stride)), np.float32)
    if m is not None:
        st[:, int(lay.m):int(lay.m) + pt], st[:, int(lay.v):int(lay.v) + pt] = m, v
    st[:, int(lay.epochs):int(lay.epochs) + 2] = np.array([count], np.int64).view(np.float32)
    return st


def _fit(dev, spec, params, feats, targets, epochs, *, state=None, rngs=None, train=("ln", "fc0", "fc3"), scale=None, **hyper):
    """one nsd_head_fit launch on copies of the inputs, loss_out NaN-filled -> numpy params [M,P], state [M,stride], loss [M,E]"""
    from nsd_amd import ops
    p = to_dev(np.atleast_2d(params).astype(np.float32), dev)
    M = int(p.shape[0])
    st = ops.head_fit_state(spec, M, dev) if state is None else to_dev(state, dev)
    loss = torch.full((M, epochs), NAN, device=dev)
    kw = dict(HYPER)
    kw.update(hyper)
    out = ops.head_fit(spec, p, to_dev(feats, dev), to_dev(np.asarray(targets, np.float32), dev), st, epochs=epochs, rngs=rngs, train=train,
                       scale=scale, loss_out=loss, **kw)
    assert out is loss
    return p.cpu().numpy(), st.cpu().numpy(), loss.cpu().numpy()


def _rng(seed, base=0, p=0.3):
    return dict(seed=seed, base_stream=base, p_lstm=0.0, p_head=p)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. features
# ---------------------------------------------------------------------------------------------------------------------------------
def _numpy_readout(spec, flat, feats):
    """float64 eval-mode read-out of pooled vectors: the logits of lstm_eeg_model.py:38-39"""
    q = np.zeros((feats.shape[0], spec.K))
    return hf.epoch(_theta(spec, flat), feats, q, 1.0)[3]


def test_features_are_the_pooled_vector_of_the_slots(nsd, dev):
    from nsd_amd import ops
    spec = _spec()
    flat = to_dev(_flat(32, 3, seed=11), dev)
    S, T = 3, 17
    x = to_dev(synth_x(2, T, seed=5), dev)
    lay = ops.stream_layout(spec)
    state = torch.full((S, int(lay.stride)), NAN, device=dev)
    ops.stream_reset(spec, state)
    slots = torch.tensor([2, 0], dtype=torch.int32, device=dev)          # slot 1 is never stepped
    logits, _ = ops.stream_step(spec, flat, x, state, slots=slots)
    before = snapshot(state)
    ask = torch.tensor([0, 2, 1, 3, -1], dtype=torch.int32, device=dev)  # permuted, a never-stepped slot, two out-of-range ones
    feats, check = guarded((5, H), torch.float32, dev, "nan32")
    out = ops.stream_features(spec, state, slots=ask, out=feats)
    assert out is feats
    check("feats")
    assert before.unchanged()
    st, f = state.cpu().numpy(), feats.cpu().numpy()
    acc, den = st[:, int(lay.pool_acc):int(lay.pool_acc) + H], st[:, int(lay.pool_den)]
    for row, slot in ((0, 0), (1, 2)):
        assert _same_bits(f[row], (acc[slot] / den[slot]).astype(np.float32)), slot          # one correctly rounded fp32 division
    assert np.isnan(f[2:]).all() and den[1] == 0.0
    lg = logits.cpu().numpy()                                             # stream b of the step lives in slot slots[b]
    err = max(float(np.abs(_numpy_readout(spec, flat.cpu().numpy(), f[1:2])[0] - lg[0]).max()),
              float(np.abs(_numpy_readout(spec, flat.cpu().numpy(), f[0:1])[0] - lg[1]).max()))
    print(f"features: numpy read-out of the rows against the stream's logits {err:.2e}")
    assert err < LOGIT_TOL
    # slots == NULL: rows 0 .. n-1
    every = ops.stream_features(spec, state).cpu().numpy()
    assert _same_bits(every[0], f[0]) and _same_bits(every[2], f[1]) and np.isnan(every[1]).all()


def test_features_read_an_ensemble_state_as_flat_slots(nsd, dev):
    from nsd_amd import ops
    spec = _spec()
    M, S, T = 2, 3, 9
    params = to_dev(np.stack([_flat(32, 3, seed=21 + m) for m in range(M)]), dev)
    state = ops.multi_stream_state(spec, M, S, dev)
    x = to_dev(synth_x(S, T, seed=9), dev)
    ops.multi_stream_step(spec, params, x, state)
    lay = ops.stream_layout(spec)
    f = ops.stream_features(spec, state).cpu().numpy().reshape(M, S, H)
    st = state.cpu().numpy()
    ref = (st[..., int(lay.pool_acc):int(lay.pool_acc) + H] / st[..., int(lay.pool_den):int(lay.pool_den) + 1]).astype(np.float32)
    assert _same_bits(f, ref)
    for m in range(M):                                                    # a model's part is an ordinary state
        assert _same_bits(ops.stream_features(spec, state[m]).cpu().numpy(), ref[m])
    assert not _same_bits(ref[0], ref[1])


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. gradient and loss of one epoch against float64
# ---------------------------------------------------------------------------------------------------------------------------------
GRAD_CASES = [(N, 32, 3) for N in (1, 2, 3, 4, 5, 63, 64, 65, 255, 256)] + [(N, F, K) for F, K in ((64, 8), (33, 9), (1, 64)) for N in (5, 64)]


@pytest.mark.parametrize("N,F,K", GRAD_CASES)
def test_gradient_and_loss_of_one_epoch_against_float64(nsd, dev, N, F, K):
    from nsd_amd import ops
    spec = _spec(F, K)
    assert ops.head_fit_path(spec, 1, N)
    flat = _flat(F, K, seed=F + K)
    feats = _kink_free_feats(spec, flat, N, seed0=1000 * N + F)
    q = soft_targets(N, K, seed=N + K)
    b1 = float(np.float32(HYPER["beta1"]))
    for rng in (None, _rng(seed=77 + N, base=12)):
        ref = hf.HeadFitRef(_theta(spec, flat), H, F, K, rng=rng, **HYPER)
        ref_loss = ref.fit(feats, q, 1.0 / N, 1)
        assert ref.min_pre >= KINK_MARGIN
        _, st, loss = _fit(dev, spec, flat, feats, q, 1, rngs=None if rng is None else [rng])
        fld = _fields(spec, st)
        assert fld["epochs"][0] == 1 and fld["status"][0] == 0
        g = hf.tail_dict(fld["m"][0].astype(np.float64) / (1.0 - b1), H, F, K)
        g_ref = hf.tail_dict(ref.last_grad, H, F, K)
        worst = {k: float(np.abs(g[k] - g_ref[k]).max()) / float(np.abs(g_ref[k]).max()) for k in hf.TAIL}
        e_loss = abs(float(loss[0, 0]) - float(ref_loss[0]))
        print(f"head_fit N={N} F={F} K={K} rng={'on' if rng else 'off'}: loss {e_loss:.2e}  grad error / largest element",
              {k: f"{v:.2e}" for k, v in worst.items()})
        assert e_loss < LOSS_TOL
        for k in hf.TAIL:
            assert worst[k] <= FP32_EXACT["rtol"], (k, worst[k])


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the update
# ---------------------------------------------------------------------------------------------------------------------------------
def test_one_update_from_a_run_in_progress_against_float64(nsd, dev):
    spec = _spec()
    N, F, K = 12, 32, 3
    rs = np.random.RandomState(3)
    flat = _flat(F, K, seed=8)
    tail = _tail_mask(spec)
    flat[tail] = rs.uniform(-0.3, 0.3, int(tail.sum())).astype(np.float32)            # |p| <= 1
    pt = hf.tail_count(H, F, K)
    m0, v0 = (1e-3 * rs.standard_normal(pt)).astype(np.float32), (1e-6 * rs.random_sample(pt)).astype(np.float32)
    feats, q = _feats(N, 31), (np.eye(K)[rs.randint(0, K, N)] * 0.9 + 0.1 / K).astype(np.float32)      # smoothed one-hot rows
    kw = dict(HYPER, weight_decay=1e-2)
    ref = hf.HeadFitRef(_theta(spec, flat), H, F, K, count=6, m=m0, v=v0, **kw)
    ref.fit(feats, q, 1.0 / N, 1)
    p, st, _ = _fit(dev, spec, flat, feats, q, 1, state=_make_state(spec, 1, m0, v0, count=6), **kw)
    fld = _fields(spec, st)
    assert fld["epochs"][0] == 7 and fld["status"][0] == 0
    rm, rv = ref.moments()
    errs = dict(p=float(np.abs(_tail(spec, p[0]) - ref.vec).max()), m=float(np.abs(fld["m"][0] - rm).max()), v=float(np.abs(fld["v"][0] - rv).max()))
    moved = float(np.abs(_tail(spec, p[0]) - _tail(spec, flat)).max())
    print(f"head_fit update at epoch 7: errors {errs}, largest step {moved:.2e}")
    assert moved > 1e-4                                                                 # lr 1e-3: Adam moved the parameters
    assert all(e < UPDATE_TOL for e in errs.values()), errs
    assert _same_bits(p[0][~tail], flat[~tail])


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. cut invariance   5. model batching   6. train mask
# ---------------------------------------------------------------------------------------------------------------------------------
def test_epochs_cut_into_calls_leave_the_same_bits(nsd, dev):
    spec = _spec()
    N = 13
    flat, feats, q = _flat(32, 3, seed=4), _feats(N, 41), soft_targets(N, 3, seed=6)
    rng, kw = [_rng(seed=5, base=0xFFFFFFF8)], dict(lr=1e-2, weight_decay=1e-3)      # the stream id wraps inside the run
    whole = _fit(dev, spec, flat, feats, q, 7, rngs=rng, **kw)
    assert np.isfinite(whole[2]).all() and _fields(spec, whole[1])["epochs"][0] == 7
    for cut in ((3, 4), (1,) * 7):
        p, st, losses = flat, None, []
        for e in cut:
            p, st, loss = _fit(dev, spec, p, feats, q, e, state=st, rngs=rng, **kw)
            losses.append(loss)
        assert _same_bits(p, whole[0]) and _same_bits(st, whole[1]) and _same_bits(np.concatenate(losses, 1), whole[2]), cut
    assert whole[2][0, -1] < whole[2][0, 0]


def test_models_of_one_launch_are_the_single_model_calls(nsd, dev):
    from nsd_amd import _lib
    spec = _spec()
    N, M, E = 9, 3, 3
    params = np.stack([_flat(32, 3, seed=50 + m) for m in range(M)])
    feats = np.stack([_feats(N, 60 + m) for m in range(M)])
    q = np.stack([soft_targets(N, 3, seed=70 + m) for m in range(M)])
    rngs = [_rng(seed=80 + m, base=4 * m, p=0.2 + 0.1 * m) for m in range(M)]
    kw = dict(lr=1e-2)
    got = _fit(dev, spec, params, feats, q, E, rngs=rngs, **kw)
    for m in range(M):
        one = _fit(dev, spec, params[m], feats[m], q[m], E, rngs=[rngs[m]], **kw)
        assert all(_same_bits(a[m], b[0]) for a, b in zip(got, one)), m
    # one feature set for all models (stride 0) is the replicated set
    shared = _fit(dev, spec, params, feats[0], q, E, rngs=rngs, **kw)
    repl = _fit(dev, spec, params, np.stack([feats[0]] * M), q, E, rngs=rngs, **kw)
    assert all(_same_bits(a, b) for a, b in zip(shared, repl))
    # the largest launch once
    MM = _lib.NSD_MAX_MODELS
    big_p = np.stack([_flat(32, 3, seed=100 + m) for m in range(MM)])
    big_q = np.stack([soft_targets(N, 3, seed=200 + m) for m in range(MM)])
    big = _fit(dev, spec, big_p, feats[1], big_q, E, **kw)
    for m in (0, MM - 1):
        one = _fit(dev, spec, big_p[m], feats[1], big_q[m], E, **kw)
        assert all(_same_bits(a[m], b[0]) for a, b in zip(big, one)), m
    assert (_fields(spec, big[1])["epochs"] == E).all() and (_fields(spec, big[1])["status"] == 0).all()


MASKS = [("ln",), ("fc0",), ("fc3",), ("ln", "fc0"), ("ln", "fc3"), ("fc0", "fc3"), ("ln", "fc0", "fc3")]


def test_train_mask_changes_the_named_tensors_only(nsd, dev):
    spec = _spec()
    N = 10
    flat, feats, q = _flat(32, 3, seed=14), _feats(N, 15), soft_targets(N, 3, seed=16)
    rng, kw = [_rng(seed=17)], dict(lr=1e-2, weight_decay=1e-3)
    full = _fit(dev, spec, flat, feats, q, 1, rngs=rng, **kw)
    full2 = _fit(dev, spec, flat, feats, q, 2, rngs=rng, **kw)
    for train in MASKS:
        trained = _group_mask(spec, train)
        p, st, loss = _fit(dev, spec, flat, feats, q, 1, rngs=rng, train=train, **kw)
        assert _same_bits(p[0][~trained], flat[~trained]), train                      # LSTM, attention and the unnamed head tensors
        assert _same_bits(p[0][trained], full[0][0][trained]), train                   # the first update does not depend on the mask
        assert (p[0][trained] != flat[trained]).mean() > 0.9
        assert _same_bits(loss, full[2])
        idx = hf.trained_index(train, H, 32, 3)
        fld, ffl = _fields(spec, st), _fields(spec, full[1])
        assert _same_bits(fld["m"][0][idx], ffl["m"][0][idx]) and (fld["m"][0][~idx] == 0).all() and (fld["v"][0][~idx] == 0).all()
        if len(train) < 3:                                                             # the gradient flows through the frozen tensors
            p2 = _fit(dev, spec, flat, feats, q, 2, rngs=rng, train=train, **kw)[0]
            assert _same_bits(p2[0][~trained], flat[~trained]) and not _same_bits(p2[0][trained], full2[0][0][trained])


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. non-finite inputs
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["nan_feature", "inf_target"])
def test_a_non_finite_input_freezes_that_model_alone(nsd, dev, what):
    spec = _spec()
    N, M, E = 8, 3, 4
    params = np.stack([_flat(32, 3, seed=30 + m) for m in range(M)])
    feats = np.stack([_feats(N, 33 + m) for m in range(M)])
    q = np.stack([soft_targets(N, 3, seed=36 + m) for m in range(M)])
    rngs, kw = [_rng(seed=40 + m) for m in range(M)], dict(lr=1e-2)
    clean = _fit(dev, spec, params, feats, q, E, rngs=rngs, **kw)
    bad_f, bad_q = feats.copy(), q.copy()
    if what == "nan_feature":
        bad_f[1, 5, 7] = np.nan
    else:
        bad_q[1, 3, 2] = np.inf
    p, st, loss = _fit(dev, spec, params, bad_f, bad_q, E, rngs=rngs, **kw)
    fld = _fields(spec, st)
    assert _same_bits(p[1], params[1]) and np.isnan(loss[1]).all()
    assert fld["status"].tolist() == [0, 1, 0] and fld["epochs"].tolist() == [E, 0, E]
    assert (fld["m"][1] == 0).all() and (fld["v"][1] == 0).all()
    for m in (0, 2):
        assert all(_same_bits(a[m], b[m]) for a, b in zip((p, st, loss), clean)), m
    # clean inputs, the same state: model 1 stays refused until its state is zeroed
    p2, st2, loss2 = _fit(dev, spec, p, feats, q, E, state=st, rngs=rngs, **kw)
    assert _same_bits(p2[1], params[1]) and np.isnan(loss2[1]).all() and _fields(spec, st2)["status"].tolist() == [0, 1, 0]
    assert _fields(spec, st2)["epochs"].tolist() == [2 * E, 0, 2 * E] and np.isfinite(loss2[[0, 2]]).all()
    st2[1] = 0.0
    p3, st3, loss3 = _fit(dev, spec, p2, feats, q, E, state=st2, rngs=rngs, **kw)
    assert _fields(spec, st3)["status"].tolist() == [0, 0, 0] and all(_same_bits(a[1], b[1]) for a, b in zip((p3, st3, loss3), clean))


def test_a_non_finite_loss_keeps_the_last_good_epoch(nsd, dev):
    """parameters that overflow the logits: the first epoch's loss is not finite -> nothing moves, status 1, the other model is clean"""
    spec = _spec()
    N, E = 6, 3
    params = np.stack([_flat(32, 3, seed=90), _flat(32, 3, seed=91)])
    offs = spec.offsets()
    params[1, offs["fc.3.bias"]] = 3.0e38
    params[1, offs["fc.3.bias"] + 1] = -3.0e38
    feats, q = _feats(N, 92), np.stack([soft_targets(N, 3, seed=93)] * 2)
    clean = _fit(dev, spec, params[0], feats, q[0], E, lr=1e-2)
    p, st, loss = _fit(dev, spec, params, feats, q, E, lr=1e-2)
    fld = _fields(spec, st)
    assert _same_bits(p[1], params[1]) and np.isnan(loss[1]).all() and fld["status"].tolist() == [0, 1] and fld["epochs"].tolist() == [E, 0]
    assert all(_same_bits(a[0], b[0]) for a, b in zip((p, st, loss), clean))


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. the buffer and stream contract
# ---------------------------------------------------------------------------------------------------------------------------------
def _arena(dev, spec, M, N, E, params, feats, q, fill):
    """params, state, loss_out and feats of exactly the stated sizes between guards"""
    from nsd_amd import ops
    bufs = {"params": guarded((M, spec.param_count), torch.float32, dev, "zeros"),
            "state": guarded((M, int(ops.head_fit_layout(spec).stride)), torch.float32, dev, "zeros"),
            "loss_out": guarded((M, E), torch.float32, dev, fill), "feats": guarded((M, N, H), torch.float32, dev, "zeros"),
            "targets": guarded((M, N, spec.K), torch.float32, dev, "zeros")}
    bufs["params"][0].copy_(to_dev(params, dev))
    bufs["feats"][0].copy_(to_dev(feats, dev))
    bufs["targets"][0].copy_(to_dev(q, dev))
    return bufs


def _check(bufs):
    for name, (_, check) in bufs.items():
        check(name)


def test_buffers_of_the_stated_sizes_side_stream_and_graph_replay(nsd, dev):
    from nsd_amd import ops
    spec = _spec()
    M, N, E = 2, 7, 3
    assert int(ops.head_fit_state(spec, M, dev).numel()) * 4 == int(nsd.load_library().nsd_head_fit_state_bytes(C.byref(spec.dims(1, 1)), M))
    params = np.stack([_flat(32, 3, seed=110 + m) for m in range(M)])
    feats = np.stack([_feats(N, 112 + m) for m in range(M)])
    q = np.stack([soft_targets(N, 3, seed=114 + m) for m in range(M)])
    rngs = [_rng(seed=116 + m) for m in range(M)]
    kw = dict(epochs=E, lr=1e-2, rngs=rngs)
    ref = _fit(dev, spec, params, feats, q, E, rngs=rngs, lr=1e-2)

    def launch(b):
        ops.head_fit(spec, b["params"][0], b["feats"][0], b["targets"][0], b["state"][0], loss_out=b["loss_out"][0], **kw)

    def result(b):
        return tuple(b[k][0].cpu().numpy() for k in ("params", "state", "loss_out"))

    for fill in ("ones", "nan32"):
        b = _arena(dev, spec, M, N, E, params, feats, q, fill)
        inputs = snapshot(b["feats"][0], b["targets"][0])
        launch(b)
        torch.cuda.synchronize()
        _check(b)
        assert inputs.unchanged()
        assert all(_same_bits(a, r) for a, r in zip(result(b), ref)), fill
    # a side stream
    b = _arena(dev, spec, M, N, E, params, feats, q, "nan32")
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        launch(b)
    side.synchronize()
    _check(b)
    assert all(_same_bits(a, r) for a, r in zip(result(b), ref))
    # a captured graph, replayed: the epoch count lives in the state, so two replays are E + E epochs of one run
    b = _arena(dev, spec, M, N, E, params, feats, q, "nan32")
    two = _fit(dev, spec, ref[0], feats, q, E, state=ref[1], rngs=rngs, lr=1e-2)
    warm = _arena(dev, spec, M, N, E, params, feats, q, "nan32")
    launch(warm)                                                                        # the kernel's LDS attribute is set outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(b)
    graph.replay()
    torch.cuda.synchronize()
    assert all(_same_bits(a, r) for a, r in zip(result(b), ref))
    graph.replay()
    torch.cuda.synchronize()
    _check(b)
    assert all(_same_bits(a, r) for a, r in zip(result(b), two))


def test_every_refusal_leaves_guarded_buffers_untouched(nsd, dev):
    from nsd_amd import _lib, ops
    from nsd_amd._lib import NsdError
    spec = _spec()
    M, N, E = 2, 7, 3
    params = np.stack([_flat(32, 3, seed=120 + m) for m in range(M)])
    feats = np.stack([_feats(N, 122 + m) for m in range(M)])
    q = np.stack([soft_targets(N, 3, seed=124 + m) for m in range(M)])
    b = _arena(dev, spec, M, N, E, params, feats, q, "nan32")
    before = snapshot(*(v[0] for v in b.values()))
    L = nsd.load_library()
    d = spec.dims(N, 1)
    ptr = {k: v[0].data_ptr() for k, v in b.items()}
    nbytes = ops._nbytes(b["state"][0])

    def call(dd=d, MM=M, params=ptr["params"], feats=ptr["feats"], stride=N * H, targets=ptr["targets"], fit=None, rng=None,
             state=ptr["state"], nb=nbytes, **ch):
        f = _lib.Fit(E, 7, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0 / N)
        for k, v in ch.items():
            setattr(f, k, v)
        return L.nsd_head_fit(C.byref(dd), MM, params, feats, stride, targets, None if fit == "null" else C.byref(f), rng, state, nb,
                              ptr["loss_out"], None)

    bad_rng = (_lib.Rng * M)(_lib.Rng(1, 0, 0.0, 0.5), _lib.Rng(2, 0, 0.0, 1.0))
    refusals = [dict(params=None), dict(feats=None), dict(targets=None), dict(fit="null"), dict(state=None), dict(MM=0), dict(MM=33),
                dict(dd=spec.dims(0, 1)), dict(dd=spec.dims(257, 1)), dict(dd=_spec(64, 8).dims(193, 1)), dict(epochs=0),
                dict(epochs=_lib.NSD_FIT_MAX_EPOCHS + 1), dict(train=0), dict(train=8), dict(lr=-1.0), dict(lr=float("inf")),
                dict(beta1=1.0), dict(beta2=1.5), dict(eps=0.0), dict(weight_decay=-1.0), dict(stride=-1), dict(stride=N * H - 1),
                dict(rng=bad_rng)]
    for kw in refusals:
        assert call(**kw) == -1, kw
    assert call(nb=nbytes - 1) == -3
    with pytest.raises(NsdError):
        ops.head_fit(spec, b["params"][0], b["feats"][0], b["targets"][0], b["state"][0], epochs=E, train=("attn",))
    torch.cuda.synchronize()
    _check(b)
    assert before.unchanged()
    # the stream features' refusals, on a guarded state
    lay = ops.stream_layout(spec)
    state, check_state = guarded((3, int(lay.stride)), torch.float32, dev, "zeros")
    out, check_out = guarded((3, H), torch.float32, dev, "nan32")
    sb, keep = ops._nbytes(state), snapshot(state, out)
    sd = spec.dims(0, 1)
    for args in ((None, sb, 3, None, 3, out.data_ptr()), (state.data_ptr(), sb, 3, None, 3, None), (state.data_ptr(), sb, 0, None, 0, out.data_ptr()),
                 (state.data_ptr(), sb, 3, None, -1, out.data_ptr()), (state.data_ptr(), sb, 3, None, 4, out.data_ptr())):
        assert L.nsd_stream_features(C.byref(sd), *args, None) == -1, args
    assert L.nsd_stream_features(C.byref(sd), state.data_ptr(), sb - 1, 3, None, 3, out.data_ptr(), None) == -3
    h64 = ops.ModelSpec(C=8, H=64, L=2, K=3, F=32).dims(0, 1)                          # outside nsd_stream_path
    assert L.nsd_stream_features(C.byref(h64), state.data_ptr(), sb, 3, None, 3, out.data_ptr(), None) == -1
    torch.cuda.synchronize()
    check_state("state")
    check_out("feats")
    assert keep.unchanged()


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. it learns
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_it_separates_three_clusters(nsd, dev, seed):
    """K = 3 Gaussian clusters in feature space (centres N(0, 1), spread 0.1, N = 24), a randomly initialised head, 100 eval-mode epochs
    at lr 1e-2.  A float64 PyTorch loop on seeds 0, 1, 2 takes the loss from ~1.1 to below 1e-6 at 100 % accuracy; asserted here: 100 %
    and a final loss at most 1/100 of the first (compounding fp32 Adam trajectories are not comparable element-wise)."""
    spec = _spec()
    N, K = 24, 3
    rs = np.random.RandomState(seed)
    centres = rs.standard_normal((K, H))
    y = np.arange(N) % K
    feats = (centres[y] + 0.1 * rs.standard_normal((N, H))).astype(np.float32)
    flat = _flat(32, 3, seed=300 + seed)
    p, st, loss = _fit(dev, spec, flat, feats, np.eye(K, dtype=np.float32)[y], 100, lr=1e-2)
    logits = _numpy_readout(spec, p[0], feats)
    print(f"clusters seed {seed}: loss {loss[0, 0]:.4f} -> {loss[0, -1]:.3e}")
    assert _fields(spec, st)["status"][0] == 0
    assert (logits.argmax(1) == y).all()
    assert loss[0, -1] <= loss[0, 0] / 100.0


# ---------------------------------------------------------------------------------------------------------------------------------
# 10. end to end
# ---------------------------------------------------------------------------------------------------------------------------------
FROZEN = ("lstm.", "attn.")


def _trials(n, T, seed):
    """n synthetic cued trials of three classes: a class-dependent offset pattern over the channels plus noise"""
    rs = np.random.RandomState(seed)
    y = np.arange(n) % 3
    pattern = 2.0 * rs.standard_normal((3, 1, 8))
    return (pattern[y] + rs.standard_normal((n, T, 8))).astype(np.float32), y


def _pth(tmp_path, name, seed):
    os.makedirs(os.path.join(tmp_path, name), exist_ok=True)
    st = synth_params(8, H, 2, 3, seed=seed)
    return write_pth(os.path.join(tmp_path, name), st), st


def test_simple_predictor_calibrate_end_to_end(nsd, dev, tmp_path):
    from nsd_amd.trainer import save_reference_checkpoint
    path, st0 = _pth(str(tmp_path), "a", seed=7)
    pred = nsd.SimplePredictor(path, 125, preprocess="identity")
    x, y = _trials(12, 20, seed=1)
    live = pred.open_stream(streams=2)
    chunk1, chunk2 = synth_x(2, 9, seed=2), synth_x(2, 8, seed=3)
    live.push(chunk1)
    rep = pred.calibrate(x, y, epochs=60, lr=1e-2)
    assert rep["n"] == 12 and rep["epochs"] == [60] and rep["status"] == [0]
    assert rep["loss_after"] < rep["loss_before"] and rep["acc_after"] >= rep["acc_before"]
    assert rep["fit_losses"].shape == (1, 60) and rep["fit_losses"][0, -1] < rep["fit_losses"][0, 0]
    out = os.path.join(str(tmp_path), "calibrated.pth")
    save_reference_checkpoint(pred.model, out)
    sd = torch.load(out, map_location="cpu", weights_only=True)
    assert list(sd.keys()) == list(st0.keys())
    for k, v in st0.items():
        same = np.array_equal(sd[k].numpy().view(np.uint32), np.asarray(v).view(np.uint32))
        assert same == k.startswith(FROZEN), k
    # the open decoder kept its state and reads the fitted head: bit-equal to a fresh decoder of the written checkpoint
    got, _ = live.push(chunk2)
    fresh = nsd.SimplePredictor(out, 125, preprocess="identity").open_stream(streams=2)
    fresh.push(chunk1, read=False)
    want, _ = fresh.push(chunk2)
    assert _same_bits(got, want)
    assert (live.steps == 17).all()
    with pytest.raises(nsd.NsdError):
        pred.open_stream(streams=1, window_seconds=0.08, hop_seconds=0.04).decoder.features()


def test_ensemble_predictor_calibrate_and_the_command_line(nsd, dev, tmp_path, capsys):
    from nsd_amd import calibrate
    from nsd_amd.trainer import save_reference_checkpoint
    paths, states = zip(*[_pth(str(tmp_path), f"m{m}", seed=17 + m) for m in range(2)])
    pred = nsd.EnsemblePredictor(list(paths), 125, preprocess="identity")
    x, y = _trials(12, 20, seed=4)
    live = pred.open_stream(streams=2)
    chunk1, chunk2 = synth_x(2, 9, seed=5), synth_x(2, 8, seed=6)
    live.push(chunk1)
    rep = pred.calibrate(x, y, epochs=60, lr=1e-2)
    assert rep["epochs"] == [60, 60] and rep["status"] == [0, 0] and rep["loss_after"] < rep["loss_before"]
    outs = []
    for m, member in enumerate(pred.members):
        outs.append(os.path.join(str(tmp_path), f"cal{m}.pth"))
        save_reference_checkpoint(member, outs[-1])
        sd = torch.load(outs[-1], map_location="cpu", weights_only=True)
        assert list(sd.keys()) == list(states[m].keys())
        for k, v in states[m].items():
            assert np.array_equal(sd[k].numpy().view(np.uint32), np.asarray(v).view(np.uint32)) == k.startswith(FROZEN), (m, k)
    got, _ = live.push(chunk2)
    fresh = nsd.EnsemblePredictor(outs, 125, preprocess="identity").open_stream(streams=2)
    fresh.push(chunk1, read=False)
    want, _ = fresh.push(chunk2)
    assert _same_bits(got, want)
    # the command line on a packed session: one JSON line, checkpoints with the reference's keys
    xs, ys = _trials(18, 20, seed=8)
    names = ["water", "food", "backgroundnoise"]
    data = os.path.join(str(tmp_path), "session.npz")
    np.savez(data, x=xs, stem=np.array([f"{names[k]}_{i:03d}" for i, k in enumerate(ys)]))
    capsys.readouterr()
    rc = calibrate.main(["--model", paths[0], "--model", paths[1], "--data", data, "--calib-per-class", "4", "--epochs", "40", "--lr", "1e-2",
                         "--T", "20", "--out", os.path.join(str(tmp_path), "cli.pth")])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert rc == 0 and len(line) == 1
    rec = json.loads(line[0])
    assert rec["models"] == 2 and rec["calib_trials"] == 12 and rec["held_out_trials"] == 6 and rec["status"] == [0, 0]
    assert 0.0 <= rec["held_out_acc_before"] <= 1.0 and 0.0 <= rec["held_out_acc_after"] <= 1.0
    for m, out in enumerate(rec["out"]):
        sd = torch.load(out, map_location="cpu", weights_only=True)
        assert list(sd.keys()) == list(states[m].keys())
        assert all(np.array_equal(sd[k].numpy(), np.asarray(v)) for k, v in states[m].items() if k.startswith(FROZEN))
        assert not np.array_equal(sd["fc.3.weight"].numpy(), states[m]["fc.3.weight"])
