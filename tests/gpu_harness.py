"""What the fp32 GPU parity tests share: fixtures, the bound table, the gradient comparator, the driver of ops.train_step_grads, the
oracle's side of a train step and the comparison of the two.  A plain helper module (no conftest): test files import the fixtures
and helpers they use by name.  Imports without a GPU; tests/test_gpu_harness_cpu.py holds the comparators and the table to their
word on the host.  The bf16 sequence path has a bound family of its own (tests/test_gpu_seqpath*.py) and takes only dev, nsd and
to_dev from here."""
import os

import numpy as np
import pytest
import torch

from oracle import nsd_oracle as orc
from tests import mixup_ref as mr
from tests.golden.make_goldens import counter_masks, synth_labels, synth_params, synth_x

NAN = float("nan")
D = orc.Dims()                   # the reference model: C = 8, H = 48, L = 2, K = 3, F = 32


# ---------------------------------------------------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def nsd():
    import nsd_amd
    nsd_amd.load_library()          # raises if libnsd_hip.so is missing: no fallback
    return nsd_amd


@pytest.fixture(scope="module")
def cus(dev):
    return int(torch.cuda.get_device_properties(dev).multi_processor_count)


@pytest.fixture(autouse=True)
def sync_at_the_end():
    """autouse in the files that import it: every test ends with the device idle (ops._call has checked the return code of every
    ABI call)"""
    yield
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# small helpers
# ---------------------------------------------------------------------------------------------------------------------------------
def to_dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def spec_of(d):
    from nsd_amd import ops
    return ops.ModelSpec(C=d.C, H=d.H, L=d.L, K=d.K, F=d.F)


def model_from_state(nsd, dev, state, **kw):
    H = state["lstm.weight_hh_l0"].shape[1]
    L = sum(1 for k in state if k.startswith("lstm.weight_hh_l"))
    m = nsd.EEG_LSTM(input_size=state["lstm.weight_ih_l0"].shape[1], hidden_size=H, num_layers=L,
                     num_classes=state["fc.3.weight"].shape[0], **kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}, strict=True)
    return m.to(dev)


def write_pth(tmp_path, ref_state, wrapped=False):
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in ref_state.items()}
    p = os.path.join(tmp_path, "model.pth")
    torch.save({"state_dict": sd} if wrapped else sd, p)
    return p


def kink_safe(st, F):
    """fc.0.bias = +-4, alternating (the convention of tests/test_gpu_seqpath_bf16ref.py): for batches of hundreds of trials, where
    no seed keeps tens of thousands of fc.0 pre-activations 1e-4 away from the RReLU kink.  Both slopes stay in use."""
    st = dict(st)
    st["fc.0.bias"] = np.where(np.arange(F) % 2 == 0, 4.0, -4.0).astype(np.float32)
    return st


def head_inputs(Cc, H, K, F, B, T, L=2, safe=False):
    """(dims, flat parameters, x, labels, masks) of a shape: every input from the generators of tests/golden/make_goldens.py
    (safe: fc.0.bias replaced by kink_safe's)"""
    d = orc.Dims(C=Cc, H=H, L=L, K=K, F=F)
    st = synth_params(Cc, H, L, K, F=F, seed=H + F + K)
    flat = orc.flatten_state(kink_safe(st, F) if safe else st, d)
    x, y = synth_x(B, T, C=Cc, seed=F), synth_labels(B, K=K, seed=K)
    dl, sl, dh = counter_masks(B, T, H, F, L=L, seed=F + K)
    masks = dict(rrelu_slope=sl, drop_head=dh)
    if L > 1:
        masks["drop_lstm"] = dl
    return d, flat, x, y, masks


def kink_margin(fw):
    """smallest |fc.0 pre-activation| of the ORACLE's forward: the distance of the data from the RReLU kink"""
    return float(np.abs(fw["fc0_pre"]).min())


def soft_targets(B, K, seed):
    """non-negative rows with sums != 1 and (B > 1) a zero row"""
    q = (1.5 * np.random.RandomState(seed).rand(B, K)).astype(np.float32)
    q[np.random.RandomState(seed + 1).rand(B, K) < 0.2] = 0.0
    if B > 1:
        q[1] = 0.0
    return q


def oracle_streams(seed, sid, B, T, H, F, p=0.6):
    """the multipliers the kernels draw from rng=dict(seed=, base_stream=sid, p_lstm=p, p_head=p), as the oracle's tensors"""
    return dict(drop_lstm=orc.dropout_mask(seed, sid, p, (1, B, T, H)), rrelu_slope=orc.rrelu_noise(seed, sid + 1, (B, F)),
                drop_head=orc.dropout_mask(seed, sid + 2, p, (B, F)))


# Shapes shared by a GPU file and the CPU file that pins the oracle at them.
# (C, H, K, F, B, T), L = 2: the shapes of tests/test_gpu_head_dims.py
BASE_SHAPES = [(8, 48, 3, 32, 6, 20), (8, 48, 8, 64, 5, 33), (8, 48, 9, 33, 5, 33), (8, 48, 64, 1, 4, 12),
               (5, 48, 1, 17, 4, 12), (8, 64, 33, 48, 6, 15), (8, 32, 5, 7, 6, 15), (8, 48, 2, 63, 7, 40)]
# (C, H, K, F, B, T, residual), L = 2.  T: the first step, the step after it (layer 0's backward lags by two macro steps), both sides of
# each 32-step chunk of the staged x / dropout-mask double buffer, and a fourth chunk (both buffers reused).  Each H sees every C of
# {8, 7, 5, 1} (C = 7, 5, 1: the odd split of the two-channel pairs of a quad) and both values of the residual flag.
T_EDGES = [(8, 32, 3, 32, 5, 1, False), (7, 32, 5, 7, 6, 2, True), (5, 32, 3, 32, 8, 31, False), (1, 32, 2, 33, 7, 32, True),
           (8, 32, 4, 33, 4, 33, True), (7, 32, 3, 32, 8, 64, False), (5, 32, 2, 32, 6, 65, True), (1, 32, 3, 32, 5, 97, False),
           (1, 64, 3, 32, 4, 1, True), (5, 64, 4, 33, 7, 2, False), (7, 64, 3, 32, 8, 31, True), (8, 64, 5, 7, 5, 32, False),
           (1, 64, 2, 32, 6, 33, False), (5, 64, 3, 32, 8, 64, True), (7, 64, 2, 33, 5, 65, False), (8, 64, 3, 32, 4, 97, True)]
# Two branches of the head launchers (csrc/nsd_head.hip) that no other row of the suite takes, on the generic route (section d of
# tests/test_gpu_fp32_routes.py; (C, H, L, K, F, (m, a): B = m * cus + a, T, residual, grid loops)): H % 4 != 0 -- the scalar score loop, the
# sequence read in place -- and a sequence that does not fit in LDS beside the vectors (560 rows of 68 floats = 152 320 B of the 144 KB):
# head_fwd_kernel / head_bwd_kernel read the rows from memory, 16 bytes at a time, and the fused train head declines (150 KB).
HEAD_BRANCH_ROWS = [(3, 30, 1, 3, 32, (0, 3), 5, False, False), (8, 60, 1, 3, 32, (0, 2), 560, False, False)]
# Step counts at the loop edges of the one-trial H = 48 kernels, shared by the files that sweep them.
# T' of the forward's prefix pairs: around the ring (16), the x chunk (32) and their multiples, +-2 for layer 1's lag
FWD_T = (1, 2, 3, 13, 14, 15, 16, 17, 18, 29, 30, 31, 32, 33, 34, 47, 48, 49, 63, 64, 65)
# ... and what the backward adds: its 8-step ring, the four-step hand-off groups and layer 0's five-step lag
BWD_T = tuple(sorted(set(FWD_T) | {4, 5, 6, 7, 8, 9, 11, 12, 20, 21, 24, 25}))
# inference: every T of 1..100, the step counts around 128 and 256 and the fast path's limit of 1024 (1025 and 1026 leave it)
INFER_T = tuple(range(1, 101)) + (126, 127, 158, 250, 254, 255, 256, 257, 1022, 1023, 1024, 1025, 1026)


def worse(a, b):
    """the larger of a running worst value and a new one; a NaN is worse than any number and stays"""
    return b if (b != b or b > a) else a


# ---------------------------------------------------------------------------------------------------------------------------------
# the bound table of the fp32 paths
# ---------------------------------------------------------------------------------------------------------------------------------
# Class logits of any fp32 route, train forward or inference, against the oracle or the reference goldens, absolute (the project's
# north star; argmax identical where the top-two gap is clear).  Measured <= 3.8e-6 (train) / 1.4e-6 (inference) over
# tests/test_gpu_head_dims.py, 2.9e-6 / 1.4e-6 over tests/test_gpu_fp32_routes.py.
LOGIT_TOL = 1e-4
PROB_TOL = 1e-5                  # class probabilities, absolute; measured <= 3.6e-7
# Batch-mean loss against the oracle's, absolute.  Measured <= 3.8e-7 (head dims), 3.1e-7 (fp32 routes).
LOSS_TOL = 5e-5
# alpha, pooled, fc0_pre of the workspace against the oracle's forward, absolute (section (a) of tests/test_gpu_head_dims.py);
# measured 1.2e-7, 1.1e-6, 4.3e-6 over tests/test_gpu_fp32_routes.py.
HEAD_TOL = 5e-5
# dL/dx against the oracle's, of its largest element.  Measured <= 2.4e-6 over the whole suite, 6.1e-7 over the head sizes.
DX_TOL = 2e-5
# Gradients of the H = 48, C <= 8 fast path (the benchmarked kernels) against the oracle and the reference goldens: the LSTM weight
# gradients (split-bf16 sums over time, nsd_lstm2_bwd48*.hip) within wtol = 5e-5 of each tensor's largest element, every other tensor
# within rtol = 2e-5 (grad_close adds a 1e-7 floor and holds attn.bias to 2e-6 absolute).  Measured over the whole suite on the MI355X
# (178 comparisons, the "grad_close worst" lines): LSTM weight gradients <= 2.5e-5, the other tensors <= 1.7e-5 wherever the 1e-7 floor
# is not what holds them (tensors with a largest element below ~5e-3 at T <= 2); 5.1e-6 / 2.1e-6 over the head sizes of
# tests/test_gpu_head_dims.py (FAST48, first measured at F = 32, K = 3, holds at every head size).  Dropping one of the three
# split-bf16 MFMAs of either backward kernel fails dozens of these comparisons.
FAST48 = dict(rtol=2e-5, wtol=5e-5)
# Gradients of the exact-fp32 routes -- no reduced-precision products: the first-generation H = 32 / 64 kernels of nsd_lstm2.hip, the
# generic path and the batched MFMA path -- against the oracle, of each tensor's largest element: the LSTM weight gradients within
# 1e-5, every other tensor within 2e-5 (floor and attn.bias as above).  About eight times the worst value measured over
# tests/test_gpu_fp32_routes.py on one MI355X (1.25e-6: weight_ih_l0 of the generic path at 2051 trials; 2.25e-6: attn.weight at
# T = 2, and fc.3.bias at K = 2, where the sum over the batch nearly cancels): the room FAST48 has.  Neither exceeds FAST48's
# (asserted by that file).  The comparisons of these routes in tests/test_gpu_parity.py measure <= 7.5e-7 / 4.8e-6.
FP32_EXACT = dict(rtol=2e-5, wtol=1e-5)
# A model of a model-batched launch against its single run, every tensor of its largest element (H = 48: split-bf16 sums in another
# order; the same arithmetic twice).  Measured 1.1e-5.
MULTI_RTOL = 3e-4
# The general gradient bound of tests/test_gpu_parity.py, every tensor of its largest element, where FAST48 / FP32_EXACT are not what is
# claimed: two launch sequences of one step against each other (the fused head against the two launches it replaces, soft targets on
# one-hot rows against hard labels), the gradients of the reference goldens' residual extension and the residual step from 513
# trials, soft targets against the oracle -- on the one- / two-trial H = 48 kernels ...
GRAD_RTOL_12 = 2e-4
# ... and where the four-trial H = 48 kernels run (from 513 trials, or pinned), the module's autograd at H = 32 and the sampled
# cfg3 goldens of the generic path (H = 256).
GRAD_RTOL_X4 = 3e-4
# Inputs that drive the gates to both rails (|pre-activation| up to ~1e4) or lie near zero, against the oracle
# (test_tiny_and_saturating_inputs).
GRAD_RTOL_SATURATED = 5e-4
# The smallest |fc.0 pre-activation| of the ORACLE that a gradient comparison accepts: a pre-activation that oracle and kernel round
# to different sides of the RReLU kink changes that trial's whole backward without either being wrong.  KINK_MARGIN: 100x the fp32
# forward error the GPU suite measures on fc.0's pre-activation (head sizes, fp32 routes, buffer contract).  KINK: the model-batched
# twins, whose inputs are drawn again until they pass -- three times the 48 x 2^-24 x 0.6 = 1.7e-6 that two orders of fc.0's sum of
# 48 products (LayerNorm outputs |.| <= 3, weights |.| <= 0.2) can differ by.
KINK_MARGIN = 1e-4
KINK = 5e-6


def bounds_of(d):
    """the gradient bounds of a shape's route: FAST48 on the H = 48 fast path (its forward and backward kernels, whichever head
    follows them), the exact-fp32 FP32_EXACT on every other route"""
    return FAST48 if (d.H == 48 and d.L == 2 and d.C <= 8) else FP32_EXACT


# ---------------------------------------------------------------------------------------------------------------------------------
# the gradient comparator
# ---------------------------------------------------------------------------------------------------------------------------------
def grad_class(name):
    return "attn.bias" if name == "attn.bias" else "lstm.weight" if name.startswith("lstm.weight") else "other"


def grad_errors(got_flat, ref_flat, d):
    """(per, worst): per[name] = (largest |got - ref| of the tensor, scale = its largest |ref| element, at least 1e-6);
    worst[class] = the largest error / scale of the class (attn.bias: the error itself), nan if any of them is NaN"""
    got, ref = orc.unflatten(got_flat, d), orc.unflatten(ref_flat, d)
    per, worst = {}, {"lstm.weight": 0.0, "other": 0.0, "attn.bias": 0.0}
    for k in orc.param_names(d):
        err = float(np.abs(got[k] - ref[k]).max())
        scale = max(float(np.abs(ref[k]).max()), 1e-6)
        per[k] = (err, scale)
        cls = grad_class(k)
        worst[cls] = worse(worst[cls], err if cls == "attn.bias" else err / scale)
    return per, worst


def grad_close(got_flat, ref_flat, d, rtol, wtol=None):
    """Every gradient tensor within rtol of its largest element (+1e-7); the LSTM weight gradients within wtol where given;
    attn.bias within 2e-6 absolute.  Prints the worst ratio per tensor class (error / largest element; attn.bias: the error).
    Every comparison is written so that a NaN fails it."""
    per, worst = grad_errors(got_flat, ref_flat, d)
    bad = []
    for k, (err, scale) in per.items():
        cls = grad_class(k)
        if cls == "attn.bias":
            if not err < 2e-6:
                bad.append((k, err))
            continue
        tol = wtol if (wtol is not None and cls == "lstm.weight") else rtol
        if not err <= tol * scale + 1e-7:
            bad.append((k, err, scale))
    print("grad_close worst", {k: f"{v:.2e}" for k, v in worst.items()}, "bounds", (rtol, wtol))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# one train step: the kernels' side and the oracle's
# ---------------------------------------------------------------------------------------------------------------------------------
HEAD_SAVES = ("alpha", "pooled", "fc0_pre", "dscore", "dpooled")         # the head's workspace outputs


def train_step(dev, spec, flat_np, x, *, labels=None, targets=None, masks=None, rng=None, residual=False, fused=True, want_dx=False,
               saves=()):
    """ops.train_step_grads (the launch sequence of Trainer.step) with the workspace, logits, gradients and dx full of NaN beforehand
    -- nothing may be left unwritten -> dict of logits, grads, loss (per trial), mean_loss (their float64 sum / B), loss_sum
    (ops.loss_sum's fp32 value), dx with want_dx, and the workspace regions named in saves"""
    from nsd_amd import ops
    B, T, _ = x.shape
    flat, xt = to_dev(flat_np, dev), to_dev(x, dev)
    ws = ops.new_workspace(spec, B, T, dev)
    ws.fill_(NAN)
    logits = torch.full((B, spec.K), NAN, device=dev)
    grads = torch.full_like(flat, NAN)
    dx = torch.full_like(xt, NAN) if want_dx else None
    lab = None if labels is None else to_dev(np.asarray(labels).astype(np.int32), dev)
    ops.train_step_grads(spec, flat, xt, ws, lab, logits, grads, residual=residual, fused_head=fused, rng=rng, dx=dx,
                         targets=to_dev(targets, dev), **{k: to_dev(v, dev) for k, v in (masks or {}).items()})
    out = {r: ops.ws_view(ws, spec, B, T, r).cpu().numpy().copy() for r in ("loss",) + tuple(saves)}
    out.update(logits=logits.cpu().numpy(), grads=grads.cpu().numpy(), mean_loss=float(out["loss"].astype(np.float64).sum()) / B,
               loss_sum=float(ops.loss_sum(spec, ws, B, T).item()))
    if want_dx:
        out["dx"] = dx.cpu().numpy()
    return out


def forward_backward(dev, flat_np, x, y, spec=None, scale=None, **masks):
    """the step as three calls of their own entry points -- ops.train_forward, ops.train_backward, ops.loss_sum -- -> (batch-mean
    loss, flat gradient, logits); residual= rides among the masks"""
    from nsd_amd import ops
    spec = spec or ops.ModelSpec()
    B, T, _ = x.shape
    flat, xt = to_dev(flat_np, dev), to_dev(x, dev)
    ws = ops.new_workspace(spec, B, T, dev)
    mk = {k: to_dev(v, dev) for k, v in masks.items() if k != "residual"}
    res = masks.get("residual", False)
    logits, _ = ops.train_forward(spec, flat, xt, ws, residual=res, **mk)
    g = ops.train_backward(spec, flat, xt, ws, logits, labels=to_dev(y.astype(np.int32), dev), scale=scale, residual=res, **mk)
    loss = float(ops.loss_sum(spec, ws, B, T).item()) / B
    return loss, g.cpu().numpy(), logits.cpu().numpy()


def oracle_step(d, flat_np, x, *, labels=None, targets=None, masks=None, residual=False, want_dx=False, kink=None):
    """The oracle's train evaluation: forward, cross-entropy of hard labels (orc.ce_loss) or of soft targets (mixup_ref.soft_ce,
    float64), backward -> dict of logits, loss (batch mean), loss_per_trial (soft targets), grads, dx (None without want_dx) and
    fw, the forward's saves.  With kink= it first asserts that ITS fc.0 pre-activations stay further than that from the RReLU kink."""
    masks = masks or {}
    B = x.shape[0]
    fw = orc.forward(flat_np, x, d, saves=True, residual=residual, **masks)
    if kink is not None:
        margin = kink_margin(fw)
        assert margin > kink, margin
    if targets is None:
        loss, dl = orc.ce_loss(fw["logits"], labels)
        per = None
    else:
        per, dl = mr.soft_ce(fw["logits"], targets, 1.0 / B)
        loss, dl = float(np.sum(per)) / B, dl.astype(np.float32)
    g = orc.backward(flat_np, x, d, fw, dl, residual=residual, want_dx=want_dx, **masks)
    g, dx = g if want_dx else (g, None)
    return dict(logits=fw["logits"], loss=loss, loss_per_trial=per, grads=g, dx=dx, fw=fw)


def assert_step_vs_oracle(out, ref, d, bounds, tag=None):
    """A train evaluation (train_step's dict, or any dict of logits, grads and mean_loss) against oracle_step's: logits and gradients
    finite, logits within LOGIT_TOL, mean loss within LOSS_TOL, grad_close with `bounds`, and dx within DX_TOL of its largest element
    where both sides have one.  One class: CE and all of its gradients are exactly zero in the oracle, so |loss| < 1e-7 and every
    gradient entry <= 1e-7.  Prints before it asserts (with a tag); returns the errors it measured."""
    logits, grads = out["logits"], out["grads"]
    errs = dict(logits=float(np.abs(logits - ref["logits"]).max()), loss=abs(out["mean_loss"] - ref["loss"]))
    if tag is not None:
        print(f"[{tag}] C={d.C} H={d.H} L={d.L} K={d.K} F={d.F}: logits {errs['logits']:.2e}  loss {errs['loss']:.2e}")
    assert np.isfinite(logits).all() and np.isfinite(grads).all(), tag
    assert errs["logits"] < LOGIT_TOL, (tag, errs["logits"])
    if d.K == 1:
        errs.update(loss=abs(out["mean_loss"]), k1_grad=float(np.abs(grads).max()))
        assert abs(ref["loss"]) < 1e-7 and np.abs(ref["grads"]).max() <= 1e-7
        assert errs["loss"] < 1e-7 and errs["k1_grad"] <= 1e-7, (tag, out["mean_loss"], errs["k1_grad"])
        return errs
    assert errs["loss"] < LOSS_TOL, (tag, out["mean_loss"], ref["loss"])
    grad_close(grads, ref["grads"], d, **bounds)
    if "dx" in out and ref.get("dx") is not None:
        err, scale = float(np.abs(out["dx"] - ref["dx"]).max()), float(np.abs(ref["dx"]).max())
        errs["dx"] = err / scale
        print(f"dx {tag or out['dx'].shape}: max error / largest element {errs['dx']:.2e}")
        assert np.isfinite(out["dx"]).all() and err <= DX_TOL * scale, (tag, err, scale)
    return errs


# ---------------------------------------------------------------------------------------------------------------------------------
# the model-batched path: M models of one launch and the same model alone
# ---------------------------------------------------------------------------------------------------------------------------------
def multi_problem(spec, M, B, T, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    params = ((torch.rand((M, spec.param_count), generator=g) - 0.5) * 0.4).to(dev)
    x = torch.randn((M, B, T, spec.C), generator=g).to(dev)
    y = torch.randint(0, spec.K, (M, B), generator=g, dtype=torch.int32).to(dev)
    rngs = [dict(seed=1000 + 17 * m, base_stream=4 * (m + 1), p_lstm=0.6, p_head=0.6) for m in range(M)]
    return params, x, y, rngs


def multi_single(nsd, spec, flat, x, y, rng, dev, adam=None):
    from nsd_amd import ops
    B, T, _ = x.shape
    ws = ops.new_workspace(spec, B, T, dev)
    logits = torch.empty((B, spec.K), dtype=torch.float32, device=dev)
    grads = torch.empty(spec.param_count, dtype=torch.float32, device=dev)
    ops.train_step_grads(spec, flat, x.contiguous(), ws, y.contiguous(), logits, grads, rng=rng, adam=adam)
    loss = ops.loss_sum(spec, ws, B, T)
    return logits, grads, float(loss.item()) / B


def multi_step(nsd, spec, params, x, y, rngs, dev, fuse_adam=False, m=None, v=None, step=1):
    from nsd_amd import ops
    M = params.shape[0]
    B, T = y.shape[1], x.shape[-2]
    ws = ops.multi_workspace(spec, M, B, T, dev)
    grads = torch.empty_like(params)
    logits = ops.multi_train_step(spec, params, x, y.contiguous().view(-1), ws, grads, rngs=rngs, fuse_adam=fuse_adam, m=m, v=v, step=step)
    losses = ops.multi_loss_sum(spec, ws, M, B, T).cpu().double() / B
    return logits.view(M, B, spec.K), grads, losses


def multi_grad_ok(spec, got, ref):
    """grad_close's rule with FAST48 on device tensors: LSTM weight gradients within 5e-5 of their largest element, the other
    tensors within 2e-5 (+1e-7), attn.bias (a sum over time that is zero but for rounding) within 2e-6 absolute."""
    offs, shapes = spec.offsets(), spec.shapes()
    for n, shp in shapes.items():
        n_el = int(np.prod(shp))
        a, b = got[offs[n]:offs[n] + n_el], ref[offs[n]:offs[n] + n_el]
        err = float((a - b).abs().max())
        if n == "attn.bias":
            assert err < 2e-6, (n, err)
            continue
        tol = FAST48["wtol"] if n.startswith("lstm.weight") else FAST48["rtol"]
        scale = max(float(b.abs().max()), 1e-6)
        assert err <= tol * scale + 1e-7, (n, err, scale)
