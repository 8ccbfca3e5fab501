"""The exact-fp32 routes beside the H = 48 fast path, against the CPU oracle in every band of their dispatch: the first-generation
fused kernels lstm2_fwd_kernel<H, NB> / lstm2_bwd_kernel<H, NB> of csrc/nsd_lstm2.hip (H = 32 and H = 64: what EEG_LSTM(hidden_size=32)
or 64 runs) and the shape-generic kernels of csrc/nsd_lstm_generic.hip at batches that make their grids loop.  Needs a real MI355X:
run with `pytest -m gpu -s` (every comparison prints its errors before it asserts, the last test of the file the worst per class).
tests/test_fp32_routes_cpu.py pins the oracle to a float64 restatement of the model at these widths, channel counts and T edges.

  a. T edges, one trial per workgroup (T_EDGES of the CPU file): T = 1 and 2 (layer 0's backward lags by two macro steps), both sides
     of each 32-step chunk of the staged x / dropout-mask double buffer (XCH = 32: 31, 32, 33, 64, 65) and a fourth chunk that reuses
     both buffers (97); C in {8, 7, 5, 1} (the odd split of the two-channel pairs, the guarded dW_ih0 slab write) and the residual flag.
  b. the batch bands.  With cus = the device's CU count (nothing here hard-codes 256): pick_nb takes one trial per workgroup up to cus
     trials, two up to 2 cus, four beyond; the backward takes one up to 2 cus and two beyond, on at most cus workgroups (= gradient
     slabs), the forward on at most 2 cus.  The rows reach fwd<32,1|2|4>, fwd<64,2|4>, bwd<32,1|2>, bwd<64,1|2>, partly filled last
     groups of two and of four, the group loop of both kernels, the register prefetch of several trials through a chunk change
     (T = 66), and either side of H = 64's switch to the batched MFMA path at 384 trials.  Each row restates the plan from cus and
     asserts that it reaches what it is there for: n_slabs of the workspace layout == cus and more trial groups than that where the
     backward must loop, more forward groups than 2 cus where the forward must.
  c. inference at the band rows: logits, probabilities, argmax, and trials 0, B // 2, B - 1 of the batch bit for bit against three
     single-trial calls (the per-trial arithmetic of these kernels does not depend on NB).
  d. the generic route at many trials: a shape no other route takes (H = 40, C = 3, L = 1) and one beyond gen_grid's cap of eight
     workgroups per CU (L = 3 with the residual flag), train step and inference.
  e. one Trainer.step at hidden_size = 32 with cus + 44 trials: explicit masks from nsd_train_masks, two-launch forward, the
     one-trial backward on a second pass, reduce + Adam.

Every case takes fc.0.bias = +-4 (head_inputs(safe=True)) and asserts that the ORACLE's fc.0 pre-activations stay KINK_MARGIN away
from the RReLU kink before it compares gradients.  Every train case runs with all three masks on (L = 1 has no inter-layer dropout).

Bounds: logits 1e-4 (LOGIT_TOL), mean loss 5e-5, alpha / pooled / fc0_pre 5e-5, attn.bias 2e-6 absolute, probabilities 1e-5: the
suite's own.  Gradients: FP32_EXACT (tests/gpu_harness.py), of each tensor's largest element (+1e-7) -- about eight times the worst
value measured over this whole file on one MI355X against the oracle, rounded up to one significant digit (the room FAST48 has), and
no more than FAST48's 5e-5 / 2e-5:
  LSTM weights   wtol = 1e-5   measured 1.25e-6 (weight_ih_l0 of the generic L = 3 case, 2051 trials: 4102 rows summed by one workgroup;
                               the fused H = 32 / 64 kernels: at most 9.6e-7)
  other tensors  rtol = 2e-5   measured 2.25e-6 (attn.weight at T = 2, H = 64) and 2.21e-6 (fc.3.bias at K = 2, T = 65: its two entries
                               are what is left of a sum over the batch that nearly cancels; the oracle itself is 2.7e-6 from float64
                               there, tests/test_fp32_routes_cpu.py); the worst tensor of every other case: at most 1.5e-6
Other worst values of that run: logits 2.9e-6 (train) / 1.4e-6 (inference), probabilities 3.6e-7, mean loss 3.1e-7, alpha 1.2e-7,
pooled 1.1e-6, fc0_pre 4.3e-6, attn.bias 9.7e-9, parameters after the trainer's Adam step 0; every batch-invariance check bit for bit.
T = 1: the oracle's weight_hh (and attn.weight) gradients are exactly zero; the kernels' entries are finite and <= 1e-7 (measured 0).
Wall time of the file on the MI355X: 9 s (39 tests), the CPU oracle included; the slowest case takes 1.8 s.
"""
import functools
import time

import numpy as np
import pytest
import torch

from oracle import nsd_oracle as orc
from tests.golden.make_goldens import synth_labels, synth_params, synth_x
from tests.gpu_harness import (FAST48, FP32_EXACT, HEAD_BRANCH_ROWS, HEAD_TOL, KINK_MARGIN, LOGIT_TOL, PROB_TOL, T_EDGES, assert_step_vs_oracle, cus, dev, grad_class,  # noqa: F401
                               grad_errors, head_inputs, kink_safe, model_from_state, nsd, oracle_step, spec_of, to_dev, train_step)

pytestmark = pytest.mark.gpu

WORST = {}                       # class of number -> (worst value seen in this run, where): printed by the last test
T_START = time.time()


def test_fp32_exact_is_no_looser_than_fast48():
    assert FP32_EXACT["rtol"] <= FAST48["rtol"] and FP32_EXACT["wtol"] <= FAST48["wtol"]


def _note(key, value, where):
    v = float(value)
    if v != v or v >= WORST.get(key, (0.0, ""))[0]:          # (a NaN is noted, and stays)
        WORST[key] = (v, where)


@functools.lru_cache(maxsize=None)
def _inputs(Cc, H, L, K, F, B, T):
    """head_inputs(safe=True) of a shape, shared by the train and the inference case of a row (nothing writes to them)"""
    return head_inputs(Cc, H, K, F, B, T, L=L, safe=True)


def _oracle(d, flat, x, y, masks, residual):
    """the oracle's step; asserts the kink margin on ITS pre-activations first"""
    return oracle_step(d, flat, x, labels=y, masks=masks, residual=residual, kink=KINK_MARGIN)


def _step(dev, d, flat_np, x, y, residual, **masks):
    """the launch sequence of Trainer.step: for these shapes nsd_lstm_fwd + nsd_head_train, nsd_lstm_bwd, nsd_grad_reduce"""
    return train_step(dev, spec_of(d), flat_np, x, labels=y, residual=residual, masks=masks, saves=("alpha", "pooled", "fc0_pre"))


def _note_grad_errors(tag, got_flat, ref_flat, d):
    """error / largest element of the worst tensor per class, against the oracle: what FP32_EXACT is derived from"""
    per, ref = grad_errors(got_flat, ref_flat, d)[0], orc.unflatten(ref_flat, d)
    worst = {"lstm.weight": (0.0, ""), "other": (0.0, "")}
    for k, (err, scale) in per.items():
        cls = grad_class(k)
        if cls == "attn.bias":
            _note("grad attn.bias (abs)", err, tag)
        elif not np.abs(ref[k]).any():                      # exactly zero in the oracle (T = 1): absolute, held by grad_close's 1e-7 floor
            _note("grad of a zero tensor (abs)", err, f"{tag}: {k}")
        else:
            ratio = err / scale
            if ratio != ratio or ratio >= worst[cls][0]:
                worst[cls] = (ratio, k)
            _note(f"grad {cls} / max", ratio, f"{tag}: {k}")
    return worst


def _vs_oracle(tag, d, out, ref, head=True):
    """logits, mean loss, the head's saved intermediates and every gradient tensor of a train step against _oracle's; prints first"""
    logits, grads = out["logits"], out["grads"]
    lerr, serr = float(np.abs(logits - ref["logits"]).max()), abs(out["mean_loss"] - ref["loss"])
    herr = {k: float(np.abs(out[k] - ref["fw"][k]).max()) for k in ("alpha", "pooled", "fc0_pre")} if head else {}
    finite = bool(np.isfinite(logits).all() and np.isfinite(grads).all())
    w = _note_grad_errors(tag, grads, ref["grads"], d) if finite else {}
    print(f"[{tag}] C={d.C} H={d.H} L={d.L} K={d.K} F={d.F} B={logits.shape[0]}: logits {lerr:.2e}  loss {serr:.2e}  "
          + "  ".join(f"{k} {v:.2e}" for k, v in herr.items())
          + "  grads / max: " + "  ".join(f"{c} {v:.2e} ({k})" for c, (v, k) in w.items()))
    assert finite, tag
    _note("logits (abs)", lerr, tag)
    _note("loss (abs)", serr, tag)
    for k, v in herr.items():
        _note(f"{k} (abs)", v, tag)
        assert v < HEAD_TOL, (tag, k, v)
    assert_step_vs_oracle(out, ref, d, FP32_EXACT)


def _infer_vs_oracle(tag, dev, d, flat_np, x, residual):
    """ops.infer against the oracle's eval-mode forward: logits, probabilities (rows summing to 1), argmax where the oracle's top-two
    gap is clear, and trials 0, B // 2, B - 1 of the batch equal to their single-trial runs bit for bit"""
    from nsd_amd import ops
    spec, flat, xt = spec_of(d), to_dev(flat_np, dev), to_dev(x, dev)
    B = x.shape[0]
    lg_t, pr_t = ops.infer(spec, flat, xt, residual=residual)
    lg, pr = lg_t.cpu().numpy(), pr_t.cpu().numpy()
    ref = orc.forward(flat_np, x, d, residual=residual)
    lerr, perr = float(np.abs(lg - ref["logits"]).max()), float(np.abs(pr - ref["probs"]).max())
    singles = [(i, *ops.infer(spec, flat, xt[i:i + 1].contiguous(), residual=residual)) for i in sorted({0, B // 2, B - 1})]
    same = [bool(torch.equal(l1[0], lg_t[i]) and torch.equal(p1[0], pr_t[i])) for i, l1, p1 in singles]
    print(f"[{tag}] C={d.C} H={d.H} L={d.L} K={d.K} F={d.F} B={B}: infer logits {lerr:.2e}  probs {perr:.2e}  "
          f"trials {[i for i, _, _ in singles]} == their single-trial calls: {same}")
    _note("infer logits (abs)", lerr, tag)
    _note("infer probs (abs)", perr, tag)
    assert np.isfinite(lg).all() and np.isfinite(pr).all(), tag
    assert lerr < LOGIT_TOL, (tag, lerr)
    assert perr < PROB_TOL, (tag, perr)
    assert np.abs(pr.sum(1) - 1.0).max() < 1e-5
    srt = np.sort(ref["logits"], axis=1)
    clear = (srt[:, -1] - srt[:, -2]) > 2 * LOGIT_TOL
    assert clear.any() and np.array_equal(lg.argmax(1)[clear], ref["logits"].argmax(1)[clear]), tag
    assert all(same), (tag, [i for (i, _, _), s in zip(singles, same) if not s])


def _fast_path(d, B, T):
    """nsd_fast_path at the batch of the call (ModelSpec.fast_path asks at one trial; H = 64 depends on B)"""
    import ctypes as C
    from nsd_amd import _lib
    dd = spec_of(d).dims(B, T)
    return int(_lib.lib().nsd_fast_path(C.byref(dd)))


# ---------------------------------------------------------------------------------------------------------------------------------
# a. T edges, one trial per workgroup
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc,H,K,F,B,T,residual", T_EDGES)
def test_t_edges_one_trial_per_workgroup_vs_oracle(nsd, dev, cus, Cc, H, K, F, B, T, residual):
    from nsd_amd import ops
    d, flat, x, y, masks = _inputs(Cc, H, 2, K, F, B, T)
    assert B <= cus and _fast_path(d, B, T) == 1 and not ops.rng_path(spec_of(d), B, T)
    assert ops.workspace_layout(spec_of(d), B, T)[1].n_slabs == B            # one workgroup, one slab per trial
    ref = _oracle(d, flat, x, y, masks, residual)
    out = _step(dev, d, flat, x, y, residual, **masks)
    _vs_oracle(f"a T={T} residual={residual}", d, out, ref)
    if T == 1:                                             # h[-1] = 0: exactly zero in the oracle
        g, g_ref = orc.unflatten(out["grads"], d), orc.unflatten(ref["grads"], d)
        for k in ("lstm.weight_hh_l0", "lstm.weight_hh_l1"):
            assert np.abs(g_ref[k]).max() == 0.0
            _note("T=1 max |weight_hh grad|", np.abs(g[k]).max(), k)
            assert np.isfinite(g[k]).all() and np.abs(g[k]).max() <= 1e-7, (k, np.abs(g[k]).max())


# ---------------------------------------------------------------------------------------------------------------------------------
# b. the batch bands
# ---------------------------------------------------------------------------------------------------------------------------------
# (H, C, K, F, (m, a): B = m * cus + a, T, residual, (forward NB, backward NB) or None where the band depends on cus, forward loops,
#  backward loops, fast path)
BANDS = [
    (32, 8, 3, 32, (1, 0), 2, False, (1, 1), False, False, 1),      # the last batch without any loop
    (32, 8, 3, 32, (1, 1), 66, False, (2, 1), False, True, 1),      # fwd<32,2>, last group half filled; bwd<32,1>: workgroup 0 twice; chunk change
    (32, 8, 3, 32, (2, 0), 3, False, (2, 1), False, True, 1),       # two-trial groups, all full
    (32, 7, 5, 7, (2, 1), 5, False, (4, 2), False, True, 1),        # fwd<32,4> last group 1 of 4; bwd<32,2> last group 1 of 2
    (32, 8, 3, 32, (2, 3), 66, True, (4, 2), False, True, 1),       # fwd<32,4> last group 3 of 4; bwd<32,2> cus + 2 groups; chunk change, four trials
    (32, 7, 5, 7, (8, 3), 3, False, (4, 2), True, True, 1),         # forward loop: 2 cus + 1 groups, last 3 of 4; backward: four passes and more
    (64, 8, 3, 32, (1, 3), 66, True, (2, 1), False, True, 1),       # fwd<64,2>; bwd<64,1> loops
    (64, 8, 3, 32, (0, 383), 4, False, None, False, None, 1),       # the last batch of H = 64 on the fused kernels ...
    (64, 8, 3, 32, (0, 384), 4, False, None, False, None, 0),       # ... and the first on the batched MFMA path
    (64, 5, 4, 33, (2, 5), 5, False, (4, 2), False, True, 1),       # C % 4 != 0 keeps the fused kernels: fwd<64,4>, bwd<64,2>
    (64, 5, 4, 33, (2, 5), 66, True, (4, 2), False, True, 1),       # the same through a chunk change (the slow one)
    (64, 6, 3, 32, (8, 5), 2, False, (4, 2), True, True, 1),        # forward loop at H = 64
]


def _band_id(r):
    (m, a) = r[4]
    return f"H{r[0]}-C{r[1]}-B{f'{m}cus+{a}' if m else a}-T{r[5]}" + ("-res" if r[6] else "")


def _plan(B, cus):
    """pick_nb / plan48 / nsd_lstm2_fwd_launch of csrc/nsd_lstm2.hip restated for the first-generation kernels:
    (forward NB, forward groups, forward grid, backward NB, backward groups, backward grid == slabs)"""
    nf = 1 if B <= cus else 2 if B <= 2 * cus else 4
    nb = 1 if B <= 2 * cus else 2
    gf, gb = -(-B // nf), -(-B // nb)
    return nf, gf, min(gf, 2 * cus), nb, gb, min(gb, cus)


@pytest.mark.parametrize("row", BANDS, ids=_band_id)
def test_batch_bands_vs_oracle(nsd, dev, cus, row):
    from nsd_amd import ops
    H, Cc, K, F, (m, a), T, residual, nbs, fwd_loops, bwd_loops, fast = row
    B = m * cus + a
    d, flat, x, y, masks = _inputs(Cc, H, 2, K, F, B, T)
    nf, gf, grid_f, nb, gb, grid_b = _plan(B, cus)
    n_slabs = ops.workspace_layout(spec_of(d), B, T)[1].n_slabs
    print(f"[b {_band_id(row)}] cus={cus} B={B}: fast_path {_fast_path(d, B, T)}  n_slabs {n_slabs}  restated plan: fwd<{H},{nf}> {gf} groups on "
          f"{grid_f} workgroups, bwd<{H},{nb}> {gb} groups on {grid_b}")
    assert _fast_path(d, B, T) == fast
    if fast:
        assert n_slabs == grid_b
        if nbs is not None:
            assert (nf, nb) == nbs, (nf, nb)
        assert (gf > 2 * cus) == fwd_loops
        if bwd_loops is not None:
            assert (gb > cus) == bwd_loops
        if bwd_loops:
            assert n_slabs == cus and gb > cus
    else:
        assert n_slabs == 1                                # the batched path's weight-gradient GEMMs write one slab
    ref = _oracle(d, flat, x, y, masks, residual)
    out = _step(dev, d, flat, x, y, residual, **masks)
    _vs_oracle(f"b {_band_id(row)}", d, out, ref)


# ---------------------------------------------------------------------------------------------------------------------------------
# c. inference at the band rows
# ---------------------------------------------------------------------------------------------------------------------------------
INFER_ROWS = [r for r in BANDS if (r[0], r[4]) in ((32, (1, 1)), (32, (2, 3)), (32, (8, 3)), (64, (1, 3)), (64, (2, 5)))]


@pytest.mark.parametrize("row", INFER_ROWS, ids=_band_id)
def test_inference_in_the_batch_bands_vs_oracle(nsd, dev, cus, row):
    H, Cc, K, F, (m, a), T, residual = row[:7]
    B = m * cus + a
    d, flat, x, _, _ = _inputs(Cc, H, 2, K, F, B, T)
    assert _fast_path(d, B, T) == 1 and _plan(B, cus)[0] == row[7][0]
    _infer_vs_oracle(f"c {_band_id(row)}", dev, d, flat, x, residual)


# ---------------------------------------------------------------------------------------------------------------------------------
# d. the generic route at many trials
# ---------------------------------------------------------------------------------------------------------------------------------
# (C, H, L, K, F, (m, a), T, residual, every kernel's grid loops)
GENERIC = [(3, 40, 1, 3, 32, (1, 44), 5, False, False),     # no other route: H % 16 != 0, C % 4 != 0
           (8, 48, 3, 3, 32, (8, 3), 2, True, True)]        # beyond gen_grid's cap of eight workgroups per CU
GENERIC += HEAD_BRANCH_ROWS                                  # the head launchers' scalar score loop and unstaged sequence


@pytest.mark.parametrize("Cc,H,L,K,F,mb,T,residual,loops", GENERIC, ids=["H40-L1", "H48-L3-res", "H30-scalar-scores", "H60-T560-unstaged"])
def test_generic_route_at_many_trials_vs_oracle(nsd, dev, cus, Cc, H, L, K, F, mb, T, residual, loops):
    from nsd_amd import ops
    B = mb[0] * cus + mb[1]
    d, flat, x, y, masks = _inputs(Cc, H, L, K, F, B, T)
    assert _fast_path(d, B, T) == 0 and not (H % 16 == 0 and H >= 64) and ops.workspace_layout(spec_of(d), B, T)[1].n_slabs == 1
    assert (B > 8 * cus) == loops and ("drop_lstm" in masks) == (L > 1)
    tag = f"d generic H={H} L={L}"
    ref = _oracle(d, flat, x, y, masks, residual)
    out = _step(dev, d, flat, x, y, residual, **masks)
    _vs_oracle(tag, d, out, ref)
    _infer_vs_oracle(tag, dev, d, flat, x, residual)


# ---------------------------------------------------------------------------------------------------------------------------------
# e. the trainer outside the single-launch path
# ---------------------------------------------------------------------------------------------------------------------------------
def test_trainer_step_at_hidden_size_32_matches_oracle_with_its_own_streams(nsd, dev, cus):
    """EEG_LSTM(hidden_size=32): Trainer.step finds nsd_rng_path == 0, fills explicit masks with nsd_train_masks and runs the two-launch
    forward (fwd<32,2>), the one-trial backward on a second pass, reduce + Adam; one step == the oracle's forward / backward with the
    same counter streams + the oracle's Adam"""
    from nsd_amd.trainer import Trainer
    H, K, F = 32, 3, 32
    d = orc.Dims(C=8, H=H, L=2, K=K, F=F)
    state = kink_safe(synth_params(8, H, 2, K, F=F, seed=H + F + K), F)
    m = model_from_state(nsd, dev, state).train()
    tr = Trainer(m, lr=1e-3, seed=7)
    B, T = cus + 44, 12
    x, y = synth_x(B, T, seed=F), synth_labels(B, K=K, seed=K)
    flat0 = orc.flatten_state(state, d)
    tr.step(to_dev(x, dev), to_dev(y, dev))
    assert tr._bufs[(B, T)]["rng_ok"] is False
    masks = dict(drop_lstm=orc.dropout_mask(tr.seed, 4, 0.6, (1, B, T, H)), rrelu_slope=orc.rrelu_noise(tr.seed, 5, (B, F)),
                 drop_head=orc.dropout_mask(tr.seed, 6, 0.6, (B, F)))
    ref = _oracle(d, flat0, x, y, masks, False)
    g = tr.grads.cpu().numpy()
    out = dict(logits=tr._bufs[(B, T)]["logits"].cpu().numpy(), grads=g, mean_loss=tr.last_loss())
    _vs_oracle("e trainer H=32", d, out, ref, head=False)
    p, mm, vv = flat0.copy(), np.zeros_like(flat0), np.zeros_like(flat0)
    orc.adam(p, g, mm, vv, lr=1e-3, step=1)
    perr = float(np.abs(m.flat_parameters().cpu().numpy() - p).max())
    print(f"[e trainer H=32] B={B}: parameters after the step vs the oracle's Adam {perr:.2e}")
    _note("adam (abs)", perr, "e trainer H=32")
    assert perr < 2e-6


# ---------------------------------------------------------------------------------------------------------------------------------
def test_zz_worst_errors_of_this_file(nsd, dev):
    """prints the worst value of every class of number compared above (run the whole file with -s) and the file's wall time"""
    torch.cuda.synchronize()
    print("\nworst errors of tests/test_gpu_fp32_routes.py:")
    for k in sorted(WORST):
        print(f"  {k:28s} {WORST[k][0]:.2e}   {WORST[k][1]}")
    print(f"  FP32_EXACT {FP32_EXACT}")
    print(f"  wall time since import: {time.time() - T_START:.0f} s")
