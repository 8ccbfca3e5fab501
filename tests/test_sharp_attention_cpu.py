"""The peaked-attention inputs of tests/sharp_attention.py, measured on the CPU: is the fp32 oracle a good enough reference there, and
do the inputs reach the code they are meant to reach?  No GPU.

tests/test_gpu_h48_sharp_attention.py holds the kernels to the fp32 oracle at the project's bounds (logits 1e-4, probabilities 1e-5,
batch-mean loss 5e-5, LSTM weight gradients 5e-5 and the other tensors 2e-5 of each tensor's largest element, attn.bias 2e-6
absolute, dL/dx 2e-5; the exact-fp32 routes 1e-5 on the LSTM weights).  Here the oracle itself is held to a QUARTER of each bound
against the float64 model (oracle.torch_ref.TorchRefEEG in double, same multipliers) on exactly those inputs -- gradients at s = 100,
logits / probabilities / loss at s = 100 and 1000.  Measured (the lines this file prints): at s = 100 logits <= 4.1e-7, probabilities
<= 5.9e-8, loss <= 1.4e-7, LSTM weight gradients <= 2.2e-6, other tensors <= 1.3e-6, attn.bias <= 7.1e-9, dL/dx <= 2.0e-6; at
s = 1000 logits <= 1.2e-6, probabilities <= 2.5e-7, loss <= 1.8e-7, while the gradients are off by up to 2.9e-5 of the largest
element (alpha is exactly 0 or 1 there, and 1 - alpha is lost), which is why they are not compared at that factor.

Spread of the attention, log(max alpha / min alpha), printed by the last two tests: the synthetic parameters <= 0.09 at
T = 3 .. 250; the reference checkpoint (ref_state) on the same windows <= 3.04 (a trained model: sharper, but alpha never below
1 / 21 of the largest); s = 100: 5.6 .. 16.6 with the training multipliers and 2.7 .. 8.9 in eval mode; s = 1000: 27 .. inf
(alpha = 0 exactly from T = 64).
"""
import numpy as np
import pytest

from oracle import nsd_oracle as orc
from tests import mixup_ref as mr
from tests import sharp_attention as sa

# a quarter of the GPU tests' bounds
Q_LOGIT, Q_PROB, Q_LOSS, Q_W, Q_OTHER, Q_ATTN_B, Q_DX, Q_W_EXACT = 2.5e-5, 2.5e-6, 1.25e-5, 1.25e-5, 5e-6, 5e-7, 5e-6, 2.5e-6


def _grad_errors(g_flat, ref, d):
    got = orc.unflatten(g_flat, d)
    w = o = 0.0
    for k in orc.param_names(d):
        if k == "attn.bias":
            continue
        r = float(np.abs(got[k] - ref[k]).max()) / max(float(np.abs(ref[k]).max()), 1e-6)
        w, o = (max(w, r), o) if k.startswith("lstm.weight") else (w, max(o, r))
    return w, o, float(np.abs(got["attn.bias"] - ref["attn.bias"]).max())


def _oracle_step(flat, x, d, masks, labels=None, targets=None):
    fw = orc.forward(flat, x, d, saves=True, **masks)
    if targets is None:
        loss, dl = orc.ce_loss(fw["logits"], labels)
    else:
        per, dl = mr.soft_ce(fw["logits"], targets, 1.0 / x.shape[0])
        loss = float(np.sum(per)) / x.shape[0]
    g, dx = orc.backward(flat, x, d, fw, np.asarray(dl, np.float32), want_dx=True, **masks)
    return fw, loss, g, dx


@pytest.mark.parametrize("B", [5, 6])
@pytest.mark.parametrize("T", sa.SHARP_T)
def test_oracle_is_within_a_quarter_of_each_bound_of_the_float64_model(T, B):
    d = orc.Dims()
    x, y, q, masks = sa.sharp_inputs(B, T)
    for s in (sa.S_GRAD, sa.S_SAT):
        st = sa.sharp_state(s)
        flat = orc.flatten_state(st, d)
        # eval mode (ops.infer / ops.multi_infer)
        ev, ev64 = orc.forward(flat, x, d), sa.f64_step(st, x)
        e_l, e_p = float(np.abs(ev["logits"] - ev64["logits"]).max()), float(np.abs(ev["probs"] - ev64["probs"]).max())
        print(f"s={s:g} T={T} B={B} eval: logits {e_l:.2e} probs {e_p:.2e}")
        assert e_l < Q_LOGIT and e_p < Q_PROB
        for kind, tgt in (("hard", dict(labels=y)), ("soft", dict(targets=q))):
            fw, loss, g, dx = _oracle_step(flat, x, d, masks, **tgt)
            r = sa.f64_step(st, x, masks=masks, **tgt)
            e_l, e_s = float(np.abs(fw["logits"] - r["logits"]).max()), abs(loss - r["loss"])
            w, o, ab = _grad_errors(g, r["grads"], d)
            e_dx = float(np.abs(dx - r["dx"]).max()) / float(np.abs(r["dx"]).max())
            print(f"s={s:g} T={T} B={B} {kind}: spread {sa.spread(fw['alpha']):.1f} logits {e_l:.2e} loss {e_s:.2e} "
                  f"lstm.weight {w:.2e} other {o:.2e} attn.bias {ab:.2e} dx {e_dx:.2e}")
            assert e_l < Q_LOGIT and e_s < Q_LOSS
            if s == sa.S_GRAD:
                assert w < Q_W and o < Q_OTHER and ab < Q_ATTN_B and e_dx < Q_DX


@pytest.mark.parametrize("T", sa.SHARP_T)
def test_oracle_vs_float64_on_the_model_batched_case(T):
    """both models of sharp_attention.multi_case with the streams of their rngs; the second model in eval mode at both factors too"""
    d = orc.Dims()
    states, xs, ys, _, masks = sa.multi_case(T)
    for m, st in enumerate(states):
        flat = orc.flatten_state(st, d)
        fw, loss, g, _ = _oracle_step(flat, xs[m], d, masks[m], labels=ys[m])
        r = sa.f64_step(st, xs[m], labels=ys[m], masks=masks[m])
        w, o, ab = _grad_errors(g, r["grads"], d)
        print(f"model {m} T={T}: spread {sa.spread(fw['alpha']):.1f} lstm.weight {w:.2e} other {o:.2e} attn.bias {ab:.2e}")
        assert sa.spread(fw["alpha"]) > 4.0
        assert float(np.abs(fw["logits"] - r["logits"]).max()) < Q_LOGIT and abs(loss - r["loss"]) < Q_LOSS
        assert w < Q_W and o < Q_OTHER and ab < Q_ATTN_B
    x = sa.sharp_inputs(sa.SHARP_B, T)[0]
    for s in (sa.S_GRAD, sa.S_SAT):
        st = sa.sharp_state(s, seed=sa.PARAM_SEED + 1)
        ev, ev64 = orc.forward(orc.flatten_state(st, d), x, d), sa.f64_step(st, x)
        assert float(np.abs(ev["logits"] - ev64["logits"]).max()) < Q_LOGIT and float(np.abs(ev["probs"] - ev64["probs"]).max()) < Q_PROB


@pytest.mark.parametrize("H", [32, 40])
def test_oracle_vs_float64_on_the_exact_fp32_routes_cases(H):
    """the H = 32 fast-path and the generic-path (H = 40) case of the GPU file: T = 64, B = 5, s = 100, FP32_EXACT's quarter"""
    d = orc.Dims(H=H)
    st = sa.sharp_state(sa.S_GRAD, H=H)
    flat = orc.flatten_state(st, d)
    x, y, _, masks = sa.sharp_inputs(5, 64, H=H)
    fw, loss, g, _ = _oracle_step(flat, x, d, masks, labels=y)
    r = sa.f64_step(st, x, labels=y, masks=masks, dims=d.tup)
    w, o, ab = _grad_errors(g, r["grads"], d)
    print(f"H={H}: spread {sa.spread(fw['alpha']):.1f} lstm.weight {w:.2e} other {o:.2e} attn.bias {ab:.2e}")
    assert sa.spread(fw["alpha"]) > 5.0
    assert float(np.abs(fw["logits"] - r["logits"]).max()) < Q_LOGIT and abs(loss - r["loss"]) < Q_LOSS
    assert w < Q_W_EXACT and o < Q_OTHER and ab < Q_ATTN_B


def test_inputs_reach_the_rescale_and_both_ends_of_the_chunk_walk():
    """Conditions on the INPUTS at s = 100 (with the training multipliers and in eval mode): somewhere in the cases there is a trial
    whose largest alpha lies in the first 8-step chunk, one whose largest alpha lies in the last, partial chunk, and one whose running
    maximum over the chunks rises at least three times (scale = exp(mrun - mnew) < 1 three times); the spread is what the docstring
    of tests/sharp_attention.py says."""
    for mode in ("train", "eval"):
        first = last = rises = False
        for T in sa.SHARP_T:
            x, _, _, masks = sa.sharp_inputs(sa.SHARP_B, T)
            al = sa.oracle_alpha(sa.sharp_state(sa.S_GRAD), x, **(masks if mode == "train" else {}))
            print(f"{mode} T={T}: spread {sa.spread(al):.1f}; facts {sa.chunk_facts(al)}")
            assert sa.spread(al) > (2.0 if T < 8 else 4.0), (mode, T)
            sat = sa.oracle_alpha(sa.sharp_state(sa.S_SAT), x, **(masks if mode == "train" else {}))
            print(f"   s = 1000: spread {sa.spread(sat):.1f}, largest alpha {float(sat.max()):.6f}")
            assert sa.spread(sat) > 20.0, (mode, T)
            for am, lc, r in sa.chunk_facts(al):
                partial = (T + 2) % 8 != 0
                first |= lc > 0 and am == 0
                last |= lc > 0 and partial and am == lc
                rises |= r >= 3
        assert first and last and rises, (mode, first, last, rises)


def test_spread_of_the_parameters_the_other_tests_use(ref_state):
    """The synthetic parameters' alpha is within e^0.3 of uniform at T = 3 .. 250; the reference checkpoint's is printed (and recorded
    in this file's docstring): it is a trained model and spreads alpha further, but rescales by no less than e^-3 = 0.05."""
    worst = {"synthetic": 0.0, "checkpoint": 0.0}
    for T in sa.SHARP_T:
        x = sa.sharp_inputs(sa.SHARP_B, T)[0]
        for name, st in (("checkpoint", ref_state), ("synthetic", sa.sharp_state(1.0))):
            worst[name] = max(worst[name], sa.spread(sa.oracle_alpha(st, x)))
    print("log(max alpha / min alpha), eval mode, T = 3 .. 250:", {k: f"{v:.2f}" for k, v in worst.items()})
    assert worst["synthetic"] < 0.3
