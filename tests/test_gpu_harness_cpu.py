"""tests/gpu_harness.py on the host (no GPU, numpy only): the gradient comparator at both sides of every bound and on a NaN, the
oracle's side of a step against orc.loss_and_grads, and the bound table's numbers, literally -- a later loosening has to edit this file.

The reference gradient has 1.0 as the first element of every tensor and 0 elsewhere, so every tensor's scale is exactly 1 and the
bound of a tensor is tol + 1e-7 (attn.bias, one element: 2e-6 absolute).  One zero element of one tensor (attn.bias: its only one)
is moved by a factor f of that bound: 0.9 must pass, 1.1 must fail, in every class of tensor and with both bound sets."""
import numpy as np
import pytest

from oracle import nsd_oracle as orc
from tests import gpu_harness as gh

D = orc.Dims()
BOUNDS = {"FAST48": gh.FAST48, "FP32_EXACT": gh.FP32_EXACT}
# tensor -> (its class, which of the two bounds holds it)
TENSORS = {"lstm.weight_ih_l0": ("lstm.weight", "wtol"), "lstm.weight_hh_l1": ("lstm.weight", "wtol"), "fc.0.weight": ("other", "rtol"),
           "lstm.bias_ih_l0": ("other", "rtol"), "fc.3.bias": ("other", "rtol"), "attn.bias": ("attn.bias", None)}


def _reference():
    ref = {k: np.zeros(s, np.float32) for k, s in orc.param_shapes(D).items()}
    for v in ref.values():
        v.reshape(-1)[0] = 1.0
    return ref


def _perturbed(name, delta):
    """(got, ref) as flat vectors: ref with `delta` added to a zero element of `name` (attn.bias: to its only element)"""
    ref = _reference()
    got = {k: v.copy() for k, v in ref.items()}
    got[name].reshape(-1)[0 if name == "attn.bias" else 1] += np.float32(delta)
    return orc.flatten_state(got, D), orc.flatten_state(ref, D)


def _bound(name, bounds):
    return 2e-6 if name == "attn.bias" else bounds[TENSORS[name][1]] * 1.0 + 1e-7


def test_the_tensors_cover_every_class():
    assert set(TENSORS) <= set(orc.param_names(D)) and orc.param_shapes(D)["attn.bias"] == (1,)
    assert {gh.grad_class(k) for k in TENSORS} == {"lstm.weight", "other", "attn.bias"}
    assert all(gh.grad_class(k) == cls for k, (cls, _) in TENSORS.items())


@pytest.mark.parametrize("name", sorted(TENSORS))
@pytest.mark.parametrize("which", sorted(BOUNDS))
def test_grad_close_separates_either_side_of_the_bound(which, name):
    bounds = BOUNDS[which]
    gh.grad_close(*_perturbed(name, 0.9 * _bound(name, bounds)), D, **bounds)
    with pytest.raises(AssertionError, match=name.replace(".", r"\.")):
        gh.grad_close(*_perturbed(name, 1.1 * _bound(name, bounds)), D, **bounds)
    with pytest.raises(AssertionError, match=name.replace(".", r"\.")):
        gh.grad_close(*_perturbed(name, float("nan")), D, **bounds)


def test_grad_close_without_wtol_holds_the_lstm_weights_to_rtol():
    gh.grad_close(*_perturbed("lstm.weight_hh_l0", 0.9 * (gh.GRAD_RTOL_12 + 1e-7)), D, rtol=gh.GRAD_RTOL_12)
    with pytest.raises(AssertionError):
        gh.grad_close(*_perturbed("lstm.weight_hh_l0", 1.1 * (gh.GRAD_RTOL_12 + 1e-7)), D, rtol=gh.GRAD_RTOL_12)


@pytest.mark.parametrize("name", sorted(TENSORS))
def test_grad_errors_reports_the_perturbed_class_and_nan(name, capsys):
    cls = TENSORS[name][0]
    base = np.float32(1.0 if name == "attn.bias" else 0.0)     # the element that moves
    delta = float(np.float32(base + np.float32(3e-6)) - base)   # ... by this much, exactly
    per, worst = gh.grad_errors(*_perturbed(name, 3e-6), D)
    assert 2.9e-6 < delta < 3.1e-6 and worst == {c: (delta if c == cls else 0.0) for c in ("lstm.weight", "other", "attn.bias")}
    assert per[name] == (delta, 1.0) and all(v == (0.0, 1.0) for k, v in per.items() if k != name)
    per, worst = gh.grad_errors(*_perturbed(name, float("nan")), D)
    assert np.isnan(worst[cls]) and all(v == 0.0 for c, v in worst.items() if c != cls)
    assert np.isnan(per[name][0])
    with pytest.raises(AssertionError):
        gh.grad_close(*_perturbed(name, float("nan")), D, **gh.FAST48)
    assert f"'{cls}': 'nan'" in capsys.readouterr().out         # the "grad_close worst" line says so


def test_worse_keeps_a_nan():
    nan = float("nan")
    assert gh.worse(0.0, 1.0) == 1.0 and gh.worse(1.0, 0.5) == 1.0
    assert np.isnan(gh.worse(0.0, nan)) and np.isnan(gh.worse(nan, 1.0)) and np.isnan(gh.worse(gh.worse(0.0, nan), 2.0))


def test_oracle_step_is_loss_and_grads_and_asserts_the_kink_margin():
    d, flat, x, y, masks = gh.head_inputs(8, 48, 3, 32, 3, 5, safe=True)
    loss, g, fw = orc.loss_and_grads(flat, x, y, d, **masks)
    ref = gh.oracle_step(d, flat, x, labels=y, masks=masks)
    assert ref["loss"] == loss and ref["grads"].tobytes() == g.tobytes() and ref["logits"].tobytes() == fw["logits"].tobytes()
    assert ref["dx"] is None and ref["loss_per_trial"] is None
    with_dx = gh.oracle_step(d, flat, x, labels=y, masks=masks, want_dx=True)
    assert with_dx["grads"].tobytes() == g.tobytes() and with_dx["dx"].shape == x.shape
    margin = gh.kink_margin(fw)
    assert margin > gh.KINK_MARGIN                              # fc.0.bias = +-4
    gh.oracle_step(d, flat, x, labels=y, masks=masks, kink=0.5 * margin)
    with pytest.raises(AssertionError):
        gh.oracle_step(d, flat, x, labels=y, masks=masks, kink=2.0 * margin)


def test_assert_step_vs_oracle_on_the_oracle_itself_and_on_a_nan():
    d, flat, x, y, masks = gh.head_inputs(8, 48, 3, 32, 3, 5, safe=True)
    ref = gh.oracle_step(d, flat, x, labels=y, masks=masks, want_dx=True)
    out = dict(logits=ref["logits"].copy(), grads=ref["grads"].copy(), mean_loss=ref["loss"], dx=ref["dx"].copy())
    errs = gh.assert_step_vs_oracle(out, ref, d, gh.FP32_EXACT)
    assert errs == dict(logits=0.0, loss=0.0, dx=0.0)
    for key, idx in (("logits", (0, 0)), ("grads", 7), ("dx", (0, 0, 0))):
        bad = dict(out, **{key: out[key].copy()})
        bad[key][idx] = np.nan
        with pytest.raises(AssertionError):
            gh.assert_step_vs_oracle(bad, ref, d, gh.FP32_EXACT)
    with pytest.raises(AssertionError):
        gh.assert_step_vs_oracle(dict(out, mean_loss=ref["loss"] + 1.1 * gh.LOSS_TOL), ref, d, gh.FP32_EXACT)
    with pytest.raises(AssertionError):
        gh.assert_step_vs_oracle(dict(out, mean_loss=float("nan")), ref, d, gh.FP32_EXACT)


def test_the_bound_table_is_todays():
    assert gh.LOGIT_TOL == 1e-4 and gh.PROB_TOL == 1e-5 and gh.LOSS_TOL == 5e-5 and gh.HEAD_TOL == 5e-5 and gh.DX_TOL == 2e-5
    assert gh.FAST48 == {"rtol": 2e-5, "wtol": 5e-5} and gh.FP32_EXACT == {"rtol": 2e-5, "wtol": 1e-5}
    assert gh.MULTI_RTOL == 3e-4 and gh.GRAD_RTOL_12 == 2e-4 and gh.GRAD_RTOL_X4 == 3e-4 and gh.GRAD_RTOL_SATURATED == 5e-4
    assert gh.KINK_MARGIN == 1e-4 and gh.KINK == 5e-6
    assert gh.bounds_of(orc.Dims()) is gh.FAST48 and gh.bounds_of(orc.Dims(C=5)) is gh.FAST48
    assert all(gh.bounds_of(d) is gh.FP32_EXACT for d in (orc.Dims(H=32), orc.Dims(H=64), orc.Dims(L=3), orc.Dims(C=9)))
