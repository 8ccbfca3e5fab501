"""The reference tests/test_gpu_fp32_routes.py rests on, pinned on the host (no GPU): the CPU oracle against the float64 torch
restatement of the model (oracle/torch_ref.py) at H = 32 / 64 with the residual flag, with C < 8 and at the T edges of the
first-generation fused kernels (csrc/nsd_lstm2.hip) -- shapes the oracle had never been compared with anything at.

T_EDGES (tests/gpu_harness.py) is the table of section (a) of the GPU file; the rows with T in {1, 2, 33, 65, 97} (all of B <= 7) are compared here, with
the kink-safe fc.0.bias = +-4 the GPU cases use and with the generators' own bias.

Bounds are those of test_oracle_matches_a_float64_restatement_of_the_model (tests/test_head_dims_cpu.py): every gradient tensor within
5e-6 of its largest element (measured here: 1.3e-6 with the generators' bias, 2.7e-6 with +-4 -- fc.3.bias at K = 2, whose two entries
are what is left of a sum over the batch that nearly cancels), attn.bias within 2e-6 absolute
(measured 1.5e-8).  The logits keep that test's 1e-6 with the generators' own bias (measured 2.3e-7); with fc.0.bias = +-4 the fc.0
activations, and with them the logits, are several times larger, the fp32 oracle differs from float64 by up to 2.1e-6 there, and the
bound is 5e-6.  The mean loss is held to twice the logits' bound (measured 6.3e-8 / 2.4e-7).  At T = 1 the recurrent weights see
h[-1] = 0 and the attention's softmax runs over a single step: the gradients of weight_hh and attn.weight are exactly zero in the
restatement, and the oracle's are compared absolutely (<= 1e-7) instead of being divided by a scale of zero.
"""
import numpy as np
import pytest
import torch

from oracle import nsd_oracle as orc
from oracle.torch_ref import TorchRefEEG
from tests.gpu_harness import FP32_EXACT, HEAD_BRANCH_ROWS, KINK_MARGIN, T_EDGES, grad_class, head_inputs, kink_margin

CPU_T = (1, 2, 33, 65, 97)
LOGIT_TOL_OWN_BIAS, LOGIT_TOL_SAFE_BIAS = 1e-6, 5e-6


def test_the_table_covers_what_it_promises():
    for H in (32, 64):
        rows = [r for r in T_EDGES if r[1] == H]
        assert sorted(r[5] for r in rows) == [1, 2, 31, 32, 33, 64, 65, 97]
        assert {r[0] for r in rows} == {8, 7, 5, 1} and {r[6] for r in rows} == {False, True}
        assert all(4 <= r[4] <= 8 for r in rows)
    assert all(r[4] <= 7 for r in T_EDGES if r[5] in CPU_T)


@pytest.mark.parametrize("safe", [True, False], ids=["safe_bias", "own_bias"])
@pytest.mark.parametrize("Cc,H,K,F,B,T,residual", [r for r in T_EDGES if r[5] in CPU_T])
def test_oracle_matches_float64_at_the_fused_kernels_edges(Cc, H, K, F, B, T, residual, safe):
    _oracle_vs_float64(Cc, H, 2, K, F, B, T, residual, safe, rtol=5e-6, wtol=5e-6)


@pytest.mark.parametrize("Cc,H,L,K,F,mb,T,residual,loops", HEAD_BRANCH_ROWS, ids=["H30-scalar-scores", "H60-T560-unstaged"])
def test_oracle_matches_float64_at_the_head_branch_rows(Cc, H, L, K, F, mb, T, residual, loops):
    """the widths of HEAD_BRANCH_ROWS (section d of the GPU file, B = mb[1]): a quarter of FP32_EXACT, which the GPU rows are held to;
    measured 1.8e-7 / 5.2e-7 (H = 30) and 1.1e-7 / 4.1e-7 (H = 60, T = 560) of the largest element, logits 6.2e-7 / 1.0e-6"""
    assert mb[0] == 0
    _oracle_vs_float64(Cc, H, L, K, F, mb[1], T, residual, True, rtol=FP32_EXACT["rtol"] / 4, wtol=FP32_EXACT["wtol"] / 4)


def _oracle_vs_float64(Cc, H, L, K, F, B, T, residual, safe, rtol, wtol):
    """rtol / wtol: every tensor / the LSTM weight gradients, of the tensor's largest element"""
    d, flat, x, y, masks = head_inputs(Cc, H, K, F, B, T, L=L, safe=safe)
    loss, g, fw = orc.loss_and_grads(flat, x, y, d, residual=residual, **masks)
    margin = kink_margin(fw)
    m = TorchRefEEG(Cc, H, L, K, F=F, residual=residual)
    m.load_reference_state({k: torch.from_numpy(v) for k, v in orc.unflatten(flat, d).items()})
    m = m.double()
    t = lambda a: torch.from_numpy(a).double()           # noqa: E731
    logits = m(t(x), t(masks["drop_lstm"]) if L > 1 else None, t(masks["rrelu_slope"]), t(masks["drop_head"]))
    loss64 = torch.nn.functional.cross_entropy(logits, torch.from_numpy(y.astype(np.int64)))
    loss64.backward()
    loss64 = float(loss64.detach())
    lerr = float(np.abs(fw["logits"] - logits.detach().numpy()).max())
    ref = {k: v.detach().numpy() for k, v in m.reference_named_grads().items()}
    got = orc.unflatten(g, d)
    worst, worst_k, zero, ab, bad = 0.0, "", [], 0.0, []
    for k in orc.param_names(d):
        scale = float(np.abs(ref[k]).max())
        err = float(np.abs(got[k] - ref[k].reshape(got[k].shape)).max())
        if k == "attn.bias":                               # analytically zero: both sides are round-off
            ab = err
            if not err < 2e-6:
                bad.append((k, err))
        elif scale == 0.0:                                 # an exactly zero reference tensor: absolute, never divided by its scale
            zero.append(k)
            if not err <= 1e-7:
                bad.append((k, err, scale))
        else:
            if err / scale > worst:
                worst, worst_k = err / scale, k
            if not err <= (wtol if grad_class(k) == "lstm.weight" else rtol) * scale:
                bad.append((k, err, scale))
    print(f"oracle vs float64 C={Cc} H={H} K={K} F={F} B={B} T={T} residual={residual} safe={safe}: logits {lerr:.2e}  "
          f"loss {abs(loss - loss64):.2e}  grads/max {worst:.2e} ({worst_k})  attn.bias {ab:.1e}  kink margin {margin:.1e}  zero tensors {zero}")
    assert not bad, bad
    # T = 1: h[-1] = 0 in both layers, and the softmax over one step is 1 whatever the score
    assert sorted(zero) == (["attn.weight"] + [f"lstm.weight_hh_l{l}" for l in range(L)] if T == 1 else []), zero
    ltol = LOGIT_TOL_SAFE_BIAS if safe else LOGIT_TOL_OWN_BIAS
    assert lerr < ltol, lerr
    assert abs(loss - loss64) < 2 * ltol           # log-sum-exp and the label's logit each move by at most the logits' bound
    assert margin > KINK_MARGIN, margin
