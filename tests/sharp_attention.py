"""Inputs with PEAKED attention, shared by tests/test_sharp_attention_cpu.py and tests/test_gpu_h48_sharp_attention.py.

With the synthetic parameters the attention weights are nearly uniform (log(max alpha / min alpha) <= 0.10 at T = 3..250; the
reference checkpoint reaches 3.0), so the online softmax's rescale, the numerators and every alpha-weighted term of the attention
backward run next to a no-op.  Here `attn.weight` is multiplied by a factor s: s = 100 spreads alpha over e^5 .. e^17 (gradients are
compared there), s = 1000 drives alpha to exact 0 / 1 (logits, probabilities and the loss only: the fp32 oracle's own gradient error
grows there).

Chunks are the pooling waves' own: layer 1 runs two steps behind the 8-step save ring, so chunk c holds the steps 8c - 2 .. 8c + 5.
"""
import numpy as np
import torch

from oracle import nsd_oracle as orc
from oracle.torch_ref import TorchRefEEG
from tests.golden.make_goldens import counter_masks, synth_labels, synth_params, synth_x

S_GRAD, S_SAT = 100.0, 1000.0          # gradients are compared at S_GRAD; S_SAT: logits / probabilities / loss only
SHARP_T = (3, 17, 64, 250)
SHARP_B = 5
PARAM_SEED = 7


def sharp_state(s, C=8, H=48, L=2, K=3, seed=PARAM_SEED):
    """synth_params with attn.weight multiplied by s (name -> fp32 array)"""
    st = dict(synth_params(C, H, L, K, seed=seed))
    st["attn.weight"] = (st["attn.weight"] * np.float32(s)).astype(np.float32)
    return st


def sharp_inputs(B, T, C=8, K=3, H=48):
    """x, labels, soft targets and explicit multipliers of the (B, T) case: the same on the CPU and on the GPU"""
    x, y = synth_x(B, T, C=C, seed=1000 + 7 * B + T), synth_labels(B, K=K, seed=B + T)
    q = (1.5 * np.random.RandomState(31 * B + T).rand(B, K)).astype(np.float32)
    q[1 % B] = 0.0                                            # a row without weight
    dl, sl, dh = counter_masks(B, T, H, 32, seed=3 * B + T)
    return x, y, q, dict(drop_lstm=dl, rrelu_slope=sl, drop_head=dh)


def multi_case(T, M=2, B=SHARP_B):
    """The model-batched case: M sharp models (parameter seeds 7, 8, ..), own windows and labels, in-kernel streams rngs[m] and the same
    streams regenerated on the host (the oracle's counter generators) -> states, x [M,B,T,C], y [M,B], rngs, masks per model"""
    states = [sharp_state(S_GRAD, seed=PARAM_SEED + m) for m in range(M)]
    xs = np.stack([synth_x(B, T, seed=2000 + 31 * m + T) for m in range(M)])
    ys = np.stack([synth_labels(B, seed=50 + m + T) for m in range(M)]).astype(np.int32)
    rngs = [dict(seed=900 + 13 * m, base_stream=4 * (m + 1), p_lstm=0.6, p_head=0.6) for m in range(M)]
    masks = [dict(drop_lstm=orc.dropout_mask(r["seed"], r["base_stream"], 0.6, (1, B, T, 48)),
                  rrelu_slope=orc.rrelu_noise(r["seed"], r["base_stream"] + 1, (B, 32)),
                  drop_head=orc.dropout_mask(r["seed"], r["base_stream"] + 2, 0.6, (B, 32))) for r in rngs]
    return states, xs, ys, rngs, masks


def chunk_of(t):
    return (np.asarray(t) + 2) // 8


def spread(alpha):
    """log(max alpha / min alpha) over the batch (inf where an alpha is exactly 0)"""
    a = np.asarray(alpha, np.float64)
    with np.errstate(divide="ignore"):
        return float(np.max(np.log(a.max(axis=1)) - np.log(a.min(axis=1))))


def chunk_facts(alpha):
    """per trial: (chunk of the largest alpha, last chunk, number of times the running maximum over the chunks rises after the first)"""
    out = []
    for a in np.asarray(alpha, np.float64):
        T = a.size
        ch = chunk_of(np.arange(T))
        cmax = np.array([a[ch == c].max() for c in range(ch[-1] + 1)])
        rises, run = 0, cmax[0]
        for v in cmax[1:]:
            if v > run:
                rises, run = rises + 1, v
        out.append((int(ch[np.argmax(a)]), int(ch[-1]), rises))
    return out


def oracle_alpha(state, x, d=None, **masks):
    d = d or orc.Dims()
    return orc.forward(orc.flatten_state(state, d), x, d, saves=True, **masks)["alpha"]


def f64_step(state, x, *, labels=None, targets=None, masks=None, dims=(8, 48, 2, 3, 32)):
    """The float64 model (oracle.torch_ref.TorchRefEEG in double: unlike StackedTorchEEG it takes the explicit multipliers the GPU
    tests run with; the same ATen LSTM layers; masks=None: eval mode) -> logits, probs,
    batch-mean loss, name -> gradient, dL/dx (gradients only with labels or targets; the soft loss is - sum_k q log softmax / B)."""
    C, H, L, K, F = dims
    m = TorchRefEEG(C, H, L, K, F).double()
    m.load_reference_state({k: torch.from_numpy(np.asarray(v)).double() for k, v in state.items()})
    m.eval()
    xt = torch.from_numpy(np.asarray(x)).double().requires_grad_(labels is not None or targets is not None)
    mk = {k: torch.from_numpy(np.asarray(v)).double() for k, v in (masks or {}).items()}
    logits = m(xt, **mk)
    out = dict(logits=logits.detach().numpy(), probs=torch.softmax(logits, 1).detach().numpy())
    if labels is None and targets is None:
        return out
    lsm = torch.log_softmax(logits, 1)
    if targets is None:
        loss = -lsm[torch.arange(x.shape[0]), torch.from_numpy(np.asarray(labels)).long()].mean()
    else:
        loss = -(torch.from_numpy(np.asarray(targets)).double() * lsm).sum() / x.shape[0]
    loss.backward()
    out.update(loss=float(loss.detach()), grads={k: v.numpy() for k, v in m.reference_named_grads().items()}, dx=xt.grad.numpy())
    return out
