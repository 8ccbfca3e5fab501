"""Backward from any loss and dL/dx on the bf16 sequence path (nsd_seq_train_fwd_logits -> nsd_seq_head_bwd ->
nsd_seq_train_bwd[_dx]) and the module surface built on it.  Needs a real MI355X: run with `pytest -m gpu -s` (every comparison
prints its worst errors).

1. fused-route equivalence: dlogits = (softmax - onehot) / B through the any-loss sequence gives the fused CE route's gradients;
   the logits are the fused route's bit for bit and train_bwd_dx's gradients are train_bwd's bit for bit;
2. Gaussian dlogits: every gradient and dx against float64 autograd of oracle.torch_ref.TorchRefEEG at bf16-rounded x and LSTM
   weights (the bf16 path's precision gap is what is left);
3. dx duality: sum_d <bf16(W_ih0_d), dW_ih0_d> = <bf16(x), dx> -- both sides from one run, free of bf16 noise: a wrong row, trial,
   channel, gate or direction map breaks it;
4. the module: eval forward with grad, saliency, loss() with x.grad, normalize=True, retain_graph, cfg5-sized bidirectional;
5. a NaN sample: what dx and the gradients are then.
"""

import numpy as np
import pytest
import torch

from oracle import nsd_oracle as orc
from oracle.seq_bf16_ref import bf16_round_f32
from oracle.torch_ref import TorchRefEEG
from tests.golden.make_goldens import synth_labels, synth_params, synth_x
from tests.gpu_harness import dev, nsd  # noqa: F401  (fixtures)
from tests.seq_bf16_harness import DUAL_RTOL, EQUIV_RTOL, any_loss, duality, per_tensor, rel

pytestmark = pytest.mark.gpu

# Bounds: about 3x the worst value measured on one MI355X with this file run with -s (measured values beside them); EQUIV_RTOL and
# DUAL_RTOL, which other files use too, are in tests/seq_bf16_harness.py.
REF_RTOL = 2.5e-2                # vs float64 autograd at bf16-rounded x and W, per tensor / max |tensor|: measured 9.2e-3 (normalize,
                                 # grads), 6.8e-3 (normalize, dx), 6.1e-3 (t1, dx), 5.9e-3 (fused_h64, attn.weight)
RNG_SEED, RNG_BASE = 0x5EED0D1, 40

# name -> (C, H, L, K, D, residual, B, T)
SHAPES = {
    "fused_h64":      (8, 64, 2, 5, 1, False, 40, 24),
    "fused_h256":     (8, 256, 2, 5, 1, False, 96, 30),
    "general_l1_bi":  (8, 128, 1, 3, 2, False, 33, 17),     # padding trials: B = 33
    "general_l3_res": (8, 64, 3, 3, 2, True, 70, 9),
    "wide_c40":       (40, 64, 2, 3, 1, False, 200, 7),     # CP = 48
    "tiles64_h256":   (8, 256, 2, 5, 1, False, 1030, 3),    # 64-trial tiles
    "t1":             (8, 128, 2, 3, 1, False, 64, 1),
    "cfg5_t64":       (64, 512, 2, 5, 2, False, 576, 64),   # cfg5's kernels, two launch waves
}
REF_SHAPES = ["fused_h64", "fused_h256", "general_l1_bi", "general_l3_res", "wide_c40", "t1"]   # float64 CPU autograd affordable


def setup(name, dev, rng_on, seed=0):
    from nsd_amd import ops
    C, H, L, K, D, res, B, T = SHAPES[name]
    spec = ops.ModelSpec(C=C, H=H, L=L, K=K, F=ops.FC_HIDDEN, D=D, residual=res)
    st = synth_params(C, H, L, K, seed=500 + H + 7 * L + C + seed, D=D)
    # fc.0.bias = +-4: no fc.0 pre-activation near the RReLU kink, where a bf16-sized change flips the slope (a property of the data,
    # not of the kernels: tests/test_gpu_seqpath_bf16ref.py, kink_safe)
    st["fc.0.bias"] = np.where(np.arange(ops.FC_HIDDEN) % 2 == 0, 4.0, -4.0).astype(np.float32)
    flat = torch.from_numpy(np.concatenate([st[n].ravel() for n in spec.names()]).astype(np.float32)).to(dev)
    x = torch.from_numpy(synth_x(B, T, C=C, seed=B + T + seed)).to(dev)
    y = torch.from_numpy(synth_labels(B, K, seed=B + seed)).to(dev)
    p = 0.4 if rng_on else None
    rng = dict(seed=RNG_SEED, base_stream=RNG_BASE, p_lstm=p, p_head=p) if rng_on else None
    return spec, st, flat, x, y, rng


@pytest.mark.parametrize("rng_on", [False, True])
@pytest.mark.parametrize("name", list(SHAPES))
def test_any_loss_sequence_reproduces_the_fused_cross_entropy(nsd, dev, name, rng_on):
    from nsd_amd import ops
    spec, _, flat, x, y, rng = setup(name, dev, rng_on)
    B, T, _ = x.shape
    ws = ops.seq_workspace(spec, B, T, dev)
    lf = ops.seq_train_fwd(spec, flat, x, y.to(torch.int32), ws, rng=rng).clone()
    gf = ops.seq_train_bwd(spec, flat, ws, B, T, rng=rng).clone()
    assert ops.seq_status(ws) == 0
    ce = lambda lg: (torch.softmax(lg, 1) - torch.nn.functional.one_hot(y.long(), spec.K).float()) / B
    la, _, ga, dx = any_loss(spec, flat, x, ws, ce, rng)
    g_plain = ops.seq_train_bwd(spec, flat, ws, B, T, rng=rng)          # nsd_seq_train_bwd on the same state
    torch.cuda.synchronize()
    assert ops.seq_status(ws) == 0
    errs = per_tensor(spec, ga, gf)
    worst = max(errs.items(), key=lambda kv: kv[1])
    print(f"[{name} rng={rng_on}] grads vs fused: worst {worst[1]:.2e} ({worst[0]})  dx max {dx.abs().max().item():.2e}")
    assert torch.equal(la, lf)                                           # same forward, same streams: same bits
    assert torch.equal(ga, g_plain)                                      # train_bwd_dx's grads are train_bwd's
    assert torch.isfinite(dx).all() and dx.abs().max().item() > 0
    assert worst[1] < EQUIV_RTOL, errs


def ref_autograd(spec, st, x, dlogits, rng, normalize=False):
    """float64 autograd of TorchRefEEG at bf16-rounded x (straight-through) and LSTM weights; explicit masks = the rng streams"""
    C, H, L, K, D = spec.C, spec.H, spec.L, spec.K, spec.D
    B, T, _ = x.shape
    state = {}
    for n, v in st.items():
        t = torch.from_numpy(np.ascontiguousarray(v))
        state[n] = bf16_round_f32(t) if n.startswith("lstm.weight") else t
    m = TorchRefEEG(C, H, L, K, residual=spec.residual, bidirectional=D == 2)
    m.load_reference_state(state)
    m = m.double()
    masks = {}
    if rng is not None:
        p = rng["p_lstm"]
        masks = dict(drop_lstm=torch.from_numpy(orc.dropout_mask(RNG_SEED, RNG_BASE, p, (L - 1, B, T, D * H))).double() if L > 1 else None,
                     rrelu_slope=torch.from_numpy(orc.rrelu_noise(RNG_SEED, RNG_BASE + 1, (B, 32))).double(),
                     drop_head=torch.from_numpy(orc.dropout_mask(RNG_SEED, RNG_BASE + 2, p, (B, 32))).double())
    xr = x.detach().cpu().double().requires_grad_(True)
    z = xr
    if normalize:
        d = z - z.mean(dim=1, keepdim=True)
        z = d / (d.square().mean(dim=1, keepdim=True).sqrt() + 1e-6)
    zb = z + (bf16_round_f32(z.detach().float()).double() - z.detach())   # the kernel's bf16 input copy, straight-through
    torch.set_num_threads(16)
    logits = m(zb, **masks)
    logits.backward(dlogits.detach().cpu().double())
    g = m.reference_named_grads()
    flat = torch.cat([g[n].reshape(-1) for n in spec.names()])
    return logits.detach(), flat, xr.grad


@pytest.mark.parametrize("rng_on", [False, True])
@pytest.mark.parametrize("name", REF_SHAPES)
def test_gaussian_dlogits_and_dx_against_float64_autograd(nsd, dev, name, rng_on):
    from nsd_amd import ops
    spec, st, flat, x, y, rng = setup(name, dev, rng_on, seed=1)
    B, T, _ = x.shape
    ws = ops.seq_workspace(spec, B, T, dev)
    gen = torch.Generator().manual_seed(B + T)
    dlog = torch.randn((B, spec.K), generator=gen).to(dev)
    logits, _, g, dx = any_loss(spec, flat, x, ws, lambda lg: dlog, rng)
    torch.cuda.synchronize()
    assert ops.seq_status(ws) == 0
    rl, rg, rdx = ref_autograd(spec, st, x, dlog, rng)
    errs = per_tensor(spec, g.cpu(), rg)
    worst = max(errs.items(), key=lambda kv: kv[1])
    edx, elg = rel(dx.cpu(), rdx), float((logits.cpu().double() - rl).abs().max())
    print(f"[{name} rng={rng_on}] vs float64: logits {elg:.2e}  grads worst {worst[1]:.2e} ({worst[0]})  dx {edx:.2e}")
    assert worst[1] < REF_RTOL, errs
    assert edx < REF_RTOL, edx


@pytest.mark.parametrize("rng_on", [False, True])
@pytest.mark.parametrize("name", list(SHAPES))
def test_dx_duality_with_the_input_weight_gradient(nsd, dev, name, rng_on):
    from nsd_amd import ops
    spec, _, flat, x, y, rng = setup(name, dev, rng_on, seed=2)
    B, T, _ = x.shape
    ws = ops.seq_workspace(spec, B, T, dev)
    dlog = torch.randn((B, spec.K), generator=torch.Generator().manual_seed(7 + B)).to(dev)
    _, _, g, dx = any_loss(spec, flat, x, ws, lambda lg: dlog, rng)
    diff, scale = duality(spec, flat, x, g, dx)
    # the fused CE route forms the same dx through nsd_seq_train_bwd_dx
    ops.seq_train_fwd(spec, flat, x, y.to(torch.int32), ws, rng=rng)
    dx2 = torch.empty_like(x)
    g2 = ops.seq_train_bwd(spec, flat, ws, B, T, rng=rng, dx=dx2)
    diff2, scale2 = duality(spec, flat, x, g2, dx2)
    torch.cuda.synchronize()
    assert ops.seq_status(ws) == 0
    print(f"[{name} rng={rng_on}] duality {diff / scale:.2e} (any loss)  {diff2 / scale2:.2e} (fused CE)")
    assert diff / scale < DUAL_RTOL and diff2 / scale2 < DUAL_RTOL
    assert scale > 0 and scale2 > 0


def module(nsd, dev, C=8, H=64, L=2, K=5, D=1, normalize=False, seed=0):
    torch.manual_seed(seed)
    m = nsd.EEG_LSTM(C, H, L, K, dropout=0.5, bidirectional=D == 2, normalize=normalize, precision="bf16").to(dev).eval()
    # no fc.0 pre-activation near the RReLU kink (a bf16-sized change would flip the slope: a property of the data)
    with torch.no_grad():
        m.fc[0].bias.copy_(torch.where(torch.arange(32, device=dev) % 2 == 0, 4.0, -4.0))
    return m


def test_module_eval_forward_is_differentiable(nsd, dev):
    """eval m(x) with grad: bitwise the no-grad logits; F.cross_entropy(m(x), y).backward() == loss().backward(); saliency and
    retain_graph; x.grad from loss()"""
    from nsd_amd import ops
    m = module(nsd, dev)
    B, T = 48, 20
    x = torch.from_numpy(synth_x(B, T, seed=11)).to(dev)
    y = torch.from_numpy(synth_labels(B, K=5, seed=11)).to(dev).long()
    with torch.no_grad():
        lg0 = m(x)
    lg = m(x)
    assert lg.requires_grad and torch.equal(lg.detach(), lg0)
    torch.nn.functional.cross_entropy(lg, y).backward()
    g_ce = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    m.loss(x, y)[1].backward()
    g_loss = torch.cat([dict(m.named_parameters())[n].grad.reshape(-1) for n in m.spec.names()])
    errs = per_tensor(m.spec, torch.cat([g_ce[n].reshape(-1) for n in m.spec.names()]), g_loss)
    worst = max((v, n) for n, v in errs.items())
    print(f"[module] F.cross_entropy(m(x)) vs loss(): worst {worst[0]:.2e} ({worst[1]})")
    assert worst[0] < EQUIV_RTOL
    # saliency: x.grad of one class's logits, against float64 autograd
    m.zero_grad(set_to_none=True)
    xs = x.clone().requires_grad_(True)
    out = m(xs)
    out[:, 2].sum().backward(retain_graph=True)
    sal = xs.grad.clone()
    grads1 = {n: p.grad.clone() for n, p in m.named_parameters()}
    st = {n: p.detach().cpu().numpy() for n, p in m.state_dict().items()}
    dl = torch.zeros((B, 5), device=dev); dl[:, 2] = 1.0
    _, _, rdx = ref_autograd(m.spec, st, x, dl, None)
    print(f"[module] saliency vs float64: {rel(sal.cpu(), rdx):.2e}")
    assert rel(sal.cpu(), rdx) < REF_RTOL
    # retain_graph: a second backward on the same graph (same workspace) gives the same bits
    m.zero_grad(set_to_none=True); xs.grad = None
    out[:, 2].sum().backward()
    assert torch.equal(xs.grad, sal)
    for n, p in m.named_parameters():
        assert torch.equal(p.grad, grads1[n]), n
    # loss() fills x.grad; it is the eval node's dx for dlogits = (softmax - onehot) / B
    xl = x.clone().requires_grad_(True)
    m.loss(xl, y)[1].backward()
    assert xl.grad is not None and torch.isfinite(xl.grad).all()
    xe = x.clone().requires_grad_(True)
    torch.nn.functional.cross_entropy(m(xe), y).backward()
    print(f"[module] loss() x.grad vs F.cross_entropy(m(x)) x.grad: {rel(xl.grad, xe.grad):.2e}")
    assert rel(xl.grad, xe.grad) < EQUIV_RTOL
    # train-mode forward still refuses
    with pytest.raises(nsd.NsdError, match="eval"):
        m.train()(x)


def test_module_normalize_and_bidirectional_h512(nsd, dev):
    """normalize=True: dx flows through the z-score node and agrees with float64 autograd of zscore o model; a bidirectional
    H = 512, C = 64 module (cfg5's shape class) gives finite gradients and dx that satisfy the duality identity"""
    from nsd_amd import ops
    m = module(nsd, dev, normalize=True, seed=1)
    B, T = 40, 16
    x = torch.from_numpy(synth_x(B, T, seed=21)).to(dev).requires_grad_(True)
    dl = torch.randn((B, 5), generator=torch.Generator().manual_seed(3)).to(dev)
    m(x).backward(dl)
    st = {n: p.detach().cpu().numpy() for n, p in m.state_dict().items()}
    _, rg, rdx = ref_autograd(m.spec, st, x.detach(), dl, None, normalize=True)
    offs = m.spec.offsets()
    gw = torch.cat([dict(m.named_parameters())[n].grad.reshape(-1) for n in m.spec.names()]).cpu()
    worst = max(per_tensor(m.spec, gw, rg).values())
    print(f"[normalize] grads vs float64 {worst:.2e}  dx {rel(x.grad.cpu(), rdx):.2e}")
    assert worst < REF_RTOL and rel(x.grad.cpu(), rdx) < REF_RTOL
    mb = module(nsd, dev, C=64, H=512, D=2, seed=2)
    B, T = 64, 24
    xb = torch.from_numpy(synth_x(B, T, C=64, seed=22)).to(dev).requires_grad_(True)
    yb = torch.from_numpy(synth_labels(B, K=5, seed=22)).to(dev).long()
    torch.nn.functional.cross_entropy(mb(xb), yb).backward()
    gb = torch.cat([dict(mb.named_parameters())[n].grad.reshape(-1) for n in mb.spec.names()])
    assert torch.isfinite(gb).all() and torch.isfinite(xb.grad).all() and xb.grad.abs().max().item() > 0
    diff, scale = duality(mb.spec, mb.flat_parameters(), xb.detach(), gb, xb.grad)
    print(f"[bidir h512 module] duality {diff / scale:.2e}")
    assert diff / scale < DUAL_RTOL


def test_nan_sample_poisons_only_its_trial(nsd, dev):
    """One NaN sample in trial 3: that trial's logits and dx are NaN, every other trial's dx is finite, the parameter gradients
    (sums over trials) are NaN, and the evaluation reports status bit 2 (value 4)"""
    from nsd_amd import ops
    spec, _, flat, x, y, _ = setup("general_l1_bi", dev, False, seed=3)
    B, T, _ = x.shape
    x[3, 5, 2] = float("nan")
    ws = ops.seq_workspace(spec, B, T, dev)
    dlog = torch.randn((B, spec.K), generator=torch.Generator().manual_seed(5)).to(dev)
    logits, _, g, dx = any_loss(spec, flat, x, ws, lambda lg: dlog, None)
    torch.cuda.synchronize()
    st = ops.seq_status(ws)
    others = torch.ones(B, dtype=torch.bool, device=dev); others[3] = False
    print(f"[nan] status {st}  trial 3 dx non-finite {int((~torch.isfinite(dx[3])).sum())} / {dx[3].numel()}  "
          f"grads non-finite {int((~torch.isfinite(g)).sum())} / {g.numel()}")
    assert st == ops.SEQ_ST_NONFINITE
    assert torch.isnan(logits[3]).all() and torch.isfinite(logits[others]).all()
    assert torch.isnan(dx[3]).all()
    assert torch.isfinite(dx[others]).all()
    assert torch.isnan(g[:spec.offsets()["ln.weight"]]).any()
