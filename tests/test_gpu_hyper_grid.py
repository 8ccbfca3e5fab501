"""Per-model step settings on the model-batched H = 48 path: a hyper-parameter grid in the launches one model uses.  Needs the MI355X.

"Bit for bit" is always against the UNIFORM launch of the same M and B through the entry point that existed before, with model m's
setting given to every model: a model's workgroups are the same workgroups in both launches and run the same instructions on the
same data.  (A single-model run dispatches differently; there only MULTI_RTOL holds.)"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.gpu_harness import LOGIT_TOL, LOSS_TOL, D, dev, multi_grad_ok, multi_problem, nsd, soft_targets, spec_of, sync_at_the_end  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBS = [(0.0, 0.0), (0.3, 0.6), (0.6, 0.25)]                     # (p_lstm, p_head): one without dropout, two with p_lstm != p_head


def with_probs(rngs, probs):
    return [dict(r, p_lstm=p[0], p_head=p[1]) for r, p in zip(rngs, probs)]


def raw_step(spec, params, x, y, rngs, dev, *, flag=None, targets=None):
    """nsd_multi_train_fwd(_soft) + nsd_multi_train_bwd + nsd_multi_grad_reduce through the C ABI with the flags given (None: the flag
    goes exactly where the probabilities differ, as ops.multi_train_step passes it) -> logits [M,B,K], loss sums [M], grads [M,P]"""
    from nsd_amd import _lib, ops
    M, B, T = params.shape[0], x.shape[1], x.shape[2]
    d = spec.dims(B, T)
    ws = ops.multi_workspace(spec, M, B, T, dev)
    ws.fill_(float("nan"))
    logits = torch.full((M * B, spec.K), float("nan"), device=dev)
    grads = torch.full_like(params, float("nan"))
    r = ops._rng_array(rngs, M, "test")
    if flag is None:
        flag = _lib.NSD_FLAG_MODEL_P if len({(g["p_lstm"], g["p_head"]) for g in rngs}) > 1 else 0
    rp = C.cast(r, C.c_void_p)
    if targets is None:
        ops._call("nsd_multi_train_fwd", dev, C.byref(d), M, params.data_ptr(), x.data_ptr(), B * T * spec.C, rp, y.data_ptr(), flag, ws.data_ptr(),
                  ws.numel() * 4, logits.data_ptr(), ops.STREAM)
    else:
        ops._call("nsd_multi_train_fwd_soft", dev, C.byref(d), M, params.data_ptr(), x.data_ptr(), B * T * spec.C, rp, targets.data_ptr(), flag,
                  ws.data_ptr(), ws.numel() * 4, logits.data_ptr(), ops.STREAM)
    ops._call("nsd_multi_train_bwd", dev, C.byref(d), M, params.data_ptr(), x.data_ptr(), B * T * spec.C, rp, flag, ws.data_ptr(), ws.numel() * 4,
              ops.STREAM)
    ops._call("nsd_multi_grad_reduce", dev, C.byref(d), M, ws.data_ptr(), ws.numel() * 4, grads.data_ptr(), ops.STREAM)
    loss = ops.multi_loss_sum(spec, ws, M, B, T)
    return logits.view(M, B, spec.K), loss, grads


def probs_for(M):
    return [PROBS[m % 3] for m in range(M)]


# (M, B, T, F, K, models checked, soft targets)
CASES = [(3, 32, 9, 32, 3, None, False),        # one-trial kernels
         (3, 32, 9, 32, 3, None, True),         # ... with soft targets
         (2, 200, 9, 32, 3, None, False),       # two-trial forward, one-trial backward
         (3, 171, 9, 32, 3, None, False),       # four-trial kernels, partial groups in every model
         (25, 32, 9, 32, 3, (0, 12, 24), False),  # four-trial kernels
         (3, 32, 9, 64, 8, None, False)]


@pytest.mark.parametrize("M,B,T,F,K,checked,soft", CASES, ids=[f"M{c[0]}-B{c[1]}-F{c[3]}-K{c[4]}{'-soft' if c[6] else ''}" for c in CASES])
def test_per_model_probabilities_equal_the_uniform_launch_bitwise(nsd, dev, M, B, T, F, K, checked, soft):
    from nsd_amd import _lib, ops
    spec = ops.ModelSpec(C=8, H=48, L=2, K=K, F=F)
    params, x, y, rngs = multi_problem(spec, M, B, T, dev, seed=M * 100 + B + F)
    y = y.contiguous().view(-1)
    tg = torch.from_numpy(soft_targets(M * B, K, seed=5)).to(dev) if soft else None
    probs = probs_for(M)
    lg, ls, gr = raw_step(spec, params, x, y, with_probs(rngs, probs), dev, flag=_lib.NSD_FLAG_MODEL_P, targets=tg)
    assert torch.isfinite(lg).all() and torch.isfinite(gr).all()
    seen = {}
    for m in (checked if checked is not None else range(M)):
        if probs[m] not in seen:                                   # the uniform launch with model m's probabilities, unflagged
            seen[probs[m]] = raw_step(spec, params, x, y, with_probs(rngs, [probs[m]] * M), dev, flag=0, targets=tg)
        lu, su, gu = seen[probs[m]]
        assert torch.equal(lg[m], lu[m]) and torch.equal(ls[m], su[m]) and torch.equal(gr[m], gu[m]), m
    # the probabilities matter: two models' rows differ between two uniform launches
    if len(seen) > 1:
        a, b = list(seen.values())[:2]
        assert not torch.equal(a[0], b[0])
    # the flag with equal probabilities is the unflagged call, all of it
    lu, su, gu = seen[probs[0]]
    lf, sf, gf = raw_step(spec, params, x, y, with_probs(rngs, [probs[0]] * M), dev, flag=_lib.NSD_FLAG_MODEL_P, targets=tg)
    assert torch.equal(lf, lu) and torch.equal(sf, su) and torch.equal(gf, gu)


def test_per_model_probabilities_against_the_oracle(nsd, dev):
    """The check that does not share the model view's code: each model of a flagged (3, 32, 40) launch against the CPU oracle with the
    masks of rng[m] and ITS probabilities regenerated on the host."""
    from oracle import nsd_oracle as orc
    spec = spec_of(D)
    M, B, T = 3, 32, 40
    probs = [(0.0, 0.5), (0.3, 0.0), (0.6, 0.6)]
    params, x, y, rngs = multi_problem(spec, M, B, T, dev, seed=340)
    rngs = with_probs(rngs, probs)
    lg, ls, gr = raw_step(spec, params, x, y.contiguous().view(-1), rngs, dev)
    d = orc.Dims()
    for m in range(M):
        r = rngs[m]
        dl = orc.dropout_mask(r["seed"], r["base_stream"], r["p_lstm"], (1, B, T, 48))
        sl = orc.rrelu_noise(r["seed"], r["base_stream"] + 1, (B, 32))
        dh = orc.dropout_mask(r["seed"], r["base_stream"] + 2, r["p_head"], (B, 32))
        assert (r["p_lstm"] > 0 or (dl == 1.0).all()) and (r["p_head"] > 0 or (dh == 1.0).all())
        loss_ref, g_ref, fw = orc.loss_and_grads(params[m].cpu().numpy(), x[m].cpu().numpy(), y[m].cpu().numpy(), d, drop_lstm=dl,
                                                 rrelu_slope=sl, drop_head=dh)
        err = np.abs(lg[m].cpu().numpy() - fw["logits"]).max()
        print(f"model {m} p {probs[m]}: logits {err:.2e}  loss {abs(float(ls[m]) / B - loss_ref):.2e}")
        assert err < LOGIT_TOL, m
        assert abs(float(ls[m]) / B - loss_ref) < LOSS_TOL, (m, float(ls[m]) / B, loss_ref)
        multi_grad_ok(spec, gr[m].cpu(), torch.from_numpy(np.asarray(g_ref, np.float32)))


# ---- the whole step with per-model settings, through ops ------------------------------------------------------------------------------
def full_step(spec, params, x, y, rngs, augs, mixes, weights, opts, dev, *, zscore=False, step=3):
    """nsd_augment(_each) -> nsd_mixup(_each) -> forward, backward -> nsd_multi_grad_reduce_clip_adam(_each) on clones of the parameters:
    -> dict of logits, grads, p, m, v, records.  augs / mixes / opts: one setting or a list of M; mixes: (mix, smoothing)."""
    from nsd_amd import ops
    M, B, T = params.shape[0], x.shape[-3], x.shape[-2]
    P = spec.param_count
    xa = ops.augment(x, augs, rngs, M=M, zscore=zscore)
    mix = [a for a, _ in mixes] if isinstance(mixes, list) else mixes[0]
    smooth = [e for _, e in mixes] if isinstance(mixes, list) else mixes[1]
    xm, tg = ops.mixup(xa, y, spec.K, rngs, mix=mix, label_smoothing=smooth, class_weights=weights, M=M)
    p, m_, v_ = params.clone(), torch.full_like(params, 1e-4), torch.full_like(params, 1e-7)
    grads = torch.full_like(params, float("nan"))
    ws = ops.multi_workspace(spec, M, B, T, dev)
    state = ops.opt_state(P, M, dev)
    logits = ops.multi_train_step(spec, p, xm, None, ws, grads, rngs=rngs, m=m_, v=v_, step=step, targets=tg, opt=opts, opt_state=state)
    return dict(logits=logits.view(M, B, spec.K).clone(), grads=grads, p=p, m=m_, v=v_, records=ops.opt_records(state, M), x=xm, targets=tg.view(M, B, -1))


def grid_settings(ops):
    augs = [ops.Augment(), ops.Augment(max_shift=3), ops.Augment(scale_range=0.2, noise_std=0.1), ops.Augment(max_shift=2, scale_range=0.1, p_channel=0.2, noise_std=0.3),
            ops.Augment(p_channel=0.3)]
    mixes = [(0.0, 0.0), (0.0, 0.1), (0.5, 0.0), (1.0, 0.2), (0.3, 0.05)]
    sched = ops.LrSchedule(kind="cosine", warmup_steps=2, total_steps=20, min_ratio=0.1)
    opts = [ops.opt_struct(lr=1e-3), ops.opt_struct(lr=3e-3, weight_decay=1e-2), ops.opt_struct(lr=1e-3, max_norm=1e-3),
            ops.opt_struct(lr=2e-3, schedule=sched), ops.opt_struct(lr=1e-3, grad_scale=0.5, schedule=ops.LrSchedule(kind="step", step_size=2, gamma=0.5))]
    return augs, mixes, opts


def test_models_with_their_own_settings_are_isolated(nsd, dev):
    """(5, 32, 24): model 2's probabilities, opt, aug and mix change; every other model's logits, gradients, parameters, m, v and
    record keep their bits -- and each model's bits are those of the uniform launch with its settings."""
    from nsd_amd import ops
    spec = spec_of(D)
    M, B, T = 5, 32, 24
    params, x, y, rngs = multi_problem(spec, M, B, T, dev, seed=524)
    y = y.contiguous().view(-1)
    augs, mixes, opts = grid_settings(ops)
    probs = [PROBS[m % 3] for m in range(M)]
    a = full_step(spec, params, x, y, with_probs(rngs, probs), augs, mixes, None, opts, dev)
    augs2, mixes2, opts2, probs2 = list(augs), list(mixes), list(opts), list(probs)
    augs2[2], mixes2[2], opts2[2], probs2[2] = ops.Augment(max_shift=5, noise_std=0.2), (0.9, 0.3), ops.opt_struct(lr=5e-3, max_norm=0.5), (0.45, 0.1)
    b = full_step(spec, params, x, y, with_probs(rngs, probs2), augs2, mixes2, None, opts2, dev)
    for m in range(M):
        same = all(torch.equal(a[k][m], b[k][m]) for k in ("logits", "grads", "p", "m", "v")) and a["records"][m] == b["records"][m]
        assert same == (m != 2), m
    assert torch.isfinite(a["p"]).all() and not torch.equal(a["p"], params)
    for m in (1, 3):                                              # ... and the uniform launch with model m's settings everywhere
        u = full_step(spec, params, x, y, with_probs(rngs, [probs[m]] * M), augs[m], mixes[m], None, opts[m], dev)
        assert all(torch.equal(a[k][m], u[k][m]) for k in ("logits", "grads", "p", "m", "v")) and a["records"][m] == u["records"][m], m


@pytest.mark.parametrize("Cc,T,zscore", [(3, 11, False), (8, 40, True)])
def test_augment_each_and_mixup_each_equal_their_twins_per_model(nsd, dev, Cc, T, zscore):
    """M = 4, B = 5: one model with everything off, one with only a shift, one with only mix, one with everything on.  Model m's block
    of y and targets is the M = 1 call with its entry, rng[m], its windows and its weight row, bitwise."""
    from nsd_amd import ops
    M, B, K = 4, 5, 3
    g = torch.Generator().manual_seed(Cc * 100 + T)
    x = torch.randn((M, B, T, Cc), generator=g).to(dev)
    y = torch.randint(0, K, (M * B,), generator=g, dtype=torch.int32).to(dev)
    w = (0.5 + torch.rand((M, K), generator=g)).to(dev)
    rngs = [dict(seed=77 + 13 * m, base_stream=4 * (m + 2)) for m in range(M)]
    augs = [ops.Augment(), ops.Augment(max_shift=3), ops.Augment(), ops.Augment(max_shift=2, scale_range=0.25, p_channel=0.3, noise_std=0.4)]
    mix, smooth = [0.0, 0.0, 0.6, 1.0], [0.0, 0.0, 0.0, 0.15]
    step_dev = torch.tensor([7], dtype=torch.int64, device=dev)
    for sd in (None, step_dev):
        ya = ops.augment(x, augs, rngs, M=M, zscore=zscore, step_dev=sd)
        assert ya.shape == x.shape and torch.isfinite(ya).all()
        for m in range(M):
            y1 = ops.augment(x[m].contiguous(), augs[m], rngs[m], zscore=zscore, step_dev=sd)
            assert torch.equal(ya[m], y1), (m, sd is not None)
        if not zscore:
            assert torch.equal(ya[0], x[0]) and torch.equal(ya[2], x[2]) and not torch.equal(ya[1], x[1]) and not torch.equal(ya[3], x[3])
        for weights in (w, None):
            ym, tg = ops.mixup(x, y, K, rngs, mix=mix, label_smoothing=smooth, class_weights=weights, M=M, step_dev=sd)
            for m in range(M):
                y1, t1 = ops.mixup(x[m].contiguous(), y[m * B:(m + 1) * B].contiguous(), K, rngs[m], mix=mix[m], label_smoothing=smooth[m],
                                   class_weights=None if weights is None else weights[m].contiguous(), step_dev=sd)
                assert torch.equal(ym[m], y1) and torch.equal(tg.view(M, B, K)[m], t1), (m, weights is None, sd is not None)
            # mix == 0: a bitwise copy of the windows and un-multiplied (one-hot, here weighted) target rows
            assert torch.equal(ym[0], x[0]) and torch.equal(ym[1], x[1]) and not torch.equal(ym[2], x[2])
            onehot = torch.nn.functional.one_hot(y[:B].long(), K).float()
            assert torch.equal(tg.view(M, B, K)[0], onehot * weights[0] if weights is not None else onehot)
    # the shared-window form (x_model_stride = 0): every model reads model 0's windows, each with its own setting and draws
    shared = x[0].contiguous()
    ya = ops.augment(shared, augs, rngs, M=M, zscore=zscore)
    ym, tg = ops.mixup(shared, y, K, rngs, mix=mix, label_smoothing=smooth, class_weights=w, M=M)
    for m in range(M):
        assert torch.equal(ya[m], ops.augment(shared, augs[m], rngs[m], zscore=zscore)), m
        y1, t1 = ops.mixup(shared, y[m * B:(m + 1) * B].contiguous(), K, rngs[m], mix=mix[m], label_smoothing=smooth[m], class_weights=w[m].contiguous())
        assert torch.equal(ym[m], y1) and torch.equal(tg.view(M, B, K)[m], t1), m
    # lists of equal entries are the twin's launch
    assert torch.equal(ops.augment(x, [augs[3]] * M, rngs, M=M, zscore=zscore), ops.augment(x, augs[3], rngs, M=M, zscore=zscore))


def _tail(spec, ws, grads, p, m_, v_, opt, step, step_dev, state, dev):
    """nsd_multi_grad_reduce_clip_adam (opt: one nsd_opt) or its `_each` twin (opt: a list of M) on the slabs a backward left in ws"""
    from nsd_amd import _lib, ops
    M, B, T = p.shape[0], *ws._bt
    d = spec.dims(B, T)
    each = isinstance(opt, list)
    arr = (_lib.Opt * M)(*opt) if each else opt
    ops._call("nsd_multi_grad_reduce_clip_adam_each" if each else "nsd_multi_grad_reduce_clip_adam", dev, C.byref(d), M, ws.data_ptr(), ws.numel() * 4,
              grads.data_ptr(), p.data_ptr(), m_.data_ptr(), v_.data_ptr(), C.cast(C.pointer(arr), C.c_void_p), step,
              None if step_dev is None else step_dev.data_ptr(), state.data_ptr(), state.numel(), ops.STREAM)


def _tails(spec, ws, params, opt, step, step_dev, dev):
    from nsd_amd import ops
    M = params.shape[0]
    p, m_, v_ = params.clone(), torch.full_like(params, 1e-4), torch.full_like(params, 1e-7)
    grads = torch.full_like(params, float("nan"))
    state = ops.opt_state(spec.param_count, M, dev)
    _tail(spec, ws, grads, p, m_, v_, opt, step, step_dev, state, dev)
    return dict(grads=grads, p=p, m=m_, v=v_, records=ops.opt_records(state, M))


class _Ws:
    """a workspace after a real forward and backward of M models"""

    def __init__(self, spec, params, x, y, rngs, dev):
        from nsd_amd import ops
        M, B, T = params.shape[0], x.shape[1], x.shape[2]
        self.t = ops.multi_workspace(spec, M, B, T, dev)
        self._bt = (B, T)
        ops.multi_train_step(spec, params, x, y, self.t, torch.empty_like(params), rngs=rngs, fuse_adam=False)

    def data_ptr(self):
        return self.t.data_ptr()

    def numel(self):
        return self.t.numel()


def test_clip_adam_each_equals_the_uniform_tail_per_model(nsd, dev):
    """(4, 32, 9) after a real forward and backward; four opt entries: another lr and weight decay, a max_norm small enough to clip,
    cosine with warm-up, a step schedule with another grad_scale.  Host step = 3 and step_dev.  Then a NaN in one model's windows."""
    from nsd_amd import ops
    spec = spec_of(D)
    M, B, T = 4, 32, 9
    params, x, y, rngs = multi_problem(spec, M, B, T, dev, seed=432)
    y = y.contiguous().view(-1)
    opts = [ops.opt_struct(lr=3e-3, weight_decay=1e-2), ops.opt_struct(lr=1e-3, max_norm=1e-3),
            ops.opt_struct(lr=2e-3, schedule=ops.LrSchedule(kind="cosine", warmup_steps=2, total_steps=20, min_ratio=0.1)),
            ops.opt_struct(lr=1e-3, grad_scale=0.5, schedule=ops.LrSchedule(kind="step", step_size=2, gamma=0.5))]
    ws = _Ws(spec, params, x, y, rngs, dev)
    step_dev = torch.tensor([3], dtype=torch.int64, device=dev)
    for sd in (None, step_dev):
        e = _tails(spec, ws, params, opts, 3, sd, dev)
        for m in range(M):
            u = _tails(spec, ws, params, opts[m], 3, sd, dev)
            assert all(torch.equal(e[k][m], u[k][m]) for k in ("grads", "p", "m", "v")) and e["records"][m] == u["records"][m], (m, sd is not None)
        r = e["records"]
        assert 0.0 < r[1]["coef"] < 1.0 and r[0]["coef"] == r[2]["coef"] == r[3]["coef"] == 1.0 and all(q["skipped"] == 0 for q in r)
        assert len({q["lr"] for q in r}) == 4 and abs(r[3]["norm"] - 0.5 * _tails(spec, ws, params, opts[0], 3, sd, dev)["records"][3]["norm"]) < 1e-6 * r[3]["norm"] + 1e-12
        if sd is None:
            host = e
    assert all(torch.equal(host[k], e[k]) for k in ("grads", "p", "m", "v")) and host["records"] == e["records"]      # step_dev = 3 is step = 3
    # a NaN in model 1's windows: its update is skipped and counted, its record says so, the others keep the clean run's bits
    x2 = x.clone()
    x2[1, 3, 2, 1] = float("nan")
    bad = _tails(spec, _Ws(spec, params, x2, y, rngs, dev), params, opts, 3, None, dev)
    for m in range(M):
        if m == 1:
            assert torch.equal(bad["p"][1], params[1]) and float(bad["m"][1].min()) == float(bad["m"][1].max()) == float(np.float32(1e-4))
            assert float(bad["v"][1].min()) == float(bad["v"][1].max()) == float(np.float32(1e-7))
            rec = bad["records"][1]
            assert rec["skipped"] == 1 and rec["coef"] == 0.0 and rec["norm"] != rec["norm"] and rec["lr"] == host["records"][1]["lr"]
        else:
            assert all(torch.equal(bad[k][m], host[k][m]) for k in ("grads", "p", "m", "v")) and bad["records"][m] == host["records"][m], m


def _trainer_models(nsd, dev, drops):
    out = []
    for i, (pl, ph) in enumerate(drops):
        torch.manual_seed(100 + i)
        mdl = nsd.EEG_LSTM().to(dev).train()
        mdl.dropout_p, mdl.head_dropout_p = pl, ph
        out.append(mdl)
    return out


def test_model_batch_trainer_with_per_model_settings(nsd, dev):
    """M = 3, B = 32, T = 40, five steps; lr, weight decay, clip, schedule, augment, loss (one with mixup, one with smoothing only, one
    None) and dropout all differ per model.  Model m's parameters are, bitwise, model m's of a uniform ModelBatchTrainer of the same
    three models and seeds with configuration m everywhere."""
    from nsd_amd import ops
    M, B, T = 3, 32, 40
    g = torch.Generator().manual_seed(63)
    xs = torch.randn((M, B, T, 8), generator=g).to(dev)
    ys = torch.randint(0, 3, (M, B), generator=g, dtype=torch.int32).to(dev)
    seeds = [5, 6, 7]
    drops = [(0.0, 0.0), (0.3, 0.6), (0.6, 0.25)]
    cfg = dict(lr=[1e-3, 3e-3, 2e-3], weight_decay=[0.0, 1e-2, 1e-3], clip_grad_norm=[10.0, 0.05, 1.0],
               lr_schedule=[None, ops.LrSchedule(kind="cosine", warmup_steps=2, total_steps=10, min_ratio=0.1), ops.LrSchedule(kind="step", step_size=2, gamma=0.5)],
               augment=[ops.Augment(max_shift=3, noise_std=0.1), None, ops.Augment(scale_range=0.2, p_channel=0.2)],
               loss=[ops.Loss(mixup=0.5, label_smoothing=0.1), ops.Loss(label_smoothing=0.1, class_weights=(1.0, 2.0, 0.5)), None])
    het_models = _trainer_models(nsd, dev, drops)
    het = nsd.ModelBatchTrainer(het_models, seeds=seeds, **cfg)
    with pytest.raises(nsd.NsdError, match="last_lrs"):
        het.last_lr()
    uni_models = [_trainer_models(nsd, dev, [drops[m]] * M) for m in range(M)]
    uni = [nsd.ModelBatchTrainer(uni_models[m], seeds=seeds, **{k: v[m] for k, v in cfg.items()}) for m in range(M)]
    for _ in range(5):
        het.step(xs, ys)
        for u in uni:
            u.step(xs, ys)
    lrs, norms, skipped, losses = het.last_lrs(), het.last_grad_norms(), het.skipped_steps(), het.last_losses()
    for m in range(M):
        assert torch.equal(het_models[m].flat_parameters(), uni_models[m][m].flat_parameters()), m
        assert torch.equal(het.m[m], uni[m].m[m]) and torch.equal(het.v[m], uni[m].v[m]), m
        assert lrs[m] == uni[m].last_lrs()[m] == uni[m].last_lr() and norms[m] == uni[m].last_grad_norms()[m], m
        assert skipped[m] == uni[m].skipped_steps()[m] == 0 and losses[m] == uni[m].last_losses()[m], m
    assert len(set(lrs)) == 3 and all(np.isfinite(norms)) and torch.isfinite(het.params).all()
    with pytest.raises(nsd.NsdError, match="lr has 2 entries for 3 models"):
        nsd.ModelBatchTrainer(_trainer_models(nsd, dev, drops), lr=[1e-3, 2e-3])


def test_model_batch_trainer_scalars_and_repeated_lists_issue_the_same_calls(nsd, dev):
    """Scalar arguments (and equal dropout) are the calls the trainer always issued; a list that repeats one element is the scalar."""
    from nsd_amd import ops
    M, B, T = 3, 32, 40
    g = torch.Generator().manual_seed(64)
    xs = torch.randn((M, B, T, 8), generator=g).to(dev)
    ys = torch.randint(0, 3, (M, B), generator=g, dtype=torch.int32).to(dev)
    one = dict(lr=2e-3, betas=(0.9, 0.99), eps=1e-7, weight_decay=1e-3, clip_grad_norm=0.5, lr_schedule=ops.LrSchedule(kind="step", step_size=2, gamma=0.5),
               augment=ops.Augment(max_shift=2, noise_std=0.1), loss=ops.Loss(mixup=0.4, label_smoothing=0.1))
    calls = {}

    def run(kw, tag):
        names = calls.setdefault(tag, [])
        models = _trainer_models(nsd, dev, [(0.6, 0.6)] * M)
        tr = nsd.ModelBatchTrainer(models, seeds=[1, 2, 3], **kw)

        class hook:
            def __init__(self, name):
                names.append(name)

            def __enter__(self):
                return self

            def __exit__(self, *a):
                return False
        ops.set_launch_hook(hook)
        try:
            for _ in range(3):
                tr.step(xs, ys)
        finally:
            ops.set_launch_hook(None)
        return tr
    a = run(one, "scalar")
    b = run({k: [v] * M for k, v in one.items()}, "lists")
    assert torch.equal(a.params, b.params) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
    assert calls["scalar"] == calls["lists"] and a.last_lr() == b.last_lr() == b.last_lrs()[0]
    assert calls["scalar"][:5] == ["nsd_augment", "nsd_mixup", "nsd_multi_train_fwd_soft", "nsd_multi_train_bwd", "nsd_multi_grad_reduce_clip_adam"]
    plain = run({}, "plain")
    assert calls["plain"][:3] == ["nsd_multi_train_fwd", "nsd_multi_train_bwd", "nsd_multi_grad_reduce_adam"] and len(calls["plain"]) == 9
    assert torch.isfinite(plain.params).all()


def test_grid_end_to_end_matches_train_concurrent_per_configuration(dev, tmp_path):
    """python -m nsd_amd.grid on the recorded trials, two configurations x three folds, one epoch: exit 0, six fold records, two
    summaries, one `done` line; each configuration's per-fold last-epoch validation accuracy within one validation window of
    `train --kfold 3 --concurrent` with that configuration (the rule of test_train_kfold_concurrent_matches_sequential)."""
    fx = os.path.join(ROOT, "tests", "golden", "recorded_trials.npz")
    common = ["--data", fx, "--kfold", "3", "--epochs", "1", "--batch", "32"]

    def run(module, extra):
        cmd = [sys.executable, "-c", f"import sys, nsd_amd.{module} as t; sys.exit(t.main(sys.argv[1:]))"] + common + extra
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        return [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    out = run("grid", ["--grid", "dropout=0.4,0.6"])
    folds = [r for r in out if "epoch" in r]
    sums = [r for r in out if r.get("summary")]
    done = [r for r in out if r.get("done")]
    assert len(folds) == 6 and len(sums) == 2 and len(done) == 1 and len(out) == 9
    assert [r["config"] for r in sums] == [{"dropout": 0.4}, {"dropout": 0.6}] and done[0]["groups"] == [[0, 1]]
    assert done[0]["selection"] == "best mean over folds: an optimistic estimate, re-estimate on fresh folds"
    assert [r["config_index"] for r in done[0]["ranking"]] == sorted(range(2), key=lambda c: (-sums[c]["acc_val_mean"], c))
    assert done[0]["best"]["train_args"] == ["--dropout", repr(done[0]["best"]["config"]["dropout"])]
    for c, p in enumerate((0.4, 0.6)):
        con = run("train", ["--concurrent", "--dropout", str(p), "--out", str(tmp_path / f"c{c}.pth")])
        ref = {f"fold{r['fold']}": r for r in con if "fold" in r and "done" not in r}
        mine = {r["run"]: r for r in folds if r["config_index"] == c}
        assert sorted(mine) == sorted(ref) == ["fold0", "fold1", "fold2"]
        for k, r in mine.items():
            assert r["config"] == {"dropout": p} and r["concurrent"] is True and r["n_val"] == ref[k]["n_val"]
            print(f"dropout {p} {k}: grid {r['acc_val']} concurrent {ref[k]['acc_val_last_epoch']} (1 / n_val = {1.0 / r['n_val']:.4f})")
            assert abs(r["acc_val"] - ref[k]["acc_val_last_epoch"]) <= 1.0 / r["n_val"] + 1e-9, (p, k, r, ref[k])
        assert sums[c]["acc_val_folds"] == [mine[f"fold{f}"]["acc_val"] for f in range(3)]
