"""Sharpness-aware minimisation on the MI355X (nsd_sam, include/nsd.h): the ascent bit for bit against tests/sam_ref.py on every route,
the non-finite case, pass 2 as a lone pass, its gradient against the oracle, the unchanged tail, the trainers (eager, hipGraph replay,
model-batched with per-model rho), the bf16 sequence path and the buffer contract of the three entry points.  Everything goes
through the C ABI / nsd_amd.ops."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from tests import buffer_contract as bc
from tests import sam_ref
from tests.golden.make_goldens import synth_labels, synth_x
from tests.gpu_harness import (BASE_SHAPES, assert_step_vs_oracle, bounds_of, dev, head_inputs, multi_problem, nsd, oracle_step,  # noqa: F401
                               spec_of, sync_at_the_end, to_dev)

pytestmark = pytest.mark.gpu

LR = 1e-3
NAN = float("nan")


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """bit for bit (NaN payloads and signed zeros included)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _words(t) -> np.ndarray:
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


def _sam_state(ops, n, M, dev):
    """a sam_state whose rows hold NaN words: an element the ascent leaves unwritten shows"""
    st = ops.sam_state(n, M, dev)
    bc.fill_payload(st[16 * M:], "nan32")
    return st


def _check_row(ops, state, M, i, n, p, g, rho, gscale=1.0, tag=None):
    """row i and record i of a sam_state against sam_ref.ascend from the gradient the call left"""
    row = ops.sam_rows(state, M, n)[i]
    want, rec = sam_ref.ascend(p.cpu().numpy(), g.cpu().numpy(), rho, gscale)
    got = ops.sam_records(state, M)[i]
    assert np.array_equal(_words(row), _words(want)), (tag, int((_words(row) != _words(want)).sum()))
    assert got["scale"] == rec["scale"] and got["nonfinite"] == rec["nonfinite"], (tag, got, rec)
    assert got["norm"] == rec["norm"] or abs(got["norm"] - rec["norm"]) <= 2.0 ** -23 * rec["norm"], (tag, got, rec)   # (S in another order)
    return got


# ---- the fused route: one real forward + backward, then the ascent from its slabs -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _evaluated(shape, safe=False):
    """a shape's inputs and, on the device, the workspace after forward + backward with the gradient nsd_grad_reduce leaves"""
    from nsd_amd import ops
    Cc, H, K, F, B, T = shape
    dev = torch.device("cuda:0")
    d, flat, x, y, masks = head_inputs(Cc, H, K, F, B, T, safe=safe)
    spec = spec_of(d)
    ws, logits, g = ops.new_workspace(spec, B, T, dev), torch.empty((B, K), device=dev), torch.full((spec.param_count,), NAN, device=dev)
    mk = {k: to_dev(v, dev) for k, v in masks.items()}
    ops.train_step_grads(spec, to_dev(flat, dev), to_dev(x, dev), ws, to_dev(y.astype(np.int32), dev), logits, g, **mk)
    torch.cuda.synchronize()
    return dict(d=d, spec=spec, P=spec.param_count, B=B, T=T, flat=flat, x=x, y=y.astype(np.int32), masks=masks, mk=mk, ws=ws, g=g)


@pytest.mark.parametrize("shape", [BASE_SHAPES[0], BASE_SHAPES[2]], ids=["P31764", "F33-K9"])
@pytest.mark.parametrize("rho,gscale", [(0.05, 1.0), (0.2, 1.0 / 3.0), (0.0, 1.0)])
def test_ascent_from_the_slabs(nsd, dev, shape, rho, gscale):
    """BASE_SHAPES[0]: P = 31 764, 993 partial sums (more than one round of the 256-thread loop over them); F = 33 / K = 9: P no
    multiple of 32.  grads bitwise nsd_grad_reduce's, p untouched, row and record sam_ref's"""
    from nsd_amd import ops
    e = _evaluated(shape)
    spec, P = e["spec"], e["P"]
    assert (P == 31764 and (P + 31) // 32 == 993) if shape == BASE_SHAPES[0] else P % 32 != 0
    p = to_dev(e["flat"], dev)
    p[5] = -0.0
    p0, ws0 = p.clone(), e["ws"].clone()
    g, ostate, sstate = torch.full((P,), NAN, device=dev), ops.opt_state(P, 1, dev), _sam_state(ops, P, 1, dev)
    ops.sam_ascend(spec, e["ws"], e["B"], e["T"], g, p, ops.Sam(rho), ostate, sstate, grad_scale=gscale)
    assert _same(g, e["g"]) and _same(p, p0) and _same(e["ws"], ws0)
    rec = _check_row(ops, sstate, 1, 0, P, p, g, rho, gscale, (shape, rho))
    row = ops.sam_rows(sstate, 1, P)[0]
    if rho == 0:
        assert _same(row, p) and rec["scale"] == 0.0 and _words(row)[5] == 0x80000000
    else:
        moved = float((row.double() - p.double()).norm())
        print(f"[ascent] {shape} rho {rho}: |p_adv - p| {moved:.6f}  norm {rec['norm']:.4e}  scale {rec['scale']:.4e}")
        assert abs(moved - rho) < 1e-5 and not _same(row, p)
    assert int(ostate[:16].max()) == 0                                   # the tail's record is the tail's


# ---- the flat route ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 2048 * 256 + 1])
def test_ascent_from_a_flat_gradient(nsd, dev, n):
    """one thread, the edges of a block, and one element past what 2048 blocks take in one grid-stride round"""
    from nsd_amd import ops
    rs = np.random.RandomState(n % 9973)
    p, g = to_dev(rs.uniform(-1, 1, n).astype(np.float32), dev), to_dev(rs.standard_normal(n).astype(np.float32), dev)
    p[0] = -0.0
    p0, g0 = p.clone(), g.clone()
    for rho, gscale in ((0.05, 1.0), (0.2, 0.125), (0.0, 1.0)):
        ostate, sstate = ops.opt_state(n, 1, dev), _sam_state(ops, n, 1, dev)
        ops.sam_ascend_flat(p, g, ops.Sam(rho), ostate, sstate, grad_scale=gscale)
        assert _same(p, p0) and _same(g, g0)
        _check_row(ops, sstate, 1, 0, n, p, g, rho, gscale, (n, rho))
        if rho == 0:
            assert _same(ops.sam_rows(sstate, 1, n)[0], p)


# ---- M models ------------------------------------------------------------------------------------------------------------------------
BB, TB = 2, 4


@functools.lru_cache(maxsize=None)
def _batched(M):
    """M models after one forward + backward: the workspace keeps every model's slabs"""
    from nsd_amd import _lib, ops
    dev, spec = torch.device("cuda:0"), ops.ModelSpec()
    params, x, y, rngs = multi_problem(spec, M, BB, TB, dev, seed=M)
    ws, grads = ops.multi_workspace(spec, M, BB, TB, dev), torch.empty_like(params)
    ops.multi_train_step(spec, params, x, y.contiguous().view(-1), ws, grads, rngs=rngs, fuse_adam=False)
    lay, d = _lib.WsLayout(), spec.dims(BB, TB)
    assert _lib.lib().nsd_multi_workspace_bytes(C.byref(d), M, C.byref(lay)) > 0
    torch.cuda.synchronize()
    return dict(spec=spec, P=spec.param_count, params=params, x=x, y=y, rngs=rngs, ws=ws, grads=grads, lay=lay)


def _single_ws(ops, dev, b, M, mdl):
    """a single-model workspace that holds model mdl's slabs (at these sizes either launch writes one LSTM slab per trial)"""
    spec, lay, ws = b["spec"], b["lay"], b["ws"]
    nb, one = ops.workspace_layout(spec, BB, TB)
    assert one.n_slabs == BB and lay.n_slabs == M * BB
    p_lstm = spec.offsets()["ln.weight"]
    stride, ph = (p_lstm + 3) // 4 * 4, b["P"] - p_lstm
    w1 = torch.full((nb // 4,), NAN, device=dev)
    w1[one.slabs:one.slabs + BB * stride] = ws[lay.slabs + mdl * BB * stride:lay.slabs + (mdl + 1) * BB * stride]
    w1[one.hslabs:one.hslabs + BB * ph] = ws[lay.hslabs + mdl * BB * ph:lay.hslabs + (mdl + 1) * BB * ph]
    return w1


@pytest.mark.parametrize("each", [True, False])
def test_models_in_the_same_two_launches(nsd, dev, each):
    """M = 3, rho = [0.05, 0, 0.2] with a grad_scale of its own per model (each), or one setting for all: every row is the single-model
    call's on that model's slabs and sam_ref's; the rho = 0 row is p, a planted -0.0 included"""
    from nsd_amd import ops
    M = 3
    b = _batched(M)
    spec, P = b["spec"], b["P"]
    rhos, gss = ([0.05, 0.0, 0.2], [1.0, 0.5, 1.0 / 3.0]) if each else ([0.1] * M, [0.25] * M)
    p = b["params"].clone()
    p[:, 7] = -0.0
    p0, ws0 = p.clone(), b["ws"].clone()
    g, ostate, sstate = torch.full((M, P), NAN, device=dev), ops.opt_state(P, M, dev), _sam_state(ops, P, M, dev)
    sams = [ops.Sam(r) if r else None for r in rhos]
    ops.multi_sam_ascend(spec, b["ws"], BB, TB, g, p, sams if each else sams[0], ostate, sstate, grad_scale=gss if each else gss[0])
    assert _same(g, b["grads"]) and _same(p, p0) and _same(b["ws"], ws0)
    rows = ops.sam_rows(sstate, M, P)
    for i in range(M):
        _check_row(ops, sstate, M, i, P, p[i], g[i], rhos[i], gss[i], (each, i))
        g1, o1, s1 = torch.full((P,), NAN, device=dev), ops.opt_state(P, 1, dev), _sam_state(ops, P, 1, dev)
        ops.sam_ascend(spec, _single_ws(ops, dev, b, M, i), BB, TB, g1, p[i].clone(), sams[i], o1, s1, grad_scale=gss[i])
        assert _same(g1, g[i]) and _same(ops.sam_rows(s1, 1, P)[0], rows[i]) and torch.equal(s1[:16], sstate[16 * i:16 * i + 16]), (each, i)
    if each:
        assert _same(rows[1], p[1]) and _words(rows[1])[7] == 0x80000000 and not _same(rows[0], p[0]) and not _same(rows[2], p[2])


# ---- 2. a non-finite gradient ------------------------------------------------------------------------------------------------------------
def test_a_non_finite_gradient_copies_and_the_tail_skips(nsd, dev):
    from nsd_amd import ops
    e = _evaluated(BASE_SHAPES[0])
    spec, P, B, T = e["spec"], e["P"], e["B"], e["T"]
    _, lay = ops.workspace_layout(spec, B, T)
    ws = e["ws"].clone()
    ws[lay.slabs + 77] = float("inf")                                   # slab 0, LSTM column 77
    p = to_dev(e["flat"], dev)
    p[3] = -0.0
    p0 = p.clone()
    g, ostate, sstate = torch.full((P,), NAN, device=dev), ops.opt_state(P, 1, dev), _sam_state(ops, P, 1, dev)
    for n in (1, 2):
        ops.sam_ascend(spec, ws, B, T, g, p, ops.Sam(0.05), ostate, sstate)
        rec = ops.sam_records(sstate)[0]
        assert _same(ops.sam_rows(sstate, 1, P)[0], p0) and _same(p, p0) and rec["nonfinite"] == n and rec["scale"] == 0.0
        assert not math.isfinite(rec["norm"]) and math.isinf(float(g[77]))
    # the step's tail on the same slabs (a non-finite pass 2): skipped and counted as it is today
    m, v = torch.zeros(P, device=dev), torch.zeros(P, device=dev)
    adam = dict(m=m, v=v, opt=ops.opt_struct(lr=LR), opt_state=ostate, step=1)
    d = spec.dims(B, T)
    ops._call("nsd_grad_reduce_clip_adam", dev, C.byref(d), ws.data_ptr(), ops._nbytes(ws), g.data_ptr(), p.data_ptr(), m.data_ptr(), v.data_ptr(),
              C.byref(adam["opt"]), 1, None, ostate.data_ptr(), ops._nbytes(ostate), ops.STREAM)
    orec = ops.opt_records(ostate)[0]
    assert _same(p, p0) and float(m.abs().max()) == 0.0 and float(v.abs().max()) == 0.0 and orec["skipped"] == 1 and orec["coef"] == 0.0
    # and a finite ascent afterwards moves again; the counter is sticky
    ops.sam_ascend(spec, e["ws"], B, T, g, p, ops.Sam(0.05), ostate, sstate)
    rec = ops.sam_records(sstate)[0]
    assert rec["nonfinite"] == 2 and rec["scale"] > 0 and not _same(ops.sam_rows(sstate, 1, P)[0], p0)


# ---- 3. pass 2 is a lone pass ---------------------------------------------------------------------------------------------------------
def _slab_regions(ops, spec, B, T, ws):
    nb, lay = ops.workspace_layout(spec, B, T)
    p_lstm = spec.offsets()["ln.weight"]
    stride, ph = (p_lstm + 3) // 4 * 4, spec.param_count - p_lstm
    return ws[lay.slabs:lay.slabs + lay.n_slabs * stride], ws[lay.hslabs:lay.hslabs + B * ph], ops.ws_view(ws, spec, B, T, "loss")


@pytest.mark.parametrize("streams", ["rng", "masks"])
def test_pass_two_is_a_lone_pass(nsd, dev, streams):
    """B = 6: forward + backward at p, the ascent, forward + backward at p_adv in the SAME workspace, against the same calls at a copy of
    p_adv in a fresh workspace full of NaN: slabs, loss, logits and the reduced gradient bit for bit -- nothing accumulates across calls.
    With rho = 0 the second pass reproduces the first."""
    from nsd_amd import ops
    e = _evaluated(BASE_SHAPES[0])
    spec, P, B, T = e["spec"], e["P"], e["B"], e["T"]
    kw = dict(rng=dict(seed=99, base_stream=8, p_lstm=0.6, p_head=0.6)) if streams == "rng" else dict(e["mk"])
    p, x, y = to_dev(e["flat"], dev), to_dev(e["x"], dev), to_dev(e["y"], dev)
    for rho in (0.05, 0.0):
        ws, lg, g = ops.new_workspace(spec, B, T, dev), torch.empty((B, spec.K), device=dev), torch.full((P,), NAN, device=dev)
        ws.fill_(NAN)
        ostate, sstate = ops.opt_state(P, 1, dev), _sam_state(ops, P, 1, dev)
        ops.train_step_grads(spec, p, x, ws, y, lg, g, **kw)
        first = [t.clone() for t in _slab_regions(ops, spec, B, T, ws)] + [lg.clone(), g.clone()]
        ops.sam_ascend(spec, ws, B, T, g, p, ops.Sam(rho), ostate, sstate)
        row = ops.sam_rows(sstate, 1, P)[0]
        ops.train_step_grads(spec, row, x, ws, y, lg, g, **kw)
        second = list(_slab_regions(ops, spec, B, T, ws)) + [lg, g]
        ws2, lg2, g2 = torch.full_like(ws, NAN), torch.full_like(lg, NAN), torch.full_like(g, NAN)
        ops.train_step_grads(spec, row.clone(), x, ws2, y, lg2, g2, **kw)
        lone = list(_slab_regions(ops, spec, B, T, ws2)) + [lg2, g2]
        assert all(_same(a, b) for a, b in zip(second, lone)), (streams, rho)
        assert bool(torch.isfinite(g).all())
        assert all(_same(a, b) for a, b in zip(second, first)) == (rho == 0.0), (streams, rho)


def test_pass_two_of_a_model_batch_is_a_lone_pass(nsd, dev):
    from nsd_amd import ops
    M = 3
    b = _batched(M)
    spec, P = b["spec"], b["P"]
    y = b["y"].contiguous().view(-1)
    ws, g = torch.full_like(b["ws"], NAN), torch.full((M, P), NAN, device=dev)
    ostate, sstate = ops.opt_state(P, M, dev), _sam_state(ops, P, M, dev)
    lg1 = ops.multi_train_step(spec, b["params"], b["x"], y, ws, g, rngs=b["rngs"], fuse_adam=False).clone()
    g1 = g.clone()
    ops.multi_sam_ascend(spec, ws, BB, TB, g, b["params"], [ops.Sam(0.05), None, ops.Sam(0.2)], ostate, sstate)
    rows = ops.sam_rows(sstate, M, P)
    lg = ops.multi_train_step(spec, rows, b["x"], y, ws, g, rngs=b["rngs"], fuse_adam=False)
    ws2, g2 = torch.full_like(b["ws"], NAN), torch.full((M, P), NAN, device=dev)
    lg2 = ops.multi_train_step(spec, rows.clone(), b["x"], y, ws2, g2, rngs=b["rngs"], fuse_adam=False)
    lay = b["lay"]
    stride = (spec.offsets()["ln.weight"] + 3) // 4 * 4
    assert _same(g, g2) and _same(lg, lg2) and _same(ws[lay.slabs:lay.slabs + lay.n_slabs * stride], ws2[lay.slabs:lay.slabs + lay.n_slabs * stride])
    assert _same(ops.multi_loss_sum(spec, ws, M, BB, TB), ops.multi_loss_sum(spec, ws2, M, BB, TB))
    # the model without SAM ran its second pass on a copy of its parameters: the first pass again, and the others did not
    assert _same(g[1], g1[1]) and _same(lg.view(M, BB, -1)[1], lg1.view(M, BB, -1)[1]) and not _same(g[0], g1[0]) and not _same(g[2], g1[2])


# ---- 4. the gradient of pass 2 against the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [BASE_SHAPES[0], BASE_SHAPES[2]], ids=["P31764", "F33-K9"])
def test_pass_two_against_the_oracle(nsd, dev, shape):
    """the GPU's p_adv on the host, the oracle's train step there with the same masks: the existing bounds of the route"""
    from nsd_amd import ops
    e = _evaluated(shape, safe=True)
    spec, P, B, T, d = e["spec"], e["P"], e["B"], e["T"], e["d"]
    p, x, y = to_dev(e["flat"], dev), to_dev(e["x"], dev), to_dev(e["y"], dev)
    ws, lg, g = ops.new_workspace(spec, B, T, dev), torch.empty((B, spec.K), device=dev), torch.full((P,), NAN, device=dev)
    ostate, sstate = ops.opt_state(P, 1, dev), _sam_state(ops, P, 1, dev)
    ops.train_step_grads(spec, p, x, ws, y, lg, g, **e["mk"])
    ops.sam_ascend(spec, ws, B, T, g, p, ops.Sam(0.05), ostate, sstate)
    row = ops.sam_rows(sstate, 1, P)[0]
    ops.train_step_grads(spec, row, x, ws, y, lg, g, **e["mk"])
    loss = ops.ws_view(ws, spec, B, T, "loss").cpu().numpy().astype(np.float64)
    out = dict(logits=lg.cpu().numpy(), grads=g.cpu().numpy(), mean_loss=float(loss.sum()) / B)
    ref = oracle_step(d, row.cpu().numpy(), e["x"], labels=e["y"], masks=e["masks"])
    assert_step_vs_oracle(out, ref, d, bounds_of(d), tag=f"sam pass 2 {shape}")
    first = oracle_step(d, e["flat"], e["x"], labels=e["y"], masks=e["masks"])
    print(f"[sam] oracle loss at p {first['loss']:.6f}, at p_adv {ref['loss']:.6f}")
    assert ref["loss"] > first["loss"]                                   # uphill


# ---- 5. the update is today's tail --------------------------------------------------------------------------------------------------------
def _tail(ops, spec, B, T, ws, g, p, m, v, opt, state, step, avg=None, astate=None):
    d = spec.dims(B, T)
    av = () if avg is None else (C.byref(avg.struct()), astate.data_ptr(), ops._nbytes(astate))
    ops._call("nsd_grad_reduce_clip_adam_avg" if av else "nsd_grad_reduce_clip_adam", ws.device, C.byref(d), ws.data_ptr(), ops._nbytes(ws),
              g.data_ptr(), p.data_ptr(), m.data_ptr(), v.data_ptr(), C.byref(opt), step, None, state.data_ptr(), ops._nbytes(state), ops.STREAM, *av)


@pytest.mark.parametrize("averaged", [False, True])
def test_the_update_is_todays_tail(nsd, dev, averaged):
    """two SAM steps through ops.train_step_grads(sam=, adam=) against the composition by hand -- pass 1, nsd_sam_ascend, pass 2, then
    nsd_grad_reduce_clip_adam(_avg) from the workspace that holds pass 2's slabs: p, m, v, grads, the opt record and the averaged row"""
    from nsd_amd import ops
    e = _evaluated(BASE_SHAPES[0])
    spec, P, B, T = e["spec"], e["P"], e["B"], e["T"]
    x, y = to_dev(e["x"], dev), to_dev(e["y"], dev)
    opt = ops.opt_struct(lr=LR, weight_decay=1e-2, max_norm=0.05, grad_scale=0.5)
    avg = ops.Average("ema", 0.9) if averaged else None
    sam = ops.Sam(0.05)

    def fresh():
        return dict(p=to_dev(e["flat"], dev), m=torch.zeros(P, device=dev), v=torch.zeros(P, device=dev), g=torch.full((P,), NAN, device=dev),
                    ws=ops.new_workspace(spec, B, T, dev), lg=torch.empty((B, spec.K), device=dev), o=ops.opt_state(P, 1, dev),
                    s=_sam_state(ops, P, 1, dev), a=ops.avg_state(P, 1, dev) if averaged else None)
    a, b = fresh(), fresh()
    for step in (1, 2):
        rng = dict(seed=5, base_stream=4 * step, p_lstm=0.6, p_head=0.6)
        ops.train_step_grads(spec, a["p"], x, a["ws"], y, a["lg"], a["g"], rng=rng, sam=sam, sam_state=a["s"],
                             adam=dict(m=a["m"], v=a["v"], opt=opt, opt_state=a["o"], step=step, avg=avg, avg_state=a["a"]))
        ops.train_step_grads(spec, b["p"], x, b["ws"], y, b["lg"], b["g"], rng=rng)
        ops.sam_ascend(spec, b["ws"], B, T, b["g"], b["p"], sam, b["o"], b["s"], grad_scale=opt.grad_scale)
        ops.train_step_grads(spec, ops.sam_rows(b["s"], 1, P)[0], x, b["ws"], y, b["lg"], b["g"], rng=rng)
        _tail(ops, spec, B, T, b["ws"], b["g"], b["p"], b["m"], b["v"], opt, b["o"], step, avg, b["a"])
        assert all(_same(a[k], b[k]) for k in ("p", "m", "v", "g", "lg")) and torch.equal(a["o"][:16], b["o"][:16]) and torch.equal(a["s"], b["s"]), step
        if averaged:
            assert torch.equal(a["a"], b["a"]) and ops.avg_records(a["a"])[0]["n_avg"] == step
        rec = ops.opt_records(a["o"])[0]
        assert rec["coef"] < 1.0 and rec["skipped"] == 0 and not _same(a["p"], to_dev(e["flat"], dev))


# ---- 6. trainers ---------------------------------------------------------------------------------------------------------------------------
BT, TT = 6, 20


def _ref_model(nsd, dev, ref_state, **kw):
    m = nsd.EEG_LSTM(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in ref_state.items()}, strict=True)
    return m.to(dev).train()


def _xy(dev, seed=8, B=BT):
    return to_dev(synth_x(B, TT, seed=seed), dev), to_dev(synth_labels(B, seed=seed), dev)


def test_trainer_steps_are_the_composition_through_ops(nsd, dev, ref_state):
    """three Trainer(sam=Sam(0.05)) steps against pass 1, nsd_sam_ascend, pass 2 and the guarded tail issued by hand with the recipe's
    streams; last_loss() is the second pass's and last_sam() the ascent's record"""
    from nsd_amd import ops
    from nsd_amd.step_recipe import step_rng, trainer_seed
    from nsd_amd.trainer import Trainer
    x, y = _xy(dev)
    sam = ops.Sam(0.05)
    tr = Trainer(_ref_model(nsd, dev, ref_state), lr=LR, seed=5, sam=sam, weight_decay=1e-2)
    model = _ref_model(nsd, dev, ref_state)
    spec, P = model.spec, model.spec.param_count
    p, m, v, g = model.flat_parameters().detach().clone(), torch.zeros(P, device=dev), torch.zeros(P, device=dev), torch.full((P,), NAN, device=dev)
    ws, lg, o, s = ops.new_workspace(spec, BT, TT, dev), torch.empty((BT, spec.K), device=dev), ops.opt_state(P, 1, dev), ops.sam_state(P, 1, dev)
    opt = ops.opt_struct(lr=LR, weight_decay=1e-2, max_norm=None)
    xin = ops.zscore(x) if model.normalize else x
    for step in (1, 2, 3):
        tr.step(x, y)
        rng = step_rng(trainer_seed(5), step, model.dropout_p, model.head_dropout_p)
        ops.train_step_grads(spec, p, xin, ws, y, lg, g, rng=rng)
        ops.sam_ascend(spec, ws, BT, TT, g, p, sam, o, s)
        ops.train_step_grads(spec, ops.sam_rows(s, 1, P)[0], xin, ws, y, lg, g, rng=rng)
        loss2 = float(ops.loss_sum(spec, ws, BT, TT).item()) / BT
        _tail(ops, spec, BT, TT, ws, g, p, m, v, opt, o, step)
        assert _same(tr.flat, p) and _same(tr.m, m) and _same(tr.v, v) and _same(tr.grads, g), step
        assert tr.last_loss() == loss2 and tr.last_sam() == ops.sam_records(s)[0] and tr.last_sam()["scale"] > 0
    assert tr.skipped_steps() == 0 and tr.step_count == 3 and tr.last_sam()["nonfinite"] == 0
    plain = Trainer(_ref_model(nsd, dev, ref_state), lr=LR, seed=5, weight_decay=1e-2, clip_grad_norm=0.0)
    for _ in range(3):
        plain.step(x, y)
    assert not _same(plain.flat, tr.flat) and plain.last_sam() is None


def test_graph_replay_equals_the_eager_step(nsd, dev, ref_state):
    from nsd_amd import ops
    from nsd_amd.trainer import Trainer
    x, y = _xy(dev)
    kw = dict(lr=LR, seed=5, sam=ops.Sam(0.05))
    ta, tb = Trainer(_ref_model(nsd, dev, ref_state), **kw), Trainer(_ref_model(nsd, dev, ref_state), **kw)
    xs, ys = tb.static_inputs(BT, TT)
    xs.copy_(x); ys.copy_(y)
    for _ in range(3):
        ta.step(x, y)
        tb.step_static(BT, TT)
    d = float((ta.flat - tb.flat).abs().max())
    print(f"[graph replay] sam: |flat eager - flat graph| {d:.3e}")
    assert _same(ta.flat, tb.flat) and _same(ta.m, tb.m) and _same(ta.v, tb.v)
    assert ta.last_sam() == tb.last_sam() and ta.last_loss() == tb.last_loss() and ta.skipped_steps() == tb.skipped_steps() == 0


def test_model_batch_with_a_rho_per_model(nsd, dev, ref_state):
    """ModelBatchTrainer(sam=[Sam(.05), None, Sam(.2)]), three steps: models 0 and 2 are Trainer(model_m, seed=seeds[m], sam=...)'s bit
    for bit; model 1 is the same model of a batch trained with the guarded tail and no SAM"""
    from nsd_amd import ops
    from nsd_amd.trainer import Trainer
    x, y = _xy(dev)
    M, seeds = 3, [1, 2, 3]
    sams = [ops.Sam(0.05), None, ops.Sam(0.2)]
    models = lambda: [_ref_model(nsd, dev, ref_state) for _ in range(M)]                     # noqa: E731
    mt = nsd.ModelBatchTrainer(models(), lr=LR, seeds=seeds, sam=sams, stochastic=True)
    guarded = nsd.ModelBatchTrainer(models(), lr=LR, seeds=seeds, clip_grad_norm=0.0, stochastic=True)
    singles = [Trainer(_ref_model(nsd, dev, ref_state), lr=LR, seed=seeds[i], sam=sams[i], stochastic=True) for i in (0, 2)]
    for _ in range(3):
        mt.step(x, y)
        guarded.step(x, y)
        for t in singles:
            t.step(x, y)
    recs = mt.last_sams()
    assert recs[1]["scale"] == 0.0 and recs[0]["scale"] > 0 and recs[2]["scale"] > 0 and mt.skipped_steps() == [0, 0, 0]
    assert _same(mt.params[1], guarded.params[1]) and _same(mt.m[1], guarded.m[1]) and _same(mt.v[1], guarded.v[1])
    assert not _same(mt.params[0], guarded.params[0]) and not _same(mt.params[2], guarded.params[2])
    for i, t in zip((0, 2), singles):
        d = float((mt.params[i] - t.flat).abs().max())
        print(f"[model batch] model {i}: |params batched - params single| {d:.3e}")
        assert _same(mt.params[i], t.flat) and _same(mt.m[i], t.m) and _same(mt.v[i], t.v), i
        assert recs[i] == t.last_sam()
    # a sequence of equal entries issues the single setting's calls
    same = nsd.ModelBatchTrainer(models(), lr=LR, seeds=seeds, sam=[ops.Sam(0.1)] * M)
    one = nsd.ModelBatchTrainer(models(), lr=LR, seeds=seeds, sam=ops.Sam(0.1))
    assert same.sam == one.sam == ops.Sam(0.1)
    same.step(x, y)
    one.step(x, y)
    assert _same(same.params, one.params)


# ---- 7. the bf16 sequence path ---------------------------------------------------------------------------------------------------------------
def test_bf16_sequence_path(nsd, dev):
    """the model and batch tests/test_gpu_seqpath.py trains: the flat ascent from the gradient nsd_seq_train_bwd left, and one
    Trainer(precision='bf16', sam=) step"""
    from nsd_amd import ops
    from nsd_amd.trainer import Trainer
    torch.manual_seed(0)
    model = nsd.EEG_LSTM(8, 64, 2, 5, dropout=0.5, precision="bf16").to(dev).train()
    B, T = 48, 20
    x, y = to_dev(synth_x(B, T, seed=5), dev), to_dev(synth_labels(B, K=5, seed=5).astype(np.int32), dev)
    spec, flat = model.spec, model.flat_parameters().detach()
    P = spec.param_count
    ws = ops.seq_workspace(spec, B, T, dev)
    ops.seq_train_fwd(spec, flat, x, y, ws)
    g = ops.seq_train_bwd(spec, flat, ws, B, T)
    g0, p0 = g.clone(), flat.clone()
    ostate, sstate = ops.opt_state(P, 1, dev), _sam_state(ops, P, 1, dev)
    ops.sam_ascend_flat(flat, g, ops.Sam(0.05), ostate, sstate)
    assert _same(g, g0) and _same(flat, p0)
    _check_row(ops, sstate, 1, 0, P, flat, g, 0.05, 1.0, "bf16")
    tr = Trainer(model, lr=3e-3, seed=3, sam=ops.Sam(0.05))
    tr.step(x, y)
    tr.check()
    rec = tr.last_sam()
    assert tr.scan_status() == 0 and tr.skipped_steps() == 0 and not _same(tr.flat, p0) and bool(torch.isfinite(tr.flat).all())
    assert rec["scale"] > 0 and rec["nonfinite"] == 0 and math.isfinite(tr.last_loss())


# ---- 8. the buffer contract of the three entry points ---------------------------------------------------------------------------------------
def _contract(ops, dev, n, M, launch, inputs, grads_shape):
    """launch(sam_state, grads) with sam_state of exactly nsd_sam_state_bytes between 0xA5 guards, pre-filled and then initialised, and
    grads pre-filled; plain and on a side stream: the same bits everywhere, guards intact, inputs unchanged"""
    nb = ops.sam_state_bytes(n, M)
    assert nb == 16 * M + 4 * M * n

    def once(fill, side):
        state, check = bc.guarded((nb,), torch.uint8, dev, fill)
        ops._call("nsd_sam_state_init", dev, state.data_ptr(), nb, ops.STREAM)
        assert int(state.max()) == 0                                                # zeroed, all of it
        bc.fill_payload(state[16 * M:], fill)                                       # the rows are scratch: whatever they hold
        g, gcheck = (None, None) if grads_shape is None else bc.guarded(grads_shape, torch.float32, dev, fill)
        snap = bc.snapshot(*inputs)
        torch.cuda.synchronize()
        if side:
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                launch(state, g)
            torch.cuda.current_stream().wait_stream(st)
        else:
            launch(state, g)
        torch.cuda.synchronize()
        check("sam_state")
        if gcheck is not None:
            gcheck("grads")
        assert snap.unchanged(), (fill, side, snap.changed())
        return [state.clone()] + ([] if g is None else [bc._bits(g)])
    base = once("ones", False)
    for fill, side in (("nan32", False), ("ones", True), ("nan32", True)):
        got = once(fill, side)
        assert all(torch.equal(u, w) for u, w in zip(base, got)), (fill, side)
    return base


@pytest.mark.parametrize("n", [257, 2048 * 256 + 1])
def test_buffer_contract_flat_route(nsd, dev, n):
    from nsd_amd import ops
    rs = np.random.RandomState(n % 9973)
    p, g = to_dev(rs.uniform(-1, 1, n).astype(np.float32), dev), to_dev(rs.standard_normal(n).astype(np.float32), dev)
    ostate = ops.opt_state(n, 1, dev)
    base = _contract(ops, dev, n, 1, lambda state, _: ops.sam_ascend_flat(p, g, ops.Sam(0.05), ostate, state), [p, g], None)
    assert ops.sam_records(base[0])[0]["scale"] > 0


def test_buffer_contract_single_model(nsd, dev):
    from nsd_amd import ops
    e = _evaluated(BASE_SHAPES[2])
    spec, P = e["spec"], e["P"]
    p, ostate = to_dev(e["flat"], dev), ops.opt_state(P, 1, dev)
    base = _contract(ops, dev, P, 1, lambda state, g: ops.sam_ascend(spec, e["ws"], e["B"], e["T"], g, p, ops.Sam(0.05), ostate, state),
                     [p, e["ws"]], (P,))
    assert torch.equal(base[1], bc._bits(e["g"]))


def test_buffer_contract_model_batch(nsd, dev):
    from nsd_amd import ops
    M = 3
    b = _batched(M)
    spec, P = b["spec"], b["P"]
    ostate = ops.opt_state(P, M, dev)
    sams = [ops.Sam(0.05), None, ops.Sam(0.2)]
    base = _contract(ops, dev, P, M, lambda state, g: ops.multi_sam_ascend(spec, b["ws"], BB, TB, g, b["params"], sams, ostate, state),
                     [b["params"], b["ws"]], (M, P))
    assert torch.equal(base[1], bc._bits(b["grads"])) and [r["scale"] > 0 for r in ops.sam_records(base[0], M)] == [True, False, True]


def test_refusals_launch_nothing(nsd, dev):
    """NULL pointers, a negative or NaN rho, n < 0, rows over p or grads (NSD_E_INVALID) and short state buffers (NSD_E_WORKSPACE): every
    buffer keeps its bits"""
    from nsd_amd import _lib, ops
    L = _lib.lib()
    n = 1000
    p, g = torch.rand(n, device=dev), torch.rand(n, device=dev)
    ostate, sstate = ops.opt_state(n, 1, dev), _sam_state(ops, n, 1, dev)
    both = torch.full((4 + 2 * n,), NAN, device=dev)                 # one allocation: a "state" whose rows are p's own words
    snap = bc.snapshot(p, g, ostate, sstate, both)
    ob, sb = ops._nbytes(ostate), ops._nbytes(sstate)

    def call(rho=0.05, n=n, p=p.data_ptr(), g=g.data_ptr(), o=ostate.data_ptr(), o_bytes=ob, s=sstate.data_ptr(), s_bytes=sb):
        return L.nsd_sam_ascend_flat(n, p, g, C.byref(_lib.Sam(rho)), 1.0, o, o_bytes, s, s_bytes, None)
    assert call(p=None) == -1 and call(g=None) == -1 and call(o=None) == -1 and call(s=None) == -1 and call(n=-1) == -1
    assert call(rho=-1.0) == -1 and call(rho=NAN) == -1
    assert call(o_bytes=ob - 8) == -3 and call(s_bytes=sb - 4) == -3
    assert call(p=both.data_ptr() + 16, s=both.data_ptr(), s_bytes=sb) == -1 and "overlap" in L.nsd_last_error().decode()
    assert call(g=both.data_ptr() + 16 + 4 * (n - 1), s=both.data_ptr(), s_bytes=sb) == -1
    e = _evaluated(BASE_SHAPES[0])
    spec, P = e["spec"], e["P"]
    d = spec.dims(e["B"], e["T"])
    pp, gg, oo, ss = to_dev(e["flat"], dev), torch.full((P,), NAN, device=dev), ops.opt_state(P, 1, dev), _sam_state(ops, P, 1, dev)
    snap2 = bc.snapshot(pp, gg, oo, ss, e["ws"])
    ws, wb = e["ws"].data_ptr(), ops._nbytes(e["ws"])
    for rho, args in ((-0.5, {}), (NAN, {}), (0.05, dict(s_bytes=ops._nbytes(ss) - 4)), (0.05, dict(o_bytes=ops._nbytes(oo) - 8)), (0.05, dict(wb=wb - 4)),
                      (0.05, dict(s=gg.data_ptr() - 16))):
        rc = L.nsd_sam_ascend(C.byref(d), ws, args.get("wb", wb), gg.data_ptr(), pp.data_ptr(), C.byref(_lib.Sam(rho)), 1.0, oo.data_ptr(),
                              args.get("o_bytes", ops._nbytes(oo)), args.get("s", ss.data_ptr()), args.get("s_bytes", ops._nbytes(ss)), None)
        assert rc in (-1, -3), (rho, args, rc)
    torch.cuda.synchronize()
    assert snap.unchanged() and snap2.unchanged()


# ---- 9. the command lines ------------------------------------------------------------------------------------------------------------------
def _json_lines(capsys):
    import json
    return [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]


def test_train_and_grid_command_lines(nsd, dev, tmp_path, capsys):
    """train --sam-rho through both drivers (with --avg beside it in the concurrent one), and grid --grid sam_rho=0,... : the
    configuration without SAM is the run without the option, and the best-configuration line carries train's own option"""
    from nsd_amd import grid, train
    out = str(tmp_path / "m.pth")
    base = ["--synthetic", "120", "--T", "12", "--epochs", "3", "--batch", "14", "--lr", "0.01", "--seed", "3", "--out", out]
    assert train.main(base + ["--sam-rho", "0.05"]) == 0
    recs = _json_lines(capsys)
    done = [r for r in recs if r.get("done")][0]
    logged = [r for r in recs if "epoch" in r]
    assert done["args"]["sam_rho"] == 0.05 and logged and all(r["skipped"] == 0 and np.isfinite(r["grad_norm"]) for r in logged)
    assert train.main(base) == 0
    plain = [r for r in _json_lines(capsys) if r.get("done")][0]
    assert "sam_rho" not in plain["args"]
    conc = base + ["--kfold", "3", "--concurrent"]
    assert train.main(conc + ["--sam-rho", "0.1", "--avg", "ema", "--avg-decay", "0.9"]) == 0
    recs = _json_lines(capsys)
    done = [r for r in recs if r.get("done")][0]
    assert done["args"]["sam_rho"] == 0.1 and len(done["acc_val_folds"]) == 3 and all(r["skipped"] == 0 for r in recs if r.get("concurrent") and "epoch" in r)
    kf = ["--synthetic", "120", "--T", "12", "--kfold", "3", "--epochs", "3", "--batch", "14", "--lr", "0.01", "--seed", "3", "--log-every", "100"]
    assert grid.main(kf + ["--grid", "sam_rho=0,0.05,0.2"]) == 0
    recs = _json_lines(capsys)
    sums = sorted((r for r in recs if r.get("summary")), key=lambda r: r["config_index"])
    done = [r for r in recs if r.get("done")][0]
    assert [s["config"] for s in sums] == [{"sam_rho": 0.0}, {"sam_rho": 0.05}, {"sam_rho": 0.2}]
    assert [s["train_args"] for s in sums] == [["--sam-rho", "0.0"], ["--sam-rho", "0.05"], ["--sam-rho", "0.2"]]
    assert done["best"]["train_args"][0] == "--sam-rho" and done["best"]["train_args"] in [s["train_args"] for s in sums]
    # rho = 0 of the grid is the concurrent run without the option (the three configurations share one launch: model m of a batch
    # with SAM and rho = 0 trains bit for bit as without it)
    assert train.main(conc) == 0
    ref = [r for r in _json_lines(capsys) if r.get("done")][0]
    assert sums[0]["acc_val_folds"] == ref["acc_val_folds"]
