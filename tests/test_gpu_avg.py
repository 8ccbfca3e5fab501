"""Weight averaging in the fused step tail (nsd_avg of include/nsd.h) on the MI355X: the flat route, start and stride, skips, the fused
single-model tail, the model-batched tails (`_each` included), the device step counter under graph replay, launch accounting, the
consumers of the averaged rows, the bf16 flat route, resume, and the buffer contract.  Run with `pytest -m gpu -s`.

Everything here is bit for bit.  The references never come from the code under test:
  p, m, v, grads, nsd_opt_record   the twin entry point WITHOUT averaging, on a second set of buffers
  the averaged row                 tests/avg_ref.py in float32 (tests/test_avg_cpu.py pins it to torch's AveragedModel), applied to the
                                   GPU's own p read back after each step: every operation of the rule is one rounded fp32 operation
  n_avg / arrive                   counted by hand
Problem sizes of the flat and fused routes are those of tests/test_gpu_optim.py, by value."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import buffer_contract as bc
from tests.avg_ref import EMA, SWA, AveragedWeights
from tests.golden.make_goldens import synth_labels, synth_x
from tests.gpu_harness import dev, head_inputs, multi_problem, nsd, sync_at_the_end, to_dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

LR = 1e-3
NAN_WORD = 0x7FC00000


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """bit for bit (NaN payloads included)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _words(t) -> np.ndarray:
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


def _ref(avg, dtype=np.float32) -> AveragedWeights:
    return AveragedWeights(EMA if avg.kind == "ema" else SWA, avg.decay, avg.start_step, avg.every, dtype=dtype)


def _prefilled(ops, n, M, dev):
    """an avg_state whose rows hold NaN words: whatever is read before it is written shows"""
    st = ops.avg_state(n, M, dev)
    bc.fill_payload(st[16 * M:], "nan32")
    return st


def _kinds(nsd):
    from nsd_amd import ops
    return {"ema0.9": ops.Average("ema", 0.9), "ema0.999": ops.Average("ema", 0.999), "swa": ops.Average("swa")}


# ---- 1. flat route ---------------------------------------------------------------------------------------------------------------------
FLAT_N = [1, 3, 33, 31764, 2**20 + 1]


@functools.lru_cache(maxsize=None)
def _flat_problem(n):
    rs = np.random.RandomState(n % 9973)
    p0 = rs.uniform(-1, 1, n).astype(np.float32)
    gs = [rs.standard_normal(n).astype(np.float32) for _ in range(7)]
    return p0, gs, float(np.sqrt((gs[0].astype(np.float64) ** 2).sum()))


class _Flat:
    """two sets of flat buffers stepped side by side: nsd_adam_step_clip_avg, and its twin nsd_adam_step_clip"""

    def __init__(self, ops, dev, n, avg, kw=None, prefill=True):
        self.ops, self.dev, self.n, self.avg = ops, dev, n, avg
        p0, self.gs, norm = _flat_problem(n)
        kw = dict(weight_decay=1e-2, max_norm=0.1 * norm) if kw is None else kw
        self.opt = ops.opt_struct(lr=LR, **kw)
        self.a = [to_dev(p0, dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev), ops.opt_state(n, 1, dev)]
        self.b = [to_dev(p0, dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev), ops.opt_state(n, 1, dev)]
        self.astate = _prefilled(ops, n, 1, dev) if prefill else ops.avg_state(n, 1, dev)
        self.row = ops.avg_rows(self.astate, 1, n)[0]
        self.ref = _ref(avg)

    def step(self, s, g=None, skip=None, twin=True):
        ops = self.ops
        gt = to_dev(self.gs[s - 1] if g is None else g, self.dev)
        p, m, v, st = self.a
        ops.grad_norm(gt, st, self.opt.grad_scale)
        ops.adam_step_clip_avg(p, gt, m, v, self.opt, st, self.avg, self.astate, step=s, skip=skip)
        if twin:
            p, m, v, st = self.b
            ops.grad_norm(gt, st, self.opt.grad_scale)
            ops.adam_step_clip(p, gt, m, v, self.opt, st, step=s, skip=skip)

    def twins_agree(self):
        return all(_same(x, y) for x, y in zip(self.a[:3], self.b[:3])) and torch.equal(self.a[3][:16], self.b[3][:16])

    def record(self):
        torch.cuda.synchronize()
        return self.ops.avg_records(self.astate)[0]


@pytest.mark.parametrize("kind", ["ema0.9", "ema0.999", "swa"])
@pytest.mark.parametrize("n", FLAT_N)
def test_flat_route(nsd, dev, n, kind):
    """Seven steps, weight decay on, a threshold that clips every step.  n = 2^20 + 1: more elements than 2048 workgroups x 256 lanes, so
    the grid-stride loop runs more than once whatever grid the launch picks, and the last arriver counts its largest grid."""
    from nsd_amd import ops
    f = _Flat(ops, dev, n, _kinds(nsd)[kind])
    for s in range(1, 8):
        f.step(s)
        assert f.twins_agree(), (n, kind, s)
        assert ops.opt_records(f.a[3])[0]["coef"] < 1.0        # the threshold bites
        assert f.ref.update(f.a[0].cpu().numpy(), s)
        assert np.array_equal(_words(f.row), _words(f.ref.row)), (n, kind, s, int((_words(f.row) != _words(f.ref.row)).sum()))
        assert f.record() == dict(n_avg=s, arrive=0), (n, kind, s)


# ---- 2. start and stride ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 31764])
def test_start_and_stride(nsd, dev, n):
    from nsd_amd import ops
    f = _Flat(ops, dev, n, ops.Average("swa", start_step=3, every=2))
    took = []
    for s in range(1, 8):
        f.step(s)
        if f.ref.update(f.a[0].cpu().numpy(), s):
            took.append(s)
        if s < 3:                                              # the NaN-word pre-fill, byte for byte
            assert (_words(f.row) == NAN_WORD).all() and f.record() == dict(n_avg=0, arrive=0)
        else:
            assert np.array_equal(_words(f.row), _words(f.ref.row)), (n, s)
            assert f.record() == dict(n_avg=len(took), arrive=0)
        assert f.twins_agree()
    assert took == [3, 5, 7]


# ---- 3. skips --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ema0.9", "swa"])
def test_a_non_finite_step_does_not_average(nsd, dev, kind):
    """one Inf in the gradient of step 4: p, m, v, the row and n_avg untouched, skipped + 1; steps 5 .. 7 go on from there"""
    from nsd_amd import ops
    n = 31764
    f = _Flat(ops, dev, n, _kinds(nsd)[kind])
    for s in range(1, 8):
        before = [t.clone() for t in f.a[:3]] + [f.row.clone()]
        g = f.gs[s - 1]
        if s == 4:
            g = g.copy()
            g[n // 2] = np.inf
        f.step(s, g=g)
        assert f.twins_agree()
        took = f.ref.update(f.a[0].cpu().numpy(), s, skipped=(s == 4))
        assert took == (s != 4)
        if s == 4:
            assert all(_same(x, y) for x, y in zip(before, f.a[:3] + [f.row]))
            assert ops.opt_records(f.a[3])[0]["skipped"] == 1
        assert np.array_equal(_words(f.row), _words(f.ref.row)), s
        assert f.record() == dict(n_avg=f.ref.n, arrive=0)
    assert f.ref.n == 6 and ops.opt_records(f.a[3])[0]["skipped"] == 1


def test_the_callers_skip_flag_does_not_average(nsd, dev):
    """skip[0] != 0 at step 4: as above, and the opt record stays as it was too"""
    from nsd_amd import ops
    n = 31764
    f = _Flat(ops, dev, n, ops.Average("ema", 0.9))
    flag = torch.zeros(1, device=dev)
    for s in range(1, 8):
        before = [t.clone() for t in f.a[:3]] + [f.row.clone(), f.a[3][:16].clone(), f.astate[:16].clone()]
        flag.fill_(1.0 if s == 4 else 0.0)
        f.step(s, skip=flag)
        assert f.twins_agree()
        assert f.ref.update(f.a[0].cpu().numpy(), s, skipped=(s == 4)) == (s != 4)
        if s == 4:
            after = f.a[:3] + [f.row, f.a[3][:16], f.astate[:16]]
            assert all(torch.equal(x.view(torch.uint8), y.contiguous().view(torch.uint8)) for x, y in zip(before, after))
        assert np.array_equal(_words(f.row), _words(f.ref.row)), s
        assert f.record() == dict(n_avg=f.ref.n, arrive=0)
    assert f.ref.n == 6


# ---- 4. fused single-model tail ----------------------------------------------------------------------------------------------------------
def _tail(ops, spec, B, T, ws, g, p, m, v, opt, state, step, avg=None, astate=None, step_dev=None):
    """nsd_grad_reduce_clip_adam, or with avg its `_avg` twin, on a workspace that holds an evaluation's slabs"""
    d = spec.dims(B, T)
    av = () if avg is None else (C.byref(avg.struct()), astate.data_ptr(), ops._nbytes(astate))
    ops._call("nsd_grad_reduce_clip_adam_avg" if av else "nsd_grad_reduce_clip_adam", ws.device, C.byref(d), ws.data_ptr(), ops._nbytes(ws),
              g.data_ptr(), p.data_ptr(), m.data_ptr(), v.data_ptr(), C.byref(opt), step, None if step_dev is None else step_dev.data_ptr(),
              state.data_ptr(), ops._nbytes(state), ops.STREAM, *av)


@pytest.mark.parametrize("kind", ["ema0.9", "swa"])
@pytest.mark.parametrize("shape", [(8, 48, 2, 3, 32, 3, 5), (8, 5, 1, 3, 32, 3, 5)], ids=lambda s: "C%d-H%d-L%d-K%d-F%d-B%d-T%d" % s)
def test_fused_tail(nsd, dev, shape, kind):
    """three steps on the slabs of one real forward + backward (H = 48: the fast path; H = 5, L = 1: the generic one)"""
    from nsd_amd import ops
    Cc, H, L, K, F, B, T = shape
    _, flat, x, y, _ = head_inputs(Cc, H, K, F, B, T, L=L)
    spec = ops.ModelSpec(C=Cc, H=H, L=L, K=K, F=F)
    P = spec.param_count
    ws, logits, g0 = ops.new_workspace(spec, B, T, dev), torch.empty((B, K), device=dev), torch.empty(P, device=dev)
    ops.train_step_grads(spec, to_dev(flat, dev), to_dev(x, dev), ws, to_dev(y, dev), logits, g0)
    norm = float(g0.double().norm())
    assert np.isfinite(norm) and norm > 0
    opt = ops.opt_struct(lr=LR, weight_decay=1e-2, max_norm=0.1 * norm)
    avg = _kinds(nsd)[kind]
    a = [torch.full((P,), float("nan"), device=dev), to_dev(flat, dev), torch.zeros(P, device=dev), torch.zeros(P, device=dev), ops.opt_state(P, 1, dev)]
    b = [torch.full((P,), float("nan"), device=dev), to_dev(flat, dev), torch.zeros(P, device=dev), torch.zeros(P, device=dev), ops.opt_state(P, 1, dev)]
    astate = _prefilled(ops, P, 1, dev)
    row, R = ops.avg_rows(astate, 1, P)[0], _ref(avg)
    for s in range(1, 4):
        _tail(ops, spec, B, T, ws, *a[:4], opt, a[4], s, avg, astate)
        _tail(ops, spec, B, T, ws, *b[:4], opt, b[4], s)
        assert all(_same(u, w) for u, w in zip(a[:4], b[:4])) and torch.equal(a[4][:16], b[4][:16]), (shape, s)
        assert _same(a[0], g0) and ops.opt_records(a[4])[0]["coef"] < 1.0
        R.update(a[1].cpu().numpy(), s)
        assert np.array_equal(_words(row), _words(R.row)), (shape, kind, s)
        assert ops.avg_records(astate)[0] == dict(n_avg=s, arrive=0)


# ---- 5. model-batched tails ----------------------------------------------------------------------------------------------------------
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
    return dict(spec=spec, P=spec.param_count, params=params, ws=ws, grads=grads, lay=lay)


def _single_ws(ops, dev, b, M, mdl, ws=None):
    """a single-model workspace that holds model mdl's slabs (at these sizes either launch writes one LSTM slab per trial)"""
    spec, lay, ws = b["spec"], b["lay"], b["ws"] if ws is None else ws
    nb, one = ops.workspace_layout(spec, BB, TB)
    assert one.n_slabs == BB and lay.n_slabs == M * BB
    p_lstm = spec.offsets()["ln.weight"]
    stride, ph = (p_lstm + 3) // 4 * 4, b["P"] - p_lstm
    w1 = torch.full((nb // 4,), float("nan"), device=dev)
    w1[one.slabs:one.slabs + BB * stride] = ws[lay.slabs + mdl * BB * stride:lay.slabs + (mdl + 1) * BB * stride]
    w1[one.hslabs:one.hslabs + BB * ph] = ws[lay.hslabs + mdl * BB * ph:lay.hslabs + (mdl + 1) * BB * ph]
    return w1


def _multi_tail(ops, spec, M, ws, g, p, m, v, opts, state, step, avgs=None, astate=None):
    """opts / avgs: one entry (the uniform entry points) or lists of M (the `_each` ones); avgs None: the twins without averaging"""
    d = spec.dims(BB, TB)
    each = isinstance(opts, list)
    name = "nsd_multi_grad_reduce_clip_adam" + ("" if avgs is None else "_avg") + ("_each" if each else "")
    oarg = C.cast((ops._lib.Opt * M)(*opts), C.c_void_p) if each else C.byref(opts)
    av = ()
    if avgs is not None:
        arr = (ops._lib.Avg * M)(*[ops._avg_struct(a) for a in avgs]) if each else None
        av = (C.cast(arr, C.c_void_p) if each else C.byref(avgs.struct()), astate.data_ptr(), ops._nbytes(astate))
    ops._call(name, ws.device, C.byref(d), M, ws.data_ptr(), ops._nbytes(ws), g.data_ptr(), p.data_ptr(), m.data_ptr(), v.data_ptr(), oarg, step,
              None, state.data_ptr(), ops._nbytes(state), ops.STREAM, *av)


def _model_bufs(b, M, dev):
    return [torch.full((M, b["P"]), float("nan"), device=dev), b["params"].clone(), torch.zeros_like(b["params"]), torch.zeros_like(b["params"])]


@pytest.mark.parametrize("M", [3, 32])
def test_model_batched_tail_is_the_single_model_tail_per_model(nsd, dev, M):
    """one nsd_avg for all models, three steps: p, m, v, grads and records are the twin's without averaging; model m's row and avg
    record are the single-model `_avg` call's on its slabs, and the row follows avg_ref"""
    from nsd_amd import ops
    b = _batched(M)
    spec, P = b["spec"], b["P"]
    norms = sorted(float(b["grads"][i].double().norm()) for i in range(M))
    opt = ops.opt_struct(lr=LR, weight_decay=1e-2, max_norm=norms[M // 2])          # some models clip, some do not
    avg = ops.Average("ema", 0.9)
    a, t = _model_bufs(b, M, dev), _model_bufs(b, M, dev)
    sa, st, astate = ops.opt_state(P, M, dev), ops.opt_state(P, M, dev), _prefilled(ops, P, M, dev)
    rows = ops.avg_rows(astate, M, P)
    singles = [dict(ws=_single_ws(ops, dev, b, M, i), bufs=[torch.empty(P, device=dev), b["params"][i].clone(), torch.zeros(P, device=dev),
                                                            torch.zeros(P, device=dev)], st=ops.opt_state(P, 1, dev), ast=_prefilled(ops, P, 1, dev),
                    ref=_ref(avg)) for i in range(M)]
    for s in range(1, 4):
        _multi_tail(ops, spec, M, b["ws"], *a, opt, sa, s, avg, astate)
        _multi_tail(ops, spec, M, b["ws"], *t, opt, st, s)
        assert all(_same(u, w) for u, w in zip(a, t)) and torch.equal(sa[:16 * M], st[:16 * M]), (M, s)
        recs, pa = ops.avg_records(astate, M), a[1].cpu().numpy()
        for i, one in enumerate(singles):
            _tail(ops, spec, BB, TB, one["ws"], *one["bufs"], opt, one["st"], s, avg, one["ast"])
            assert all(_same(u, w[i]) for u, w in zip(one["bufs"], a)), (M, s, i)
            assert torch.equal(one["st"][:16], sa[16 * i:16 * i + 16])
            assert _same(ops.avg_rows(one["ast"], 1, P)[0], rows[i]) and torch.equal(one["ast"][:16], astate[16 * i:16 * i + 16]), (M, s, i)
            one["ref"].update(pa[i], s)
            assert np.array_equal(_words(rows[i]), _words(one["ref"].row)), (M, s, i)
            assert recs[i] == dict(n_avg=s, arrive=0)
    coefs = [r["coef"] for r in ops.opt_records(sa, M)]
    assert any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs)


@pytest.mark.parametrize("M", [3, 32])
def test_each_mixes_modes_over_the_models(nsd, dev, M):
    """{EMA 0.9, SWA, no averaging, EMA 0.99 from step 2} cycled over the models, each model with its own lr: model m is the single-model
    call with entry m (without averaging: the twin without it), and a model that does not average keeps its row's pre-fill"""
    from nsd_amd import ops
    b = _batched(M)
    spec, P = b["spec"], b["P"]
    cycle = [ops.Average("ema", 0.9), ops.Average("swa"), None, ops.Average("ema", 0.99, start_step=2)]
    avgs = [cycle[i % 4] for i in range(M)] if M > 3 else [cycle[3], cycle[1], cycle[2]]
    opts = [ops.opt_struct(lr=LR * (1 + i % 3), weight_decay=1e-2, max_norm=0.05) for i in range(M)]
    a, t = _model_bufs(b, M, dev), _model_bufs(b, M, dev)
    sa, st, astate = ops.opt_state(P, M, dev), ops.opt_state(P, M, dev), _prefilled(ops, P, M, dev)
    rows = ops.avg_rows(astate, M, P)
    refs = [None if g is None else _ref(g) for g in avgs]
    check = sorted(set(range(min(M, 5))) | {M - 1})            # the single-model comparison: one of each kind, and the last model
    singles = {i: dict(ws=_single_ws(ops, dev, b, M, i), bufs=[torch.empty(P, device=dev), b["params"][i].clone(), torch.zeros(P, device=dev),
                                                               torch.zeros(P, device=dev)], st=ops.opt_state(P, 1, dev), ast=_prefilled(ops, P, 1, dev))
               for i in check}
    for s in range(1, 4):
        _multi_tail(ops, spec, M, b["ws"], *a, opts, sa, s, avgs, astate)
        _multi_tail(ops, spec, M, b["ws"], *t, opts, st, s)
        assert all(_same(u, w) for u, w in zip(a, t)) and torch.equal(sa[:16 * M], st[:16 * M]), (M, s)
        recs, pa = ops.avg_records(astate, M), a[1].cpu().numpy()
        for i in range(M):
            if refs[i] is None:
                assert (_words(rows[i]) == NAN_WORD).all() and recs[i] == dict(n_avg=0, arrive=0), (M, s, i)
                continue
            refs[i].update(pa[i], s)
            if refs[i].n:
                assert np.array_equal(_words(rows[i]), _words(refs[i].row)), (M, s, i)
            else:
                assert (_words(rows[i]) == NAN_WORD).all()
            assert recs[i] == dict(n_avg=refs[i].n, arrive=0), (M, s, i)
        for i, one in singles.items():
            _tail(ops, spec, BB, TB, one["ws"], *one["bufs"], opts[i], one["st"], s, avgs[i], one["ast"])
            assert all(_same(u, w[i]) for u, w in zip(one["bufs"], a)), (M, s, i)
            assert _same(ops.avg_rows(one["ast"], 1, P)[0], rows[i]) and torch.equal(one["ast"][:16], astate[16 * i:16 * i + 16]), (M, s, i)
    assert [None if r is None else r.n for r in refs] == [None if g is None else 4 - g.start_step for g in avgs]


def test_a_non_finite_model_is_frozen_alone(nsd, dev):
    from nsd_amd import ops
    M = 3
    b = _batched(M)
    spec, P, lay = b["spec"], b["P"], b["lay"]
    ws = b["ws"].clone()
    stride = (spec.offsets()["ln.weight"] + 3) // 4 * 4
    opt, avg = ops.opt_struct(lr=LR, max_norm=0.0), ops.Average("swa")
    a, sa, astate = _model_bufs(b, M, dev), ops.opt_state(P, M, dev), _prefilled(ops, P, M, dev)
    rows, refs = ops.avg_rows(astate, M, P), [_ref(avg) for _ in range(M)]
    for s in range(1, 4):
        before = [u[1].clone() for u in a[1:]] + [rows[1].clone(), astate[16:32].clone()]
        w = ws if s == 2 else b["ws"]
        if s == 2:
            ws[lay.slabs + 1 * BB * stride + stride + 77] = float("inf")             # model 1, slab 1, LSTM column 77
        _multi_tail(ops, spec, M, w, *a, opt, sa, s, avg, astate)
        recs, pa = ops.avg_records(astate, M), a[1].cpu().numpy()
        for i in range(M):
            refs[i].update(pa[i], s, skipped=(s == 2 and i == 1))
            assert np.array_equal(_words(rows[i]), _words(refs[i].row)) and recs[i] == dict(n_avg=refs[i].n, arrive=0), (s, i)
        if s == 2:
            after = [u[1] for u in a[1:]] + [rows[1], astate[16:32]]
            assert all(torch.equal(x.view(torch.uint8), y.contiguous().view(torch.uint8)) for x, y in zip(before, after))
    assert [r.n for r in refs] == [3, 2, 3] and [r["skipped"] for r in ops.opt_records(sa, M)] == [0, 1, 0]


# ---- 6. trainers: device step counter and graph replay, launches, consumers, bf16, resume ---------------------------------------------
BT, TT = 16, 30
COSINE = dict(kind="cosine", warmup_steps=2, total_steps=10, min_ratio=0.1)


def _ref_model(nsd, dev, ref_state, **kw):
    m = nsd.EEG_LSTM(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in ref_state.items()}, strict=True)
    return m.to(dev).train()


def _xy(dev, seed=8):
    return to_dev(synth_x(BT, TT, seed=seed), dev), to_dev(synth_labels(BT, seed=seed), dev)


@pytest.mark.parametrize("kind", ["ema0.9", "swa"])
def test_graph_replay_equals_eager_and_the_warm_up_does_not_count(nsd, dev, ref_state, kind):
    from nsd_amd.trainer import Trainer
    x, y = _xy(dev)
    kw = dict(lr=LR, seed=5, lr_schedule=nsd.LrSchedule(**COSINE), average=_kinds(nsd)[kind])
    ta, tb = Trainer(_ref_model(nsd, dev, ref_state), **kw), Trainer(_ref_model(nsd, dev, ref_state), **kw)
    xs, ys = tb.static_inputs(BT, TT)
    xs.copy_(x); ys.copy_(y)
    R = _ref(kw["average"])
    for s in range(1, 7):
        ta.step(x, y)
        tb.step_static(BT, TT)
        R.update(ta.flat.cpu().numpy(), s)
    d = float((ta.flat - tb.flat).abs().max())
    print(f"[graph replay] {kind}: |flat eager - flat graph| {d:.3e}  n_avg {ta.averaged_count()} / {tb.averaged_count()}")
    assert ta.averaged_count() == tb.averaged_count() == 6     # the warm-up step did not count
    assert np.array_equal(_words(ta.averaged_weights()), _words(R.row))
    assert _same(ta.flat, tb.flat) and _same(ta.averaged_weights(), tb.averaged_weights())
    assert torch.equal(ta._avg_state[:16], tb._avg_state[:16]) and ta.skipped_steps() == tb.skipped_steps() == 0


def _launches(fn, steps=3):
    from nsd_amd import ops
    names = []

    @contextlib.contextmanager
    def hook(name):
        names.append(name)
        yield
    ops.set_launch_hook(hook)
    try:
        for _ in range(steps):
            fn()
    finally:
        ops.set_launch_hook(None)
    return names


def test_launch_accounting(nsd, dev, ref_state):
    """average=None: today's call names.  With averaging: the count of clip_grad_norm=0.0 (the guarded tail), its last call replaced by
    the `_avg` twin -- no extra launch.  The same for ModelBatchTrainer."""
    from nsd_amd import ops
    from nsd_amd.trainer import Trainer
    x, y = _xy(dev)
    today = ["nsd_lstm_head_train_rng", "nsd_lstm_bwd_rng", "nsd_grad_reduce_adam"]
    tr = Trainer(_ref_model(nsd, dev, ref_state), lr=LR, seed=5, average=None)
    assert _launches(lambda: tr.step(x, y)) == today * 3
    tg = Trainer(_ref_model(nsd, dev, ref_state), lr=LR, seed=5, clip_grad_norm=0.0)
    guarded = _launches(lambda: tg.step(x, y))
    ta = Trainer(_ref_model(nsd, dev, ref_state), lr=LR, seed=5, average=ops.Average("swa"))
    got = _launches(lambda: ta.step(x, y))
    assert guarded == (today[:2] + ["nsd_grad_reduce_clip_adam"]) * 3
    assert got == (today[:2] + ["nsd_grad_reduce_clip_adam_avg"]) * 3 and len(got) == len(guarded)
    assert _same(ta.flat, tg.flat) and ta.averaged_count() == 3            # averaging does not change the trajectory: the guarded tail's bits
    models = lambda: [_ref_model(nsd, dev, ref_state) for _ in range(3)]
    multi = ["nsd_multi_train_fwd", "nsd_multi_train_bwd"]
    mt = nsd.ModelBatchTrainer(models(), lr=LR, seeds=[1, 2, 3], average=None)
    assert _launches(lambda: mt.step(x, y)) == (multi + ["nsd_multi_grad_reduce_adam"]) * 3
    mg = nsd.ModelBatchTrainer(models(), lr=LR, seeds=[1, 2, 3], clip_grad_norm=0.0)
    assert _launches(lambda: mg.step(x, y)) == (multi + ["nsd_multi_grad_reduce_clip_adam"]) * 3
    ma = nsd.ModelBatchTrainer(models(), lr=LR, seeds=[1, 2, 3], average=ops.Average("ema", 0.9))
    assert _launches(lambda: ma.step(x, y)) == (multi + ["nsd_multi_grad_reduce_clip_adam_avg"]) * 3
    me = nsd.ModelBatchTrainer(models(), lr=LR, seeds=[1, 2, 3], average=[ops.Average("ema", 0.9), None, ops.Average("swa")])
    assert _launches(lambda: me.step(x, y)) == (multi + ["nsd_multi_grad_reduce_clip_adam_avg_each"]) * 3
    assert ma.averaged_counts() == [3, 3, 3] and me.averaged_counts() == [3, 0, 3]
    # averaging does not change the trajectory: the guarded tail's bits
    assert _same(ma.params, mg.params) and _same(me.params, mg.params)


def test_consumers_of_the_averaged_rows(nsd, dev, ref_state, tmp_path):
    from nsd_amd import ops
    from nsd_amd.trainer import Trainer, save_reference_checkpoint
    x, y = _xy(dev)
    tr = Trainer(_ref_model(nsd, dev, ref_state), lr=LR, seed=5, average=ops.Average("ema", 0.9))
    am = tr.averaged_model()                                   # taken before the steps: it follows them
    for _ in range(3):
        tr.step(x, y)
    row = tr.averaged_weights()
    want, _ = ops.infer(tr.spec, row.clone(), x, want_probs=False)
    with torch.no_grad():
        assert _same(am(x), want) and not _same(am(x), tr.model.eval()(x))
    tr.model.train()
    offs = tr.spec.offsets()
    for k, v in am.state_dict().items():
        assert _same(v.reshape(-1), row[offs[k]:offs[k] + v.numel()]), k
    path = str(tmp_path / "avg.pth")
    save_reference_checkpoint(am, path)
    sd = torch.load(path)
    assert all(torch.equal(sd[k], v.cpu()) for k, v in am.state_dict().items())
    # model batches: evaluate / track_best / restore_best on the averaged rows
    M = 3
    models = lambda: [_ref_model(nsd, dev, ref_state) for _ in range(M)]
    mt = nsd.ModelBatchTrainer(models(), lr=LR, seeds=[1, 2, 3], average=ops.Average("swa"))
    for _ in range(3):
        mt.step(x, y)
    xe, ye = to_dev(synth_x(9, TT, seed=21), dev), to_dev(synth_labels(9, seed=21), dev)
    other = nsd.ModelBatchTrainer(models(), lr=LR, seeds=[1, 2, 3])
    other.params.copy_(mt.averaged_params())
    got, want = mt.evaluate(xe, ye, weights="average"), other.evaluate(xe, ye)
    last = mt.evaluate(xe, ye)
    for g, w, l in zip(got, want, last):
        assert g["loss"] == w["loss"] and g["acc"] == w["acc"] and np.array_equal(g["confusion"], w["confusion"]) and g["loss"] != l["loss"]
    for i, mdl in enumerate(mt.averaged_models()):
        assert _same(mdl.flat_parameters(), mt.averaged_params()[i])
    recs = mt.track_best(xe, ye, weights="average")
    assert [r["best_eval"] for r in recs] == [1] * M
    snap = ops.select_snapshot(mt._sel_state, M, mt.spec.param_count)
    avg_rows = mt.averaged_params().clone()
    assert _same(snap, avg_rows) and not _same(mt.params, avg_rows)
    assert mt.restore_best() == [1] * M and _same(mt.params, avg_rows)
    with pytest.raises(nsd.NsdError, match="'last' or 'average'"):
        mt.evaluate(xe, ye, weights="best")
    with pytest.raises(nsd.NsdError, match="no weight averaging"):
        other.evaluate(xe, ye, weights="average")


def test_bf16_flat_route_follows_the_rule_and_honours_the_guard(nsd, dev):
    from nsd_amd import ops
    from nsd_amd.trainer import Trainer
    torch.manual_seed(11)
    model = nsd.EEG_LSTM(8, 64, 2, 5, dropout=0.6, precision="bf16").to(dev).train()
    avg = ops.Average("ema", 0.9)
    tr = Trainer(model, lr=LR, seed=3, average=avg)
    x, y = to_dev(synth_x(32, 5, seed=4), dev), to_dev(synth_labels(32, 5, seed=4), dev)
    R = _ref(avg)
    names = []
    for s in range(1, 4):
        names = _launches(lambda: tr.step(x, y), steps=1)
        R.update(tr.flat.cpu().numpy(), s)
        assert np.array_equal(_words(tr.averaged_weights()), _words(R.row)), s
    assert names[-2:] == ["nsd_grad_norm", "nsd_adam_step_clip_avg"] and tr.scan_status() == 0 and tr.averaged_count() == 3
    before = (tr.flat.clone(), tr._avg_state.clone(), tr._opt_state[:16].clone())
    tr._skip.fill_(1.0)                                        # what nsd_seq_guard raises after a time-out on any rank
    tr.step_count += 1
    tr._adam()
    torch.cuda.synchronize()
    assert _same(tr.flat, before[0]) and torch.equal(tr._avg_state, before[1]) and torch.equal(tr._opt_state[:16], before[2])
    tr._skip.zero_()
    tr._adam()
    R.update(tr.flat.cpu().numpy(), 4)
    assert not _same(tr.flat, before[0]) and np.array_equal(_words(tr.averaged_weights()), _words(R.row)) and tr.averaged_count() == 4


@pytest.mark.parametrize("kind", ["ema0.999", "swa"])
def test_resume_from_a_state_dict(nsd, dev, ref_state, kind):
    """four steps, state_dict -> a fresh trainer, three steps: bitwise the seven steps of one trainer"""
    from nsd_amd.trainer import Trainer
    x, y = _xy(dev)
    kw = dict(lr=LR, seed=5, clip_grad_norm=0.05, average=_kinds(nsd)[kind])
    ta, tb = Trainer(_ref_model(nsd, dev, ref_state), **kw), Trainer(_ref_model(nsd, dev, ref_state), **kw)
    for _ in range(7):
        ta.step(x, y)
    for _ in range(4):
        tb.step(x, y)
    sd = tb.state_dict()
    assert sd["avg_n"] == 4 and _same(sd["avg_row"], tb.averaged_weights().cpu())
    tc = Trainer(_ref_model(nsd, dev, ref_state), **kw)
    tc.load_state_dict(sd)
    assert tc.averaged_count() == 4
    for _ in range(3):
        tc.step(x, y)
    assert _same(tc.flat, ta.flat) and _same(tc.m, ta.m) and _same(tc.v, ta.v)
    assert _same(tc.averaged_weights(), ta.averaged_weights()) and tc.averaged_count() == ta.averaged_count() == 7


# ---- 7. buffer contract ------------------------------------------------------------------------------------------------------------------
def _contract(ops, dev, n, M, launch, inputs, outputs, off=()):
    """launch(avg_state, *fresh copies of outputs), twice (the first averaged step copies, the second averages), with avg_state of exactly
    nsd_avg_state_bytes between 0xA5 guards, pre-filled with 0xFF bytes / NaN words and then initialised; plain and on a side stream: the
    same bits everywhere, guards intact, inputs unchanged.  off: the models that do not average -- their rows keep the pre-fill, byte for
    byte, and are left out of the comparison between fills"""
    nb = ops.avg_state_bytes(n, M)
    assert nb == 16 * M + 4 * M * n

    def once(fill, side):
        state, check = bc.guarded((nb,), torch.uint8, dev, fill)
        ops._call("nsd_avg_state_init", dev, state.data_ptr(), nb, M, ops.STREAM)
        want = torch.empty_like(state[16 * M:])
        bc.fill_payload(want, fill)
        assert int(state[:16 * M].max()) == 0 and torch.equal(state[16 * M:], want)          # the records zeroed, and nothing else
        outs = [t.clone() for t in outputs]
        snap = bc.snapshot(*inputs)
        torch.cuda.synchronize()
        if side:
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                launch(state, 1, *outs)
                launch(state, 2, *outs)
            torch.cuda.current_stream().wait_stream(st)
        else:
            launch(state, 1, *outs)
            launch(state, 2, *outs)
        torch.cuda.synchronize()
        check("avg_state")
        assert snap.unchanged(), (fill, side, snap.changed())
        final = state.clone()
        for i in off:
            lo = 16 * M + 4 * n * i
            assert torch.equal(final[lo:lo + 4 * n], want[4 * n * i:4 * n * (i + 1)]), (fill, side, i)
            final[lo:lo + 4 * n] = 0
        return [bc._bits(t) for t in outs] + [final]
    base = once("ones", False)
    for fill, side in (("nan32", False), ("ones", True), ("nan32", True)):
        got = once(fill, side)
        assert all(torch.equal(u, w) for u, w in zip(base, got)), (fill, side)
    return base


@pytest.mark.parametrize("n", [31764, 2**20 + 1])
def test_buffer_contract_flat_route(nsd, dev, n):
    from nsd_amd import ops
    p0, gs, norm = _flat_problem(n)
    g, p, m, v = to_dev(gs[0], dev), to_dev(p0, dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    opt, ostate, avg = ops.opt_struct(lr=LR, max_norm=0.1 * norm), ops.opt_state(n, 1, dev), ops.Average("swa")

    def launch(state, s, p, m, v):
        ops.grad_norm(g, ostate)
        ops.adam_step_clip_avg(p, g, m, v, opt, ostate, avg, state, step=s)
    base = _contract(ops, dev, n, 1, launch, [g], [p, m, v])
    assert ops.avg_records(base[-1])[0] == dict(n_avg=2, arrive=0)


def test_buffer_contract_model_batched_tail(nsd, dev):
    from nsd_amd import ops
    M = 3
    b = _batched(M)
    spec, P = b["spec"], b["P"]
    opts = [ops.opt_struct(lr=LR * (1 + i), max_norm=1.0) for i in range(M)]
    avgs = [ops.Average("ema", 0.9), None, ops.Average("swa")]
    ostate, z = ops.opt_state(P, M, dev), torch.zeros_like(b["params"])

    def launch(state, s, g, p, m, v):
        _multi_tail(ops, spec, M, b["ws"], g, p, m, v, opts, ostate, s, avgs, state)
    base = _contract(ops, dev, P, M, launch, [b["ws"]], [torch.empty_like(b["params"]), b["params"], z, z], off=(1,))
    assert [r["n_avg"] for r in ops.avg_records(base[-1], M)] == [2, 0, 2]
