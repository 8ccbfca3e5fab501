"""Supervised session alignment on the MI355X (nsd_spatial_bwd / nsd_spatial_fit_step of include/nsd.h, csrc/nsd_align.hip;
nsd_amd.SpatialFit) against the numpy restatements of tests/spatial_fit_ref.py: both kernels BIT FOR BIT over the shapes at which
they take another path (one step, both sides of the 64-step tile of the apply's kernel and of the 128-step tile of dW's stage 1, C not a multiple of 4 -- the dword route -- and C = 32, four matrix
entries per thread), the buffer contract, the chain rule through the frozen model against the oracle's dx, the fit's eager, replayed
and continued runs, and autograd through ops.spatial_apply and EEG_LSTM(align=, align_grad=True).

The chain rule's bound carries the project's own dx bound through the sum, with no new number: dA[i][j] = sum_{b,t} dx[b,t,i] v[b,t,j], and
every dx element is within DX_TOL * max|dx| of the oracle's, so entry (i, j) is within DX_TOL * max|dx| * sum_{b,t} |v[b,t,j]|."""
import numpy as np
import pytest
import torch

from tests import spatial_fit_ref as sr
from tests.buffer_contract import guarded, snapshot
from tests.gpu_harness import (D, DX_TOL, LOSS_TOL, dev, head_inputs, nsd, oracle_step, spec_of, sync_at_the_end, to_dev,  # noqa: F401  (fixtures)
                               train_step)

pytestmark = pytest.mark.gpu

# the issue's shapes, and one more for stage 1 of dW: two full tiles of 128 steps, whole groups of 8 steps and a remainder
SHAPES = [(1, 1, 1), (3, 5, 3), (5, 64, 4), (2, 65, 8), (4, 129, 7), (2, 3, 32), (3, 300, 8)]


def _problem(B, T, Cc, n_mat=1, seed=0):
    rs = np.random.RandomState(seed + 100 * B + 10 * T + Cc)
    v = (10.0 * rs.standard_normal((B, T, Cc))).astype(np.float32)
    dy = (1e-3 * rs.standard_normal((B, T, Cc))).astype(np.float32)
    W = (np.eye(Cc) + 0.3 * rs.standard_normal((n_mat, Cc, Cc))).astype(np.float32)
    return v, dy, W


def _bwd(dev, v, dy, W, sel=None, **kw):
    from nsd_amd import ops
    dv, dW, counts = ops.spatial_bwd(to_dev(v, dev), to_dev(dy, dev), to_dev(W, dev),
                                     sel=None if sel is None else to_dev(np.asarray(sel, np.int32), dev), **kw)
    return tuple(None if t is None else t.cpu().numpy() for t in (dv, dW, counts))


def _same(got, want):
    return all(sr.same_bits(g, w) for g, w in zip(got, want))


# ---- nsd_spatial_bwd ----
@pytest.mark.parametrize("B,T,Cc", SHAPES)
def test_bwd_equals_the_restatement_bitwise(nsd, dev, B, T, Cc):
    v, dy, W = _problem(B, T, Cc)
    want = sr.bwd_ref(v, dy, W)
    got = _bwd(dev, v, dy, W)
    assert _same(got, want), (B, T, Cc)
    assert got[2].tolist() == [B, 0]
    # dv only and dW only: the bits of the pair
    only_dv = _bwd(dev, v, dy, W, want_dW=False)
    only_dW = _bwd(dev, v, dy, W, want_dv=False)
    assert only_dv[1] is None and only_dv[2] is None and sr.same_bits(only_dv[0], want[0])
    assert only_dW[0] is None and sr.same_bits(only_dW[1], want[1]) and only_dW[2].tolist() == [B, 0]


@pytest.mark.parametrize("B,T,Cc", [(5, 64, 4), (4, 129, 7), (6, 3, 32)])
def test_bwd_with_a_matrix_table_and_rows_outside_it(nsd, dev, B, T, Cc):
    v, dy, W = _problem(B, T, Cc, n_mat=3, seed=2)
    sel = np.array([2, -1, 0, 3, 2, 0][:B])
    want = sr.bwd_ref(v, dy, W, sel)
    got = _bwd(dev, v, dy, W, sel)
    assert _same(got, want)
    left = [b for b in range(B) if not 0 <= sel[b] < 3]
    assert np.isnan(got[0][left]).all() and np.isfinite(np.delete(got[0], left, axis=0)).all()
    assert got[2].tolist() == [B - len(left), len(left)] and not got[1][1].any()     # no row selects matrix 1: zeros
    keep = [b for b in range(B) if b not in left]
    assert sr.same_bits(_bwd(dev, v[keep], dy[keep], W, sel[keep])[1], got[1])        # the rows are left out of dW


@pytest.mark.parametrize("B,T,Cc", [(2, 65, 8), (5, 64, 4)])
def test_bwd_misaligned_input_takes_the_dword_route(nsd, dev, B, T, Cc):
    from nsd_amd import ops
    v, dy, W = _problem(B, T, Cc, seed=4)
    want = sr.bwd_ref(v, dy, W)
    n = v.size
    fv, fy = torch.zeros(n + 4, device=dev), torch.zeros(n + 4, device=dev)
    xv, xy = fv[1:1 + n].view(v.shape), fy[1:1 + n].view(v.shape)                     # 4 bytes off a 16-byte boundary
    xv.copy_(to_dev(v, dev)); xy.copy_(to_dev(dy, dev))
    assert xv.data_ptr() % 16 == 4 and xy.data_ptr() % 16 == 4
    dv, dW, counts = ops.spatial_bwd(xv, xy, to_dev(W, dev))
    assert _same((dv.cpu().numpy(), dW.cpu().numpy(), counts.cpu().numpy()), want)


def test_bwd_one_nan_reaches_exactly_its_step_and_its_entries(nsd, dev):
    B, T, Cc = 3, 70, 8
    v, dy, W = _problem(B, T, Cc, n_mat=2, seed=6)
    sel = np.array([0, 1, 0])
    clean = _bwd(dev, v, dy, W, sel)
    dy2 = dy.copy()
    dy2[1, 64, 5] = np.nan
    want = sr.bwd_ref(v, dy2, W, sel)
    got = _bwd(dev, v, dy2, W, sel)
    assert _same(got, want)
    nan_dv, nan_dW = np.isnan(got[0]), np.isnan(got[1])
    assert nan_dv[1, 64].all() and nan_dv.sum() == Cc and nan_dW[1, 5].all() and nan_dW.sum() == Cc
    assert sr.same_bits(np.where(nan_dv, 0, got[0]), np.where(nan_dv, 0, clean[0]))
    assert sr.same_bits(np.where(nan_dW, 0, got[1]), np.where(nan_dW, 0, clean[1]))
    v2 = v.copy()
    v2[2, 0, 3] = np.inf                                                              # in v: column j = 3 of trial 2's matrix, no dv
    got = _bwd(dev, v2, dy, W, sel)
    assert _same(got, sr.bwd_ref(v2, dy, W, sel)) and np.isfinite(got[0]).all()
    assert (~np.isfinite(got[1]))[0, :, 3].all() and (~np.isfinite(got[1])).sum() == Cc


@pytest.mark.parametrize("B,T,Cc", [(4, 129, 7), (5, 64, 4), (2, 3, 32)])
def test_bwd_buffer_contract_side_stream_and_graph_replay(nsd, dev, B, T, Cc):
    from nsd_amd import ops
    n_mat = 2
    v, dy, W = _problem(B, T, Cc, n_mat=n_mat, seed=8)
    sel = np.arange(B) % n_mat
    want = sr.bwd_ref(v, dy, W, sel)
    xv, xy, xw, xs = to_dev(v, dev), to_dev(dy, dev), to_dev(W, dev), to_dev(sel.astype(np.int32), dev)
    assert ops.spatial_bwd_scratch_bytes(B, T, Cc) == B * Cc * Cc * 8
    bufs = {}

    def outputs():
        bufs.clear()
        for name, shape, dt in (("dv", (B, T, Cc), torch.float32), ("dW", (n_mat, Cc, Cc), torch.float32), ("counts", (2,), torch.int64),
                                ("scratch", (B * Cc * Cc,), torch.float64)):
            bufs[name] = guarded(shape, dt, dev, "nan32")
        return {k: b[0] for k, b in bufs.items()}

    def checked(out):
        for name, (_, check) in bufs.items():
            check(name)
        assert snap.unchanged()
        return _same((out["dv"].cpu().numpy(), out["dW"].cpu().numpy(), out["counts"].cpu().numpy()), want)

    snap = snapshot(xv, xy, xw, xs)
    out = outputs()
    ops.spatial_bwd(xv, xy, xw, sel=xs, **out)
    assert checked(out)
    # a side stream
    out = outputs()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.spatial_bwd(xv, xy, xw, sel=xs, **out)
    torch.cuda.current_stream().wait_stream(side)
    assert checked(out)
    # a replayed graph: the bits do not depend on it
    out = outputs()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.spatial_bwd(xv, xy, xw, sel=xs, **out)
    g.replay()
    g.replay()
    assert checked(out)
    # a scratch one double short is refused and nothing is written
    out = outputs()
    before = {k: t.clone() for k, t in out.items()}
    with pytest.raises(nsd.NsdError, match="scratch"):
        ops.spatial_bwd(xv, xy, xw, sel=xs, **dict(out, scratch=out["scratch"][:-1]))
    assert all(torch.equal(out[k].view(torch.uint8), before[k].view(torch.uint8)) for k in out)


# ---- nsd_spatial_fit_step ----
def _fit_problem(Cc, n_mat, steps, seed=0):
    rs = np.random.RandomState(seed + Cc)
    A = (np.eye(Cc)[None] + 0.1 * rs.standard_normal((n_mat, Cc, Cc))).astype(np.float32)
    prior = np.broadcast_to(np.eye(Cc, dtype=np.float32), A.shape).copy()
    gs = [(1e-2 * rs.standard_normal((n_mat, Cc, Cc))).astype(np.float32) for _ in range(steps)]
    return A, prior, gs


def _state_equals(ops, Cc, n_mat, state, ref):
    recs = ops.spatial_fit_records(Cc, n_mat, state)
    return all(sr.same_bits(r["m"], ref.m[k]) and sr.same_bits(r["v"], ref.v[k]) and r["step"] == ref.step_count[k]
               and r["skipped"] == ref.skipped[k] and r["status"] == ref.status[k] and r["calls"] == ref.calls for k, r in enumerate(recs))


@pytest.mark.parametrize("Cc,n_mat", [(8, 1), (3, 3), (32, 2)])
def test_fit_step_equals_the_restatement_bitwise_and_continues(nsd, dev, Cc, n_mat):
    from nsd_amd import ops
    A0, prior, gs = _fit_problem(Cc, n_mat, 3)
    kw = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, decay=0.1)
    ref, want = sr.FitRef(Cc, n_mat), A0.copy()
    A, P = to_dev(A0, dev), to_dev(prior, dev)
    state = ops.spatial_fit_state(Cc, n_mat, dev)
    snap = snapshot(P)
    for s, g in enumerate(gs):
        ref.step(want, g, prior, **kw)
        ops.spatial_fit_step(A, to_dev(g, dev), state, A0=P, **kw)
        assert sr.same_bits(A.cpu().numpy(), want), s
        assert _state_equals(ops, Cc, n_mat, state, ref), s
    assert snap.unchanged()
    # 2 + 1 steps with the state carried by the caller: the bits of 3
    A2, state2 = to_dev(A0, dev), ops.spatial_fit_state(Cc, n_mat, dev)
    for g in gs[:2]:
        ops.spatial_fit_step(A2, to_dev(g, dev), state2, A0=P, **kw)
    carried = state2.clone()
    ops.spatial_fit_step(A2, to_dev(gs[2], dev), carried, A0=P, **kw)
    assert torch.equal(A2, A) and torch.equal(carried, state)
    # no prior: no pull
    A3, state3 = to_dev(A0, dev), ops.spatial_fit_state(Cc, n_mat, dev)
    ops.spatial_fit_step(A3, to_dev(gs[0], dev), state3, **kw)
    ref3, want3 = sr.FitRef(Cc, n_mat), A0.copy()
    ref3.step(want3, gs[0], None, **kw)
    assert sr.same_bits(A3.cpu().numpy(), want3)


def test_fit_step_replayed_from_a_graph_advances_its_counter_and_records_the_loss(nsd, dev):
    from nsd_amd import ops
    Cc, n_mat, steps, cap = 8, 2, 4, 3
    A0, prior, gs = _fit_problem(Cc, n_mat, 1, seed=3)
    kw = dict(lr=3e-3, decay=0.05)
    ref, want, want_loss = sr.FitRef(Cc, n_mat), A0.copy(), np.full(cap, np.nan, np.float32)
    for _ in range(steps):
        ref.step(want, gs[0], prior, loss_in=2.25, loss_out=want_loss, **kw)
    A, P, g = to_dev(A0, dev), to_dev(prior, dev), to_dev(gs[0], dev)
    state = ops.spatial_fit_state(Cc, n_mat, dev)
    loss_in = torch.full((1,), 2.25, device=dev)
    loss_out, check = guarded((cap,), torch.float32, dev, "nan32")
    ops.spatial_fit_step(A, g, state, A0=P, loss_in=loss_in, loss_out=loss_out, **kw)        # step 1 eagerly (and the warm-up)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.spatial_fit_step(A, g, state, A0=P, loss_in=loss_in, loss_out=loss_out, **kw)
    for _ in range(steps - 1):
        graph.replay()
    assert sr.same_bits(A.cpu().numpy(), want) and _state_equals(ops, Cc, n_mat, state, ref)
    assert ref.step_count.tolist() == [steps] * n_mat
    check("loss_out")                                                                         # call 4 is past the cap: not written
    assert sr.same_bits(loss_out.cpu().numpy(), want_loss) and want_loss.tolist() == [2.25] * cap


def test_fit_step_a_nonfinite_gradient_stops_its_matrix_alone(nsd, dev):
    from nsd_amd import ops
    Cc, n_mat = 7, 3
    A0, prior, gs = _fit_problem(Cc, n_mat, 2, seed=5)
    kw = dict(lr=1e-2, decay=0.1)
    A, P = to_dev(A0, dev), to_dev(prior, dev)
    state = ops.spatial_fit_state(Cc, n_mat, dev)
    ops.spatial_fit_step(A, to_dev(gs[0], dev), state, A0=P, **kw)
    lay = ops.spatial_fit_layout(Cc)
    slot1 = state[int(lay.stride):2 * int(lay.stride)].clone()
    A_before = A.clone()
    bad = gs[1].copy()
    bad[1, 6, 6] = np.nan
    ops.spatial_fit_step(A, to_dev(bad, dev), state, A0=P, **kw)
    ref, want = sr.FitRef(Cc, n_mat), A0.copy()
    ref.step(want, gs[0], prior, **kw)
    ref.step(want, bad, prior, **kw)
    assert sr.same_bits(A.cpu().numpy(), want) and _state_equals(ops, Cc, n_mat, state, ref)
    assert torch.equal(A[1], A_before[1]) and not torch.equal(A[0], A_before[0]) and not torch.equal(A[2], A_before[2])
    now = state[int(lay.stride):2 * int(lay.stride)]
    upto = int(lay.skipped)                                                                   # m, v and the step counter: bitwise unchanged
    assert torch.equal(now[:upto], slot1[:upto])
    recs = ops.spatial_fit_records(Cc, n_mat, state)
    assert [r["status"] for r in recs] == [0, ops.SPATIAL_FIT_NONFINITE, 0] and [r["skipped"] for r in recs] == [0, 1, 0]
    assert [r["step"] for r in recs] == [2, 1, 2]
    # a prior that is not finite is a g that is not finite
    Pbad = P.clone()
    Pbad[0, 0, 0] = float("inf")
    ops.spatial_fit_step(A, to_dev(gs[1], dev), state, A0=Pbad, **kw)
    assert [r["skipped"] for r in ops.spatial_fit_records(Cc, n_mat, state)] == [1, 1, 0]


def test_fit_step_refusals_leave_guarded_outputs_untouched(nsd, dev):
    from nsd_amd import ops
    Cc, n_mat = 8, 2
    A0, prior, gs = _fit_problem(Cc, n_mat, 1, seed=7)
    A, checkA = guarded((n_mat, Cc, Cc), torch.float32, dev, "nan32")
    A.copy_(to_dev(A0, dev))
    nbytes = int(ops.spatial_fit_state(Cc, n_mat, dev).numel())
    state, checkS = guarded((nbytes,), torch.uint8, dev, "zeros")
    loss_out, checkL = guarded((2,), torch.float32, dev, "nan32")
    g, loss_in = to_dev(gs[0], dev), torch.ones(1, device=dev)
    snap = snapshot(A, state, loss_out)
    ok = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, decay=1e-2)
    for field, value in (("lr", -1.0), ("lr", float("nan")), ("decay", -1e-3), ("decay", float("inf")), ("beta1", 1.0), ("beta2", -0.5),
                         ("eps", 0.0), ("eps", float("nan"))):
        with pytest.raises(nsd.NsdError, match=field):
            ops.spatial_fit_step(A, g, state, loss_in=loss_in, loss_out=loss_out, **dict(ok, **{field: value}))
    with pytest.raises(nsd.NsdError, match="state"):
        ops.spatial_fit_step(A, g, state[:-8], loss_in=loss_in, loss_out=loss_out, **ok)
    torch.cuda.synchronize()
    assert snap.unchanged()
    # ... and the accepted call writes inside the guards only
    ops.spatial_fit_step(A, g, state, loss_in=loss_in, loss_out=loss_out, **ok)
    for check, name in ((checkA, "A"), (checkS, "state"), (checkL, "loss_out")):
        check(name)
    assert not snap.unchanged() and loss_out.cpu().numpy()[0] == 1.0 and np.isnan(loss_out.cpu().numpy()[1])


# ---- the chain rule through the frozen model ----
def test_dA_through_the_model_against_the_oracles_dx(nsd, dev):
    from nsd_amd import ops
    B, T = 4, 20
    d, flat, x, y, masks = head_inputs(D.C, D.H, D.K, D.F, B, T)
    spec = spec_of(d)
    rs = np.random.RandomState(11)
    a = 0.15 * rs.standard_normal((D.C, D.C))
    W = (np.eye(D.C) + a).astype(np.float32)
    xa = ops.spatial_apply(to_dev(x, dev), to_dev(W, dev)).cpu().numpy()
    out = train_step(dev, spec, flat, xa, labels=y, masks=masks, want_dx=True)
    _, dA, counts = ops.spatial_bwd(to_dev(x, dev), to_dev(out["dx"], dev), to_dev(W, dev), want_dv=False)
    ref = oracle_step(d, flat, xa, labels=y, masks=masks, want_dx=True)
    dx64, v64 = ref["dx"].astype(np.float64), x.astype(np.float64)
    want = np.einsum("bti,btj->ij", dx64, v64)
    bound = DX_TOL * np.abs(dx64).max() * np.abs(v64).sum(axis=(0, 1))[None, :]
    err = np.abs(dA[0].cpu().numpy().astype(np.float64) - want)
    print(f"dA vs oracle: worst error / bound {float((err / bound).max()):.3e}; largest |dA| {float(np.abs(want).max()):.3e}")
    assert np.isfinite(err).all() and (err <= bound).all(), float((err / bound).max())
    assert counts.tolist() == [B, 0] and np.abs(want).max() > 0


# ---- SpatialFit ----
def _eval_model(nsd, dev, ref_state, **kw):
    m = nsd.EEG_LSTM(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in ref_state.items()}, strict=True)
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def shifted(golden):
    """6 recorded trials (their first 20 steps) mixed by a fixed 8 x 8 matrix, and labels: the reference's decisions on the whole trials"""
    z = golden("real_trials")
    rs = np.random.RandomState(21)
    M = (np.eye(8) + 0.25 * rs.standard_normal((8, 8))).astype(np.float32)
    x = np.ascontiguousarray(z["x"][:6, :20].astype(np.float32) @ M.T)
    return x, z["argmax"][:6].astype(np.int64)


def test_spatial_fit_eager_replayed_and_continued_runs_agree(nsd, dev, ref_state, shifted):
    from nsd_amd import ops
    x, y = shifted
    kw = dict(lr=1e-4, decay=0.0)
    runs = {}
    for name, graph in (("eager", False), ("graph", True), ("2+3", None)):
        model = _eval_model(nsd, dev, ref_state)
        snap = snapshot(model.flat_parameters())
        fit = nsd.SpatialFit(model, epochs=5, graph=graph, **kw)
        if name == "2+3":
            losses = torch.cat([fit.fit(x, y, epochs=2), fit.fit(x, y, epochs=3)])
        else:
            losses = fit.fit(x, y)
        assert snap.unchanged()                                                       # the model's parameters are never written
        assert fit.replayed == (name != "eager") and fit.status() == [0] and fit.epochs_done() == 5
        fit.check()
        runs[name] = (losses.cpu().numpy(), fit.A.cpu().numpy(), model)
    for name in ("graph", "2+3"):
        assert sr.same_bits(runs[name][0], runs["eager"][0]) and sr.same_bits(runs[name][1], runs["eager"][1]), name
    losses, A, model = runs["eager"]
    print("SpatialFit losses", losses)
    assert np.isfinite(losses).all() and losses[1] < losses[0]
    # set_alignment has been called with the fitted matrix, and predict_proba uses it
    assert sr.same_bits(model.align_matrix.cpu().numpy(), A[0] if A.ndim == 3 else A)
    rec = model.align_record["spatial_fit"]
    assert rec["epochs"] == 5 and rec["lr"] == 1e-4 and rec["decay"] == 0.0 and rec["status"] == 0
    assert rec["loss_first"] == float(losses[0]) and rec["loss_last"] == float(losses[-1])
    plain = _eval_model(nsd, dev, ref_state)
    xt = to_dev(x, dev)
    with torch.no_grad():
        want = plain.predict_proba(ops.spatial_apply(xt, model.align_matrix))
    assert torch.equal(model.predict_proba(xt), want) and not torch.equal(want, plain.predict_proba(xt))


def test_spatial_fit_first_step_moves_every_entry_by_lr_against_its_gradient(nsd, dev, ref_state, shifted):
    from nsd_amd import ops
    x, y = shifted
    lr = 1e-4
    model = _eval_model(nsd, dev, ref_state)
    fit = nsd.SpatialFit(model, epochs=1, lr=lr, decay=0.0)
    losses = fit.fit(x, y)
    # the gradient the fit used, formed with the fit's own launches at A = I: apply -> train_dx -> spatial_bwd, bit for bit its dA
    xt, eye = to_dev(x, dev), torch.eye(8, device=dev)
    sp, flat = model.spec, model.flat_parameters()
    N, T = x.shape[0], x.shape[1]
    xa, dx = ops.spatial_apply(xt, eye), torch.empty_like(xt)
    ws, logits, loss1 = ops.new_workspace(sp, N, T, dev), torch.empty((N, sp.K), device=dev), torch.zeros(1, device=dev)
    ops.train_dx(sp, flat, xa, ws, logits, dx, labels=to_dev(y.astype(np.int32), dev), loss_out=loss1)
    _, dA, _ = ops.spatial_bwd(xt, dx, eye, want_dv=False)
    g = dA[0].cpu().numpy()
    assert abs(float(loss1) / N - float(losses[0])) <= 2.0 ** -22 * abs(float(losses[0]))   # (the same launches; one fp32 division apart)
    # ... so the fitted matrix is the restated step from the identity, bit for bit (decay 0 with a prior adds 0 * (A - A0))
    ref, want = sr.FitRef(8, 1), np.eye(8, dtype=np.float32)[None].copy()
    ref.step(want, g[None], np.eye(8, dtype=np.float32)[None], lr=lr, decay=0.0)
    got = fit.A.cpu().numpy()
    assert sr.same_bits(got, want[0])
    # EVERY entry moves against its gradient's sign, by lr * |g| / (|g| + eps): m^ = g and sqrt(v^) = |g| at step 1.  The bound: the
    # fp32 evaluation of the update takes fewer than 16 roundings (16 * 2^-24 of lr), and A - update rounds once, to half an ulp of an
    # entry in [1, 2): 2^-24.  For |g| >= 1e-4, a thousand times eps and more, that is lr itself within 1e-3 of lr.
    moved = got.astype(np.float64) - np.eye(8)
    g64 = np.abs(g.astype(np.float64))
    expect = lr * g64 / (g64 + 1e-8)
    tol = 2.0 ** -24 + 16 * 2.0 ** -24 * lr
    large = g64 >= 1e-4
    print(f"first step: {g.size} entries, smallest |g| {g64.min():.3e}, largest {g64.max():.3e}; {int(large.sum())} with |g| >= 1e-4; "
          f"worst | |moved| - lr |g| / (|g| + eps) | = {np.abs(np.abs(moved) - expect).max():.3e} (bound {tol:.3e})")
    assert g.shape == (8, 8) and (np.sign(moved) == -np.sign(g)).all()
    assert (np.abs(np.abs(moved) - expect) <= tol).all()
    assert large.any() and (np.abs(np.abs(moved[large]) - lr) <= 1e-3 * lr).all()
    # the same stage through autograd: ops.spatial_apply as a node in front of a twin, mean cross-entropy behind it.  At W = I the
    # serial sum makes x.grad the model's dx itself, so W.grad is nsd_spatial_bwd of (x, x.grad), bit for bit
    plain = _eval_model(nsd, dev, ref_state)
    W = torch.eye(8, device=dev, requires_grad=True)
    xg = to_dev(x, dev).requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(plain(ops.spatial_apply(xg, W)), to_dev(y, dev))
    loss.backward()
    assert abs(float(loss.detach()) - float(losses[0])) < LOSS_TOL                   # (the loss of two launch sequences)
    _, dW_auto, _ = ops.spatial_bwd(xt, xg.grad, eye, want_dv=False)
    assert W.grad.shape == (8, 8) and torch.equal(W.grad, dW_auto[0]) and bool(torch.isfinite(W.grad).all())
    # label smoothing builds target rows; mixup is refused
    soft = nsd.SpatialFit(_eval_model(nsd, dev, ref_state), epochs=2, lr=lr, decay=0.0, loss=nsd.Loss(label_smoothing=0.1))
    ls = soft.fit(x, y).cpu().numpy()
    assert np.isfinite(ls).all() and ls[0] != float(losses[0]) and soft.status() == [0]
    with pytest.raises(nsd.NsdError, match="mixup"):
        nsd.SpatialFit(model, loss=nsd.Loss(mixup=0.5))


def test_spatial_fit_starts_from_the_whitening_matrix_and_pulls_towards_it(nsd, dev, ref_state, shifted):
    x, y = shifted
    A = nsd.SessionAlign()
    model = _eval_model(nsd, dev, ref_state, align=A)
    Wh, _ = A.fit(model, x)
    model.set_alignment(Wh[0], record={"steps": 120, "status": 0})
    fit = nsd.SpatialFit(model, epochs=3, lr=1e-4, decay=1e-2)
    assert torch.equal(fit.A0, Wh[0]) and torch.equal(fit.A, Wh[0])
    fit.fit(x, y)
    assert not torch.equal(model.align_matrix, Wh[0]) and float((model.align_matrix - Wh[0]).abs().max()) <= 1e-3   # (three Adam steps of at most 3.2 lr each)
    assert model.align_record["steps"] == 120 and model.align_record["spatial_fit"]["epochs"] == 3
    # a non-finite step in the frozen input: every epoch is refused on the device, the matrix stays
    bad = x.copy()
    bad[2, 7, 1] = np.nan
    stuck = nsd.SpatialFit(_eval_model(nsd, dev, ref_state), epochs=2)
    stuck.fit(bad, y)
    assert stuck.status() == [1] and stuck.epochs_done() == 0 and torch.equal(stuck.A, torch.eye(8, device=dev))
    with pytest.raises(nsd.NsdError, match="not finite"):
        stuck.check()
    stuck.reset()
    assert stuck.status() == [0]


# ---- autograd ----
def test_input_gradient_through_an_aligned_model(nsd, dev, ref_state, shifted):
    from nsd_amd import ops
    x, _ = shifted
    rs = np.random.RandomState(31)
    W = to_dev((np.eye(8) + 0.2 * rs.standard_normal((8, 8))).astype(np.float32), dev)
    A = nsd.SessionAlign()
    m = _eval_model(nsd, dev, ref_state, align=A, align_matrix=W, align_grad=True)
    plain = _eval_model(nsd, dev, ref_state)
    xt = to_dev(x, dev).requires_grad_(True)
    la = m(xt).square().sum()
    la.backward()
    xa = ops.spatial_apply(to_dev(x, dev), W).requires_grad_(True)
    lb = plain(xa).square().sum()
    lb.backward()
    assert torch.equal(la, lb)
    want, _, _ = ops.spatial_bwd(to_dev(x, dev), xa.grad, W, want_dW=False)
    assert xt.grad is not None and torch.equal(xt.grad, want) and bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
    for (n, a), (_, b) in zip(m.named_parameters(), plain.named_parameters()):
        assert torch.equal(a.grad, b.grad), n
    # with gradients off the stage is the plain launch; gate= and prep= still refuse, with or without the switch
    with torch.no_grad():
        assert torch.equal(m(to_dev(x, dev)), plain(ops.spatial_apply(to_dev(x, dev), W)))
    G = nsd.SignalGate(rail=100.0, hold_samples=2, max_bad=2)
    P = nsd.CausalPrep.design(highpass=1.0, lowpass=40.0, zscore_seconds=0.4, var0=250.0, car=True)
    with pytest.raises(nsd.NsdError, match="dx through the signal-quality gate"):
        _eval_model(nsd, dev, ref_state, align=A, align_grad=True, gate=G)(to_dev(x, dev).requires_grad_(True))
    with pytest.raises(nsd.NsdError, match="dx through the causal front end"):
        _eval_model(nsd, dev, ref_state, align=A, align_grad=True, prep=P)(to_dev(x, dev).requires_grad_(True))
    with pytest.raises(nsd.NsdError, match="dx through the session alignment"):
        _eval_model(nsd, dev, ref_state, align=A)(to_dev(x, dev).requires_grad_(True))


# ---- calibrate: the launches without the stage, the stage's own, the report and the checkpoint ----
def _names_of(fn):
    import contextlib
    from nsd_amd import ops
    names = []

    @contextlib.contextmanager
    def hook(name):
        names.append(name)
        yield
    ops.set_launch_hook(hook)
    try:
        out = fn()
    finally:
        ops.set_launch_hook(None)
    return names, out


NEW = ("nsd_spatial_bwd", "nsd_spatial_fit_step")


def test_calibrate_runs_the_spatial_stage_only_where_asked(nsd, dev, ref_state, shifted, tmp_path):
    from nsd_amd import ops
    from nsd_amd.trainer import save_reference_checkpoint
    from tests.gpu_harness import write_pth
    x, y = shifted
    path = write_pth(str(tmp_path), ref_state)
    plain = nsd.SimplePredictor(path, sr=125, preprocess="identity")
    names, rep = _names_of(lambda: plain.calibrate(x, y, epochs=3))
    assert not any(n in NEW for n in names) and "nsd_spatial_apply" not in names and plain.model.align is None
    assert "spatial_losses" not in rep and "acc_spatial" not in rep
    again = nsd.SimplePredictor(path, sr=125, preprocess="identity")
    names2, _ = _names_of(lambda: again.calibrate(x, y, epochs=3, spatial=None))
    assert names2 == names                                                            # spatial=None: the launches of the call without it
    # an aligned model with gradients off: the apply's one launch, nothing of the backward
    W = to_dev((np.eye(8) + 0.1).astype(np.float32), dev)
    m = _eval_model(nsd, dev, ref_state, align=nsd.SessionAlign(), align_matrix=W, align_grad=True)
    names3, _ = _names_of(lambda: m.predict_proba(to_dev(x, dev)))
    assert names3.count("nsd_spatial_apply") == 1 and not any(n in NEW for n in names3)
    # with the stage: the epoch's six calls, the report, the record, the checkpoint
    pred = nsd.SimplePredictor(path, sr=125, preprocess="identity")
    snap = snapshot(*[p for n, p in pred.model.named_parameters() if n.startswith("lstm.") or n.startswith("attn")])
    names4, rep = _names_of(lambda: pred.calibrate(x, y, epochs=3, spatial=dict(epochs=2, lr=1e-4, decay=0.0, graph=False)))
    k = names4.index("nsd_spatial_bwd")
    assert names4[k - 4:k + 2] == ["nsd_spatial_apply", "nsd_lstm_head_train", "nsd_lstm_bwd", "nsd_loss_sum", "nsd_spatial_bwd",
                                   "nsd_spatial_fit_step"]
    assert names4.count("nsd_spatial_bwd") == 2 and names4.count("nsd_spatial_fit_step") == 2
    assert names4.index("nsd_head_fit") > len(names4) - 1 - names4[::-1].index("nsd_spatial_fit_step")     # spatial fit, then the head fit
    assert snap.unchanged()                                                           # the LSTM stack and the attention: frozen
    assert rep["spatial_losses"].shape == (2,) and rep["spatial_status"] == [0] and 0.0 <= rep["acc_spatial"] <= 1.0
    assert np.isfinite(rep["loss_spatial"]) and rep["spatial_losses"][1] < rep["spatial_losses"][0]
    assert pred.model.align is not None and pred.model.align_record["spatial_fit"]["epochs"] == 2
    out = str(tmp_path / "fitted.pth")
    save_reference_checkpoint(pred.model, out)
    state = torch.load(out, map_location="cpu", weights_only=True)
    assert state["nsd_align"]["record"]["spatial_fit"]["lr"] == 1e-4
    back = nsd.SimplePredictor(out, sr=125, preprocess="identity")
    xt = to_dev(x, dev)
    assert torch.equal(back.model.align_matrix, pred.model.align_matrix) and back.model.align_record == pred.model.align_record
    assert torch.equal(back.model.predict_proba(xt), pred.model.predict_proba(xt))
    # refusals come before anything runs: the predictor, its matrix (a whitening refit would write it) and its head stay as they were
    snap_all = snapshot(pred.model.flat_parameters(), pred.model.align_matrix)
    for kw, what, exc in ((dict(spatial={}, chunk_transform=lambda c: c), "chunk_transform", nsd.NsdError),
                          (dict(spatial=dict(lr=-1.0)), "lr", ValueError)):
        names5, _ = _names_of(lambda: pytest.raises(exc, pred.calibrate, x, y, align=True, **kw).match(what))
        assert names5 == [] and snap_all.unchanged(), what
    ens = nsd.EnsemblePredictor([path, path], 125, preprocess="identity")
    names6, _ = _names_of(lambda: pytest.raises(nsd.NsdError, ens.calibrate, x, y, spatial={}).match("ensemble"))
    assert names6 == []
