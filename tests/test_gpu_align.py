"""Session alignment on the MI355X (nsd_cov_step / nsd_whiten_fit / nsd_spatial_apply of include/nsd.h, csrc/nsd_align.hip) against the
numpy restatements of tests/align_ref.py: the accumulator and the apply stage BIT FOR BIT (window mode over the shapes at which the
kernels take another path -- the tile of 64 steps, one to four matrix entries per thread, 16-byte and dword staging; stream mode over
cuts, slots, HIP streams and a graph replay), the fit against a float64 eigh within twice the fp32 rounding of the largest element,
every status bit on its own, the buffer contract (every output between 0xA5 guards, every input checked unchanged), and the path
through the Python layers.

The fit's bound: |W - W_ref| <= 2^-23 * max|W_ref| elementwise.  The fp32 rounding of an element is at most 2^-24 of the largest one,
the double eigen-solve's error is orders below that at condition numbers up to 1e4; the bound is twice the rounding.
NSD_WHITEN_NOT_CONVERGED has no test here: the sweep cap is a constant of the library, and no finite symmetric matrix of 32 channels
is known to need 40 sweeps."""
import numpy as np
import pytest
import torch

from tests import align_ref as ar
from tests.buffer_contract import guarded, snapshot
from tests.gpu_harness import dev, nsd, sync_at_the_end, to_dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

FIT_BOUND = 2.0 ** -23


def _scattered(B, T, Cc, seed=0):
    """noise of EEG size with a NaN sample, an Inf sample and nonzero mask words where the shape has room, at the edges of the 64-step
    tile among other places -> (v [B,T,C] fp32, mask [B,T] uint32)"""
    rs = np.random.RandomState(seed + 1000 * B + 10 * T + Cc)
    v = (10.0 * rs.standard_normal((B, T, Cc))).astype(np.float32)
    mask = np.zeros((B, T), np.uint32)
    if T >= 3:
        v[0, T // 2, Cc - 1] = np.nan
        v[B - 1, T - 1, 0] = np.inf
        mask[B - 1, 0] = 5
        mask[0, 1] = 0x80000000
    for t in (63, 64):
        if t < T - 1:
            mask[(t + 1) % B, t] = 1 << (t % 32)
            v[t % B, t, (t * 7) % Cc] = -np.inf if t == 63 else np.nan
    return v, mask


def _mask_dev(mask, dev):
    return to_dev(mask.view(np.int32), dev)


def _cov_window(dev, v, mask):
    """ops.cov_step in window mode into guarded outputs -> numpy (sums, counts); the inputs are checked to be unchanged"""
    from nsd_amd import ops
    B, T, Cc = v.shape
    x, m = to_dev(v, dev), None if mask is None else _mask_dev(mask, dev)
    sums, check_s = guarded((B, Cc, Cc), torch.float64, dev, "ones")
    counts, check_c = guarded((B, 2), torch.int64, dev, "ones")
    snap = snapshot(x, m)
    out = ops.cov_step(x, mask=m, out=(sums, counts))
    assert out[0] is sums and out[1] is counts and snap.unchanged()
    check_s("sums")
    check_c("counts")
    return sums.cpu().numpy(), counts.cpu().numpy()


@pytest.mark.parametrize("Cc", [1, 3, 8, 32])
def test_cov_window_mode_equals_the_reference_bitwise(nsd, dev, Cc):
    for T in (1, 63, 64, 65, 250):
        for B in (1, 5):
            v, mask = _scattered(B, T, Cc)
            want = ar.cov_ref(v, mask)
            got = _cov_window(dev, v, mask)
            assert ar.same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]), (T, B)
            assert np.array_equal(got[0], got[0].transpose(0, 2, 1)), (T, B)        # symmetric bit for bit
            assert (got[1].sum(axis=1) == T).all()
            if T >= 3:
                assert got[1][:, 1].sum() >= 3, (T, B)                               # the NaN, the Inf and the mask words were skipped
            if B == 5 and T == 65:
                nomask = _cov_window(dev, v, None)
                wn = ar.cov_ref(v, None)
                assert ar.same_bits(nomask[0], wn[0]) and np.array_equal(nomask[1], wn[1])
                assert nomask[1][:, 0].sum() > got[1][:, 0].sum()


def test_cov_misaligned_input_takes_the_dword_path(nsd, dev):
    from nsd_amd import ops
    v, mask = _scattered(2, 70, 8)
    flat = torch.zeros(v.size + 3, device=dev)
    for off in (1, 2, 3):
        x = flat[off:off + v.size].view(v.shape)
        x.copy_(to_dev(v, dev))
        sums, counts = ops.cov_step(x, mask=_mask_dev(mask, dev))
        want = ar.cov_ref(v, mask)
        assert ar.same_bits(sums.cpu().numpy(), want[0]) and np.array_equal(counts.cpu().numpy(), want[1]), off


def _new_cov_state(dev, Cc, S):
    from nsd_amd import ops
    state, check = guarded((S, Cc * Cc + 2), torch.float64, dev, "ones")
    ops.cov_reset(Cc, state)
    return state, check


def _state_parts(state, Cc):
    raw = state.cpu().numpy()
    return raw[:, :Cc * Cc].reshape(-1, Cc, Cc), raw[:, Cc * Cc:].view(np.int64)


CUTS = {"1+249": [1, 249], "sevens": [7] * 35 + [5], "64s": [64, 64, 64, 58], "whole": [250]}


def test_cov_stream_mode_does_not_depend_on_the_cut_or_the_slot(nsd, dev):
    from nsd_amd import ops
    B, T, Cc, S = 4, 250, 8, 6
    v, mask = _scattered(B, T, Cc, seed=3)
    want_s, want_c = _cov_window(dev, v, mask)
    assert ar.same_bits(want_s, ar.cov_ref(v, mask)[0])
    lay = ops.cov_layout(Cc)
    assert (lay.sum, lay.count, lay.skipped, lay.stride) == (0, Cc * Cc, Cc * Cc + 1, Cc * Cc + 2)
    slots_np = np.array([2, 7, 0, 4], np.int32)                                     # stream 1 names a slot outside [0, S)
    slots = to_dev(slots_np, dev)
    x, m = to_dev(v, dev), _mask_dev(mask, dev)
    for name, cut in CUTS.items():
        state, check = _new_cov_state(dev, Cc, S)
        t0 = 0
        for n in cut:
            assert ops.cov_step(x[:, t0:t0 + n].contiguous(), state, mask=m[:, t0:t0 + n].contiguous(), slots=slots) is state
            t0 += n
        check("state")
        sums, counts = _state_parts(state, Cc)
        for b, s in enumerate(slots_np):
            if s < S:
                assert ar.same_bits(sums[s], want_s[b]) and np.array_equal(counts[s], want_c[b]), (name, b)
        for s in (1, 3, 5):                                                         # the neighbours: still reset
            assert not sums[s].any() and not counts[s].any(), (name, s)
        assert np.array_equal(ops.cov_counts(Cc, state, [2, 0]), want_c[[0, 2]])
    # a reset of two slots leaves the others as they are
    before = state.clone()
    ops.cov_reset(Cc, state, to_dev(np.array([4, 9], np.int32), dev))
    check("state")
    assert not state[4].view(torch.int64).any() and torch.equal(state[:4].view(torch.int64), before[:4].view(torch.int64))


def test_cov_stream_mode_on_a_side_stream_and_from_a_replayed_graph(nsd, dev):
    from nsd_amd import ops
    B, T, Cc, n = 3, 250, 8, 50
    v, mask = _scattered(B, T, Cc, seed=5)
    want_s, want_c = ar.cov_ref(v, mask)
    x, m = to_dev(v, dev), _mask_dev(mask, dev)
    side = torch.cuda.Stream(device=dev)
    # eager, on a side stream
    st0, check0 = _new_cov_state(dev, Cc, B)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        for t0 in range(0, T, n):
            ops.cov_step(x[:, t0:t0 + n].contiguous(), st0, mask=m[:, t0:t0 + n].contiguous())
    side.synchronize()
    # captured once, replayed per chunk
    st1, check1 = _new_cov_state(dev, Cc, B)
    xin, min_ = torch.zeros((B, n, Cc), device=dev), torch.zeros((B, n), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ops.cov_step(xin, st1, mask=min_)
    ops.cov_reset(Cc, st1)                                                          # (whatever the capture ran)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        for t0 in range(0, T, n):
            xin.copy_(x[:, t0:t0 + n])
            min_.copy_(m[:, t0:t0 + n])
            graph.replay()
    side.synchronize()
    for state, check in ((st0, check0), (st1, check1)):
        check("state")
        sums, counts = _state_parts(state, Cc)
        assert ar.same_bits(sums, want_s) and np.array_equal(counts, want_c)


# ---- the fit -------------------------------------------------------------------------------------------------------------------------
def _fit(dev, nsd, Cc, cfg, sums, counts, groups=None, G=1):
    """ops.whiten_fit on window-mode style accumulators into guarded outputs -> (W numpy [G,C,C], records); inputs checked unchanged"""
    from nsd_amd import ops
    s, c = to_dev(np.ascontiguousarray(sums, np.float64), dev), to_dev(np.ascontiguousarray(counts, np.int64), dev)
    g = None if groups is None else to_dev(np.asarray(groups, np.int32), dev)
    W, check_w = guarded((G, Cc, Cc), torch.float32, dev, "nan32")
    rec, check_r = guarded((G * ar.RECORD_BYTES,), torch.uint8, dev, "ones")
    snap = snapshot(s, c, g)
    out = ops.whiten_fit(Cc, cfg, s, c, group=g, G=G, out=W, records=rec)
    assert out[0] is W and out[1] is rec and snap.unchanged()
    check_w("W")
    check_r("records")
    return W.cpu().numpy(), ops.whiten_records(rec, G)


def _records_match(got, want):
    for g, w in zip(got, want):
        for k in ("steps", "skipped", "status", "accumulators", "ignored"):
            assert g[k] == w[k], (k, g, w)
        for k in ("trace_mean", "eig_min", "eig_max"):
            assert abs(g[k] - w[k]) <= 1e-10 * max(abs(w["eig_max"]), 1e-300), (k, g, w)
        if not w["status"] & (ar.FEW | ar.NONFINITE):
            assert 1 <= g["sweeps"] <= 40, g


@pytest.mark.parametrize("Cc", [1, 2, 8, 17, 32])
def test_fit_equals_float64_eigh_within_twice_the_fp32_rounding(nsd, dev, Cc):
    cfg = nsd.SessionAlign(floor=1e-6, min_steps=1)                                 # (the floor below 1 / cond: nothing is clipped)
    for cond in (1.0, 1e2, 1e4):
        for G in (1, 3):
            accs = [ar.constructed(Cc, cond, seed=10 * g + k) for g in range(G) for k in range(2)]   # two accumulators per group
            sums, counts = np.stack([a[0] for a in accs]), np.stack([a[1] for a in accs])
            groups = None if G == 1 else np.repeat(np.arange(G), 2)
            W, recs = _fit(dev, nsd, Cc, cfg, sums, counts, groups, G)
            Wr, rr = ar.whiten_ref(sums, counts, cfg.shrinkage, cfg.floor, 1, groups, G)
            for g in range(G):
                err, bound = np.abs(W[g].astype(np.float64) - Wr[g]).max(), FIT_BOUND * np.abs(Wr[g]).max()
                assert err <= bound, (cond, G, g, err, bound)
                assert np.array_equal(W[g], W[g].T)                                 # symmetric bit for bit
                assert recs[g]["status"] == 0 and recs[g]["steps"] == 2 * 4096 and recs[g]["skipped"] == 6
            _records_match(recs, rr)
    # shrinkage: the same bound on R'
    accs = ar.constructed(Cc, 1e4, seed=77)
    cfg = nsd.SessionAlign(shrinkage=0.25, floor=1e-6, min_steps=1)
    W, recs = _fit(dev, nsd, Cc, cfg, accs[0][None], accs[1][None])
    Wr, rr = ar.whiten_ref(accs[0][None], accs[1][None], 0.25, 1e-6, 1)
    assert np.abs(W[0].astype(np.float64) - Wr[0]).max() <= FIT_BOUND * np.abs(Wr[0]).max()
    _records_match(recs, rr)


def test_fit_status_bits_each_on_its_own_and_a_bad_group_touches_no_neighbour(nsd, dev):
    Cc, G = 8, 5
    cfg = nsd.SessionAlign(floor=1e-4, min_steps=100)
    good = [ar.constructed(Cc, 1e2, seed=s) for s in (1, 2)]
    few = (good[0][0] * (50.0 / 4096.0), np.array([50, 0], np.int64))               # 50 < min_steps
    nonfinite = (good[0][0].copy(), good[0][1].copy())
    nonfinite[0][2, 3] = nonfinite[0][3, 2] = np.inf
    flat = ar.constructed(Cc, 1e2, seed=4)
    flat[0][5, :] = 0.0
    flat[0][:, 5] = 0.0                                                             # channel 5 is flat at zero: an eigenvalue 0
    accs = [good[0], few, nonfinite, flat, good[1]]
    sums, counts = np.stack([a[0] for a in accs]), np.stack([a[1] for a in accs])
    groups = np.array([0, 1, 2, 3, 4])
    W, recs = _fit(dev, nsd, Cc, cfg, sums, counts, groups, G)
    Wr, rr = ar.whiten_ref(sums, counts, 0.0, 1e-4, 100, groups, G)
    assert [r["status"] for r in recs] == [0, ar.FEW, ar.NONFINITE, ar.CLIPPED, 0] == [r["status"] for r in rr]
    eye = np.eye(Cc, dtype=np.float32)
    assert np.array_equal(W[1], eye) and np.array_equal(W[2], eye)
    assert recs[3]["clipped"] and recs[3]["eig_min"] < 1e-4 * recs[3]["eig_max"]
    for g in (0, 3, 4):
        assert np.abs(W[g].astype(np.float64) - Wr[g]).max() <= FIT_BOUND * np.abs(Wr[g]).max(), g
    _records_match(recs, rr)
    # trace <= 0 (all-zero sums with enough steps) is NONFINITE; a group without an accumulator is FEW; an index outside [0, G) is counted
    zero = (np.zeros((Cc, Cc)), np.array([500, 0], np.int64))
    accs2 = [good[0], zero, good[1], good[1]]
    sums2, counts2 = np.stack([a[0] for a in accs2]), np.stack([a[1] for a in accs2])
    groups2 = np.array([0, 1, 4, 9])                                                # groups 2 and 3 stay empty, 9 is outside
    W2, recs2 = _fit(dev, nsd, Cc, cfg, sums2, counts2, groups2, G)
    assert [r["status"] for r in recs2] == [0, ar.NONFINITE, ar.FEW, ar.FEW, 0]
    assert [r["accumulators"] for r in recs2] == [1, 1, 0, 0, 1] and all(r["ignored"] == 1 for r in recs2)
    assert all(np.array_equal(W2[g], eye) for g in (1, 2, 3))
    # the neighbours of the bad groups: bit-identical to a fit without them, W and records
    only = [0, 4]
    W3, recs3 = _fit(dev, nsd, Cc, cfg, sums[only], counts[only], np.array([0, 4]), G)
    for g in only:
        assert np.array_equal(W[g], W3[g]) and np.array_equal(W2[g], W3[g]), g
        assert {k: v for k, v in recs[g].items() if k != "ignored"} == {k: v for k, v in recs3[g].items() if k != "ignored"}, g


def test_fit_reads_a_stream_state_in_place_with_the_bits_of_window_mode(nsd, dev):
    from nsd_amd import ops
    B, T, Cc = 3, 250, 8
    v, mask = _scattered(B, T, Cc, seed=9)
    x, m = to_dev(v, dev), _mask_dev(mask, dev)
    cfg = nsd.SessionAlign(min_steps=10)
    sums, counts = ops.cov_step(x, mask=m)
    state, check = _new_cov_state(dev, Cc, B)
    ops.cov_step(x, state, mask=m)
    snap = snapshot(state)
    groups = to_dev(np.array([1, 0, 1], np.int32), dev)
    Ww, rw = ops.whiten_fit(Cc, cfg, sums, counts, group=groups, G=2)
    Ws, rs = ops.whiten_fit(Cc, cfg, state=state, group=groups, G=2)
    check("state")
    assert snap.unchanged() and torch.equal(Ww.view(torch.int32), Ws.view(torch.int32))
    assert ops.whiten_records(rw, 2) == ops.whiten_records(rs, 2)
    # and what the whitening is for: W R' W = I on the data's own moment
    Wr, _ = ar.whiten_ref(sums.cpu().numpy(), counts.cpu().numpy(), 0.0, cfg.floor, 10, [1, 0, 1], 2)
    assert np.abs(Ww.cpu().numpy().astype(np.float64) - Wr).max() <= FIT_BOUND * np.abs(Wr).max()
    # captured and replayed: the same bits
    side = torch.cuda.Stream(device=dev)
    Wg, rg = torch.zeros_like(Ws), torch.zeros_like(rs)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ops.whiten_fit(Cc, cfg, state=state, group=groups, G=2, out=Wg, records=rg)
    Wg.zero_()
    with torch.cuda.stream(side):
        graph.replay()
    side.synchronize()
    assert torch.equal(Wg.view(torch.int32), Ws.view(torch.int32)) and torch.equal(rg, rs)


# ---- the apply stage -----------------------------------------------------------------------------------------------------------------
def _matrices(n_mat, Cc, seed=0):
    rs = np.random.RandomState(seed + Cc)
    return (rs.standard_normal((n_mat, Cc, Cc)) / np.sqrt(Cc)).astype(np.float32)


def _apply(dev, v, W, sel=None, *, in_place=False, offset=0):
    """ops.spatial_apply into a NaN-filled, guarded output (offset: v and out start that many floats into their buffers) -> numpy"""
    from nsd_amd import ops
    Wd, s = to_dev(W, dev), None if sel is None else to_dev(np.asarray(sel, np.int32), dev)
    src = torch.zeros(v.size + offset, device=dev)
    x = src[offset:].view(v.shape)
    x.copy_(to_dev(v, dev))
    snap = snapshot(Wd, s) if in_place else snapshot(x, Wd, s)
    if in_place:
        buf, check = guarded(v.shape, torch.float32, dev)
        buf.copy_(x)
        out = ops.spatial_apply(buf, Wd, sel=s, out=buf)
        assert out is buf
    else:
        flat, check = guarded((v.size + offset,), torch.float32, dev, "nan32")
        out = ops.spatial_apply(x, Wd, sel=s, out=flat[offset:].view(v.shape))
        assert offset == 0 or np.isnan(flat[:offset].cpu().numpy()).all()
    check("out")
    assert snap.unchanged()
    return out.cpu().numpy()


@pytest.mark.parametrize("B,T,Cc", [(1, 1, 1), (5, 33, 3), (3, 70, 8), (2, 65, 32), (4, 250, 8)])
def test_apply_equals_the_reference_bitwise(nsd, dev, B, T, Cc):
    v = _scattered(B, T, Cc)[0]
    v[~np.isfinite(v)] = 1.0
    W = _matrices(4, Cc)
    assert ar.same_bits(_apply(dev, v, W[0]), ar.apply_ref(v, W[0]))                # sel = NULL: matrix 0
    assert ar.same_bits(_apply(dev, v, W), ar.apply_ref(v, W))
    perm = [(3 * b + 1) % 4 for b in range(B)]
    want = ar.apply_ref(v, W, perm)
    assert ar.same_bits(_apply(dev, v, W, perm), want)
    assert ar.same_bits(_apply(dev, v, W, perm, in_place=True), want)
    for off in (1, 3):                                                              # a base pointer that is not 16-byte aligned
        assert ar.same_bits(_apply(dev, v, W, perm, offset=off), want), off
    assert np.array_equal(_apply(dev, v, np.eye(Cc, dtype=np.float32)), v)          # the identity is a copy (0 * x adds a zero)


def test_apply_selection_outside_the_table_gives_nan_rows_and_a_nan_step_stays_a_step(nsd, dev):
    B, T, Cc = 4, 70, 8
    v = _scattered(B, T, Cc)[0]
    v[~np.isfinite(v)] = 1.0
    W = _matrices(2, Cc)
    sel = [1, 2, 0, -1]                                                             # rows 1 and 3 select outside [0, 2)
    got = _apply(dev, v, W, sel)
    assert np.isnan(got[[1, 3]]).all() and ar.same_bits(got, ar.apply_ref(v, W, sel)) and np.isfinite(got[[0, 2]]).all()
    assert ar.same_bits(_apply(dev, v, W, sel, in_place=True), got)
    v[0, 5, 3], v[2, 64, 0] = np.nan, np.nan
    got = _apply(dev, v, W, [0, 1, 1, 0])
    bad = np.zeros((B, T), bool)
    bad[0, 5] = bad[2, 64] = True
    assert np.isnan(got[bad]).all() and np.isfinite(got[~bad]).all()                # the whole step, and nothing else
    assert ar.same_bits(got, ar.apply_ref(v, W, [0, 1, 1, 0]))


def test_refusals_and_empty_calls(nsd, dev):
    from nsd_amd import ops
    Cc = 8
    x = torch.zeros((2, 10, Cc), device=dev)
    state = ops.cov_state(Cc, 2, dev)
    with pytest.raises(nsd.NsdError, match="slots without a state"):
        ops.cov_step(x, slots=torch.zeros(2, dtype=torch.int32, device=dev))
    with pytest.raises(nsd.NsdError, match="smaller than nsd_cov_state_bytes"):
        ops.cov_step(x[:1], state[0, :-1].view(1, -1))
    with pytest.raises(nsd.NsdError, match="B = 2 streams, S = 1"):
        ops.cov_step(x, state[:1])
    with pytest.raises(nsd.NsdError, match="outside \\[1, 32\\]"):
        ops.cov_step(torch.zeros((1, 4, 33), device=dev))
    with pytest.raises(nsd.NsdError, match="overlaps v partially"):
        flat = torch.zeros(2 * 10 * Cc + 8, device=dev)
        ops.spatial_apply(flat[:160].view(2, 10, Cc), torch.eye(Cc, device=dev), out=flat[8:168].view(2, 10, Cc))
    # B = 0 launches nothing; N = 0 still writes the identities
    sums, counts = ops.cov_step(torch.zeros((0, 10, Cc), device=dev))
    assert tuple(sums.shape) == (0, Cc, Cc)
    W, rec = ops.whiten_fit(Cc, nsd.SessionAlign(), sums, counts, G=2)
    assert torch.equal(W, torch.eye(Cc, device=dev).expand(2, Cc, Cc)) and all(r["few"] for r in ops.whiten_records(rec, 2))
    assert ops.spatial_apply(torch.zeros((0, 10, Cc), device=dev), W).numel() == 0


# ---- through the Python layers: with the stage on, every path equals the align-free path on hand-aligned input, bit for bit ------------
def _np_eq(a, b):
    return ar.same_bits(a.detach().cpu().numpy(), b.detach().cpu().numpy())


def _eval_model(nsd, dev, ref_state, scale=1.0, **kw):
    m = nsd.EEG_LSTM(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v) * np.float32(scale)) for k, v in ref_state.items()}, strict=True)
    return m.to(dev).eval()


def _train_model(nsd, dev, seed, **kw):
    torch.manual_seed(seed)
    return nsd.EEG_LSTM(**kw).to(dev).train()


def _mix(dev, seed=0, n=None):
    """alignment-like matrices: symmetric, near the identity -> [8,8] or [n,8,8] on the device"""
    rs = np.random.RandomState(100 + seed)
    a = 0.15 * rs.standard_normal((n or 1, 8, 8))
    W = (np.eye(8) + 0.5 * (a + a.transpose(0, 2, 1))).astype(np.float32)
    return to_dev(W if n else W[0], dev)


def _gate_prep(nsd):
    return (nsd.SignalGate(rail=100.0, hold_samples=2, max_bad=2),
            nsd.CausalPrep.design(highpass=1.0, lowpass=40.0, zscore_seconds=0.4, var0=250.0, car=True))


def _signal8(B, T, seed=3):
    """clean noise of 10 units on 8 channels; stream 0 railed on channel 2 from sample 30 on, stream 1 a pop on three channels at
    sample 37 (with the gate of _gate_prep: a zeroed channel, and three rejected steps)"""
    x = np.clip(10.0 * np.random.RandomState(seed).standard_normal((B, T, 8)), -40, 40).astype(np.float32)
    if T > 37:
        x[0, 30:, 2] = 3000.0
        if B > 1:
            x[1, 37, 1:4] = 500.0
    return x


def _hand(x, W, G=None, P=None, max_bad=None, sel=None):
    """align(apply(prep(gate(x)))) over whole windows, made with the ops calls"""
    from nsd_amd import ops
    v, mask = (ops.gate_step(x, G) if G is not None else (x, None))
    v = ops.prep_step(v, P) if P is not None else v
    v = ops.gate_apply(v, G, mask, max_bad=max_bad) if mask is not None else v
    return ops.spatial_apply(v, W, sel=sel)


@pytest.mark.parametrize("front", [False, True])
def test_the_model_runs_the_align_stage_wherever_its_front_end_runs(nsd, dev, ref_state, front):
    A, W = nsd.SessionAlign(), _mix(dev)
    G, P = _gate_prep(nsd) if front else (None, None)
    x = to_dev(_signal8(6, 64), dev)
    snap = snapshot(x)
    hand = _hand(x, W, G, P)
    m = _eval_model(nsd, dev, ref_state, align=A, align_matrix=W, gate=G, prep=P)
    plain = _eval_model(nsd, dev, ref_state)
    assert "align_matrix" not in m.state_dict() and torch.equal(m.align_matrix, W)
    with torch.no_grad():
        assert _np_eq(m(x), plain(hand))
    pa = m.predict_proba(x)
    assert _np_eq(pa, plain.predict_proba(hand)) and np.isnan(pa[1].cpu().numpy()).all() == front   # a rejected step stays "no decision"
    ta, wa = m.predict_trials(x, window=20, hop=10)
    tb, wb = plain.predict_trials(hand, window=20, hop=10)
    assert _np_eq(ta, tb) and _np_eq(wa, wb) and snap.unchanged()
    # the identity until set; a twin on an averaged row carries the stage
    fresh = _eval_model(nsd, dev, ref_state, align=A, gate=G, prep=P)
    assert _np_eq(fresh.predict_proba(x), _eval_model(nsd, dev, ref_state, gate=G, prep=P).predict_proba(x))
    twin = m.view_of(m.flat_parameters().clone())
    assert twin.align == A and _np_eq(twin.predict_proba(x), pa)
    # train mode: the training node sees the aligned windows
    m.train(); plain.train()
    m._mask_override = plain._mask_override = (None, None, None)
    la, lb = m(x).square().sum(), plain(_hand(x, W, G, P, max_bad=8)).square().sum()
    la.backward(); lb.backward()
    assert torch.equal(la, lb) and bool(torch.isfinite(la))
    for (n, a), (_, b) in zip(m.named_parameters(), plain.named_parameters()):
        assert torch.equal(a.grad, b.grad), n
    with pytest.raises(nsd.NsdError, match="dx through the signal-quality gate" if front else "dx through the session alignment"):
        m(x.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="normalize"):
        nsd.EEG_LSTM(align=A, normalize=True)


def _batch8(dev, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    x = (10.0 * torch.randn((B, T, 8), generator=g)).clamp_(-40, 40)
    return x.to(dev), torch.randint(0, 3, (B,), generator=g, dtype=torch.int32).to(dev)


def test_trainer_steps_with_alignment_equal_plain_steps_on_hand_aligned_windows(nsd, dev):
    from nsd_amd.trainer import Trainer
    A, (B, T) = nsd.SessionAlign(), (4, 32)
    G, P = _gate_prep(nsd)
    # Trainer.step, the stage behind gate and prep
    W = _mix(dev, 1)
    ma, mb = _train_model(nsd, dev, 11, align=A, align_matrix=W, gate=G, prep=P), _train_model(nsd, dev, 11)
    ta, tb = Trainer(ma, lr=1e-3, seed=9), Trainer(mb, lr=1e-3, seed=9)
    for step in range(1, 3):
        x, y = _batch8(dev, B, T, seed=step)
        snap = snapshot(x)
        ta.step(x, y)
        tb.step(_hand(x, W, G, P, max_bad=8), y)
        assert torch.equal(ta.flat, tb.flat) and torch.equal(ta.m, tb.m) and torch.equal(ta.v, tb.v), step
        assert ta.last_loss() == tb.last_loss() and np.isfinite(ta.last_loss()) and snap.unchanged(), step
    # the replayed step, the stage alone: out of the static input into xn
    x, y = _batch8(dev, B, T, seed=8)
    W = _mix(dev, 2)
    ma, mb = _train_model(nsd, dev, 21, align=A, align_matrix=W), _train_model(nsd, dev, 21)
    ta, tb = Trainer(ma, lr=1e-3, seed=5), Trainer(mb, lr=1e-3, seed=5)
    (xa, ya), (xb, yb) = ta.static_inputs(B, T), tb.static_inputs(B, T)
    xa.copy_(x); ya.copy_(y); xb.copy_(_hand(x, W)); yb.copy_(y)
    for step in range(1, 3):
        ta.step_static(B, T)
        tb.step_static(B, T)
        assert torch.equal(ta._buffers(B, T)["xn"], xb), step
        assert torch.equal(ta.flat, tb.flat) and torch.equal(ta.grads, tb.grads), step
    assert torch.equal(xa, x)                                                       # the static input is not written
    # a new matrix reaches the captured step at its next replay
    W2 = _mix(dev, 3)
    ma.set_alignment(W2)
    xb.copy_(_hand(x, W2))
    ta.step_static(B, T)
    tb.step_static(B, T)
    assert torch.equal(ta.flat, tb.flat)
    # ModelBatchTrainer, M = 2, one matrix per model
    M = 2
    Ws = _mix(dev, 4, n=M)
    aligned = [_train_model(nsd, dev, 30 + m, align=A, prep=P) for m in range(M)]
    plain = [_train_model(nsd, dev, 30 + m) for m in range(M)]
    ta = nsd.ModelBatchTrainer(aligned, lr=1e-3, seeds=[1, 2])
    tb = nsd.ModelBatchTrainer(plain, lr=1e-3, seeds=[1, 2])
    ta.set_alignment(Ws)
    assert all(torch.equal(aligned[m].align_matrix, Ws[m]) for m in range(M))
    sel = to_dev(np.repeat(np.arange(M), B).astype(np.int32), dev)
    for step in range(1, 3):
        xs, ys = zip(*[_batch8(dev, B, T, seed=10 * step + m) for m in range(M)])
        x, y = torch.stack(xs), torch.stack(ys)
        ta.step(x, y)
        tb.step(_hand(x, Ws, None, P, sel=sel), y)
        for m in range(M):
            for (n, a), (_, b) in zip(aligned[m].state_dict().items(), plain[m].state_dict().items()):
                assert torch.equal(a, b), (step, m, n)
    ea = ta.evaluate(x, y)
    eb = tb.evaluate(_hand(x, Ws, None, P, sel=sel), y)
    assert [r["loss_sum"] for r in ea] == [r["loss_sum"] for r in eb]
    with pytest.raises(nsd.NsdError):
        nsd.ModelBatchTrainer([_train_model(nsd, dev, 1, align=A), _train_model(nsd, dev, 2)], lr=1e-3, seeds=[1, 2])


def test_stream_decoders_with_alignment_equal_plain_ones_on_hand_aligned_chunks(nsd, dev, ref_state):
    from nsd_amd import ops
    A, W = nsd.SessionAlign(min_steps=20), _mix(dev, 5)
    G, P = _gate_prep(nsd)
    B, T, S = 3, 70, 4
    x = to_dev(_signal8(B, T), dev)
    hand = _hand(x, W, G, P)
    m, plain = _eval_model(nsd, dev, ref_state, align=A, align_matrix=W, gate=G, prep=P), _eval_model(nsd, dev, ref_state)
    a, b = nsd.StreamDecoder(m, streams=S), nsd.StreamDecoder(plain, streams=S)
    a.align_accumulate(True)
    t = 0
    for n in (7, 1, 32, 30):
        assert _np_eq(a.push(x[:, t:t + n]), b.push(hand[:, t:t + n])), t
        t += n
    assert _np_eq(a.state, b.state)
    # the accumulators saw what stands behind the gate's apply: the sums of the hand-made windows under the gate's mask
    v, mask = ops.gate_step(x, G)
    v = ops.gate_apply(ops.prep_step(v, P), G, mask)
    want_s, want_c = ar.cov_ref(v.cpu().numpy(), mask.cpu().numpy().view(np.uint32))
    got = a.cov_state.cpu().numpy()
    assert ar.same_bits(got[:B, :64].reshape(B, 8, 8), want_s) and np.array_equal(got[:B, 64:].view(np.int64), want_c)
    assert not a.cov_state[3].view(torch.int64).any() and want_c[1, 1] == 3 and want_c[0, 1] == 40
    # refit_alignment(slots=[1]) changes slot 1's matrix and decisions only
    W0, r0 = a.alignment()
    assert all(np.array_equal(W0[s], W.cpu().numpy()) for s in range(S)) and all(r["steps"] == 0 for r in r0)
    a.refit_alignment(slots=[1])
    W1, r1 = a.alignment()
    Wr, rr = ar.whiten_ref(want_s[1:2], want_c[1:2], 0.0, A.floor, 20)
    assert np.abs(W1[1].astype(np.float64) - Wr[0]).max() <= FIT_BOUND * np.abs(Wr[0]).max() and r1[1]["steps"] == 67 and r1[1]["status"] == 0
    assert all(np.array_equal(W1[s], W0[s]) and r1[s] == r0[s] for s in (0, 2, 3))
    more = to_dev(_signal8(B, 12, seed=8), dev)
    a.reset(); b.reset()
    pa, pb = a.push(more), b.push(_hand(more, W, G, P))
    assert _np_eq(pa[[0, 2]], pb[[0, 2]]) and not _np_eq(pa[1:2], pb[1:2])
    one, _ = a.alignment(slots=[1])
    assert np.array_equal(one[0], W1[1])
    # state dicts carry the table and the accumulators, and refuse a decoder without them
    sd = a.state_dict()
    assert {"align_table", "cov_state"} <= set(sd)
    c = nsd.StreamDecoder(m, streams=S)
    c.load_state_dict(sd)
    c.align_accumulate(True)
    assert _np_eq(a.push(more), c.push(more)) and torch.equal(a.cov_state.view(torch.int64), c.cov_state.view(torch.int64))
    assert torch.equal(a.align_table, c.align_table)
    with pytest.raises(nsd.NsdError, match="session alignment"):
        nsd.StreamDecoder(_eval_model(nsd, dev, ref_state, gate=G, prep=P), streams=S).load_state_dict(sd)
    with pytest.raises(nsd.NsdError, match="no session alignment"):
        b.refit_alignment()
    # refit of all slots (slot 3 never saw a sample: the identity, few), set and reset
    a.refit_alignment()
    W2, r2 = a.alignment()
    assert r2[3]["few"] and np.array_equal(W2[3], np.eye(8, dtype=np.float32)) and r2[0]["status"] == 0
    a.set_alignment([0, 3], W)
    a.reset_alignment([2])
    W3, _ = a.alignment()
    assert all(np.array_equal(W3[s], W.cpu().numpy()) for s in (0, 2, 3)) and np.array_equal(W3[1], W2[1])
    assert not a.cov_state[2].view(torch.int64).any() and a.cov_state[1].view(torch.int64).any()


def test_the_other_three_decoders_with_alignment_equal_plain_ones_on_hand_aligned_chunks(nsd, dev, ref_state):
    A, W = nsd.SessionAlign(), _mix(dev, 6)
    B, T, WIN, HOP = 2, 70, 20, 10
    x = to_dev(_signal8(B, T, seed=11)[:, :, :], dev).clamp_(-40, 40)
    hand = _hand(x, W)
    m2 = [_eval_model(nsd, dev, ref_state, align=A, align_matrix=W), _eval_model(nsd, dev, ref_state, scale=0.9, align=A, align_matrix=W)]
    p2 = [_eval_model(nsd, dev, ref_state), _eval_model(nsd, dev, ref_state, scale=0.9)]
    pairs = [(nsd.EnsembleStreamDecoder(m2, streams=B), nsd.EnsembleStreamDecoder(p2, streams=B)),
             (nsd.SlidingStreamDecoder(m2[0], streams=B, window=WIN, hop=HOP), nsd.SlidingStreamDecoder(p2[0], streams=B, window=WIN, hop=HOP)),
             (nsd.EnsembleSlidingStreamDecoder(m2, streams=B, window=WIN, hop=HOP),
              nsd.EnsembleSlidingStreamDecoder(p2, streams=B, window=WIN, hop=HOP))]
    for a, b in pairs:
        assert tuple(a.align_table.shape) == (B, 8, 8)                              # one table, shared by the members
        t = 0
        for n in (7, 33, 30):
            ra, rb = a.push(x[:, t:t + n]), b.push(hand[:, t:t + n])
            t += n
            ra, rb = (ra, rb) if isinstance(ra, (tuple, list)) else ((ra,), (rb,))
            for u, v in zip(ra, rb):
                assert u is None or (_np_eq(u, v) if u.is_floating_point() else torch.equal(u, v)), (type(a).__name__, t)
        assert _np_eq(a.state, b.state), type(a).__name__
        sd = a.state_dict()
        assert {"align_table", "cov_state"} <= set(sd)
        a.load_state_dict(sd)


def test_a_checkpoint_carries_the_alignment_and_calibration_refits_it(nsd, dev, ref_state, tmp_path):
    from nsd_amd.trainer import save_reference_checkpoint
    A = nsd.SessionAlign(shrinkage=0.1, min_steps=50)
    model = _eval_model(nsd, dev, ref_state, align=A)
    rs = np.random.RandomState(4)
    mixing = (np.eye(8) + 0.3 * rs.standard_normal((8, 8))).astype(np.float32)
    trials = (np.clip(10.0 * rs.standard_normal((6, 125, 8)), -40, 40) @ mixing.T).astype(np.float32)
    # SessionAlign.fit: the device route against the restatements
    Wd, recs = A.fit(model, trials)
    sums, counts = A.cov_reference(trials)
    Wr, rr = A.fit_reference(sums, counts)
    assert np.abs(Wd.cpu().numpy().astype(np.float64) - Wr).max() <= FIT_BOUND * np.abs(Wr).max()
    assert recs[0]["steps"] == 6 * 125 == rr[0]["steps"] and recs[0]["status"] == 0
    Wg, rg = A.fit(model, trials, groups=[0, 1, 0, 1, 2, 2])
    assert tuple(Wg.shape) == (3, 8, 8) and [r["steps"] for r in rg] == [250] * 3
    model.set_alignment(Wd[0], record=recs[0])
    path = str(tmp_path / "align.pth")
    save_reference_checkpoint(model, path)
    state = torch.load(path, map_location="cpu", weights_only=True)
    assert set(state) == {"state_dict", "nsd_align"} and set(state["nsd_align"]) == {"config", "matrix", "record"}
    pred = nsd.SimplePredictor(path, sr=125, device="cpu", preprocess="identity")
    assert pred.model.align == A and torch.equal(pred.model.align_matrix.cpu(), Wd[0].cpu()) and pred.model.align_record == recs[0]
    assert pred.predict(trials[0])[0].tobytes() == model.predict_proba(to_dev(trials[:1], dev))[0].cpu().numpy().tobytes()
    st = pred.open_stream(streams=2)                                                # decoders start from the checkpoint's matrix
    assert torch.equal(st.decoder.align_table[1].cpu(), Wd[0].cpu())
    # a new session: the same trials through another mixing; calibrate(align=True) refits the matrix first, label-free
    shifted = (trials @ (np.eye(8) + 0.3 * rs.standard_normal((8, 8))).astype(np.float32).T).astype(np.float32)
    labels = np.array([0, 1, 2, 0, 1, 2])
    rep = pred.calibrate(shifted, labels, epochs=3)
    s2, c2 = A.cov_reference(shifted)
    W2, _ = A.fit_reference(s2, c2)                                                 # (all six accumulators in one group)
    got = pred.model.align_matrix.cpu().numpy()
    assert rep["align"]["steps"] == 750 and np.abs(got.astype(np.float64) - W2[0]).max() <= FIT_BOUND * np.abs(W2[0]).max()
    assert not np.array_equal(got, Wd[0].cpu().numpy()) and pred.model.align_record == rep["align"]
    keep = got.copy()
    pred.calibrate(shifted[:, :5], labels, epochs=1)                                # 30 steps < min_steps: the matrix stays
    assert np.array_equal(pred.model.align_matrix.cpu().numpy(), keep)
    pred.calibrate(trials, labels, epochs=1, align=False)
    assert np.array_equal(pred.model.align_matrix.cpu().numpy(), keep)
    plain_path = str(tmp_path / "plain.pth")
    save_reference_checkpoint(_eval_model(nsd, dev, ref_state), plain_path)
    assert nsd.SimplePredictor(plain_path, sr=125, device="cpu", preprocess="identity").model.align is None


def test_an_ensemble_predictor_shares_one_matrix_and_calibration_refits_it_for_all_members(nsd, dev, ref_state, tmp_path):
    from nsd_amd.trainer import save_reference_checkpoint
    A = nsd.SessionAlign(min_steps=50)
    W = _mix(dev, 7)
    paths = []
    for i, scale in enumerate((1.0, 0.9)):
        paths.append(str(tmp_path / f"m{i}.pth"))
        save_reference_checkpoint(_eval_model(nsd, dev, ref_state, scale=scale, align=A, align_matrix=W), paths[-1])
    pred = nsd.EnsemblePredictor(paths, sr=125, device="cpu", preprocess="identity")
    assert all(torch.equal(m.align_matrix, W) for m in pred.members) and pred.model.align == A
    rs = np.random.RandomState(6)
    trials = np.clip(10.0 * rs.standard_normal((6, 125, 8)), -40, 40).astype(np.float32)
    plain = [_eval_model(nsd, dev, ref_state, scale=s) for s in (1.0, 0.9)]
    hand = _hand(to_dev(trials, dev), W)
    want = torch.stack([m.predict_proba(hand) for m in plain]).mean(0)
    got = np.stack([pred.predict(t)[0] for t in trials])
    assert np.abs(got - want.cpu().numpy()).max() < 1e-6                             # (the members share member 0's front end)
    rep = pred.calibrate(trials, np.array([0, 1, 2, 0, 1, 2]), epochs=2)
    Wr, _ = A.fit_reference(*A.cov_reference(trials))
    for m in pred.members:
        got_w = m.align_matrix.cpu().numpy()
        assert np.abs(got_w.astype(np.float64) - Wr[0]).max() <= FIT_BOUND * np.abs(Wr[0]).max() and m.align_record == rep["align"]
    assert rep["align"]["steps"] == 750 and rep["align"]["accumulators"] == 6
