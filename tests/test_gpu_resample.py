"""The rate conversion on the MI355X (nsd_resample_* of include/nsd.h, csrc/nsd_resample.hip) against its numpy restatement
(tests/resample_ref.py): every finite value BIT FOR BIT, NaNs by position.  Window mode over the ratios, tap counts and shapes at which
the kernel takes another path (the input tile, the LDS tap table's edge, 16-byte and dword staging and stores, the grid cap), stream
mode over cuts, slots, HIP streams, a graph replay and resets, the buffer contract, the poison window, and the path through the Python
layers: the model, the four stream decoders, a decoder checkpoint and train's checkpoint."""
import ctypes as C
import itertools
import json

import numpy as np
import pytest
import torch

from tests import resample_ref as rr
from tests.buffer_contract import Guarded, guarded, snapshot
from tests.gpu_harness import NAN, dev, nsd, sync_at_the_end, to_dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

TILE = 256                       # RS_TI of csrc/nsd_args.h: input samples staged through LDS at once
GRID_CAP = 1024                  # RS_GRID_CAP: workgroups of a launch
TAPS_LDS = 768                   # RS_TAPS_LDS: the tap table lives in LDS up to this many floats
EDGE_P = TAPS_LDS // 3           # (3, 2, P): L * P exactly at the table's edge
# the configurations of the window-mode table, and (5, 8, 154): 770 taps, the first table past the edge at a ratio that is not 125-phase
CONFIGS = [(1, 2, 3), (1, 2, 47), (5, 8, 36), (2, 1, 24), (125, 128, 23), (1, 1, 1), (1, 8, 256), (3, 2, EDGE_P), (5, 8, 154)]
CS, BS = (1, 3, 8, 64), (1, 5, 70)
CUTS = ([41], [1] * 41, [7, 1, 33], [16, 16, 9])


def _rs(nsd, L, M, P, seed=0):
    """a converter with random taps of both signs: a bitwise comparison is no easier on a designed filter"""
    rs = np.random.RandomState(1000 * L + 10 * M + P + seed)
    return nsd.Resample(L=L, M=M, P=P, taps=(rs.standard_normal((L, P)) / np.sqrt(P)).astype(np.float32))


def _raw(B, T, Cc, seed=0):
    rs = np.random.RandomState(seed + 1000 * B + 10 * T + Cc)
    return (20.0 * rs.standard_normal((B, T, Cc)) + 500.0 * rs.uniform(-1, 1, (B, 1, Cc))).astype(np.float32)


def _ref_trials(x, r):
    """window mode: channels and trials are independent, so all of them run as the channels of ONE reference stream"""
    B, T, Cc = x.shape
    y = rr.step(np.ascontiguousarray(x.transpose(1, 0, 2)).reshape(T, B * Cc), r.taps, r.L, r.M)[0]
    return np.ascontiguousarray(y.reshape(-1, B, Cc).transpose(1, 0, 2))


def _window(dev, x_np, r, *, offset=0, fill="nan32"):
    """ops.resample_step in window mode into a guarded y (offset: y starts that many floats into its buffer: not 16-byte aligned)
    -> numpy y; x and the taps are checked to be unchanged"""
    from nsd_amd import ops
    x = to_dev(x_np, dev)
    To = rr.ceil_div(x_np.shape[1] * r.L, r.M)
    shape = (x_np.shape[0], To, x_np.shape[2])
    flat, check = guarded((int(np.prod(shape)) + offset,), torch.float32, dev, fill)
    y = flat[offset:].view(shape)
    cnt, check_cnt = guarded((shape[0],), torch.int32, dev, "ones")
    snap = snapshot(x, r.device_taps(dev))
    assert ops.resample_step(x, r, out=y, cnt=cnt) is y and snap.unchanged()
    check("y"); check_cnt("cnt")
    assert cnt.cpu().tolist() == [To] * shape[0]
    return y.cpu().numpy()


def _t_values(P):
    return sorted({t for t in (1, 2, P - 2, P - 1, P, TILE - 1, TILE, TILE + 1) if t >= 1})


def _shapes(P):
    """every T against two (B, C) pairs, the largest batches at the shortest T; every C and every B occurs"""
    pairs = sorted(itertools.product(BS, CS), key=lambda bc: -bc[0] * bc[1])
    ts = _t_values(P)
    out = []
    for i, T in enumerate(ts):
        k = 2 * i if 2 * i + 1 < len(pairs) else len(pairs) - 1 - (2 * i) % len(pairs)      # (past the list: again from its small end)
        out += [(pairs[k][0], T, pairs[k][1]), (pairs[k ^ 1][0], T, pairs[k ^ 1][1])]
    seen = {(b, c) for b, _, c in out}
    out += [(b, ts[-1] if b * c <= 64 else 2, c) for b, c in pairs if (b, c) not in seen]
    return out


@pytest.mark.parametrize("L,M,P", CONFIGS)
def test_window_mode_equals_the_reference_bitwise(nsd, dev, L, M, P):
    r = _rs(nsd, L, M, P)
    assert (L * P <= TAPS_LDS) == ((L, M, P) not in [(125, 128, 23), (5, 8, 154)])
    shapes = _shapes(P)
    assert {c for _, _, c in shapes} == set(CS) and {b for b, _, _ in shapes} == set(BS)
    for B, T, Cc in shapes:
        x = _raw(B, T, Cc)
        want = _ref_trials(x, r)
        assert want.shape[1] == rr.ceil_div(T * L, M) and np.isfinite(want).all()
        assert rr.same_bits(_window(dev, x, r), want), (B, T, Cc)


def test_the_table_edge_and_one_tap_past_it(nsd, dev):
    for L, M, P in ((3, 2, EDGE_P), (3, 2, EDGE_P - 1), (7, 2, TAPS_LDS // 7 + 1)):
        r = _rs(nsd, L, M, P)
        x = _raw(5, 300, 8)
        assert rr.same_bits(_window(dev, x, r), _ref_trials(x, r)), (L, M, P)


def test_dword_staging_and_stores(nsd, dev):
    """T * C % 4 != 0 (dword loads), C % 4 != 0 (an element per thread) and a y that is 1 .. 3 floats off 16 bytes (dword stores)"""
    for L, M, P in ((1, 2, 47), (5, 8, 36), (2, 1, 24)):
        r = _rs(nsd, L, M, P)
        for B, T, Cc in ((5, 131, 5), (3, 263, 3), (5, 33, 1), (2, 259, 2), (3, 517, 6)):
            x = _raw(B, T, Cc)
            assert rr.same_bits(_window(dev, x, r), _ref_trials(x, r)), (L, M, P, B, T, Cc)
        x = _raw(5, 300, 8)
        want = _ref_trials(x, r)
        for off in (1, 2, 3):
            assert rr.same_bits(_window(dev, x, r, offset=off), want), (L, M, P, off)


@pytest.mark.parametrize("B,T,Cc", [(GRID_CAP + 6, 3, 8), (300, 4 * TILE + 5, 8), (GRID_CAP + 1, 2, 3)])
def test_more_work_units_than_the_grid_cap(nsd, dev, B, T, Cc):
    r = _rs(nsd, 1, 2, 3)
    x = _raw(B, T, Cc)
    assert B * rr.ceil_div(T, TILE) > GRID_CAP
    assert rr.same_bits(_window(dev, x, r), _ref_trials(x, r))


def test_a_designed_decimator_passes_dc_and_delays_by_its_group_delay(nsd, dev):
    r = nsd.Resample.design(250, 125)
    t = np.arange(1250, dtype=np.float64) / 250.0
    x = (30.0 * np.sin(2 * np.pi * 10.0 * t) + 100.0)[None, :, None].repeat(8, 2).astype(np.float32)
    y = _window(dev, x, r)
    assert rr.same_bits(y, _ref_trials(x, r))
    j = np.arange(100, 600)
    want = 30.0 * np.sin(2 * np.pi * 10.0 * (j - r.delay) / 125.0) + 100.0
    assert np.abs(y[0, j, 0] - want).max() < 1e-2 * 30.0 + 1e-4 * 100.0        # design()'s passband bound on the sine, its DC bound on the offset


# ---- stream mode -----------------------------------------------------------------------------------------------------------------------
def _new_state(dev, Cc, r, S, fill="nan32"):
    """S slots of exactly nsd_resample_state_bytes between guards, filled, then reset through the library -> (state, check, layout)"""
    from nsd_amd import _lib, ops
    lay = ops.resample_layout(Cc, r)
    nbytes = int(_lib.lib().nsd_resample_state_bytes(Cc, C.cast(C.pointer(r.struct()), C.c_void_p), S))
    assert nbytes == S * int(lay.stride) * 4 and int(lay.n_in) % 2 == 0 and int(lay.hist) == 0
    state, check = guarded((S, int(lay.stride)), torch.float32, dev, fill)
    ops.resample_reset(Cc, r, state)
    return state, check, lay


def _state_bits(state):
    return state.cpu().numpy().view(np.uint32)


def _run_cut(dev, x_np, r, cut, state, lay, slots=None, ref=None, spare_rows=0):
    """the chunks of `cut` through ops.resample_step in stream mode, each into a guarded y; after EVERY chunk the outputs, cnt and
    the state are the reference's (ref = (n_in [B], hist [B,P-1,C]) of the pushed streams, in stream order; None: reset slots)
    -> (numpy outputs [B, total, C], ref)"""
    from nsd_amd import ops
    B, _, Cc = x_np.shape
    n_in, hist = (np.zeros(B, np.int64), np.zeros((B, r.P - 1, Cc), np.float32)) if ref is None else ref
    rows = list(range(B)) if slots is None else [int(v) for v in slots.cpu().tolist()]
    parts, t = [], 0
    for n in cut:
        xc = to_dev(x_np[:, t:t + n], dev)
        To = rr.ceil_div(n * r.L, r.M) + spare_rows
        y, check = guarded((B, To, Cc), torch.float32, dev, "ones")
        cnt, check_cnt = guarded((B,), torch.int32, dev, "ones")
        snap = snapshot(xc, slots, r.device_taps(dev))
        assert ops.resample_step(xc, r, state, slots=slots, out=y, cnt=cnt) is y and snap.unchanged()
        check("y"); check_cnt("cnt")
        want, wcnt, n_in, hist = rr.step_batch(x_np[:, t:t + n], r.taps, r.L, r.M, To, n_in, hist)
        assert rr.same_bits(y.cpu().numpy(), want), (cut, t)                     # (NaN behind each row's outputs included)
        assert cnt.cpu().tolist() == list(wcnt), (cut, t)
        words = rr.state_words(n_in, hist, int(lay.n_in), int(lay.stride))
        assert (_state_bits(state)[rows] == words).all(), (cut, t)
        parts.append(want[:, :int(wcnt[0])])
        t += n
    return np.concatenate(parts, 1), (n_in, hist)


@pytest.mark.parametrize("L,M,P", [(5, 8, 36), (1, 2, 47)])
@pytest.mark.parametrize("Cc", [8, 3])
def test_cuts_slots_and_neighbours_do_not_show(nsd, dev, L, M, P, Cc):
    r = _rs(nsd, L, M, P)
    x = _raw(3, 41, Cc)
    want = _ref_trials(x, r)
    blank, _, lay = _new_state(dev, Cc, r, 1)
    assert not _state_bits(blank).any()                                        # a reset slot is all zero
    finals = []
    for cut in CUTS:
        state, check, lay = _new_state(dev, Cc, r, 3)
        got, _ = _run_cut(dev, x, r, cut, state, lay, spare_rows=len(cut) % 2)
        check("state")
        assert rr.same_bits(got, want), cut
        finals.append(_state_bits(state))
        assert (finals[-1] == finals[0]).all(), cut
    assert any(rr.out_steps(L, M, n, 1) == 0 for n in range(41))                # [1] * 41 held chunks that emit nothing
    # permuted slots inside a larger state, with other streams in the same calls
    S, perm = 7, [5, 0, 3, 6, 2]
    other = _raw(2, 41, Cc, seed=9)
    state, check, lay = _new_state(dev, Cc, r, S)
    slots = torch.tensor(perm, dtype=torch.int32, device=dev)
    got, _ = _run_cut(dev, np.concatenate([x, other]), r, [7, 1, 33], state, lay, slots=slots)
    check("state")
    assert rr.same_bits(got[:3], want) and rr.same_bits(got[3:], _ref_trials(other, r))
    st = _state_bits(state)
    for b in range(3):
        assert (st[perm[b]] == finals[0][b]).all(), b
    assert not st[1].any() and not st[4].any()                                 # slots nobody named stay reset


def test_a_slot_index_outside_the_state_gives_a_nan_row_count_zero_and_touches_nothing(nsd, dev):
    from nsd_amd import ops
    r = _rs(nsd, 5, 8, 36)
    x = _raw(4, 37, 8)
    for bad in (4, -1, 2**31 - 1, -2**31):
        state, check, lay = _new_state(dev, 8, r, 4)
        slots = torch.tensor([1, bad, 0, 2], dtype=torch.int32, device=dev)
        To = rr.ceil_div(37 * 5, 8)
        y, check_y = guarded((4, To, 8), torch.float32, dev, "zeros")
        cnt, check_cnt = guarded((4,), torch.int32, dev, "ones")
        ops.resample_step(to_dev(x, dev), r, state, slots=slots, out=y, cnt=cnt)
        check("state"); check_y("y"); check_cnt("cnt")
        got = y.cpu().numpy()
        assert np.isnan(got[1]).all() and cnt.cpu().tolist() == [To, 0, To, To], bad
        want, _, n_in, hist = rr.step_batch(x[[2, 0, 3]], r.taps, 5, 8, To)    # slot 0 <- stream 2, slot 1 <- stream 0, slot 2 <- stream 3
        assert rr.same_bits(got[[2, 0, 3]], want), bad
        st = _state_bits(state)
        assert (st[:3] == rr.state_words(n_in, hist, int(lay.n_in), int(lay.stride))).all() and not st[3].any(), bad


def test_more_streams_than_the_grid_cap(nsd, dev):
    r = _rs(nsd, 1, 2, 3)
    B = GRID_CAP + 7
    x = _raw(B, 6, 8)
    state, check, lay = _new_state(dev, 8, r, B)
    got, _ = _run_cut(dev, x, r, [3, 3], state, lay)
    check("state")
    assert rr.same_bits(got, _ref_trials(x, r))


def test_side_stream_and_graph_replay(nsd, dev):
    from nsd_amd import ops
    r = _rs(nsd, 1, 2, 47)
    x = _raw(3, 60, 8)
    xd = to_dev(x, dev)
    chunks = [xd[:, :20].contiguous(), xd[:, 20:40].contiguous(), xd[:, 40:].contiguous()]
    s0, _, lay = _new_state(dev, 8, r, 3)
    y0 = [ops.resample_step(c, r, s0) for c in chunks]
    want = _ref_trials(x, r)
    assert rr.same_bits(torch.cat(y0, 1).cpu().numpy(), want)
    # a side stream
    side = torch.cuda.Stream(device=dev)
    s1, _, _ = _new_state(dev, 8, r, 3)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        y1 = [ops.resample_step(c, r, s1) for c in chunks]
    side.synchronize()
    assert torch.equal(s1, s0) and all(torch.equal(a, b) for a, b in zip(y0, y1))
    # one captured call on a static chunk of even length, replayed once per chunk: every replay advances the slots by 20 samples
    s2, check, _ = _new_state(dev, 8, r, 3)
    xs, ys = torch.zeros_like(chunks[0]), torch.full((3, 10, 8), NAN, device=dev)
    cnt = torch.full((3,), -1, dtype=torch.int32, device=dev)
    r.device_taps(dev)                                                         # (the table goes to the device outside the capture)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.resample_step(xs, r, s2, out=ys, cnt=cnt)
    ops.resample_reset(8, r, s2)                                               # (whatever the capture did or did not run)
    for k, c in enumerate(chunks):
        xs.copy_(c); ys.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(ys, y0[k]) and cnt.cpu().tolist() == [10] * 3, k
    check("state")
    assert torch.equal(s2, s0)


def test_reset_of_named_slots_leaves_the_others(nsd, dev):
    from nsd_amd import ops
    r = _rs(nsd, 5, 8, 36)
    x = _raw(4, 20, 8)
    state, check, lay = _new_state(dev, 8, r, 4)
    _, ref = _run_cut(dev, x, r, [20], state, lay)
    before = _state_bits(state)
    ops.resample_reset(8, r, state, torch.tensor([2, 9, -1], dtype=torch.int32, device=dev))    # indices outside [0, S) are skipped
    check("state")
    after = _state_bits(state)
    assert not after[2].any() and (np.delete(after, 2, 0) == np.delete(before, 2, 0)).all()
    # the reset slot starts over, the others go on -- pushed apart, since their counts differ
    more = _raw(4, 13, 8, seed=3)
    keep = torch.tensor([0, 1, 3], dtype=torch.int32, device=dev)
    _run_cut(dev, more[[0, 1, 3]], r, [13], state, lay, slots=keep, ref=(ref[0][[0, 1, 3]], ref[1][[0, 1, 3]]))
    _run_cut(dev, more[[2]], r, [13], state, lay, slots=torch.tensor([2], dtype=torch.int32, device=dev))


# ---- the buffer contract -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", ["zeros", "ones", "nan32", "stale"])
def test_buffers_of_exact_size_inputs_unchanged_outputs_fully_written(nsd, dev, fill):
    from nsd_amd import ops
    r = _rs(nsd, 5, 8, 36)
    prior = None
    for B, T in ((5, 90), (3, 41)) if fill == "stale" else ((3, 41),):        # stale: the buffers of an earlier, larger call
        x = _raw(B, T, 8, seed=B)
        xg, check_x = guarded(x.shape, torch.float32, dev)
        xg.copy_(to_dev(x, dev))
        tg, check_t = guarded((r.L, r.P), torch.float32, dev)
        tg.copy_(to_dev(r.taps.copy(), dev))
        lay = ops.resample_layout(8, r)
        To = rr.ceil_div(T * r.L, r.M) + 2
        this = fill if prior else ("nan32" if fill == "stale" else fill)
        gy = Guarded((B, To, 8), torch.float32, dev, this, prior["y"] if prior else None)
        gs = Guarded((B, int(lay.stride)), torch.float32, dev, this, prior["s"] if prior else None)
        gc = Guarded((B,), torch.int32, dev, this, prior["c"] if prior else None)
        ops.resample_reset(8, r, gs.payload)
        snap = snapshot(xg, tg)
        ops.resample_step(xg, r, gs.payload, out=gy.payload, cnt=gc.payload, taps=tg)
        for g, name in ((gy, "y"), (gs, "state"), (gc, "cnt")):
            g.check(name)
        check_x("x"); check_t("taps")
        assert snap.unchanged()
        want, wcnt, n_in, hist = rr.step_batch(x, r.taps, 5, 8, To)
        assert rr.same_bits(gy.payload.cpu().numpy(), want) and gc.payload.cpu().tolist() == list(wcnt)
        assert (_state_bits(gs.payload) == rr.state_words(n_in, hist, int(lay.n_in), int(lay.stride))).all()
        prior = {"y": gy, "s": gs, "c": gc}


# ---- poison ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,M,P", [(5, 8, 36), (1, 2, 47), (2, 1, 24)])
def test_an_inf_and_a_nan_sample_poison_exactly_their_window_and_the_stage_heals(nsd, dev, L, M, P):
    r = nsd.Resample.design({(5, 8): 200, (1, 2): 250, (2, 1): 62.5}[(L, M)], 125)           # (zero-padded taps: 0 * Inf is NaN too)
    assert (r.L, r.M, r.P) == (L, M, P)
    T = 4 * P + 30
    x = _raw(3, T, 8)
    n_inf, n_nan = 5, 2 * P + 9
    x[1, n_inf, 4], x[1, n_nan, 2] = np.inf, np.nan
    state, check, lay = _new_state(dev, 8, r, 3)
    got, _ = _run_cut(dev, x, r, [9, 3, T - 12], state, lay)
    check("state")
    bad = ~np.isfinite(got)
    assert not bad[0].any() and not bad[2].any()
    for c, n in ((4, n_inf), (2, n_nan)):
        want = np.zeros(got.shape[1], bool)
        want[rr.poisoned_outputs(L, M, P, n, T)] = True
        assert want.any() and not want[-1] and (bad[1, :, c] == want).all(), (c, n)
    assert not np.delete(bad[1], [2, 4], axis=1).any()
    assert rr.same_bits(_window(dev, x, r), got)


# ---- through the Python layers ---------------------------------------------------------------------------------------------------------
def _eval_model(nsd, dev, ref_state, seed=None, **kw):
    if seed is not None:
        torch.manual_seed(seed)
    m = nsd.EEG_LSTM(**kw)
    if seed is None:
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in ref_state.items()}, strict=True)
    return m.to(dev).eval()


def test_the_model_runs_the_conversion_as_stage_0(nsd, dev, ref_state):
    from nsd_amd import ops
    r = nsd.Resample.design(200, 125)
    P = nsd.CausalPrep.design(highpass=1.0, lowpass=40.0, zscore_seconds=0.4, var0=250.0)
    x = to_dev(_raw(6, 90, 8), dev)
    xr = ops.resample_trials(x, r)
    assert rr.same_bits(xr.cpu().numpy(), _ref_trials(x.cpu().numpy(), r))
    for kw in ({}, {"prep": P}, {"prep": P, "gate": nsd.SignalGate(rail=4000.0, hold_samples=3, max_bad=8)}):
        m, plain = _eval_model(nsd, dev, ref_state, resample=r, **kw), _eval_model(nsd, dev, ref_state, **kw)
        assert torch.equal(m.predict_proba(x), plain.predict_proba(xr)), kw
        with torch.no_grad():
            assert torch.equal(m(x), plain(xr)), kw
        pa, pb = m.predict_trials(x, window=16, hop=8), plain.predict_trials(xr, window=16, hop=8)
        assert torch.equal(pa[0], pb[0]) and torch.equal(pa[1], pb[1]), kw
        assert m.view_of(m.flat_parameters().clone()).resample == r
    with pytest.raises(nsd.NsdError, match="dx through the rate conversion"):
        m(x.clone().requires_grad_(True))
    with pytest.raises(nsd.NsdError):
        nsd.EnsembleStreamDecoder([m, _eval_model(nsd, dev, ref_state, seed=3)], streams=1)


def _same(u, v) -> bool:
    """device tensors bit for bit (NaN rows of unused windows included); None only against None"""
    if u is None or v is None:
        return u is None and v is None
    if isinstance(u, tuple):
        return len(u) == len(v) and all(_same(p, q) for p, q in zip(u, v))
    return u.shape == v.shape and u.dtype == v.dtype and torch.equal(u.contiguous().view(torch.uint8), v.contiguous().view(torch.uint8))


def _ref_chunks(x, r, cut):
    """the reference's resampled chunks of streams pushed together -> [(input chunk, resampled chunk [B,cnt,C])]"""
    n_in, hist, t, out = None, None, 0, []
    for n in cut:
        y, cnt, n_in, hist = rr.step_batch(x[:, t:t + n], r.taps, r.L, r.M, rr.ceil_div(n * r.L, r.M), n_in, hist)
        out.append((x[:, t:t + n], y[:, :int(cnt[0])]))
        t += n
    return out


@pytest.mark.parametrize("kind", ["stream", "ensemble", "sliding", "ensemble_sliding"])
@pytest.mark.parametrize("L,M,cut", [(5, 8, [7, 1, 33, 23]), (1, 2, [14, 1, 1, 40, 24])])
def test_each_decoder_with_the_conversion_equals_the_plain_one_on_the_reference_chunks(nsd, dev, ref_state, kind, L, M, cut):
    r = nsd.Resample.design({(5, 8): 200, (1, 2): 250}[(L, M)], 125)
    P = nsd.CausalPrep.design(highpass=1.0, zscore_seconds=0.4, var0=250.0)
    x = _raw(2, sum(cut), 8)
    assert rr.out_steps(L, M, 0, sum(cut)) == 40                              # T = 40 at the model's rate; window 16, hop 8

    def build(**kw):
        if kind in ("stream", "sliding"):
            return _eval_model(nsd, dev, ref_state, prep=P, **kw)
        return [_eval_model(nsd, dev, ref_state, prep=P, **kw), _eval_model(nsd, dev, ref_state, seed=5, prep=P, **kw)]
    cls = {"stream": nsd.StreamDecoder, "ensemble": nsd.EnsembleStreamDecoder, "sliding": nsd.SlidingStreamDecoder,
           "ensemble_sliding": nsd.EnsembleSlidingStreamDecoder}[kind]
    extra = dict(window=16, hop=8) if "sliding" in kind else {}
    a, b = cls(build(resample=r), streams=3, **extra), cls(build(), streams=3, **extra)
    mid, decided = None, 0
    for k, (xin, xres) in enumerate(_ref_chunks(x, r, cut)):
        out = a.push(xin)
        if xres.shape[1] == 0:                                                 # no step: the conversion alone advanced
            assert out is None if "sliding" not in kind else (out[0].shape[1] == 0 and out[2].cpu().tolist() == [0, 0]), k
        else:
            want = b.push(xres)
            assert _same(out, want), k
            if "sliding" in kind:
                decided += int(out[2].sum())
        assert torch.equal(a.state, b.state) and torch.equal(a.prep_state, b.prep_state), k
        assert list(a.steps) == list(b.steps) and list(a.input_steps[:2]) == [sum(cut[:k + 1])] * 2, k
        if k == 1:
            mid = a.state_dict()
    assert list(a.steps[:2]) == [40, 40] and ("sliding" not in kind or decided == 2 * 4)
    # a checkpoint taken mid-stream: a second decoder goes on from it, bit for bit
    assert "resample_state" in mid and mid["resample_n_in"].tolist()[:2] == [sum(cut[:2])] * 2
    c = cls(build(resample=r), streams=3, **extra)
    c.load_state_dict(mid)
    d = cls(build(resample=r), streams=3, **extra)
    for xin, _ in _ref_chunks(x, r, cut)[:2]:
        d.push(xin)
    for xin, _ in _ref_chunks(x, r, cut)[2:]:
        assert _same(c.push(xin), d.push(xin))
    assert torch.equal(c.state, a.state) and torch.equal(c.resample_state, a.resample_state) and list(c.input_steps) == list(a.input_steps)
    with pytest.raises(nsd.NsdError, match="rate conversion"):
        b.load_state_dict(mid)
    # streams that hold different counts and would emit different numbers of steps are refused before anything runs
    if (L, M) == (1, 2):
        before = a.resample_state.clone()
        a.push(x[:1, :1], slots=[2])
        held = a.resample_state.clone()
        with pytest.raises(nsd.NsdError, match="push those slots separately"):
            a.push(x[:2, :1], slots=[0, 2])
        assert torch.equal(a.resample_state, held) and not torch.equal(held, before)
    a.reset([0])
    assert list(a.input_steps) == [0] + list(c.input_steps[1:2]) + [a.input_steps[2]] and not a.resample_state[0].any()


def test_trains_checkpoint_carries_the_conversion_and_the_predictor_rebuilds_it(nsd, dev, tmp_path, capsys):
    from nsd_amd import ops, train
    out = str(tmp_path / "m.pth")
    rc = train.main(["--synthetic", "24", "--T", "80", "--epochs", "1", "--batch", "8", "--input-rate", "250", "--out", out])
    assert rc == 0
    done = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert done["done"] and done["args"]["input_rate"] == 250.0 and done["args"]["T"] == 40
    ckpt = torch.load(out, map_location="cpu", weights_only=True)
    want = nsd.Resample.design(250, 125)
    assert nsd.Resample.from_dict(ckpt["nsd_resample"]) == want
    pred = nsd.SimplePredictor(out, sr=250, device="cpu", preprocess="identity")
    assert pred.model.resample == want and pred.model_rate == 125.0
    x = _raw(1, 80, 8)
    probs, _ = pred.predict(x[0])
    plain = nsd.EEG_LSTM().to(dev).eval()
    plain.load_state_dict(ckpt["state_dict"], strict=True)
    assert probs.tobytes() == plain.predict_proba(ops.resample_trials(to_dev(x, dev), want))[0].cpu().numpy().tobytes()
    # a plain checkpoint and another amplifier: model_rate= designs the conversion; with neither, nothing is converted
    from nsd_amd.trainer import save_reference_checkpoint
    path = str(tmp_path / "plain.pth")
    save_reference_checkpoint(plain, path)
    assert nsd.SimplePredictor(path, sr=125, device="cpu", preprocess="identity").model.resample is None
    p256 = nsd.SimplePredictor(path, sr=256, device="cpu", preprocess="identity", model_rate=125)
    assert p256.model.resample == nsd.Resample.design(256, 125) and abs(p256.model_rate - 125.0) < 1e-9
    st = p256.open_stream(streams=1, window_seconds=0.128, hop_seconds=0.064)
    assert (st.decoder.window, st.decoder.hop) == (16, 8)
