"""Sliding-window decisions for continuous streams (nsd_window_* of include/nsd.h, csrc/nsd_window48.hip).  Needs the MI355X.

The contract is one of BITS: the decision of window k is what nsd_stream_step writes when a freshly reset slot is given
x[k hop : k hop + window] -- whatever the cut of the stream into calls, B, the slot, the placement in the grid, the HIP stream or a graph
replay.  So the reference of every test here is nsd_stream_step itself (tests/test_gpu_stream.py holds that one to the oracle), run
once per (variant, window start, window length) and left unchanged; one decision is held to the oracle directly, at the bound that
file uses for prefix outputs.  Which windows a call completes, their rows and ends come from the integer schedule of
tests/window_ref.py.  Outputs are pre-filled with 0xFF bytes, states with NaN.  Each case takes a few milliseconds.
"""
import re

import numpy as np
import pytest
import torch

from oracle import nsd_oracle as orc
from tests import prep_ref as pr
from tests import stream_ref as sr
from tests import test_gpu_stream as tgs
from tests import window_ref as wr
from tests.buffer_contract import guarded, snapshot
from tests.golden.make_goldens import synth_x
from tests.gpu_harness import NAN, PROB_TOL, D, cus, dev, nsd, spec_of, sync_at_the_end, to_dev, write_pth  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

T41, B41 = tgs.T41, tgs.B41
WINDOWS_41 = [(12, 4), (12, 12), (1, 1), (5, 1)]


# ---------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------
def _new_state(dev, spec, W, Hp, S):
    """S streams, NaN-filled, then reset through the library"""
    from nsd_amd import ops
    state = torch.full((S, int(ops.window_layout(spec, W, Hp).stream_stride)), NAN, device=dev)
    ops.window_reset(spec, W, Hp, state)
    return state


def _outs(dev, B, Dr, K):
    """output buffers of one call, every byte 0xFF"""
    lg = torch.full((B, Dr, K), -1, dtype=torch.int32, device=dev).view(torch.float32)
    prb = torch.full((B, Dr, K), -1, dtype=torch.int32, device=dev).view(torch.float32)
    return lg, prb, torch.full((B, Dr), -7, dtype=torch.int64, device=dev), torch.full((B,), -7, dtype=torch.int32, device=dev)


def _wstep(dev, spec, flat, x, state, W, Hp, *, slots=None, residual=False):
    """one nsd_window_step into 0xFF-filled outputs -> numpy logits [B,D,K], probs, ends [B,D], counts [B]"""
    from nsd_amd import ops
    B, T = int(x.shape[0]), int(x.shape[1])
    out = _outs(dev, B, wr.rows(T, Hp), spec.K)
    got = ops.window_step(spec, flat, x.contiguous(), state, window=W, hop=Hp, slots=slots, residual=residual, out=out)
    assert all(g is o for g, o in zip(got, out))
    return tuple(t.cpu().numpy() for t in out)


def _unused_ok(lg, prb, ends, b, first):
    return np.isnan(lg[b, first:]).all() and np.isnan(prb[b, first:]).all() and (ends[b, first:] == -1).all()


def _run(dev, spec, flat, x, cut, state, W, Hp, *, slots=None, residual=False, n0=0):
    """push x [B, sum(cut), C] in the chunks of `cut` onto streams that have seen n0 samples; the schedule of every call is held to
    window_ref.  -> {k: (logits [B,K], probs [B,K])} of the completed windows"""
    got, t = {}, 0
    B = int(x.shape[0])
    for n in cut:
        lg, prb, ends, counts = _wstep(dev, spec, flat, x[:, t:t + n], state, W, Hp, slots=slots, residual=residual)
        exp = wr.completed(n0 + t, n, W, Hp)
        assert lg.shape == (B, wr.rows(n, Hp), spec.K) and list(counts) == [len(exp)] * B, (n0 + t, n, counts)
        for k, e, row in exp:
            assert (ends[:, row] == e).all() and k not in got, (k, e, row, ends)
            got[k] = (lg[:, row].copy(), prb[:, row].copy())
        for b in range(B):
            assert _unused_ok(lg, prb, ends, b, len(exp)), (n0 + t, n, b)
        t += n
    return got


_refs = {}


def _window_ref(dev, name, ref_state, start, length):
    """(logits [3,K], probs [3,K], slot bytes per stream) of nsd_stream_step from reset slots on x[:, start:start+length] of a variant of
    tests/test_gpu_stream.py: computed once and left unchanged"""
    key = (name, start, length)
    if key not in _refs:
        d, residual, flat, x, _ = tgs._case(name, ref_state)
        spec = spec_of(d)
        st = tgs._new_state(dev, spec, B41)
        lg, prb = tgs._step(dev, spec, to_dev(flat, dev), to_dev(x[:, start:start + length], dev), st, residual=residual)
        _refs[key] = (lg, prb, st.cpu().numpy())
    return _refs[key]


def _phase_slots(spec, state_np, W, Hp):
    """[S, R, stride] phase slots and [S] header counts (phase 0's copy), [S, R] all copies"""
    from nsd_amd import ops
    lay = ops.window_layout(spec, W, Hp)
    R, ps = int(lay.phases), int(lay.phase_stride)
    S = state_np.shape[0]
    slots = state_np[:, :R * ps].reshape(S, R, ps)
    counts = np.ascontiguousarray(state_np[:, int(lay.count):int(lay.count) + 2 * R]).view(np.int64)
    return slots, counts


def _check_final_state(dev, name, ref_state, state, W, Hp, n):
    """every phase slot == the nsd_stream_step slot fed that phase's partial window; every copy of the count == n"""
    d = tgs._case(name, ref_state)[0]
    spec = spec_of(d)
    slots, counts = _phase_slots(spec, state.cpu().numpy(), W, Hp)
    assert (counts == n).all(), counts
    reset = tgs._new_state(dev, spec, 1).cpu().numpy()[0]
    for r, (start, p) in enumerate(wr.phases(n, W, Hp)):
        for b in range(B41):
            want = reset if p == 0 else _window_ref(dev, name, ref_state, start, p)[2][b]
            assert slots[b, r].tobytes() == want.tobytes(), (name, W, Hp, "phase", r, "stream", b, start, p)


# ---------------------------------------------------------------------------------------------------
# 1. every decision equals nsd_stream_step on the window, and the cut does not show
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", sr.CUTS_41, ids=["ones", "fib", "40+1", "whole"])
@pytest.mark.parametrize("W,Hp", WINDOWS_41)
@pytest.mark.parametrize("name", list(tgs.VARIANTS))
def test_every_decision_is_stream_step_on_its_window_and_the_cut_does_not_show(nsd, dev, ref_state, name, W, Hp, cut):
    d, residual, flat_np, xn, _ = tgs._case(name, ref_state)
    spec = spec_of(d)
    state = _new_state(dev, spec, W, Hp, B41)
    got = _run(dev, spec, to_dev(flat_np, dev), to_dev(xn, dev), cut, state, W, Hp, residual=residual)
    assert sorted(got) == list(range((T41 - W) // Hp + 1)), sorted(got)
    for k, (lg, prb) in got.items():
        rl, rp, _ = _window_ref(dev, name, ref_state, k * Hp, W)
        assert lg.tobytes() == rl.tobytes() and prb.tobytes() == rp.tobytes(), (name, W, Hp, cut, "window", k)
    _check_final_state(dev, name, ref_state, state, W, Hp, T41)


# ---------------------------------------------------------------------------------------------------
# 2. staging across a boundary that is not a multiple of 32
# ---------------------------------------------------------------------------------------------------
def test_segments_that_begin_off_the_staging_grid(nsd, dev, ref_state):
    W, Hp, T, B = 70, 35, 200, 2
    spec = spec_of(D)
    flat_np, xn = orc.flatten_state(ref_state, D), synth_x(B, T, seed=7035)
    flat, x = to_dev(flat_np, dev), to_dev(xn, dev)
    want = {}
    for k in range((T - W) // Hp + 1):
        st = tgs._new_state(dev, spec, B)
        want[k] = tgs._step(dev, spec, flat, x[:, k * Hp:k * Hp + W], st)
    assert len(wr.completed(0, T, W, Hp)) == 4 and len(want) == 4       # two windows of each phase complete inside the single call
    states = []
    for cut in ([200], [100, 100], [33, 67, 99, 1]):
        state = _new_state(dev, spec, W, Hp, B)
        got = _run(dev, spec, flat, x, cut, state, W, Hp)
        assert sorted(got) == sorted(want), cut
        for k in want:
            assert got[k][0].tobytes() == want[k][0].tobytes() and got[k][1].tobytes() == want[k][1].tobytes(), (cut, k)
        states.append(state.cpu().numpy().tobytes())
    assert states[0] == states[1] == states[2]


# ---------------------------------------------------------------------------------------------------
# 3. one decision from the oracle
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tgs.VARIANTS))
def test_window_zero_against_the_oracle(nsd, dev, ref_state, name):
    d, residual, flat_np, xn, refs = tgs._case(name, ref_state)
    spec = spec_of(d)
    state = _new_state(dev, spec, 12, 4, B41)
    got = _run(dev, spec, to_dev(flat_np, dev), to_dev(xn, dev), [T41], state, 12, 4, residual=residual)
    tgs._check_outputs(got[0][0], got[0][1], refs[12], (name, "window 0"))          # refs[12]: orc.forward on x[:, :12]


# ---------------------------------------------------------------------------------------------------
# 4. invariance: slot, batch, placement; more (stream, phase) pairs than compute units
# ---------------------------------------------------------------------------------------------------
def test_slot_and_batch_invariance(nsd, dev, ref_state):
    """B = 3 in slots [5, 0, 2] of S = 6 equals three B = 1 runs; the streams not named keep the bytes of the reset."""
    d, _, flat_np, xn, _ = tgs._case("ref", ref_state)
    spec, flat, x = spec_of(d), to_dev(flat_np, dev), to_dev(xn, dev)
    W, Hp, S, cut = 12, 4, 6, [7, 9, 25]
    perm = torch.tensor([5, 0, 2], dtype=torch.int32, device=dev)
    together = _new_state(dev, spec, W, Hp, S)
    before = together.cpu().numpy().copy()
    got3 = _run(dev, spec, flat, x, cut, together, W, Hp, slots=perm)
    tog = together.cpu().numpy()
    for s in (1, 3, 4):
        assert tog[s].tobytes() == before[s].tobytes(), s
    for b, slot in enumerate([5, 0, 2]):
        alone = _new_state(dev, spec, W, Hp, S)
        got1 = _run(dev, spec, flat, x[b:b + 1], cut, alone, W, Hp, slots=perm[b:b + 1].contiguous())
        assert sorted(got1) == sorted(got3)
        for k in got3:
            assert got1[k][0].tobytes() == got3[k][0][b:b + 1].tobytes() and got1[k][1].tobytes() == got3[k][1][b:b + 1].tobytes(), (b, k)
        a = alone.cpu().numpy()
        assert a[slot].tobytes() == tog[slot].tobytes(), slot
        assert all(a[s].tobytes() == before[s].tobytes() for s in range(S) if s != slot)


def test_more_stream_phase_pairs_than_compute_units(nsd, dev, cus, ref_state):
    """B * R just above the CU count, chunks of 3 and 4 with (5, 1): some workgroups walk a second pair; a sample of single-stream runs."""
    W, Hp = 5, 1
    R = W // Hp
    B = cus // R + 1
    assert B * R > cus
    spec = spec_of(D)
    flat_np, xn = orc.flatten_state(ref_state, D), synth_x(B, 7, seed=1707)
    flat, x = to_dev(flat_np, dev), to_dev(xn, dev)
    state = _new_state(dev, spec, W, Hp, B)
    got = _run(dev, spec, flat, x, [3, 4], state, W, Hp)
    assert sorted(got) == [0, 1, 2]
    big = state.cpu().numpy()
    for b in (0, 1, B // 2, B - 2, B - 1):
        one = _new_state(dev, spec, W, Hp, 1)
        g1 = _run(dev, spec, flat, x[b:b + 1], [3, 4], one, W, Hp)
        for k in got:
            assert g1[k][0].tobytes() == got[k][0][b:b + 1].tobytes() and g1[k][1].tobytes() == got[k][1][b:b + 1].tobytes(), (b, k)
        assert one.cpu().numpy()[0].tobytes() == big[b].tobytes(), b
    st = tgs._new_state(dev, spec, B)                                  # and window 1 of every stream against nsd_stream_step
    lg, prb = tgs._step(dev, spec, flat, x[:, 1:6], st)
    assert got[1][0].tobytes() == lg.tobytes() and got[1][1].tobytes() == prb.tobytes()


def test_a_sample_count_past_2_to_the_31(nsd, dev, ref_state):
    """After W samples the phases stand where they stand after W * 2^30: the count is set there in the header and the stream goes on --
    the same decisions, in the same rows, with ends that are int64."""
    from nsd_amd import ops
    d, _, flat_np, xn, _ = tgs._case("ref", ref_state)
    spec, flat, x = spec_of(d), to_dev(flat_np, dev), to_dev(xn, dev)
    W, Hp = 12, 4
    far = W * 2 ** 30
    assert far > 2 ** 31 and wr.phases(far, W, Hp)[1:] == [(far - p, p) for _, p in wr.phases(W, W, Hp)[1:]]
    near, moved = _new_state(dev, spec, W, Hp, B41), _new_state(dev, spec, W, Hp, B41)
    for state in (near, moved):
        _run(dev, spec, flat, x[:, :W], [W], state, W, Hp)
    lay = ops.window_layout(spec, W, Hp)
    col = int(lay.count) // 2
    moved.view(torch.int64)[:, col:col + int(lay.phases)] = far
    for cut in ([5], [24]):
        t0 = W if cut == [5] else W + 5
        a = _wstep(dev, spec, flat, x[:, t0:t0 + cut[0]], near, W, Hp)
        b = _wstep(dev, spec, flat, x[:, t0:t0 + cut[0]], moved, W, Hp)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[3].tobytes() == b[3].tobytes(), cut
        assert list(a[3]) == [len(wr.completed(t0, cut[0], W, Hp))] * B41 and a[3][0] > 0
        assert np.array_equal(np.where(a[2] >= 0, a[2] + (far - W), -1), b[2]) and b[2].dtype == np.int64 and b[2].max() > 2 ** 31
        assert [(k - (far - W) // Hp, e - (far - W), row) for k, e, row in wr.completed(t0 + far - W, cut[0], W, Hp)] == wr.completed(t0, cut[0], W, Hp)
    sa, sb = _phase_slots(spec, near.cpu().numpy(), W, Hp), _phase_slots(spec, moved.cpu().numpy(), W, Hp)
    assert sa[0].tobytes() == sb[0].tobytes() and (sa[1] == T41).all() and (sb[1] == T41 + far - W).all()


# ---------------------------------------------------------------------------------------------------
# 5. reset
# ---------------------------------------------------------------------------------------------------
def test_reset_of_one_stream_restarts_only_it(nsd, dev, ref_state):
    from nsd_amd import ops
    d, _, flat_np, xn, _ = tgs._case("ref", ref_state)
    spec, flat, x = spec_of(d), to_dev(flat_np, dev), to_dev(xn, dev)
    W, Hp = 12, 4
    state = _new_state(dev, spec, W, Hp, B41)
    _run(dev, spec, flat, x[:, :13], [13], state, W, Hp)
    ops.window_reset(spec, W, Hp, state, torch.tensor([1], dtype=torch.int32, device=dev))
    now = state.cpu().numpy()
    assert now[1].tobytes() == _new_state(dev, spec, W, Hp, 1).cpu().numpy()[0].tobytes()
    assert [list(c) for c in _phase_slots(spec, now, W, Hp)[1]] == [[13] * 3, [0] * 3, [13] * 3]
    # stream 1 starts over with its samples 13..; the others go on
    lg, prb, ends, counts = _wstep(dev, spec, flat, x[:, 13:], state, W, Hp)
    fresh = _new_state(dev, spec, W, Hp, 1)
    l1, p1, e1, c1 = _wstep(dev, spec, flat, x[1:2, 13:], fresh, W, Hp)
    assert list(counts) == [len(wr.completed(13, 28, W, Hp)), len(wr.completed(0, 28, W, Hp)), len(wr.completed(13, 28, W, Hp))]
    assert lg[1:2].tobytes() == l1.tobytes() and prb[1:2].tobytes() == p1.tobytes() and ends[1:2].tobytes() == e1.tobytes() and counts[1] == c1[0]
    assert state.cpu().numpy()[1].tobytes() == fresh.cpu().numpy()[0].tobytes()
    for k, e, row in wr.completed(13, 28, W, Hp):
        rl, rp, _ = _window_ref(dev, "ref", ref_state, k * Hp, W)
        assert lg[[0, 2], row].tobytes() == rl[[0, 2]].tobytes() and prb[[0, 2], row].tobytes() == rp[[0, 2]].tobytes() and ends[0, row] == e


# ---------------------------------------------------------------------------------------------------
# 6. skips
# ---------------------------------------------------------------------------------------------------
def test_a_bad_slot_or_another_window_is_skipped_and_never_silent(nsd, dev, ref_state):
    from nsd_amd import ops
    d, _, flat_np, xn, _ = tgs._case("ref", ref_state)
    spec, flat, x = spec_of(d), to_dev(flat_np, dev), to_dev(xn, dev)
    W, Hp, S = 12, 4, 4
    state, check = guarded((S, int(ops.window_layout(spec, W, Hp).stream_stride)), torch.float32, dev, "nan32")
    ops.window_reset(spec, W, Hp, state)
    check("window state after reset")
    before = state.cpu().numpy().copy()
    clean = _new_state(dev, spec, W, Hp, S)
    lc, pc, ec, cc = _wstep(dev, spec, flat, x[:, :17], clean, W, Hp, slots=torch.tensor([2, 1, 0], dtype=torch.int32, device=dev))
    for bad in (S, -1):
        state.copy_(torch.from_numpy(before).to(dev))
        lg, prb, ends, counts = _wstep(dev, spec, flat, x[:, :17], state, W, Hp, slots=torch.tensor([2, bad, 0], dtype=torch.int32, device=dev))
        check("window state")
        assert counts[1] == -1 and _unused_ok(lg, prb, ends, 1, 0), bad
        assert list(counts[[0, 2]]) == [2, 2] and lg[[0, 2]].tobytes() == lc[[0, 2]].tobytes() and prb[[0, 2]].tobytes() == pc[[0, 2]].tobytes()
        assert ends[[0, 2]].tobytes() == ec[[0, 2]].tobytes()
        now = state.cpu().numpy()
        assert now[1].tobytes() == before[1].tobytes() and now[3].tobytes() == before[3].tobytes(), bad
    ops.window_reset(spec, W, Hp, state, torch.tensor([S, 1], dtype=torch.int32, device=dev))       # a reset that names it skips it
    check("window state after a reset with a bad index")
    # a state reset with (12, 4), stepped with (12, 6): every stream skipped, no byte of the state touched
    state.copy_(torch.from_numpy(before).to(dev))
    lg, prb, ends, counts = _wstep(dev, spec, flat, x[:, :17], state, 12, 6)
    check("window state, other hop")
    assert list(counts) == [-1] * 3 and all(_unused_ok(lg, prb, ends, b, 0) for b in range(3))
    assert state.cpu().numpy().tobytes() == before.tobytes()


# ---------------------------------------------------------------------------------------------------
# 7. a sample that is not finite poisons exactly the windows that contain it
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", [[T41], [9, 32], [1] * T41], ids=["whole", "9+32", "ones"])
def test_nan_containment(nsd, dev, ref_state, cut):
    d, _, flat_np, xn, _ = tgs._case("ref", ref_state)
    spec, flat = spec_of(d), to_dev(flat_np, dev)
    W, Hp = 12, 4
    for poison in (np.nan, -np.inf):
        xb = xn.copy()
        xb[1, 17, 2] = poison
        dirty = _new_state(dev, spec, W, Hp, B41)
        got = _run(dev, spec, flat, to_dev(xb, dev), cut, dirty, W, Hp)
        assert sorted(got) == list(range(8))
        for k, (lg, prb) in got.items():
            rl, rp, _ = _window_ref(dev, "ref", ref_state, k * Hp, W)
            hit = k in (2, 3, 4)                                        # [8, 20), [12, 24), [16, 28) hold sample 17
            assert hit == (k * Hp <= 17 < k * Hp + W)
            if hit:
                assert np.isnan(lg[1]).all() and np.isnan(prb[1]).all(), k
                assert lg[[0, 2]].tobytes() == rl[[0, 2]].tobytes() and prb[[0, 2]].tobytes() == rp[[0, 2]].tobytes(), k
            else:                                                       # including windows 5 .. 7, completed after it has left
                assert lg.tobytes() == rl.tobytes() and prb.tobytes() == rp.tobytes(), k
        _check_final_state(dev, "ref", ref_state, dirty, W, Hp, T41)    # the stream has healed: its state is the clean run's


# ---------------------------------------------------------------------------------------------------
# 8. side stream, graph replay
# ---------------------------------------------------------------------------------------------------
def test_side_stream_and_prep_plus_window_replayed_as_one_graph(nsd, dev, ref_state):
    from nsd_amd import ops
    d, _, flat_np, xn, _ = tgs._case("ref", ref_state)
    spec, flat, x = spec_of(d), to_dev(flat_np, dev), to_dev(xn, dev)
    W, Hp = 12, 4
    side = torch.cuda.Stream(device=dev)
    state = _new_state(dev, spec, W, Hp, B41)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        got = _run(dev, spec, flat, x, [20, 21], state, W, Hp)
    side.synchronize()
    for k, (lg, prb) in got.items():
        rl, rp, _ = _window_ref(dev, "ref", ref_state, k * Hp, W)
        assert lg.tobytes() == rl.tobytes() and prb.tobytes() == rp.tobytes(), k
    _check_final_state(dev, "ref", ref_state, state, W, Hp, T41)

    # nsd_prep_step + nsd_window_step captured once (a chain: no parallel branches), replayed over five chunks of 8 samples
    P = nsd.CausalPrep.design(highpass=1.0, lowpass=40.0, zscore_seconds=0.4, var0=250.0)
    n, chunks = 8, 5
    Dr = wr.rows(n, Hp)
    eager = []
    ps, ws = ops.prep_state(spec.C, B41, dev), _new_state(dev, spec, W, Hp, B41)
    for i in range(chunks):
        y = ops.prep_step(x[:, i * n:(i + 1) * n].contiguous(), P, ps)
        eager.append(tuple(a.tobytes() for a in _wstep(dev, spec, flat, y, ws, W, Hp)))
    xin, y = torch.empty((B41, n, spec.C), device=dev), torch.empty((B41, n, spec.C), device=dev)
    gps, gws = ops.prep_state(spec.C, B41, dev), _new_state(dev, spec, W, Hp, B41)
    out = _outs(dev, B41, Dr, spec.K)
    xin.copy_(x[:, :n])
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.prep_step(xin, P, gps, out=y)
        ops.window_step(spec, flat, y, gws, window=W, hop=Hp, out=out)
    ops.prep_reset(spec.C, gps)                                        # (whatever the capture did or did not run)
    ops.window_reset(spec, W, Hp, gws)
    for i in range(chunks):
        xin.copy_(x[:, i * n:(i + 1) * n])
        for o in out:
            o.view(torch.uint8).fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert tuple(o.cpu().numpy().tobytes() for o in out) == eager[i], i
    assert gws.cpu().numpy().tobytes() == ws.cpu().numpy().tobytes() and gps.cpu().numpy().tobytes() == ps.cpu().numpy().tobytes()
    assert sum(len(wr.completed(i * n, n, W, Hp)) for i in range(chunks)) == 8


# ---------------------------------------------------------------------------------------------------
# 9. buffer contract
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", ["ones", "nan32"])
def test_buffer_contract(nsd, dev, ref_state, fill):
    from nsd_amd import ops
    d, _, flat_np, xn, _ = tgs._case("ref", ref_state)
    spec, flat, x = spec_of(d), to_dev(flat_np, dev), to_dev(xn[:, :17], dev).contiguous()
    W, Hp, S = 12, 4, B41
    Dr = wr.rows(17, Hp)
    nbytes = ops.window_layout(spec, W, Hp).stream_stride * 4 * S
    state, cs = guarded((S, int(ops.window_layout(spec, W, Hp).stream_stride)), torch.float32, dev, fill)
    assert state.numel() * 4 == nbytes
    bufs = [guarded((B41, Dr, spec.K), torch.float32, dev, fill), guarded((B41, Dr, spec.K), torch.float32, dev, fill),
            guarded((B41, Dr), torch.int64, dev, fill), guarded((B41,), torch.int32, dev, fill)]
    ops.window_reset(spec, W, Hp, state)
    cs("state after nsd_window_reset")
    assert state.cpu().numpy().tobytes() == _new_state(dev, spec, W, Hp, S).cpu().numpy().tobytes()     # nothing of the fill is left
    snap = snapshot(flat, x)
    out = tuple(b[0] for b in bufs)
    ops.window_step(spec, flat, x, state, window=W, hop=Hp, out=out)
    torch.cuda.synchronize(dev)
    cs("state after nsd_window_step")
    for (_, check), what in zip(bufs, ("logits", "probs", "ends", "counts")):
        check(what)
    assert snap.unchanged()
    ref = _new_state(dev, spec, W, Hp, S)
    want = _wstep(dev, spec, flat, x, ref, W, Hp)
    assert all(o.cpu().numpy().tobytes() == w.tobytes() for o, w in zip(out, want))     # no byte of the fill shows in an output
    assert state.cpu().numpy().tobytes() == ref.cpu().numpy().tobytes()


# ---------------------------------------------------------------------------------------------------
# 10. the Python surface
# ---------------------------------------------------------------------------------------------------
def _kw(p):
    return dict(sections=p.sections, alpha=p.alpha, var0=p.var0, baseline=p.baseline, car=p.car)


@pytest.mark.parametrize("with_prep", [False, True], ids=["plain", "prep"])
def test_sliding_decoder_push_equals_stream_decoder_on_every_window(nsd, dev, golden, ref_state, with_prep):
    g = golden("real_trials")
    x = np.ascontiguousarray(g["x"][:2, :250], np.float32)                 # two recorded streams, 2 s at 125 Hz
    P = nsd.CausalPrep.design(highpass=1.0, lowpass=40.0, zscore_seconds=0.4, var0=250.0) if with_prep else None
    model, plain = tgs._eval_model(nsd, dev, ref_state, prep=P), tgs._eval_model(nsd, dev, ref_state)
    W, Hp, n = 100, 50, 25
    fed = pr.prep_ref(x, **_kw(P)) if with_prep else x                      # the continuously prepped stream
    dec = nsd.SlidingStreamDecoder(model, streams=3, window=W, hop=Hp)
    one = nsd.StreamDecoder(plain, streams=2)
    assert dec.latest() == [None] * 3
    seen = {}
    for t0 in range(0, 250, n):
        probs, ends, counts = dec.push(x[:, t0:t0 + n])
        assert probs.is_cuda and tuple(probs.shape) == (2, 1, 3) and ends.dtype == torch.int64 and counts.dtype == torch.int32
        exp = wr.completed(t0, n, W, Hp)
        assert list(counts.cpu().numpy()) == [len(exp)] * 2
        for k, e, row in exp:
            assert list(ends[:, row].cpu().numpy()) == [e, e]
            seen[k] = probs[:, row].cpu().numpy().copy()
            one.reset()
            want = one.push(fed[:, k * Hp:k * Hp + W]).cpu().numpy()
            assert seen[k].tobytes() == want.tobytes(), (with_prep, k)
            last = dec.latest()
            assert last[2] is None and all(last[b][0] == e and last[b][1].tobytes() == want[b].tobytes() for b in range(2))
    assert sorted(seen) == [0, 1, 2, 3] and list(dec.steps) == [250, 250, 0]


def test_sliding_decoder_state_dict_reset_and_refusals(nsd, dev, ref_state):
    d, _, _, xn, _ = tgs._case("ref", ref_state)
    model = tgs._eval_model(nsd, dev, ref_state)
    dec = nsd.SlidingStreamDecoder(model, streams=3, window=12, hop=4)
    dec.push(xn[:, :18])
    sd = dec.state_dict()
    other = nsd.SlidingStreamDecoder(model, streams=3, window=12, hop=4)
    other.load_state_dict(sd)
    a, b = dec.push(xn[:, 18:]), other.push(xn[:, 18:].copy())
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and torch.equal(dec.state, other.state)
    assert [e for e, _ in dec.latest()] == [40] * 3 and [e for e, _ in other.latest()] == [40] * 3
    with pytest.raises(nsd.NsdError, match="window"):
        nsd.SlidingStreamDecoder(model, streams=3, window=12, hop=6).load_state_dict(sd)
    with pytest.raises(nsd.NsdError):
        nsd.SlidingStreamDecoder(model, streams=2, window=12, hop=4).load_state_dict(sd)
    dec.reset([1])
    assert list(dec.steps) == [T41, 0, T41] and dec.latest()[1] is None and dec.latest()[0][0] == 40
    for W, Hp in ((12, 5), (4, 12), (0, 0), (12, 0), (129, 1)):
        with pytest.raises(nsd.NsdError, match="nsd_window_path"):
            nsd.SlidingStreamDecoder(model, window=W, hop=Hp)
    with pytest.raises(nsd.NsdError, match="z-score"):
        nsd.SlidingStreamDecoder(tgs._eval_model(nsd, dev, ref_state, normalize=True), window=12, hop=4)
    with pytest.raises(nsd.NsdError, match="eval"):
        nsd.SlidingStreamDecoder(tgs._eval_model(nsd, dev, ref_state).train(), window=12, hop=4)
    with pytest.raises(nsd.NsdError, match="nsd_stream_path"):
        nsd.SlidingStreamDecoder(nsd.EEG_LSTM(hidden_size=32).to(dev).eval(), window=12, hop=4)
    with pytest.raises(nsd.NsdError, match="bf16"):
        nsd.SlidingStreamDecoder(nsd.EEG_LSTM(hidden_size=64, precision="bf16").to(dev).eval(), window=12, hop=4)
    with pytest.raises(nsd.NsdError):
        dec.push(xn[:, :2], slots=[0, 0, 1])


def test_open_stream_and_run_trials_with_a_hop(nsd, dev, golden, ref_state, tmp_path, capsys):
    """(run_trials starts the replay producer, a process of its own: once here; its start is most of this test's time)"""
    g = golden("real_trials")
    pth = write_pth(str(tmp_path), ref_state)
    names = ["Food", "Water", "None"]
    pred = nsd.SimplePredictor(pth, sr=125, device="cpu", class_names=names, preprocess="identity")
    assert type(pred.open_stream()).__name__ == "PredictorStream"          # without the new arguments: today's object
    with pytest.raises(ValueError):
        pred.open_stream(window_seconds=1.0)
    st = pred.open_stream(streams=2, window_seconds=2.0, hop_seconds=1.0)   # W = 250, hop = 125
    w = np.stack([g["x"][0], g["x"][1]])
    one = nsd.StreamDecoder(tgs._eval_model(nsd, dev, ref_state), streams=2)
    found = [[], []]
    for t0 in range(0, 625, 25):
        res = st.push(w[:, t0:t0 + 25])
        assert len(res) == 2
        for b in range(2):
            found[b] += res[b]
    assert [[e for e, _, _ in f] for f in found] == [[250, 375, 500, 625]] * 2 and list(st.steps) == [625, 625]
    for i, e in enumerate([250, 375, 500, 625]):
        one.reset()
        want = one.push(w[:, e - 250:e]).cpu().numpy()
        for b in range(2):
            _, probs, label = found[b][i]
            assert probs.dtype == np.float32 and probs.tobytes() == want[b].tobytes() and label == names[int(want[b].argmax())]

    # run_trials on the replay source: the 5 s windows of the producer as one continuous stream, a decision every second from 5 s on
    dd = tmp_path / "trials"
    dd.mkdir()
    for i in range(4):
        np.savetxt(dd / f"food_{i:02d}.csv", g["x"][i], fmt="%.7f", delimiter=",")
    kw = dict(serial_port=f"replay:{dd}", model_path=pth, verbose=True, queue_timeout=20.0, predictor_kwargs={"preprocess": "identity"})

    def run(**extra):
        capsys.readouterr()
        res = nsd.run_trials(**kw, **extra)
        return res, capsys.readouterr().out

    # (run_trials without hop_seconds is today's path, line for line: tests/test_gpu_stream.py and tests/test_gpu_parity.py hold it)
    hop, out_hop = run(trials=8, chunk_seconds=0.2, hop_seconds=1.0)
    assert not re.findall(r"^\[Trial ", out_hop, re.M)
    lines = re.findall(r"^\[Window end=(\d+) @ [^\]]*\] pred=(\S+) probs=", out_hop, re.M)
    assert [int(e) for e, _ in lines] == list(range(625, 1501, 125)) and hop.trials == 8      # one decision per hop
    whole, want = np.concatenate([g["x"][i] for i in range(4)]), []         # the files in order: one stream of 2500 samples
    for e in range(625, 1501, 125):
        one.reset()
        want.append(one.push(whole[e - 625:e]).cpu().numpy()[0])
    for (_, label), p in zip(lines, want):                                  # the label wherever the decision is clear
        top = np.sort(p)
        if top[-1] - top[-2] > 1e-3:
            assert label == names[int(p.argmax())]
    assert hop.avg_chunk.shape == (625, 8) and np.abs(hop.avg_probs - np.mean(want, 0)).max() < PROB_TOL     # (the CSV keeps 7 decimals)
    assert np.abs(hop.avg_chunk - np.mean([whole[e - 625:e] for e in range(625, 1501, 125)], 0)).max() < 1e-5
    with pytest.raises(ValueError):
        nsd.run_trials(trials=1, hop_seconds=1.0, **kw)
