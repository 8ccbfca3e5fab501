"""Sliding-window decisions from an ensemble (nsd_multi_window_* of include/nsd.h, csrc/nsd_multi_window48.hip).  Needs the MI355X.

The contract is one of BITS: model m's part of the state after a call, and its blocks of logits / probs / ends / counts -- the NaN / -1
rows from counts[m,b] on included -- are what nsd_window_step leaves and writes for that model alone, for any M, B, cut of the stream,
slot, placement in the grid, HIP stream or graph replay.  So the reference of every test here is nsd_window_step itself
(tests/test_gpu_window.py holds that one to nsd_stream_step and the oracle), run beside the call under test on states of its own.  The
mean is the serial fp32 mean of tests/multi_stream_ref.py on the rows every member completed, and NaN (isnan, whatever the payload) on
every other row.  Which windows a call completes, their rows and ends come from the integer schedule of tests/window_ref.py.  Outputs
are pre-filled with 0xFF bytes, states with NaN.  Unless said otherwise T = 41, B = 3, M = 3, with the parameter sets and variants of
tests/test_gpu_multi_stream.py.  Each case takes milliseconds.
"""
import contextlib
import re

import numpy as np
import pytest
import torch

from oracle import nsd_oracle as orc
from tests import multi_stream_ref as mr
from tests import stream_ref as sr
from tests import test_gpu_multi_stream as tms
from tests import test_gpu_window as tgw
from tests import window_ref as wr
from tests.buffer_contract import guarded, snapshot
from tests.golden.make_goldens import synth_x
from tests.gpu_harness import NAN, PROB_TOL, D, cus, dev, nsd, spec_of, sync_at_the_end, to_dev, write_pth  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

T41, B41, M3 = tms.T41, tms.B41, tms.M3
WINDOWS_41 = tgw.WINDOWS_41
VARIANTS = tms.VARIANTS


# ---------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------
def _stride(spec, W, Hp):
    from nsd_amd import ops
    return int(ops.window_layout(spec, W, Hp).stream_stride)


def _new_multi(dev, spec, W, Hp, M, S):
    """[M,S,stream_stride], NaN-filled, then reset as the flat state of M*S streams"""
    from nsd_amd import ops
    state = torch.full((M, S, _stride(spec, W, Hp)), NAN, device=dev)
    ops.window_reset(spec, W, Hp, state.view(M * S, -1))
    return state


def _new_singles(dev, spec, W, Hp, M, S):
    return [tgw._new_state(dev, spec, W, Hp, S) for _ in range(M)]


def _outs(dev, M, B, Dr, K):
    """output buffers of one call, every byte 0xFF: logits, probs, mean, ends, counts"""
    f = lambda *s: torch.full(s, -1, dtype=torch.int32, device=dev).view(torch.float32)
    return (f(M, B, Dr, K), f(M, B, Dr, K), f(B, Dr, K), torch.full((M, B, Dr), -7, dtype=torch.int64, device=dev),
            torch.full((M, B), -7, dtype=torch.int32, device=dev))


def _mstep(dev, spec, params, x, state, W, Hp, *, slots=None, residual=False):
    """one nsd_multi_window_step into 0xFF-filled outputs -> numpy logits [M,B,D,K], probs, mean [B,D,K], ends [M,B,D], counts [M,B]"""
    from nsd_amd import ops
    M, B, T = int(params.shape[0]), int(x.shape[-3]), int(x.shape[-2])
    out = _outs(dev, M, B, wr.rows(T, Hp), spec.K)
    got = ops.multi_window_step(spec, params, x.contiguous(), state, window=W, hop=Hp, slots=slots, residual=residual, out=out)
    assert all(g is o for g, o in zip(got, out))
    return tuple(t.cpu().numpy() for t in out)


def _singles(dev, spec, params, x, states, W, Hp, *, slots=None, residual=False):
    """the M independent nsd_window_step calls of the same chunk (x [B,n,C] shared or [M,B,n,C]) -> stacked numpy logits, probs, ends,
    counts"""
    outs = []
    for m in range(int(params.shape[0])):
        xm = x[m] if x.dim() == 4 else x
        outs.append(tgw._wstep(dev, spec, params[m], xm, states[m], W, Hp, slots=slots, residual=residual))
    return tuple(np.stack([o[i] for o in outs]) for i in range(4))


def _bytes(state):
    return (torch.stack(list(state)) if isinstance(state, (list, tuple)) else state).cpu().numpy().tobytes()


def _mean_ok(mean, probs, what):
    """the serial fp32 mean, bit for bit, on the rows every member completed; NaN on every other row -> the completed rows [B,D]"""
    with np.errstate(invalid="ignore"):
        want = mr.mean_probs(probs)
    done = ~np.isnan(probs).any(axis=(0, 3))
    assert mean[done].tobytes() == want[done].tobytes(), (what, "mean")
    assert np.isnan(mean[~done]).all(), (what, "mean of rows that are not decisions")
    return done


def _same(multi_out, single_out, what):
    (lg, pr, mean, ends, counts), (slg, spr, sends, scounts) = multi_out, single_out
    assert lg.tobytes() == slg.tobytes(), (what, "logits")
    assert pr.tobytes() == spr.tobytes(), (what, "probs")
    assert ends.tobytes() == sends.tobytes() and ends.dtype == np.int64, (what, "ends")
    assert counts.tobytes() == scounts.tobytes() and counts.dtype == np.int32, (what, "counts")
    return _mean_ok(mean, spr, what)


def _schedule_ok(out, n0, n, W, Hp, what):
    """rows, ends and counts of a call on streams that have seen n0 samples, by tests/window_ref.py, in every member"""
    lg, pr, mean, ends, counts = out
    M, B = counts.shape
    exp = wr.completed(n0, n, W, Hp)
    assert lg.shape == (M, B, wr.rows(n, Hp), lg.shape[-1]) and (counts == len(exp)).all(), (what, counts)
    for k, e, row in exp:
        assert (ends[:, :, row] == e).all(), (what, k, e, row)
    first = len(exp)
    assert not np.isnan(lg[:, :, :first]).any() and not np.isnan(pr[:, :, :first]).any() and not np.isnan(mean[:, :first]).any(), what
    assert np.isnan(lg[:, :, first:]).all() and np.isnan(pr[:, :, first:]).all() and (ends[:, :, first:] == -1).all(), what
    assert np.isnan(mean[:, first:]).all(), what
    return exp


def _run_both(dev, spec, params, x, cut, state, singles, W, Hp, *, slots=None, residual=False, what=()):
    """push x in the chunks of `cut` through the call under test and through M nsd_window_step calls, compare every call's outputs and
    the state after it -> {k: (logits [M,B,K], probs [M,B,K], mean [B,K])} of the completed windows"""
    got, t = {}, 0
    for n in cut:
        chunk = x[..., t:t + n, :]
        out = _mstep(dev, spec, params, chunk, state, W, Hp, slots=slots, residual=residual)
        _same(out, _singles(dev, spec, params, chunk, singles, W, Hp, slots=slots, residual=residual), what + (t, n))
        assert _bytes(state) == _bytes(singles), what + (t, n, "state")
        for k, e, row in _schedule_ok(out, t, n, W, Hp, what + (t, n)):
            assert k not in got
            got[k] = (out[0][:, :, row].copy(), out[1][:, :, row].copy(), out[2][:, row].copy())
        t += n
    return got


_whole = {}


def _whole_singles(dev, name, ref_state, W, Hp):
    """the M single-model 41-step calls of a variant: ({k: (logits [M,B,K], probs [M,B,K])}, final state bytes), computed once"""
    key = (name, W, Hp)
    if key not in _whole:
        d, residual, pn, xn = tms._case(name, ref_state)
        spec, params, x = spec_of(d), to_dev(pn, dev), to_dev(xn, dev)
        states = _new_singles(dev, spec, W, Hp, M3, B41)
        per = [tgw._run(dev, spec, params[m], x, [T41], states[m], W, Hp, residual=residual) for m in range(M3)]
        wins = {k: (np.stack([per[m][k][0] for m in range(M3)]), np.stack([per[m][k][1] for m in range(M3)])) for k in per[0]}
        _whole[key] = (wins, _bytes(states))
    return _whole[key]


# ---------------------------------------------------------------------------------------------------
# 1. bitwise against the single-model call, for every cut, window and variant
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", sr.CUTS_41, ids=["ones", "fib", "40+1", "whole"])
@pytest.mark.parametrize("W,Hp", WINDOWS_41)
@pytest.mark.parametrize("name", list(VARIANTS))
def test_every_call_leaves_the_bits_of_the_single_model_calls(nsd, dev, ref_state, name, W, Hp, cut):
    from nsd_amd import ops
    d, residual, pn, xn = tms._case(name, ref_state)
    spec, params, x = spec_of(d), to_dev(pn, dev), to_dev(xn, dev)
    state = _new_multi(dev, spec, W, Hp, M3, B41)
    assert _bytes(state) == _bytes(ops.multi_window_state(spec, W, Hp, M3, B41, dev))
    assert state.numel() * 4 == M3 * B41 * _stride(spec, W, Hp) * 4
    singles = _new_singles(dev, spec, W, Hp, M3, B41)
    got = _run_both(dev, spec, params, x, cut, state, singles, W, Hp, residual=residual, what=(name, W, Hp))
    assert sorted(got) == list(range((T41 - W) // Hp + 1)), sorted(got)
    wins, sb = _whole_singles(dev, name, ref_state, W, Hp)                 # ... and the cut does not show
    assert _bytes(state) == sb
    for k, (lg, pr, mean) in got.items():
        assert lg.tobytes() == wins[k][0].tobytes() and pr.tobytes() == wins[k][1].tobytes(), (name, W, Hp, cut, "window", k)
        assert mean.tobytes() == mr.mean_probs(wins[k][1]).tobytes(), (name, W, Hp, cut, "mean of window", k)


# ---------------------------------------------------------------------------------------------------
# 2. a segment that begins off the 32-sample staging grid
# ---------------------------------------------------------------------------------------------------
def test_segments_that_begin_off_the_staging_grid(nsd, dev, ref_state):
    W, Hp = 36, 12
    d, residual, pn, xn = tms._case("ref", ref_state)
    spec, params, x = spec_of(d), to_dev(pn, dev), to_dev(xn, dev)
    ends = []
    for cut in ([41], [5, 36]):
        state, singles = _new_multi(dev, spec, W, Hp, M3, B41), _new_singles(dev, spec, W, Hp, M3, B41)
        got = _run_both(dev, spec, params, x, cut, state, singles, W, Hp, what=(W, Hp, tuple(cut)))
        assert sorted(got) == [0], cut                                     # [0, 36): phases 1 and 2 stop inside their first window
        ends.append((got[0][0].tobytes(), got[0][1].tobytes(), got[0][2].tobytes(), _bytes(state)))
    assert ends[0] == ends[1]
    assert [p for _, p in wr.phases(T41, W, Hp)] == [5, 29, 17] and wr.phases(5, W, Hp)[1] == (None, 0)   # phase 1 starts at sample 7 of the chunk


# ---------------------------------------------------------------------------------------------------
# 3. M = 1
# ---------------------------------------------------------------------------------------------------
def test_one_model_is_the_single_model_call_and_the_state_is_interchangeable(nsd, dev, ref_state):
    W, Hp = 12, 4
    d, _, pn, xn = tms._case("ref", ref_state)
    spec, params, x = spec_of(d), to_dev(pn[:1], dev), to_dev(xn, dev)
    a, b = x[:, :13], x[:, 13:]
    single = _new_singles(dev, spec, W, Hp, 1, B41)
    _singles(dev, spec, params, a, single, W, Hp)
    want = _singles(dev, spec, params, b, single, W, Hp)
    multi = _new_multi(dev, spec, W, Hp, 1, B41)
    _mstep(dev, spec, params, a, multi, W, Hp)
    got = _mstep(dev, spec, params, b, multi, W, Hp)
    done = _same(got, want, "M = 1")
    assert done.sum() == B41 * len(wr.completed(13, 28, W, Hp)) > 0
    assert got[2][done].tobytes() == got[1][0][done].tobytes()              # the mean of one model is that model: p / 1.0f
    assert _bytes(multi) == _bytes(single)
    # advance with one entry, continue with the other
    s1 = _new_singles(dev, spec, W, Hp, 1, B41)
    _singles(dev, spec, params, a, s1, W, Hp)
    _same(_mstep(dev, spec, params, b, s1[0][None], W, Hp), want, "single then multi")
    assert _bytes(s1) == _bytes(single)
    m1 = _new_multi(dev, spec, W, Hp, 1, B41)
    _mstep(dev, spec, params, a, m1, W, Hp)
    again = _singles(dev, spec, params, b, [m1[0]], W, Hp)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(again, want)) and _bytes(m1) == _bytes(single)


# ---------------------------------------------------------------------------------------------------
# 4. a chunk per model
# ---------------------------------------------------------------------------------------------------
def test_per_model_chunks_give_each_member_its_own_single_run(nsd, dev, ref_state):
    import ctypes
    from nsd_amd import _lib, ops
    W, Hp, T = 12, 4, 17
    d, _, pn, _ = tms._case("ref", ref_state)
    spec, params = spec_of(d), to_dev(pn, dev)
    xs = to_dev(np.stack([synth_x(B41, 2 * T, C=d.C, seed=4300 + m) for m in range(M3)]), dev)      # [M,B,34,C], different data per model
    state, singles = _new_multi(dev, spec, W, Hp, M3, B41), _new_singles(dev, spec, W, Hp, M3, B41)
    got = _run_both(dev, spec, params, xs, [T, T], state, singles, W, Hp, what=("x [M,B,n,C]",))       # x_model_stride = B*T*C
    assert sorted(got) == list(range((2 * T - W) // Hp + 1))
    assert got[0][1][0].tobytes() != got[0][1][1].tobytes()                                         # (the members do differ)
    # ... and a stride above B*T*C, through the C ABI
    n, pad = B41 * T * d.C, 24
    buf = torch.full((M3, n + pad), NAN, device=dev)
    buf[:, :n] = xs[:, :, :T].reshape(M3, n)
    strided, ones = _new_multi(dev, spec, W, Hp, M3, B41), _new_singles(dev, spec, W, Hp, M3, B41)
    out = _outs(dev, M3, B41, wr.rows(T, Hp), spec.K)
    dims, w = spec.dims(B41, T), _lib.Window(W, Hp)
    ops._call("nsd_multi_window_step", dev, ctypes.byref(dims), ctypes.byref(w), M3, params.data_ptr(), buf.data_ptr(), n + pad, None, 0,
              strided.data_ptr(), strided.numel() * 4, B41, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(),
              out[4].data_ptr(), ops.STREAM)
    _same(tuple(o.cpu().numpy() for o in out), _singles(dev, spec, params, xs[:, :, :T].contiguous(), ones, W, Hp), "stride above B*T*C")
    assert _bytes(strided) == _bytes(ones)


# ---------------------------------------------------------------------------------------------------
# 5. slot and batch invariance
# ---------------------------------------------------------------------------------------------------
def test_slot_and_batch_invariance(nsd, dev, ref_state):
    """B = 3 in streams [5, 0, 2] of S = 6, shared by the models: the outputs of the plain run, the states moved; a stream alone gives
    its rows of the call; the streams not named keep the bytes of the reset."""
    W, Hp, S, cut = 12, 4, 6, [7, 9, 25]
    d, _, pn, xn = tms._case("ref", ref_state)
    spec, params, x = spec_of(d), to_dev(pn, dev), to_dev(xn, dev)
    plain, ps = _new_multi(dev, spec, W, Hp, M3, S), _new_singles(dev, spec, W, Hp, M3, S)
    reset = plain.cpu().numpy().copy()
    want = _run_both(dev, spec, params, x, cut, plain, ps, W, Hp, what=("plain",))
    perm = torch.tensor([5, 0, 2], dtype=torch.int32, device=dev)
    moved, ms = _new_multi(dev, spec, W, Hp, M3, S), _new_singles(dev, spec, W, Hp, M3, S)
    got = _run_both(dev, spec, params, x, cut, moved, ms, W, Hp, slots=perm, what=("permuted",))
    assert sorted(got) == sorted(want) and all(all(u.tobytes() == v.tobytes() for u, v in zip(got[k], want[k])) for k in want)
    mv, pl = moved.cpu().numpy(), plain.cpu().numpy()
    for m in range(M3):
        for b, s in enumerate((5, 0, 2)):
            assert mv[m, s].tobytes() == pl[m, b].tobytes(), (m, b)
        for s in (1, 3, 4):
            assert mv[m, s].tobytes() == reset[m, s].tobytes(), (m, s)
        for s in range(3, S):
            assert pl[m, s].tobytes() == reset[m, s].tobytes(), (m, s)
    # stream 1 alone in stream 0 of the state
    lone, ls = _new_multi(dev, spec, W, Hp, M3, S), _new_singles(dev, spec, W, Hp, M3, S)
    one = _run_both(dev, spec, params, x[1:2], cut, lone, ls, W, Hp, slots=perm[1:2].contiguous(), what=("alone",))
    for k in want:
        assert one[k][0].tobytes() == want[k][0][:, 1:2].tobytes() and one[k][1].tobytes() == want[k][1][:, 1:2].tobytes(), k
        assert one[k][2].tobytes() == want[k][2][1:2].tobytes(), k
    assert _bytes(lone[:, 0]) == _bytes(plain[:, 1])


# ---------------------------------------------------------------------------------------------------
# 6. more (stream, phase) pairs per model than its workgroups
# ---------------------------------------------------------------------------------------------------
def test_more_pairs_per_model_than_its_workgroups(nsd, dev, cus, ref_state):
    """G = max(1, CUs / M) workgroups per model and B * R just above it: some workgroups of every model walk a second pair; the second
    call loads every pair's state."""
    W, Hp, T = 12, 1, 13
    R = W // Hp
    per = max(1, cus // M3)
    B = per // R + 1
    assert B * R > per
    spec = spec_of(D)
    pn = np.stack([orc.flatten_state(st, D) for st in tms._states(D, ref_state)])
    params, x = to_dev(pn, dev), to_dev(synth_x(B, 2 * T, seed=1713), dev)
    state, singles = _new_multi(dev, spec, W, Hp, M3, B), _new_singles(dev, spec, W, Hp, M3, B)
    got = _run_both(dev, spec, params, x, [T, T], state, singles, W, Hp, what=("B", B))
    assert sorted(got) == list(range(2 * T - W + 1))


# ---------------------------------------------------------------------------------------------------
# 7. skips: another (window, hop) in one model's header, a slot outside the state
# ---------------------------------------------------------------------------------------------------
def test_a_member_with_another_window_is_skipped_alone_and_a_bad_slot_in_every_member(nsd, dev, ref_state):
    from nsd_amd import ops
    W, Hp, S = 12, 4, 4
    d, _, pn, xn = tms._case("ref", ref_state)
    spec, params, x = spec_of(d), to_dev(pn, dev), to_dev(xn[:, :17], dev)
    clean = _new_multi(dev, spec, W, Hp, M3, S)
    lc, pc, mc, ec, cc = _mstep(dev, spec, params, x, clean, W, Hp)
    assert (cc == 2).all()
    state, check = guarded((M3, S, _stride(spec, W, Hp)), torch.float32, dev, "nan32")
    ops.window_reset(spec, W, Hp, state.view(M3 * S, -1))
    check("state after reset")
    # stream 1 of model 1 alone records (24, 8): the same R, so the header stands where this call looks for it
    ops.window_reset(spec, 24, 8, state[1], torch.tensor([1], dtype=torch.int32, device=dev))
    check("state after the reset of one stream of one model")
    before = state.cpu().numpy().copy()
    lg, pr, mean, ends, counts = _mstep(dev, spec, params, x, state, W, Hp)
    check("state")
    assert counts[1, 1] == -1 and np.isnan(lg[1, 1]).all() and np.isnan(pr[1, 1]).all() and (ends[1, 1] == -1).all()
    assert np.isnan(mean[1]).all()                                       # the stream's mean: one member has no decision
    now, ok = state.cpu().numpy(), clean.cpu().numpy()
    assert now[1, 1].tobytes() == before[1, 1].tobytes()                 # untouched
    keep = np.ones((M3, B41), bool)
    keep[1, 1] = False
    for a, c in ((lg, lc), (pr, pc), (ends, ec), (counts, cc)):          # every other (member, stream): the clean run's bits
        assert a[keep].tobytes() == c[keep].tobytes()
    assert mean[[0, 2]].tobytes() == mc[[0, 2]].tobytes()
    for m in range(M3):
        for s in range(S):
            if (m, s) != (1, 1):
                assert now[m, s].tobytes() == ok[m, s].tobytes(), (m, s)
    # the whole part of model 1 reset with (24, 8): that member skipped, every mean row NaN, the others clean
    ops.window_reset(spec, W, Hp, state.view(M3 * S, -1))
    ops.window_reset(spec, 24, 8, state[1])
    before = state.cpu().numpy().copy()
    lg, pr, mean, ends, counts = _mstep(dev, spec, params, x, state, W, Hp)
    check("state, one member's part reset with another window")
    assert (counts[1] == -1).all() and np.isnan(lg[1]).all() and np.isnan(pr[1]).all() and (ends[1] == -1).all() and np.isnan(mean).all()
    assert state.cpu().numpy()[1].tobytes() == before[1].tobytes()
    for a, c in ((lg, lc), (pr, pc), (ends, ec), (counts, cc)):
        assert a[[0, 2]].tobytes() == c[[0, 2]].tobytes()
    assert _bytes(state[[0, 2]]) == _bytes(clean[[0, 2]])
    # a slot outside [0, S): skipped in every member
    good = _new_multi(dev, spec, W, Hp, M3, S)
    gl, gp, gm, ge, gc = _mstep(dev, spec, params, x, good, W, Hp, slots=torch.tensor([2, 1, 0], dtype=torch.int32, device=dev))
    ops.window_reset(spec, W, Hp, state.view(M3 * S, -1))
    before = state.cpu().numpy().copy()
    for bad in (S, -1, M3 * S):
        state.copy_(torch.from_numpy(before).to(dev))
        lg, pr, mean, ends, counts = _mstep(dev, spec, params, x, state, W, Hp, slots=torch.tensor([2, bad, 0], dtype=torch.int32, device=dev))
        check("state, bad slot")
        assert (counts[:, 1] == -1).all() and np.isnan(lg[:, 1]).all() and np.isnan(pr[:, 1]).all() and (ends[:, 1] == -1).all(), bad
        assert np.isnan(mean[1]).all(), bad
        for a, g in ((lg, gl), (pr, gp), (ends, ge), (counts, gc)):
            assert a[:, [0, 2]].tobytes() == g[:, [0, 2]].tobytes(), bad
        assert mean[[0, 2]].tobytes() == gm[[0, 2]].tobytes(), bad
        now, ok = state.cpu().numpy(), good.cpu().numpy()
        assert now[:, [1, 3]].tobytes() == before[:, [1, 3]].tobytes() and now[:, [0, 2]].tobytes() == ok[:, [0, 2]].tobytes(), bad


# ---------------------------------------------------------------------------------------------------
# 8. a sample that is not finite poisons exactly the windows that contain it, in every member and in the mean
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", [[T41], [9, 32], [1] * T41], ids=["whole", "9+32", "ones"])
def test_nan_containment(nsd, dev, ref_state, cut):
    W, Hp = 12, 4
    d, _, pn, xn = tms._case("ref", ref_state)
    spec, params = spec_of(d), to_dev(pn, dev)
    wins, sb = _whole_singles(dev, "ref", ref_state, W, Hp)
    for poison in (np.nan, -np.inf):
        xb = xn.copy()
        xb[1, 17, 2] = poison
        x = to_dev(xb, dev)
        dirty, got, t = _new_multi(dev, spec, W, Hp, M3, B41), {}, 0
        for n in cut:
            lg, pr, mean, ends, counts = _mstep(dev, spec, params, x[:, t:t + n], dirty, W, Hp)
            exp = wr.completed(t, n, W, Hp)
            assert (counts == len(exp)).all()
            for k, e, row in exp:
                assert (ends[:, :, row] == e).all()
                got[k] = (lg[:, :, row].copy(), pr[:, :, row].copy(), mean[:, row].copy())
            assert np.isnan(mean[:, len(exp):]).all()
            t += n
        assert sorted(got) == list(range(8))
        for k, (lg, pr, mean) in got.items():
            rl, rp = wins[k]
            rm = mr.mean_probs(rp)
            hit = k in (2, 3, 4)                                        # [8, 20), [12, 24), [16, 28) hold sample 17
            assert hit == (k * Hp <= 17 < k * Hp + W)
            if hit:
                assert np.isnan(lg[:, 1]).all() and np.isnan(pr[:, 1]).all() and np.isnan(mean[1]).all(), k
                assert lg[:, [0, 2]].tobytes() == rl[:, [0, 2]].tobytes() and pr[:, [0, 2]].tobytes() == rp[:, [0, 2]].tobytes(), k
                assert mean[[0, 2]].tobytes() == rm[[0, 2]].tobytes(), k
            else:                                                       # including windows 5 .. 7, completed after it has left
                assert lg.tobytes() == rl.tobytes() and pr.tobytes() == rp.tobytes() and mean.tobytes() == rm.tobytes(), k
        assert _bytes(dirty) == sb                                      # the stream has healed: its state is the clean run's


# ---------------------------------------------------------------------------------------------------
# 9. side stream, graph replay: prep_step + multi_window_step (step and mean launches) on one stream
# ---------------------------------------------------------------------------------------------------
def test_side_stream_and_prep_plus_step_replayed_as_one_graph(nsd, dev, ref_state):
    from nsd_amd import ops
    W, Hp = 12, 4
    d, _, pn, xn = tms._case("ref", ref_state)
    spec, params, x = spec_of(d), to_dev(pn, dev), to_dev(xn, dev)
    wins, sb = _whole_singles(dev, "ref", ref_state, W, Hp)
    side = torch.cuda.Stream(device=dev)
    state = _new_multi(dev, spec, W, Hp, M3, B41)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        a = _mstep(dev, spec, params, x[:, :20], state, W, Hp)
        b = _mstep(dev, spec, params, x[:, 20:], state, W, Hp)
    side.synchronize()
    for out, t, n in ((a, 0, 20), (b, 20, 21)):
        for k, e, row in _schedule_ok(out, t, n, W, Hp, ("side stream", t)):
            assert out[0][:, :, row].tobytes() == wins[k][0].tobytes() and out[1][:, :, row].tobytes() == wins[k][1].tobytes(), k
            assert out[2][:, row].tobytes() == mr.mean_probs(wins[k][1]).tobytes(), k
    assert _bytes(state) == sb

    # nsd_prep_step + nsd_multi_window_step captured once (a chain: no parallel branches), replayed over five chunks of 8 samples
    P = nsd.CausalPrep.design(highpass=1.0, lowpass=40.0, zscore_seconds=0.4, var0=250.0)
    raw = to_dev((xn * 20.0 + 300.0).astype(np.float32), dev)
    n, chunks = 8, 5
    eager = []
    ps, ws = ops.prep_state(spec.C, B41, dev), _new_multi(dev, spec, W, Hp, M3, B41)
    for i in range(chunks):
        y = ops.prep_step(raw[:, i * n:(i + 1) * n].contiguous(), P, ps)
        eager.append(_mstep(dev, spec, params, y, ws, W, Hp))
    xin, y = torch.empty((B41, n, spec.C), device=dev), torch.empty((B41, n, spec.C), device=dev)
    gps, gws = ops.prep_state(spec.C, B41, dev), _new_multi(dev, spec, W, Hp, M3, B41)
    out = _outs(dev, M3, B41, wr.rows(n, Hp), spec.K)
    xin.copy_(raw[:, :n])
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.prep_step(xin, P, gps, out=y)
        ops.multi_window_step(spec, params, y, gws, window=W, hop=Hp, out=out)
    ops.prep_reset(spec.C, gps)                                        # (whatever the capture did or did not run)
    ops.window_reset(spec, W, Hp, gws.view(M3 * B41, -1))
    for i in range(chunks):
        xin.copy_(raw[:, i * n:(i + 1) * n])
        for o in out:
            o.view(torch.uint8).fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize(dev)
        got = tuple(o.cpu().numpy() for o in out)
        for j, (g, e) in enumerate(zip(got, eager[i])):
            if j == 2:                                                  # the mean: bits on decisions, NaN (any payload) elsewhere
                done = ~np.isnan(e).any(-1)
                assert g[done].tobytes() == e[done].tobytes() and np.isnan(g[~done]).all(), i
            else:
                assert g.tobytes() == e.tobytes(), (i, j)
        _schedule_ok(got, i * n, n, W, Hp, ("graph", i))
    assert _bytes(gws) == _bytes(ws) and gps.cpu().numpy().tobytes() == ps.cpu().numpy().tobytes()
    assert sum(len(wr.completed(i * n, n, W, Hp)) for i in range(chunks)) == 8


# ---------------------------------------------------------------------------------------------------
# 10. buffer contract
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", ["ones", "nan32"])
def test_buffer_contract(nsd, dev, ref_state, fill):
    from nsd_amd import _lib, ops
    import ctypes
    W, Hp, S, T = 12, 4, B41, 17
    d, _, pn, xn = tms._case("c3", ref_state)
    spec, params, x = spec_of(d), to_dev(pn, dev), to_dev(xn[:, :T], dev).contiguous()
    Dr, K = wr.rows(T, Hp), spec.K
    dims, w = spec.dims(1, 1), _lib.Window(W, Hp)
    nbytes = int(_lib.lib().nsd_multi_window_state_bytes(ctypes.byref(dims), ctypes.byref(w), M3, S))
    state, cs = guarded((M3, S, _stride(spec, W, Hp)), torch.float32, dev, fill)
    assert state.numel() * 4 == nbytes
    bufs = [guarded((M3, B41, Dr, K), torch.float32, dev, fill), guarded((M3, B41, Dr, K), torch.float32, dev, fill),
            guarded((B41, Dr, K), torch.float32, dev, fill), guarded((M3, B41, Dr), torch.int64, dev, fill),
            guarded((M3, B41), torch.int32, dev, fill)]
    names = ("logits", "probs", "mean_probs", "ends", "counts")
    ops.window_reset(spec, W, Hp, state.view(M3 * S, -1))
    cs("state after nsd_window_reset of the flat state")
    assert _bytes(state) == _bytes(_new_multi(dev, spec, W, Hp, M3, S))             # nothing of the fill is left
    snap = snapshot(params, x)
    out = tuple(b[0] for b in bufs)
    ops.multi_window_step(spec, params, x, state, window=W, hop=Hp, out=out)
    torch.cuda.synchronize(dev)
    cs("state after nsd_multi_window_step")
    for (_, check), what in zip(bufs, names):
        check(what)
    assert snap.unchanged()
    ref = _new_multi(dev, spec, W, Hp, M3, S)
    want = _mstep(dev, spec, params, x, ref, W, Hp)
    for o, v, what in zip(out, want, names):                            # no byte of the fill shows in an output
        if what == "mean_probs":
            done = ~np.isnan(v).any(-1)
            assert o.cpu().numpy()[done].tobytes() == v[done].tobytes() and torch.isnan(o).cpu().numpy()[~done].all()
        else:
            assert o.cpu().numpy().tobytes() == v.tobytes(), what
    assert _bytes(state) == _bytes(ref)
    # mean_probs == NULL: no second launch, nothing is written to the mean buffer of the call before; probs == NULL too
    out[2].view(torch.uint8).fill_(0x5A)
    got = ops.multi_window_step(spec, params, x, state, window=W, hop=Hp, want_mean=False, out=out[:2] + (None,) + out[3:])
    torch.cuda.synchronize(dev)
    assert got[2] is None and (out[2].view(torch.uint8) == 0x5A).all() and snap.unchanged()
    for (_, check), what in zip(bufs, names):
        check(what + " (no mean)")
    cs("state (no mean)")


# ---------------------------------------------------------------------------------------------------
# 11. EnsembleSlidingStreamDecoder
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_prep", [False, True], ids=["plain", "prep"])
def test_ensemble_sliding_decoder_equals_single_decoders_per_member(nsd, dev, ref_state, with_prep):
    from nsd_amd import ops
    from nsd_amd.multimodel import _EnsembleModel
    W, Hp = 12, 4
    _, _, _, xn = tms._case("ref", ref_state)
    raw = (xn * 20.0 + 300.0).astype(np.float32) if with_prep else xn
    P = nsd.CausalPrep.design(highpass=1.0, lowpass=40.0, zscore_seconds=0.4, var0=250.0) if with_prep else None
    kw = dict(prep=P) if with_prep else {}
    members = tms._members(nsd, dev, ref_state, **kw)
    ens = _EnsembleModel(members)
    dec = nsd.EnsembleSlidingStreamDecoder(ens, streams=4, window=W, hop=Hp)
    assert dec.params is ens.params and dec.member_probs is None           # the ensemble's own stacked buffer, not a copy
    assert dec.latest() == [None] * 4 and tuple(dec.state.shape) == (M3, 4, _stride(members[0].spec, W, Hp))
    ones = [nsd.SlidingStreamDecoder(m, streams=4, window=W, hop=Hp) for m in members]
    names = []

    @contextlib.contextmanager
    def hook(name):
        names.append(name)
        yield
    t, last = 0, None
    for n in (7, 9, 25):
        ops.set_launch_hook(hook)
        try:
            mean, ends, counts = dec.push(raw[:, t:t + n])
        finally:
            ops.set_launch_hook(None)
        assert names == (["nsd_prep_step"] if with_prep else []) + ["nsd_multi_window_step"], names      # one front end, one step call
        names.clear()
        assert mean.is_cuda and tuple(mean.shape) == (B41, wr.rows(n, Hp), 3) and ends.dtype == torch.int64 and counts.dtype == torch.int32
        assert tuple(dec.member_probs.shape) == (M3, B41, wr.rows(n, Hp), 3)
        each = []
        for o in ones:                                                   # (the single decoders share window_step's buffers: copy)
            p, e, c = o.push(raw[:, t:t + n])
            each.append((p.clone(), e.clone(), c.clone()))
        probs = torch.stack([p for p, _, _ in each])
        assert dec.member_probs.cpu().numpy().tobytes() == probs.cpu().numpy().tobytes(), t
        assert torch.equal(ends, each[0][1]) and torch.equal(counts, each[0][2])
        exp = wr.completed(t, n, W, Hp)
        assert list(counts.cpu().numpy()) == [len(exp)] * B41
        done = _mean_ok(mean.cpu().numpy(), probs.cpu().numpy(), ("decoder", t))
        assert done[:, :len(exp)].all() and not done[:, len(exp):].any()
        if exp:
            last = (exp[-1][1], mean[:, len(exp) - 1].cpu().numpy().copy())
        t += n
        got = dec.latest()
        assert got[3] is None
        for b in range(B41):
            assert (got[b] is None) == (last is None)
            if last is not None:
                assert got[b][0] == last[0] and got[b][1].tobytes() == last[1][b].tobytes()
    assert torch.equal(dec.state, torch.stack([o.state for o in ones])) and list(dec.steps) == [T41] * 3 + [0]
    if with_prep:
        assert all(torch.equal(dec.prep_state, o.prep_state) for o in ones)
    # a state_dict round trip in the middle of a stream continues bitwise
    sd = dec.state_dict()
    assert set(sd) == {"state", "window", "hop", "last_end", "last_probs"} | ({"prep_state"} if with_prep else set())
    assert tuple(sd["state"].shape) == tuple(dec.state.shape) and (sd["window"], sd["hop"]) == (W, Hp)
    other = nsd.EnsembleSlidingStreamDecoder(members, streams=4, window=W, hop=Hp)
    other.load_state_dict(sd)
    more = (synth_x(4, 6, seed=77) * (20.0 if with_prep else 1.0)).astype(np.float32)
    a = tuple(u.clone() for u in dec.push(more)) + (dec.member_probs.clone(),)      # (the two decoders share multi_window_step's buffers)
    b = other.push(more.copy()) + (other.member_probs,)
    assert all(u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes() for u, v in zip(a, b)) and not torch.isnan(a[0][:3, 0]).any()
    assert torch.equal(dec.state, other.state)
    assert [None if v is None else v[0] for v in other.latest()] == [None if v is None else v[0] for v in dec.latest()] == [44, 44, 44, None]
    # refusals: a checkpoint of another M, stream count, window or hop
    for bad in (dict(models=members[:2], streams=4, window=W, hop=Hp), dict(models=members, streams=2, window=W, hop=Hp),
                dict(models=members, streams=4, window=24, hop=8), dict(models=members, streams=4, window=W, hop=6)):
        with pytest.raises(nsd.NsdError):
            nsd.EnsembleSlidingStreamDecoder(bad.pop("models"), **bad).load_state_dict(sd)
    # reset of one slot: that stream restarts in every model and in the front end; the others go on
    dec.reset([1])
    assert list(dec.steps) == [T41 + 6, 0, T41 + 6, 6] and dec.latest()[1] is None and dec.latest()[0][0] == 44
    assert torch.equal(dec.state[:, [0, 2, 3]], other.state[:, [0, 2, 3]])
    fresh = nsd.EnsembleSlidingStreamDecoder(members, streams=4, window=W, hop=Hp)
    assert torch.equal(dec.state[:, 1], fresh.state[:, 1])
    if with_prep:
        assert not dec.prep_state[1].any() and dec.prep_state[0].any()
    dec.reset()
    assert list(dec.steps) == [0] * 4 and dec.latest() == [None] * 4 and torch.equal(dec.state, fresh.state)


def test_ensemble_sliding_decoder_refusals(nsd, dev, ref_state):
    ok = tms._members(nsd, dev, ref_state)
    with pytest.raises(nsd.NsdError, match="mixed shapes"):
        nsd.EnsembleSlidingStreamDecoder(ok[:2] + [nsd.EEG_LSTM(num_classes=5).to(dev).eval()], window=12, hop=4)
    with pytest.raises(nsd.NsdError, match="eval"):
        nsd.EnsembleSlidingStreamDecoder(ok[:2] + [tms._members(nsd, dev, ref_state)[2].train()], window=12, hop=4)
    with pytest.raises(nsd.NsdError, match="z-score"):
        nsd.EnsembleSlidingStreamDecoder(tms._members(nsd, dev, ref_state, normalize=True), window=12, hop=4)
    with pytest.raises(nsd.NsdError, match="bf16"):
        nsd.EnsembleSlidingStreamDecoder([nsd.EEG_LSTM(hidden_size=64, precision="bf16").to(dev).eval() for _ in range(2)], window=12, hop=4)
    with pytest.raises(nsd.NsdError, match="more than once"):
        nsd.EnsembleSlidingStreamDecoder([ok[0], ok[0]], window=12, hop=4)
    with pytest.raises(nsd.NsdError, match="options"):                   # members with and without a front end
        P = nsd.CausalPrep.design(highpass=1.0, lowpass=40.0, zscore_seconds=0.4, var0=250.0)
        nsd.EnsembleSlidingStreamDecoder(ok[:2] + tms._members(nsd, dev, ref_state, prep=P)[2:], window=12, hop=4)
    for W, Hp in ((12, 5), (4, 12), (0, 0), (12, 0), (129, 1)):
        with pytest.raises(nsd.NsdError, match="nsd_multi_window_path"):
            nsd.EnsembleSlidingStreamDecoder(ok, window=W, hop=Hp)
    with pytest.raises(nsd.NsdError, match="model-batched path"):
        nsd.EnsembleSlidingStreamDecoder([nsd.EEG_LSTM(hidden_size=32).to(dev).eval() for _ in range(2)], window=12, hop=4)
    dec = nsd.EnsembleSlidingStreamDecoder(ok, streams=2, window=12, hop=4)
    with pytest.raises(nsd.NsdError, match="3 streams pushed"):
        dec.push(np.zeros((3, 4, 8), np.float32))
    with pytest.raises(nsd.NsdError):
        dec.push(np.zeros((2, 4, 8), np.float32), slots=[0, 0])


# ---------------------------------------------------------------------------------------------------
# 12. end to end: EnsemblePredictor.open_stream and run_trials with a hop
# ---------------------------------------------------------------------------------------------------
def test_open_stream_and_run_trials_with_a_hop_and_three_models(nsd, dev, golden, ref_state, tmp_path, capsys):
    """(run_trials starts the replay producer, a process of its own: once here; its start is most of this test's time).  The reference
    is the mean of three single-model sliding runs, formed on the host in float64: not the serial fp32 sum, so PROB_TOL and not bits."""
    g = golden("real_trials")
    names = ["Food", "Water", "None"]
    paths = []
    for m, st in enumerate(tms._states(D, ref_state)):
        (tmp_path / f"m{m}").mkdir()
        paths.append(write_pth(str(tmp_path / f"m{m}"), st))
    pred = nsd.EnsemblePredictor(paths, 125, device="cpu", class_names=names, preprocess="identity")
    assert type(pred.open_stream()).__name__ == "PredictorStream"          # without the new arguments: today's object
    st = pred.open_stream(streams=2, window_seconds=2.0, hop_seconds=1.0)   # W = 250, hop = 125
    assert isinstance(st.decoder, nsd.EnsembleSlidingStreamDecoder) and st.decoder.params is pred.model.params
    assert (st.decoder.window, st.decoder.hop) == (250, 125)
    ones = [nsd.SimplePredictor(p, sr=125, device="cpu", class_names=names, preprocess="identity")
            .open_stream(streams=2, window_seconds=2.0, hop_seconds=1.0) for p in paths]
    assert all(type(o.decoder) is nsd.SlidingStreamDecoder for o in ones)
    w = np.stack([g["x"][0], g["x"][1]])
    found, each = [[], []], [[[], []] for _ in ones]
    for t0 in range(0, 625, 25):
        res = st.push(w[:, t0:t0 + 25])
        assert len(res) == 2
        for b in range(2):
            found[b] += res[b]
        for o, e in zip(ones, each):
            r = o.push(w[:, t0:t0 + 25])
            for b in range(2):
                e[b] += r[b]
    assert [[e for e, _, _ in f] for f in found] == [[250, 375, 500, 625]] * 2 and list(st.steps) == [625, 625]
    worst = 0.0
    for b in range(2):
        for i in range(4):
            want = np.mean([np.asarray(e[b][i][1], np.float64) for e in each], axis=0)
            _, probs, label = found[b][i]
            assert probs.dtype == np.float32
            worst = max(worst, float(np.abs(probs - want).max()))
            top = np.sort(want)
            if top[-1] - top[-2] > 1e-3:
                assert label == names[int(want.argmax())]
    print(f"ensemble open_stream(window, hop) vs the mean of three single-model sliding streams: {worst:.2e}")
    assert worst < PROB_TOL

    # run_trials on the replay source: the 5 s windows of the producer as one continuous stream, a decision every second from 5 s on
    dd = tmp_path / "trials"
    dd.mkdir()
    for i in range(3):
        np.savetxt(dd / f"food_{i:02d}.csv", g["x"][i], fmt="%.7f", delimiter=",")
    capsys.readouterr()
    res = nsd.run_trials(trials=5, serial_port=f"replay:{dd}", model_path=paths, verbose=True, queue_timeout=20.0,
                         predictor_kwargs={"preprocess": "identity"}, chunk_seconds=0.2, hop_seconds=1.0)
    out = capsys.readouterr().out
    assert not re.findall(r"^\[Trial ", out, re.M)
    lines = re.findall(r"^\[Window end=(\d+) @ [^\]]*\] pred=(\S+) probs=\[([^\]]*)\]", out, re.M)
    ends = list(range(625, 1126, 125))
    assert [int(e) for e, _, _ in lines] == ends and res.trials == 5       # one decision per hop
    whole = np.concatenate([g["x"][i] for i in range(3)])                  # the files in order: one stream of 1875 samples
    singles = [nsd.SlidingStreamDecoder(tgw.tgs._eval_model(nsd, dev, s), streams=1, window=625, hop=125) for s in tms._states(D, ref_state)]
    want = {}
    for t0 in range(0, 1125, 25):                                          # three single-model sliding runs, in the producer's chunks
        per = []
        for o in singles:
            p, e, c = o.push(whole[t0:t0 + 25])
            per.append((p.cpu().numpy().astype(np.float64), e.cpu().numpy(), int(c.cpu().numpy()[0])))
        for i in range(max(per[0][2], 0)):
            want[int(per[0][1][0, i])] = np.mean([p[0][0, i] for p in per], axis=0)
    assert sorted(want) == ends
    for (e, label, shown), end in zip(lines, ends):
        p = want[end]
        top = np.sort(p)
        if top[-1] - top[-2] > 1e-3:                                       # the label wherever the decision is clear
            assert label == names[int(p.argmax())]
        assert np.abs(np.array(shown.split(), np.float64) - p).max() < 5e-4 + PROB_TOL      # printed with three decimals
    err = float(np.abs(res.avg_probs - np.mean([want[e] for e in ends], 0)).max())
    print(f"run_trials(model_path=[a, b, c], hop_seconds=) vs the mean of three single-model sliding runs: {err:.2e}")
    assert res.avg_chunk.shape == (625, 8) and err < PROB_TOL              # (the CSV keeps 7 decimals)
