"""Resumable inference of an ensemble (nsd_multi_stream_step of include/nsd.h, csrc/nsd_multi_stream48.hip).  Needs the MI355X.

The contract is bit for bit: model m's slots, logits and probabilities after a call are what nsd_stream_step leaves and writes for that
model alone -- for any M, B, cut of the stream and placement in the grid -- and mean_probs is the serial fp32 mean of
tests/multi_stream_ref.py.  Against the oracle the existing bounds hold (logits 1e-4, probabilities 1e-5, rows summing to 1 within
1e-6, the argmax wherever the oracle's top two logits are more than 1e-3 apart); no tolerance is new here.  Outputs and state are
NaN-filled before use.  Unless said otherwise T = 41, B = 3, M = 3.  Each case takes milliseconds.
"""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

from oracle import nsd_oracle as orc
from tests import multi_stream_ref as mr
from tests import stream_ref as sr
from tests.buffer_contract import guarded, snapshot
from tests.golden.make_goldens import synth_params, synth_x
from tests.gpu_harness import LOGIT_TOL, NAN, PROB_TOL, D, dev, model_from_state, nsd, spec_of, to_dev  # noqa: F401  (dev, nsd: fixtures)

pytestmark = pytest.mark.gpu

ROW_SUM_TOL, ARGMAX_GAP = 1e-6, 1e-3
T41, B41, M3 = 41, 3, 3
SEEDS = (43, 44, 45)


# ---------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------
def _stride(spec):
    from nsd_amd import ops
    return int(ops.stream_layout(spec).stride)


def _new_state(dev, spec, S):
    """one model's S slots, NaN-filled, then reset through the library"""
    from nsd_amd import ops
    state = torch.full((S, _stride(spec)), NAN, device=dev)
    ops.stream_reset(spec, state)
    return state


def _new_multi(dev, spec, M, S):
    """[M,S,stride], NaN-filled, then reset as the flat state of M*S slots"""
    from nsd_amd import ops
    state = torch.full((M, S, _stride(spec)), NAN, device=dev)
    ops.stream_reset(spec, state.view(M * S, -1))
    return state


def _multi(dev, spec, params, x, state, *, slots=None, residual=False, read=True):
    """one nsd_multi_stream_step into NaN-filled outputs -> numpy logits [M,B,K], probs [M,B,K], mean [B,K] (Nones with read=False)"""
    from nsd_amd import ops
    M, B = int(params.shape[0]), int(x.shape[-3])
    out = [torch.full(s, NAN, device=dev) if read else None for s in ((M, B, spec.K), (M, B, spec.K), (B, spec.K))]
    got = ops.multi_stream_step(spec, params, x.contiguous(), state, slots=slots, residual=residual, read=read, logits=out[0], probs=out[1],
                                mean=out[2])
    if not read:
        assert got == (None, None, None)
        return None, None, None
    assert all(g is o for g, o in zip(got, out))
    return tuple(o.cpu().numpy() for o in out)


def _singles(dev, spec, params, x, states, *, slots=None, residual=False, read=True):
    """the M independent nsd_stream_step calls of the same chunk (x [B,n,C] shared or [M,B,n,C]) -> stacked numpy logits, probs"""
    from nsd_amd import ops
    M, B = int(params.shape[0]), int(x.shape[-3])
    lgs, prs = [], []
    for m in range(M):
        xm = (x[m] if x.dim() == 4 else x).contiguous()
        lg = torch.full((B, spec.K), NAN, device=dev) if read else None
        pr = torch.full((B, spec.K), NAN, device=dev) if read else None
        ops.stream_step(spec, params[m], xm, states[m], slots=slots, residual=residual, read=read, logits=lg, probs=pr)
        lgs.append(lg); prs.append(pr)
    if not read:
        return None, None
    return torch.stack(lgs).cpu().numpy(), torch.stack(prs).cpu().numpy()


def _bytes(state):
    return (torch.stack(list(state)) if isinstance(state, (list, tuple)) else state).cpu().numpy().tobytes()


def _same(multi_out, single_out, what):
    (lg, pr, mean), (slg, spr) = multi_out, single_out
    assert lg.tobytes() == slg.tobytes(), (what, "logits")
    assert pr.tobytes() == spr.tobytes(), (what, "probs")
    assert mean.tobytes() == mr.mean_probs(spr).tobytes(), (what, "mean")


def _check_outputs(lg, pr, ref, what):
    e_l = float(np.abs(lg - ref["logits"]).max())
    e_p, e_s = float(np.abs(pr - ref["probs"]).max()), float(np.abs(pr.astype(np.float64).sum(1) - 1.0).max())
    assert e_l < LOGIT_TOL, (what, e_l)                       # (a NaN left in an output fails here)
    assert e_p < PROB_TOL, (what, e_p)
    assert e_s < ROW_SUM_TOL, (what, e_s)
    top = np.sort(ref["logits"], axis=1)
    clear = (top[:, -1] - top[:, -2]) > ARGMAX_GAP
    assert np.array_equal(lg.argmax(1)[clear], ref["logits"].argmax(1)[clear]), what
    return e_l, e_p, e_s


VARIANTS = {"ref": (orc.Dims(), False), "residual": (orc.Dims(), True), "c3": (orc.Dims(C=3), False), "c3_residual": (orc.Dims(C=3), True)}
_cases = {}


def _states(d, ref_state, M=M3):
    """M parameter sets of shape d: synth_params of different seeds; the recorded checkpoint is member 0 where C = 8"""
    sts = [synth_params(d.C, 48, 2, d.K, seed=SEEDS[m % 3] + 10 * (m // 3)) for m in range(M)]
    if d.C == 8 and d.K == 3:
        sts[0] = ref_state
    return sts


def _case(name, ref_state):
    """(dims, residual, params [3,P], x [3,41,C]): computed once per variant and left unchanged"""
    if name not in _cases:
        d, residual = VARIANTS[name]
        params = np.stack([orc.flatten_state(st, d) for st in _states(d, ref_state)])
        _cases[name] = (d, residual, params, synth_x(B41, T41, C=d.C, seed=4100 + d.C))
    return _cases[name]


_whole = {}


def _whole_singles(dev, name, ref_state):
    """the M single-model 41-step calls of a variant: final state bytes, logits, probs"""
    if name not in _whole:
        d, residual, pn, xn = _case(name, ref_state)
        spec = spec_of(d)
        states = [_new_state(dev, spec, B41) for _ in range(M3)]
        lg, pr = _singles(dev, spec, to_dev(pn, dev), to_dev(xn, dev), states, residual=residual)
        _whole[name] = (_bytes(states), lg, pr)
    return _whole[name]


# ---------------------------------------------------------------------------------------------------
# 1. bitwise against the single-model call
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", sr.CUTS_41, ids=["ones", "fib", "40+1", "whole"])
@pytest.mark.parametrize("name", list(VARIANTS))
def test_every_chunk_leaves_the_bits_of_the_single_model_calls(nsd, dev, ref_state, name, cut):
    from nsd_amd import ops
    d, residual, pn, xn = _case(name, ref_state)
    spec, params, x = spec_of(d), to_dev(pn, dev), to_dev(xn, dev)
    state = _new_multi(dev, spec, M3, B41)
    assert _bytes(state) == _bytes(ops.multi_stream_state(spec, M3, B41, dev))
    singles = [_new_state(dev, spec, B41) for _ in range(M3)]
    t = 0
    for n in cut:
        chunk = x[:, t:t + n]
        t += n
        _same(_multi(dev, spec, params, chunk, state, residual=residual), _singles(dev, spec, params, chunk, singles, residual=residual),
              (name, cut, t))
        assert _bytes(state) == _bytes(singles), (name, cut, t)
    sb, lg, pr = _whole_singles(dev, name, ref_state)                 # ... and the cut does not show
    assert _bytes(state) == sb


@pytest.mark.parametrize("cut", sr.CUTS_41[:3], ids=["ones", "fib", "40+1"])
def test_advance_only_calls_end_in_the_same_bits(nsd, dev, ref_state, cut):
    d, residual, pn, xn = _case("ref", ref_state)
    spec, params, x = spec_of(d), to_dev(pn, dev), to_dev(xn, dev)
    state = _new_multi(dev, spec, M3, B41)
    t, out = 0, None
    for i, n in enumerate(cut):
        out = _multi(dev, spec, params, x[:, t:t + n], state, read=i == len(cut) - 1)
        t += n
    sb, lg, pr = _whole_singles(dev, "ref", ref_state)
    assert _bytes(state) == sb
    _same(out, (lg, pr), cut)


# ---------------------------------------------------------------------------------------------------
# 2. against the oracle, once per variant: every prefix, every model, and the mean
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(VARIANTS))
def test_every_prefix_of_every_model_matches_the_oracle(nsd, dev, ref_state, name):
    d, residual, pn, xn = _case(name, ref_state)
    spec, params, x = spec_of(d), to_dev(pn, dev), to_dev(xn, dev)
    refs = [sr.prefix_refs(pn[m], xn, d, range(1, T41 + 1), residual=residual) for m in range(M3)]
    state = _new_multi(dev, spec, M3, B41)
    worst = [0.0, 0.0, 0.0, 0.0]
    for t in range(1, T41 + 1):
        lg, pr, mean = _multi(dev, spec, params, x[:, t - 1:t], state, residual=residual)
        for m in range(M3):
            e = _check_outputs(lg[m], pr[m], refs[m][t], (name, "model", m, "t", t))
            worst[:3] = [max(a, b) for a, b in zip(worst, e)]
        want = np.mean([refs[m][t]["probs"].astype(np.float64) for m in range(M3)], axis=0)
        e_m = float(np.abs(mean - want).max())
        worst[3] = max(worst[3], e_m)
        assert e_m < PROB_TOL, (name, "mean", t, e_m)
        assert np.abs(mean.astype(np.float64).sum(1) - 1.0).max() < ROW_SUM_TOL
    print(f"multi stream {name}: logits {worst[0]:.2e} probs {worst[1]:.2e} row sums {worst[2]:.2e} mean {worst[3]:.2e}")


# ---------------------------------------------------------------------------------------------------
# 3. M = 1
# ---------------------------------------------------------------------------------------------------
def test_one_model_is_the_single_model_call_and_the_state_is_interchangeable(nsd, dev, ref_state):
    d, _, pn, xn = _case("ref", ref_state)
    spec, params, x = spec_of(d), to_dev(pn[:1], dev), to_dev(xn, dev)
    a, b = x[:, :13], x[:, 13:]
    # either entry alone
    single = _new_state(dev, spec, B41)
    _singles(dev, spec, params, a, [single])
    want = _singles(dev, spec, params, b, [single])
    multi = _new_multi(dev, spec, 1, B41)
    _multi(dev, spec, params, a, multi)
    got = _multi(dev, spec, params, b, multi)
    _same(got, want, "M = 1")
    assert got[2].tobytes() == got[1][0].tobytes()                      # the mean of one model is that model: p / 1.0f
    assert _bytes(multi) == _bytes([single])
    # advance with one, continue with the other
    s1 = _new_state(dev, spec, B41)
    _singles(dev, spec, params, a, [s1])
    _same(_multi(dev, spec, params, b, s1[None]), want, "single then multi")
    assert _bytes(s1) == _bytes(single)
    m1 = _new_multi(dev, spec, 1, B41)
    _multi(dev, spec, params, a, m1)
    lg, pr = _singles(dev, spec, params, b, [m1[0]])
    assert lg.tobytes() == want[0].tobytes() and pr.tobytes() == want[1].tobytes() and _bytes(m1[0]) == _bytes(single)


# ---------------------------------------------------------------------------------------------------
# 4. placement
# ---------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_placement(nsd, dev, ref_state):
    from nsd_amd import ops
    d, _, pn, xn = _case("ref", ref_state)
    spec, params, x = spec_of(d), to_dev(pn, dev), to_dev(xn, dev)
    cut, S = [7, 9, 25], 8

    def run(params, x, state, **kw):
        t, out = 0, None
        for n in cut:
            out = _multi(dev, spec, params, x[..., t:t + n, :], state, **kw)
            t += n
        return out

    plain = _new_multi(dev, spec, M3, S)
    reset = plain.cpu().numpy().copy()
    lg, pr, mean = run(params, x, plain)
    # the model count: model 1 of M = 3 is model 0 of M = 1 with the same parameters
    alone = _new_multi(dev, spec, 1, S)
    l1, p1, _ = run(params[1:2].contiguous(), x, alone)
    assert l1[0].tobytes() == lg[1].tobytes() and p1[0].tobytes() == pr[1].tobytes() and _bytes(alone[0]) == _bytes(plain[1])
    # the slot permutation, shared by the models; unnamed slots keep what the reset left
    perm = torch.tensor([6, 5, 2], dtype=torch.int32, device=dev)
    moved = _new_multi(dev, spec, M3, S)
    lp, pp, mp = run(params, x, moved, slots=perm)
    assert lp.tobytes() == lg.tobytes() and pp.tobytes() == pr.tobytes() and mp.tobytes() == mean.tobytes()
    mv, pl = moved.cpu().numpy(), plain.cpu().numpy()
    for m in range(M3):
        for b, s in enumerate((6, 5, 2)):
            assert mv[m, s].tobytes() == pl[m, b].tobytes(), (m, b)
        for s in (0, 1, 3, 4, 7):
            assert mv[m, s].tobytes() == reset[m, s].tobytes(), (m, s)
        for s in range(3, S):
            assert pl[m, s].tobytes() == reset[m, s].tobytes(), (m, s)
    # the other streams of the call: stream 1 alone in slot 5
    lone = _new_multi(dev, spec, M3, S)
    lo, po, mo = run(params, x[1:2], lone, slots=perm[1:2].contiguous())
    assert lo.tobytes() == lg[:, 1:2].tobytes() and po.tobytes() == pr[:, 1:2].tobytes() and mo.tobytes() == mean[1:2].tobytes()
    assert _bytes(lone[:, 5]) == _bytes(plain[:, 1])
    # x_model_stride: a shared chunk, and M copies of it at stride B*T*C
    copies = _new_multi(dev, spec, M3, S)
    lc, pc, mc = run(params, x[None].expand(M3, -1, -1, -1).contiguous(), copies)
    assert lc.tobytes() == lg.tobytes() and pc.tobytes() == pr.tobytes() and mc.tobytes() == mean.tobytes() and _bytes(copies) == _bytes(plain)
    # ... and a stride above B*T*C with another chunk per model, through the C ABI: what the single calls give on each model's chunk
    T, pad = 11, 24
    xs = np.stack([synth_x(B41, T, C=d.C, seed=4200 + m) for m in range(M3)])
    n = B41 * T * d.C
    buf = torch.full((M3, n + pad), NAN, device=dev)
    buf[:, :n] = to_dev(xs.reshape(M3, n), dev)
    strided, singles = _new_multi(dev, spec, M3, B41), [_new_state(dev, spec, B41) for _ in range(M3)]
    out = [torch.full(s, NAN, device=dev) for s in ((M3, B41, spec.K), (M3, B41, spec.K), (B41, spec.K))]
    dims = spec.dims(B41, T)
    import ctypes
    ops._call("nsd_multi_stream_step", dev, ctypes.byref(dims), M3, params.data_ptr(), buf.data_ptr(), n + pad, None, 0, strided.data_ptr(),
              strided.numel() * 4, B41, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), ops.STREAM)
    _same(tuple(o.cpu().numpy() for o in out), _singles(dev, spec, params, to_dev(xs, dev), singles), "stride above B*T*C")
    assert _bytes(strided) == _bytes(singles)


# ---------------------------------------------------------------------------------------------------
# 5. more (model, stream) pairs than compute units: every model's workgroups walk their stream loop again
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,B,T", [(32, 9, 5), (3, 100, 3)])
def test_more_work_than_compute_units(nsd, dev, ref_state, M, B, T):
    spec = spec_of(D)
    pn = np.stack([orc.flatten_state(st, D) for st in _states(D, ref_state, M)])
    params, x = to_dev(pn, dev), to_dev(synth_x(B, 2 * T, seed=1700 + M), dev)
    state, singles = _new_multi(dev, spec, M, B), [_new_state(dev, spec, B) for _ in range(M)]
    for t in (0, T):                                               # the second call loads every stream's state
        _same(_multi(dev, spec, params, x[:, t:t + T], state), _singles(dev, spec, params, x[:, t:t + T], singles), (M, B, t))
        assert _bytes(state) == _bytes(singles), (M, B, t)


# ---------------------------------------------------------------------------------------------------
# 6. failure behaviour on the device
# ---------------------------------------------------------------------------------------------------
def test_a_slot_index_outside_the_state_is_skipped_in_every_model(nsd, dev, ref_state):
    from nsd_amd import ops
    d, _, pn, xn = _case("ref", ref_state)
    spec, params, x = spec_of(d), to_dev(pn, dev), to_dev(xn, dev)
    S = 4
    state, check = guarded((M3, S, _stride(spec)), torch.float32, dev, "nan32")
    ops.stream_reset(spec, state.view(M3 * S, -1))
    before = state.cpu().numpy().copy()
    good = _new_multi(dev, spec, M3, S)
    glg, gpr, gmean = _multi(dev, spec, params, x[:, :9], good, slots=torch.tensor([2, 1, 0], dtype=torch.int32, device=dev))
    for bad in (S, -1, M3 * S):
        state.copy_(torch.from_numpy(before).to(dev))
        lg, pr, mean = _multi(dev, spec, params, x[:, :9], state, slots=torch.tensor([2, bad, 0], dtype=torch.int32, device=dev))
        check("multi stream state")
        assert np.isnan(lg[:, 1]).all() and np.isnan(pr[:, 1]).all() and np.isnan(mean[1]).all(), bad
        for a, g in ((lg, glg), (pr, gpr)):                        # the other streams are right
            assert a[:, [0, 2]].tobytes() == g[:, [0, 2]].tobytes(), bad
        assert mean[[0, 2]].tobytes() == gmean[[0, 2]].tobytes(), bad
        now, ok = state.cpu().numpy(), good.cpu().numpy()
        for m in range(M3):
            assert now[m, 1].tobytes() == before[m, 1].tobytes() and now[m, 3].tobytes() == before[m, 3].tobytes(), (bad, m)
            assert now[m, 0].tobytes() == ok[m, 0].tobytes() and now[m, 2].tobytes() == ok[m, 2].tobytes(), (bad, m)


def test_a_nan_sample_poisons_its_stream_in_every_model_until_reset(nsd, dev, ref_state):
    from nsd_amd import ops
    d, _, pn, xn = _case("ref", ref_state)
    spec, params, x = spec_of(d), to_dev(pn, dev), to_dev(xn, dev)
    clean = _new_multi(dev, spec, M3, B41)
    _multi(dev, spec, params, x[:, :9], clean)
    lc, pc, mc = _multi(dev, spec, params, x[:, 9:], clean)
    fresh = _new_multi(dev, spec, M3, B41)
    lf, pf, mf = _multi(dev, spec, params, x[:, :9], fresh)
    for poison in (np.nan, -np.inf):
        xb = xn.copy()
        xb[1, 4, 2] = poison
        xd = to_dev(xb, dev)
        dirty = _new_multi(dev, spec, M3, B41)
        first = _multi(dev, spec, params, xd[:, :9], dirty)
        lg, pr, mean = _multi(dev, spec, params, xd[:, 9:], dirty)          # clean samples: still NaN
        for a in first[:2] + (lg, pr):
            assert np.isnan(a[:, 1]).all() and not np.isnan(a[:, [0, 2]]).any(), poison
        assert np.isnan(first[2][1]).all() and np.isnan(mean[1]).all() and not np.isnan(mean[[0, 2]]).any()
        assert lg[:, [0, 2]].tobytes() == lc[:, [0, 2]].tobytes() and pr[:, [0, 2]].tobytes() == pc[:, [0, 2]].tobytes()
        assert mean[[0, 2]].tobytes() == mc[[0, 2]].tobytes()
        assert _bytes(dirty[:, [0, 2]]) == _bytes(clean[:, [0, 2]])
        # reset of slots {m*S + 1}: the stream restarts bitwise like a fresh one
        ops.stream_reset(spec, dirty.view(M3 * B41, -1), torch.tensor([m * B41 + 1 for m in range(M3)], dtype=torch.int32, device=dev))
        l2, p2, m2 = _multi(dev, spec, params, x[1:2, :9], dirty, slots=torch.tensor([1], dtype=torch.int32, device=dev))
        assert l2.tobytes() == lf[:, 1:2].tobytes() and p2.tobytes() == pf[:, 1:2].tobytes() and m2.tobytes() == mf[1:2].tobytes()
        assert _bytes(dirty[:, 1]) == _bytes(fresh[:, 1])


# ---------------------------------------------------------------------------------------------------
# 7. buffer contract
# ---------------------------------------------------------------------------------------------------
def test_outputs_and_state_are_written_inside_their_stated_sizes_and_inputs_are_left_alone(nsd, dev, ref_state):
    from nsd_amd import ops
    d, _, pn, xn = _case("c3", ref_state)
    spec, params, x = spec_of(d), to_dev(pn, dev), to_dev(xn[:, :9], dev)
    S = B41
    state, c_state = guarded((M3, S, _stride(spec)), torch.float32, dev, "nan32")
    ops.stream_reset(spec, state.view(M3 * S, -1))
    c_state("state after reset")
    lg, c_lg = guarded((M3, B41, spec.K), torch.float32, dev, "nan32")
    pr, c_pr = guarded((M3, B41, spec.K), torch.float32, dev, "nan32")
    mean, c_mean = guarded((B41, spec.K), torch.float32, dev, "nan32")
    snap = snapshot(params, x)
    ops.multi_stream_step(spec, params, x, state, logits=lg, probs=pr, mean=mean)
    torch.cuda.synchronize(dev)
    for c, what in ((c_state, "state"), (c_lg, "logits"), (c_pr, "probs"), (c_mean, "mean_probs")):
        c(what)
    assert snap.unchanged()
    for t in (state, lg, pr, mean):                                # everything stated is written
        assert not torch.isnan(t).any()
    # mean_probs == NULL: nothing is written beyond probs (and nothing to the mean buffer of the call before)
    mean.fill_(NAN)
    assert ops.multi_stream_step(spec, params, x, state, want_mean=False, logits=lg, probs=pr)[2] is None
    torch.cuda.synchronize(dev)
    for c, what in ((c_state, "state"), (c_lg, "logits"), (c_pr, "probs"), (c_mean, "mean_probs")):
        c(what + " (no mean)")
    assert torch.isnan(mean).all() and snap.unchanged() and not torch.isnan(pr).any()


# ---------------------------------------------------------------------------------------------------
# 8. side stream and graph replay: prep_step + multi_stream_step on one stream
# ---------------------------------------------------------------------------------------------------
def test_a_replayed_graph_of_prep_and_step_gives_the_bits_of_the_eager_run(nsd, dev, ref_state):
    from nsd_amd import ops
    d, _, pn, xn = _case("ref", ref_state)
    spec, params = spec_of(d), to_dev(pn, dev)
    P = nsd.CausalPrep.design(highpass=1.0, lowpass=40.0, zscore_seconds=0.4, var0=250.0)
    raw = to_dev((xn * 20.0 + 300.0).astype(np.float32), dev)
    cut = [8] * 5 + [1]                                            # 41 = 5 * 8 + 1: one graph per chunk length
    # eager, on the default stream
    est, eps = _new_multi(dev, spec, M3, B41), ops.prep_state(d.C, B41, dev)
    eager, t = [], 0
    for n in cut:
        eager.append(_multi(dev, spec, params, ops.prep_step(raw[:, t:t + n].contiguous(), P, eps), est))
        t += n
    # captured on a side stream, replayed
    gst, gps = _new_multi(dev, spec, M3, B41), ops.prep_state(d.C, B41, dev)
    out = [torch.full(s, NAN, device=dev) for s in ((M3, B41, spec.K), (M3, B41, spec.K), (B41, spec.K))]
    graphs = {}
    for n in sorted(set(cut)):
        xin, xout = torch.zeros((B41, n, d.C), device=dev), torch.empty((B41, n, d.C), device=dev)
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ops.prep_step(xin, P, gps, out=xout)
            ops.multi_stream_step(spec, params, xout, gst, logits=out[0], probs=out[1], mean=out[2])
        graphs[n] = (g, xin)
    ops.stream_reset(spec, gst.view(M3 * B41, -1))                    # (whatever the captures did or did not run)
    ops.prep_reset(d.C, gps)
    t = 0
    for i, n in enumerate(cut):
        g, xin = graphs[n]
        xin.copy_(raw[:, t:t + n])
        for o in out:
            o.fill_(NAN)
        g.replay()
        torch.cuda.synchronize(dev)
        t += n
        for o, e in zip(out, eager[i]):
            assert o.cpu().numpy().tobytes() == e.tobytes(), (i, t)
    assert _bytes(gst) == _bytes(est) and torch.equal(gps, eps)


# ---------------------------------------------------------------------------------------------------
# 9. EnsembleStreamDecoder
# ---------------------------------------------------------------------------------------------------
def _members(nsd, dev, ref_state, **kw):
    return [model_from_state(nsd, dev, st, **kw).eval() for st in _states(D, ref_state)]


def test_ensemble_decoder_push_against_the_ensemble_on_the_whole_window(nsd, dev, ref_state):
    from nsd_amd.multimodel import _EnsembleModel
    _, _, pn, xn = _case("ref", ref_state)
    ens = _EnsembleModel(_members(nsd, dev, ref_state))
    whole = ens.predict_proba(to_dev(xn, dev)).cpu().numpy()
    dec = nsd.EnsembleStreamDecoder(ens, streams=4)
    assert dec.params is ens.params and dec.member_probs is None      # the ensemble's own stacked buffer, not a copy
    assert dec.push(xn[:, :10], read=False) is None and dec.member_probs is None
    p = dec.push(to_dev(xn[:, 10:25], dev))
    assert tuple(p.shape) == (3, 3) and p.is_cuda and tuple(dec.member_probs.shape) == (M3, 3, 3)
    p = dec.push(xn[:, 25:]).cpu().numpy()
    assert list(dec.steps) == [T41, T41, T41, 0]
    e = float(np.abs(p - whole).max())
    print(f"ensemble decoder vs EnsemblePredictor's predict_proba: {e:.2e}")
    assert e < PROB_TOL and np.abs(p.astype(np.float64).sum(1) - 1).max() < ROW_SUM_TOL
    assert p.tobytes() == mr.mean_probs(dec.member_probs.cpu().numpy()).tobytes()
    # a state_dict round trip in mid-stream continues bitwise
    sd = dec.state_dict()
    assert set(sd) == {"state", "stride"} and tuple(sd["state"].shape) == (M3, 4, 256)
    other = nsd.EnsembleStreamDecoder(ens.models, streams=4)
    other.load_state_dict(sd)
    more = synth_x(4, 6, seed=77)
    assert torch.equal(dec.push(more), other.push(more)) and torch.equal(dec.state, other.state)
    assert torch.equal(dec.member_probs, other.member_probs)
    with pytest.raises(nsd.NsdError):
        nsd.EnsembleStreamDecoder(ens, streams=2).load_state_dict(sd)
    dec.reset([0])
    assert list(dec.steps) == [0, T41 + 6, T41 + 6, 6] and torch.equal(dec.state[:, 1:], other.state[:, 1:])
    assert not dec.state[:, 0, :192].any()
    dec.reset()
    assert list(dec.steps) == [0] * 4
    with pytest.raises(nsd.NsdError):
        dec.push(np.zeros((5, 2, 8), np.float32))                      # too many streams pushed


def test_ensemble_decoder_shares_one_front_end_and_equals_single_decoders_per_member(nsd, dev, ref_state):
    from nsd_amd import ops
    P = nsd.CausalPrep.design(highpass=1.0, lowpass=40.0, zscore_seconds=0.4, var0=250.0)
    _, _, pn, xn = _case("ref", ref_state)
    raw = (xn * 20.0 + 300.0).astype(np.float32)
    members = _members(nsd, dev, ref_state, prep=P)
    dec = nsd.EnsembleStreamDecoder(members, streams=B41)
    ones = [nsd.StreamDecoder(m, streams=B41) for m in members]
    names = []

    @contextlib.contextmanager
    def hook(name):
        names.append(name)
        yield
    t = 0
    for n in (7, 9, 25):
        ops.set_launch_hook(hook)
        try:
            mean = dec.push(raw[:, t:t + n])
        finally:
            ops.set_launch_hook(None)
        assert names == ["nsd_prep_step", "nsd_multi_stream_step"], names     # the prep kernel once per push, one step launch
        names.clear()
        each = torch.stack([o.push(raw[:, t:t + n]) for o in ones])
        t += n
        assert torch.equal(dec.member_probs, each), t
        assert mean.cpu().numpy().tobytes() == mr.mean_probs(each.cpu().numpy()).tobytes()
    assert torch.equal(dec.state, torch.stack([o.state for o in ones])) and all(torch.equal(dec.prep_state, o.prep_state) for o in ones)
    sd = dec.state_dict()
    assert set(sd) == {"state", "stride", "prep_state"}
    dec.reset([1])
    assert not dec.prep_state[1].any() and dec.prep_state[0].any() and list(dec.steps) == [T41, 0, T41]


def test_ensemble_decoder_refusals(nsd, dev, ref_state):
    ok = _members(nsd, dev, ref_state)
    with pytest.raises(nsd.NsdError, match="mixed shapes"):
        nsd.EnsembleStreamDecoder(ok[:2] + [nsd.EEG_LSTM(num_classes=5).to(dev).eval()])
    with pytest.raises(nsd.NsdError, match="eval"):
        nsd.EnsembleStreamDecoder(ok[:2] + [_members(nsd, dev, ref_state)[2].train()])
    with pytest.raises(nsd.NsdError, match="z-score"):
        nsd.EnsembleStreamDecoder(_members(nsd, dev, ref_state, normalize=True))
    with pytest.raises(nsd.NsdError, match="bf16"):
        nsd.EnsembleStreamDecoder([nsd.EEG_LSTM(hidden_size=64, precision="bf16").to(dev).eval() for _ in range(2)])
    with pytest.raises(nsd.NsdError, match="more than once"):
        nsd.EnsembleStreamDecoder([ok[0], ok[0]])
    dec = nsd.EnsembleStreamDecoder(ok, streams=2)
    with pytest.raises(nsd.NsdError, match="3 streams pushed"):
        dec.push(np.zeros((3, 4, 8), np.float32))
    with pytest.raises(nsd.NsdError):
        dec.push(np.zeros((2, 4, 8), np.float32), slots=[0, 0])


# ---------------------------------------------------------------------------------------------------
# 10. end to end: train the folds together, keep them, decode a stream with all of them
# ---------------------------------------------------------------------------------------------------
def _train(tmp, name, *extra):
    """`--seed 2`: with the default seed the two stratified folds of the 64 synthetic trials have 31 and 33 training windows, 1 and 2
    batches of 16 per epoch, which `--concurrent` refuses (train.concurrent_runs: one shared step needs the same count for every fold);
    seed 2 gives 32 / 32."""
    from nsd_amd import train
    d = tmp / name
    d.mkdir()
    out = str(d / "m.pth")
    argv = ["--synthetic", "64", "--T", "16", "--epochs", "1", "--batch", "16", "--kfold", "2", "--seed", "2", "--out", out] + list(extra)
    assert train.main(argv) == 0
    return d, out


def test_train_the_folds_keep_them_and_decode_a_stream_with_the_ensemble(nsd, dev, golden, tmp_path, capsys):
    d, out = _train(tmp_path, "concurrent", "--concurrent", "--save-folds")
    done = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    paths = [str(d / "m.fold0.pth"), str(d / "m.fold1.pth")]
    assert done["done"] and done["fold_checkpoints"] == paths and done["args"]["save_folds"] is True
    assert sorted(os.listdir(d)) == ["m.fold0.pth", "m.fold1.pth", "m.pth"]
    pred = nsd.EnsemblePredictor(paths, 125, preprocess="identity")
    w = synth_x(1, 16, seed=160)[0]
    want_p, want_label = pred.predict(w)
    st = pred.open_stream(streams=2)
    assert isinstance(st.decoder, nsd.EnsembleStreamDecoder) and st.decoder.params is pred.model.params
    assert st.push(w[:5], read=False) is None
    st.push(w[5:10])
    probs, labels = st.push(w[10:])
    e = float(np.abs(probs[0] - want_p).max())
    print(f"ensemble open_stream vs predict: {e:.2e}")
    assert probs.shape == (1, 3) and e < PROB_TOL and labels == [want_label] and list(st.steps) == [16, 0]
    # run_trials on a replay source with the fold models, chunked: predict() of the window (one trial: the producer is a process)
    rep = tmp_path / "trials"
    rep.mkdir()
    np.savetxt(rep / "food_00.csv", golden("real_trials")["x"][0], fmt="%.7f", delimiter=",")
    res = nsd.run_trials(trials=1, serial_port=f"replay:{rep}", model_path=paths, verbose=False, queue_timeout=20.0,
                         predictor_kwargs={"preprocess": "identity"}, chunk_seconds=0.2)
    want = pred.predict(np.loadtxt(rep / "food_00.csv", delimiter=",", dtype=np.float32))[0]
    assert res.trials == 1 and np.abs(res.avg_probs - want).max() < PROB_TOL
    capsys.readouterr()
    # without the flag no fold files appear and the final line has no new keys; the sequential mode writes the same names
    d2, _ = _train(tmp_path, "plain", "--concurrent")
    done2 = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert sorted(os.listdir(d2)) == ["m.pth"] and "fold_checkpoints" not in done2 and "save_folds" not in done2["args"]
    assert set(done) - set(done2) == {"fold_checkpoints"}
    d3, _ = _train(tmp_path, "sequential", "--save-folds")
    done3 = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert sorted(os.listdir(d3)) == ["m.fold0.pth", "m.fold1.pth", "m.pth"]
    assert [os.path.basename(p) for p in done3["fold_checkpoints"]] == ["m.fold0.pth", "m.fold1.pth"]
    seq = nsd.EnsemblePredictor(done3["fold_checkpoints"], 125, preprocess="identity")
    ps, _ = seq.open_stream().push(w)
    assert np.abs(ps[0] - seq.predict(w)[0]).max() < PROB_TOL
