"""Resumable H = 48 inference (nsd_stream_* of include/nsd.h, csrc/nsd_stream48.hip) against the CPU oracle.  Needs the MI355X.

A stream advanced chunk by chunk must give, after every chunk, what the oracle gives on the prefix seen so far -- at the project's
bounds: logits 1e-4, probabilities 1e-5, rows of probabilities summing to 1 within 1e-6, the same argmax wherever the oracle's top two
logits are more than 1e-3 apart, the stored h / c within 2e-5 / 5e-5 of the oracle's saved sequences and pool_acc / pool_den within 2e-5
of its `pooled` (the bounds tests/test_gpu_parity.py holds the training workspace to) -- and its state and outputs must be, BIT FOR
BIT, a function of the samples alone: not of the cut, the slot, the other streams of the call, the HIP stream or a graph replay.
State and outputs are NaN-filled before use.  Each case takes a few milliseconds.
"""
import re

import numpy as np
import pytest
import torch

from oracle import nsd_oracle as orc
from tests import sharp_attention as sa
from tests import stream_ref as sr
from tests.buffer_contract import guarded
from tests.golden.make_goldens import synth_params, synth_x
from tests.gpu_harness import LOGIT_TOL, NAN, PROB_TOL, D, dev, nsd, spec_of, to_dev, write_pth  # noqa: F401  (dev, nsd: fixtures)

pytestmark = pytest.mark.gpu

ROW_SUM_TOL, ARGMAX_GAP = 1e-6, 1e-3
H_TOL, C_TOL, POOLED_TOL = 2e-5, 5e-5, 2e-5
T41, B41 = 41, 3


# ---------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------
def _new_state(dev, spec, S):
    """S slots, NaN-filled, then reset through the library"""
    from nsd_amd import ops
    state = torch.full((S, int(ops.stream_layout(spec).stride)), NAN, device=dev)
    ops.stream_reset(spec, state)
    return state


def _step(dev, spec, flat, x, state, *, slots=None, residual=False, read=True):
    """one nsd_stream_step into NaN-filled outputs -> numpy logits, probs (None, None with read=False)"""
    from nsd_amd import ops
    B = x.shape[0]
    lg = torch.full((B, spec.K), NAN, device=dev) if read else None
    pr = torch.full((B, spec.K), NAN, device=dev) if read else None
    out = ops.stream_step(spec, flat, x.contiguous(), state, slots=slots, residual=residual, read=read, logits=lg, probs=pr)
    if not read:
        assert out == (None, None)
        return None, None
    assert out[0] is lg and out[1] is pr
    return lg.cpu().numpy(), pr.cpu().numpy()


def _fields(spec, state_np):
    """state [S, stride] as numpy -> dict of h [L,S,H], c [L,S,H], pooled [S,H], steps [S], max, den"""
    from nsd_amd import ops
    lay, H = ops.stream_layout(spec), spec.H
    cut = lambda o, n=H: state_np[:, int(o):int(o) + n]
    den = cut(lay.pool_den, 1)
    return dict(h=np.stack([cut(lay.h[l]) for l in range(spec.L)]), c=np.stack([cut(lay.c[l]) for l in range(spec.L)]),
                pooled=np.divide(cut(lay.pool_acc), den, out=np.full((state_np.shape[0], H), np.nan, np.float32), where=den != 0), den=den[:, 0], max=cut(lay.pool_max, 1)[:, 0],
                steps=np.ascontiguousarray(cut(lay.steps, 2)).view(np.int64)[:, 0])


def _check_outputs(lg, pr, ref, what):
    e_l = float(np.abs(lg - ref["logits"]).max())
    e_p, e_s = float(np.abs(pr - ref["probs"]).max()), float(np.abs(pr.astype(np.float64).sum(1) - 1.0).max())
    print(f"stream {what}: logits {e_l:.2e} probs {e_p:.2e} row sums {e_s:.2e}")
    assert e_l < LOGIT_TOL, (what, e_l)                       # (a NaN left in an output fails here)
    assert e_p < PROB_TOL, (what, e_p)
    assert e_s < ROW_SUM_TOL, (what, e_s)
    top = np.sort(ref["logits"], axis=1)
    clear = (top[:, -1] - top[:, -2]) > ARGMAX_GAP
    assert np.array_equal(lg.argmax(1)[clear], ref["logits"].argmax(1)[clear]), what


def _check_state(spec, state, ref, t, what, rows=None):
    """the stored state of the slots `rows` (default: the first B) against the oracle's saves of the prefix of length t"""
    f = _fields(spec, state.cpu().numpy())
    B = ref["pooled"].shape[0]
    rows = list(range(B)) if rows is None else rows
    e_h = float(np.abs(f["h"][:, rows] - ref["hseq"][:, :, t - 1]).max())
    e_c = float(np.abs(f["c"][:, rows] - ref["cseq"][:, :, t - 1]).max())
    e_p = float(np.abs(f["pooled"][rows] - ref["pooled"]).max())
    print(f"stream {what}: h {e_h:.2e} c {e_c:.2e} pooled {e_p:.2e}")
    assert e_h < H_TOL and e_c < C_TOL and e_p < POOLED_TOL, (what, e_h, e_c, e_p)
    assert np.array_equal(f["steps"][rows], np.full(len(rows), t)), (what, f["steps"])


VARIANTS = {"ref": (orc.Dims(), False), "residual": (orc.Dims(), True), "c3": (orc.Dims(C=3), False), "c3_residual": (orc.Dims(C=3), True)}
_cases = {}


def _case(name, ref_state):
    """(dims, residual, flat, x [3,41,C], oracle of every prefix): computed once per variant and left unchanged"""
    if name not in _cases:
        d, residual = VARIANTS[name]
        flat = orc.flatten_state(ref_state, d) if d.C == 8 else orc.flatten_state(synth_params(3, 48, 2, 3, seed=43), d)
        x = synth_x(B41, T41, C=d.C, seed=4100 + d.C)
        _cases[name] = (d, residual, flat, x, sr.prefix_refs(flat, x, d, range(1, T41 + 1), residual=residual))
    return _cases[name]


def _run_cut(dev, spec, flat, x, cut, state, *, slots=None, residual=False, read_all=True, each=None):
    """advance by the chunks of `cut`; each(t, lg, pr) after every call that reads -> last logits, probs"""
    t, lg, pr = 0, None, None
    for i, n in enumerate(cut):
        read = read_all or i == len(cut) - 1
        lg, pr = _step(dev, spec, flat, x[:, t:t + n], state, slots=slots, residual=residual, read=read)
        t += n
        if read and each is not None:
            each(t, lg, pr)
    return lg, pr


_whole = {}


def _whole_run(dev, name, ref_state):
    """the single 41-step call of a variant: final state bytes, logits, probs"""
    if name not in _whole:
        d, residual, flat, x, _ = _case(name, ref_state)
        spec = spec_of(d)
        state = _new_state(dev, spec, B41)
        lg, pr = _run_cut(dev, spec, to_dev(flat, dev), to_dev(x, dev), [T41], state, residual=residual)
        _whole[name] = (state.cpu().numpy().tobytes(), lg.tobytes(), pr.tobytes())
    return _whole[name]


# ---------------------------------------------------------------------------------------------------
# prefix parity and cut invariance
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", sr.CUTS_41, ids=["ones", "fib", "40+1", "whole"])
@pytest.mark.parametrize("name", list(VARIANTS))
def test_every_prefix_matches_the_oracle_and_the_cut_does_not_show(nsd, dev, ref_state, name, cut):
    d, residual, flat_np, xn, refs = _case(name, ref_state)
    spec, flat, x = spec_of(d), to_dev(flat_np, dev), to_dev(xn, dev)
    state = _new_state(dev, spec, B41)

    def each(t, lg, pr):
        _check_outputs(lg, pr, refs[t], (name, "t", t))
        _check_state(spec, state, refs[t], t, (name, "t", t))

    lg, pr = _run_cut(dev, spec, flat, x, cut, state, residual=residual, each=each)
    sb, lb, pb = _whole_run(dev, name, ref_state)
    assert state.cpu().numpy().tobytes() == sb, (name, cut)            # bit for bit: the state is a function of the samples alone
    assert lg.tobytes() == lb and pr.tobytes() == pb, (name, cut)


@pytest.mark.parametrize("cut", sr.CUTS_41[:3], ids=["ones", "fib", "40+1"])
def test_advance_only_calls_end_in_the_same_bits(nsd, dev, ref_state, cut):
    d, residual, flat_np, xn, refs = _case("ref", ref_state)
    spec = spec_of(d)
    state = _new_state(dev, spec, B41)
    lg, pr = _run_cut(dev, spec, to_dev(flat_np, dev), to_dev(xn, dev), cut, state, read_all=False)
    sb, lb, pb = _whole_run(dev, "ref", ref_state)
    assert state.cpu().numpy().tobytes() == sb and lg.tobytes() == lb and pr.tobytes() == pb, cut


def test_slot_and_batch_invariance(nsd, dev, ref_state):
    """Stream 1 alone in slot 5 of S = 8 == its row when advanced with two others under a permuted slots array; unnamed slots untouched."""
    d, _, flat_np, xn, refs = _case("ref", ref_state)
    spec, flat, x = spec_of(d), to_dev(flat_np, dev), to_dev(xn, dev)
    cut, S = [7, 9, 25], 8
    perm = torch.tensor([6, 5, 2], dtype=torch.int32, device=dev)
    together = _new_state(dev, spec, S)
    before = together.cpu().numpy().copy()
    lg3, pr3 = _run_cut(dev, spec, flat, x, cut, together, slots=perm)
    _check_outputs(lg3, pr3, refs[T41], "permuted slots")
    _check_state(spec, together, refs[T41], T41, "permuted slots", rows=[6, 5, 2])
    alone = _new_state(dev, spec, S)
    lg1, pr1 = _run_cut(dev, spec, flat, x[1:2], cut, alone, slots=perm[1:2].contiguous())
    assert lg1.tobytes() == lg3[1:2].tobytes() and pr1.tobytes() == pr3[1:2].tobytes()
    a, t = alone.cpu().numpy(), together.cpu().numpy()
    assert a[5].tobytes() == t[5].tobytes()
    for s in (0, 1, 3, 4, 7):                                  # not named: bitwise what the reset left
        assert t[s].tobytes() == before[s].tobytes(), s
    for s in (0, 1, 2, 3, 4, 6, 7):
        assert a[s].tobytes() == before[s].tobytes(), s


def test_more_streams_than_compute_units(nsd, dev, ref_state):
    """multi_processor_count + 2 streams, chunks of 7 and 9: two workgroups load a second stream's state and walk the loop again."""
    spec = spec_of(D)
    B = torch.cuda.get_device_properties(dev).multi_processor_count + 2
    flat_np, xn = orc.flatten_state(ref_state, D), synth_x(B, 16, seed=1607)
    flat, x = to_dev(flat_np, dev), to_dev(xn, dev)
    state = _new_state(dev, spec, B)
    lg7, pr7 = _step(dev, spec, flat, x[:, :7], state)
    _check_outputs(lg7, pr7, orc.forward(flat_np, np.ascontiguousarray(xn[:, :7]), D), ("B", B, "t", 7))
    lg, pr = _step(dev, spec, flat, x[:, 7:], state)
    ref = orc.forward(flat_np, xn, D, saves=True)
    _check_outputs(lg, pr, ref, ("B", B, "t", 16))
    _check_state(spec, state, ref, 16, ("B", B))
    big = state.cpu().numpy()
    for b in (0, 1, B - 2, B - 1):                             # first and second stream of the workgroups that loop
        one = _new_state(dev, spec, 1)
        _step(dev, spec, flat, x[b:b + 1, :7], one)
        l1, p1 = _step(dev, spec, flat, x[b:b + 1, 7:], one)
        assert l1.tobytes() == lg[b:b + 1].tobytes() and p1.tobytes() == pr[b:b + 1].tobytes(), b
        assert one.cpu().numpy()[0].tobytes() == big[b].tobytes(), b


def test_a_stream_longer_than_the_one_shot_limit(nsd, dev, ref_state):
    """1300 samples as ten chunks of 125 and one of 50 (ops.infer leaves its fast path above T = 1024)."""
    spec, B, T = spec_of(D), 2, 1300
    flat_np, xn = orc.flatten_state(ref_state, D), synth_x(B, T, seed=1300)
    ref = orc.forward(flat_np, xn, D, saves=True)
    state = _new_state(dev, spec, B)
    lg, pr = _run_cut(dev, spec, to_dev(flat_np, dev), to_dev(xn, dev), [125] * 10 + [50], state, read_all=False)
    _check_outputs(lg, pr, ref, ("T", T))
    _check_state(spec, state, ref, T, ("T", T))


@pytest.mark.parametrize("s", [sa.S_GRAD, sa.S_SAT])
@pytest.mark.parametrize("T", [17, 64])
def test_peaked_attention_in_chunks_of_five(nsd, dev, T, s):
    """attn.weight times 100 / 1000: the running max rises along the stream and the sums are rescaled by exp(-large)."""
    spec, B = spec_of(D), sa.SHARP_B
    flat_np, xn = orc.flatten_state(sa.sharp_state(s), D), sa.sharp_inputs(B, T)[0]
    cut = [5] * (T // 5) + ([T % 5] if T % 5 else [])
    refs = sr.prefix_refs(flat_np, xn, D, sr.cut_points(cut))
    state = _new_state(dev, spec, B)
    seen = []

    def each(t, lg, pr):
        _check_outputs(lg, pr, refs[t], ("sharp", s, "t", t))
        _check_state(spec, state, refs[t], t, ("sharp", s, "t", t))
        seen.append(_fields(spec, state.cpu().numpy())["max"].copy())

    _run_cut(dev, spec, to_dev(flat_np, dev), to_dev(xn, dev), cut, state, each=each)
    if s == sa.S_SAT:                                           # the oracle's own alphas: the case does rescale by a vanishing factor
        assert sa.spread(refs[T]["alpha"]) > 40.0              # exp(-40) = 4e-18
    assert (np.diff(np.stack(seen), axis=0) >= 0).all() and (np.stack(seen)[-1] > np.stack(seen)[0]).any()


# ---------------------------------------------------------------------------------------------------
# reset, bad slot, non-finite sample
# ---------------------------------------------------------------------------------------------------
def test_reset_of_one_slot_restarts_it(nsd, dev, ref_state):
    from nsd_amd import ops
    d, _, flat_np, xn, refs = _case("ref", ref_state)
    spec, flat, x = spec_of(d), to_dev(flat_np, dev), to_dev(xn, dev)
    state = _new_state(dev, spec, B41)
    _step(dev, spec, flat, x[:, :13], state, read=False)
    ops.stream_reset(spec, state, torch.tensor([1], dtype=torch.int32, device=dev))
    f = _fields(spec, state.cpu().numpy())
    assert list(f["steps"]) == [13, 0, 13] and f["max"][1] == -np.inf and f["den"][1] == 0 and not f["h"][:, 1].any() and not f["c"][:, 1].any()
    # stream 1 starts over with its samples 13..; the others go on
    lg, pr = _step(dev, spec, flat, x[:, 13:], state)
    fresh = _new_state(dev, spec, 1)
    l1, p1 = _step(dev, spec, flat, x[1:2, 13:], fresh)
    assert lg[1:2].tobytes() == l1.tobytes() and pr[1:2].tobytes() == p1.tobytes()
    assert state.cpu().numpy()[1].tobytes() == fresh.cpu().numpy()[0].tobytes()
    ref1 = orc.forward(flat_np, np.ascontiguousarray(xn[1:2, 13:]), D)
    _check_outputs(l1, p1, ref1, "restarted stream")
    _check_outputs(lg[[0, 2]], pr[[0, 2]], {k: refs[T41][k][[0, 2]] for k in ("logits", "probs")}, "streams that went on")


def test_a_slot_index_outside_the_state_gives_nan_rows_and_touches_nothing(nsd, dev, ref_state):
    from nsd_amd import ops
    d, _, flat_np, xn, refs = _case("ref", ref_state)
    spec, flat, x = spec_of(d), to_dev(flat_np, dev), to_dev(xn, dev)
    S = 4
    state, check = guarded((S, int(ops.stream_layout(spec).stride)), torch.float32, dev, "nan32")
    ops.stream_reset(spec, state)
    before = state.cpu().numpy().copy()
    for bad in (S, -1):
        slots = torch.tensor([2, bad, 0], dtype=torch.int32, device=dev)
        state.copy_(torch.from_numpy(before).to(dev))
        lg, pr = _step(dev, spec, flat, x[:, :9], state, slots=slots)
        check("stream state")
        assert np.isnan(lg[1]).all() and np.isnan(pr[1]).all(), bad
        _check_outputs(lg[[0, 2]], pr[[0, 2]], {k: refs[9][k][[0, 2]] for k in ("logits", "probs")}, ("bad slot", bad))
        now = state.cpu().numpy()
        assert now[1].tobytes() == before[1].tobytes() and now[3].tobytes() == before[3].tobytes(), bad
    # a reset that names the same index skips it
    ops.stream_reset(spec, state, torch.tensor([S, 2], dtype=torch.int32, device=dev))
    check("stream state after reset")
    assert state.cpu().numpy()[2].tobytes() == before[2].tobytes()


def test_a_nan_sample_poisons_its_stream_until_reset(nsd, dev, ref_state):
    from nsd_amd import ops
    d, _, flat_np, xn, refs = _case("ref", ref_state)
    spec, flat = spec_of(d), to_dev(flat_np, dev)
    for poison in (np.nan, np.inf):
        xb = xn.copy()
        xb[1, 4, 2] = poison
        clean, dirty = _new_state(dev, spec, B41), _new_state(dev, spec, B41)
        x, xd = to_dev(xn, dev), to_dev(xb, dev)
        lc, pc = _run_cut(dev, spec, flat, x, [9, 32], clean)
        lg9, pr9 = _step(dev, spec, flat, xd[:, :9], dirty)
        lg, pr = _step(dev, spec, flat, xd[:, 9:], dirty)                   # clean samples: still NaN
        for a in (lg9, pr9, lg, pr):
            assert np.isnan(a[1]).all() and not np.isnan(a[[0, 2]]).any(), poison
        assert lg[[0, 2]].tobytes() == lc[[0, 2]].tobytes() and pr[[0, 2]].tobytes() == pc[[0, 2]].tobytes()
        dn, cn = dirty.cpu().numpy(), clean.cpu().numpy()
        assert dn[0].tobytes() == cn[0].tobytes() and dn[2].tobytes() == cn[2].tobytes()
        f = _fields(spec, dn)
        assert np.isnan(f["h"][:, 1]).all() and np.isnan(f["c"][:, 1]).all() and np.isnan(f["pooled"][1]).all()
        ops.stream_reset(spec, dirty, torch.tensor([1], dtype=torch.int32, device=dev))
        l2, p2 = _step(dev, spec, flat, x[:, :9], dirty)
        _check_outputs(l2[1:2], p2[1:2], {k: refs[9][k][1:2] for k in ("logits", "probs")}, "after reset")


# ---------------------------------------------------------------------------------------------------
# side stream, graph replay
# ---------------------------------------------------------------------------------------------------
def test_side_stream_and_graph_replay_give_the_same_bits(nsd, dev, ref_state):
    from nsd_amd import ops
    d, _, flat_np, xn, refs = _case("ref", ref_state)
    spec, flat, x = spec_of(d), to_dev(flat_np, dev), to_dev(xn, dev)
    sb, lb, pb = _whole_run(dev, "ref", ref_state)
    side = torch.cuda.Stream(device=dev)
    state = _new_state(dev, spec, B41)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        lg, pr = _run_cut(dev, spec, flat, x, [20, 21], state)
    side.synchronize()
    assert state.cpu().numpy().tobytes() == sb and lg.tobytes() == lb and pr.tobytes() == pb
    # one captured graph of two consecutive calls (20 samples, then 21 with readout), replayed: every replay advances by 41
    xa, xb = x[:, :20].contiguous(), x[:, 20:].contiguous()
    gstate = _new_state(dev, spec, B41)
    glg, gpr = torch.full((B41, spec.K), NAN, device=dev), torch.full((B41, spec.K), NAN, device=dev)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.stream_step(spec, flat, xa, gstate, read=False)
        ops.stream_step(spec, flat, xb, gstate, logits=glg, probs=gpr)
    ops.stream_reset(spec, gstate)                                 # (whatever the capture did or did not run)
    glg.fill_(NAN); gpr.fill_(NAN)
    graph.replay()
    torch.cuda.synchronize(dev)
    assert gstate.cpu().numpy().tobytes() == sb and glg.cpu().numpy().tobytes() == lb and gpr.cpu().numpy().tobytes() == pb
    graph.replay()
    torch.cuda.synchronize(dev)
    assert list(_fields(spec, gstate.cpu().numpy())["steps"]) == [2 * T41] * B41
    eager = _new_state(dev, spec, B41)
    l2, p2 = _run_cut(dev, spec, flat, torch.cat([x, x], 1), [T41, T41], eager)
    assert gstate.cpu().numpy().tobytes() == eager.cpu().numpy().tobytes()
    assert glg.cpu().numpy().tobytes() == l2.tobytes() and gpr.cpu().numpy().tobytes() == p2.tobytes()


# ---------------------------------------------------------------------------------------------------
# the Python surface
# ---------------------------------------------------------------------------------------------------
def _eval_model(nsd, dev, ref_state, **kw):
    m = nsd.EEG_LSTM(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in ref_state.items()}, strict=True)
    return m.to(dev).eval()


@pytest.mark.parametrize("residual", [False, True])
def test_stream_decoder_push_equals_predict_proba(nsd, dev, ref_state, residual):
    d, _, flat_np, xn, _ = _case("ref", ref_state)
    model = _eval_model(nsd, dev, ref_state, residual=residual)
    whole = model.predict_proba(to_dev(xn, dev)).cpu().numpy()
    ref = orc.forward(flat_np, xn, D, residual=residual)
    dec = nsd.StreamDecoder(model, streams=4)
    assert dec.push(xn[:, :10], read=False) is None
    p = dec.push(to_dev(xn[:, 10:25], dev))
    assert tuple(p.shape) == (3, 3) and p.is_cuda
    p = dec.push(xn[:, 25:]).cpu().numpy()
    assert list(dec.steps) == [T41, T41, T41, 0]
    assert np.abs(p - whole).max() < PROB_TOL and np.abs(p - ref["probs"]).max() < PROB_TOL
    assert np.abs(p.astype(np.float64).sum(1) - 1).max() < ROW_SUM_TOL
    # one stream as [n, C] into a named slot; state_dict round trip into a second decoder
    p3 = dec.push(xn[2], slots=[3]).cpu().numpy()
    assert p3.shape == (1, 3) and np.abs(p3[0] - ref["probs"][2]).max() < PROB_TOL and list(dec.steps) == [T41] * 4
    sd = dec.state_dict()
    other = nsd.StreamDecoder(model, streams=4)
    other.load_state_dict(sd)
    more = synth_x(4, 6, seed=77)
    assert torch.equal(dec.push(more), other.push(more)) and torch.equal(dec.state, other.state)
    with pytest.raises(nsd.NsdError):
        nsd.StreamDecoder(model, streams=2).load_state_dict(sd)
    dec.reset([0])
    assert list(dec.steps) == [0, T41 + 6, T41 + 6, T41 + 6]
    dec.reset()
    assert list(dec.steps) == [0] * 4
    with pytest.raises(nsd.NsdError):
        dec.push(xn[:, :2], slots=[0, 0, 1])
    with pytest.raises(nsd.NsdError):
        dec.push(np.zeros((5, 2, 8), np.float32))


def test_stream_decoder_refusals(nsd, dev, ref_state):
    with pytest.raises(nsd.NsdError, match="z-score"):
        nsd.StreamDecoder(_eval_model(nsd, dev, ref_state, normalize=True))
    with pytest.raises(nsd.NsdError, match="eval"):
        nsd.StreamDecoder(_eval_model(nsd, dev, ref_state).train())
    with pytest.raises(nsd.NsdError, match="nsd_stream_path"):
        nsd.StreamDecoder(nsd.EEG_LSTM(hidden_size=32).to(dev).eval())
    with pytest.raises(nsd.NsdError, match="bf16"):
        nsd.StreamDecoder(nsd.EEG_LSTM(hidden_size=64, precision="bf16").to(dev).eval())
    with pytest.raises(nsd.NsdError, match="bidirectional"):
        nsd.StreamDecoder(nsd.EEG_LSTM(hidden_size=64, precision="bf16", bidirectional=True).to(dev).eval())


class _WindowFilter:
    """stands for the reference's per-window PreProcessor: anything that is not the identity preprocessor"""

    def transform(self, x):
        return np.asarray(x, np.float32) - np.asarray(x, np.float32).mean(0, keepdims=True)


def test_open_stream_and_chunked_run_trials(nsd, dev, golden, ref_state, tmp_path, capsys):
    g = golden("real_trials")
    pth = write_pth(str(tmp_path), ref_state)
    names = ["Food", "Water", "None"]
    filt = nsd.SimplePredictor(pth, sr=125, device="cpu", class_names=names, preprocess=_WindowFilter())
    with pytest.raises(nsd.NsdError, match="not causal"):
        filt.open_stream()
    pred = nsd.SimplePredictor(pth, sr=125, device="cpu", class_names=names, preprocess="identity")
    st = pred.open_stream(streams=2)
    w = np.stack([g["x"][0], g["x"][1]])
    for t0 in range(0, 600, 25):
        assert st.push(w[:, t0:t0 + 25], read=False) is None
    probs, labels = st.push(w[:, 600:])
    assert np.abs(probs - g["probs"][:2]).max() < PROB_TOL and labels == [names[int(i)] for i in g["argmax"][:2]]
    # a caller's per-chunk transform in place of the window filter
    half = filt.open_stream(chunk_transform=lambda c: 0.5 * np.asarray(c, np.float32))
    ph, _ = half.push(2.0 * g["x"][0])
    assert np.abs(ph[0] - g["probs"][0]).max() < PROB_TOL
    # run_trials on the replay source, chunked: the labels of the window mode wherever the probability gap exceeds 1e-3
    d = tmp_path / "trials"
    d.mkdir()
    for i in range(4):
        np.savetxt(d / f"food_{i:02d}.csv", g["x"][i], fmt="%.7f", delimiter=",")
    kw = dict(trials=4, serial_port=f"replay:{d}", model_path=pth, verbose=True, queue_timeout=20.0, predictor_kwargs={"preprocess": "identity"})

    def run(**extra):
        capsys.readouterr()
        res = nsd.run_trials(**kw, **extra)
        lines = re.findall(r"^\[Trial (\d+) @ [^\]]*\] pred=(\S+) probs=", capsys.readouterr().out, re.M)
        return res, [label for _, label in sorted(lines)]

    (win, lwin), (chk, lchk) = run(), run(chunk_seconds=0.2)
    assert chk.trials == 4 and len(lwin) == 4 and len(lchk) == 4
    assert chk.avg_chunk.shape == (625, 8) and np.array_equal(chk.avg_chunk, win.avg_chunk)
    assert np.abs(chk.avg_probs - win.avg_probs).max() < PROB_TOL and np.abs(chk.avg_probs - g["probs"][:4].mean(0)).max() < PROB_TOL
    for i in range(4):                                           # the window mode's label wherever its decision is clear
        top = np.sort(g["probs"][i])
        if top[-1] - top[-2] > 1e-3:
            assert lchk[i] == lwin[i] == names[int(g["argmax"][i])], i
