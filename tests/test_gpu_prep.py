"""The causal front end on the MI355X (nsd_prep_* of include/nsd.h, csrc/nsd_prep.hip) against its numpy restatement
(tests/prep_ref.py): every finite value BIT FOR BIT, NaNs by position (the quiet-NaN pattern differs between the host and the GPU).
Window mode over every switch and the shapes at which the kernel takes another path (the time tile of 32 steps, 64 / C streams per wave,
16-byte and dword staging, the grid cap), stream mode over cuts, slots, HIP streams and a graph replay, the buffer contract, and the
path through every Python layer: the model, both trainers, the stream decoder and a checkpoint."""
import numpy as np
import pytest
import torch

from oracle import nsd_oracle as orc
from tests import prep_ref as pr
from tests import stream_ref as sr
from tests.buffer_contract import guarded, snapshot
from tests.gpu_harness import LOGIT_TOL, NAN, PROB_TOL, D, dev, nsd, spec_of, sync_at_the_end, to_dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

TILE = 32                        # PREP_TT of csrc/nsd_args.h: time steps staged through LDS at once
GRID_CAP = 1024                  # PREP_GRID_CAP: workgroups of a launch
CUTS = ([41], [1] * 41, [7, 1, 33], [16, 16, 9], [32, 9])
T41, B41 = 41, 3


def _design(nsd, n=3, **kw):
    secs = nsd.CausalPrep.design(highpass=1.0, lowpass=40.0, notch=50.0).sections + nsd.CausalPrep.design(highpass=4.0).sections
    return nsd.CausalPrep(sections=secs[:n], **kw)


def _configs(nsd):
    """each of the five switches on and off against a non-trivial neighbour"""
    z = dict(alpha=0.01, var0=300.0)
    return {
        "off": nsd.CausalPrep(baseline=False),
        "baseline": nsd.CausalPrep(),
        "car": nsd.CausalPrep(baseline=False, car=True),
        "baseline_car": nsd.CausalPrep(car=True),
        "s1": _design(nsd, 1), "s2": _design(nsd, 2, baseline=False), "s3": _design(nsd, 3), "s4": _design(nsd, 4, car=True),
        "zscore": nsd.CausalPrep(baseline=False, **z),
        "s3_zscore": _design(nsd, 3, **z),
        "full": _design(nsd, 3, car=True, **z),
        "full_no_baseline": _design(nsd, 4, baseline=False, car=True, **z),
    }


def _kw(p):
    return dict(sections=p.sections, alpha=p.alpha, var0=p.var0, baseline=p.baseline, car=p.car)


def _raw(B, T, Cc, seed=0):
    """raw-amplifier-like windows: noise of 20 units on per-channel DC offsets of up to 5000"""
    rs = np.random.RandomState(seed + 1000 * B + 10 * T + Cc)
    return (20.0 * rs.standard_normal((B, T, Cc)) + 5000.0 * rs.uniform(-1, 1, (B, 1, Cc))).astype(np.float32)


def _window(dev, x_np, p, *, in_place=False, offset=0):
    """ops.prep_step in window mode into a NaN-filled, guarded y (offset: y starts that many floats into its buffer: not 16-byte
    aligned) -> numpy y; the input is checked to be unchanged"""
    from nsd_amd import ops
    x = to_dev(x_np, dev)
    if in_place:
        buf, check = guarded(x_np.shape, torch.float32, dev)
        buf.copy_(x)
        out = ops.prep_step(buf, p, out=buf)
        assert out is buf
        check("x / y in place")
        return out.cpu().numpy()
    flat, check = guarded((x_np.size + offset,), torch.float32, dev, "nan32")
    y = flat[offset:].view(x_np.shape)
    snap = snapshot(x)
    out = ops.prep_step(x, p, out=y)
    assert out is y and snap.unchanged()
    check("y")
    assert offset == 0 or np.isnan(flat[:offset].cpu().numpy()).all()
    return y.cpu().numpy()


# C in {1, 3, 8, 64}, B in {1, 5, 70}, T in {1, 2, 33, 65, 131} and 31 / 32 / 33 around the time tile; B = 70 at C = 1 fills a wave and
# starts a second, at C = 8 and C = 3 it ends inside a wave; T * C % 4 != 0 takes the dword staging
SHAPES = [(1, 1, 1), (5, 2, 3), (70, 33, 1), (5, 65, 1), (1, 131, 3), (70, 2, 3), (5, 33, 3), (1, 31, 8), (5, 32, 8), (70, 33, 8),
          (1, 65, 8), (5, 131, 8), (1, 2, 64), (5, 33, 64), (1, 64, 64), (70, 1, 64), (5, 131, 5)]


@pytest.mark.parametrize("B,T,Cc", SHAPES)
def test_window_mode_equals_the_reference_bitwise(nsd, dev, B, T, Cc):
    x = _raw(B, T, Cc)
    for name, p in _configs(nsd).items():
        want = pr.prep_ref(x, **_kw(p))
        assert pr.same_bits(_window(dev, x, p), want), name
    assert np.isfinite(want).all()


def test_everything_off_is_a_copy_and_in_place_is_allowed(nsd, dev):
    x = _raw(5, 40, 8)
    x[0, 0, 0], x[1, 3, 2], x[2, 5, 1] = -0.0, np.inf, 1e-42                  # a negative zero, an Inf and a denormal pass through
    assert _window(dev, x, nsd.CausalPrep(baseline=False)).tobytes() == x.tobytes()
    x = _raw(5, 70, 8)
    for name in ("off", "full", "s4"):
        p = _configs(nsd)[name]
        assert pr.same_bits(_window(dev, x, p, in_place=True), pr.prep_ref(x, **_kw(p))), name
    # a y that is not 16-byte aligned while T * C is a multiple of 4: the dword staging
    p = _configs(nsd)["full"]
    for off in (1, 2, 3):
        assert pr.same_bits(_window(dev, x, p, offset=off), pr.prep_ref(x, **_kw(p))), off


@pytest.mark.parametrize("B,T,Cc", [(GRID_CAP + 6, 3, 64), (8 * GRID_CAP + 3, 2, 8), (64 * GRID_CAP + 1, 1, 1)])
def test_more_stream_groups_than_the_grid_cap(nsd, dev, B, T, Cc):
    x = _raw(B, T, Cc)
    p = _configs(nsd)["full"]
    assert pr.same_bits(_window(dev, x, p), pr.prep_ref(x, **_kw(p)))


# ---- stream mode -----------------------------------------------------------------------------------------------------------------------
def _new_state(dev, Cc, S):
    """S slots between guards, NaN-filled, then reset through the library -> (state, check)"""
    from nsd_amd import ops
    state, check = guarded((S, int(ops.prep_layout(Cc).stride)), torch.float32, dev, "nan32")
    ops.prep_reset(Cc, state)
    return state, check


def _run_cut(dev, x_np, p, cut, state, slots=None):
    """the chunks of `cut` through ops.prep_step in stream mode, each into a NaN-filled guarded y -> numpy y [B,T,C]"""
    from nsd_amd import ops
    parts, t = [], 0
    for n in cut:
        xc = to_dev(x_np[:, t:t + n], dev)
        y, check = guarded(xc.shape, torch.float32, dev, "nan32")
        snap = snapshot(xc, slots)
        assert ops.prep_step(xc, p, state, slots=slots, out=y) is y and snap.unchanged()
        check("y")
        parts.append(y.cpu().numpy())
        t += n
    return np.concatenate(parts, 1)


@pytest.mark.parametrize("name", ["full", "s4", "zscore", "baseline_car"])
def test_cuts_slots_and_neighbours_do_not_show(nsd, dev, name):
    from nsd_amd import ops
    p = _configs(nsd)[name]
    x = _raw(B41, T41, 8)
    want = pr.prep_ref(x, **_kw(p))
    ref_state = pr.State(B41, 8)
    pr.prep_ref(x, state=ref_state, **_kw(p))
    rows = ref_state.slot_rows()
    assert pr.same_bits(_window(dev, x, p), want)
    blank, _ = _new_state(dev, 8, 1)
    assert not blank.cpu().numpy().any()                                       # a reset slot is all zero
    states = []
    for cut in CUTS:
        state, check = _new_state(dev, 8, B41)
        assert pr.same_bits(_run_cut(dev, x, p, cut, state), want), cut
        check("state")
        states.append(state.cpu().numpy())
        assert pr.same_bits(states[-1], rows), cut
        assert states[-1].tobytes() == states[0].tobytes(), cut
        assert list(states[-1][:, int(ops.prep_layout(8).steps):][:, :2].copy().view(np.int64).reshape(-1)) == [T41] * B41
    # permuted slots inside a larger state, with other streams in the same calls: stream b of x lives in slot perm[b], and two more
    # streams of other data ride along
    S, perm = 7, [5, 0, 3, 6, 2]
    other = _raw(2, T41, 8, seed=9)
    state, check = _new_state(dev, 8, S)
    slots = torch.tensor(perm, dtype=torch.int32, device=dev)
    got = _run_cut(dev, np.concatenate([x, other]), p, [7, 1, 33], state, slots=slots)
    check("state")
    assert pr.same_bits(got[:B41], want) and pr.same_bits(got[B41:], pr.prep_ref(other, **_kw(p)))
    st = state.cpu().numpy()
    for b in range(B41):
        assert st[perm[b]].tobytes() == states[0][b].tobytes(), b
    assert not st[1].any() and not st[4].any()                                 # slots nobody named stay reset


def test_side_stream_and_graph_replay_of_prep_and_stream_step(nsd, dev, ref_state):
    from nsd_amd import ops
    p = _configs(nsd)["full"]
    spec, flat = spec_of(D), to_dev(orc.flatten_state(ref_state, D), dev)
    x = _raw(B41, T41, 8)
    xd = to_dev(x, dev)

    def new_states():
        ps, _ = _new_state(dev, 8, B41)
        ms = torch.full((B41, int(ops.stream_layout(spec).stride)), NAN, device=dev)
        ops.stream_reset(spec, ms)
        return ps, ms

    def run(ps, ms, chunks, bufs=None):
        """prep step then stream step per chunk; the last one reads the decision"""
        out = None
        for k, xc in enumerate(chunks):
            xp = ops.prep_step(xc, p, ps, out=None if bufs is None else bufs[k])
            out = ops.stream_step(spec, flat, xp, ms, read=k == len(chunks) - 1, logits=None if bufs is None else bufs[-2],
                                  probs=None if bufs is None else bufs[-1])
        return out

    chunks = [xd[:, :20].contiguous(), xd[:, 20:].contiguous()]
    ps0, ms0 = new_states()
    lg0, pr0 = run(ps0, ms0, chunks)
    want = pr.prep_ref(x, **_kw(p))
    # the eager pair against the window-mode front end and one stream step over all 41 samples
    ms1 = torch.full_like(ms0, NAN)
    ops.stream_reset(spec, ms1)
    lg1, pr1 = ops.stream_step(spec, flat, ops.prep_step(xd, p), ms1)
    assert torch.equal(ms0, ms1) and torch.equal(lg0, lg1) and torch.equal(pr0, pr1)
    refs = orc.forward(orc.flatten_state(ref_state, D), want, D)
    assert np.abs(lg0.cpu().numpy() - refs["logits"]).max() < LOGIT_TOL and np.abs(pr0.cpu().numpy() - refs["probs"]).max() < PROB_TOL
    # a side stream
    side = torch.cuda.Stream(device=dev)
    ps2, ms2 = new_states()
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        lg2, pr2 = run(ps2, ms2, chunks)
    side.synchronize()
    assert torch.equal(ps2, ps0) and torch.equal(ms2, ms0) and torch.equal(lg2, lg0) and torch.equal(pr2, pr0)
    # one captured graph of both chunks (prep step + stream step each), replayed: every replay advances both states by 41
    ps3, ms3 = new_states()
    bufs = [torch.full_like(c, NAN) for c in chunks] + [torch.full((B41, spec.K), NAN, device=dev) for _ in range(2)]
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(ps3, ms3, chunks, bufs)
    ops.prep_reset(8, ps3); ops.stream_reset(spec, ms3)                       # (whatever the capture did or did not run)
    for b in bufs:
        b.fill_(NAN)
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(ps3, ps0) and torch.equal(ms3, ms0) and torch.equal(bufs[-2], lg0) and torch.equal(bufs[-1], pr0)
    assert pr.same_bits(torch.cat(bufs[:2], 1).cpu().numpy(), want)
    graph.replay()
    torch.cuda.synchronize(dev)
    two = np.concatenate([x, x], 1)
    ref2 = pr.State(B41, 8)
    want2 = pr.prep_ref(two, state=ref2, **_kw(p))
    assert pr.same_bits(ps3.cpu().numpy(), ref2.slot_rows()) and pr.same_bits(torch.cat(bufs[:2], 1).cpu().numpy(), want2[:, T41:])


def test_reset_of_one_slot_leaves_the_others(nsd, dev):
    from nsd_amd import ops
    p = _configs(nsd)["full"]
    x = _raw(4, 20, 8)
    state, check = _new_state(dev, 8, 4)
    _run_cut(dev, x, p, [20], state)
    before = state.cpu().numpy()
    ops.prep_reset(8, state, torch.tensor([2, 9, -1], dtype=torch.int32, device=dev))      # indices outside [0, S) are skipped
    check("state")
    after = state.cpu().numpy()
    assert not after[2].any()
    for s in (0, 1, 3):
        assert after[s].tobytes() == before[s].tobytes(), s
    # the reset slot starts over; the others go on
    got = _run_cut(dev, x, p, [20], state)
    ref = pr.State(4, 8)
    pr.prep_ref(x, state=ref, **_kw(p))
    cont = pr.prep_ref(x, state=ref, **_kw(p))
    assert pr.same_bits(got[2], pr.prep_ref(x, **_kw(p))[2])
    for s in (0, 1, 3):
        assert pr.same_bits(got[s], cont[s]), s


def test_a_slot_index_outside_the_state_gives_nan_rows_and_touches_nothing(nsd, dev):
    p = _configs(nsd)["full"]
    x = _raw(4, 37, 8)
    for bad in (4, -1, 2**31 - 1, -2**31):
        state, check = _new_state(dev, 8, 4)
        slots = torch.tensor([1, bad, 0, 2], dtype=torch.int32, device=dev)
        got = _run_cut(dev, x, p, [37], state, slots=slots)                    # (y is guarded inside)
        check("state")
        assert np.isnan(got[1]).all(), bad
        want = pr.prep_ref(x[[0, 2, 3]], **_kw(p))
        assert pr.same_bits(got[[0, 2, 3]], want), bad
        ref = pr.State(3, 8)
        pr.prep_ref(x[[2, 0, 3]], state=ref, **_kw(p))                         # slot 0 <- stream 2, slot 1 <- stream 0, slot 2 <- stream 3
        assert pr.same_bits(state[:3].cpu().numpy(), ref.slot_rows()) and not state[3].any(), bad


@pytest.mark.parametrize("car", [False, True])
def test_a_nan_sample_poisons_its_channel_and_with_the_common_average_its_stream(nsd, dev, car):
    from nsd_amd import ops
    p = _design(nsd, 3, car=car, alpha=0.01, var0=300.0)
    x = _raw(3, 50, 8)
    x[1, 10, 4] = np.nan
    state, check = _new_state(dev, 8, 3)
    got = _run_cut(dev, x, p, [9, 3, 38], state)
    check("state")
    assert pr.same_bits(got, pr.prep_ref(x, **_kw(p)))
    nan = np.isnan(got)
    assert not nan[0].any() and not nan[2].any() and not nan[1, :10].any()    # only that stream, only from that sample on
    if car:
        assert nan[1, 10:].all()
    else:
        assert nan[1, 10:, 4].all() and not np.delete(nan[1], 4, axis=1).any()
    # it stays poisoned on clean samples until the slot is reset
    more = _raw(3, 5, 8, seed=4)
    assert np.isnan(_run_cut(dev, more, p, [5], state)[1, :, 4]).all()
    ops.prep_reset(8, state, torch.tensor([1], dtype=torch.int32, device=dev))
    again = _run_cut(dev, more, p, [5], state)
    assert pr.same_bits(again[1], pr.prep_ref(more, **_kw(p))[1])


# ---- through the Python layers ---------------------------------------------------------------------------------------------------------
def _prep(nsd):
    return nsd.CausalPrep.design(highpass=1.0, lowpass=40.0, zscore_seconds=0.4, var0=250.0)


def _eval_model(nsd, dev, ref_state, **kw):
    m = nsd.EEG_LSTM(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in ref_state.items()}, strict=True)
    return m.to(dev).eval()


def test_stream_decoder_with_prep_equals_a_plain_decoder_on_prepped_windows(nsd, dev, ref_state):
    from nsd_amd import ops
    P = _prep(nsd)
    x = _raw(B41, T41, 8)
    xd = to_dev(x, dev)
    with_prep, plain = _eval_model(nsd, dev, ref_state, prep=P), _eval_model(nsd, dev, ref_state)
    xp = ops.prep_step(xd, P)
    want = pr.prep_ref(x, **_kw(P))
    assert pr.same_bits(xp.cpu().numpy(), want)
    refs = sr.prefix_refs(orc.flatten_state(ref_state, D), want, D, range(1, T41 + 1))
    for cut in CUTS:
        a, b = nsd.StreamDecoder(with_prep, streams=4), nsd.StreamDecoder(plain, streams=4)
        t = 0
        for n in cut:
            pa, pb = a.push(xd[:, t:t + n]), b.push(xp[:, t:t + n])
            t += n
            assert torch.equal(pa, pb), (cut, t)
            assert np.abs(pa.cpu().numpy() - refs[t]["probs"]).max() < PROB_TOL, (cut, t)
        assert torch.equal(a.state, b.state) and list(a.steps) == [T41] * 3 + [0]
    # the logits of every prefix, through the ops
    ps, ms = ops.prep_state(8, B41, dev), ops.stream_state(with_prep.spec, B41, dev)
    t = 0
    for n in (7, 1, 33):
        lg, _ = ops.stream_step(with_prep.spec, with_prep.flat_parameters(), ops.prep_step(xd[:, t:t + n].contiguous(), P, ps), ms)
        t += n
        assert np.abs(lg.cpu().numpy() - refs[t]["logits"]).max() < LOGIT_TOL, t
    # reset and state_dict cover both states
    sd = a.state_dict()
    assert set(sd) == {"state", "stride", "prep_state"}
    c = nsd.StreamDecoder(with_prep, streams=4)
    c.load_state_dict(sd)
    more = _raw(4, 6, 8, seed=5)
    assert torch.equal(a.push(more), c.push(more)) and torch.equal(a.prep_state, c.prep_state)
    with pytest.raises(nsd.NsdError):
        nsd.StreamDecoder(plain, streams=4).load_state_dict(sd)
    a.reset([1])
    fresh = nsd.StreamDecoder(with_prep, streams=4)
    assert torch.equal(a.push(more[:1], slots=[1]), fresh.push(more[:1], slots=[1])) and not torch.equal(a.prep_state[0], fresh.prep_state[0])
    a.reset()
    assert not a.prep_state.any() and list(a.steps) == [0] * 4


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_the_model_runs_the_front_end_where_normalize_runs_its_zscore(nsd, dev, ref_state, precision):
    from nsd_amd import ops
    P = _prep(nsd)
    x = to_dev(_raw(8, 40, 8), dev)
    xp = ops.prep_step(x, P)
    if precision == "fp32":
        m, plain = _eval_model(nsd, dev, ref_state, prep=P), _eval_model(nsd, dev, ref_state)
        lg, probs = ops.infer(m.spec, m.flat_parameters(), xp)
        assert torch.equal(m.predict_proba(x), probs)
        with torch.no_grad():
            assert torch.equal(m(x), lg)
        # with autograd on the parameters: the training node sees the prepped windows
        m.train(); plain.train()
        m._mask_override = plain._mask_override = (None, None, None)
        la, lb = m(x).square().sum(), plain(xp).square().sum()
        la.backward(); lb.backward()
        assert torch.equal(la, lb)
        for (n, a), (_, b) in zip(m.named_parameters(), plain.named_parameters()):
            assert torch.equal(a.grad, b.grad), n
    else:
        kw = dict(input_size=8, hidden_size=64, num_layers=2, num_classes=3, precision="bf16")
        torch.manual_seed(3); m = nsd.EEG_LSTM(prep=P, **kw).to(dev).eval()
        torch.manual_seed(3); plain = nsd.EEG_LSTM(**kw).to(dev).eval()
        assert torch.equal(m.predict_proba(x), plain.predict_proba(xp))
        with torch.no_grad():
            assert torch.equal(m(x), plain(xp))
        y = torch.tensor([0, 1, 2, 1, 0, 2, 2, 1], dtype=torch.int32, device=dev)
        assert torch.equal(m.loss(x, y)[1], plain.loss(xp, y)[1])
    # dx through the front end is refused, never a silent None gradient
    xg = x.clone().requires_grad_(True)
    with pytest.raises(nsd.NsdError, match="dx through the causal front end"):
        m(xg)
    if precision == "bf16":
        with pytest.raises(nsd.NsdError, match="dx through the causal front end"):
            m.loss(xg, y)


def _model(nsd, dev, seed, **kw):
    torch.manual_seed(seed)
    return nsd.EEG_LSTM(**kw).to(dev).train()


def _batch(dev, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    x = 20.0 * torch.randn((B, T, 8), generator=g) + 5000.0 * (2 * torch.rand((B, 1, 8), generator=g) - 1)
    return x.to(dev), torch.randint(0, 3, (B,), generator=g, dtype=torch.int32).to(dev)


@pytest.mark.parametrize("augment", [False, True])
def test_trainer_step_equals_the_prep_free_step_on_prepped_windows(nsd, dev, augment):
    from nsd_amd import ops
    from nsd_amd.trainer import Trainer
    P = _prep(nsd)
    A = nsd.Augment(max_shift=5, scale_range=0.15, p_channel=0.2, noise_std=0.4) if augment else None
    ma, mb = _model(nsd, dev, 11, prep=P), _model(nsd, dev, 11)
    ta, tb = Trainer(ma, lr=1e-3, seed=9, augment=A), Trainer(mb, lr=1e-3, seed=9)
    for step in range(1, 3):
        x, y = _batch(dev, 16, 40, seed=step)
        ta.step(x, y)
        xa = ops.augment(x, A, dict(seed=tb.seed, base_stream=4 * step)) if augment else x       # augment -> prep, composed by hand
        tb.step(ops.prep_step(xa, P), y)
        assert torch.equal(ta.flat, tb.flat) and torch.equal(ta.m, tb.m) and torch.equal(ta.v, tb.v), step
        assert ta.last_loss() == tb.last_loss(), step
    assert not torch.equal(ta.flat, _model(nsd, dev, 11).flat_parameters())


def test_graph_replay_step_with_prep_equals_the_prep_free_replay_on_prepped_windows(nsd, dev):
    from nsd_amd import ops
    from nsd_amd.trainer import Trainer
    P, (B, T) = _prep(nsd), (16, 40)
    x, y = _batch(dev, B, T, seed=8)
    ma, mb = _model(nsd, dev, 21, prep=P), _model(nsd, dev, 21)
    ta, tb = Trainer(ma, lr=1e-3, seed=5), Trainer(mb, lr=1e-3, seed=5)
    (xa, ya), (xb, yb) = ta.static_inputs(B, T), tb.static_inputs(B, T)
    xa.copy_(x); ya.copy_(y); xb.copy_(ops.prep_step(x, P)); yb.copy_(y)
    for step in range(1, 3):
        ta.step_static(B, T)
        tb.step_static(B, T)
        assert torch.equal(ta._buffers(B, T)["xn"], xb) and "xn" not in tb._buffers(B, T), step
        assert torch.equal(ta.flat, tb.flat) and torch.equal(ta.grads, tb.grads), step
    assert torch.equal(xa, x)                                                   # the static input is not written


def test_model_batch_trainer_with_prep_equals_the_prep_free_one_on_prepped_windows(nsd, dev):
    from nsd_amd import ops
    P, M = _prep(nsd), 2
    with_prep = [_model(nsd, dev, 30 + m, prep=P) for m in range(M)]
    plain = [_model(nsd, dev, 30 + m) for m in range(M)]
    ta = nsd.ModelBatchTrainer(with_prep, lr=1e-3, seeds=[1, 2])
    tb = nsd.ModelBatchTrainer(plain, lr=1e-3, seeds=[1, 2])
    for step in range(1, 3):
        xs, ys = zip(*[_batch(dev, 8, 40, seed=10 * step + m) for m in range(M)])
        x, y = torch.stack(xs), torch.stack(ys)
        ta.step(x, y)
        tb.step(ops.prep_step(x, P), y)
        for m in range(M):
            for (n, a), (_, b) in zip(with_prep[m].state_dict().items(), plain[m].state_dict().items()):
                assert torch.equal(a, b), (step, m, n)
    with pytest.raises(nsd.NsdError):
        nsd.ModelBatchTrainer([_model(nsd, dev, 1, prep=P), _model(nsd, dev, 2)], lr=1e-3, seeds=[1, 2])


def test_a_checkpoint_with_prep_rebuilds_the_predictor_and_streams(nsd, dev, ref_state, tmp_path):
    from nsd_amd.trainer import save_reference_checkpoint
    P = _prep(nsd)
    model = _eval_model(nsd, dev, ref_state, prep=P)
    path = str(tmp_path / "prep.pth")
    save_reference_checkpoint(model, path)
    names = ["Food", "Water", "None"]
    pred = nsd.SimplePredictor(path, sr=125, device="cpu", class_names=names, preprocess="identity")
    assert pred.model.prep == P and torch.equal(pred.model.flat_parameters(), model.flat_parameters())
    x = _raw(2, 250, 8)
    whole = [pred.predict(w) for w in x]
    want = np.concatenate([model.predict_proba(to_dev(x[b:b + 1], dev)).cpu().numpy() for b in range(2)])
    for b in range(2):
        assert whole[b][0].tobytes() == want[b].tobytes() and whole[b][1] == names[int(want[b].argmax())]
    # 0.2 s chunks through open_stream: the decision after the last chunk is predict()'s, at the bound the resumable path is held to
    # against nsd_infer (the front end's output is bitwise the same on both routes, above; the readout's pooling is not nsd_infer's:
    # measured on 40 recorded windows max 1.5e-7, 7 of 40 bitwise equal)
    # what IS bitwise: the front end's output, chunk by chunk in the decoder's own state against window mode on the whole window
    from nsd_amd import ops
    xd, dec = to_dev(x, dev), nsd.StreamDecoder(pred.model, streams=2)
    fed = torch.cat([ops.prep_step(xd[:, t0:t0 + 25].contiguous(), P, dec.prep_state) for t0 in range(0, 250, 25)], 1)
    assert torch.equal(fed, ops.prep_step(xd, P)) and pr.same_bits(fed.cpu().numpy(), pr.prep_ref(x, **_kw(P)))
    st = pred.open_stream(streams=2)
    for t0 in range(0, 225, 25):
        assert st.push(x[:, t0:t0 + 25], read=False) is None
    probs, labels = st.push(x[:, 225:])
    assert list(st.steps) == [250, 250]
    assert np.abs(probs - want).max() < PROB_TOL and labels == [w[1] for w in whole]
    # the plain checkpoint is the plain predictor it always was
    plain_path = str(tmp_path / "plain.pth")
    save_reference_checkpoint(_eval_model(nsd, dev, ref_state), plain_path)
    assert nsd.SimplePredictor(plain_path, sr=125, device="cpu", preprocess="identity").model.prep is None
