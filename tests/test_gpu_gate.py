"""The signal-quality gate on the MI355X (nsd_gate_* of include/nsd.h, csrc/nsd_gate.hip) against its numpy restatement
(tests/gate_ref.py): y, the mask words and the whole state BIT FOR BIT (the NaN rows of a skipped stream and of a rejected step by
position).  Window mode over the shapes at which the kernel takes another path (the time tile of 32 steps, 64 / C streams per wave,
16-byte and dword staging, the grid cap), the threshold edges of every detector, stream mode over cuts, slots, HIP streams and a graph
replay, the apply stage, the buffer contract (every output of every call lies between 0xA5 guards, every input is checked unchanged),
and the path through the Python layers: the model, the decoders, the trainers and a checkpoint."""
import numpy as np
import pytest
import torch

from oracle import nsd_oracle as orc
from tests import gate_ref as gr
from tests import prep_ref as pr
from tests.buffer_contract import guarded, snapshot
from tests.gpu_harness import NAN, D, dev, nsd, spec_of, sync_at_the_end, to_dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

TILE = 32                        # PREP_TT of csrc/nsd_args.h: time steps staged through LDS at once
GRID_CAP = 1024                  # PREP_GRID_CAP: workgroups of a launch


def _configs(nsd):
    """each detector alone, all together (with a hang-over and a rejection bound), and nothing"""
    G = nsd.SignalGate
    return {
        "rail": G(rail=100.0),
        "jump": G(jump=60.0),
        "flat": G(flat_samples=4, flat_eps=0.25),
        "pp": G(pp=80.0, pp_samples=64),                  # the longest span: it crosses two tiles
        "pp_short": G(pp=50.0, pp_samples=5, hold_samples=2),
        "all": G(rail=100.0, jump=60.0, flat_samples=4, flat_eps=0.25, pp=80.0, pp_samples=64, hold_samples=3, max_bad=1),
        "off": G(),
    }


def _signal(B, T, Cc, seed=0):
    """EEG-like noise of 10 units with events of every kind: a railed sample, a step, a flat run, a swing inside the peak-to-peak span
    and a NaN, each on a (stream, channel) of its own where the shape has room, at n = 0, the last step of a tile, the first of the
    next, and the last sample of the call"""
    rs = np.random.RandomState(seed + 1000 * B + 10 * T + Cc)
    x = (10.0 * rs.standard_normal((B, T, Cc))).astype(np.float32)
    at = sorted({0, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, T - 1} & set(range(T)))
    k = 0
    for n in at:
        for kind in range(5):
            b, c = k % B, (k // B) % Cc
            k += 1
            if kind == 0:
                x[b, n, c] = -150.0
            elif kind == 1:
                x[b, n:, c] += 90.0
            elif kind == 2:
                x[b, n:n + 6, c] = x[b, n, c]
            elif kind == 3:
                x[b, n, c] = 45.0
                x[b, min(n + 3, T - 1), c] = -45.0
            else:
                x[b, n, c] = np.nan if k % 2 else np.inf
    return x


def _bits(mask):
    return mask.cpu().numpy().view(np.uint32)


def _window(dev, x_np, G, *, in_place=False, offset=0):
    """ops.gate_step in window mode into NaN-filled, guarded outputs (offset: y starts that many floats into its buffer: not 16-byte
    aligned) -> numpy (y, mask); the input is checked to be unchanged"""
    from nsd_amd import ops
    x = to_dev(x_np, dev)
    mask, check_m = guarded(x_np.shape[:2], torch.int32, dev, "nan32")
    if in_place:
        buf, check = guarded(x_np.shape, torch.float32, dev)
        buf.copy_(x)
        y, m = ops.gate_step(buf, G, out=buf, mask=mask)
        assert y is buf and m is mask
    else:
        flat, check = guarded((x_np.size + offset,), torch.float32, dev, "nan32")
        y = flat[offset:].view(x_np.shape)
        snap = snapshot(x)
        out, m = ops.gate_step(x, G, out=y, mask=mask)
        assert out is y and m is mask and snap.unchanged()
        assert offset == 0 or np.isnan(flat[:offset].cpu().numpy()).all()
    check("y")
    check_m("mask")
    return y.cpu().numpy(), _bits(mask)


def _same(got, want):
    """(y, mask) pairs: y bitwise (NaN rows by position), mask words equal"""
    return gr.same_bits(got[0], want[0]) and np.array_equal(got[1], want[1])


# (1,1,1); two full tiles and a tail with the 64-sample span crossing both; C that does not divide 64 with T * C % 4 != 0 (dword staging);
# the C limit and the full mask word
SHAPES = [(1, 1, 1), (3, 70, 8), (5, 33, 3), (2, 40, 32)]


@pytest.mark.parametrize("B,T,Cc", SHAPES)
def test_window_mode_and_the_state_equal_the_reference_bitwise(nsd, dev, B, T, Cc):
    x = _signal(B, T, Cc)
    fired = {}
    for name, G in _configs(nsd).items():
        want = gr.gate_ref(x, G.to_dict())
        assert _same(_window(dev, x, G), want), name
        fired[name] = int(want[1].astype(bool).sum())
        # stream mode in one call: the same outputs, and the whole state
        ref = gr.State(B, Cc)
        gr.gate_ref(x, G.to_dict(), ref)
        state, check = _new_state(dev, Cc, B)
        assert _same(_run_cut(dev, x, G, [T], state), want), name
        check("state")
        assert np.array_equal(state.cpu().numpy().view(np.uint32), ref.slot_rows()), name
    assert fired["off"] == int((~np.isfinite(x)).sum())                        # (a non-finite sample is bad whatever is configured)
    if T >= 40:
        assert all(fired[k] > 0 for k in ("rail", "jump", "flat", "pp", "pp_short", "all")), fired


def test_more_stream_groups_than_the_grid_cap(nsd, dev):
    B, T, Cc = 2 * GRID_CAP + 3, 2, 32                                         # 64 / 32 = 2 streams per group
    x = _signal(B, T, Cc)
    G = _configs(nsd)["all"]
    assert _same(_window(dev, x, G), gr.gate_ref(x, G.to_dict()))


def test_in_place_and_a_y_that_is_not_16_byte_aligned(nsd, dev):
    x = _signal(3, 70, 8)
    G = _configs(nsd)["all"]
    want = gr.gate_ref(x, G.to_dict())
    assert _same(_window(dev, x, G, in_place=True), want)
    for off in (1, 2, 3):
        assert _same(_window(dev, x, G, offset=off), want), off


def test_all_detectors_off_is_a_copy_with_a_zero_mask(nsd, dev):
    from nsd_amd import ops
    x = _signal(5, 40, 8)
    x[np.isnan(x) | np.isinf(x)] = 1.0                                         # (a non-finite sample is bad whatever is configured)
    x[0, 0, 0], x[2, 5, 1] = -0.0, 1e-42                                        # a negative zero and a denormal pass through
    G = nsd.SignalGate()
    y, mask = _window(dev, x, G)
    assert y.tobytes() == x.tobytes() and not mask.any()
    v = to_dev(x, dev)
    out, check = guarded(x.shape, torch.float32, dev, "nan32")
    ops.gate_apply(v, G, to_dev(mask.view(np.int32), dev), out=out)
    check("out")
    assert out.cpu().numpy().tobytes() == x.tobytes()


# ---- threshold edges -------------------------------------------------------------------------------------------------------------------
def _column(values):
    return np.asarray(values, np.float32).reshape(1, -1, 1)


def _mask_of(dev, x, G):
    got = _window(dev, x, G)
    assert _same(got, gr.gate_ref(x, G.to_dict()))
    return list(got[1][0] & 1)


def test_threshold_edges_of_every_detector(nsd, dev):
    """the hand-worked cases of tests/gate_ref.py: |x| == rail and the float below it, a flat run of flat_samples - 1 and of
    flat_samples, an extreme sample pp_samples - 1 and pp_samples steps old, the hang-over"""
    for kw, samples, want in gr.HAND_CASES:
        assert _mask_of(dev, _column(samples), nsd.SignalGate(**kw)) == list(want), kw


def test_a_hang_over_running_out_around_a_cut(nsd, dev):
    Gt = nsd.SignalGate(rail=100.0, hold_samples=5)
    x = _signal(2, 40, 4)
    x[np.isnan(x) | np.isinf(x)] = 0.0
    x = np.clip(x, -50, 50)
    x[0, 20, 1] = 300.0                                                        # bad 20 .. 25
    want = gr.gate_ref(x, Gt.to_dict())
    assert list(want[1][0, 19:28]) == [0] + [2] * 6 + [0, 0]
    for cut in ([25, 15], [26, 14], [27, 13], [21, 19]):                       # the last bad sample before / after the cut
        state, check = _new_state(dev, 4, 2)
        assert _same(_run_cut(dev, x, Gt, cut, state), want), cut
        check("state")


def test_a_non_finite_sample_is_held_and_the_front_end_behind_stays_finite(nsd, dev):
    from nsd_amd import ops
    Gt = nsd.SignalGate(hold_samples=2)
    P = nsd.CausalPrep.design(highpass=1.0, lowpass=40.0, zscore_seconds=0.4, var0=250.0, car=True)
    x = np.clip(_signal(3, 50, 8), -50, 50)
    x[np.isnan(x)] = 0.0
    x[1, 10, 4], x[1, 30, 2], x[2, 0, 0] = np.nan, -np.inf, np.inf
    y, mask = _window(dev, x, Gt)
    assert _same((y, mask), gr.gate_ref(x, Gt.to_dict()))
    assert np.isfinite(y).all() and y[1, 10, 4] == x[1, 9, 4] and y[2, 0, 0] == 0.0     # the held value; 0 after a reset
    assert list(mask[1, 9:14]) == [0, 16, 16, 16, 0] and mask[2, 0] == 1
    assert np.isfinite(ops.prep_step(to_dev(y, dev), P).cpu().numpy()).all()
    assert np.isnan(ops.prep_step(to_dev(x, dev), P).cpu().numpy()[1, 10:]).all()          # what the gate is for


# ---- stream mode -----------------------------------------------------------------------------------------------------------------------
def _new_state(dev, Cc, S):
    """S slots between guards, NaN-filled, then reset through the library -> (state, check)"""
    from nsd_amd import ops
    state, check = guarded((S, int(ops.gate_layout(Cc).stride)), torch.float32, dev, "nan32")
    ops.gate_reset(Cc, state)
    return state, check


def _run_cut(dev, x_np, G, cut, state, slots=None):
    """the chunks of `cut` through ops.gate_step in stream mode, each into NaN-filled guarded outputs -> numpy (y [B,T,C], mask [B,T])"""
    from nsd_amd import ops
    ys, ms, t = [], [], 0
    for n in cut:
        xc = to_dev(x_np[:, t:t + n], dev)
        y, check = guarded(xc.shape, torch.float32, dev, "nan32")
        mask, check_m = guarded(xc.shape[:2], torch.int32, dev, "nan32")
        snap = snapshot(xc, slots)
        out = ops.gate_step(xc, G, state, slots=slots, out=y, mask=mask)
        assert out[0] is y and out[1] is mask and snap.unchanged()
        check("y")
        check_m("mask")
        ys.append(y.cpu().numpy())
        ms.append(_bits(mask))
        t += n
    return np.concatenate(ys, 1), np.concatenate(ms, 1)


T70, B70 = 70, 3
CUTS = ([70], [1] * 70, [7] * 10, [32, 32, 6], [33, 33, 4])


@pytest.mark.parametrize("name", ["all", "pp", "flat"])
def test_cuts_slots_and_neighbours_do_not_show(nsd, dev, name):
    G = _configs(nsd)[name]
    x = _signal(B70, T70, 8)
    want = gr.gate_ref(x, G.to_dict())
    ref = gr.State(B70, 8)
    gr.gate_ref(x, G.to_dict(), ref)
    rows = ref.slot_rows()
    assert _same(_window(dev, x, G), want)
    blank, _ = _new_state(dev, 8, 1)
    assert not blank.cpu().numpy().view(np.uint32).any()                       # a reset slot is all zero
    for cut in CUTS:
        state, check = _new_state(dev, 8, B70)
        assert _same(_run_cut(dev, x, G, cut, state), want), cut
        check("state")
        assert np.array_equal(state.cpu().numpy().view(np.uint32), rows), cut
    # permuted slots inside a larger state, with other streams in the same calls
    S, perm = 7, [5, 0, 3, 6, 2]
    other = _signal(2, T70, 8, seed=9)
    state, check = _new_state(dev, 8, S)
    slots = torch.tensor(perm, dtype=torch.int32, device=dev)
    got = _run_cut(dev, np.concatenate([x, other]), G, [7, 1, 32, 30], state, slots=slots)
    check("state")
    assert _same((got[0][:B70], got[1][:B70]), want) and _same((got[0][B70:], got[1][B70:]), gr.gate_ref(other, G.to_dict()))
    st = state.cpu().numpy().view(np.uint32)
    for b in range(B70):
        assert np.array_equal(st[perm[b]], rows[b]), b
    assert not st[1].any() and not st[4].any()                                 # slots nobody named stay reset


def test_reset_of_one_slot_leaves_the_others(nsd, dev):
    from nsd_amd import ops
    G = _configs(nsd)["all"]
    x = _signal(4, 20, 8)
    state, check = _new_state(dev, 8, 4)
    _run_cut(dev, x, G, [20], state)
    before = state.cpu().numpy().view(np.uint32)
    ops.gate_reset(8, state, torch.tensor([2, 9, -1], dtype=torch.int32, device=dev))      # indices outside [0, S) are skipped
    check("state")
    after = state.cpu().numpy().view(np.uint32)
    assert not after[2].any()
    for s in (0, 1, 3):
        assert np.array_equal(after[s], before[s]), s
    got = _run_cut(dev, x, G, [20], state)                                     # the reset slot starts over; the others go on
    ref = gr.State(4, 8)
    gr.gate_ref(x, G.to_dict(), ref)
    cont = gr.gate_ref(x, G.to_dict(), ref)
    fresh = gr.gate_ref(x, G.to_dict())
    assert _same((got[0][2], got[1][2]), (fresh[0][2], fresh[1][2]))
    for s in (0, 1, 3):
        assert _same((got[0][s], got[1][s]), (cont[0][s], cont[1][s])), s


def test_a_slot_index_outside_the_state_gives_nan_rows_an_all_ones_mask_and_touches_nothing(nsd, dev):
    G = _configs(nsd)["all"]
    x = _signal(4, 37, 8)
    for bad in (4, -1, 2**31 - 1, -2**31):
        state, check = _new_state(dev, 8, 4)
        slots = torch.tensor([1, bad, 0, 2], dtype=torch.int32, device=dev)
        y, mask = _run_cut(dev, x, G, [37], state, slots=slots)
        check("state")
        assert np.isnan(y[1]).all() and (mask[1] == 0xFFFFFFFF).all(), bad
        want = gr.gate_ref(x[[0, 2, 3]], G.to_dict())
        assert _same((y[[0, 2, 3]], mask[[0, 2, 3]]), want), bad
        ref = gr.State(3, 8)
        gr.gate_ref(x[[2, 0, 3]], G.to_dict(), ref)                            # slot 0 <- stream 2, slot 1 <- stream 0, slot 2 <- stream 3
        st = state.cpu().numpy().view(np.uint32)
        assert np.array_equal(st[:3], ref.slot_rows()) and not st[3].any(), bad


# ---- the apply stage -------------------------------------------------------------------------------------------------------------------
def _apply(dev, v_np, mask_np, G, *, in_place=False, max_bad=None):
    from nsd_amd import ops
    v, mask = to_dev(v_np, dev), to_dev(mask_np.view(np.int32), dev)
    out, check = guarded(v_np.shape, torch.float32, dev, "nan32")
    if in_place:
        out.copy_(v)
        snap = snapshot(mask)
        assert ops.gate_apply(out, G, mask, out=out, max_bad=max_bad) is out
    else:
        snap = snapshot(v, mask)
        assert ops.gate_apply(v, G, mask, out=out, max_bad=max_bad) is out
    assert snap.unchanged()
    check("out")
    return out.cpu().numpy()


@pytest.mark.parametrize("B,T,Cc", [(3, 70, 8), (5, 33, 3), (2, 40, 32), (1, 1, 1)])
def test_apply_equals_the_reference_with_and_without_zeroing(nsd, dev, B, T, Cc):
    rs = np.random.RandomState(B + T + Cc)
    v = rs.standard_normal((B, T, Cc)).astype(np.float32)
    v[0, 0, 0] = -0.0
    mask = (rs.randint(0, 2**32, (B, T), dtype=np.uint64).astype(np.uint32) & rs.randint(0, 2**32, (B, T), dtype=np.uint64).astype(np.uint32)
            & np.uint32((1 << Cc) - 1 if Cc < 32 else 0xFFFFFFFF))
    mask[:, ::3] = 0
    for max_bad in (0, 1, Cc // 2, Cc, 32):
        for zero in (True, False):
            G = nsd.SignalGate(max_bad=max_bad, zero=zero)
            want = gr.apply_ref(v, mask, G.to_dict())
            assert gr.same_bits(_apply(dev, v, mask, G), want), (max_bad, zero)
            assert gr.same_bits(_apply(dev, v, mask, G, in_place=True), want), (max_bad, zero)
            if max_bad >= Cc:
                assert not np.isnan(want).any()                                 # max_bad >= C never rejects
    # the max_bad argument replaces the gate's
    G = nsd.SignalGate(max_bad=0)
    assert gr.same_bits(_apply(dev, v, mask, G, max_bad=Cc), gr.apply_ref(v, mask, dict(G.to_dict(), max_bad=Cc)))


def test_apply_rejects_above_max_bad_and_passes_at_it(nsd, dev):
    v = np.ones((1, 4, 8), np.float32)
    mask = np.array([[0b0, 0b101, 0b10101, 0b11111111]], np.uint32)            # 0, 2, 3 and 8 bad channels
    out = _apply(dev, v, mask, nsd.SignalGate(max_bad=2))
    assert not np.isnan(out[0, :2]).any() and np.isnan(out[0, 2:]).all()
    assert list(out[0, 1]) == [0, 1, 0, 1, 1, 1, 1, 1]
    out = _apply(dev, v, mask, nsd.SignalGate(max_bad=2, zero=False))
    assert out[0, :2].tobytes() == v[0, :2].tobytes() and np.isnan(out[0, 2:]).all()
    out = _apply(dev, v, mask, nsd.SignalGate(max_bad=8))
    assert not np.isnan(out).any() and not out[0, 3].any()


# ---- side stream and graph replay ------------------------------------------------------------------------------------------------------
def _prep(nsd):
    return nsd.CausalPrep.design(highpass=1.0, lowpass=40.0, zscore_seconds=0.4, var0=250.0, car=True)


def _stream_signal(B, T, seed=3):
    """clean noise of 10 units on 8 channels with: stream 0 railed on channel 2 from sample 30 on (one bad channel: held, then zeroed),
    stream 1 a pop on three channels at sample 37 (too many bad channels: with a hang-over of 2 samples the steps 37 .. 39 are
    rejected), every other stream clean"""
    x = np.clip(10.0 * np.random.RandomState(seed).standard_normal((B, T, 8)), -40, 40).astype(np.float32)
    x[0, 30:, 2] = 3000.0
    if B > 1 and T > 37:
        x[1, 37, 1:4] = 500.0
    return x


def _np_eq(a, b):
    return gr.same_bits(a.detach().cpu().numpy(), b.detach().cpu().numpy())


def test_graph_replay_of_gate_prep_apply_and_window_step_on_a_side_stream(nsd, dev, ref_state):
    from nsd_amd import ops
    G, P = nsd.SignalGate(rail=100.0, hold_samples=2, max_bad=2), _prep(nsd)
    spec, flat = spec_of(D), to_dev(orc.flatten_state(ref_state, D), dev)
    W, HOP, n, B = 20, 10, 10, 2
    x = _stream_signal(B, 6 * n)
    chunks = [to_dev(x[:, k * n:(k + 1) * n], dev) for k in range(6)]
    rows = ops.window_rows(n, W, HOP)

    def new():
        st = dict(g=ops.gate_state(8, B, dev), p=ops.prep_state(8, B, dev), w=ops.window_state(spec, W, HOP, B, dev))
        bufs = dict(y=torch.full((B, n, 8), NAN, device=dev), m=torch.zeros((B, n), dtype=torch.int32, device=dev),
                    p=torch.full((B, n, 8), NAN, device=dev),
                    out=(torch.full((B, rows, spec.K), NAN, device=dev), torch.full((B, rows, spec.K), NAN, device=dev),
                         torch.zeros((B, rows), dtype=torch.int64, device=dev), torch.zeros((B,), dtype=torch.int32, device=dev)))
        return st, bufs

    def step(xc, st, bufs):
        y, m = ops.gate_step(xc, G, st["g"], out=bufs["y"], mask=bufs["m"])
        v = ops.prep_step(y, P, st["p"], out=bufs["p"])
        ops.gate_apply(v, G, m, out=v)
        return ops.window_step(spec, flat, v, st["w"], window=W, hop=HOP, out=bufs["out"])

    def snap(bufs):
        return [t.clone() for t in (bufs["p"], bufs["m"]) + tuple(bufs["out"])]

    st0, b0 = new()
    eager = []
    for xc in chunks:
        step(xc, st0, b0)
        eager.append(snap(b0))
    # the eager run is the restatement's: the mask words, and the rejected step of stream 1 poisons exactly the windows that contain it
    want = gr.gate_ref(x, G.to_dict())
    assert np.array_equal(np.concatenate([_bits(e[1]) for e in eager], 1), want[1])
    lost = {0: [], 1: []}                                                      # per stream: the ends of the windows without a decision
    done = 0
    for e in eager:
        probs, ends, counts = (t.cpu().numpy() for t in e[3:])
        for s in range(B):
            for i in range(int(counts[s])):
                done += 1
                if np.isnan(probs[s, i]).any():
                    lost[s].append(int(ends[s, i]))
    assert done == 2 * 5 and lost == {0: [], 1: [40, 50]}                     # the steps 37 .. 39 lie in the windows that end at 40 and 50
    st1, b1 = new()
    xin = torch.zeros((B, n, 8), device=dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step(xin, st1, b1)
    ops.gate_reset(8, st1["g"]); ops.prep_reset(8, st1["p"]); ops.window_reset(spec, W, HOP, st1["w"])   # (whatever the capture ran)
    torch.cuda.synchronize(dev)
    for k, xc in enumerate(chunks):
        with torch.cuda.stream(side):
            xin.copy_(xc)
            graph.replay()
            got = snap(b1)
        side.synchronize()
        for a, b in zip(got, eager[k]):
            assert (_np_eq(a, b) if a.is_floating_point() else torch.equal(a, b)), k
    for key in st0:
        assert np.array_equal(st0[key].cpu().numpy().view(np.uint32), st1[key].cpu().numpy().view(np.uint32)), key


# ---- through the Python layers ---------------------------------------------------------------------------------------------------------
def _eval_model(nsd, dev, ref_state, scale=1.0, **kw):
    m = nsd.EEG_LSTM(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v) * np.float32(scale)) for k, v in ref_state.items()}, strict=True)
    return m.to(dev).eval()


def _hand(x, G, P, max_bad=None):
    """apply(prep(gate(x))) over whole windows, made with the ops calls"""
    from nsd_amd import ops
    y, mask = ops.gate_step(x, G)
    v = ops.prep_step(y, P) if P is not None else y
    return ops.gate_apply(v, G, mask, max_bad=max_bad)


T70_CUTS = ([70], [7, 1, 32, 30], [33, 33, 4])


@pytest.mark.parametrize("with_prep", [False, True])
def test_stream_decoders_with_a_gate_equal_gate_free_ones_on_hand_gated_chunks(nsd, dev, ref_state, with_prep):
    G, P = nsd.SignalGate(rail=100.0, hold_samples=2, max_bad=2), (_prep(nsd) if with_prep else None)
    B, T = 3, 70
    x = _stream_signal(B, T)
    xd = to_dev(x, dev)
    hand = _hand(xd, G, P)
    assert np.isnan(hand[1, 37].cpu().numpy()).all() and not np.isnan(hand[[0, 2]].cpu().numpy()).any()
    assert not hand[0, 30:, 2].any() and np.isnan(hand.cpu().numpy()).sum() == 3 * 8      # zeroed; the rejected steps 37 .. 39
    gated, plain = _eval_model(nsd, dev, ref_state, gate=G, prep=P), _eval_model(nsd, dev, ref_state)
    ref = gr.State(B, 8)
    gr.gate_ref(x, G.to_dict(), ref)
    for cut in T70_CUTS:
        a, b = nsd.StreamDecoder(gated, streams=4), nsd.StreamDecoder(plain, streams=4)
        t = 0
        for n in cut:
            pa, pb = a.push(xd[:, t:t + n]), b.push(hand[:, t:t + n])
            t += n
            assert _np_eq(pa, pb), (cut, t)
            assert np.isnan(pa[1].cpu().numpy()).all() == (t > 37), (cut, t)             # the cumulative decoder reads NaN from there on
        assert np.isfinite(pa[[0, 2]].cpu().numpy()).all()
        assert _np_eq(a.state, b.state) and list(a.steps) == [T] * 3 + [0]
        q = a.quality()
        want = ref.quality()
        assert np.array_equal(q["bad_fraction"][:3], want["bad_fraction"]) and np.array_equal(q["rejected_fraction"][:3], want["rejected_fraction"])
        assert list(q["steps"]) == [T] * 3 + [0] and not q["bad_fraction"][3].any()
        assert q["rejected_fraction"][1] == 3 / T and q["bad_fraction"][0, 2] == 40 / T
        one = a.quality(slots=[2, 0])
        assert np.array_equal(one["bad_fraction"], q["bad_fraction"][[2, 0]]) and list(one["steps"]) == [T, T]
    # state_dict / load_state_dict / reset cover the gate state
    sd = a.state_dict()
    assert set(sd) == {"state", "stride", "gate_state"} | ({"prep_state"} if with_prep else set())
    c = nsd.StreamDecoder(gated, streams=4)
    c.load_state_dict(sd)
    more = to_dev(_stream_signal(4, 6, seed=5), dev)
    assert _np_eq(a.push(more), c.push(more)) and torch.equal(a.gate_state.view(torch.int32), c.gate_state.view(torch.int32))
    with pytest.raises(nsd.NsdError, match="signal-quality gate"):
        nsd.StreamDecoder(_eval_model(nsd, dev, ref_state, prep=P), streams=4).load_state_dict(sd)
    with pytest.raises(nsd.NsdError, match="no signal-quality gate"):
        nsd.StreamDecoder(plain, streams=4).quality()
    a.reset([1])                                                               # the poisoned stream starts over
    fresh = nsd.StreamDecoder(gated, streams=4)
    pa, pf = a.push(more[:1], slots=[1]), fresh.push(more[:1], slots=[1])
    assert _np_eq(pa, pf) and np.isfinite(pa.cpu().numpy()).all()
    assert list(a.quality()["steps"]) == [T + 6, 6, T + 6, 6]
    a.reset()
    assert not a.gate_state.view(torch.int32).any() and list(a.steps) == [0] * 4
    # an ensemble of two: one gate state, its output read by both models
    g2 = [_eval_model(nsd, dev, ref_state, gate=G, prep=P), _eval_model(nsd, dev, ref_state, scale=0.9, gate=G, prep=P)]
    p2 = [_eval_model(nsd, dev, ref_state), _eval_model(nsd, dev, ref_state, scale=0.9)]
    ea, eb = nsd.EnsembleStreamDecoder(g2, streams=3), nsd.EnsembleStreamDecoder(p2, streams=3)
    t = 0
    for n in (7, 1, 32, 30):
        pa, pb = ea.push(xd[:, t:t + n]), eb.push(hand[:, t:t + n])
        t += n
        assert _np_eq(pa, pb) and _np_eq(ea.member_probs, eb.member_probs), t
    assert np.array_equal(ea.quality()["bad_fraction"], ref.quality()["bad_fraction"])
    with pytest.raises(nsd.NsdError):
        nsd.EnsembleStreamDecoder([g2[0], _eval_model(nsd, dev, ref_state, scale=0.9, prep=P)], streams=3)


def test_a_rejected_step_costs_the_sliding_decoder_exactly_the_windows_that_contain_it(nsd, dev, ref_state):
    G = nsd.SignalGate(rail=100.0, max_bad=0)                                  # any bad channel rejects the step
    W, HOP, B, T = 20, 10, 2, 70
    x = np.clip(10.0 * np.random.RandomState(7).standard_normal((B, T, 8)), -40, 40).astype(np.float32)
    x[0, 37, 3] = 300.0                                                        # sample 37 (0-based): inside the windows that end at 40 and 50
    raw = x.copy()
    raw[0, 37, 3] = 30.0                                                       # the ungated run sees a harmless sample there
    gated, plain = _eval_model(nsd, dev, ref_state, gate=G), _eval_model(nsd, dev, ref_state)
    a = nsd.SlidingStreamDecoder(gated, streams=B, window=W, hop=HOP)
    b = nsd.SlidingStreamDecoder(plain, streams=B, window=W, hop=HOP)
    t = 0
    seen = []
    for n in (7, 33, 30):
        pa, ea, ca = (v.cpu().numpy().copy() for v in a.push(to_dev(x[:, t:t + n], dev)))
        pb, eb, cb = (v.cpu().numpy().copy() for v in b.push(to_dev(raw[:, t:t + n], dev)))
        t += n
        assert np.array_equal(ea, eb) and np.array_equal(ca, cb), t           # counts and ends are unchanged
        for s in range(B):
            for i in range(int(ca[s])):
                e = int(ea[s, i])
                hit = s == 0 and e - W <= 37 <= e - 1
                seen.append((s, e, hit))
                if hit:
                    assert np.isnan(pa[s, i]).all(), (s, e)
                else:
                    assert pa[s, i].tobytes() == pb[s, i].tobytes(), (s, e)       # every other window has the bits of the ungated run
    assert sorted(e for s, e, hit in seen if hit) == [40, 50] and len(seen) == 2 * 6
    q = a.quality()
    assert list(q["steps"]) == [T, T] and q["rejected_fraction"][0] == 1 / T and q["rejected_fraction"][1] == 0
    assert a.latest()[0][0] == 70 and np.isfinite(a.latest()[0][1]).all()      # the stream healed on its own


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_the_model_runs_gate_prep_apply_wherever_its_front_end_runs(nsd, dev, ref_state, precision):
    from nsd_amd import ops
    G, P = nsd.SignalGate(rail=100.0, hold_samples=2, max_bad=2), _prep(nsd)
    x = to_dev(_stream_signal(8, 40), dev)
    hand = _hand(x, G, P)
    assert np.isnan(hand[1].cpu().numpy()).any()
    if precision == "fp32":
        m, plain = _eval_model(nsd, dev, ref_state, gate=G, prep=P), _eval_model(nsd, dev, ref_state)
    else:
        kw = dict(input_size=8, hidden_size=64, num_layers=2, num_classes=3, precision="bf16")
        torch.manual_seed(3); m = nsd.EEG_LSTM(gate=G, prep=P, **kw).to(dev).eval()
        torch.manual_seed(3); plain = nsd.EEG_LSTM(**kw).to(dev).eval()
    pa = m.predict_proba(x)
    assert _np_eq(pa, plain.predict_proba(hand))
    assert np.isnan(pa[1].cpu().numpy()).all() and np.isfinite(pa[[0, 2, 3]].cpu().numpy()).all()       # "no decision" for the rejected trial
    with torch.no_grad():
        assert _np_eq(m(x), plain(hand))
    ta, wa = m.predict_trials(x, window=20, hop=10)
    tb, wb = plain.predict_trials(hand, window=20, hop=10)
    assert _np_eq(ta, tb) and _np_eq(wa, wb)
    if precision == "fp32":
        # train mode never rejects: the training node sees the gated windows with every step kept
        m.train(); plain.train()
        m._mask_override = plain._mask_override = (None, None, None)
        la, lb = m(x).square().sum(), plain(_hand(x, G, P, max_bad=8)).square().sum()
        la.backward(); lb.backward()
        assert torch.equal(la, lb) and bool(torch.isfinite(la))
        for (n, a), (_, b) in zip(m.named_parameters(), plain.named_parameters()):
            assert torch.equal(a.grad, b.grad), n
    xg = x.clone().requires_grad_(True)
    with pytest.raises(nsd.NsdError, match="dx through the signal-quality gate"):
        m(xg)
    # a gate without a front end behind it
    only = _eval_model(nsd, dev, ref_state, gate=G) if precision == "fp32" else None
    if only is not None:
        assert _np_eq(only.predict_proba(x), _eval_model(nsd, dev, ref_state).predict_proba(_hand(x, G, None)))


def _model(nsd, dev, seed, **kw):
    torch.manual_seed(seed)
    return nsd.EEG_LSTM(**kw).to(dev).train()


def _batch(dev, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    x = (10.0 * torch.randn((B, T, 8), generator=g)).clamp_(-40, 40)
    x[0, 10:, 2] = 3000.0                                                      # a railed channel
    x[1, 20, 1:5] = 500.0                                                      # a pop on four channels: rejected outside a training step
    return x.to(dev), torch.randint(0, 3, (B,), generator=g, dtype=torch.int32).to(dev)


def test_trainer_steps_with_a_gate_equal_gate_free_steps_on_hand_gated_windows(nsd, dev):
    from nsd_amd.trainer import Trainer
    G, P, (B, T) = nsd.SignalGate(rail=100.0, hold_samples=2, max_bad=2), _prep(nsd), (4, 40)
    # Trainer.step
    ma, mb = _model(nsd, dev, 11, gate=G, prep=P), _model(nsd, dev, 11)
    ta, tb = Trainer(ma, lr=1e-3, seed=9), Trainer(mb, lr=1e-3, seed=9)
    for step in range(1, 3):
        x, y = _batch(dev, B, T, seed=step)
        hand = _hand(x, G, P, max_bad=8)                                       # inside a training step nothing is rejected
        assert np.isfinite(hand.cpu().numpy()).all() and np.isnan(_hand(x, G, P).cpu().numpy()).any()
        ta.step(x, y)
        tb.step(hand, y)
        assert torch.equal(ta.flat, tb.flat) and torch.equal(ta.m, tb.m) and torch.equal(ta.v, tb.v), step
        assert ta.last_loss() == tb.last_loss() and np.isfinite(ta.last_loss()), step
    assert not torch.equal(ta.flat, _model(nsd, dev, 11).flat_parameters())
    # the replayed step
    x, y = _batch(dev, B, T, seed=8)
    ma, mb = _model(nsd, dev, 21, gate=G), _model(nsd, dev, 21)
    ta, tb = Trainer(ma, lr=1e-3, seed=5), Trainer(mb, lr=1e-3, seed=5)
    (xa, ya), (xb, yb) = ta.static_inputs(B, T), tb.static_inputs(B, T)
    xa.copy_(x); ya.copy_(y); xb.copy_(_hand(x, G, None, max_bad=8)); yb.copy_(y)
    for step in range(1, 3):
        ta.step_static(B, T)
        tb.step_static(B, T)
        assert torch.equal(ta._buffers(B, T)["xn"], xb) and "gm" not in tb._buffers(B, T), step
        assert torch.equal(ta.flat, tb.flat) and torch.equal(ta.grads, tb.grads), step
    assert torch.equal(xa, x)                                                   # the static input is not written
    # ModelBatchTrainer, M = 2
    M = 2
    gated = [_model(nsd, dev, 30 + m, gate=G, prep=P) for m in range(M)]
    plain = [_model(nsd, dev, 30 + m) for m in range(M)]
    ta = nsd.ModelBatchTrainer(gated, lr=1e-3, seeds=[1, 2])
    tb = nsd.ModelBatchTrainer(plain, lr=1e-3, seeds=[1, 2])
    for step in range(1, 3):
        xs, ys = zip(*[_batch(dev, B, T, seed=10 * step + m) for m in range(M)])
        x, y = torch.stack(xs), torch.stack(ys)
        ta.step(x, y)
        tb.step(_hand(x, G, P, max_bad=8), y)
        for m in range(M):
            for (n, a), (_, b) in zip(gated[m].state_dict().items(), plain[m].state_dict().items()):
                assert torch.equal(a, b), (step, m, n)
    with pytest.raises(nsd.NsdError):
        nsd.ModelBatchTrainer([_model(nsd, dev, 1, gate=G), _model(nsd, dev, 2)], lr=1e-3, seeds=[1, 2])


def test_a_checkpoint_with_gate_and_prep_rebuilds_the_predictor_and_streams(nsd, dev, ref_state, tmp_path):
    from nsd_amd.trainer import save_reference_checkpoint
    from tests.gpu_harness import PROB_TOL
    G, P = nsd.SignalGate(rail=100.0, hold_samples=2, max_bad=2), _prep(nsd)
    model = _eval_model(nsd, dev, ref_state, gate=G, prep=P)
    path = str(tmp_path / "gate.pth")
    save_reference_checkpoint(model, path)
    names = ["Food", "Water", "None"]
    pred = nsd.SimplePredictor(path, sr=125, device="cpu", class_names=names, preprocess="identity")
    assert pred.model.gate == G and pred.model.prep == P and torch.equal(pred.model.flat_parameters(), model.flat_parameters())
    x = _stream_signal(2, 250)[[0, 0]]                                          # two streams of the railed-channel trial: no rejection
    x[1, 30:, 2] = x[1, 29, 2]
    want = np.concatenate([model.predict_proba(to_dev(x[b:b + 1], dev)).cpu().numpy() for b in range(2)])
    whole = [pred.predict(w) for w in x]
    for b in range(2):
        assert whole[b][0].tobytes() == want[b].tobytes() and whole[b][1] == names[int(want[b].argmax())]
    st = pred.open_stream(streams=2)
    for t0 in range(0, 225, 25):
        assert st.push(x[:, t0:t0 + 25], read=False) is None
    probs, labels = st.push(x[:, 225:])
    assert list(st.steps) == [250, 250]
    assert np.abs(probs - want).max() < PROB_TOL and labels == [w[1] for w in whole]
    q = st.decoder.quality()
    assert q["bad_fraction"][0, 2] == 220 / 250 and not q["rejected_fraction"].any()
    plain_path = str(tmp_path / "plain.pth")
    save_reference_checkpoint(_eval_model(nsd, dev, ref_state), plain_path)
    assert nsd.SimplePredictor(plain_path, sr=125, device="cpu", preprocess="identity").model.gate is None


def test_screen_trials_on_the_device_equals_the_host_route(nsd, dev, golden):
    from nsd_amd import data as Dt
    x = golden("real_trials")["x"].copy()
    x[3, 200:, 5] = 4000.0
    x[7, 100:140, :3] += 500.0
    G = nsd.SignalGate.design(rail=1000.0, pp=100.0, hold_seconds=0.1, max_bad_channels=2)
    bad, rejected = Dt.screen_trials(to_dev(x, dev), G)
    hb, hr = Dt.screen_trials(x, G)
    assert np.array_equal(bad, hb) and np.array_equal(rejected, hr) and rejected[7] > 0 and bad[3, 5] == 425 / 625
