"""CPU-side checks of the signal-quality gate (no GPU): the numpy restatement of tests/gate_ref.py against hand-worked cases and against
SignalGate.reference (written the other way round: whole windows, no ring), SignalGate's design / dictionary / struct, every refusal
of the nsd_gate_* entry points through the C ABI, the model's refusals, and data.screen_trials' bookkeeping on recorded trials."""
import ctypes as C
import os

import numpy as np
import pytest

import nsd_amd
from nsd_amd import _lib
from nsd_amd import data as D
from tests import gate_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_WORKSPACE = -1, -3
FAKE = 4096                      # a pointer that is never dereferenced: every refusal comes before any launch


@pytest.mark.parametrize("case", range(len(gr.HAND_CASES)))
def test_the_restatement_gives_the_hand_worked_masks(case):
    kw, samples, want = gr.HAND_CASES[case]
    x = np.asarray(samples, np.float32).reshape(1, -1, 1)
    y, mask = gr.gate_ref(x, gr.config(**kw))
    assert list(mask[0]) == list(want), kw
    # y: the sample itself where it is good, the last good one (0 before the first) where it is bad
    held, expect = np.float32(0.0), []
    for v, bad in zip(x[0, :, 0], want):
        held = held if bad else v
        expect.append(held)
    assert y[0, :, 0].tobytes() == np.asarray(expect, np.float32).tobytes(), kw
    assert np.isfinite(y).all()


def test_the_hang_over_and_the_counters_of_the_restatement():
    x = np.zeros((1, 12, 2), np.float32)
    x[0, 4, 0] = 200.0
    x[0, 5, 1] = -300.0
    st = gr.State(1, 2)
    y, mask = gr.gate_ref(x, gr.config(rail=100.0, hold_samples=3, max_bad=1), st)
    assert list(mask[0]) == [0, 0, 0, 0, 1, 3, 3, 3, 2, 0, 0, 0]
    assert list(st.bad[0]) == [4, 4] and int(st.rejected[0]) == 3 and int(st.n[0]) == 12
    q = st.quality()
    assert np.allclose(q["bad_fraction"], [[4 / 12, 4 / 12]]) and np.allclose(q["rejected_fraction"], [3 / 12]) and list(q["steps"]) == [12]
    # the state after the call: the last sample, the held value, the ring
    assert st.prev.tobytes() == x[0, -1].tobytes() and not st.run.any() and not st.hang.any()
    assert st.ring[0, :12].tobytes() == x[0].tobytes() and not st.ring[0, 12:].any()


def _events(B, T, Cc, seed):
    rs = np.random.RandomState(seed)
    x = (10.0 * rs.standard_normal((B, T, Cc))).astype(np.float32)
    for _ in range(3 * B):
        b, c, n = rs.randint(B), rs.randint(Cc), rs.randint(T)
        kind = rs.randint(5)
        if kind == 0:
            x[b, n, c] = 150.0
        elif kind == 1:
            x[b, n:, c] += 90.0
        elif kind == 2:
            x[b, n:n + 7, c] = x[b, n, c]
        elif kind == 3:
            x[b, n, c] = np.nan
        else:
            x[b, n, c] = -np.inf
    return x


CONFIGS = [dict(rail=100.0), dict(jump=60.0), dict(flat_samples=4, flat_eps=0.25), dict(pp=80.0, pp_samples=64),
           dict(pp=50.0, pp_samples=5, hold_samples=2), dict(),
           dict(rail=100.0, jump=60.0, flat_samples=4, flat_eps=0.25, pp=80.0, pp_samples=40, hold_samples=3, max_bad=1, zero=False)]


@pytest.mark.parametrize("kw", CONFIGS)
def test_signal_gate_reference_equals_the_restatement_and_cuts_do_not_show(kw):
    G = nsd_amd.SignalGate(**kw)
    assert G.to_dict() == gr.config(**kw)
    x = _events(4, 150, 5, seed=len(kw))
    y, mask = gr.gate_ref(x, G.to_dict())
    y2, mask2 = G.reference(x)
    assert y.tobytes() == y2.tobytes() and np.array_equal(mask, mask2) and mask2.dtype == np.uint32
    ref = gr.State(4, 5)
    gr.gate_ref(x, G.to_dict(), ref)
    for cut in ([1, 7, 64, 78], [33] * 4 + [18], [149, 1]):
        st, ys, ms, t = gr.State(4, 5), [], [], 0
        for n in cut:
            yy, mm = gr.gate_ref(x[:, t:t + n], G.to_dict(), st)
            ys.append(yy); ms.append(mm); t += n
        assert np.concatenate(ys, 1).tobytes() == y.tobytes() and np.array_equal(np.concatenate(ms, 1), mask), cut
        assert np.array_equal(st.slot_rows(), ref.slot_rows()), cut
    # the apply stage: both restatements, and a good channel is a bitwise copy
    v = np.random.RandomState(1).standard_normal(x.shape).astype(np.float32)
    out = gr.apply_ref(v, mask, G.to_dict())
    assert gr.same_bits(G.apply_reference(v, mask), out)
    keep = ~np.isnan(out) & ~((mask[..., None] >> np.arange(5, dtype=np.uint32)) & 1).astype(bool)
    assert out[keep].tobytes() == v[keep].tobytes()
    assert gr.same_bits(G.apply_reference(v, mask, max_bad=5), gr.apply_ref(v, mask, dict(G.to_dict(), max_bad=5)))


def test_design_rounds_seconds_to_samples():
    G = nsd_amd.SignalGate
    g = G.design(fs=125.0, rail=200.0, jump=80.0, flat_seconds=0.1, pp=100.0, hold_seconds=0.25, max_bad_channels=2)
    assert (g.rail, g.jump, g.pp) == (200.0, 80.0, 100.0)
    assert g.flat_samples == 13                       # 12.5 -> 13: halves go up
    assert g.pp_samples == 63                         # the default 0.5 s: 62.5 -> 63
    assert g.hold_samples == 31                       # 31.25 -> 31
    assert g.max_bad == 2 and g.zero
    assert G.design(fs=250.0, pp=50.0, pp_seconds=0.256).pp_samples == 64
    off = G.design()
    assert off == G() and off.max_bad == 32 and off.pp_samples == 0 and off.flat_samples == 0     # pp_seconds alone turns nothing on
    assert G.design(hold_seconds=0.004).hold_samples == 1 and G.design(hold_seconds=0.0039).hold_samples == 0
    for bad in (dict(pp=50.0, pp_seconds=0.52), dict(pp=50.0, pp_seconds=0.003), dict(flat_seconds=0.008), dict(hold_seconds=-1.0)):
        with pytest.raises(ValueError):
            G.design(**bad)
    for bad in (dict(rail=-1.0), dict(jump=float("nan")), dict(pp=float("inf")), dict(flat_eps=-0.5), dict(flat_samples=-1),
                dict(pp_samples=65), dict(hold_samples=-2), dict(max_bad=-1), dict(flat_samples=2.5)):
        with pytest.raises(ValueError):
            G(**bad)


def test_to_dict_round_trip_and_the_struct():
    g = nsd_amd.SignalGate(rail=0.1, jump=60.0, flat_eps=0.25, flat_samples=4, pp=80.0, pp_samples=64, hold_samples=3, max_bad=1, zero=False)
    assert nsd_amd.SignalGate.from_dict(g.to_dict()) == g
    assert g.rail == float(np.float32(0.1))           # thresholds are kept as the fp32 values the kernels compare with
    import json
    assert nsd_amd.SignalGate.from_dict(json.loads(json.dumps(g.to_dict()))) == g
    assert nsd_amd.SignalGate.from_dict({}) == nsd_amd.SignalGate()
    s = g.struct()
    assert (s.rail, s.jump, s.flat_eps, s.flat_samples, s.pp, s.pp_samples, s.hold_samples, s.max_bad, s.flags) == \
        (np.float32(0.1), 60.0, 0.25, 4, 80.0, 64, 3, 1, 0)
    assert nsd_amd.SignalGate().struct().flags == _lib.NSD_GATE_ZERO == 1
    assert C.sizeof(_lib.Gate) == 36 and C.sizeof(_lib.GateLayout) == 72


@pytest.mark.parametrize("Cc", [1, 3, 8, 31, 32])
def test_the_state_layout_is_the_restatements(Cc):
    L = nsd_amd.load_library()
    lay = _lib.GateLayout()
    assert L.nsd_gate_state_layout(Cc, C.byref(lay)) == 0
    want = gr.layout(Cc)
    assert {k: int(getattr(lay, k)) for k in want} == want
    assert want["bad"] % 2 == 0 and want["steps"] % 2 == 0 and want["stride"] % 4 == 0 and want["stride"] >= want["steps"] + 2
    assert L.nsd_gate_state_bytes(Cc, 5) == 5 * 4 * want["stride"]
    assert gr.State(2, Cc).slot_rows().shape == (2, want["stride"])


def _gate(**kw):
    return nsd_amd.SignalGate(**kw).struct()


def test_bad_arguments_are_refused_without_a_gpu():
    L = nsd_amd.load_library()
    d = _lib.Dims(4, 10, 8, 1, 1, 1, 1)
    g = C.cast(C.pointer(_gate(rail=100.0)), C.c_void_p)
    need = L.nsd_gate_state_bytes(8, 4)
    assert need > 0
    ok = [C.byref(d), g, FAKE, None, None, 0, 0, FAKE, FAKE, None]                   # window mode: what nsd_gate_step would launch

    def step(**kw):
        names = ("d", "g", "x", "slots", "state", "bytes", "S", "y", "mask", "stream")
        a = dict(zip(names, ok), **kw)
        return L.nsd_gate_step(*[a[n] for n in names])

    # NULL pointers
    for name in ("d", "g", "x", "y", "mask"):
        assert step(**{name: None}) == E_INVALID, name
        assert b"null pointer" in L.nsd_last_error()
    # the shape
    for B, T, Cc in ((4, 10, 0), (4, 10, 33), (4, 10, -1), (4, 0, 8), (-1, 10, 8)):
        bad = _lib.Dims(B, T, Cc, 1, 1, 1, 1)
        assert step(d=C.byref(bad)) == E_INVALID, (B, T, Cc)
        assert L.nsd_gate_apply(C.byref(bad), g, FAKE, FAKE, FAKE, None) == E_INVALID, (B, T, Cc)
    assert b"B >= 0, T >= 1" in L.nsd_last_error()
    # the configuration, through every entry point that reads it
    def raw(**kw):
        s = _gate()
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    for kw, text in ((dict(rail=-1.0), b"rail"), (dict(jump=float("nan")), b"jump"), (dict(flat_eps=float("inf")), b"flat_eps"),
                     (dict(pp=-0.5), b"pp"), (dict(flat_samples=-1), b"flat_samples"), (dict(pp_samples=-1), b"pp_samples"),
                     (dict(pp_samples=65), b"pp_samples"), (dict(hold_samples=-1), b"hold_samples"), (dict(max_bad=-1), b"max_bad"),
                     (dict(flags=2), b"unknown flag bits"), (dict(flags=0x80000001), b"unknown flag bits")):
        s = raw(**kw)
        p = C.cast(C.pointer(s), C.c_void_p)
        assert step(g=p) == E_INVALID, kw
        assert text in L.nsd_last_error(), (kw, L.nsd_last_error())
        assert L.nsd_gate_apply(C.byref(d), p, FAKE, FAKE, FAKE, None) == E_INVALID, kw
        assert L.nsd_gate_path(8, p) == 0, kw
    assert L.nsd_gate_path(8, g) == 1 and L.nsd_gate_path(8, None) == 1 and L.nsd_gate_path(32, None) == 1
    assert L.nsd_gate_path(0, None) == 0 and L.nsd_gate_path(33, None) == 0
    # x / y: in place is allowed, a partial overlap is not (checked before the launch: B = 0 launches nothing and returns NSD_OK)
    empty = _lib.Dims(0, 10, 8, 1, 1, 1, 1)
    assert step(d=C.byref(empty)) == 0 and step(d=C.byref(empty), y=FAKE) == 0
    assert step(y=FAKE + 4) == E_INVALID and b"overlaps" in L.nsd_last_error()
    assert step(x=FAKE + 4 * (4 * 10 * 8 - 1), y=FAKE) == E_INVALID
    assert L.nsd_gate_apply(C.byref(d), g, FAKE, FAKE, FAKE + 8, None) == E_INVALID and b"overlaps" in L.nsd_last_error()
    assert L.nsd_gate_apply(C.byref(empty), g, FAKE, FAKE, FAKE, None) == 0
    for k in range(5):
        args = [C.byref(d), g, FAKE, FAKE, FAKE, None]
        if k in (0, 1, 2, 3, 4):
            args[k] = None
        assert L.nsd_gate_apply(*args) == E_INVALID, k
        assert b"null pointer" in L.nsd_last_error()
    # stream mode: slots without a state, S, B > S, a short state
    assert step(slots=FAKE) == E_INVALID and b"slots without a state" in L.nsd_last_error()
    assert step(state=FAKE, bytes=need, S=0) == E_INVALID
    assert step(state=FAKE, bytes=need, S=3) == E_INVALID and b"B = 4 streams, S = 3 slots" in L.nsd_last_error()
    assert step(state=FAKE, bytes=need - 4, S=4) == E_WORKSPACE and b"smaller than nsd_gate_state_bytes" in L.nsd_last_error()
    assert step(state=FAKE + 4, bytes=need, S=4) == E_INVALID and b"8-byte aligned" in L.nsd_last_error()
    assert step(d=C.byref(empty), state=FAKE, bytes=need, S=4) == 0
    # reset, sizes, layout
    assert L.nsd_gate_reset(8, None, need, 4, None, 0, None) == E_INVALID
    assert L.nsd_gate_reset(33, FAKE, need, 4, None, 0, None) == E_INVALID
    assert L.nsd_gate_reset(8, FAKE, need, 0, None, 0, None) == E_INVALID
    assert L.nsd_gate_reset(8, FAKE, need - 1, 4, None, 0, None) == E_WORKSPACE
    assert L.nsd_gate_reset(8, FAKE, need, 4, FAKE, 5, None) == E_INVALID and L.nsd_gate_reset(8, FAKE, need, 4, FAKE, -1, None) == E_INVALID
    assert L.nsd_gate_reset(8, FAKE, need, 4, FAKE, 0, None) == 0                      # no slots named: nothing is launched
    assert L.nsd_gate_state_bytes(0, 4) < 0 and L.nsd_gate_state_bytes(33, 4) < 0 and L.nsd_gate_state_bytes(8, 0) < 0
    lay = _lib.GateLayout()
    assert L.nsd_gate_state_layout(33, C.byref(lay)) == E_INVALID and L.nsd_gate_state_layout(8, None) == E_INVALID


def test_the_model_refuses_a_gate_with_normalize_and_what_is_no_gate():
    G = nsd_amd.SignalGate(rail=100.0)
    with pytest.raises(ValueError, match="gate together with normalize=True"):
        nsd_amd.EEG_LSTM(gate=G, normalize=True)
    with pytest.raises(ValueError, match="expected a SignalGate"):
        nsd_amd.EEG_LSTM(gate=dict(rail=100.0))
    with pytest.raises(ValueError, match="1 .. 32 channels"):
        nsd_amd.EEG_LSTM(input_size=33, gate=G)
    m = nsd_amd.EEG_LSTM(gate=G, prep=nsd_amd.CausalPrep())
    assert m.gate == G and nsd_amd.EEG_LSTM().gate is None
    import torch
    twin = m.view_of(torch.zeros(m.spec.param_count))
    assert twin.gate == G and twin.prep == m.prep


def test_a_checkpoint_carries_the_gate(tmp_path):
    import torch
    from nsd_amd.trainer import save_reference_checkpoint
    G = nsd_amd.SignalGate.design(pp=100.0, max_bad_channels=2)
    path = str(tmp_path / "gate.pth")
    save_reference_checkpoint(nsd_amd.EEG_LSTM(gate=G), path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert set(ck) == {"state_dict", "nsd_gate"} and nsd_amd.SignalGate.from_dict(ck["nsd_gate"]) == G
    plain = str(tmp_path / "plain.pth")
    save_reference_checkpoint(nsd_amd.EEG_LSTM(), plain)
    assert "state_dict" not in torch.load(plain, map_location="cpu", weights_only=True)       # a raw state_dict, as before


def test_train_options_describe_the_gate():
    from nsd_amd import train
    ap = train.build_parser()
    base = ["--synthetic", "10"]
    assert train.gate_for(ap.parse_args(base)) is None
    g = train.gate_for(ap.parse_args(base + ["--gate-pp", "100", "--gate-max-bad-channels", "2", "--gate-drop-trials", "0.1"]))
    assert g == nsd_amd.SignalGate(pp=100.0, pp_samples=63, max_bad=2)
    g = train.gate_for(ap.parse_args(base + ["--gate-rail", "200", "--gate-jump", "80", "--gate-flat-seconds", "0.1", "--gate-hold-seconds", "0.2"]))
    assert g == nsd_amd.SignalGate(rail=200.0, jump=80.0, flat_samples=13, hold_samples=25)
    for bad in (["--gate-hold-seconds", "0.2"], ["--gate-pp", "100", "--gate-drop-trials", "0.1"],
                ["--gate-pp", "100", "--gate-max-bad-channels", "2", "--gate-drop-trials", "1.5"], ["--gate-pp", "100", "--gate-pp-seconds", "1.0"]):
        with pytest.raises(ValueError):
            train.gate_for(ap.parse_args(base + bad))
    from nsd_amd import grid
    assert grid.build_parser().parse_args(["--gate-pp", "100"]).gate_pp == 100.0


def test_screen_trials_bookkeeping_on_recorded_trials():
    x = np.load(os.path.join(ROOT, "tests", "golden", "real_trials.npz"))["x"].copy()           # [16, 625, 8]
    x[3, 200:, 5] = 4000.0                                                     # a railed electrode from sample 200 on
    x[7, 100:140, :3] += 500.0                                                  # a pop on three channels for 40 samples
    G = nsd_amd.SignalGate.design(rail=1000.0, pp=100.0, hold_seconds=0.1, max_bad_channels=2)
    bad, rejected = D.screen_trials(x, G)
    assert bad.shape == (16, 8) and rejected.shape == (16,)
    st = gr.State(16, 8)
    _, mask = gr.gate_ref(x, G.to_dict(), st)
    q = st.quality()
    assert np.array_equal(bad, q["bad_fraction"]) and np.array_equal(rejected, q["rejected_fraction"])
    assert bad[3, 5] == (625 - 200) / 625 and rejected[3] == 0.0               # one bad channel is no rejection
    assert rejected[7] >= 40 / 625 and bad[7, :3].min() >= 40 / 625
    # the drop rule of the train CLI
    from nsd_amd.train import drop_bad_trials
    y = np.arange(16)
    xs, ys = drop_bad_trials(x, y, G, 0.05, "test")
    assert list(ys) == [i for i in range(16) if rejected[i] <= 0.05] and 7 not in ys and xs.shape[0] == len(ys)
    assert drop_bad_trials(x, y, None, 0.05, "test")[0] is x and drop_bad_trials(x, y, G, None, "test")[0] is x
    import torch
    b2, r2 = D.screen_trials(torch.from_numpy(x), G)                           # a host tensor takes the host route
    assert np.array_equal(b2, bad) and np.array_equal(r2, rejected)
