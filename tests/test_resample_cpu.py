"""The rate conversion without a GPU: the ABI surface and its refusals (all made before any launch, so pointers that are never
dereferenced serve), nsd_resample_out_steps against its formula, the numpy restatement (tests/resample_ref.py) on its own -- cut
independence and the poison window --, Resample.design's table and frequency response, and the decoders' host logic with the launches
replaced by recording stand-ins."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import nsd_amd
from nsd_amd import _lib, ops
from nsd_amd import stream as st_mod
from nsd_amd.resample import Resample
from tests import resample_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nsd_resample_path", "nsd_resample_out_steps", "nsd_resample_state_bytes", "nsd_resample_state_layout", "nsd_resample_reset",
         "nsd_resample_step")
PAIRS = {(250, 125): (1, 2, 47), (500, 125): (1, 4, 91), (1000, 125): (1, 8, 179), (256, 125): (125, 256, 46), (200, 125): (5, 8, 36),
         (128, 125): (125, 128, 23), (125, 250): (2, 1, 24)}


def _cfg(L, M, P):
    return C.cast(C.pointer(_lib.Resample(L, M, P)), C.c_void_p)


def _err():
    return _lib.lib().nsd_last_error().decode()


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_bound_and_exported_and_the_version_stays():
    header = open(os.path.join(ROOT, "include", "nsd.h")).read()
    L = _lib.lib()
    for name in NAMES:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert "typedef struct nsd_resample { int32_t L, M, P; } nsd_resample;" in header
    assert "typedef struct nsd_resample_layout { int64_t hist, n_in, stride; } nsd_resample_layout;" in header
    assert L.nsd_version() == 301
    assert C.sizeof(_lib.Resample) == 12 and C.sizeof(_lib.ResampleLayout) == 24
    assert "nsd_resample.hip" in open(os.path.join(ROOT, "neural-speech-decoding_amd", "csrc", "Makefile")).read()


def test_path_layout_and_state_bytes():
    L = _lib.lib()
    assert L.nsd_resample_path(8, None) == 1 and L.nsd_resample_path(64, _cfg(1, 2, 47)) == 1
    for C_, cfg in ((0, (1, 2, 3)), (65, (1, 2, 3)), (8, (0, 1, 1)), (8, (1, 1025, 1)), (8, (1025, 1, 1)), (8, (2, 4, 3)), (8, (6, 4, 3)),
                    (8, (1, 2, 0)), (8, (1, 2, 257)), (8, (1024, 1, 65))):
        assert L.nsd_resample_path(C_, _cfg(*cfg)) == 0, (C_, cfg)
        assert L.nsd_resample_state_bytes(C_, _cfg(*cfg), 1) < 0, (C_, cfg)
    assert L.nsd_resample_path(8, _cfg(1024, 1, 64)) == 1                       # L * P = 65536 is the last one in
    for C_, P in ((8, 47), (3, 36), (1, 2), (64, 256), (5, 1), (1, 1)):
        lay = _lib.ResampleLayout()
        assert L.nsd_resample_state_layout(C_, _cfg(1, 2, P), C.byref(lay)) == 0
        assert lay.hist == 0 and lay.n_in >= (P - 1) * C_ and lay.n_in % 2 == 0 and lay.n_in - (P - 1) * C_ <= 1
        assert lay.stride >= lay.n_in + 2 and lay.stride % 4 == 0 and lay.stride - lay.n_in - 2 <= 3
        assert L.nsd_resample_state_bytes(C_, _cfg(1, 2, P), 7) == 7 * lay.stride * 4
        assert ops.resample_layout(C_, Resample(1, 2, P, np.zeros((1, P), np.float32))).stride == lay.stride
    assert L.nsd_resample_state_bytes(8, _cfg(1, 2, 3), 0) < 0 and L.nsd_resample_state_bytes(8, None, 1) < 0
    assert L.nsd_resample_state_layout(8, _cfg(1, 2, 3), None) != 0


def test_out_steps_equals_the_formula():
    L = _lib.lib()
    for (Lr, M, P) in list(PAIRS.values()) + [(3, 2, 5), (1, 1, 1), (1024, 1023, 2), (1, 1024, 1)]:
        for n in (0, 1, 2, 7, 40, 41, 1000, 2**31 + 5, 2**40 - 50):
            for T in (0, 1, 2, 13, 25, 50, 1250):
                want = rr.ceil_div((n + T) * Lr, M) - rr.ceil_div(n * Lr, M)
                assert L.nsd_resample_out_steps(_cfg(Lr, M, P), n, T) == want == rr.out_steps(Lr, M, n, T), (Lr, M, n, T)
                assert want in (T * Lr // M, rr.ceil_div(T * Lr, M))
                assert Resample(Lr, M, P, np.zeros((Lr, P), np.float32)).out_steps(n, T) == want
    assert L.nsd_resample_out_steps(_cfg(1, 2, 3), 0, 1) == 1 and L.nsd_resample_out_steps(_cfg(1, 2, 3), 1, 1) == 0     # it can be 0
    for bad in ((_cfg(2, 4, 3), 0, 1), (_cfg(1, 2, 3), -1, 1), (_cfg(1, 2, 3), 0, -1), (None, 0, 1)):
        assert L.nsd_resample_out_steps(*bad) < 0


def test_the_step_and_the_reset_refuse_before_any_launch():
    L = _lib.lib()
    X, Y, TAPS, STATE = 0x10000, 0x900000, 0x5000000, 0x7000000                 # never dereferenced: every call below is refused first
    d = _lib.Dims(2, 10, 8, 1, 1, 1, 1)
    good = _cfg(1, 2, 47)
    need = L.nsd_resample_state_bytes(8, good, 4)

    def step(d=d, r=good, taps=TAPS, x=X, slots=None, state=STATE, nbytes=need, S=4, y=Y, To=5, cnt=None):
        return L.nsd_resample_step(C.byref(d) if d is not None else None, r, taps, x, slots, state, nbytes, S, y, To, cnt, None)
    INVALID, WORKSPACE = -1, L.nsd_resample_step(C.byref(d), good, TAPS, X, None, STATE, need - 4, 4, Y, 5, None, None)
    assert WORKSPACE < 0 and "smaller than nsd_resample_state_bytes" in _err()
    INVALID = step(r=_cfg(2, 4, 3))
    assert INVALID < 0 and INVALID != WORKSPACE and "not reduced" in _err()
    cases = {
        "null d": dict(d=None), "null r": dict(r=None), "null taps": dict(taps=None), "null x": dict(x=None), "null y": dict(y=None),
        "C = 0": dict(d=_lib.Dims(2, 10, 0, 1, 1, 1, 1)), "C = 65": dict(d=_lib.Dims(2, 10, 65, 1, 1, 1, 1)),
        "T = 0": dict(d=_lib.Dims(2, 0, 8, 1, 1, 1, 1)), "B < 0": dict(d=_lib.Dims(-1, 10, 8, 1, 1, 1, 1)),
        "L = 0": dict(r=_cfg(0, 1, 3)), "M = 1025": dict(r=_cfg(1, 1025, 3)), "L = 1025": dict(r=_cfg(1025, 1, 3)),
        "gcd": dict(r=_cfg(4, 6, 3)), "P = 0": dict(r=_cfg(1, 2, 0)), "P = 257": dict(r=_cfg(1, 2, 257)), "L * P": dict(r=_cfg(1023, 1, 65)),
        "B > S": dict(S=1, nbytes=need), "S = 0": dict(S=0), "odd state": dict(state=STATE + 4),
        "To too small": dict(To=4), "slots without a state": dict(state=None, slots=0x100),
        "window mode To too large": dict(state=None, To=6), "window mode To too small": dict(state=None, To=4),
        "y overlaps the end of x": dict(y=X + 4 * (2 * 10 * 8 - 1)), "x overlaps the end of y": dict(x=Y + 4 * (2 * 5 * 8 - 1)),
        "y is x": dict(y=X),
    }
    for name, kw in cases.items():
        assert step(**kw) == INVALID, name
        assert _err().startswith("resample_step:"), (name, _err())
    # what is allowed is not refused for its arguments: B = 0 launches nothing and returns 0, also with a larger To in stream mode
    assert step(d=_lib.Dims(0, 10, 8, 1, 1, 1, 1)) == 0 and step(d=_lib.Dims(0, 10, 8, 1, 1, 1, 1), To=9) == 0
    assert step(d=_lib.Dims(0, 10, 8, 1, 1, 1, 1), state=None) == 0
    assert step(d=_lib.Dims(0, 10, 8, 1, 1, 1, 1), y=X + 4 * 2 * 10 * 8) == 0     # y right behind x is no overlap

    def reset(C_=8, r=good, state=STATE, nbytes=need, S=4, slots=None, n=0):
        return L.nsd_resample_reset(C_, r, state, nbytes, S, slots, n, None)
    assert reset(nbytes=need - 1) == WORKSPACE
    for kw in (dict(C_=0), dict(r=None), dict(r=_cfg(2, 2, 1)), dict(state=None), dict(state=STATE + 4), dict(S=0), dict(slots=0x100, n=5),
               dict(slots=0x100, n=-1)):
        assert reset(**kw) == INVALID, kw
    assert reset(slots=0x100, n=0) == 0                                         # no slot named: nothing to launch


# ---- the reference on its own -------------------------------------------------------------------------------------------------------------
def _random(L, M, P, seed=0):
    rs = np.random.RandomState(seed)
    return (rs.standard_normal((L, P)) / np.sqrt(P)).astype(np.float32)


def _by_cuts(x, taps, L, M, cuts):
    n_in, hist, outs, t = 0, None, [], 0
    for n in cuts:
        y, cnt, n_in, hist = rr.step(x[t:t + n], taps, L, M, n_in, hist)
        assert cnt == len(y) == rr.out_steps(L, M, t, n)
        outs.append(y)
        t += n
    return np.concatenate(outs), n_in, hist


def test_the_reference_does_not_depend_on_the_cut():
    taps = Resample.design(200, 125).taps
    x = (20.0 * np.random.RandomState(1).standard_normal((97, 3))).astype(np.float32)
    whole, n_in, hist = _by_cuts(x, taps, 5, 8, [97])
    assert len(whole) == 61 == rr.ceil_div(97 * 5, 8) and n_in == 97
    for cuts in ([1] * 97, [7, 13, 29, 48], [96, 1], [50, 47]):
        got, n2, h2 = _by_cuts(x, taps, 5, 8, cuts)
        assert rr.same_bits(got, whole) and n2 == 97 and h2.tobytes() == hist.tobytes(), cuts
    assert hist.tobytes() == x[97 - 35:].tobytes()                              # the last P - 1 samples, oldest first
    # the definition itself, one output spelled out in scalar float32 arithmetic
    j = 40
    q, ph = (j * 8) // 5, (j * 8) % 5
    acc = np.float32(0.0)
    for i in range(36):
        acc = np.float32(acc + np.float32(taps[ph, i] * (x[q - i, 1] if q - i >= 0 else np.float32(0.0))))
    assert acc.tobytes() == whole[j, 1].tobytes()
    # a chunk shorter than the history, a history of nothing (P = 1), an upsampler
    for (L, M, P), cuts in (((1, 2, 47), [3, 1, 1, 60, 32]), ((1, 1, 1), [1, 96]), ((2, 1, 24), [5, 92]), ((125, 128, 23), [64, 33])):
        t = _random(L, M, P)
        assert rr.same_bits(_by_cuts(x, t, L, M, cuts)[0], _by_cuts(x, t, L, M, [97])[0]), (L, M, P)


def test_the_poison_window_is_exact_and_the_stage_heals():
    for (L, M, P) in ((5, 8, 36), (1, 2, 47), (2, 1, 24), (1, 1, 1)):
        taps = _random(L, M, P, seed=2)
        taps[:, ::3] = 0.0                                                      # zero taps poison too: 0 * Inf is NaN
        T = 4 * P + 30
        x = np.random.RandomState(3).standard_normal((T, 2)).astype(np.float32)
        for n, bad in ((0, np.inf), (P + 3, np.nan), (T - 1, -np.inf)):
            xp = x.copy()
            xp[n, 1] = bad
            y = _by_cuts(xp, taps, L, M, [n + 1, T - n - 1] if n + 1 < T else [T])[0]
            want = np.zeros(len(y), bool)
            want[rr.poisoned_outputs(L, M, P, n, T)] = True
            assert (~np.isfinite(y[:, 1]) == want).all() and np.isfinite(y[:, 0]).all(), (L, M, P, n)
            clean = _by_cuts(x, taps, L, M, [T])[0]
            assert rr.same_bits(y[~want], clean[~want])                          # everything outside the window is untouched


# ---- the design ---------------------------------------------------------------------------------------------------------------------------
def test_design_gives_the_table_of_ratios_and_tap_counts():
    for (fi, fo), (L, M, P) in PAIRS.items():
        r = Resample.design(fi, fo)
        assert (r.L, r.M, r.P) == (L, M, P) and r.taps.shape == (L, P) and r.taps.dtype == np.float32, (fi, fo)
        half = int(np.ceil(10 * max(L, M) / 0.9))
        assert abs(r.delay - half / M) < 1e-6 and 11.0 <= (half / M if L <= M else half / M / 2) <= 11.6
        # every phase passes DC
        assert np.abs(r.taps.astype(np.float64).sum(1) - 1.0).max() < 1e-4, (fi, fo)
        assert Resample.from_dict(r.to_dict()) == r and hash(Resample.from_dict(r.to_dict())) == hash(r)
    assert Resample.design(62.5, 125).L == 2 and Resample.design(125, 125).taps.shape == (1, 25)


def test_the_decimator_by_two_passes_the_band_and_stops_the_images():
    r = Resample.design(250, 125)
    h = r.prototype()
    f = np.arange(0.0, 125.0, 0.25)
    H = np.abs(np.exp(-2j * np.pi * np.outer(f, np.arange(len(h))) / 250.0) @ h)
    dev_pass, stop = np.abs(H[f <= 45.0] - 1.0).max(), H[f >= 80.0].max()
    print(f"passband deviation up to 45 Hz {dev_pass:.2e}, response from 80 Hz {stop:.2e}")
    assert dev_pass <= 1e-2 and stop <= 1e-4


def test_validation_on_the_host():
    ok = np.zeros((1, 3), np.float32)
    for kw in (dict(L=0, M=1, P=3, taps=ok), dict(L=1, M=1025, P=3, taps=ok), dict(L=2, M=4, P=3, taps=np.zeros((2, 3))),
               dict(L=1, M=2, P=257, taps=np.zeros((1, 257))), dict(L=1, M=2, P=2, taps=ok), dict(L=1, M=2, P=3, taps=ok + np.nan),
               dict(L=1024, M=1, P=65, taps=np.zeros((1024, 65)))):
        with pytest.raises(ValueError):
            Resample(**kw)
    with pytest.raises(ValueError):
        Resample.design(125, 125 * 1025)
    with pytest.raises(ValueError, match="resample together with normalize"):
        nsd_amd.EEG_LSTM(resample=Resample.design(250, 125), normalize=True)
    with pytest.raises(ValueError, match="expected a Resample"):
        nsd_amd.EEG_LSTM(resample=(1, 2))
    m = nsd_amd.EEG_LSTM(resample=Resample.design(250, 125)).eval()
    assert m.view_of(torch.zeros(m.spec.param_count)).resample == m.resample
    assert nsd_amd.EEG_LSTM().resample is None


# ---- the decoders on the host: recording stand-ins for the launches ---------------------------------------------------------------------------
S, Cc, K = 4, 8, 3


def _n_in_words(state, r):
    """the int64 n_in of every slot inside a resample state [S, stride] (a view)"""
    return state.view(torch.int64)[:, ops.resample_layout(Cc, r).n_in // 2]


def _rows(slots, n):
    return list(range(n)) if slots is None else [int(v) for v in slots.tolist()]


@pytest.fixture
def launches(monkeypatch):
    rec = []

    def resample_step(x, resample, state=None, *, slots=None, out=None, cnt=None, taps=None):
        rec.append(dict(name="resample_step", x=x, state=state, slots=slots, out=out))
        _n_in_words(state, resample)[_rows(slots, x.shape[0])] += x.shape[1]      # as the kernel: the count lives in the state
        return out

    def prep_step(x, prep, state=None, *, slots=None, out=None):
        rec.append(dict(name="prep_step", x=x, state=state, slots=slots, out=out))
        return out

    def gate_step(x, gate, state=None, *, slots=None, out=None, mask=None):
        rec.append(dict(name="gate_step", x=x, state=state, slots=slots, out=out))
        return out, mask

    def gate_apply(v, gate, mask, *, out=None, max_bad=None):
        rec.append(dict(name="gate_apply", x=v, out=out))
        return out

    def stream_step(spec, flat, x, state, *, slots=None, residual=False, read=True):
        rec.append(dict(name="stream_step", x=x, slots=slots))
        return None, torch.zeros((x.shape[0], K))

    def window_step(spec, flat, x, state, *, window, hop, slots=None, residual=False):
        rec.append(dict(name="window_step", x=x, slots=slots))
        D = -(-x.shape[1] // hop)
        return None, torch.zeros((x.shape[0], D, K)), torch.zeros((x.shape[0], D), dtype=torch.int64), torch.zeros(x.shape[0], dtype=torch.int32)

    def reset_of(name):
        def f(*a):
            rec.append(dict(name=name, args=a))
            if name == "resample_reset":                                        # (C, resample, state, slots)
                _n_in_words(a[2], a[1])[_rows(a[3], S)] = 0
        return f

    def resample_state(C_, r, S_, device=None):
        st = torch.ones((S_, ops.resample_layout(C_, r).stride))
        _n_in_words(st, r)[:] = 0
        return st

    for f in (resample_step, prep_step, gate_step, gate_apply, stream_step, window_step, resample_state):
        monkeypatch.setattr(ops, f.__name__, f)
    for name in ("resample_reset", "prep_reset", "gate_reset", "stream_reset", "window_reset"):
        monkeypatch.setattr(ops, name, reset_of(name))
    monkeypatch.setattr(ops, "prep_state", lambda C_, S_, device=None: torch.ones((S_, 10)))
    monkeypatch.setattr(ops, "gate_state", lambda C_, S_, device=None: torch.ones((S_, 12)))
    return rec


def _stand_in(kind, resample, gate=False, prep=True):
    """a decoder of class `kind` on the host: what __init__ sets, without the model living on a GPU"""
    model = nsd_amd.EEG_LSTM(resample=resample, prep=nsd_amd.CausalPrep.design(highpass=1.0) if prep else None,
                             gate=nsd_amd.SignalGate(rail=100.0) if gate else None).eval()
    model.flat_parameters = lambda: None
    cls = {"stream": st_mod.StreamDecoder, "sliding": st_mod.SlidingStreamDecoder}[kind]
    dec = cls.__new__(cls)
    dec.model, dec.streams, dec.device = model, S, torch.device("cpu")
    dec.state = torch.zeros((S, 16))
    if kind == "sliding":
        dec.window, dec.hop = 16, 8
        dec._all = torch.arange(S)
        dec._last_end, dec._last_probs = torch.full((S,), -1, dtype=torch.int64), torch.zeros((S, K))
    dec._init_front(model)
    return dec


@pytest.mark.parametrize("kind", ["stream", "sliding"])
def test_push_runs_stage_0_first_and_hands_on_the_steps_it_emitted(launches, kind):
    r = Resample.design(200, 125)
    dec = _stand_in(kind, r, gate=True)
    assert dec.resample is r and tuple(dec.resample_state.shape) == (S, ops.resample_layout(Cc, r).stride) and list(dec.input_steps) == [0] * S
    x = torch.zeros((2, 7, Cc))
    dec.push(x, slots=[3, 1])
    own = "stream_step" if kind == "stream" else "window_step"
    assert [c["name"] for c in launches] == ["resample_step", "gate_step", "prep_step", "gate_apply", own]
    first = launches[0]
    assert first["state"] is dec.resample_state and first["slots"].tolist() == [3, 1] and tuple(first["x"].shape) == (2, 7, Cc)
    assert tuple(first["out"].shape) == (2, 5, Cc)                              # ceil(7 * 5 / 8): all of them emitted
    assert launches[1]["x"] is first["out"] and tuple(launches[-1]["x"].shape) == (2, 5, Cc) and launches[-1]["slots"].tolist() == [3, 1]
    assert list(dec.input_steps) == [0, 7, 0, 7]
    # one more sample: ceil(40 / 8) - ceil(35 / 8) = 0 steps.  Only the conversion advances, and nothing is decided
    del launches[:]
    out = dec.push(torch.zeros((2, 1, Cc)), slots=[3, 1])
    assert [c["name"] for c in launches] == ["resample_step"] and list(dec.input_steps) == [0, 8, 0, 8]
    if kind == "stream":
        assert out is None
    else:
        assert tuple(out[0].shape) == (2, 0, K) and tuple(out[1].shape) == (2, 0) and out[2].tolist() == [0, 0]
    # a chunk that emits floor(T L / M) steps: the call may write ceil rows, the stages behind get the emitted ones, dense
    del launches[:]
    dec.push(torch.zeros((2, 23, Cc)), slots=[3, 1])                            # ceil(31 * 5 / 8) - 5 = 15 of ceil(23 * 5 / 8) = 15
    dec.push(torch.zeros((2, 2, Cc)), slots=[3, 1])                             # ceil(33 * 5 / 8) - 20 = 1 of 2
    calls = [c for c in launches if c["name"] == "resample_step"]
    assert tuple(calls[1]["out"].shape) == (2, 2, Cc) and tuple(launches[-1]["x"].shape) == (2, 1, Cc) and launches[-1]["x"].is_contiguous()
    # streams whose counts differ are refused before any launch, and nothing moves
    del launches[:]
    with pytest.raises(nsd_amd.NsdError, match="push those slots separately"):
        dec.push(torch.zeros((2, 2, Cc)), slots=[0, 1])                         # slot 0 holds 0 samples (2 steps), slot 1 holds 33 (1 step)
    assert launches == [] and list(dec.input_steps) == [0, 33, 0, 33]
    # without a conversion push is what it was
    del launches[:]
    plain = _stand_in(kind, None, gate=True)
    plain.push(x, slots=[3, 1])
    assert [c["name"] for c in launches] == ["gate_step", "prep_step", "gate_apply", own] and plain.resample_state is None
    assert "resample_state" not in plain._front_state_dict({})


def test_reset_and_the_checkpoint_cover_the_conversion(launches):
    r = Resample.design(250, 125)
    a, b, plain = _stand_in("stream", r), _stand_in("stream", r), _stand_in("stream", None)
    a.push(torch.zeros((3, 10, Cc)))
    a.resample_state[:, :ops.resample_layout(Cc, r).n_in].mul_(3.0)             # (the history words)
    sd = a._front_state_dict({})
    assert set(sd) == {"resample_state", "resample_n_in", "prep_state"} and sd["resample_n_in"].tolist() == [10, 10, 10, 0]
    assert sd["resample_n_in"].tolist() == _n_in_words(sd["resample_state"], r).tolist()
    b._load_front_state(*b._check_front_state(sd, "who"))
    b._load_resample_state(sd)
    assert torch.equal(b.resample_state, a.resample_state) and list(b.input_steps) == [10, 10, 10, 0]
    # the mirror is also in the state itself
    col = ops.resample_layout(Cc, r).n_in // 2
    st = torch.zeros_like(a.resample_state)
    st.view(torch.int64)[:, col] = torch.tensor([5, 0, 7, 9])
    b._load_resample_state({"resample_state": st})
    assert list(b.input_steps) == [5, 0, 7, 9] and torch.equal(b.resample_state, st)
    # ... and a resample_n_in that disagrees with it is refused, with neither the state nor the mirror written
    for state, wrong in ((sd["resample_state"], torch.tensor([10, 10, 11, 0])), (sd["resample_state"], torch.tensor([10, 10, 10])),
                         (torch.zeros_like(st), [5, 0, 7, 9])):
        with pytest.raises(nsd_amd.NsdError, match="load_state_dict: resample_n_in .* disagrees with the counts"):
            b._load_resample_state({"resample_state": state, "resample_n_in": wrong})
        assert list(b.input_steps) == [5, 0, 7, 9] and torch.equal(b.resample_state, st)
    # a checkpoint without the key loads into a decoder without a conversion, and only there
    old = {"prep_state": sd["prep_state"]}
    plain._load_front_state(*plain._check_front_state(old, "who"))
    plain._load_resample_state(old)
    for dec, ckpt in ((plain, sd), (a, old), (a, dict(sd, resample_state=sd["resample_state"][:2]))):
        with pytest.raises(nsd_amd.NsdError, match="who: .*rate conversion's state"):
            dec._check_front_state(ckpt, "who")
    # reset restarts the conversion with the stream, all slots or the named ones
    del launches[:]
    a.reset([2, 0])
    names = [c["name"] for c in launches]
    assert sorted(names) == ["prep_reset", "resample_reset", "stream_reset"] and list(a.input_steps) == [0, 10, 0, 0]
    by = {c["name"]: c["args"] for c in launches}
    assert by["resample_reset"][2] is a.resample_state and by["resample_reset"][-1].tolist() == [2, 0]
    a.reset()
    assert list(a.input_steps) == [0] * S
    del launches[:]
    plain.reset()
    assert sorted(c["name"] for c in launches) == ["prep_reset", "stream_reset"]


@pytest.mark.parametrize("kind", ["stream", "sliding"])
def test_the_mirror_is_never_trusted_over_the_state(launches, kind):
    """A decoder whose launches were replayed (here: the stand-in launch called on its state, as a captured graph does) has a mirror
    that never moved.  Its checkpoint carries the state's counts, and a fresh decoder loaded from it cuts an odd chunk by them."""
    r = Resample.design(250, 125)
    a, fresh = _stand_in(kind, r), _stand_in(kind, r)
    a.push(torch.zeros((3, 10, Cc)))
    ops.resample_step(torch.zeros((3, 3, Cc)), r, a.resample_state, slots=None, out=torch.zeros((3, 2, Cc)))     # the replay: 13 samples held
    assert list(a.input_steps) == [10, 10, 10, 0] and _n_in_words(a.resample_state, r).tolist() == [13, 13, 13, 0]
    sd = a._front_state_dict({})
    assert sd["resample_n_in"].tolist() == _n_in_words(sd["resample_state"], r).tolist() == [13, 13, 13, 0]
    fresh._load_front_state(*fresh._check_front_state(sd, "who"))
    fresh._load_resample_state(sd)
    assert list(fresh.input_steps) == [13, 13, 13, 0]
    # one more sample at 1 / 2: ceil(14 / 2) - ceil(13 / 2) = 0 steps (the stale count of 10 would emit one, a NaN row)
    del launches[:]
    out = fresh.push(torch.zeros((3, 1, Cc)))
    assert [c["name"] for c in launches] == ["resample_step"] and list(fresh.input_steps) == [14, 14, 14, 0]
    assert out is None if kind == "stream" else tuple(out[0].shape) == (3, 0, K)
    # ... and the next one emits exactly one
    del launches[:]
    fresh.push(torch.zeros((3, 1, Cc)))
    assert tuple(launches[-1]["x"].shape) == (3, 1, Cc) and _n_in_words(fresh.resample_state, r).tolist() == list(fresh.input_steps)
    # the stale mirror travelling beside the state (a checkpoint written before the counts came from the state) is refused
    with pytest.raises(nsd_amd.NsdError, match="disagrees with the counts"):
        _stand_in(kind, r)._load_resample_state(dict(sd, resample_n_in=torch.tensor([10, 10, 10, 0])))
