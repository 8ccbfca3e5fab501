"""Sliding-window decisions (nsd_window_* of include/nsd.h): everything that can be held without a GPU -- the ABI surface, the path /
rows / state-size queries over a table, every host-side refusal, the integer schedule of tests/window_ref.py against brute-force
enumeration, the state layout, the new kernels' code object (no private segment) and the decoder's refusal without a GPU."""
import ctypes as C
import os
import re

import pytest

import nsd_amd
from nsd_amd import _lib, ops
from tests import window_ref as wr
from tests.code_object import device_elf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nsd_window_path", "nsd_window_rows", "nsd_window_state_bytes", "nsd_window_state_layout", "nsd_window_reset", "nsd_window_step")
E_INVALID, E_WORKSPACE = -1, -3
PTR = 4096                       # stands for a device pointer: a refusal returns before anything looks at it


def _dims(B=1, T=1, Cc=8, H=48, L=2, K=3, F=32):
    return _lib.Dims(B, T, Cc, H, L, K, F)


def test_symbols_are_declared_bound_and_exported_and_the_version_stays():
    full = open(os.path.join(ROOT, "include", "nsd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    declared = set(re.findall(r"\b(nsd_[a-z0-9_]+)\s*\(", hdr))
    L = nsd_amd.load_library()
    for name in SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS and hasattr(L, name), name
    assert L.nsd_version() == 301
    assert re.search(r"#define\s+NSD_WINDOW_MAX_PHASES\s+128\b", hdr) and _lib.NSD_WINDOW_MAX_PHASES == 128
    assert "nsd_window48.hip" in open(os.path.join(ROOT, "neural-speech-decoding_amd", "csrc", "Makefile")).read()
    assert "SlidingStreamDecoder" in nsd_amd.__all__ and issubclass(nsd_amd.SlidingStreamDecoder, nsd_amd.StreamDecoder)
    for fn in ("window_path", "window_rows", "window_layout", "window_state", "window_reset", "window_step"):
        assert callable(getattr(ops, fn)), fn
    # the header states what a caller leans on: the definition, the outputs, the device-side behaviour
    for words in ("[k Hp, k Hp + W)", "e_k = k Hp + W", "PHASE r = k mod R", "n0 < e_k <= n0 + T", "counts[b] = -1",
                  "poisons exactly the windows that contain it", "B * D * K", "NSD_VERSION stays 301"):
        assert words in full, words


WINDOWS = [((12, 4), 1), ((12, 12), 1), ((1, 1), 1), ((625, 25), 1), ((128, 1), 1), ((256, 2), 1),      # R = 128: the last one allowed
           ((129, 1), 0), ((258, 2), 0), ((12, 5), 0), ((12, 8), 0), ((4, 12), 0), ((12, 13), 0), ((0, 0), 0), ((12, 0), 0), ((0, 4), 0),
           ((-12, 4), 0), ((12, -4), 0), ((-12, -4), 0)]


@pytest.mark.parametrize("wh,w_ok", WINDOWS)
@pytest.mark.parametrize("dims,inside", [(dict(), 1), (dict(Cc=3, K=2), 1), (dict(F=64, K=64), 1), (dict(H=32), 0), (dict(H=64), 0),
                                         (dict(L=1), 0), (dict(Cc=9), 0), (dict(K=0), 0)])
def test_path_rows_and_state_bytes_over_a_table(dims, inside, wh, w_ok):
    L, d, w = nsd_amd.load_library(), _dims(**dims), _lib.Window(*wh)
    W, Hp = wh
    assert L.nsd_stream_path(C.byref(d)) == inside
    assert L.nsd_window_path(C.byref(d), C.byref(w)) == (inside & w_ok)
    assert L.nsd_window_path(None, C.byref(w)) == 0 and L.nsd_window_path(C.byref(d), None) == 0
    for T in (1, 24, 25, 26, 2 ** 31 - 1):
        assert L.nsd_window_rows(T, C.byref(w)) == (-(-T // Hp) if w_ok else E_INVALID), T
    assert L.nsd_window_rows(0, C.byref(w)) == E_INVALID and L.nsd_window_rows(-3, C.byref(w)) == E_INVALID and L.nsd_window_rows(5, None) == E_INVALID
    lay = _lib.WindowLayout()
    rc = L.nsd_window_state_layout(C.byref(d), C.byref(w), C.byref(lay))
    for S in (1, 4, 257):
        n = L.nsd_window_state_bytes(C.byref(d), C.byref(w), S)
        if inside and w_ok:
            assert rc == 0 and n == S * lay.stream_stride * 4
        else:
            assert rc == E_INVALID and n == E_INVALID
    for S in (0, -1):
        assert L.nsd_window_state_bytes(C.byref(d), C.byref(w), S) == E_INVALID
    assert L.nsd_window_state_bytes(None, C.byref(w), 1) == E_INVALID and L.nsd_window_state_bytes(C.byref(d), None, 1) == E_INVALID
    if inside:
        assert ops.window_path(ops.ModelSpec(C=d.C, H=d.H, L=d.L, K=d.K, F=d.F), W, Hp) == bool(w_ok)
    assert not ops.window_path(ops.ModelSpec(D=2), 12, 4)


@pytest.mark.parametrize("W,Hp", [(12, 4), (12, 12), (1, 1), (70, 35), (128, 1), (625, 25)])
def test_the_phase_slots_are_stream_layout_slots(W, Hp):
    spec = ops.ModelSpec()
    lay, sl = ops.window_layout(spec, W, Hp), ops.stream_layout(spec)
    R = W // Hp
    assert lay.phases == R and lay.phase_stride == sl.stride
    assert lay.window == R * sl.stride and lay.hop == lay.window + 1           # the header follows the R phase slots
    assert lay.count >= lay.hop + 1 and lay.count % 2 == 0                     # int64: 8-byte aligned
    assert lay.stream_stride % 4 == 0 and lay.stream_stride >= lay.count + 2 * R   # room for the count, one copy per phase
    assert lay.stream_stride - R * sl.stride < 4 + 2 * R + 4                   # a small header
    assert ops.window_rows(26, W, Hp) == wr.rows(26, Hp)
    with pytest.raises(nsd_amd.NsdError):
        ops.window_layout(spec, W, W + 1)


def test_every_host_side_refusal_returns_its_code_without_a_gpu():
    L = nsd_amd.load_library()
    d, w, S = _dims(B=3, T=5), _lib.Window(12, 4), 4
    need = L.nsd_window_state_bytes(C.byref(d), C.byref(w), S)
    err = lambda: L.nsd_last_error().decode()

    def step(dd=d, ww=w, params=PTR, x=PTR, slots=None, flags=0, state=PTR, nbytes=need, s=S, logits=PTR, probs=PTR, ends=PTR, counts=PTR):
        return L.nsd_window_step(None if dd is None else C.byref(dd), None if ww is None else C.byref(ww), params, x, slots, flags, state,
                                 nbytes, s, logits, probs, ends, counts, None)

    def reset(dd=d, ww=w, state=PTR, nbytes=need, s=S, slots=None, n=0):
        return L.nsd_window_reset(None if dd is None else C.byref(dd), None if ww is None else C.byref(ww), state, nbytes, s, slots, n, None)

    assert step(dd=None) == E_INVALID and step(ww=None) == E_INVALID and "null" in err()
    for name in ("params", "x", "state", "logits", "ends", "counts"):
        assert step(**{name: None}) == E_INVALID and "null" in err(), name
    assert step(dd=_dims(B=0, T=5), probs=None) == 0                         # probs may be NULL
    for bad in (dict(H=32), dict(H=64), dict(L=3), dict(Cc=9), dict(F=65), dict(K=65), dict(K=0)):
        assert step(dd=_dims(B=3, T=5, **bad)) == E_INVALID, bad
    for wh, w_ok in WINDOWS:
        if not w_ok:
            assert step(ww=_lib.Window(*wh)) == E_INVALID and reset(ww=_lib.Window(*wh)) == E_INVALID, wh
    assert "nsd_window_path" in err()
    assert step(dd=_dims(B=3, T=0)) == E_INVALID and step(dd=_dims(B=-1, T=5)) == E_INVALID
    assert step(dd=_dims(B=5, T=5)) == E_INVALID and "B = 5" in err()
    assert step(s=0) == E_INVALID and step(s=-2) == E_INVALID
    assert step(flags=_lib.NSD_FLAG_TRAIN) == E_INVALID and step(flags=_lib.NSD_FLAG_BF16 | _lib.NSD_FLAG_RESIDUAL) == E_INVALID
    assert step(nbytes=need - 1) == E_WORKSPACE and "nsd_window_state_bytes" in err() and step(nbytes=0) == E_WORKSPACE
    assert step(nbytes=L.nsd_stream_state_bytes(C.byref(d), S) * 3) == E_WORKSPACE        # the phase slots alone: no room for the header
    # B * D * K above 2^31 - 1: hop 1, so D = T
    big, one = _dims(B=2 ** 20, T=2 ** 12, K=64), _lib.Window(1, 1)
    huge = 2 ** 62
    assert step(dd=big, ww=one, s=2 ** 20, nbytes=huge) == E_INVALID and "B * D * K" in err()
    assert step(dd=_dims(B=2 ** 25, T=1, K=64), ww=one, s=2 ** 25, nbytes=huge) == E_INVALID and "B * D * K" in err()      # 2^31 exactly
    assert step(dd=_dims(B=0, T=5)) == 0                                     # nothing to advance: nothing launched
    assert step(dd=_dims(B=0, T=5), ww=_lib.Window(12, 5)) == E_INVALID
    # reset
    assert reset(dd=None) == E_INVALID and reset(ww=None) == E_INVALID and reset(state=None) == E_INVALID
    assert reset(s=0) == E_INVALID and reset(nbytes=need - 1) == E_WORKSPACE
    assert reset(slots=PTR, n=-1) == E_INVALID and reset(slots=PTR, n=S + 1) == E_INVALID
    assert reset(slots=PTR, n=0) == 0                                        # no stream named: nothing launched


@pytest.mark.parametrize("W,Hp", [(1, 1), (4, 2), (12, 4), (12, 12), (70, 35)])
def test_the_schedule_against_brute_force_enumeration(W, Hp):
    R = W // Hp
    for n0 in range(3 * W):
        for T in range(1, 2 * W + 4):
            ends = [(k, k * Hp + W) for k in range((n0 + T) // Hp + 2) if n0 < k * Hp + W <= n0 + T]      # the definition, window by window
            want = [(k, e, row) for row, (k, e) in enumerate(sorted(ends, key=lambda ke: ke[1]))]
            got = wr.completed(n0, T, W, Hp)
            assert got == want, (n0, T, got, want)
            assert len(got) <= wr.rows(T, Hp)
            assert all(k % R == (e // Hp) % R for k, e, _ in got)                  # the phase of a window, from its end alone
        # phase positions: replay the definition sample by sample
        pos = []
        for r in range(R):
            began = [k * Hp for k in range(n0 // Hp + 1) if k % R == r and k * Hp < n0]
            pos.append((None, 0) if not began else ((began[-1], n0 - began[-1]) if n0 - began[-1] < W else (n0, 0)))
        assert wr.phases(n0, W, Hp) == pos, (n0, wr.phases(n0, W, Hp), pos)


def test_the_window_kernels_have_no_private_segment(tmp_path):
    notes = device_elf("nsd_window48", str(tmp_path))
    sizes = {}
    for block in re.split(r"^\s*- \.agpr_count:", notes, flags=re.M)[1:]:
        kv = dict(re.findall(r"^\s*(\.[a-z_]+):\s*(.+?)\s*$", block, re.M))
        sizes[kv[".name"]] = int(kv[".private_segment_fixed_size"], 0)
    assert len(sizes) == 2 and any("window48_kernel" in k for k in sizes) and any("window_reset_kernel" in k for k in sizes), sorted(sizes)
    assert all(v == 0 for v in sizes.values()), sizes


def test_sliding_stream_decoder_needs_the_gpu_and_says_so():
    with pytest.raises(nsd_amd.NsdError, match="GPU"):
        nsd_amd.SlidingStreamDecoder(nsd_amd.EEG_LSTM().eval(), window=12, hop=4)
    with pytest.raises(nsd_amd.NsdError, match="nsd_window_path"):
        nsd_amd.SlidingStreamDecoder(nsd_amd.EEG_LSTM().eval(), window=12, hop=5)
    with pytest.raises(nsd_amd.NsdError, match="eval"):
        nsd_amd.SlidingStreamDecoder(nsd_amd.EEG_LSTM(), window=12, hop=4)
    with pytest.raises(nsd_amd.NsdError, match="^SlidingStreamDecoder: normalize=True z-scores over the whole window"):
        nsd_amd.SlidingStreamDecoder(nsd_amd.EEG_LSTM(normalize=True).eval(), window=12, hop=4)
    with pytest.raises(TypeError):
        nsd_amd.SlidingStreamDecoder(nsd_amd.EEG_LSTM().eval())              # window and hop are required
    # StreamDecoder's own refusals are what they were
    with pytest.raises(nsd_amd.NsdError, match="^StreamDecoder: normalize=True z-scores over the whole window"):
        nsd_amd.StreamDecoder(nsd_amd.EEG_LSTM(normalize=True).eval())
    with pytest.raises(nsd_amd.NsdError, match="StreamDecoder runs only on the MI355X HIP path"):
        nsd_amd.StreamDecoder(nsd_amd.EEG_LSTM().eval())
