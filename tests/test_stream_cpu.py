"""Resumable H = 48 inference (nsd_stream_* of include/nsd.h): everything that can be held without a GPU -- the ABI surface, the path
query, the public state layout, every host-side refusal, the per-step pooling reference the GPU tests lean on, the chunked producer
protocol, and the kernel's code object (no private segment)."""
import ctypes as C
import os
import re
from multiprocessing import Queue

import numpy as np
import pytest

import nsd_amd
from nsd_amd import _lib, ops
from nsd_amd.streaming_process import SAMPLING_RATE, StreamingProcess, synthetic_window
from oracle import nsd_oracle as orc
from tests import stream_ref as sr
from tests.golden.make_goldens import synth_x
from tests.code_object import device_elf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_SYMBOLS = ("nsd_stream_path", "nsd_stream_state_bytes", "nsd_stream_state_layout", "nsd_stream_reset", "nsd_stream_step")
E_INVALID, E_WORKSPACE = -1, -3
PTR = 4096                       # stands for a device pointer: a refusal returns before anything looks at it


def _dims(B=1, T=1, Cc=8, H=48, L=2, K=3, F=32):
    return _lib.Dims(B, T, Cc, H, L, K, F)


def test_stream_symbols_are_declared_bound_and_exported_and_the_version_stays():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nsd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(nsd_[a-z0-9_]+)\s*\(", hdr))
    L = nsd_amd.load_library()
    for name in STREAM_SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS and hasattr(L, name), name
    assert "typedef struct nsd_stream_layout" in hdr
    assert L.nsd_version() == 301
    assert "nsd_stream48.hip" in open(os.path.join(ROOT, "neural-speech-decoding_amd", "csrc", "Makefile")).read()
    assert {"StreamDecoder", "PredictorStream"} <= set(nsd_amd.__all__)


@pytest.mark.parametrize("dims,inside", [
    (dict(), 1), (dict(Cc=1), 1), (dict(Cc=3, K=2), 1), (dict(F=64, K=64), 1), (dict(F=1, K=1), 1), (dict(B=0, T=0), 1),
    (dict(B=1000, T=100000), 1),                                  # B and T are the call's, not the model's
    (dict(H=32), 0), (dict(H=64), 0), (dict(H=47), 0), (dict(L=1), 0), (dict(L=3), 0), (dict(Cc=9), 0), (dict(F=65), 0), (dict(K=65), 0),
    (dict(Cc=0), 0), (dict(K=0), 0), (dict(F=0), 0), (dict(L=0), 0), (dict(H=0), 0), (dict(Cc=-1), 0),
])
def test_stream_path_over_a_table_of_dims(dims, inside):
    L, d = nsd_amd.load_library(), _dims(**dims)
    assert L.nsd_stream_path(C.byref(d)) == inside
    assert L.nsd_stream_path(None) == 0
    assert (L.nsd_stream_state_bytes(C.byref(d), 4) > 0) == bool(inside)
    lay = _lib.StreamLayout()
    assert L.nsd_stream_state_layout(C.byref(d), C.byref(lay)) == (0 if inside else E_INVALID)
    spec = ops.ModelSpec(C=d.C, H=d.H, L=d.L, K=d.K, F=d.F)
    if d.C >= 1 and d.H >= 1 and d.L >= 1 and d.K >= 1 and d.F >= 1:
        assert ops.stream_path(spec) == bool(inside)
    assert not ops.stream_path(ops.ModelSpec(D=2))


def test_state_layout_is_disjoint_aligned_and_sized():
    L, d, H = nsd_amd.load_library(), _dims(), 48
    lay = ops.stream_layout(ops.ModelSpec())
    regions = [(lay.h[0], H), (lay.h[1], H), (lay.c[0], H), (lay.c[1], H), (lay.pool_max, 1), (lay.pool_den, 1), (lay.pool_acc, H),
               (lay.steps, 2)]
    used = np.zeros(int(lay.stride), np.int32)
    for off, n in regions:
        assert 0 <= off and off + n <= lay.stride, (off, n)
        used[off:off + n] += 1
    assert used.max() == 1                                           # disjoint
    assert (lay.steps * 4) % 8 == 0 and (lay.stride * 4) % 8 == 0    # the int64 step count of every slot is 8-byte aligned
    assert all(v == 0 for v in list(lay.h)[2:] + list(lay.c)[2:])
    assert int(used.sum()) <= 256                                    # "about 250 floats"
    for S in (1, 2, 7, 256, 100000):
        assert L.nsd_stream_state_bytes(C.byref(d), S) == S * lay.stride * 4 == ops.stream_state_bytes(ops.ModelSpec(), S)
    assert L.nsd_stream_state_bytes(C.byref(d), 0) == E_INVALID and L.nsd_stream_state_bytes(None, 1) == E_INVALID
    assert L.nsd_stream_state_layout(C.byref(d), None) == E_INVALID
    with pytest.raises(nsd_amd.NsdError):
        ops.stream_state_bytes(ops.ModelSpec(H=64), 1)


def test_every_host_side_refusal_returns_its_code_without_a_gpu():
    L = nsd_amd.load_library()
    d, S = _dims(B=3, T=5), 4
    need = L.nsd_stream_state_bytes(C.byref(d), S)
    err = lambda: L.nsd_last_error().decode()
    step = lambda dd=d, params=PTR, x=PTR, slots=None, flags=0, state=PTR, nbytes=need, s=S, logits=PTR, probs=PTR: \
        L.nsd_stream_step(None if dd is None else C.byref(dd), params, x, slots, flags, state, nbytes, s, logits, probs, None)
    assert step(dd=None) == E_INVALID
    assert step(params=None) == E_INVALID and "null" in err()
    assert step(x=None) == E_INVALID and step(state=None) == E_INVALID
    assert step(logits=None, probs=PTR) == E_INVALID and "probs without logits" in err()
    assert step(dd=_dims(B=3, T=0)) == E_INVALID and step(dd=_dims(B=-1, T=5)) == E_INVALID
    for bad in (dict(H=32), dict(H=64), dict(L=3), dict(Cc=9), dict(F=65), dict(K=65), dict(K=0)):
        assert step(dd=_dims(B=3, T=5, **bad)) == E_INVALID, bad
    assert "nsd_stream_path" in err() or "bad model dims" in err()
    assert step(dd=_dims(B=5, T=5)) == E_INVALID and "B = 5" in err()          # more streams than slots, slots NULL or not
    assert step(dd=_dims(B=5, T=5), slots=PTR) == E_INVALID
    assert step(s=0) == E_INVALID and step(s=-2) == E_INVALID
    assert step(flags=_lib.NSD_FLAG_TRAIN) == E_INVALID and step(flags=_lib.NSD_FLAG_BF16 | _lib.NSD_FLAG_RESIDUAL) == E_INVALID
    assert step(nbytes=need - 1) == E_WORKSPACE and "nsd_stream_state_bytes" in err()
    assert step(nbytes=0) == E_WORKSPACE
    assert step(dd=_dims(B=0, T=5)) == 0                                       # nothing to advance: accepted, nothing launched
    reset = lambda dd=d, state=PTR, nbytes=need, s=S, slots=None, n=0: \
        L.nsd_stream_reset(None if dd is None else C.byref(dd), state, nbytes, s, slots, n, None)
    assert reset(dd=None) == E_INVALID and reset(state=None) == E_INVALID and reset(dd=_dims(H=64)) == E_INVALID
    assert reset(s=0) == E_INVALID and reset(nbytes=need - 4) == E_WORKSPACE
    assert reset(slots=PTR, n=-1) == E_INVALID and reset(slots=PTR, n=S + 1) == E_INVALID
    assert reset(slots=PTR, n=0) == 0                                          # an empty list: accepted, nothing launched
    # the header states the behaviour the device decides: a bad slot index, duplicates, a non-finite sample
    hdr = open(os.path.join(ROOT, "include", "nsd.h")).read()
    for words in ("outside [0, S)", "Duplicate slots", "not finite", "No host synchronisation"):
        assert words in hdr, words


@pytest.mark.parametrize("residual", [False, True])
def test_the_per_step_pooling_reference_matches_the_oracle_on_prefixes(ref_state, residual):
    """tests/stream_ref.OnlinePool -- one update per step, fp32 -- against orc.forward(...)["pooled"] of every prefix, at the bound
    tests/test_gpu_parity.py holds `pooled` to; cutting the steps into chunks cannot matter to it (it has no notion of a chunk)."""
    d = orc.Dims()
    flat, x = orc.flatten_state(ref_state, d), synth_x(2, 41, seed=4108)
    top, _ = sr.top_sequence(flat, x, d, residual=residual)
    refs = sr.prefix_refs(flat, x, d, range(1, 42), residual=residual)
    worst = 0.0
    for b in range(2):
        pool = sr.OnlinePool(ref_state["attn.weight"], ref_state["attn.bias"])
        for t in range(41):
            pool.step(top[b, t])
            assert pool.steps == t + 1
            worst = max(worst, float(np.abs(pool.pooled - refs[t + 1]["pooled"][b]).max()))
    print(f"online pooling vs oracle pooled, residual={residual}: {worst:.2e}")
    assert worst < 2e-5
    assert [sum(c) for c in sr.CUTS_41] == [41] * 4 and sr.cut_points([40, 1]) == [40, 41]


def _collect(proc, q, n):
    proc.start()
    try:
        return [q.get(timeout=30) for _ in range(n)]
    finally:
        proc.stop()
        proc.join(timeout=5)
        if proc.is_alive():
            proc.terminate()


def test_chunked_producer_protocol_and_the_untouched_default():
    T, Cn = int(2.0 * SAMPLING_RATE), 8
    windows = [synthetic_window(T, Cn, rs) for rs in [np.random.RandomState(11)] for _ in range(2)]
    # default: today's payloads -- whole windows, the four keys
    q = Queue(maxsize=8)
    got = _collect(StreamingProcess("synthetic:11", Cn, 2.0, q, True), q, 2)
    for p, w in zip(got, windows):
        assert set(p) == {"sr", "channels", "data", "t_emit"}
        assert p["sr"] == SAMPLING_RATE and p["channels"] == list(range(1, 9)) and np.array_equal(p["data"], w)
    # chunk_seconds = 0.3 s = 37 samples: 250 = 6 * 37 + 28
    q = Queue(maxsize=8)
    proc = StreamingProcess("synthetic:11", Cn, 2.0, q, True, chunk_seconds=0.3)
    assert proc.chunk_seconds == 0.3
    got = _collect(proc, q, 14)
    for k, w in enumerate(windows):
        part = got[7 * k:7 * k + 7]
        assert [p["seq"] for p in part] == list(range(7)) and [p["last"] for p in part] == [False] * 6 + [True]
        assert [p["data"].shape[0] for p in part] == [37] * 6 + [28]
        assert np.array_equal(np.concatenate([p["data"] for p in part]), w)
        for p in part:
            assert set(p) == {"sr", "channels", "data", "t_emit", "seq", "last"} and p["data"].dtype == np.float32
            assert p["sr"] == SAMPLING_RATE and p["channels"] == list(range(1, 9))
    # a chunk longer than the window: one chunk, first and last
    q = Queue(maxsize=8)
    one = _collect(StreamingProcess("synthetic:11", Cn, 2.0, q, True, chunk_seconds=5.0), q, 1)[0]
    assert one["seq"] == 0 and one["last"] is True and np.array_equal(one["data"], windows[0])
    for bad in (0, -1.0):
        with pytest.raises(ValueError):
            StreamingProcess("synthetic:", Cn, 2.0, Queue(), chunk_seconds=bad)
    import inspect
    rt = inspect.signature(nsd_amd.run_trials).parameters
    assert rt["chunk_seconds"].default is None and rt["chunk_seconds"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(StreamingProcess.__init__).parameters["chunk_seconds"].default is None


def test_stream_decoder_needs_the_gpu_and_says_so():
    m = nsd_amd.EEG_LSTM().eval()
    with pytest.raises(nsd_amd.NsdError, match="GPU"):
        nsd_amd.StreamDecoder(m)
    with pytest.raises(nsd_amd.NsdError, match="eval"):
        nsd_amd.StreamDecoder(nsd_amd.EEG_LSTM())
    with pytest.raises(nsd_amd.NsdError, match="z-score"):
        nsd_amd.StreamDecoder(nsd_amd.EEG_LSTM(normalize=True).eval())
    with pytest.raises(nsd_amd.NsdError, match="nsd_stream_path"):
        nsd_amd.StreamDecoder(nsd_amd.EEG_LSTM(hidden_size=32).eval())
    with pytest.raises(nsd_amd.NsdError, match="bf16"):
        nsd_amd.StreamDecoder(nsd_amd.EEG_LSTM(hidden_size=64, precision="bf16").eval())


def test_stream_kernels_have_no_private_segment(tmp_path):
    notes = device_elf("nsd_stream48", str(tmp_path))
    sizes = {}
    for block in re.split(r"^\s*- \.agpr_count:", notes, flags=re.M)[1:]:
        kv = dict(re.findall(r"^\s*(\.[a-z_]+):\s*(.+?)\s*$", block, re.M))
        sizes[kv[".name"]] = int(kv[".private_segment_fixed_size"], 0)
    assert len(sizes) == 2 and any("stream48_kernel" in k for k in sizes) and any("stream_reset_kernel" in k for k in sizes), sorted(sizes)
    assert all(v == 0 for v in sizes.values()), sizes
