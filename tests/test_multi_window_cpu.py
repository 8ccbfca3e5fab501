"""Sliding-window decisions from an ensemble (nsd_multi_window_* of include/nsd.h): everything that can be held without a GPU -- the ABI
surface, the path query and the state size over a table of model counts and (window, hop), every host-side refusal, the new kernels'
code object (no private segment) and the decoder's refusals without a GPU."""
import ctypes as C
import os
import re

import pytest

import nsd_amd
from nsd_amd import _lib, ops
from tests.code_object import device_elf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nsd_multi_window_path", "nsd_multi_window_state_bytes", "nsd_multi_window_step")
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
    assert "nsd_multi_window48.hip" in open(os.path.join(ROOT, "neural-speech-decoding_amd", "csrc", "Makefile")).read()
    assert "EnsembleSlidingStreamDecoder" in nsd_amd.__all__
    assert issubclass(nsd_amd.EnsembleSlidingStreamDecoder, nsd_amd.SlidingStreamDecoder)
    for fn in ("multi_window_path", "multi_window_state", "multi_window_step"):
        assert callable(getattr(ops, fn)), fn
    # the header states what a caller leans on: the state layout, the outputs, the mean, the device-side behaviour
    for words in ("[M][S][stream_stride]", "m * S * stream_stride", "logits [M,B,D,K]", "ends int64 [M,B,D]", "counts int32 [M,B]",
                  "(((p_0 + p_1) + p_2) + ... + p_{M-1}) / (float)M", "mean_probs without probs", "M * B * D * K",
                  "skipped in every model", "skipped for that model alone", "G = min(B*R, max(1, CUs / M))"):
        assert words in full, words


WINDOWS = [((12, 4), 1), ((12, 12), 1), ((1, 1), 1), ((625, 25), 1), ((128, 1), 1),
           ((129, 1), 0), ((12, 5), 0), ((4, 12), 0), ((0, 0), 0), ((12, 0), 0), ((-12, 4), 0), ((12, -4), 0)]


@pytest.mark.parametrize("M,m_ok", [(0, 0), (1, 1), (32, 1), (33, 0), (-1, 0)])
@pytest.mark.parametrize("wh,w_ok", WINDOWS)
@pytest.mark.parametrize("dims,inside", [(dict(), 1), (dict(Cc=3, K=2), 1), (dict(F=64, K=64), 1), (dict(H=32), 0), (dict(L=1), 0),
                                         (dict(Cc=9), 0), (dict(K=0), 0)])
def test_path_and_state_bytes_over_a_table(dims, inside, wh, w_ok, M, m_ok):
    L, d, w = nsd_amd.load_library(), _dims(**dims), _lib.Window(*wh)
    assert L.nsd_window_path(C.byref(d), C.byref(w)) == (inside & w_ok)
    assert L.nsd_multi_window_path(C.byref(d), C.byref(w), M) == (inside & w_ok & m_ok)
    assert L.nsd_multi_window_path(None, C.byref(w), M) == 0 and L.nsd_multi_window_path(C.byref(d), None, M) == 0
    for S in (1, 4, 257):
        n = L.nsd_multi_window_state_bytes(C.byref(d), C.byref(w), M, S)
        if inside and w_ok and m_ok:
            assert n == M * L.nsd_window_state_bytes(C.byref(d), C.byref(w), S) > 0
        else:
            assert n == E_INVALID
    for S in (0, -1):
        assert L.nsd_multi_window_state_bytes(C.byref(d), C.byref(w), M, S) == E_INVALID
    assert L.nsd_multi_window_state_bytes(None, C.byref(w), M, 1) == E_INVALID
    assert L.nsd_multi_window_state_bytes(C.byref(d), None, M, 1) == E_INVALID
    if inside:
        spec = ops.ModelSpec(C=d.C, H=d.H, L=d.L, K=d.K, F=d.F)
        assert ops.multi_window_path(spec, wh[0], wh[1], M) == bool(w_ok and m_ok)
    assert not ops.multi_window_path(ops.ModelSpec(D=2), 12, 4, 2)


def test_every_host_side_refusal_returns_its_code_without_a_gpu():
    L = nsd_amd.load_library()
    d, w, S, M = _dims(B=3, T=5), _lib.Window(12, 4), 4, 3
    need = L.nsd_multi_window_state_bytes(C.byref(d), C.byref(w), M, S)
    n_x = 3 * 5 * 8
    err = lambda: L.nsd_last_error().decode()

    def step(dd=d, ww=w, m=M, params=PTR, x=PTR, stride=0, slots=None, flags=0, state=PTR, nbytes=need, s=S, logits=PTR, probs=PTR, mean=PTR,
             ends=PTR, counts=PTR):
        return L.nsd_multi_window_step(None if dd is None else C.byref(dd), None if ww is None else C.byref(ww), m, params, x, stride, slots,
                                       flags, state, nbytes, s, logits, probs, mean, ends, counts, None)

    # everything nsd_window_step refuses
    assert step(dd=None) == E_INVALID and step(ww=None) == E_INVALID and "null" in err()
    for name in ("params", "x", "state", "logits", "ends", "counts"):
        assert step(**{name: None}) == E_INVALID and "null" in err(), name
    for bad in (dict(H=32), dict(H=64), dict(L=3), dict(Cc=9), dict(F=65), dict(K=65), dict(K=0)):
        assert step(dd=_dims(B=3, T=5, **bad)) == E_INVALID, bad
    for wh, w_ok in WINDOWS:
        if not w_ok:
            assert step(ww=_lib.Window(*wh)) == E_INVALID, wh
    assert "nsd_window_path" in err()
    assert step(dd=_dims(B=3, T=0)) == E_INVALID and step(dd=_dims(B=-1, T=5)) == E_INVALID
    assert step(dd=_dims(B=5, T=5)) == E_INVALID and "B = 5" in err()
    assert step(s=0) == E_INVALID and step(s=-2) == E_INVALID
    assert step(flags=_lib.NSD_FLAG_TRAIN) == E_INVALID and step(flags=_lib.NSD_FLAG_BF16 | _lib.NSD_FLAG_RESIDUAL) == E_INVALID
    # ... and what the model count adds
    for m in (0, -1, 33):
        assert step(m=m) == E_INVALID and "models outside [1, 32]" in err(), m
    assert step(probs=None, mean=PTR) == E_INVALID and "mean_probs without probs" in err()
    for bad in (-1, 1, n_x - 1):
        assert step(stride=bad) == E_INVALID and "x_model_stride" in err(), bad
    assert step(nbytes=need - 1) == E_WORKSPACE and "nsd_multi_window_state_bytes" in err()
    assert step(nbytes=need // M) == E_WORKSPACE and step(nbytes=0) == E_WORKSPACE      # one model's state is not enough
    # M * B * D * K above 2^31 - 1 where B * D * K alone is not: hop 1, so D = T
    one, huge = _lib.Window(1, 1), 2 ** 62
    big = _dims(B=2 ** 20, T=2 ** 4, K=64)                          # B * D * K = 2^30: one model's outputs would pass
    assert step(dd=big, ww=one, m=2, s=2 ** 20, nbytes=huge) == E_INVALID and "M * B * D * K" in err()      # 2^31 exactly
    assert step(dd=_dims(B=2 ** 25, T=1, K=64), ww=one, m=1, s=2 ** 25, nbytes=huge) == E_INVALID and "M * B * D * K" in err()
    # nothing to advance: nothing launched (and the refusals still come first)
    assert step(dd=_dims(B=0, T=5)) == 0 and step(dd=_dims(B=0, T=5), probs=None, mean=None) == 0
    assert step(dd=_dims(B=0, T=5), stride=0, mean=None) == 0
    assert step(dd=_dims(B=0, T=5), m=33) == E_INVALID and step(dd=_dims(B=0, T=5), ww=_lib.Window(12, 5)) == E_INVALID


def test_the_model_batched_window_kernels_have_no_private_segment(tmp_path):
    notes = device_elf("nsd_multi_window48", str(tmp_path))
    sizes = {}
    for block in re.split(r"^\s*- \.agpr_count:", notes, flags=re.M)[1:]:
        kv = dict(re.findall(r"^\s*(\.[a-z_]+):\s*(.+?)\s*$", block, re.M))
        sizes[kv[".name"]] = int(kv[".private_segment_fixed_size"], 0)
    assert len(sizes) == 2 and any("multi_window48_kernel" in k for k in sizes) and any("multi_window_mean_kernel" in k for k in sizes), sorted(sizes)
    assert all(v == 0 for v in sizes.values()), sizes


def test_ensemble_sliding_stream_decoder_needs_the_gpu_and_says_so():
    pair = lambda **kw: [nsd_amd.EEG_LSTM(**kw).eval(), nsd_amd.EEG_LSTM(**kw).eval()]
    with pytest.raises(nsd_amd.NsdError, match="GPU"):
        nsd_amd.EnsembleSlidingStreamDecoder(pair(), window=12, hop=4)
    with pytest.raises(nsd_amd.NsdError, match="nsd_multi_window_path"):
        nsd_amd.EnsembleSlidingStreamDecoder(pair(), window=12, hop=5)
    with pytest.raises(nsd_amd.NsdError, match="eval"):
        nsd_amd.EnsembleSlidingStreamDecoder([nsd_amd.EEG_LSTM().eval(), nsd_amd.EEG_LSTM()], window=12, hop=4)
    with pytest.raises(nsd_amd.NsdError, match="^EnsembleSlidingStreamDecoder: normalize=True z-scores over the whole window"):
        nsd_amd.EnsembleSlidingStreamDecoder(pair(normalize=True), window=12, hop=4)
    with pytest.raises(nsd_amd.NsdError, match="mixed shapes"):
        nsd_amd.EnsembleSlidingStreamDecoder([nsd_amd.EEG_LSTM().eval(), nsd_amd.EEG_LSTM(num_classes=5).eval()], window=12, hop=4)
    with pytest.raises(nsd_amd.NsdError, match="bf16"):
        nsd_amd.EnsembleSlidingStreamDecoder(pair(hidden_size=64, precision="bf16"), window=12, hop=4)
    with pytest.raises(nsd_amd.NsdError, match="EEG_LSTM"):
        nsd_amd.EnsembleSlidingStreamDecoder([object()], window=12, hop=4)
    with pytest.raises(nsd_amd.NsdError, match="no models"):
        nsd_amd.EnsembleSlidingStreamDecoder([], window=12, hop=4)
    with pytest.raises(TypeError):
        nsd_amd.EnsembleSlidingStreamDecoder(pair())                   # window and hop are required
    # the decoders this one is built beside refuse what they refused
    with pytest.raises(nsd_amd.NsdError, match="GPU"):
        nsd_amd.EnsembleStreamDecoder(pair())
    with pytest.raises(nsd_amd.NsdError, match="nsd_window_path"):
        nsd_amd.SlidingStreamDecoder(nsd_amd.EEG_LSTM().eval(), window=12, hop=5)
