"""Resumable inference of an ensemble (nsd_multi_stream_* of include/nsd.h): everything that can be held without a GPU -- the ABI
surface, the path query, the state size, every host-side refusal, the mean's fp32 restatement, the decoder's refusal without a GPU,
the new kernels' code object (no private segment) and the argument handling of `train.py --save-folds`."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import nsd_amd
from nsd_amd import _lib, ops
from tests import multi_stream_ref as mr
from tests.code_object import device_elf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nsd_multi_stream_path", "nsd_multi_stream_state_bytes", "nsd_multi_stream_step")
E_INVALID, E_WORKSPACE = -1, -3
PTR = 4096                       # stands for a device pointer: a refusal returns before anything looks at it


def _dims(B=1, T=1, Cc=8, H=48, L=2, K=3, F=32):
    return _lib.Dims(B, T, Cc, H, L, K, F)


def test_symbols_are_declared_bound_and_exported_and_the_version_stays():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nsd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(nsd_[a-z0-9_]+)\s*\(", hdr))
    L = nsd_amd.load_library()
    for name in SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS and hasattr(L, name), name
    assert L.nsd_version() == 301
    assert "nsd_multi_stream48.hip" in open(os.path.join(ROOT, "neural-speech-decoding_amd", "csrc", "Makefile")).read()
    assert "EnsembleStreamDecoder" in nsd_amd.__all__ and issubclass(nsd_amd.EnsembleStreamDecoder, nsd_amd.StreamDecoder)
    for fn in ("multi_stream_path", "multi_stream_state", "multi_stream_step"):
        assert callable(getattr(ops, fn)), fn
    # the header states what a caller leans on: the state layout, the mean, the device-side behaviour
    full = open(os.path.join(ROOT, "include", "nsd.h")).read()
    for words in ("[M][S][stride]", "m * S * stride", "(((p_0 + p_1) + p_2) + ... + p_{M-1}) / (float)M", "mean_probs without probs",
                  "skipped in every model"):
        assert words in full, words


@pytest.mark.parametrize("M,m_ok", [(0, 0), (1, 1), (32, 1), (33, 0), (-1, 0)])
@pytest.mark.parametrize("dims,inside", [
    (dict(), 1), (dict(Cc=1), 1), (dict(Cc=3, K=2), 1), (dict(F=64, K=64), 1), (dict(B=0, T=0), 1), (dict(B=1000, T=100000), 1),
    (dict(H=32), 0), (dict(H=64), 0), (dict(L=1), 0), (dict(L=3), 0), (dict(Cc=9), 0), (dict(F=65), 0), (dict(K=65), 0), (dict(K=0), 0),
])
def test_path_and_state_bytes_over_a_table_of_dims_and_model_counts(dims, inside, M, m_ok):
    L, d = nsd_amd.load_library(), _dims(**dims)
    assert L.nsd_stream_path(C.byref(d)) == inside
    assert L.nsd_multi_stream_path(C.byref(d), M) == (inside & m_ok)
    assert L.nsd_multi_stream_path(None, M) == 0
    for S in (1, 4, 257):
        n = L.nsd_multi_stream_state_bytes(C.byref(d), M, S)
        if inside and m_ok:
            assert n == M * L.nsd_stream_state_bytes(C.byref(d), S) == M * S * ops.stream_layout(ops.ModelSpec()).stride * 4
        else:
            assert n == E_INVALID
    assert L.nsd_multi_stream_state_bytes(C.byref(d), M, 0) == E_INVALID and L.nsd_multi_stream_state_bytes(None, M, 1) == E_INVALID
    if inside:
        spec = ops.ModelSpec(C=d.C, H=d.H, L=d.L, K=d.K, F=d.F)
        assert ops.multi_stream_path(spec, M) == bool(m_ok)
    assert not ops.multi_stream_path(ops.ModelSpec(D=2), 2)


def test_every_host_side_refusal_returns_its_code_without_a_gpu():
    L = nsd_amd.load_library()
    d, S, M = _dims(B=3, T=5), 4, 3
    need = L.nsd_multi_stream_state_bytes(C.byref(d), M, S)
    n_x = 3 * 5 * 8
    err = lambda: L.nsd_last_error().decode()

    def step(dd=d, m=M, params=PTR, x=PTR, stride=0, slots=None, flags=0, state=PTR, nbytes=need, s=S, logits=PTR, probs=PTR, mean=PTR):
        return L.nsd_multi_stream_step(None if dd is None else C.byref(dd), m, params, x, stride, slots, flags, state, nbytes, s, logits,
                                       probs, mean, None)
    # what nsd_stream_step refuses
    assert step(dd=None) == E_INVALID
    assert step(params=None) == E_INVALID and "null" in err()
    assert step(x=None) == E_INVALID and step(state=None) == E_INVALID
    assert step(logits=None, probs=PTR, mean=None) == E_INVALID and "probs without logits" in err()
    assert step(dd=_dims(B=3, T=0)) == E_INVALID and step(dd=_dims(B=-1, T=5)) == E_INVALID
    for bad in (dict(H=32), dict(H=64), dict(L=3), dict(Cc=9), dict(F=65), dict(K=65), dict(K=0)):
        assert step(dd=_dims(B=3, T=5, **bad)) == E_INVALID, bad
    assert "nsd_stream_path" in err() or "bad model dims" in err()
    assert step(dd=_dims(B=5, T=5)) == E_INVALID and "B = 5" in err()
    assert step(dd=_dims(B=5, T=5), slots=PTR) == E_INVALID
    assert step(s=0) == E_INVALID and step(s=-2) == E_INVALID
    assert step(flags=_lib.NSD_FLAG_TRAIN) == E_INVALID and step(flags=_lib.NSD_FLAG_BF16 | _lib.NSD_FLAG_RESIDUAL) == E_INVALID
    # ... and what the model count adds
    for m in (0, -1, 33):
        assert step(m=m) == E_INVALID and "models outside [1, 32]" in err(), m
    assert step(probs=None, mean=PTR) == E_INVALID and "mean_probs without probs" in err()
    assert step(logits=None, probs=None, mean=PTR) == E_INVALID
    for bad in (-1, 1, n_x - 1):
        assert step(stride=bad) == E_INVALID and "x_model_stride" in err(), bad
    assert step(nbytes=need - 1) == E_WORKSPACE and "nsd_multi_stream_state_bytes" in err()
    assert step(nbytes=need // M) == E_WORKSPACE and step(nbytes=0) == E_WORKSPACE      # one model's state is not enough
    assert step(dd=_dims(B=0, T=5)) == 0 and step(dd=_dims(B=0, T=5), stride=0, mean=None) == 0   # nothing to advance: nothing launched
    assert step(dd=_dims(B=0, T=5), m=33) == E_INVALID


@pytest.mark.parametrize("M", [1, 2, 3, 5, 10, 32])
def test_the_mean_restatement_against_float64(M):
    """A serial fp32 sum of M probabilities: the i-th addition rounds a partial sum <= i + 1 (error <= (i + 1) 2^-24), so the sum is
    within (M (M + 1) / 2) 2^-24 and, divided by M, within ((M + 1) / 2) 2^-24; the division of a value <= 1 adds at most 2^-25."""
    rs = np.random.RandomState(500 + M)
    z = rs.standard_normal((M, 64, 5)) * 3.0
    p = (np.exp(z) / np.exp(z).sum(-1, keepdims=True)).astype(np.float32)
    got = mr.mean_probs(p)
    assert got.dtype == np.float32 and got.shape == (64, 5)
    err = float(np.abs(got.astype(np.float64) - p.astype(np.float64).mean(0)).max())
    print(f"M = {M}: fp32 serial mean vs float64 {err:.2e}")
    assert err <= (M + 2) / 2 * 2.0 ** -24
    if M == 1:
        assert got.tobytes() == p[0].tobytes()
    if M == 2:                                                      # one rounding of the sum, an exact halving
        assert got.tobytes() == ((p[0] + p[1]) * np.float32(0.5)).tobytes()


def test_ensemble_stream_decoder_needs_the_gpu_and_says_so():
    pair = lambda **kw: [nsd_amd.EEG_LSTM(**kw).eval(), nsd_amd.EEG_LSTM(**kw).eval()]
    with pytest.raises(nsd_amd.NsdError, match="GPU"):
        nsd_amd.EnsembleStreamDecoder(pair())
    with pytest.raises(nsd_amd.NsdError, match="eval"):
        nsd_amd.EnsembleStreamDecoder([nsd_amd.EEG_LSTM().eval(), nsd_amd.EEG_LSTM()])
    with pytest.raises(nsd_amd.NsdError, match="z-score"):
        nsd_amd.EnsembleStreamDecoder(pair(normalize=True))
    with pytest.raises(nsd_amd.NsdError, match="mixed shapes"):
        nsd_amd.EnsembleStreamDecoder([nsd_amd.EEG_LSTM().eval(), nsd_amd.EEG_LSTM(num_classes=5).eval()])
    with pytest.raises(nsd_amd.NsdError, match="bf16"):
        nsd_amd.EnsembleStreamDecoder(pair(hidden_size=64, precision="bf16"))
    with pytest.raises(nsd_amd.NsdError, match="EEG_LSTM"):
        nsd_amd.EnsembleStreamDecoder([object()])
    with pytest.raises(nsd_amd.NsdError, match="no models"):
        nsd_amd.EnsembleStreamDecoder([])
    # StreamDecoder's own refusals are what they were
    with pytest.raises(nsd_amd.NsdError, match="expected an EEG_LSTM"):
        nsd_amd.StreamDecoder(pair())
    with pytest.raises(nsd_amd.NsdError, match="^StreamDecoder: normalize=True z-scores over the whole window"):
        nsd_amd.StreamDecoder(nsd_amd.EEG_LSTM(normalize=True).eval())


def test_the_model_batched_stream_kernels_have_no_private_segment(tmp_path):
    notes = device_elf("nsd_multi_stream48", str(tmp_path))
    sizes = {}
    for block in re.split(r"^\s*- \.agpr_count:", notes, flags=re.M)[1:]:
        kv = dict(re.findall(r"^\s*(\.[a-z_]+):\s*(.+?)\s*$", block, re.M))
        sizes[kv[".name"]] = int(kv[".private_segment_fixed_size"], 0)
    assert len(sizes) == 2 and any("multi_stream48_kernel" in k for k in sizes) and any("multi_stream_mean_kernel" in k for k in sizes), sorted(sizes)
    assert all(v == 0 for v in sizes.values()), sizes


def test_save_folds_argument_handling(capsys):
    from nsd_amd import train
    for argv in (["--synthetic", "64", "--save-folds"], ["--synthetic", "64", "--kfold", "1", "--save-folds"],
                 ["--synthetic", "64", "--kfold", "2", "--save-folds", "--out", ""]):
        with pytest.raises(SystemExit) as e:
            train.main(argv)
        assert e.value.code == 2 and "--save-folds" in capsys.readouterr().err, argv
