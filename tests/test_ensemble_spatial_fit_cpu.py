"""Ensemble input gradients and the shared alignment fit without a GPU: the ABI's declarations, the refusals that need no device, the
numpy restatement of the mean over the models (NSD_DX_MEAN / nsd_multi_loss_mean) on hand-made arrays, EnsembleSpatialFit's validation,
the parser, and the code-object notes of the model-batched H = 48 backward, which gained the da0 offset in its model view: two kernels
still, and no more private segment or registers than the commit before had (28 B / 127 VGPRs one-trial, 20 B / 128 two-trial)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import nsd_amd
from nsd_amd import _lib
from nsd_amd.align import EnsembleSpatialFit, mean_over_models
from tests import spatial_fit_ref as sr
from tests.code_object import device_elf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nsd_multi_dx_path", "nsd_multi_train_bwd_dx", "nsd_multi_loss_mean")
F32 = np.float32


def test_the_abi_declares_binds_and_exports_the_symbols():
    text = open(os.path.join(ROOT, "include", "nsd.h")).read()
    declared = set(re.findall(r"\b(nsd_[a-z0-9_]+)\s*\(", text))
    L = _lib.lib()
    for name in SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS and hasattr(L, name), name
    assert re.search(rf"#define NSD_DX_PER_MODEL\s+{_lib.NSD_DX_PER_MODEL}\b", text) and re.search(rf"#define NSD_DX_MEAN\s+{_lib.NSD_DX_MEAN}\b", text)
    assert (_lib.NSD_DX_PER_MODEL, _lib.NSD_DX_MEAN) == (0, 1)
    assert re.search(r"#define NSD_VERSION\s+301\b", text) and L.nsd_version() == 301           # additive: detected by the symbols
    for name in ("EnsembleSpatialFit",):
        assert name in nsd_amd.__all__ and hasattr(nsd_amd, name)
    assert all(hasattr(nsd_amd.ops, n) for n in ("multi_dx_path", "multi_train_dx", "multi_loss_mean"))
    assert hasattr(nsd_amd.EnsemblePredictor, "input_gradient")


def test_the_path_predicate_and_the_refusals_before_any_launch():
    L = _lib.lib()
    d = _lib.Dims(3, 20, 8, 48, 2, 3, 32)                                            # B, T, C, H, L, K, F
    assert L.nsd_multi_dx_path(C.byref(d), 1) == 1 and L.nsd_multi_dx_path(C.byref(d), 32) == 1
    assert L.nsd_multi_dx_path(C.byref(d), 0) == 0 and L.nsd_multi_dx_path(C.byref(d), 33) == 0 and L.nsd_multi_dx_path(None, 2) == 0
    assert L.nsd_multi_dx_path(C.byref(_lib.Dims(3, 20, 8, 64, 2, 3, 32)), 2) == 0   # outside nsd_multi_path
    assert L.nsd_multi_dx_path(C.byref(_lib.Dims(3, 1025, 8, 48, 2, 3, 32)), 2) == 0
    fake, INV = C.c_void_p(4096), -1                                                 # never dereferenced: every call below is refused
    stride = 3 * 20 * 8

    def call(dd=d, M=2, p=fake, x=fake, st=stride, fl=0, ws=fake, n=1 << 40, dx=fake, red=0):
        return L.nsd_multi_train_bwd_dx(None if dd is None else C.byref(dd), M, p, x, st, fl, ws, n, dx, red, None)

    cases = [(dict(dd=None), b"dims"), (dict(p=None), b"null"), (dict(x=None), b"null"), (dict(ws=None), b"null"), (dict(dx=None), b"null"),
             (dict(dd=_lib.Dims(3, 20, 8, 64, 2, 3, 32)), b"nsd_multi"), (dict(M=0), b"M = 0"), (dict(M=33), b"M = 33"),
             (dict(red=2), b"reduce = 2"), (dict(red=-1), b"reduce = -1"), (dict(red=1), b"NSD_DX_MEAN"), (dict(red=1, M=1), b"NSD_DX_MEAN"),
             (dict(fl=_lib.NSD_FLAG_RESIDUAL), b"residual"), (dict(st=stride - 1), b"x_model_stride"), (dict(st=-1), b"x_model_stride"),
             (dict(dd=_lib.Dims(1 << 14, 1024, 8, 48, 2, 3, 32), st=0), b"2 GB")]
    for kw, text in cases:
        assert call(**kw) == INV, kw
        assert text in L.nsd_last_error(), (kw, L.nsd_last_error())
    assert call(n=16) == -3 and b"nsd_multi_workspace_bytes" in L.nsd_last_error()   # NSD_E_WORKSPACE
    assert call(dd=_lib.Dims(0, 20, 8, 48, 2, 3, 32), st=0) == 0                     # B = 0: accepted, nothing is launched
    assert L.nsd_multi_loss_mean(C.byref(d), 2, fake, 1 << 40, None, None) == INV and b"null" in L.nsd_last_error()
    assert L.nsd_multi_loss_mean(C.byref(d), 33, fake, 1 << 40, fake, None) == INV
    assert L.nsd_multi_loss_mean(C.byref(d), 2, None, 1 << 40, fake, None) == INV
    assert L.nsd_multi_loss_mean(C.byref(d), 2, fake, 16, fake, None) == -3


def test_the_mean_restatement_on_hand_made_arrays():
    # M = 1: the bits of the only model, the sign of zero included
    one = np.array([[1.5, -0.0, 3e-39, np.inf]], F32)
    assert sr.same_bits(mean_over_models(one), one[0])
    # the sum is serial in fp32 over m ascending: 2^24 + 1 + 1 stays 2^24 (each 1 is lost), while 1 + 1 + 2^24 = 2^24 + 2
    big = F32(2.0 ** 24)
    assert mean_over_models(np.array([[big], [1.0], [1.0]], F32))[0] == F32(big / F32(3))
    assert mean_over_models(np.array([[1.0], [1.0], [big]], F32))[0] == F32(F32(big + F32(2)) / F32(3))
    # one division, not a product with fp32(1 / M): (1 + 1 + 1) / 3 is 1 exactly
    assert mean_over_models(np.ones((3, 4), F32)).tolist() == [1.0] * 4
    v = F32(0.1)
    assert mean_over_models(np.array([[v], [v]], F32))[0] == v                       # (d + d) / 2 is exact
    assert mean_over_models(np.array([[v], [v], [v], [v], [v]], F32))[0] == F32(F32(F32(F32(F32(v + v) + v) + v) + v) / F32(5))
    # a NaN stays in its own element; the shape behind the model axis is kept
    d = np.arange(24, dtype=F32).reshape(2, 3, 4)
    d[1, 2, 1] = np.nan
    out = mean_over_models(d)
    assert out.shape == (3, 4) and out.dtype == F32 and np.isnan(out[2, 1]) and np.isnan(out).sum() == 1
    assert sr.same_bits(np.where(np.isnan(out), 0, out), np.where(np.isnan(out), 0, ((d[0] + d[1]) / F32(2)).astype(F32)))
    with pytest.raises(ValueError, match="M >= 1"):
        mean_over_models(np.zeros((0, 3), F32))


def test_config_validation_and_refusals():
    ok = [nsd_amd.EEG_LSTM(), nsd_amd.EEG_LSTM()]
    with pytest.raises(nsd_amd.NsdError, match="sequence of EEG_LSTM"):
        EnsembleSpatialFit([ok[0], "not a model"])
    with pytest.raises(nsd_amd.NsdError, match="sequence of EEG_LSTM"):
        EnsembleSpatialFit([])
    with pytest.raises(nsd_amd.NsdError, match="another shape"):
        EnsembleSpatialFit([ok[0], nsd_amd.EEG_LSTM(num_classes=5)])
    with pytest.raises(nsd_amd.NsdError, match="more than once"):
        EnsembleSpatialFit([ok[0], ok[0]])
    with pytest.raises(nsd_amd.NsdError):                                            # outside the model-batched path: the limit is named
        EnsembleSpatialFit([nsd_amd.EEG_LSTM(hidden_size=32), nsd_amd.EEG_LSTM(hidden_size=32)])
    for kw in (dict(epochs=0), dict(lr=-1.0), dict(decay=float("inf")), dict(betas=(1.0, 0.9)), dict(eps=0.0)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            EnsembleSpatialFit(ok, **kw)
    with pytest.raises(nsd_amd.NsdError, match="mixup"):
        EnsembleSpatialFit(ok, loss=nsd_amd.Loss(mixup=0.2))
    a, b = (nsd_amd.EEG_LSTM(align=nsd_amd.SessionAlign()) for _ in range(2))
    b.set_alignment(torch.eye(8) * 1.5)
    with pytest.raises(nsd_amd.NsdError, match="another alignment matrix"):
        EnsembleSpatialFit([a, b])
    with pytest.raises(nsd_amd.NsdError, match="no CPU fallback"):
        EnsembleSpatialFit(ok)
    assert all(m.align is None for m in ok)                                          # a refused construction leaves the members as they were
    with pytest.raises(nsd_amd.NsdError, match="no CPU fallback"):
        EnsembleSpatialFit([nsd_amd.EEG_LSTM()])                                     # one member is an ensemble of one
    assert "ONE alignment matrix" in EnsembleSpatialFit.__doc__


def test_cli_takes_several_models_with_fit_spatial():
    from nsd_amd import calibrate
    c = calibrate.build_parser()
    on = c.parse_args(["--model", "a.pth", "--model", "b.pth", "--data", "d", "--out", "o", "--fit-spatial", "--spatial-epochs", "20"])
    assert on.model == ["a.pth", "b.pth"] and on.fit_spatial and on.spatial_epochs == 20
    src = open(os.path.join(ROOT, "neural-speech-decoding_amd", "calibrate.py")).read()
    assert "--fit-spatial takes one --model" not in src and 'spatial["shared"] = True' in src


# the commit before this feature, per kernel: (private segment bytes, VGPRs)
PARENT = {"lstm2_bwd48_multi_kernelILi1E": (28, 127), "lstm2_bwd48_multi_kernelILi2E": (20, 128)}


def test_the_model_batched_backward_kernels_grew_by_nothing(tmp_path):
    notes = device_elf("nsd_lstm2_multi_bwd48", str(tmp_path))
    kernels = {}
    for block in re.split(r"^\s*- \.agpr_count:", notes, flags=re.M)[1:]:
        kv = dict(re.findall(r"^\s*(\.[a-z_]+):\s*(.+?)\s*$", ".agpr_count:" + block, re.M))
        if "lstm2_bwd48" in kv[".name"]:
            kernels[kv[".name"]] = {k: int(kv[k], 0) for k in (".private_segment_fixed_size", ".vgpr_count", ".agpr_count")}
    assert len(kernels) == 2, sorted(kernels)                                        # the one-trial kernel serves dx through its runtime branch
    for key, (private, vgprs) in PARENT.items():
        (sym, rec), = [(k, v) for k, v in kernels.items() if key in k]
        print(sym, rec)
        assert rec[".private_segment_fixed_size"] <= private and rec[".vgpr_count"] <= vgprs and rec[".agpr_count"] == 0, (sym, rec)
    # the feature itself: the model view moves da0_out, and the launcher no longer refuses it
    assert "v.da0_out" in open(os.path.join(ROOT, "neural-speech-decoding_amd", "csrc", "nsd_multi.h")).read()
