"""Session calibration on the host: the float64 restatement of nsd_head_fit (tests/head_fit_ref.py) against torch autograd +
torch.optim.Adam, its epoch <-> stream numbering against the trainers', the state layout and the path's LDS arithmetic against the
library's host entry points, and the declarations of the new symbols.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import torch

import nsd_amd
from nsd_amd import _lib, ops, step_recipe
from oracle import nsd_oracle as orc
from tests import head_fit_ref as hf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nsd_stream_features", "nsd_head_fit_path", "nsd_head_fit_state_bytes", "nsd_head_fit_state_layout", "nsd_head_fit")


def problem(N, H, F, K, seed):
    rs = np.random.RandomState(seed)
    theta = {k: 0.3 * rs.standard_normal(shp) for k, shp in hf.tail_shapes(H, F, K).items()}
    theta["ln.weight"] = 1.0 + 0.2 * rs.standard_normal(H)
    feats = rs.standard_normal((N, H)) * (1.0 + rs.rand(N, 1))
    labels = rs.randint(0, K, N)
    return theta, feats, labels


def smoothed_targets(labels, K, smoothing, weights):
    """nsd_mixup's rows at mix = 0: w_k * (k == label ? (1 - eps) + eps / K : eps / K)"""
    base = np.full((len(labels), K), smoothing / K)
    base[np.arange(len(labels)), labels] += 1.0 - smoothing
    return base * np.asarray(weights)[None, :]


def test_restatement_matches_torch_autograd_and_adam_over_five_epochs():
    N, H, F, K, E = 7, 48, 32, 3, 5
    theta, feats, labels = problem(N, H, F, K, seed=3)
    q = smoothed_targets(labels, K, 0.1, [1.0, 2.5, 0.5])
    rs = np.random.RandomState(11)
    masks = [(rs.uniform(1 / 8, 1 / 3, (N, F)), (rs.rand(N, F) >= 0.4) / 0.6) for _ in range(E)]
    kw = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.05)
    ref = hf.HeadFitRef(theta, H, F, K, fp32_fields=False, **kw)
    losses = ref.fit(feats, q, 1.0 / N, E, masks=masks)

    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in theta.items()}
    opt = torch.optim.Adam([t[k] for k in hf.TAIL], lr=kw["lr"], betas=(kw["beta1"], kw["beta2"]), eps=kw["eps"], weight_decay=kw["weight_decay"])
    x, qt = torch.tensor(feats, dtype=torch.float64), torch.tensor(q, dtype=torch.float64)
    tl = []
    for slope, drop in masks:
        opt.zero_grad()
        ln = torch.nn.functional.layer_norm(x, (H,), t["ln.weight"], t["ln.bias"], eps=1e-5)
        pre = torch.nn.functional.linear(ln, t["fc.0.weight"], t["fc.0.bias"])
        z = torch.where(pre >= 0, pre, pre * torch.tensor(slope)) * torch.tensor(drop)
        logits = torch.nn.functional.linear(z, t["fc.3.weight"], t["fc.3.bias"])
        loss = -(qt * torch.log_softmax(logits, -1)).sum() / N
        loss.backward()
        tl.append(float(loss.detach()))
        opt.step()
    np.testing.assert_allclose(losses, tl, rtol=1e-10)
    got = ref.theta()
    for k in hf.TAIL:
        np.testing.assert_allclose(got[k], t[k].detach().numpy(), rtol=1e-10, atol=1e-14, err_msg=k)
    assert ref.count == E


def test_train_mask_freezes_the_other_groups_and_keeps_the_gradient_flowing():
    N, H, F, K = 5, 48, 9, 4
    theta, feats, labels = problem(N, H, F, K, seed=5)
    q = smoothed_targets(labels, K, 0.0, np.ones(K))
    full = hf.HeadFitRef(theta, H, F, K, lr=1e-2)
    full.fit(feats, q, 1.0 / N, 1)
    for train in (("ln",), ("fc0",), ("fc3",), ("ln", "fc3")):
        part = hf.HeadFitRef(theta, H, F, K, lr=1e-2, train=train)
        part.fit(feats, q, 1.0 / N, 1)
        idx = hf.trained_index(train, H, F, K)
        assert np.array_equal(part.vec[~idx], hf.tail_vector(theta, H, F, K)[~idx])
        assert np.array_equal(part.vec[idx], full.vec[idx])            # the first epoch's update does not depend on the mask
        assert np.abs(part.vec[idx] - hf.tail_vector(theta, H, F, K)[idx]).max() > 0


def test_epoch_numbering_is_the_trainers_step_numbering_for_a_batch_of_n_trials():
    """global epoch e of nsd_head_fit draws streams base + 4e + {1, 2}: with base_stream = 0, what a trainer's step e draws for B = N"""
    seed, N, F, p = 77, 13, 32, 0.3
    for e in (0, 1, 5, 1000):
        rng = step_recipe.step_rng(seed, e, p_lstm=0.0, p_head=p)
        slope, drop = hf.epoch_masks(seed, 0, e, p, N, F)
        assert np.array_equal(slope, orc.rrelu_noise(seed, rng["base_stream"] + ops.SLOT_RRELU, (N, F)))
        assert np.array_equal(drop, orc.dropout_mask(seed, rng["base_stream"] + ops.SLOT_HEAD_DROPOUT, p, (N, F)))
    a = hf.epoch_masks(seed, 0xFFFFFFFE, 1, p, N, F)                  # uint32 wrap of the stream id
    assert np.array_equal(a[0], orc.rrelu_noise(seed, 3, (N, F))) and np.array_equal(a[1], orc.dropout_mask(seed, 4, p, (N, F)))
    a, b = hf.epoch_masks(seed, 0, 2, p, N, F), hf.epoch_masks(seed, 8, 0, p, N, F)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert set(np.unique(b[1])) <= {0.0, float(np.float32(1.0 / (1.0 - np.float32(p))))}


def test_state_layout_and_path_arithmetic_match_the_library():
    L = nsd_amd.load_library()
    for F, K in ((32, 3), (32, 8), (64, 8), (33, 9), (1, 64), (64, 64)):
        spec = ops.ModelSpec(C=8, H=48, L=2, K=K, F=F)
        lay, ref = ops.head_fit_layout(spec), hf.state_layout(48, F, K)
        assert {k: int(getattr(lay, k)) for k in ref} == ref
        assert ref["epochs"] % 2 == 0 and ref["epochs"] >= 2 * hf.tail_count(48, F, K) and ref["stride"] % 4 == 0
        assert ref["status"] >= ref["epochs"] + 2 and ref["stride"] > ref["status"]
        d = spec.dims(1, 1)
        for M in (1, 3, 32):
            assert int(L.nsd_head_fit_state_bytes(C.byref(d), M)) == 4 * M * ref["stride"]
        assert int(L.nsd_head_fit_state_bytes(C.byref(d), 0)) < 0 and int(L.nsd_head_fit_state_bytes(C.byref(d), 33)) < 0
        n_max = max(n for n in range(1, 257) if hf.lds_bytes(n, 48, F, K) <= 160 * 1024)
        for N in sorted({1, n_max, min(n_max + 1, 256), 256}):
            assert ops.head_fit_path(spec, 1, N) == (N <= n_max), (F, K, N)
        assert not ops.head_fit_path(spec, 1, 0) and not ops.head_fit_path(spec, 1, 257)
        assert not ops.head_fit_path(spec, 0, 1) and not ops.head_fit_path(spec, 33, 1) and ops.head_fit_path(spec, 32, 1)
    # what the header promises: the reference head fits 256 trials; the limits it names at F = 64
    assert all(hf.lds_bytes(256, 48, 32, K) <= 160 * 1024 for K in range(1, 9))
    assert hf.lds_bytes(192, 48, 64, 8) <= 160 * 1024 < hf.lds_bytes(193, 48, 64, 8)
    assert hf.lds_bytes(112, 48, 64, 64) <= 160 * 1024 < hf.lds_bytes(113, 48, 64, 64)
    assert not ops.head_fit_path(ops.ModelSpec(C=8, H=64, L=2, K=3, F=32), 1, 8)          # outside nsd_stream_path


def test_refusals_happen_on_the_host_without_a_gpu():
    """every refusal of nsd_head_fit / nsd_stream_features comes before any launch: it is reachable, and named, with no device"""
    L = nsd_amd.load_library()
    spec = ops.ModelSpec()
    d = spec.dims(12, 1)
    fit = _lib.Fit(5, 7, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0 / 12)
    sbytes = int(L.nsd_head_fit_state_bytes(C.byref(d), 2))
    P = 0x1000                                                          # any non-null address: nothing is dereferenced before a launch

    def call(dd=d, M=2, params=P, feats=P, stride=0, targets=P, f=fit, rng=None, state=P, nbytes=sbytes):
        return L.nsd_head_fit(C.byref(dd) if dd is not None else None, M, params, feats, stride, targets, C.byref(f) if f is not None else None,
                              rng, state, nbytes, None, None)

    def err():
        return L.nsd_last_error().decode()

    for kw in (dict(dd=None), dict(params=None), dict(feats=None), dict(targets=None), dict(f=None), dict(state=None)):
        assert call(**kw) == -1 and "null" in err(), kw
    for kw in (dict(M=0), dict(M=33), dict(dd=spec.dims(0, 1)), dict(dd=spec.dims(257, 1)),
               dict(dd=ops.ModelSpec(C=8, H=64, L=2, K=3, F=32).dims(12, 1)), dict(dd=ops.ModelSpec(K=8, F=64).dims(193, 1))):
        assert call(**kw) == -1 and "nsd_head_fit_path" in err(), kw

    def with_fit(**ch):
        f = _lib.Fit(5, 7, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0 / 12)
        for k, v in ch.items():
            setattr(f, k, v)
        return f

    for ch, word in ((dict(epochs=0), "epochs"), (dict(epochs=65537), "epochs"), (dict(train=0), "train"), (dict(train=8), "train"),
                     (dict(lr=-1.0), "lr"), (dict(lr=float("nan")), "lr"), (dict(beta1=1.0), "betas"), (dict(beta2=-0.1), "betas"),
                     (dict(eps=0.0), "eps"), (dict(eps=float("inf")), "eps"), (dict(weight_decay=-1e-3), "weight_decay"),
                     (dict(scale=float("nan")), "scale")):
        assert call(f=with_fit(**ch)) == -1 and word in err(), ch
    for stride in (-1, 1, 12 * 48 - 1):
        assert call(stride=stride) == -1 and "feats_model_stride" in err()
    for p in (1.0, -0.1, float("nan")):
        rng = (_lib.Rng * 2)(_lib.Rng(1, 0, 0.0, 0.0), _lib.Rng(2, 0, 0.0, p))
        assert call(rng=rng) == -1 and "rng[1].p_head" in err()
    assert call(nbytes=sbytes - 1) == -3 and "nsd_head_fit_state_bytes" in err()

    sd = spec.dims(0, 1)
    lay = ops.stream_layout(spec)
    nb = 3 * int(lay.stride) * 4
    assert L.nsd_stream_features(C.byref(sd), None, nb, 3, None, 3, P, None) == -1
    assert L.nsd_stream_features(C.byref(sd), P, nb, 3, None, 3, None, None) == -1
    assert L.nsd_stream_features(C.byref(sd), P, nb, 0, None, 0, P, None) == -1
    assert L.nsd_stream_features(C.byref(sd), P, nb, 3, None, -1, P, None) == -1
    assert L.nsd_stream_features(C.byref(sd), P, nb, 3, None, 4, P, None) == -1          # rows 0 .. n-1 need n <= S
    assert L.nsd_stream_features(C.byref(sd), P, nb - 1, 3, None, 3, P, None) == -3
    assert L.nsd_stream_features(C.byref(ops.ModelSpec(C=8, H=64, L=2, K=3, F=32).dims(0, 1)), P, nb, 3, None, 3, P, None) == -1
    assert L.nsd_stream_features(C.byref(sd), P, nb, 3, None, 0, P, None) == 0           # n = 0 launches nothing


def test_header_binding_and_readme_declare_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "nsd.h")).read()
    assert int(re.search(r"#define NSD_VERSION (\d+)", hdr).group(1)) == 301              # additive: detected by the symbols
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(nsd_[a-z0-9_]+)\s*\(", code))
    L = nsd_amd.load_library()
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(L, name), name
    for macro, val in (("NSD_FIT_MAX_TRIALS", 256), ("NSD_FIT_MAX_EPOCHS", 65536), ("NSD_FIT_LN", 1), ("NSD_FIT_FC0", 2), ("NSD_FIT_FC3", 4)):
        assert int(re.search(rf"#define {macro}\s+(\d+)", hdr).group(1)) == val == getattr(_lib, macro)
    assert C.sizeof(_lib.Fit) == 32 and C.sizeof(_lib.FitLayout) == 40
    readme = open(os.path.join(ROOT, "README.md")).read()
    for word in ("nsd_head_fit", "nsd_stream_features", "HeadFit", "calibrate"):
        assert word in readme, word
    assert "nsd_head_fit.hip" in open(os.path.join(ROOT, "neural-speech-decoding_amd", "csrc", "Makefile")).read()
    for name in ("HeadFit",):
        assert hasattr(nsd_amd, name)
    assert ops.fit_mask(("ln", "fc3")) == 5 and ops.fit_mask(("ln", "fc0", "fc3")) == 7
