"""Cropped training (nsd_crop / nsd_crop_pool), the parts that need no GPU: the numpy restatement the kernels are held to
(tests/crop_ref.py) against its own properties, the draw slots against those of nsd_augment / nsd_mixup, the refusals of the C entry
points, ops.Crop, StepRecipe(crop=) and the command-line flags."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import nsd_amd
from nsd_amd import _lib, ops
from nsd_amd import step_recipe as sr
from tests import augment_ref as ar
from tests import crop_ref as cr
from tests import mixup_ref as mr
from tests import window_ref as wr
from tests.train_cli import parse_train_args

E_INVALID = -1


def _x(B, T, Cc, seed=0):
    return (2.7 * np.random.RandomState(seed).standard_normal((B, T, Cc))).astype(np.float32)


# ---- the numpy restatement by itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,W,R", [(3, 12, 5, 4), (5, 9, 1, 64), (4, 33, 32, 2), (200, 625, 250, 4)])
def test_drawn_offsets_stay_inside_the_trial_and_copy_it(B, T, W, R):
    o = cr.offsets(B, T, W, R, 0, seed=11, base_stream=8)
    assert o.shape == (B, R) and o.min() >= 0 and o.max() <= T - W
    x = _x(B, T, 3)
    lab = np.arange(B, dtype=np.int32) % 3
    tg = _x(B, 1, 3, seed=1)[:, 0]
    y, yl, yt, off = cr.crop(x, W, R, 0, 11, 8, labels=lab, targets=tg)
    assert y.shape == (B * R, W, 3) and np.array_equal(off.reshape(B, R), o)
    for b, r in ((0, 0), (B - 1, R - 1), (B // 2, R // 2)):
        assert y[b * R + r].tobytes() == x[b, o[b, r]:o[b, r] + W].tobytes()
        assert yl[b * R + r] == lab[b] and yt[b * R + r].tobytes() == tg[b].tobytes()
    if B * R >= 400 and T - W >= 8:                                # the draws spread: both ends of the range are reached
        assert o.min() == 0 and o.max() == T - W and len(np.unique(o)) > (T - W) // 2
    # another step, another seed: other offsets; the same call: the same
    if T > W:
        assert not np.array_equal(o, cr.offsets(B, T, W, R, 0, seed=11, base_stream=12))
        assert not np.array_equal(o, cr.offsets(B, T, W, R, 0, seed=12, base_stream=8))
    assert np.array_equal(o, cr.offsets(B, T, W, R, 0, seed=11, base_stream=8))


def test_whole_window_is_offset_zero_and_a_copy():
    x = _x(2, 7, 3)
    y, _, _, off = cr.crop(x, 7, 1, 0, seed=5, base_stream=4)
    assert not off.any() and y.tobytes() == x.tobytes()
    y, _, _, off = cr.crop(x, 7, 5, 0, seed=5, base_stream=4)
    assert not off.any() and all(y[b * 5 + r].tobytes() == x[b].tobytes() for b in range(2) for r in range(5))


@pytest.mark.parametrize("T,W,Hp", [(20, 8, 4), (625, 250, 125), (33, 32, 1), (12, 4, 4), (41, 10, 5)])
def test_regular_grid_is_the_sliding_decoders_windows(T, W, Hp):
    """the windows a trial of T samples completes from a reset state start at the grid's offsets, in row order"""
    done = wr.completed(0, T, W, Hp)
    starts = [end - W for _, end, _ in done]
    g = ops.Crop.grid(T, W, Hp)
    assert g.crops == len(done) and g.hop == Hp and g.span <= T < g.span + Hp
    assert cr.offsets(2, T, W, g.crops, Hp).tolist() == [starts, starts]
    assert [k for k, _, _ in done] == list(range(g.crops)) and [row for _, _, row in done] == list(range(g.crops))


def test_model_draws_do_not_depend_on_the_other_models():
    x = _x(3, 12, 8)
    rngs = [(5, 8), (6, 8), (5, 12)]
    y, _, _, off = cr.crop_models(x, 5, 4, rngs)
    for m, (s, bs) in enumerate(rngs):
        assert y[m].tobytes() == cr.crop(x, 5, 4, 0, s, bs)[0].tobytes()
    assert not np.array_equal(off[0], off[1]) and not np.array_equal(off[0], off[2])


def test_draw_slots_are_disjoint_from_augment_and_mixup():
    """the per-trial slots: nsd_augment draws 0 (shift), 1 (scale), 256 + c (channel drop, c < 256); nsd_mixup 1024 (lambda) and, outside
    the per-trial space, the index 2^63 | 2^62.  The references are read for the slots they pass to trial_index."""
    aug = {0, 1} | set(range(256, 256 + 256))
    for fn, slot in ((ar.shifts, "trial_index(np.arange(B), 0)"), (ar.scales, "trial_index(np.arange(B), 1)"), (ar.dropped, "np.uint64(256)")):
        assert slot in inspect.getsource(fn), fn.__name__
    mix = {mr.LAMBDA_SLOT}
    assert mr.LAMBDA_SLOT == 1024 and "LAMBDA_SLOT" in inspect.getsource(mr.lambdas)
    crop = cr.crop_slots()
    assert crop == set(range(2048, 2048 + _lib.NSD_CROP_MAX)) and not crop & aug and not crop & mix and max(crop) < 1 << 16
    # the indices themselves: no crop draw of any trial is an augment / mixup draw of any trial, nor the rotation's index
    b = np.array([0, 1, 7, 65535, 70000], dtype=np.uint64)
    mine = {int(v) for s in crop for v in ar.trial_index(b, s)}
    theirs = {int(v) for s in aug | mix for v in ar.trial_index(b, s)} | {int(mr.ROT_INDEX)}
    assert not mine & theirs and all(v >> 63 == 1 for v in mine)   # (and the top bit keeps them off the per-element indices)


def test_pool_reference_properties():
    rs = np.random.RandomState(3)
    p = rs.rand(5, 4, 3).astype(np.float32)
    mean, lg = cr.pool(p)
    assert mean.dtype == np.float32 and np.allclose(mean, p.mean(1), atol=1e-6) and np.array_equal(lg, np.log(mean.astype(np.float64)))
    # the serial order: ((p0 + p1) + p2) + p3, not a pairwise tree
    s = ((p[:, 0] + p[:, 1]) + p[:, 2]) + p[:, 3]
    assert np.array_equal(mean, s / np.float32(4))
    # counts: only the first cnt rows; a count outside [1, R] and a non-finite counted value give NaN rows, an uncounted one does not
    q = p.copy()
    q[1, 3, 0] = np.nan
    q[2, 0, 1] = np.inf
    mean, _ = cr.pool(q, counts=[4, 3, 2, 0, 5])
    assert np.array_equal(mean[0], s[0] / np.float32(4)) and np.array_equal(mean[1], ((p[1, 0] + p[1, 1]) + p[1, 2]) / np.float32(3))
    assert np.isnan(mean[2]).all() and np.isnan(mean[3]).all() and np.isnan(mean[4]).all()
    # R = 1: the row itself
    assert np.array_equal(cr.pool(p[:, :1])[0], p[:, 0])


# ---- the C entry points' refusals: before any launch, so no device is needed -------------------------------------------------------------
def _crop(L, d, M=1, x=4096, stride=0, cfg=(5, 4, 0), rng=True, labels=None, targets=None, y=1 << 30, labels_out=None, targets_out=None):
    c = _lib.CropCfg(*cfg) if cfg is not None else None
    r = (_lib.Rng * 32)()
    return L.nsd_crop(C.byref(d), M, x, stride, C.byref(c) if c is not None else None, C.cast(r, C.c_void_p) if rng else None, None,
                      labels, targets, y, labels_out, targets_out, None, None)


def test_crop_refusals_without_a_gpu():
    L = nsd_amd.load_library()
    d = _lib.Dims(3, 12, 8, 48, 2, 3, 32)
    n = 3 * 12 * 8
    err = lambda: L.nsd_last_error()
    for M in (0, -1, _lib.NSD_MAX_MODELS + 1):
        assert _crop(L, d, M=M) == E_INVALID and b"M =" in err()
    assert _crop(L, d, x=None) == E_INVALID and b"null" in err()
    assert _crop(L, d, y=None) == E_INVALID and b"null" in err()
    assert _crop(L, d, cfg=None) == E_INVALID and b"null" in err()
    assert L.nsd_crop(None, 1, 4096, 0, None, None, None, None, None, 1 << 30, None, None, None, None) == E_INVALID
    for W in (0, -1, 13):
        assert _crop(L, d, cfg=(W, 4, 0)) == E_INVALID and b"window" in err()
    for R in (0, -1, _lib.NSD_CROP_MAX + 1):
        assert _crop(L, d, cfg=(5, R, 0)) == E_INVALID and b"crops" in err()
    assert _crop(L, d, cfg=(5, 4, -1)) == E_INVALID and b"hop" in err()
    assert _crop(L, d, cfg=(5, 4, 3)) == E_INVALID and b"regular grid" in err()            # 3 * 3 + 5 = 14 > 12
    assert _crop(L, d, rng=False) == E_INVALID and b"rng" in err()
    assert _crop(L, d, labels_out=1 << 29) == E_INVALID and b"labels_out" in err()
    assert _crop(L, d, targets_out=1 << 29) == E_INVALID and b"targets_out" in err()
    assert _crop(L, _lib.Dims(3, 12, 8, 48, 2, 0, 32), targets=1 << 28, targets_out=1 << 29) == E_INVALID and b"K =" in err()
    assert _crop(L, d, M=3, stride=-1) == E_INVALID and b"x_model_stride" in err()
    assert _crop(L, d, M=3, stride=n - 1) == E_INVALID and b"x_model_stride" in err()
    rows = 3 * 4 * 5 * 8                                                                    # floats of y per model
    assert _crop(L, d, x=4096, y=4096) == E_INVALID and b"overlaps" in err()
    assert _crop(L, d, x=4096, y=4096 + 4 * (n - 1)) == E_INVALID
    assert _crop(L, d, M=3, x=4096 + 4 * (3 * rows - 1), y=4096) == E_INVALID
    assert _crop(L, _lib.Dims(2 ** 30, 12, 8, 48, 2, 3, 32), M=2, cfg=(5, 4, 0), x=4096, y=1 << 50) == E_INVALID and b"2^31" in err()
    for bad in (_lib.Dims(3, 0, 8, 48, 2, 3, 32), _lib.Dims(3, 12, 0, 48, 2, 3, 32), _lib.Dims(-1, 12, 8, 48, 2, 3, 32)):
        assert _crop(L, bad) == E_INVALID
    # B = 0 launches nothing; a regular grid needs no rng; only B, T, C are read
    assert _crop(L, _lib.Dims(0, 12, 8, -5, 99, 0, 0)) == 0
    assert _crop(L, _lib.Dims(0, 12, 8, 48, 2, 3, 32), cfg=(5, 4, 2), rng=False, M=32) == 0
    # the path query is these checks
    q = lambda dd, cfg: L.nsd_crop_path(C.byref(dd), C.byref(_lib.CropCfg(*cfg)))
    assert q(d, (5, 4, 0)) == 1 and q(d, (12, 64, 0)) == 1 and q(d, (5, 4, 2)) == 1 and q(d, (4, 3, 4)) == 1
    assert q(d, (13, 1, 0)) == 0 and q(d, (5, 65, 0)) == 0 and q(d, (5, 4, 3)) == 0 and q(d, (5, 4, -1)) == 0
    assert L.nsd_crop_path(None, None) == 0 and L.nsd_crop_path(C.byref(d), None) == 0


def test_crop_pool_refusals_without_a_gpu():
    L = nsd_amd.load_library()
    f = lambda N=4, R=3, K=3, probs=4096, out=1 << 30: L.nsd_crop_pool(N, R, K, probs, None, out, None, None)
    for kw in (dict(N=-1), dict(R=0), dict(K=0), dict(probs=None), dict(out=None), dict(N=2 ** 20, R=2 ** 10, K=4)):
        assert f(**kw) == E_INVALID and L.nsd_last_error().startswith(b"crop_pool"), kw
    assert f(N=0) == 0


# ---- Python surface -----------------------------------------------------------------------------------------------------------------
def test_crop_dataclass():
    Cr = nsd_amd.Crop
    assert Cr(250) == Cr(250, 1, 0) and Cr(250, 4).span == 250 and Cr(8, 3, 4).span == 16
    for a in ((0,), (-1,), (8, 0), (8, 65), (8, 1, -1), (8.5,), (8, 1.5), (True,)):
        with pytest.raises(ValueError):
            Cr(*a)
    with pytest.raises(Exception):
        Cr(8).window = 3                                           # frozen
    assert Cr.grid(20, 8, 4) == Cr(8, 4, 4) and Cr.grid(625, 250, 125) == Cr(250, 4, 125) and Cr.grid(8, 8, 3) == Cr(8, 1, 3)
    with pytest.raises(ValueError):
        Cr.grid(7, 8, 1)
    Cr(8, 3, 4).check_trial(16)
    for c, T in ((Cr(8, 3, 4), 15), (Cr(8), 7)):
        with pytest.raises(nsd_amd.NsdError):
            c.check_trial(T)


def _recipe(stochastic=True, augment=None, loss=None, crop=None, models=None, **model_kw):
    return sr.StepRecipe(nsd_amd.EEG_LSTM(**model_kw), stochastic, augment, loss, "cpu", models=models, crop=crop)


def test_step_recipe_refusals_and_dims():
    Cr = nsd_amd.Crop
    assert _recipe().crop is None and _recipe().dims(4, 20) == (4, 20)
    r = _recipe(crop=Cr(8, 3))
    assert r.crop == Cr(8, 3) and r.dims(4, 20) == (12, 8)
    with pytest.raises(nsd_amd.NsdError, match="too short"):
        r.dims(4, 7)
    with pytest.raises(nsd_amd.NsdError, match="stochastic=False"):
        _recipe(stochastic=False, crop=Cr(8, 3))
    assert _recipe(stochastic=False, crop=Cr(8, 3, 4)).crop == Cr(8, 3, 4)          # a regular grid draws nothing and stays
    with pytest.raises(ValueError, match="ops.Crop"):
        _recipe(crop="8x3")
    models = [nsd_amd.EEG_LSTM() for _ in range(2)]
    assert _recipe(crop=[Cr(8, 3), Cr(8, 3)], models=models).crop == Cr(8, 3)       # equal entries: the one setting
    with pytest.raises(nsd_amd.NsdError, match="not a per-model setting"):
        _recipe(crop=[Cr(8, 3), Cr(8, 2)], models=models)
    with pytest.raises(nsd_amd.NsdError, match="not a per-model setting"):
        _recipe(crop=[Cr(8, 3), None], models=models)
    with pytest.raises(nsd_amd.NsdError, match="crop entries"):
        _recipe(crop=[Cr(8, 3)], models=models)


@pytest.fixture
def calls(monkeypatch):
    """the ops of StepRecipe.prepare as stand-ins that record (name, arguments) and return CPU tensors of the right shape"""
    rec = []

    def augment(x, aug, rngs, *, M=1, zscore=False, step_dev=None, out=None):
        rec.append(("augment", dict(x=x, zscore=zscore, out=out, step_dev=step_dev, rngs=rngs)))
        return out if out is not None else torch.full(tuple(x.shape), 7.0)

    def zscore(x, out=None):
        rec.append(("zscore", dict(x=x, out=out)))
        return out if out is not None else x + 1.0

    def prep_step(x, prep, state=None, *, slots=None, out=None):
        rec.append(("prep", dict(x=x, out=out)))
        return out if out is not None else x * 2.0

    def crop(x, cfg, rngs=None, *, M=1, labels=None, targets=None, step_dev=None, out=None, labels_out=None, targets_out=None, offsets=None):
        rec.append(("crop", dict(x=x, cfg=cfg, rngs=rngs, M=M, labels=labels, targets=targets, step_dev=step_dev, out=out, labels_out=labels_out)))
        B, T, Cc = x.shape[-3:]
        y = out if out is not None else torch.full((B * cfg.crops, cfg.window, Cc) if M == 1 else (M, B * cfg.crops, cfg.window, Cc), 3.0)
        lo = None if labels is None else (labels_out if labels_out is not None else labels.repeat_interleave(cfg.crops))
        return y, lo, None if targets is None else targets.repeat_interleave(cfg.crops, 0)

    def mixup(x, labels, K, rngs, *, label_smoothing=0.0, mix=0.0, class_weights=None, M=1, step_dev=None, out=None, targets=None):
        rec.append(("mixup", dict(x=x, labels=labels, M=M, out=out, targets=targets)))
        tg = targets if targets is not None else torch.zeros((labels.numel(), K))
        return (None if x is None else out if out is not None else x * 0.5), tg

    for name, f in (("augment", augment), ("zscore", zscore), ("prep_step", prep_step), ("crop", crop), ("mixup", mixup)):
        monkeypatch.setattr(ops, name, f)
    return rec


def _batch(B=4, T=20):
    g = torch.Generator().manual_seed(0)
    return torch.randn((B, T, 8), generator=g), torch.randint(0, 3, (B,), generator=g, dtype=torch.int32)


AUG = nsd_amd.Augment(max_shift=2, noise_std=0.1)
LOSS = nsd_amd.Loss(label_smoothing=0.1, mixup=0.5)


def test_prepare_stage_order_with_a_crop(calls):
    """augment (never z-scoring) -> crop -> z-score of the crops in place -> mixup on crops; labels repeated per crop"""
    c = nsd_amd.Crop(8, 3)
    r = _recipe(augment=AUG, loss=LOSS, normalize=True, crop=c)
    x, y = _batch()
    xo, labels, tg = r.prepare(x, y, [77], 5)
    assert [n for n, _ in calls] == ["augment", "crop", "zscore", "mixup"]
    a, k, z, m = (calls[i][1] for i in range(4))
    assert a["zscore"] is False and torch.equal(a["x"], x)
    assert k["cfg"] == c and k["rngs"] == [sr.step_rng(77, 5)] == a["rngs"] and k["labels"] is y and k["targets"] is None and k["step_dev"] is None
    assert tuple(z["x"].shape) == (12, 8, 8) and z["out"].data_ptr() == z["x"].data_ptr()
    assert tuple(m["x"].shape) == (12, 8, 8) and m["labels"].tolist() == y.repeat_interleave(3).tolist()
    assert tuple(xo.shape) == (12, 8, 8) and labels is None and tuple(tg.shape) == (12, 3)
    # a regular grid draws nothing: no rngs, no step counter
    del calls[:]
    xo, labels, tg = _recipe(crop=nsd_amd.Crop(8, 3, 4)).prepare(x, y, [77], 5)
    assert [n for n, _ in calls] == ["crop"] and calls[0][1]["rngs"] is None and calls[0][1]["step_dev"] is None
    assert tuple(xo.shape) == (12, 8, 8) and labels.tolist() == y.repeat_interleave(3).tolist() and tg is None
    # float target rows are repeated per crop
    del calls[:]
    q = torch.rand(4, 3)
    xo, labels, tg = _recipe(crop=c).prepare(x, q, [77], 5)
    assert labels is None and torch.equal(tg, q.repeat_interleave(3, 0)) and calls[0][1]["labels"] is None
    # crop=None: today's calls (the fused z-score rides in the augment launch)
    del calls[:]
    _recipe(augment=AUG, loss=LOSS, normalize=True).prepare(x, y, [77], 5)
    assert [n for n, _ in calls] == ["augment", "mixup"] and calls[0][1]["zscore"] is True


def test_prepare_static_buffers_with_a_crop(calls):
    c = nsd_amd.Crop(8, 3)
    r = _recipe(augment=AUG, loss=LOSS, normalize=True, crop=c)
    x, y = _batch()
    bufs = dict(x=x, y=y, **r.static_buffers(x))
    assert sorted(bufs) == ["tg", "x", "xc", "xm", "xn", "y", "yc"]
    assert tuple(bufs["xc"].shape) == (12, 8, 8) == tuple(bufs["xm"].shape) and tuple(bufs["yc"].shape) == (12,) and tuple(bufs["tg"].shape) == (12, 3)
    assert bufs["yc"].dtype == torch.int32 and bufs["xn"].shape == x.shape
    step_dev = torch.zeros(1, dtype=torch.int64)
    xo, labels, tg = r.prepare(x, y, [77], 0, step_dev=step_dev, bufs=bufs)
    a, k, z, m = (calls[i][1] for i in range(4))
    assert a["out"] is bufs["xn"] and k["x"] is bufs["xn"] and k["out"] is bufs["xc"] and k["labels_out"] is bufs["yc"] and k["step_dev"] is step_dev
    assert z["out"].data_ptr() == bufs["xc"].data_ptr() and m["x"] is bufs["xc"] and m["labels"] is bufs["yc"] and m["out"] is bufs["xm"]
    assert xo is bufs["xm"] and tg is bufs["tg"]
    # normalize + crop alone: the z-score runs on the crops in place, no trial-sized buffer
    assert sorted(_recipe(normalize=True, crop=c).static_buffers(x)) == ["xc", "yc"]
    assert sorted(_recipe(crop=c).static_buffers(x)) == ["xc", "yc"] and _recipe().static_buffers(x) == {}


def test_prepare_puts_the_crop_behind_the_front_end(calls):
    prep = nsd_amd.CausalPrep.design(fs=125.0, highpass=1.0)
    x, y = _batch()
    _recipe(prep=prep, crop=nsd_amd.Crop(8, 3)).prepare(x, y, [77], 5)
    assert [n for n, _ in calls] == ["prep", "crop"] and tuple(calls[0][1]["x"].shape) == (4, 20, 8)
    assert torch.equal(calls[1][1]["x"], x * 2.0)                  # the crop cuts what the front end made of the whole trial


# ---- command line ---------------------------------------------------------------------------------------------------------------------
def test_cli_flags_parse(monkeypatch):
    from nsd_amd import train
    seen = parse_train_args(["--synthetic", "16", "--crop-seconds", "2.0", "--crops-per-trial", "4", "--crop-hop-seconds", "0.5"], monkeypatch)
    a = seen["args"]
    assert (a.crop_seconds, a.crops_per_trial, a.crop_hop_seconds) == (2.0, 4, 0.5) and seen.get("reached_device")
    assert train.crop_for(a) == (nsd_amd.Crop(250, 4, 0), nsd_amd.Crop(250, 7, 62))
    d = parse_train_args(["--synthetic", "16"], monkeypatch)["args"]
    assert (d.crop_seconds, d.crops_per_trial, d.crop_hop_seconds) == (None, None, None) and train.crop_for(d) is None
    h = parse_train_args(["--synthetic", "16", "--crop-seconds", "2"], monkeypatch)["args"]
    assert train.crop_for(h) == (nsd_amd.Crop(250, 1, 0), nsd_amd.Crop(250, 4, 125))      # H defaults to half the window
    # the grid driver shares the options
    from nsd_amd import grid
    g = grid.build_parser().parse_args(["--synthetic", "16", "--kfold", "2", "--crop-seconds", "3", "--crops-per-trial", "2"])
    assert train.crop_for(g) == (nsd_amd.Crop(375, 2, 0), nsd_amd.Crop(375, 2, 187))


@pytest.mark.parametrize("bad", [["--crops-per-trial", "4"], ["--crop-hop-seconds", "1"], ["--crop-seconds", "6"], ["--crop-seconds", "0"],
                                 ["--crop-seconds", "2", "--crops-per-trial", "65"], ["--crop-seconds", "2", "--crops-per-trial", "0"],
                                 ["--crop-seconds", "2", "--crop-hop-seconds", "0"]])
def test_cli_out_of_range_is_an_argparse_error_before_any_device(bad, monkeypatch, capsys):
    with pytest.raises(SystemExit) as e:
        parse_train_args(["--synthetic", "16"] + bad, monkeypatch)
    assert e.value.code == 2 and "error:" in capsys.readouterr().err


def test_checkpoint_keys_are_additive(tmp_path):
    """a model trained on crops is written with its crop beside the weights; one without is the raw state_dict it was"""
    from nsd_amd.trainer import save_reference_checkpoint
    torch.manual_seed(0)
    plain, cropped = nsd_amd.EEG_LSTM(), nsd_amd.EEG_LSTM(crop=nsd_amd.Crop(250, 4))
    assert plain.crop is None and cropped.crop == nsd_amd.Crop(250, 4)
    with pytest.raises(ValueError, match="ops.Crop"):
        nsd_amd.EEG_LSTM(crop=(250, 4))
    a, b = str(tmp_path / "a.pth"), str(tmp_path / "b.pth")
    save_reference_checkpoint(plain, a)
    save_reference_checkpoint(cropped, b)
    sa, sb = torch.load(a, weights_only=True), torch.load(b, weights_only=True)
    assert sorted(sa) == sorted(plain.state_dict()) and "nsd_crop" not in sa
    assert sorted(sb) == ["nsd_crop", "state_dict"] and sb["nsd_crop"] == dict(window=250, crops=4, hop=0)
    assert sorted(sb["state_dict"]) == sorted(sa)
    both = nsd_amd.EEG_LSTM(prep=nsd_amd.CausalPrep.design(fs=125.0, highpass=1.0), crop=nsd_amd.Crop(250, 4))
    save_reference_checkpoint(both, b)
    assert sorted(torch.load(b, weights_only=True)) == ["nsd_crop", "nsd_prep", "state_dict"]
