"""The whole-window callers of the rate conversion on the MI355X: every surface that gained an ops.resample_trials line (or runs through
open_stream behind a conversion) gives, with resample=r on trials x at the amplifier's rate, BIT FOR BIT (torch.equal / bytes; records
and reports too) what its resample-free twin gives on xr -- the REFERENCE's conversion of x (tests/resample_ref.py), uploaded; not
ops.resample_trials', so a wrong stage 0 cannot cancel, and a removed line shows as another shape or other bits.

The reference model (C = 8, H = 48, L = 2, K = 3; the second ensemble member: its scale = 0.9 twin), the converter (L, M, P) = (1, 2, 7)
with random taps of both signs (built as _rs of tests/test_gpu_resample.py builds them), the smallest shapes the issue names.  The
file holds no tolerance.  The kernel itself is held by tests/test_gpu_resample.py, the decoders by tests/test_gpu_serve_pipeline.py;
tests/test_resample_surfaces_cpu.py holds the call order and the trainers' refusal on the host.

Measured on one MI355X, the file alone: 13 tests, 1.2 s from import to the last test (pytest: 2.9 s with start-up); the slowest test
0.3 s (the first, which loads the kernels).  New at this commit: the parent has no such file (tests/test_gpu_serve_pipeline.py: 1.8 s there).
The mutants this file catches are in the table of tests/test_gpu_serve_pipeline.py (1, 3, 4, 8, 9, 10).
"""
import json
import time

import numpy as np
import pytest
import torch

from tests import resample_ref as rr
from tests.gpu_harness import dev, nsd, sync_at_the_end, to_dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

L, M, P = 1, 2, 7
GATE = dict(rail=100.0, hold_samples=2, max_bad=2)
PREP = dict(highpass=1.0, lowpass=40.0, zscore_seconds=0.4, var0=250.0, car=True)
ALIGN = dict(shrinkage=0.1, floor=1e-4, min_steps=10)
_T0 = time.perf_counter()


def _converter(nsd):
    taps = (np.random.RandomState(1000 * L + 10 * M + P).standard_normal((L, P)) / np.sqrt(P)).astype(np.float32)
    return nsd.Resample(L=L, M=M, P=P, taps=taps)


def _trials(N, T_in, seed):
    """(x [N,T_in,8] at the amplifier's rate, the reference's conversion [N, T_in / 2, 8], labels [N])"""
    rs = np.random.RandomState(seed)
    y = rs.randint(0, 3, N).astype(np.int64)
    x = (10.0 * rs.standard_normal((N, T_in, 8))).astype(np.float32)
    x[np.arange(N), :, y] += 6.0
    taps = (np.random.RandomState(1000 * L + 10 * M + P).standard_normal((L, P)) / np.sqrt(P)).astype(np.float32)
    xr = rr.trials(x, taps, L, M)
    assert xr.shape == (N, T_in // 2, 8) and np.isfinite(xr).all()
    return x, xr, y


def _model(nsd, dev, ref_state, scale=1.0, **kw):
    m = nsd.EEG_LSTM(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v) * np.float32(scale)) for k, v in ref_state.items()}, strict=True)
    return m.to(dev).eval()


def _pair(nsd, dev, ref_state, scale=1.0, **kw):
    """(the model with the conversion, its resample-free twin)"""
    return _model(nsd, dev, ref_state, scale, resample=_converter(nsd), **kw), _model(nsd, dev, ref_state, scale, **kw)


def _front(nsd, gate=True, prep=True, align=False):
    kw = dict(gate=nsd.SignalGate(**GATE) if gate else None, prep=nsd.CausalPrep.design(**PREP) if prep else None)
    if align:
        kw["align"] = nsd.SessionAlign(**ALIGN)
    return kw


def _same_report(a, b, path="report"):
    if isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), path
        for k in a:
            _same_report(a[k], b[k], f"{path}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (u, v) in enumerate(zip(a, b)):
            _same_report(u, v, f"{path}[{i}]")
    elif isinstance(a, (np.ndarray, torch.Tensor)):
        a, b = (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t for t in (a, b))
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), path
    elif isinstance(a, float):
        assert np.float64(a).tobytes() == np.float64(b).tobytes(), (path, a, b)
    else:
        assert a == b, (path, a, b)


# ---- align.py --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [None, [i % 3 for i in range(12)]], ids=["one-matrix", "groups"])
def test_session_align_fit(nsd, dev, ref_state, groups):
    x, xr, _ = _trials(12, 80, 1)
    m, twin = _pair(nsd, dev, ref_state, **_front(nsd))
    cfg = nsd.SessionAlign(**ALIGN)
    (Wa, ra), (Wb, rb) = cfg.fit(m, x, groups=groups), cfg.fit(twin, xr, groups=groups)
    assert tuple(Wa.shape) == ((3 if groups else 1), 8, 8) and torch.equal(Wa, Wb)
    _same_report(ra, rb)
    assert all(r["status"] == 0 and r["steps"] > 0 for r in ra) and sum(r["steps"] + r["skipped"] for r in ra) == 12 * 40


def test_spatial_fit(nsd, dev, ref_state):
    from nsd_amd.align import SpatialFit
    x, xr, y = _trials(6, 64, 2)
    m, twin = _pair(nsd, dev, ref_state, **_front(nsd, gate=False))
    fa, fb = SpatialFit(m, epochs=2), SpatialFit(twin, epochs=2)
    la, lb = fa.fit(x, y), fb.fit(xr, y)
    assert tuple(la.shape) == (2,) and bool(torch.isfinite(la).all()) and torch.equal(la, lb)
    assert torch.equal(fa.A, fb.A) and not torch.equal(fa.A, fa.A0) and torch.equal(m.align_matrix, twin.align_matrix)
    _same_report(m.align_record, twin.align_record)
    _same_report(fa.status(), fb.status())


def test_ensemble_spatial_fit(nsd, dev, ref_state):
    from nsd_amd.align import EnsembleSpatialFit
    x, xr, y = _trials(6, 64, 3)
    pairs = [_pair(nsd, dev, ref_state, s, **_front(nsd, gate=False)) for s in (1.0, 0.9)]
    fa, fb = EnsembleSpatialFit([p[0] for p in pairs], epochs=2), EnsembleSpatialFit([p[1] for p in pairs], epochs=2)
    la, lb = fa.fit(x, y), fb.fit(xr, y)
    assert tuple(la.shape) == (2,) and bool(torch.isfinite(la).all()) and torch.equal(la, lb)
    assert torch.equal(fa.A, fb.A) and not torch.equal(fa.A, fa.A0)
    for a, b in pairs:
        assert torch.equal(a.align_matrix, b.align_matrix) and torch.equal(a.align_matrix, fa.A)
        _same_report(a.align_record, b.align_record)


# ---- EEG_LSTM --------------------------------------------------------------------------------------------------------------------------
def _seeded(nsd, dev, seed, *a, **kw):
    torch.manual_seed(seed)                               # the same seed: the same parameters and the same dropout / RReLU streams
    return nsd.EEG_LSTM(*a, **kw).to(dev)


def _grads(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters()}


def test_forward_in_train_mode_fp32(nsd, dev):
    x, xr, y = _trials(6, 64, 4)
    m, twin = _seeded(nsd, dev, 11, resample=_converter(nsd), **_front(nsd)), _seeded(nsd, dev, 11, **_front(nsd))
    yd = to_dev(y, dev)
    out = []
    for mod, inp in ((m, x), (twin, xr)):
        mod.train()
        logits = mod(to_dev(inp, dev))
        torch.nn.functional.cross_entropy(logits, yd).backward()
        out.append((logits.detach(), _grads(mod)))
    assert tuple(out[0][0].shape) == (6, 3) and torch.equal(out[0][0], out[1][0])
    assert set(out[0][1]) == set(out[1][1]) and all(torch.equal(out[0][1][n], out[1][1][n]) and bool(out[0][1][n].any()) for n in out[0][1])


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_loss_on_the_bf16_path(nsd, dev, mode):
    x, xr, y = _trials(8, 48, 5)
    shape = dict(input_size=8, hidden_size=64, num_layers=2, num_classes=3, precision="bf16")
    prep = nsd.CausalPrep.design(**PREP)
    m, twin = _seeded(nsd, dev, 12, resample=_converter(nsd), prep=prep, **shape), _seeded(nsd, dev, 12, prep=prep, **shape)
    yd = to_dev(y, dev)
    out = []
    for mod, inp in ((m, x), (twin, xr)):
        mod.train(mode == "train")
        logits, loss = mod.loss(to_dev(inp, dev), yd)
        loss.backward()
        out.append((logits.detach(), loss.detach(), _grads(mod)))
    assert tuple(out[0][0].shape) == (8, 3) and torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert bool(torch.isfinite(out[0][1]).all())
    assert all(torch.equal(out[0][2][n], out[1][2][n]) and bool(out[0][2][n].any()) for n in out[0][2])


def test_predict_trials_with_gate_prep_and_alignment(nsd, dev, ref_state):
    x, xr, _ = _trials(5, 80, 6)
    W = (np.eye(8) + 0.15 * np.random.RandomState(7).standard_normal((8, 8))).astype(np.float32)
    m, twin = _pair(nsd, dev, ref_state, align_matrix=to_dev(W, dev), **_front(nsd, align=True))
    (ta, wa), (tb, wb) = m.predict_trials(to_dev(x, dev), window=20, hop=10), twin.predict_trials(to_dev(xr, dev), window=20, hop=10)
    assert tuple(wa.shape) == (5, 3, 3) and torch.equal(ta, tb) and torch.equal(wa, wb) and bool(torch.isfinite(ta).all())


# ---- the predictors --------------------------------------------------------------------------------------------------------------------
def _checkpoints(nsd, dev, ref_state, tmp_path, scales=(1.0,), **kw):
    """-> (paths of checkpoints that carry the conversion, paths of their resample-free twins)"""
    from nsd_amd.trainer import save_reference_checkpoint
    with_r, without = [], []
    for i, s in enumerate(scales):
        plain = _model(nsd, dev, ref_state, s, **kw)
        a, b = str(tmp_path / f"r{i}.pth"), str(tmp_path / f"p{i}.pth")
        save_reference_checkpoint(plain, a, resample=_converter(nsd))          # the sanctioned route: the conversion goes into the checkpoint
        save_reference_checkpoint(plain, b)
        with_r.append(a)
        without.append(b)
    return with_r, without


def test_ensemble_predictor_predicts_and_refuses_the_input_gradient(nsd, dev, ref_state, tmp_path):
    x, xr, y = _trials(4, 80, 8)
    with_r, without = _checkpoints(nsd, dev, ref_state, tmp_path, (1.0, 0.9), **_front(nsd))
    pa = nsd.EnsemblePredictor(with_r, sr=250, device="cpu", preprocess="identity")
    pb = nsd.EnsemblePredictor(without, sr=125, device="cpu", preprocess="identity")
    assert pa.model.resample == _converter(nsd) and pb.model.resample is None and pa.model_rate == 125.0
    for i in range(4):
        (qa, la), (qb, lb) = pa.predict(x[i]), pb.predict(xr[i])
        assert qa.tobytes() == qb.tobytes() and la == lb and np.isfinite(qa).all()
    with pytest.raises(nsd.NsdError, match="dx through the rate conversion"):
        pa.input_gradient(x, y)
    plain_r, plain = _checkpoints(nsd, dev, ref_state, tmp_path, (1.0, 0.9))
    with pytest.raises(nsd.NsdError, match="dx through the rate conversion"):
        nsd.EnsemblePredictor(plain_r, sr=250, device="cpu", preprocess="identity").input_gradient(x, y)
    g = nsd.EnsemblePredictor(plain, sr=125, device="cpu", preprocess="identity").input_gradient(xr, y)      # (the twin is served)
    assert g.shape == xr.shape and np.isfinite(g).all()


def test_calibrate_with_alignment(nsd, dev, ref_state, tmp_path):
    x, xr, y = _trials(9, 80, 9)
    with_r, without = _checkpoints(nsd, dev, ref_state, tmp_path, **_front(nsd, align=True))
    pa = nsd.SimplePredictor(with_r[0], sr=250, device="cpu", preprocess="identity")
    pb = nsd.SimplePredictor(without[0], sr=125, device="cpu", preprocess="identity")
    ra, rb = pa.calibrate(x, y, align=True, epochs=5), pb.calibrate(xr, y, align=True, epochs=5)
    assert ra["n"] == 9 and "align" in ra and ra["align"]["steps"] > 0
    _same_report(ra, rb)
    assert torch.equal(pa.model.flat_parameters(), pb.model.flat_parameters()) and torch.equal(pa.model.align_matrix, pb.model.align_matrix)
    assert not torch.equal(pa.model.align_matrix.cpu(), torch.eye(8))


def test_predictor_streams_through_a_chunk_that_emits_no_step(nsd, dev, ref_state, tmp_path):
    x, _, _ = _trials(2, 80, 10)
    taps = _converter(nsd).taps
    with_r, without = _checkpoints(nsd, dev, ref_state, tmp_path, **_front(nsd))
    pa = nsd.SimplePredictor(with_r[0], sr=250, device="cpu", preprocess="identity")
    pb = nsd.SimplePredictor(without[0], sr=125, device="cpu", preprocess="identity")
    for sliding in (False, True):
        kw = dict(window_seconds=20 / 125.0, hop_seconds=10 / 125.0) if sliding else {}
        sa, sb = pa.open_stream(streams=2, **kw), pb.open_stream(streams=2, **kw)
        n_in, hist, t, seen, empty = None, None, 0, 0, 0
        for n in (7, 1, 1, 40, 31):                       # 7 -> 8 samples: no step at 1 / 2
            yr, cnt, n_in, hist = rr.step_batch(x[:, t:t + n], taps, L, M, rr.ceil_div(n * L, M), n_in, hist)
            got = sa.push(x[:, t:t + n])
            t += n
            if cnt[0] == 0:
                empty += 1
                assert got is None if not sliding else got == [[], []]
                continue
            want = sb.push(yr[:, :cnt[0]])
            if sliding:
                assert [[(e, q.tobytes(), l) for e, q, l in row] for row in got] == [[(e, q.tobytes(), l) for e, q, l in row] for row in want]
                seen += sum(len(row) for row in got)
            else:
                assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1] and np.isfinite(got[0]).all()
        assert empty == 1 and sa.steps.tolist() == sb.steps.tolist() == [40, 40] and sa.decoder.input_steps.tolist() == [80, 80]
        assert not sliding or seen == 2 * 3


# ---- grid --input-rate ------------------------------------------------------------------------------------------------------------------
def test_grid_with_an_input_rate_trains_on_the_reference_conversion(nsd, dev, capsys, monkeypatch):
    """end to end on --synthetic: the runs of `grid --input-rate 250` are, line for line, the runs of the same command with the
    loaded trials converted by the reference instead (stage 0 is the only thing that differs), and they are runs on 40 samples"""
    from nsd_amd import grid, train
    argv = ["--synthetic", "24", "--T", "80", "--kfold", "2", "--epochs", "1", "--batch", "6", "--seed", "3", "--input-rate", "250",
            "--grid", "lr=1e-3,1e-2"]

    def lines():
        out = [json.loads(s) for s in capsys.readouterr().out.strip().splitlines() if s.startswith("{")]
        for rec in out:
            for k in [k for k in rec if "time" in k or "sec" in k or k.endswith("_s") or "per_s" in k]:
                del rec[k]
        return out
    assert grid.main(argv) == 0
    mine = lines()
    seen = {}

    def by_reference(x_np, resample, dev_):
        seen["shape"] = x_np.shape
        return rr.trials(x_np, resample.taps, resample.L, resample.M)
    monkeypatch.setattr(train, "resample_loaded", by_reference)      # (grid takes it from train inside main)
    assert grid.main(argv) == 0
    theirs = lines()
    assert seen["shape"] == (24, 80, 8) and len(mine) == len(theirs) >= 2
    _same_report(mine, theirs)


def test_wall_time_of_this_file():
    """(the last test) -- the figure the docstring records"""
    print(f"tests/test_gpu_resample_surfaces.py: {time.perf_counter() - _T0:.1f} s since the file was imported")
