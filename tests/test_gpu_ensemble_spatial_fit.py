"""The shared supervised alignment fit of an ensemble on the MI355X (nsd_amd.EnsembleSpatialFit over nsd_multi_train_bwd_dx(NSD_DX_MEAN) and
nsd_multi_loss_mean; calibrate(spatial=dict(shared=True, ...)); EnsemblePredictor.input_gradient).

Everything here is a BITWISE statement, so no bound is chosen: one member and two copies of one model leave SpatialFit's bits; three
distinct members are held, epoch by epoch, to a restatement built from pieces the suite already holds -- per member ops.train_dx on the
applied trials (the single-model path), the serial mean in numpy (align.mean_over_models), spatial_fit_ref.bwd_ref and FitRef for dA and
the Adam step.  N = 6 trials of 20 steps, 8 channels, at most 5 epochs (18 trials in the launch: the one-trial band, where the
model-batched dx is the single-model one bit for bit)."""
import contextlib

import numpy as np
import pytest
import torch

from tests import spatial_fit_ref as sr
from tests.buffer_contract import snapshot
from tests.gpu_harness import dev, nsd, sync_at_the_end, to_dev, write_pth  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

KW = dict(lr=1e-4, decay=0.0)
EPOCH = ["nsd_spatial_apply", "nsd_multi_train_fwd", "nsd_multi_train_bwd_dx", "nsd_multi_loss_mean", "nsd_spatial_bwd", "nsd_spatial_fit_step"]
NEW = ("nsd_multi_train_bwd_dx", "nsd_multi_loss_mean", "nsd_multi_dx_path")


def _eval_model(nsd, dev, state, **kw):
    m = nsd.EEG_LSTM(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}, strict=True)
    return m.to(dev).eval()


def _member_states(ref_state, M):
    """the reference checkpoint and M - 1 relatives of it: every tensor moved by 5 % of its own spread"""
    out = [dict(ref_state)]
    for m in range(1, M):
        rs = np.random.RandomState(100 + m)
        out.append({k: (np.asarray(v) + 0.05 * float(np.asarray(v).std() + 1e-3) * rs.standard_normal(np.shape(v))).astype(np.float32)
                    for k, v in ref_state.items()})
    return out


@pytest.fixture(scope="module")
def shifted(golden):
    """6 recorded trials (their first 20 steps) mixed by a fixed 8 x 8 matrix, and labels: the reference's decisions on the whole trials"""
    z = golden("real_trials")
    rs = np.random.RandomState(21)
    mix = (np.eye(8) + 0.25 * rs.standard_normal((8, 8))).astype(np.float32)
    x = np.ascontiguousarray(z["x"][:6, :20].astype(np.float32) @ mix.T)
    return x, z["argmax"][:6].astype(np.int64)


def _names_of(fn):
    from nsd_amd import ops
    names = []

    @contextlib.contextmanager
    def hook(name):
        names.append(name)
        yield
    ops.set_launch_hook(hook)
    try:
        out = fn()
    finally:
        ops.set_launch_hook(None)
    return names, out


def _moments(ops, fit):
    r = ops.spatial_fit_records(8, 1, fit.state)[0]
    return np.asarray(r["m"]), np.asarray(r["v"]), r["step"]


def test_one_member_and_two_copies_leave_the_bits_of_spatial_fit(nsd, dev, ref_state, shifted):
    from nsd_amd import ops
    x, y = shifted
    single = nsd.SpatialFit(_eval_model(nsd, dev, ref_state), epochs=4, **KW)
    want = single.fit(x, y).cpu().numpy()
    wm, wv, ws = _moments(ops, single)
    for copies in (1, 2):
        members = [_eval_model(nsd, dev, ref_state) for _ in range(copies)]
        fit = nsd.EnsembleSpatialFit(members, epochs=4, **KW)
        got = fit.fit(x, y).cpu().numpy()
        m, v, s = _moments(ops, fit)
        assert sr.same_bits(got, want) and sr.same_bits(fit.A.cpu().numpy(), single.A.cpu().numpy()), copies
        assert sr.same_bits(m, wm) and sr.same_bits(v, wv) and s == ws == 4, copies
        assert fit.status() == [0] and fit.epochs_done() == 4 and fit.M == copies
    assert np.isfinite(want).all() and want[1] < want[0]


def test_three_members_epoch_by_epoch_against_the_restatement(nsd, dev, ref_state, shifted):
    from nsd_amd import ops
    from nsd_amd.align import mean_over_models
    x, y = shifted
    M, N, T, E = 3, x.shape[0], x.shape[1], 4
    kw = dict(lr=1e-3, decay=1e-2)
    members = [_eval_model(nsd, dev, st) for st in _member_states(ref_state, M)]
    snap = snapshot(*[m.flat_parameters() for m in members])
    fit = nsd.EnsembleSpatialFit(members, epochs=1, graph=False, **kw)
    assert torch.equal(fit.A0, torch.eye(8, device=dev)) and all(m.align is not None for m in members)
    # the restatement's side: the single-model launches per member, numpy for the mean, dA and the step
    sp = members[0].spec
    v, yt = to_dev(x, dev), to_dev(y.astype(np.int32), dev)
    ref, A, A0 = sr.FitRef(8, 1), np.eye(8, dtype=np.float32)[None].copy(), np.eye(8, dtype=np.float32)[None].copy()
    ws, logits = ops.new_workspace(sp, N, T, dev), torch.empty((N, sp.K), device=dev)
    for e in range(E):
        xa = ops.spatial_apply(v, to_dev(A[0], dev))
        dxs, sums = [], []
        for m in members:
            dx, loss1 = torch.empty_like(xa), torch.zeros(1, device=dev)
            ops.train_dx(sp, m.flat_parameters(), xa, ws, logits, dx, labels=yt, loss_out=loss1)
            dxs.append(dx.cpu().numpy())
            sums.append(loss1.cpu().numpy()[0])
        dmean = mean_over_models(np.stack(dxs))
        _, dA, _ = sr.bwd_ref(x, dmean, A[0])
        want_loss = np.full(1, np.nan, np.float32)
        ref.calls = 0                                                                  # (each fit() call indexes its own losses)
        ref.step(A, dA, A0, loss_in=mean_over_models(np.asarray(sums, np.float32)), loss_out=want_loss, **kw)
        got = fit.fit(x, y, epochs=1).cpu().numpy()                                   # one more epoch of the same run
        m_, v_, s_ = _moments(ops, fit)
        assert sr.same_bits(fit.A.cpu().numpy(), A[0]), e
        assert sr.same_bits(m_, ref.m[0]) and sr.same_bits(v_, ref.v[0]) and s_ == e + 1, e
        # (fit() returns losses / N as torch divides a device tensor by a scalar: the same operation on the restated sum)
        assert sr.same_bits(got, (to_dev(want_loss, dev) / float(N)).cpu().numpy()) and np.isfinite(got).all(), e
    assert snap.unchanged()                                                            # the members' parameters are never written
    assert not np.array_equal(A[0], np.eye(8, dtype=np.float32)) and fit.status() == [0] and fit.epochs_done() == E
    # every member holds the fitted matrix and the record
    for m in members:
        assert sr.same_bits(m.align_matrix.cpu().numpy(), A[0])
        rec = m.align_record["spatial_fit"]
        assert rec["members"] == M and rec["shared"] is True and rec["epochs"] == E and rec["lr"] == 1e-3 and rec["status"] == 0


def test_eager_replayed_and_continued_runs_agree_and_reset_and_status(nsd, dev, ref_state, shifted):
    x, y = shifted
    states = _member_states(ref_state, 3)
    runs = {}
    for name, graph in (("eager", False), ("graph", True), ("2+3", None)):
        members = [_eval_model(nsd, dev, st) for st in states]
        fit = nsd.EnsembleSpatialFit(members, epochs=5, graph=graph, **KW)
        if name == "2+3":
            losses = torch.cat([fit.fit(x, y, epochs=2), fit.fit(x, y, epochs=3)])
        else:
            losses = fit.fit(x, y)
        assert fit.replayed == (name != "eager") and fit.capture_error is None and fit.status() == [0] and fit.epochs_done() == 5
        fit.check()
        runs[name] = (losses.cpu().numpy(), fit.A.cpu().numpy(), fit)
    for name in ("graph", "2+3"):
        assert sr.same_bits(runs[name][0], runs["eager"][0]) and sr.same_bits(runs[name][1], runs["eager"][1]), name
    losses, _, fit = runs["eager"]
    print("EnsembleSpatialFit losses", losses)
    assert np.isfinite(losses).all() and losses[1] < losses[0]
    fit.reset()
    assert fit.epochs_done() == 0 and fit.status() == [0]
    # a non-finite step in the frozen input: every epoch is refused on the device, the matrix stays
    bad = x.copy()
    bad[2, 7, 1] = np.nan
    stuck = nsd.EnsembleSpatialFit([_eval_model(nsd, dev, st) for st in states], epochs=2)
    stuck.fit(bad, y)
    assert stuck.status() == [1] and stuck.epochs_done() == 0 and torch.equal(stuck.A, torch.eye(8, device=dev))
    with pytest.raises(nsd.NsdError, match="not finite"):
        stuck.check()
    stuck.reset()
    assert stuck.status() == [0]
    # members that hold different matrices are refused; label smoothing builds target rows
    a, b = (_eval_model(nsd, dev, st, align=nsd.SessionAlign()) for st in states[:2])
    b.set_alignment(np.eye(8, dtype=np.float32) * 2)
    with pytest.raises(nsd.NsdError, match="another alignment matrix"):
        nsd.EnsembleSpatialFit([a, b])
    soft = nsd.EnsembleSpatialFit([_eval_model(nsd, dev, st) for st in states], epochs=2, loss=nsd.Loss(label_smoothing=0.1), **KW)
    ls = soft.fit(x, y).cpu().numpy()
    assert np.isfinite(ls).all() and ls[0] != float(losses[0]) and soft.status() == [0]


def test_calibrate_shared_runs_the_epochs_six_calls_before_the_head_fit(nsd, dev, ref_state, shifted, tmp_path):
    from nsd_amd import ops
    from nsd_amd.trainer import save_reference_checkpoint
    x, y = shifted
    paths = []
    for i, st in enumerate(_member_states(ref_state, 3)):
        d = tmp_path / f"m{i}"
        d.mkdir()
        paths.append(write_pth(str(d), st))
    # without the keyword, and with spatial=None: the launches of the call as it was -- nothing of the new entry points
    ens = nsd.EnsemblePredictor(paths, 125, preprocess="identity")
    names, rep = _names_of(lambda: ens.calibrate(x, y, epochs=3))
    again = nsd.EnsemblePredictor(paths, 125, preprocess="identity")
    names2, _ = _names_of(lambda: again.calibrate(x, y, epochs=3, spatial=None))
    assert names2 == names and not any(n in NEW or n.startswith("nsd_spatial") for n in names) and "spatial_losses" not in rep
    # a single model: its epoch is the single-model one, with or without shared=True
    for extra in ({}, dict(shared=True)):
        one = nsd.SimplePredictor(paths[0], sr=125, preprocess="identity")
        names3, _ = _names_of(lambda: one.calibrate(x, y, epochs=3, spatial=dict(epochs=2, graph=False, **KW, **extra)))
        k = names3.index("nsd_spatial_bwd")
        assert names3[k - 4:k + 2] == ["nsd_spatial_apply", "nsd_lstm_head_train", "nsd_lstm_bwd", "nsd_loss_sum", "nsd_spatial_bwd",
                                       "nsd_spatial_fit_step"] and not any(n in NEW for n in names3), extra
    # the ensemble with the key
    pred = nsd.EnsemblePredictor(paths, 125, preprocess="identity")
    snap = snapshot(*[p for m in pred.members for n, p in m.named_parameters() if n.startswith("lstm.") or n.startswith("attn")])
    names4, rep = _names_of(lambda: pred.calibrate(x, y, epochs=3, spatial=dict(shared=True, epochs=2, graph=False, **KW)))
    k = names4.index("nsd_spatial_bwd")
    assert names4[k - 4:k + 2] == EPOCH
    assert names4.count("nsd_spatial_bwd") == 2 and names4.count("nsd_multi_train_bwd_dx") == 2 and names4.count("nsd_spatial_fit_step") == 2
    assert names4.index("nsd_head_fit") > len(names4) - 1 - names4[::-1].index("nsd_spatial_fit_step")     # spatial fit, then the head fit
    assert snap.unchanged()
    assert rep["spatial_losses"].shape == (2,) and rep["spatial_status"] == [0] and 0.0 <= rep["acc_spatial"] <= 1.0
    assert np.isfinite(rep["loss_spatial"]) and rep["spatial_losses"][1] < rep["spatial_losses"][0]
    for m in pred.members:
        assert m.align is not None and torch.equal(m.align_matrix, pred.members[0].align_matrix)
        assert m.align_record["spatial_fit"]["members"] == 3 and m.align_record["spatial_fit"]["shared"] is True
    assert pred.model.align is not None and not torch.equal(pred.model.align_matrix, torch.eye(8, device=dev))
    # the checkpoint round trip serves the same probabilities
    outs = []
    for i, m in enumerate(pred.members):
        outs.append(str(tmp_path / f"fitted_m{i}.pth"))
        save_reference_checkpoint(m, outs[-1])
    state = torch.load(outs[1], map_location="cpu", weights_only=True)
    assert state["nsd_align"]["record"]["spatial_fit"]["shared"] is True
    back = nsd.EnsemblePredictor(outs, 125, preprocess="identity")
    xt = to_dev(x, dev)
    assert torch.equal(back.model.align_matrix, pred.model.align_matrix)
    assert torch.equal(back.model.predict_proba(xt), pred.model.predict_proba(xt))
    # unkeyed: refused before anything runs, and the text names the key
    names5, _ = _names_of(lambda: pytest.raises(nsd.NsdError, pred.calibrate, x, y, spatial={}).match("shared=True"))
    assert names5 == []


def test_input_gradient_is_multi_train_dx_on_what_the_members_are_fed(nsd, dev, ref_state, shifted, tmp_path):
    from nsd_amd import ops
    x, y = shifted
    paths = []
    for i, st in enumerate(_member_states(ref_state, 2)):
        d = tmp_path / f"m{i}"
        d.mkdir()
        paths.append(write_pth(str(d), st))
    ens = nsd.EnsemblePredictor(paths, 125, preprocess="identity")
    em, M, N, T = ens.model, 2, x.shape[0], x.shape[1]
    with torch.no_grad():
        fed = em.models[0]._front_end(to_dev(x, dev)).contiguous()
    yt = to_dev(np.tile(y.astype(np.int32), M), dev)
    ws, logits = ops.multi_workspace(em.spec, M, N, T, dev), torch.empty((M * N, em.spec.K), device=dev)
    for reduce, shape in (("mean", (N, T, 8)), ("per_model", (M, N, T, 8))):
        want = torch.empty(shape, device=dev)
        ops.multi_train_dx(em.spec, em.params, fed, ws, logits, want, labels=yt, reduce=reduce)
        got = ens.input_gradient(x, y, reduce=reduce)
        assert got.shape == shape and sr.same_bits(got, want.cpu().numpy()) and np.isfinite(got).all() and np.abs(got).max() > 0
    snap = snapshot(em.params)
    ens.input_gradient(x, y)
    assert snap.unchanged()
