"""The model-batched H = 48 path (nsd_multi_*): M models per launch against M single-model runs.  Needs the MI355X."""
import numpy as np
import pytest
import torch

from tests.gpu_harness import LOGIT_TOL, LOSS_TOL, D, dev, multi_grad_ok, multi_problem, multi_single, multi_step, nsd, spec_of  # noqa: F401  (dev, nsd: fixtures)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B", [32, 300, 600])
def test_one_model_is_todays_path_bitwise(nsd, dev, B):
    """M = 1 IS today's path: the nsd_multi_* entry points hand a single model to nsd_lstm_head_train_rng / nsd_lstm_bwd_rng /
    nsd_grad_reduce(_adam) themselves, so no model-batched kernel runs here.  The test pins that routing (and the 1/B loss scale,
    the workspace layout and the Adam tail of the multi entry points at M = 1); the model-batched kernels are held to single-model
    runs and to the oracle by the tests below."""
    spec = spec_of(D)
    params, x, y, rngs = multi_problem(spec, 1, B, 40, dev, seed=B)
    lg, gr, ls = multi_step(nsd, spec, params, x, y, rngs, dev)
    l1, g1, s1 = multi_single(nsd, spec, params[0].clone(), x[0], y[0], rngs[0], dev)
    assert torch.equal(lg[0], l1) and torch.equal(gr[0], g1) and float(ls[0]) == s1
    # Adam rides in the reduction: p / m / v after the step equal the single-model fused launch
    p_multi, p_single = params.clone(), params[0].clone()
    mm, vv = torch.zeros_like(p_multi), torch.zeros_like(p_multi)
    m1, v1 = torch.zeros_like(p_single), torch.zeros_like(p_single)
    multi_step(nsd, spec, p_multi, x, y, rngs, dev, fuse_adam=True, m=mm, v=vv, step=1)
    multi_single(nsd, spec, p_single, x[0], y[0], rngs[0], dev, adam=dict(m=m1, v=v1, step=1))
    assert torch.equal(p_multi[0], p_single) and torch.equal(mm[0], m1) and torch.equal(vv[0], v1)


@pytest.mark.parametrize("M,B,T", [(5, 32, 40), (10, 32, 9), (25, 32, 9), (3, 171, 9), (5, 32, 625), (2, 200, 625), (17, 32, 625)])
def test_models_equal_separate_runs(nsd, dev, M, B, T):
    """(5, 32) / (10, 32): one-trial kernels, (2, 200): two-trial forward + one-trial backward, (25, 32) / (3, 171) / (17, 32): the
    four-trial kernels (3 x 171: partial groups in every model), at T = 9 .. 625 (625: the recorded trials' length)."""
    spec = spec_of(D)
    params, x, y, rngs = multi_problem(spec, M, B, T, dev, seed=M * 1000 + B)
    lg, gr, ls = multi_step(nsd, spec, params, x, y, rngs, dev)
    for m in range(M):
        l1, g1, s1 = multi_single(nsd, spec, params[m].clone(), x[m], y[m], rngs[m], dev)
        assert float((lg[m] - l1).abs().max()) <= 1e-6 * max(float(l1.abs().max()), 1.0), m
        multi_grad_ok(spec, gr[m], g1)
        assert abs(float(ls[m]) - s1) <= 1e-6 * max(1.0, abs(s1)), (m, float(ls[m]), s1)


@pytest.mark.parametrize("M,B", [(5, 32), (5, 120)])
def test_models_are_isolated(nsd, dev, M, B):
    spec = spec_of(D)
    params, x, y, rngs = multi_problem(spec, M, B, 24, dev, seed=7)
    lg, gr, _ = multi_step(nsd, spec, params, x, y, rngs, dev)
    p2, x2 = params.clone(), x.clone()
    p2[2] += 0.01
    x2[2] *= -1.5
    lg2, gr2, _ = multi_step(nsd, spec, p2, x2, y, rngs, dev)
    for m in range(M):
        if m == 2:
            assert not torch.equal(lg[m], lg2[m])
        else:
            assert torch.equal(lg[m], lg2[m]) and torch.equal(gr[m], gr2[m]), m


def test_shared_input_equals_replicated(nsd, dev):
    spec = spec_of(D)
    M, B, T = 4, 32, 30
    params, x, y, rngs = multi_problem(spec, M, B, T, dev, seed=11)
    shared = x[0].contiguous()
    lg, gr, ls = multi_step(nsd, spec, params, shared, y, rngs, dev)
    lr, grr, lsr = multi_step(nsd, spec, params, shared.unsqueeze(0).expand(M, B, T, spec.C).contiguous(), y, rngs, dev)
    assert torch.equal(lg, lr) and torch.equal(gr, grr) and torch.equal(ls, lsr)


def test_fused_reduce_adam_equals_reduce_then_adam(nsd, dev):
    from nsd_amd import ops
    spec = spec_of(D)
    M, B, T = 6, 32, 20
    params, x, y, rngs = multi_problem(spec, M, B, T, dev, seed=3)
    pa, ma, va = params.clone(), torch.rand_like(params) * 1e-3, torch.rand_like(params) * 1e-6
    pb, mb, vb = pa.clone(), ma.clone(), va.clone()
    _, ga, _ = multi_step(nsd, spec, pa, x, y, rngs, dev, fuse_adam=True, m=ma, v=va, step=3)
    _, gb, _ = multi_step(nsd, spec, pb, x, y, rngs, dev, fuse_adam=False)
    ops.adam_step(pb.view(-1), gb.view(-1), mb.view(-1), vb.view(-1), step=3, lr=1e-3)
    assert torch.equal(ga, gb) and torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb)


@pytest.mark.parametrize("M,B", [(3, 40), (8, 32)])
def test_multi_infer_equals_infer(nsd, dev, M, B):
    from nsd_amd import ops
    spec = spec_of(D)
    params, x, _, _ = multi_problem(spec, M, B, 50, dev, seed=5)
    lg, pr = ops.multi_infer(spec, params, x)
    for m in range(M):
        l1, p1 = ops.infer(spec, params[m].contiguous(), x[m].contiguous())
        assert torch.equal(lg[m], l1) and torch.equal(pr[m], p1), m
    lgs, prs = ops.multi_infer(spec, params, x[0].contiguous())
    for m in range(M):
        l1, p1 = ops.infer(spec, params[m].contiguous(), x[0].contiguous())
        assert torch.equal(lgs[m], l1) and torch.equal(prs[m], p1), m


def test_ensemble_predictor_matches_simple_predictor(nsd, dev, tmp_path):
    import os
    from nsd_amd.tester import DEFAULT_MODEL
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "recorded_trials.npz"))
    key = [k for k in fx.files if fx[k].ndim == 3][0]
    wins = fx[key].astype(np.float32)
    T = wins.shape[1]
    sp = nsd.SimplePredictor(DEFAULT_MODEL, sr=125, preprocess="identity")
    ens = nsd.EnsemblePredictor([DEFAULT_MODEL] * 3, sr=125, preprocess="identity")
    rec = wins.reshape(-1, wins.shape[2])
    p1, lab1 = sp.predict_windows(rec, T)
    pe, labe = ens.predict_windows(rec, T)
    assert np.abs(p1 - pe).max() <= 1e-6 and lab1 == labe
    # three different models: the mean of the three predictions
    sd = torch.load(DEFAULT_MODEL, map_location="cpu", weights_only=True)
    paths = []
    for i in range(3):
        s2 = {k: v + 0.01 * i * torch.randn_like(v) for k, v in sd.items()}
        paths.append(str(tmp_path / f"m{i}.pth"))
        torch.save(s2, paths[-1])
    ens3 = nsd.EnsemblePredictor(paths, sr=125, preprocess="identity")
    ref = np.mean([nsd.SimplePredictor(p, sr=125, preprocess="identity").predict_windows(rec[:20 * T], T)[0] for p in paths], axis=0)
    got, _ = ens3.predict_windows(rec[:20 * T], T)
    assert np.abs(got - ref).max() <= 1e-6


def test_model_batch_trainer_matches_sequential_trainers(nsd, dev):
    from nsd_amd.trainer import Trainer
    M, B, T = 5, 32, 40
    g = torch.Generator().manual_seed(21)
    xs = torch.randn((M, B, T, 8), generator=g).to(dev)
    ys = torch.randint(0, 3, (M, B), generator=g, dtype=torch.int32).to(dev)
    seeds = [3 + m for m in range(M)]

    def models():
        out = []
        for m in range(M):
            torch.manual_seed(100 + m)
            out.append(nsd.EEG_LSTM().to(dev).train())
        return out
    batched = models()
    tr = nsd.ModelBatchTrainer(batched, lr=1e-3, seeds=seeds)
    singles = models()
    trs = [Trainer(singles[m], lr=1e-3, seed=seeds[m]) for m in range(M)]
    for step in range(30):
        tr.step(xs, ys)
        losses = tr.last_losses()
        for m in range(M):
            trs[m].step(xs[m].contiguous(), ys[m].contiguous())
            ref = trs[m].last_loss()
            assert abs(losses[m] - ref) < 2e-4 * max(1.0, abs(ref)), (step, m, losses[m], ref)
    for m in range(M):
        diff = (batched[m].flat_parameters() - singles[m].flat_parameters()).abs().cpu().numpy()
        assert diff.max() <= 30 * 2e-3
        assert np.mean(diff > 1e-4) < 0.01
        assert np.median(diff) < 2e-6
    # the models stay ordinary modules: their parameters are views of the packed buffer
    assert batched[1].flat_parameters().data_ptr() == tr.params[1].data_ptr()


def test_models_against_the_oracle(nsd, dev):
    """Each model of a (5, 32, 250) model-batched step against the CPU oracle, with the dropout / RReLU masks of rng[m] regenerated
    on the host (as test_thirty_step_training_trajectory_matches_oracle does): the oracle is independent of the shared role code.
    Bounds of tests/gpu_harness.py against the oracle: logits 1e-4, loss 5e-5, gradients those of multi_grad_ok."""
    from oracle import nsd_oracle as orc
    spec = spec_of(D)
    M, B, T = 5, 32, 250
    params, x, y, rngs = multi_problem(spec, M, B, T, dev, seed=250)
    lg, gr, ls = multi_step(nsd, spec, params, x, y, rngs, dev)
    d = orc.Dims()
    for m in range(M):
        r = rngs[m]
        dl = orc.dropout_mask(r["seed"], r["base_stream"], 0.6, (1, B, T, 48))
        sl = orc.rrelu_noise(r["seed"], r["base_stream"] + 1, (B, 32))
        dh = orc.dropout_mask(r["seed"], r["base_stream"] + 2, 0.6, (B, 32))
        loss_ref, g_ref, fw = orc.loss_and_grads(params[m].cpu().numpy(), x[m].cpu().numpy(), y[m].cpu().numpy(), d, drop_lstm=dl,
                                                 rrelu_slope=sl, drop_head=dh)
        assert np.abs(lg[m].cpu().numpy() - fw["logits"]).max() < LOGIT_TOL, m
        assert abs(float(ls[m]) - loss_ref) < LOSS_TOL, (m, float(ls[m]), loss_ref)
        multi_grad_ok(spec, gr[m].cpu(), torch.from_numpy(np.asarray(g_ref, np.float32)))


def test_train_kfold_concurrent_matches_sequential(dev, tmp_path):
    """train.py --kfold 3 --concurrent on the recorded trials: exit 0, the sequential run's JSON keys per fold (+ "concurrent"), and
    per-fold last-epoch validation accuracy within one window of the sequential run."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fx = os.path.join(root, "tests", "golden", "recorded_trials.npz")

    def run(extra, out):
        cmd = [sys.executable, "-c", "import sys, nsd_amd.train as t; sys.exit(t.main(sys.argv[1:]))", "--data", fx, "--kfold", "3",
               "--epochs", "2", "--batch", "32", "--out", str(tmp_path / out)] + extra
        p = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        return [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    seq = run([], "seq.pth")
    con = run(["--concurrent"], "con.pth")
    fs = [r for r in seq if "fold" in r and "done" not in r]
    fc = [r for r in con if "fold" in r and "done" not in r]
    assert len(fs) == len(fc) == 3
    for a, b in zip(fs, fc):
        assert set(b) == set(a) | {"concurrent"} and b["concurrent"] is True
        assert a["n_train"] == b["n_train"] and a["n_val"] == b["n_val"]
        assert abs(a["acc_val_last_epoch"] - b["acc_val_last_epoch"]) <= 1.0 / a["n_val"] + 1e-9, (a, b)
    es = [r for r in seq if "epoch" in r]
    ec = [r for r in con if "epoch" in r]
    assert sorted((r["run"], r["epoch"]) for r in es if r["run"] != "all") == sorted((r["run"], r["epoch"]) for r in ec if r["run"] != "all")
    assert all(set(b) == set(a) | {"concurrent"} for a in es for b in ec if b["run"] != "all" and a["run"] != "all")
    assert [r for r in con if r.get("done")][0]["concurrent"] is True
