"""Cost and effect of the shared alignment fit of an ensemble (nsd_multi_train_bwd_dx / nsd_multi_loss_mean, nsd_amd.EnsembleSpatialFit),
written as tables for profiles/ensemble_spatial_fit.md.

    python tools/ensemble_spatial_fit_latency.py [--reps 300] [--warmup 30] [--parent-lib <libnsd_hip.so of the parent commit>]
                                                 [--no-latency] [--accuracy] [--work <dir>] [--out <file.md>]

Latency (tools/align_latency.py's method and helpers): GPU time between two HIP events around the call(s), median, 10th / 90th
percentile and mean; the legs of a point alternate inside each repetition, in one process; the "existing launches" leg runs twice.
  epoch        M = 5, N = 12, T = 625, C = 8.  Existing launches: five single-model SpatialFit epochs, one per member (what the parent
               commit offers for the job; with --parent-lib they run on the parent's own library, loaded beside this tree's).  New: the
               shared epoch.  Both eagerly and replayed from captured graphs.
  dx alone     the model-batched dx kernel, per model and mean, against M launches of the single-model kernel on the same rows
               (nsd_diag_dx of the diagnostic build), at 5 x 12 x 625 and 5 x 256 x 250 rows.
  untouched    a ModelBatchTrainer step at M = 5, B = 64, T = 250 (no dx requested) on this tree's library and, with --parent-lib, on the
               parent's, in alternation.
Accuracy (--accuracy): the shift experiment of tools/spatial_fit_latency.py with ensembles.  The recipe, trials, seeds and mixing matrix
are that tool's; the FOLDS are those of seed 1 for all five seeds (train.py draws each seed's folds from the seed, so the five seeds'
fold-f models would each have trained on other seeds' held-out trials: an ensemble of them has no held-out trials).  Per fold the five
seeds' models form the ensemble; 4 calibration trials per class, the rest scored; every fit at its defaults.
"""
import argparse
import contextlib
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from align_latency import _fmt, _measure  # noqa: E402

M_FIT, N_FIT, T_FIT = 5, 12, 625


def other_library(path):
    """`with use():` sends every C-ABI call of the block to the library at `path` (an older build: the symbols it has are bound)"""
    from nsd_amd import _lib
    L = C.CDLL(path)
    for name, (res, args) in _lib.SYMBOLS.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args

    @contextlib.contextmanager
    def use():
        _lib.lib()
        saved, _lib._lib = _lib._lib, L
        try:
            yield
        finally:
            _lib._lib = saved
    return use


def latency(a, torch, nsd_amd, ops, dev):
    from nsd_amd import _lib
    med = statistics.median
    parent = other_library(a.parent_lib) if a.parent_lib else contextlib.nullcontext
    where = "the parent commit's library" if a.parent_lib else "this tree's library (no --parent-lib)"
    g = torch.Generator().manual_seed(0)
    members = []
    for m in range(M_FIT):
        torch.manual_seed(1 + m)
        members.append(nsd_amd.EEG_LSTM().to(dev).eval())
    sp = members[0].spec
    flats = [m.flat_parameters() for m in members]
    params = torch.stack(flats).contiguous()
    v = (2.7 * torch.randn((N_FIT, T_FIT, 8), generator=g)).to(dev)
    y = torch.randint(0, 3, (N_FIT,), generator=g, dtype=torch.int32).to(dev)
    yM = y.repeat(M_FIT).contiguous()
    A0 = torch.eye(8, device=dev)
    A = (A0 + 0.1 * torch.randn((8, 8), generator=g).to(dev)).contiguous()
    xa, dx = torch.empty_like(v), torch.empty_like(v)
    ws1, wsM = ops.new_workspace(sp, N_FIT, T_FIT, dev), ops.multi_workspace(sp, M_FIT, N_FIT, T_FIT, dev)
    logits1, logitsM = torch.empty((N_FIT, sp.K), device=dev), torch.empty((M_FIT * N_FIT, sp.K), device=dev)
    dA, counts = torch.empty((1, 8, 8), device=dev), torch.empty(2, dtype=torch.int64, device=dev)
    scratch = torch.empty(N_FIT * 64, dtype=torch.float64, device=dev)
    loss1, losses = torch.zeros(1, device=dev), torch.zeros(4, device=dev)
    state = ops.spatial_fit_state(8, 1, dev)

    def tail():
        ops.spatial_bwd(v, dx, A, want_dv=False, dW=dA, counts=counts, scratch=scratch)
        ops.spatial_fit_step(A, dA, state, A0=A0, lr=0.0, decay=0.0, loss_in=loss1, loss_out=losses)   # (lr 0: A stays the same input)

    def one_by_one():
        with parent():
            for flat in flats:                                 # five single-model epochs: one matrix per member
                ops.spatial_apply(v, A, out=xa)
                ops.train_dx(sp, flat, xa, ws1, logits1, dx, labels=y, loss_out=loss1)
                tail()

    def single():
        with parent():
            ops.spatial_apply(v, A, out=xa)
            ops.train_dx(sp, flats[0], xa, ws1, logits1, dx, labels=y, loss_out=loss1)
            tail()

    def shared():
        ops.spatial_apply(v, A, out=xa)
        ops.multi_train_dx(sp, params, xa, wsM, logitsM, dx, labels=yM, reduce="mean", loss_out=loss1)
        tail()

    for fn in (one_by_one, single, shared):
        fn()
    torch.cuda.synchronize()
    graphs = {}
    for name, fn in (("one_by_one", one_by_one), ("single", single), ("shared", shared)):
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            fn()
    lines = ["## Time per epoch", "", f"M = {M_FIT} members, N = {N_FIT} trials, T = {T_FIT}, C = 8 (H = 48, L = 2, K = 3), fp32.  "
             f"\"Five single-model epochs\" and \"one single-model epoch\" run on {where}.", "",
             "| point | five single-model epochs (existing launches), us | one single-model epoch, us | the shared epoch, us | shared / five | "
             "shared - one | spread (five' - five) |", "|---|---|---|---|---|---|---|"]
    for point, calls in (("eager", dict(five=one_by_one, five2=one_by_one, one=single, shared=shared)),
                         ("replayed", dict(five=graphs["one_by_one"].replay, five2=graphs["one_by_one"].replay, one=graphs["single"].replay,
                                           shared=graphs["shared"].replay))):
        t = _measure(calls, a.reps, a.warmup, torch)
        lines.append(f"| {point} | {_fmt(t['five'])} | {_fmt(t['one'])} | {_fmt(t['shared'])} | {med(t['shared']) / med(t['five']):.3f} | "
                     f"{med(t['shared']) - med(t['one']):+.1f} | {abs(med(t['five2']) - med(t['five'])):.1f} |")
    lines.append("")
    # the dx launch alone
    lines += ["## The dx launch alone", "", "`nsd_diag_dx` of the diagnostic build: the kernels on caller-made operands, nothing else in the window.", "",
              "| rows | M launches of the single-model kernel, us | the same again, us | model-batched, per model (one launch), us | "
              "model-batched, mean (one launch), us |", "|---|---|---|---|---|"]
    with _lib.diagnostic_library():
        for B, T in ((N_FIT, T_FIT), (256, 250)):
            rows = B * T
            da0 = (1e-2 * torch.randn((M_FIT, rows, 4 * sp.H), generator=g)).to(dev)
            per, mean = torch.empty((M_FIT, rows, 8), device=dev), torch.empty((rows, 8), device=dev)
            t = _measure({"calls": lambda: ops.dx_diag(sp, da0, params, "single_calls", dx=per),
                          "calls2": lambda: ops.dx_diag(sp, da0, params, "single_calls", dx=per),
                          "per": lambda: ops.dx_diag(sp, da0, params, "per_model", dx=per),
                          "mean": lambda: ops.dx_diag(sp, da0, params, "mean", dx=mean)}, a.reps, a.warmup, torch)
            lines.append(f"| {M_FIT} x {B} x {T} = {M_FIT * rows} | {_fmt(t['calls'])} | {_fmt(t['calls2'])} | {_fmt(t['per'])} | {_fmt(t['mean'])} |")
    lines.append("")
    # an untouched path: the model-batched train step without dx
    M, B, T = 5, 64, 250
    x = torch.randn((M, B, T, 8), generator=g).to(dev)
    yb = torch.randint(0, 3, (M, B), generator=g, dtype=torch.int32).to(dev)
    trainers = {}
    for name in ("this", "parent"):
        torch.manual_seed(7)
        trainers[name] = nsd_amd.ModelBatchTrainer([nsd_amd.EEG_LSTM().to(dev).train() for _ in range(M)], seeds=list(range(M)))

    def step_parent():
        with parent():
            trainers["parent"].step(x, yb)
    t = _measure({"parent": step_parent, "parent2": step_parent, "this": lambda: trainers["this"].step(x, yb)}, a.reps, a.warmup, torch)
    lines += ["## An untouched path: the model-batched train step, no dx requested", "",
              f"ModelBatchTrainer.step, M = {M}, B = {B}, T = {T}; the first two columns on {where}.", "",
              "| step, us | the same again, us | this tree, us | this - first (medians) | spread |", "|---|---|---|---|---|",
              f"| {_fmt(t['parent'])} | {_fmt(t['parent2'])} | {_fmt(t['this'])} | {med(t['this']) - med(t['parent']):+.1f} | "
              f"{abs(med(t['parent2']) - med(t['parent'])):.1f} |", ""]
    return lines


def accuracy(a, torch, nsd_amd, ops, dev):
    import numpy as np
    from nsd_amd import data as D
    from nsd_amd import train
    from nsd_amd.calibrate import split_calibration
    if a.work is None:
        import tempfile
        a.work = tempfile.mkdtemp(prefix="ensemble_spatial_fit_accuracy_")
    os.makedirs(a.work, exist_ok=True)
    ts = D.load_trials_npz(a.data, x_key="x_filt")
    folds_of = D.stratified_folds
    D.stratified_folds = lambda y, k, seed=0: folds_of(y, k, 1)                        # every seed trains on seed 1's folds (see the header)
    recipe = ["--data", a.data, "--npz-key", "x_filt", "--classes", "3", "--T", "625", "--epochs", "200", "--batch", "32", "--lr", "0.001",
              "--dropout", "0.6", "--seed", "1", "--kfold", "5", "--concurrent", "--kfold-seeds", "5", "--log-every", "100000", "--save-folds"]
    done = {}
    try:
        for arm, extra in (("off", []), ("on", ["--align"])):
            log = os.path.join(a.work, f"{arm}.jsonl")
            if os.path.exists(log):
                os.remove(log)
            rc = train.main(recipe + extra + ["--out", os.path.join(a.work, f"{arm}.pth"), "--log-jsonl", log])
            if rc:
                raise SystemExit(f"ensemble_spatial_fit_latency: train ({arm}) returned {rc}")
            done[arm] = json.loads(open(log).read().strip().splitlines()[-1])
            print(f"trained the {arm} arm", flush=True)
        runs = train.concurrent_runs(ts.y, 5, 5, 1, 32)
    finally:
        D.stratified_folds = folds_of
    rs = np.random.RandomState(2024)                                                 # tools/align_latency.py's mixing matrix
    U, _ = np.linalg.qr(rs.standard_normal((8, 8)))
    V, _ = np.linalg.qr(rs.standard_normal((8, 8)))
    mixing = ((U * np.logspace(0.0, -1.0, 8)) @ V.T).astype(np.float32)
    mixing /= np.float32(np.sqrt((mixing ** 2).sum() / 8))

    def ens(arm, ks):
        return nsd_amd.EnsemblePredictor([done[arm]["fold_checkpoints"][k] for k in ks], 125, device="cpu", preprocess="identity")

    def probs(model, xs):
        return model.predict_proba(torch.from_numpy(xs).to(dev)).cpu().numpy()

    def acc(p, ys):
        return float((p.argmax(1) == ys).mean())

    names = ["ensemble, unaligned", "ensemble + shared spatial fit", "ensemble + shared spatial fit + head fit",
             "ensemble: whitening + shared spatial + head", "members fitted one by one (SpatialFit), probabilities averaged",
             "ensemble, unshifted (check, the same held-out rest)"]
    arms, statuses, curves, singles = {n: [] for n in names}, [], [], []
    for f in range(5):
        ks = [s * 5 + f for s in range(5)]
        assert all(runs[k]["fold"] == f and np.array_equal(runs[k]["va"], runs[ks[0]]["va"]) for k in ks)
        va = runs[ks[0]]["va"]
        xs, ys = ts.x[va], ts.y[va]
        shifted = np.ascontiguousarray(xs @ mixing.T)
        cal, rest = split_calibration(ys, 4, 0)
        xc, yc, xr, yr = shifted[cal], ys[cal], shifted[rest], ys[rest]
        arms[names[0]].append(acc(probs(ens("off", ks).model, xr), yr))
        arms[names[5]].append(acc(probs(ens("off", ks).model, xs[rest]), yr))
        p = ens("off", ks)
        fit = nsd_amd.EnsembleSpatialFit(p.model)
        ls = fit.fit(xc, yc).cpu().numpy()
        statuses += fit.status()
        curves.append((float(ls[0]), float(ls[-1])))
        arms[names[1]].append(acc(probs(p.model, xr), yr))
        p = ens("off", ks)
        rep = p.calibrate(xc, yc, align=False, spatial=dict(shared=True))
        statuses += rep["spatial_status"]
        arms[names[2]].append(acc(probs(p.model, xr), yr))
        p = ens("on", ks)
        rep = p.calibrate(xc, yc, align=True, spatial=dict(shared=True))
        statuses += rep["spatial_status"]
        arms[names[3]].append(acc(probs(p.model, xr), yr))
        each = []
        for k in ks:
            one = nsd_amd.SimplePredictor(done["off"]["fold_checkpoints"][k], sr=125, device="cpu", preprocess="identity")
            singles.append(acc(probs(one.model, xr), yr))
            sf = nsd_amd.SpatialFit(one.model)
            sf.fit(xc, yc)
            statuses += sf.status()
            each.append(probs(one.model, xr))
        arms[names[4]].append(acc(np.mean(each, axis=0), yr))
        print(f"fold {f}: " + ", ".join(f"{100 * arms[n][-1]:.1f}" for n in names), flush=True)

    lines = ["## The shift experiment with ensembles", "",
             f"`{os.path.relpath(a.data, ROOT)}`, {len(ts.y)} trials; the recipe, seeds and mixing matrix of `profiles/spatial_fit.md`, the folds of "
             "seed 1 for all five seeds (see *Method*).  Per fold the five seeds' models form the ensemble; 4 calibration trials per class of "
             "the SHIFTED held-out trials, the rest is scored.  Mean +- sd over the five folds.  EnsembleSpatialFit, SpatialFit and HeadFit at "
             "their defaults (50 epochs, lr 1e-2, decay 1e-2; 100 epochs, lr 1e-3): choices, not tuned.", "",
             "| arm | accuracy on the rest | per fold |", "|---|---|---|"]
    for n in names:
        v = np.asarray(arms[n])
        lines.append(f"| {n} | {100 * v.mean():.1f} % +- {100 * v.std(ddof=1):.1f} % | " + ", ".join(f"{100 * s:.1f}" for s in v) + " |")
    c, s = np.asarray(curves), np.asarray(singles)
    lines += ["", f"The 25 members alone, unaligned, on the same rests: {100 * s.mean():.1f} % +- {100 * s.std(ddof=1):.1f} %.  Shared fit alone, mean "
              f"calibration loss over the {len(c)} fits: {c[:, 0].mean():.3f} before the first epoch, {c[:, 1].mean():.3f} before the last; fits "
              f"with a status set: {int(np.count_nonzero(statuses))} of {len(statuses)}.", ""]
    return lines


def main():
    import torch
    import nsd_amd
    from nsd_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--commit", default="working tree")
    ap.add_argument("--parent-lib", default=None, help="libnsd_hip.so built from the parent commit: the existing-launch legs run on it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_spatial_fit_latency.md"))
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--no-latency", action="store_true")
    ap.add_argument("--data", default=os.path.join(ROOT, "tests", "golden", "recorded_trials_filtered.npz"))
    ap.add_argument("--work", default=None, help="where the accuracy runs keep their logs and fold checkpoints (default: a temporary directory)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_spatial_fit_latency: needs the MI355X (no GPU, no figures)")
    dev = torch.device("cuda:0")
    lines = [f"Machine: {torch.cuda.get_device_name(dev)}, torch {torch.__version__}.  Commit: {a.commit}.", "",
             f"Method: `python tools/ensemble_spatial_fit_latency.py --reps {a.reps} --warmup {a.warmup}{' --parent-lib <parent build>' if a.parent_lib else ''}"
             f"{' --accuracy' if a.accuracy else ''}`.  GPU time between two HIP events around the call(s), microseconds, median (10th .. 90th "
             f"percentile; mean) of {a.reps} repetitions after {a.warmup} untimed ones; the legs of a point alternate inside each repetition, one process.", ""]
    if not a.no_latency:
        lines += latency(a, torch, nsd_amd, ops, dev)
    if a.accuracy:
        lines += accuracy(a, torch, nsd_amd, ops, dev)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
