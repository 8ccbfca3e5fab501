"""Cost and effect of the supervised session alignment (nsd_spatial_bwd / nsd_spatial_fit_step, nsd_amd.SpatialFit), written as tables
for profiles/spatial_fit.md.

    python tools/spatial_fit_latency.py [--reps 300] [--warmup 30] [--commit <text>] [--out profiles/spatial_fit_latency.md]
                                        [--accuracy] [--data tests/golden/recorded_trials_filtered.npz] [--work <dir>]

Latency (tools/align_latency.py's method and helpers): GPU time between two HIP events around the call(s), median, 10th / 90th
percentile and mean; the legs of a point alternate inside one repetition, in one process.  N = 12 trials, T = 625, C = 8:
  epoch        the launches of one SpatialFit epoch, eagerly and replayed from a captured graph: the epoch's existing launches alone
               (nsd_spatial_apply, nsd_lstm_head_train, nsd_lstm_bwd with dx, nsd_loss_sum -- kernels this change does not touch; run
               twice per repetition, their difference is the spread), and with nsd_spatial_bwd and nsd_spatial_fit_step behind them
  alone        nsd_spatial_bwd (dW alone: its two launches; dv alone; both) and nsd_spatial_fit_step, one call each
Accuracy (--accuracy): the shift experiment of tools/align_latency.py rerun with labels -- the same recipe, folds, seeds and mixing
matrix; per fold, 4 and 8 trials per class of the SHIFTED held-out trials calibrate (calibrate.split_calibration, seed 0), the rest is
scored.  Arms: unaligned; label-free whitening refit on the calibration trials; head fit only; spatial fit only; whitening + spatial
+ head (calibrate(align=True, spatial={})); and the unshifted check on the same rest.  Every fit runs at its defaults: nothing is tuned.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from align_latency import _fmt, _measure  # noqa: E402

N_FIT, T_FIT = 12, 625


def latency(a, torch, nsd_amd, ops, dev):
    med = statistics.median
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(1)
    model = nsd_amd.EEG_LSTM().to(dev).eval()
    sp, flat = model.spec, model.flat_parameters()
    v = (2.7 * torch.randn((N_FIT, T_FIT, 8), generator=g)).to(dev)
    y = torch.randint(0, 3, (N_FIT,), generator=g, dtype=torch.int32).to(dev)
    A0 = torch.eye(8, device=dev)
    A = (A0 + 0.1 * torch.randn((8, 8), generator=g).to(dev)).contiguous()
    xa, dx, dv = torch.empty_like(v), torch.empty_like(v), torch.empty_like(v)
    ws = ops.new_workspace(sp, N_FIT, T_FIT, dev)
    logits = torch.empty((N_FIT, sp.K), device=dev)
    dA, counts = torch.empty((1, 8, 8), device=dev), torch.empty(2, dtype=torch.int64, device=dev)
    scratch = torch.empty(N_FIT * 64, dtype=torch.float64, device=dev)
    loss1, losses = torch.zeros(1, device=dev), torch.zeros(4, device=dev)
    state = ops.spatial_fit_state(8, 1, dev)

    def base():
        ops.spatial_apply(v, A, out=xa)
        ops.train_dx(sp, flat, xa, ws, logits, dx, labels=y, loss_out=loss1)

    def new():
        ops.spatial_bwd(v, dx, A, want_dv=False, dW=dA, counts=counts, scratch=scratch)
        ops.spatial_fit_step(A, dA, state, A0=A0, lr=0.0, decay=0.0, loss_in=loss1, loss_out=losses)   # (lr 0: A stays the same input)

    def full():
        base()
        new()

    full()
    torch.cuda.synchronize()
    graphs = {}
    for name, fn in (("base", base), ("full", full)):
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            fn()
    lines = ["## Time per epoch", "", f"N = {N_FIT} trials, T = {T_FIT}, C = 8 (H = 48, L = 2, K = 3), fp32.", "",
             "| point | existing launches, us | whole epoch, us | epoch - existing (medians) | spread (existing' - existing) |", "|---|---|---|---|---|"]
    t = _measure({"base": base, "base2": base, "full": full}, a.reps, a.warmup, torch)
    lines.append(f"| eager | {_fmt(t['base'])} | {_fmt(t['full'])} | {med(t['full']) - med(t['base']):+.1f} | {abs(med(t['base2']) - med(t['base'])):.1f} |")
    t = _measure({"base": graphs["base"].replay, "base2": graphs["base"].replay, "full": graphs["full"].replay}, a.reps, a.warmup, torch)
    lines.append(f"| replayed | {_fmt(t['base'])} | {_fmt(t['full'])} | {med(t['full']) - med(t['base']):+.1f} | {abs(med(t['base2']) - med(t['base'])):.1f} |")
    base()
    alone = {
        "nsd_spatial_apply (one launch, for scale)": lambda: ops.spatial_apply(v, A, out=xa),
        "nsd_spatial_bwd, dW alone (stage 1 + stage 2: two launches)": lambda: ops.spatial_bwd(v, dx, A, want_dv=False, dW=dA, counts=counts, scratch=scratch),
        "nsd_spatial_bwd, dv alone (one launch)": lambda: ops.spatial_bwd(v, dx, A, want_dW=False, dv=dv),
        "nsd_spatial_bwd, dv and dW (three launches)": lambda: ops.spatial_bwd(v, dx, A, dv=dv, dW=dA, counts=counts, scratch=scratch),
        "nsd_spatial_fit_step (one launch)": lambda: ops.spatial_fit_step(A, dA, state, A0=A0, lr=0.0, decay=0.0, loss_in=loss1, loss_out=losses),
    }
    t = _measure(alone, a.reps, a.warmup, torch)
    lines += ["", "| call alone | us |", "|---|---|"] + [f"| {k} | {_fmt(v_)} |" for k, v_ in t.items()] + [""]
    # a whole fit as a user runs it: 50 epochs, wall time with the set-up (front end, buffers, capture) and the final read-back
    for graph in (False, True):
        torch.manual_seed(1)
        m = nsd_amd.EEG_LSTM().to(dev).eval()
        fit = nsd_amd.SpatialFit(m, graph=graph)
        fit.fit(v, y, epochs=2)                                # (warm)
        fit.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit.fit(v, y)
        torch.cuda.synchronize()
        lines.append(f"SpatialFit.fit, {fit.epochs} epochs, {'replayed' if graph else 'eager'}: {1e3 * (time.perf_counter() - t0):.2f} ms wall.")
    lines.append("")
    return lines


def accuracy(a, torch, nsd_amd, ops, dev):
    import numpy as np
    from nsd_amd import data as D
    from nsd_amd import train
    from nsd_amd.calibrate import split_calibration
    if a.work is None:
        import tempfile
        a.work = tempfile.mkdtemp(prefix="spatial_fit_accuracy_")
    os.makedirs(a.work, exist_ok=True)
    ts = D.load_trials_npz(a.data, x_key="x_filt")
    recipe = ["--data", a.data, "--npz-key", "x_filt", "--classes", "3", "--T", "625", "--epochs", "200", "--batch", "32", "--lr", "0.001",
              "--dropout", "0.6", "--seed", "1", "--kfold", "5", "--concurrent", "--kfold-seeds", "5", "--log-every", "100000", "--save-folds"]
    done = {}
    for arm, extra in (("off", []), ("on", ["--align"])):
        log = os.path.join(a.work, f"{arm}.jsonl")
        if os.path.exists(log):
            os.remove(log)
        rc = train.main(recipe + extra + ["--out", os.path.join(a.work, f"{arm}.pth"), "--log-jsonl", log])
        if rc:
            raise SystemExit(f"spatial_fit_latency: train ({arm}) returned {rc}")
        done[arm] = json.loads(open(log).read().strip().splitlines()[-1])
    runs = train.concurrent_runs(ts.y, 5, 5, 1, 32)
    rs = np.random.RandomState(2024)                                                 # tools/align_latency.py's mixing matrix
    U, _ = np.linalg.qr(rs.standard_normal((8, 8)))
    V, _ = np.linalg.qr(rs.standard_normal((8, 8)))
    mixing = ((U * np.logspace(0.0, -1.0, 8)) @ V.T).astype(np.float32)
    mixing /= np.float32(np.sqrt((mixing ** 2).sum() / 8))

    def pred(arm, k):
        return nsd_amd.SimplePredictor(done[arm]["fold_checkpoints"][k], sr=125, device="cpu", preprocess="identity")

    def acc(model, xs, ys):
        return float((model.predict_proba(torch.from_numpy(xs).to(dev)).argmax(1).cpu().numpy() == ys).mean())

    names = ["unaligned", "whitening refit (label-free, on the calibration trials)", "head fit only", "spatial fit only",
             "whitening + spatial + head", "unshifted (check, the same held-out rest)"]
    tables, statuses, curves = {}, [], []
    for per_class in (4, 8):
        arms = {n: [] for n in names}
        for k, r in enumerate(runs):
            xs, ys = ts.x[r["va"]], ts.y[r["va"]]
            shifted = np.ascontiguousarray(xs @ mixing.T)
            cal, rest = split_calibration(ys, per_class, 0)
            xc, yc, xr, yr = shifted[cal], ys[cal], shifted[rest], ys[rest]
            arms[names[0]].append(acc(pred("off", k).model, xr, yr))
            arms[names[5]].append(acc(pred("off", k).model, xs[rest], yr))
            p = pred("on", k)
            W, rec = p.model.align.fit(p.model, xc)
            if not (rec[0]["few"] or rec[0]["nonfinite"]):
                p.model.set_alignment(W[0], record=rec[0])
            arms[names[1]].append(acc(p.model, xr, yr))
            p = pred("off", k)
            p.calibrate(xc, yc, align=False)
            arms[names[2]].append(acc(p.model, xr, yr))
            p = pred("off", k)
            fit = nsd_amd.SpatialFit(p.model)
            ls = fit.fit(xc, yc).cpu().numpy()
            statuses += fit.status()
            curves.append((float(ls[0]), float(ls[-1])))
            arms[names[3]].append(acc(p.model, xr, yr))
            p = pred("on", k)
            rep = p.calibrate(xc, yc, align=True, spatial={})
            statuses += rep["spatial_status"]
            arms[names[4]].append(acc(p.model, xr, yr))
        tables[per_class] = arms

    def ms(v):
        v = np.asarray(v)
        per_seed = [float(v[i * 5:(i + 1) * 5].mean()) for i in range(5)]
        return f"{100 * v.mean():.1f} % +- {100 * v.std(ddof=1):.1f} %", ", ".join(f"{100 * s:.1f}" for s in per_seed)

    lines = ["## The shift experiment with labels", "",
             f"The recipe, folds, seeds, checkpoints' training and mixing matrix of `profiles/session_alignment.md` (`{os.path.relpath(a.data, ROOT)}`, "
             f"{len(ts.y)} trials, 5 folds x 5 seeds; M with singular values 1 .. 0.1).  Per fold the SHIFTED held-out trials are split: "
             "4 or 8 per class calibrate, the rest is scored.  Mean +- sd over the 25 runs; per-seed means in brackets.  SpatialFit and "
             "HeadFit at their defaults (50 epochs, lr 1e-2, decay 1e-2; 100 epochs, lr 1e-3): choices, not tuned.", ""]
    for per_class, arms in tables.items():
        lines += [f"{per_class} calibration trials per class:", "", "| arm | accuracy on the rest | per-seed means |", "|---|---|---|"]
        for name, v in arms.items():
            m, p = ms(v)
            lines.append(f"| {name} | {m} | {p} |")
        lines.append("")
    c = np.asarray(curves)
    lines += [f"Spatial fit alone, mean calibration loss over the {len(c)} fits: {c[:, 0].mean():.3f} before the first epoch, {c[:, 1].mean():.3f} "
              f"before the last; fits with a status set: {int(np.count_nonzero(statuses))} of {len(statuses)}.", ""]
    return lines


def main():
    import torch
    import nsd_amd
    from nsd_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--commit", default="working tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spatial_fit_latency.md"))
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--no-latency", action="store_true")
    ap.add_argument("--data", default=os.path.join(ROOT, "tests", "golden", "recorded_trials_filtered.npz"))
    ap.add_argument("--work", default=None, help="where the accuracy runs keep their logs and fold checkpoints (default: a temporary directory)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spatial_fit_latency: needs the MI355X (no GPU, no figures)")
    dev = torch.device("cuda:0")
    lines = [f"Machine: {torch.cuda.get_device_name(dev)}, torch {torch.__version__}.  Commit: {a.commit}.", "",
             f"Method: `python tools/spatial_fit_latency.py --reps {a.reps} --warmup {a.warmup}{' --accuracy' if a.accuracy else ''}`.  GPU time "
             f"between two HIP events around the call(s), microseconds, median (10th .. 90th percentile; mean) of {a.reps} repetitions after "
             f"{a.warmup} untimed ones; the legs of a point alternate inside each repetition, one process.", ""]
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
