"""Early stopping for model batches measured: one evaluation of all models through ModelBatchTrainer.track_best against the per-model
host loop, the nsd_multi_eval launch on its own, and the cross-validated accuracy of the recorded trials with and without early
stopping.  Writes profiles/model_selection.md.

    python tools/model_selection.py [--reps 30] [--epochs 200] [--commit <text>] [--out profiles/model_selection.md]

1. One evaluation of all models, M = 5 and M = 32, T = 250, 65 held-out windows per model (the size of an inner split or a fold of the
   recorded trials).  WALL time of the host, from an idle device to the metrics on the host, median (10th .. 90th percentile); the two
   legs alternate in one process:
     track_best   nsd_multi_infer + nsd_multi_eval (metrics, decision, snapshot) and one read of the records per kind
     host loop    M calls of nsd_amd.train.evaluate(model_m, x_m, y_m): a forward launch, an argmax, a comparison and an .item() per
                  model -- accuracy only; what the drivers did per logged epoch, once for the training and once for the held-out part
2. The nsd_multi_eval call alone at M = 32, B = 65, K = 3: GPU time between two HIP events around the one call (the launch's own
   latency included; no kernel trace), for metrics only, for a decision that improves no model (no snapshot) and for one that improves
   all 32 (32 rows of P floats copied).
3. `python -m nsd_amd.train --kfold 5 --concurrent --kfold-seeds 5` with the README's recipe on the recorded trials, once with the
   fixed epoch count and once per --patience value with --early-stop-patience N --inner-fraction 0.2 (5: the setting asked about; 30
   and 0, the best of all epochs, for comparison), same seeds: the outer-fold accuracy of the 25 models.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
T, HELD = 250, 65


def _pct(v, q):
    s = sorted(v)
    return s[min(len(s) - 1, int(q * len(s)))]


def _fmt(v, digits=1):
    return f"{statistics.median(v):.{digits}f} ({_pct(v, 0.1):.{digits}f} .. {_pct(v, 0.9):.{digits}f})"


def clocks() -> str:
    """the card's clocks as rocm-smi shows them (read only), or why they are not known"""
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=60).stdout
        keep = [ln.split(":", 1)[1].strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln]
        return "; ".join(keep) if keep else "rocm-smi printed no sclk / mclk line"
    except Exception as e:                                                 # noqa: BLE001
        return f"not read ({type(e).__name__})"


def wall_time(a, torch, nsd_amd, dev, lines):
    from nsd_amd.train import evaluate
    lines += ["## 1. One evaluation of all models: wall time, microseconds", "",
              "| M | track_best (2 launches, records read once) | host loop: M x train.evaluate | host loop / track_best |", "|---|---|---|---|"]
    notes = []
    for M in (5, 32):
        models = []
        for m in range(M):
            torch.manual_seed(m)
            models.append(nsd_amd.EEG_LSTM(8, 48, 2, 3, 0.6).to(dev).train())
        mbt = nsd_amd.ModelBatchTrainer(models, seeds=list(range(M)))
        g = torch.Generator().manual_seed(M)
        x = (2.7 * torch.randn((M, HELD, T, 8), generator=g)).to(dev)
        y = torch.randint(0, 3, (M, HELD), generator=g, dtype=torch.int32).to(dev)
        counts = [HELD - (m % 2) for m in range(M)]
        xs, ys = [x[m, :counts[m]].contiguous() for m in range(M)], [y[m, :counts[m]].contiguous() for m in range(M)]
        t_new, t_old = [], []
        for r in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            new = mbt.track_best(x, y, counts, metric="loss", patience=0)
            t1 = time.perf_counter()
            old = [evaluate(models[m], xs[m], ys[m]) for m in range(M)]
            t2 = time.perf_counter()
            if r >= a.warmup:
                t_new.append((t1 - t0) * 1e6)
                t_old.append((t2 - t1) * 1e6)
        apart = max(abs(e["acc"] - v) for e, v in zip(new, old))
        lines.append(f"| {M} | {_fmt(t_new)} | {_fmt(t_old)} | {statistics.median(t_old) / statistics.median(t_new):.1f}x |")
        notes.append(f"M = {M}: the accuracies of the two routes differ by at most {apart:.4f}")
        print(lines[-1], flush=True)
        del mbt, models
    lines += ["", "; ".join(notes) + ".", ""]


def launch_time(a, torch, ops, dev, lines):
    M, K, P = 32, 3, ops.ModelSpec().param_count
    g = torch.Generator().manual_seed(1)
    logits = (3.0 * torch.randn((M, HELD, K), generator=g)).to(dev)
    labels = torch.randint(0, K, (M, HELD), generator=g, dtype=torch.int32).to(dev)
    params = torch.randn((M, P), generator=g).to(dev)
    out, state = ops.eval_buffer(M, dev), ops.select_state(M, P, dev)
    rule = dict(metric="loss", patience=0, min_delta=0.0)
    nrec = ops.select_records_bytes(M)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    legs = {"metrics only (sel = NULL)": (lambda: None, lambda: ops.multi_eval(logits, labels, out=out)),
            "decision, no model improves (no snapshot)": (lambda: None, lambda: ops.multi_eval(logits, labels, out=out, select=rule, params=params, state=state)),
            f"decision, all 32 improve (32 x {P} floats copied)": (lambda: state[:nrec].zero_(),
                                                                   lambda: ops.multi_eval(logits, labels, out=out, select=rule, params=params, state=state))}
    times = {k: [] for k in legs}
    ops.multi_eval(logits, labels, out=out, select=rule, params=params, state=state)          # every model now holds a best evaluation
    for r in range(a.warmup + a.reps):
        for name, (prepare, fn) in legs.items():
            prepare()
            torch.cuda.synchronize()
            t = timed(fn)
            if r >= a.warmup:
                times[name].append(t)
    lines += [f"## 2. The nsd_multi_eval call alone, M = 32, B = {HELD}, K = 3: GPU time between two HIP events, microseconds", "",
              "| call | time |", "|---|---|"] + [f"| {k} | {_fmt(v)} |" for k, v in times.items()] + [""]
    print("\n".join(lines[-6:]), flush=True)


def cross_validation(a, lines):
    from nsd_amd import train
    data = os.path.join(ROOT, "tests", "golden", "recorded_trials_filtered.npz")
    recipe = ["--data", data, "--npz-key", "x_filt", "--classes", "3", "--T", "625", "--epochs", str(a.epochs), "--batch", "32", "--lr", "0.001",
              "--dropout", "0.6", "--seed", "1", "--kfold", "5", "--concurrent", "--kfold-seeds", "5", "--log-every", "100000"]
    tmp, notes = tempfile.mkdtemp(), []
    lines += ["## 3. 5 folds x 5 seeds on the recorded trials: outer-fold accuracy of the 25 models", "",
              f"Recipe (the README's): `python -m nsd_amd.train {' '.join(recipe[2:])}` on `tests/golden/recorded_trials_filtered.npz`.", "",
              "| selection | accuracy, mean +- sd over the 25 folds | per-seed means | epochs trained | chosen epochs (0-based) | wall time of the 25 runs, s |",
              "|---|---|---|---|---|---|"]
    arms = [("none: fixed epoch count, last-epoch model", [])]
    arms += [(f"inner split: early stopping on loss, patience {p}", ["--early-stop-patience", str(p), "--inner-fraction", "0.2"]) for p in a.patience]
    for name, extra in arms:
        log = os.path.join(tmp, f"{len(lines)}.jsonl")
        t0 = time.time()
        rc = train.main(recipe + extra + ["--out", os.path.join(tmp, "all.pth"), "--log-jsonl", log])
        assert rc == 0, rc
        recs = [json.loads(ln) for ln in open(log)]
        done = [r for r in recs if r.get("done")][0]
        folds = [r for r in recs if "fold" in r and "n_val" in r]
        t_folds = max(r["elapsed_s"] for r in recs if r.get("concurrent") and "elapsed_s" in r)
        assert done["selection"] == name and len(folds) == 25, (done["selection"], len(folds))
        acc = done["acc_val_folds"]
        seed_means = [statistics.mean(acc[5 * i:5 * i + 5]) for i in range(5)]
        chosen = sorted(done["best_epochs"]) if extra else "-"
        lines.append(f"| {name} | {100 * done['acc_val_mean']:.1f} % +- {100 * done['acc_val_sd']:.1f} % | "
                     f"{', '.join(f'{100 * v:.1f}' for v in seed_means)} | {done.get('epochs_run', a.epochs)} | {chosen} | {t_folds:.1f} |")
        print(lines[-1], f"(whole command {time.time() - t0:.0f} s)", flush=True)
        if extra:
            conf = [[sum(r["confusion_val"][i][j] for r in folds) for j in range(3)] for i in range(3)]
            notes.append(f"Patience {extra[1]}: outer confusion matrix of the selected models, summed over the 25 folds (rows: label, columns: "
                         f"prediction) `{conf}`; the same models after their last trained epoch, before restore_best, score "
                         f"{100 * statistics.mean(r['acc_val_last_epoch'] for r in folds):.2f} % on their outer folds.")
    lines += [""] + notes + [""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--skip-cv", action="store_true")
    ap.add_argument("--patience", type=int, nargs="+", default=[5, 30, 0], help="early-stopping arms of the cross-validation (0: best epoch, never stop)")
    ap.add_argument("--commit", default="working tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_selection.md"))
    a = ap.parse_args()
    clk = clocks()
    import torch
    import nsd_amd
    from nsd_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("model_selection: needs the MI355X (no GPU, no figures)")
    dev = torch.device("cuda:0")
    prop = torch.cuda.get_device_properties(dev)
    lines = ["# Early stopping for model batches: one evaluation of all models, the launch, and what selection does to the accuracy", "",
             f"Machine: {prop.name} ({prop.multi_processor_count} CUs), torch {torch.__version__}.  Clocks before the run: {clk}.  Commit: {a.commit}.", "",
             f"Method: `python tools/model_selection.py --reps {a.reps} --epochs {a.epochs}` (its docstring describes the legs): medians (10th .. 90th "
             f"percentile) of {a.reps} repetitions after {a.warmup} untimed ones, the legs of a table alternating in one process.", ""]
    wall_time(a, torch, nsd_amd, dev, lines)
    launch_time(a, torch, ops, dev, lines)
    if not a.skip_cv:
        cross_validation(a, lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
