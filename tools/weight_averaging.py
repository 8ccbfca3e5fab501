"""Weight averaging in the fused step tail measured: what the averaged row costs per step, and what scoring the averaged model does to
the cross-validated accuracy of the recorded trials.  Writes profiles/weight_averaging.md.

    python tools/weight_averaging.py [--reps 30] [--epochs 200] [--commit <text>] [--out profiles/weight_averaging.md]

1. Cost of a step.  Two trainers of the same model, seed and data step side by side in one process, the legs alternating:
     guarded    clip_grad_norm=0.0 -- the guarded tail without averaging: what the parent commit runs, launch for launch and bit for bit
                (tests/test_gpu_avg.py::test_launch_accounting), and so the yardstick
     averaging  average=ops.Average("ema", 0.999) -- the same tail's `_avg` twin
   A repetition is STEPS steps between two device synchronisations, timed with the host clock and divided by STEPS; medians (10th .. 90th
   percentile) of --reps repetitions after --warmup untimed ones.  Trainer at B = 256, T = 250, eager (Trainer.step) and replayed
   from its hipGraph (Trainer.step_static); ModelBatchTrainer at M = 25, B = 32, T = 625 (5 folds x 5 seeds of the recorded trials).
   The extra traffic per model and step is one read and one write of P = 31 764 floats (254 KB).
2. The update launch pair alone (nsd_grad_reduce_clip_adam against its `_avg` twin, and the model-batched pair at M = 25) on the slabs
   of one evaluation: GPU time between two HIP events around the one call, launch latencies included.
3. `python -m nsd_amd.train --kfold 5 --concurrent --kfold-seeds 5` with the README's recipe on the recorded trials, per arm of --avg:
   every fold record carries the outer accuracy of the last iterate and of the averaged weights of the SAME training run; with
   --early-stop-patience the inner split is scored, and the snapshot taken, on the averaged rows (track_best(weights="average")).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = 10


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


def _alternate(a, torch, legs):
    """legs: name -> fn() that enqueues STEPS steps.  -> name -> microseconds per step of each timed repetition"""
    times = {k: [] for k in legs}
    for r in range(a.warmup + a.reps):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= a.warmup:
                times[name].append((time.perf_counter() - t0) * 1e6 / STEPS)
    return times


def _row(what, times):
    g, v = times["guarded"], times["averaging"]
    delta = statistics.median(v) - statistics.median(g)
    spread = max(_pct(g, 0.9) - _pct(g, 0.1), _pct(v, 0.9) - _pct(v, 0.1))
    return f"| {what} | {_fmt(g)} | {_fmt(v)} | {delta:+.1f} | {spread:.1f} |"


def step_cost(a, torch, nsd_amd, ops, dev, lines):
    from nsd_amd.trainer import Trainer
    lines += [f"## 1. Cost of a step: microseconds per step ({STEPS} steps per repetition, host clock between two synchronisations)", "",
              "| step | guarded tail (clip_grad_norm=0.0) | with averaging (EMA 0.999) | delta of the medians | wider 10th .. 90th spread of the two legs |",
              "|---|---|---|---|---|"]
    avg = ops.Average("ema", 0.999)
    B, T = 256, 250
    g = torch.Generator().manual_seed(1234)
    x = (2.7 * torch.randn((B, T, 8), generator=g)).to(dev)
    y = torch.randint(0, 3, (B,), generator=g, dtype=torch.int32).to(dev)

    def trainer(**kw):
        torch.manual_seed(0)
        return Trainer(nsd_amd.EEG_LSTM(8, 48, 2, 3, 0.6).to(dev).train(), seed=1, **kw)
    for mode in ("eager", "graph"):
        pair = {"guarded": trainer(clip_grad_norm=0.0), "averaging": trainer(average=avg)}
        if mode == "graph":
            for t in pair.values():
                xs, ys = t.static_inputs(B, T)
                xs.copy_(x); ys.copy_(y)
        legs = {k: (lambda t=t: [t.step(x, y) for _ in range(STEPS)]) if mode == "eager" else (lambda t=t: [t.step_static(B, T) for _ in range(STEPS)])
                for k, t in pair.items()}
        times = _alternate(a, torch, legs)
        same = torch.equal(pair["guarded"].flat, pair["averaging"].flat)
        lines.append(_row(f"Trainer, B = {B}, T = {T}, {mode} (same parameters after the run: {same}; n_avg {pair['averaging'].averaged_count()})", times))
        print(lines[-1], flush=True)
        del pair, legs
    M, B, T = 25, 32, 625
    xm = (2.7 * torch.randn((M, B, T, 8), generator=g)).to(dev)
    ym = torch.randint(0, 3, (M, B), generator=g, dtype=torch.int32).to(dev)

    def batch(**kw):
        models = []
        for m in range(M):
            torch.manual_seed(m)
            models.append(nsd_amd.EEG_LSTM(8, 48, 2, 3, 0.6).to(dev).train())
        return nsd_amd.ModelBatchTrainer(models, seeds=list(range(M)), **kw)
    pair = {"guarded": batch(clip_grad_norm=0.0), "averaging": batch(average=avg)}
    times = _alternate(a, torch, {k: (lambda t=t: [t.step(xm, ym) for _ in range(STEPS)]) for k, t in pair.items()})
    same = torch.equal(pair["guarded"].params, pair["averaging"].params)
    lines.append(_row(f"ModelBatchTrainer, M = {M}, B = {B}, T = {T} (same parameters after the run: {same})", times))
    print(lines[-1], flush=True)
    lines.append("")
    return pair["averaging"]


def launch_cost(a, torch, ops, dev, mbt, lines):
    """the tails alone, on the slabs the last step of `mbt` (M = 25, B = 32, T = 625) left in its workspace"""
    spec, M = mbt.spec, mbt.M
    (B, T), P = mbt._last, mbt.spec.param_count
    ws, d = mbt._bufs[(B, T)]["ws"], spec.dims(B, T)
    opt, avg = ops.opt_struct(max_norm=0.0), ops.Average("ema", 0.999).struct()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3
    z = lambda: torch.zeros((M, P), device=dev)                                            # noqa: E731
    g, p, m, v, st, ast = z(), mbt.params.clone(), z(), z(), ops.opt_state(P, M, dev), ops.avg_state(P, M, dev)
    head = (C.byref(d), M, ws.data_ptr(), ops._nbytes(ws), g.data_ptr(), p.data_ptr(), m.data_ptr(), v.data_ptr(), C.byref(opt), 1, None,
            st.data_ptr(), ops._nbytes(st), ops.STREAM)
    legs = {"guarded": lambda: ops._call("nsd_multi_grad_reduce_clip_adam", dev, *head),
            "averaging": lambda: ops._call("nsd_multi_grad_reduce_clip_adam_avg", dev, *head, C.byref(avg), ast.data_ptr(), ops._nbytes(ast))}
    times = {k: [] for k in legs}
    for r in range(a.warmup + a.reps):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t = timed(fn)
            if r >= a.warmup:
                times[name].append(t)
    lines += ["## 2. The two launches of the tail alone: GPU time between two HIP events around the one call, microseconds", "",
              "| call | without averaging | `_avg` twin | delta of the medians | wider 10th .. 90th spread of the two legs |", "|---|---|---|---|---|",
              _row(f"nsd_multi_grad_reduce_clip_adam(_avg), M = {M}, P = {P} ({M * P * 4 / 1e6:.1f} MB read + written more)", times), ""]
    print(lines[-2], flush=True)


def cross_validation(a, lines):
    from nsd_amd import train
    data = os.path.join(ROOT, "tests", "golden", "recorded_trials_filtered.npz")
    recipe = ["--data", data, "--npz-key", "x_filt", "--classes", "3", "--T", "625", "--epochs", str(a.epochs), "--batch", "32", "--lr", "0.001",
              "--dropout", "0.6", "--seed", "1", "--kfold", "5", "--concurrent", "--kfold-seeds", "5", "--log-every", "100000"]
    tmp = tempfile.mkdtemp()
    lines += ["## 3. 5 folds x 5 seeds on the recorded trials: outer-fold accuracy of the 25 models, last iterate and averaged weights", "",
              f"Recipe (the README's): `python -m nsd_amd.train {' '.join(recipe[2:])}` on `tests/golden/recorded_trials_filtered.npz`, plus the arm's "
              "options.  Mean +- sd over the 25 folds; per-seed means in brackets.", "",
              "| arm | scored model (averaged; with early stopping: the selected averaged snapshot) | last iterate of the same runs | averaged weights "
              "after the last epoch | chosen epochs (0-based) |", "|---|---|---|---|---|"]
    half = str(a.epochs // 2)
    arms = [("no averaging (fixed epoch count, last-epoch model)", [])]
    arms += [(f"--avg ema --avg-decay {d}", ["--avg", "ema", "--avg-decay", str(d)]) for d in (0.9, 0.99, 0.999)]
    arms += [(f"--avg swa --avg-start-epoch {half}", ["--avg", "swa", "--avg-start-epoch", half])]
    arms += [(f"--avg ema --avg-decay {d} --early-stop-patience {p} --inner-fraction 0.2", ["--avg", "ema", "--avg-decay", str(d), "--early-stop-patience",
                                                                                         str(p), "--inner-fraction", "0.2"])
             for d in (0.99, 0.999) for p in a.patience]

    def ms(v):
        seeds = ", ".join(f"{100 * statistics.mean(v[5 * i:5 * i + 5]):.1f}" for i in range(5))
        return f"{100 * statistics.mean(v):.1f} % +- {100 * statistics.stdev(v):.1f} % [{seeds}]"
    for name, extra in arms:
        log = os.path.join(tmp, f"{len(lines)}.jsonl")
        t0 = time.time()
        rc = train.main(recipe + extra + ["--out", os.path.join(tmp, "all.pth"), "--log-jsonl", log])
        assert rc == 0, rc
        recs = [json.loads(ln) for ln in open(log)]
        done = [r for r in recs if r.get("done")][0]
        folds = [r for r in recs if "fold" in r and "n_val" in r]
        assert len(folds) == 25, len(folds)
        scored = done["acc_val_folds"]
        if extra:
            it, av = [r["acc_val_last_iterate"] for r in folds], [r["acc_val_averaged"] for r in folds]
            lines.append(f"| {name} | {ms(scored)} | {ms(it)} | {ms(av)} | {sorted(done['best_epochs']) if 'best_epochs' in done else '-'} |")
        else:
            lines.append(f"| {name} | - | {ms(scored)} | - | - |")
        print(lines[-1], f"(whole command {time.time() - t0:.0f} s)", flush=True)
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--skip-cv", action="store_true")
    ap.add_argument("--skip-cost", action="store_true")
    ap.add_argument("--patience", type=int, nargs="+", default=[5, 30], help="early-stopping arms of the cross-validation")
    ap.add_argument("--commit", default="working tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weight_averaging.md"))
    a = ap.parse_args()
    clk = clocks()
    import torch
    import nsd_amd
    from nsd_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("weight_averaging: needs the MI355X (no GPU, no figures)")
    dev = torch.device("cuda:0")
    prop = torch.cuda.get_device_properties(dev)
    lines = ["# Weight averaging in the fused step tail: what the averaged row costs, and what it does to the accuracy", "",
             f"Machine: {prop.name} ({prop.multi_processor_count} CUs), torch {torch.__version__}.  Clocks before the run: {clk}.  Commit: {a.commit}.", "",
             f"Method: `python tools/weight_averaging.py --reps {a.reps} --epochs {a.epochs}` (its docstring describes the legs): medians (10th .. 90th "
             f"percentile) of {a.reps} repetitions after {a.warmup} untimed ones, the legs of a row alternating in one process.", ""]
    if not a.skip_cost:
        mbt = step_cost(a, torch, nsd_amd, ops, dev, lines)
        launch_cost(a, torch, ops, dev, mbt, lines)
        del mbt
    if not a.skip_cv:
        cross_validation(a, lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
