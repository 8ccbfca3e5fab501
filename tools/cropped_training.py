"""Cropped training measured: what the crop stage costs in a step, and what training on random windows and deciding trials by pooled
windows does to the cross-validated accuracy of the recorded trials.  Writes the tables of profiles/cropped_training.md.

    python tools/cropped_training.py [--reps 30] [--epochs 200] [--commit <text>] [--out profiles/cropped_training.md]

1. Cost of a step.  Two trainers of the same model and seed step side by side in one process, the legs alternating:
     plain    Trainer() on a pre-cropped [256, 250, 8] batch -- with crop=None the trainer issues the parent commit's calls on kernels this
              change does not touch, so this leg is the parent's step, measured in the same session
     cropped  Trainer(crop=Crop(250, 4)) on [64, 625, 8] trials: the same 256 rows of 250 samples, cut on the device inside the step
   eager and replayed from the step's hipGraph.  A repetition is STEPS steps between two device synchronisations, host clock, divided
   by STEPS.  The difference of the medians stands beside the wider 10th .. 90th spread of the two legs.
2. nsd_crop alone at that shape (and for 25 models of 32 trials): GPU time between two HIP events around the one call, launch latency
   included.
3. `python -m nsd_amd.train --kfold 5 --concurrent --kfold-seeds 5` with the README's recipe on the recorded trials, for windows of 250,
   375 and 500 samples, 4 drawn crops per trial and step, each once without and once with `--avg ema --avg-decay 0.99`: the trial-level
   accuracy (pooled over the windows half a window apart) and the accuracy of each trial's first window alone.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = 10
WINDOWS = (250, 375, 500)


def _pct(v, q):
    s = sorted(v)
    return s[min(len(s) - 1, int(q * len(s)))]


def _fmt(v, digits=1):
    return f"{statistics.median(v):.{digits}f} ({_pct(v, 0.1):.{digits}f} .. {_pct(v, 0.9):.{digits}f})"


def _spread(v):
    return _pct(v, 0.9) - _pct(v, 0.1)


def _alternate(a, torch, legs):
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


def step_cost(a, torch, nsd_amd, ops, dev, lines):
    from nsd_amd.trainer import Trainer
    lines += [f"## 1. Cost of a step: microseconds per step ({STEPS} steps per repetition, host clock between two synchronisations)", "",
              "| step | plain: the parent's step on pre-cropped [256, 250, 8] | cropped: Trainer(crop=Crop(250, 4)) on [64, 625, 8] | cropped - plain | "
              "spread: wider of the legs' 10th .. 90th |", "|---|---|---|---|---|"]
    B, T, W, R = 64, 625, 250, 4
    crop = ops.Crop(W, R)
    g = torch.Generator().manual_seed(1234)
    x = (2.7 * torch.randn((B, T, 8), generator=g)).to(dev)
    y = torch.randint(0, 3, (B,), generator=g, dtype=torch.int32).to(dev)
    xc, yc, _ = ops.crop(x, crop, dict(seed=1, base_stream=4), labels=y)

    def trainer(**kw):
        torch.manual_seed(0)
        return Trainer(nsd_amd.EEG_LSTM(8, 48, 2, 3, 0.6).to(dev).train(), seed=1, **kw)
    for mode in ("eager", "graph"):
        plain, cropped = trainer(), trainer(crop=crop)
        if mode == "graph":
            xs, ys = plain.static_inputs(B * R, W)
            xs.copy_(xc); ys.copy_(yc)
            xs, ys = cropped.static_inputs(B, T)
            xs.copy_(x); ys.copy_(y)
            legs = {"plain": lambda: [plain.step_static(B * R, W) for _ in range(STEPS)],
                    "cropped": lambda: [cropped.step_static(B, T) for _ in range(STEPS)]}
        else:
            legs = {"plain": lambda: [plain.step(xc, yc) for _ in range(STEPS)], "cropped": lambda: [cropped.step(x, y) for _ in range(STEPS)]}
        t = _alternate(a, torch, legs)
        d = statistics.median(t["cropped"]) - statistics.median(t["plain"])
        lines.append(f"| Trainer, B x R = {B * R}, W = {W} from T = {T}, {mode} | {_fmt(t['plain'])} | {_fmt(t['cropped'])} | {d:+.1f} | "
                     f"{max(_spread(t['plain']), _spread(t['cropped'])):.1f} |")
        print(lines[-1], flush=True)
    lines.append("")


def launch_cost(a, torch, ops, dev, lines):
    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3
    legs = {}
    for name, M, B in (("one model, 64 trials -> 256 rows of 250 x 8 (2.0 MB written)", 1, 64),
                       ("25 models, 32 trials each -> 3200 rows of 250 x 8 (25.6 MB written)", 25, 32)):
        x = torch.randn((M, B, 625, 8), device=dev)
        lab = torch.zeros(M * B, dtype=torch.int32, device=dev)
        out = torch.empty((M, B * 4, 250, 8), device=dev)
        lo = torch.empty(M * B * 4, dtype=torch.int32, device=dev)
        rngs = [dict(seed=m, base_stream=4) for m in range(M)]
        legs[name] = lambda x=x, lab=lab, out=out, lo=lo, rngs=rngs: ops.crop(x, ops.Crop(250, 4), rngs, labels=lab, out=out, labels_out=lo)
    probs = torch.softmax(torch.randn((25 * 65, 4, 3), device=dev), -1)
    po, pl = torch.empty((25 * 65, 3), device=dev), torch.empty((25 * 65, 3), device=dev)
    legs["nsd_crop_pool, 25 x 65 trials of 4 windows, K = 3"] = lambda: ops.crop_pool(probs, out=po, logits=pl)
    times = {k: [] for k in legs}
    for r in range(a.warmup + a.reps):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t = timed(fn)
            if r >= a.warmup:
                times[name].append(t)
    lines += ["## 2. The calls alone: GPU time between two HIP events around the one call, microseconds", "", "| call | time |", "|---|---|"]
    lines += [f"| {k} | {_fmt(v)} |" for k, v in times.items()] + [""]
    print("\n".join(lines[-len(times) - 1:]), flush=True)


def cross_validation(a, lines):
    from nsd_amd import train
    data = os.path.join(ROOT, "tests", "golden", "recorded_trials_filtered.npz")
    recipe = ["--data", data, "--npz-key", "x_filt", "--classes", "3", "--T", "625", "--epochs", str(a.epochs), "--batch", "32", "--lr", "0.001",
              "--dropout", "0.6", "--seed", "1", "--kfold", "5", "--concurrent", "--kfold-seeds", "5", "--log-every", "100000"]
    tmp = tempfile.mkdtemp()
    lines += ["## 3. 5 folds x 5 seeds on the recorded trials: outer-fold accuracy of the 25 models of each window", "",
              f"Recipe (the README's): `python -m nsd_amd.train {' '.join(recipe[2:])}` on `tests/golden/recorded_trials_filtered.npz`, plus "
              "`--crop-seconds S --crops-per-trial 4` (the evaluation grid: half a window apart) and the arm's options.  Mean +- sd over the 25 "
              "folds; per-seed means in brackets.  pooled: every held-out trial decided by the mean of its windows' probabilities; first window: by "
              "its first window alone, the decision a live user has after S seconds.", "",
              "| arm | window | windows per trial at evaluation | pooled | first window | whole command |", "|---|---|---|---|---|---|"]

    def ms(v):
        seeds = ", ".join(f"{100 * statistics.mean(v[5 * i:5 * i + 5]):.1f}" for i in range(5))
        return f"{100 * statistics.mean(v):.1f} % +- {100 * statistics.stdev(v):.1f} % [{seeds}]"
    for name, extra in (("last iterate", []), ("--avg ema --avg-decay 0.99 (the averaged models are scored)", ["--avg", "ema", "--avg-decay", "0.99"])):
        for W in WINDOWS:
            log = os.path.join(tmp, f"{len(lines)}.jsonl")
            t0 = time.time()
            rc = train.main(recipe + extra + ["--crop-seconds", repr(W / 125.0), "--crops-per-trial", "4", "--log-jsonl", log,
                                              "--out", os.path.join(tmp, "model.pth")])
            assert rc == 0, rc
            folds = [r for r in map(json.loads, open(log)) if "fold" in r and "acc_val_last_epoch" in r]
            assert len(folds) == 25, len(folds)
            grid = (625 - W) // (W // 2) + 1
            lines.append(f"| {name} | {W} samples ({W / 125.0:g} s) | {grid} | {ms([r['acc_val_last_epoch'] for r in folds])} | "
                         f"{ms([r['acc_val_first_window'] for r in folds])} | {time.time() - t0:.0f} s |")
            print(lines[-1], flush=True)
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--skip-cv", action="store_true")
    ap.add_argument("--skip-cost", action="store_true")
    ap.add_argument("--commit", default="working tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cropped_training.md"))
    a = ap.parse_args()
    import torch
    import nsd_amd
    from nsd_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("cropped_training: needs the MI355X (no GPU, no figures)")
    dev = torch.device("cuda:0")
    prop = torch.cuda.get_device_properties(dev)
    lines = ["# Cropped training: what the crop stage costs in a step, and what random windows and pooled decisions do to the accuracy", "",
             f"Machine: {prop.name} ({prop.multi_processor_count} CUs), torch {torch.__version__}.  Commit: {a.commit}.", "",
             f"Method: `python tools/cropped_training.py --reps {a.reps} --epochs {a.epochs}` (its docstring describes the legs): medians (10th .. 90th "
             f"percentile) of {a.reps} repetitions after {a.warmup} untimed ones, the legs of a row alternating in one process.", ""]
    if not a.skip_cost:
        step_cost(a, torch, nsd_amd, ops, dev, lines)
        launch_cost(a, torch, ops, dev, lines)
    if not a.skip_cv:
        cross_validation(a, lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
