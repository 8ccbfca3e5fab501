"""Time the model-batched training step with per-model settings (a hyper-parameter grid in one launch).

    python tools/hyper_grid_step.py [--steps 30] [--warmup 8] [--rounds 3] [--base libnsd_hip_base.so] [--grid] [--out profiles/hyper_grid.jsonl]

HIP-event timing after a warm-up and a synchronise, all legs alternating in ONE process, at least three rounds after one round that is
thrown away (first launches, allocations, clock ramp).  Per (M, B, T) point
one JSON line with the ms per ModelBatchTrainer step of
  uniform        one setting for all models (the calls the trainer always issued), this tree's library;
  heterogeneous  every setting per model (lr, weight decay, clip, schedule, augmentation, loss and dropout all differ);
  base_uniform   with --base: the uniform step on another build of the library loaded into the same process (tools/build_base.sh
                 builds the parent commit's as libnsd_hip_base.so),
each leg's rounds, its spread (max - min over its rounds), and the rules
  (a) uniform <= base_uniform + the larger spread of the two legs      (the uniform step is not slower than the parent's)
  (b) heterogeneous <= uniform + the larger spread of the two legs     (per-model settings cost nothing)
on the legs' best rounds.  Both uniform legs run with clipping on, so that the tail is the kernel pair this change touches.

--grid adds the end-to-end leg on tests/golden/recorded_trials.npz: `nsd_amd.grid` with 4 configurations x 5 folds, 20 epochs, batch 32,
against four `train --kfold 5 --concurrent` processes, one per configuration (wall time of the processes and the ratio; train also
trains its final all-trials model, which the grid does not)."""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nsd_amd  # noqa: E402
from nsd_amd import _lib, ops  # noqa: E402


def _load(name):
    """another build of the library in this process: the handle _lib.lib() returns while it is selected"""
    keep_path, keep = _lib.LIB_PATH, _lib._lib
    _lib.LIB_PATH, _lib._lib = os.path.join(os.path.dirname(keep_path), name), None
    try:
        return _lib.lib()
    finally:
        _lib.LIB_PATH, _lib._lib = keep_path, keep


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def _models(M, dev, drops):
    out = []
    for i in range(M):
        m = nsd_amd.EEG_LSTM().to(dev).train()
        m.dropout_p, m.head_dropout_p = drops[i]
        out.append(m)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--base", default=None, help="file name of another build beside libnsd_hip.so (tools/build_base.sh: libnsd_hip_base.so)")
    ap.add_argument("--grid", action="store_true", help="also the end-to-end leg: nsd_amd.grid against four train --kfold 5 --concurrent processes")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds: at least three")
    dev = torch.device("cuda:0")
    here = _lib.lib()
    base = _load(args.base) if args.base else None
    g = torch.Generator().manual_seed(0)
    lines = []
    for M, B, T in [(25, 32, 625), (32, 64, 625)]:
        x = torch.randn((M, B, T, 8), generator=g).to(dev)
        y = torch.randint(0, 3, (M, B), generator=g, dtype=torch.int32).to(dev)
        one = dict(lr=1e-3, weight_decay=1e-3, clip_grad_norm=1.0, lr_schedule=ops.LrSchedule(kind="cosine", warmup_steps=5, total_steps=10 ** 6),
                   augment=ops.Augment(max_shift=4, scale_range=0.1, p_channel=0.1, noise_std=0.1), loss=ops.Loss(label_smoothing=0.1, mixup=0.4))
        per = dict(lr=[1e-3 * (1 + i % 4) for i in range(M)], weight_decay=[1e-3 * (i % 3) for i in range(M)],
                   clip_grad_norm=[0.5 + 0.25 * (i % 5) for i in range(M)],
                   lr_schedule=[ops.LrSchedule(kind="cosine", warmup_steps=5 + i % 3, total_steps=10 ** 6) if i % 2 else
                                ops.LrSchedule(kind="step", step_size=1000 + i, gamma=0.9) for i in range(M)],
                   augment=[ops.Augment(max_shift=1 + i % 6, scale_range=0.05 * (1 + i % 3), p_channel=0.05 * (1 + i % 4), noise_std=0.05 * (1 + i % 5))
                            for i in range(M)],
                   loss=[ops.Loss(label_smoothing=0.05 * (1 + i % 3), mixup=0.2 + 0.1 * (i % 5)) for i in range(M)])
        uni_drops, het_drops = [(0.6, 0.6)] * M, [(0.3 + 0.05 * (i % 7), 0.6 - 0.05 * (i % 5)) for i in range(M)]
        legs = {"uniform": (here, nsd_amd.ModelBatchTrainer(_models(M, dev, uni_drops), seeds=list(range(M)), **one)),
                "heterogeneous": (here, nsd_amd.ModelBatchTrainer(_models(M, dev, het_drops), seeds=list(range(M)), **per))}
        if base is not None:
            legs["base_uniform"] = (base, nsd_amd.ModelBatchTrainer(_models(M, dev, uni_drops), seeds=list(range(M)), **one))
        rounds = {k: [] for k in legs}
        for rnd in range(-1, args.rounds):                 # alternating legs: drift hits all of them
            for k, (handle, tr) in legs.items():
                _lib._lib = handle
                try:
                    t = _time(lambda: tr.step(x, y), args.steps, args.warmup)
                finally:
                    _lib._lib = here
                if rnd >= 0:                               # (round -1 is thrown away: first launches, allocations, clock ramp)
                    rounds[k].append(t)
        best = {k: min(v) for k, v in rounds.items()}
        spread = {k: max(v) - min(v) for k, v in rounds.items()}
        rec = dict(M=M, B=B, T=T, steps=args.steps, warmup=args.warmup, device=torch.cuda.get_device_name(0),
                   **{f"ms_{k}": round(best[k], 4) for k in legs}, **{f"rounds_{k}": [round(v, 4) for v in rounds[k]] for k in legs},
                   **{f"spread_{k}": round(spread[k], 4) for k in legs})
        tol_b = max(spread["uniform"], spread["heterogeneous"])
        rec["rule_b_heterogeneous_not_slower_than_uniform"] = bool(best["heterogeneous"] <= best["uniform"] + tol_b)
        rec["heterogeneous_over_uniform"] = round(best["heterogeneous"] / best["uniform"], 4)
        if base is not None:
            tol_a = max(spread["uniform"], spread["base_uniform"])
            rec["rule_a_uniform_not_slower_than_base"] = bool(best["uniform"] <= best["base_uniform"] + tol_a)
            rec["uniform_over_base"] = round(best["uniform"] / best["base_uniform"], 4)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del legs
    if args.grid:
        fx = os.path.join(ROOT, "tests", "golden", "recorded_trials.npz")
        common = ["--data", fx, "--kfold", "5", "--epochs", "20", "--batch", "32"]

        def run(module, extra):
            cmd = [sys.executable, "-c", f"import sys, nsd_amd.{module} as t; sys.exit(t.main(sys.argv[1:]))"] + common + extra
            t0 = time.time()
            p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
            wall = time.time() - t0
            if p.returncode != 0:
                raise SystemExit(f"{module} {extra}: rc={p.returncode}\n{p.stderr[-2000:]}")
            return wall, [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
        wall_grid, out = run("grid", ["--grid", "dropout=0.4,0.6", "--grid", "lr=0.001,0.003"])
        sums = [r for r in out if r.get("summary")]
        walls, means = [], []
        for s in sums:
            w, recs = run("train", ["--concurrent", "--out", os.path.join("/tmp", "hyper_grid_step.pth")] + s["train_args"])
            walls.append(round(w, 2))
            means.append([r for r in recs if r.get("done")][0]["acc_val_mean"])
        done = [r for r in out if r.get("done")][0]
        rec = dict(leg="4 configurations x 5 folds, 20 epochs, batch 32 (recorded trials)", wall_s_grid=round(wall_grid, 2),
                   train_s_grid=done["elapsed_s"], wall_s_four_concurrent=round(sum(walls), 2), wall_s_each_concurrent=walls,
                   four_concurrent_over_grid=round(sum(walls) / wall_grid, 2), acc_val_mean_grid=[s["acc_val_mean"] for s in sums],
                   acc_val_mean_concurrent=means, best=done["best"])
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
