"""Time a model-batched training step (ModelBatchTrainer: M models of B trials per launch) against single-model Trainer steps.

    python tools/multi_model_step.py [--steps 50] [--warmup 10] [--train] [--out profiles/multi_model_step.jsonl]

HIP-event timing after a warm-up and a synchronise, the batched and the single-model legs alternating in one process.  Prints one
JSON line per (M, B, T) point: ms per batched step, ms per single-model step at the same B, and the throughput ratio
M * single / batched (how many single-model steps one batched step replaces per unit of time).

--train adds the end-to-end leg: `train.py --kfold 5 --epochs 20 --batch 32` on tests/golden/recorded_trials.npz with and without
--concurrent (wall time of each process, and the time to the folds' last epoch from their own elapsed_s lines, per-epoch evaluation
included; the final all-trials model trains the same way in both)."""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nsd_amd  # noqa: E402
from nsd_amd.trainer import Trainer  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--train", action="store_true", help="also time train.py --kfold 5 --epochs 20 --batch 32 with / without --concurrent")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    lines = []
    for M, B, T in [(5, 32, 625), (25, 32, 625), (5, 64, 625)]:
        x = torch.randn((M, B, T, 8), generator=g).to(dev)
        y = torch.randint(0, 3, (M, B), generator=g, dtype=torch.int32).to(dev)
        models = [nsd_amd.EEG_LSTM().to(dev).train() for _ in range(M)]
        mbt = nsd_amd.ModelBatchTrainer(models, seeds=list(range(M)))
        single = Trainer(nsd_amd.EEG_LSTM().to(dev).train(), seed=0)
        xs, ys = x[0].contiguous(), y[0].contiguous()
        tb, ts = [], []
        for _ in range(args.rounds):                       # alternating legs: drift hits both
            tb.append(_time(lambda: mbt.step(x, y), args.steps, args.warmup))
            ts.append(_time(lambda: single.step(xs, ys), args.steps, args.warmup))
        bt, st = min(tb), min(ts)
        rec = dict(M=M, B=B, T=T, ms_batched_step=round(bt, 4), ms_single_step=round(st, 4), batched_over_single=round(bt / st, 3),
                   throughput_ratio=round(M * st / bt, 2), rounds_batched=[round(v, 4) for v in tb], rounds_single=[round(v, 4) for v in ts],
                   steps=args.steps, warmup=args.warmup, device=torch.cuda.get_device_name(0))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.train:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        legs = {}
        for name, extra in (("sequential", []), ("concurrent", ["--concurrent"])):
            cmd = [sys.executable, "-c", "import sys, nsd_amd.train as t; sys.exit(t.main(sys.argv[1:]))", "--data",
                   os.path.join(root, "tests", "golden", "recorded_trials.npz"), "--kfold", "5", "--epochs", "20", "--batch", "32",
                   "--out", os.path.join("/tmp", f"multi_model_step_{name}.pth")] + extra
            t0 = time.time()
            p = subprocess.run(cmd, cwd=root, capture_output=True, text=True)
            wall = time.time() - t0
            if p.returncode != 0:
                raise SystemExit(f"train.py {name}: rc={p.returncode}\n{p.stderr[-2000:]}")
            recs = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
            last = {}
            for r in recs:
                if "epoch" in r and r["run"] != "all":
                    last[r["run"]] = r["elapsed_s"]
            folds_s = sum(last.values()) if name == "sequential" else max(last.values())
            legs[name] = dict(wall_s=round(wall, 2), folds_s=round(folds_s, 2),
                              acc_val_folds=[r["acc_val_last_epoch"] for r in recs if "fold" in r and "done" not in r])
        rec = dict(leg="train.py --kfold 5 --epochs 20 --batch 32 (recorded trials)", **{k: v for k, v in legs.items()},
                   folds_speedup=round(legs["sequential"]["folds_s"] / legs["concurrent"]["folds_s"], 2),
                   wall_speedup=round(legs["sequential"]["wall_s"] / legs["concurrent"]["wall_s"], 2))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
