"""Whole epochs timed on the recorded trials: what fetching each step's batch costs on the host, and what gathering it on the device
(nsd_gather, Trainer.bind_batches / step_scheduled) makes of it.  Writes the tables of profiles/device_batches.md.

    python tools/bench_epoch.py [--reps 40] [--warmup 3] [--legs a,b,c,d,e5,f5,e25,f25,g] [--tag this] [--json out.jsonl]

The 324 recorded trials, their first 250 samples (T = 250, C = 8), batches of train.py's default 64: 5 steps per epoch for one model on
all trials, 4 per epoch for the folds of a 5-fold split.  Legs, each with a trainer of its own and the reference model's shape
(H = 48; five classes, so that every recorded trial has a label):
  a    Trainer.step fed by train.py's host loop: permute, copy the indices, index x_all / y_all, make both contiguous
  b    Trainer.step_static, the static inputs filled by index_select(out=) from host-copied indices
  c    Trainer.step_scheduled()             -- the gather issued eagerly in front of a's step
  d    Trainer.step_scheduled(static=True)  -- the gather as the first node of b's graph
  e5 / e25   ModelBatchTrainer.step fed by train.py's concurrent loop for 5 folds / 5 seeds x 5 folds (M index copies, 2 M index
             kernels, two stacks per step)
  f5 / f25   its step_scheduled(): one gather for all M models
  g    nsd_gather alone: GPU time between two HIP events around LAUNCHES back-to-back launches, for one model at B = 256 and for 25
       models at B = 64; bytes moved = 2 x M x B x T x C x 4 (read and written), against the HBM copy rate of the device
A repetition is one epoch between two device synchronisations on the host clock, divided by its steps; the legs alternate inside every
repetition, so they share whatever else the host is doing.  Reported: the median and the 10th .. 90th percentile of the repetitions.
Legs a, b and e use nothing this feature adds: the same file run from a checkout of the parent commit (--legs a,b,e5,e25 --tag parent)
is the baseline.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
T, BATCH, LAUNCHES = 250, 64, 200
HBM_COPY_TBS = 6.29                      # measured float4 copy rate of the MI355X (79 % of the 8.0 TB/s specification)


def _pct(v, q):
    s = sorted(v)
    return s[min(len(s) - 1, int(q * len(s)))]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", default=os.path.join(ROOT, "tests", "golden", "recorded_trials.npz"))
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="a,b,c,d,e5,f5,e25,f25,g")
    ap.add_argument("--tag", default="this")
    ap.add_argument("--json", default=None, help="append the result lines to this file")
    args = ap.parse_args(argv)

    import numpy as np
    import torch

    import nsd_amd
    from nsd_amd import data as D
    from nsd_amd.train import concurrent_epoch, concurrent_runs
    from nsd_amd.trainer import Trainer
    if not torch.cuda.is_available():
        print("bench_epoch: needs an MI355X (a timing without the device says nothing)", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    ts = D.load_trials_npz(args.data, D.LABELS_5CLASS)         # all five classes: every recorded trial
    x_np, y_np = np.ascontiguousarray(ts.x[:, :T]), ts.y
    x_all, y_all = torch.from_numpy(x_np).to(dev), torch.from_numpy(y_np).to(dev)
    N, epochs = len(y_np), args.warmup + args.reps
    legs = [s for s in args.legs.split(",") if s]

    def model(seed):
        torch.manual_seed(seed)
        return nsd_amd.EEG_LSTM(8, 48, 2, 5).to(dev).train()

    # every leg: (steps per epoch, epoch(e) -> issues epoch e's steps)
    made = {}
    everything = np.arange(N)
    tr_dev = torch.from_numpy(everything).to(dev)
    for leg in legs:
        if leg in ("a", "b", "c", "d"):
            tr = Trainer(model(1), lr=1e-3, seed=2)
            n_steps = N // BATCH
            if leg == "a":
                def epoch(e, tr=tr):
                    for idx in D.epoch_batches(N, BATCH, 0, e, drop_last=True):
                        sel = tr_dev[torch.from_numpy(idx).to(dev)]
                        tr.step(x_all[sel].contiguous(), y_all[sel].contiguous(), global_batch=len(idx))
            elif leg == "b":
                xs, ys = tr.static_inputs(BATCH, T)

                def epoch(e, tr=tr, xs=xs, ys=ys):
                    for idx in D.epoch_batches(N, BATCH, 0, e, drop_last=True):
                        sel = tr_dev[torch.from_numpy(idx).to(dev)]
                        torch.index_select(x_all, 0, sel, out=xs)
                        torch.index_select(y_all, 0, sel, out=ys)
                        tr.step_static(BATCH, T)
            else:
                tr.bind_batches(D.DeviceTrialSet(x_all, y_all, dev), D.BatchSchedule.for_run(everything, BATCH, 0, epochs))

                def epoch(e, tr=tr, static=leg == "d", n=n_steps):
                    for _ in range(n):
                        tr.step_scheduled(static=static)
            made[leg] = (n_steps, epoch)
        elif leg[0] in ("e", "f"):
            M = int(leg[1:])
            runs = concurrent_runs(y_np, 5, M // 5, 0, BATCH)
            assert len(runs) == M, (leg, len(runs))
            mbt = nsd_amd.ModelBatchTrainer([model(10 + k) for k in range(M)], lr=1e-3, seeds=[r["seed"] + 1 for r in runs])
            n_steps = concurrent_epoch(runs, BATCH, 0, lambda idxs: None)
            if leg[0] == "e":
                tr_devs = [torch.from_numpy(r["tr"]).to(dev) for r in runs]

                def step(idxs, mbt=mbt, tr_devs=tr_devs):
                    sel = [tr_devs[k][torch.from_numpy(ix).to(dev)] for k, ix in enumerate(idxs)]
                    mbt.step(torch.stack([x_all[s_] for s_ in sel]), torch.stack([y_all[s_] for s_ in sel]))
            else:
                mbt.bind_batches(D.DeviceTrialSet(x_all, y_all, dev), D.BatchSchedule.for_runs(runs, BATCH, epochs))

                def step(idxs, mbt=mbt):
                    mbt.step_scheduled()
            made[leg] = (n_steps, lambda e, runs=runs, step=step: concurrent_epoch(runs, BATCH, e, step))
        elif leg != "g":
            ap.error(f"--legs: unknown leg {leg!r}")

    out = []
    times = {leg: [] for leg in made}
    for e in range(epochs):                                          # the legs alternate inside every repetition
        for leg, (n_steps, epoch) in made.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            epoch(e)
            torch.cuda.synchronize()
            if e >= args.warmup:
                times[leg].append((time.perf_counter() - t0) / n_steps * 1e6)
    for leg, v in times.items():
        out.append({"tag": args.tag, "leg": leg, "steps_per_epoch": made[leg][0], "reps": len(v), "us_per_step_median": round(statistics.median(v), 1),
                    "us_per_step_p10": round(_pct(v, 0.1), 1), "us_per_step_p90": round(_pct(v, 0.9), 1)})

    if "g" in legs:
        from nsd_amd import ops
        for M, B in ((1, 256), (25, 64)):
            table = torch.from_numpy(np.random.RandomState(0).randint(0, N, (M, 8, B)).astype(np.int32)).to(dev)
            xo = torch.empty((M, B, T, 8), dtype=torch.float32, device=dev)
            lo = torch.empty((M * B,), dtype=torch.int32, device=dev)
            call = lambda s: ops.gather_batch(x_all, table, step=s, labels_all=y_all, out=xo, labels_out=lo)      # noqa: E731
            for s in range(20):
                call(s)
            v = []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for s in range(LAUNCHES):
                    call(s)
                b.record()
                b.synchronize()
                v.append(a.elapsed_time(b) * 1e3 / LAUNCHES)
            nbytes = 2 * M * B * T * 8 * 4
            us = statistics.median(v)
            out.append({"tag": args.tag, "leg": f"g M={M} B={B}", "reps": len(v), "launches_per_rep": LAUNCHES, "us_per_launch_median": round(us, 2),
                        "us_per_launch_p10": round(_pct(v, 0.1), 2), "us_per_launch_p90": round(_pct(v, 0.9), 2), "bytes": nbytes,
                        "gb_per_s": round(nbytes / us / 1e3, 1), "share_of_hbm_copy_rate": round(nbytes / us / 1e3 / (HBM_COPY_TBS * 1e3), 3)})
    for rec in out:
        line = json.dumps(rec)
        print(line, flush=True)
        if args.json:
            with open(args.json, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
