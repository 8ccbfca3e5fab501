"""Cost and effect of session alignment (nsd_cov_step / nsd_whiten_fit / nsd_spatial_apply), written as tables for
profiles/session_alignment.md.

    python tools/align_latency.py [--reps 300] [--warmup 30] [--commit <text>] [--out profiles/session_alignment_latency.md]
                                  [--accuracy] [--data tests/golden/recorded_trials_filtered.npz] [--work <dir>]

Latency (tools/gate_latency.py's method): every figure is GPU time between two HIP events recorded around the call(s) on the current
stream, after `--warmup` untimed repetitions, repeated `--reps` times; the table gives the median, the 10th / 90th percentile and the
mean.  The legs of a point alternate inside one repetition, in one process, on one GPU.  The plain legs run twice per repetition
(plain, plain'): their difference is the spread a difference of legs has to beat.  The legs:
  push         StreamDecoder.push of a 25-sample chunk, B = 1, 8, 64 streams: a model without the stage (launch for launch the push
               before the stage existed), with it, and with it and the accumulator on
  step         Trainer.step and the replayed Trainer.step_static at B = 64, T = 250, without and with the stage
  alone        nsd_spatial_apply, nsd_cov_step (a 25-sample chunk of 64 streams; 64 windows of 250 samples) and nsd_whiten_fit
               (64 accumulators, one group; C = 8 and C = 32), one launch each
Accuracy (--accuracy): the README's recipe on the recorded trials, 5 folds x 5 seeds in one model-batched run, without and with
--align; then a synthetic session shift -- every held-out trial multiplied by one fixed random mixing matrix of condition number 10 --
decoded (a) by the unaligned models, (b) by the aligned models with their training matrix, (c) by the aligned models after a label-free
refit of the matrix on the shifted held-out trials.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHUNK, STREAMS, B_STEP, T_STEP = 25, (1, 8, 64), 64, 250


def _pct(v, q):
    s = sorted(v)
    return s[min(len(s) - 1, int(q * len(s)))]


def _fmt(v):
    return f"{statistics.median(v):6.1f} ({_pct(v, 0.1):.1f} .. {_pct(v, 0.9):.1f}; mean {statistics.fmean(v):.1f})"


def _measure(calls, reps, warmup, torch):
    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3                       # microseconds
    t = {k: [] for k in calls}
    for rep in range(warmup + reps):
        got = {k: timed(fn) for k, fn in calls.items()}
        if rep >= warmup:
            for k, v in got.items():
                t[k].append(v)
    torch.cuda.synchronize()
    return t


def latency(a, torch, nsd_amd, ops, dev):
    from nsd_amd.trainer import Trainer
    med = statistics.median
    A = nsd_amd.SessionAlign()
    g = torch.Generator().manual_seed(0)
    mix = (torch.eye(8) + 0.1 * torch.randn((8, 8), generator=g)).to(dev)

    def model(align, train=False):
        torch.manual_seed(1)
        m = nsd_amd.EEG_LSTM(align=A if align else None, align_matrix=mix if align else None).to(dev)
        return m.train() if train else m.eval()

    lines = ["## Latency", "",
             "| point | plain, us | aligned, us | aligned - plain (medians) | spread (plain' - plain) | more |", "|---|---|---|---|---|---|"]
    for B in STREAMS:
        x = (2.7 * torch.randn((B, CHUNK, 8), generator=g)).to(dev)
        dec = {k: nsd_amd.StreamDecoder(model(k.startswith("aligned")), streams=B) for k in ("plain", "plain2", "aligned", "aligned_acc")}
        dec["aligned_acc"].align_accumulate(True)
        t = _measure({k: (lambda d=d: d.push(x)) for k, d in dec.items()}, a.reps, a.warmup, torch)
        lines.append(f"| push, B = {B} | {_fmt(t['plain'])} | {_fmt(t['aligned'])} | {med(t['aligned']) - med(t['plain']):+.1f} | "
                     f"{abs(med(t['plain2']) - med(t['plain'])):.1f} | accumulating: {_fmt(t['aligned_acc'])} "
                     f"({med(t['aligned_acc']) - med(t['plain']):+.1f}) |")
    x = (2.7 * torch.randn((B_STEP, T_STEP, 8), generator=g)).to(dev)
    y = torch.randint(0, 3, (B_STEP,), generator=g, dtype=torch.int32).to(dev)
    tr = {k: Trainer(model(k == "aligned", train=True), lr=1e-3, seed=3) for k in ("plain", "plain2", "aligned")}
    t = _measure({k: (lambda q=q: q.step(x, y)) for k, q in tr.items()}, a.reps, a.warmup, torch)
    lines.append(f"| Trainer.step, B = {B_STEP}, T = {T_STEP} | {_fmt(t['plain'])} | {_fmt(t['aligned'])} | "
                 f"{med(t['aligned']) - med(t['plain']):+.1f} | {abs(med(t['plain2']) - med(t['plain'])):.1f} | |")
    for q in tr.values():
        xs, ys = q.static_inputs(B_STEP, T_STEP)
        xs.copy_(x)
        ys.copy_(y)
    t = _measure({k: (lambda q=q: q.step_static(B_STEP, T_STEP)) for k, q in tr.items()}, a.reps, a.warmup, torch)
    lines.append(f"| Trainer.step_static (replayed), B = {B_STEP}, T = {T_STEP} | {_fmt(t['plain'])} | {_fmt(t['aligned'])} | "
                 f"{med(t['aligned']) - med(t['plain']):+.1f} | {abs(med(t['plain2']) - med(t['plain'])):.1f} | |")
    # the three launches alone
    xc = (2.7 * torch.randn((64, CHUNK, 8), generator=g)).to(dev)
    out_c, out_w = torch.empty_like(xc), torch.empty_like(x)
    state = ops.cov_state(8, 64, dev)
    win = (torch.empty((64, 8, 8), dtype=torch.float64, device=dev), torch.empty((64, 2), dtype=torch.int64, device=dev))
    sums8, counts8 = ops.cov_step(x)
    x32 = (2.7 * torch.randn((64, T_STEP, 32), generator=g)).to(dev)
    sums32, counts32 = ops.cov_step(x32)
    W8, r8 = ops.whiten_fit(8, A, sums8, counts8)
    W32, r32 = ops.whiten_fit(32, A, sums32, counts32)
    sweeps = (ops.whiten_records(r8, 1)[0]["sweeps"], ops.whiten_records(r32, 1)[0]["sweeps"])
    alone = {
        f"nsd_spatial_apply, 64 x {CHUNK} x 8": lambda: ops.spatial_apply(xc, mix, out=out_c),
        f"nsd_spatial_apply, 64 x {T_STEP} x 8": lambda: ops.spatial_apply(x, mix, out=out_w),
        f"nsd_cov_step, stream mode, 64 x {CHUNK} x 8": lambda: ops.cov_step(xc, state),
        f"nsd_cov_step, window mode, 64 x {T_STEP} x 8": lambda: ops.cov_step(x, out=win),
        f"nsd_cov_step, window mode, 64 x {T_STEP} x 32": lambda: ops.cov_step(x32, out=(sums32, counts32)),
        f"nsd_whiten_fit, C = 8, 64 accumulators, {sweeps[0]} sweeps": lambda: ops.whiten_fit(8, A, sums8, counts8, out=W8, records=r8),
        f"nsd_whiten_fit, C = 32, 64 accumulators, {sweeps[1]} sweeps": lambda: ops.whiten_fit(32, A, sums32, counts32, out=W32, records=r32),
    }
    t = _measure(alone, a.reps, a.warmup, torch)
    lines += ["", "| launch alone | us |", "|---|---|"] + [f"| {k} | {_fmt(v)} |" for k, v in t.items()] + [""]
    return lines


def accuracy(a, torch, nsd_amd, ops, dev):
    import numpy as np
    from nsd_amd import data as D
    from nsd_amd import train
    if a.work is None:
        import tempfile
        a.work = tempfile.mkdtemp(prefix="align_accuracy_")
    os.makedirs(a.work, exist_ok=True)
    ts = D.load_trials_npz(a.data, x_key="x_filt")
    recipe = ["--data", a.data, "--npz-key", "x_filt", "--classes", "3", "--T", "625", "--epochs", "200", "--batch", "32", "--lr", "0.001",
              "--dropout", "0.6", "--seed", "1", "--kfold", "5", "--concurrent", "--kfold-seeds", "5", "--log-every", "100000", "--save-folds"]
    done = {}
    for arm, extra in (("off", []), ("on", ["--align"])):
        log = os.path.join(a.work, f"{arm}.jsonl")
        if os.path.exists(log):
            os.remove(log)
        t0 = time.time()
        rc = train.main(recipe + extra + ["--out", os.path.join(a.work, f"{arm}.pth"), "--log-jsonl", log])
        if rc:
            raise SystemExit(f"align_latency: train ({arm}) returned {rc}")
        done[arm] = json.loads(open(log).read().strip().splitlines()[-1])
        done[arm]["wall_s"] = time.time() - t0
    runs = train.concurrent_runs(ts.y, 5, 5, 1, 32)
    rs = np.random.RandomState(2024)
    U, _ = np.linalg.qr(rs.standard_normal((8, 8)))
    V, _ = np.linalg.qr(rs.standard_normal((8, 8)))
    mixing = ((U * np.logspace(0.0, -1.0, 8)) @ V.T).astype(np.float32)              # singular values 1 .. 0.1: condition number 10
    mixing /= np.float32(np.sqrt((mixing ** 2).sum() / 8))                           # (overall scale kept)
    x_all, y_all = torch.from_numpy(ts.x).to(dev), ts.y

    def fold_models(arm):
        paths = done[arm]["fold_checkpoints"]
        assert len(paths) == len(runs), (len(paths), len(runs))
        return [nsd_amd.SimplePredictor(p, sr=125, device="cpu", preprocess="identity").model for p in paths]

    def acc(model, xs, ys):
        return float((model.predict_proba(xs).argmax(1).cpu().numpy() == ys).mean())

    arms = {"a: unaligned models": [], "b: aligned models, training matrix": [], "c: aligned models, label-free refit on the shifted trials": [],
            "aligned models, unshifted (check: the run's own figure)": [], "unaligned models, unshifted (check)": []}
    off, on = fold_models("off"), fold_models("on")
    few = 0
    for k, r in enumerate(runs):
        va = torch.from_numpy(r["va"]).to(dev)
        xs, ys = x_all[va], y_all[r["va"]]
        shifted = (xs @ torch.from_numpy(mixing).to(dev).T).contiguous()
        arms["unaligned models, unshifted (check)"].append(acc(off[k], xs, ys))
        arms["aligned models, unshifted (check: the run's own figure)"].append(acc(on[k], xs, ys))
        arms["a: unaligned models"].append(acc(off[k], shifted, ys))
        arms["b: aligned models, training matrix"].append(acc(on[k], shifted, ys))
        W, rec = on[k].align.fit(on[k], shifted)
        few += int(rec[0]["few"] or rec[0]["nonfinite"])
        on[k].set_alignment(W[0], record=rec[0])
        arms["c: aligned models, label-free refit on the shifted trials"].append(acc(on[k], shifted, ys))

    def ms(v):
        v = np.asarray(v)
        per_seed = [float(v[i * 5:(i + 1) * 5].mean()) for i in range(5)]
        return f"{100 * v.mean():.1f} % +- {100 * v.std(ddof=1):.1f} %", ", ".join(f"{100 * s:.1f}" for s in per_seed)

    lines = ["## Accuracy on the recorded trials", "",
             f"Recipe (the README's): `python -m nsd_amd.train {' '.join(recipe[2:-1])}` on `{os.path.relpath(a.data, ROOT)}` "
             f"({len(ts.y)} trials), plus `--align` for the aligned arm: 25 models in one model-batched run per arm "
             f"(wall time {done['off']['wall_s']:.1f} s / {done['on']['wall_s']:.1f} s including the all-trials model).  Mean +- sd over the 25 "
             "folds; per-seed means in brackets.", "",
             "| arm | held-out accuracy | per-seed means |", "|---|---|---|"]
    for arm in ("off", "on"):
        v = np.asarray(done[arm]["acc_val_folds"])
        m, p = ms(v)
        lines.append(f"| alignment {arm} | {m} | {p} |")
    lines += ["", "Synthetic session shift: every held-out trial x -> M x with one fixed random mixing matrix M (singular values 1 .. 0.1, "
              "condition number 10, Frobenius norm sqrt(8)); the fold models are the checkpoints of the runs above "
              f"({few} of 25 refits kept the identity).", "",
              "| decoded by | held-out accuracy under the shift | per-seed means |", "|---|---|---|"]
    for name, v in arms.items():
        m, p = ms(v)
        lines.append(f"| {name} | {m} | {p} |")
    lines.append("")
    return lines


def main():
    import torch
    import nsd_amd
    from nsd_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--commit", default="working tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_alignment_latency.md"))
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--no-latency", action="store_true")
    ap.add_argument("--data", default=os.path.join(ROOT, "tests", "golden", "recorded_trials_filtered.npz"))
    ap.add_argument("--work", default=None, help="where the accuracy runs keep their logs and fold checkpoints (default: a temporary directory)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("align_latency: needs the MI355X (no GPU, no figures)")
    dev = torch.device("cuda:0")
    lines = [f"Machine: {torch.cuda.get_device_name(dev)}, torch {torch.__version__}.  Commit: {a.commit}.", "",
             f"Method: `python tools/align_latency.py --reps {a.reps} --warmup {a.warmup}{' --accuracy' if a.accuracy else ''}`.  GPU time "
             f"between two HIP events around the call(s), microseconds, median (10th .. 90th percentile; mean) of {a.reps} repetitions after "
             f"{a.warmup} untimed ones; the legs of a point alternate inside each repetition, one process.  Reference shape (C = 8, H = 48, "
             "L = 2, K = 3), fp32.", ""]
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
