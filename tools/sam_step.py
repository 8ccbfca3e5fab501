"""Sharpness-aware minimisation measured: what a SAM step costs beyond two plain steps, and what it does to the cross-validated accuracy
of the recorded trials.  Writes the tables of profiles/sam.md.

    python tools/sam_step.py [--reps 30] [--epochs 200] [--commit <text>] [--out profiles/sam.md]

1. Cost of a step.  Trainers of the same model, seed and data step side by side in one process, the legs alternating:
     plain    Trainer() -- the default step: with sam=None the trainer issues the parent commit's calls on kernels this change does not
              touch, so this leg is the parent's step, measured in the same session
     guarded  clip_grad_norm=0.0 -- the parent's step with the guarded tail SAM switches on
     sam      sam=ops.Sam(0.05) -- two forward/backward pairs, the ascent's two launches, one guarded tail
   The yardstick is TWICE the plain step: the excess is median(sam) - 2 * median(plain), beside the wider 10th .. 90th spread of the
   two legs (the plain one's counted twice).  A repetition is STEPS steps between two device synchronisations, host clock, divided by
   STEPS.  Trainer at B = 256, T = 250, eager and replayed from its hipGraph; ModelBatchTrainer at M = 25, B = 32, T = 625.
2. The ascent alone (nsd_sam_ascend at P = 31 764, nsd_multi_sam_ascend at M = 25) and the clipped tail alone, each on the slabs of one
   evaluation: GPU time between two HIP events around the one call, launch latencies included.
3. `python -m nsd_amd.grid --grid sam_rho=0,0.02,0.05,0.1,0.2` with the README's recipe on the recorded trials, 5 folds x 5 seeds, once
   without and once with `--avg ema --avg-decay 0.99`.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = 10
RHOS = "0,0.02,0.05,0.1,0.2"


def _pct(v, q):
    s = sorted(v)
    return s[min(len(s) - 1, int(q * len(s)))]


def _fmt(v, digits=1):
    return f"{statistics.median(v):.{digits}f} ({_pct(v, 0.1):.{digits}f} .. {_pct(v, 0.9):.{digits}f})"


def _spread(v):
    return _pct(v, 0.9) - _pct(v, 0.1)


def _alternate(a, torch, legs, per=STEPS):
    times = {k: [] for k in legs}
    for r in range(a.warmup + a.reps):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= a.warmup:
                times[name].append((time.perf_counter() - t0) * 1e6 / per)
    return times


def _row(what, t):
    p, g, s = (statistics.median(t[k]) for k in ("plain", "guarded", "sam"))
    return (f"| {what} | {_fmt(t['plain'])} | {_fmt(t['guarded'])} | {_fmt(t['sam'])} | {s - 2 * p:+.1f} | {s - 2 * g:+.1f} | "
            f"{max(2 * _spread(t['plain']), _spread(t['sam'])):.1f} |")


def step_cost(a, torch, nsd_amd, ops, dev, lines):
    from nsd_amd.trainer import Trainer
    lines += [f"## 1. Cost of a step: microseconds per step ({STEPS} steps per repetition, host clock between two synchronisations)", "",
              "| step | plain (the parent's step) | guarded tail (clip_grad_norm=0.0) | SAM (rho 0.05) | SAM - 2 x plain | SAM - 2 x guarded | "
              "spread: wider of 2 x plain's and SAM's 10th .. 90th |", "|---|---|---|---|---|---|---|"]
    sam = ops.Sam(0.05)
    B, T = 256, 250
    g = torch.Generator().manual_seed(1234)
    x = (2.7 * torch.randn((B, T, 8), generator=g)).to(dev)
    y = torch.randint(0, 3, (B,), generator=g, dtype=torch.int32).to(dev)

    def trainer(**kw):
        torch.manual_seed(0)
        return Trainer(nsd_amd.EEG_LSTM(8, 48, 2, 3, 0.6).to(dev).train(), seed=1, **kw)
    for mode in ("eager", "graph"):
        trio = {"plain": trainer(), "guarded": trainer(clip_grad_norm=0.0), "sam": trainer(sam=sam)}
        if mode == "graph":
            for t in trio.values():
                xs, ys = t.static_inputs(B, T)
                xs.copy_(x); ys.copy_(y)
        legs = {k: (lambda t=t: [t.step(x, y) for _ in range(STEPS)]) if mode == "eager" else (lambda t=t: [t.step_static(B, T) for _ in range(STEPS)])
                for k, t in trio.items()}
        times = _alternate(a, torch, legs)
        rec = trio["sam"].last_sam()
        lines.append(_row(f"Trainer, B = {B}, T = {T}, {mode} (skipped {trio['sam'].skipped_steps()}, last ascent: norm {rec['norm']:.3g}, "
                          f"nonfinite {rec['nonfinite']})", times))
        print(lines[-1], flush=True)
        del trio, legs
    M, B, T = 25, 32, 625
    xm = (2.7 * torch.randn((M, B, T, 8), generator=g)).to(dev)
    ym = torch.randint(0, 3, (M, B), generator=g, dtype=torch.int32).to(dev)

    def batch(**kw):
        models = []
        for m in range(M):
            torch.manual_seed(m)
            models.append(nsd_amd.EEG_LSTM(8, 48, 2, 3, 0.6).to(dev).train())
        return nsd_amd.ModelBatchTrainer(models, seeds=list(range(M)), **kw)
    trio = {"plain": batch(), "guarded": batch(clip_grad_norm=0.0), "sam": batch(sam=sam)}
    times = _alternate(a, torch, {k: (lambda t=t: [t.step(xm, ym) for _ in range(STEPS)]) for k, t in trio.items()})
    lines.append(_row(f"ModelBatchTrainer, M = {M}, B = {B}, T = {T} (skipped {sum(trio['sam'].skipped_steps())})", times))
    print(lines[-1], flush=True)
    lines.append("")
    return trio["sam"]


def launch_cost(a, torch, ops, dev, mbt, lines):
    """the ascent and the clipped tail alone, on the slabs the last step of `mbt` (M = 25, B = 32, T = 625) left in its workspace, and for
    one model on a workspace of its own"""
    spec, M = mbt.spec, mbt.M
    (B, T), P = mbt._last, mbt.spec.param_count
    ws, d = mbt._bufs[(B, T)]["ws"], spec.dims(B, T)
    opt = ops.opt_struct(max_norm=0.0)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3
    z = lambda *s: torch.zeros(s, device=dev)                                               # noqa: E731
    g, p, m, v, st, sst = z(M, P), mbt.params.clone(), z(M, P), z(M, P), ops.opt_state(P, M, dev), ops.sam_state(P, M, dev)
    tail = (C.byref(d), M, ws.data_ptr(), ops._nbytes(ws), g.data_ptr(), p.data_ptr(), m.data_ptr(), v.data_ptr(), C.byref(opt), 1, None,
            st.data_ptr(), ops._nbytes(st), ops.STREAM)
    ws1, lg1, g1, p1 = ops.new_workspace(spec, B, T, dev), z(B, spec.K), z(P), mbt.params[0].clone()
    xs, ys = 2.7 * torch.randn((B, T, 8), device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    ops.train_step_grads(spec, p1, xs, ws1, ys, lg1, g1)
    st1, sst1, m1, v1 = ops.opt_state(P, 1, dev), ops.sam_state(P, 1, dev), z(P), z(P)
    d1 = spec.dims(B, T)
    legs = {f"nsd_multi_grad_reduce_clip_adam, M = {M}": lambda: ops._call("nsd_multi_grad_reduce_clip_adam", dev, *tail),
            f"nsd_multi_sam_ascend, M = {M}": lambda: ops.multi_sam_ascend(spec, ws, B, T, g, p, ops.Sam(0.05), st, sst),
            "nsd_grad_reduce_clip_adam, one model": lambda: ops._call("nsd_grad_reduce_clip_adam", dev, C.byref(d1), ws1.data_ptr(), ops._nbytes(ws1),
                                                                      g1.data_ptr(), p1.data_ptr(), m1.data_ptr(), v1.data_ptr(), C.byref(opt), 1, None,
                                                                      st1.data_ptr(), ops._nbytes(st1), ops.STREAM),
            "nsd_sam_ascend, one model": lambda: ops.sam_ascend(spec, ws1, B, T, g1, p1, ops.Sam(0.05), st1, sst1),
            "nsd_sam_ascend_flat, n = P": lambda: ops.sam_ascend_flat(p1, g1, ops.Sam(0.05), st1, sst1)}
    times = {k: [] for k in legs}
    for r in range(a.warmup + a.reps):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t = timed(fn)
            if r >= a.warmup:
                times[name].append(t)
    lines += [f"## 2. The calls alone: GPU time between two HIP events around the one call (two launches each), microseconds; P = {P}", "",
              "| call | time |", "|---|---|"] + [f"| {k} | {_fmt(v)} |" for k, v in times.items()] + [""]
    print("\n".join(lines[-len(times) - 1:]), flush=True)


def cross_validation(a, lines):
    from nsd_amd import grid
    data = os.path.join(ROOT, "tests", "golden", "recorded_trials_filtered.npz")
    recipe = ["--data", data, "--npz-key", "x_filt", "--classes", "3", "--T", "625", "--epochs", str(a.epochs), "--batch", "32", "--lr", "0.001",
              "--dropout", "0.6", "--seed", "1", "--kfold", "5", "--kfold-seeds", "5", "--log-every", "100000", "--grid", f"sam_rho={RHOS}"]
    tmp = tempfile.mkdtemp()
    lines += ["## 3. 5 folds x 5 seeds on the recorded trials: outer-fold accuracy of the 25 models of each rho", "",
              f"Recipe (the README's): `python -m nsd_amd.grid {' '.join(recipe[2:])}` on `tests/golden/recorded_trials_filtered.npz`, plus the arm's "
              "options.  Mean +- sd over the 25 folds; per-seed means in brackets.  rho = 0 is the configuration without SAM of the same run.", "",
              "| arm | " + " | ".join(f"rho = {r}" for r in RHOS.split(",")) + " | whole command |", "|---|" + "---|" * (len(RHOS.split(",")) + 1)]

    def ms(v):
        seeds = ", ".join(f"{100 * statistics.mean(v[5 * i:5 * i + 5]):.1f}" for i in range(5))
        return f"{100 * statistics.mean(v):.1f} % +- {100 * statistics.stdev(v):.1f} % [{seeds}]"
    for name, extra in (("last iterate", []), ("--avg ema --avg-decay 0.99 (the averaged models are scored)", ["--avg", "ema", "--avg-decay", "0.99"])):
        log = os.path.join(tmp, f"{len(lines)}.jsonl")
        t0 = time.time()
        rc = grid.main(recipe + extra + ["--log-jsonl", log])
        assert rc == 0, rc
        recs = [json.loads(ln) for ln in open(log)]
        sums = sorted((r for r in recs if r.get("summary")), key=lambda r: r["config_index"])
        assert len(sums) == len(RHOS.split(",")) and all(len(s["acc_val_folds"]) == 25 for s in sums), len(sums)
        done = [r for r in recs if r.get("done")][0]
        lines.append(f"| {name} | " + " | ".join(ms(s["acc_val_folds"]) for s in sums) + f" | {time.time() - t0:.0f} s; best: {' '.join(done['best']['train_args'])} |")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam.md"))
    a = ap.parse_args()
    import torch
    import nsd_amd
    from nsd_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("sam_step: needs the MI355X (no GPU, no figures)")
    dev = torch.device("cuda:0")
    prop = torch.cuda.get_device_properties(dev)
    lines = ["# Sharpness-aware minimisation in the fused step: what the second pass and the ascent cost, and what they do to the accuracy", "",
             f"Machine: {prop.name} ({prop.multi_processor_count} CUs), torch {torch.__version__}.  Commit: {a.commit}.", "",
             f"Method: `python tools/sam_step.py --reps {a.reps} --epochs {a.epochs}` (its docstring describes the legs): medians (10th .. 90th "
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
