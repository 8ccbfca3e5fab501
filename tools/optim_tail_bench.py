"""Cost of the clipped / scheduled step tail (nsd_grad_reduce_clip_adam) on Trainer.step, and the gate that the options-off step is the
parent's.

    tools/build_base.sh <parent ref>                     # the parent's kernels as libnsd_hip_base.so (needs no GPU)
    python tools/optim_tail_bench.py [--runs 5] [--steps 200] [--out profiles/optim_tail.md]

Procedure (that of profiles/h48_step_loops.md): cfg2's shape (B = 256, T = 250) and cfg4's (B = 1024), Trainer.step trials/s, one fresh
process per run, the legs alternating inside one GPU visit -- parent library with options off, this library with options off, clip only,
clip + cosine -- five runs each, medians.  Gate: the options-off median must lie inside the parent's own min .. max.  One more process
times every launch of a cfg2 step through ops.set_launch_hook (HIP events around each C-ABI call, one synchronisation per step).
The driver itself never touches the GPU; each leg is a child process started with NSD_LIB naming its library."""
import argparse
import contextlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"cfg2": (256, 250), "cfg4": (1024, 250)}
LEGS = [("parent_off", "libnsd_hip_base.so", "off"), ("off", "libnsd_hip.so", "off"), ("clip", "libnsd_hip.so", "clip"),
        ("clip_cosine", "libnsd_hip.so", "clip_cosine")]


def _trainer(opts: str, dev):
    import nsd_amd
    from nsd_amd.trainer import Trainer
    kw = {}
    if opts != "off":
        kw["clip_grad_norm"] = 1.0
    if opts == "clip_cosine":
        kw["lr_schedule"] = nsd_amd.LrSchedule("cosine", warmup_steps=100, total_steps=100000, min_ratio=0.1)
    return Trainer(nsd_amd.EEG_LSTM().to(dev).train(), seed=0, **kw)


def _batch(B, T, dev):
    import torch
    g = torch.Generator().manual_seed(0)
    return (2.7 * torch.randn((B, T, 8), generator=g)).to(dev), torch.randint(0, 3, (B,), generator=g, dtype=torch.int32).to(dev)


def child(opts: str, steps: int, preheat: int) -> None:
    import torch
    sys.path.insert(0, ROOT)
    dev = torch.device("cuda:0")
    out = {}
    for name, (B, T) in SHAPES.items():
        tr, (x, y) = _trainer(opts, dev), _batch(B, T, dev)
        for _ in range(preheat):
            tr.step(x, y)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            tr.step(x, y)
        b.record()
        b.synchronize()
        out[name] = B * steps / (a.elapsed_time(b) * 1e-3)
    print("RESULT " + json.dumps(out), flush=True)


def child_launch_times(steps: int, preheat: int) -> None:
    import torch
    sys.path.insert(0, ROOT)
    from nsd_amd import ops
    dev = torch.device("cuda:0")
    B, T = SHAPES["cfg2"]
    out = {}
    for opts in ("off", "clip"):
        tr, (x, y) = _trainer(opts, dev), _batch(B, T, dev)
        for _ in range(preheat):
            tr.step(x, y)
        torch.cuda.synchronize()
        spans = []

        @contextlib.contextmanager
        def hook(name):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            yield
            b.record()
            spans.append((name, a, b))
        ops.set_launch_hook(hook)
        sums = {}
        for _ in range(steps):
            tr.step(x, y)
            torch.cuda.synchronize()
            for name, a, b in spans:
                sums.setdefault(name, []).append(a.elapsed_time(b) * 1e3)
            del spans[:]
        ops.set_launch_hook(None)
        out[opts] = {k: round(statistics.median(v), 2) for k, v in sums.items()}
    print("RESULT " + json.dumps(out), flush=True)


def _spawn(args, lib):
    env = dict(os.environ, NSD_LIB=lib)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise SystemExit(f"optim_tail_bench: a leg failed (rc {r.returncode}); nothing more is started\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--preheat", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child == "launch_times":
        return child_launch_times(50, 100)
    if args.child:
        return child(args.child, args.steps, args.preheat)
    have_parent = os.path.exists(os.path.join(ROOT, "neural-speech-decoding_amd", "libnsd_hip_base.so"))
    if not have_parent:
        raise SystemExit("optim_tail_bench: libnsd_hip_base.so is missing: tools/build_base.sh <parent ref> builds it")
    runs = {leg: {s: [] for s in SHAPES} for leg, _, _ in LEGS}
    for _ in range(args.runs):
        for leg, lib, opts in LEGS:
            res = _spawn(["--child", opts, "--steps", str(args.steps), "--preheat", str(args.preheat)], lib)
            for s in SHAPES:
                runs[leg][s].append(res[s])
            print(leg, {k: round(v) for k, v in res.items()}, flush=True)
    launches = _spawn(["--child", "launch_times"], "libnsd_hip.so")
    md = ["| shape | leg | runs (trials/s) | median | min .. max | vs options off |", "|---|---|---|---|---|---|"]
    gate = {}
    for s in SHAPES:
        off = statistics.median(runs["off"][s])
        for leg, _, _ in LEGS:
            v = runs[leg][s]
            med = statistics.median(v)
            md.append(f"| {s} | {leg} | {' '.join(str(round(t)) for t in v)} | {round(med)} | {round(min(v))} .. {round(max(v))} | {100 * (med / off - 1):+.2f} % |")
        pv = runs["parent_off"][s]
        gate[s] = min(pv) <= off <= max(pv)
        B, T = SHAPES[s]
        step_us = B / off * 1e6
        for leg in ("clip", "clip_cosine"):
            extra = B / statistics.median(runs[leg][s]) * 1e6 - step_us
            md.append(f"| {s} | {leg}: step time | | {step_us + extra:.1f} us | | {extra:+.2f} us of {step_us:.1f} us ({100 * extra / step_us:+.2f} %) |")
    md += ["", "Gate (options-off median inside the parent's min .. max): " + ", ".join(f"{s}: {'inside' if ok else 'OUTSIDE'}" for s, ok in gate.items()), "",
           "Per-launch medians of a cfg2 step, us (HIP events around each C-ABI call; nsd_grad_reduce_clip_adam spans its two kernels):", "",
           "```", json.dumps(launches, indent=1), "```", ""]
    text = "\n".join(md)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
