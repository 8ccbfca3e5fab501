"""What the causal front end (nsd_prep_step) costs, written to profiles/causal_prep.md.

    python tools/prep_latency.py [--reps 300] [--warmup 30] [--commit <text>] [--out profiles/causal_prep.md]

Method: every figure is GPU time between two HIP events recorded around the call(s) on the current stream, after `--warmup` untimed
repetitions, repeated `--reps` times; the tables give the median and the 10th / 90th percentile.  The legs of a comparison alternate
inside one repetition.  The two parts run one after the other as child processes of their own, each under `timeout`; a part that fails
ends the run.
  window   nsd_prep_step in window mode (baseline, 1-40 Hz band-pass, 50 Hz notch, running z-score: three sections) at the training
           shapes, beside the nsd_zscore_fwd launch it stands beside in the step recipe and the Trainer.step of a model without a front
           end at that shape -- both untouched by the front end, so they are the parent commit's
  stream   25-sample chunks with readout, B = 1 and B = 64: nsd_stream_step alone (the parent's), nsd_prep_step + nsd_stream_step
           enqueued eagerly, and the pair as one replayed graph
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((256, 250), (64, 625))
CHUNK = 25


def _pct(v, q):
    s = sorted(v)
    return s[min(len(s) - 1, int(q * len(s)))]


def _fmt(v):
    return f"{statistics.median(v):8.1f} ({_pct(v, 0.1):.1f} .. {_pct(v, 0.9):.1f})"


def _setup():
    import torch
    import nsd_amd
    if not torch.cuda.is_available():
        raise SystemExit("prep_latency: needs the MI355X (no GPU, no figures)")
    dev = torch.device("cuda:0")
    prep = nsd_amd.CausalPrep.design(highpass=1.0, lowpass=40.0, notch=50.0, zscore_seconds=2.0, var0=400.0)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3                       # microseconds

    def raw(B, T, seed):
        g = torch.Generator().manual_seed(seed)
        return (20.0 * torch.randn((B, T, 8), generator=g) + 5000.0 * (2 * torch.rand((B, 1, 8), generator=g) - 1)).to(dev)
    return torch, nsd_amd, dev, prep, timed, raw


def part_window(a):
    torch, nsd_amd, dev, prep, timed, raw = _setup()
    from nsd_amd import ops
    from nsd_amd.trainer import Trainer
    out = {"machine": f"{torch.cuda.get_device_name(dev)} ({torch.cuda.get_device_properties(dev).multi_processor_count} CUs), torch {torch.__version__}"}
    for B, T in SHAPES:
        x = raw(B, T, 1)
        y = torch.randint(0, 3, (B,), dtype=torch.int32).to(dev)
        yp, yz = torch.empty_like(x), torch.empty_like(x)
        torch.manual_seed(0)
        plain = Trainer(nsd_amd.EEG_LSTM().to(dev).train(), lr=1e-3, seed=1)
        torch.manual_seed(0)
        front = Trainer(nsd_amd.EEG_LSTM(prep=prep).to(dev).train(), lr=1e-3, seed=1)
        xs = ops.prep_step(x, prep)                             # the model without a front end trains on the same windows
        legs = {"prep": lambda: ops.prep_step(x, prep, out=yp), "zscore": lambda: ops.zscore(x, out=yz),
                "step": lambda: plain.step(xs, y), "step_prep": lambda: front.step(x, y)}
        res = {k: [] for k in legs}
        for rep in range(a.warmup + a.reps):
            for k, fn in legs.items():
                t = timed(fn)
                if rep >= a.warmup:
                    res[k].append(t)
        out[f"{B}x{T}"] = res
    return out


def part_stream(a):
    torch, nsd_amd, dev, prep, timed, raw = _setup()
    from nsd_amd import ops
    model = nsd_amd.EEG_LSTM().to(dev).eval()
    spec, flat = model.spec, model.flat_parameters()
    out = {}
    for B in (1, 64):
        x = raw(B, CHUNK, 2)
        xp = torch.empty_like(x)
        ms, ps = ops.stream_state(spec, B, dev), ops.prep_state(8, B, dev)
        lg, pr = torch.empty((B, 3), device=dev), torch.empty((B, 3), device=dev)
        alone = lambda: ops.stream_step(spec, flat, x, ms, logits=lg, probs=pr)

        def pair():
            ops.prep_step(x, prep, ps, out=xp)
            ops.stream_step(spec, flat, xp, ms, logits=lg, probs=pr)
        pair(); alone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            pair()
        legs = {"step": alone, "prep": lambda: ops.prep_step(x, prep, ps, out=xp), "eager": pair, "graph": graph.replay}
        res = {k: [] for k in legs}
        for rep in range(a.warmup + a.reps):
            if rep % 50 == 0:                                   # (the running states stay far from overflow either way)
                ops.stream_reset(spec, ms); ops.prep_reset(8, ps)
            for k, fn in legs.items():
                t = timed(fn)
                if rep >= a.warmup:
                    res[k].append(t)
        out[str(B)] = res
    return out


def report(a, win, stream):
    med = statistics.median
    lines = ["# Causal front end: what nsd_prep_step costs", "",
             f"Machine: {win['machine']}.  Commit: {a.commit}.", "",
             f"Method: `python tools/prep_latency.py --reps {a.reps} --warmup {a.warmup}`.  GPU time between two HIP events around the "
             f"call(s), microseconds, median (10th .. 90th percentile) of {a.reps} repetitions after {a.warmup} untimed ones; the legs of a "
             "comparison alternate inside each repetition.  Front end: baseline, 1-40 Hz band-pass + 50 Hz notch (three sections), running "
             "z-score; C = 8.  nsd_zscore_fwd, nsd_stream_step and the Trainer.step of a model without a front end are not touched by "
             "this change: they are the parent commit's.", "",
             "## Window mode, at the training shapes", "",
             "| B x T | nsd_prep_step, us | nsd_zscore_fwd, us | Trainer.step without front end, us | with front end, us | nsd_prep_step / Trainer.step |",
             "|---|---|---|---|---|---|"]
    for B, T in SHAPES:
        r = win[f"{B}x{T}"]
        lines.append(f"| {B} x {T} | {_fmt(r['prep'])} | {_fmt(r['zscore'])} | {_fmt(r['step'])} | {_fmt(r['step_prep'])} | "
                     f"{100 * med(r['prep']) / med(r['step']):.1f} % |")
    per = {f"{B}x{T}": med(win[f"{B}x{T}"]["prep"]) / T for B, T in SHAPES}
    lines += ["", "One lane per (trial, channel), serial in T: " + ", ".join(f"{v:.3f} us per step at {k}" for k, v in per.items()) + ".", "",
              f"## Stream mode, {CHUNK}-sample chunks with readout", "",
              "| streams | nsd_stream_step alone, us | nsd_prep_step alone, us | prep + step, eager, us | prep + step, one replayed graph, us |",
              "|---|---|---|---|---|"]
    for B in ("1", "64"):
        r = stream[B]
        lines.append(f"| {B} | {_fmt(r['step'])} | {_fmt(r['prep'])} | {_fmt(r['eager'])} | {_fmt(r['graph'])} |")
    lines.append("")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--commit", default="working tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "causal_prep.md"))
    ap.add_argument("--part", choices=("window", "stream"), default=None, help="internal: run one part and print its figures as JSON")
    ap.add_argument("--part-timeout", type=int, default=240, help="seconds a part may take")
    a = ap.parse_args()
    if a.part:
        print("PREP_LATENCY_JSON " + json.dumps({"window": part_window, "stream": part_stream}[a.part](a)))
        return
    got = {}
    for part in ("window", "stream"):
        cmd = ["timeout", "-k", "10", str(a.part_timeout), sys.executable, os.path.abspath(__file__), "--part", part,
               "--reps", str(a.reps), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"prep_latency: part `{part}` ended with status {r.returncode}; nothing further is started")
        got[part] = json.loads([l for l in r.stdout.splitlines() if l.startswith("PREP_LATENCY_JSON ")][-1].split(" ", 1)[1])
    report(a, got["window"], got["stream"])


if __name__ == "__main__":
    main()
