"""Cost of the signal-quality gate's two launches per chunk of a sliding decoder (nsd_gate_step in front of nsd_prep_step, nsd_gate_apply
behind it), eager and as one replayed graph, written as a table for profiles/signal_gate.md.

    python tools/gate_latency.py [--reps 300] [--warmup 30] [--commit <text>] [--out profiles/signal_gate_latency.md]

Method (tools/window_latency.py's): every figure is GPU time between two HIP events recorded around the call(s) on the current stream,
after `--warmup` untimed repetitions, repeated `--reps` times over CONSECUTIVE chunks of running streams; the table gives the median,
the 10th / 90th percentile and the mean.  The legs of a point alternate inside one repetition, in one process, on one GPU, each on
streams of its own that are window + 10 samples in.  25-sample chunks, window = 625 samples, hop = 625, 125, 25, B = 1, 8, 64 streams:
the sliding decoder's configuration of profiles/sliding_window.md.  The legs:
  plain        nsd_prep_step + nsd_window_step, enqueued eagerly: the chunk of a decoder without a gate (launch for launch the chunk
               before the gate existed)
  gated        nsd_gate_step + nsd_prep_step + nsd_gate_apply + nsd_window_step, enqueued eagerly
  plain graph  the plain pair captured once and replayed
  gated graph  the four calls captured once and replayed
  gate, apply  nsd_gate_step and nsd_gate_apply alone, one launch each
The plain legs are run twice per repetition (plain, plain'): their difference is the spread a difference of legs has to beat.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHUNK, WINDOW, LEAD = 25, 625, 10
HOPS, STREAMS = (625, 125, 25), (1, 8, 64)


def _pct(v, q):
    s = sorted(v)
    return s[min(len(s) - 1, int(q * len(s)))]


def _fmt(v):
    return f"{statistics.median(v):6.1f} ({_pct(v, 0.1):.1f} .. {_pct(v, 0.9):.1f}; mean {statistics.fmean(v):.1f})"


def main():
    import torch
    import nsd_amd
    from nsd_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--commit", default="working tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "signal_gate_latency.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gate_latency: needs the MI355X (no GPU, no figures)")
    dev = torch.device("cuda:0")
    spec = ops.ModelSpec()
    K = spec.K
    prep = nsd_amd.CausalPrep.design(highpass=1.0, lowpass=40.0, zscore_seconds=2.0)
    gate = nsd_amd.SignalGate.design(rail=1000.0, jump=80.0, flat_seconds=0.1, pp=100.0, hold_seconds=0.1, max_bad_channels=2)
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(1)
    params = nsd_amd.EEG_LSTM().to(dev).eval().flat_parameters().clone()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3                       # microseconds

    rows = []
    for Hp in HOPS:
        D = ops.window_rows(CHUNK, WINDOW, Hp)
        for B in STREAMS:
            lead = (2.7 * torch.randn((B, WINDOW + LEAD, 8), generator=g)).to(dev)
            x = (2.7 * torch.randn((B, CHUNK, 8), generator=g)).to(dev)

            class Leg:
                """streams of a leg's own, window + 10 samples in: window, prep and gate state, and the buffers of a chunk"""

                def __init__(self, gated):
                    self.gated = gated
                    self.ws, self.ps = ops.window_state(spec, WINDOW, Hp, B, dev), ops.prep_state(8, B, dev)
                    self.gs = ops.gate_state(8, B, dev) if gated else None
                    self.y, self.v = torch.empty_like(x), torch.empty_like(x)
                    self.m = torch.empty((B, CHUNK), dtype=torch.int32, device=dev)
                    self.out = (torch.empty((B, D, K), device=dev), torch.empty((B, D, K), device=dev),
                                torch.empty((B, D), dtype=torch.int64, device=dev), torch.empty((B,), dtype=torch.int32, device=dev))
                    v = lead
                    if gated:
                        v, m = ops.gate_step(v, gate, self.gs)
                    v = ops.prep_step(v, prep, self.ps)
                    if gated:
                        ops.gate_apply(v, gate, m, out=v)
                    ops.window_step(spec, params, v, self.ws, window=WINDOW, hop=Hp)

                def chunk(self):
                    v = x
                    if self.gated:
                        v, _ = ops.gate_step(v, gate, self.gs, out=self.y, mask=self.m)
                    v = ops.prep_step(v, prep, self.ps, out=self.v)
                    if self.gated:
                        ops.gate_apply(v, gate, self.m, out=v)
                    ops.window_step(spec, params, v, self.ws, window=WINDOW, hop=Hp, out=self.out)

                def graph(self):
                    torch.cuda.synchronize(dev)
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        self.chunk()
                    return graph

            legs = dict(plain=Leg(False), plain2=Leg(False), gated=Leg(True))
            graphs = dict(plain_graph=Leg(False).graph(), plain2_graph=Leg(False).graph(), gated_graph=Leg(True).graph())
            alone = Leg(True)
            calls = {k: leg.chunk for k, leg in legs.items()}
            calls.update({k: gr.replay for k, gr in graphs.items()})
            calls["gate"] = lambda: ops.gate_step(x, gate, alone.gs, out=alone.y, mask=alone.m)
            calls["apply"] = lambda: ops.gate_apply(alone.y, gate, alone.m, out=alone.v)
            t = {k: [] for k in calls}
            for rep in range(a.warmup + a.reps):
                got = {k: timed(fn) for k, fn in calls.items()}
                if rep >= a.warmup:
                    for k, v in got.items():
                        t[k].append(v)
            torch.cuda.synchronize(dev)
            rows.append((Hp, B, t))

    med = statistics.median
    lines = [
        f"Machine: {torch.cuda.get_device_name(dev)}, torch {torch.__version__}.  Commit: {a.commit}.", "",
        f"Method: `python tools/gate_latency.py --reps {a.reps} --warmup {a.warmup}`.  GPU time between two HIP events around the call(s), "
        f"microseconds, median (10th .. 90th percentile; mean) of {a.reps} consecutive chunks after {a.warmup} untimed ones; the legs of a "
        f"point alternate inside each repetition, one process, each leg on streams of its own that are {WINDOW + LEAD} samples in.  "
        f"Reference shape (C = 8, H = 48, L = 2, K = 3), fp32, {CHUNK}-sample chunks, window = {WINDOW} samples.  `plain`: nsd_prep_step + "
        "nsd_window_step (the chunk of a decoder without a gate); `gated`: nsd_gate_step + nsd_prep_step + nsd_gate_apply + "
        "nsd_window_step; `graph`: the same calls captured once and replayed; `gate`, `apply`: the two new launches alone.  "
        "`spread`: |median(plain) - median(plain')| of two identical plain legs in the same repetitions (eager / graph).", "",
        "| hop | B | plain, us | gated, us | gated - plain (medians) | plain graph, us | gated graph, us | graph: gated - plain | spread eager / graph | gate alone, us | apply alone, us |",
        "|---|---|---|---|---|---|---|---|---|---|---|"]
    for Hp, B, t in rows:
        lines.append(f"| {Hp} | {B} | {_fmt(t['plain'])} | {_fmt(t['gated'])} | {med(t['gated']) - med(t['plain']):+.1f} | {_fmt(t['plain_graph'])} | "
                     f"{_fmt(t['gated_graph'])} | {med(t['gated_graph']) - med(t['plain_graph']):+.1f} | "
                     f"{abs(med(t['plain']) - med(t['plain2'])):.1f} / {abs(med(t['plain_graph']) - med(t['plain2_graph'])):.1f} | "
                     f"{_fmt(t['gate'])} | {_fmt(t['apply'])} |")
    lines.append("")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
