"""Latency of decoding live streams with an ensemble (nsd_multi_stream_step) against the route without it, written to
profiles/ensemble_stream.md.

    python tools/ensemble_stream_latency.py [--reps 300] [--warmup 30] [--commit <text>] [--out profiles/ensemble_stream.md]

Method: every figure is GPU time between two HIP events recorded around the call(s) on the current stream, after `--warmup` untimed
repetitions of the same shape, repeated `--reps` times; the table gives the median and the 10th / 90th percentile.  The legs of a point
alternate inside one repetition, in one process, on one GPU.  25-sample chunks with readout, M = 1, 5, 10, 32 models, B = 1 and 64
streams.  The legs of a point:
  one      one nsd_stream_step of the B streams (one model): what a call of the single-model path costs
  multi    one nsd_multi_stream_step of the M models, without mean_probs
  +mean    the same with mean_probs: the difference to `multi` is the second launch
  M calls  the only route without the model-batched entry: M nsd_stream_step calls enqueued back to back, then torch.mean over the
           stacked probabilities
  graph    nsd_prep_step + nsd_multi_stream_step (with mean_probs) captured once and replayed: one graph launch per chunk
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHUNK = 25
MODELS, STREAMS = (1, 5, 10, 32), (1, 64)


def _pct(v, q):
    s = sorted(v)
    return s[min(len(s) - 1, int(q * len(s)))]


def _fmt(v):
    return f"{statistics.median(v):7.1f} ({_pct(v, 0.1):.1f} .. {_pct(v, 0.9):.1f})"


def main():
    import torch
    import nsd_amd
    from nsd_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--commit", default="working tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_stream.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_stream_latency: needs the MI355X (no GPU, no figures)")
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    spec = ops.ModelSpec()
    K = spec.K
    prep = nsd_amd.CausalPrep.design(highpass=1.0, lowpass=40.0, zscore_seconds=2.0)
    g = torch.Generator().manual_seed(0)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3                       # microseconds

    rows, agree = [], 0.0
    for B in STREAMS:
        for M in MODELS:
            torch.manual_seed(M)
            params = torch.stack([nsd_amd.EEG_LSTM().to(dev).eval().flat_parameters().clone() for _ in range(M)]).contiguous()
            x = (2.7 * torch.randn((B, CHUNK, 8), generator=g)).to(dev)
            st_multi, st_graph = ops.multi_stream_state(spec, M, B, dev), ops.multi_stream_state(spec, M, B, dev)
            st_each = ops.multi_stream_state(spec, M, B, dev)          # the M separate calls: one model's part each
            st_one = ops.stream_state(spec, B, dev)
            ps = ops.prep_state(8, B, dev)
            lg, pr, mean = (torch.empty(s, device=dev) for s in ((M, B, K), (M, B, K), (B, K)))
            lg2, pr2, mean2 = (torch.empty(s, device=dev) for s in ((M, B, K), (M, B, K), (B, K)))
            lg1, pr1 = torch.empty((B, K), device=dev), torch.empty((B, K), device=dev)
            xin, xout = x.clone(), torch.empty_like(x)

            one = lambda: ops.stream_step(spec, params[0], x, st_one, logits=lg1, probs=pr1)
            multi = lambda: ops.multi_stream_step(spec, params, x, st_multi, want_mean=False, logits=lg, probs=pr)
            with_mean = lambda: ops.multi_stream_step(spec, params, x, st_multi, logits=lg, probs=pr, mean=mean)

            def calls():
                for m in range(M):
                    ops.stream_step(spec, params[m], x, st_each[m], logits=lg2[m], probs=pr2[m])
                torch.mean(pr2, 0, out=mean2)

            torch.cuda.synchronize(dev)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                ops.prep_step(xin, prep, ps, out=xout)
                ops.multi_stream_step(spec, params, xout, st_graph, logits=lg, probs=pr, mean=mean)
            t = {k: [] for k in ("one", "multi", "mean", "calls", "graph")}
            for rep in range(a.warmup + a.reps):
                got = dict(one=timed(one), multi=timed(multi), mean=timed(with_mean), calls=timed(calls), graph=timed(graph.replay))
                if rep >= a.warmup:
                    for k, v in got.items():
                        t[k].append(v)
            torch.cuda.synchronize(dev)
            # the two routes on one state history (fresh states, one chunk): the same probabilities up to the mean's rounding
            ops.stream_reset(spec, st_multi.view(M * B, -1)); ops.stream_reset(spec, st_each.view(M * B, -1))
            with_mean(); calls()
            torch.cuda.synchronize(dev)
            assert torch.equal(pr, pr2), "the model-batched step and the M separate calls differ"
            agree = max(agree, float((mean - mean2).abs().max()))
            G = min(B, max(1, cus // M))
            rows.append((M, B, G, -(-B // G), t))

    med = lambda v: statistics.median(v)
    lines = [
        "# Decoding live streams with an ensemble: nsd_multi_stream_step against M nsd_stream_step calls", "",
        f"Machine: {torch.cuda.get_device_name(dev)} ({cus} CUs), torch {torch.__version__}.  Commit: {a.commit}.", "",
        f"Method: `python tools/ensemble_stream_latency.py --reps {a.reps} --warmup {a.warmup}`.  GPU time between two HIP events around the "
        f"call(s), microseconds, median (10th .. 90th percentile) of {a.reps} repetitions after {a.warmup} untimed ones; the legs of a "
        f"point alternate inside each repetition, one process.  Reference shape (C = 8, H = 48, L = 2, K = 3), fp32, {CHUNK}-sample chunks "
        "with readout.  `one`: one nsd_stream_step of the B streams of one model.  `multi`: one nsd_multi_stream_step without mean_probs.  "
        "`+mean`: with mean_probs (a second small launch).  `M calls`: M nsd_stream_step calls back to back and torch.mean over the "
        "stacked probabilities -- the only route the parent commit has.  `graph`: nsd_prep_step + nsd_multi_stream_step (with "
        "mean_probs) as one replayed graph.  G: workgroups per model, min(B, max(1, CUs / M)); a model's workgroups walk "
        "ceil(B / G) streams each.  The member probabilities of the two routes are bitwise equal on the timed shapes; the means differ "
        f"by at most {agree:.1e} (torch.mean's summation order).", "",
        "| M | B | G | ceil(B/G) | one, us | multi, us | +mean, us | mean launch, us | M calls + torch.mean, us | graph (prep + step + mean), us | multi / one | M calls / +mean |",
        "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    slower = []
    for M, B, G, loops, t in rows:
        lines.append(f"| {M} | {B} | {G} | {loops} | {_fmt(t['one'])} | {_fmt(t['multi'])} | {_fmt(t['mean'])} | {med(t['mean']) - med(t['multi']):.1f} | "
                     f"{_fmt(t['calls'])} | {_fmt(t['graph'])} | {med(t['multi']) / med(t['one']):.2f} | {med(t['calls']) / med(t['mean']):.2f} |")
        if med(t["mean"]) > med(t["calls"]):
            slower.append((M, B))
    lines += ["", ("Points where the model-batched call (with mean_probs) is SLOWER than the M separate calls plus torch.mean: "
                   + ", ".join(f"M = {M}, B = {B}" for M, B in slower) + ".") if slower else
              "At no measured point is the model-batched call (with mean_probs) slower than the M separate calls plus torch.mean.", ""]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
