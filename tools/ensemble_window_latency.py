"""Latency of sliding-window decisions from an ensemble (nsd_multi_window_step) against one nsd_window_step and against the route
without it, written to profiles/ensemble_window.md.

    python tools/ensemble_window_latency.py [--reps 200] [--warmup 40] [--commit <text>] [--out profiles/ensemble_window.md]

Method: every figure is GPU time between two HIP events recorded around the call(s) on the current stream, after `--warmup` untimed
repetitions of the same shape (at least 25: one whole window of 625 samples, so that every phase is running), repeated `--reps` times;
the table gives the median and the 10th / 90th percentile.  The legs of a point alternate inside one repetition, in one process, on
one GPU, each on a state of its own that it advances by one chunk per repetition.  Reference shape, 25-sample chunks, window 625;
hop 625, 125 and 25 (R = 1, 5, 25 phases), M = 1, 5, 10 models, B = 1 and 8 streams.  The legs of a point:
  window   one nsd_window_step of the B streams of one model: what a call of the single-model path costs
  multi    one nsd_multi_window_step of the M models, without mean_probs
  +mean    the same with mean_probs: the difference to `multi` is the second launch
  M calls  the only route without the model-batched entry: M nsd_window_step calls enqueued back to back, then torch.mean over the
           stacked probabilities
  graph    nsd_prep_step + nsd_multi_window_step (with mean_probs) captured once and replayed: one graph launch per chunk
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHUNK, WINDOW = 25, 625
HOPS, MODELS, STREAMS = (625, 125, 25), (1, 5, 10), (1, 8)


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
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--commit", default="working tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_window.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_window_latency: needs the MI355X (no GPU, no figures)")
    if a.warmup * CHUNK < WINDOW:
        raise SystemExit(f"ensemble_window_latency: --warmup {a.warmup} chunks of {CHUNK} samples do not fill one window of {WINDOW}")
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
    for hop in HOPS:
        R, D = WINDOW // hop, ops.window_rows(CHUNK, WINDOW, hop)
        for B in STREAMS:
            for M in MODELS:
                torch.manual_seed(M)
                params = torch.stack([nsd_amd.EEG_LSTM().to(dev).eval().flat_parameters().clone() for _ in range(M)]).contiguous()
                x = (2.7 * torch.randn((B, CHUNK, 8), generator=g)).to(dev)
                st_multi, st_mean, st_graph, st_each = (ops.multi_window_state(spec, WINDOW, hop, M, B, dev) for _ in range(4))
                st_one = ops.window_state(spec, WINDOW, hop, B, dev)
                ps = ops.prep_state(8, B, dev)
                new = lambda: (torch.empty((M, B, D, K), device=dev), torch.empty((M, B, D, K), device=dev), torch.empty((B, D, K), device=dev),
                               torch.empty((M, B, D), dtype=torch.int64, device=dev), torch.empty((M, B), dtype=torch.int32, device=dev))
                o_multi, o_mean, o_graph, o_each = new(), new(), new(), new()
                o_one = (torch.empty((B, D, K), device=dev), torch.empty((B, D, K), device=dev),
                         torch.empty((B, D), dtype=torch.int64, device=dev), torch.empty((B,), dtype=torch.int32, device=dev))
                xin, xout = x.clone(), torch.empty_like(x)
                kw = dict(window=WINDOW, hop=hop)

                one = lambda: ops.window_step(spec, params[0], x, st_one, out=o_one, **kw)
                multi = lambda: ops.multi_window_step(spec, params, x, st_multi, want_mean=False, out=o_multi[:2] + (None,) + o_multi[3:], **kw)
                with_mean = lambda: ops.multi_window_step(spec, params, x, st_mean, out=o_mean, **kw)

                def calls():
                    for m in range(M):
                        ops.window_step(spec, params[m], x, st_each[m], out=(o_each[0][m], o_each[1][m], o_each[3][m], o_each[4][m]), **kw)
                    torch.mean(o_each[1], 0, out=o_each[2])

                torch.cuda.synchronize(dev)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    ops.prep_step(xin, prep, ps, out=xout)
                    ops.multi_window_step(spec, params, xout, st_graph, out=o_graph, **kw)
                t = {k: [] for k in ("one", "multi", "mean", "calls", "graph")}
                for rep in range(a.warmup + a.reps):
                    got = dict(one=timed(one), multi=timed(multi), mean=timed(with_mean), calls=timed(calls), graph=timed(graph.replay))
                    if rep >= a.warmup:
                        for k, v in got.items():
                            t[k].append(v)
                torch.cuda.synchronize(dev)
                # the two routes have seen the same chunks from the same reset: the same member outputs, bit for bit (NaN rows included)
                same = lambda u, v: torch.equal(u.view(torch.int32) if u.dtype == torch.float32 else u, v.view(torch.int32) if v.dtype == torch.float32 else v)
                assert all(same(o_mean[i], o_each[i]) for i in (0, 1, 3, 4)), "the model-batched step and the M separate calls differ"
                done = ~torch.isnan(o_each[2])
                if bool(done.any()):
                    agree = max(agree, float((o_mean[2][done] - o_each[2][done]).abs().max()))
                items = B * R
                G = min(items, max(1, cus // M))
                rows.append((hop, R, M, B, G, -(-items // G), t))

    med = lambda v: statistics.median(v)
    lines = [
        "# Sliding-window decisions from an ensemble: nsd_multi_window_step against nsd_window_step and against M calls of it", "",
        f"Machine: {torch.cuda.get_device_name(dev)} ({cus} CUs), torch {torch.__version__}.  Commit: {a.commit}.", "",
        f"Method: `python tools/ensemble_window_latency.py --reps {a.reps} --warmup {a.warmup}`.  GPU time between two HIP events around the "
        f"call(s), microseconds, median (10th .. 90th percentile) of {a.reps} repetitions after {a.warmup} untimed ones (more than one "
        f"window: every phase is running); the legs of a point alternate inside each repetition, one process, each leg on a state of "
        f"its own.  Reference shape (C = 8, H = 48, L = 2, K = 3), fp32, {CHUNK}-sample chunks, window {WINDOW}.  `window`: one "
        "nsd_window_step of the B streams of one model.  `multi`: one nsd_multi_window_step without mean_probs.  `+mean`: with mean_probs "
        "(a second small launch).  `M calls`: M nsd_window_step calls back to back and torch.mean over the stacked probabilities -- the "
        "only route the parent commit has.  `graph`: nsd_prep_step + nsd_multi_window_step (with mean_probs) as one replayed graph.  "
        "R = window / hop phases per stream; G: workgroups per model, min(B R, max(1, CUs / M)); a model's workgroups walk "
        "ceil(B R / G) (stream, phase) pairs each.  The member outputs of the two routes are bitwise equal on the timed shapes; the means "
        f"differ by at most {agree:.1e} (torch.mean's summation order).", "",
        "| hop | R | M | B | M B R | G | ceil(BR/G) | window, us | multi, us | +mean, us | mean launch, us | M calls + torch.mean, us | graph (prep + step + mean), us | multi / window | M calls / +mean | +mean slower than M calls? |",
        "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    slower = []
    for hop, R, M, B, G, loops, t in rows:
        slow = med(t["mean"]) > med(t["calls"])
        lines.append(f"| {hop} | {R} | {M} | {B} | {M * B * R} | {G} | {loops} | {_fmt(t['one'])} | {_fmt(t['multi'])} | {_fmt(t['mean'])} | "
                     f"{med(t['mean']) - med(t['multi']):.1f} | {_fmt(t['calls'])} | {_fmt(t['graph'])} | {med(t['multi']) / med(t['one']):.2f} | "
                     f"{med(t['calls']) / med(t['mean']):.2f} | {'YES' if slow else 'no'} |")
        if slow:
            slower.append((hop, M, B))
    lines += ["", ("Points where the model-batched call (with mean_probs) is SLOWER than the M separate calls plus torch.mean: "
                   + ", ".join(f"hop = {h}, M = {M}, B = {B}" for h, M, B in slower) + ".") if slower else
              "At no measured point is the model-batched call (with mean_probs) slower than the M separate calls plus torch.mean.", ""]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
