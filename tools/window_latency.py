"""Latency of sliding-window decisions (nsd_window_step) against one nsd_stream_step and against the host emulation that was the only
route before it, written to profiles/sliding_window.md.

    python tools/window_latency.py [--reps 300] [--warmup 30] [--commit <text>] [--out profiles/sliding_window.md]

Method: every figure is GPU time between two HIP events recorded around the call(s) on the current stream, after `--warmup` untimed
repetitions, repeated `--reps` times over CONSECUTIVE chunks of a running stream; the table gives the median, the 10th / 90th percentile
and the mean (a chunk that holds a window boundary is one in hop / 25: the median does not see it for the longer hops, the mean does).
The legs of a point alternate inside one repetition, in one process, on one GPU.  25-sample chunks, window = 625 samples (5 s at
125 Hz), hop = 625, 125, 25 (R = 1, 5, 25 phases), B = 1, 8, 64 streams.  Every stream is advanced by window + 10 samples before the
timing, so that all phases run and the hop boundaries fall INSIDE chunks (10 samples in), not between them.  The legs:
  one      one nsd_stream_step of the chunk on B slots, with readout: what a call of the cued path costs
  window   one nsd_window_step of the chunk
  emul     the host emulation: R nsd_stream_step slots per stream, the chunk replicated R times on the device and split on the host at
           the hop boundary; per piece one nsd_stream_step over all B * R slots (with readout when the piece ends a window), then one
           nsd_stream_reset of the phase that ended
  graph    nsd_prep_step + nsd_window_step captured once and replayed: one graph launch per chunk
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
    return f"{statistics.median(v):7.1f} ({_pct(v, 0.1):.1f} .. {_pct(v, 0.9):.1f}; mean {statistics.fmean(v):.1f})"


class Emulation:
    """R slots per stream (slot b * R + r: phase r of stream b), the bookkeeping on the host"""

    def __init__(self, ops, spec, params, B, W, Hp, dev):
        import torch
        self.ops, self.spec, self.params, self.B, self.W, self.Hp, self.R = ops, spec, params, B, W, Hp, W // Hp
        self.state = ops.stream_state(spec, B * self.R, dev)
        self.n = 0
        self.lg, self.pr = torch.empty((B * self.R, spec.K), device=dev), torch.empty((B * self.R, spec.K), device=dev)
        self.phase_slots = [(torch.arange(B, dtype=torch.int32, device=dev) * self.R + r).contiguous() for r in range(self.R)]
        self.decisions = []

    def push(self, x, keep=False):
        """x [B, n, C].  Phases that have not begun yet (the stream's first window) run on samples they should not see: they are reset
        when they begin, so their first windows are right; only the steady state is timed."""
        ops, Hp, R = self.ops, self.Hp, self.R
        xr = x.repeat_interleave(R, 0)
        t, T = 0, int(x.shape[1])
        while t < T:
            nxt = (self.n // Hp + 1) * Hp                      # the next hop boundary of the stream
            m = min(T - t, nxt - self.n)
            ends = self.n + m == nxt
            piece = xr if (t == 0 and m == T) else xr[:, t:t + m].contiguous()
            ops.stream_step(self.spec, self.params, piece, self.state, read=ends, logits=self.lg, probs=self.pr)
            self.n += m
            t += m
            if ends:
                r = (nxt // Hp) % R                            # the phase whose window ends here also begins its next one here
                if keep and nxt >= self.W:
                    self.decisions.append((nxt, self.pr.view(self.B, R, -1)[:, r].clone()))
                ops.stream_reset(self.spec, self.state, self.phase_slots[r])


def main():
    import torch
    import nsd_amd
    from nsd_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--commit", default="working tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sliding_window.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("window_latency: needs the MI355X (no GPU, no figures)")
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    spec = ops.ModelSpec()
    K = spec.K
    prep = nsd_amd.CausalPrep.design(highpass=1.0, lowpass=40.0, zscore_seconds=2.0)
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
        R = WINDOW // Hp
        D = ops.window_rows(CHUNK, WINDOW, Hp)
        for B in STREAMS:
            lead = (2.7 * torch.randn((B, WINDOW + LEAD, 8), generator=g)).to(dev)
            x = (2.7 * torch.randn((B, CHUNK, 8), generator=g)).to(dev)
            # the two routes on one stream: the same decisions, bit for bit (two windows' worth of boundaries)
            ws, em = ops.window_state(spec, WINDOW, Hp, B, dev), Emulation(ops, spec, params, B, WINDOW, Hp, dev)
            both, got = torch.cat([lead] + [x] * (2 * Hp // CHUNK + 1), 1), []
            for t0 in range(0, both.shape[1], CHUNK):
                piece = both[:, t0:t0 + CHUNK].contiguous()
                _, pr, ends, counts = ops.window_step(spec, params, piece, ws, window=WINDOW, hop=Hp)
                em.push(piece, keep=True)
                for i in range(int(counts[0])):
                    got.append((int(ends[0, i]), pr[:, i].clone()))
            assert [e for e, _ in got] == [e for e, _ in em.decisions] and len(got) >= 2, (Hp, B)
            assert all(torch.equal(p, q) for (_, p), (_, q) in zip(got, em.decisions)), "nsd_window_step and the emulation differ"

            ws, wg = ops.window_state(spec, WINDOW, Hp, B, dev), ops.window_state(spec, WINDOW, Hp, B, dev)
            em = Emulation(ops, spec, params, B, WINDOW, Hp, dev)
            st_one, ps = ops.stream_state(spec, B, dev), ops.prep_state(8, B, dev)
            lg1, pr1 = torch.empty((B, K), device=dev), torch.empty((B, K), device=dev)
            out = (torch.empty((B, D, K), device=dev), torch.empty((B, D, K), device=dev),
                   torch.empty((B, D), dtype=torch.int64, device=dev), torch.empty((B,), dtype=torch.int32, device=dev))
            gout = tuple(torch.empty_like(o) for o in out)
            xin, xout = x.clone(), torch.empty_like(x)
            for state in (ws, wg):
                ops.window_step(spec, params, lead, state, window=WINDOW, hop=Hp)
            em.push(lead)

            one = lambda: ops.stream_step(spec, params, x, st_one, logits=lg1, probs=pr1)
            window = lambda: ops.window_step(spec, params, x, ws, window=WINDOW, hop=Hp, out=out)
            emul = lambda: em.push(x)
            torch.cuda.synchronize(dev)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                ops.prep_step(xin, prep, ps, out=xout)
                ops.window_step(spec, params, xout, wg, window=WINDOW, hop=Hp, out=gout)
            t = {k: [] for k in ("one", "window", "emul", "graph")}
            for rep in range(a.warmup + a.reps):
                got = dict(one=timed(one), window=timed(window), emul=timed(emul), graph=timed(graph.replay))
                if rep >= a.warmup:
                    for k, v in got.items():
                        t[k].append(v)
            torch.cuda.synchronize(dev)
            rows.append((Hp, R, B, t))

    mean = statistics.fmean
    lines = [
        "# Sliding-window decisions: nsd_window_step against one nsd_stream_step and against the host emulation", "",
        f"Machine: {torch.cuda.get_device_name(dev)} ({cus} CUs), torch {torch.__version__}.  Commit: {a.commit}.", "",
        f"Method: `python tools/window_latency.py --reps {a.reps} --warmup {a.warmup}`.  GPU time between two HIP events around the call(s), "
        f"microseconds, median (10th .. 90th percentile; mean) of {a.reps} consecutive chunks of a running stream after {a.warmup} untimed "
        f"ones; the legs of a point alternate inside each repetition, one process.  Reference shape (C = 8, H = 48, L = 2, K = 3), fp32, "
        f"{CHUNK}-sample chunks, window = {WINDOW} samples; every stream is {WINDOW + LEAD} samples in when the timing begins, so all "
        f"phases run and a hop boundary falls {LEAD} samples into a chunk, once every hop / {CHUNK} chunks.  `one`: one nsd_stream_step "
        "of the chunk on B slots with readout.  `window`: one nsd_window_step.  `emul`: the host emulation (R nsd_stream_step slots per "
        "stream, the chunk replicated R times, split at the hop boundary on the host; per piece one nsd_stream_step over B * R slots and, "
        "at a boundary, one nsd_stream_reset).  `graph`: nsd_prep_step + nsd_window_step as one replayed graph.  The decisions of "
        "`window` and `emul` are bitwise equal on every timed shape (checked over two windows' worth of boundaries before the timing).", "",
        "| hop | R | B | B*R | passes ceil(B*R / CUs) | one, us | window, us | emul, us | graph (prep + window), us | window / one (medians) | emul / window (means) |",
        "|---|---|---|---|---|---|---|---|---|---|---|"]
    for Hp, R, B, t in rows:
        lines.append(f"| {Hp} | {R} | {B} | {B * R} | {-(-B * R // cus)} | {_fmt(t['one'])} | {_fmt(t['window'])} | {_fmt(t['emul'])} | {_fmt(t['graph'])} | "
                     f"{statistics.median(t['window']) / statistics.median(t['one']):.2f} | {mean(t['emul']) / mean(t['window']):.2f} |")
    lines.append("")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
