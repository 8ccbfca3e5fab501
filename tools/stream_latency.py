"""Latency of resumable decoding (nsd_stream_step) against the one-shot nsd_infer, written to profiles/stream_decode.md.

    python tools/stream_latency.py [--reps 300] [--warmup 30] [--commit <text>] [--out profiles/stream_decode.md]

Method: every figure is GPU time between two HIP events recorded around the call(s) on the current stream, after `--warmup` untimed
repetitions of the same shape, repeated `--reps` times; the table gives the median and the 10th / 90th percentile.  The legs of a
comparison alternate inside one repetition, in one process, on one GPU.  nsd_infer is not touched by the resumable path (its own
source files, one new object in the library), so the one-shot leg is the parent commit's kernel.
  (a) decision latency   B = 1, T = 625 in 25-sample chunks: the LAST nsd_stream_step, with readout (the 24 before it have run while
                         the samples arrived), against nsd_infer on the whole window
  (b) cost of cutting    the 25 chunk calls' GPU times summed, and the 25 calls enqueued back to back under one event pair, against it
  (c) many streams       64 and 256 streams, 25-sample chunks: microseconds per call, with readout and advance-only
  (d) the drain          B = 1 advance-only calls of 25 / 50 / 100 / 200 samples: the slope is the cost of a step; a call runs T + 3
                         macro steps, the 3 that drain the skew between the roles cost 3 slopes; the intercept is launch, state and
                         weight load
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
T_WIN, CHUNK = 625, 25


def _pct(v, q):
    s = sorted(v)
    return s[min(len(s) - 1, int(q * len(s)))]


def _fmt(v):
    return f"{statistics.median(v):8.1f} ({_pct(v, 0.1):.1f} .. {_pct(v, 0.9):.1f})"


def main():
    import torch
    import nsd_amd
    from nsd_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--commit", default="working tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_decode.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_latency: needs the MI355X (no GPU, no figures)")
    dev = torch.device("cuda:0")
    model = nsd_amd.EEG_LSTM().to(dev).eval()
    spec, flat = model.spec, model.flat_parameters()
    g = torch.Generator().manual_seed(0)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3                       # microseconds

    # ---- (a), (b): one stream, the reference window ----
    x = (2.7 * torch.randn((1, T_WIN, 8), generator=g)).to(dev)
    chunks = [x[:, t:t + CHUNK].contiguous() for t in range(0, T_WIN, CHUNK)]
    state = ops.stream_state(spec, 1, dev)
    lg, pr = torch.empty((1, 3), device=dev), torch.empty((1, 3), device=dev)
    lg1, pr1 = torch.empty((1, 3), device=dev), torch.empty((1, 3), device=dev)
    nscr = ops.stream_state_bytes(spec, 1) + T_WIN * 48 * 4 + 1024
    scratch = torch.empty(nscr // 4, device=dev)
    one_shot = lambda: ops.infer(spec, flat, x, logits=lg1, probs=pr1, scratch=scratch)

    def chunk_call(i):
        last = i == len(chunks) - 1
        return lambda: ops.stream_step(spec, flat, chunks[i], state, read=last, logits=lg if last else None, probs=pr if last else None)

    last_us, sum_us, b2b_us, shot_us = [], [], [], []
    for rep in range(a.warmup + a.reps):
        ops.stream_reset(spec, state)
        per = [timed(chunk_call(i)) for i in range(len(chunks))]
        shot = timed(one_shot)
        ops.stream_reset(spec, state)
        b2b = timed(lambda: [chunk_call(i)() for i in range(len(chunks))])
        if rep >= a.warmup:
            last_us.append(per[-1]); sum_us.append(sum(per)); b2b_us.append(b2b); shot_us.append(shot)
    torch.cuda.synchronize()
    agree = float((pr - pr1).abs().max())

    # ---- (c): many streams ----
    many = {}
    for S in (64, 256):
        xs = (2.7 * torch.randn((S, CHUNK, 8), generator=g)).to(dev)
        st = ops.stream_state(spec, S, dev)
        lS, pS = torch.empty((S, 3), device=dev), torch.empty((S, 3), device=dev)
        rd, adv = [], []
        for rep in range(a.warmup + a.reps):
            t_r = timed(lambda: ops.stream_step(spec, flat, xs, st, logits=lS, probs=pS))
            t_a = timed(lambda: ops.stream_step(spec, flat, xs, st, read=False))
            if rep >= a.warmup:
                rd.append(t_r); adv.append(t_a)
        many[S] = (rd, adv)

    # ---- (d): the drain ----
    lens, by_len = (25, 50, 100, 200), {}
    xl = {n: (2.7 * torch.randn((1, n, 8), generator=g)).to(dev) for n in lens}
    for rep in range(a.warmup + a.reps):
        for n in lens:
            t = timed(lambda: ops.stream_step(spec, flat, xl[n], state, read=False))
            if rep >= a.warmup:
                by_len.setdefault(n, []).append(t)
    med = {n: statistics.median(v) for n, v in by_len.items()}
    mx, my = statistics.mean(lens), statistics.mean(med.values())
    slope = sum((n - mx) * (med[n] - my) for n in lens) / sum((n - mx) ** 2 for n in lens)
    icpt = my - slope * mx

    m_last, m_shot, m_sum, m_b2b = (statistics.median(v) for v in (last_us, shot_us, sum_us, b2b_us))
    verdict = (f"The last chunk's call is {m_shot / m_last:.1f}x shorter than the one-shot call: the condition (a) < one-shot holds."
               if m_last < m_shot else
               "The last chunk's call is NOT shorter than the one-shot call on this machine in this run: the fixed cost of a call "
               f"(intercept of (d): {icpt:.1f} us) exceeds what {T_WIN - CHUNK} saved steps are worth.")
    lines = [
        "# Resumable decoding: latency of nsd_stream_step against the one-shot nsd_infer", "",
        f"Machine: {torch.cuda.get_device_name(dev)} ({torch.cuda.get_device_properties(dev).multi_processor_count} CUs), torch {torch.__version__}.  "
        f"Commit: {a.commit}.", "",
        f"Method: `python tools/stream_latency.py --reps {a.reps} --warmup {a.warmup}`.  GPU time between two HIP events around the "
        f"call(s), microseconds, median (10th .. 90th percentile) of {a.reps} repetitions after {a.warmup} untimed ones; the legs of a "
        "comparison alternate inside each repetition, one process.  Reference model (C = 8, H = 48, L = 2, K = 3), fp32.  nsd_infer is "
        "the parent commit's kernel (its sources are not touched).  The probabilities of the two routes agree within "
        f"{agree:.1e} on the timed window.", "",
        f"## (a) Decision latency, B = 1, T = {T_WIN}, {CHUNK}-sample chunks", "",
        "| call | GPU time, us |", "|---|---|",
        f"| last nsd_stream_step ({CHUNK} samples, readout) | {_fmt(last_us)} |",
        f"| nsd_infer on the whole window ({T_WIN} samples) | {_fmt(shot_us)} |", "",
        verdict + f"  Expectation was about {CHUNK}/{T_WIN} of the one-shot time plus launch and weight load: "
        f"{CHUNK / T_WIN * m_shot:.1f} us + the intercept of (d) = {CHUNK / T_WIN * m_shot + icpt:.1f} us.", "",
        "## (b) Cost of cutting", "",
        "| route | GPU time, us |", "|---|---|",
        f"| {T_WIN // CHUNK} chunk calls, each timed alone, summed | {_fmt(sum_us)} |",
        f"| {T_WIN // CHUNK} chunk calls enqueued back to back, one event pair | {_fmt(b2b_us)} |",
        f"| one nsd_infer | {_fmt(shot_us)} |", "",
        f"Cutting the window into {T_WIN // CHUNK} calls costs {m_sum / m_shot:.2f}x the one-shot GPU time summed ({m_b2b / m_shot:.2f}x "
        "back to back, launch gaps included) -- spent while the samples arrive, not after the last one.", "",
        f"## (c) Many streams, {CHUNK}-sample chunks, one launch", "",
        "| streams | with readout, us per call | advance only, us per call | us per stream (readout) |", "|---|---|---|---|"]
    for S, (rd, adv) in many.items():
        lines.append(f"| {S} | {_fmt(rd)} | {_fmt(adv)} | {statistics.median(rd) / S:.2f} |")
    lines += ["", "## (d) The drain", "",
              "| samples per call (B = 1, advance only) | GPU time, us |", "|---|---|"]
    lines += [f"| {n} | {_fmt(by_len[n])} |" for n in lens]
    lines += ["", f"Least-squares line through the medians: {slope:.3f} us per step, intercept {icpt:.1f} us (launch, state and weight "
              f"load, and the drain).  A call of T samples runs T + 3 macro steps; the three that drain the skew between the roles cost "
              f"about {3 * slope:.2f} us per call ({100 * 3 / (CHUNK + 3):.0f} % of the macro steps of a {CHUNK}-sample call).", ""]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
