"""What the rate conversion (nsd_resample_step, nsd_amd.Resample) costs and what it does to the recorded trials, written as tables for
profiles/resample.md.

    python tools/resample_latency.py [--reps 300] [--warmup 30] [--commit <text>] [--out profiles/resample_latency.md]

Per push (tools/gate_latency.py's method): GPU time between two HIP events recorded around StreamDecoder.push on the current stream,
after `--warmup` untimed pushes, over `--reps` CONSECUTIVE chunks of running streams; median, 10th / 90th percentile, mean.  The legs of
a point alternate inside one repetition, in one process, on one GPU, each on a decoder of its own:
  plain, plain'   a decoder without a conversion fed 0.2 s chunks at 125 Hz (25 samples): launch for launch the push before the stage
                  existed; run twice -- the difference of the twins is the spread a difference of legs has to beat
  resampled       the same model with Resample.design(250, 125), fed 0.2 s chunks at 250 Hz (50 samples -> 25 steps)
  step alone      nsd_resample_step in stream mode on that chunk, one launch
Window mode: ops.resample_trials on 324 x 1250 x 8 (the recorded trial set's size at 250 Hz).
Round trip: the recorded trials upsampled to 250 Hz on the host in float64 (band-limited: zero-padded spectrum, so every second sample
IS the recorded one), advanced by the filter's group delay (23 samples at 250 Hz, circularly: the interpolation is periodic), served
through EEG_LSTM(resample=design(250, 125)) with the shipped checkpoint; and every second sample taken without a filter.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STREAMS, CHUNK_SECONDS = (1, 64), 0.2


def _pct(v, q):
    s = sorted(v)
    return s[min(len(s) - 1, int(q * len(s)))]


def _fmt(v):
    return f"{statistics.median(v):6.1f} ({_pct(v, 0.1):.1f} .. {_pct(v, 0.9):.1f}; mean {statistics.fmean(v):.1f})"


def main():
    import numpy as np
    import torch
    import nsd_amd
    from nsd_amd import data as D
    from nsd_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--commit", default="working tree")
    ap.add_argument("--data", default=os.path.join(ROOT, "tests", "golden", "recorded_trials_filtered.npz"))
    ap.add_argument("--model", default=os.path.join(ROOT, "neural-speech-decoding_amd", "LSTM_Model", "lstm_classifier_Water_Food_Bg_Noise.pth"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_latency.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_latency: needs the MI355X (no GPU, no figures)")
    dev = torch.device("cuda:0")
    r = nsd_amd.Resample.design(250, 125)
    prep = nsd_amd.CausalPrep.design(highpass=1.0, lowpass=40.0, zscore_seconds=2.0)
    g = torch.Generator().manual_seed(0)

    def model(**kw):
        torch.manual_seed(1)
        return nsd_amd.EEG_LSTM(prep=prep, **kw).to(dev).eval()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3                       # microseconds

    n125, n250 = int(round(CHUNK_SECONDS * 125)), int(round(CHUNK_SECONDS * 250))
    rows = []
    for S in STREAMS:
        x125 = (2.7 * torch.randn((S, n125, 8), generator=g)).to(dev)
        x250 = (2.7 * torch.randn((S, n250, 8), generator=g)).to(dev)
        decs = dict(plain=nsd_amd.StreamDecoder(model(), S), plain2=nsd_amd.StreamDecoder(model(), S),
                    resampled=nsd_amd.StreamDecoder(model(resample=r), S))
        rs_state, y = ops.resample_state(8, r, S, dev), torch.empty((S, n125, 8), device=dev)
        calls = {k: (lambda d=d, x=(x250 if k == "resampled" else x125): d.push(x)) for k, d in decs.items()}
        calls["step"] = lambda: ops.resample_step(x250, r, rs_state, out=y)
        t = {k: [] for k in calls}
        for rep in range(a.warmup + a.reps):
            got = {k: timed(fn) for k, fn in calls.items()}
            if rep >= a.warmup:
                for k, v in got.items():
                    t[k].append(v)
        torch.cuda.synchronize(dev)
        rows.append((S, t))

    # window mode on the recorded set's size at 250 Hz
    xw = (2.7 * torch.randn((324, 1250, 8), generator=g)).to(dev)
    for _ in range(a.warmup):
        ops.resample_trials(xw, r)
    tw = [timed(lambda: ops.resample_trials(xw, r)) for _ in range(a.reps)]
    moved = (xw.numel() + 324 * 625 * 8) * 4

    # the round trip on the recorded trials
    ts = D.load_trials_npz(a.data, D.LABELS_3CLASS_CHECKPOINT, x_key="x_filt")
    x, labels = ts.x.astype(np.float64), ts.y
    N, T, _ = x.shape
    spec = np.fft.rfft(x, axis=1)
    pad = np.zeros((N, T + 1, x.shape[2]), complex)
    pad[:, :spec.shape[1]] = spec
    up = np.fft.irfft(pad, n=2 * T, axis=1) * 2.0
    interp_err = float(np.abs(up[:, ::2] - x).max())
    half = int(round(r.prototype_delay()))                     # 23 samples at 250 Hz
    adv = np.roll(up, -half, axis=1).astype(np.float32)
    state = torch.load(a.model, map_location="cpu", weights_only=True)
    state = state["state_dict"] if "state_dict" in state else state
    plain, conv = nsd_amd.EEG_LSTM().to(dev).eval(), nsd_amd.EEG_LSTM(resample=r).to(dev).eval()
    plain.load_state_dict(state, strict=True)
    conv.load_state_dict(state, strict=True)
    p_native = plain.predict_proba(torch.from_numpy(ts.x).to(dev)).cpu().numpy()
    p_conv = conv.predict_proba(torch.from_numpy(adv).to(dev)).cpu().numpy()
    p_late = conv.predict_proba(torch.from_numpy(up.astype(np.float32)).to(dev)).cpu().numpy()
    p_skip = plain.predict_proba(torch.from_numpy(np.ascontiguousarray(up[:, ::2]).astype(np.float32)).to(dev)).cpu().numpy()
    acc = lambda p: float((p.argmax(1) == labels).mean())                      # noqa: E731
    fed = ops.resample_trials(torch.from_numpy(adv).to(dev), r).cpu().numpy()
    start = r.P - 1 - half // 2                                                # outputs whose taps reach before the trial's first sample
    scale = float(np.abs(ts.x).max())

    med = statistics.median
    lines = [
        f"Machine: {torch.cuda.get_device_name(dev)}, torch {torch.__version__}.  Commit: {a.commit}.", "",
        f"Method: `python tools/resample_latency.py --reps {a.reps} --warmup {a.warmup}`.  GPU time between two HIP events around the call, "
        f"microseconds, median (10th .. 90th percentile; mean) of {a.reps} consecutive chunks after {a.warmup} untimed ones; the legs of a "
        "point alternate inside each repetition, one process, each leg on a decoder of its own.  Reference shape (C = 8, H = 48, L = 2, "
        f"K = 3), fp32, a causal front end (high-pass, low-pass, running z-score), {CHUNK_SECONDS} s chunks: `plain` / `plain'` "
        f"StreamDecoder.push of {n125} samples at 125 Hz without a conversion (nsd_prep_step + nsd_stream_step); `resampled` the push of "
        f"{n250} samples at 250 Hz through Resample.design(250, 125) (L / M = {r.L} / {r.M}, P = {r.P}: nsd_resample_step in front); "
        "`spread` |median(plain) - median(plain')|; `step alone`: nsd_resample_step on that chunk.", "",
        "| streams | plain, us | plain', us | resampled, us | resampled - plain (medians) | spread | step alone, us |",
        "|---|---|---|---|---|---|---|"]
    for S, t in rows:
        lines.append(f"| {S} | {_fmt(t['plain'])} | {_fmt(t['plain2'])} | {_fmt(t['resampled'])} | {med(t['resampled']) - med(t['plain']):+.1f} | "
                     f"{abs(med(t['plain']) - med(t['plain2'])):.1f} | {_fmt(t['step'])} |")
    lines += ["",
              f"Window mode, ops.resample_trials on 324 x 1250 x 8 -> 324 x 625 x 8: {_fmt(tw)} us; {moved / 1e6:.1f} MB read and written, "
              f"{moved / med(tw) / 1e3:.1f} GB/s at the median (the algorithm's bytes over the call's time; {2 * r.P * 324 * 625 * 8 / med(tw) / 1e3:.1f} "
              "GFLOP/s of multiplies and adds).", "",
              f"Round trip on the {N} recorded trials (`{os.path.relpath(a.data, ROOT)}`, x_filt; the shipped checkpoint): upsampled to 250 Hz "
              f"in float64 by a zero-padded spectrum (every second sample is the recorded one to {interp_err:.1e}), advanced by the group "
              f"delay of {half} samples at 250 Hz (circularly), served through EEG_LSTM(resample=design(250, 125)).", "",
              "| what the model is fed | accuracy | max abs change of a class probability against native | trials whose decision changes |",
              "|---|---|---|---|",
              f"| the native 125 Hz trials | {acc(p_native):.4f} | -- | -- |",
              f"| 250 Hz through the conversion, group delay taken out | {acc(p_conv):.4f} | {np.abs(p_conv - p_native).max():.3e} | {int((p_conv.argmax(1) != p_native.argmax(1)).sum())} |",
              f"| 250 Hz through the conversion, as it arrives (11.5 steps late) | {acc(p_late):.4f} | {np.abs(p_late - p_native).max():.3e} | {int((p_late.argmax(1) != p_native.argmax(1)).sum())} |",
              f"| every second 250 Hz sample, no filter | {acc(p_skip):.4f} | {np.abs(p_skip - p_native).max():.3e} | {int((p_skip.argmax(1) != p_native.argmax(1)).sum())} |",
              "",
              f"What the conversion feeds the model against the native samples (largest native sample {scale:.1f}): max abs difference "
              f"{np.abs(fed[:, start:] - ts.x[:, start:]).max():.3e} from step {start} on (behind the filter's start-up from rest), "
              f"{np.abs(fed[:, :start] - ts.x[:, :start]).max():.3e} inside it.", ""]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
