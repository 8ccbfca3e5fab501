"""Time nsd_augment (plain and with the fused z-score) against nsd_zscore_fwd at the same shapes, and a cfg2-shaped Trainer.step with
augmentation on against the same step without.

    python tools/augment_bench.py [--launches 200] [--rounds 5] [--out profiles/r06_augment.jsonl]

HIP-event timing after a warm-up, the legs of one shape alternating inside one process (drift hits all of them); every figure is the
minimum over the rounds of the mean of --launches back-to-back launches, with all rounds listed.  nsd_zscore_fwd is the yardstick:
it moves the same bytes with the same access pattern.  bytes = 2 * M*B*T*C * 4 (x read once, y written once; a shared input
is read M times, from cache).  Back-to-back launches of a few MB keep the data in the 256 MB Infinity Cache, so the rate is the
kernel's rate on cache-resident data, set against the HBM peak only as a scale."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nsd_amd  # noqa: E402
from nsd_amd import ops  # noqa: E402
from nsd_amd.trainer import Trainer  # noqa: E402

HBM_PEAK_SPEC, HBM_PEAK_MEASURED = 8.0e12, 6.29e12       # bytes/s: data sheet, and a float4 copy on this part


def _time(fn, n, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n                          # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench: needs the MI355X (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    A = nsd_amd.Augment(max_shift=12, scale_range=0.1, p_channel=0.1, noise_std=0.3)
    lines = []
    for M, B, T, Cc in [(1, 256, 250, 8), (1, 179, 625, 8), (1, 1024, 250, 8), (25, 36, 625, 8)]:
        x = (2.7 * torch.randn((B, T, Cc), generator=g)).to(dev)
        out = torch.empty((M, B, T, Cc), dtype=torch.float32, device=dev)
        rngs = [dict(seed=100 + m, base_stream=8) for m in range(M)]
        zin = out.clone().normal_().view(M * B, T, Cc)     # the yardstick z-scores M*B distinct windows (more bytes read when M > 1)
        zout = torch.empty_like(zin)
        legs = {"augment": lambda: ops.augment(x, A, rngs, M=M, out=out),
                "augment_zscore": lambda: ops.augment(x, A, rngs, M=M, zscore=True, out=out),
                "augment_noise_only": lambda: ops.augment(x, nsd_amd.Augment(noise_std=0.3), rngs, M=M, out=out),
                "augment_all_off_copy": lambda: ops.augment(x, nsd_amd.Augment(), rngs, M=M, out=out),
                "zscore_fwd": lambda: ops.zscore(zin, out=zout)}
        rounds = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                rounds[k].append(_time(fn, args.launches, args.warmup))
        nbytes = 2 * M * B * T * Cc * 4
        rec = dict(kind="launch", M=M, B=B, T=T, C=Cc, bytes=nbytes, launches=args.launches, rounds=args.rounds)
        for k, v in rounds.items():
            us = min(v) * 1e3
            rec[k] = dict(us=round(us, 3), rounds_us=[round(t * 1e3, 3) for t in v], TB_per_s=round(nbytes / (us * 1e-6) / 1e12, 3),
                          share_of_hbm_spec=round(nbytes / (us * 1e-6) / HBM_PEAK_SPEC, 3),
                          share_of_hbm_measured=round(nbytes / (us * 1e-6) / HBM_PEAK_MEASURED, 3))
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    # cfg2's shape: Trainer.step, B = 256, T = 250, dropout on; augment=None is the parent's launch sequence
    B, T = 256, 250
    x = (2.7 * torch.randn((B, T, 8), generator=g)).to(dev)
    y = torch.randint(0, 3, (B,), generator=g, dtype=torch.int32).to(dev)
    for normalize in (False, True):
        t_off = Trainer(nsd_amd.EEG_LSTM(normalize=normalize).to(dev).train(), seed=0)
        t_on = Trainer(nsd_amd.EEG_LSTM(normalize=normalize).to(dev).train(), seed=0, augment=A)
        off, on = [], []
        for _ in range(args.rounds):
            off.append(_time(lambda: t_off.step(x, y), args.launches, args.warmup))
            on.append(_time(lambda: t_on.step(x, y), args.launches, args.warmup))
        rec = dict(kind="step", B=B, T=T, normalize=normalize, steps=args.launches, rounds=args.rounds,
                   ms_step_augment_none=round(min(off), 5), ms_step_augment_on=round(min(on), 5),
                   rounds_none=[round(v, 5) for v in off], rounds_on=[round(v, 5) for v in on],
                   increase_us=round((min(on) - min(off)) * 1e3, 3), spread_none_us=round((max(off) - min(off)) * 1e3, 3),
                   device=torch.cuda.get_device_name(0))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
