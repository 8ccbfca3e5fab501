"""Time nsd_mixup (targets only, and targets + mixed windows) and a cfg2-shaped Trainer.step with a soft-target loss against the same
step on hard labels.

    python tools/soft_targets_bench.py [--launches 200] [--rounds 5] [--out profiles/r07_soft_targets.jsonl]

HIP-event timing after a warm-up, the legs alternating inside one process (drift hits all of them); every figure is the minimum over
the rounds of the mean of --launches back-to-back launches, with all rounds listed.  bytes of a mixing launch = 3 * B*T*C * 4 (two
windows read, one written) + the target rows; back-to-back launches of a few MB keep the data in the 256 MB Infinity Cache, so the rate
is the kernel's rate on cache-resident data, set against the HBM peak only as a scale."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nsd_amd  # noqa: E402
from nsd_amd import ops  # noqa: E402
from nsd_amd.trainer import Trainer  # noqa: E402

HBM_PEAK_SPEC = 8.0e12                                    # bytes/s, data sheet


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
        raise SystemExit("soft_targets_bench: needs the MI355X (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    lines = []
    K = 3
    w = torch.tensor([0.5, 1.75, 1.0], device=dev)
    for M, B, T, Cc in [(1, 256, 250, 8), (1, 1024, 250, 8), (25, 36, 625, 8)]:
        x = (2.7 * torch.randn((B, T, Cc), generator=g)).to(dev)
        y = torch.randint(0, K, (M * B,), generator=g, dtype=torch.int32).to(dev)
        out = torch.empty((M, B, T, Cc), dtype=torch.float32, device=dev)
        tg = torch.empty((M * B, K), dtype=torch.float32, device=dev)
        rngs = [dict(seed=100 + m, base_stream=8) for m in range(M)]
        legs = {"mixup": lambda: ops.mixup(x, y, K, rngs, label_smoothing=0.1, mix=1.0, class_weights=w, M=M, out=out, targets=tg),
                "mix_off_copy": lambda: ops.mixup(x, y, K, rngs, label_smoothing=0.1, mix=0.0, class_weights=w, M=M, out=out, targets=tg),
                "targets_only": lambda: ops.mixup(None, y, K, rngs, label_smoothing=0.1, mix=0.0, class_weights=w, M=M, targets=tg)}
        rounds = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                rounds[k].append(_time(fn, args.launches, args.warmup))
        nbytes = {"mixup": 3 * M * B * T * Cc * 4, "mix_off_copy": 2 * M * B * T * Cc * 4, "targets_only": M * B * (K + 1) * 4}
        rec = dict(kind="launch", M=M, B=B, T=T, C=Cc, K=K, launches=args.launches, rounds=args.rounds)
        for k, v in rounds.items():
            us = min(v) * 1e3
            rec[k] = dict(us=round(us, 3), rounds_us=[round(t * 1e3, 3) for t in v], bytes=nbytes[k],
                          TB_per_s=round(nbytes[k] / (us * 1e-6) / 1e12, 3), share_of_hbm_spec=round(nbytes[k] / (us * 1e-6) / HBM_PEAK_SPEC, 3))
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    # cfg2's shape: Trainer.step, B = 256, T = 250, dropout on; loss=None is the hard-label launch sequence
    B, T = 256, 250
    x = (2.7 * torch.randn((B, T, 8), generator=g)).to(dev)
    y = torch.randint(0, 3, (B,), generator=g, dtype=torch.int32).to(dev)
    losses = {"hard": None, "smoothing_weights": nsd_amd.Loss(label_smoothing=0.1, class_weights=(0.5, 1.75, 1.0)),
              "smoothing_weights_mixup": nsd_amd.Loss(label_smoothing=0.1, class_weights=(0.5, 1.75, 1.0), mixup=1.0)}
    trainers = {k: Trainer(nsd_amd.EEG_LSTM().to(dev).train(), seed=0, loss=v) for k, v in losses.items()}
    rounds = {k: [] for k in trainers}
    for _ in range(args.rounds):
        for k, t in trainers.items():
            rounds[k].append(_time(lambda: t.step(x, y), args.launches, args.warmup))
    rec = dict(kind="step", B=B, T=T, steps=args.launches, rounds=args.rounds, device=torch.cuda.get_device_name(0))
    for k, v in rounds.items():
        rec[k] = dict(ms_step=round(min(v), 5), rounds_ms=[round(t, 5) for t in v], increase_us=round((min(v) - min(rounds["hard"])) * 1e3, 3))
    rec["spread_hard_us"] = round((max(rounds["hard"]) - min(rounds["hard"])) * 1e3, 3)
    print(json.dumps(rec), flush=True)
    lines.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
