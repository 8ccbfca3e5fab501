"""Augmentation recipes on the recorded trials: `nsd_amd.train --kfold 5 --concurrent --kfold-seeds 5` (25 models per launch) on
tests/golden/recorded_trials_filtered.npz (x_filt: the windows as the reference's PreProcessor hands them to the model), the shipped
recipe once without and once with each augmentation of a small grid.

    python tools/augment_recipes.py [--epochs 200] [--out profiles/r06_augment_recipes.jsonl]

One JSON line per recipe: mean and sd of the 25 last-epoch fold accuracies (no epoch selection), the five per-seed k-fold means and
their sd -- the spread a difference between two recipes has to exceed before it means anything.  All recipes run in one process."""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nsd_amd.train as train  # noqa: E402

GRID = [("baseline", []),
        ("shift12", ["--aug-shift", "12"]),
        ("shift31", ["--aug-shift", "31"]),
        ("scale0.1", ["--aug-scale", "0.1"]),
        ("chdrop0.1", ["--aug-channel-drop", "0.1"]),
        ("noise0.3", ["--aug-noise", "0.3"]),
        ("shift12_scale0.1", ["--aug-shift", "12", "--aug-scale", "0.1"]),
        ("shift12_chdrop0.1", ["--aug-shift", "12", "--aug-channel-drop", "0.1"]),
        ("shift31_scale0.1_chdrop0.1", ["--aug-shift", "31", "--aug-scale", "0.1", "--aug-channel-drop", "0.1"]),
        ("shift12_scale0.1_chdrop0.1_noise0.3", ["--aug-shift", "12", "--aug-scale", "0.1", "--aug-channel-drop", "0.1", "--aug-noise", "0.3"]),
        ("shift31_scale0.1_chdrop0.1_noise0.3", ["--aug-shift", "31", "--aug-scale", "0.1", "--aug-channel-drop", "0.1", "--aug-noise", "0.3"]),
        # soft-target recipes (ops.Loss: nsd_mixup + the `_soft` step); not run yet -- no accuracy is claimed for them
        ("smooth0.1", ["--label-smoothing", "0.1"]),
        ("balanced", ["--class-weights", "balanced"]),
        ("mixup1", ["--mixup", "1.0"]),
        ("smooth0.1_balanced", ["--label-smoothing", "0.1", "--class-weights", "balanced"]),
        ("mixup0.5_smooth0.1", ["--mixup", "0.5", "--label-smoothing", "0.1"]),
        ("shift12_mixup1_smooth0.1_balanced", ["--aug-shift", "12", "--mixup", "1.0", "--label-smoothing", "0.1", "--class-weights", "balanced"]),
        # optimizer recipes (clipping / schedules in the step tail); not run yet -- no accuracy is claimed for them
        ("clip1", ["--clip-grad-norm", "1.0"]),
        ("clip0.1", ["--clip-grad-norm", "0.1"]),
        ("cosine_warm50", ["--lr-schedule", "cosine", "--warmup-steps", "50", "--lr-min-ratio", "0.05"]),
        ("clip1_cosine_warm50", ["--clip-grad-norm", "1.0", "--lr-schedule", "cosine", "--warmup-steps", "50", "--lr-min-ratio", "0.05"]),
        ("shift12_clip1_cosine_warm50", ["--aug-shift", "12", "--clip-grad-norm", "1.0", "--lr-schedule", "cosine", "--warmup-steps", "50",
                                         "--lr-min-ratio", "0.05"])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--normalize", action="store_true", help="also run every recipe with --normalize (noise is then relative to unit variance)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    data = os.path.join(ROOT, "tests", "golden", "recorded_trials_filtered.npz")
    tmp = tempfile.mkdtemp(prefix="augment_recipes_")
    lines = []
    variants = [("", [])] + ([("_n", ["--normalize"])] if args.normalize else [])
    for suffix, extra in variants:
        for name, aug in GRID:
            log = os.path.join(tmp, f"{name}{suffix}.jsonl")
            argv = ["--data", data, "--npz-key", "x_filt", "--classes", "3", "--kfold", "5", "--concurrent", "--kfold-seeds", "5",
                    "--epochs", str(args.epochs), "--batch", "32", "--lr", "0.001", "--seed", str(args.seed), "--log-every", "1000",
                    "--out", os.path.join(tmp, f"{name}{suffix}.pth"), "--log-jsonl", log] + extra + aug
            rc = train.main(argv)
            if rc != 0:
                raise SystemExit(f"augment_recipes: {name}{suffix}: train.main returned {rc}")
            done = [json.loads(l) for l in open(log) if '"done"' in l][-1]
            folds = done["acc_val_folds"]
            means = [round(statistics.mean(folds[i:i + 5]), 4) for i in range(0, len(folds), 5)]
            rec = {"recipe": name + suffix, "args": argv[argv.index("--epochs"):argv.index("--out")] + extra + aug, "seeds": len(means),
                   "folds": len(folds), "acc_val_mean": round(statistics.mean(folds), 4),
                   "acc_val_sd_over_folds": round(statistics.pstdev(folds), 4), "kfold_means_per_seed": means,
                   "sd_of_seed_means": round(statistics.pstdev(means), 4),
                   "acc_train_last_epoch_all_trials": done["shipped"]["acc_train_last_epoch"]}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            if args.out:                                   # written as it goes: a run that is cut short leaves what it has
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    for r in lines:
                        f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
