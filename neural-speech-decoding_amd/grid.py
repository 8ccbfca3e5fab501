"""Hyper-parameter grid over the recorded trials: configurations x cross-validation folds in the launches one model uses.

    python -m nsd_amd.grid --data trials.npz --T 40 --kfold 5 --epochs 20 --batch 32 --grid lr=1e-3,3e-3 --grid dropout=0.4,0.6

--grid key=v1,v2,... is repeatable and forms the cartesian product (the first key varies slowest).  The keys name options of
nsd_amd.train: lr, weight_decay, dropout, label_smoothing, mixup, clip_grad_norm, aug_shift, aug_scale, aug_channel_drop, aug_noise, and
beside --avg ema (weight averaging: the averaged models are the scored ones, as in train) avg_decay; and sam_rho (sharpness-aware
minimisation, train's --sam-rho; 0 means off for that configuration).
Every other option is that of `train --kfold K --concurrent` and is shared by all configurations.  The runs are configurations x the
folds of train.concurrent_runs -- the folds, seeds and initial parameters `train --kfold K --concurrent` trains for that configuration --
packed as whole configurations into launches of at most 32 models (ModelBatchTrainer with per-model settings); the groups run one after
another.  `--class-weights balanced` is formed per fold over its training split (the sequential --kfold definition).

Output, JSON lines: one per (configuration, fold, epoch) as --concurrent emits them, with the configuration; per configuration the
mean +- sd of the last-epoch validation accuracy; one `done` line with the ranking and the best configuration as train.py arguments.
The best mean over folds is an optimistic estimate (it is selected on the folds it is scored on): re-estimate it on fresh folds.
No final model is trained.

--early-stop-patience N [--early-stop-metric loss|acc] [--early-stop-min-delta d] [--inner-fraction f] (train's options): every run
holds out an inner part of its training trials, all models of a launch are scored on theirs after each epoch in two launches
(ModelBatchTrainer.track_best), and the validation accuracy of a run is that of its best-epoch model, scored once at the end; the
summaries then carry the selection rule, the chosen epochs and the confusion matrices.

--crop-seconds S [--crops-per-trial R] [--crop-hop-seconds H] (train's options, shared by all configurations: the window sets the launch
dimensions): cropped training; every accuracy is then trial-level, pooled over the evaluation grid, and the records carry the first
window's accuracy beside it.
"""
from __future__ import annotations

import argparse
import itertools
import json
import sys
import time
from typing import Dict, List, Sequence, Tuple

import numpy as np

MAX_MODELS = 32                    # NSD_MAX_MODELS of include/nsd.h: models per launch
SELECTION = "best mean over folds: an optimistic estimate, re-estimate on fresh folds"
# --grid key -> (attribute of train.py's options, type)
GRID_KEYS = {"lr": ("lr", float), "weight_decay": ("weight_decay", float), "dropout": ("dropout", float),
             "label_smoothing": ("label_smoothing", float), "mixup": ("mixup", float), "clip_grad_norm": ("clip_grad_norm", float),
             "aug_shift": ("aug_shift", int), "aug_scale": ("aug_scale", float), "aug_channel_drop": ("aug_channel_drop", float),
             "aug_noise": ("aug_noise", float)}
# an axis that exists only beside another option: --grid avg_decay=... needs --avg ema (weight averaging; the scored models are then the
# averaged ones, as in train)
AVG_GRID_KEYS = {"avg_decay": ("avg_decay", float)}
# sharpness-aware minimisation: train's --sam-rho as an axis; 0 is a configuration without it
SAM_GRID_KEYS = {"sam_rho": ("sam_rho", float)}
ALL_KEYS = {**GRID_KEYS, **AVG_GRID_KEYS, **SAM_GRID_KEYS}


def parse_grid(specs: Sequence[str]) -> List[Tuple[str, list]]:
    """['lr=1e-3,3e-3', 'dropout=0.4,0.6'] -> [('lr', [0.001, 0.003]), ('dropout', [0.4, 0.6])]; ValueError names what is wrong."""
    out, seen = [], set()
    for spec in specs:
        key, sep, vals = spec.partition("=")
        key = key.strip().replace("-", "_")
        if not sep or key not in ALL_KEYS:
            raise ValueError(f"--grid {spec!r}: unknown key {key!r}: key=v1,v2,... with key one of {', '.join(ALL_KEYS)}")
        if key in seen:
            raise ValueError(f"--grid {spec!r}: {key} is given twice")
        seen.add(key)
        conv = ALL_KEYS[key][1]
        try:
            values = [conv(v) for v in vals.split(",")]
        except ValueError:
            raise ValueError(f"--grid {spec!r}: {conv.__name__} values separated by commas") from None
        if len(set(values)) != len(values):
            raise ValueError(f"--grid {spec!r}: a value is given twice")
        out.append((key, values))
    return out


def grid_product(grid: Sequence[Tuple[str, list]]) -> List[Dict[str, object]]:
    """The configurations of a parsed grid in product order: the first key varies slowest.  No --grid: one empty configuration."""
    keys = [k for k, _ in grid]
    return [dict(zip(keys, combo)) for combo in itertools.product(*[v for _, v in grid])]


def pack_groups(n_configs: int, runs_per_config: int, cap: int = MAX_MODELS) -> List[List[int]]:
    """Configurations 0 .. n-1, each with runs_per_config models, packed in order as WHOLE configurations into launches of at most `cap`
    models -> the configuration indices of each launch."""
    if runs_per_config < 1:
        raise ValueError(f"grid: {runs_per_config} runs per configuration")
    if runs_per_config > cap:
        raise ValueError(f"grid: {runs_per_config} folds per configuration but one launch takes at most {cap} models")
    per = cap // runs_per_config
    return [list(range(lo, min(lo + per, n_configs))) for lo in range(0, n_configs, per)]


def train_args(config: Dict[str, object]) -> List[str]:
    """A configuration as train.py arguments: ['--lr', '0.003', '--dropout', '0.4']"""
    out = []
    for k, v in config.items():
        out += ["--" + k.replace("_", "-"), repr(v)]
    return out


def build_parser() -> argparse.ArgumentParser:
    from .train import build_parser as train_parser
    ap = train_parser()
    ap.description = __doc__
    ap.add_argument("--grid", action="append", default=[], metavar="KEY=V1,V2,...",
                    help="repeatable; the cartesian product of all --grid options is searched.  Keys: " + ", ".join(ALL_KEYS))
    return ap


def main(argv=None) -> int:
    import copy

    import torch

    from . import data as D
    from .lstm_eeg_model import EEG_LSTM
    from .multimodel import ModelBatchTrainer
    from .ops import Augment, Crop, Loss
    from .prep import CausalPrep
    from .train import (average_for, concurrent_epoch, concurrent_runs, crop_for, drop_bad_trials, early_stop_settings, evaluate, evaluate_cropped,
                        align_for, fit_alignment, gate_for, loss_for, resample_for, resample_loaded,
                        padded_parts, parse_class_weights, sam_for, schedule_for, selection_text)

    ap = build_parser()
    args = ap.parse_args(argv)
    try:
        configs = grid_product(parse_grid(args.grid))
    except ValueError as e:
        ap.error(str(e))
    if args.kfold < 2:
        ap.error("grid: the runs are the folds of --kfold K (K >= 2)")
    if args.precision != "fp32" or args.bidirectional or args.hidden != 48:
        ap.error("grid: the model-batched path is H = 48 fp32 (--hidden 48, --precision fp32, no --bidirectional)")
    if args.save_folds:
        ap.error("grid: no models are kept (train the chosen configuration with nsd_amd.train)")
    if args.lr_schedule is None and (args.warmup_steps or args.lr_min_ratio or args.lr_step_size != 1 or args.lr_gamma != 1.0):
        args.lr_schedule = "constant"
    try:
        es = early_stop_settings(args, concurrent=True)          # (the grid's runs are always the model-batched folds)
        crops = crop_for(args)
    except ValueError as e:
        ap.error(str(e))
    crop_train, crop_eval = crops if crops is not None else (None, None)
    pooled = dict(crop=crop_eval) if crop_eval is not None else {}           # held-out scoring of a cropped run is trial-level

    def score(mdl, xs, ys):
        """(accuracy, first-window accuracy or None), as train's"""
        return (evaluate(mdl, xs, ys), None) if crop_eval is None else evaluate_cropped(mdl, xs, ys, crop_eval)
    prep_stage = any(v is not None for v in (args.prep_highpass, args.prep_lowpass, args.prep_notch, args.prep_zscore_seconds)) or args.prep_car
    prep_design = None
    if prep_stage:
        if args.normalize:
            ap.error("--prep-* with --normalize: the running z-score (--prep-zscore-seconds) replaces the whole-window one")
        try:
            prep_design = CausalPrep.design(fs=125.0, highpass=args.prep_highpass, lowpass=args.prep_lowpass, notch=args.prep_notch,
                                            zscore_seconds=args.prep_zscore_seconds, baseline=not args.prep_no_baseline, car=args.prep_car)
        except ValueError as e:
            ap.error(str(e))

    try:
        gate = gate_for(args)
    except ValueError as e:
        ap.error(str(e))
    if gate is not None and args.normalize:
        ap.error("--gate-* with --normalize: the whole-window z-score would be taken over held and zeroed channels")
    try:
        align = align_for(args)
    except ValueError as e:
        ap.error(str(e))
    if align is not None and args.normalize:
        ap.error("--align with --normalize: the whole-window z-score would undo the whitening channel by channel")
    try:
        resample = resample_for(args)
    except ValueError as e:
        ap.error(str(e))

    # every configuration as the options `train` would see, checked before anything runs
    cfg_args, augments = [], []
    for cfg in configs:
        a = copy.copy(args)
        for k, v in cfg.items():
            setattr(a, ALL_KEYS[k][0], v)
        try:
            average_for(a, 1)
            sam_for(a)
            if a.clip_grad_norm is not None and not a.clip_grad_norm >= 0.0:
                raise ValueError(f"clip_grad_norm {a.clip_grad_norm} negative")
            if not 0.0 <= a.dropout < 1.0:
                raise ValueError(f"dropout {a.dropout} outside [0, 1)")
            schedule_for(a, 1 + max(a.warmup_steps, 0))
            Loss(label_smoothing=a.label_smoothing, mixup=a.mixup)
            parse_class_weights(a.class_weights, a.classes)
            aug = Augment(max_shift=a.aug_shift, scale_range=a.aug_scale, p_channel=a.aug_channel_drop, noise_std=a.aug_noise)
            if aug.max_shift >= a.T:
                raise ValueError(f"aug_shift {aug.max_shift} must be smaller than --T {a.T}")
        except ValueError as e:
            ap.error(f"configuration {cfg}: {e}")
        cfg_args.append(a)
        augments.append(aug)

    if not torch.cuda.is_available():
        print("grid: needs an MI355X (no CPU training path)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", torch.cuda.current_device())
    if args.synthetic:
        rs = np.random.RandomState(args.seed)
        y_np = rs.randint(0, args.classes, args.synthetic).astype(np.int32)
        x_np = (2.7 * rs.standard_normal((args.synthetic, args.T, 8))).astype(np.float32)
        x_np[np.arange(args.synthetic), :, y_np % 8] += 1.5
    else:
        if not args.data:
            ap.error("give --data or --synthetic")
        lm = D.LABELS_5CLASS if args.classes == 5 else (D.LABELS_3CLASS_CHECKPOINT if args.label_order == "checkpoint" else D.LABELS_3CLASS_CODE)
        ts = D.load_trials_npz(args.data, lm, x_key=args.npz_key) if args.data.endswith(".npz") else D.load_trials(args.data, lm, samples=args.T)
        if ts.x.shape[1] != args.T:
            ap.error(f"--T {args.T} but the trials have {ts.x.shape[1]} samples")
        x_np, y_np = ts.x, ts.y
    if resample is not None:             # (as train: the runs see trials at the models' rate; --T counts the recorded samples)
        x_np = resample_loaded(x_np, resample, dev)
        if max(a.max_shift for a in augments) >= x_np.shape[1]:
            ap.error(f"aug_shift must be smaller than the {x_np.shape[1]} samples of a trial at --model-rate")
    x_np, y_np = drop_bad_trials(x_np, y_np, gate, args.gate_drop_trials, "grid")
    try:
        runs = concurrent_runs(y_np, args.kfold, args.kfold_seeds, args.seed, args.batch, es["inner_fraction"] if es else None)
        groups = pack_groups(len(configs), len(runs))
    except ValueError as e:
        print(f"grid: {e}", file=sys.stderr)
        return 2
    x_all, y_all = torch.from_numpy(x_np).to(dev), torch.from_numpy(y_np).to(dev)
    prep_all = prep_design if prep_design is None or prep_design.alpha == 0 else prep_design.calibrate(x_np)
    trials_dev = D.DeviceTrialSet(x_all, y_all, dev) if args.device_batches else None

    def emit(rec: dict) -> None:
        line = json.dumps(rec)
        print(line, flush=True)
        if args.log_jsonl:
            with open(args.log_jsonl, "a") as f:
                f.write(line + "\n")

    def tag(r) -> str:
        return f"fold{r['fold']}" if args.kfold_seeds == 1 else f"seed{r['seed_run']}_fold{r['fold']}"

    tr_devs = [torch.from_numpy(r["tr"]).to(dev) for r in runs]
    steps_per_epoch = concurrent_epoch(runs, args.batch, 0, lambda idxs: None)
    balanced = args.class_weights == "balanced"
    t0 = time.time()
    summaries = []
    for group in groups:
        # model (c, r) of the launch: configuration c's fold r, with the seed and initial parameters of its --concurrent run
        members = [(c, k) for c in group for k in range(len(runs))]
        models = []
        for c, k in members:
            torch.manual_seed(runs[k]["seed"])
            models.append(EEG_LSTM(8, args.hidden, 2, args.classes, cfg_args[c].dropout, normalize=args.normalize, prep=prep_all, crop=crop_train, gate=gate, align=align).to(dev).train())
        per = lambda f: [f(c, k) for c, k in members]                                         # noqa: E731
        mbt = ModelBatchTrainer(
            models, lr=per(lambda c, k: cfg_args[c].lr), weight_decay=per(lambda c, k: cfg_args[c].weight_decay),
            seeds=[runs[k]["seed"] + 1 for _, k in members], augment=per(lambda c, k: augments[c]),
            loss=per(lambda c, k: loss_for(cfg_args[c], y_np[runs[k]["tr"]] if balanced else y_np)),
            clip_grad_norm=per(lambda c, k: cfg_args[c].clip_grad_norm), lr_schedule=schedule_for(args, args.epochs * steps_per_epoch),
            average=per(lambda c, k: average_for(cfg_args[c], steps_per_epoch)), sam=per(lambda c, k: sam_for(cfg_args[c])),
            crop=crop_train)
        if align is not None:            # every member's matrix from its own fold's training part (label-free; not a grid axis)
            mbt.set_alignment(torch.stack([fit_alignment(mdl, x_all[tr_devs[k]], f"grid fold {k}")[0] for (_, k), mdl in zip(members, models)]))
        opt_on, avg_on, inner, es_epoch0 = mbt._opt_on, args.avg is not None, None, 0
        avg_start = average_for(cfg_args[0], steps_per_epoch).start_step if avg_on else 0      # (kind, start and stride are shared)
        res = [dict(acc_train_last=float("nan"), acc_val_last=float("nan")) for _ in members]
        member_runs = [runs[k] for _, k in members]

        def step(idxs):
            sel = [tr_devs[k][torch.from_numpy(ix).to(dev)] for (_, k), ix in zip(members, idxs)]
            mbt.step(torch.stack([x_all[s_] for s_ in sel]), torch.stack([y_all[s_] for s_ in sel]))
        if args.device_batches:          # the group's schedule on the device, one gather per step for all members (as train's)
            mbt.bind_batches(trials_dev, D.BatchSchedule.for_runs(member_runs, args.batch, args.epochs))
            step = lambda idxs, mbt=mbt: mbt.step_scheduled()                                 # noqa: E731

        if es:       # the held-out sets of all members, padded to one B each: built once per group
            held = {part: padded_parts(x_all, y_all, [r[part] for r in member_runs]) for part in ("tr", "inner", "va")}
        for epoch in range(args.epochs):
            concurrent_epoch(member_runs, args.batch, epoch, step)
            last = epoch == args.epochs - 1
            # --avg: the averaged rows are what is scored, compared and snapshotted, once averaging has begun (as in train)
            avg_ready = avg_on and (epoch + 1) * steps_per_epoch >= avg_start
            wts = dict(weights="average") if avg_ready else {}
            if es and (avg_ready or not avg_on):
                # every epoch: all members on their inner parts, the best-epoch decision and the snapshot, in two launches
                if inner is None:
                    es_epoch0 = epoch        # (--avg-start-epoch: evaluation n is epoch es_epoch0 + n - 1)
                inner = mbt.track_best(*held["inner"], metric=es["metric"], patience=es["patience"], min_delta=es["min_delta"], **wts, **pooled)
                last = last or all(e["stopped"] for e in inner)
            if epoch % args.log_every == 0 or last:
                losses = mbt.last_losses()
                norms, lrs, skipped = (mbt.last_grad_norms(), mbt.last_lrs(), mbt.skipped_steps()) if opt_on else (None, None, None)
                if es:
                    ev_tr, ev_va = mbt.evaluate(*held["tr"], **wts, **pooled), mbt.evaluate(*held["va"], **wts, **pooled)
                    ev_first = mbt.evaluate(*held["va"], **wts, crop=Crop(crop_eval.window, 1, 1)) if pooled else None
                scored = mbt.averaged_models() if avg_ready else models
                for i, (c, k) in enumerate(members):
                    if es:
                        acc_tr, acc_va, acc_first = ev_tr[i]["acc"], ev_va[i]["acc"], ev_first[i]["acc"] if pooled else None
                    else:
                        acc_tr = score(scored[i], x_all[tr_devs[k]], y_all[tr_devs[k]])[0]
                        acc_va, acc_first = score(scored[i], x_all[runs[k]["va"]], y_all[runs[k]["va"]])
                    res[i] = dict(acc_train_last=acc_tr, acc_val_last=acc_va)
                    emit({"run": tag(runs[k]), "config_index": c, "config": configs[c], "epoch": epoch, "loss_last_batch": round(losses[i], 5),
                          "acc_train": round(acc_tr, 4), "acc_val": round(acc_va, 4), "n_val": int(len(runs[k]["va"])),
                          "elapsed_s": round(time.time() - t0, 2), "concurrent": True,
                          **({"grad_norm": norms[i], "lr": lrs[i], "skipped": skipped[i]} if opt_on else {}),
                          **({"acc_val_first_window": round(acc_first, 4)} if acc_first is not None else {}),
                          **({"loss_inner": round(inner[i]["loss"], 5), "acc_inner": round(inner[i]["acc"], 4),
                              "best_epoch": es_epoch0 + inner[i]["best_eval"] - 1, "stopped": inner[i]["stopped"]} if inner is not None else {})})
            if es and last:
                break
        if es:       # the outer folds of the best-epoch models, in one call
            best = mbt.restore_best()
            final = mbt.evaluate(*held["va"], **pooled)
            for i in range(len(members)):
                res[i]["acc_val_last"] = final[i]["acc"]
        for c in group:
            mine = [i for i, (cc, _) in enumerate(members) if cc == c]
            accs = [res[i]["acc_val_last"] for i in mine]
            summaries.append({"summary": True, "config_index": c, "config": configs[c], "acc_val_mean": round(float(np.mean(accs)), 4),
                              "acc_val_sd": round(float(np.std(accs, ddof=1)), 4), "acc_val_folds": [round(float(a), 4) for a in accs],
                              **({"selection": selection_text(es), "best_epochs": [es_epoch0 + best[i] - 1 for i in mine],
                                  "confusion_val": [final[i]["confusion"].tolist() for i in mine]} if es else {}),
                              "train_args": train_args(configs[c])})
            emit(summaries[-1])
        del mbt, models
    ranking = sorted(summaries, key=lambda s: (-s["acc_val_mean"], s["config_index"]))
    emit({"done": True, "kfold": args.kfold, "kfold_seeds": args.kfold_seeds, "configurations": len(configs), "groups": groups,
          "ranking": [{k: s[k] for k in ("config_index", "config", "acc_val_mean", "acc_val_sd")} for s in ranking],
          "best": {"config": ranking[0]["config"], "train_args": ranking[0]["train_args"], "acc_val_mean": ranking[0]["acc_val_mean"],
                   "acc_val_sd": ranking[0]["acc_val_sd"]},
          "selection": SELECTION, "elapsed_s": round(time.time() - t0, 2)})
    return 0


if __name__ == "__main__":
    sys.exit(main())
