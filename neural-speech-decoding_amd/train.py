"""Command-line trainer standing in for the reference's missing notebook (DeepLearning/lstm_trainer.ipynb,
.MISSING_LARGE_BLOBS:1).  Trains EEG_LSTM on recorded trials (or synthetic windows) on 1..8 MI355X and writes a
checkpoint the reference's SimplePredictor loads unchanged (lstm_eeg_model.py:77-81).

    python -m nsd_amd.train --data /path/to/EEG_data_collection --classes 3 --epochs 60 --out model.pth
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m nsd_amd.train --synthetic 8192 ...

Every rank holds the whole data set in HBM (6.5 MB); each global batch is split contiguously over the ranks
(shard_range) and the flat gradient is summed with one RCCL all-reduce per step (trainer.py).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

from . import data as D
from .lstm_eeg_model import EEG_LSTM
from .ops import Augment, Average, Crop, Loss, LrSchedule, Sam
from .gate import SignalGate
from .align import SessionAlign
from .prep import CausalPrep
from .resample import Resample
from .trainer import Trainer, init_distributed, save_reference_checkpoint, shard_range


def evaluate(model: EEG_LSTM, x: torch.Tensor, y: torch.Tensor, batch: int = 512) -> float:
    was_training = model.training
    model.eval()
    correct = 0
    with torch.no_grad():
        for lo in range(0, x.shape[0], batch):
            pred = model(x[lo:lo + batch]).argmax(-1)
            correct += int((pred == y[lo:lo + batch].long()).sum().item())
    model.train(was_training)
    return correct / max(int(x.shape[0]), 1)


def evaluate_cropped(model: EEG_LSTM, x: torch.Tensor, y: torch.Tensor, grid: Crop, batch: int = 256):
    """(trial-level accuracy: each trial decided by the pooled probabilities of the windows of `grid`, accuracy of each trial's FIRST
    window alone -- what a live user gets after one window) of a model trained on crops; EEG_LSTM.predict_trials does the work."""
    pooled_ok = first_ok = 0
    for lo in range(0, x.shape[0], batch):
        pooled, wins = model.predict_trials(x[lo:lo + batch], hop=grid.hop, window=grid.window)
        lab = y[lo:lo + batch].long()
        pooled_ok += int((pooled.argmax(-1) == lab).sum().item())
        first_ok += int((wins[:, 0].argmax(-1) == lab).sum().item())
    n = max(int(x.shape[0]), 1)
    return pooled_ok / n, first_ok / n


CROP_OPTIONS = ("crop_seconds", "crops_per_trial", "crop_hop_seconds")
GATE_OPTIONS = ("gate_rail", "gate_jump", "gate_flat_seconds", "gate_pp", "gate_pp_seconds", "gate_hold_seconds", "gate_max_bad_channels",
                "gate_drop_trials")


def gate_for(args) -> Optional[SignalGate]:
    """The signal-quality gate the --gate-* options describe (None: none of its detectors is on); ValueError names a bad option."""
    if all(v is None for v in (args.gate_rail, args.gate_jump, args.gate_flat_seconds, args.gate_pp)):
        if any(getattr(args, k) is not None for k in GATE_OPTIONS):
            raise ValueError("--gate-*: no detector is on: give --gate-rail, --gate-jump, --gate-flat-seconds or --gate-pp")
        return None
    if args.gate_drop_trials is not None and not 0.0 <= args.gate_drop_trials <= 1.0:
        raise ValueError(f"--gate-drop-trials {args.gate_drop_trials} outside [0, 1]")
    if args.gate_drop_trials is not None and args.gate_max_bad_channels is None:
        raise ValueError("--gate-drop-trials needs --gate-max-bad-channels: without it no step is ever rejected and no trial dropped")
    return SignalGate.design(fs=125.0, rail=args.gate_rail, jump=args.gate_jump, flat_seconds=args.gate_flat_seconds, pp=args.gate_pp,
                             pp_seconds=0.5 if args.gate_pp_seconds is None else args.gate_pp_seconds,
                             hold_seconds=0.0 if args.gate_hold_seconds is None else args.gate_hold_seconds,
                             max_bad_channels=args.gate_max_bad_channels)


ALIGN_OPTIONS = ("align", "align_shrinkage", "align_floor")
RESAMPLE_OPTIONS = ("input_rate", "model_rate", "resample_zeros")


def resample_for(args):
    """--input-rate R [--model-rate 125 --resample-zeros Z] -> the Resample that brings the loaded trials to the models' rate, or None
    (no --input-rate, or the two rates are equal).  ValueError for rates the rate conversion does not cover."""
    if args.input_rate is None:
        return None
    if not (args.input_rate > 0 and args.model_rate > 0):
        raise ValueError(f"--input-rate {args.input_rate} / --model-rate {args.model_rate}: both positive")
    if float(args.input_rate) == float(args.model_rate):
        return None
    return Resample.design(args.input_rate, args.model_rate, zeros=args.resample_zeros)


def resample_loaded(x_np: np.ndarray, resample, dev) -> np.ndarray:
    """The loaded trials [N,T,C] at the amplifier's rate -> [N, ceil(T L / M), C] at the models', once, on the device (window mode:
    every trial from rest).  The trainers and everything they score are handed these."""
    from . import ops
    return ops.resample_trials(torch.from_numpy(np.ascontiguousarray(x_np, dtype=np.float32)).to(dev), resample).cpu().numpy()


def align_for(args) -> Optional[SessionAlign]:
    """The session alignment the --align* options describe (None without --align); ValueError names a bad option."""
    if not args.align:
        if args.align_shrinkage is not None or args.align_floor is not None:
            raise ValueError("--align-shrinkage / --align-floor without --align")
        return None
    return SessionAlign(shrinkage=0.0 if args.align_shrinkage is None else args.align_shrinkage,
                        floor=1e-4 if args.align_floor is None else args.align_floor)


def fit_alignment(model: EEG_LSTM, x_train: torch.Tensor, who: str):
    """--align: the model's matrix from its own training trials (label-free), before the first step -> (W [C,C] on the device, record)"""
    W, recs = model.align.fit(model, x_train)
    if recs[0]["few"] or recs[0]["nonfinite"]:
        print(f"{who}: --align: the fit kept the identity (status {recs[0]['status']}, {recs[0]['steps']} steps)", file=sys.stderr)
    model.set_alignment(W[0], record=recs[0])
    return W[0], recs[0]


def drop_bad_trials(x_np, y_np, gate: Optional[SignalGate], fraction: Optional[float], who: str):
    """--gate-drop-trials: the trials whose rejected fraction (data.screen_trials) exceeds `fraction` leave the set before the folds
    are made -> (x, y); prints how many."""
    if gate is None or fraction is None:
        return x_np, y_np
    _, rejected = D.screen_trials(x_np, gate)
    keep = rejected <= fraction
    print(f"{who}: --gate-drop-trials {fraction}: dropped {int((~keep).sum())} of {len(keep)} trials", file=sys.stderr)
    return x_np[keep], y_np[keep]


def crop_for(args, fs: float = 125.0):
    """None without --crop-seconds, else (the training Crop: --crops-per-trial drawn windows of --crop-seconds per trial and step, the
    evaluation grid: every whole window of the trial, --crop-hop-seconds apart -- default half the window).  ValueError, with the
    rule, for an option without --crop-seconds or out of range."""
    given = [o for o in CROP_OPTIONS[1:] if getattr(args, o, None) is not None]
    if getattr(args, "crop_seconds", None) is None:
        if given:
            raise ValueError(f"--{given[0].replace('_', '-')} needs --crop-seconds S")
        return None
    W = int(round(args.crop_seconds * fs))
    if not 1 <= W <= args.T:
        raise ValueError(f"--crop-seconds {args.crop_seconds}: {W} samples, outside [1, --T {args.T}]")
    hop = max(W // 2, 1) if args.crop_hop_seconds is None else int(round(args.crop_hop_seconds * fs))
    if hop < 1:
        raise ValueError(f"--crop-hop-seconds {args.crop_hop_seconds}: less than one sample")
    return Crop(W, 1 if args.crops_per_trial is None else args.crops_per_trial, 0), Crop.grid(args.T, W, hop)


def concurrent_runs(y_np: np.ndarray, kfold: int, seeds: int, seed: int, batch: int, inner_fraction=None):
    """The runs of `--kfold K --concurrent [--kfold-seeds N]`: for seed i in 0..N-1 and fold f, run seed seed + i with the folds of
    D.stratified_folds(y, K, seed + i) and per-fold seed (seed + i) + 101 f -- exactly what `--kfold K --seed <seed + i>` trains one
    after another.  Refuses (ValueError, with the rule) what would change what a fold sees when the runs share one step: a fold with
    fewer training windows than --batch, or folds that draw different numbers of batches per epoch.
    inner_fraction (early stopping): each run's training indices are split once more, D.stratified_split(y[tr], inner_fraction, the
    run's seed): `tr` becomes the part the model is fitted on -- the checks above apply to it -- and `inner` the part its epochs are
    compared on; `va`, the outer fold, is disjoint from both."""
    runs = []
    for i in range(seeds):
        s_i = seed + i
        for f, va in enumerate(D.stratified_folds(y_np, kfold, s_i)):
            tr = np.setdiff1d(np.arange(len(y_np)), va)
            runs.append(dict(seed_run=s_i, fold=f, tr=tr, va=va, seed=s_i + 101 * f))
            if inner_fraction is not None:
                fit_part, inner = D.stratified_split(y_np[tr], inner_fraction, s_i + 101 * f)
                if len(inner) == 0:
                    raise ValueError(f"--inner-fraction {inner_fraction}: fold {f} (seed {s_i}) gets an empty inner split")
                runs[-1].update(tr=tr[fit_part], inner=tr[inner])
    if len(runs) > 32:
        raise ValueError(f"--concurrent: {len(runs)} runs (--kfold-seeds x --kfold) but one launch takes at most 32 models")
    for r in runs:
        if len(r["tr"]) < batch:
            raise ValueError(f"--concurrent: fold {r['fold']} (seed {r['seed_run']}) has {len(r['tr'])} training windows, fewer than "
                             f"--batch {batch}: its sequential run takes one short batch per epoch, which one shared step cannot")
    counts = sorted({len(r["tr"]) // batch for r in runs})
    if len(counts) > 1:
        raise ValueError(f"--concurrent: the folds draw {counts} batches of {batch} per epoch; one shared step needs the same count "
                         "for every fold (use the sequential --kfold, or a --batch that divides the fold sizes alike)")
    return runs


def concurrent_epoch(runs, batch: int, epoch: int, step) -> int:
    """One epoch of the concurrent runs: step(list of index arrays, one per run) for the j-th batch of every run, each run's batches
    being D.epoch_batches(n_train, batch, seed_f, epoch, drop_last=True) -- those of its sequential run.  Returns the steps taken."""
    its = [D.epoch_batches(len(r["tr"]), batch, r["seed"], epoch, drop_last=True) for r in runs]
    n = 0
    for idxs in zip(*its):
        step(list(idxs))
        n += 1
    return n


EARLY_STOP_OPTIONS = ("early_stop_patience", "early_stop_metric", "early_stop_min_delta", "inner_fraction")


def early_stop_settings(args, concurrent: bool):
    """None where none of --early-stop-patience / --early-stop-metric / --early-stop-min-delta / --inner-fraction is given, else
    dict(metric, patience, min_delta, inner_fraction) with the defaults filled in.  ValueError, with the rule, for the options without
    the model-batched runs they need, without a patience, or out of range."""
    given = [o for o in EARLY_STOP_OPTIONS if getattr(args, o, None) is not None]
    if not given:
        return None
    flag = "--" + given[0].replace("_", "-")
    if not concurrent:
        raise ValueError(f"{flag}: early stopping runs on the model-batched folds: give --kfold K --concurrent (or use nsd_amd.grid)")
    if args.early_stop_patience is None:
        raise ValueError(f"{flag} needs --early-stop-patience N (N evaluations without improvement stop a model; 0: keep the best epoch, "
                         "never stop)")
    if args.early_stop_patience < 0:
        raise ValueError(f"--early-stop-patience {args.early_stop_patience} negative")
    min_delta = 0.0 if args.early_stop_min_delta is None else args.early_stop_min_delta
    if not min_delta >= 0.0:
        raise ValueError(f"--early-stop-min-delta {min_delta} negative")
    f = 0.2 if args.inner_fraction is None else args.inner_fraction
    if not 0.0 < f <= 0.5:
        raise ValueError(f"--inner-fraction {f} outside (0, 0.5]")
    return dict(metric=args.early_stop_metric or "loss", patience=args.early_stop_patience, min_delta=min_delta, inner_fraction=f)


def selection_text(es) -> str:
    """The `selection` field of a result: what picked the scored model"""
    if es is None:
        return "none: fixed epoch count, last-epoch model"
    return f"inner split: early stopping on {es['metric']}, patience {es['patience']}"


def padded_parts(x_all: torch.Tensor, y_all: torch.Tensor, parts):
    """The windows of M index arrays of unequal length as one [M,Bmax,T,C] / [M,Bmax] pair for ModelBatchTrainer.evaluate /
    track_best, and the counts: part m is padded with its own first window, which counts nowhere."""
    counts = [int(len(p)) for p in parts]
    bmax = max(counts)
    idx = np.stack([np.concatenate([np.asarray(p, dtype=np.int64), np.full(bmax - len(p), p[0], dtype=np.int64)]) for p in parts])
    it = torch.from_numpy(idx).to(x_all.device)
    return x_all[it].contiguous(), y_all[it].contiguous(), counts


def balanced_class_weights(y: np.ndarray, K: int):
    """--class-weights balanced: w_k = N / (K * n_k) over the labels of the training split (sklearn's `balanced`); a class without
    trials gets weight 0 (it has no target row to weigh)."""
    n = np.bincount(np.asarray(y).astype(np.int64), minlength=K)[:K].astype(np.float64)
    return tuple(float(len(y) / (K * c)) if c > 0 else 0.0 for c in n)


def parse_class_weights(text, K: int):
    """None, the string 'balanced' (resolved per training split by loss_for), or K comma-separated non-negative weights (ValueError)."""
    if text is None or text == "balanced":
        return text
    try:
        w = tuple(float(v) for v in text.split(","))
    except ValueError:
        raise ValueError(f"--class-weights {text!r}: 'balanced' or {K} comma-separated numbers") from None
    if len(w) != K:
        raise ValueError(f"--class-weights {text!r}: {len(w)} weights for --classes {K}")
    Loss(class_weights=w)                    # (range check)
    return w


def loss_for(args, y_train: np.ndarray) -> Loss:
    """The ops.Loss of a run from --label-smoothing / --class-weights / --mixup and the labels of its training split."""
    cw = parse_class_weights(args.class_weights, args.classes)
    if cw == "balanced":
        cw = balanced_class_weights(y_train, args.classes)
    return Loss(label_smoothing=args.label_smoothing, class_weights=cw, mixup=args.mixup)


def schedule_for(args, total_steps: int):
    """The ops.LrSchedule of a run of total_steps optimisation steps (epochs x steps per epoch) from --lr-schedule and its options;
    None without them."""
    if args.lr_schedule is None:
        return None
    return LrSchedule(kind=args.lr_schedule, warmup_steps=args.warmup_steps, total_steps=max(int(total_steps), args.warmup_steps + 1),
                      min_ratio=args.lr_min_ratio, step_size=args.lr_step_size, gamma=args.lr_gamma)


AVG_OPTIONS = ("avg", "avg_decay", "avg_start_epoch", "avg_every_steps")


def average_for(args, steps_per_epoch: int):
    """The ops.Average of a run from --avg and its options (None without --avg): --avg-start-epoch E, counted from 0, becomes the 1-based
    step E * steps_per_epoch + 1 -- the first step of that epoch.  ValueError, with the rule, for an option without --avg or out of range."""
    given = [o for o in AVG_OPTIONS[1:] if getattr(args, o, None) is not None]
    if getattr(args, "avg", None) is None:
        if given:
            raise ValueError(f"--{given[0].replace('_', '-')} needs --avg ema|swa")
        return None
    start = 0 if args.avg_start_epoch is None else args.avg_start_epoch
    if not 0 <= start < args.epochs:
        raise ValueError(f"--avg-start-epoch {start} outside [0, --epochs {args.epochs})")
    return Average(kind=args.avg, decay=0.999 if args.avg_decay is None else args.avg_decay, start_step=start * max(int(steps_per_epoch), 1) + 1,
                   every=1 if args.avg_every_steps is None else args.avg_every_steps)


def sam_for(args):
    """The ops.Sam of a run from --sam-rho (None without it, and for 0: a grid's configuration without SAM).  ValueError for a
    negative or non-finite rho."""
    rho = getattr(args, "sam_rho", None)
    if rho is None:
        return None
    if not 0.0 <= rho < float("inf"):
        raise ValueError(f"--sam-rho {rho} must be a finite number >= 0")
    return Sam(rho) if rho > 0 else None


def build_parser() -> argparse.ArgumentParser:
    """The options of this command (nsd_amd.grid shares them: its --grid keys name options of this parser)."""
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", help="directory with <prefix>_*.csv trials (reference: EEG_data_collection/), or a packed .npz "
                                   "of them (data.load_trials_npz)")
    ap.add_argument("--log-jsonl", default=None, help="also append the per-epoch JSON lines to this file (rank 0)")
    ap.add_argument("--synthetic", type=int, default=0, help="use N synthetic windows x = 2.7*N(0,1) instead of --data")
    ap.add_argument("--classes", type=int, default=3, choices=(3, 5))
    ap.add_argument("--label-order", default="checkpoint", choices=("checkpoint", "code"))
    ap.add_argument("--T", type=int, default=625)
    ap.add_argument("--epochs", type=int, default=40)
    ap.add_argument("--batch", type=int, default=64, help="GLOBAL batch size")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--weight-decay", type=float, default=0.0)
    ap.add_argument("--hidden", type=int, default=48)
    ap.add_argument("--dropout", type=float, default=0.60)
    ap.add_argument("--precision", default="fp32", choices=("fp32", "bf16"),
                    help="bf16: the sequence-batched path (hidden 64/128/256/512; BASELINE cfg3 = --hidden 256 --classes 5 --precision bf16)")
    ap.add_argument("--bidirectional", action="store_true", help="bidirectional LSTM (needs --precision bf16)")
    ap.add_argument("--val-fraction", type=float, default=0.2)
    ap.add_argument("--normalize", action="store_true", help="per-channel z-score of each window (app.py:166-170)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="eeg_lstm.pth")
    ap.add_argument("--log-every", type=int, default=1)
    ap.add_argument("--npz-key", default="x", help="array of a packed --data .npz holding the windows (`x_filt`: the windows as the "
                                                   "reference's PreProcessor hands them to the model, tests/golden/recorded_trials_filtered.npz)")
    ap.add_argument("--kfold", type=int, default=0, help="K > 1: K-fold cross-validation (mean +- sd of the LAST-epoch validation accuracy, "
                                                         "no epoch selection), then --out is trained on ALL trials with the same recipe")
    ap.add_argument("--concurrent", action="store_true", help="with --kfold: train the folds together, one model-batched step for all "
                                                                "of them (ModelBatchTrainer; single GPU, H = 48 fp32)")
    ap.add_argument("--save-folds", action="store_true", help="with --kfold K (sequential or --concurrent): keep the fold models -- each is "
                    "written after its last epoch next to --out, as <out stem>.fold<f>.pth (<out stem>.seed<s>_fold<f>.pth with "
                    "--kfold-seeds), and the final JSON line lists them under fold_checkpoints: the members of an EnsemblePredictor")
    ap.add_argument("--kfold-seeds", type=int, default=1, help="with --kfold K --concurrent: the K folds for N seeds --seed .. --seed + N - 1 "
                                                              "in the same launches (N * K <= 32)")
    ap.add_argument("--aug-shift", type=int, default=0, help="augmentation: shift each training trial by up to +-N steps (0 = off)")
    ap.add_argument("--aug-scale", type=float, default=0.0, help="augmentation: one amplitude factor in [1 - r, 1 + r] per trial (0 = off)")
    ap.add_argument("--aug-channel-drop", type=float, default=0.0, help="augmentation: probability that a channel of a trial is zeroed (0 = off)")
    ap.add_argument("--aug-noise", type=float, default=0.0, help="augmentation: standard deviation of additive noise per sample (0 = off)")
    ap.add_argument("--label-smoothing", type=float, default=0.0, help="loss: label smoothing eps in [0, 1) (0 = off)")
    ap.add_argument("--class-weights", default=None, help="loss: `balanced` (N / (K n_k) over the training split; with --concurrent over "
                                                          "all trials: one weight vector per launch) or K comma-separated weights w0,w1,...")
    ap.add_argument("--mixup", type=float, default=0.0, help="loss: mix every training trial with a partner of its batch, lambda = 1 - M * U(0,1) "
                                                             "(0 = off, 1 = uniform mixup)")
    ap.add_argument("--clip-grad-norm", type=float, default=None, help="optimizer: clip the global L2 norm of the gradient to this "
                                                                       "(0 = report the norm and skip non-finite steps, no clipping)")
    ap.add_argument("--lr-schedule", default=None, choices=("constant", "cosine", "step"),
                    help="optimizer: learning-rate schedule over epochs x steps per epoch, after --warmup-steps of linear warm-up")
    ap.add_argument("--warmup-steps", type=int, default=0, help="optimizer: linear warm-up over the first N steps")
    ap.add_argument("--lr-min-ratio", type=float, default=0.0, help="optimizer: cosine schedule's floor as a fraction of --lr")
    ap.add_argument("--lr-step-size", type=int, default=1, help="optimizer: step schedule: steps between two decays")
    ap.add_argument("--lr-gamma", type=float, default=1.0, help="optimizer: step schedule: factor of a decay, in (0, 1]")
    ap.add_argument("--prep-highpass", type=float, default=None, help="causal front end (CausalPrep): 2nd-order Butterworth high-pass corner, Hz")
    ap.add_argument("--prep-lowpass", type=float, default=None, help="causal front end: 2nd-order Butterworth low-pass corner, Hz")
    ap.add_argument("--prep-notch", type=float, default=None, help="causal front end: notch frequency, Hz (Q = 30)")
    ap.add_argument("--prep-zscore-seconds", type=float, default=None, help="causal front end: running z-score with this time constant; its "
                                                                            "starting variance is calibrated on the training split (with --concurrent: on all trials)")
    ap.add_argument("--prep-car", action="store_true", help="causal front end: common-average reference")
    ap.add_argument("--prep-no-baseline", action="store_true", help="causal front end: do not subtract each window's first sample")
    ap.add_argument("--gate-rail", type=float, default=None, help="signal-quality gate (SignalGate): a sample with |x| >= this is bad")
    ap.add_argument("--gate-jump", type=float, default=None, help="signal-quality gate: a sample-to-sample step >= this is bad")
    ap.add_argument("--gate-flat-seconds", type=float, default=None, help="signal-quality gate: equal samples for this long are bad")
    ap.add_argument("--gate-pp", type=float, default=None, help="signal-quality gate: a peak-to-peak swing >= this within --gate-pp-seconds is bad")
    ap.add_argument("--gate-pp-seconds", type=float, default=None, help="signal-quality gate: the span of --gate-pp (default 0.5, at most 64 samples)")
    ap.add_argument("--gate-hold-seconds", type=float, default=None, help="signal-quality gate: a channel stays bad this long after its last bad sample")
    ap.add_argument("--gate-max-bad-channels", type=int, default=None, help="signal-quality gate: a step with more bad channels than this is "
                                                                             "rejected: no decision (default: never)")
    ap.add_argument("--align", action="store_true", help="session alignment (SessionAlign): whiten the channels by the inverse square root of "
                    "their mean second moment, fitted per fold on the training trials before the first step and applied to the held-out ones")
    ap.add_argument("--align-shrinkage", type=float, default=None, help="session alignment: shrink the moment towards its mean diagonal, in [0, 1] (default 0)")
    ap.add_argument("--align-floor", type=float, default=None, help="session alignment: eigenvalues below this share of the largest are raised to it (default 1e-4)")
    ap.add_argument("--input-rate", type=float, default=None, metavar="HZ",
                    help="rate conversion (Resample): the loaded trials were recorded at this rate; they are brought to --model-rate once, on "
                         "the device, before anything else sees them (--T counts the recorded samples), and the checkpoint carries the "
                         "conversion so that a predictor or a stream decoder built from it takes samples at this rate")
    ap.add_argument("--model-rate", type=float, default=125.0, metavar="HZ", help="rate conversion: the rate the model decides at (default 125)")
    ap.add_argument("--resample-zeros", type=int, default=10, help="rate conversion: zero crossings of the windowed sinc on each side (default 10)")
    ap.add_argument("--gate-drop-trials", type=float, default=None, metavar="FRACTION",
                    help="signal-quality gate: drop the trials whose share of rejected steps exceeds FRACTION before the folds are made")
    ap.add_argument("--early-stop-patience", type=int, default=None,
                    help="with --kfold K --concurrent: early stopping per fold on an inner split of its training trials -- after every epoch "
                         "all folds are scored on their inner parts in two launches, each keeps the parameters of its best epoch on the "
                         "device and stops counting after N epochs without improvement (0: keep the best epoch, never stop); the outer "
                         "fold is scored once, at the end, with the best-epoch models")
    ap.add_argument("--early-stop-metric", default=None, choices=("loss", "acc"), help="early stopping: what is compared on the inner split "
                                                                                      "(default loss; acc: ties go to the lower loss)")
    ap.add_argument("--early-stop-min-delta", type=float, default=None, help="early stopping: an epoch is better only by more than this (default 0)")
    ap.add_argument("--inner-fraction", type=float, default=None, help="early stopping: share of each fold's training trials held out as its "
                                                                       "inner split, in (0, 0.5] (default 0.2)")
    ap.add_argument("--avg", default=None, choices=("ema", "swa"),
                    help="weight averaging in the update launch: an exponential moving average (ema) or the running mean (swa) of the "
                         "parameters over the steps; the scored and saved model is then the AVERAGED one, and every record carries the "
                         "last iterate's accuracy beside it.  Turns the guarded step tail on (non-finite steps are skipped and counted)")
    ap.add_argument("--avg-decay", type=float, default=None, help="weight averaging: EMA decay in [0, 1) (default 0.999)")
    ap.add_argument("--avg-start-epoch", type=int, default=None, help="weight averaging: first epoch (from 0) whose steps are averaged (default 0)")
    ap.add_argument("--avg-every-steps", type=int, default=None, help="weight averaging: average every N-th step from the start (default 1)")
    ap.add_argument("--sam-rho", type=float, default=None,
                    help="sharpness-aware minimisation: every step takes its gradient at the weights moved this distance uphill along the "
                         "normalised gradient (two forward/backward passes per step, about twice the time; 0.05 is the paper's default; 0 "
                         "is off).  Turns the guarded step tail on, and loss_last_batch is then the loss at the perturbed weights")
    ap.add_argument("--crop-seconds", type=float, default=None,
                    help="cropped training: every training trial is shown as --crops-per-trial windows of this length, cut at drawn offsets "
                         "on the device in every step; held-out trials are then decided by the pooled decisions of their windows on a "
                         "regular grid, and every record carries the accuracy of the first window alone beside it")
    ap.add_argument("--crops-per-trial", type=int, default=None, help="cropped training: windows per trial and step, 1 .. 64 (default 1)")
    ap.add_argument("--crop-hop-seconds", type=float, default=None, help="cropped training: distance of the evaluation grid's windows "
                                                                         "(default: half of --crop-seconds)")
    ap.add_argument("--device-batches", action="store_true",
                    help="keep each run's index schedule on the device beside the trials and gather every step's batch there (nsd_gather) "
                         "instead of indexing it on the host; a single fp32 model then replays its whole step, gather included, from one "
                         "hipGraph.  The batches are those of the host loop.  One GPU")
    return ap


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    prep_stage = any(v is not None for v in (args.prep_highpass, args.prep_lowpass, args.prep_notch, args.prep_zscore_seconds)) or args.prep_car
    prep_design = None
    if args.prep_no_baseline and not prep_stage:
        ap.error("--prep-no-baseline alone leaves the front end with nothing to do: give it a filter, a z-score or --prep-car")
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
    if resample is not None and args.normalize:
        ap.error("--input-rate with --normalize: a predictor built from the checkpoint would z-score over the filter's start-up")
    # (the models below are built without the conversion: they are trained and scored on trials already at their rate; the
    # checkpoints carry it)
    save_checkpoint = save_reference_checkpoint if resample is None else (lambda mdl, path: save_reference_checkpoint(mdl, path, resample=resample))

    def prep_for(idx):
        """The front end of a run trained on the trials idx: the design, its starting variance calibrated on those trials."""
        if prep_design is None or prep_design.alpha == 0:
            return prep_design
        return prep_design.calibrate(x_np[idx])
    if args.clip_grad_norm is not None and not args.clip_grad_norm >= 0.0:
        ap.error(f"--clip-grad-norm {args.clip_grad_norm} negative")
    if args.lr_schedule is None and (args.warmup_steps or args.lr_min_ratio or args.lr_step_size != 1 or args.lr_gamma != 1.0):
        args.lr_schedule = "constant"        # a schedule option alone (warm-up) turns the schedule on
    try:
        schedule_for(args, 1 + max(args.warmup_steps, 0))
    except ValueError as e:
        ap.error(str(e))
    try:
        Loss(label_smoothing=args.label_smoothing, mixup=args.mixup)
        parse_class_weights(args.class_weights, args.classes)
    except ValueError as e:
        ap.error(str(e))
    try:
        augment = Augment(max_shift=args.aug_shift, scale_range=args.aug_scale, p_channel=args.aug_channel_drop, noise_std=args.aug_noise)
    except ValueError as e:
        ap.error(str(e))
    if augment.max_shift >= args.T:
        ap.error(f"--aug-shift {augment.max_shift} must be smaller than --T {args.T}")
    if args.save_folds and (args.kfold < 2 or not args.out):
        ap.error("--save-folds keeps the fold models of --kfold K (K >= 2) next to --out")
    if args.kfold_seeds != 1 and not args.concurrent:
        ap.error("--kfold-seeds needs --kfold K --concurrent (sequentially: one --kfold run per --seed)")
    if args.concurrent:
        if args.kfold < 2:
            ap.error("--concurrent trains the folds of --kfold K (K >= 2) together")
        if args.kfold_seeds < 1 or args.kfold_seeds * args.kfold > 32:
            ap.error(f"--concurrent: --kfold-seeds {args.kfold_seeds} x --kfold {args.kfold} models; one launch takes 1 .. 32")
        if args.precision != "fp32" or args.bidirectional or args.hidden != 48:
            ap.error("--concurrent: the model-batched path is H = 48 fp32 (--hidden 48, --precision fp32, no --bidirectional)")

    try:
        es = early_stop_settings(args, concurrent=args.concurrent and args.kfold >= 2)
        average_for(args, 1)
        sam_for(args)
        crops = crop_for(args)
    except ValueError as e:
        ap.error(str(e))
    crop_train, crop_eval = crops if crops is not None else (None, None)

    rank, local, world = init_distributed()
    if not torch.cuda.is_available():
        print("train: needs an MI355X (no CPU training path)", file=sys.stderr)
        return 2
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)

    if args.synthetic:
        rs = np.random.RandomState(args.seed)
        y_np = rs.randint(0, args.classes, args.synthetic).astype(np.int32)
        # class-dependent mean shift on one channel so that there is something to learn
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
    if resample is not None:
        x_np = resample_loaded(x_np, resample, dev)
        args.T = int(x_np.shape[1])
        if augment.max_shift >= args.T:
            ap.error(f"--aug-shift {augment.max_shift} must be smaller than the {args.T} samples of a trial at --model-rate")
    x_np, y_np = drop_bad_trials(x_np, y_np, gate, args.gate_drop_trials, "train")
    tr_idx, va_idx = D.stratified_split(y_np, args.val_fraction, args.seed)
    x_all = torch.from_numpy(x_np).to(dev)
    y_all = torch.from_numpy(y_np).to(dev)
    if args.device_batches and world > 1:
        print("train: --device-batches runs on one GPU (a schedule sharded over ranks is not built)", file=sys.stderr)
        return 2
    trials_dev = D.DeviceTrialSet(x_all, y_all, dev) if args.device_batches else None

    def emit(rec: dict) -> None:
        if rank != 0:
            return
        line = json.dumps(rec)
        print(line, flush=True)
        if args.log_jsonl:
            with open(args.log_jsonl, "a") as f:
                f.write(line + "\n")

    def fold_path(tag: str) -> str:
        return f"{os.path.splitext(args.out)[0]}.{tag}.pth"

    def done_extra() -> dict:
        """What --save-folds adds to the final line; without the flag the line is what it was (the flag itself is left out of args)."""
        return {"fold_checkpoints": fold_paths} if args.save_folds else {}

    def shown_args() -> dict:
        return {k: v for k, v in vars(args).items() if (k != "save_folds" or v) and k != "device_batches" and (k not in EARLY_STOP_OPTIONS + AVG_OPTIONS + CROP_OPTIONS + GATE_OPTIONS + ("sam_rho",) or v is not None) and (k not in ALIGN_OPTIONS or v) and (k not in RESAMPLE_OPTIONS or args.input_rate is not None)}

    def score(mdl, xs, ys):
        """(accuracy, first-window accuracy or None): whole trials, or with --crop-seconds trials pooled over the evaluation grid"""
        if crop_eval is None:
            return evaluate(mdl, xs, ys), None
        return evaluate_cropped(mdl, xs, ys, crop_eval)

    fold_paths = []

    def fit(tr_idx, va_idx, seed: int, tag: str, out_path, keep_best: bool):
        """Train one model on tr_idx for args.epochs epochs.  keep_best: write the checkpoint of the best validation epoch
        (model selection ON the validation set: its accuracy is then optimistic); otherwise the model after the LAST epoch is
        what is written / scored -- the number of epochs is fixed beforehand, nothing is selected."""
        torch.manual_seed(seed)           # (Trainer also broadcasts rank 0's parameters when world > 1)
        model = EEG_LSTM(8, args.hidden, 2, args.classes, args.dropout, normalize=args.normalize, precision=args.precision,
                         bidirectional=args.bidirectional, prep=prep_for(tr_idx), crop=crop_train, gate=gate, align=align).to(dev).train()
        if align is not None:            # label-free, on this run's training trials; the held-out trials are scored through it
            fit_alignment(model, x_all[torch.from_numpy(tr_idx).to(dev)], f"train {tag}")
        steps_per_epoch = sum(1 for _ in D.epoch_batches(len(tr_idx), args.batch, seed, 0, drop_last=len(tr_idx) >= args.batch))
        average = average_for(args, steps_per_epoch)
        trainer = Trainer(model, lr=args.lr, weight_decay=args.weight_decay, seed=seed + 1, augment=augment, loss=loss_for(args, y_np[tr_idx]),
                          clip_grad_norm=args.clip_grad_norm, lr_schedule=schedule_for(args, args.epochs * steps_per_epoch), average=average,
                          sam=sam_for(args), crop=crop_train)
        opt_on = args.clip_grad_norm is not None or args.lr_schedule is not None or average is not None or sam_for(args) is not None
        scored = model                   # --avg: the averaged model, from its first averaged step on
        acc_va_last_iterate = float("nan")
        tr_dev = torch.from_numpy(tr_idx).to(dev)
        # --device-batches: the run's schedule goes to the device once and every step gathers its batch there; a single fp32 model with
        # all three random streams replays the step from one hipGraph.  A run of fewer trials than a batch keeps the host loop.
        scheduled = trials_dev is not None and len(tr_idx) >= args.batch
        graph_route = scheduled and args.precision == "fp32" and args.dropout > 0
        if scheduled:
            trainer.bind_batches(trials_dev, D.BatchSchedule.for_run(tr_idx, args.batch, seed, args.epochs))
        best = (-1.0, -1)
        t0 = time.time()
        acc_tr = acc_va = float("nan")
        for epoch in range(args.epochs):
            for _ in range(steps_per_epoch if scheduled else 0):
                trainer.step_scheduled(static=graph_route)
            for idx in (() if scheduled else D.epoch_batches(len(tr_idx), args.batch, seed, epoch, drop_last=len(tr_idx) >= args.batch)):
                # every rank takes part in every step (the step ends in a collective): a rank whose shard of a short tail
                # batch is empty passes zero trials and contributes a zero gradient; the mean is over the GLOBAL batch
                lo, hi = shard_range(len(idx), rank, world)
                sel = tr_dev[torch.from_numpy(idx[lo:hi]).to(dev)]
                trainer.step(x_all[sel].contiguous(), y_all[sel].contiguous(), global_batch=len(idx))
            last = epoch == args.epochs - 1
            if epoch % args.log_every == 0 or last:
                trainer.check()                  # every rank: raises (non-zero exit) if a scan group timed out anywhere
            if rank == 0 and (epoch % args.log_every == 0 or last):
                if average is not None and trainer.averaged_count() > 0:
                    scored = trainer.averaged_model()
                acc_tr = score(scored, x_all[tr_dev], y_all[tr_dev])[0]
                acc_va, acc_va_first = score(scored, x_all[va_idx], y_all[va_idx]) if len(va_idx) else (float("nan"), None)
                if keep_best and out_path and acc_va > best[0]:
                    best = (acc_va, epoch)
                    save_checkpoint(scored, out_path)
                extra = {"grad_norm": trainer.last_grad_norm(), "lr": trainer.last_lr(), "skipped": trainer.skipped_steps()} if opt_on else {}
                if acc_va_first is not None:
                    extra["acc_val_first_window"] = round(acc_va_first, 4)
                if average is not None:
                    acc_va_last_iterate = score(model, x_all[va_idx], y_all[va_idx])[0] if len(va_idx) else float("nan")
                    extra.update(acc_val_last_iterate=round(acc_va_last_iterate, 4), averaged_steps=trainer.averaged_count())
                emit({"run": tag, "epoch": epoch, "loss_last_batch": round(trainer.last_loss(), 5), "acc_train": round(acc_tr, 4),
                      "acc_val": round(acc_va, 4), "elapsed_s": round(time.time() - t0, 2), **extra})
        if rank == 0 and out_path and (not keep_best or best[1] < 0):
            save_checkpoint(scored, out_path)
        return {"acc_train_last": acc_tr, "acc_val_last": acc_va, "best_val_acc": best[0], "best_epoch": best[1],
                "acc_val_last_iterate": acc_va_last_iterate}

    if args.kfold > 1 and args.concurrent:
        if world > 1:
            print("train: --concurrent runs on one GPU (the model-batched path has no data parallel)", file=sys.stderr)
            return 2
        try:
            runs = concurrent_runs(y_np, args.kfold, args.kfold_seeds, args.seed, args.batch, es["inner_fraction"] if es else None)
        except ValueError as e:
            print(f"train: {e}", file=sys.stderr)
            return 2
        from .multimodel import ModelBatchTrainer
        models, prep_all = [], prep_for(np.arange(len(y_np)))
        for r in runs:
            torch.manual_seed(r["seed"])     # the initial parameters of the sequential run of this fold
            models.append(EEG_LSTM(8, args.hidden, 2, args.classes, args.dropout, normalize=args.normalize, prep=prep_all, crop=crop_train, gate=gate, align=align).to(dev).train())
        steps_per_epoch = concurrent_epoch(runs, args.batch, 0, lambda idxs: None)
        average = average_for(args, steps_per_epoch)
        mbt = ModelBatchTrainer(models, lr=args.lr, weight_decay=args.weight_decay, seeds=[r["seed"] + 1 for r in runs], augment=augment,
                                loss=loss_for(args, y_np), clip_grad_norm=args.clip_grad_norm,
                                lr_schedule=schedule_for(args, args.epochs * steps_per_epoch), average=average, sam=sam_for(args), crop=crop_train)
        pooled = dict(crop=crop_eval) if crop_eval is not None else {}       # held-out scoring of a cropped run is trial-level
        opt_on = args.clip_grad_norm is not None or args.lr_schedule is not None or average is not None or sam_for(args) is not None
        avg_on, inner, es_epoch0 = average is not None, None, 0
        tr_devs = [torch.from_numpy(r["tr"]).to(dev) for r in runs]
        if align is not None:            # every fold's matrix from its own training part
            mbt.set_alignment(torch.stack([fit_alignment(mdl, x_all[tr_devs[k]], f"train run {k}")[0] for k, mdl in enumerate(models)]))
        t0 = time.time()
        res = [dict(acc_train_last=float("nan"), acc_val_last=float("nan")) for _ in runs]

        def step(idxs):
            sel = [tr_devs[k][torch.from_numpy(ix).to(dev)] for k, ix in enumerate(idxs)]
            mbt.step(torch.stack([x_all[s_] for s_ in sel]), torch.stack([y_all[s_] for s_ in sel]))
        if trials_dev is not None:       # --device-batches: all runs' schedule on the device, one gather per step for all of them
            mbt.bind_batches(trials_dev, D.BatchSchedule.for_runs(runs, args.batch, args.epochs))
            step = lambda idxs: mbt.step_scheduled()

        def tag(r):
            return f"fold{r['fold']}" if args.kfold_seeds == 1 else f"seed{r['seed_run']}_fold{r['fold']}"
        if es:       # the held-out sets of all folds, padded to one B each (folds differ in size by one): built once
            held = {part: padded_parts(x_all, y_all, [r[part] for r in runs]) for part in ("tr", "inner", "va")}
        for epoch in range(args.epochs):
            concurrent_epoch(runs, args.batch, epoch, step)
            last = epoch == args.epochs - 1
            # --avg: what is scored (and, with early stopping, compared and snapshotted) is the averaged row, once averaging has begun
            avg_ready = avg_on and (epoch + 1) * steps_per_epoch >= average.start_step
            wts = dict(weights="average") if avg_ready else {}
            if es and (avg_ready or not avg_on):
                # every epoch: all folds on their inner parts, the best-epoch decision and the snapshot, in two launches
                if inner is None:
                    es_epoch0 = epoch        # (--avg-start-epoch: the first evaluation is that epoch's, so evaluation n is epoch es_epoch0 + n - 1)
                inner = mbt.track_best(*held["inner"], metric=es["metric"], patience=es["patience"], min_delta=es["min_delta"], **wts, **pooled)
                last = last or all(e["stopped"] for e in inner)
            if epoch % args.log_every == 0 or last:
                losses = mbt.last_losses()
                norms, lr_now, skipped = (mbt.last_grad_norms(), mbt.last_lr(), mbt.skipped_steps()) if opt_on else (None, None, None)
                if es:
                    ev_tr, ev_va = mbt.evaluate(*held["tr"], **wts, **pooled), mbt.evaluate(*held["va"], **wts, **pooled)
                    ev_va_iter = mbt.evaluate(*held["va"], **pooled) if avg_on else ev_va
                    ev_va_first = mbt.evaluate(*held["va"], **wts, crop=Crop(crop_eval.window, 1, 1)) if pooled else None
                scored = mbt.averaged_models() if avg_ready else models
                for k, r in enumerate(runs):
                    if es:
                        acc_tr, acc_va, acc_va_iter = ev_tr[k]["acc"], ev_va[k]["acc"], ev_va_iter[k]["acc"]
                        acc_va_first = ev_va_first[k]["acc"] if pooled else None
                    else:
                        acc_tr = score(scored[k], x_all[tr_devs[k]], y_all[tr_devs[k]])[0]
                        acc_va, acc_va_first = score(scored[k], x_all[r["va"]], y_all[r["va"]])
                        acc_va_iter = score(models[k], x_all[r["va"]], y_all[r["va"]])[0] if avg_on else acc_va
                    res[k] = dict(acc_train_last=acc_tr, acc_val_last=acc_va, acc_val_last_iterate=acc_va_iter, acc_val_first_window=acc_va_first)
                    emit({"run": tag(r), "epoch": epoch, "loss_last_batch": round(losses[k], 5), "acc_train": round(acc_tr, 4),
                          "acc_val": round(acc_va, 4), "elapsed_s": round(time.time() - t0, 2), "concurrent": True,
                          **({"grad_norm": norms[k], "lr": lr_now, "skipped": skipped[k]} if opt_on else {}),
                          **({"acc_val_last_iterate": round(acc_va_iter, 4)} if avg_on else {}),
                          **({"acc_val_first_window": round(acc_va_first, 4)} if acc_va_first is not None else {}),
                          **({"loss_inner": round(inner[k]["loss"], 5), "acc_inner": round(inner[k]["acc"], 4),
                              "best_epoch": es_epoch0 + inner[k]["best_eval"] - 1, "stopped": inner[k]["stopped"]} if inner is not None else {})})
            if es and last:
                break
        if es:       # the outer folds, looked at for the first time as far as the models are concerned: the best-epoch models, one call
            best = mbt.restore_best()
            final = mbt.evaluate(*held["va"], **pooled)
        accs = []
        for k, r in enumerate(runs):
            accs.append(final[k]["acc"] if es else res[k]["acc_val_last"])
            if args.save_folds:
                fold_paths.append(fold_path(tag(r)))
                # (with early stopping restore_best has put the selected row -- the averaged one with --avg -- into the model)
                save_checkpoint(models[k] if es or not avg_on else mbt.averaged_models()[k], fold_paths[-1])
            rec = {"fold": r["fold"], "n_train": int(len(r["tr"])), "n_val": int(len(r["va"])),
                   "acc_val_last_epoch": round(res[k]["acc_val_last"], 4), "acc_train_last_epoch": round(res[k]["acc_train_last"], 4),
                   "concurrent": True}
            if res[k].get("acc_val_first_window") is not None:
                rec["acc_val_first_window"] = round(res[k]["acc_val_first_window"], 4)
            if avg_on:       # the same training run scored twice: its last iterate and its averaged weights (both after the last epoch)
                rec.update(acc_val_last_iterate=round(res[k]["acc_val_last_iterate"], 4), acc_val_averaged=round(res[k]["acc_val_last"], 4))
            if es:
                rec.update(n_inner=int(len(r["inner"])), best_epoch=es_epoch0 + best[k] - 1, acc_val_best_epoch=round(final[k]["acc"], 4),
                           loss_val_best_epoch=round(final[k]["loss"], 5), confusion_val=final[k]["confusion"].tolist())
            if args.kfold_seeds > 1:
                rec["seed"] = r["seed_run"]
            emit(rec)
        everything = np.arange(len(y_np))
        r = fit(everything, everything[:0], args.seed + 7777, "all", args.out, keep_best=False)
        emit({"done": True, "kfold": args.kfold, "kfold_seeds": args.kfold_seeds, "acc_val_mean": round(float(np.mean(accs)), 4),
              "acc_val_sd": round(float(np.std(accs, ddof=1)), 4),
              "acc_val_folds": [round(float(a), 4) for a in accs], "selection": selection_text(es),
              **({"best_epochs": [es_epoch0 + b - 1 for b in best], "epochs_run": epoch + 1} if es else {}),
              "shipped": {"checkpoint": args.out, "trained_on": int(len(everything)), "acc_train_last_epoch": r["acc_train_last"]},
              "world": world, "concurrent": True, "args": shown_args(), **done_extra()})
        return 0

    if args.kfold > 1:
        # accuracy estimate: k stratified folds, every model trained for the SAME, pre-set number of epochs and scored after its
        # last epoch (no epoch picked on the validation data); then the shipped model: all trials, same recipe, no held-out set
        folds = D.stratified_folds(y_np, args.kfold, args.seed)
        accs = []
        for f, va in enumerate(folds):
            tr = np.setdiff1d(np.arange(len(y_np)), va)
            if args.save_folds:
                fold_paths.append(fold_path(f"fold{f}"))
            r = fit(tr, va, args.seed + 101 * f, f"fold{f}", fold_paths[-1] if args.save_folds else None, keep_best=False)
            accs.append(r["acc_val_last"])
            emit({"fold": f, "n_train": int(len(tr)), "n_val": int(len(va)), "acc_val_last_epoch": round(r["acc_val_last"], 4),
                  "acc_train_last_epoch": round(r["acc_train_last"], 4),
                  **({"acc_val_last_iterate": round(r["acc_val_last_iterate"], 4), "acc_val_averaged": round(r["acc_val_last"], 4)} if args.avg else {})})
        everything = np.arange(len(y_np))
        r = fit(everything, everything[:0], args.seed + 7777, "all", args.out, keep_best=False)
        emit({"done": True, "kfold": args.kfold, "acc_val_mean": round(float(np.mean(accs)), 4) if rank == 0 else None,
              "acc_val_sd": round(float(np.std(accs, ddof=1)), 4) if rank == 0 else None,
              "acc_val_folds": [round(float(a), 4) for a in accs], "selection": "none: fixed epoch count, last-epoch model",
              "shipped": {"checkpoint": args.out, "trained_on": int(len(everything)), "acc_train_last_epoch": r["acc_train_last"]},
              "world": world, "args": shown_args(), **done_extra()})
        return 0

    r = fit(tr_idx, va_idx, args.seed, "split", args.out, keep_best=True)
    emit({"done": True, "best_val_acc": r["best_val_acc"], "best_epoch": r["best_epoch"], "acc_val_last_epoch": r["acc_val_last"],
          **({"acc_val_last_iterate": r["acc_val_last_iterate"], "acc_val_averaged": r["acc_val_last"]} if args.avg else {}),
          "checkpoint": args.out, "world": world,
          "n_train": int(len(tr_idx)), "n_val": int(len(va_idx)), "args": shown_args()})
    return 0


if __name__ == "__main__":
    sys.exit(main())
