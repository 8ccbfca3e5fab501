"""Session calibration on the MI355X: refit the read-out of a trained model on a dozen cued trials of a new session, with the recurrent
layers and the attention frozen (nsd_stream_features / nsd_head_fit of include/nsd.h, csrc/nsd_head_fit.hip).

An extension: the reference has no training code at all.  A model trained on earlier sessions meets electrodes whose impedances and a
posture that differ; standard BCI practice records a few cued trials and refits the last layers.  The trials go through a
StreamDecoder (so preprocessing and a causal front end are exactly what the live stream applies), the pooled vector each slot holds
is read out, and LayerNorm / fc.0 / fc.3 are fitted on those frozen vectors by E full-batch Adam epochs in ONE launch, all the
models of an ensemble together.

    python -m nsd_amd.calibrate --model old.pth [--model fold1.pth ...] --data session_dir_or.npz --calib-per-class 4 --out new.pth
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import Optional, Sequence

import numpy as np
import torch

from . import ops
from ._lib import NSD_FIT_MAX_EPOCHS, NsdError
from .ops import Loss


class HeadFit:
    """Refit the read-out (LayerNorm, fc.0, fc.3) of M EEG_LSTM models of one shape on frozen pooled features.

      fit(feats, labels) -> losses [M, E]   feats [N,H] (one set for all models) or [M,N,H] (device fp32, StreamDecoder.features /
                                            EnsembleStreamDecoder.features), labels [N] class indices.  Runs `epochs` full-batch Adam
                                            epochs in one launch and updates the models' flat parameters in place (only the tensors
                                            `train` names; the LSTM stack and the attention never change).  losses[m, e]: model m's
                                            mean loss before epoch e's update.  A second call continues the same run: Adam's moments
                                            and the epoch count live in the state, and 3 + 4 epochs leave the bits 7 leave.
      reset()                               forget the moments and the epoch count (the parameters stay as they are)
      epochs_done() / status()              per model: epochs run since the reset; 1 where the fit was refused on the device (a
                                            non-finite feature, target or loss -- that model's parameters keep the last good bits)
      check()                               raises NsdError where a status is set

    models: a sequence of EEG_LSTM (eval or train mode; their flat parameters are gathered into one [M,P] buffer for the launch and
    written back), or the ensemble an EnsemblePredictor holds (`predictor.model`: its stacked parameter buffer is fitted in place, so an
    open EnsembleStreamDecoder reads the fitted head at its next push, and the members' own tensors are updated too).  A single
    EEG_LSTM is fitted in place as well: an open StreamDecoder shares its parameter tensor.
    lr defaults to Trainer's 1e-3.  epochs = 100 is a CHOICE, not a measurement: at 1.8 k parameters and a dozen trials an epoch
    costs microseconds, and nothing here has tuned the count against held-out data.
    head_dropout: None = eval-mode fit (eval RReLU slope, no dropout, deterministic); a probability p in [0, 1) = train-mode noise, the
    RReLU slopes and head-dropout masks a Trainer's step e would draw with `seed` (model m uses seed + m).
    loss: an nsd_amd.Loss -- label smoothing and class weights build the target rows with the nsd_mixup launch at mix = 0; mixup is
    refused (the features are frozen: there are no windows to mix)."""

    def __init__(self, models, *, epochs: int = 100, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 train: Sequence[str] = ("ln", "fc0", "fc3"), head_dropout: Optional[float] = None, loss: Optional[Loss] = None,
                 seed: int = 0):
        from .lstm_eeg_model import EEG_LSTM
        from .multimodel import _check_models
        self._ensemble = None
        if isinstance(models, EEG_LSTM):
            members = [models]
        elif hasattr(models, "models") and hasattr(models, "params"):
            self._ensemble, members = models, list(models.models)
        else:
            members = list(models)
        if not members or not all(isinstance(m, EEG_LSTM) for m in members):
            raise NsdError("HeadFit: expected an EEG_LSTM, a sequence of them, or the ensemble an EnsemblePredictor holds")
        if len(members) > 1:
            _check_models(members, "HeadFit")
        first = members[0]
        if first.precision != "fp32" or first.spec.D != 1 or not ops.stream_path(first.spec):
            raise NsdError(f"HeadFit: model shape {first.spec} is outside nsd_head_fit_path (the resumable path: fp32, hidden size 48, "
                           "2 layers, <= 8 channels, fc width and classes <= 64)")
        if not 1 <= int(epochs) <= NSD_FIT_MAX_EPOCHS:
            raise NsdError(f"HeadFit: epochs = {epochs} outside [1, {NSD_FIT_MAX_EPOCHS}]")
        if loss is not None and loss.mixup:
            raise NsdError("HeadFit: mixup is refused -- the features are frozen, there are no windows to mix; label smoothing and "
                           "class weights apply")
        if loss is not None:
            loss.check_classes(first.spec.K)
        if head_dropout is not None and not 0.0 <= float(head_dropout) < 1.0:
            raise NsdError(f"HeadFit: head_dropout = {head_dropout} outside [0, 1)")
        self.mask = ops.fit_mask(tuple(train))
        if not self.mask:
            raise NsdError("HeadFit: train names no tensor group (\"ln\", \"fc0\", \"fc3\")")
        flats = [m.flat_parameters() for m in members]
        if not all(f.is_cuda for f in flats):
            raise NsdError("HeadFit runs only on the MI355X HIP path: move the models to the GPU first; there is no CPU fallback")
        self.members, self.spec, self.device = members, first.spec, flats[0].device
        self.epochs, self.lr, self.betas, self.eps, self.weight_decay = int(epochs), float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.loss, self.head_dropout, self.seed = loss, head_dropout, int(seed)
        self.state = ops.head_fit_state(self.spec, len(members), self.device)
        self._layout = ops.head_fit_layout(self.spec)

    @property
    def M(self) -> int:
        return len(self.members)

    def _params(self) -> torch.Tensor:
        """[M,P]: the ensemble's own buffer, the single model's own vector, or a gathered copy of the members'"""
        if self._ensemble is not None:
            return self._ensemble.params
        if self.M == 1:
            return self.members[0].flat_parameters().view(1, -1)
        return torch.stack([m.flat_parameters() for m in self.members]).contiguous()

    def targets(self, labels, N: int) -> torch.Tensor:
        """target rows [M*N, K] of the labels [N] (the same for every model): one nsd_mixup launch at mix = 0"""
        y = labels if torch.is_tensor(labels) else torch.from_numpy(np.ascontiguousarray(labels))
        y = y.to(device=self.device, dtype=torch.int32).reshape(-1)
        if int(y.numel()) != N:
            raise NsdError(f"HeadFit.fit: {int(y.numel())} labels for {N} trials")
        return ops.target_rows(y.repeat(self.M).contiguous(), self.spec.K, self.M, self.loss)

    @torch.no_grad()
    def fit(self, feats: torch.Tensor, labels, epochs: Optional[int] = None) -> torch.Tensor:
        if not torch.is_tensor(feats) or feats.dim() not in (2, 3) or int(feats.shape[-1]) != self.spec.H:
            raise NsdError(f"HeadFit.fit: feats must be a device tensor [N, {self.spec.H}] or [{self.M}, N, {self.spec.H}]")
        if feats.dim() == 3 and int(feats.shape[0]) != self.M:
            raise NsdError(f"HeadFit.fit: feats of {int(feats.shape[0])} models for {self.M}")
        N = int(feats.shape[-2])
        if not ops.head_fit_path(self.spec, self.M, N):
            raise NsdError(f"HeadFit.fit: {N} trials for {self.M} models of shape {self.spec} are outside nsd_head_fit_path "
                           "(1 .. 256 trials, fewer where fc width and classes are large; 1 .. 32 models)")
        feats = feats.to(self.device).contiguous().float()
        q = self.targets(labels, N)
        rngs = None
        if self.head_dropout is not None:
            rngs = [dict(seed=self.seed + m, base_stream=0, p_lstm=0.0, p_head=float(self.head_dropout)) for m in range(self.M)]
        params = self._params()
        losses = ops.head_fit(self.spec, params, feats, q, self.state, epochs=self.epochs if epochs is None else int(epochs), lr=self.lr,
                              beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, weight_decay=self.weight_decay, train=self.mask,
                              rngs=rngs)
        if self._ensemble is not None or self.M > 1:                 # the members' own tensors follow the fitted buffer
            for m, row in zip(self.members, params):
                m.flat_parameters().copy_(row)
        return losses

    def reset(self) -> None:
        self.state.zero_()

    def epochs_done(self) -> list:
        col = int(self._layout.epochs) // 2
        return [int(v) for v in self.state.view(torch.int64)[:, col].cpu()]

    def status(self) -> list:
        return [int(v) for v in self.state.view(torch.int32)[:, int(self._layout.status)].cpu()]

    def check(self) -> None:
        bad = [m for m, s in enumerate(self.status()) if s]
        if bad:
            raise NsdError(f"HeadFit: the fit of model(s) {bad} was refused on the device (a feature, a target or an epoch's loss was not "
                           "finite); their parameters keep the last good values.  reset() clears the status")


def _accuracy_and_loss(probs: np.ndarray, labels: np.ndarray):
    p = np.asarray(probs, dtype=np.float64)
    acc = float((p.argmax(1) == labels).mean())
    loss = float(-np.log(np.clip(p[np.arange(len(labels)), labels], 1e-300, None)).mean())
    return acc, loss


def calibrate_predictor(predictor, trials, labels, align: bool = True, spatial: Optional[dict] = None, **fit_kw) -> dict:
    """SimplePredictor.calibrate / EnsemblePredictor.calibrate: run `trials` ([N,T,C] numpy, or a list of [T,C]) through open_stream on
    reset slots, read the pooled features, fit the read-out(s) on (features, labels), and report loss and accuracy on the calibration
    trials before and after.  labels: class indices [N].  fit_kw: HeadFit's keywords.  Returns dict(n, epochs, loss_before, loss_after,
    acc_before, acc_after, fit_losses [M,E] numpy, status).  The predictor's model(s) are updated in place.
    spatial: None (nothing more is launched), or a dict of align.SpatialFit's keywords ({} for its defaults): the supervised fit of the
    alignment matrix through the frozen model, between the label-free whitening refit and the features -- the order is whitening refit
    (if align), SpatialFit, features, HeadFit.  A model without an alignment stage gains one at the identity.  The report gains
    spatial_losses [E], spatial_status, and loss_spatial / acc_spatial: the calibration trials after the spatial stage alone.
    An ensemble takes spatial=dict(shared=True, ...): ONE matrix is fitted through all members (align.EnsembleSpatialFit: the launches
    of a single model's epoch, dx the serial mean over the members) and written to every member; without the key an ensemble is refused
    before anything runs.  shared=True on a single model is SpatialFit."""
    x = np.stack([np.asarray(t, dtype=np.float32) for t in trials]) if not isinstance(trials, np.ndarray) else trials
    if x.ndim != 3:
        raise ValueError(f"calibrate: trials must be [N, T, C], got {x.shape}")
    y = np.asarray(labels).astype(np.int64).reshape(-1)
    N = int(x.shape[0])
    if y.shape[0] != N:
        raise ValueError(f"calibrate: {y.shape[0]} labels for {N} trials")
    K = len(predictor.class_names)
    if y.min() < 0 or y.max() >= K:
        raise ValueError(f"calibrate: labels must be class indices in [0, {K})")
    chunk_transform = fit_kw.pop("chunk_transform", None)
    if spatial is not None:                               # refused before anything runs: a refused call leaves the predictor as it was
        from .align import check_spatial_fit
        cfg = dict(epochs=50, lr=1e-2, decay=1e-2, betas=(0.9, 0.999), eps=1e-8)
        check_spatial_fit(**{k: spatial.get(k, d) for k, d in cfg.items()})
        if not isinstance(spatial.get("shared", False), bool):
            raise ValueError(f"calibrate: spatial['shared'] {spatial['shared']!r} must be True or False")
        if hasattr(predictor.model, "models") and not spatial.get("shared"):
            raise NsdError("calibrate: spatial= for an ensemble needs the key shared=True -- an ensemble's decoders share one alignment "
                           "matrix, so ONE matrix is fitted through all members (align.EnsembleSpatialFit); without the key nothing is "
                           "fitted.  (Members fitted one by one with align.SpatialFit hold M matrices and have to be served apart)")
        if chunk_transform is not None:
            raise NsdError("calibrate: spatial= with chunk_transform= is not offered -- the fit runs the model's own front end over the "
                           "trials; give the model a CausalPrep")
    stream = predictor.open_stream(streams=N, chunk_transform=chunk_transform)
    align_record = None
    if align and getattr(predictor.model, "align", None) is not None:
        # label-free, first: the session's matrix from the second moment of all calibration trials as the live stream delivers them,
        # then a fresh decoder that starts from it -- features and the head fit run on aligned input
        stream.decoder.align_accumulate(True)
        before, _ = stream.push(x)
        W, rec = ops.whiten_fit(predictor.model.spec.C, predictor.model.align, state=stream.decoder.cov_state)
        align_record = ops.whiten_records(rec, 1)[0]
        if not (align_record["few"] or align_record["nonfinite"]):
            predictor.model.set_alignment(W[0], record=align_record)
        if spatial is None:                               # (with a spatial stage the decoder behind it is the one that is read)
            stream = predictor.open_stream(streams=N, chunk_transform=chunk_transform)
            stream.push(x)
    else:
        before, _ = stream.push(x)
    spatial_report = {}
    if spatial is not None:
        from .align import EnsembleSpatialFit, SpatialFit
        skw = {k: v for k, v in spatial.items() if k != "shared"}
        # (shared=True on a single model is SpatialFit; an ensemble -- refused above without the key -- fits one matrix through all members)
        sfit = EnsembleSpatialFit(predictor.model, **skw) if hasattr(predictor.model, "models") else SpatialFit(predictor.model, **skw)
        sl = sfit.fit(x, y)
        stream = predictor.open_stream(streams=N)              # a fresh decoder: it starts from the fitted matrix
        mid, _ = stream.push(x)
        acc_s, loss_s = _accuracy_and_loss(mid, y)
        spatial_report = dict(spatial_losses=sl.cpu().numpy(), spatial_status=sfit.status(), loss_spatial=loss_s, acc_spatial=acc_s)
    feats = stream.decoder.features()
    fit = HeadFit(predictor.model, **fit_kw)          # an EEG_LSTM, or the ensemble an EnsemblePredictor holds
    losses = fit.fit(feats, y)
    # the decision of the same slots through the fitted head: a reset and a second pass of the same samples
    stream.reset()
    after, _ = stream.push(x)
    acc0, loss0 = _accuracy_and_loss(before, y)
    acc1, loss1 = _accuracy_and_loss(after, y)
    return dict(n=N, epochs=fit.epochs_done(), loss_before=loss0, loss_after=loss1, acc_before=acc0, acc_after=acc1,
                fit_losses=losses.cpu().numpy(), status=fit.status(), **({} if align_record is None else {"align": align_record}),
                **spatial_report)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m nsd_amd.calibrate", description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", action="append", required=True, help="a checkpoint (.pth); several --model: an ensemble, calibrated together")
    ap.add_argument("--data", required=True, help="directory with <prefix>_*.csv trials of the new session, or a packed .npz of them")
    ap.add_argument("--x-key", default="x", help="array of the windows inside a packed .npz")
    ap.add_argument("--classes", type=int, default=3, choices=(3, 5))
    ap.add_argument("--sr", type=int, default=125)
    ap.add_argument("--model-rate", type=float, default=None, metavar="HZ",
                    help="the rate the model decides at, where --sr is another and the checkpoint records no rate conversion: one is "
                         "designed (Resample.design) and the trials go through it on the device (default: the checkpoint's, or none)")
    ap.add_argument("--T", type=int, default=625, help="samples per trial")
    ap.add_argument("--calib-per-class", type=int, default=4, help="cued trials per class the read-out is fitted on; the rest is held out")
    ap.add_argument("--seed", type=int, default=0, help="which trials calibrate (a seeded permutation per class)")
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--weight-decay", type=float, default=0.0)
    ap.add_argument("--train", default="ln,fc0,fc3", help="tensor groups to fit, of ln, fc0, fc3")
    ap.add_argument("--label-smoothing", type=float, default=0.0)
    ap.add_argument("--head-dropout", type=float, default=None, help="train-mode noise of the head during the fit (default: eval-mode fit)")
    ap.add_argument("--align", action="store_true", help="refit the session alignment of a checkpoint that carries one (nsd_align) from the "
                    "calibration trials, label-free, before the read-out is fitted (without it the checkpoint's matrix stays)")
    ap.add_argument("--fit-spatial", action="store_true", help="fit the alignment matrix on the labelled calibration trials by gradient "
                    "descent through the frozen model (align.SpatialFit), behind --align's label-free refit and before the read-out is "
                    "fitted; a checkpoint without nsd_align gains a matrix that starts at the identity; with several --model ONE matrix is fitted "
                    "through all members (align.EnsembleSpatialFit) and every member's checkpoint carries it")
    ap.add_argument("--spatial-epochs", type=int, default=50, help="a choice, not tuned on held-out data")
    ap.add_argument("--spatial-lr", type=float, default=1e-2, help="a choice, not tuned on held-out data")
    ap.add_argument("--spatial-decay", type=float, default=1e-2, help="pull towards the matrix the fit starts from; a choice")
    ap.add_argument("--out", required=True, help="calibrated checkpoint; with several --model: <out stem>_m<i>.pth per member")
    return ap


def split_calibration(y: np.ndarray, per_class: int, seed: int):
    """(calibration indices, held-out indices): per class a seeded permutation's first `per_class` trials calibrate"""
    rs = np.random.RandomState(seed)
    cal = []
    for k in sorted(set(int(v) for v in y)):
        idx = np.flatnonzero(y == k)
        cal.extend(int(i) for i in rs.permutation(idx)[:per_class])
    cal = np.array(sorted(cal), dtype=np.int64)
    return cal, np.setdiff1d(np.arange(len(y)), cal)


def main(argv=None) -> int:
    from .data import LABELS_5CLASS, load_trials, load_trials_npz
    from .multimodel import EnsemblePredictor
    from .lstm_eeg_model import SimplePredictor
    from .trainer import save_reference_checkpoint
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.calib_per_class < 1:
        ap.error("--calib-per-class must be at least 1")
    if not torch.cuda.is_available():
        print("calibrate: needs an MI355X (no CPU path)", file=sys.stderr)
        return 2
    label_map = LABELS_5CLASS if args.classes == 5 else None
    ts = load_trials_npz(args.data, label_map, x_key=args.x_key) if args.data.endswith(".npz") else load_trials(args.data, label_map, samples=args.T)
    kw = dict(num_classes=args.classes, preprocess="identity")
    if args.model_rate is not None:
        kw["model_rate"] = args.model_rate
    pred = EnsemblePredictor(args.model, args.sr, **kw) if len(args.model) > 1 else SimplePredictor(args.model[0], args.sr, **kw)
    cal, held = split_calibration(ts.y, args.calib_per_class, args.seed)
    if len(cal) > 256:
        ap.error(f"{len(cal)} calibration trials: one launch takes up to 256")

    def held_out_accuracy():
        if not len(held):
            return None
        probs, _ = pred.predict_windows(ts.x[held].reshape(-1, ts.x.shape[-1]), ts.x.shape[1])
        return float((probs.argmax(1) == ts.y[held]).mean())

    acc0 = held_out_accuracy()
    loss = Loss(label_smoothing=args.label_smoothing) if args.label_smoothing else None
    spatial = dict(epochs=args.spatial_epochs, lr=args.spatial_lr, decay=args.spatial_decay) if args.fit_spatial else None
    if spatial is not None and len(args.model) > 1:
        spatial["shared"] = True                              # an ensemble's decoders share one matrix: one fit through all members
    rep = pred.calibrate(ts.x[cal], ts.y[cal], spatial=spatial, epochs=args.epochs, lr=args.lr, weight_decay=args.weight_decay,
                         train=tuple(s for s in args.train.split(",") if s), head_dropout=args.head_dropout, loss=loss, seed=args.seed, align=args.align)
    acc1 = held_out_accuracy()
    members = getattr(pred, "members", None) or [pred.model]
    stem, ext = os.path.splitext(args.out)
    outs = [args.out] if len(members) == 1 else [f"{stem}_m{i}{ext or '.pth'}" for i in range(len(members))]
    for m, path in zip(members, outs):
        save_reference_checkpoint(m, path)
    print(json.dumps(dict(models=len(members), calib_trials=int(len(cal)), held_out_trials=int(len(held)), epochs=rep["epochs"],
                          calib_loss_before=rep["loss_before"], calib_loss_after=rep["loss_after"], calib_acc_before=rep["acc_before"],
                          calib_acc_after=rep["acc_after"],
                          **({"spatial_loss_first": float(rep["spatial_losses"][0]), "spatial_loss_last": float(rep["spatial_losses"][-1]),
                              "spatial_status": rep["spatial_status"], "calib_acc_spatial": rep["acc_spatial"]} if args.fit_spatial else {}),
                          held_out_acc_before=acc0, held_out_acc_after=acc1, status=rep["status"],
                          out=outs)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
