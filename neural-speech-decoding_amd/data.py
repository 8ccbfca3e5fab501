"""Trial loader for the reference's recorded data set (EEG_data_collection/*.csv).

On-disk format (written by the reference's Neural_decoding_data_collector.py:129-139): one file per trial,
no header, comma-separated `%.7f` floats, 625 rows (5 s @ 125 Hz) x 8 channels, already band-limited and
zero-mean.  The class is the file-name prefix before the first '_'
(backgroundnoise / food / no / water / yes) -- the prefix is the only label carrier.

The whole data set is 324 x 20 KB = 6.5 MB: it is parsed once, kept as one [N,625,8] fp32 array (optionally
cached as .npz next to the CSVs) and moved to HBM in full; there is no per-step I/O.
"""
from __future__ import annotations

import glob
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

PREFIXES = ("backgroundnoise", "food", "no", "water", "yes")

# Explicit label maps (the reference's own naming is inconsistent, SURVEY 6 / BASELINE.md 2):
#  * LABELS_3CLASS_CHECKPOINT: the order the shipped checkpoint was evidently trained with (its file name
#    says Water_Food_Bg_Noise; with this order the reference reproduces its ~70 % claim)
#  * LABELS_3CLASS_CODE: the order of CLASS_NAMES in the reference code (Food, Water, BG-Noise)
LABELS_3CLASS_CHECKPOINT: Dict[str, int] = {"water": 0, "food": 1, "backgroundnoise": 2}
LABELS_3CLASS_CODE: Dict[str, int] = {"food": 0, "water": 1, "backgroundnoise": 2}
LABELS_5CLASS: Dict[str, int] = {"yes": 0, "no": 1, "food": 2, "water": 3, "backgroundnoise": 4}


@dataclass
class TrialSet:
    x: np.ndarray            # [N, T, C] float32
    y: np.ndarray            # [N] int32 class index under `label_map`
    prefix: List[str]        # file-name prefix of each trial
    files: List[str]
    label_map: Dict[str, int]

    def __len__(self) -> int:
        return int(self.x.shape[0])

    @property
    def num_classes(self) -> int:
        return len(set(self.label_map.values()))


def parse_trial_csv(path: str) -> np.ndarray:
    """[T, C] float32 from one trial file."""
    a = np.loadtxt(path, delimiter=",", dtype=np.float64, ndmin=2)
    return a.astype(np.float32)


def prefix_of(path: str) -> str:
    return os.path.basename(path).split("_", 1)[0].lower()


def load_trials(directory: str, label_map: Optional[Dict[str, int]] = None, *, samples: int = 625, channels: int = 8,
                cache: bool = False) -> TrialSet:
    """Parse every `<prefix>_*.csv` under `directory` whose prefix is in `label_map` (default: the 3-class map of
    the shipped checkpoint).  Files with another shape than [samples, channels] are rejected loudly."""
    label_map = dict(LABELS_3CLASS_CHECKPOINT if label_map is None else label_map)
    files = sorted(f for f in glob.glob(os.path.join(directory, "*.csv")) if prefix_of(f) in label_map)
    if not files:
        raise FileNotFoundError(f"no trial CSVs with prefixes {sorted(label_map)} under {directory!r}")
    cache_path = os.path.join(directory, f".nsd_cache_{samples}x{channels}_{len(files)}.npz")
    x = None
    if cache and os.path.exists(cache_path):
        z = np.load(cache_path, allow_pickle=False)
        if list(z["files"]) == [os.path.basename(f) for f in files]:
            x = z["x"]
    if x is None:
        x = np.empty((len(files), samples, channels), np.float32)
        for i, f in enumerate(files):
            a = parse_trial_csv(f)
            if a.shape != (samples, channels):
                raise ValueError(f"{f}: expected [{samples},{channels}] got {a.shape}")
            x[i] = a
        if cache:
            try:
                np.savez(cache_path, x=x, files=np.array([os.path.basename(f) for f in files]))
            except OSError:
                pass                      # read-only data directory: just skip the cache
    prefix = [prefix_of(f) for f in files]
    y = np.array([label_map[p] for p in prefix], np.int32)
    return TrialSet(x=x, y=y, prefix=prefix, files=files, label_map=label_map)


def load_trials_npz(path: str, label_map: Optional[Dict[str, int]] = None, x_key: str = "x") -> TrialSet:
    """The same TrialSet from a packed copy of the data set (`x` [N,T,C] float32, `stem` [N] and optionally `prefix` [N]; written
    by tests/golden/make_trials_fixture.py with load_trials itself) -- the form in which the recorded trials travel to
    machines that do not hold the CSV directory.  `x_key`: the array holding the windows (`x_filt` in
    tests/golden/recorded_trials_filtered.npz: the same trials as the reference's PreProcessor hands them to the model)."""
    label_map = dict(LABELS_3CLASS_CHECKPOINT if label_map is None else label_map)
    z = np.load(path, allow_pickle=False)
    if x_key not in z.files:
        raise KeyError(f"{path!r} has no array {x_key!r} (arrays: {z.files})")
    prefix_all = [str(p) for p in z["prefix"]] if "prefix" in z.files else [prefix_of(str(s)) for s in z["stem"]]
    keep = np.array([p in label_map for p in prefix_all])
    if not keep.any():
        raise FileNotFoundError(f"no trials with prefixes {sorted(label_map)} in {path!r}")
    prefix = [p for p, k in zip(prefix_all, keep) if k]
    files = [str(s) + ".csv" for s, k in zip(z["stem"], keep) if k]
    x = np.ascontiguousarray(z[x_key][keep], dtype=np.float32)
    y = np.array([label_map[p] for p in prefix], np.int32)
    return TrialSet(x=x, y=y, prefix=prefix, files=files, label_map=label_map)


def stratified_folds(y: Sequence[int], k: int, seed: int = 0) -> List[np.ndarray]:
    """k disjoint validation index sets covering every trial once, each with (nearly) the class proportions of the whole set."""
    y = np.asarray(y)
    rs = np.random.RandomState(seed)
    folds: List[List[int]] = [[] for _ in range(k)]
    for cls in np.unique(y):
        idx = np.flatnonzero(y == cls)
        rs.shuffle(idx)
        for i, v in enumerate(idx):
            folds[i % k].append(int(v))
    return [np.sort(np.array(f, dtype=np.int64)) for f in folds]


def stratified_split(y: Sequence[int], val_fraction: float = 0.2, seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """Indices (train, val): every class contributes round(val_fraction * count) trials to the validation set."""
    y = np.asarray(y)
    rs = np.random.RandomState(seed)
    tr, va = [], []
    for cls in np.unique(y):
        idx = np.flatnonzero(y == cls)
        rs.shuffle(idx)
        k = int(round(val_fraction * idx.size))
        va.append(idx[:k]); tr.append(idx[k:])
    return np.sort(np.concatenate(tr)), np.sort(np.concatenate(va))


def epoch_batches(n: int, batch: int, seed: int, epoch: int, drop_last: bool = False):
    """Shuffled index batches of one epoch (same permutation on every rank: seed + epoch)."""
    perm = np.random.RandomState(seed + 1000003 * epoch).permutation(n)
    for lo in range(0, n, batch):
        idx = perm[lo:lo + batch]
        if drop_last and idx.size < batch:
            break
        yield idx


# ---- device-resident trials and the run's index schedule (nsd_gather of include/nsd.h) --------------------------------------------------
class DeviceTrialSet:
    """The trials of a run resident on the device: x [N,T,C] fp32 and either int32 labels [N] (an integer y) or fp32 target rows [N,K]
    (a floating-point y).  Trainer.bind_batches / ModelBatchTrainer.bind_batches gather every step's batch from it on the device."""

    def __init__(self, x, y_or_targets, device):
        import torch
        x = torch.as_tensor(x)
        y = torch.as_tensor(y_or_targets)
        if x.dim() != 3 or x.shape[0] < 1:
            raise ValueError(f"DeviceTrialSet: x must be [N,T,C] with N >= 1, got {tuple(x.shape)}")
        self.x = x.to(device=device, dtype=torch.float32).contiguous()
        self.labels = self.targets = None
        if y.is_floating_point():
            if y.dim() != 2 or y.shape[0] != x.shape[0]:
                raise ValueError(f"DeviceTrialSet: target rows must be [N,K] = [{x.shape[0]},K], got {tuple(y.shape)}")
            self.targets = y.to(device=device, dtype=torch.float32).contiguous()
        else:
            if y.dim() != 1 or y.shape[0] != x.shape[0]:
                raise ValueError(f"DeviceTrialSet: labels must be [N] = [{x.shape[0]}], got {tuple(y.shape)}")
            self.labels = y.to(device=device, dtype=torch.int32).contiguous()

    def __len__(self) -> int:
        return int(self.x.shape[0])

    @property
    def y(self):
        """the labels, or the target rows"""
        return self.labels if self.labels is not None else self.targets


class BatchSchedule:
    """The index schedule of a run: table int32 [M][S][B] -- row s of model m holds the trial indices (into the DeviceTrialSet) of that
    model's batch in step s -- and steps_per_epoch.  The constructors restate the host loops of nsd_amd.train: a run through a schedule
    sees the batches its host loop would have indexed, in the same order."""

    def __init__(self, table, steps_per_epoch: int):
        table = np.ascontiguousarray(table)
        if table.ndim != 3 or table.shape[0] < 1 or table.shape[1] < 1 or table.shape[2] < 1:
            raise ValueError(f"BatchSchedule: table must be [M,S,B] with M, S, B >= 1, got {table.shape}")
        if not np.issubdtype(table.dtype, np.integer):
            raise ValueError(f"BatchSchedule: table holds {table.dtype}, not trial indices")
        if table.min() < 0 or table.max() > 0x7fffffff:
            raise ValueError("BatchSchedule: a trial index is negative or above 2^31 - 1")
        if steps_per_epoch < 1 or table.shape[1] % steps_per_epoch:
            raise ValueError(f"BatchSchedule: {table.shape[1]} rows are no whole number of epochs of {steps_per_epoch} steps")
        self.table, self.steps_per_epoch = table.astype(np.int32), int(steps_per_epoch)

    M = property(lambda self: int(self.table.shape[0]))
    steps = property(lambda self: int(self.table.shape[1]))
    batch = property(lambda self: int(self.table.shape[2]))
    epochs = property(lambda self: self.steps // self.steps_per_epoch)

    def check_trials(self, n: int) -> None:
        """ValueError unless every index names one of n trials"""
        if int(self.table.max()) >= n:
            raise ValueError(f"BatchSchedule: trial index {int(self.table.max())} for a set of {n} trials")

    @staticmethod
    def _rows(tr_idx, batch: int, seed: int, epochs: int, drop_last: bool, who: str):
        tr_idx = np.asarray(tr_idx)
        n = len(tr_idx)
        if batch < 1 or epochs < 1:
            raise ValueError(f"{who}: batch {batch}, epochs {epochs} (both >= 1)")
        if n < batch:
            raise ValueError(f"{who}: {n} trials are fewer than one batch of {batch}: the run's only batch is a short one, which a "
                             "schedule of equal rows cannot hold (such a run keeps the host loop)")
        if not drop_last and n % batch:
            raise ValueError(f"{who}: drop_last=False leaves a short tail batch of {n % batch} trials ({n} trials, batch {batch}), which "
                             "a schedule of equal rows cannot hold (drop it, or choose a batch that divides the trials)")
        return [tr_idx[idx] for e in range(epochs) for idx in epoch_batches(n, batch, seed, e, drop_last=True)]

    @classmethod
    def for_run(cls, tr_idx, batch: int, seed: int, epochs: int, drop_last: bool = True) -> "BatchSchedule":
        """The steps of nsd_amd.train's fit(): tr_idx[idx] for idx in epoch_batches(len(tr_idx), batch, seed, e, drop_last=True),
        e = 0 .. epochs - 1."""
        rows = cls._rows(tr_idx, batch, seed, epochs, drop_last, "BatchSchedule.for_run")
        return cls(np.stack(rows)[None], len(rows) // epochs)

    @classmethod
    def for_runs(cls, runs, batch: int, epochs: int) -> "BatchSchedule":
        """The steps of nsd_amd.train's concurrent_epoch: runs is a sequence of dicts with `tr` (the run's trial indices) and `seed`;
        step j of epoch e gives run k the j-th batch of epoch_batches(len(tr_k), batch, seed_k, e, drop_last=True)."""
        if len(runs) < 1:
            raise ValueError("BatchSchedule.for_runs: no runs")
        per = [cls._rows(r["tr"], batch, r["seed"], epochs, True, f"BatchSchedule.for_runs: run {k}") for k, r in enumerate(runs)]
        counts = sorted({len(p) for p in per})
        if len(counts) > 1:
            raise ValueError(f"BatchSchedule.for_runs: the runs draw {[c // epochs for c in counts]} batches of {batch} per epoch; one "
                             "shared step needs the same count for every run")
        return cls(np.stack([np.stack(p) for p in per]), counts[0] // epochs)


def screen_trials(x, gate) -> Tuple[np.ndarray, np.ndarray]:
    """Signal quality of every trial of a set under the SignalGate `gate`: x [N,T,C] -> (bad_fraction float64 [N,C]: the share of each
    channel's samples the gate calls bad, rejected_fraction float64 [N]: the share of steps with more than gate.max_bad bad channels).
    A device tensor goes through one window-mode nsd_gate_step over the whole set (every trial from a reset state); a numpy array or a
    host tensor through the gate's numpy restatement, which gives the same mask words.  train's --gate-drop-trials drops the trials
    whose rejected fraction exceeds a bound, before the folds are made."""
    import torch
    if torch.is_tensor(x) and x.is_cuda:
        from . import ops
        if x.dim() != 3:
            raise ValueError(f"screen_trials: x must be [N,T,C], got {tuple(x.shape)}")
        N, T, Cc = (int(v) for v in x.shape)
        if N == 0:
            return np.zeros((0, Cc)), np.zeros((0,))
        _, mask = ops.gate_step(x.contiguous().float(), gate)
        bits = (mask[..., None] >> torch.arange(32, dtype=torch.int32, device=x.device)) & 1          # [N,T,32]
        bad = bits[..., :Cc].sum(1, dtype=torch.int64).cpu().numpy()
        rejected = (bits.sum(2) > int(gate.max_bad)).sum(1, dtype=torch.int64).cpu().numpy()
    else:
        xs = np.asarray(x.numpy() if torch.is_tensor(x) else x, np.float32)
        if xs.ndim != 3:
            raise ValueError(f"screen_trials: x must be [N,T,C], got {xs.shape}")
        N, T, Cc = xs.shape
        if N == 0:
            return np.zeros((0, Cc)), np.zeros((0,))
        _, mask = gate.reference(xs)
        bits = (mask[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
        bad = bits[..., :Cc].sum(1, dtype=np.int64)
        rejected = (bits.sum(2, dtype=np.int64) > int(gate.max_bad)).sum(1, dtype=np.int64)
    return bad / float(T), rejected / float(T)
