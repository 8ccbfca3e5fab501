"""numpy float64 restatement of nsd_multi_eval (include/nsd.h): the held-out metrics of one model from its logits, and the early-stopping
rule as a state machine over a sequence of evaluations.  Used by tests/test_eval_cpu.py (pinned to torch there) and
tests/test_gpu_eval.py (the kernel against it).

  row_losses(logits, labels)          per row: loss = log(sum_k exp(l_k - max)) + max - l_y in double from the fp32 logits (k ascending),
                                      the first maximal index, and whether the row counts (finite logits, label in [0, K))
  eval_record(logits, labels, count)  one model's record: only the first `count` rows count; a counted row that does not count as
                                      finite goes to `nonfinite` alone and makes loss_sum NaN; loss_sum in the kernel's order: lane i of
                                      256 sums rows i, i + 256, ... ascending, then a halving tree over the lanes
  Selector(M, metric, patience, min_delta).offer(records)
                                      the rule per model; .records are the select records, .held[m] the 0-based index of the offer whose
                                      parameters model m's snapshot holds (None: never written)
  pack_eval / pack_select             the records as the bytes of nsd_eval_record / nsd_select_record
"""
from __future__ import annotations

import struct

import numpy as np

LANES = 256
MAX_K = 8
EVAL_BYTES, SELECT_BYTES = 280, 40


def row_losses(logits, labels):
    lg = np.asarray(logits, dtype=np.float32)
    y = np.asarray(labels).astype(np.int64)
    B, K = lg.shape
    ok = np.isfinite(lg).all(axis=1) & (y >= 0) & (y < K)
    l64 = np.where(ok[:, None], lg, np.float32(0)).astype(np.float64)
    ys = np.where(ok, y, 0)
    mx = l64.max(axis=1)
    e = np.zeros(B)
    for k in range(K):
        e = e + np.exp(l64[:, k] - mx)
    loss = (np.log(e) + mx) - l64[np.arange(B), ys]
    pred = np.argmax(l64, axis=1)                      # numpy's argmax returns the first maximal index
    return loss, pred, ok


def lane_tree_sum(values) -> float:
    """sum of `values` in the kernel's order: lane i takes elements i, i + LANES, ... ascending, then lane i += lane i + s, s = 128 .. 1"""
    v = np.asarray(values, dtype=np.float64)
    trips = max((len(v) + LANES - 1) // LANES, 1)
    pad = np.zeros(trips * LANES)
    pad[:len(v)] = v
    lanes = np.zeros(LANES)
    for t in range(trips):
        lanes = lanes + pad[t * LANES:(t + 1) * LANES]
    s = LANES // 2
    while s >= 1:
        lanes[:s] = lanes[:s] + lanes[s:2 * s]
        s //= 2
    return float(lanes[0])


def eval_record(logits, labels, count=None) -> dict:
    lg = np.asarray(logits, dtype=np.float32)
    B, K = lg.shape
    count = B if count is None else int(count)
    loss, pred, ok = row_losses(lg[:count], np.asarray(labels)[:count])
    y = np.asarray(labels)[:count].astype(np.int64)
    conf = np.zeros((MAX_K, MAX_K), dtype=np.int64)
    np.add.at(conf, (y[ok], pred[ok]), 1)
    nonfinite = int((~ok).sum())
    # a row that does not count adds nothing; the lanes keep their places (row r is lane r % 256 whether or not its neighbours count)
    loss_sum = float("nan") if nonfinite else lane_tree_sum(np.where(ok, loss, 0.0))
    return dict(loss_sum=loss_sum, n=int(ok.sum()), correct=int((pred[ok] == y[ok]).sum()), nonfinite=nonfinite, confusion=conf)


def pack_eval(r: dict) -> bytes:
    return struct.pack("<d4i64i", r["loss_sum"], r["n"], r["correct"], r["nonfinite"], 0, *[int(v) for v in np.asarray(r["confusion"]).reshape(-1)])


def unpack_eval(raw: bytes) -> dict:
    v = struct.unpack("<d4i64i", raw)
    return dict(loss_sum=v[0], n=v[1], correct=v[2], nonfinite=v[3], confusion=np.array(v[5:], dtype=np.int64).reshape(MAX_K, MAX_K))


def new_select_record() -> dict:
    return dict(best_loss=0.0, best_correct=0, best_n=0, best_eval=0, evals=0, bad=0, stopped=0, status=0)


def pack_select(r: dict) -> bytes:
    return struct.pack("<d5i3I", r["best_loss"], r["best_correct"], r["best_n"], r["best_eval"], r["evals"], r["bad"], r["stopped"], r["status"], 0)


def unpack_select(raw: bytes) -> dict:
    v = struct.unpack("<d5i3I", raw)
    return dict(zip(("best_loss", "best_correct", "best_n", "best_eval", "evals", "bad", "stopped", "status"), v[:8]))


class Selector:
    """The early-stopping rule of include/nsd.h for M models.  min_delta is rounded to fp32 first (it travels as a float) and widened
    exactly; every comparison is in double."""

    def __init__(self, M: int, metric: str = "loss", patience: int = 0, min_delta: float = 0.0):
        assert metric in ("loss", "acc")
        self.M, self.metric, self.patience = int(M), metric, int(patience)
        self.min_delta = float(np.float32(min_delta))
        self.records = [new_select_record() for _ in range(self.M)]
        self.held = [None] * self.M
        self.offers = 0

    def offer(self, evals) -> list:
        """evals: M dicts with loss_sum, n, correct -> per model: did it improve (its snapshot is then this offer's parameters)"""
        improved = []
        for m, (r, e) in enumerate(zip(self.records, evals)):
            better = False
            if not r["stopped"]:
                r["evals"] += 1
                n = int(e["n"])
                with np.errstate(all="ignore"):
                    mean = float(np.float64(e["loss_sum"]) / np.float64(n))
                if n <= 0 or not np.isfinite(mean):
                    r["status"] |= 1
                elif r["best_eval"] == 0:
                    better = True
                elif self.metric == "loss":
                    better = mean < r["best_loss"] - self.min_delta
                else:
                    acc, best_acc = e["correct"] / n, r["best_correct"] / r["best_n"]
                    better = acc > best_acc + self.min_delta or (acc == best_acc and mean < r["best_loss"])
                if better:
                    r.update(best_loss=mean, best_correct=int(e["correct"]), best_n=n, best_eval=r["evals"], bad=0)
                    self.held[m] = self.offers
                else:
                    r["bad"] += 1
                    if self.patience > 0 and r["bad"] >= self.patience:
                        r["stopped"] = 1
            improved.append(better)
        self.offers += 1
        return improved
