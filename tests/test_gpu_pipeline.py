"""The whole training front end -- gather -> augment (+ z-score) -> gate -> prep -> gate-apply -> align -> crop (+ z-score on the crops) ->
mixup / target rows -- held to ONE composed reference (tests/pipeline_ref.py) on the MI355X, in every mode that drives it: Trainer.step,
Trainer.step_static, Trainer.step_scheduled (eager and static) and ModelBatchTrainer (one setting, and per-model lists).

Two layers per row of pipeline_ref.CASES, both BIT FOR BIT (the file holds no tolerance):
  A  StepRecipe.prepare (behind StepRecipe.gather for bound rows; into the static buffers and from the device step counter in the static
     modes) at steps 1, 2, 3 against prepare_ref -- windows and labels / target rows as uint32 words -- with the caller's inputs, the
     resident set and the schedule table checked unchanged;
  B  the trainer under test, three steps in its row's mode with the row's stages and tail, against plain Trainer(s) -- same weights, seed,
     dropout and tail, no front end -- stepping on layer A's REFERENCE windows and labels / rows: parameters, both Adam moments,
     last_loss, and where the tail has them the averaged weights, the SAM record and the skipped-step count, after every step.  Between
     steps 1 and 2 a second schedule of the same shape is bound (a captured graph survives and reads row 0); in front of step 3 the
     static inputs are refilled, as before every step, and set_alignment writes new matrices.
The plain trainers step eagerly: float target rows (every row with a loss) exist for Trainer.step only.

Measured on one MI355X: 35 rows, 71 tests (two layers per row and the timing line), 1.6 s from import to the last test (pytest: 3.3 s
with start-up); the slowest test 0.4 s (the first, which loads the kernels).  Every one of the 612 tensor and 210 word comparisons is exact.

That the rows bite: seven Python-only mutants of step_recipe.py, each made to compute something else (never another launch dimension
or buffer size: every launcher checks the sizes it is handed), each built once, run once against this file and once against the
pre-existing GPU files of the touched feature, and never committed.  Rows by their number in pipeline_ref.CASES; a row that fails
fails in both layers.
  mutant                                              rows of this file that fail                        the older GPU files
  (a) align in front of gate-apply                    00-04 10 12 15 17 18 23 26 29 (every gate+align)   test_gpu_align, test_gpu_gate: all pass
  (b) crop in front of align                          none: the same bits, see below                     test_gpu_align, test_gpu_crop: all pass
  (c) fresh=True always in align_apply's call         32 33 (align as the first stage: the caller's      test_gpu_align: the trainer test fails
                                                      windows / the static input are written)
  (d) mixup's streams taken from step + 1             00 03 04 05 13 18 25 (every eager and              test_gpu_soft_targets: 5 fail
                                                      model-batched mix row; a replayed step reads
                                                      the device counter and is not touched by it)
  (e) the front end run again for SAM's second pass   10 15 27 30 (every SAM row without a crop)         test_gpu_sam: all pass
  (f) the crops' z-score skipped behind an augment    05 08 16 25 28 (every normalize+crop+augment)      test_gpu_crop: 1 fails (launch sequence)
  (g) every model's rows aligned with matrix 0        03 04 07 15 18 23 26 (every model-batched align)   test_gpu_align: the trainer test fails
(b) is an equivalent mutant on the device: nsd_crop copies samples and nsd_spatial_apply acts on one time step at a time, so cutting
first and aligning the crops gives the same bits -- all 71 tests of this file and the older files pass under it.  Only the launch order
tells the two apart, and the order is held on the host: tests/test_pipeline_cpu.py fails under (b) in the thirteen rows with both
stages on (and under (a), (c)-(f) in the rows above; under (g) by its selection check).
(e) as a fused two-pass launch lets Python express it: with sam= the step trains on prepare(prepare(x)) where the windows keep their
shape.  Calling prepare() a second time on the SAME input is no mutant at all -- the streams are counter-based, so it draws what the
first call drew, which is the documented reason both passes may share one batch.
"""
import time

import numpy as np
import pytest
import torch

from tests import pipeline_ref as pl
from tests.buffer_contract import snapshot
from tests.gpu_harness import dev, nsd, sync_at_the_end, to_dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

IDS = [pl.case_id(c) for c in pl.CASES]
LR = 1e-3
_T0 = time.perf_counter()
_REF = {}


def _reference(c, dev):
    """prepare_ref for the row's three steps, computed once and shared by both layers; the z-score link is the kernel (pipeline_ref)"""
    if c.id not in _REF:
        from nsd_amd import ops
        _REF[c.id] = pl.reference(c, zscore=lambda a: ops.zscore(to_dev(a, dev)).cpu().numpy())
    return _REF[c.id]


def _words(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _same_words(tag, what, got, want):
    g, w = _words(got).reshape(-1), _words(want).reshape(-1)
    diff = int((g != w).sum()) if g.shape == w.shape else -1
    print(f"[{tag}] {what}: {g.size} words, {diff} differ")
    assert diff == 0, (tag, what)


def _models(nsd, dev, c, st):
    """the row's model(s) with their front end, and plain twins on the same weights and dropout"""
    inp = pl.inputs(c)
    mine, plain = [], []
    for m, p in enumerate(st["dropouts"]):
        torch.manual_seed(1000 * c.id + m)
        a = nsd.EEG_LSTM(dropout=p, **st["model"]).to(dev).train()
        if c.align:
            W = inp["align"][1]
            a.set_alignment(to_dev(W if W.ndim == 2 else W[m], dev))
        b = nsd.EEG_LSTM(dropout=p).to(dev).train()
        b.load_state_dict(a.state_dict(), strict=True)
        mine.append(a)
        plain.append(b)
    return mine, plain


def _trainer(nsd, c, st, models):
    from nsd_amd.trainer import Trainer
    if pl.models_of(c) == 1:
        return Trainer(models[0], lr=LR, seed=pl.SEEDS[0], **st["trainer"])
    return nsd.ModelBatchTrainer(models, lr=LR, seeds=list(pl.SEEDS), **st["trainer"])


class _Feed:
    """the row's inputs on the device and what changes between its steps: the bound schedule (A in front of step 1, B in front of step
    2) and the alignment matrices (new ones in front of step 3)"""

    def __init__(self, nsd, dev, c, tr, models):
        from nsd_amd.data import BatchSchedule, DeviceTrialSet
        self.c, self.tr, self.models, self.dev, self.inp = c, tr, models, dev, pl.inputs(c)
        self.held = []                                   # the caller's tensors: no step may write them
        if c.source == "bound":
            xa, ya = self.inp["trials"]
            self.trials = DeviceTrialSet(xa, ya, dev)
            self.schedules = [BatchSchedule(t, pl.S) for t in self.inp["schedules"]]
            self.held += [self.trials.x, self.trials.y]
        else:
            self.x = {s: to_dev(self.inp["x"][s], dev) for s in pl.STEPS}
            self.y = {s: to_dev(self.inp["y"][s], dev) for s in pl.STEPS}

    def before(self, step):
        """-> the tensors that must come through the step unchanged"""
        c, tr = self.c, self.tr
        if c.source == "bound" and step in (1, 2):
            assert tr.step_count == step - 1
            graphs = dict(getattr(tr, "_graphs", {}))
            tr.bind_batches(self.trials, self.schedules[step - 1])
            if step == 2 and c.mode == "sched" and graphs:
                assert tr._graphs == graphs, "the captured graph did not survive a schedule of the bound shape"
        if c.align and step == 3:
            W = to_dev(self.inp["align"][3], self.dev)
            tr.set_alignment(W) if pl.models_of(c) > 1 else self.models[0].set_alignment(W)
        held = list(self.held)
        if c.source == "bound":
            held.append(tr._bound["table"])
        elif c.mode == "static":
            x, y = tr.static_inputs(pl.B, pl.T)
            x.copy_(self.x[step])
            y.copy_(self.y[step])
            held += [x, y]
        else:
            held += [self.x[step], self.y[step]]
        return held


def _prepare(c, tr, feed, step):
    """StepRecipe.prepare (and gather) as the row's mode drives them -> (windows, labels, targets)"""
    n, recipe = pl.models_of(c), tr.recipe
    seeds = tr.seeds if n > 1 else [tr.seed]
    if c.mode in ("static", "sched"):
        tr.static_inputs(pl.B, pl.T)
        buf = tr._buffers(*recipe.dims(pl.B, pl.T))
        tr._step_dev.fill_(step)
        if c.mode == "sched":
            recipe.gather(tr._bound, 0, step_dev=tr._step_dev, x=buf["x"], y=buf["y"])
        return recipe.prepare(buf["x"], buf["y"], seeds, 0, step_dev=tr._step_dev, bufs=buf)
    if c.source == "bound":
        x, y = recipe.gather(tr._bound, step)
        if n > 1:
            x, y = x.view(n, pl.B, pl.T, -1), y.view(n, pl.B)
    else:
        x, y = feed.x[step], feed.y[step]
    if n > 1:                                            # as ModelBatchTrainer.step hands them over
        y = (y.unsqueeze(0).expand(n, pl.B) if y.dim() == 1 else y).contiguous().view(-1)
    return recipe.prepare(x, y, seeds, step, M=n)


@pytest.mark.parametrize("c", pl.CASES, ids=IDS)
def test_the_kernels_chain_equals_the_composed_reference(nsd, dev, c):
    st, ref, n = pl.settings(c), _reference(c, dev), pl.models_of(c)
    models, _ = _models(nsd, dev, c, st)
    tr = _trainer(nsd, c, st, models)
    feed = _Feed(nsd, dev, c, tr, models)
    for step in pl.STEPS:
        held = feed.before(step)
        snap = snapshot(*held)
        x, labels, targets = _prepare(c, tr, feed, step)
        torch.cuda.synchronize()
        tr.step_count = step                             # (what the step itself would have counted: the next binding names its row by it)
        w, lab, tg, trace = ref[step]
        tag = f"{pl.case_id(c)} step {step}"
        print(f"[{tag}] stages that acted: {[k for k in pl.STAGES if k in trace]}")
        _same_words(tag, "windows", x.reshape(w.shape), w)
        if lab is not None:
            assert targets is None and labels.dtype == torch.int32
            _same_words(tag, "labels", labels.reshape(lab.shape), lab)
        else:
            assert labels is None and targets.dtype == torch.float32
            _same_words(tag, "target rows", targets.reshape(tg.shape), tg)
        changed = snap.changed()
        print(f"[{tag}] inputs / resident set / schedule table written: {changed}")
        assert changed == []
        if c.source == "bound":
            assert tr._bound["status"].cpu().tolist() == [0] * n


def _step(c, tr, feed, step):
    if c.source == "bound":
        tr.step_scheduled(static=True) if c.mode == "sched" else tr.step_scheduled()
    elif c.mode == "static":
        tr.step_static(pl.B, pl.T)
    else:
        tr.step(feed.x[step], feed.y[step])


@pytest.mark.parametrize("c", pl.CASES, ids=IDS)
def test_the_trainer_equals_plain_trainers_on_the_reference_windows(nsd, dev, c):
    from nsd_amd.trainer import Trainer
    st, ref, n = pl.settings(c), _reference(c, dev), pl.models_of(c)
    models, twins = _models(nsd, dev, c, st)
    tr = _trainer(nsd, c, st, models)
    plain = [Trainer(twins[m], lr=LR, seed=pl.SEEDS[m], **pl.plain_tail(c, m)) for m in range(n)]
    feed = _Feed(nsd, dev, c, tr, models)
    parts = pl.TAILS[c.tail]
    row = (lambda t: t) if n == 1 else None
    for step in pl.STEPS:
        held = feed.before(step)
        snap = snapshot(*held)
        _step(c, tr, feed, step)
        w, lab, tg, _ = ref[step]
        for m in range(n):
            plain[m].step(to_dev(w[m], dev), to_dev(lab[m] if lab is not None else tg[m], dev))
        torch.cuda.synchronize()
        tag = f"{pl.case_id(c)} step {step}"
        assert snap.changed() == [], tag
        losses = [tr.last_loss()] if n == 1 else tr.last_losses()
        skipped = [tr.skipped_steps()] if n == 1 else tr.skipped_steps()
        sams = ([tr.last_sam()] if n == 1 else tr.last_sams()) if "sam" in parts else None
        for m in range(n):
            p = plain[m]
            mine = dict(parameters=tr.flat if n == 1 else tr.params[m], adam_m=tr.m if n == 1 else tr.m[m], adam_v=tr.v if n == 1 else tr.v[m])
            theirs = dict(parameters=p.flat, adam_m=p.m, adam_v=p.v)
            if "avg" in parts:
                mine["averaged"] = tr.averaged_weights() if n == 1 else tr.averaged_params()[m]
                theirs["averaged"] = p.averaged_weights()
            for k in mine:
                eq = bool(torch.equal(mine[k], theirs[k]))
                print(f"[{tag}] model {m} {k}: {mine[k].numel()} floats, equal {eq}, largest difference "
                      f"{float((mine[k] - theirs[k]).abs().max()):.3e}")
                assert eq, (tag, m, k)
            pl_loss = p.last_loss()
            print(f"[{tag}] model {m} last_loss {losses[m]!r} vs {pl_loss!r}; skipped {skipped[m]} vs {p.skipped_steps()}")
            assert losses[m] == pl_loss and np.isfinite(pl_loss), (tag, m)
            assert skipped[m] == p.skipped_steps() == 0, (tag, m)
            if "avg" in parts:
                counts = tr.averaged_count() if n == 1 else tr.averaged_counts()[m]
                print(f"[{tag}] model {m} averaged steps {counts} vs {p.averaged_count()}")
                assert counts == p.averaged_count() == step, (tag, m)
            if sams is not None and p.sam is not None:
                print(f"[{tag}] model {m} SAM record {sams[m]} vs {p.last_sam()}")
                assert sams[m] == p.last_sam() and sams[m]["nonfinite"] == 0 and sams[m]["norm"] > 0, (tag, m)
        assert tr.step_count == step and all(p.step_count == step for p in plain)
    if c.mode in ("static", "sched"):
        assert len(tr._graphs) == 1, "one capture, three replays"


def test_wall_time_of_this_file():
    """(the last test) -- the figure the docstring records"""
    print(f"tests/test_gpu_pipeline.py: {len(pl.CASES)} rows, two layers each, {time.perf_counter() - _T0:.1f} s since the file was imported")
