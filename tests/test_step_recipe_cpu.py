"""The one step recipe (nsd_amd/step_recipe.py), the parts that need no GPU: the seed and stream literals of the formulas the trainers
used to spell out themselves, the stochastic policy, and StepRecipe.prepare driven as each of its three callers drives it (eager,
hipGraph replay, model-batched) with ops.augment / ops.mixup / ops.zscore replaced by recording stand-ins on CPU tensors."""
import glob
import os

import pytest
import torch

import nsd_amd
from nsd_amd import ops
from nsd_amd import step_recipe as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUG = nsd_amd.Augment(max_shift=3, scale_range=0.1, p_channel=0.2, noise_std=0.3)
STEPS = (1, 3, 2**30 - 1, 2**30, 2**30 + 5, 2**31 + 1)


def test_seed_literals():
    assert sr.trainer_seed(1234, 0) == 11400714819323199719
    assert sr.trainer_seed(1234, 1) == 4354685564936846588
    assert sr.trainer_seed(0, 0) == 11400714819323198485
    assert sr.trainer_seed(2**64 - 1, 7) == 17418742259747381415
    assert sr.trainer_seed(1234) == sr.trainer_seed(1234, 0)
    # ModelBatchTrainer's seed of model m was spelled (seeds[m] + golden ratio) mod 2^64: trainer_seed(seeds[m], 0), value for value
    # (tests/test_gpu_soft_targets.py checks it on an instance)
    for s in (0, 3, 1234, 2**63, 2**64 - 1):
        assert sr.trainer_seed(s, 0) == (s + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF


def test_stream_literals_and_slots():
    assert sr.base_stream(1) == 4 and sr.base_stream(2**30 - 1) == 4294967292
    assert sr.base_stream(2**30) == 0 and sr.base_stream(2**30 + 5) == 20
    for step in STEPS:                                  # EEG_LSTM's former 4 * step, as the uint32 ABI argument keeps it
        assert sr.base_stream(step) == (4 * step) & 0xFFFFFFFF, step
    assert (sr.SLOT_LSTM_DROPOUT, sr.SLOT_RRELU, sr.SLOT_HEAD_DROPOUT, sr.SLOT_AUGMENT) == (0, 1, 2, 3)
    assert sr.step_rng(9, 2**30 + 5, 0.6, 0.25) == dict(seed=9, base_stream=20, p_lstm=0.6, p_head=0.25)
    assert sr.step_rng(9, 1) == dict(seed=9, base_stream=4, p_lstm=0.0, p_head=0.0)


def test_one_definition_in_the_package():
    """The greps that say the copies are gone: the step mask and the golden-ratio constant once each (in step_recipe.py), one call
    site of ops.augment / ops.mixup outside ops.py, no direct library call in the trainers."""
    src = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(ROOT, "neural-speech-decoding_amd", "*.py"))}
    for needle in ("0x3FFFFFFF", "0x9E3779B97F4A7C15"):
        assert {n: s.count(needle) for n, s in src.items() if needle in s} == {"step_recipe.py": 1}, needle
    for needle in ("ops.augment(", "ops.mixup("):
        assert {n: s.count(needle) for n, s in src.items() if needle in s and n != "ops.py"} == {"step_recipe.py": 1}, needle
    for name in ("trainer.py", "multimodel.py"):
        for needle in ("_lib.lib()", ".cuda_stream", "data_ptr()", "import _lib"):
            assert needle not in src[name], (name, needle)
    assert (ops.SLOT_LSTM_DROPOUT, ops.SLOT_RRELU, ops.SLOT_HEAD_DROPOUT, ops.SLOT_AUGMENT) == (0, 1, 2, 3)      # one definition, re-exported


def test_rng_dicts_of_the_training_entry_points_need_their_probabilities():
    """A step's rng dict without p_lstm / p_head is refused, not trained with dropout 0; nsd_augment / nsd_mixup draw no dropout and ask for
    neither."""
    full, bare = sr.step_rng(5, 3, 0.6, 0.25), dict(seed=5, base_stream=12)
    r = ops._rng_struct(full)
    assert (r.seed, r.base_stream, r.p_lstm, r.p_head) == (5, 12, pytest.approx(0.6), 0.25)
    with pytest.raises(KeyError):
        ops._rng_struct(bare)
    with pytest.raises(KeyError):
        ops._rng_array([full, bare], 2, "multi")
    a = ops._rng_array([full, bare], 2, "augment", probs=False)
    assert [(g.seed, g.base_stream, g.p_lstm, g.p_head) for g in a] == [(5, 12, 0.0, 0.0)] * 2


def _recipe(stochastic=True, augment=None, loss=None, **model_kw):
    return sr.StepRecipe(nsd_amd.EEG_LSTM(**model_kw), stochastic, augment, loss, "cpu")


def test_policy_table():
    assert _recipe(augment=nsd_amd.Augment()).augment is None and _recipe(augment=None).augment is None
    assert _recipe(augment=AUG).augment == AUG
    assert _recipe(augment=AUG, stochastic=False).augment is None
    r = _recipe(loss=nsd_amd.Loss(label_smoothing=0.1, mixup=0.5), stochastic=False)
    assert r.loss == nsd_amd.Loss(label_smoothing=0.1) and r.loss.mixup == 0
    assert _recipe(loss=nsd_amd.Loss(mixup=0.5), stochastic=False).loss is None
    assert _recipe(loss=nsd_amd.Loss()).loss is None and _recipe(loss=None).loss is None
    r = _recipe(loss=nsd_amd.Loss(class_weights=(1.0, 2.0, 0.5)), stochastic=False)
    assert r.loss.class_weights == (1.0, 2.0, 0.5) and torch.equal(r.class_weights, torch.tensor([1.0, 2.0, 0.5]))
    with pytest.raises(ValueError, match="class_weights"):
        _recipe(loss=nsd_amd.Loss(class_weights=(1.0, 2.0)))
    r = _recipe(dropout=0.4, normalize=True)
    assert (r.p_lstm, r.p_head, r.normalize) == (0.4, 0.4, True)
    assert r.rng(5, 3) == dict(seed=5, base_stream=12, p_lstm=0.4, p_head=0.4) and _recipe(stochastic=False).rng(5, 3) is None


@pytest.fixture
def calls(monkeypatch):
    """ops.augment / ops.mixup / ops.zscore as stand-ins that record (name, arguments) and return fresh CPU tensors (or the `out` given)."""
    rec = []

    def augment(x, aug, rngs, *, M=1, zscore=False, step_dev=None, out=None):
        rec.append(("augment", dict(x=x, aug=aug, rngs=rngs, M=M, zscore=zscore, step_dev=step_dev, out=out)))
        shape = tuple(x.shape) if x.dim() == 4 or M == 1 else (M,) + tuple(x.shape)
        return out if out is not None else torch.full(shape, 7.0)

    def zscore(x, out=None):
        rec.append(("zscore", dict(x=x, out=out)))
        return out if out is not None else x + 1.0

    def mixup(x, labels, K, rngs, *, label_smoothing=0.0, mix=0.0, class_weights=None, M=1, step_dev=None, out=None, targets=None):
        rec.append(("mixup", dict(x=x, labels=labels, K=K, rngs=rngs, label_smoothing=label_smoothing, mix=mix, class_weights=class_weights,
                                  M=M, step_dev=step_dev, out=out, targets=targets)))
        tg = targets if targets is not None else torch.zeros((labels.numel(), K))
        return (None if x is None else out if out is not None else x * 0.5), tg

    monkeypatch.setattr(ops, "augment", augment)
    monkeypatch.setattr(ops, "zscore", zscore)
    monkeypatch.setattr(ops, "mixup", mixup)
    return rec


def _batch(B=4, T=5, M=None):
    g = torch.Generator().manual_seed(0)
    x = torch.randn((B, T, 8) if M is None else (M, B, T, 8), generator=g)
    return x, torch.randint(0, 3, ((M or 1) * B,), generator=g, dtype=torch.int32)


LOSS = nsd_amd.Loss(label_smoothing=0.1, class_weights=(1.0, 2.0, 0.5), mixup=0.5)


@pytest.mark.parametrize("step", [1, 2**30 + 5])
def test_prepare_as_the_eager_step_drives_it(calls, step):
    r = _recipe(augment=AUG, loss=LOSS, normalize=True)
    x, y = _batch()
    xo, labels, tg = r.prepare(x, y, [77], step)
    assert [n for n, _ in calls] == ["augment", "mixup"]            # no z-score launch of its own: it rides in the augment call
    a, m = calls[0][1], calls[1][1]
    assert torch.equal(a["x"], x) and a["aug"] == AUG and a["zscore"] is True and a["M"] == 1 and a["step_dev"] is None and a["out"] is None
    assert a["rngs"] == [sr.step_rng(77, step)] and a["rngs"][0]["base_stream"] == sr.base_stream(step)
    aug_out = torch.full((4, 5, 8), 7.0)
    assert torch.equal(m["x"], aug_out) and m["labels"] is y and m["K"] == 3 and m["rngs"] == a["rngs"] and m["M"] == 1
    assert (m["label_smoothing"], m["mix"]) == (0.1, 0.5) and m["class_weights"] is r.class_weights
    assert m["step_dev"] is None and m["out"] is None and m["targets"] is None
    assert torch.equal(xo, aug_out * 0.5) and labels is None and tuple(tg.shape) == (4, 3)


def test_prepare_as_the_graph_step_drives_it(calls):
    r = _recipe(augment=AUG, loss=LOSS, normalize=True)
    x, y = _batch()
    bufs = dict(x=x, y=y, **r.static_buffers(x))
    assert sorted(bufs) == ["tg", "x", "xm", "xn", "y"] and bufs["xn"].shape == x.shape == bufs["xm"].shape and tuple(bufs["tg"].shape) == (4, 3)
    step_dev = torch.zeros(1, dtype=torch.int64)
    xo, labels, tg = r.prepare(x, y, [77], 0, step_dev=step_dev, bufs=bufs)
    assert [n for n, _ in calls] == ["augment", "mixup"]
    a, m = calls[0][1], calls[1][1]
    assert a["x"] is x and a["out"] is bufs["xn"] and a["step_dev"] is step_dev and a["zscore"] is True
    assert a["rngs"] == [sr.step_rng(77, 0)] and a["rngs"][0]["base_stream"] == 0      # the stream id comes from the device counter
    assert m["x"] is bufs["xn"] and m["out"] is bufs["xm"] and m["targets"] is bufs["tg"] and m["step_dev"] is step_dev and m["rngs"] == a["rngs"]
    assert xo is bufs["xm"] and labels is None and tg is bufs["tg"]
    # a host step number is ignored once the device counter is given
    r.prepare(x, y, [77], 9, step_dev=step_dev, bufs=bufs)
    assert calls[2][1]["rngs"][0]["base_stream"] == 0
    # which static buffers a recipe needs
    assert _recipe().static_buffers(x) == {}
    assert sorted(_recipe(normalize=True).static_buffers(x)) == ["xn"]
    b = _recipe(loss=nsd_amd.Loss(label_smoothing=0.1)).static_buffers(x)
    assert sorted(b) == ["tg", "xm"] and b["xm"] is None
    # z-score alone: into the static buffer
    del calls[:]
    rz = _recipe(normalize=True)
    bz = rz.static_buffers(x)
    xo, labels, tg = rz.prepare(x, y, [77], 0, step_dev=step_dev, bufs=bz)
    assert [n for n, _ in calls] == ["zscore"] and calls[0][1]["out"] is bz["xn"] and xo.data_ptr() == bz["xn"].data_ptr() and labels is y and tg is None


@pytest.mark.parametrize("shared", [True, False])
def test_prepare_as_the_model_batched_step_drives_it(calls, shared):
    M, seeds = 3, [5, 6, 7]
    r = _recipe(augment=AUG, loss=LOSS)
    x, y = _batch(M=None if shared else M)
    if shared:
        y = y.repeat(M)
    xo, labels, tg = r.prepare(x, y, seeds, 4, M=M)
    assert [n for n, _ in calls] == ["augment", "mixup"]
    a, m = calls[0][1], calls[1][1]
    assert a["M"] == M == m["M"] and a["zscore"] is False and torch.equal(a["x"], x)
    assert a["rngs"] == [sr.step_rng(s, 4) for s in seeds] == m["rngs"]
    assert tuple(m["x"].shape) == (M, 4, 5, 8) and tuple(xo.shape) == (M, 4, 5, 8) and labels is None and tuple(tg.shape) == (M * 4, 3)
    # normalize without augmentation: one z-score launch over all models' trials, in the caller's shape
    del calls[:]
    xo, labels, tg = _recipe(normalize=True).prepare(x, y, seeds, 4, M=M)
    assert [n for n, _ in calls] == ["zscore"] and tuple(calls[0][1]["x"].shape) == ((4 if shared else M * 4), 5, 8)
    assert torch.equal(xo, x + 1.0) and xo.shape == x.shape and labels is y and tg is None


def test_prepare_parts_off(calls):
    x, y = _batch()
    # mixup off: the launch builds the target rows alone and the windows come back untouched
    xo, labels, tg = _recipe(loss=nsd_amd.Loss(label_smoothing=0.1)).prepare(x, y, [1], 2)
    assert [n for n, _ in calls] == ["mixup"] and calls[0][1]["x"] is None and calls[0][1]["mix"] == 0.0
    assert xo is x and labels is None and tuple(tg.shape) == (4, 3)
    # loss off and augmentation off: nothing, apart from the z-score when normalize is set
    del calls[:]
    assert _recipe().prepare(x, y, [1], 2) == (x, y, None) and calls == []
    xo, labels, tg = _recipe(normalize=True).prepare(x, y, [1], 2)
    assert [n for n, _ in calls] == ["zscore"] and calls[0][1]["out"] is None and torch.equal(xo, x + 1.0) and labels is y and tg is None
    # stochastic=False with both given: as off (mixup stripped, smoothing kept)
    del calls[:]
    xo, labels, tg = _recipe(stochastic=False, augment=AUG, loss=LOSS).prepare(x, y, [1], 2)
    assert [n for n, _ in calls] == ["mixup"] and calls[0][1]["x"] is None and xo is x
    # float [B,K] targets come back as given and record nothing
    del calls[:]
    q = torch.rand((4, 3))
    xo, labels, tg = _recipe().prepare(x, q, [1], 2)
    assert calls == [] and xo is x and labels is None and tg is q
    # ... while the windows are still what the model sees
    xo, labels, tg = _recipe(augment=AUG).prepare(x, q, [1], 2)
    assert [n for n, _ in calls] == ["augment"] and labels is None and tg is q
    # an empty shard launches nothing
    del calls[:]
    x0, y0 = torch.zeros((0, 5, 8)), torch.zeros((0,), dtype=torch.int32)
    xo, labels, tg = _recipe(augment=AUG, loss=LOSS, normalize=True).prepare(x0, y0, [1], 2)
    assert calls == [] and xo.shape == x0.shape and labels is y0 and tg is None
