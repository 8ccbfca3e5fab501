"""The whole-window callers of the rate conversion and the trainers' refusal, the parts that need no GPU (the twin of
tests/test_gpu_resample_surfaces.py): with the launches replaced by recording stand-ins, every caller that gained an
ops.resample_trials line runs it FIRST and hands its result -- not the caller's trials -- to the stage behind; and a trainer built on a
model with a rate conversion is refused at construction, with the sanctioned route in the message."""
import inspect
import re

import numpy as np
import pytest
import torch

import nsd_amd
from nsd_amd import align as align_mod
from nsd_amd import grid, ops, train
from nsd_amd.step_recipe import StepRecipe

C, T_IN = 8, 24


def _converter():
    taps = (np.random.RandomState(1027).standard_normal((1, 7)) / np.sqrt(7)).astype(np.float32)
    return nsd_amd.Resample(L=1, M=2, P=7, taps=taps)


@pytest.fixture
def launches(monkeypatch):
    rec = []

    def resample_trials(x, resample):
        out = torch.full((x.shape[0], resample.out_steps(0, x.shape[1]), x.shape[2]), 7.0)
        rec.append(dict(name="resample_trials", x=x, resample=resample, out=out))
        return out

    def gate_step(x, gate, state=None, *, slots=None, out=None, mask=None):
        rec.append(dict(name="gate_step", x=x))
        return x.clone(), torch.zeros(tuple(x.shape[:2]), dtype=torch.int32)

    def prep_step(x, prep, state=None, *, slots=None, out=None):
        rec.append(dict(name="prep_step", x=x))
        return x

    def gate_apply(v, gate, mask, *, out=None, max_bad=None):
        rec.append(dict(name="gate_apply", x=v, max_bad=max_bad))
        return v

    def spatial_apply(v, W, *, sel=None, out=None):
        rec.append(dict(name="spatial_apply", x=v))
        return v

    def cov_step(v, state=None, *, mask=None, slots=None, out=None):
        rec.append(dict(name="cov_step", x=v, mask=mask))
        return torch.zeros((1, C, C), dtype=torch.float64), torch.zeros((1, 2), dtype=torch.int64)

    def whiten_fit(C_, cfg, sums=None, counts=None, **kw):
        rec.append(dict(name="whiten_fit"))
        return torch.zeros((kw.get("G", 1), C_, C_)), torch.zeros(kw.get("G", 1) * ops.WHITEN_RECORD_BYTES, dtype=torch.uint8)

    for f in (resample_trials, gate_step, prep_step, gate_apply, spatial_apply, cov_step, whiten_fit):
        monkeypatch.setattr(ops, f.__name__, f)
    return rec


def _model(resample=True, gate=True, prep=True, align=True):
    return nsd_amd.EEG_LSTM(resample=_converter() if resample else None, gate=nsd_amd.SignalGate(rail=100.0) if gate else None,
                            prep=nsd_amd.CausalPrep.design(highpass=1.0) if prep else None,
                            align=nsd_amd.SessionAlign() if align else None).eval()


def test_the_front_end_converts_first_and_every_stage_reads_the_converted_trials(launches):
    m = _model()
    x = torch.zeros((3, T_IN, C))
    m._front(x)
    assert [c["name"] for c in launches] == ["resample_trials", "gate_step", "prep_step", "gate_apply", "spatial_apply"]
    first = launches[0]
    assert first["x"] is x and first["resample"] is m.resample and launches[1]["x"] is first["out"]
    assert all(tuple(c["x"].shape) == (3, T_IN // 2, C) for c in launches[1:])
    # a model without the stage launches nothing new
    del launches[:]
    _model(resample=False)._front(x)
    assert [c["name"] for c in launches] == ["gate_step", "prep_step", "gate_apply", "spatial_apply"] and launches[0]["x"] is x


@pytest.mark.parametrize("groups", [None, [0, 1, 1]])
def test_session_align_fit_converts_the_trials_before_the_models_front_end(launches, groups):
    m = _model(align=False)
    x = np.zeros((3, T_IN, C), np.float32)
    nsd_amd.SessionAlign().fit(m, x, groups=groups)
    assert [c["name"] for c in launches] == ["resample_trials", "gate_step", "prep_step", "gate_apply", "cov_step", "whiten_fit"]
    assert tuple(launches[0]["x"].shape) == (3, T_IN, C) and launches[1]["x"] is launches[0]["out"]
    assert launches[3]["max_bad"] is None                                      # eval mode: a rejected step is left out of the moment
    assert tuple(launches[4]["x"].shape) == (3, T_IN // 2, C) and launches[4]["mask"] is not None
    del launches[:]
    nsd_amd.SessionAlign().fit(_model(resample=False, align=False), x, groups=groups)
    assert [c["name"] for c in launches] == ["gate_step", "prep_step", "gate_apply", "cov_step", "whiten_fit"]


def test_every_whole_window_caller_holds_the_conversion_in_front_of_its_front_end():
    """SpatialFit.fit and EnsembleSpatialFit.fit need the device from their first line on (tests/test_gpu_resample_surfaces.py runs
    them); here their text is held: the conversion stands between the shape check and the front end, once."""
    for fn, who in ((align_mod.SpatialFit.fit, "model"), (align_mod.EnsembleSpatialFit.fit, "self.members[0]"),
                    (align_mod.SessionAlign.fit, "model")):
        src = inspect.getsource(fn)
        assert src.count("ops.resample_trials(") == 1, fn.__qualname__
        assert src.index("ops.resample_trials(x, " + who + ".resample)") < src.index("._gate_prep(x"), fn.__qualname__
        assert src.index("x.shape[-1] != ") < src.index("ops.resample_trials("), fn.__qualname__


# ---- trainers refuse what they would silently ignore -----------------------------------------------------------------------------------
ROUTE = "train a resample-free model on converted trials .* hand resample= to save_reference_checkpoint"


def test_a_trainer_on_a_model_with_a_rate_conversion_is_refused_at_construction():
    from nsd_amd.multimodel import ModelBatchTrainer
    from nsd_amd.trainer import Trainer
    m, twin = nsd_amd.EEG_LSTM(resample=_converter()), nsd_amd.EEG_LSTM(resample=_converter())
    with pytest.raises(nsd_amd.NsdError, match="^Trainer: the model has a rate conversion .*" + ROUTE):
        Trainer(m)                                        # (Trainer.step_static is a method of the same object: no trainer, no static step)
    with pytest.raises(nsd_amd.NsdError, match="^ModelBatchTrainer: the model has a rate conversion .*" + ROUTE):
        ModelBatchTrainer([m, twin])
    with pytest.raises(nsd_amd.NsdError, match="^ModelBatchTrainer: .*" + ROUTE):
        ModelBatchTrainer([m])
    with pytest.raises(nsd_amd.NsdError, match="^StepRecipe: the model has a rate conversion .*" + ROUTE):
        StepRecipe(m, True, None, None, "cpu")
    with pytest.raises(nsd_amd.NsdError, match="^StepRecipe: .*" + ROUTE):
        StepRecipe(m, True, None, None, "cpu", models=[m, twin])
    # the resample-free model is taken as before: the first refusal it meets is the old one (no GPU here), not the new
    with pytest.raises(nsd_amd.NsdError, match="Trainer needs the model on the MI355X"):
        Trainer(nsd_amd.EEG_LSTM())
    assert StepRecipe(nsd_amd.EEG_LSTM(), True, None, None, "cpu").prep is None


def test_train_and_grid_follow_the_sanctioned_route():
    """--input-rate builds the Resample, converts the loaded trials, trains resample-free models and writes the conversion into the
    checkpoint: neither tool hands resample= to a model it trains (the GPU tests run both end to end)."""
    args = train.build_parser().parse_args(["--synthetic", "8", "--input-rate", "250"])
    r = train.resample_for(args)
    assert r == nsd_amd.Resample.design(250, 125) and train.resample_for(train.build_parser().parse_args(["--synthetic", "8"])) is None
    for mod in (train, grid):
        src = inspect.getsource(mod)
        assert "resample_loaded(x_np, resample, dev)" in src, mod.__name__
        for call in re.findall(r"EEG_LSTM\([^)]*\)", src):
            assert "resample" not in call, (mod.__name__, call)
    assert "save_reference_checkpoint(mdl, path, resample=resample)" in inspect.getsource(train)
