"""Trial augmentation on the MI355X: nsd_augment against its numpy restatement (tests/augment_ref.py) bit for bit, the fused z-score
against nsd_zscore_fwd, and both trainers with augmentation on against the unaugmented step fed augmented input."""
import contextlib

import numpy as np
import pytest
import torch

from tests import augment_ref as ar
from tests.gpu_harness import dev, nsd, sync_at_the_end  # noqa: F401  (fixtures; sync_at_the_end is autouse)

pytestmark = pytest.mark.gpu

ALL = dict(max_shift=3, scale_range=0.2, p_channel=0.25, noise_std=0.3)


def _x(shape, seed=0):
    return (2.7 * np.random.RandomState(seed).standard_normal(shape)).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(t: torch.Tensor, ref: np.ndarray) -> bool:
    return np.array_equal(_bits(t.cpu().numpy()), _bits(ref))


def _configs(T):
    """each operation alone (the shift at S = 1 and S = T - 1) and all four together"""
    out = [dict(scale_range=0.2), dict(noise_std=0.3), dict(p_channel=0.25)]
    shifts = sorted({s for s in (1, T - 1) if 1 <= s < T})
    out += [dict(max_shift=s) for s in shifts]
    out += [dict(ALL, max_shift=s) for s in shifts] if shifts else [dict(scale_range=0.2, p_channel=0.25, noise_std=0.3)]
    return out


# B in {1, 5, 256, 1030}, T in {1, 2, 250, 625, 1000}, C in {1, 5, 8, 64}: 64 x 1000 is past the LDS staging limit (used by the z-score
# tests below with the same shapes), C = 5 leaves a thread idle (255 of 256 take part), 1030 trials exceed no grid cap but B = 1030 at
# M = 3 loops the grid (3090 workgroups of work on 8 x #CU).
SHAPES = [(1, 1, 1), (5, 1, 64), (5, 2, 5), (1030, 2, 5), (5, 250, 1), (256, 250, 8), (5, 625, 8), (1030, 625, 8), (1, 1000, 64),
          (5, 1000, 64), (5, 625, 5)]


@pytest.mark.parametrize("B,T,C", SHAPES)
def test_kernel_equals_numpy_bitwise(nsd, dev, B, T, C):
    from nsd_amd import ops
    x_np = _x((B, T, C), seed=B + T + C)
    x = torch.from_numpy(x_np).to(dev)
    for i, kw in enumerate(_configs(T)):
        seed, base = 0x9E3779B97F4A7C15 + 31 * i, 4 * (i + 1)
        y = ops.augment(x, nsd.Augment(**kw), dict(seed=seed, base_stream=base))
        assert y.shape == x.shape and _same_bits(y, ar.augment(x_np, seed, base, **kw)), kw


@pytest.mark.parametrize("B,T,C", [(5, 250, 8), (1030, 2, 5), (256, 250, 8), (5, 1000, 64), (1, 1, 1)])
def test_models_in_one_launch(nsd, dev, B, T, C):
    """M = 3 with shared windows (x_model_stride 0) and with per-model windows (B*T*C): row m is the M = 1 call with rng[m], bitwise,
    and the numpy restatement."""
    from nsd_amd import ops
    kw = dict(ALL, max_shift=min(3, T - 1))
    A = nsd.Augment(**kw)
    rngs = [dict(seed=1000 + 17 * m, base_stream=4 * (m + 2)) for m in range(3)]
    pairs = [(r["seed"], r["base_stream"]) for r in rngs]
    xs_np = _x((3, B, T, C), seed=7)
    xs = torch.from_numpy(xs_np).to(dev)
    shared = ops.augment(xs[0].contiguous(), A, rngs, M=3)
    own = ops.augment(xs, A, rngs)
    assert shared.shape == own.shape == (3, B, T, C)
    assert _same_bits(shared, ar.augment_models(xs_np[0], pairs, **kw)) and _same_bits(own, ar.augment_models(xs_np, pairs, **kw))
    for m in range(3):
        one_shared = ops.augment(xs[0].contiguous(), A, rngs[m])
        one_own = ops.augment(xs[m].contiguous(), A, rngs[m])
        assert one_shared.shape == (B, T, C)
        assert _same_bits(shared[m], one_shared.cpu().numpy()) and _same_bits(own[m], one_own.cpu().numpy()), m


# T * C * 4 = 20 000 (staged), 65 536 (the largest staged window), 65 568 and 256 000 (recomputed per pass); C = 5: an idle thread
@pytest.mark.parametrize("B,T,C", [(5, 625, 8), (300, 250, 8), (4, 2048, 8), (4, 2049, 8), (5, 1000, 64), (3, 625, 5), (2, 1, 8), (3, 64, 256),
                                   (2, 65, 256)])
def test_fused_zscore_equals_zscore_of_the_unfused_output(nsd, dev, B, T, C):
    from nsd_amd import ops
    x = torch.from_numpy(_x((B, T, C), seed=T)).to(dev)
    rng = dict(seed=77, base_stream=28)
    step_dev = torch.tensor([7], dtype=torch.int64, device=dev)          # base = 4 * 7
    for kw in (dict(ALL, max_shift=min(3, T - 1)), dict(noise_std=0.5), {}):
        A = nsd.Augment(**kw)
        plain = ops.augment(x, A, rng)
        fused = ops.augment(x, A, rng, zscore=True)
        assert torch.equal(fused, ops.zscore(plain)), kw
        # the device step counter gives the stream id of the explicit form (the base_stream of rng is then ignored)
        assert torch.equal(ops.augment(x, A, dict(seed=77, base_stream=999), step_dev=step_dev), plain), kw
        assert torch.equal(ops.augment(x, A, dict(seed=77, base_stream=0), zscore=True, step_dev=step_dev), fused), kw
    three = ops.augment(x, nsd.Augment(**ALL) if T > 3 else nsd.Augment(noise_std=0.3), [dict(seed=s, base_stream=8) for s in (1, 2, 3)], M=3,
                        zscore=True)
    for m, s in enumerate((1, 2, 3)):
        one = ops.augment(x, nsd.Augment(**ALL) if T > 3 else nsd.Augment(noise_std=0.3), dict(seed=s, base_stream=8), zscore=True)
        assert torch.equal(three[m], one), m


def test_all_off_is_a_bitwise_copy(nsd, dev):
    from nsd_amd import ops
    x_np = _x((6, 40, 8), seed=3)
    x_np[0, 0, 0], x_np[1, 5, 2], x_np[2, 7, 3], x_np[3, 1, 1] = -0.0, np.nan, np.inf, -np.inf
    x_np[4, 2, 2] = np.frombuffer(np.uint32(0x7FC12345).tobytes(), np.float32)[0]      # a NaN with a payload
    x = torch.from_numpy(x_np).to(dev)
    y = ops.augment(x, nsd.Augment(), dict(seed=5, base_stream=4))
    assert y.data_ptr() != x.data_ptr() and _same_bits(y, x_np)
    y3 = ops.augment(x, nsd.Augment(), [dict(seed=s, base_stream=4) for s in (1, 2, 3)], M=3)
    for m in range(3):
        assert _same_bits(y3[m], x_np)
    # the special values pass through the operations that do not touch them: a shift moves them, a scale keeps -0.0 / Inf / NaN
    kw = dict(max_shift=2, scale_range=0.1)
    assert _same_bits(ops.augment(x, nsd.Augment(**kw), dict(seed=5, base_stream=4)), ar.augment(x_np, 5, 4, **kw))


# ---- the trainers ---------------------------------------------------------------------------------------------------------------------
def _model(nsd, dev, seed, *a, **kw):
    torch.manual_seed(seed)
    return nsd.EEG_LSTM(*a, **kw).to(dev).train()


def _batch(dev, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return (2.7 * torch.randn((B, T, 8), generator=g)).to(dev), torch.randint(0, 3, (B,), generator=g, dtype=torch.int32).to(dev)


@pytest.mark.parametrize("case", ["fp32", "fp32_normalize", "bf16_h64", "bf16_h64_normalize"])
def test_trainer_step_equals_unaugmented_step_on_augmented_input(nsd, dev, case):
    """Trainer(augment=A).step(x, y) leaves bitwise the parameters, Adam moments and loss of Trainer(augment=None).step(ops.augment(x, A,
    seed, 4 * step), y), over three steps (different batches)."""
    from nsd_amd import ops
    from nsd_amd.trainer import Trainer
    norm = case.endswith("normalize")
    args = (8, 64, 2, 3, 0.6) if case.startswith("bf16") else ()
    kw = dict(normalize=norm, precision="bf16") if case.startswith("bf16") else dict(normalize=norm)
    A = nsd.Augment(max_shift=5, scale_range=0.15, p_channel=0.2, noise_std=0.4)
    ma, mb = _model(nsd, dev, 11, *args, **kw), _model(nsd, dev, 11, *args, **kw)
    ta, tb = Trainer(ma, lr=1e-3, seed=9, augment=A), Trainer(mb, lr=1e-3, seed=9)
    assert ta.augment == A and tb.augment is None and ta.seed == tb.seed
    for step in range(1, 4):
        x, y = _batch(dev, 32, 40, seed=step)
        ta.step(x, y)
        tb.step(ops.augment(x, A, dict(seed=tb.seed, base_stream=4 * step)), y)
        assert torch.equal(ta.flat, tb.flat) and torch.equal(ta.m, tb.m) and torch.equal(ta.v, tb.v), step
        assert ta.last_loss() == tb.last_loss(), step
    assert not torch.equal(ta.flat, _model(nsd, dev, 11, *args, **kw).flat_parameters())
    # evaluation never augments: the eval-mode forward of the trained model is that of the reference trainer's model
    x, _ = _batch(dev, 8, 40, seed=99)
    ma.eval(); mb.eval()
    with torch.no_grad():
        assert torch.equal(ma(x), mb(x))


@pytest.mark.parametrize("normalize", [False, True])
def test_graph_replay_step_equals_eager_step_with_augmentation(nsd, dev, normalize):
    """As test_gpu_parity.py::test_graph_replay_step_equals_eager_step, with augmentation on: the replayed graph draws the step's
    augmentation from the device step counter.  The augmented buffer of every replay is bitwise the explicit-stream launch; gradients
    are bit-identical; the parameters differ by the parent's device-pow() vs host-pow() Adam bias corrections only (its bound: 1e-6)."""
    from nsd_amd import ops
    from nsd_amd.trainer import Trainer
    B, T = 16, 30
    A = nsd.Augment(max_shift=4, scale_range=0.1, p_channel=0.2, noise_std=0.3)
    x, y = _batch(dev, B, T, seed=8)
    ma, mb = _model(nsd, dev, 21, normalize=normalize), _model(nsd, dev, 21, normalize=normalize)
    ta, tb = Trainer(ma, lr=1e-3, seed=5, augment=A), Trainer(mb, lr=1e-3, seed=5, augment=A)
    xs, ys = tb.static_inputs(B, T)
    xs.copy_(x); ys.copy_(y)
    for step in range(1, 4):
        ta.step(x, y)
        tb.step_static(B, T)
        want = ops.augment(x, A, dict(seed=tb.seed, base_stream=4 * step), zscore=normalize)
        assert torch.equal(tb._buffers(B, T)["xn"], want), step
    assert tb.step_count == 3 and int(tb._step_dev.item()) == 3
    assert torch.equal(ta.grads, tb.grads)
    assert (ma.flat_parameters() - mb.flat_parameters()).abs().max().item() < 1e-6
    assert abs(ta.last_loss() - tb.last_loss()) < 1e-6


def _launches(trainer, x, y, steps=2):
    from nsd_amd import ops
    names = []

    @contextlib.contextmanager
    def hook(name):
        names.append(name)
        yield
    ops.set_launch_hook(hook)
    try:
        for _ in range(steps):
            trainer.step(x, y)
    finally:
        ops.set_launch_hook(None)
    return names


@pytest.mark.parametrize("normalize", [False, True])
def test_augmentation_off_is_the_parents_launch_sequence(nsd, dev, normalize):
    from nsd_amd.trainer import Trainer
    x, y = _batch(dev, 32, 40, seed=2)

    def run(**kw):
        return _launches(Trainer(_model(nsd, dev, 3, normalize=normalize), lr=1e-3, seed=4, **kw), x, y)
    base = run()
    assert base and "nsd_augment" not in base and ("nsd_zscore_fwd" in base) == normalize
    assert run(augment=None) == base and run(augment=nsd.Augment()) == base
    assert run(augment=nsd.Augment(**ALL), stochastic=False) == run(stochastic=False)      # deterministic steps are never augmented
    on = run(augment=nsd.Augment(**ALL))
    assert on.count("nsd_augment") == 2 and "nsd_zscore_fwd" not in on
    assert len(on) == len(base) + (0 if normalize else 2)          # per step: one launch more, or nsd_augment in nsd_zscore_fwd's place
    assert [n for n in on if n != "nsd_augment"] == [n for n in base if n != "nsd_zscore_fwd"]
    # the model-batched trainer likewise
    def run_multi(**kw):
        models = [_model(nsd, dev, 30 + m, normalize=normalize) for m in range(3)]
        return _launches(nsd.ModelBatchTrainer(models, lr=1e-3, seeds=[1, 2, 3], **kw), x, y)
    mbase = run_multi()
    assert run_multi(augment=None) == mbase and run_multi(augment=nsd.Augment()) == mbase
    mon = run_multi(augment=nsd.Augment(**ALL))
    assert mon.count("nsd_augment") == 2 and len(mon) == len(mbase) + (0 if normalize else 2)


@pytest.mark.parametrize("normalize,shared", [(False, False), (True, False), (False, True)])
def test_model_batch_trainer_equals_separate_trainers_with_augmentation(nsd, dev, normalize, shared):
    """ModelBatchTrainer(models, seeds, augment=A) over three steps == M separate Trainer(model_m, seed=seeds[m], augment=A) runs, bitwise.
    3 x 32 trials and 32 trials are both served by the one-trial H = 48 kernels on one workgroup per trial (up to one trial per CU),
    so the model-batched launch does each model's arithmetic in the single-model order."""
    from nsd_amd.trainer import Trainer
    M, B, T = 3, 32, 40
    A = nsd.Augment(max_shift=5, scale_range=0.15, p_channel=0.2, noise_std=0.4)
    seeds = [3, 4, 5]
    batched = [_model(nsd, dev, 100 + m, normalize=normalize) for m in range(M)]
    singles = [_model(nsd, dev, 100 + m, normalize=normalize) for m in range(M)]
    tr = nsd.ModelBatchTrainer(batched, lr=1e-3, seeds=seeds, augment=A)
    trs = [Trainer(singles[m], lr=1e-3, seed=seeds[m], augment=A) for m in range(M)]
    for step in range(1, 4):
        g = torch.Generator().manual_seed(step)
        xs = torch.randn((M, B, T, 8), generator=g).to(dev)
        ys = torch.randint(0, 3, (M, B), generator=g, dtype=torch.int32).to(dev)
        if shared:
            tr.step(xs[0].contiguous(), ys[0].contiguous())
        else:
            tr.step(xs, ys)
        losses = tr.last_losses()
        for m in range(M):
            k = 0 if shared else m
            trs[m].step(xs[k].contiguous(), ys[k].contiguous())
            assert torch.equal(tr.params[m], trs[m].flat) and torch.equal(tr.m[m], trs[m].m) and torch.equal(tr.v[m], trs[m].v), (step, m)
            assert losses[m] == trs[m].last_loss(), (step, m)
    if shared:
        assert not torch.equal(tr.grads[0], tr.grads[1])          # own draws (and own parameters) per model
