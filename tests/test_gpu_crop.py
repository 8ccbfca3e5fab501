"""Cropped training on the MI355X: nsd_crop and nsd_crop_pool against their numpy restatement (tests/crop_ref.py) bit for bit, the
crop stage inside the three trainers against the same step fed hand-cropped input, trial-level evaluation against its hand composition,
and the crops of a regular grid against the sliding decoder's decisions on the same trial (train / serve agreement)."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from tests import augment_ref as ar
from tests import crop_ref as cr
from tests import mixup_ref as mr
from tests.buffer_contract import GUARD_BYTE, guarded, snapshot
from tests.gpu_harness import LOGIT_TOL, PROB_TOL, dev, nsd, sync_at_the_end  # noqa: F401  (fixtures; sync_at_the_end is autouse)

pytestmark = pytest.mark.gpu

ARGMAX_GAP = 1e-3                  # tests/test_gpu_stream.py: the same argmax wherever the top two logits are further apart
# (B, T, C, W, R): the vector (C % 4 == 0) and scalar copy paths, W == T, W == 1, T - W + 1 not a power of two, R = NSD_CROP_MAX
SHAPES = [(3, 12, 8, 5, 4), (2, 7, 3, 7, 1), (5, 9, 1, 1, 64), (4, 33, 4, 32, 2)]
K = 3


def _x(shape, seed=0):
    return (2.7 * np.random.RandomState(seed).standard_normal(shape)).astype(np.float32)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(t: torch.Tensor, ref: np.ndarray) -> bool:
    got = t.cpu().numpy()
    return got.size == ref.size and np.array_equal(_bits(got).reshape(-1), _bits(ref).reshape(-1))


def _regular(T, W, R):
    """a regular grid of the shape: as many of its R crops as fit at hop 1"""
    return min(R, T - W + 1), 1


def _launch(ops, nsd, x, cfg, rngs, M, labels, targets, step_dev=None):
    """one nsd_crop into 0xA5-guarded, NaN-filled outputs; the guards are checked and the inputs compared with their snapshot"""
    Mx, B, T, Cc = (x.shape if x.dim() == 4 else (M,) + tuple(x.shape))
    rows = M * B * cfg.crops
    (y, cy), (lo, cl), (to, ct), (off, co) = (guarded((rows, cfg.window, Cc), torch.float32, x.device, "nan32"),
                                              guarded((rows,), torch.int32, x.device, "ones"),
                                              guarded((rows, K), torch.float32, x.device, "nan32"), guarded((rows,), torch.int32, x.device, "ones"))
    snap = snapshot(x, labels, targets)
    out = ops.crop(x, cfg, rngs, M=M, labels=labels, targets=targets, step_dev=step_dev, out=y, labels_out=lo, targets_out=to, offsets=off)
    torch.cuda.synchronize()
    assert out[0] is y and out[1] is lo and out[2] is to
    for c, name in ((cy, "y"), (cl, "labels_out"), (ct, "targets_out"), (co, "offsets")):
        c(name)
    assert snap.unchanged()
    return y, lo, to, off


@pytest.mark.parametrize("mode", ["one", "shared", "strided"])
@pytest.mark.parametrize("B,T,Cc,W,R", SHAPES)
def test_crop_equals_numpy_bitwise(nsd, dev, B, T, Cc, W, R, mode):
    from nsd_amd import ops
    M = 1 if mode == "one" else 3
    rngs = [dict(seed=0x9E3779B97F4A7C15 + 31 * m, base_stream=4 * (m + 2)) for m in range(M)]
    pairs = [(r["seed"], r["base_stream"]) for r in rngs]
    x_np = _x((B, T, Cc) if mode != "strided" else (M, B, T, Cc), seed=B + T + Cc)
    x_np.reshape(-1)[:3] = (-0.0, np.nan, np.frombuffer(np.uint32(0x7FC12345).tobytes(), np.float32)[0])    # a copy keeps every bit
    lab_np = np.random.RandomState(1).randint(0, K, (M, B)).astype(np.int32)
    tg_np = _x((M, B, K), seed=2)
    x, lab, tg = torch.from_numpy(x_np).to(dev), torch.from_numpy(lab_np.reshape(-1)).to(dev), torch.from_numpy(tg_np.reshape(M * B, K)).to(dev)
    want = cr.crop_models(x_np, W, R, pairs, 0, lab_np, tg_np)
    y, lo, to, off = _launch(ops, nsd, x, nsd.Crop(W, R), rngs if M > 1 else rngs[0], M, lab, tg)
    assert _same(y, want[0]) and _same(lo, want[1]) and _same(to, want[2]) and _same(off, want[3])
    o = off.cpu().numpy()
    assert o.min() >= 0 and o.max() <= T - W
    # the device step counter gives the stream id of the host-numbered call (the base_stream of rng is then ignored)
    step_dev = torch.tensor([5 + (1 << 30)], dtype=torch.int64, device=dev)            # base = 4 * 5: the counter is taken mod 2^30
    at5 = [dict(seed=r["seed"], base_stream=20) for r in rngs]
    stale = [dict(seed=r["seed"], base_stream=999) for r in rngs]
    y5 = _launch(ops, nsd, x, nsd.Crop(W, R), at5 if M > 1 else at5[0], M, lab, tg)
    yd = _launch(ops, nsd, x, nsd.Crop(W, R), stale if M > 1 else stale[0], M, lab, tg, step_dev=step_dev)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(y5, yd))          # (bits: x holds NaNs)
    assert _same(y5[3], cr.crop_models(x_np, W, R, [(s, 20) for s, _ in pairs])[3])
    # the regular grid: no draws, no rng
    Rg, hop = _regular(T, W, R)
    want = cr.crop_models(x_np, W, Rg, pairs, hop, lab_np, tg_np)
    y, lo, to, off = _launch(ops, nsd, x, nsd.Crop(W, Rg, hop), None, M, lab, tg)
    assert _same(y, want[0]) and _same(lo, want[1]) and _same(to, want[2]) and _same(off, want[3])
    assert off.view(M, B, Rg).cpu().tolist() == [[[r * hop for r in range(Rg)]] * B] * M
    # labels / targets are optional, one by one
    first = cr.crop_models(x_np, W, R, pairs, 0, lab_np)
    y2, lo2, to2 = ops.crop(x, nsd.Crop(W, R), rngs if M > 1 else rngs[0], M=M, labels=lab)
    assert to2 is None and _same(y2, first[0]) and _same(lo2, first[1])
    assert ops.crop(x, nsd.Crop(W, R), rngs if M > 1 else rngs[0], M=M)[1:] == (None, None)


def test_crop_covers_more_rows_than_the_grid_and_unaligned_pointers(nsd, dev):
    """B * R rows beyond 8 x #CU workgroups (the grid-stride loop), at the training shape's C = 8; and a source that is only 4-byte
    aligned, which takes the one-word path"""
    from nsd_amd import ops
    B, T, Cc, W, R = 700, 40, 8, 16, 4
    x_np = _x((B, T, Cc), seed=9)
    x = torch.from_numpy(x_np).to(dev)
    y, _, _ = ops.crop(x, nsd.Crop(W, R), dict(seed=3, base_stream=8))
    assert _same(y, cr.crop(x_np, W, R, 0, 3, 8)[0])
    flat = torch.empty(x.numel() + 1, dtype=torch.float32, device=dev)
    xu = flat[1:].view(B, T, Cc)
    xu.copy_(x)
    assert xu.data_ptr() % 16 == 4 and xu.is_contiguous()
    assert torch.equal(ops.crop(xu, nsd.Crop(W, R), dict(seed=3, base_stream=8))[0], y)


def test_side_stream_and_graph_replay_give_the_same_bits(nsd, dev):
    from nsd_amd import ops
    B, T, Cc, W, R = SHAPES[0]
    x = torch.from_numpy(_x((B, T, Cc), seed=4)).to(dev)
    lab = torch.arange(B, dtype=torch.int32, device=dev)
    cfg, rng = nsd.Crop(W, R), dict(seed=77, base_stream=0)
    step_dev = torch.tensor([3], dtype=torch.int64, device=dev)
    want = ops.crop(x, cfg, dict(seed=77, base_stream=12), labels=lab)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = ops.crop(x, cfg, dict(seed=77, base_stream=12), labels=lab)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    y, lo = torch.full_like(want[0], float("nan")), torch.full_like(want[1], -1)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.crop(x, cfg, rng, labels=lab, step_dev=step_dev, out=y, labels_out=lo)          # warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.crop(x, cfg, rng, labels=lab, step_dev=step_dev, out=y, labels_out=lo)
    for step in (3, 4, 9):                                          # the replay reads the offsets' stream from the counter
        step_dev.fill_(step)
        y.fill_(float("nan")); lo.fill_(-1)
        g.replay()
        want = ops.crop(x, cfg, dict(seed=77, base_stream=4 * step), labels=lab)
        assert torch.equal(y, want[0]) and torch.equal(lo, want[1]), step


# ---- an augmented and mixed step's draws do not move when cropping is switched on ---------------------------------------------------------
def test_cropping_leaves_the_augment_and_mixup_draws_alone(nsd, dev):
    """the nsd_augment output of a trainer's replayed step is the same buffer of bits with and without a crop stage behind it, and
    the whole prepared batch is the numpy chain augment -> crop -> mixup with each stage's own slots of the one stream"""
    from nsd_amd import ops
    from nsd_amd.step_recipe import StepRecipe
    from nsd_amd.trainer import Trainer
    B, T, W, R = 4, 20, 8, 3
    A, L = nsd.Augment(max_shift=3, scale_range=0.2, p_channel=0.25, noise_std=0.3), nsd.Loss(label_smoothing=0.1, mixup=0.7)
    x_np = _x((B, T, 8), seed=6)
    y_np = np.array([0, 2, 1, 1], dtype=np.int32)
    x, y = torch.from_numpy(x_np).to(dev), torch.from_numpy(y_np).to(dev)
    xn = {}
    for name, crop in (("plain", None), ("cropped", nsd.Crop(W, R))):
        torch.manual_seed(5)
        tr = Trainer(nsd.EEG_LSTM().to(dev).train(), seed=9, augment=A, loss=L, crop=crop)
        xs, ys = tr.static_inputs(B, T)
        xs.copy_(x); ys.copy_(y)
        for _ in range(2):
            tr.step_static(B, T)
        xn[name] = tr._buffers(*tr.recipe.dims(B, T))["xn"].clone()
        seed = tr.seed
    assert torch.equal(xn["plain"], xn["cropped"]) and _same(xn["plain"], ar.augment(x_np, seed, 8, 3, 0.2, 0.25, 0.3))
    torch.manual_seed(5)
    r = StepRecipe(nsd.EEG_LSTM().to(dev), True, A, L, dev, crop=nsd.Crop(W, R))
    xm, labels, tg = r.prepare(x, y, [seed], 2)
    a_np = ar.augment(x_np, seed, 8, 3, 0.2, 0.25, 0.3)
    c_np, l_np, _, _ = cr.crop(a_np, W, R, 0, seed, 8, labels=y_np)
    m_np, t_np = mr.mixup(c_np, l_np, 3, seed, 8, mix=0.7, eps=0.1)
    assert labels is None and _same(xm, m_np) and _same(tg, t_np)


# ---- nsd_crop_pool --------------------------------------------------------------------------------------------------------------------
def _ulps(a: np.ndarray, b: np.ndarray) -> int:
    """largest distance in fp32 steps between two arrays of finite values of equal sign (equal infinities count 0)"""
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    ai, bi = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    assert np.isfinite(a[~same]).all() and np.isfinite(b[~same]).all()
    return int(np.abs(ai - bi)[~same].max()) if (~same).any() else 0


@pytest.mark.parametrize("N,R,Kk", [(7, 4, 3), (300, 5, 8), (3, 1, 2), (2, 64, 1), (1030, 3, 5)])
def test_crop_pool_equals_numpy(nsd, dev, N, R, Kk):
    """probs_out bit for bit; logits_out within 1 fp32 ulp of float32(log(float64(mean))): a double log good to 1 ulp moves the rounded
    float by at most one step"""
    from nsd_amd import ops
    rs = np.random.RandomState(N + R)
    p_np = rs.dirichlet(np.ones(max(Kk, 2)), (N, R)).astype(np.float32)[..., :Kk]
    p_np[0, 0] = 0.0                                                # log 0 = -inf (only with R = 1), an exact zero among the terms
    p = torch.from_numpy(np.ascontiguousarray(p_np)).to(dev)
    (out, c1), (lg, c2) = guarded((N, Kk), torch.float32, dev, "nan32"), guarded((N, Kk), torch.float32, dev, "nan32")
    snap = snapshot(p)
    got = ops.crop_pool(p, out=out, logits=lg)
    torch.cuda.synchronize()
    c1("probs_out"); c2("logits_out")
    assert got[0] is out and got[1] is lg and snap.unchanged()
    mean, log64 = cr.pool(p_np)
    assert _same(out, mean)
    assert _ulps(lg.cpu().numpy(), log64.astype(np.float32)) <= 1
    assert ops.crop_pool(p, want_logits=False)[1] is None
    # counts: rows of their own, bad counts and non-finite counted values -> NaN rows (probabilities and logarithms alike)
    counts_np = rs.randint(1, R + 1, N).astype(np.int32)
    q_np = p_np.copy()
    if N >= 7:
        counts_np[1], counts_np[2], counts_np[3] = 0, R + 1, -4
        counts_np[4], counts_np[5] = R, max(R - 1, 1)
        q_np[4, R - 1, Kk - 1] = np.nan                             # counted: the whole row is NaN
        q_np[5, R - 1, 0] = np.inf                                  # counted only when R = 1
        q_np[6, 0, 0], counts_np[6] = -np.inf, 1
    q = torch.from_numpy(np.ascontiguousarray(q_np)).to(dev)
    out2, lg2 = ops.crop_pool(q, torch.from_numpy(counts_np).to(dev))
    mean2, log2 = cr.pool(q_np, counts_np)
    got2 = out2.cpu().numpy()
    assert np.array_equal(np.isnan(got2), np.isnan(mean2)) and _same(torch.nan_to_num(out2, nan=-1.0), np.nan_to_num(mean2, nan=-1.0))
    assert np.array_equal(np.isnan(lg2.cpu().numpy()), np.isnan(log2))
    if N >= 7:
        assert np.isnan(got2[[1, 2, 3, 4, 6]]).all() and np.isnan(got2[5]).all() == (R == 1) and not np.isnan(got2[0]).any()


def _ref_model(nsd, dev, ref_state, **kw):
    from tests.gpu_harness import model_from_state
    return model_from_state(nsd, dev, ref_state, **kw).eval()


def test_crop_pool_takes_a_sliding_decoders_output_as_it_is(nsd, dev, ref_state):
    """probs [B,D,K] + counts straight from nsd_window_step: rows beyond the count are NaN there and are not read"""
    from nsd_amd import ops
    model = _ref_model(nsd, dev, ref_state)
    sp, flat = model.spec, model.flat_parameters()
    B, T, W, hop = 3, 20, 8, 4
    x = torch.from_numpy(_x((B, T, 8), seed=12)).to(dev)
    state = ops.window_state(sp, W, hop, B, dev)
    _, probs, _, counts = ops.window_step(sp, flat, x, state, window=W, hop=hop)
    assert tuple(probs.shape) == (B, 5, 3) and counts.tolist() == [4] * B and torch.isnan(probs[:, 4]).all()
    pooled, lg = ops.crop_pool(probs, counts)
    mean, _ = cr.pool(probs.cpu().numpy(), counts.cpu().numpy())
    assert _same(pooled, mean) and not torch.isnan(pooled).any() and torch.equal(lg.argmax(-1), pooled.argmax(-1))


# ---- the trainers ---------------------------------------------------------------------------------------------------------------------
BT, TT, WT, RT = 4, 20, 8, 3                                        # (B, T, W, R) of the composition tests: 12 rows of 8 samples


def _model(nsd, dev, seed, *a, **kw):
    torch.manual_seed(seed)
    return nsd.EEG_LSTM(*a, **kw).to(dev).train()


def _batch(dev, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return (2.7 * torch.randn((B, T, 8), generator=g)).to(dev), torch.randint(0, 3, (B,), generator=g, dtype=torch.int32).to(dev)


@pytest.mark.parametrize("case", ["fp32", "fp32_normalize", "bf16_h64"])
def test_trainer_step_equals_plain_step_on_hand_cropped_input(nsd, dev, case):
    """Trainer(crop=c).step(x, y) leaves bitwise the parameters, Adam moments and loss of Trainer().step(*ops.crop(x, c, seed, 4 * step,
    labels=y)) on the [12, 8, C] batch, over three steps (different batches).  With normalize the plain trainer z-scores what it is
    given: the crops, as the cropped one does."""
    from nsd_amd import ops
    from nsd_amd.trainer import Trainer
    args = (8, 64, 2, 3, 0.6) if case.startswith("bf16") else ()
    kw = dict(precision="bf16") if case.startswith("bf16") else dict(normalize=case.endswith("normalize"))
    c = nsd.Crop(WT, RT)
    ma, mb = _model(nsd, dev, 11, *args, **kw), _model(nsd, dev, 11, *args, **kw)
    ta, tb = Trainer(ma, lr=1e-3, seed=9, crop=c), Trainer(mb, lr=1e-3, seed=9)
    assert ta.crop == c and tb.crop is None and ta.seed == tb.seed
    assert ma.crop == c and mb.crop is None                         # the trained window travels with the model (and its checkpoints)
    for step in range(1, 4):
        x, y = _batch(dev, BT, TT, seed=step)
        ta.step(x, y)
        xc, yc, _ = ops.crop(x, c, dict(seed=tb.seed, base_stream=4 * step), labels=y)
        assert tuple(xc.shape) == (BT * RT, WT, 8)
        tb.step(xc, yc)
        assert torch.equal(ta.flat, tb.flat) and torch.equal(ta.m, tb.m) and torch.equal(ta.v, tb.v), step
        assert ta.last_loss() == tb.last_loss(), step
    assert not torch.equal(ta.flat, _model(nsd, dev, 11, *args, **kw).flat_parameters())


def test_graph_replay_step_equals_eager_step_with_a_crop(nsd, dev):
    """step_static (replayed) against the eager step over three steps: the crops and their labels of every replay are the
    host-numbered launch, and parameters and Adam moments are compared bit for bit"""
    from nsd_amd import ops
    from nsd_amd.trainer import Trainer
    c = nsd.Crop(WT, RT)
    x, y = _batch(dev, BT, TT, seed=8)
    ma, mb = _model(nsd, dev, 21), _model(nsd, dev, 21)
    ta, tb = Trainer(ma, lr=1e-3, seed=5, crop=c), Trainer(mb, lr=1e-3, seed=5, crop=c)
    xs, ys = tb.static_inputs(BT, TT)
    assert tuple(xs.shape) == (BT, TT, 8) and tuple(ys.shape) == (BT,)
    xs.copy_(x); ys.copy_(y)
    for step in range(1, 4):
        ta.step(x, y)
        tb.step_static(BT, TT)
        xc, yc, _ = ops.crop(x, c, dict(seed=tb.seed, base_stream=4 * step), labels=y)
        buf = tb._buffers(BT * RT, WT)
        assert torch.equal(buf["xc"], xc) and torch.equal(buf["yc"], yc), step
        dp = (ta.flat - tb.flat).abs().max().item()
        print(f"crop graph step {step}: grads equal {torch.equal(ta.grads, tb.grads)} max |dp| {dp:.3e} m equal {torch.equal(ta.m, tb.m)}")
        assert torch.equal(ta.grads, tb.grads), step
        assert torch.equal(ta.flat, tb.flat) and torch.equal(ta.m, tb.m) and torch.equal(ta.v, tb.v), step
    assert tb.step_count == 3 and int(tb._step_dev.item()) == 3 and ta.last_loss() == tb.last_loss()


@pytest.mark.parametrize("shared", [False, True])
def test_model_batch_trainer_equals_separate_trainers_with_a_crop(nsd, dev, shared):
    from nsd_amd.trainer import Trainer
    M, c, seeds = 3, nsd.Crop(WT, RT), [3, 4, 5]
    batched = [_model(nsd, dev, 100 + m) for m in range(M)]
    singles = [_model(nsd, dev, 100 + m) for m in range(M)]
    tr = nsd.ModelBatchTrainer(batched, lr=1e-3, seeds=seeds, crop=c)
    trs = [Trainer(singles[m], lr=1e-3, seed=seeds[m], crop=c) for m in range(M)]
    assert all(m.crop == c for m in batched + singles)
    for step in range(1, 4):
        g = torch.Generator().manual_seed(step)
        xs = torch.randn((M, BT, TT, 8), generator=g).to(dev)
        ys = torch.randint(0, 3, (M, BT), generator=g, dtype=torch.int32).to(dev)
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
        assert not torch.equal(tr.grads[0], tr.grads[1])          # own offsets (and own parameters) per model
    with pytest.raises(nsd.NsdError, match="not a per-model setting"):
        nsd.ModelBatchTrainer([_model(nsd, dev, 200 + m) for m in range(2)], crop=[c, nsd.Crop(WT, 2)])


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
def test_crop_off_is_todays_launch_sequence(nsd, dev, normalize):
    from nsd_amd.trainer import Trainer
    x, y = _batch(dev, BT, TT, seed=2)
    c = nsd.Crop(WT, RT)

    def run(**kw):
        return _launches(Trainer(_model(nsd, dev, 3, normalize=normalize), lr=1e-3, seed=4, **kw), x, y)
    base = run()
    assert base and "nsd_crop" not in base and run(crop=None) == base
    on = run(crop=c)
    assert on.count("nsd_crop") == 2 and len(on) == len(base) + 2 and [n for n in on if n != "nsd_crop"] == base
    if normalize:                                                   # the z-score moved behind the cut: it is of what the model sees
        assert [n for n in on if n in ("nsd_crop", "nsd_zscore_fwd")] == ["nsd_crop", "nsd_zscore_fwd"] * 2
    A = nsd.Augment(noise_std=0.3)
    aug = run(augment=A, crop=c)
    assert [n for n in aug if n in ("nsd_augment", "nsd_crop", "nsd_zscore_fwd")] == (["nsd_augment", "nsd_crop"] + ["nsd_zscore_fwd"] * normalize) * 2

    def run_multi(**kw):
        models = [_model(nsd, dev, 30 + m, normalize=normalize) for m in range(3)]
        return _launches(nsd.ModelBatchTrainer(models, lr=1e-3, seeds=[1, 2, 3], **kw), x, y)
    mbase = run_multi()
    assert "nsd_crop" not in mbase and run_multi(crop=None) == mbase
    mon = run_multi(crop=c)
    assert mon.count("nsd_crop") == 2 and [n for n in mon if n != "nsd_crop"] == mbase


# ---- trial-level evaluation -----------------------------------------------------------------------------------------------------------
def test_evaluate_with_a_crop_equals_the_hand_composition(nsd, dev):
    """crop -> multi_infer -> pool -> multi_eval by hand gives evaluate(crop=)'s records; unequal counts; a NaN sample in one trial makes
    that trial non-finite and no other"""
    from nsd_amd import ops
    M, B, T = 3, 6, 20
    grid = nsd.Crop.grid(T, 8, 4)
    assert grid == nsd.Crop(8, 4, 4)
    models = [_model(nsd, dev, 300 + m) for m in range(M)]
    tr = nsd.ModelBatchTrainer(models, seeds=[1, 2, 3], crop=nsd.Crop(8, 3))
    g = torch.Generator().manual_seed(1)
    x = (2.7 * torch.randn((M, B, T, 8), generator=g)).to(dev)
    y = torch.randint(0, 3, (M, B), generator=g, dtype=torch.int32).to(dev)
    counts = [6, 5, 4]

    def by_hand(x):
        xc, _, _ = ops.crop(x, grid)
        assert tuple(xc.shape) == (M, B * 4, 8, 8)
        _, probs = ops.multi_infer(tr.spec, tr.params, xc)
        pooled, lg = ops.crop_pool(probs.view(M * B, 4, 3))
        return ops.eval_records(ops.multi_eval(lg.view(M, B, 3), y.contiguous(), counts=counts), M, 3), pooled.view(M, B, 3)

    def same(a, b):
        return all(ra["n"] == rb["n"] and ra["nonfinite"] == rb["nonfinite"] and np.array_equal(ra["confusion"], rb["confusion"])
                   and (ra["loss"] == rb["loss"] or (ra["loss"] != ra["loss"] and rb["loss"] != rb["loss"])) and ra["acc"] == rb["acc"]
                   for ra, rb in zip(a, b))
    got = tr.evaluate(x, y, counts=counts, crop=grid)
    want, pooled = by_hand(x)
    assert same(got, want) and [r["n"] for r in got] == counts and all(r["nonfinite"] == 0 for r in got)
    # the records are those of the pooled decisions: accuracy from the pooled argmax, loss = mean of -log pooled[label]
    for m in range(M):
        p = pooled[m, :counts[m]].cpu().double()
        lab = y[m, :counts[m]].long().cpu()
        assert got[m]["acc"] == float((p.argmax(-1) == lab).double().mean())
        # (nsd_multi_eval forms logsumexp(l) - l_y in double from l = float(log(pooled)): l_y carries one fp32 rounding, 6e-8 * |l_y|
        # with |l_y| < 10 here, and the row of pooled probabilities sums to 1 within a few fp32 steps: 2e-6 covers both)
        assert abs(got[m]["loss"] - float(-torch.log(p.gather(1, lab[:, None])).mean())) < 2e-6
    # without crop= the whole trials are scored, as before
    assert [r["n"] for r in tr.evaluate(x, y, counts=counts)] == counts
    # a NaN sample in the last window of model 1's trial 2: that trial is non-finite, the others are what they were
    xb = x.clone()
    xb[1, 2, 19, 3] = float("nan")
    bad = tr.evaluate(xb, y, counts=counts, crop=grid)
    assert [r["nonfinite"] for r in bad] == [0, 1, 0] and [r["n"] for r in bad] == [6, 4, 4] and bad[1]["loss"] != bad[1]["loss"]
    assert same([bad[0], bad[2]], [got[0], got[2]]) and same(bad, by_hand(xb)[0])
    # track_best runs its rule on the pooled metrics; a drawn crop is refused (an evaluation draws nothing)
    tb = tr.track_best(x, y, counts=counts, crop=grid)
    assert same(tb, got) and [r["best_eval"] for r in tb] == [1, 1, 1]
    with pytest.raises(nsd.NsdError, match="regular grid"):
        tr.evaluate(x, y, crop=nsd.Crop(8, 3))
    # shared trials
    assert same(tr.evaluate(x[0].contiguous(), y[0].contiguous(), crop=grid)[:1], tr.evaluate(x[:1].expand(M, B, T, 8).contiguous(), y[:1].expand(M, B).contiguous(), crop=grid)[:1])


# ---- train / serve agreement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,W,hop", [(20, 8, 4), (41, 10, 5), (12, 4, 4)])
def test_crops_of_a_regular_grid_are_the_sliding_decoders_windows(nsd, dev, ref_state, T, W, hop):
    """nsd_infer on crop r of a trial against decision r of nsd_window_step(W, hop) on the same trial, at the bounds
    tests/test_gpu_stream.py holds the stream readout to: logits 1e-4, probabilities 1e-5, the same argmax outside its ARGMAX_GAP"""
    from nsd_amd import ops
    model = _ref_model(nsd, dev, ref_state)
    sp, flat = model.spec, model.flat_parameters()
    B = 3
    x = torch.from_numpy(_x((B, T, 8), seed=T)).to(dev)
    grid = nsd.Crop.grid(T, W, hop)
    xc, _, _ = ops.crop(x, grid)
    lg_c, pr_c = ops.infer(sp, flat, xc)
    state = ops.window_state(sp, W, hop, B, dev)
    lg_w, pr_w, ends, counts = ops.window_step(sp, flat, x, state, window=W, hop=hop)
    R = grid.crops
    assert counts.tolist() == [R] * B and ends[:, :R].tolist() == [[r * hop + W for r in range(R)]] * B
    a, b = lg_c.view(B, R, 3).cpu().numpy(), lg_w[:, :R].cpu().numpy()
    e_l = float(np.abs(a - b).max())
    e_p = float(np.abs(pr_c.view(B, R, 3).cpu().numpy() - pr_w[:, :R].cpu().numpy()).max())
    print(f"crop vs window T={T} W={W} hop={hop}: logits {e_l:.2e} probs {e_p:.2e}")
    assert e_l < LOGIT_TOL and e_p < PROB_TOL
    top = np.sort(a, axis=-1)
    clear = (top[..., -1] - top[..., -2]) > ARGMAX_GAP
    assert np.array_equal(a.argmax(-1)[clear], b.argmax(-1)[clear])
    # and the model's own trial-level surface is that pooling
    pooled, wins = model.predict_trials(x, hop=hop, window=W)
    assert torch.equal(wins.view(-1, 3), pr_c) and torch.equal(pooled, ops.crop_pool(pr_c.view(B, R, 3), want_logits=False)[0])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(nsd, dev):
    """every refusal of nsd_crop / nsd_crop_pool once, on real device buffers: NSD_E_INVALID with a text, the outputs at their fill"""
    from nsd_amd import _lib
    L = nsd.load_library()
    B, T, Cc, W, R = SHAPES[0]
    x = torch.from_numpy(_x((3, B, T, Cc), seed=1)).to(dev)
    lab = torch.zeros(3 * B, dtype=torch.int32, device=dev)
    tg = torch.zeros((3 * B, K), dtype=torch.float32, device=dev)
    y = torch.empty(3 * B * 64 * T * Cc, dtype=torch.uint8, device=dev).fill_(GUARD_BYTE)       # room for every legal shape, as bytes
    lo = torch.empty(3 * B * 64 * 4, dtype=torch.uint8, device=dev).fill_(GUARD_BYTE)
    to = torch.empty(3 * B * 64 * K * 4, dtype=torch.uint8, device=dev).fill_(GUARD_BYTE)
    n = B * T * Cc
    d = _lib.Dims(B, T, Cc, 48, 2, K, 32)
    rng = (_lib.Rng * 32)()
    rp = C.cast(rng, C.c_void_p)

    def call(d=d, M=1, xp=x.data_ptr(), stride=0, cfg=(W, R, 0), rng=rp, labels=lab.data_ptr(), targets=tg.data_ptr(), yp=y.data_ptr(),
             lop=lo.data_ptr(), top=to.data_ptr()):
        c = _lib.CropCfg(*cfg) if cfg is not None else None
        return L.nsd_crop(C.byref(d), M, xp, stride, C.byref(c) if c is not None else None, rng, None, labels, targets, yp, lop, top, None,
                          torch.cuda.current_stream().cuda_stream)
    bad = [dict(M=0), dict(M=_lib.NSD_MAX_MODELS + 1), dict(cfg=(0, R, 0)), dict(cfg=(T + 1, R, 0)), dict(cfg=(W, 0, 0)),
           dict(cfg=(W, _lib.NSD_CROP_MAX + 1, 0)), dict(cfg=(W, R, -1)), dict(cfg=(W, R, 3)), dict(xp=None), dict(yp=None), dict(cfg=None),
           dict(rng=None), dict(labels=None), dict(targets=None), dict(M=3, stride=-1), dict(M=3, stride=n - 1),
           dict(xp=y.data_ptr(), yp=y.data_ptr()), dict(xp=y.data_ptr() + 4 * (B * R * W * Cc - 1)),
           dict(d=_lib.Dims(2 ** 30, T, Cc, 48, 2, K, 32), M=2)]
    for kw in bad:
        assert call(**kw) == -1 and L.nsd_last_error().startswith(b"crop:"), kw
    pool_bad = [dict(N=-1), dict(R=0), dict(Kk=0), dict(probs=None), dict(out=None), dict(N=2 ** 20, R=2 ** 10, Kk=4)]
    for kw in pool_bad:
        a = dict(N=4, R=3, Kk=K, probs=tg.data_ptr(), out=to.data_ptr())
        a.update(kw)
        assert L.nsd_crop_pool(a["N"], a["R"], a["Kk"], a["probs"], None, a["out"], lo.data_ptr(), torch.cuda.current_stream().cuda_stream) == -1, kw
        assert L.nsd_last_error().startswith(b"crop_pool:"), kw
    # B == 0 and N == 0 are fine and launch nothing
    assert call(d=_lib.Dims(0, T, Cc, 48, 2, K, 32)) == 0
    assert L.nsd_crop_pool(0, 3, K, tg.data_ptr(), None, to.data_ptr(), None, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    for buf, name in ((y, "y"), (lo, "labels_out"), (to, "targets_out")):
        assert bool((buf == GUARD_BYTE).all()), name
    # the Python surface refuses what the C entry point would, in its own words where it can
    from nsd_amd import ops
    with pytest.raises(nsd.NsdError):
        ops.crop(x[0].contiguous(), nsd.Crop(T + 1, 1), dict(seed=1, base_stream=0))
    with pytest.raises(nsd.NsdError, match="rng"):
        ops.crop(x[0].contiguous(), nsd.Crop(W, R))


# ---- checkpoints and prediction ---------------------------------------------------------------------------------------------------------
def test_checkpoint_carries_the_crop_and_the_predictor_pools(nsd, dev, ref_state, tmp_path):
    """save_reference_checkpoint writes the crop beside the weights, SimplePredictor rebuilds the model with it, predict_trial is the
    pooled decision of the trial's windows, open_stream defaults to the trained window; a checkpoint without the key loads as before"""
    from nsd_amd import ops
    from nsd_amd.trainer import save_reference_checkpoint
    from tests.gpu_harness import model_from_state, write_pth
    W, hop, T = 8, 4, 20
    model = model_from_state(nsd, dev, ref_state, crop=nsd.Crop(W, 3)).eval()
    path = str(tmp_path / "cropped.pth")
    save_reference_checkpoint(model, path)
    raw = torch.load(path, map_location="cpu", weights_only=True)
    assert sorted(raw) == ["nsd_crop", "state_dict"] and raw["nsd_crop"] == {"window": W, "crops": 3, "hop": 0}
    pred = nsd.SimplePredictor(path, sr=125, preprocess="identity")
    assert pred.model.crop == nsd.Crop(W, 3) and torch.equal(pred.model.flat_parameters(), model.flat_parameters())
    trial = _x((T, 8), seed=31)
    probs, label = pred.predict_trial(trial, hop_seconds=hop / 125.0)
    pooled, wins = model.predict_trials(torch.from_numpy(trial[None]).to(dev), hop=hop)
    assert tuple(wins.shape) == (1, 4, 3) and _same(pooled[0], probs) and label == pred.class_names[int(probs.argmax())]
    # each window is what predict() says of it, and the default hop is half the window
    for r in range(4):
        assert np.array_equal(pred.predict(trial[r * hop:r * hop + W])[0], wins[0, r].cpu().numpy())
    assert np.array_equal(pred.predict_trial(trial)[0], probs)
    stream = pred.open_stream(hop_seconds=hop / 125.0)
    assert (stream.decoder.window, stream.decoder.hop) == (W, hop)
    # a checkpoint of whole-trial training: no trained window, predict_trial says so, open_stream keeps its rule
    plain = nsd.SimplePredictor(write_pth(str(tmp_path), ref_state), sr=125, preprocess="identity")
    assert plain.model.crop is None
    with pytest.raises(nsd.NsdError, match="no trained window"):
        plain.predict_trial(trial)
    with pytest.raises(ValueError, match="go together"):
        plain.open_stream(hop_seconds=hop / 125.0)
    assert ops.Crop.grid(T, W, hop).crops == 4
