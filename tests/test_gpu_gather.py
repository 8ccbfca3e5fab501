"""Device-resident batches on the GPU: nsd_gather against its numpy restatement (tests/gather_ref.py) bit for bit -- both access paths,
the stride loop, every row rule, optional labels / targets, the buffer contract, side stream and graph replay, out-of-range indices --
and the trainers' bind_batches / step_scheduled against the host-fed steps they replace, bit for bit; the command-line flag."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import gather_ref as gr
from tests.buffer_contract import guarded, snapshot
from tests.gpu_harness import dev, nsd, sync_at_the_end  # noqa: F401  (fixtures; sync_at_the_end is autouse)
from tests.seq_bf16_harness import SHORT_SHAPES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _x(shape, seed=0):
    x = (2.7 * np.random.RandomState(seed).standard_normal(shape)).astype(np.float32)
    x.reshape(-1)[::7] = np.array([0x7FA00001], np.uint32).view(np.float32)[0]      # NaNs with a payload: a copy keeps them
    x.reshape(-1)[3::11] = -0.0
    return x


def _table(M, S, B, N, seed=1):
    """random indices; every model's table holds 0, N - 1 and (B > 2) a duplicate inside a batch"""
    t = np.random.RandomState(seed).randint(0, N, (M, S, B)).astype(np.int32)
    t[:, 0, 0] = 0
    t[:, -1, -1] = N - 1
    if B > 2:
        t[:, S // 2, 1] = t[:, S // 2, 0]
    return t


def _words(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _run(ops, dev, x_all, table, c, base=0, lab=None, tg=None, on_dev=False, x_dev=None):
    """one ops.gather_batch on fresh device copies -> (x, labels, targets, status) tensors"""
    xa = torch.from_numpy(x_all).to(dev) if x_dev is None else x_dev
    M = table.shape[0]
    st = torch.zeros(M, dtype=torch.int32, device=dev)
    kw = dict(step_dev=torch.tensor([c], dtype=torch.int64, device=dev), step=-12345) if on_dev else dict(step=c)
    x, lo, to = ops.gather_batch(xa, torch.from_numpy(table).to(dev), step_base=base, status=st,
                                 labels_all=None if lab is None else torch.from_numpy(lab).to(dev),
                                 targets_all=None if tg is None else torch.from_numpy(tg).to(dev), **kw)
    return x, lo, to, st


def _agrees(got, want) -> bool:
    x, lo, to, st = got
    xr, lr, tr, sr_ = want
    return (np.array_equal(_words(x).reshape(xr.shape), xr) and (lr is None) == (lo is None) and (tr is None) == (to is None)
            and (lr is None or np.array_equal(lo.cpu().numpy(), lr)) and (tr is None or np.array_equal(_words(to), tr))
            and np.array_equal(st.cpu().numpy(), sr_))


# ---- the kernel against its restatement ------------------------------------------------------------------------------------------------
# (M, N, S, B, T, C): the dword path (T * C = 15), the 16-byte path, a row longer than two passes of 256 lanes x 16 bytes plus a
# remainder (300 * 8 / 4 = 600 = 2 * 256 + 88), one model and three, a batch of one
SHAPES = [(1, 7, 4, 3, 5, 3), (3, 7, 4, 3, 5, 3), (1, 7, 4, 3, 6, 8), (3, 7, 4, 3, 6, 8), (3, 7, 2, 3, 300, 8), (2, 5, 3, 1, 6, 8), (2, 5, 3, 1, 5, 3)]


@pytest.mark.parametrize("M,N,S,B,T,Cc", SHAPES)
def test_gather_equals_numpy_bitwise(nsd, dev, M, N, S, B, T, Cc):
    from nsd_amd import ops
    x_all, table = _x((N, T, Cc), seed=M + T), _table(M, S, B, N)
    assert M == 1 or not np.array_equal(table[0], table[1])                          # the models have tables of their own
    lab = np.random.RandomState(2).randint(0, 3, N).astype(np.int32)
    tg = _x((N, 3), seed=3)
    for c in range(S):                                                               # every row
        assert _agrees(_run(ops, dev, x_all, table, c, lab=lab, tg=tg), gr.gather(x_all, table, c, 0, lab, tg)), c
    # a [S,B] table is one model's, and the output then has no model axis
    x1, l1, _ = ops.gather_batch(torch.from_numpy(x_all).to(dev), torch.from_numpy(table[0]).to(dev), step=1,
                                 labels_all=torch.from_numpy(lab).to(dev))
    want = gr.gather(x_all, table[:1], 1, 0, lab)
    assert tuple(x1.shape) == (B, T, Cc) and np.array_equal(_words(x1), want[0][0]) and np.array_equal(l1.cpu().numpy(), want[1])


def test_misaligned_source_takes_the_dword_path_and_stays_exact(nsd, dev):
    from nsd_amd import ops
    M, N, S, B, T, Cc = 3, 7, 4, 3, 6, 8
    x_all, table = _x((N, T, Cc), seed=5), _table(M, S, B, N)
    flat = torch.empty(N * T * Cc + 1, dtype=torch.float32, device=dev)
    xu = flat[1:].view(N, T, Cc)
    xu.copy_(torch.from_numpy(x_all))
    assert xu.data_ptr() % 16 == 4 and xu.is_contiguous()
    assert _agrees(_run(ops, dev, x_all, table, 2, x_dev=xu), gr.gather(x_all, table, 2))
    # ... and a misaligned destination
    out = torch.empty(M * B * T * Cc + 1, dtype=torch.float32, device=dev)[1:]
    ops.gather_batch(torch.from_numpy(x_all).to(dev), torch.from_numpy(table).to(dev), step=3, out=out)
    assert np.array_equal(_words(out).reshape(M, B, T, Cc), gr.gather(x_all, table, 3)[0])


@pytest.mark.parametrize("on_dev", [False, True])
def test_row_selection(nsd, dev, on_dev):
    """S = 4: counters below step_base, inside the table and two wraps past it, with base 0 and a non-zero base, from the host's step
    and from the device counter (the host's step is then ignored)"""
    from nsd_amd import ops
    M, N, S, B, T, Cc = 2, 7, 4, 3, 5, 3
    x_all, table = _x((N, T, Cc), seed=6), _table(M, S, B, N, seed=4)
    assert len({table[0, r].tobytes() for r in range(S)}) == S                       # the rows differ: a wrong row shows
    for base in (0, 10, -3):
        for c in (base - 5, base - 1, base, base + 1, base + 3, base + S, base + 2 * S + 1, base + 3 * S - 1):
            got = _run(ops, dev, x_all, table, c, base, on_dev=on_dev)
            assert _agrees(got, gr.gather(x_all, table, c, base)), (base, c)
            assert np.array_equal(_words(got[0])[0], x_all.view(np.uint32)[table[0, gr.row(c, base, S)]]), (base, c)


@pytest.mark.parametrize("K", [3, 5])
@pytest.mark.parametrize("pairs", ["labels", "targets", "both", "neither"])
def test_optional_labels_and_targets(nsd, dev, pairs, K):
    from nsd_amd import ops
    M, N, S, B, T, Cc = 2, 7, 3, 3, 6, 8
    x_all, table = _x((N, T, Cc), seed=7), _table(M, S, B, N, seed=5)
    lab = np.arange(10, 10 + N, dtype=np.int32) if pairs in ("labels", "both") else None
    tg = _x((N, K), seed=8) if pairs in ("targets", "both") else None
    got = _run(ops, dev, x_all, table, 1, lab=lab, tg=tg)
    assert (got[1] is None) == (lab is None) and (got[2] is None) == (tg is None)
    assert _agrees(got, gr.gather(x_all, table, 1, 0, lab, tg))


@pytest.mark.parametrize("fill", ["nan32", "ones"])
@pytest.mark.parametrize("T,Cc", [(5, 3), (6, 8), (300, 8)])
def test_buffer_contract(nsd, dev, fill, T, Cc):
    """outputs of exactly the stated size between 0xA5 guards, pre-filled: nothing outside is written, nothing of the fill shows, the
    inputs keep their bits"""
    from nsd_amd import ops
    M, N, S, B, K = 3, 7, 2, 3, 5
    x_all, table = _x((N, T, Cc), seed=9), _table(M, S, B, N, seed=6)
    lab, tg = np.arange(N, dtype=np.int32) + 1, _x((N, K), seed=10)
    xa, tb, la, ta = (torch.from_numpy(a).to(dev) for a in (x_all, table, lab, tg))
    x, cx = guarded((M, B, T, Cc), torch.float32, dev, fill)
    lo, cl = guarded((M * B,), torch.int32, dev, fill)
    to, ct = guarded((M * B, K), torch.float32, dev, fill)
    st, cs = guarded((M,), torch.int32, dev, "zeros")
    before = snapshot(xa, tb, la, ta)
    ops.gather_batch(xa, tb, step=1, labels_all=la, targets_all=ta, out=x, labels_out=lo, targets_out=to, status=st)
    torch.cuda.synchronize()
    cx("x"); cl("labels"); ct("targets"); cs("status")
    assert before.unchanged()
    assert _agrees((x, lo, to, st), gr.gather(x_all, table, 1, 0, lab, tg))


def test_empty_batch_leaves_the_outputs_untouched(nsd, dev):
    import ctypes as C

    from nsd_amd import _lib, ops
    xa, la = torch.from_numpy(_x((7, 6, 8))).to(dev), torch.arange(7, dtype=torch.int32, device=dev)
    tb = torch.zeros((2, 3, 4), dtype=torch.int32, device=dev)
    # through the C ABI with B = 0 and real buffers (more than the call may touch: it touches nothing) ...
    x, cx = guarded((2, 4, 6, 8), torch.float32, dev, "ones")
    lo, cl = guarded((8,), torch.int32, dev, "ones")
    st, cs = guarded((2,), torch.int32, dev, "ones")
    d = _lib.Dims(0, 6, 8, 1, 1, 1, 1)
    ops._call("nsd_gather", dev, C.byref(d), 2, 7, xa.data_ptr(), la.data_ptr(), None, tb.data_ptr(), 3, 0, None, 0, x.data_ptr(),
              lo.data_ptr(), None, st.data_ptr(), ops.STREAM)
    torch.cuda.synchronize()
    cx("x"); cl("labels"); cs("status")
    assert (x.view(torch.int32) == -1).all() and (lo == -1).all() and (st == -1).all()
    # ... and through the wrapper, whose empty outputs have no address to hand over
    xo, lo2, _ = ops.gather_batch(xa, tb[:, :, :0], step=0, labels_all=la, status=st)
    assert tuple(xo.shape) == (2, 0, 6, 8) and lo2.numel() == 0 and (st == -1).all()


def test_side_stream_and_graph_replay_give_the_same_bits(nsd, dev):
    from nsd_amd import ops
    M, N, S, B, T, Cc = 3, 7, 4, 3, 6, 8
    x_all, table = _x((N, T, Cc), seed=11), _table(M, S, B, N, seed=7)
    lab = np.arange(N, dtype=np.int32)
    xa, tb, la = (torch.from_numpy(a).to(dev) for a in (x_all, table, lab))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = ops.gather_batch(xa, tb, step=2, labels_all=la)
    torch.cuda.current_stream().wait_stream(side)
    want = gr.gather(x_all, table, 2, 0, lab)
    assert np.array_equal(_words(got[0]), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
    step_dev = torch.tensor([5], dtype=torch.int64, device=dev)
    x, lo = torch.full((M, B, T, Cc), float("nan"), device=dev), torch.full((M * B,), -1, dtype=torch.int32, device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.gather_batch(xa, tb, step_dev=step_dev, step_base=3, labels_all=la, out=x, labels_out=lo)       # warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.gather_batch(xa, tb, step_dev=step_dev, step_base=3, labels_all=la, out=x, labels_out=lo)
    for c in (3, 4, 6, 9, 1):                                                        # the replay reads its row from the counter
        step_dev.fill_(c)
        x.fill_(float("nan")); lo.fill_(-1)
        g.replay()
        want = gr.gather(x_all, table, c, 3, lab)
        assert np.array_equal(_words(x), want[0]) and np.array_equal(lo.cpu().numpy(), want[1]), c


def test_out_of_range_indices_give_nan_rows_and_a_status_bit(nsd, dev):
    from nsd_amd import ops
    M, N, S, B, K = 3, 7, 2, 4, 3
    for T, Cc in ((5, 3), (6, 8)):
        x_all = (2.7 * np.random.RandomState(12).standard_normal((N, T, Cc))).astype(np.float32)       # finite: a NaN is the fault's
        table = _table(M, S, B, N, seed=8)
        table[1, 1, 1], table[1, 1, 3] = N, -1
        lab, tg = np.arange(N, dtype=np.int32) + 1, np.ones((N, K), np.float32)
        xa, tb, la, ta = (torch.from_numpy(a).to(dev) for a in (x_all, table, lab, tg))
        x, cx = guarded((M, B, T, Cc), torch.float32, dev, "zeros")
        lo, cl = guarded((M * B,), torch.int32, dev, "ones")
        to, ct = guarded((M * B, K), torch.float32, dev, "zeros")
        st = torch.zeros(M, dtype=torch.int32, device=dev)
        ops.gather_batch(xa, tb, step=1, labels_all=la, targets_all=ta, out=x, labels_out=lo, targets_out=to, status=st)
        torch.cuda.synchronize()
        cx("x"); cl("labels"); ct("targets")
        assert st.tolist() == [0, 1, 0]
        for b in (1, 3):
            assert (_words(x[1, b]) == 0x7FC00000).all() and (_words(to[B + b]) == 0x7FC00000).all() and int(lo[B + b]) == 0
        assert _agrees((x, lo, to, st), gr.gather(x_all, table, 1, 0, lab, tg))       # every other row is exact
        assert int(torch.isnan(x).reshape(M * B, -1).any(1).sum()) == 2
        # the other row of the table has no fault: the status stays clear
        st.zero_()
        ops.gather_batch(xa, tb, step=0, out=x, status=st)
        assert st.tolist() == [0, 0, 0] and not torch.isnan(x).any()


def test_refusals_launch_nothing(nsd, dev):
    from nsd_amd import ops
    xa = torch.zeros(7, 6, 8, device=dev)
    tb = torch.zeros((2, 3, 3), dtype=torch.int32, device=dev)
    with pytest.raises(nsd.NsdError, match="overlaps"):
        ops.gather_batch(xa, tb, out=xa.view(-1)[:2 * 3 * 6 * 8])
    with pytest.raises(nsd.NsdError, match="out has"):
        ops.gather_batch(xa, tb, out=torch.empty(5, device=dev))
    with pytest.raises(nsd.NsdError, match="labels_all"):
        ops.gather_batch(xa, tb, labels_all=torch.zeros(6, dtype=torch.int32, device=dev))
    with pytest.raises(nsd.NsdError, match="status"):
        ops.gather_batch(xa, tb, status=torch.zeros(3, dtype=torch.int32, device=dev))
    with pytest.raises(nsd.NsdError, match="step_dev"):
        ops.gather_batch(xa, tb, step_dev=torch.zeros(1, dtype=torch.int32, device=dev))


# ---- the trainers: a scheduled step is the host-fed step ------------------------------------------------------------------------------------
NT, BT, TT, EP = 10, 4, 16, 2                                        # 10 trials, batches of 4: 2 steps per epoch, 2 epochs


def _model(nsd, dev, seed, *a, **kw):
    torch.manual_seed(seed)
    return nsd.EEG_LSTM(*a, **kw).to(dev).train()


def _trials(dev, seed=0, Cc=8):
    g = torch.Generator().manual_seed(seed)
    return (2.7 * torch.randn((NT, TT, Cc), generator=g)).to(dev), torch.randint(0, 3, (NT,), generator=g, dtype=torch.int32).to(dev)


def _recipe(nsd):
    return dict(augment=nsd.Augment(max_shift=2, scale_range=0.1, p_channel=0.2, noise_std=0.3),
                loss=nsd.Loss(label_smoothing=0.1, mixup=0.5))


def _same_state(ta, tb) -> bool:
    return torch.equal(ta.flat, tb.flat) and torch.equal(ta.m, tb.m) and torch.equal(ta.v, tb.v)


@pytest.mark.parametrize("case", ["fp32", "crop", "bf16"])
def test_scheduled_step_equals_the_host_fed_step(nsd, dev, case):
    """Trainer fed by train.py's host loop against bind_batches + step_scheduled(): parameters, Adam moments and loss bit for bit after
    every step -- dropout, augmentation, label smoothing and mixup on; with a crop; on the bf16 sequence path (eager)."""
    from nsd_amd import data as D
    from nsd_amd.trainer import Trainer
    H, L = SHORT_SHAPES[0]
    args = (8, H, L, 3, 0.6) if case == "bf16" else ()
    kw = dict(precision="bf16") if case == "bf16" else {}
    opt = dict(crop=nsd.Crop(8, 2, 0)) if case == "crop" else {}
    x_all, y_all = _trials(dev)
    tr_idx, seed = np.array([0, 1, 2, 3, 5, 6, 7, 8, 9]), 3           # trial 4 is held out
    ta = Trainer(_model(nsd, dev, 11, *args, **kw), lr=1e-3, seed=9, **_recipe(nsd), **opt)
    tb = Trainer(_model(nsd, dev, 11, *args, **kw), lr=1e-3, seed=9, **_recipe(nsd), **opt)
    sched = D.BatchSchedule.for_run(tr_idx, BT, seed, EP)
    assert sched.steps == 4 and sched.steps_per_epoch == 2
    tb.bind_batches(D.DeviceTrialSet(x_all, y_all, dev), sched)
    tr_dev = torch.from_numpy(tr_idx).to(dev)
    start = ta.flat.clone()
    for epoch in range(EP):
        for idx in D.epoch_batches(len(tr_idx), BT, seed, epoch, drop_last=True):
            sel = tr_dev[torch.from_numpy(idx).to(dev)]
            ta.step(x_all[sel].contiguous(), y_all[sel].contiguous(), global_batch=len(idx))
            tb.step_scheduled()
            assert _same_state(ta, tb), (epoch, ta.step_count)
            assert ta.last_loss() == tb.last_loss()
    assert ta.step_count == tb.step_count == 4 and not torch.equal(ta.flat, start)
    with pytest.raises(nsd.NsdError, match="4 steps are taken"):
        tb.step_scheduled()
    assert tb.step_count == 4
    if case == "bf16":
        with pytest.raises(nsd.NsdError, match="fp32 path only"):
            tb.step_static(BT, TT)


def test_scheduled_graph_step_equals_step_static_filled_by_hand(nsd, dev):
    """step_scheduled(static=True) -- the gather captured as the graph's first node behind the counter -- against step_static on
    inputs the host fills, bit for bit after every step; a second schedule of the same shape keeps the graph, another shape drops it."""
    from nsd_amd import data as D
    from nsd_amd.trainer import Trainer
    x_all, y_all = _trials(dev, seed=1)
    tr_idx, seed = np.arange(NT), 5
    ta, tb = Trainer(_model(nsd, dev, 21), lr=1e-3, seed=4, **_recipe(nsd)), Trainer(_model(nsd, dev, 21), lr=1e-3, seed=4, **_recipe(nsd))
    trials = D.DeviceTrialSet(x_all, y_all, dev)
    tb.bind_batches(trials, D.BatchSchedule.for_run(tr_idx, BT, seed, EP))
    xs, ys = ta.static_inputs(BT, TT)

    def run(seed_):
        for epoch in range(EP):
            for idx in D.epoch_batches(NT, BT, seed_, epoch, drop_last=True):
                sel = torch.from_numpy(idx).to(dev)
                xs.copy_(x_all[sel]); ys.copy_(y_all[sel])
                ta.step_static(BT, TT)
                tb.step_scheduled(static=True)
                assert torch.equal(tb._buffers(BT, TT)["x"], xs) and torch.equal(tb._buffers(BT, TT)["y"], ys), ta.step_count
                assert torch.equal(ta.grads, tb.grads) and _same_state(ta, tb), ta.step_count
                assert ta.last_loss() == tb.last_loss()
    run(seed)
    assert ta.step_count == tb.step_count == 4 == int(tb._step_dev.item())
    with pytest.raises(nsd.NsdError, match="4 steps are taken"):
        tb.step_scheduled(static=True)
    # a second schedule of the same shape: copied into the bound table, the captured graph stays
    key = ("scheduled", BT, TT)
    graph = tb._graphs[key]
    table_at = tb._bound["table"].data_ptr()
    tb.bind_batches(trials, D.BatchSchedule.for_run(tr_idx, BT, seed + 1, EP))
    assert tb._graphs[key] is graph and tb._bound["table"].data_ptr() == table_at
    run(seed + 1)
    assert tb._graphs[key] is graph and tb.step_count == 8
    # ... also when it is bound in the middle of the table (the rows are rotated to the counter)
    tb.bind_batches(trials, D.BatchSchedule.for_run(tr_idx, BT, seed + 2, EP))
    for idx in list(D.epoch_batches(NT, BT, seed + 2, 0, drop_last=True))[:1]:
        sel = torch.from_numpy(idx).to(dev)
        xs.copy_(x_all[sel]); ys.copy_(y_all[sel])
        ta.step_static(BT, TT); tb.step_scheduled(static=True)
    tb.bind_batches(trials, D.BatchSchedule.for_run(tr_idx, BT, seed + 3, EP))
    assert tb._graphs[key] is graph
    run(seed + 3)
    # another shape drops the graph
    tb.bind_batches(trials, D.BatchSchedule.for_run(tr_idx, BT, seed, EP + 1))
    assert key not in tb._graphs


def test_model_batch_scheduled_step_equals_its_host_fed_step(nsd, dev):
    """ModelBatchTrainer, M = 3 with three different fold index sets: the concurrent loop of train.py against bind_batches +
    step_scheduled(), bit for bit after every step"""
    from nsd_amd import data as D
    from nsd_amd.train import concurrent_epoch
    M, seeds = 3, [3, 4, 5]
    x_all, y_all = _trials(dev, seed=2)
    runs = [dict(tr=np.array([0, 1, 2, 3, 4, 5, 6, 7]), seed=10), dict(tr=np.array([2, 3, 4, 5, 6, 7, 8, 9, 0]), seed=11),
            dict(tr=np.array([9, 8, 7, 5, 3, 1, 0, 2]), seed=12)]
    ta = nsd.ModelBatchTrainer([_model(nsd, dev, 100 + m) for m in range(M)], lr=1e-3, seeds=seeds, **_recipe(nsd))
    tb = nsd.ModelBatchTrainer([_model(nsd, dev, 100 + m) for m in range(M)], lr=1e-3, seeds=seeds, **_recipe(nsd))
    sched = D.BatchSchedule.for_runs(runs, BT, EP)
    assert sched.table.shape == (M, 4, BT)
    tb.bind_batches(D.DeviceTrialSet(x_all, y_all, dev), sched)
    tr_devs = [torch.from_numpy(r["tr"]).to(dev) for r in runs]

    def step(idxs):
        sel = [tr_devs[k][torch.from_numpy(ix).to(dev)] for k, ix in enumerate(idxs)]
        ta.step(torch.stack([x_all[s_] for s_ in sel]), torch.stack([y_all[s_] for s_ in sel]))
        tb.step_scheduled()
        assert torch.equal(ta.params, tb.params) and torch.equal(ta.m, tb.m) and torch.equal(ta.v, tb.v), ta.step_count
        assert ta.last_losses() == tb.last_losses()
    for epoch in range(EP):
        assert concurrent_epoch(runs, BT, epoch, step) == 2
    assert tb.step_count == 4 and not torch.equal(tb.params[0], tb.params[1])
    with pytest.raises(nsd.NsdError, match="4 steps are taken"):
        tb.step_scheduled()
    with pytest.raises(nsd.NsdError, match="holds 1 models' batches, the trainer 3"):
        tb.bind_batches(tb._bound["trials"], D.BatchSchedule.for_run(np.arange(NT), BT, 0, 1))


def test_a_faulty_table_is_named_by_the_trainer(nsd, dev):
    """an index the bind-time check could not see (the device table is overwritten behind it): the step's rows are NaN and the next
    record read raises, naming the model"""
    from nsd_amd import data as D
    from nsd_amd.trainer import Trainer
    x_all, y_all = _trials(dev, seed=3)
    t = Trainer(_model(nsd, dev, 31), lr=1e-3, seed=1, clip_grad_norm=0.0)
    t.bind_batches(D.DeviceTrialSet(x_all, y_all, dev), D.BatchSchedule.for_run(np.arange(NT), BT, 0, 1))
    before = t.flat.clone()
    t._bound["table"][0, 2] = NT
    t.step_scheduled()
    with pytest.raises(nsd.NsdError, match=r"model\(s\) \[0\]"):
        t.last_loss()
    assert t.skipped_steps() == 1 and torch.equal(t.flat, before)                    # the guarded tail skipped the step


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def _cli(argv, tmp_path, name):
    out = subprocess.run([sys.executable, "-c", "import sys, nsd_amd.train as t; sys.exit(t.main(sys.argv[1:]))", *argv, "--out", str(tmp_path / f"{name}.pth")], cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    recs = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
    for r in recs:
        r.pop("elapsed_s", None)
        for k in ("checkpoint",):
            r.pop(k, None)
        if "shipped" in r:
            r["shipped"].pop("checkpoint", None)
        if "args" in r:
            r["args"].pop("out", None)
    return recs


@pytest.mark.parametrize("mode", ["plain", "kfold_concurrent"])
def test_cli_emits_the_same_lines_with_device_batches(nsd, dev, tmp_path, mode):
    """24 synthetic trials (T = 32) in a packed .npz, --epochs 2 --batch 8: the JSON lines with --device-batches are those without,
    except elapsed_s (and the --out path, which differs between the two runs of this test)"""
    rs = np.random.RandomState(0)
    prefix = np.array(["water", "food", "backgroundnoise"] * 8)
    x = (2.7 * rs.standard_normal((24, 32, 8))).astype(np.float32)
    x[np.arange(24), :, np.arange(24) % 3] += 1.5
    path = tmp_path / "trials.npz"
    np.savez(path, x=x, stem=np.array([f"{p}_{i}" for i, p in enumerate(prefix)]), prefix=prefix)
    argv = ["--data", str(path), "--T", "32", "--epochs", "2", "--batch", "8"] + (["--kfold", "2", "--concurrent"] if mode != "plain" else [])
    host = _cli(argv, tmp_path, "host")
    device = _cli(argv + ["--device-batches"], tmp_path, "device")
    assert len(host) >= 3 and host[-1]["done"] is True
    assert device == host
