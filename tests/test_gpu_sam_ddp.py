"""Sharpness-aware minimisation at world = 2 on the product kernels (both ranks share cuda:0, the collective runs over gloo, as in
tests/test_gpu_ddp.py): each rank ascends along its own shard's gradient (nsd_grad_reduce -> nsd_sam_ascend_flat; the bf16 path between
its two forward/backward pairs), with uneven and EMPTY shards, and the ranks stay in lock step bit for bit.  fp32: a trainer with rho = 0
-- both passes, the second on a bitwise copy of the parameters -- is bit for bit the trainer without SAM on the guarded tail."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _make(precision):
    import nsd_amd
    torch.manual_seed(11)
    if precision == "bf16":
        return nsd_amd.EEG_LSTM(8, 64, 2, 5, dropout=0.6, precision="bf16")
    return nsd_amd.EEG_LSTM(8, 48, 2, 3, dropout=0.6)


def _batches(precision):
    from tests.golden.make_goldens import synth_labels, synth_x
    K = 5 if precision == "bf16" else 3
    return [(synth_x(B, 20, seed=40 + i), synth_labels(B, K, seed=40 + i)) for i, B in enumerate((7, 1, 6, 2))]


def _worker(rank, world, port, precision, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from nsd_amd import ops
        from nsd_amd.trainer import Trainer, shard_range
        dev = torch.device("cuda:0")
        arms = dict(sam=dict(sam=ops.Sam(0.05)), zero=dict(sam=ops.Sam(0.0)), guarded=dict(clip_grad_norm=0.0))
        for name, kw in arms.items():
            tr = Trainer(_make(precision).to(dev).train(), lr=1e-3, seed=7, **kw)
            empty = 0
            for x, y in _batches(precision):
                lo, hi = shard_range(len(y), rank, world)
                empty += int(hi == lo)
                tr.step(torch.from_numpy(x[lo:hi]).to(dev), torch.from_numpy(y[lo:hi]).to(dev), global_batch=len(y))
            torch.cuda.synchronize()
            tr.check()
            rec = tr.last_sam()
            assert tr.scan_status() == 0 and tr.skipped_steps() == 0 and bool(torch.isfinite(tr.flat).all())
            if name == "sam":
                assert rec["scale"] > 0 and rec["nonfinite"] == 0
            elif name == "zero":
                assert rec["scale"] == 0.0 and rec["nonfinite"] == 0
            else:
                assert rec is None
            np.save(os.path.join(out_dir, f"{name}{rank}.npy"), tr.flat.cpu().numpy())
            np.save(os.path.join(out_dir, f"empty{rank}.npy"), np.array([empty]))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_two_ranks_ascend_along_their_own_shards(tmp_path, precision):
    assert torch.cuda.is_available()
    mp.spawn(_worker, args=(2, _free_port(), precision, str(tmp_path)), nprocs=2, join=True)
    got = {n: [np.load(tmp_path / f"{n}{r}.npy") for r in (0, 1)] for n in ("sam", "zero", "guarded")}
    assert int(np.load(tmp_path / "empty0.npy")[0]) + int(np.load(tmp_path / "empty1.npy")[0]) >= 1      # a rank stepped on an empty shard
    for n, (p0, p1) in got.items():
        assert np.array_equal(p0, p1), n                        # ranks in lock step, bit for bit
    assert not np.array_equal(got["sam"][0], got["guarded"][0])
    d = float(np.abs(got["zero"][0] - got["guarded"][0]).max())
    print(f"[sam world 2] {precision}: |rho = 0 - guarded| {d:.3e}  |rho = 0.05 - guarded| {float(np.abs(got['sam'][0] - got['guarded'][0]).max()):.3e}")
    if precision == "fp32":                                     # (pass 2 of the fp32 kernels is a lone pass: tests/test_gpu_sam.py)
        assert np.array_equal(got["zero"][0], got["guarded"][0])
