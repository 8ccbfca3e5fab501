"""Every entry point of include/nsd.h held to its buffer and stream contract (the header's "Conventions"): the caller owns every buffer,
buffer contents before a call are never read unless documented, nothing outside the stated extents is written, inputs are never
written, work is enqueued on `stream`, nothing is allocated and nothing synchronises.  The numeric comparisons elsewhere in the suite
cannot see a breach of these: a kernel can be exact and still spill a padding trial's row past its buffer, read a ring slot the last
test happened to leave finite, or send a helper launch to the legacy stream.  Needs a real MI355X: run with `pytest -m gpu -s`.

Every ROUTE below (a call sequence at the smallest shape that reaches it; batch thresholds come from the device's CU count) runs once
per MODE on buffers of tests/buffer_contract.py -- every caller-owned output, workspace and scratch buffer between two 0xA5 guards and
exactly as long as the library says it must be:
  zeros / ones / nan32 / stale   what outputs and workspaces hold beforehand (bit patterns of buffer_contract.FILLS; stale: what a complete
                                 evaluation of the same route at B + 3, T + 2 with other parameters left in the same allocation; the
                                 sequence workspace is initialised once, before that earlier evaluation)
  side                           the whole sequence on a side stream (inputs ordered with wait_stream, outputs read after its synchronize)
                                 while the legacy default stream is kept busy with a few large matrix products: a launch or memset
                                 that went to stream 0 instead of `stream` runs after them, too late for the launches that follow it
  graph                          eager warm-up on a side stream, the sequence captured into one torch.cuda.graph (a synchronisation or
                                 an allocation inside the library fails the capture with an NsdError; a launch on the legacy stream
                                 does so or, where the runtime lets it run, is missing from the graph), the route's input changed in
                                 place, every output poisoned, one replay, against an eager run on the new input bit for bit.  Not for
                                 the nsd_seq_* path: it is not graph-replayed by design (Trainer.step_static refuses it).
and asserts (a) all guards intact, (b) all inputs bitwise unchanged, (c) every output bitwise equal to the "zeros" run's, whatever the
fill or stream, (d) every output finite, (e) in the "zeros" run every output against the route's existing reference at its existing
bound (the imports below; none is restated, none is new), (f) on the sequence path nsd_seq_status == 0 right after each evaluation,
before any result is used: a time-out fails the test there, nothing further is launched on that workspace, no sequence route runs
after it and nothing is retried.

Found by these tests and fixed with them: nothing -- the library keeps the contract on every route below.  What they can find was tried
with three faults seeded into a build of the library (not committed): the four-trial H = 48 forward storing a padding trial's logits row
without its b < B guard (h48-four-trial*, multi-m3-four-trial*: the guard after `logits` reports byte 0 past the payload), the memset of
the padded trials' alpha rows in nsd_seq.hip shortened from T * Bp to T * B floats (every sequence route with B = 33 under "ones",
"nan32" and "side": gradients not finite; "stale" passes, finite leftovers being what the suite had before), zscore_kernel launched on
stream 0 (zscore-* under "side" and "graph").

Wall time of the file on the MI355X: 8 s (417 tests, the CPU references and the bf16 emulations included); the slowest case takes 0.4 s
(seq-fused_l2_streams-zeros).  test_zz_wall_time prints both with `-s`.
"""
import ctypes as C
import functools
import time
import types

import numpy as np
import pytest
import torch

from oracle import nsd_oracle as orc
from oracle import seq_bf16_ref as sr
from tests import augment_ref as ar
from tests import buffer_contract as bc
from tests import mixup_ref as mr
from tests.golden.make_goldens import synth_labels, synth_params, synth_x
from tests.gpu_harness import (KINK_MARGIN, LOGIT_TOL, PROB_TOL, assert_step_vs_oracle, bounds_of, cus, dev, head_inputs, kink_safe, multi_grad_ok,  # noqa: F401
                               nsd, oracle_step, oracle_streams, to_dev)
from tests.seq_bf16_harness import CASES, DUAL_RTOL, EQUIV_RTOL, case_F, case_inputs, compare, duality, emulate, per_tensor

pytestmark = pytest.mark.gpu

T_START = time.time()
SLOWEST = [0.0, ""]
_BASE = {}                       # route id -> outputs of its "zeros" run (or the exception that run ended with)
_SEQ_TIMED_OUT = []              # route ids whose workspace reported a scan time-out: no sequence route runs after one


def _np(t):
    return t.detach().float().cpu().numpy() if t.dtype == torch.bfloat16 else t.detach().cpu().numpy()


def _other(a):
    """other values of the same shape and kind for the earlier evaluation of a "stale" run"""
    return (np.roll(np.asarray(a), 1) * np.float32(0.9)).astype(np.float32)


class Route:
    """One call sequence.  setup(dev, cus, grow) -> ctx with ctx.inputs (device tensors the library may only read); grow: the earlier,
    larger evaluation of a "stale" run.  run(ctx, arena) launches on the current stream with every output taken from `arena` and
    returns {name: output}: no host read-back in it (it is captured into a graph) unless graph is False.  check(ctx, got, dev): (e)."""
    graph = True
    seq = False

    def __init__(self, rid):
        self.id = rid

    def mutate(self, ctx):
        ctx.x.mul_(-0.75)


# ---- the fp32 train step ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(Cc, H, L, K, F, B, T):
    return head_inputs(Cc, H, K, F, B, T, L=L, safe=True)


RNG = dict(seed=0xB0FFE2, base_stream=8, p_lstm=0.6, p_head=0.6)


def _batch(mb, cus, grow):
    return mb[0] * cus + mb[1] + (3 if grow else 0)


class Fp32Step(Route):
    """ops.train_step_grads (nsd_lstm_head_train[_rng] or nsd_lstm_fwd + nsd_head_train, nsd_lstm_bwd[_rng], nsd_grad_reduce) and
    nsd_loss_sum.  how: "masks" explicit mask tensors, "rng" in-kernel streams, "unfused" fused_head=False (three launches before the
    reduction).  Reference: the oracle through assert_step_vs_oracle (FAST48 on the H = 48 fast path, FP32_EXACT on
    every other route, LOGIT_TOL, its loss bound); dx at DX_TOL."""

    def __init__(self, rid, Cc, H, L, K, F, mb, T, residual=False, how="masks", dx=False):
        super().__init__(rid)
        self.shape, self.mb, self.T, self.residual, self.how, self.dx = (Cc, H, L, K, F), mb, T, residual, how, dx

    def setup(self, dev, cus, grow=False):
        from nsd_amd import ops
        Cc, H, L, K, F = self.shape
        B, T = _batch(self.mb, cus, grow), self.T + (2 if grow else 0)
        d, flat, x, y, masks = _inputs(Cc, H, L, K, F, B, T)
        if grow:
            flat = _other(flat)
        if self.how == "rng":
            masks = dict(drop_lstm=orc.dropout_mask(RNG["seed"], RNG["base_stream"], RNG["p_lstm"], (L - 1, B, T, H)),
                         rrelu_slope=orc.rrelu_noise(RNG["seed"], RNG["base_stream"] + 1, (B, F)),
                         drop_head=orc.dropout_mask(RNG["seed"], RNG["base_stream"] + 2, RNG["p_head"], (B, F)))
        ctx = types.SimpleNamespace(d=d, spec=ops.ModelSpec(C=Cc, H=H, L=L, K=K, F=F), B=B, T=T, flat_np=flat, x_np=x, y_np=y, masks_np=masks,
                                    flat=to_dev(flat, dev), x=to_dev(x.copy(), dev), y=to_dev(y.astype(np.int32), dev),
                                    masks={} if self.how == "rng" else {k: to_dev(v, dev) for k, v in masks.items()})
        ctx.inputs = [ctx.flat, ctx.x, ctx.y] + list(ctx.masks.values())
        if self.how == "rng":
            assert ops.rng_path(ctx.spec, B, T)
        if self.dx:
            assert ops.dx_path(ctx.spec, B, T)
        return ctx

    def run(self, ctx, arena):
        from nsd_amd import ops
        spec, B, T = ctx.spec, ctx.B, ctx.T
        ws = arena.buf("workspace", (bc.workspace_bytes(spec, B, T) // 4,))
        out = dict(logits=arena.buf("logits", (B, spec.K)), grads=arena.buf("grads", (spec.param_count,)), loss_sum=arena.buf("loss_sum", (1,)))
        if self.dx:
            out["dx"] = arena.buf("dx", (B, T, spec.C))
        ops.train_step_grads(spec, ctx.flat, ctx.x, ws, ctx.y, out["logits"], out["grads"], residual=self.residual,
                             fused_head=self.how != "unfused", rng=RNG if self.how == "rng" else None, dx=out.get("dx"), **ctx.masks)
        ops.loss_sum(spec, ws, B, T, out=out["loss_sum"])
        return out

    def check(self, ctx, got, dev):
        d, flat, x, y, masks = ctx.d, ctx.flat_np, ctx.x_np, ctx.y_np, ctx.masks_np
        ref = oracle_step(d, flat, x, labels=y, masks=masks, residual=self.residual, want_dx=self.dx, kink=KINK_MARGIN)
        out = dict(logits=_np(got["logits"]), grads=_np(got["grads"]), mean_loss=float(got["loss_sum"][0]) / ctx.B)
        if self.dx:
            out["dx"] = _np(got["dx"])
        assert_step_vs_oracle(out, ref, d, bounds_of(d), tag=self.id)


class Infer(Route):
    """nsd_infer with guarded logits, probs and scratch (the scratch exactly nsd_infer_scratch_bytes long).  Reference: the oracle's
    eval-mode forward at the bounds of _infer_vs_oracle (tests/test_gpu_fp32_routes.py, tests/test_gpu_head_dims.py): LOGIT_TOL, 1e-5."""

    def __init__(self, rid, Cc, H, L, K, F, mb, T, residual=False, probs=True):
        super().__init__(rid)
        self.shape, self.mb, self.T, self.residual, self.probs = (Cc, H, L, K, F), mb, T, residual, probs

    def setup(self, dev, cus, grow=False):
        from nsd_amd import ops
        Cc, H, L, K, F = self.shape
        B, T = _batch(self.mb, cus, grow), self.T + (2 if grow else 0)
        d, flat, x, _, _ = _inputs(Cc, H, L, K, F, B, T)
        flat = _other(flat) if grow else flat
        ctx = types.SimpleNamespace(d=d, spec=ops.ModelSpec(C=Cc, H=H, L=L, K=K, F=F), B=B, T=T, flat_np=flat, x_np=x, flat=to_dev(flat, dev),
                                    x=to_dev(x.copy(), dev))
        ctx.inputs = [ctx.flat, ctx.x]
        return ctx

    def run(self, ctx, arena):
        from nsd_amd import ops
        spec, B, T = ctx.spec, ctx.B, ctx.T
        n = bc.infer_scratch_bytes(spec, B, T)
        out = dict(logits=arena.buf("logits", (B, spec.K)))
        if self.probs:
            out["probs"] = arena.buf("probs", (B, spec.K))
        ops.infer(spec, ctx.flat, ctx.x, residual=self.residual, want_probs=self.probs, logits=out["logits"], probs=out.get("probs"),
                  scratch=arena.buf("scratch", (n,), torch.uint8) if n else None)
        return out

    def check(self, ctx, got, dev):
        ref = orc.forward(ctx.flat_np, ctx.x_np, ctx.d, residual=self.residual)
        lerr = float(np.abs(_np(got["logits"]) - ref["logits"]).max())
        perr = float(np.abs(_np(got["probs"]) - ref["probs"]).max()) if self.probs else 0.0
        print(f"[{self.id}] infer logits {lerr:.2e}  probs {perr:.2e}  scratch {bc.infer_scratch_bytes(ctx.spec, ctx.B, ctx.T)} bytes")
        assert lerr < LOGIT_TOL and perr < PROB_TOL, (lerr, perr)


# (id, C, H, L, K, F, (m, a): B = m * cus + a, T, residual, how, dx)
_STEPS = [
    ("h48-one-trial-masks-dx", 8, 48, 2, 3, 32, (0, 5), 9, False, "masks", True),          # fused single launch, one trial per workgroup
    ("h48-one-trial-rng", 8, 48, 2, 3, 32, (0, 5), 9, False, "rng", False),
    ("h48-one-trial-unfused", 8, 48, 2, 3, 32, (0, 5), 9, False, "unfused", False),         # three launches
    ("h48-two-trial-fwd", 8, 48, 2, 3, 32, (1, 3), 5, False, "masks", False),
    ("h48-four-trial", 8, 48, 2, 3, 32, (2, 3), 5, False, "masks", False),                  # a partly filled last group of four
    ("h48-four-trial-dx", 8, 48, 2, 3, 32, (2, 3), 5, False, "masks", True),                # the small attention-backward kernel runs first
    ("h48-k9-two-launch", 8, 48, 2, 9, 33, (0, 5), 9, False, "masks", False),
    ("h48-residual", 8, 48, 2, 3, 32, (0, 5), 9, True, "masks", False),
    ("h32-c5-t33", 5, 32, 2, 3, 32, (0, 5), 33, False, "masks", False),                     # first-generation kernels, the second 32-step chunk
    ("h64-c5-t33", 5, 64, 2, 3, 32, (0, 5), 33, False, "masks", False),
    ("h32-four-trial", 8, 32, 2, 3, 32, (2, 3), 3, False, "masks", False),                  # fwd<32,4>, the backward's group loop
    ("h64-b387-mfma", 8, 64, 2, 3, 32, (0, 387), 3, False, "masks", False),                 # past the switch to the batched MFMA path
    ("mfma-h112", 8, 112, 2, 3, 32, (0, 70), 9, False, "masks", False),
    ("mfma-h80-l3-ragged", 4, 80, 3, 3, 32, (0, 64), 2, False, "masks", False),
    ("generic-h40-l1-dx", 3, 40, 1, 2, 32, (0, 5), 37, False, "masks", True),
    ("generic-h48-l3-residual", 8, 48, 3, 4, 32, (0, 5), 9, True, "masks", False),
]
ROUTES = [Fp32Step(*r) for r in _STEPS]
_seen = set()
for r in _STEPS:                                            # nsd_infer: one row per band of each of the above
    key = r[1:9]
    if key not in _seen:
        _seen.add(key)
        ROUTES.append(Infer("infer-" + r[0].replace("-masks-dx", "").replace("-dx", ""), *r[1:9]))
ROUTES.append(Infer("infer-h48-one-trial-no-probs", 8, 48, 2, 3, 32, (0, 5), 9, probs=False))


# ---- the model-batched H = 48 path -------------------------------------------------------------------------------------------------
# K = 5, F = 24: P = 31398, P % 4 == 2 -- every model's block of parameters, gradients and head slabs after the first starts 8 bytes off
# a 16-byte boundary.  K = 4, F = 24 (the last two rows of the multi routes): P = 31373, odd -- 4 bytes off.
MULTI_HEAD, MULTI_HEAD_ODD, MULTI_M = (5, 24), (4, 24), 3


def _multi_batch(band, cus, grow):
    """"small": 5 trials per model.  "four-trial": the smallest B with M * B >= 2 cus + 3 that is no multiple of 4 (2 cus + 3 itself is
    no multiple of 3 at 256 CUs), so the launch's last group of four is partly filled and model boundaries fall inside groups."""
    if band == "small":
        B = 5
    else:
        B = -(-(2 * cus + 3) // MULTI_M)
        B += 1 if (MULTI_M * B) % 4 == 0 else 0
        assert MULTI_M * B >= 2 * cus + 3 and (MULTI_M * B) % 4
    return B + (3 if grow else 0)


def _multi_problem(B, T, dev, grow, head=MULTI_HEAD):
    from nsd_amd import ops
    M, (K, F) = MULTI_M, head
    spec, d = ops.ModelSpec(C=8, H=48, L=2, K=K, F=F), orc.Dims(C=8, H=48, L=2, K=K, F=F)
    assert spec.param_count % 4 == (1 if head == MULTI_HEAD_ODD else 2) and ops.multi_path(spec, M, B, T)
    params = np.stack([orc.flatten_state(kink_safe(synth_params(8, 48, 2, K, F=F, seed=100 + m + (50 if grow else 0)), F), d) for m in range(M)])
    x = np.stack([synth_x(B, T, seed=20 + m) for m in range(M)])
    y = np.stack([synth_labels(B, K=K, seed=30 + m) for m in range(M)]).astype(np.int32)
    rngs = [dict(seed=1000 + 17 * m, base_stream=4 * (m + 1), p_lstm=0.6, p_head=0.6) for m in range(M)]
    return types.SimpleNamespace(spec=spec, d=d, M=M, B=B, T=T, params_np=params, x_np=x, y_np=y, rngs=rngs, params=to_dev(params, dev),
                                 x=to_dev(x.copy(), dev), y=to_dev(y.reshape(-1), dev))


class MultiStep(Route):
    """ops.multi_train_step + nsd_multi_loss_sum.  soft=False, adam=False: nsd_multi_train_fwd, _bwd, _grad_reduce; soft=True, adam=True:
    nsd_multi_train_fwd_soft, _bwd, _grad_reduce_adam (parameters, m and v are then caller-owned in / out buffers, guarded too).
    Reference: each model's single-model run at the bounds of tests/test_gpu_multimodel.py (test_models_equal_separate_runs), the oracle
    for the last model (test_last_model_of_a_batch_against_the_oracle's _vs_oracle), Adam's p / m / v against reduce-then-nsd_adam_step
    bit for bit (test_fused_reduce_adam_equals_reduce_then_adam)."""
    HYPER = dict(step=3, lr=1e-3, weight_decay=1e-2, grad_scale=0.5)

    def __init__(self, rid, band, T, soft, adam, head=MULTI_HEAD):
        super().__init__(rid)
        self.band, self.T, self.soft, self.adam, self.head = band, T, soft, adam, head

    def setup(self, dev, cus, grow=False):
        ctx = _multi_problem(_multi_batch(self.band, cus, grow), self.T + (2 if grow else 0), dev, grow, self.head)
        M, B, K = ctx.M, ctx.B, ctx.spec.K
        ctx.inputs = [ctx.x, ctx.y]
        if self.soft:                                       # smoothed, weighted rows: any row sum
            q = np.stack([mr.base_rows(ctx.y_np[m], K, 0.1, np.linspace(0.5, 1.5, K).astype(np.float32)) for m in range(M)])
            ctx.q_np, ctx.q = q, to_dev(q.reshape(M * B, K), dev)
            ctx.inputs.append(ctx.q)
        if self.adam:
            rs = np.random.RandomState(3)
            ctx.m0 = to_dev((rs.random_sample(ctx.params_np.shape) * 1e-3).astype(np.float32), dev)
            ctx.v0 = to_dev((rs.random_sample(ctx.params_np.shape) * 1e-6).astype(np.float32), dev)
            ctx.inputs += [ctx.params, ctx.m0, ctx.v0]     # the launches work on copies inside the arena
        else:
            ctx.inputs.append(ctx.params)
        return ctx

    def run(self, ctx, arena):
        from nsd_amd import ops
        spec, M, B, T, P = ctx.spec, ctx.M, ctx.B, ctx.T, ctx.spec.param_count
        ws = arena.buf("workspace", (bc.multi_workspace_bytes(spec, M, B, T) // 4,))
        out = dict(logits=arena.buf("logits", (M * B, spec.K)), grads=arena.buf("grads", (M, P)), losses=arena.buf("losses", (M,)))
        params, kw = ctx.params, {}
        if self.adam:
            out.update(p=arena.buf("p", (M, P)), m=arena.buf("m", (M, P)), v=arena.buf("v", (M, P)))
            out["p"].copy_(ctx.params), out["m"].copy_(ctx.m0), out["v"].copy_(ctx.v0)
            params, kw = out["p"], dict(m=out["m"], v=out["v"], **self.HYPER)
        ops.multi_train_step(spec, params, ctx.x, None if self.soft else ctx.y, ws, out["grads"], rngs=ctx.rngs, logits=out["logits"],
                             fuse_adam=self.adam, targets=ctx.q if self.soft else None, **kw)
        ops.multi_loss_sum(spec, ws, M, B, T, out=out["losses"])
        return out

    def check(self, ctx, got, dev):
        from nsd_amd import ops
        spec, M, B, T, P = ctx.spec, ctx.M, ctx.B, ctx.T, ctx.spec.param_count
        lg = got["logits"].view(M, B, spec.K)
        for m in range(M):                                  # per-model single-model runs
            ws = ops.new_workspace(spec, B, T, dev)
            l1, g1 = torch.empty((B, spec.K), device=dev), torch.empty(P, device=dev)
            ops.train_step_grads(spec, ctx.params[m].contiguous(), ctx.x[m].contiguous(), ws, None if self.soft else ctx.y.view(M, B)[m].contiguous(),
                                 l1, g1, rng=ctx.rngs[m], targets=ctx.q.view(M, B, spec.K)[m].contiguous() if self.soft else None)
            s1, sm = float(ops.loss_sum(spec, ws, B, T).item()) / B, float(got["losses"][m]) / B
            l1, g1 = l1.cpu(), g1.cpu()
            assert float((lg[m] - l1).abs().max()) <= 1e-6 * max(float(l1.abs().max()), 1.0), m
            multi_grad_ok(spec, got["grads"][m], g1)
            assert abs(sm - s1) <= 1e-6 * max(1.0, abs(s1)), (m, sm, s1)
        if not self.soft:                                   # the last model against the oracle, its masks from its own streams
            r, m = ctx.rngs[M - 1], M - 1
            ref = oracle_step(ctx.d, ctx.params_np[m], ctx.x_np[m], labels=ctx.y_np[m], kink=KINK_MARGIN,
                              masks=oracle_streams(r["seed"], r["base_stream"], B, T, 48, spec.F))
            out = dict(logits=_np(lg[m]), grads=_np(got["grads"][m]), mean_loss=float(got["losses"][m]) / B)
            assert_step_vs_oracle(out, ref, ctx.d, bounds_of(ctx.d), tag=f"{self.id} model {m}")
        if self.adam:
            pb, mb, vb = ctx.params.clone(), ctx.m0.clone(), ctx.v0.clone()
            gb = torch.empty_like(pb)
            ops.multi_train_step(spec, pb, ctx.x, None, ops.multi_workspace(spec, M, B, T, dev), gb, rngs=ctx.rngs, fuse_adam=False, targets=ctx.q)
            ops.adam_step(pb.view(-1), gb.view(-1), mb.view(-1), vb.view(-1), **self.HYPER)
            assert torch.equal(got["grads"], gb.cpu()) and torch.equal(got["p"], pb.cpu()) and torch.equal(got["m"], mb.cpu()) and torch.equal(got["v"], vb.cpu())
            assert not torch.equal(got["p"], ctx.params.cpu())


class MultiInfer(Route):
    """nsd_multi_infer with x_model_stride 0 (shared windows) or B * T * C.  Reference: ops.infer per model, bit for bit
    (tests/test_gpu_multimodel.py::test_multi_infer_equals_infer)."""

    def __init__(self, rid, shared):
        super().__init__(rid)
        self.shared = shared

    def setup(self, dev, cus, grow=False):
        ctx = _multi_problem(5 + (3 if grow else 0), 9 + (2 if grow else 0), dev, grow)
        if self.shared:
            ctx.x = ctx.x[0].contiguous()
        ctx.inputs = [ctx.params, ctx.x]
        return ctx

    def run(self, ctx, arena):
        from nsd_amd import ops
        spec, M, B, T = ctx.spec, ctx.M, ctx.B, ctx.T
        n = bc.multi_infer_scratch_bytes(spec, M, B, T)
        out = dict(logits=arena.buf("logits", (M, B, spec.K)), probs=arena.buf("probs", (M, B, spec.K)))
        ops.multi_infer(spec, ctx.params, ctx.x, logits=out["logits"], probs=out["probs"],
                        scratch=arena.buf("scratch", (n,), torch.uint8) if n else None)
        return out

    def check(self, ctx, got, dev):
        from nsd_amd import ops
        for m in range(ctx.M):
            l1, p1 = ops.infer(ctx.spec, ctx.params[m].contiguous(), (ctx.x if self.shared else ctx.x[m]).contiguous())
            assert torch.equal(got["logits"][m], l1.cpu()) and torch.equal(got["probs"][m], p1.cpu()), m


ROUTES += [MultiStep("multi-m3-b5-labels-reduce", "small", 9, False, False), MultiStep("multi-m3-b5-soft-adam", "small", 9, True, True),
           MultiStep("multi-m3-four-trial-labels-reduce", "four-trial", 5, False, False),
           MultiStep("multi-m3-four-trial-soft-adam", "four-trial", 5, True, True),
           MultiStep("multi-m3-b5-odd-p-labels-reduce", "small", 9, False, False, MULTI_HEAD_ODD),
           MultiStep("multi-m3-b5-odd-p-soft-adam", "small", 9, True, True, MULTI_HEAD_ODD),
           MultiInfer("multi-infer-shared-x", True), MultiInfer("multi-infer-own-x", False)]


# ---- the bf16 sequence path --------------------------------------------------------------------------------------------------------
class SeqCase(Route):
    """nsd_seq_workspace_init (not again on a stale workspace), nsd_seq_train_fwd -> nsd_seq_train_bwd_dx (with dx), nsd_seq_loss_sum,
    nsd_seq_guard, nsd_seq_infer, and with any_loss nsd_seq_train_fwd_logits -> nsd_seq_head_bwd -> nsd_seq_train_bwd_dx, all on one
    workspace of exactly nsd_seq_workspace_bytes.  Reference: the bf16 emulation through compare() at the case's REF_* bounds
    (tests/test_gpu_seqpath_bf16ref.py); dx by its duality with the input weight gradient at DUAL_RTOL and the any-loss gradients against
    the fused ones at EQUIV_RTOL, logits bit for bit (tests/test_gpu_seq_autograd.py)."""
    graph = False
    seq = True

    def __init__(self, rid, case, any_loss=False):
        super().__init__(rid)
        self.case, self.any_loss = case, any_loss

    def setup(self, dev, cus, grow=False):
        from nsd_amd import ops
        case = self.case
        if grow:
            case = case[:5] + (case[5] + 3, case[6] + 2) + case[7:]
        Cc, H, L, K, D, B, T = case[:7]
        flat, x, y, masks, rng = case_inputs(case, seed=1 if grow else 0)
        spec = ops.ModelSpec(C=Cc, H=H, L=L, K=K, F=case_F(case), D=D)
        assert spec.seq_path(B, T)
        ctx = types.SimpleNamespace(case=case, spec=spec, B=B, T=T, flat_np=flat, x_np=x, y_np=y, masks_np=masks, rng=rng, flat=to_dev(flat, dev),
                                    x=to_dev(x.copy(), dev), y=to_dev(y, dev))
        ctx.inputs = [ctx.flat, ctx.x, ctx.y]
        return ctx

    def _status(self, ws, what):
        """(f): right after an evaluation, before any result is used"""
        from nsd_amd import ops
        st = ops.seq_status(ws)
        if st & ops.SEQ_ST_TIMEOUT_MASK:
            _SEQ_TIMED_OUT.append(self.id)
        assert st == 0, (self.id, what, st)

    def run(self, ctx, arena):
        from nsd_amd import ops
        spec, B, T, rng = ctx.spec, ctx.B, ctx.T, ctx.rng
        ws = arena.buf("workspace", (bc.seq_workspace_bytes(spec, B, T),), torch.uint8)
        if arena.fill != "stale":                           # after the fill; a stale workspace keeps the header of its first user
            ops._call("nsd_seq_workspace_init", ws.device, ws.data_ptr(), ws.numel(), ops.STREAM)
        out = dict(logits=arena.buf("logits", (B, spec.K)), grads=arena.buf("grads", (spec.param_count,)), dx=arena.buf("dx", (B, T, spec.C)),
                   loss_sum=arena.buf("loss_sum", (1,)), guard_flag=arena.buf("guard_flag", (1,)),
                   infer_logits=arena.buf("infer_logits", (B, spec.K)), probs=arena.buf("probs", (B, spec.K)))
        ops.seq_train_fwd(spec, ctx.flat, ctx.x, ctx.y, ws, rng=rng, logits=out["logits"])
        ops.seq_train_bwd(spec, ctx.flat, ws, B, T, rng=rng, grads=out["grads"], dx=out["dx"])
        ops.seq_loss_sum(spec, ws, B, T, out=out["loss_sum"])
        ops.seq_guard(ws, out["guard_flag"])
        self._status(ws, "train")
        if self.any_loss:
            out.update(any_logits=arena.buf("any_logits", (B, spec.K)), any_grads=arena.buf("any_grads", (spec.param_count,)),
                       any_dx=arena.buf("any_dx", (B, T, spec.C)))
            ops.seq_train_fwd_logits(spec, ctx.flat, ctx.x, ws, rng=rng, logits=out["any_logits"])
            dl = ((torch.softmax(out["any_logits"], 1) - torch.nn.functional.one_hot(ctx.y.long(), spec.K).float()) / B).contiguous()
            ops.seq_head_bwd(spec, ctx.flat, ws, dl, B, T, rng=rng)
            ops.seq_train_bwd(spec, ctx.flat, ws, B, T, rng=rng, grads=out["any_grads"], dx=out["any_dx"])
            self._status(ws, "any loss")
        ops.seq_infer(spec, ctx.flat, ctx.x, ws, logits=out["infer_logits"], probs=out["probs"])
        self._status(ws, "infer")
        return out

    def check(self, ctx, got, dev):
        case, spec = ctx.case, ctx.spec
        route = sr.product_route(case[1], case[2], case[4], case[5], case[0])
        case = case[:8] + (route,) + case[9:]
        t0 = time.time()
        ref = emulate(case, ctx.flat_np, ctx.x_np, ctx.y_np, ctx.masks_np)
        ev = emulate(case, ctx.flat_np, ctx.x_np, None, {}) if ctx.rng is not None else ref
        print(f"[{self.id}] route {route}, emulation {time.time() - t0:.1f} s")
        compare(self.id, case, _np(got["logits"]), _np(got["grads"]), ref, got_loss=float(got["loss_sum"][0]) / ctx.B)
        compare(self.id + " infer", case, _np(got["infer_logits"]), None, ev, got_probs=_np(got["probs"]))
        assert float(got["guard_flag"][0]) == 0.0
        diff, scale = duality(spec, ctx.flat.cpu(), ctx.x.cpu(), got["grads"], got["dx"])
        print(f"[{self.id}] dx duality {diff / scale:.2e}")
        assert scale > 0 and diff / scale < DUAL_RTOL, (diff, scale)
        if self.any_loss:
            errs = per_tensor(spec, got["any_grads"], got["grads"])
            worst = max(errs.items(), key=lambda kv: kv[1])
            print(f"[{self.id}] any-loss grads vs fused: worst {worst[1]:.2e} ({worst[0]})")
            assert torch.equal(got["any_logits"], got["logits"]) and worst[1] < EQUIV_RTOL, errs
            d2, s2 = duality(spec, ctx.flat.cpu(), ctx.x.cpu(), got["any_grads"], got["any_dx"])
            assert s2 > 0 and d2 / s2 < DUAL_RTOL, (d2, s2)


for tag in ("fused_h64", "fused_l2_streams", "general_l1", "general_l3", "wide_c40", "bidir_h128", "tiles64_h256"):
    ROUTES.append(SeqCase("seq-" + tag, CASES[tag], any_loss=tag in ("fused_l2_streams", "bidir_h128")))
for H, L in ((64, 2), (128, 1)):
    for T in (1, 2):                                        # B = 33: one padded tile of 32 beyond the first
        ROUTES.append(SeqCase(f"seq-short-h{H}-l{L}-t{T}", (8, H, L, 3, 1, 33, T, None, "fused2" if L == 2 else "general", "short", False)))


# ---- small kernels -----------------------------------------------------------------------------------------------------------------
class Small(Route):
    """a route from three functions: make(dev, grow) -> ctx, launch(ctx, arena) -> outputs, verify(ctx, got, dev); change(ctx): the
    in-place change of an input before the graph replay (None: the launch has no device input)"""

    def __init__(self, rid, make, launch, verify, change=None):
        super().__init__(rid)
        self.make, self.launch, self.verify, self.change = make, launch, verify, change

    def setup(self, dev, cus, grow=False):
        return self.make(dev, grow)

    def run(self, ctx, arena):
        return self.launch(ctx, arena)

    def check(self, ctx, got, dev):
        self.verify(ctx, got, dev)

    def mutate(self, ctx):
        if self.change is not None:
            self.change(ctx)
        elif hasattr(ctx, "x"):
            ctx.x.mul_(-0.75)


def _ns(**kw):
    ctx = types.SimpleNamespace(**kw)
    ctx.inputs = [v for v in kw.values() if torch.is_tensor(v)]
    return ctx


# nsd_zscore_fwd: the shape and bound of tests/test_gpu_parity.py's z-score test (2e-5 against the oracle)
def _zs_make(dev, grow):
    x = synth_x(9 + (3 if grow else 0), 77 + (2 if grow else 0), C=5, seed=2 + grow)
    return _ns(x_np=x, x=to_dev(x.copy(), dev))


def _zs_out(ctx, arena):
    from nsd_amd import ops
    return dict(y=ops.zscore(ctx.x, out=arena.buf("y", ctx.x.shape)))


def _zs_in_place(ctx, arena):
    from nsd_amd import ops
    y = arena.buf("y", ctx.x.shape)
    y.copy_(ctx.x)
    return dict(y=ops.zscore(y, out=y))


def _zs_verify(ctx, got, dev):
    assert np.abs(_np(got["y"]) - orc.zscore(ctx.x_np)).max() < 2e-5


ROUTES += [Small("zscore-out-of-place", _zs_make, _zs_out, _zs_verify), Small("zscore-in-place", _zs_make, _zs_in_place, _zs_verify)]

# nsd_augment / nsd_mixup: M = 3, B = 5, T = 7, C = 5, K = 3, bit for bit against tests/augment_ref.py / tests/mixup_ref.py
AUG = dict(max_shift=3, scale_range=0.2, p_channel=0.25, noise_std=0.3)
AUG_RNGS = [dict(seed=1000 + 17 * m, base_stream=4 * (m + 2)) for m in range(3)]
MIX = dict(mix=0.8, eps=0.1, weights=np.linspace(0.5, 1.5, 3).astype(np.float32))


def _aug_make(dev, grow):
    B, T = 5 + (3 if grow else 0), 7 + (2 if grow else 0)
    x = synth_x(3 * B, T, C=5, seed=7 + grow).reshape(3, B, T, 5)
    lab = synth_labels(3 * B, 3, seed=9 + grow).reshape(3, B).astype(np.int32)
    return _ns(x_np=x, lab_np=lab, x=to_dev(x.copy(), dev), lab=to_dev(lab.reshape(-1), dev), w=to_dev(MIX["weights"], dev))


def _aug_launch(zscore):
    def launch(ctx, arena):
        import nsd_amd
        from nsd_amd import ops
        return dict(y=ops.augment(ctx.x, nsd_amd.Augment(**AUG), AUG_RNGS, zscore=zscore, out=arena.buf("y", ctx.x.shape)))
    return launch


def _aug_verify(zscore):
    def verify(ctx, got, dev):
        from nsd_amd import ops
        ref = ar.augment_models(ctx.x_np, [(r["seed"], r["base_stream"]) for r in AUG_RNGS], **AUG)
        if zscore:                                          # bitwise what nsd_zscore_fwd gives on the unfused output (include/nsd.h)
            ref = _np(ops.zscore(to_dev(ref.reshape((-1,) + ref.shape[2:]), dev))).reshape(ref.shape)
        assert np.array_equal(_np(got["y"]).view(np.uint32), ref.view(np.uint32))
    return verify


def _mix_launch(ctx, arena):
    from nsd_amd import ops
    M, B = ctx.lab_np.shape
    y, tg = ops.mixup(ctx.x, ctx.lab, 3, AUG_RNGS, label_smoothing=MIX["eps"], mix=MIX["mix"], class_weights=ctx.w, out=arena.buf("y", ctx.x.shape),
                      targets=arena.buf("targets", (M * B, 3)))
    return dict(y=y, targets=tg)


def _mix_verify(ctx, got, dev):
    y_ref, tg_ref = mr.mixup_models(ctx.x_np, ctx.lab_np, 3, [(r["seed"], r["base_stream"]) for r in AUG_RNGS], **MIX)
    assert np.array_equal(_np(got["y"]).view(np.uint32), y_ref.view(np.uint32))
    assert np.array_equal(_np(got["targets"]).view(np.uint32).reshape(tg_ref.shape), tg_ref.view(np.uint32))


ROUTES += [Small("augment", _aug_make, _aug_launch(False), _aug_verify(False)), Small("augment-zscore", _aug_make, _aug_launch(True), _aug_verify(True)),
           Small("mixup", _aug_make, _mix_launch, _mix_verify)]

# the counter streams: bit for bit against the oracle's (tests/test_gpu_parity.py: test_counter_streams_bit_exact, test_fused_train_masks_bit_exact)
MASK_SEED, N_LSTM, N_HEAD, N_ODD = 12345678901234, 3 * 17 * 48 + 1, 97, 1001


def _masks_make(on_dev):
    def make(dev, grow):
        g = 3 if grow else 0
        ctx = _ns(step_dev=torch.tensor([5 + g], dtype=torch.int64, device=dev)) if on_dev else _ns()
        ctx.n_lstm, ctx.n_head, ctx.base = N_LSTM + g, N_HEAD + g, 4 * (5 + g)
        return ctx
    return make


def _masks_launch(on_dev):
    def launch(ctx, arena):
        from nsd_amd import ops
        out = dict(drop_lstm=arena.buf("drop_lstm", (ctx.n_lstm,)), rrelu=arena.buf("rrelu", (ctx.n_head,)), drop_head=arena.buf("drop_head", (ctx.n_head,)))
        ops.train_masks(MASK_SEED, ctx.step_dev if on_dev else ctx.base, 0.6, 0.5, out["drop_lstm"], out["rrelu"], out["drop_head"])
        return out
    return launch


def _masks_verify(ctx, got, dev):
    assert np.array_equal(_np(got["drop_lstm"]), orc.dropout_mask(MASK_SEED, ctx.base, 0.6, (ctx.n_lstm,)))
    assert np.array_equal(_np(got["rrelu"]), orc.rrelu_noise(MASK_SEED, ctx.base + 1, (ctx.n_head,)))
    assert np.array_equal(_np(got["drop_head"]), orc.dropout_mask(MASK_SEED, ctx.base + 2, 0.5, (ctx.n_head,)))


def _one_stream_make(dev, grow):
    ctx = _ns()
    ctx.n = N_ODD + (3 if grow else 0)
    return ctx


def _dropout_launch(ctx, arena):
    from nsd_amd import ops
    out = arena.buf("out", (ctx.n,))
    ops._call("nsd_dropout_mask", out.device, MASK_SEED, 3, 0.6, ctx.n, out.data_ptr(), ops.STREAM)
    return dict(out=out)


def _rrelu_launch(ctx, arena):
    from nsd_amd import ops
    out = arena.buf("out", (ctx.n,))
    ops._call("nsd_rrelu_noise", out.device, MASK_SEED, 3, ctx.n, out.data_ptr(), ops.STREAM)
    return dict(out=out)


def _step_inc(ctx):
    ctx.step_dev.add_(1)
    ctx.base += 4


ROUTES += [Small("train-masks", _masks_make(False), _masks_launch(False), _masks_verify),
           Small("train-masks-dev", _masks_make(True), _masks_launch(True), _masks_verify, _step_inc),
           Small("dropout-mask-n1001", _one_stream_make, _dropout_launch,
                 lambda ctx, got, dev: np.testing.assert_array_equal(_np(got["out"]), orc.dropout_mask(MASK_SEED, 3, 0.6, (ctx.n,)))),
           Small("rrelu-noise-n1001", _one_stream_make, _rrelu_launch,
                 lambda ctx, got, dev: np.testing.assert_array_equal(_np(got["out"]), orc.rrelu_noise(MASK_SEED, 3, (ctx.n,))))]

# nsd_adam_step / _guarded / _dev at n = 1001: p within 1e-6 of the oracle's Adam (tests/test_gpu_parity.py), the three forms bit for bit
# (tests/test_gpu_head_dims.py, section i); a raised skip flag leaves p, m, v as they were
ADAM = dict(lr=1e-3, weight_decay=1e-2, grad_scale=1.0)


def _adam_make(dev, grow):
    n = N_ODD + (3 if grow else 0)
    rs = np.random.RandomState(11 + grow)
    p, g = rs.standard_normal(n).astype(np.float32), rs.standard_normal(n).astype(np.float32)
    m, v = (rs.standard_normal(n) * 1e-3).astype(np.float32), (rs.random_sample(n) * 1e-6).astype(np.float32)
    return _ns(p0_np=p, g_np=g, m0_np=m, v0_np=v, p0=to_dev(p, dev), g=to_dev(g, dev), m0=to_dev(m, dev), v0=to_dev(v, dev),
               skip0=torch.zeros(1, device=dev), skip1=torch.ones(1, device=dev), step_dev=torch.tensor([3], dtype=torch.int64, device=dev))


def _adam_launch(form):
    def launch(ctx, arena):
        from nsd_amd import ops
        n = ctx.p0.numel()
        p, m, v = arena.buf("p", (n,)), arena.buf("m", (n,)), arena.buf("v", (n,))
        p.copy_(ctx.p0), m.copy_(ctx.m0), v.copy_(ctx.v0)
        kw = dict(skip=ctx.skip0) if form == "guarded" else dict(skip=ctx.skip1) if form == "skipped" else dict(step_dev=ctx.step_dev) if form == "dev" else {}
        ops.adam_step(p, ctx.g, m, v, step=3, **ADAM, **kw)
        return dict(p=p, m=m, v=v)
    return launch


def _adam_verify(form):
    def verify(ctx, got, dev):
        from nsd_amd import ops
        if form == "skipped":
            assert all(torch.equal(got[k], getattr(ctx, k + "0").cpu()) for k in ("p", "m", "v"))
            return
        p, m, v = ctx.p0_np.copy(), ctx.m0_np.copy(), ctx.v0_np.copy()
        orc.adam(p, ctx.g_np, m, v, lr=ADAM["lr"], weight_decay=ADAM["weight_decay"], step=3)
        assert np.abs(_np(got["p"]) - p).max() < 1e-6
        pt, mt, vt = ctx.p0.clone(), ctx.m0.clone(), ctx.v0.clone()
        ops.adam_step(pt, ctx.g, mt, vt, step=3, **ADAM)
        assert torch.equal(got["p"], pt.cpu()) and torch.equal(got["m"], mt.cpu()) and torch.equal(got["v"], vt.cpu())
    return verify


def _adam_change(ctx):
    ctx.g.mul_(-0.5)


ROUTES += [Small(f"adam-step{'-' + f if f else ''}-n1001", _adam_make, _adam_launch(f), _adam_verify(f), _adam_change) for f in ("", "guarded", "skipped", "dev")]


# nsd_grad_reduce with accumulate = 1 at an odd parameter count: old + the overwriting reduction, bit for bit
# (tests/test_gpu_head_dims.py::test_grad_reduce_accumulates_bitwise_at_an_odd_parameter_count)
def _acc_make(dev, grow):
    ctx = Fp32Step("", 8, 48, 2, 8, 64, (0, 5), 9).setup(dev, 0, grow)
    assert ctx.spec.param_count == 33753
    ctx.old = to_dev((np.random.RandomState(5).standard_normal(ctx.spec.param_count) * 1e-2).astype(np.float32), dev)
    ctx.inputs.append(ctx.old)
    return ctx


def _acc_launch(ctx, arena):
    from nsd_amd import ops
    spec, B, T = ctx.spec, ctx.B, ctx.T
    ws = arena.buf("workspace", (bc.workspace_bytes(spec, B, T) // 4,))
    out = dict(logits=arena.buf("logits", (B, spec.K)), grads=arena.buf("grads", (spec.param_count,)), acc=arena.buf("acc", (spec.param_count,)))
    out["acc"].copy_(ctx.old)
    ops.train_step_grads(spec, ctx.flat, ctx.x, ws, ctx.y, out["logits"], out["grads"], **ctx.masks)
    dd = spec.dims(B, T)
    ops._call("nsd_grad_reduce", ws.device, C.byref(dd), ws.data_ptr(), ws.numel() * 4, out["acc"].data_ptr(), 1, ops.STREAM)
    return out


def _acc_verify(ctx, got, dev):
    assert got["grads"].abs().max().item() > 0 and torch.equal(got["acc"], ctx.old.cpu() + got["grads"])


ROUTES.append(Small("grad-reduce-accumulate-odd-p", _acc_make, _acc_launch, _acc_verify))


# nsd_gemm_bf16.  Bounds: fp32 C 2e-5 * sqrt(K) * 4, bf16 C and tiles 2^-8 * max + 1e-3, epilogue 3 a permutation of epilogue 2 bit for
# bit: tests/test_gpu_seqpath.py (test_gemm_bf16_all_operand_layouts, _split_k_shift_and_tile_epilogue, _large_tile_kernel)
def _bf(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(torch.bfloat16)


def _gemm_make(M, N, K, kmajor, seed, grow_m=8):
    def make(dev, grow):
        Mm = M + (grow_m if grow else 0)
        rs = np.random.RandomState(seed + grow)
        a = _bf(rs.standard_normal((K, Mm) if kmajor else (Mm, K)).astype(np.float32), dev)
        b = _bf(rs.standard_normal((K, N) if kmajor else (N, K)).astype(np.float32), dev)
        return _ns(a=a, b=b, bias=to_dev(rs.standard_normal(Mm).astype(np.float32), dev), x=a)
    return make


def _gemm_dims(ctx, kmajor):
    return (ctx.a.shape[1] if kmajor else ctx.a.shape[0]), (ctx.b.shape[1] if kmajor else ctx.b.shape[0]), (ctx.a.shape[0] if kmajor else ctx.a.shape[1])


def _gemm_ep0_launch(splits, shift, kmajor):
    def launch(ctx, arena):
        from nsd_amd import ops
        M, N, K = _gemm_dims(ctx, kmajor)
        c = arena.buf("c", (splits * M, N)).view(splits, M, N)             # splits * M * ldc floats, exactly (one guard row = one row of C)
        ops.gemm_bf16(ctx.a, ctx.b, a_kmajor=kmajor, b_kmajor=kmajor, b_shift=shift, splits=splits, c=c)
        return dict(c=c)
    return launch


def _gemm_ep0_verify(shift, kmajor):
    def verify(ctx, got, dev):
        a, b = ctx.a.cpu().double(), ctx.b.cpu().double()
        am, bm = (a.t(), b) if kmajor else (a, b.t())                        # [M,K], [K,N]
        bs = torch.zeros_like(bm)
        if shift < 0:
            bs[-shift:] = bm[:shift]
        elif shift > 0:
            bs[:-shift] = bm[shift:]
        else:
            bs = bm
        err = float((got["c"].double().sum(0) - am @ bs).abs().max())
        print(f"gemm epilogue 0: max error {err:.2e}")
        assert err < 2e-5 * am.shape[1] ** 0.5 * 4, err
    return verify


def _gemm_ep_launch(ep):
    def launch(ctx, arena):
        from nsd_amd import ops
        M, N, _ = _gemm_dims(ctx, False)
        shape = {1: (M, N), 2: (N // 32, M // 32, 64, 16), 3: (N // 32, M // 32, 4, 64, 4)}[ep]
        c = arena.buf("c", (shape[0] * shape[1],) + shape[2:], torch.bfloat16).view(shape) if ep > 1 else arena.buf("c", shape, torch.bfloat16)
        ops.gemm_bf16(ctx.a, ctx.b, epilogue=ep, bias=ctx.bias if ep > 1 else None, c=c)
        return dict(c=c)
    return launch


def _gemm_ep_verify(ep):
    def verify(ctx, got, dev):
        M, N, _ = _gemm_dims(ctx, False)
        ref = (ctx.a.cpu().double() @ ctx.b.cpu().double().t()).float().numpy()
        if ep == 1:
            assert np.abs(_np(got["c"]) - ref).max() <= 2 ** -8 * np.abs(ref).max() + 1e-3
            return
        tiles = got["c"]
        if ep == 3:                                          # [N/32][M/32][4][64][4] -> epilogue 2's [N/32][M/32][64][16]
            tiles = tiles.permute(0, 1, 3, 2, 4).contiguous().view(N // 32, M // 32, 64, 16)
        tiles, ref = _np(tiles), ref + _np(ctx.bias)[:, None]
        lane, r = np.arange(64)[:, None], np.arange(16)[None, :]
        rows = 8 * (r // 4) + 4 * (lane >> 5) + (r % 4)
        cols = np.broadcast_to(lane & 31, rows.shape)
        for nt in range(N // 32):
            for mt in range(M // 32):
                want = ref[32 * mt + rows, 32 * nt + cols]
                assert np.abs(tiles[nt, mt] - want).max() <= 2 ** -8 * np.abs(want).max() + 1e-3, (nt, mt)
    return verify


def _gemm_large_verify(ctx, got, dev):
    ref = ctx.a.float() @ ctx.b.float().t()                  # (fp32 on the GPU, as the existing test: exact bf16 products, another order)
    err = float((got["c"][0].to(dev) - ref).abs().max())
    assert err < 2e-5 * ctx.a.shape[1] ** 0.5 * 4, err


def _gemm_change(ctx):
    ctx.a.mul_(-0.5)


for splits in (1, 4):
    for shift in (1, -1):
        ROUTES.append(Small(f"gemm-ep0-splits{splits}-shift{shift:+d}", _gemm_make(40, 24, 72, True, 5), _gemm_ep0_launch(splits, shift, True),
                            _gemm_ep0_verify(shift, True), _gemm_change))
ROUTES += [Small(f"gemm-ep{ep}-m64-n32", _gemm_make(64, 32, 72, False, 6, grow_m=32), _gemm_ep_launch(ep), _gemm_ep_verify(ep), _gemm_change)
           for ep in (1, 2, 3)]
ROUTES.append(Small("gemm-large-tile", _gemm_make(4096 + 72, 4096 - 56, 200, False, 11, grow_m=0), _gemm_ep0_launch(1, 0, False),
                    _gemm_large_verify, _gemm_change))


# ---- the driver --------------------------------------------------------------------------------------------------------------------
def _finite(route, got):
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), (route.id, k, "not finite")


def _evaluate(route, dev, cus, fill, ctx=None):
    """one evaluation of a route on guarded buffers with `fill`: (a), (b), (d) -> (ctx, outputs on the host)"""
    cur = torch.cuda.current_stream(dev)
    prior = None
    if fill == "stale":                                     # a complete earlier evaluation: larger shape, other parameters
        prior = bc.Arena(dev, "zeros")
        route.run(route.setup(dev, cus, True), prior)
        cur.synchronize()
        prior.check()
    ctx = route.setup(dev, cus, False) if ctx is None else ctx
    arena = bc.Arena(dev, fill, prior)
    snap = bc.snapshot(*ctx.inputs)
    outs = route.run(ctx, arena)
    cur.synchronize()
    arena.check()                                           # (a)
    assert snap.unchanged(), (route.id, "inputs written", snap.changed())           # (b)
    got = {k: v.detach().clone().cpu() for k, v in outs.items()}
    _finite(route, got)                                     # (d)
    return ctx, got


def _baseline(route, dev, cus):
    """the "zeros" run of a route and its comparison with the route's reference (e), once per session"""
    if route.id not in _BASE:
        try:
            ctx, got = _evaluate(route, dev, cus, "zeros")
            route.check(ctx, got, dev)
            _BASE[route.id] = got
        except BaseException as e:
            _BASE[route.id] = e
            raise
    if isinstance(_BASE[route.id], BaseException):
        raise AssertionError(f"{route.id}: the 'zeros' run failed: {_BASE[route.id]!r}")
    return _BASE[route.id]


def _same_bits(route, mode, base, got):
    assert set(base) == set(got)
    for k in base:                                          # (c)
        a, b = base[k].contiguous().view(-1).view(torch.uint8), got[k].contiguous().view(-1).view(torch.uint8)
        if not torch.equal(a, b):
            bad = (a != b).nonzero()
            raise AssertionError(f"{route.id} [{mode}]: output {k!r} differs from the 'zeros' run in {bad.numel()} bytes, first at byte {int(bad[0, 0])}")


_BUSY = {}


def _busy(dev):
    """keeps the CURRENT stream busy for some milliseconds (eight 4096^3 fp32 products): what is enqueued on it next starts late"""
    if dev not in _BUSY:
        a = torch.randn((4096, 4096), device=dev)
        _BUSY[dev] = (a, torch.empty_like(a))
    a, out = _BUSY[dev]
    for _ in range(8):
        torch.mm(a, a, out=out)


def _graph_replay(route, dev, cus):
    cur = torch.cuda.current_stream(dev)
    ctx = route.setup(dev, cus, False)
    arena = bc.Arena(dev, "nan32")
    side = torch.cuda.Stream(dev)
    side.wait_stream(cur)
    with torch.cuda.stream(side):                           # eager warm-up, as Trainer.step_static does: it also allocates the arena's buffers
        route.run(ctx, arena)
    cur.wait_stream(side)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                               # one stream, a linear graph, the default capture error mode
        outs = route.run(ctx, arena)
    route.mutate(ctx)
    for gd in arena.bufs.values():                          # whatever the warm-up left: the replay writes every output again
        bc.fill_payload(gd.store[gd.off:gd.off + gd.nbytes], "ones")
    snap = bc.snapshot(*ctx.inputs)
    g.replay()
    torch.cuda.synchronize(dev)
    arena.check()
    assert snap.unchanged(), (route.id, "inputs written by the replay", snap.changed())
    got = {k: v.detach().clone().cpu() for k, v in outs.items()}
    _finite(route, got)
    _, eager = _evaluate(route, dev, cus, "nan32", ctx)
    for k in eager:
        assert torch.equal(got[k].contiguous().view(-1).view(torch.uint8), eager[k].contiguous().view(-1).view(torch.uint8)), (route.id, k, "replay != eager")


PARAMS = [pytest.param(r, m, id=f"{r.id}-{m}") for r in ROUTES for m in bc.FILLS + ("side",) + (("graph",) if r.graph else ())]


def test_route_ids_are_unique_and_cover_the_modes():
    ids = [r.id for r in ROUTES]
    assert len(set(ids)) == len(ids)
    assert all(r.graph != r.seq for r in ROUTES) and sum(r.seq for r in ROUTES) == 11


@pytest.mark.parametrize("route,mode", PARAMS)
def test_route_keeps_the_buffer_and_stream_contract(nsd, dev, cus, route, mode):
    t0 = time.time()
    if route.seq:
        assert not _SEQ_TIMED_OUT, f"a scan group timed out in {_SEQ_TIMED_OUT}: no further launch on the sequence path, nothing is retried"
    try:
        base = _baseline(route, dev, cus)
        if mode in bc.FILLS[1:]:
            _, got = _evaluate(route, dev, cus, mode)
            _same_bits(route, mode, base, got)
        elif mode == "side":
            cur, side = torch.cuda.current_stream(dev), torch.cuda.Stream(dev)
            ctx = route.setup(dev, cus, False)
            side.wait_stream(cur)
            _busy(dev)                                      # the legacy default stream, after the side stream's wait was recorded
            with torch.cuda.stream(side):
                _, got = _evaluate(route, dev, cus, "nan32", ctx)        # (it synchronises the side stream before it reads)
            _same_bits(route, mode, base, got)
        elif mode == "graph":
            _graph_replay(route, dev, cus)
    except Exception as e:                                  # a GPU fault ends the session: nothing more is started on a faulted device
        if "illegal memory access" in str(e) or "hipErrorIllegalAddress" in str(e) or "hipErrorLaunchFailure" in str(e):
            pytest.exit(f"GPU fault in {route.id} [{mode}]: {e}", returncode=3)
        raise
    dt = time.time() - t0
    if dt > SLOWEST[0]:
        SLOWEST[:] = [dt, f"{route.id}-{mode}"]
    print(f"[{route.id}] {mode}: ok, {dt:.2f} s  outputs: {', '.join(base)}")


def test_zz_wall_time(nsd, dev):
    torch.cuda.synchronize()
    print(f"\ntests/test_gpu_buffer_contract.py: {len(PARAMS)} cases, wall time since import {time.time() - T_START:.0f} s, slowest case "
          f"{SLOWEST[0]:.1f} s ({SLOWEST[1]})")
