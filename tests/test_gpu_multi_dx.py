"""Input gradients of M frozen models in one launch chain (nsd_multi_train_bwd_dx / nsd_multi_loss_mean of include/nsd.h; the model-batched
dx kernel of csrc/nsd_misc.hip) on the MI355X, through the C ABI.

  per model       dx against the oracle's within DX_TOL of its largest element, the gradients read through nsd_multi_grad_reduce AFTER the
                  dx call within the bounds of assert_step_vs_oracle (FAST48), hard labels and soft targets, shared and per-model windows,
                  T on both sides of the loader's 8-step chunk, C of every odd split -- and one case per launch band of the M*B trials:
                  one-trial forward (24 trials), two-trial forward with the one-trial backward on its grid (300), four-trial forward
                  with open attention records (513: the closing pass).
  single model    BIT EQUALITY holds below 513 trials in the launch (M*B: the one- and two-trial forward kernels save the same bits):
                  model m's rows are nsd_lstm_bwd's dx for that model alone on the same windows (the same backward kernel on the same
                  saved activations, and the dx kernel forms the chain of nsd_dx_launch).  From 513 trials the four-trial forward forms
                  the gate products on the matrix pipe, which the single-model launch of B = 171 trials does not: that band is held to
                  the oracle only (measured: the bits differ there), and the band test prints what it finds.
  mean            NSD_DX_MEAN is bit for bit align.mean_over_models (serial fp32 sum over m ascending, one division by float32(M)) of
                  the SAME inputs' NSD_DX_PER_MODEL output; two copies of one model give that model's dx bitwise.
  contract        dx of exactly the stated size between guards, NaN words beforehand; params / x unchanged; the same bits on a side
                  stream and from a replayed graph; refusals before any launch; a NaN sample stays in its trial's rows.

No bound here is new: DX_TOL, FAST48, LOGIT_TOL and LOSS_TOL are the table of tests/gpu_harness.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import spatial_fit_ref as sr
from tests.buffer_contract import guarded, multi_workspace_bytes, snapshot
from tests.gpu_harness import (D, FAST48, KINK_MARGIN, NAN, assert_step_vs_oracle, dev, kink_safe, nsd, oracle_step, soft_targets,  # noqa: F401  (fixtures)
                               spec_of, sync_at_the_end, to_dev)
from tests.golden.make_goldens import synth_labels, synth_params, synth_x
from oracle import nsd_oracle as orc

pytestmark = pytest.mark.gpu

E_INVALID, E_WORKSPACE = -1, -3          # NSD_E_INVALID, NSD_E_WORKSPACE of include/nsd.h


def _problem(M, B, T, Cc, shared, soft, seed=0):
    """(dims, flat [M,P], x [B,T,C] or [M,B,T,C], labels [M,B] or None, targets [M,B,K] or None) from the generators of the goldens"""
    d = orc.Dims(C=Cc)
    flats = np.stack([orc.flatten_state(kink_safe(synth_params(Cc, d.H, d.L, d.K, F=d.F, seed=seed + 11 + m), d.F), d) for m in range(M)])
    x = synth_x(B, T, C=Cc, seed=seed + 5) if shared else np.stack([synth_x(B, T, C=Cc, seed=seed + 5 + m) for m in range(M)])
    y = None if soft else np.stack([synth_labels(B, K=d.K, seed=seed + 3 + m) for m in range(M)]).astype(np.int32)
    q = np.stack([soft_targets(B, d.K, seed + 7 + 2 * m) for m in range(M)]) if soft else None
    return d, flats, x, y, q


def _names_of(fn):
    """the ABI calls ops issues while fn runs (the launch hook)"""
    import contextlib
    from nsd_amd import ops
    names = []

    @contextlib.contextmanager
    def hook(name):
        names.append(name)
        yield
    ops.set_launch_hook(hook)
    try:
        fn()
    finally:
        ops.set_launch_hook(None)
    return names


class Run:
    """forward -> nsd_multi_train_bwd_dx -> (reads) of one problem on the device, every output full of NaN beforehand"""

    def __init__(self, dev, d, flats, x, y, q):
        from nsd_amd import ops
        self.ops, self.dev, self.d, self.spec = ops, dev, d, spec_of(d)
        self.M = flats.shape[0]
        self.shared = x.ndim == 3
        self.B, self.T = x.shape[-3], x.shape[-2]
        self.params, self.x = to_dev(flats, dev), to_dev(x, dev)
        self.y = None if y is None else to_dev(y.reshape(-1), dev)
        self.q = None if q is None else to_dev(q.reshape(-1, d.K), dev)
        self.ws = ops.multi_workspace(self.spec, self.M, self.B, self.T, dev)
        self.logits = torch.empty((self.M * self.B, d.K), device=dev)

    def dx_buffer(self, reduce):
        shape = (self.B, self.T, self.d.C) if reduce == "mean" else (self.M, self.B, self.T, self.d.C)
        return guarded(shape, torch.float32, self.dev, "nan32")

    def go(self, reduce, dx=None):
        self.ws.fill_(NAN)
        self.logits.fill_(NAN)
        check = None
        if dx is None:
            dx, check = self.dx_buffer(reduce)
        loss1 = torch.full((1,), NAN, device=self.dev)
        self.ops.multi_train_dx(self.spec, self.params, self.x, self.ws, self.logits, dx, labels=self.y, targets=self.q, reduce=reduce,
                                loss_out=loss1)
        if check is not None:
            check("dx")
        return dx, loss1

    def grads(self):
        g = torch.full_like(self.params, NAN)
        d = self.spec.dims(self.B, self.T)
        self.ops._call("nsd_multi_grad_reduce", self.dev, C.byref(d), self.M, self.ws.data_ptr(), self.ws.numel() * 4, g.data_ptr(), self.ops.STREAM)
        return g.cpu().numpy()

    def loss_sums(self):
        return self.ops.multi_loss_sum(self.spec, self.ws, self.M, self.B, self.T).cpu().numpy()

    def single_dx(self, m):
        """nsd_lstm_head_train[_soft] -> nsd_lstm_bwd with dx for model m alone on its windows"""
        ops, sp, B, T = self.ops, self.spec, self.B, self.T
        xm = self.x if self.shared else self.x[m].contiguous()
        ws = ops.new_workspace(sp, B, T, self.dev)
        logits, dx = torch.empty((B, sp.K), device=self.dev), torch.full((B, T, sp.C), NAN, device=self.dev)
        ops.train_dx(sp, self.params[m].contiguous(), xm, ws, logits, dx,
                     labels=None if self.y is None else self.y[m * B:(m + 1) * B].contiguous(),
                     targets=None if self.q is None else self.q[m * B:(m + 1) * B].contiguous())
        return dx.cpu().numpy()


def _against_the_oracle(run, flats, x, y, q, dx, tag):
    d, M, B = run.d, run.M, run.B
    logits, grads, sums = run.logits.cpu().numpy().reshape(M, B, d.K), run.grads(), run.loss_sums()
    for m in range(M):
        xm = x if x.ndim == 3 else x[m]
        ref = oracle_step(d, flats[m], xm, labels=None if y is None else y[m], targets=None if q is None else q[m], want_dx=True,
                          kink=KINK_MARGIN)
        out = dict(logits=logits[m], grads=grads[m], mean_loss=float(sums[m]) / B, dx=dx[m])
        assert_step_vs_oracle(out, ref, d, FAST48, tag=f"{tag} model {m}")


# (M, B, T, C, shared windows, soft targets): M in {2, 3}, B in {1, 3}, T in {1, 5, 13, 70}, C in {1, 5, 8}, both strides, both losses
SMALL = [(2, 1, 1, 8, True, False), (3, 3, 5, 5, False, True), (2, 3, 13, 1, True, True), (3, 1, 13, 8, False, False),
         (3, 3, 70, 8, False, False), (2, 3, 70, 5, True, True), (2, 1, 5, 1, False, False), (3, 3, 1, 8, True, True)]


@pytest.mark.parametrize("M,B,T,Cc,shared,soft", SMALL)
def test_per_model_dx_and_gradients_against_the_oracle_and_the_single_model_path(nsd, dev, M, B, T, Cc, shared, soft):
    d, flats, x, y, q = _problem(M, B, T, Cc, shared, soft)
    run = Run(dev, d, flats, x, y, q)
    snap = snapshot(run.params, run.x)
    dx, _ = run.go("per_model")
    dx = dx.cpu().numpy()
    _against_the_oracle(run, flats, x, y, q, dx, f"M={M} B={B} T={T}")
    assert snap.unchanged()
    # the one-trial band -- every model's rows are nsd_lstm_bwd's dx for that model alone, bit for bit
    for m in range(M):
        assert sr.same_bits(dx[m], run.single_dx(m)), m


# one case per launch band of the M*B trials, at small T
BANDS = [(3, 8, 3, "one-trial forward"), (3, 100, 3, "two-trial forward, one-trial backward on its grid"),
         (3, 171, 5, "four-trial forward, open records closed first")]


@pytest.mark.parametrize("M,B,T,what", BANDS)
def test_every_launch_band_against_the_oracle(nsd, dev, M, B, T, what):
    d, flats, x, y, q = _problem(M, B, T, 8, False, False, seed=40)
    run = Run(dev, d, flats, x, y, q)
    dx, _ = run.go("per_model")
    dx = dx.cpu().numpy()
    _against_the_oracle(run, flats, x, y, q, dx, what)
    same = [sr.same_bits(dx[m], run.single_dx(m)) for m in range(M)]
    print(f"{M} x {B} trials ({what}): per-model dx bitwise equal to the single-model path: {same}")
    if M * B < 513:
        assert all(same)
    # soft targets in the same band (the closing pass reads dpooled of the soft head too): against the oracle
    d, flats, x, y, q = _problem(M, B, T, 8, True, True, seed=41)
    run = Run(dev, d, flats, x, y, q)
    dx, _ = run.go("per_model")
    _against_the_oracle(run, flats, x, y, q, dx.cpu().numpy(), what + ", soft targets")


@pytest.mark.parametrize("M", [1, 2, 3, 5])
def test_mean_is_the_serial_restatement_of_the_per_model_output(nsd, dev, M):
    from nsd_amd.align import mean_over_models
    B, T = 3, 13
    d, flats, x, y, q = _problem(M, B, T, 8, True, False, seed=60 + M)
    run = Run(dev, d, flats, x, y, q)
    per, loss_a = run.go("per_model")
    sums = run.loss_sums()
    g_per = run.grads()
    mean, loss_b = run.go("mean")
    assert sr.same_bits(mean.cpu().numpy(), mean_over_models(per.cpu().numpy()))
    assert np.isfinite(mean.cpu().numpy()).all() and float(mean.abs().max()) > 0
    # the parameter-gradient slabs and the losses do not depend on the mode; nsd_multi_loss_mean restates nsd_multi_loss_sum's values
    assert sr.same_bits(run.grads(), g_per) and sr.same_bits(run.loss_sums(), sums)
    want = mean_over_models(sums)
    assert sr.same_bits(loss_a.cpu().numpy(), want.reshape(1)) and sr.same_bits(loss_b.cpu().numpy(), want.reshape(1))
    if M == 1:
        assert sr.same_bits(mean.cpu().numpy(), per.cpu().numpy()[0])


def test_two_copies_of_one_model_give_its_dx_bitwise(nsd, dev):
    B, T = 3, 70
    d, flats, x, y, q = _problem(1, B, T, 8, True, False, seed=70)
    one = Run(dev, d, flats, x, y, q)
    want, loss_one = one.go("mean")
    two = Run(dev, d, np.concatenate([flats, flats]), x, np.concatenate([y, y]), None)
    got, loss_two = two.go("mean")
    assert sr.same_bits(got.cpu().numpy(), want.cpu().numpy())                        # (d + d) / 2 is exact
    assert sr.same_bits(loss_two.cpu().numpy(), loss_one.cpu().numpy())
    assert sr.same_bits(want.cpu().numpy(), one.single_dx(0))


@pytest.mark.parametrize("reduce", ["per_model", "mean"])
def test_side_stream_and_graph_replay_leave_the_same_bits(nsd, dev, reduce):
    M, B, T = 3, 3, 13
    d, flats, x, y, q = _problem(M, B, T, 8, True, False, seed=80)
    run = Run(dev, d, flats, x, y, q)
    snap = snapshot(run.params, run.x, run.y)
    want, loss = run.go(reduce)
    want, loss = want.cpu().numpy(), loss.cpu().numpy()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got, l2 = run.go(reduce)
    side.synchronize()
    assert sr.same_bits(got.cpu().numpy(), want) and sr.same_bits(l2.cpu().numpy(), loss)
    # forward + backward + loss captured once, replayed twice on buffers full of NaN
    dx, check = run.dx_buffer(reduce)
    loss1 = torch.full((1,), NAN, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run.ops.multi_train_dx(run.spec, run.params, run.x, run.ws, run.logits, dx, labels=run.y, reduce=reduce, loss_out=loss1)
    for _ in range(2):
        run.ws.fill_(NAN)
        dx.view(-1).view(torch.int32).fill_(0x7FC00000)
        g.replay()
        torch.cuda.synchronize()
        check("dx")
        assert sr.same_bits(dx.cpu().numpy(), want) and sr.same_bits(loss1.cpu().numpy(), loss)
    assert snap.unchanged()


def test_workspace_of_the_exact_size_and_a_short_one(nsd, dev):
    from nsd_amd import _lib, ops
    M, B, T = 2, 3, 5
    d, flats, x, y, q = _problem(M, B, T, 8, True, False, seed=90)
    run = Run(dev, d, flats, x, y, q)
    want, _ = run.go("mean")
    n = multi_workspace_bytes(run.spec, M, B, T)
    ws, check = guarded((n // 4,), torch.float32, dev, "nan32")
    run.ws = ws
    got, _ = run.go("mean")
    check("workspace")
    assert sr.same_bits(got.cpu().numpy(), want.cpu().numpy())
    dims = run.spec.dims(B, T)
    rc = _lib.lib().nsd_multi_train_bwd_dx(C.byref(dims), M, run.params.data_ptr(), run.x.data_ptr(), 0, 0, ws.data_ptr(), n - 4,
                                           got.data_ptr(), 1, None)
    assert rc == E_WORKSPACE and "nsd_multi_workspace_bytes" in ops._lib.lib().nsd_last_error().decode()


def test_every_refusal_comes_before_any_launch(nsd, dev):
    from nsd_amd import _lib, ops
    M, B, T = 2, 3, 5
    d, flats, x, y, q = _problem(M, B, T, 8, False, False, seed=95)
    run = Run(dev, d, flats, x, y, q)
    run.go("per_model")
    dx, check = run.dx_buffer("per_model")
    torch.cuda.synchronize()
    snap = snapshot(run.ws, dx.view(torch.int32), run.params, run.x)
    L = _lib.lib()
    dims, stride, n = run.spec.dims(B, T), B * T * 8, run.ws.numel() * 4
    P, X, W, DXP = run.params.data_ptr(), run.x.data_ptr(), run.ws.data_ptr(), dx.data_ptr()

    def call(dd=dims, m=M, p=P, xx=X, st=stride, fl=0, w=W, dxp=DXP, red=0):
        return L.nsd_multi_train_bwd_dx(None if dd is None else C.byref(dd), m, p, xx, st, fl, w, n, dxp, red, None)

    big = run.spec.dims(1 << 14, 1024)                         # 2^14 * 1024 * 48 * 4 bytes = 3 GB per model
    wide = spec_of(orc.Dims(H=64)).dims(B, T)
    cases = [(dict(dd=None), "dims"), (dict(p=None), "null"), (dict(xx=None), "null"), (dict(w=None), "null"), (dict(dxp=None), "null"),
             (dict(dd=wide), "nsd_multi"), (dict(m=0), "M = 0"), (dict(m=33), "M = 33"), (dict(red=2), "reduce = 2"), (dict(red=-1), "reduce"),
             (dict(red=1), "NSD_DX_MEAN"), (dict(fl=_lib.NSD_FLAG_RESIDUAL), "residual"), (dict(st=stride - 1), "x_model_stride"),
             (dict(st=-stride), "x_model_stride"), (dict(dd=big, st=0), "2 GB")]
    for kw, text in cases:
        assert call(**kw) == E_INVALID, kw
        assert text in L.nsd_last_error().decode(), (kw, L.nsd_last_error().decode())
    out = torch.empty(1, device=dev)
    assert L.nsd_multi_loss_mean(C.byref(dims), M, W, n, None, None) == E_INVALID
    assert L.nsd_multi_loss_mean(C.byref(dims), 0, W, n, out.data_ptr(), None) == E_INVALID
    assert L.nsd_multi_loss_mean(C.byref(dims), M, W, n - 4, out.data_ptr(), None) == E_WORKSPACE
    assert L.nsd_multi_dx_path(C.byref(dims), M) == 1 and L.nsd_multi_dx_path(C.byref(wide), M) == 0
    assert L.nsd_multi_dx_path(C.byref(dims), 33) == 0 and L.nsd_multi_dx_path(None, M) == 0
    # B = 0 is accepted and launches nothing
    assert call(dd=run.spec.dims(0, T), st=0) == 0
    torch.cuda.synchronize()
    check("dx")
    assert snap.unchanged()                                    # nothing ran: workspace, dx (NaN words), params and x are as they were
    # the Python wrapper refuses the mean over per-model windows, and an unknown mode, before its first ABI call
    for kw, text in ((dict(reduce="mean"), "shared"), (dict(reduce="sum"), "reduce")):
        names = _names_of(lambda: pytest.raises(nsd.NsdError, ops.multi_train_dx, run.spec, run.params, run.x, run.ws, run.logits, dx,
                                                   labels=run.y, **kw).match(text))
        assert names == []


def test_a_nan_sample_stays_in_its_trial(nsd, dev):
    M, B, T = 3, 3, 13
    d, flats, x, y, q = _problem(M, B, T, 8, False, False, seed=99)
    x[1, 2, 6, 3] = np.nan                                     # model 1, trial 2
    run = Run(dev, d, flats, x, y, q)
    per = run.go("per_model")[0].cpu().numpy()
    bad = ~np.isfinite(per).all(axis=(2, 3))                   # [M,B]: trials with a non-finite row
    assert bad.tolist() == [[False] * 3, [False, False, True], [False] * 3]
    assert (~np.isfinite(per[1, 2])).all(axis=1).all()         # every row of that trial
    # mean mode (shared windows): the same trial index is non-finite and no other
    d, flats, x, y, q = _problem(M, B, T, 8, True, False, seed=99)
    x[2, 6, 3] = np.nan
    run = Run(dev, d, flats, x, y, q)
    mean = run.go("mean")[0].cpu().numpy()
    assert (~np.isfinite(mean).all(axis=(1, 2))).tolist() == [False, False, True]
    assert (~np.isfinite(mean[2])).all(axis=1).all()


# ---- the model-batched dx kernel alone (diagnostic build: nsd_diag_dx), in no band's hands ----
@pytest.mark.parametrize("M,rows,Cc", [(1, 1, 8), (2, 255, 5), (3, 257, 1), (5, 700, 8), (32, 64, 7)])
def test_the_dx_kernel_alone_is_the_single_model_kernel_bit_for_bit(nsd, dev, M, rows, Cc):
    """rows on both sides of the 256-row workgroup and more than one workgroup; every C the chains are unrolled over; M up to the limit"""
    from nsd_amd import _lib, ops
    from nsd_amd.align import mean_over_models
    spec = spec_of(orc.Dims(C=Cc))
    rs = np.random.RandomState(M + rows + Cc)
    da0 = to_dev((1e-2 * rs.standard_normal((M, rows, 4 * spec.H))).astype(np.float32), dev)
    params = to_dev((0.2 * rs.standard_normal((M, spec.param_count))).astype(np.float32), dev)
    snap = snapshot(da0, params)
    with _lib.diagnostic_library():
        want = ops.dx_diag(spec, da0, params, "single_calls").cpu().numpy()
        per, check_per = guarded((M, rows, Cc), torch.float32, dev, "nan32")
        mean, check_mean = guarded((rows, Cc), torch.float32, dev, "nan32")
        ops.dx_diag(spec, da0, params, "per_model", dx=per)
        ops.dx_diag(spec, da0, params, "mean", dx=mean)
    torch.cuda.synchronize()
    check_per("dx per model")
    check_mean("dx mean")
    assert snap.unchanged()
    # the chain's order against a float64 product: K = 4H terms, each fmaf rounds once -> K * 2^-24 * sum |terms| (first order, K + 1 for the rest)
    w = params.cpu().numpy()[:, spec.offsets()["lstm.weight_ih_l0"]:][:, :4 * spec.H * Cc].reshape(M, 4 * spec.H, Cc).astype(np.float64)
    d64 = da0.cpu().numpy().astype(np.float64)
    exact, mass = np.einsum("mrk,mkc->mrc", d64, w), np.einsum("mrk,mkc->mrc", np.abs(d64), np.abs(w))
    assert (np.abs(want - exact) <= (4 * spec.H + 1) * 2.0 ** -24 * mass).all()
    assert sr.same_bits(per.cpu().numpy(), want)
    assert sr.same_bits(mean.cpu().numpy(), mean_over_models(want))
