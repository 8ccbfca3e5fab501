"""Global-norm clipping and learning-rate schedules (nsd_opt of include/nsd.h), the parts that need no GPU: the host schedule factor
against tests/optim_ref.py and torch's schedulers, optim_ref's clipped Adam against clip_grad_norm_ + torch.optim.Adam, every refusal
of the launching entry points (they come before any launch), the size of opt_state, LrSchedule's validation, and the routing promise
that a trainer with both options off never names a new symbol."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import nsd_amd
from nsd_amd import _lib, ops
from tests import optim_ref as ref

NEW_SYMBOLS = {"nsd_lr_factor", "nsd_opt_state_bytes", "nsd_opt_state_init", "nsd_grad_reduce_clip_adam", "nsd_grad_norm",
               "nsd_adam_step_clip", "nsd_multi_grad_reduce_clip_adam"}
N_COS = 11                       # N' of the grids below


def _opt(kind="constant", W=0, total=0, min_ratio=0.0, step_size=1, gamma=1.0, max_norm=0.0, **kw):
    o = ops.opt_struct(max_norm=max_norm, **kw)
    o.sched, o.warmup_steps, o.total_steps, o.step_size, o.min_ratio, o.gamma = _lib.NSD_SCHED.get(kind, 7), W, total, step_size, min_ratio, gamma
    return o


def _steps(W):
    """across the warm-up edge, N' and N' + 7"""
    return sorted({1, 2, max(W - 1, 1), max(W, 1), W + 1, W + 2, W + N_COS - 1, W + N_COS, W + N_COS + 1, W + N_COS + 2, W + N_COS + 8})


@pytest.mark.parametrize("W", [0, 1, 5])
@pytest.mark.parametrize("kind", ref.KINDS)
def test_lr_factor_equals_the_restatement(kind, W):
    """nsd_lr_factor against optim_ref.lr_factor: both use libm's cos / pow in double, in the same order -> <= 1e-15"""
    L = nsd_amd.load_library()
    cfg = dict(warmup_steps=W, total_steps=W + N_COS, min_ratio=0.1, step_size=3, gamma=0.7)
    o = _opt(kind, W, W + N_COS, 0.1, 3, 0.7)
    worst = 0.0
    for s in _steps(W):
        got, want = L.nsd_lr_factor(C.byref(o), s), ref.lr_factor(kind, s, **cfg)
        worst = max(worst, abs(got - want))
        assert 0.0 <= got <= 1.0
    print(f"[lr_factor] {kind} W={W}: max |err| {worst:.2e}")
    assert worst <= 1e-15
    if kind == "cosine":                                       # past N' the factor holds at r
        assert L.nsd_lr_factor(C.byref(o), W + N_COS + 8) == L.nsd_lr_factor(C.byref(o), W + N_COS + 1) == pytest.approx(ref.f32(0.1), abs=1e-15)
    if W:
        assert L.nsd_lr_factor(C.byref(o), 1) == 1.0 / W and L.nsd_lr_factor(C.byref(o), W) == 1.0


def test_lr_factor_equals_torch_schedulers_without_warmup():
    """W = 0: CosineAnnealingLR(T_max = N', eta_min = lr r) up to T_max, and StepLR, stepped on a dummy optimizer -> 1e-12"""
    L = nsd_amd.load_library()
    lr, r, gamma = 0.05, ref.f32(0.1), ref.f32(0.7)
    for kind, make in (("cosine", lambda opt: torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=N_COS, eta_min=lr * r)),
                       ("step", lambda opt: torch.optim.lr_scheduler.StepLR(opt, step_size=3, gamma=gamma))):
        opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1, dtype=torch.float64))], lr=lr)
        sched = make(opt)
        o = _opt(kind, 0, N_COS, r, 3, gamma)
        worst = 0.0
        for s in range(1, N_COS + 2):                          # step s uses the lr after s - 1 scheduler steps: e = 0 .. N'
            worst = max(worst, abs(lr * L.nsd_lr_factor(C.byref(o), s) - opt.param_groups[0]["lr"]))
            opt.step(); sched.step()
        print(f"[lr_factor vs torch] {kind}: max |err| {worst:.2e}")
        assert worst <= 1e-12


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("clips", [True, False])
def test_restatement_equals_torch_clip_and_adam(wd, clips):
    """optim_ref.ClippedAdam (float64 fields) against clip_grad_norm_ + torch.optim.Adam in float64, 10 steps -> 1e-12"""
    rs = np.random.RandomState(3)
    n = 257
    p0 = rs.uniform(-1, 1, n)
    gs = [rs.standard_normal(n) for _ in range(10)]
    max_norm = (0.1 if clips else 10.0) * float(np.sqrt(n))
    ours = ref.ClippedAdam(p0, lr=1e-2, weight_decay=wd, max_norm=max_norm, fp32_fields=False)
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    adam = torch.optim.Adam([p], lr=1e-2, weight_decay=wd)
    clipped = []
    for g in gs:
        p.grad = torch.from_numpy(g.copy())
        total = torch.nn.utils.clip_grad_norm_([p], max_norm)
        adam.step()
        rec = ours.step(g)
        assert abs(rec["norm"] - float(total)) <= 1e-12 * float(total)
        clipped.append(rec["coef"] < 1.0)
    err = float(np.abs(ours.p - p.detach().numpy()).max())
    print(f"[optim_ref vs torch] wd={wd} clips={clips}: max |dp| {err:.2e}")
    assert all(clipped) == clips and any(clipped) == clips
    assert err <= 1e-12


def _refused(rc, code, *words):
    msg = nsd_amd.load_library().nsd_last_error().decode()
    assert rc == code, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_bad_optimizer_arguments_are_rejected_without_a_gpu():
    """Every refusal comes before any launch, so none of these needs a device; nsd_last_error names the field"""
    L = nsd_amd.load_library()
    d = _lib.Dims(4, 10, 8, 48, 2, 3, 32)
    P = ops.ModelSpec().param_count
    wsb = int(L.nsd_workspace_bytes(C.byref(d), None))
    nb = int(L.nsd_opt_state_bytes(P, 1))
    nb3 = int(L.nsd_opt_state_bytes(P, 3))
    FAKE = 4096                                                # a non-null "device pointer": nothing is dereferenced before the refusals

    def fused(o, step=1, step_dev=None, state=FAKE, bytes_=nb, ws=FAKE, wsn=wsb):
        return L.nsd_grad_reduce_clip_adam(C.byref(d), ws, wsn, FAKE, FAKE, FAKE, FAKE, C.byref(o) if o is not None else None, step, step_dev, state, bytes_, None)

    def multi(o, step=1, state=FAKE, bytes_=nb3):
        wsm = int(L.nsd_multi_workspace_bytes(C.byref(d), 3, None))
        return L.nsd_multi_grad_reduce_clip_adam(C.byref(d), 3, FAKE, wsm, FAKE, FAKE, FAKE, FAKE, C.byref(o) if o is not None else None, step, None, state, bytes_, None)

    def flat(o, step=1, step_dev=None, state=FAKE, bytes_=nb, n=P):
        return L.nsd_adam_step_clip(n, FAKE, FAKE, FAKE, FAKE, C.byref(o) if o is not None else None, step, step_dev, None, state, bytes_, None)

    bad = [(_opt(max_norm=-1.0), "max_norm"), (_opt(max_norm=float("nan")), "max_norm"), (_opt("unknown"), "sched"),
           (_opt("cosine", W=5, total=5), "total_steps"), (_opt("cosine", W=0, total=0), "total_steps"), (_opt(W=-1), "warmup_steps"),
           (_opt("step", step_size=0), "step_size"), (_opt(gamma=0.0), "gamma"), (_opt(gamma=1.5), "gamma"), (_opt(gamma=float("nan")), "gamma"),
           (_opt(min_ratio=-0.1), "min_ratio"), (_opt(min_ratio=1.1), "min_ratio")]
    for call in (fused, multi, flat):
        for o, field in bad:
            _refused(call(o), -1, field)
        _refused(call(None), -1, "opt is NULL")
        _refused(call(_opt(), step=0), -1, "step")
        _refused(call(_opt(), state=None), -1, "opt_state")
    for o, field in bad:
        assert L.nsd_lr_factor(C.byref(o), 1) < 0 and field in L.nsd_last_error().decode()
    assert L.nsd_lr_factor(C.byref(_opt()), 0) < 0 and L.nsd_lr_factor(None, 1) < 0
    # step < 1 is fine when the device counter is given: the next refusal is reached (a short opt_state)
    _refused(fused(_opt(), step=0, step_dev=FAKE, bytes_=nb - 1), -3, "opt_state", "nsd_opt_state_bytes")
    _refused(flat(_opt(), step=0, step_dev=FAKE, bytes_=nb - 1), -3, "opt_state")
    _refused(fused(_opt(), bytes_=nb - 1), -3, "opt_state")
    _refused(multi(_opt(), bytes_=nb3 - 1), -3, "opt_state")
    _refused(multi(_opt(), bytes_=nb), -3, "opt_state")      # one model's state for three
    _refused(fused(_opt(), wsn=wsb - 1), -3, "workspace")
    # null pointers
    _refused(fused(_opt(), ws=None), -1, "null")
    _refused(L.nsd_adam_step_clip(P, None, FAKE, FAKE, FAKE, C.byref(_opt()), 1, None, None, FAKE, nb, None), -1, "null")
    _refused(L.nsd_adam_step_clip(-1, FAKE, FAKE, FAKE, FAKE, C.byref(_opt()), 1, None, None, FAKE, nb, None), -1, "n<0")
    _refused(L.nsd_grad_norm(P, None, 1.0, FAKE, nb, None), -1, "null")
    _refused(L.nsd_grad_norm(P, FAKE, 1.0, None, nb, None), -1, "null")
    _refused(L.nsd_grad_norm(P, FAKE, 1.0, FAKE, nb - 1, None), -3, "opt_state")
    _refused(L.nsd_opt_state_init(None, nb, None), -1, "opt_state")
    _refused(L.nsd_opt_state_init(FAKE, 8, None), -1, "record")
    bad_d = _lib.Dims(4, 0, 8, 48, 2, 3, 32)
    assert L.nsd_grad_reduce_clip_adam(C.byref(bad_d), FAKE, wsb, FAKE, FAKE, FAKE, FAKE, C.byref(_opt()), 1, None, FAKE, nb, None) == -1
    d40 = _lib.Dims(4, 10, 8, 40, 2, 3, 32)                    # outside the model-batched path
    _refused(L.nsd_multi_grad_reduce_clip_adam(C.byref(d40), 3, FAKE, wsb, FAKE, FAKE, FAKE, FAKE, C.byref(_opt()), 1, None, FAKE, nb3, None), -1, "nsd_multi_path")


def test_opt_state_size():
    L = nsd_amd.load_library()
    for M in (1, 3, 32):
        sizes = [int(L.nsd_opt_state_bytes(n, M)) for n in (0, 1, 33, 31764, 2**20 + 1)]
        assert sizes[0] >= 16 * M and all(a < b for a, b in zip(sizes, sizes[1:])), (M, sizes)
        assert all(s % 8 == 0 for s in sizes)
    assert L.nsd_opt_state_bytes(31764, 1) == 16 + 8 * math.ceil(31764 / 32)      # one partial per 32-column reduction workgroup
    assert L.nsd_opt_state_bytes(10, 0) < 0 and L.nsd_opt_state_bytes(10, 33) < 0 and L.nsd_opt_state_bytes(-1, 1) < 0
    assert ops.opt_state_bytes(33, 2) == 2 * 16 + 2 * 8 * 2
    assert C.sizeof(_lib.Opt) == 52 and C.sizeof(_lib.OptRecord) == 16


def test_lr_schedule_validation():
    S = nsd_amd.LrSchedule
    assert S() == S(kind="constant", warmup_steps=0, total_steps=0, min_ratio=0.0, step_size=1, gamma=1.0)
    S("cosine", warmup_steps=5, total_steps=6, min_ratio=1.0); S("step", step_size=10, gamma=0.5); S(warmup_steps=100)
    for kw in (dict(kind="linear"), dict(warmup_steps=-1), dict(kind="cosine", total_steps=0), dict(kind="cosine", warmup_steps=5, total_steps=5),
               dict(step_size=0), dict(gamma=0.0), dict(gamma=1.01), dict(gamma=float("nan")), dict(min_ratio=-0.1), dict(min_ratio=1.5),
               dict(min_ratio=float("nan")), dict(warmup_steps=1.5), dict(total_steps=2**31)):
        with pytest.raises(ValueError):
            S(**kw)
    with pytest.raises(Exception):                             # frozen
        S().gamma = 0.5
    # the struct the kernels see, and the host factor through ops
    o = ops.opt_struct(lr=0.5, max_norm=None, schedule=S("cosine", warmup_steps=2, total_steps=12, min_ratio=0.25))
    assert (o.sched, o.warmup_steps, o.total_steps, o.max_norm, o.min_ratio) == (1, 2, 12, 0.0, 0.25)
    assert ops.lr_factor(o, 1) == 0.5 and ops.lr_factor(o, 3) == 1.0 and ops.lr_factor(o, 13) == 0.25
    assert ops.opt_struct().sched == 0 and ops.opt_struct(max_norm=2.0).max_norm == 2.0
    with pytest.raises(ops.NsdError):
        ops.lr_factor(o, 0)


def test_options_off_never_name_a_new_symbol(monkeypatch):
    """With clip_grad_norm and lr_schedule both None the tails are today's entry points; with either given, the clipped ones"""
    from nsd_amd.multimodel import ModelBatchTrainer
    from nsd_amd.trainer import Trainer
    names = []
    monkeypatch.setattr(ops, "_call", lambda name, dev, *a: names.append(name))
    monkeypatch.setattr(ops, "_dev_f32", lambda t, name, shape=None: None if t is None else 1)
    monkeypatch.setattr(ops, "_labels_ptr", lambda t: 1)
    spec = ops.ModelSpec()
    P = spec.param_count
    z = lambda *s: torch.zeros(*s)

    def trainer(**kw):
        t = object.__new__(Trainer)
        t.m, t.v, t.grads, t.flat, t.model = z(P), z(P), z(P), z(P), nsd_amd.EEG_LSTM()
        t.lr, t.betas, t.eps, t.weight_decay, t.step_count, t.world = 1e-3, (0.9, 0.999), 1e-8, 0.0, 1, 1
        t.clip_grad_norm, t.lr_schedule = kw.get("clip_grad_norm"), kw.get("lr_schedule")
        t._opt_on = t.clip_grad_norm is not None or t.lr_schedule is not None
        t._opt_state, t._skip, t._step_dev = torch.zeros(ops.opt_state_bytes(P), dtype=torch.uint8), z(1), None
        return t

    def tails(t):
        del names[:]
        x, y = z(4, 10, 8), torch.zeros(4, dtype=torch.int32)
        ops.train_step_grads(spec, t.flat, x, z(16), y, z(4, 3), t.grads, adam=t._fused_tail())      # world == 1
        t._adam()                                                                                  # world > 1, bf16, graph segment B
        t._issue_segment_b()
        return list(names)
    off = tails(trainer())
    assert off == ["nsd_lstm_head_train", "nsd_lstm_bwd", "nsd_grad_reduce_adam", "nsd_adam_step", "nsd_adam_step"] and not NEW_SYMBOLS & set(off)
    for kw in (dict(clip_grad_norm=0.0), dict(lr_schedule=nsd_amd.LrSchedule()), dict(clip_grad_norm=1.0, lr_schedule=nsd_amd.LrSchedule("step"))):
        on = tails(trainer(**kw))
        assert on == ["nsd_lstm_head_train", "nsd_lstm_bwd", "nsd_grad_reduce_clip_adam", "nsd_grad_norm", "nsd_adam_step_clip"], kw

    def multi(opt):
        del names[:]
        ops.multi_train_step(spec, z(2, P), z(2, 4, 10, 8), torch.zeros(8, dtype=torch.int32), torch.zeros(16, dtype=torch.uint8), z(2, P),
                             m=z(2, P), v=z(2, P), opt=opt, opt_state=torch.zeros(ops.opt_state_bytes(P, 2), dtype=torch.uint8))
        return names[-1]
    assert multi(None) == "nsd_multi_grad_reduce_adam" and multi(ops.opt_struct(max_norm=1.0)) == "nsd_multi_grad_reduce_clip_adam"
    import inspect
    for cls in (Trainer, ModelBatchTrainer):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["clip_grad_norm"].default is None and sig["lr_schedule"].default is None
