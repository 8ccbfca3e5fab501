"""Per-model step settings (nsd_multi_hyper_path, NSD_FLAG_MODEL_P, the `_each` entry points) and nsd_amd.grid, on the host: refusal
order and texts -- every call below is refused, or returns, before a launch -- and the grid's parsing and packing.  No GPU."""
import ctypes as C

import pytest

import nsd_amd
from nsd_amd import _lib

FAKE = 4096                                                         # never dereferenced
E_INVALID, E_WORKSPACE = -1, -3


def _err(L):
    return L.nsd_last_error().decode()


def _rngs(M, probs=None):
    probs = probs or [(0.6, 0.6)] * M
    return (_lib.Rng * M)(*[_lib.Rng(1 + m, 4, *probs[m]) for m in range(M)])


def _opts(M, **bad):
    base = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_scale=1.0, max_norm=0.0, sched=0, warmup_steps=0,
                total_steps=0, step_size=1, min_ratio=0.0, gamma=1.0)
    arr = (_lib.Opt * M)()
    for m in range(M):
        for k, v in {**base, **(bad if m == M - 1 else {})}.items():
            setattr(arr[m], k, v)
    return arr


def test_the_feature_is_detected_by_its_symbol_and_covers_the_model_batched_domain():
    L = nsd_amd.load_library()
    assert L.nsd_version() == 301 and _lib.NSD_FLAG_MODEL_P == 16
    for dims in ((4, 10, 8, 48, 2, 3, 32), (4, 1024, 8, 48, 2, 8, 64), (4, 1025, 8, 48, 2, 3, 32), (4, 10, 8, 64, 2, 3, 32), (4, 10, 8, 48, 2, 9, 32),
                 (4, 0, 8, 48, 2, 3, 32), (0, 10, 8, 48, 2, 3, 32)):
        d = _lib.Dims(*dims)
        for M in (0, 1, 2, 32, 33):
            assert L.nsd_multi_hyper_path(C.byref(d), M) == L.nsd_multi_path(C.byref(d), M), (dims, M)
    d = _lib.Dims(4, 10, 8, 48, 2, 3, 32)
    assert L.nsd_multi_hyper_path(C.byref(d), 3) == 1 and L.nsd_multi_hyper_path(None, 3) == 0


@pytest.mark.parametrize("sym,who", [("nsd_multi_train_fwd", "multi_train_fwd"), ("nsd_multi_train_fwd_soft", "multi_train_fwd_soft"),
                                     ("nsd_multi_train_bwd", "multi_train_bwd")])
def test_per_model_probabilities_need_the_flag(sym, who):
    """Mixed probabilities: refused with the text they always had without NSD_FLAG_MODEL_P; with it the call goes on to the workspace
    refusal.  A probability outside [0, 1) is refused with the entry named, the residual flag as before, and M = 1 strips the bit."""
    L = nsd_amd.load_library()
    d, M = _lib.Dims(4, 10, 8, 48, 2, 3, 32), 3
    need = L.nsd_multi_workspace_bytes(C.byref(d), M, None)
    mixed = [(0.0, 0.0), (0.3, 0.6), (0.6, 0.25)]

    def call(rng, flags, M=M, bytes_=need - 4):
        r = C.cast(rng, C.c_void_p) if rng is not None else None
        if sym == "nsd_multi_train_bwd":
            return getattr(L, sym)(C.byref(d), M, FAKE, FAKE, 0, r, flags, FAKE, bytes_, None)
        return getattr(L, sym)(C.byref(d), M, FAKE, FAKE, 0, r, FAKE, flags, FAKE, bytes_, FAKE, None)
    assert call(_rngs(M, mixed), 0) == E_INVALID
    assert _err(L).startswith(f"{who}: rng[1] has p_lstm / p_head 0.3 / 0.6, rng[0] 0 / 0: all models share the probabilities")
    assert call(_rngs(M, mixed), _lib.NSD_FLAG_MODEL_P) == E_WORKSPACE
    assert _err(L) == f"{who}: workspace of {need - 4} bytes is smaller than nsd_multi_workspace_bytes() = {need}"
    assert call(_rngs(M), _lib.NSD_FLAG_MODEL_P) == E_WORKSPACE                       # equal probabilities with the flag
    assert call(None, _lib.NSD_FLAG_MODEL_P) == E_WORKSPACE                           # no random streams with the flag
    assert call(_rngs(M, [(0.0, 0.0), (0.3, 0.6), (0.6, 1.0)]), _lib.NSD_FLAG_MODEL_P) == E_INVALID
    assert _err(L) == f"{who}: rng[2]: p_lstm / p_head 0.6 / 1 out of [0,1)"
    assert call(_rngs(M, [(1.0, 0.0), (0.3, 0.6), (0.6, 0.5)]), _lib.NSD_FLAG_MODEL_P) == E_INVALID and _err(L) == "rng: p out of [0,1)"
    assert call(_rngs(M, mixed), _lib.NSD_FLAG_MODEL_P | _lib.NSD_FLAG_RESIDUAL) == E_INVALID
    assert _err(L) == f"{who}: flags 0x11: no residual extension on the model-batched path"
    need1 = L.nsd_multi_workspace_bytes(C.byref(d), 1, None)
    assert call(_rngs(1), _lib.NSD_FLAG_MODEL_P, M=1, bytes_=need1 - 4) == E_WORKSPACE


def test_refusal_order_of_augment_each():
    L = nsd_amd.load_library()
    d, M = _lib.Dims(5, 11, 3, 1, 1, 1, 1), 4

    def call(augs, d=d, M=M, x=FAKE, y=FAKE + (1 << 20), rng=True, flags=0, stride=0):
        arr = (_lib.Aug * len(augs))(*[_lib.Aug(*a) for a in augs]) if augs is not None else None
        r = _rngs(max(M, 1)) if rng else None
        return L.nsd_augment_each(C.byref(d) if d is not None else None, M, x, stride, C.cast(arr, C.c_void_p) if arr is not None else None,
                                  C.cast(r, C.c_void_p) if r is not None else None, None, flags, y, None)
    ok = [(0, 0.0, 0.0, 0.0), (2, 0.0, 0.0, 0.0), (0, 0.1, 0.2, 0.3), (3, 0.2, 0.1, 0.5)]
    assert call(ok, d=None) == E_INVALID and _err(L) == "augment_each: dims is NULL"
    assert call(ok, M=33) == E_INVALID and _err(L) == "augment_each: M = 33 models outside [1, 32]"
    assert call(None) == E_INVALID and _err(L) == "augment_each: null pointer (x, y, aug, rng)"
    assert call(ok, flags=2) == E_INVALID and _err(L) == "augment_each: unknown flag bits 0x2"
    for m, bad, text in ((2, (11, 0.0, 0.0, 0.0), "max_shift 11 outside [0, T = 11)"), (0, (0, 1.0, 0.0, 0.0), "scale_range 1 outside [0, 1)"),
                         (3, (0, 0.0, 1.5, 0.0), "p_channel 1.5 outside [0, 1)"), (1, (0, 0.0, 0.0, -1.0), "noise_std -1 negative or not finite")):
        augs = list(ok)
        augs[m] = bad
        assert call(augs, stride=-1) == E_INVALID                    # a bad entry is named ahead of the stride and the overlap
        assert _err(L) == f"augment_each: aug[{m}]: {text}"
    assert call(ok, stride=-1) == E_INVALID and _err(L).startswith("augment_each: x_model_stride -1")
    assert call(ok, y=FAKE) == E_INVALID and _err(L).startswith("augment_each: y overlaps x")
    assert call(ok, d=_lib.Dims(0, 11, 3, 1, 1, 1, 1)) == 0           # an empty batch: nothing to launch
    # the twin's texts are what they were
    a = _lib.Aug(11, 0.0, 0.0, 0.0)
    r = _rngs(M)
    assert L.nsd_augment(C.byref(d), M, FAKE, 0, C.byref(a), C.cast(r, C.c_void_p), None, 0, FAKE + (1 << 20), None) == E_INVALID
    assert _err(L) == "augment: max_shift 11 outside [0, T = 11)"


def test_refusal_order_of_mixup_each():
    L = nsd_amd.load_library()
    d, M = _lib.Dims(5, 11, 3, 1, 1, 3, 1), 4

    def call(mixes, d=d, M=M, x=FAKE, y=FAKE + (1 << 20), labels=FAKE, stride=0):
        arr = (_lib.Mix * len(mixes))(*[_lib.Mix(*a) for a in mixes]) if mixes is not None else None
        r = _rngs(max(M, 1))
        return L.nsd_mixup_each(C.byref(d) if d is not None else None, M, x, stride, labels, None, C.cast(arr, C.c_void_p) if arr is not None else None,
                                C.cast(r, C.c_void_p), None, y, FAKE, None)
    ok = [(0.0, 0.0), (0.0, 0.1), (0.4, 0.0), (1.0, 0.2)]             # (mix, smoothing)
    assert call(ok, d=None) == E_INVALID and _err(L) == "mixup_each: dims is NULL"
    assert call(ok, M=0) == E_INVALID and _err(L) == "mixup_each: M = 0 models outside [1, 32]"
    assert call(None) == E_INVALID and _err(L) == "mixup_each: null pointer (labels, targets, mix, rng)"
    bad = list(ok)
    bad[2] = (0.4, 1.0)
    assert call(bad, x=None) == E_INVALID and _err(L) == "mixup_each: mix[2]: smoothing 1 outside [0, 1)"
    bad[2] = (1.5, 0.0)
    assert call(bad) == E_INVALID and _err(L) == "mixup_each: mix[2]: mix 1.5 outside [0, 1]"
    assert call(ok, y=None) == E_INVALID and _err(L) == "mixup_each: x and y are given together or not at all"
    assert call(ok, x=None, y=None) == E_INVALID and _err(L) == "mixup_each: mix[2]: mix = 0.4 needs the windows x and y"
    assert call(ok, stride=7) == E_INVALID and _err(L).startswith("mixup_each: x_model_stride 7")
    assert call(ok, y=FAKE) == E_INVALID and _err(L).startswith("mixup_each: y overlaps x")
    assert call(ok, d=_lib.Dims(0, 11, 3, 1, 1, 3, 1)) == 0
    m1 = _lib.Mix(0.4, 0.0)
    r = _rngs(M)
    assert L.nsd_mixup(C.byref(d), M, None, 0, FAKE, None, C.byref(m1), C.cast(r, C.c_void_p), None, None, FAKE, None) == E_INVALID
    assert _err(L) == "mixup: mix = 0.4 needs the windows x and y"


@pytest.mark.parametrize("M", [1, 3])
def test_refusal_order_of_multi_grad_reduce_clip_adam_each(M):
    """dims / M / shape, the null-pointer set, opt entry by entry with the index named, the step, opt_state, then the workspace."""
    L = nsd_amd.load_library()
    who = "multi_grad_reduce_clip_adam_each"
    d = _lib.Dims(4, 10, 8, 48, 2, 3, 32)
    need = L.nsd_multi_workspace_bytes(C.byref(d), M, None)
    P = L.nsd_param_count(8, 48, 2, 3, 32)
    st_need = L.nsd_opt_state_bytes(P, M)

    def call(opts, d=d, M=M, grads=FAKE, step=1, state=FAKE, st_bytes=st_need, ws=FAKE, bytes_=need - 4):
        return L.nsd_multi_grad_reduce_clip_adam_each(C.byref(d) if d is not None else None, M, ws, bytes_, grads, FAKE, FAKE, FAKE,
                                                      C.cast(opts, C.c_void_p) if opts is not None else None, step, None, state, st_bytes, None)
    assert call(_opts(M), d=None) == E_INVALID and _err(L) == f"{who}: dims is NULL"
    assert call(_opts(M), M=33) == E_INVALID and _err(L) == f"{who}: M = 33 models outside [1, 32]"
    assert call(_opts(M), d=_lib.Dims(4, 10, 8, 64, 2, 3, 32)) == E_INVALID and _err(L).startswith(f"{who}: shape outside the model-batched path")
    assert call(_opts(M, max_norm=-1.0), grads=None) == E_INVALID and _err(L) == f"{who}: null pointer"
    assert call(None) == E_INVALID and _err(L) == f"{who}: opt is NULL"
    for bad, text in ((dict(max_norm=-1.0), "max_norm -1 negative or NaN"), (dict(sched=7), "sched 7 unknown (NSD_SCHED_CONSTANT / _COSINE / _STEP)"),
                      (dict(sched=1, total_steps=3, warmup_steps=3), "total_steps 3 must exceed warmup_steps 3 for the cosine schedule"),
                      (dict(step_size=0), "step_size 0 must be >= 1"), (dict(gamma=0.0), "gamma 0 outside (0, 1]")):
        assert call(_opts(M, **bad), step=0, state=None) == E_INVALID
        assert _err(L) == f"{who}: opt[{M - 1}]: {text}"
    assert call(_opts(M), step=0) == E_INVALID and _err(L) == f"{who}: step 0 must be >= 1 (or pass step_dev)"
    assert call(_opts(M), state=None) == E_INVALID and _err(L) == f"{who}: opt_state is NULL"
    assert call(_opts(M), st_bytes=st_need - 8) == E_WORKSPACE and _err(L).startswith(f"{who}: opt_state of {st_need - 8} bytes is smaller")
    assert call(_opts(M), ws=None) == E_INVALID and _err(L) == f"{who}: workspace is NULL"
    assert call(_opts(M)) == E_WORKSPACE
    assert _err(L) == f"{who}: workspace of {need - 4} bytes is smaller than nsd_multi_workspace_bytes() = {need}"


def test_python_settings_given_once_or_per_model():
    from nsd_amd import ops
    assert ops._per_model(0.5, 3, "x") == (0.5, None)
    assert ops._per_model([0.5, 0.5, 0.5], 3, "x") == (0.5, None)                     # equal entries: the single setting's route
    assert ops._per_model([0.5, 0.25, 0.5], 3, "x") == (None, [0.5, 0.25, 0.5])
    a, b = ops.Augment(max_shift=2), ops.Augment(noise_std=0.1)
    assert ops._per_model([a, ops.Augment(max_shift=2)], 2, "x") == (a, None) and ops._per_model((a, b), 2, "x") == (None, [a, b])
    with pytest.raises(nsd_amd.NsdError, match="2 entries for 3 models"):
        ops._per_model([0.5, 0.25], 3, "augment")
    o1, o2 = ops.opt_struct(lr=1e-3), ops.opt_struct(lr=2e-3)
    assert ops._per_model([o1, ops.opt_struct(lr=1e-3)], 2, "opt", key=bytes)[1] is None
    assert ops._per_model([o1, o2], 2, "opt", key=bytes)[1] is not None


def test_grid_parsing_product_order_and_packing():
    from nsd_amd import grid
    g = grid.parse_grid(["lr=1e-3,3e-3", "dropout=0.4,0.6,0.7", "aug-shift=0,4"])
    assert g == [("lr", [1e-3, 3e-3]), ("dropout", [0.4, 0.6, 0.7]), ("aug_shift", [0, 4])] and isinstance(g[2][1][1], int)
    cfgs = grid.grid_product(g)
    assert len(cfgs) == 12 and cfgs[0] == dict(lr=1e-3, dropout=0.4, aug_shift=0) and cfgs[1] == dict(lr=1e-3, dropout=0.4, aug_shift=4)
    assert cfgs[2] == dict(lr=1e-3, dropout=0.6, aug_shift=0) and cfgs[6] == dict(lr=3e-3, dropout=0.4, aug_shift=0)       # the first key varies slowest
    assert grid.grid_product([]) == [{}]
    assert set(grid.GRID_KEYS) == {"lr", "weight_decay", "dropout", "label_smoothing", "mixup", "clip_grad_norm", "aug_shift", "aug_scale",
                                   "aug_channel_drop", "aug_noise"}
    opts = {a.dest for a in grid.build_parser()._actions}
    assert all(attr in opts for attr, _ in grid.GRID_KEYS.values()) and "grid" in opts                 # 1:1 with train.py's options
    for bad, msg in ((["momentum=0.9"], "unknown key 'momentum'"), (["lr"], "unknown key"), (["lr=1e-3", "lr=2e-3"], "lr is given twice"),
                     (["lr=fast"], "float values"), (["aug_shift=1.5"], "int values"), (["dropout=0.4,0.4"], "a value is given twice")):
        with pytest.raises(ValueError, match=msg):
            grid.parse_grid(bad)
    assert grid.train_args(dict(lr=3e-3, aug_channel_drop=0.1)) == ["--lr", "0.003", "--aug-channel-drop", "0.1"]
    # configurations x folds into launches of at most 32 models, whole configurations only
    assert grid.pack_groups(4, 5) == [[0, 1, 2, 3]]
    assert grid.pack_groups(7, 5) == [[0, 1, 2, 3, 4, 5], [6]]
    assert grid.pack_groups(3, 32) == [[0], [1], [2]] and grid.pack_groups(5, 10) == [[0, 1, 2], [3, 4]]
    assert grid.pack_groups(2, 17) == [[0], [1]]
    assert all(len(gp) * 5 <= 32 for gp in grid.pack_groups(40, 5)) and sum(grid.pack_groups(40, 5), []) == list(range(40))
    with pytest.raises(ValueError, match="33 folds per configuration but one launch takes at most 32 models"):
        grid.pack_groups(2, 33)


def test_grid_refuses_on_the_command_line_before_any_work(capsys):
    from nsd_amd import grid
    for argv, msg in ((["--synthetic", "64", "--kfold", "3", "--grid", "speed=1,2"], "unknown key 'speed'"),
                      (["--synthetic", "64", "--grid", "lr=1e-3,2e-3"], "the folds of --kfold K"),
                      (["--synthetic", "64", "--kfold", "3", "--hidden", "64", "--grid", "lr=1e-3,2e-3"], "H = 48 fp32"),
                      (["--synthetic", "64", "--kfold", "3", "--grid", "dropout=0.4,1.0"], "dropout 1.0 outside"),
                      (["--synthetic", "64", "--kfold", "3", "--T", "40", "--grid", "aug_shift=2,40"], "aug_shift 40 must be smaller than --T 40")):
        with pytest.raises(SystemExit) as e:
            grid.main(argv)
        assert e.value.code == 2 and msg in capsys.readouterr().err, argv
