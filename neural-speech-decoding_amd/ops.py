"""Tensor-level wrappers over the C ABI (include/nsd.h).  PyTorch is only the plumbing here: it owns the
device buffers and the HIP stream; every number is produced by the kernels in csrc/.

All functions require CUDA(HIP) fp32 tensors and raise otherwise -- there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from ._lib import Dims, NsdError, WsLayout, check

FC_HIDDEN = 32   # width of fc.0 in the reference (lstm_eeg_model.py:26)


@dataclass(frozen=True)
class ModelSpec:
    """Static shape of an EEG_LSTM (reference ctor kwargs, lstm_eeg_model.py:14)."""
    C: int = 8
    H: int = 48
    L: int = 2
    K: int = 3
    F: int = FC_HIDDEN
    D: int = 1          # directions: 2 = bidirectional (torch's nn.LSTM(bidirectional=True)); sequence-batched path only
    residual: bool = False   # sequence-batched path: the residual extension (NSD_FLAG_RESIDUAL) as part of the model's shape

    def dims(self, B: int, T: int) -> Dims:
        return Dims(B, T, self.C, self.H, self.L, self.K, self.F)

    @property
    def param_count(self) -> int:
        if self.D == 1:
            n = _lib.lib().nsd_param_count(self.C, self.H, self.L, self.K, self.F)
        else:
            n = _lib.lib().nsd_seq_param_count(self.C, self.H, self.L, self.K, self.F, self.D)
        if n < 0:
            raise NsdError(f"bad model dims {self}")
        return int(n)

    def names(self) -> List[str]:
        out = []
        for l in range(self.L):
            for sfx in (("",) if self.D == 1 else ("", "_reverse")):      # torch's state_dict order
                out += [f"lstm.weight_ih_l{l}{sfx}", f"lstm.weight_hh_l{l}{sfx}", f"lstm.bias_ih_l{l}{sfx}", f"lstm.bias_hh_l{l}{sfx}"]
        return out + ["ln.weight", "ln.bias", "attn.weight", "attn.bias",
                      "fc.0.weight", "fc.0.bias", "fc.3.weight", "fc.3.bias"]

    def shapes(self) -> Dict[str, Tuple[int, ...]]:
        s = {}
        DH = self.D * self.H
        for l in range(self.L):
            I = self.C if l == 0 else DH
            for sfx in (("",) if self.D == 1 else ("", "_reverse")):
                s[f"lstm.weight_ih_l{l}{sfx}"] = (4 * self.H, I)
                s[f"lstm.weight_hh_l{l}{sfx}"] = (4 * self.H, self.H)
                s[f"lstm.bias_ih_l{l}{sfx}"] = (4 * self.H,)
                s[f"lstm.bias_hh_l{l}{sfx}"] = (4 * self.H,)
        s.update({"ln.weight": (DH,), "ln.bias": (DH,), "attn.weight": (1, DH), "attn.bias": (1,),
                  "fc.0.weight": (self.F, DH), "fc.0.bias": (self.F,),
                  "fc.3.weight": (self.K, self.F), "fc.3.bias": (self.K,)})
        return s

    def offsets(self) -> Dict[str, int]:
        n = 4 * self.L * self.D + 8
        offs = (C.c_int64 * n)()
        if self.D == 1:
            _call("nsd_param_layout", None, self.C, self.H, self.L, self.K, self.F, offs)
        else:
            _call("nsd_seq_param_layout", None, self.C, self.H, self.L, self.K, self.F, self.D, offs)
        return dict(zip(self.names(), [int(o) for o in offs]))

    @property
    def seq_flags(self) -> int:
        return (_lib.NSD_FLAG_BIDIR if self.D == 2 else 0) | (_lib.NSD_FLAG_RESIDUAL if self.residual else 0) | _seq_extra_flags

    def seq_path(self, B: int = 32, T: int = 1) -> bool:
        """True where the sequence-batched bf16 path (nsd_seq_*) covers this model (H in 64/128/256/512, F, K <= 64)."""
        d = self.dims(B, T)
        return bool(_lib.lib().nsd_seq_supported(C.byref(d), self.seq_flags))

    def fast_path(self) -> bool:
        d = self.dims(1, 1)
        return bool(_lib.lib().nsd_fast_path(C.byref(d)))


def _dev_f32(t: Optional[torch.Tensor], name: str, shape=None) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise NsdError(f"{name}: expected a tensor on the MI355X (cuda/hip device), got device={t.device}; "
                       "the HIP path has no CPU fallback")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise NsdError(f"{name}: expected contiguous float32, got {t.dtype} contiguous={t.is_contiguous()}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise NsdError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t.data_ptr()


def _labels_ptr(labels: torch.Tensor) -> int:
    if labels.dtype != torch.int32 or not labels.is_cuda or not labels.is_contiguous():
        raise NsdError("labels must be a contiguous int32 tensor on the device")
    return labels.data_ptr()


# A step owns four consecutive streams of its seed, base_stream + slot (step_recipe.py numbers the steps): inter-layer dropout
# multipliers, RReLU slopes of the head, head dropout multipliers, and nsd_augment with nsd_mixup (index slots of their own inside it)
SLOT_LSTM_DROPOUT, SLOT_RRELU, SLOT_HEAD_DROPOUT, SLOT_AUGMENT = 0, 1, 2, 3


def _rng_struct(rng: dict, probs: bool = True) -> "_lib.Rng":
    """rng=dict(seed=, base_stream=, p_lstm=, p_head=) -> nsd_rng (step_recipe.step_rng builds the dict).  probs=False: the launch
    draws no dropout, the probabilities are not asked for and stay 0."""
    p = (float(rng["p_lstm"]), float(rng["p_head"])) if probs else (0.0, 0.0)
    return _lib.Rng(int(rng["seed"]) & 0xFFFFFFFFFFFFFFFF, int(rng["base_stream"]) & 0xFFFFFFFF, *p)


def _rng_array(rngs, M: int, what: str, probs: bool = True):
    """rngs: one rng dict or M of them -> nsd_rng[M] (None stays None)"""
    rngs = [rngs] if isinstance(rngs, dict) else rngs
    if rngs is not None and len(rngs) != M:
        raise NsdError(f"{what}: {len(rngs)} rng entries for {M} models")
    return None if rngs is None else (_lib.Rng * M)(*[_rng_struct(g, probs) for g in rngs])


def _per_model(v, M: int, what: str, key=lambda e: e):
    """A step setting given once or per model: a list / tuple of M entries -> (entry 0, None) where all are equal (the caller then takes
    its existing route, launch for launch) or (None, the list); anything else -> (v, None).  A wrong length raises."""
    if not isinstance(v, (list, tuple)):
        return v, None
    if len(v) != M:
        raise NsdError(f"{what}: {len(v)} entries for {M} models")
    v = list(v)
    return (v[0], None) if all(key(e) == key(v[0]) for e in v[1:]) else (None, v)


def _step_ptr(step_dev: Optional[torch.Tensor], what: str) -> Optional[int]:
    """The device step counter of the hipGraph-replayable entry points (stream ids / Adam's step are read from it on the device)."""
    if step_dev is not None and (step_dev.dtype != torch.int64 or not step_dev.is_cuda):
        raise NsdError(f"{what}: step_dev must be an int64 tensor on the device")
    return None if step_dev is None else step_dev.data_ptr()


def _model_windows(x: torch.Tensor, M: int, what: str, forms: str = "[B,T,C] or [M,B,T,C]"):
    """Model-batched windows x [B,T,C] (one model's, or shared by M models: stride 0) or [M,B,T,C] (M = 1 leaves the count to x)
    -> (M, B, T, C, x_model_stride, shape of the windows the models see).  what / forms: the caller's words for a refusal."""
    if x.dim() == 4:
        Mx, B, T, Cc = (int(v) for v in x.shape)
        if M not in (1, Mx):
            raise NsdError(f"{what}: x has {Mx} model slices, M = {M}")
        return Mx, B, T, Cc, B * T * Cc, (Mx, B, T, Cc)
    if x.dim() == 3:
        B, T, Cc = (int(v) for v in x.shape)
        return int(M), B, T, Cc, 0, ((B, T, Cc) if M == 1 else (int(M), B, T, Cc))
    raise NsdError(f"{what}: x must be {forms}, got {tuple(x.shape)}")


class _StreamOf:
    """Placeholder argument: replaced by the current HIP stream of the launch device inside _call's device guard."""


STREAM = _StreamOf()


_launch_hook = None


_extra_flags = 0
_seq_extra_flags = 0


def set_seq_diag_flags(l2_exchange: bool = True, spread_groups: bool = False, fused_layers: bool = True,
                       lose_member: bool = False) -> None:
    """Diagnostic build only (inside `with _lib.diagnostic_library():`; the product library rejects these bits):
    l2_exchange=False -> scan groups always use the write-through exchange; spread_groups=True -> every group is spread over all
    XCDs; fused_layers=False -> two unidirectional layers run as two scans + GEMMs instead of one skewed launch; lose_member=True
    -> every scan launch misses its last workgroup (that group must time out and report it)."""
    global _seq_extra_flags
    _seq_extra_flags = ((0 if l2_exchange else _lib.NSD_DIAG_FLAG_NO_L2_EXCHANGE) | (_lib.NSD_DIAG_FLAG_SPREAD_GROUPS if spread_groups else 0)
                        | (0 if fused_layers else _lib.NSD_DIAG_FLAG_NO_FUSED_LAYERS) | (_lib.NSD_DIAG_FLAG_LOSE_MEMBER if lose_member else 0))


def force_fwd48(nb: int) -> None:
    """Diagnostic build only (inside `with _lib.diagnostic_library():`): pin the H = 48 forward instantiation of the fp32 fast path
    to 1 / 2 / 4 trials per workgroup (4 = the matrix-pipe kernel where it applies), 8 = the experimental one-wave-per-layer kernel
    (unfused training launches only), 0 = the product's own choice.  Process-wide
    state of the DIAGNOSTIC library: reset it to 0 before leaving the block."""
    if not _lib.diag_active():
        raise NsdError("force_fwd48: the instantiation can be pinned in the diagnostic build only: use `with _lib.diagnostic_library():`")
    _lib.check(_lib.lib().nsd_diag_force_fwd48(int(nb)), "nsd_diag_force_fwd48")


def force_bwd48(nb: int) -> None:
    """Diagnostic build only: pin the H = 48 backward kernel -- 2 = the one- / two-trial kernel, 4 = the four-trial matrix-pipe kernel
    where it applies, 0 = the product's own choice.  Reset it to 0 before leaving the block."""
    if not _lib.diag_active():
        raise NsdError("force_bwd48: the kernel can be pinned in the diagnostic build only: use `with _lib.diagnostic_library():`")
    _lib.check(_lib.lib().nsd_diag_force_bwd48(int(nb)), "nsd_diag_force_bwd48")


def set_gemm_bf16(on: bool) -> None:
    """Large-H batched path only (NSD_FLAG_BF16): GEMM operands rounded to bf16 (fp32 accumulate / storage).  Off by default."""
    global _extra_flags
    _extra_flags = _lib.NSD_FLAG_BF16 if on else 0


def set_launch_hook(hook) -> None:
    """bench.py: hook(name) -> context manager entered around each C-ABI launch (HIP-event timing)."""
    global _launch_hook
    _launch_hook = hook


def _call(name: str, dev, *args) -> None:
    """Launch `name` on device `dev` (the device of the tensors whose pointers are in `args`): the C ABI enqueues on the
    CURRENT device, so the call is wrapped in a device guard and its stream is that device's current stream -- tensors
    on cuda:1 while cuda:0 is current would otherwise launch on the wrong GPU."""
    fn = getattr(_lib.lib(), name)
    if dev is None:                                   # host-only entry points (layouts, counts)
        check(fn(*args), name)
        return
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        args = tuple(st if a is STREAM else a for a in args)
        if _launch_hook is None:
            check(fn(*args), name)
        else:
            with _launch_hook(name):
                check(fn(*args), name)


def _nbytes(t: torch.Tensor) -> int:
    return int(t.numel()) * t.element_size()


def workspace_layout(spec: ModelSpec, B: int, T: int) -> Tuple[int, WsLayout]:
    d, w = spec.dims(B, T), WsLayout()
    n = _lib.lib().nsd_workspace_bytes(C.byref(d), C.byref(w))
    if n < 0:
        check(int(n), "nsd_workspace_bytes")
    return int(n), w


def new_workspace(spec: ModelSpec, B: int, T: int, device) -> torch.Tensor:
    nbytes, _ = workspace_layout(spec, B, T)
    return torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=device)


def ws_view(ws: torch.Tensor, spec: ModelSpec, B: int, T: int, region: str) -> torch.Tensor:
    """A shaped view of one workspace region (used by tests to inspect intermediates)."""
    _, w = workspace_layout(spec, B, T)
    H, L, F = spec.H, spec.L, spec.F
    shapes = {"hseq": (L, B, T, H), "cseq": (L, B, T, H), "gact": (L, B, T, H, 4), "inseq": (max(L - 1, 0), B, T, H),
              "top": (B, T, H), "alpha": (B, T), "pooled": (B, H), "fc0_pre": (B, F), "dscore": (B, T),
              "dpooled": (B, H), "loss": (B,), "adpack": (B, T, 4)}
    shp = shapes[region]
    n = 1
    for v in shp:
        n *= v
    off = getattr(w, region)
    return ws[off:off + n].view(shp)


ZSCORE_EPS = 1e-6


class _ZScoreFunction(torch.autograd.Function):
    """zscore as an autograd node (EEG_LSTM(normalize=True) with x.requires_grad): the forward is the kernel, the backward the
    closed form of y = d / (s + eps), d = x - mean_T x, s = sqrt(mean_T d^2) (population std) per trial and
    channel (app.py:166-170):  dL/dx = (g - mean_T g) / (s + eps) - d * sum_T(g d) / (T s (s + eps)^2)  (the second term is 0 where s = 0: d = 0 there)."""

    @staticmethod
    def forward(ctx, x: torch.Tensor) -> torch.Tensor:
        ctx.save_for_backward(x)
        return _zscore_launch(x, None)

    @staticmethod
    def backward(ctx, g: torch.Tensor) -> torch.Tensor:
        (x,) = ctx.saved_tensors
        x64, g64 = x.double(), g.double()
        T = x.shape[-2]
        d = x64 - x64.mean(dim=-2, keepdim=True)
        s = d.square().mean(dim=-2, keepdim=True).sqrt()
        se = s + ZSCORE_EPS
        gd = (g64 * d).sum(dim=-2, keepdim=True)
        corr = torch.where(s > 0, gd / (T * s.clamp_min(1e-300) * se * se), torch.zeros_like(s))
        return ((g64 - g64.mean(dim=-2, keepdim=True)) / se - d * corr).to(x.dtype)


def zscore(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(x - mean_T) / (std_T + 1e-6) per trial and channel; x [B,T,C] or [T,C].  (app.py:166-170)
    Differentiable w.r.t. x where autograd asks for it (no `out` then)."""
    if out is None and torch.is_grad_enabled() and x.requires_grad:
        return _ZScoreFunction.apply(x)
    return _zscore_launch(x, out)


def _zscore_launch(x: torch.Tensor, out: Optional[torch.Tensor]) -> torch.Tensor:
    squeeze = x.dim() == 2
    x3 = x.unsqueeze(0) if squeeze else x
    if x3.dim() != 3:
        raise ValueError(f"Expected [B,T,C] or [T,C], got {tuple(x.shape)}")
    x3 = x3.contiguous()
    y = torch.empty_like(x3) if out is None else out
    B, T, Cc = x3.shape
    _call("nsd_zscore_fwd", x3.device, _dev_f32(x3, "x"), _dev_f32(y, "y", x3.shape), B, T, Cc, STREAM)
    return y[0] if squeeze else y


@dataclass(frozen=True)
class Augment:
    """Trial augmentation of a training step (nsd_aug of include/nsd.h; an extension, the reference has none).  Each operation is OFF
    at 0.  max_shift: time shift of up to +-N steps per trial (edge sample repeated); scale_range r: one amplitude factor in
    [1 - r, 1 + r] per trial; p_channel: probability that a channel of a trial is zeroed; noise_std: additive unit-variance
    Irwin-Hall(4) noise times this, per element."""
    max_shift: int = 0
    scale_range: float = 0.0
    p_channel: float = 0.0
    noise_std: float = 0.0

    def __post_init__(self):
        if int(self.max_shift) != self.max_shift or self.max_shift < 0:
            raise ValueError(f"Augment: max_shift {self.max_shift!r} must be an integer >= 0")
        if not 0.0 <= self.scale_range < 1.0:
            raise ValueError(f"Augment: scale_range {self.scale_range!r} outside [0, 1)")
        if not 0.0 <= self.p_channel < 1.0:
            raise ValueError(f"Augment: p_channel {self.p_channel!r} outside [0, 1)")
        if not 0.0 <= self.noise_std < float("inf"):
            raise ValueError(f"Augment: noise_std {self.noise_std!r} negative or not finite")

    @property
    def enabled(self) -> bool:
        return bool(self.max_shift or self.scale_range or self.p_channel or self.noise_std)


def augment(x: torch.Tensor, aug, rngs, *, M: int = 1, zscore: bool = False, step_dev: Optional[torch.Tensor] = None,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nsd_augment: the augmented (and, with zscore, z-scored) windows, one launch for all models.
    x [B,T,C]: the windows of one model (M = 1 -> [B,T,C]) or shared by M models, each with its own draws (-> [M,B,T,C]);
    x [M,B,T,C]: per-model windows -> [M,B,T,C].  rngs: dict(seed=, base_stream=) or M of them (model m draws what a single-model call
    with rngs[m] draws; the stream used is base_stream + 3).  step_dev: device int64 step counter; base_stream is then
    4 * (step_dev[0] & 0x3fffffff) for every model (hipGraph replay).  All operations off: a bitwise copy of x.
    aug: one Augment, or a list of M (nsd_augment_each: model m is augmented with aug[m], an operation skipped where its parameter is 0;
    the z-score stays per launch).  A list of equal entries is the single Augment's launch."""
    M, B, T, Cc, stride, shape = _model_windows(x, M, "augment")
    r = _rng_array(rngs, M, "augment", probs=False)
    aug, augs = _per_model(aug, M, "augment")
    as_struct = lambda g: _lib.Aug(int(g.max_shift), float(g.scale_range), float(g.p_channel), float(g.noise_std))
    a = as_struct(aug) if augs is None else (_lib.Aug * M)(*[as_struct(g) for g in augs])
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    if out.numel() != M * B * T * Cc:
        raise NsdError(f"augment: out has {out.numel()} elements for {M} x {B} x {T} x {Cc}")
    d = Dims(B, T, Cc, 1, 1, 1, 1)
    _call("nsd_augment" if augs is None else "nsd_augment_each", x.device, C.byref(d), M, _dev_f32(x, "x"), stride, C.cast(C.pointer(a), C.c_void_p),
          C.cast(r, C.c_void_p), _step_ptr(step_dev, "augment"), _lib.NSD_AUG_ZSCORE if zscore else 0, _dev_f32(out, "out"), STREAM)
    return out


@dataclass(frozen=True)
class Loss:
    """The loss of a training step beyond mean cross-entropy on hard labels (nsd_mixup + the `_soft` entry points of include/nsd.h; an
    extension, the reference has none).  Each part is OFF at its default.  label_smoothing eps in [0, 1): the target of class k is
    (1 - eps) * onehot_k + eps / K; class_weights: K non-negative finite weights w_k multiplied into the target rows (what
    torch.nn.functional.cross_entropy(weight=w) puts in the numerator); mixup m in [0, 1]: every trial is mixed with a partner of its
    batch, window and target alike, lambda = 1 - m * U(0, 1) (m = 1: the uniform, Beta(1, 1), mixup); like the augmentation it is part
    of a trainer's stochastic steps only (stochastic=False mixes nothing).

    The step's scale stays 1 / global_batch: the loss is sum_b loss_b / B.  torch's weighted `mean` reduction divides by the sum of the
    trials' weights instead; with class weights the two differ by that (batch-dependent) factor."""
    label_smoothing: float = 0.0
    class_weights: Optional[Tuple[float, ...]] = None
    mixup: float = 0.0

    def __post_init__(self):
        if not 0.0 <= self.label_smoothing < 1.0:
            raise ValueError(f"Loss: label_smoothing {self.label_smoothing!r} outside [0, 1)")
        if not 0.0 <= self.mixup <= 1.0:
            raise ValueError(f"Loss: mixup {self.mixup!r} outside [0, 1]")
        if self.class_weights is not None:
            w = tuple(float(v) for v in self.class_weights)
            if len(w) < 1 or not all(0.0 <= v < float("inf") for v in w):
                raise ValueError(f"Loss: class_weights {self.class_weights!r} must be non-negative and finite, one per class")
            object.__setattr__(self, "class_weights", w)

    @property
    def enabled(self) -> bool:
        return bool(self.label_smoothing or self.mixup or self.class_weights is not None)

    def check_classes(self, K: int) -> None:
        if self.class_weights is not None and len(self.class_weights) != K:
            raise ValueError(f"Loss: {len(self.class_weights)} class_weights for a model of {K} classes")

    def weights_tensor(self, device) -> Optional[torch.Tensor]:
        return None if self.class_weights is None else torch.tensor(self.class_weights, dtype=torch.float32, device=device)


def mixup(x: Optional[torch.Tensor], labels: torch.Tensor, K: int, rngs, *, label_smoothing=0.0, mix=0.0,
          class_weights: Optional[torch.Tensor] = None, M: int = 1, step_dev: Optional[torch.Tensor] = None,
          out: Optional[torch.Tensor] = None, targets: Optional[torch.Tensor] = None
          ) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
    """nsd_mixup: the target rows of a step from its int32 labels (label smoothing, class weights) and, with mix > 0, the mixed windows,
    one launch for all models -> (y, targets [M*B, K]).  x [B,T,C] (one model, or shared by M models -> y [M,B,T,C]) or [M,B,T,C];
    x = None (mix = 0 only): the launch builds targets alone and y is None.  labels [M*B] int32 (model m's trial b at m * B + b).
    rngs / step_dev as ops.augment (the stream is base_stream + 3, on index slots nsd_augment does not use).  class_weights: device
    fp32 [K].  mix = 0 with x given: y is a bitwise copy of x.
    label_smoothing / mix: a float each, or a list of M each (nsd_mixup_each; a float beside a list is repeated), class_weights then
    [K], [M, K] or None; model m's rows and windows are those of the single-setting call with entry m.  Lists of equal entries with
    class_weights None or [K] are the single-setting launch.  With any mix[m] > 0, x is required."""
    if labels.dtype != torch.int32 or not labels.is_cuda or not labels.is_contiguous():
        raise NsdError("mixup: labels must be a contiguous int32 tensor on the device")
    dev = labels.device
    if x is None:
        M = int(M)
        if labels.numel() % M:
            raise NsdError(f"mixup: {labels.numel()} labels for {M} models")
        B, T, Cc, stride, shape = labels.numel() // M, 1, 1, 0, None
    else:
        M, B, T, Cc, stride, shape = _model_windows(x, M, "mixup")
    r = _rng_array(rngs, M, "mixup", probs=False)
    if labels.numel() != M * B:
        raise NsdError(f"mixup: {labels.numel()} labels for {M} x {B} trials")
    mix, mixes = _per_model(mix, M, "mixup: mix")
    label_smoothing, smooths = _per_model(label_smoothing, M, "mixup: label_smoothing")
    each = mixes is not None or smooths is not None or (class_weights is not None and class_weights.dim() == 2)
    if each:
        mixes = mixes if mixes is not None else [mix] * M
        smooths = smooths if smooths is not None else [label_smoothing] * M
        if class_weights is not None and class_weights.dim() == 1:
            class_weights = class_weights.unsqueeze(0).expand(M, K).contiguous()
        mx = (_lib.Mix * M)(*[_lib.Mix(float(a), float(e)) for a, e in zip(mixes, smooths)])
    else:
        mx = _lib.Mix(float(mix), float(label_smoothing))
    if targets is None:
        targets = torch.empty((M * B, K), dtype=torch.float32, device=dev)
    if targets.numel() != M * B * K:
        raise NsdError(f"mixup: targets has {targets.numel()} elements for {M * B} x {K}")
    if x is not None:
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=dev)
        if out.numel() != M * B * T * Cc:
            raise NsdError(f"mixup: out has {out.numel()} elements for {M} x {B} x {T} x {Cc}")
    else:
        out = None
    d = Dims(B, T, Cc, 1, 1, int(K), 1)
    _call("nsd_mixup_each" if each else "nsd_mixup", dev, C.byref(d), M, _dev_f32(x, "x"), stride, labels.data_ptr(),
          _dev_f32(class_weights, "class_weights", (M, K) if each else (K,)), C.cast(C.pointer(mx), C.c_void_p), C.cast(r, C.c_void_p), _step_ptr(step_dev, "mixup"), _dev_f32(out, "out"), _dev_f32(targets, "targets"), STREAM)
    return out, targets


def target_rows(labels: torch.Tensor, K: int, M: int = 1, loss: Optional[Loss] = None) -> torch.Tensor:
    """The target rows [M*B, K] of int32 labels [M*B] with nothing mixed (the nsd_mixup launch at mix = 0, which draws nothing): one-hot
    rows, or `loss`'s label smoothing and class weights -- what nsd_head_fit takes in place of labels."""
    loss = loss or Loss()
    rngs = [dict(seed=0, base_stream=0, p_lstm=0.0, p_head=0.0)] * int(M)
    return mixup(None, labels, K, rngs, label_smoothing=loss.label_smoothing, mix=0.0, class_weights=loss.weights_tensor(labels.device),
                 M=int(M))[1]


@dataclass(frozen=True)
class Crop:
    """Cropped training (nsd_crop_cfg of include/nsd.h; an extension, the reference trains on whole trials): every trial of a step is
    shown to the model as `crops` windows of `window` samples.  hop = 0: the offsets are drawn per trial, crop and step (part of a
    trainer's stochastic steps); hop > 0: the regular grid 0, hop, 2 hop, ... -- the windows a sliding decoder with (window, hop)
    decides on the trial, which is how a cropped model is scored (ModelBatchTrainer.evaluate(crop=)) and served."""
    window: int
    crops: int = 1
    hop: int = 0

    def __post_init__(self):
        for name in ("window", "crops", "hop"):
            v = getattr(self, name)
            if isinstance(v, bool) or int(v) != v:
                raise ValueError(f"Crop: {name} {v!r} must be an integer")
        if self.window < 1:
            raise ValueError(f"Crop: window {self.window!r} must be >= 1")
        if not 1 <= self.crops <= _lib.NSD_CROP_MAX:
            raise ValueError(f"Crop: crops {self.crops!r} outside [1, {_lib.NSD_CROP_MAX}]")
        if self.hop < 0:
            raise ValueError(f"Crop: hop {self.hop!r} negative (0: drawn offsets)")

    @property
    def span(self) -> int:
        """samples of a trial a regular grid covers (the window itself with drawn offsets)"""
        return (self.crops - 1) * self.hop + self.window

    def check_trial(self, T: int) -> None:
        if self.window > T or (self.hop > 0 and self.span > T):
            raise NsdError(f"{self}: trials of {T} samples are too short (window <= T, and for a regular grid (crops - 1) * hop + window <= T)")

    @staticmethod
    def grid(T: int, window: int, hop: int) -> "Crop":
        """The regular grid of every whole window of a trial of T samples: the decisions of a sliding decoder with (window, hop)."""
        if window > T or hop < 1:
            raise ValueError(f"Crop.grid: window {window} / hop {hop} for trials of {T} samples")
        return Crop(window, (T - window) // hop + 1, hop)


def crop(x: torch.Tensor, cfg: Crop, rngs=None, *, M: int = 1, labels: Optional[torch.Tensor] = None, targets: Optional[torch.Tensor] = None,
         step_dev: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, labels_out: Optional[torch.Tensor] = None,
         targets_out: Optional[torch.Tensor] = None, offsets: Optional[torch.Tensor] = None):
    """nsd_crop: cfg.crops windows of cfg.window samples from every trial, one launch for all models -> (y, labels_out, targets_out).
    x [B,T,C] (one model -> y [B*R,W,C], or shared by M models, each with its own offsets -> [M,B*R,W,C]) or [M,B,T,C]; row b * R + r
    is crop r of trial b.  labels int32 [M*B] / targets fp32 [M*B,K]: each trial's entry repeated for its crops ([M*B*R] / [M*B*R,K];
    None stays None).  rngs / step_dev as ops.augment (the stream is base_stream + 3, on index slots of its own); a regular grid
    (cfg.hop > 0) draws nothing and needs no rngs.  offsets: an int32 [M*B*R] tensor that receives the offsets."""
    M, B, T, Cc, stride, _ = _model_windows(x, M, "crop")
    R, W = int(cfg.crops), int(cfg.window)
    dev = x.device
    r = _rng_array(rngs, M, "crop", probs=False)
    rows = M * B * R
    if out is None:
        out = torch.empty((B * R, W, Cc) if (M == 1 and x.dim() == 3) else (M, B * R, W, Cc), dtype=torch.float32, device=dev)
    if out.numel() != rows * W * Cc:
        raise NsdError(f"crop: out has {out.numel()} elements for {rows} x {W} x {Cc}")
    K = 1
    if labels is not None:
        if labels.dtype != torch.int32 or not labels.is_cuda or not labels.is_contiguous() or labels.numel() != M * B:
            raise NsdError(f"crop: labels must be a contiguous int32 device tensor of {M} x {B} entries")
        if labels_out is None:
            labels_out = torch.empty((rows,), dtype=torch.int32, device=dev)
        if labels_out.dtype != torch.int32 or not labels_out.is_contiguous() or labels_out.numel() != rows:
            raise NsdError(f"crop: labels_out must be a contiguous int32 tensor of {rows} entries")
    else:
        labels_out = None
    if targets is not None:
        if targets.dim() != 2 or targets.shape[0] != M * B:
            raise NsdError(f"crop: targets must be [M*B, K] = [{M * B}, K], got {tuple(targets.shape)}")
        K = int(targets.shape[1])
        if targets_out is None:
            targets_out = torch.empty((rows, K), dtype=torch.float32, device=dev)
        if targets_out.numel() != rows * K:
            raise NsdError(f"crop: targets_out has {targets_out.numel()} elements for {rows} x {K}")
    else:
        targets_out = None
    if offsets is not None and (offsets.dtype != torch.int32 or not offsets.is_cuda or not offsets.is_contiguous() or offsets.numel() != rows):
        raise NsdError(f"crop: offsets must be a contiguous int32 device tensor of {rows} entries")
    d = Dims(B, T, Cc, 1, 1, K, 1)
    c = _lib.CropCfg(W, R, int(cfg.hop))
    _call("nsd_crop", dev, C.byref(d), M, _dev_f32(x, "x"), stride, C.byref(c), C.cast(r, C.c_void_p) if r is not None else None,
          _step_ptr(step_dev, "crop"), None if labels is None else labels.data_ptr(), _dev_f32(targets, "targets"), _dev_f32(out, "out"),
          None if labels_out is None else labels_out.data_ptr(), _dev_f32(targets_out, "targets_out"),
          None if offsets is None else offsets.data_ptr(), STREAM)
    return out, labels_out, targets_out


def crop_pool(probs: torch.Tensor, counts: Optional[torch.Tensor] = None, *, out: Optional[torch.Tensor] = None,
              logits: Optional[torch.Tensor] = None, want_logits: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """nsd_crop_pool: probs [N,R,K] (the class probabilities of each trial's R windows; nsd_window_step's [B,D,K]) -> (pooled
    probabilities [N,K], their logarithms [N,K] or None).  counts: None, or int32 [N] on the device -- only trial n's first counts[n]
    windows count (nsd_window_step's counts).  The mean is the serial fp32 sum in ascending window order over the count; a bad count
    or a non-finite probability among the counted rows gives a NaN row."""
    if probs.dim() != 3:
        raise NsdError(f"crop_pool: probs must be [N,R,K], got {tuple(probs.shape)}")
    N, R, K = (int(v) for v in probs.shape)
    dev = probs.device
    if counts is not None and (counts.dtype != torch.int32 or not counts.is_cuda or not counts.is_contiguous() or counts.numel() != N):
        raise NsdError(f"crop_pool: counts must be a contiguous int32 device tensor of {N} entries")
    out = _out_f32(out, (N, K), dev, "crop_pool: out")
    if logits is None and want_logits:
        logits = torch.empty((N, K), dtype=torch.float32, device=dev)
    _call("nsd_crop_pool", dev, N, R, K, _dev_f32(probs, "probs"), None if counts is None else counts.data_ptr(), _dev_f32(out, "out"),
          _dev_f32(logits, "logits", (N, K)), STREAM)
    return out, logits


def gather_path(B: int, T: int, Cc: int, M: int, N: int, S: int) -> bool:
    """nsd_gather_path: do the shape checks of nsd_gather pass (no device needed)"""
    d = Dims(int(B), int(T), int(Cc), 1, 1, 1, 1)
    return bool(_lib.lib().nsd_gather_path(C.byref(d), int(M), int(N), int(S)))


def _int32_dev(t: Optional[torch.Tensor], n: Optional[int], name: str) -> Optional[int]:
    if t is None:
        return None
    if t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous() or (n is not None and t.numel() != n):
        raise NsdError(f"gather_batch: {name} must be a contiguous int32 device tensor" + ("" if n is None else f" of {n} entries"))
    return t.data_ptr()


def gather_batch(x_all: torch.Tensor, table: torch.Tensor, *, step: int = 0, step_base: int = 0, step_dev: Optional[torch.Tensor] = None,
                 labels_all: Optional[torch.Tensor] = None, targets_all: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                 labels_out: Optional[torch.Tensor] = None, targets_out: Optional[torch.Tensor] = None,
                 status: Optional[torch.Tensor] = None):
    """nsd_gather: the batch of one step for all models of `table`, one launch -> (x, labels, targets).
    x_all [N,T,C] fp32: the resident trials; table int32 [M,S,B] (or [S,B]: one model): row r = (c - step_base) mod S holds each
    model's B trial indices, c = step_dev[0] as the kernel reads it (an int64 device counter: hipGraph replay) or `step`.
    x [M,B,T,C] ([B,T,C] for an [S,B] table) is the bitwise copy of the named trials; labels_all int32 [N] -> labels [M*B];
    targets_all fp32 [N,K] -> targets [M*B,K] (None stays None).  out / labels_out / targets_out: the buffers to fill (a static step's).
    status: int32 [M] on the device, zeroed by the caller: bit 0 is set for a model with an index outside [0, N); such a row is NaN
    with label 0."""
    if x_all.dim() != 3:
        raise NsdError(f"gather_batch: x_all must be [N,T,C], got {tuple(x_all.shape)}")
    if table.dim() not in (2, 3):
        raise NsdError(f"gather_batch: table must be int32 [M,S,B] or [S,B], got {tuple(table.shape)}")
    N, T, Cc = (int(v) for v in x_all.shape)
    S, B = int(table.shape[-2]), int(table.shape[-1])
    M = int(table.shape[0]) if table.dim() == 3 else 1
    dev = x_all.device
    tp = _int32_dev(table, None, "table")
    if out is None:
        out = torch.empty((M, B, T, Cc) if table.dim() == 3 else (B, T, Cc), dtype=torch.float32, device=dev)
    if out.numel() != M * B * T * Cc:
        raise NsdError(f"gather_batch: out has {out.numel()} elements for {M} x {B} x {T} x {Cc}")
    K = 1
    if labels_all is not None:
        if labels_out is None:
            labels_out = torch.empty((M * B,), dtype=torch.int32, device=dev)
        lp, lop = _int32_dev(labels_all, N, "labels_all"), _int32_dev(labels_out, M * B, "labels_out")
    else:
        labels_out, lp, lop = None, None, None
    if targets_all is not None:
        if targets_all.dim() != 2 or targets_all.shape[0] != N:
            raise NsdError(f"gather_batch: targets_all must be [N, K] = [{N}, K], got {tuple(targets_all.shape)}")
        K = int(targets_all.shape[1])
        if targets_out is None:
            targets_out = torch.empty((M * B, K), dtype=torch.float32, device=dev)
        if targets_out.numel() != M * B * K:
            raise NsdError(f"gather_batch: targets_out has {targets_out.numel()} elements for {M * B} x {K}")
    else:
        targets_out = None
    if B == 0:                           # nothing to launch (and an empty tensor has no address to hand over)
        return out, labels_out, targets_out
    d = Dims(B, T, Cc, 1, 1, K, 1)
    _call("nsd_gather", dev, C.byref(d), M, N, _dev_f32(x_all, "x_all"), lp, _dev_f32(targets_all, "targets_all"), tp, S, int(step),
          _step_ptr(step_dev, "gather_batch"), int(step_base), _dev_f32(out, "out"), lop, _dev_f32(targets_out, "targets_out"),
          _int32_dev(status, M, "status"), STREAM)
    return out, labels_out, targets_out


@dataclass(frozen=True)
class LrSchedule:
    """Learning-rate schedule of a trainer (the schedule fields of nsd_opt, include/nsd.h; an extension, the reference has none):
    lr_eff(s) = lr * f(s), s the 1-based step.  warmup_steps W: f = s / W for s <= W, then `kind` on e' = s - 1 - W: "constant" f = 1;
    "cosine" f = r + (1 - r) (1 + cos(pi min(e', N') / N')) / 2 with N' = total_steps - W and r = min_ratio (torch's CosineAnnealingLR
    closed form, held at r past N'); "step" f = gamma ^ floor(e' / step_size) (torch's StepLR).  The factor is a function of the step
    alone, evaluated by the update kernel -- from the device step counter under hipGraph replay."""
    kind: str = "constant"
    warmup_steps: int = 0
    total_steps: int = 0
    min_ratio: float = 0.0
    step_size: int = 1
    gamma: float = 1.0

    def __post_init__(self):
        if self.kind not in _lib.NSD_SCHED:
            raise ValueError(f"LrSchedule: kind {self.kind!r} is not one of {sorted(_lib.NSD_SCHED)}")
        for name in ("warmup_steps", "total_steps", "step_size"):
            v = getattr(self, name)
            if int(v) != v or not -2 ** 31 <= v < 2 ** 31:
                raise ValueError(f"LrSchedule: {name} {v!r} must be an int32")
        if self.warmup_steps < 0:
            raise ValueError(f"LrSchedule: warmup_steps {self.warmup_steps!r} negative")
        if self.kind == "cosine" and self.total_steps <= self.warmup_steps:
            raise ValueError(f"LrSchedule: cosine needs total_steps {self.total_steps!r} > warmup_steps {self.warmup_steps!r}")
        if self.step_size < 1:
            raise ValueError(f"LrSchedule: step_size {self.step_size!r} must be >= 1")
        if not 0.0 < self.gamma <= 1.0:
            raise ValueError(f"LrSchedule: gamma {self.gamma!r} outside (0, 1]")
        if not 0.0 <= self.min_ratio <= 1.0:
            raise ValueError(f"LrSchedule: min_ratio {self.min_ratio!r} outside [0, 1]")


def opt_struct(*, lr: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 0.0,
               grad_scale: float = 1.0, max_norm: Optional[float] = None, schedule: Optional[LrSchedule] = None) -> "_lib.Opt":
    """nsd_opt from Adam's hyper-parameters, a clip threshold (None or 0: report the norm and guard, do not clip) and a schedule."""
    sc = schedule if schedule is not None else LrSchedule()
    return _lib.Opt(lr, beta1, beta2, eps, weight_decay, grad_scale, 0.0 if max_norm is None else float(max_norm),
                    _lib.NSD_SCHED[sc.kind], int(sc.warmup_steps), int(sc.total_steps), int(sc.step_size), float(sc.min_ratio), float(sc.gamma))


def lr_factor(opt: "_lib.Opt", step: int) -> float:
    """f(step) of opt's schedule, on the host (nsd_lr_factor)."""
    f = float(_lib.lib().nsd_lr_factor(C.byref(opt), int(step)))
    if f < 0:
        check(-1, "nsd_lr_factor")
    return f


def opt_state_bytes(n: int, M: int = 1) -> int:
    nb = int(_lib.lib().nsd_opt_state_bytes(int(n), int(M)))
    if nb < 0:
        check(nb, "nsd_opt_state_bytes")
    return nb


def opt_state(n: int, M: int, device) -> torch.Tensor:
    """The opt_state of the clipped tail for M models of n parameters (or a flat vector of n, M = 1): records zeroed."""
    st = torch.empty(opt_state_bytes(n, M), dtype=torch.uint8, device=device)
    _call("nsd_opt_state_init", st.device, st.data_ptr(), _nbytes(st), STREAM)
    return st


def opt_records(state: torch.Tensor, M: int = 1) -> List[dict]:
    """The M records at the head of an opt_state: [{norm, coef, lr, skipped}] (synchronises)."""
    raw = state[:16 * M].cpu()
    f, u = raw.view(torch.float32).view(M, 4), raw.view(torch.int32).view(M, 4)
    return [dict(norm=float(f[i, 0]), coef=float(f[i, 1]), lr=float(f[i, 2]), skipped=int(u[i, 3]) & 0xFFFFFFFF) for i in range(M)]


def grad_norm(g: torch.Tensor, state: torch.Tensor, grad_scale: float = 1.0) -> None:
    """Flat route, launch 1 (nsd_grad_norm): the partial sums of (g * grad_scale)^2 -> state's scratch, for adam_step_clip."""
    _call("nsd_grad_norm", g.device, g.numel(), _dev_f32(g, "g"), grad_scale, state.data_ptr(), _nbytes(state), STREAM)


def adam_step_clip(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, opt: "_lib.Opt", state: torch.Tensor, *,
                   step: int = 0, step_dev: Optional[torch.Tensor] = None, skip: Optional[torch.Tensor] = None) -> None:
    """Flat route, launch 2 (nsd_adam_step_clip): the clipped / scheduled Adam update from the norm grad_norm(g, state, opt.grad_scale)
    left.  step_dev: the device step counter read in place of `step`; skip: the device flag of the guarded update."""
    _call("nsd_adam_step_clip", p.device, p.numel(), _dev_f32(p, "p"), _dev_f32(g, "g", p.shape), _dev_f32(m, "m", p.shape),
          _dev_f32(v, "v", p.shape), C.byref(opt), int(step), _step_ptr(step_dev, "adam_step_clip"), _dev_f32(skip, "skip"),
          state.data_ptr(), _nbytes(state), STREAM)


@dataclass(frozen=True)
class Average:
    """Weight averaging of a trainer (nsd_avg, include/nsd.h; an extension, the reference has none): the update launch also keeps an
    averaged copy of the parameters.  kind "ema": a' = a + (1 - decay) (p' - a); "swa": the equal-weight running mean a' = a + (p' - a) /
    (n + 1) of the averaged iterates (torch.optim.swa_utils.AveragedModel's default; decay is ignored).  Steps before start_step
    (1-based), steps off the stride `every` and skipped updates do not average; the first averaged step copies the parameters."""
    kind: str = "ema"
    decay: float = 0.999
    start_step: int = 1
    every: int = 1

    def __post_init__(self):
        if self.kind not in _lib.NSD_AVG:
            raise ValueError(f"Average: kind {self.kind!r} is not one of {sorted(_lib.NSD_AVG)}")
        if self.kind == "ema" and not 0.0 <= self.decay < 1.0:
            raise ValueError(f"Average: decay {self.decay!r} outside [0, 1)")
        for name in ("start_step", "every"):
            v = getattr(self, name)
            if int(v) != v or not 1 <= v < 2 ** 31:
                raise ValueError(f"Average: {name} {v!r} must be an int32 >= 1")

    def struct(self) -> "_lib.Avg":
        return _lib.Avg(_lib.NSD_AVG[self.kind], float(self.decay), int(self.start_step), int(self.every))


def _avg_struct(a) -> "_lib.Avg":
    """nsd_avg of an Average, of None (mode 0: this model does not average, `_each` only) or of a ready _lib.Avg"""
    return a if isinstance(a, _lib.Avg) else _lib.Avg(0, 0.0, 1, 1) if a is None else a.struct()


def avg_state_bytes(n: int, M: int = 1) -> int:
    nb = int(_lib.lib().nsd_avg_state_bytes(int(n), int(M)))
    if nb < 0:
        check(nb, "nsd_avg_state_bytes")
    return nb


def avg_state(n: int, M: int, device) -> torch.Tensor:
    """The avg_state of weight averaging for M models of n parameters (or a flat vector of n, M = 1): records zeroed, rows zero too
    (the kernels ask nothing of the rows before a model's first averaged step)."""
    st = torch.zeros(avg_state_bytes(n, M), dtype=torch.uint8, device=device)
    _call("nsd_avg_state_init", st.device, st.data_ptr(), _nbytes(st), int(M), STREAM)
    return st


def avg_rows(state: torch.Tensor, M: int, n: int) -> torch.Tensor:
    """The averaged rows of an avg_state as an [M, n] fp32 view (no copy: it follows later steps)."""
    return state[16 * M:16 * M + 4 * M * n].view(torch.float32).view(M, n)


def avg_records(state: torch.Tensor, M: int = 1) -> List[dict]:
    """The M records at the head of an avg_state: [{n_avg, arrive}] (synchronises)."""
    u = state[:16 * M].cpu().view(torch.int32).view(M, 4)
    return [dict(n_avg=int(u[i, 0]) & 0xFFFFFFFF, arrive=int(u[i, 1]) & 0xFFFFFFFF) for i in range(M)]


def _avg_args(avg, avg_state_: torch.Tensor):
    return C.byref(avg), avg_state_.data_ptr(), _nbytes(avg_state_)


def adam_step_clip_avg(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, opt: "_lib.Opt", state: torch.Tensor,
                       avg, avg_state: torch.Tensor, *, step: int = 0, step_dev: Optional[torch.Tensor] = None,
                       skip: Optional[torch.Tensor] = None) -> None:
    """adam_step_clip that also forms the weight average in the same launch (nsd_adam_step_clip_avg): avg an ops.Average, avg_state
    ops.avg_state(p.numel(), 1)."""
    _call("nsd_adam_step_clip_avg", p.device, p.numel(), _dev_f32(p, "p"), _dev_f32(g, "g", p.shape), _dev_f32(m, "m", p.shape),
          _dev_f32(v, "v", p.shape), C.byref(opt), int(step), _step_ptr(step_dev, "adam_step_clip_avg"), _dev_f32(skip, "skip"),
          state.data_ptr(), _nbytes(state), STREAM, *_avg_args(_avg_struct(avg), avg_state))


@dataclass(frozen=True)
class Sam:
    """Sharpness-aware minimisation of a trainer (nsd_sam, include/nsd.h; Foret et al. 2021; an extension, the reference has none): a
    step takes its gradient at the parameters moved a distance rho uphill along the normalised gradient, p + rho g / (|g| + 1e-12),
    and updates the real parameters with it: two forward/backward passes on the same batch with the same random draws, the ascent
    between them, then the step's usual tail.  rho = 0 keeps the two passes and perturbs nothing."""
    rho: float = 0.05

    def __post_init__(self):
        if not (isinstance(self.rho, (int, float)) and 0.0 <= self.rho < float("inf")):
            raise ValueError(f"Sam: rho {self.rho!r} must be a finite number >= 0")

    def struct(self) -> "_lib.Sam":
        return _lib.Sam(float(self.rho))


def _sam_struct(s) -> "_lib.Sam":
    """nsd_sam of a Sam, of None (rho 0: this model's row is a copy of its parameters, `each` only) or of a ready _lib.Sam"""
    return s if isinstance(s, _lib.Sam) else _lib.Sam(0.0) if s is None else s.struct()


def sam_state_bytes(n: int, M: int = 1) -> int:
    nb = int(_lib.lib().nsd_sam_state_bytes(int(n), int(M)))
    if nb < 0:
        check(nb, "nsd_sam_state_bytes")
    return nb


def sam_state(n: int, M: int, device) -> torch.Tensor:
    """The sam_state of the ascent for M models of n parameters (or a flat vector of n, M = 1): zeroed."""
    st = torch.empty(sam_state_bytes(n, M), dtype=torch.uint8, device=device)
    _call("nsd_sam_state_init", st.device, st.data_ptr(), _nbytes(st), STREAM)
    return st


def sam_rows(state: torch.Tensor, M: int, n: int) -> torch.Tensor:
    """The perturbed rows p_adv of a sam_state as an [M, n] fp32 view (no copy: pass 2 reads its parameters here)."""
    return state[16 * M:16 * M + 4 * M * n].view(torch.float32).view(M, n)


def sam_records(state: torch.Tensor, M: int = 1) -> List[dict]:
    """The M records at the head of a sam_state: [{norm, scale, nonfinite}] (synchronises)."""
    raw = state[:16 * M].cpu()
    f, u = raw.view(torch.float32).view(M, 4), raw.view(torch.int32).view(M, 4)
    return [dict(norm=float(f[i, 0]), scale=float(f[i, 1]), nonfinite=int(u[i, 2]) & 0xFFFFFFFF) for i in range(M)]


def sam_ascend(spec: ModelSpec, ws: torch.Tensor, B: int, T: int, grads: torch.Tensor, p: torch.Tensor, sam, opt_state: torch.Tensor,
               sam_state: torch.Tensor, *, grad_scale: float = 1.0) -> None:
    """The ascent of one model from the slabs a forward/backward left in ws (nsd_sam_ascend): grads as nsd_grad_reduce leaves it, the
    perturbed row in sam_state (sam_rows).  opt_state: the tail's (ops.opt_state(P, 1)), whose scratch carries the partial sums."""
    d = spec.dims(B, T)
    P = spec.param_count
    _call("nsd_sam_ascend", p.device, C.byref(d), _dev_f32(ws, "workspace"), _nbytes(ws), _dev_f32(grads, "grads", (P,)), _dev_f32(p, "p", (P,)),
          C.byref(_sam_struct(sam)), float(grad_scale), opt_state.data_ptr(), _nbytes(opt_state), sam_state.data_ptr(), _nbytes(sam_state), STREAM)


def multi_sam_ascend(spec: ModelSpec, ws: torch.Tensor, B: int, T: int, grads: torch.Tensor, params: torch.Tensor, sam,
                     opt_state: torch.Tensor, sam_state: torch.Tensor, *, grad_scale=1.0) -> None:
    """The ascent of M models in the same two launches (nsd_multi_sam_ascend): params / grads [M,P].  sam: a Sam for all models, or a
    list of M with None for a model that is not perturbed; grad_scale: a float, or a list of M.  Lists of equal entries issue the
    single setting's call."""
    M, P = int(params.shape[0]), spec.param_count
    d = spec.dims(B, T)
    sam, sams = _per_model(sam, M, "multi: sam")
    gs, gss = _per_model(grad_scale, M, "multi: grad_scale")
    each = sams is not None or gss is not None
    n = M if each else 1
    arr = (_lib.Sam * n)(*[_sam_struct(s) for s in (sams if sams is not None else [sam] * n)])
    garr = (C.c_float * n)(*[float(g) for g in (gss if gss is not None else [gs] * n)])
    _call("nsd_multi_sam_ascend", params.device, C.byref(d), M, ws.data_ptr(), _nbytes(ws), _dev_f32(grads, "grads", (M, P)),
          _dev_f32(params, "params", (M, P)), C.cast(arr, C.c_void_p), 1 if each else 0, C.cast(garr, C.c_void_p), opt_state.data_ptr(),
          _nbytes(opt_state), sam_state.data_ptr(), _nbytes(sam_state), STREAM)


def sam_ascend_flat(p: torch.Tensor, g: torch.Tensor, sam, opt_state: torch.Tensor, sam_state: torch.Tensor, *, grad_scale: float = 1.0) -> None:
    """The ascent from a flat gradient (nsd_sam_ascend_flat): world > 1 after nsd_grad_reduce, the bf16 sequence path after its backward."""
    _call("nsd_sam_ascend_flat", p.device, p.numel(), _dev_f32(p, "p"), _dev_f32(g, "g", p.shape), C.byref(_sam_struct(sam)), float(grad_scale),
          opt_state.data_ptr(), _nbytes(opt_state), sam_state.data_ptr(), _nbytes(sam_state), STREAM)


def _out_f32(out: Optional[torch.Tensor], shape, device, what: str) -> torch.Tensor:
    """The caller's output buffer (element count checked; dtype, device and contiguity by _dev_f32 at the launch), or a fresh one"""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    n = 1
    for v in shape:
        n *= int(v)
    if out.numel() != n:
        raise NsdError(f"{what}: the output buffer has {out.numel()} elements for {tuple(shape)}")
    return out


def _scratch_ptr(scratch: Optional[torch.Tensor], nbytes: int, device, what: str):
    """(tensor kept alive, device pointer) of an inference scratch: the caller's (at least nbytes long) or a fresh one"""
    if scratch is None:
        scratch = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=device)
    elif not scratch.is_cuda or not scratch.is_contiguous() or _nbytes(scratch) < nbytes:
        raise NsdError(f"{what}: scratch must be a contiguous device buffer of at least {nbytes} bytes")
    return scratch, scratch.data_ptr()


def infer(spec: ModelSpec, flat: torch.Tensor, x: torch.Tensor, *, residual: bool = False, want_probs: bool = True,
          logits: Optional[torch.Tensor] = None, probs: Optional[torch.Tensor] = None,
          scratch: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Eval-mode forward: logits [B,K] (+ softmax probabilities).  logits / probs / scratch: optional caller-owned buffers (scratch: at
    least nsd_infer_scratch_bytes long, any dtype)."""
    B, T, Cc = x.shape
    if Cc != spec.C:
        raise NsdError(f"x has {Cc} channels, model expects {spec.C}")
    d = spec.dims(B, T)
    logits = _out_f32(logits, (B, spec.K), x.device, "infer: logits")
    probs = _out_f32(probs, (B, spec.K), x.device, "infer: probs") if want_probs else None
    if B == 0:                      # empty batch: nothing to launch (empty tensors have no device pointer)
        _dev_f32(flat, "params", (spec.param_count,)); _dev_f32(x, "x")
        return logits, probs
    nscr = _lib.lib().nsd_infer_scratch_bytes(C.byref(d))
    scratch, scrp = _scratch_ptr(scratch, int(nscr), x.device, "infer")
    _call("nsd_infer", x.device, C.byref(d), _dev_f32(flat, "params", (spec.param_count,)), _dev_f32(x, "x"),
          (_lib.NSD_FLAG_RESIDUAL if residual else 0) | _extra_flags, _dev_f32(logits, "logits"),
          _dev_f32(probs, "probs"), scrp, STREAM)
    return logits, probs


def train_forward(spec: ModelSpec, flat: torch.Tensor, x: torch.Tensor, ws: torch.Tensor, *,
                  drop_lstm: Optional[torch.Tensor] = None, rrelu_slope: Optional[torch.Tensor] = None,
                  drop_head: Optional[torch.Tensor] = None, residual: bool = False,
                  want_probs: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Train-mode forward keeping activations in `ws` (from new_workspace)."""
    B, T, Cc = x.shape
    d = spec.dims(B, T)
    flags = _lib.NSD_FLAG_TRAIN | (_lib.NSD_FLAG_RESIDUAL if residual else 0) | _extra_flags
    pp = _dev_f32(flat, "params", (spec.param_count,))
    _call("nsd_lstm_fwd", x.device, C.byref(d), pp, _dev_f32(x, "x", (B, T, spec.C)),
          _dev_f32(drop_lstm, "drop_lstm", (spec.L - 1, B, T, spec.H)), flags, _dev_f32(ws, "workspace"), _nbytes(ws), STREAM)
    logits = torch.empty((B, spec.K), dtype=torch.float32, device=x.device)
    probs = torch.empty_like(logits) if want_probs else None
    _call("nsd_head_fwd", x.device, C.byref(d), pp, _dev_f32(rrelu_slope, "rrelu_slope", (B, spec.F)),
          _dev_f32(drop_head, "drop_head", (B, spec.F)), ws.data_ptr(), _nbytes(ws), logits.data_ptr(),
          _dev_f32(probs, "probs"), STREAM)
    return logits, probs


def train_backward(spec: ModelSpec, flat: torch.Tensor, x: torch.Tensor, ws: torch.Tensor, logits: torch.Tensor, *,
                   dlogits: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
                   scale: Optional[float] = None, drop_lstm=None, rrelu_slope=None, drop_head=None,
                   residual: bool = False, grads: Optional[torch.Tensor] = None,
                   accumulate: bool = False, dx: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Backward through head + LSTM; returns the flat gradient vector (same layout as the parameters).
    Give either dlogits [B,K], or int32 labels [B] (+ scale, default 1/B) for fused mean cross-entropy.
    `dx` [B,T,C] (optional output): the gradient w.r.t. the EEG window (H = 48 and the generic path; it consumes layer 0's saved gates
    on the H = 48 path: no second backward on the same forward then)."""
    B, T, _ = x.shape
    d = spec.dims(B, T)
    pp = _dev_f32(flat, "params", (spec.param_count,))
    if dlogits is None:
        if labels is None:
            raise NsdError("train_backward needs dlogits or labels")
        lab_ptr = _labels_ptr(labels)
    else:
        lab_ptr = None
    scale = (1.0 / max(B, 1)) if scale is None else float(scale)
    flags = _lib.NSD_FLAG_TRAIN | (_lib.NSD_FLAG_RESIDUAL if residual else 0) | _extra_flags
    wsp, wsn = _dev_f32(ws, "workspace"), _nbytes(ws)
    _call("nsd_head_bwd", x.device, C.byref(d), pp, _dev_f32(rrelu_slope, "rrelu_slope"), _dev_f32(drop_head, "drop_head"),
          _dev_f32(logits, "logits", (B, spec.K)), _dev_f32(dlogits, "dlogits", (B, spec.K)), lab_ptr, scale, wsp, wsn, STREAM)
    _call("nsd_lstm_bwd", x.device, C.byref(d), pp, _dev_f32(x, "x"), _dev_f32(drop_lstm, "drop_lstm"), flags, wsp, wsn,
          _dev_f32(dx, "dx", tuple(x.shape)) if dx is not None else None, STREAM)
    if grads is None:
        grads = torch.empty(spec.param_count, dtype=torch.float32, device=x.device)
        accumulate = False
    _call("nsd_grad_reduce", x.device, C.byref(d), wsp, wsn, _dev_f32(grads, "grads", (spec.param_count,)),
          1 if accumulate else 0, STREAM)
    return grads


def train_step_grads(spec: ModelSpec, flat: torch.Tensor, x: torch.Tensor, ws: torch.Tensor, labels: torch.Tensor,
                     logits: torch.Tensor, grads: torch.Tensor, *, scale: Optional[float] = None, drop_lstm=None,
                     rrelu_slope=None, drop_head=None, residual: bool = False, adam: Optional[dict] = None,
                     fused_head: bool = True, rng: Optional[dict] = None, dx: Optional[torch.Tensor] = None,
                     targets: Optional[torch.Tensor] = None, sam=None, sam_state: Optional[torch.Tensor] = None,
                     opt_state: Optional[torch.Tensor] = None) -> None:
    """The launches of one training evaluation: lstm fwd + head (fwd, mean CE, bwd) in one launch where the shape allows
    (nsd_lstm_head_train; fused_head=False forces the two separate launches), lstm bwd, slab reduce -> `grads` (flat,
    overwritten).  `logits` [B,K] is an output buffer.

    rng=dict(seed=, base_stream=, p_lstm=, p_head=): dropout multipliers and RReLU slopes are generated inside the kernels
    (bit-identical to passing the tensors of nsd_train_masks with the same seed / stream ids); needs rng_path(spec, B, T).

    adam=dict(m=, v=, step=, lr=, beta1=, beta2=, eps=, weight_decay=): single-rank training -- the optimizer update of
    `flat` rides in the reduction launch (nsd_grad_reduce_adam); `grads` is still written.  With opt= (ops.opt_struct) and opt_state=
    (ops.opt_state) in the dict the tail is nsd_grad_reduce_clip_adam instead (global-norm clipping, schedule; step_dev= optional).

    dx [B,T,C] (optional output): dL/dx from nsd_lstm_bwd where dx_path(spec, B, T); not with rng= (nsd_lstm_bwd_rng has no dx).

    targets [B,K] fp32 (labels is then ignored and may be None): the loss is - sum_k targets[b,k] log softmax(logits_b)[k] through the
    `_soft` entry points (nsd_lstm_head_train_soft / nsd_head_train_soft); the backward launches are the same.

    sam (ops.Sam) with sam_state (ops.sam_state(P, 1)): sharpness-aware minimisation -- the forward/backward launches above are issued
    twice with the same arguments but the parameters, first on `flat`, then on the perturbed row the ascent leaves in sam_state
    (nsd_sam_ascend with the tail's grad_scale; without adam=, the data-parallel step, nsd_grad_reduce then nsd_sam_ascend_flat: each
    rank ascends along its own shard's gradient); the tail is the same call as without sam and updates `flat`.  The ascent's scratch is
    the opt_state of adam=, or opt_state= where that carries none.  `logits` and the workspace's loss are then pass 2's.  An empty
    shard launches nothing more than it does without sam.  sam=None: exactly the calls above."""
    B, T, _ = x.shape
    d = spec.dims(B, T)
    flags = _lib.NSD_FLAG_TRAIN | (_lib.NSD_FLAG_RESIDUAL if residual else 0) | _extra_flags
    pp = _dev_f32(flat, "params", (spec.param_count,))
    tgp = _dev_f32(targets, "targets", (B, spec.K))
    labp = _labels_ptr(labels) if targets is None else None
    scale = (1.0 / max(B, 1)) if scale is None else float(scale)
    xp, wsp, wsn, st, dev = _dev_f32(x, "x", (B, T, spec.C)), _dev_f32(ws, "workspace"), _nbytes(ws), STREAM, x.device
    dl, sl, dh = _dev_f32(drop_lstm, "drop_lstm"), _dev_f32(rrelu_slope, "rrelu_slope"), _dev_f32(drop_head, "drop_head")
    lp = _dev_f32(logits, "logits", (B, spec.K))
    dxp = _dev_f32(dx, "dx", (B, T, spec.C))
    if rng is not None:
        # the three random streams of the step are generated inside the kernels: no mask tensors
        if drop_lstm is not None or rrelu_slope is not None or drop_head is not None:
            raise NsdError("train_step_grads: pass either rng= or explicit mask tensors, not both")
        if dx is not None:
            raise NsdError("train_step_grads: dx= needs explicit mask tensors (nsd_lstm_bwd_rng forms no input gradient)")
        r = _rng_struct(rng)

    def forward_backward(pp):
        if rng is not None:
            if targets is not None:
                _call("nsd_lstm_head_train_soft", dev, C.byref(d), pp, xp, None, None, None, C.byref(r), tgp, scale, flags, wsp, wsn, lp, st)
            else:
                _call("nsd_lstm_head_train_rng", dev, C.byref(d), pp, xp, C.byref(r), labp, scale, flags, wsp, wsn, lp, st)
            _call("nsd_lstm_bwd_rng", dev, C.byref(d), pp, xp, C.byref(r), flags, wsp, wsn, st)
            return
        if fused_head and targets is not None:
            _call("nsd_lstm_head_train_soft", dev, C.byref(d), pp, xp, dl, sl, dh, None, tgp, scale, flags, wsp, wsn, lp, st)
        elif fused_head:
            _call("nsd_lstm_head_train", dev, C.byref(d), pp, xp, dl, sl, dh, labp, scale, flags, wsp, wsn, lp, st)
        else:
            _call("nsd_lstm_fwd", dev, C.byref(d), pp, xp, dl, flags, wsp, wsn, st)
            if targets is not None:
                _call("nsd_head_train_soft", dev, C.byref(d), pp, sl, dh, tgp, scale, wsp, wsn, lp, st)
            else:
                _call("nsd_head_train", dev, C.byref(d), pp, sl, dh, labp, scale, wsp, wsn, lp, st)
        _call("nsd_lstm_bwd", dev, C.byref(d), pp, xp, dl, flags, wsp, wsn, dxp, st)

    forward_backward(pp)
    if sam is not None and B > 0:
        # pass 1 is done; the ascent (it reduces pass 1's slabs into grads on the way), then pass 2 at the perturbed row
        if sam_state is None:
            raise NsdError("train_step_grads: sam= needs sam_state= (ops.sam_state(P, 1))")
        scratch = adam["opt_state"] if adam is not None and adam.get("opt") is not None else opt_state
        if scratch is None:
            raise NsdError("train_step_grads: sam= needs an opt_state (in adam=, or opt_state=) for the norm's partial sums")
        if adam is None:
            _call("nsd_grad_reduce", dev, C.byref(d), wsp, wsn, _dev_f32(grads, "grads", (spec.param_count,)), 0, st)
            sam_ascend_flat(flat, grads, sam, scratch, sam_state)
        else:
            sam_ascend(spec, ws, B, T, grads, flat, sam, scratch, sam_state,
                       grad_scale=adam["opt"].grad_scale if adam.get("opt") is not None else 1.0)
        forward_backward(_dev_f32(sam_rows(sam_state, 1, spec.param_count)[0], "sam row"))
    gp = _dev_f32(grads, "grads", (spec.param_count,))
    if adam is None:
        _call("nsd_grad_reduce", dev, C.byref(d), wsp, wsn, gp, 0, st)
    elif adam.get("opt") is not None:
        # clipping / schedule on: reduction with norm, then the update (nsd_grad_reduce_clip_adam); step_dev: the graph-replay form
        # with avg= (ops.Average) and avg_state= also in the dict: its `_avg` twin, the weight average formed by the same update launch
        state = adam["opt_state"]
        av = () if adam.get("avg") is None else _avg_args(_avg_struct(adam["avg"]), adam["avg_state"])
        _call("nsd_grad_reduce_clip_adam_avg" if av else "nsd_grad_reduce_clip_adam", dev, C.byref(d), wsp, wsn, gp, pp,
              _dev_f32(adam["m"], "m", flat.shape), _dev_f32(adam["v"], "v", flat.shape),
              C.byref(adam["opt"]), int(adam.get("step", 0)), _step_ptr(adam.get("step_dev"), "train_step_grads"), state.data_ptr(),
              _nbytes(state), st, *av)
    else:
        _call("nsd_grad_reduce_adam", dev, C.byref(d), wsp, wsn, gp, pp, _dev_f32(adam["m"], "m", flat.shape), _dev_f32(adam["v"], "v", flat.shape),
              adam.get("lr", 1e-3), adam.get("beta1", 0.9), adam.get("beta2", 0.999), adam.get("eps", 1e-8),
              adam.get("weight_decay", 0.0), 1.0, int(adam["step"]), st)


def rng_path(spec: ModelSpec, B: int, T: int) -> bool:
    """True where the kernels can generate the train-mode random streams themselves (nsd_rng_path)."""
    d = spec.dims(B, T)
    return bool(_lib.lib().nsd_rng_path(C.byref(d)))


def dx_path(spec: ModelSpec, B: int, T: int) -> bool:
    """True where nsd_lstm_bwd forms the input gradient dx for this shape (nsd_dx_path)."""
    d = spec.dims(B, T)
    return bool(_lib.lib().nsd_dx_path(C.byref(d)))


def loss_sum(spec: ModelSpec, ws: torch.Tensor, B: int, T: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Sum of the per-trial CE losses written by the labels form of train_backward (device scalar)."""
    d = spec.dims(B, T)
    out = torch.empty(1, dtype=torch.float32, device=ws.device) if out is None else out
    _call("nsd_loss_sum", ws.device, C.byref(d), _dev_f32(ws, "workspace"), _nbytes(ws), out.data_ptr(), STREAM)
    return out


def adam_step(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, *, step: int, lr: float = 1e-3,
              beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 0.0,
              grad_scale: float = 1.0, skip: Optional[torch.Tensor] = None, step_dev: Optional[torch.Tensor] = None) -> None:
    """torch.optim.Adam update of the flat vector.  skip: device fp32 flag (ops.seq_guard); non-zero -> nothing is updated.
    step_dev: device int64 step counter read in place of `step` (nsd_adam_step_dev: hipGraph replay); not together with skip."""
    head = (p.numel(), _dev_f32(p, "p"), _dev_f32(g, "g", p.shape), _dev_f32(m, "m", p.shape), _dev_f32(v, "v", p.shape),
            lr, beta1, beta2, eps, weight_decay, grad_scale)
    if step_dev is not None:
        if skip is not None:
            raise NsdError("adam_step: pass either skip= or step_dev=, not both")
        _call("nsd_adam_step_dev", p.device, *head, _step_ptr(step_dev, "adam_step"), STREAM)
    elif skip is None:
        _call("nsd_adam_step", p.device, *head, step, STREAM)
    else:
        _call("nsd_adam_step_guarded", p.device, *head, step, _dev_f32(skip, "skip"), STREAM)


def step_counter_inc(step_dev: torch.Tensor) -> None:
    """step_dev[0] += 1 on the device: first launch of a hipGraph-replayed step, whose other launches read the counter."""
    _call("nsd_step_counter_inc", step_dev.device, _step_ptr(step_dev, "step_counter_inc"), STREAM)


def train_masks(seed: int, stream, p_lstm: float, p_head: float, drop_lstm: Optional[torch.Tensor], rrelu: Optional[torch.Tensor],
                drop_head: Optional[torch.Tensor]) -> None:
    """Fill the explicit mask tensors of a training step from the streams base + SLOT_* of `seed`: all three in one launch
    (nsd_train_masks), a subset (a tensor that the model does not need is None) with one launch each.  stream: the step's host
    base stream id, or the device int64 step counter it is then formed from (nsd_train_masks_dev: hipGraph replay, all three tensors)."""
    given = [t for t in (drop_lstm, rrelu, drop_head) if t is not None]
    seed, dev = int(seed) & 0xFFFFFFFFFFFFFFFF, given[0].device if given else None
    dl, sl, dh = _dev_f32(drop_lstm, "drop_lstm"), _dev_f32(rrelu, "rrelu"), _dev_f32(drop_head, "drop_head")
    on_dev = torch.is_tensor(stream)
    if len(given) == 3:
        _call("nsd_train_masks_dev" if on_dev else "nsd_train_masks", dev, seed, _step_ptr(stream, "train_masks") if on_dev else stream,
              p_lstm, p_head, drop_lstm.numel(), dl, rrelu.numel(), sl, dh, STREAM)
        return
    if on_dev and given:
        raise NsdError("train_masks: a device step counter needs all three mask tensors")
    if dl is not None:
        _call("nsd_dropout_mask", dev, seed, stream + SLOT_LSTM_DROPOUT, p_lstm, drop_lstm.numel(), dl, STREAM)
    if sl is not None:
        _call("nsd_rrelu_noise", dev, seed, stream + SLOT_RRELU, rrelu.numel(), sl, STREAM)
    if dh is not None:
        _call("nsd_dropout_mask", dev, seed, stream + SLOT_HEAD_DROPOUT, p_head, drop_head.numel(), dh, STREAM)


def dropout_mask(seed: int, stream_id: int, p: float, shape, device) -> torch.Tensor:
    out = torch.empty(shape, dtype=torch.float32, device=device)
    _call("nsd_dropout_mask", out.device, seed & 0xFFFFFFFFFFFFFFFF, stream_id, p, out.numel(), _dev_f32(out, "out"), STREAM)
    return out


def rrelu_noise(seed: int, stream_id: int, shape, device) -> torch.Tensor:
    out = torch.empty(shape, dtype=torch.float32, device=device)
    _call("nsd_rrelu_noise", out.device, seed & 0xFFFFFFFFFFFFFFFF, stream_id, out.numel(), _dev_f32(out, "out"), STREAM)
    return out


# ---- sequence-batched path (large hidden sizes): building blocks ---------------------------------------------------------
def gemm_bf16(a: torch.Tensor, b: torch.Tensor, *, a_kmajor: bool = False, b_kmajor: bool = False, b_shift: int = 0,
              epilogue: int = 0, bias: Optional[torch.Tensor] = None, splits: int = 1, c: Optional[torch.Tensor] = None) -> torch.Tensor:
    """C[M,N] = A . B on the matrix pipe (nsd_gemm_bf16): bf16 device tensors, fp32 accumulate.
    a: [M,K] (or [K,M] when a_kmajor), b: [N,K] (or [K,N] when b_kmajor).  epilogue 0 -> fp32 [splits,M,N] summed here when
    splits > 1; 1 -> bf16 [M,N]; 2 -> bf16 accumulator tiles [N/32, M/32, 64, 16] (+ bias[m]); 3 -> the same tiles, register group
    first: [N/32, M/32, 4, 64, 4].  c: optional caller-owned output of exactly that many elements of that dtype."""
    for t, n in ((a, "a"), (b, "b")):
        if not t.is_cuda or t.dtype != torch.bfloat16 or not t.is_contiguous():
            raise NsdError(f"gemm_bf16: {n} must be a contiguous bf16 tensor on the MI355X")
    K, M = (a.shape[0], a.shape[1]) if a_kmajor else (a.shape[1], a.shape[0])
    Kb, N = (b.shape[0], b.shape[1]) if b_kmajor else (b.shape[1], b.shape[0])
    if K != Kb:
        raise NsdError(f"gemm_bf16: K mismatch {K} vs {Kb}")
    dev = a.device
    cshape = {0: (max(splits, 1), M, N), 1: (M, N), 2: (N // 32, M // 32, 64, 16)}.get(epilogue, (N // 32, M // 32, 4, 64, 4))
    cdtype = torch.float32 if epilogue == 0 else torch.bfloat16
    if c is None:
        c = torch.empty(cshape, dtype=cdtype, device=dev)
    elif not c.is_cuda or c.dtype != cdtype or not c.is_contiguous() or tuple(c.shape) != cshape:
        raise NsdError(f"gemm_bf16: c must be a contiguous {cdtype} device tensor of shape {cshape}")
    _call("nsd_gemm_bf16", dev, a.data_ptr(), a.shape[1], int(a_kmajor), b.data_ptr(), b.shape[1], int(b_kmajor), int(b_shift),
          c.data_ptr(), N, int(epilogue), _dev_f32(bias, "bias", (M,)), M, N, K, int(splits), STREAM)
    if epilogue == 0:
        return c[0] if splits <= 1 else c.sum(0)
    return c


GEMM_KERNELS = {0: "the product's choice", 1: "128 x 128", 2: "register-staged 256 x 256", 22: "LDS-DMA 256 x 256, stages 2 / 2",
                23: "LDS-DMA 256 x 256, stages 2 / 3", 32: "LDS-DMA 256 x 256, stages 3 / 2"}


def gemm_bf16_diag(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor, *, M: int, N: int, K: int, kernel: int = 0,
                   a_off: int = 0, lda: Optional[int] = None, a_kmajor: bool = False,
                   b_off: int = 0, ldb: Optional[int] = None, b_kmajor: bool = False, b_shift: int = 0, b_period: int = 0,
                   b2: Optional[torch.Tensor] = None, b2_off: int = 0, ldb2: Optional[int] = None, b2_shift: int = 0, n_split: int = 0,
                   c_off: int = 0, ldc: Optional[int] = None, epilogue: int = 0, bias: Optional[torch.Tensor] = None,
                   add: Optional[torch.Tensor] = None, splits: int = 1) -> torch.Tensor:
    """Diagnostic build only (inside `with _lib.diagnostic_library():`): the bf16 GEMM with every field the sequence path sets
    (csrc/nsd_bf16.h, GemmArgs) and the kernel pinned (GEMM_KERNELS; nsd_diag_gemm_bf16 of csrc/nsd_diag.h).  a, b, b2: bf16 device
    BUFFERS; an operand is the view that starts *_off elements in, with leading dimension ld* (default: the operand's own row
    length): A [M][lda], or [K][lda] when a_kmajor; B [N][ldb], or [K][ldb] when b_kmajor; B2 [K][ldb2] for the columns from n_split.
    c: the caller's output buffer, written in place from c_off with leading dimension ldc (default N): fp32 [splits][M][ldc]
    (epilogue 0: the partials, NOT summed), bf16 [M][ldc] (1) or M * N bf16 of accumulator tiles (2, 3).  add: fp32 [M][ldc].
    A view that leaves its buffer is refused here; everything else is left to the launcher's own checks.  Returns c."""
    if not _lib.diag_active():
        raise NsdError("gemm_bf16_diag: the kernel can be pinned in the diagnostic build only: use `with _lib.diagnostic_library():`")
    M, N, K, splits, epilogue = int(M), int(N), int(K), int(splits), int(epilogue)
    lda = int(lda if lda is not None else (M if a_kmajor else K))
    ldb = int(ldb if ldb is not None else (N if b_kmajor else K))
    ldb2 = int(ldb2 if ldb2 is not None else (N - n_split if b2 is not None else 0))
    ldc = int(ldc if ldc is not None else N)
    cdtype = torch.float32 if epilogue == 0 else torch.bfloat16
    for t, n, dt in ((a, "a", torch.bfloat16), (b, "b", torch.bfloat16), (b2, "b2", torch.bfloat16), (c, "c", cdtype),
                     (bias, "bias", torch.float32), (add, "add", torch.float32)):
        if t is not None and (not t.is_cuda or t.dtype != dt or not t.is_contiguous()):
            raise NsdError(f"gemm_bf16_diag: {n} must be a contiguous {dt} tensor on the MI355X")
    if min(M, N, K, lda, ldb, ldc, a_off, b_off, b2_off, c_off) < 0 or ldb2 < 0:
        raise NsdError("gemm_bf16_diag: negative size, leading dimension or offset")

    def inside(t, name, off, rows, cols, ld, planes=1):
        last = off + (planes - 1) * rows * ld + (rows - 1) * ld + cols
        if rows < 1 or cols < 1 or planes < 1 or last > t.numel():
            raise NsdError(f"gemm_bf16_diag: the view of {name} ({planes} x {rows} x {cols}, ld {ld}, offset {off}) leaves its "
                           f"buffer of {t.numel()} elements")
    inside(a, "a", a_off, K if a_kmajor else M, M if a_kmajor else K, lda)
    ncols_b = n_split if (b2 is not None and b_kmajor) else N
    inside(b, "b", b_off, K if b_kmajor else N, ncols_b if b_kmajor else K, ldb)
    if b2 is not None:
        inside(b2, "b2", b2_off, K, N - n_split, ldb2)
    if epilogue in (0, 1):
        inside(c, "c", c_off, M, N, ldc, max(splits, 1) if epilogue == 0 else 1)
    else:
        inside(c, "c", c_off, 1, M * N, M * N)
    if add is not None:
        inside(add, "add", 0, M, N, ldc)
    if bias is not None:
        inside(bias, "bias", 0, 1, M, M)
    args = _lib.DiagGemm(a.data_ptr() + 2 * a_off, b.data_ptr() + 2 * b_off, lda, ldb, int(a_kmajor), int(b_kmajor), int(b_shift),
                         int(b_period), None if b2 is None else b2.data_ptr() + 2 * b2_off, ldb2, int(b2_shift), int(n_split), epilogue,
                         c.data_ptr() + c.element_size() * c_off, ldc, None if bias is None else bias.data_ptr(),
                         None if add is None else add.data_ptr(), M, N, K, splits, int(kernel))
    _call("nsd_diag_gemm_bf16", a.device, C.byref(args), STREAM)
    return c


def reduce_dw_diag(part: torch.Tensor, nparts: int, H: int, N: int, I: int, part_off: int = 0) -> torch.Tensor:
    """Diagnostic build only: seq_reduce_dw_kernel alone (nsd_diag_reduce_dw) -- nparts split-K partials [4H][N] of a weight-gradient
    GEMM, rows unit-major (4u + g), read from column part_off on; -> [4H][I] fp32 in torch's row order (g * H + u), I <= N - part_off."""
    if not _lib.diag_active():
        raise NsdError("reduce_dw_diag: diagnostic build only: use `with _lib.diagnostic_library():`")
    _dev_f32(part, "part")
    if min(nparts, H, I) < 1 or part_off < 0 or part_off + I > N or nparts * 4 * H * N > part.numel():
        raise NsdError("reduce_dw_diag: the partials leave their buffer")
    out = torch.empty((4 * H, I), dtype=torch.float32, device=part.device)
    _call("nsd_diag_reduce_dw", part.device, part.data_ptr() + 4 * part_off, int(nparts), int(H), int(N), int(I), out.data_ptr(), STREAM)
    return out


def reduce_db_diag(part: torch.Tensor, nparts: int, H: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Diagnostic build only: seq_reduce_db_kernel alone (nsd_diag_reduce_db) -- nparts rows [4H] in unit-major order -> (b_ih, b_hh),
    each [4H] in torch's order."""
    if not _lib.diag_active():
        raise NsdError("reduce_db_diag: diagnostic build only: use `with _lib.diagnostic_library():`")
    _dev_f32(part, "part")
    if min(nparts, H) < 1 or nparts * 4 * H > part.numel():
        raise NsdError("reduce_db_diag: the partials leave their buffer")
    b_ih = torch.empty(4 * H, dtype=torch.float32, device=part.device)
    b_hh = torch.empty_like(b_ih)
    _call("nsd_diag_reduce_db", part.device, part.data_ptr(), int(nparts), int(H), b_ih.data_ptr(), b_hh.data_ptr(), STREAM)
    return b_ih, b_hh


DX_DIAG_MODES = {"single_calls": 0, "per_model": 1, "mean": 2}


def dx_diag(spec: ModelSpec, da0: torch.Tensor, params: torch.Tensor, mode: str, dx: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Diagnostic build only: the input-gradient kernels alone (nsd_diag_dx) on da0 [M,rows,4H] and params [M,P].  mode "single_calls": M
    launches of the single-model kernel, one per model; "per_model": the model-batched kernel's one launch -> dx [M,rows,C] either way;
    "mean": its serial mean over the models -> dx [rows,C]."""
    if not _lib.diag_active():
        raise NsdError("dx_diag: diagnostic build only: use `with _lib.diagnostic_library():`")
    M, rows, G4 = (int(v) for v in da0.shape)
    if G4 != 4 * spec.H or tuple(params.shape) != (M, spec.param_count):
        raise NsdError(f"dx_diag: da0 must be [M, rows, {4 * spec.H}] and params [M, {spec.param_count}]")
    dx = _out_f32(dx, (rows, spec.C) if mode == "mean" else (M, rows, spec.C), da0.device, "dx_diag: dx")
    _call("nsd_diag_dx", da0.device, _dev_f32(da0, "da0"), params.data_ptr() + 4 * spec.offsets()["lstm.weight_ih_l0"], spec.param_count,
          dx.data_ptr(), rows, M, DX_DIAG_MODES[mode], G4, spec.C, STREAM)
    return dx


# ---- sequence-batched path (nsd_seq_*): large hidden sizes, optional bidirectional, bf16 operands -------------------------
def seq_workspace(spec: ModelSpec, B: int, T: int, device) -> torch.Tensor:
    d = spec.dims(B, T)
    n = _lib.lib().nsd_seq_workspace_bytes(C.byref(d), spec.seq_flags)
    if n < 0:
        check(int(n), "nsd_seq_workspace_bytes")
    ws = torch.empty(int(n), dtype=torch.uint8, device=device)
    _call("nsd_seq_workspace_init", ws.device, ws.data_ptr(), _nbytes(ws), STREAM)     # persistent header: sticky status = 0
    return ws


def _seq_rng(rng: Optional[dict]):
    return None if rng is None else C.byref(_rng_struct(rng))


SEQ_ST_TIMEOUT_MASK, SEQ_ST_NONFINITE = 3, 4


def seq_status(ws: torch.Tensor, detail: bool = False):
    """0 = ok; bit 0 / bit 1 = a forward / backward scan group timed out, in the last evaluation or (sticky) in any evaluation
    since the workspace was created: results invalid; bit 2 (SEQ_ST_NONFINITE, last evaluation only) = a forward scan met a NaN / Inf
    hidden state: the logits of the affected trials are NaN, as the reference's are.  detail=True: (status, groups that ran on one XCD, groups spread over
    several XCDs) counted over the scan launches since the last forward.  Synchronises."""
    out = (C.c_int32 * 4)(-1, 0, 0, 0)
    _call("nsd_seq_status", ws.device, ws.data_ptr(), out, STREAM)
    return (int(out[0]), int(out[2]), int(out[3])) if detail else int(out[0])


def seq_guard(ws: torch.Tensor, flag: torch.Tensor) -> None:
    """flag[0] (device fp32) = 1 if `ws` reports a scan time-out (last evaluation or sticky) or non-finite activations in the last
    evaluation, else 0.  Enqueued, no sync."""
    _call("nsd_seq_guard", ws.device, ws.data_ptr(), _dev_f32(flag, "flag"), STREAM)


def seq_raise_on_timeout(ws: torch.Tensor, what: str, nonfinite: bool = False) -> None:
    """Synchronises; raises NsdError when `ws` reports a scan time-out, or (nonfinite=True: what a training loop wants to know)
    non-finite activations in the last evaluation."""
    st = seq_status(ws)
    if nonfinite and (st & SEQ_ST_NONFINITE) and not (st & SEQ_ST_TIMEOUT_MASK):
        raise NsdError(f"{what}: non-finite activations (NaN / Inf hidden state) in the last evaluation of the sequence-batched path "
                       f"(status {st}): a NaN / Inf window or diverged / NaN weights.  The affected trials' logits and the gradients "
                       "are NaN as in the reference; the guarded Adam update was skipped")
    if st & SEQ_ST_TIMEOUT_MASK:
        stage = " and ".join(n for bit, n in ((1, "forward"), (2, "backward")) if st & bit) or f"code {st}"
        raise NsdError(f"{what}: a {stage} scan group of the sequence-batched path timed out (status {st}): its workgroups were not "
                       "all resident at once (another process on the GPU, a CU mask or a partition mode?).  Results since then "
                       "are invalid (NaN logits / loss, the guarded Adam update was skipped); allocate a fresh workspace to go on")


def seq_infer(spec: ModelSpec, flat: torch.Tensor, x: torch.Tensor, ws: Optional[torch.Tensor] = None, *, want_probs: bool = True,
              logits: Optional[torch.Tensor] = None, probs: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    B, T, Cc = x.shape
    if Cc != spec.C:
        raise NsdError(f"x has {Cc} channels, model expects {spec.C}")
    d = spec.dims(B, T)
    logits = _out_f32(logits, (B, spec.K), x.device, "seq_infer: logits")
    probs = _out_f32(probs, (B, spec.K), x.device, "seq_infer: probs") if want_probs else None
    if B == 0:
        return logits, probs
    ws = seq_workspace(spec, B, T, x.device) if ws is None else ws
    _call("nsd_seq_infer", x.device, C.byref(d), _dev_f32(flat, "params", (spec.param_count,)), _dev_f32(x, "x"), spec.seq_flags,
          _dev_f32(logits, "logits"), _dev_f32(probs, "probs"), ws.data_ptr(), _nbytes(ws), STREAM)
    return logits, probs


def seq_train_fwd(spec: ModelSpec, flat: torch.Tensor, x: torch.Tensor, labels: torch.Tensor, ws: torch.Tensor, *,
                  rng: Optional[dict] = None, scale: Optional[float] = None, logits: Optional[torch.Tensor] = None,
                  targets: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Forward + head + mean CE + head backward of one training evaluation; activations stay in `ws` for seq_train_bwd.
    targets [B,K] fp32 (labels is then ignored and may be None): the soft-target loss (nsd_seq_train_fwd_soft), same logits bit for bit."""
    B, T, _ = x.shape
    d = spec.dims(B, T)
    logits = torch.empty((B, spec.K), dtype=torch.float32, device=x.device) if logits is None else logits
    scale = (1.0 / max(B, 1)) if scale is None else float(scale)
    if targets is not None:
        _call("nsd_seq_train_fwd_soft", x.device, C.byref(d), _dev_f32(flat, "params", (spec.param_count,)), _dev_f32(x, "x", (B, T, spec.C)),
              _seq_rng(rng), _dev_f32(targets, "targets", (B, spec.K)), scale, spec.seq_flags, ws.data_ptr(), _nbytes(ws),
              _dev_f32(logits, "logits", (B, spec.K)), STREAM)
        return logits
    labp = _labels_ptr(labels)
    _call("nsd_seq_train_fwd", x.device, C.byref(d), _dev_f32(flat, "params", (spec.param_count,)), _dev_f32(x, "x", (B, T, spec.C)),
          _seq_rng(rng), labp, scale, spec.seq_flags, ws.data_ptr(), _nbytes(ws), _dev_f32(logits, "logits", (B, spec.K)), STREAM)
    return logits


def seq_train_bwd(spec: ModelSpec, flat: torch.Tensor, ws: torch.Tensor, B: int, T: int, *, rng: Optional[dict] = None,
                  grads: Optional[torch.Tensor] = None, dx: Optional[torch.Tensor] = None) -> torch.Tensor:
    """BPTT + every parameter gradient of the evaluation seq_train_fwd left in `ws` -> flat gradient vector (overwritten).
    dx: optional [B, T, C] fp32 device tensor that receives dL/dx (the gradients are the same bits with and without it)."""
    d = spec.dims(B, T)
    grads = torch.empty(spec.param_count, dtype=torch.float32, device=flat.device) if grads is None else grads
    _call("nsd_seq_train_bwd_dx", flat.device, C.byref(d), _dev_f32(flat, "params", (spec.param_count,)), _seq_rng(rng), spec.seq_flags,
          ws.data_ptr(), _nbytes(ws), _dev_f32(grads, "grads", (spec.param_count,)), _dev_f32(dx, "dx", (B, T, spec.C)), STREAM)
    return grads


def seq_train_fwd_logits(spec: ModelSpec, flat: torch.Tensor, x: torch.Tensor, ws: torch.Tensor, *, rng: Optional[dict] = None,
                         logits: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The training forward of seq_train_fwd with activations kept in `ws`, logits out and nothing else (no labels, no loss, no
    head backward): first call of the any-loss sequence seq_train_fwd_logits -> seq_head_bwd -> seq_train_bwd.  The logits are
    seq_train_fwd's bit for bit."""
    B, T, _ = x.shape
    d = spec.dims(B, T)
    logits = torch.empty((B, spec.K), dtype=torch.float32, device=x.device) if logits is None else logits
    _call("nsd_seq_train_fwd_logits", x.device, C.byref(d), _dev_f32(flat, "params", (spec.param_count,)), _dev_f32(x, "x", (B, T, spec.C)),
          _seq_rng(rng), spec.seq_flags, ws.data_ptr(), _nbytes(ws), _dev_f32(logits, "logits", (B, spec.K)), STREAM)
    return logits


def seq_head_bwd(spec: ModelSpec, flat: torch.Tensor, ws: torch.Tensor, dlogits: torch.Tensor, B: int, T: int, *,
                 rng: Optional[dict] = None) -> None:
    """Head backward from the caller's dL/dlogits [B, K] (fp32, any scale) on the evaluation in `ws` (either forward, same rng):
    seq_train_bwd then returns the gradients of that loss."""
    d = spec.dims(B, T)
    _call("nsd_seq_head_bwd", flat.device, C.byref(d), _dev_f32(flat, "params", (spec.param_count,)), _seq_rng(rng),
          _dev_f32(dlogits, "dlogits", (B, spec.K)), spec.seq_flags, ws.data_ptr(), _nbytes(ws), STREAM)


def seq_loss_sum(spec: ModelSpec, ws: torch.Tensor, B: int, T: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    d = spec.dims(B, T)
    out = torch.empty(1, dtype=torch.float32, device=ws.device) if out is None else out
    _call("nsd_seq_loss_sum", ws.device, C.byref(d), spec.seq_flags, ws.data_ptr(), _nbytes(ws), out.data_ptr(), STREAM)
    return out


SEQ_PROFILE_KINDS = ("scan_fwd", "scan_bwd", "gemm_xproj", "gemm_dw", "gemm_din", "head", "head_grads", "prep", "gemm_dx", "head_bwd")


def seq_profile(enable: bool) -> None:
    """Diagnostic build only (`with _lib.diagnostic_library():`): start / stop the HIP-event timing of the sequence-batched
    path's kernels (nsd_seq_profile, csrc/nsd_diag.h)."""
    if not _lib.diag_active():
        raise NsdError("seq_profile: per-kernel timing lives in the diagnostic build: use `with _lib.diagnostic_library():`")
    _call("nsd_seq_profile", None, 1 if enable else 0)


def seq_profile_read() -> Dict[str, Tuple[float, int]]:
    """kind -> (total ms, launches) recorded since seq_profile(True) / the last read.  Synchronises."""
    out = {}
    for i, name in enumerate(SEQ_PROFILE_KINDS):
        ms, n = C.c_float(0), C.c_int32(0)
        _call("nsd_seq_profile_read", None, i, C.byref(ms), C.byref(n))
        out[name] = (float(ms.value), int(n.value))
    return out


# ---- model-batched H = 48 path: M models of one shape per launch (include/nsd.h, nsd_multi_*) ----------------------------------------
def multi_path(spec: ModelSpec, M: int, B: int = 32, T: int = 1) -> bool:
    """True where nsd_multi_* cover M models of this shape (H = 48, L = 2, C <= 8, T <= 1024, F <= 64, K <= 8, 1 <= M <= 32)."""
    d = spec.dims(B, T)
    return bool(_lib.lib().nsd_multi_path(C.byref(d), int(M)))


def multi_workspace(spec: ModelSpec, M: int, B: int, T: int, device) -> torch.Tensor:
    """The training workspace of M models of B trials each (regions of a batch of M*B trials)."""
    d, w = spec.dims(B, T), WsLayout()
    n = _lib.lib().nsd_multi_workspace_bytes(C.byref(d), int(M), C.byref(w))
    if n < 0:
        check(int(n), "nsd_multi_workspace_bytes")
    return torch.empty(max(int(n) // 4, 1), dtype=torch.float32, device=device)


def _multi_x(spec: ModelSpec, x: torch.Tensor, M: int) -> Tuple[int, int, int]:
    """x [M,B,T,C] (per-model windows) or [B,T,C] (shared: x_model_stride 0) of M models of `spec` -> (B, T, stride)."""
    if x.dim() == 4 and x.shape[0] != M:                  # M is the parameters' model count here
        raise NsdError(f"multi: x has {x.shape[0]} model slices for {M} models")
    _, B, T, Cc, stride, _ = _model_windows(x, M, "multi", "[M,B,T,C] or [B,T,C]")
    if Cc != spec.C:
        raise NsdError(f"x has {Cc} channels, model expects {spec.C}")
    return B, T, stride


def multi_train_step(spec: ModelSpec, params: torch.Tensor, x: torch.Tensor, labels: torch.Tensor, ws: torch.Tensor, grads: torch.Tensor,
                     *, rngs=None, logits: Optional[torch.Tensor] = None, fuse_adam: bool = True, m: Optional[torch.Tensor] = None,
                     v: Optional[torch.Tensor] = None, step: int = 1, lr: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999,
                     eps: float = 1e-8, weight_decay: float = 0.0, grad_scale: float = 1.0,
                     targets: Optional[torch.Tensor] = None, opt=None, opt_state: Optional[torch.Tensor] = None, avg=None,
                     avg_state: Optional[torch.Tensor] = None, sam=None, sam_state: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One training step of M models at once: params [M,P], x [M,B,T,C] or shared [B,T,C], labels [M*B] int32, grads [M,P].
    Forward + head + mean CE per model + head backward, BPTT, then the reduction (+ Adam on params / m / v when fuse_adam).
    rngs: None (no dropout, eval RReLU slope) or M dicts {seed, base_stream, p_lstm, p_head}.  Returns logits [M*B, K].
    targets [M*B, K] fp32 (labels is then ignored and may be None): the soft-target loss per model (nsd_multi_train_fwd_soft).
    opt (ops.opt_struct) with opt_state (ops.opt_state(P, M)): the tail is nsd_multi_grad_reduce_clip_adam -- one norm, record and skip
    decision per model; the Adam arguments of this call are then ignored.  opt may be a list of M (nsd_multi_grad_reduce_clip_adam_each:
    every field per model); a list of equal entries is the single opt's launch.  rngs whose p_lstm / p_head differ between models go
    with NSD_FLAG_MODEL_P (each model drops with its own probabilities); equal ones go without the flag, as before.
    avg (ops.Average, or a list of M with None for a model that does not average) with avg_state (ops.avg_state(P, M)) and opt: the
    `_avg` twin of the clipped tail forms each model's weight average in the update launch; a list with different entries goes through
    nsd_multi_grad_reduce_clip_adam_avg_each together with M opt entries.
    sam (ops.Sam, or a list of M with None for a model without it) with sam_state (ops.sam_state(P, M)) and opt_state: sharpness-aware
    minimisation -- forward and backward are issued twice with the same arguments but the parameters, first on params, then on the
    perturbed rows nsd_multi_sam_ascend leaves in sam_state (each model with its own rho and its opt's grad_scale; a model without
    SAM runs pass 2 on a bitwise copy of its parameters); the tail is the same call as without sam.  logits are then pass 2's."""
    M = int(params.shape[0])
    B, T, stride = _multi_x(spec, x, M)
    d = spec.dims(B, T)
    if logits is None:
        logits = torch.empty((M * B, spec.K), dtype=torch.float32, device=params.device)
    if targets is None and (labels.dtype != torch.int32 or not labels.is_contiguous() or labels.numel() != M * B):
        raise NsdError(f"multi: labels must be contiguous int32 [M*B] = [{M * B}]")
    r = _rng_array(rngs, M, "multi")
    rp = C.cast(r, C.c_void_p) if r is not None else None
    fl = _lib.NSD_FLAG_MODEL_P if r is not None and any((g.p_lstm, g.p_head) != (r[0].p_lstm, r[0].p_head) for g in r) else 0
    opt, opts = _per_model(opt, M, "multi: opt", key=bytes)
    P = spec.param_count
    pp, xp = _dev_f32(params, "params", (M, P)), _dev_f32(x, "x")

    def forward_backward(pp):
        if targets is not None:
            _call("nsd_multi_train_fwd_soft", params.device, C.byref(d), M, pp, xp, stride, rp, _dev_f32(targets, "targets", (M * B, spec.K)), fl,
                  ws.data_ptr(), _nbytes(ws), _dev_f32(logits, "logits"), STREAM)
        else:
            _call("nsd_multi_train_fwd", params.device, C.byref(d), M, pp, xp, stride, rp, labels.data_ptr(), fl, ws.data_ptr(), _nbytes(ws),
                  _dev_f32(logits, "logits"), STREAM)
        _call("nsd_multi_train_bwd", params.device, C.byref(d), M, pp, xp, stride, rp, fl, ws.data_ptr(), _nbytes(ws), STREAM)

    forward_backward(pp)
    if sam is not None:
        # pass 1 is done; the ascent of all models (it reduces pass 1's slabs into grads on the way), then pass 2 at the perturbed rows
        if sam_state is None or opt_state is None:
            raise NsdError("multi: sam= needs sam_state= (ops.sam_state(P, M)) and opt_state= (the norm's partial sums)")
        gsc = [o.grad_scale for o in opts] if opts is not None else opt.grad_scale if opt is not None else grad_scale
        multi_sam_ascend(spec, ws, B, T, grads, params, sam, opt_state, sam_state, grad_scale=gsc)
        forward_backward(_dev_f32(sam_rows(sam_state, M, P), "sam rows", (M, P)))
    avg, avgs = _per_model(avg, M, "multi: avg")
    if (avg is not None or avgs is not None) and not (fuse_adam and (opt is not None or opts is not None) and avg_state is not None):
        raise NsdError("multi: avg= needs fuse_adam, opt= / opt_state= (the clipped tail forms the average) and avg_state=")
    if fuse_adam and (avgs is not None or (avg is not None and opts is not None)):
        # per-model settings on either side: M entries of both (an equal setting repeated)
        arr = (_lib.Opt * M)(*(opts if opts is not None else [opt] * M))
        avr = (_lib.Avg * M)(*[_avg_struct(a) for a in (avgs if avgs is not None else [avg] * M)])
        _call("nsd_multi_grad_reduce_clip_adam_avg_each", params.device, C.byref(d), M, ws.data_ptr(), _nbytes(ws), _dev_f32(grads, "grads", (M, P)), pp,
              _dev_f32(m, "m", (M, P)), _dev_f32(v, "v", (M, P)), C.cast(arr, C.c_void_p), int(step), None, opt_state.data_ptr(), _nbytes(opt_state),
              STREAM, C.cast(avr, C.c_void_p), avg_state.data_ptr(), _nbytes(avg_state))
    elif fuse_adam and avg is not None:
        _call("nsd_multi_grad_reduce_clip_adam_avg", params.device, C.byref(d), M, ws.data_ptr(), _nbytes(ws), _dev_f32(grads, "grads", (M, P)), pp,
              _dev_f32(m, "m", (M, P)), _dev_f32(v, "v", (M, P)), C.byref(opt), int(step), None, opt_state.data_ptr(), _nbytes(opt_state), STREAM,
              *_avg_args(_avg_struct(avg), avg_state))
    elif fuse_adam and opts is not None:
        arr = (_lib.Opt * M)(*opts)
        _call("nsd_multi_grad_reduce_clip_adam_each", params.device, C.byref(d), M, ws.data_ptr(), _nbytes(ws), _dev_f32(grads, "grads", (M, P)), pp,
              _dev_f32(m, "m", (M, P)), _dev_f32(v, "v", (M, P)), C.cast(arr, C.c_void_p), int(step), None, opt_state.data_ptr(), _nbytes(opt_state),
              STREAM)
    elif fuse_adam and opt is not None:
        _call("nsd_multi_grad_reduce_clip_adam", params.device, C.byref(d), M, ws.data_ptr(), _nbytes(ws), _dev_f32(grads, "grads", (M, P)), pp,
              _dev_f32(m, "m", (M, P)), _dev_f32(v, "v", (M, P)), C.byref(opt), int(step), None, opt_state.data_ptr(), _nbytes(opt_state), STREAM)
    elif fuse_adam:
        _call("nsd_multi_grad_reduce_adam", params.device, C.byref(d), M, ws.data_ptr(), _nbytes(ws), _dev_f32(grads, "grads", (M, P)), pp,
              _dev_f32(m, "m", (M, P)), _dev_f32(v, "v", (M, P)), lr, beta1, beta2, eps, weight_decay, grad_scale, int(step), STREAM)
    else:
        _call("nsd_multi_grad_reduce", params.device, C.byref(d), M, ws.data_ptr(), _nbytes(ws), _dev_f32(grads, "grads", (M, P)), STREAM)
    return logits


def multi_loss_sum(spec: ModelSpec, ws: torch.Tensor, M: int, B: int, T: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[m] = sum of model m's per-trial CE losses of the last multi_train_step (device)."""
    if out is None:
        out = torch.empty(M, dtype=torch.float32, device=ws.device)
    d = spec.dims(B, T)
    _call("nsd_multi_loss_sum", ws.device, C.byref(d), int(M), ws.data_ptr(), _nbytes(ws), _dev_f32(out, "out", (M,)), STREAM)
    return out


def multi_dx_path(spec: ModelSpec, M: int, B: int = 32, T: int = 1) -> bool:
    """True where nsd_multi_train_bwd_dx forms the input gradient of M models of this shape (nsd_multi_path and nsd_dx_path)."""
    d = spec.dims(B, T)
    return bool(_lib.lib().nsd_multi_dx_path(C.byref(d), int(M)))


DX_REDUCE = {"per_model": _lib.NSD_DX_PER_MODEL, "mean": _lib.NSD_DX_MEAN}


def multi_loss_mean(spec: ModelSpec, ws: torch.Tensor, M: int, B: int, T: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[0] = the serial fp32 sum over m ascending of multi_loss_sum's M values / float32(M) (device float [1]: spatial_fit_step's
    loss_in takes it without a host read)."""
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=ws.device)
    d = spec.dims(B, T)
    _call("nsd_multi_loss_mean", ws.device, C.byref(d), int(M), ws.data_ptr(), _nbytes(ws), _dev_f32(out, "out", (1,)), STREAM)
    return out


def multi_train_dx(spec: ModelSpec, params: torch.Tensor, x: torch.Tensor, ws: torch.Tensor, logits: torch.Tensor, dx: torch.Tensor, *,
                   labels: Optional[torch.Tensor] = None, targets: Optional[torch.Tensor] = None, reduce: str = "mean",
                   loss_out: Optional[torch.Tensor] = None) -> None:
    """The model-batched twin of train_dx: the input gradient through M FROZEN models in the launches one model uses --
    nsd_multi_train_fwd[_soft] (rng NULL: no dropout, the eval RReLU slope) -> nsd_multi_train_bwd_dx -> nsd_multi_loss_mean (where
    loss_out, a device float [1], is given).  params [M,P] are read, never written; x [B,T,C] (shared) or [M,B,T,C]; labels [M*B] int32
    or targets [M*B,K]; ws: ops.multi_workspace; logits [M*B,K].
    reduce="per_model": dx [M,B,T,C], model m's slice the gradient of ITS mean loss with respect to ITS windows.
    reduce="mean":      dx [B,T,C] = align.mean_over_models of those (shared windows only): the gradient of (1/M) sum_m mean_n CE_m.
    The parameter-gradient slabs stay in the workspace unreduced.  Needs multi_dx_path."""
    if reduce not in DX_REDUCE:
        raise NsdError(f"multi_train_dx: reduce {reduce!r} must be 'mean' or 'per_model'")
    M = int(params.shape[0])
    B, T, stride = _multi_x(spec, x, M)
    if not multi_dx_path(spec, M, B, T):
        raise NsdError(f"multi_train_dx: {M} models of {spec} at batch {B} are outside nsd_multi_dx_path (hidden size 48, 2 layers, <= 8 "
                       "channels, T <= 1024)")
    if reduce == "mean" and stride != 0:
        raise NsdError("multi_train_dx: reduce='mean' needs shared windows x [B,T,C] (the mean over the models is that of one window set)")
    d = spec.dims(B, T)
    dev = params.device
    pp, xp = _dev_f32(params, "params", (M, spec.param_count)), _dev_f32(x, "x")
    wsp, wsn, lp = _dev_f32(ws, "workspace"), _nbytes(ws), _dev_f32(logits, "logits", (M * B, spec.K))
    dxp = _dev_f32(dx, "dx", (B, T, spec.C) if reduce == "mean" else (M, B, T, spec.C))
    if targets is not None:
        _call("nsd_multi_train_fwd_soft", dev, C.byref(d), M, pp, xp, stride, None, _dev_f32(targets, "targets", (M * B, spec.K)), 0, wsp, wsn, lp, STREAM)
    else:
        if labels is None or labels.numel() != M * B:
            raise NsdError(f"multi_train_dx: labels must be contiguous int32 [M*B] = [{M * B}]")
        _call("nsd_multi_train_fwd", dev, C.byref(d), M, pp, xp, stride, None, _labels_ptr(labels), 0, wsp, wsn, lp, STREAM)
    _call("nsd_multi_train_bwd_dx", dev, C.byref(d), M, pp, xp, stride, 0, wsp, wsn, dxp, DX_REDUCE[reduce], STREAM)
    if loss_out is not None:
        _call("nsd_multi_loss_mean", dev, C.byref(d), M, wsp, wsn, _dev_f32(loss_out, "loss_out", (1,)), STREAM)


def multi_infer(spec: ModelSpec, params: torch.Tensor, x: torch.Tensor, *, want_probs: bool = True, logits: Optional[torch.Tensor] = None,
                probs: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Eval-mode forward of M models in one launch: params [M,P], x [M,B,T,C] or shared [B,T,C] -> logits [M,B,K] (+ probs).
    logits / probs / scratch: optional caller-owned buffers (scratch: at least nsd_multi_infer_scratch_bytes long, any dtype)."""
    M = int(params.shape[0])
    B, T, stride = _multi_x(spec, x, M)
    d = spec.dims(B, T)
    logits = _out_f32(logits, (M, B, spec.K), params.device, "multi_infer: logits")
    probs = _out_f32(probs, (M, B, spec.K), params.device, "multi_infer: probs") if want_probs else None
    if B == 0:
        return logits, probs
    nscr = int(_lib.lib().nsd_multi_infer_scratch_bytes(C.byref(d), M))
    if nscr < 0:
        check(nscr, "nsd_multi_infer_scratch_bytes")
    scratch, scrp = _scratch_ptr(scratch, nscr, params.device, "multi_infer")
    _call("nsd_multi_infer", params.device, C.byref(d), M, _dev_f32(params, "params", (M, spec.param_count)), _dev_f32(x, "x"), stride,
          0, _dev_f32(logits, "logits"), _dev_f32(probs, "probs"), scrp, STREAM)
    return logits, probs


# ---- resumable H = 48 inference: streams decoded chunk by chunk (nsd_stream_* of include/nsd.h) ----

def stream_path(spec: ModelSpec) -> bool:
    """True where nsd_stream_step covers this model (H = 48, L = 2, C <= 8, F <= 64, K <= 64, one direction)."""
    d = spec.dims(1, 1)
    return spec.D == 1 and bool(_lib.lib().nsd_stream_path(C.byref(d)))


def stream_layout(spec: ModelSpec) -> "_lib.StreamLayout":
    """Float offsets of h[l], c[l], pool_max, pool_den, pool_acc and the int64 step count inside one slot, and the slot stride."""
    d, lay = spec.dims(1, 1), _lib.StreamLayout()
    check(_lib.lib().nsd_stream_state_layout(C.byref(d), C.byref(lay)), "nsd_stream_state_layout")
    return lay


def stream_state_bytes(spec: ModelSpec, S: int) -> int:
    d = spec.dims(1, 1)
    n = int(_lib.lib().nsd_stream_state_bytes(C.byref(d), int(S)))
    if n < 0:
        check(n, "nsd_stream_state_bytes")
    return n


def stream_state(spec: ModelSpec, S: int, device="cuda") -> torch.Tensor:
    """A reset state of S slots on `device`: fp32 [S, stride] (one row per stream; stream_layout names the columns)."""
    state = torch.empty((int(S), int(stream_layout(spec).stride)), dtype=torch.float32, device=device)
    stream_reset(spec, state)
    return state


def _slots_ptr(slots: Optional[torch.Tensor], what: str) -> Optional[int]:
    if slots is None:
        return None
    if slots.dtype != torch.int32 or not slots.is_cuda or not slots.is_contiguous() or slots.dim() != 1:
        raise NsdError(f"{what}: slots must be a contiguous 1-D int32 tensor on the device")
    return slots.data_ptr()


def stream_reset(spec: ModelSpec, state: torch.Tensor, slots: Optional[torch.Tensor] = None) -> None:
    """Reset all slots of `state`, or the ones a device int32 tensor names: zero h and c, empty pooling state, step count 0."""
    S = int(state.shape[0]) if state.dim() == 2 else 0
    d = spec.dims(0, 1)
    n = 0 if slots is None else int(slots.numel())
    if slots is not None and n == 0:
        return
    _call("nsd_stream_reset", state.device, C.byref(d), _dev_f32(state, "state"), _nbytes(state), S, _slots_ptr(slots, "stream_reset"), n,
          STREAM)


def stream_step(spec: ModelSpec, flat: torch.Tensor, x: torch.Tensor, state: torch.Tensor, *, slots: Optional[torch.Tensor] = None,
                residual: bool = False, read: bool = True, want_probs: bool = True, logits: Optional[torch.Tensor] = None,
                probs: Optional[torch.Tensor] = None) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """Advance B streams by the chunk x [B,n,C] (stream b lives in slot slots[b], or b) and, with read=True, return what ops.infer gives
    on each stream's whole prefix: logits [B,K] (+ probs).  read=False advances only and returns (None, None).  logits / probs:
    optional caller-owned buffers."""
    if x.dim() != 3 or x.shape[-1] != spec.C:
        raise NsdError(f"stream_step: x must be [B, n, {spec.C}], got {tuple(x.shape)}")
    B, T, _ = (int(v) for v in x.shape)
    S = int(state.shape[0]) if state.dim() == 2 else 0
    if slots is not None and int(slots.numel()) != B:
        raise NsdError(f"stream_step: {int(slots.numel())} slot indices for {B} streams")
    d = spec.dims(B, T)
    if read:
        logits = _out_f32(logits, (B, spec.K), x.device, "stream_step: logits")
        probs = _out_f32(probs, (B, spec.K), x.device, "stream_step: probs") if want_probs else None
    else:
        logits = probs = None
    if B == 0:
        _dev_f32(flat, "params", (spec.param_count,)); _dev_f32(state, "state")
        return logits, probs
    _call("nsd_stream_step", x.device, C.byref(d), _dev_f32(flat, "params", (spec.param_count,)), _dev_f32(x, "x"),
          _slots_ptr(slots, "stream_step"), _lib.NSD_FLAG_RESIDUAL if residual else 0, _dev_f32(state, "state"), _nbytes(state), S,
          _dev_f32(logits, "logits"), _dev_f32(probs, "probs"), STREAM)
    return logits, probs


# ---- resumable inference of M models per launch: an ensemble decoding live streams (nsd_multi_stream_* of include/nsd.h) ----

def multi_stream_path(spec: ModelSpec, M: int) -> bool:
    """True where nsd_multi_stream_step covers M models of this shape (stream_path and 1 <= M <= 32)."""
    d = spec.dims(1, 1)
    return spec.D == 1 and bool(_lib.lib().nsd_multi_stream_path(C.byref(d), int(M)))


def multi_stream_state(spec: ModelSpec, M: int, S: int, device="cuda") -> torch.Tensor:
    """A reset state of M models with S slots each on `device`: fp32 [M, S, stride].  state[m] is an ordinary stream_state of model m
    (stream_step takes it as it is); the flat [M*S, stride] view is what stream_reset takes: slot m*S + s is stream s of model m."""
    d = spec.dims(1, 1)
    n = int(_lib.lib().nsd_multi_stream_state_bytes(C.byref(d), int(M), int(S)))
    if n < 0:
        check(n, "nsd_multi_stream_state_bytes")
    state = torch.empty((int(M), int(S), int(stream_layout(spec).stride)), dtype=torch.float32, device=device)
    if _nbytes(state) != n:
        raise NsdError(f"multi_stream_state: {_nbytes(state)} bytes for nsd_multi_stream_state_bytes = {n}")
    stream_reset(spec, state.view(int(M) * int(S), -1))
    return state


def multi_stream_step(spec: ModelSpec, params: torch.Tensor, x: torch.Tensor, state: torch.Tensor, *, slots: Optional[torch.Tensor] = None,
                      residual: bool = False, read: bool = True, want_mean: bool = True, logits: Optional[torch.Tensor] = None,
                      probs: Optional[torch.Tensor] = None, mean: Optional[torch.Tensor] = None) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor]]:
    """Advance B streams in each of M models by one launch: params [M,P], the chunk x [B,n,C] (shared by the models) or [M,B,n,C],
    state [M,S,stride]; stream b lives in slot slots[b] (or b) of every model.  With read=True returns (logits [M,B,K], probs [M,B,K],
    mean [B,K]): per model what stream_step gives, bit for bit, and the mean of the models' probabilities (a serial fp32 sum over the
    models, divided by M; None with want_mean=False: no second launch).  read=False advances only and returns (None, None, None).
    logits / probs / mean: optional caller-owned buffers."""
    if params.dim() != 2:
        raise NsdError(f"multi_stream_step: params must be [M, {spec.param_count}], got {tuple(params.shape)}")
    M = int(params.shape[0])
    if x.dim() not in (3, 4) or x.shape[-1] != spec.C or (x.dim() == 4 and int(x.shape[0]) != M):
        raise NsdError(f"multi_stream_step: x must be [B, n, {spec.C}] or [{M}, B, n, {spec.C}], got {tuple(x.shape)}")
    B, T = int(x.shape[-3]), int(x.shape[-2])
    stride = B * T * spec.C if x.dim() == 4 else 0
    if state.dim() != 3 or int(state.shape[0]) != M:
        raise NsdError(f"multi_stream_step: state must be [{M}, S, stride], got {tuple(state.shape)}")
    S = int(state.shape[1])
    if slots is not None and int(slots.numel()) != B:
        raise NsdError(f"multi_stream_step: {int(slots.numel())} slot indices for {B} streams")
    d = spec.dims(B, T)
    if read:
        logits = _out_f32(logits, (M, B, spec.K), x.device, "multi_stream_step: logits")
        probs = _out_f32(probs, (M, B, spec.K), x.device, "multi_stream_step: probs")
        mean = _out_f32(mean, (B, spec.K), x.device, "multi_stream_step: mean") if want_mean else None
    else:
        logits = probs = mean = None
    pp = _dev_f32(params, "params", (M, spec.param_count))
    if B == 0:
        _dev_f32(state, "state")
        return logits, probs, mean
    _call("nsd_multi_stream_step", x.device, C.byref(d), M, pp, _dev_f32(x, "x"), stride, _slots_ptr(slots, "multi_stream_step"),
          _lib.NSD_FLAG_RESIDUAL if residual else 0, _dev_f32(state, "state"), _nbytes(state), S, _dev_f32(logits, "logits"),
          _dev_f32(probs, "probs"), _dev_f32(mean, "mean"), STREAM)
    return logits, probs, mean


# ---- session calibration: pooled features of stream slots, the read-out refitted on them (nsd_stream_features / nsd_head_fit) ----

FIT_GROUPS = {"ln": _lib.NSD_FIT_LN, "fc0": _lib.NSD_FIT_FC0, "fc3": _lib.NSD_FIT_FC3}


def stream_features(spec: ModelSpec, state: torch.Tensor, *, slots: Optional[torch.Tensor] = None, n: Optional[int] = None,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """feats [n,H]: row i is pool_acc / pool_den of slot slots[i] (or i) of `state` -- fp32 [S, stride], or the [M, S, stride] state of an
    ensemble read as M*S flat slots.  A never-stepped or out-of-range slot gives a NaN row."""
    flat = state.view(-1, int(state.shape[-1])) if state.dim() == 3 else state
    S = int(flat.shape[0]) if flat.dim() == 2 else 0
    n = (S if slots is None else int(slots.numel())) if n is None else int(n)
    if slots is not None and int(slots.numel()) != n:
        raise NsdError(f"stream_features: {int(slots.numel())} slot indices for {n} rows")
    out = _out_f32(out, (n, spec.H), state.device, "stream_features: feats")
    d = spec.dims(0, 1)
    _call("nsd_stream_features", state.device, C.byref(d), _dev_f32(flat, "state"), _nbytes(flat), S, _slots_ptr(slots, "stream_features"), n,
          _dev_f32(out, "feats"), STREAM)
    return out


def head_fit_path(spec: ModelSpec, M: int, N: int) -> bool:
    """True where nsd_head_fit covers M models of this shape on N trials (stream_path, 1 <= M <= 32, 1 <= N <= 256, the LDS need)."""
    d = spec.dims(int(N), 1)
    return spec.D == 1 and bool(_lib.lib().nsd_head_fit_path(C.byref(d), int(M)))


def head_fit_layout(spec: ModelSpec) -> "_lib.FitLayout":
    """Float offsets of m, v, the int64 epoch count and the int32 status word inside one model's fit state, and its stride."""
    d, lay = spec.dims(1, 1), _lib.FitLayout()
    check(_lib.lib().nsd_head_fit_state_layout(C.byref(d), C.byref(lay)), "nsd_head_fit_state_layout")
    return lay


def head_fit_state(spec: ModelSpec, M: int, device="cuda") -> torch.Tensor:
    """A reset fit state of M models: fp32 zeros [M, stride] (all-zero bytes is the reset state)."""
    d = spec.dims(1, 1)
    n = int(_lib.lib().nsd_head_fit_state_bytes(C.byref(d), int(M)))
    if n < 0:
        check(n, "nsd_head_fit_state_bytes")
    state = torch.zeros((int(M), int(head_fit_layout(spec).stride)), dtype=torch.float32, device=device)
    if _nbytes(state) != n:
        raise NsdError(f"head_fit_state: {_nbytes(state)} bytes for nsd_head_fit_state_bytes = {n}")
    return state


def fit_mask(train) -> int:
    """("ln", "fc0", "fc3") names, or the NSD_FIT_* bits themselves -> the train mask of nsd_fit"""
    if isinstance(train, int):
        return train
    bad = [g for g in train if g not in FIT_GROUPS]
    if bad:
        raise NsdError(f"head_fit: unknown tensor group(s) {bad}; the groups are {sorted(FIT_GROUPS)}")
    mask = 0
    for g in train:
        mask |= FIT_GROUPS[g]
    return mask


def head_fit(spec: ModelSpec, params: torch.Tensor, feats: torch.Tensor, targets: torch.Tensor, state: torch.Tensor, *, epochs: int,
             lr: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 0.0,
             scale: Optional[float] = None, train=("ln", "fc0", "fc3"), rngs=None, loss_out: Optional[torch.Tensor] = None,
             want_loss: bool = True) -> Optional[torch.Tensor]:
    """`epochs` full-batch Adam epochs of the read-out (LayerNorm, fc.0, fc.3) of M models on frozen pooled features, in ONE launch.
    params [M,P] (or [P]) are updated in place, only the tensors `train` names; feats [N,H] (shared by the models) or [M,N,H]; targets
    [M,N,K] (or [N,K] for one model) soft target rows; state: head_fit_state, carried between calls (more epochs later continue the
    same run bit for bit); scale: 1/N by default; rngs: None (eval slope, no dropout) or one rng dict per model (p_head is read).
    Returns the losses before each epoch's update [M, epochs] (None with want_loss=False)."""
    p2 = params.view(1, -1) if params.dim() == 1 else params
    M = int(p2.shape[0])
    if feats.dim() not in (2, 3) or int(feats.shape[-1]) != spec.H or (feats.dim() == 3 and int(feats.shape[0]) != M):
        raise NsdError(f"head_fit: feats must be [N, {spec.H}] or [{M}, N, {spec.H}], got {tuple(feats.shape)}")
    N = int(feats.shape[-2])
    stride = N * spec.H if feats.dim() == 3 else 0
    d = spec.dims(N, 1)
    fit = _lib.Fit(int(epochs), fit_mask(train), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
                   float(1.0 / N if scale is None else scale))
    if want_loss:
        loss_out = _out_f32(loss_out, (M, int(epochs)), params.device, "head_fit: loss_out")
    _call("nsd_head_fit", params.device, C.byref(d), M, _dev_f32(p2, "params", (M, spec.param_count)), _dev_f32(feats, "feats"), stride,
          _dev_f32(targets.view(M * N, spec.K) if targets.numel() == M * N * spec.K else targets, "targets", (M * N, spec.K)), C.byref(fit),
          _rng_array(rngs, M, "head_fit"), _dev_f32(state, "fit_state"), _nbytes(state), _dev_f32(loss_out, "loss_out"), STREAM)
    return loss_out


# ---- early stopping for model batches: metrics, the best-evaluation decision and the snapshot in one launch (nsd_multi_eval) ----

EVAL_RECORD_BYTES, SELECT_RECORD_BYTES = C.sizeof(_lib.EvalRecord), C.sizeof(_lib.SelectRecord)      # 280, 40


def multi_eval_path(M: int, B: int, K: int, P: int = 0) -> bool:
    """True where nsd_multi_eval takes the shape (1 <= M <= 32, 1 <= K <= 8, B >= 1, M * B * K <= 2^31 - 1)."""
    return bool(_lib.lib().nsd_multi_eval_path(int(M), int(B), int(K), int(P)))


def select_records_bytes(M: int) -> int:
    """Bytes of the M select records at the head of a select state, padded to 16: the snapshot rows [M, P] follow."""
    return (int(M) * SELECT_RECORD_BYTES + 15) // 16 * 16


def select_state_bytes(M: int, P: int) -> int:
    n = int(_lib.lib().nsd_select_state_bytes(int(M), int(P)))
    if n < 0:
        check(n, "nsd_select_state_bytes")
    return n


def select_state(M: int, P: int, device, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The select state of M models of P parameters: records zeroed (nsd_select_state_init), snapshot rows [M, P] not yet written.
    out: the caller's contiguous device bytes to initialise in place of a fresh buffer (select_state_bytes(M, P) of them)."""
    n = select_state_bytes(M, P)
    st = torch.empty(n, dtype=torch.uint8, device=device) if out is None else out
    if st.dtype != torch.uint8 or not st.is_cuda or not st.is_contiguous() or st.numel() != n:
        raise NsdError(f"select_state: out must be {n} contiguous bytes on the device")
    _call("nsd_select_state_init", st.device, st.data_ptr(), _nbytes(st), int(M), int(P), STREAM)
    return st


def select_snapshot(state: torch.Tensor, M: int, P: int) -> torch.Tensor:
    """The snapshot rows [M, P] of a select state: a float32 view, no copy.  A row is defined once its model has a best evaluation."""
    off = select_records_bytes(M)
    return state[off:off + 4 * int(M) * int(P)].view(torch.float32).view(int(M), int(P))


def eval_buffer(M: int, device) -> torch.Tensor:
    """An output buffer for multi_eval: M nsd_eval_record, as bytes."""
    return torch.empty(int(M) * EVAL_RECORD_BYTES, dtype=torch.uint8, device=device)


def multi_eval(logits: torch.Tensor, labels: torch.Tensor, *, counts=None, out: Optional[torch.Tensor] = None, select=None,
               params: Optional[torch.Tensor] = None, state: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The held-out metrics of M models in ONE launch: logits [M,B,K] fp32 (what multi_infer returns), labels [M,B] int32, counts: None or
    M host ints -- only model m's first counts[m] rows count, the rest is padding that may hold anything.  Returns `out`, M
    nsd_eval_record as device bytes (eval_records reads them).  select=dict(metric="loss" | "acc", patience=, min_delta=) with params
    [M,P] and state (select_state(M, P)) also runs the early-stopping rule of include/nsd.h per model: the record update, the patience
    count and the copy of an improved model's parameter row into the state's snapshot, all in that launch."""
    if logits.dim() != 3:
        raise NsdError(f"multi_eval: logits must be [M,B,K], got {tuple(logits.shape)}")
    M, B, K = (int(v) for v in logits.shape)
    if labels.dtype != torch.int32 or not labels.is_cuda or not labels.is_contiguous() or labels.numel() != M * B:
        raise NsdError(f"multi_eval: labels must be contiguous int32 [M,B] = [{M},{B}] on the device")
    cp = None
    if counts is not None:
        counts = [int(c) for c in counts]
        if len(counts) != M:
            raise NsdError(f"multi_eval: {len(counts)} counts for {M} models")
        cp = (C.c_int32 * M)(*counts)
    if out is None:
        out = eval_buffer(M, logits.device)
    elif out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or out.numel() != M * EVAL_RECORD_BYTES:
        raise NsdError(f"multi_eval: out must be {M * EVAL_RECORD_BYTES} contiguous bytes on the device")
    sel, pp, P, sp, sbytes = None, None, 0, None, 0
    if select is not None:
        metric = select.get("metric", "loss")
        if metric not in _lib.NSD_SELECT:
            raise NsdError(f"multi_eval: metric {metric!r}: one of {sorted(_lib.NSD_SELECT)}")
        if params is None or state is None or params.dim() != 2 or int(params.shape[0]) != M:
            raise NsdError(f"multi_eval: selection needs params [M={M},P] and a select_state")
        if state.dtype != torch.uint8 or not state.is_cuda or not state.is_contiguous():
            raise NsdError("multi_eval: state must be the contiguous device bytes of select_state")
        sel = C.byref(_lib.Select(_lib.NSD_SELECT[metric], int(select.get("patience", 0)), float(select.get("min_delta", 0.0))))
        P = int(params.shape[1])
        pp, sp, sbytes = _dev_f32(params, "params"), state.data_ptr(), _nbytes(state)
    _call("nsd_multi_eval", logits.device, M, B, K, _dev_f32(logits, "logits"), labels.data_ptr(), cp, out.data_ptr(), sel, pp, P, sp, sbytes,
          STREAM)
    return out


def _records(raw: torch.Tensor, M: int, struct, what: str):
    """M C records at the head of a device byte buffer, in one device-to-host copy"""
    n = int(M) * C.sizeof(struct)
    if raw.dtype != torch.uint8 or raw.numel() < n:
        raise NsdError(f"{what}: expected at least {n} bytes, got {raw.numel()} of {raw.dtype}")
    return (struct * int(M)).from_buffer_copy(raw[:n].cpu().numpy().tobytes())


def eval_records(out: torch.Tensor, M: int, K: int) -> List[dict]:
    """The M records multi_eval wrote: [{loss_sum, loss (mean), acc, n, correct, nonfinite, confusion [K,K] numpy}] (one copy; synchronises)."""
    import numpy as np
    recs = []
    for r in _records(out, M, _lib.EvalRecord, "eval_records"):
        n = int(r.n)
        recs.append(dict(loss_sum=float(r.loss_sum), loss=float(r.loss_sum) / n if n else float("nan"), acc=int(r.correct) / n if n else float("nan"),
                         n=n, correct=int(r.correct), nonfinite=int(r.nonfinite),
                         confusion=np.array([[r.confusion[i][j] for j in range(K)] for i in range(K)], dtype=np.int64)))
    return recs


def select_records(state: torch.Tensor, M: int) -> List[dict]:
    """The M records at the head of a select state: [{best_loss, best_correct, best_n, best_eval, evals, bad, stopped, status}] (one copy;
    synchronises)."""
    return [dict(best_loss=float(r.best_loss), best_correct=int(r.best_correct), best_n=int(r.best_n), best_eval=int(r.best_eval),
                 evals=int(r.evals), bad=int(r.bad), stopped=int(r.stopped), status=int(r.status))
            for r in _records(state, M, _lib.SelectRecord, "select_records")]


# ---- sliding-window decisions for continuous streams (nsd_window_* of include/nsd.h) ----

def _window(window: int, hop: int) -> "_lib.Window":
    return _lib.Window(int(window), int(hop))


def window_path(spec: ModelSpec, window: int, hop: int) -> bool:
    """True where nsd_window_step covers this model with this window and hop (stream_path; 1 <= hop <= window, window % hop == 0,
    window / hop <= 128)."""
    if not (-2 ** 31 <= int(window) < 2 ** 31 and -2 ** 31 <= int(hop) < 2 ** 31):
        return False
    d, w = spec.dims(1, 1), _window(window, hop)
    return spec.D == 1 and bool(_lib.lib().nsd_window_path(C.byref(d), C.byref(w)))


def window_rows(T: int, window: int, hop: int) -> int:
    """D = ceil(T / hop): the decisions a chunk of T samples can complete per stream."""
    w = _window(window, hop)
    n = int(_lib.lib().nsd_window_rows(int(T), C.byref(w)))
    if n < 0:
        check(n, "nsd_window_rows")
    return n


def window_layout(spec: ModelSpec, window: int, hop: int) -> "_lib.WindowLayout":
    """Float offsets inside one stream of a window state: `phases` phase slots of `phase_stride` floats (stream_layout slots), the int32
    words `window` and `hop`, the int64 sample `count`, and `stream_stride`."""
    d, w, lay = spec.dims(1, 1), _window(window, hop), _lib.WindowLayout()
    check(_lib.lib().nsd_window_state_layout(C.byref(d), C.byref(w), C.byref(lay)), "nsd_window_state_layout")
    return lay


def window_state(spec: ModelSpec, window: int, hop: int, S: int, device="cuda") -> torch.Tensor:
    """A reset window state of S streams on `device`: fp32 [S, stream_stride] (window_layout names the columns)."""
    d, w = spec.dims(1, 1), _window(window, hop)
    n = int(_lib.lib().nsd_window_state_bytes(C.byref(d), C.byref(w), int(S)))
    if n < 0:
        check(n, "nsd_window_state_bytes")
    state = torch.empty((int(S), n // (4 * int(S))), dtype=torch.float32, device=device)
    window_reset(spec, window, hop, state)
    return state


def window_reset(spec: ModelSpec, window: int, hop: int, state: torch.Tensor, slots: Optional[torch.Tensor] = None) -> None:
    """Reset all streams of `state`, or the ones a device int32 tensor names: every phase slot a reset stream slot, sample count 0,
    window and hop recorded in the header."""
    S = int(state.shape[0]) if state.dim() == 2 else 0
    d, w = spec.dims(0, 1), _window(window, hop)
    n = 0 if slots is None else int(slots.numel())
    if slots is not None and n == 0:
        return
    _call("nsd_window_reset", state.device, C.byref(d), C.byref(w), _dev_f32(state, "state"), _nbytes(state), S,
          _slots_ptr(slots, "window_reset"), n, STREAM)


_window_out = {}   # (device, B, D, K) -> (logits, probs, ends, counts): a chunk shape's outputs are reused, window_step allocates once


def window_step(spec: ModelSpec, flat: torch.Tensor, x: torch.Tensor, state: torch.Tensor, *, window: int, hop: int,
                slots: Optional[torch.Tensor] = None, residual: bool = False,
                out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]] = None
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Advance B continuous streams by the chunk x [B,n,C] (stream b lives in slot slots[b], or b) and return the decisions of the
    windows the chunk completed: (logits [B,D,K], probs [B,D,K], ends int64 [B,D], counts int32 [B]), D = window_rows(n).  Rows
    0 .. counts[b]-1 of stream b are its completed windows in ascending end; the others are NaN / -1; counts[b] = -1: skipped stream.
    Each row is bit for bit what stream_step gives from a reset slot on that window's samples.  out: caller-owned buffers; without
    them the buffers of this chunk shape are reused from call to call (copy what must outlive the next call)."""
    if x.dim() != 3 or x.shape[-1] != spec.C:
        raise NsdError(f"window_step: x must be [B, n, {spec.C}], got {tuple(x.shape)}")
    B, T, _ = (int(v) for v in x.shape)
    S = int(state.shape[0]) if state.dim() == 2 else 0
    if slots is not None and int(slots.numel()) != B:
        raise NsdError(f"window_step: {int(slots.numel())} slot indices for {B} streams")
    d, w = spec.dims(B, T), _window(window, hop)
    D = window_rows(T, window, hop)
    if out is None:
        key = (x.device, B, D, spec.K)
        out = _window_out.get(key)
        if out is None:
            out = _window_out[key] = (torch.empty((B, D, spec.K), dtype=torch.float32, device=x.device),
                                      torch.empty((B, D, spec.K), dtype=torch.float32, device=x.device),
                                      torch.empty((B, D), dtype=torch.int64, device=x.device),
                                      torch.empty((B,), dtype=torch.int32, device=x.device))
    logits, probs, ends, counts = out
    if (int(logits.numel()) != B * D * spec.K or int(probs.numel()) != B * D * spec.K or int(ends.numel()) != B * D or int(counts.numel()) != B
            or ends.dtype != torch.int64 or counts.dtype != torch.int32 or not ends.is_cuda or not counts.is_cuda
            or not ends.is_contiguous() or not counts.is_contiguous()):
        raise NsdError(f"window_step: out must be (logits [{B},{D},{spec.K}], probs [{B},{D},{spec.K}], ends int64 [{B},{D}], counts int32 [{B}]) "
                       "on the device")
    pp = _dev_f32(flat, "params", (spec.param_count,))
    if B == 0:
        _dev_f32(state, "state")
        return logits, probs, ends, counts
    _call("nsd_window_step", x.device, C.byref(d), C.byref(w), pp, _dev_f32(x, "x"), _slots_ptr(slots, "window_step"),
          _lib.NSD_FLAG_RESIDUAL if residual else 0, _dev_f32(state, "state"), _nbytes(state), S, _dev_f32(logits, "logits"),
          _dev_f32(probs, "probs"), ends.data_ptr(), counts.data_ptr(), STREAM)
    return logits, probs, ends, counts


# ---- sliding-window decisions of M models per launch: an ensemble on continuous streams (nsd_multi_window_* of include/nsd.h) ----

def multi_window_path(spec: ModelSpec, window: int, hop: int, M: int) -> bool:
    """True where nsd_multi_window_step covers M models of this shape with this window and hop (window_path and 1 <= M <= 32)."""
    if not (-2 ** 31 <= int(window) < 2 ** 31 and -2 ** 31 <= int(hop) < 2 ** 31 and -2 ** 31 <= int(M) < 2 ** 31):
        return False
    d, w = spec.dims(1, 1), _window(window, hop)
    return spec.D == 1 and bool(_lib.lib().nsd_multi_window_path(C.byref(d), C.byref(w), int(M)))


def multi_window_state(spec: ModelSpec, window: int, hop: int, M: int, S: int, device="cuda") -> torch.Tensor:
    """A reset window state of M models with S streams each on `device`: fp32 [M, S, stream_stride].  state[m] is an ordinary
    window_state of model m (window_step takes it as it is); the flat [M*S, stream_stride] view is what window_reset takes: stream
    m*S + s is stream s of model m."""
    d, w = spec.dims(1, 1), _window(window, hop)
    n = int(_lib.lib().nsd_multi_window_state_bytes(C.byref(d), C.byref(w), int(M), int(S)))
    if n < 0:
        check(n, "nsd_multi_window_state_bytes")
    state = torch.empty((int(M), int(S), n // (4 * int(M) * int(S))), dtype=torch.float32, device=device)
    window_reset(spec, window, hop, state.view(int(M) * int(S), -1))
    return state


_multi_window_out = {}   # (device, M, B, D, K) -> (logits, probs, mean, ends, counts): reused per chunk shape, as window_step's


def multi_window_step(spec: ModelSpec, params: torch.Tensor, x: torch.Tensor, state: torch.Tensor, *, window: int, hop: int,
                      slots: Optional[torch.Tensor] = None, residual: bool = False, want_mean: bool = True,
                      out: Optional[Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor], torch.Tensor, torch.Tensor]] = None
                      ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor], torch.Tensor, torch.Tensor]:
    """Advance B continuous streams in each of M models by one launch: params [M,P], the chunk x [B,n,C] (shared by the models) or
    [M,B,n,C], state [M,S,stream_stride]; stream b lives in stream slots[b] (or b) of every model.  Returns (logits [M,B,D,K], probs
    [M,B,D,K], mean [B,D,K], ends int64 [M,B,D], counts int32 [M,B]), D = window_rows(n): per model what window_step gives, bit for bit,
    and per row the mean of the models' probabilities (a serial fp32 sum over the models, divided by M; NaN where any model's row is;
    None with want_mean=False: no second launch).  out: caller-owned buffers (logits, probs, mean, ends, counts), mean None without
    the mean; without `out` the buffers of this chunk shape are reused from call to call (copy what must outlive the next call)."""
    if params.dim() != 2:
        raise NsdError(f"multi_window_step: params must be [M, {spec.param_count}], got {tuple(params.shape)}")
    M = int(params.shape[0])
    if x.dim() not in (3, 4) or x.shape[-1] != spec.C or (x.dim() == 4 and int(x.shape[0]) != M):
        raise NsdError(f"multi_window_step: x must be [B, n, {spec.C}] or [{M}, B, n, {spec.C}], got {tuple(x.shape)}")
    B, T = int(x.shape[-3]), int(x.shape[-2])
    stride = B * T * spec.C if x.dim() == 4 else 0
    if state.dim() != 3 or int(state.shape[0]) != M:
        raise NsdError(f"multi_window_step: state must be [{M}, S, stream_stride], got {tuple(state.shape)}")
    S = int(state.shape[1])
    if slots is not None and int(slots.numel()) != B:
        raise NsdError(f"multi_window_step: {int(slots.numel())} slot indices for {B} streams")
    d, w = spec.dims(B, T), _window(window, hop)
    D = window_rows(T, window, hop)
    if out is None:
        key = (x.device, M, B, D, spec.K)
        out = _multi_window_out.get(key)
        if out is None:
            out = _multi_window_out[key] = (torch.empty((M, B, D, spec.K), dtype=torch.float32, device=x.device),
                                            torch.empty((M, B, D, spec.K), dtype=torch.float32, device=x.device),
                                            torch.empty((B, D, spec.K), dtype=torch.float32, device=x.device),
                                            torch.empty((M, B, D), dtype=torch.int64, device=x.device),
                                            torch.empty((M, B), dtype=torch.int32, device=x.device))
    logits, probs, mean, ends, counts = out
    if not want_mean:
        mean = None
    n = M * B * D * spec.K
    if (int(logits.numel()) != n or int(probs.numel()) != n or (want_mean and (mean is None or int(mean.numel()) != B * D * spec.K))
            or int(ends.numel()) != M * B * D or int(counts.numel()) != M * B
            or ends.dtype != torch.int64 or counts.dtype != torch.int32 or not ends.is_cuda or not counts.is_cuda
            or not ends.is_contiguous() or not counts.is_contiguous()):
        raise NsdError(f"multi_window_step: out must be (logits [{M},{B},{D},{spec.K}], probs [{M},{B},{D},{spec.K}], mean [{B},{D},{spec.K}]"
                       f"{'' if want_mean else ' or None'}, ends int64 [{M},{B},{D}], counts int32 [{M},{B}]) on the device")
    pp = _dev_f32(params, "params", (M, spec.param_count))
    if B == 0:
        _dev_f32(state, "state")
        return logits, probs, mean, ends, counts
    _call("nsd_multi_window_step", x.device, C.byref(d), C.byref(w), M, pp, _dev_f32(x, "x"), stride, _slots_ptr(slots, "multi_window_step"),
          _lib.NSD_FLAG_RESIDUAL if residual else 0, _dev_f32(state, "state"), _nbytes(state), S, _dev_f32(logits, "logits"),
          _dev_f32(probs, "probs"), _dev_f32(mean, "mean"), ends.data_ptr(), counts.data_ptr(), STREAM)
    return logits, probs, mean, ends, counts


# ---- causal front end for live streams and their training (nsd_prep_* of include/nsd.h; the configuration: prep.CausalPrep) ----

def prep_path(C_: int, prep=None) -> bool:
    """True where nsd_prep_step covers C_ channels (with the CausalPrep `prep`, when given)."""
    return bool(_lib.lib().nsd_prep_path(int(C_), None if prep is None else C.cast(C.pointer(prep.struct()), C.c_void_p)))


def prep_layout(C_: int) -> "_lib.PrepLayout":
    """Float offsets of x0[C], z[4][2][C], mu[C], var[C] and the int64 sample count inside one slot, and the slot stride."""
    lay = _lib.PrepLayout()
    check(_lib.lib().nsd_prep_state_layout(int(C_), C.byref(lay)), "nsd_prep_state_layout")
    return lay


def prep_state(C_: int, S: int, device="cuda") -> torch.Tensor:
    """A reset prep state of S slots on `device`: fp32 [S, stride] (one row per stream; prep_layout names the columns)."""
    state = torch.empty((int(S), int(prep_layout(C_).stride)), dtype=torch.float32, device=device)
    prep_reset(C_, state)
    return state


def prep_reset(C_: int, state: torch.Tensor, slots: Optional[torch.Tensor] = None) -> None:
    """Reset all slots of `state`, or the ones a device int32 tensor names: filters at rest, sample count 0."""
    S = int(state.shape[0]) if state.dim() == 2 else 0
    n = 0 if slots is None else int(slots.numel())
    if slots is not None and n == 0:
        return
    _call("nsd_prep_reset", state.device, int(C_), _dev_f32(state, "state"), _nbytes(state), S, _slots_ptr(slots, "prep_reset"), n, STREAM)


def prep_step(x: torch.Tensor, prep, state: Optional[torch.Tensor] = None, *, slots: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nsd_prep_step on x [B,n,C] (or [M,B,n,C]: M*B trials).  state=None: window mode, every trial from a reset state (what the
    trainers and predict run).  state [S,stride]: stream mode, stream b advances slot slots[b] (or b) by the chunk.  out: a
    caller-owned buffer of x's size; out is x: in place."""
    if x.dim() not in (3, 4):
        raise NsdError(f"prep_step: x must be [B,n,C] or [M,B,n,C], got {tuple(x.shape)}")
    T, Cc = int(x.shape[-2]), int(x.shape[-1])
    B = int(x.numel()) // max(T * Cc, 1)
    if state is None and slots is not None:
        raise NsdError("prep_step: slots without a state")
    if slots is not None and int(slots.numel()) != B:
        raise NsdError(f"prep_step: {int(slots.numel())} slot indices for {B} streams")
    if out is None:
        out = torch.empty_like(x)
    if out.numel() != x.numel():
        raise NsdError(f"prep_step: out has {out.numel()} elements for {tuple(x.shape)}")
    if B == 0:
        return out
    S = 0 if state is None else (int(state.shape[0]) if state.dim() == 2 else 0)
    d, p = Dims(B, T, Cc, 1, 1, 1, 1), prep.struct()
    _call("nsd_prep_step", x.device, C.byref(d), C.cast(C.pointer(p), C.c_void_p), _dev_f32(x, "x"), _slots_ptr(slots, "prep_step"),
          _dev_f32(state, "state"), 0 if state is None else _nbytes(state), S, _dev_f32(out, "out"), STREAM)
    return out


# ---- rate conversion, stage 0 of the front end (nsd_resample_* of include/nsd.h; the configuration: resample.Resample) ----

def _resample_ptr(resample):
    return C.cast(C.pointer(resample.struct()), C.c_void_p)


def resample_path(C_: int, resample=None) -> bool:
    """True where nsd_resample_step covers C_ channels (with the Resample `resample`, when given)."""
    return bool(_lib.lib().nsd_resample_path(int(C_), None if resample is None else _resample_ptr(resample)))


def resample_out_steps(resample, n_in: int, T: int) -> int:
    """Outputs a call that adds T samples to a stream holding n_in emits: ceil((n_in+T) L / M) - ceil(n_in L / M)."""
    n = int(_lib.lib().nsd_resample_out_steps(_resample_ptr(resample), int(n_in), int(T)))
    if n < 0:
        check(n, "nsd_resample_out_steps")
    return n


def resample_layout(C_: int, resample) -> "_lib.ResampleLayout":
    """Offsets, in 4-byte words, of hist[P-1][C] (fp32) and the int64 n_in inside one slot, and the slot stride."""
    lay = _lib.ResampleLayout()
    check(_lib.lib().nsd_resample_state_layout(int(C_), _resample_ptr(resample), C.byref(lay)), "nsd_resample_state_layout")
    return lay


def resample_state(C_: int, resample, S: int, device="cuda") -> torch.Tensor:
    """A reset resample state of S slots on `device`: [S, stride] 4-byte words carried as float32 (one row per stream; resample_layout
    names the columns, n_in is a bit pattern: read it through .view(torch.int64))."""
    state = torch.empty((int(S), int(resample_layout(C_, resample).stride)), dtype=torch.float32, device=device)
    resample_reset(C_, resample, state)
    return state


def resample_reset(C_: int, resample, state: torch.Tensor, slots: Optional[torch.Tensor] = None) -> None:
    """Reset all slots of `state`, or the ones a device int32 tensor names: everything zero."""
    S = int(state.shape[0]) if state.dim() == 2 else 0
    n = 0 if slots is None else int(slots.numel())
    if slots is not None and n == 0:
        return
    _call("nsd_resample_reset", state.device, int(C_), _resample_ptr(resample), _dev_f32(state, "state"), _nbytes(state), S,
          _slots_ptr(slots, "resample_reset"), n, STREAM)


def resample_step(x: torch.Tensor, resample, state: Optional[torch.Tensor] = None, *, slots: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None, cnt: Optional[torch.Tensor] = None, taps: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nsd_resample_step on x [B,n,C] (or [M,B,n,C]: M*B trials) -> y [B,To,C].  state=None: window mode, every trial from rest and
    To = ceil(n L / M).  state [S,stride]: stream mode, stream b advances slot slots[b] (or b) by the chunk; row b of y holds its
    outputs and NaN behind them, cnt (device int32 [B], optional) their number.  out: a caller-owned buffer [..,To,C] with
    To >= ceil(n L / M) (window mode: equal).  taps: the device table, default the Resample's own on x's device."""
    if x.dim() not in (3, 4):
        raise NsdError(f"resample_step: x must be [B,n,C] or [M,B,n,C], got {tuple(x.shape)}")
    T, Cc = int(x.shape[-2]), int(x.shape[-1])
    B = int(x.numel()) // max(T * Cc, 1)
    if state is None and slots is not None:
        raise NsdError("resample_step: slots without a state")
    if slots is not None and int(slots.numel()) != B:
        raise NsdError(f"resample_step: {int(slots.numel())} slot indices for {B} streams")
    if out is None:
        out = torch.empty(tuple(x.shape[:-2]) + (-((-T * resample.L) // resample.M), Cc), dtype=torch.float32, device=x.device)
    if out.dim() != x.dim() or tuple(out.shape[:-2]) != tuple(x.shape[:-2]) or int(out.shape[-1]) != Cc:
        raise NsdError(f"resample_step: out of shape {tuple(out.shape)} for x {tuple(x.shape)}")
    if cnt is not None and (cnt.dtype != torch.int32 or not cnt.is_cuda or not cnt.is_contiguous() or int(cnt.numel()) != B):
        raise NsdError(f"resample_step: cnt must be a contiguous int32 tensor of {B} counts on the device")
    if B == 0:
        return out
    if taps is None:
        taps = resample.device_taps(x.device)
    S = 0 if state is None else (int(state.shape[0]) if state.dim() == 2 else 0)
    d = Dims(B, T, Cc, 1, 1, 1, 1)
    _call("nsd_resample_step", x.device, C.byref(d), _resample_ptr(resample), _dev_f32(taps, "taps", (resample.L, resample.P)),
          _dev_f32(x, "x"), _slots_ptr(slots, "resample_step"), _dev_f32(state, "state"), 0 if state is None else _nbytes(state), S,
          _dev_f32(out, "out"), int(out.shape[-2]), None if cnt is None else cnt.data_ptr(), STREAM)
    return out


def resample_trials(x: torch.Tensor, resample) -> torch.Tensor:
    """Whole trials x [B,n,C] (or [M,B,n,C]) at the amplifier's rate -> [.., ceil(n L / M), C] at the models': window mode, every
    trial from rest."""
    return resample_step(x, resample)


# ---- signal-quality gate around the front end (nsd_gate_* of include/nsd.h; the configuration: gate.SignalGate) ----

def gate_path(C_: int, gate=None) -> bool:
    """True where nsd_gate_step covers C_ channels (with the SignalGate `gate`, when given)."""
    return bool(_lib.lib().nsd_gate_path(int(C_), None if gate is None else C.cast(C.pointer(gate.struct()), C.c_void_p)))


def gate_layout(C_: int) -> "_lib.GateLayout":
    """Offsets, in 4-byte words, of prev[C], held[C] (fp32), run[C], hang[C] (int32), ring[64][C] (fp32), bad[C], rejected and steps
    (int64) inside one slot, and the slot stride."""
    lay = _lib.GateLayout()
    check(_lib.lib().nsd_gate_state_layout(int(C_), C.byref(lay)), "nsd_gate_state_layout")
    return lay


def gate_state(C_: int, S: int, device="cuda") -> torch.Tensor:
    """A reset gate state of S slots on `device`: [S, stride] 4-byte words carried as float32 (one row per stream; gate_layout names
    the columns, the integer ones are bit patterns: read them through .view(torch.int32) / .view(torch.int64))."""
    state = torch.empty((int(S), int(gate_layout(C_).stride)), dtype=torch.float32, device=device)
    gate_reset(C_, state)
    return state


def gate_reset(C_: int, state: torch.Tensor, slots: Optional[torch.Tensor] = None) -> None:
    """Reset all slots of `state`, or the ones a device int32 tensor names: everything zero."""
    S = int(state.shape[0]) if state.dim() == 2 else 0
    n = 0 if slots is None else int(slots.numel())
    if slots is not None and n == 0:
        return
    _call("nsd_gate_reset", state.device, int(C_), _dev_f32(state, "state"), _nbytes(state), S, _slots_ptr(slots, "gate_reset"), n, STREAM)


def _mask_ptr(mask: torch.Tensor, what: str, steps: int) -> int:
    if mask.dtype != torch.int32 or not mask.is_cuda or not mask.is_contiguous() or int(mask.numel()) != steps:
        raise NsdError(f"{what}: mask must be a contiguous int32 tensor of {steps} words (one per step) on the device")
    return mask.data_ptr()


def gate_step(x: torch.Tensor, gate, state: Optional[torch.Tensor] = None, *, slots: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """nsd_gate_step on x [B,n,C] (or [M,B,n,C]: M*B trials) -> (y, mask): y of x's shape with every bad channel held at its last good
    value, mask int32 [B,n] (the bits of the uint32 word: bit c set where channel c is bad).  state=None: window mode, every trial from
    a reset state.  state [S,stride]: stream mode, stream b advances slot slots[b] (or b) by the chunk.  out, mask: caller-owned
    buffers; out is x: in place."""
    if x.dim() not in (3, 4):
        raise NsdError(f"gate_step: x must be [B,n,C] or [M,B,n,C], got {tuple(x.shape)}")
    T, Cc = int(x.shape[-2]), int(x.shape[-1])
    B = int(x.numel()) // max(T * Cc, 1)
    if state is None and slots is not None:
        raise NsdError("gate_step: slots without a state")
    if slots is not None and int(slots.numel()) != B:
        raise NsdError(f"gate_step: {int(slots.numel())} slot indices for {B} streams")
    if out is None:
        out = torch.empty_like(x)
    if out.numel() != x.numel():
        raise NsdError(f"gate_step: out has {out.numel()} elements for {tuple(x.shape)}")
    if mask is None:
        mask = torch.empty(tuple(x.shape[:-1]), dtype=torch.int32, device=x.device)
    if B == 0:
        return out, mask
    S = 0 if state is None else (int(state.shape[0]) if state.dim() == 2 else 0)
    d, g = Dims(B, T, Cc, 1, 1, 1, 1), gate.struct()
    _call("nsd_gate_step", x.device, C.byref(d), C.cast(C.pointer(g), C.c_void_p), _dev_f32(x, "x"), _slots_ptr(slots, "gate_step"),
          _dev_f32(state, "state"), 0 if state is None else _nbytes(state), S, _dev_f32(out, "out"), _mask_ptr(mask, "gate_step", B * T),
          STREAM)
    return out, mask


def gate_apply(v: torch.Tensor, gate, mask: torch.Tensor, *, out: Optional[torch.Tensor] = None,
               max_bad: Optional[int] = None) -> torch.Tensor:
    """nsd_gate_apply on v [B,n,C] (or [M,B,n,C]) behind the front end with gate_step's mask: a step with more than max_bad (default:
    the gate's) bad channels is NaN, else a bad channel is 0 where the gate zeroes and everything else a bitwise copy.  out is v: in
    place."""
    if v.dim() not in (3, 4):
        raise NsdError(f"gate_apply: v must be [B,n,C] or [M,B,n,C], got {tuple(v.shape)}")
    T, Cc = int(v.shape[-2]), int(v.shape[-1])
    B = int(v.numel()) // max(T * Cc, 1)
    if out is None:
        out = torch.empty_like(v)
    if out.numel() != v.numel():
        raise NsdError(f"gate_apply: out has {out.numel()} elements for {tuple(v.shape)}")
    if B == 0:
        return out
    d, g = Dims(B, T, Cc, 1, 1, 1, 1), gate.struct()
    if max_bad is not None:
        g.max_bad = int(max_bad)
    _call("nsd_gate_apply", v.device, C.byref(d), C.cast(C.pointer(g), C.c_void_p), _dev_f32(v, "v"), _mask_ptr(mask, "gate_apply", B * T),
          _dev_f32(out, "out"), STREAM)
    return out


def gate_quality(C_: int, state: torch.Tensor, slots=None) -> dict:
    """The counters of a gate state, read in one copy: {"bad_fraction": [n,C], "rejected_fraction": [n], "steps": [n]} (numpy) for all
    slots, or the listed ones.  A slot with no samples reports fractions of 0."""
    import numpy as np
    lay = gate_layout(C_)
    lo, hi = int(lay.bad), int(lay.steps) + 2
    rows = state if slots is None else state[torch.as_tensor(list(slots), dtype=torch.long, device=state.device)]
    words = rows[:, lo:hi].contiguous().cpu().numpy().view(np.int64)          # bad[C], rejected, steps
    steps = words[:, int(C_) + 1].copy()
    n = np.maximum(steps, 1).astype(np.float64)
    return {"bad_fraction": words[:, :int(C_)] / n[:, None], "rejected_fraction": words[:, int(C_)] / n, "steps": steps}


# ---- session alignment: channel covariance, whitening fit, spatial apply (nsd_cov_* / nsd_whiten_fit / nsd_spatial_apply of
# include/nsd.h; the configuration: align.SessionAlign) ----

def _dev_typed(t: Optional[torch.Tensor], name: str, dtype, numel: Optional[int] = None) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or (numel is not None and int(t.numel()) != int(numel)):
        raise NsdError(f"{name}: expected a contiguous {dtype} tensor{'' if numel is None else f' of {numel} elements'} on the device, "
                       f"got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t.data_ptr()


def cov_layout(C_: int) -> "_lib.CovLayout":
    """Offsets, in 8-byte words, of sum[C][C] (double), count and skipped (int64) inside one slot of a cov state, and the slot stride."""
    lay = _lib.CovLayout()
    check(_lib.lib().nsd_cov_state_layout(int(C_), C.byref(lay)), "nsd_cov_state_layout")
    return lay


def cov_state(C_: int, S: int, device="cuda") -> torch.Tensor:
    """A reset cov state of S slots on `device`: [S, C*C + 2] 8-byte words carried as float64 (the two counts are bit patterns: read
    them through .view(torch.int64), or with cov_counts)."""
    state = torch.empty((int(S), int(cov_layout(C_).stride)), dtype=torch.float64, device=device)
    cov_reset(C_, state)
    return state


def cov_reset(C_: int, state: torch.Tensor, slots: Optional[torch.Tensor] = None) -> None:
    """Reset all slots of `state`, or the ones a device int32 tensor names: everything zero."""
    S = int(state.shape[0]) if state.dim() == 2 else 0
    n = 0 if slots is None else int(slots.numel())
    if slots is not None and n == 0:
        return
    _call("nsd_cov_reset", state.device, int(C_), _dev_typed(state, "cov_reset: state", torch.float64), _nbytes(state), S,
          _slots_ptr(slots, "cov_reset"), n, STREAM)


def cov_step(v: torch.Tensor, state: Optional[torch.Tensor] = None, *, mask: Optional[torch.Tensor] = None,
             slots: Optional[torch.Tensor] = None, out=None):
    """nsd_cov_step on v [B,n,C] (or [M,B,n,C]: M*B trials), with the gate's mask int32 [B,n] where given.  state=None: window mode ->
    (sums float64 [B,C,C], counts int64 [B,2]: {used, skipped}) from zero for every trial (out: the two caller-owned buffers).
    state [S, C*C+2]: stream mode, stream b adds the chunk to slot slots[b] (or b); returns the state."""
    if v.dim() not in (3, 4):
        raise NsdError(f"cov_step: v must be [B,n,C] or [M,B,n,C], got {tuple(v.shape)}")
    T, Cc = int(v.shape[-2]), int(v.shape[-1])
    B = int(v.numel()) // max(T * Cc, 1)
    if state is None and slots is not None:
        raise NsdError("cov_step: slots without a state")
    if slots is not None and int(slots.numel()) != B:
        raise NsdError(f"cov_step: {int(slots.numel())} slot indices for {B} streams")
    if state is not None and out is not None:
        raise NsdError("cov_step: out with a state (stream mode keeps the sums in the state)")
    sums = counts = None
    if state is None:
        if out is None:
            out = (torch.empty((B, Cc, Cc), dtype=torch.float64, device=v.device), torch.empty((B, 2), dtype=torch.int64, device=v.device))
        sums, counts = out
    if B > 0:
        S = 0 if state is None else (int(state.shape[0]) if state.dim() == 2 else 0)
        d = Dims(B, T, Cc, 1, 1, 1, 1)
        _call("nsd_cov_step", v.device, C.byref(d), _dev_f32(v, "v"), None if mask is None else _mask_ptr(mask, "cov_step", B * T),
              _slots_ptr(slots, "cov_step"), _dev_typed(state, "cov_step: state", torch.float64), 0 if state is None else _nbytes(state), S,
              _dev_typed(sums, "cov_step: sums", torch.float64, B * Cc * Cc), _dev_typed(counts, "cov_step: counts", torch.int64, B * 2), STREAM)
    return state if state is not None else (sums, counts)


def cov_counts(C_: int, state: torch.Tensor, slots=None):
    """{used, skipped} of a cov state's slots (all, or the listed ones) as int64 numpy [n,2], in one copy."""
    lay = cov_layout(C_)
    rows = state if slots is None else state[torch.as_tensor(list(slots), dtype=torch.long, device=state.device)]
    return rows[:, int(lay.count):int(lay.count) + 2].contiguous().view(torch.int64).cpu().numpy()


WHITEN_RECORD_BYTES = C.sizeof(_lib.WhitenRecord)
WHITEN_STATUS = {"few": _lib.NSD_WHITEN_FEW, "nonfinite": _lib.NSD_WHITEN_NONFINITE, "clipped": _lib.NSD_WHITEN_CLIPPED,
                 "not_converged": _lib.NSD_WHITEN_NOT_CONVERGED}


def whiten_fit(C_: int, align, sums: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None, *,
               state: Optional[torch.Tensor] = None, group: Optional[torch.Tensor] = None, G: int = 1,
               out: Optional[torch.Tensor] = None, records: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """nsd_whiten_fit with the SessionAlign `align`: one matrix per group from N accumulators -> (W float32 [G,C,C], records: a uint8
    buffer of G nsd_whiten_record, read with whiten_records).  The accumulators are window-mode outputs (sums float64 [N,C,C], counts
    int64 [N,2]) or a cov state [N, C*C+2] read in place (state=).  group: device int32 [N] (None: all in group 0).  Nothing is read
    back: the call can be captured (out, records: caller-owned buffers)."""
    Cc, G = int(C_), int(G)
    if (state is None) == (sums is None) or (sums is None) != (counts is None):
        raise NsdError("whiten_fit: give either sums and counts, or state")
    if state is not None:
        lay = cov_layout(Cc)
        if state.dim() != 2 or int(state.shape[1]) != int(lay.stride):
            raise NsdError(f"whiten_fit: state must be [N, {int(lay.stride)}], got {tuple(state.shape)}")
        N, dev = int(state.shape[0]), state.device
        base = _dev_typed(state, "whiten_fit: state", torch.float64)
        sp, ss, cp, cs = base, int(lay.stride), (None if base is None else base + 8 * int(lay.count)), int(lay.stride)
    else:
        N, dev = int(counts.numel()) // 2, sums.device
        sp, ss = _dev_typed(sums, "whiten_fit: sums", torch.float64, N * Cc * Cc), Cc * Cc
        cp, cs = _dev_typed(counts, "whiten_fit: counts", torch.int64, N * 2), 2
    if N == 0:
        sp = cp = None
    if group is not None and (group.dtype != torch.int32 or not group.is_cuda or not group.is_contiguous() or int(group.numel()) != N):
        raise NsdError(f"whiten_fit: group must be a contiguous int32 tensor of {N} indices on the device")
    if out is None:
        out = torch.empty((G, Cc, Cc), dtype=torch.float32, device=dev)
    if records is None:
        records = torch.empty(max(G, 1) * C.sizeof(_lib.WhitenRecord), dtype=torch.uint8, device=dev)
    if int(out.numel()) != G * Cc * Cc or records.dtype != torch.uint8 or int(records.numel()) < G * C.sizeof(_lib.WhitenRecord) \
            or not records.is_cuda or not records.is_contiguous():
        raise NsdError(f"whiten_fit: out must hold [{G},{Cc},{Cc}] float32 and records {G * C.sizeof(_lib.WhitenRecord)} bytes (uint8) on the device")
    w = align.struct(Cc)
    _call("nsd_whiten_fit", dev, Cc, C.byref(w), sp, ss, cp, cs, N, None if group is None or N == 0 else group.data_ptr(), G,
          _dev_f32(out, "whiten_fit: out"), records.data_ptr(), STREAM)
    return out, records


def whiten_records(records: torch.Tensor, G: int) -> List[dict]:
    """The G records whiten_fit wrote: [{steps, skipped, trace_mean, eig_min, eig_max, sweeps, status, accumulators, ignored, and one
    bool per status bit: few, nonfinite, clipped, not_converged}] (one copy; synchronises)."""
    recs = []
    for r in _records(records, G, _lib.WhitenRecord, "whiten_records"):
        d = dict(steps=int(r.steps), skipped=int(r.skipped), trace_mean=float(r.trace_mean), eig_min=float(r.eig_min),
                 eig_max=float(r.eig_max), sweeps=int(r.sweeps), status=int(r.status), accumulators=int(r.accumulators),
                 ignored=int(r.ignored))
        d.update({name: bool(d["status"] & bit) for name, bit in WHITEN_STATUS.items()})
        recs.append(d)
    return recs


def spatial_apply(v: torch.Tensor, W: torch.Tensor, *, sel: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nsd_spatial_apply on v [B,n,C] (or [M,B,n,C]: M*B rows): out[b,t,:] = W[sel[b]] . v[b,t,:], the sum over the input channel taken
    serially in fp32.  W [C,C] or [n_mat,C,C]; sel: device int32 [B] (None: matrix 0 for every row; an entry outside the table gives
    NaN rows).  out is v: in place."""
    if v.dim() not in (3, 4):
        raise NsdError(f"spatial_apply: v must be [B,n,C] or [M,B,n,C], got {tuple(v.shape)}")
    T, Cc = int(v.shape[-2]), int(v.shape[-1])
    B = int(v.numel()) // max(T * Cc, 1)
    if W.dim() not in (2, 3) or tuple(W.shape[-2:]) != (Cc, Cc):
        raise NsdError(f"spatial_apply: W must be [{Cc},{Cc}] or [n_mat,{Cc},{Cc}], got {tuple(W.shape)}")
    n_mat = 1 if W.dim() == 2 else int(W.shape[0])
    if sel is not None and (sel.dtype != torch.int32 or not sel.is_cuda or not sel.is_contiguous() or int(sel.numel()) != B):
        raise NsdError(f"spatial_apply: sel must be a contiguous int32 tensor of {B} indices on the device")
    if torch.is_grad_enabled() and (v.requires_grad or W.requires_grad):
        # somebody differentiates through the stage: the same launch as an autograd node, nsd_spatial_bwd behind it
        if out is not None:
            raise NsdError("spatial_apply: out= with a gradient requested (v or W requires grad) -- the node owns its output")
        return _SpatialApply.apply(v, W, sel)
    return _spatial_apply(v, W, sel, out)


def _spatial_apply(v: torch.Tensor, W: torch.Tensor, sel: Optional[torch.Tensor], out: Optional[torch.Tensor]) -> torch.Tensor:
    """the launch of spatial_apply on checked arguments"""
    T, Cc = int(v.shape[-2]), int(v.shape[-1])
    B = int(v.numel()) // max(T * Cc, 1)
    n_mat = 1 if W.dim() == 2 else int(W.shape[0])
    if out is None:
        out = torch.empty_like(v)
    if out.numel() != v.numel():
        raise NsdError(f"spatial_apply: out has {out.numel()} elements for {tuple(v.shape)}")
    if B == 0:
        return out
    d = Dims(B, T, Cc, 1, 1, 1, 1)
    _call("nsd_spatial_apply", v.device, C.byref(d), _dev_f32(v, "v"), _dev_f32(W, "W"), n_mat, None if sel is None else sel.data_ptr(),
          _dev_f32(out, "out"), STREAM)
    return out


class _SpatialApply(torch.autograd.Function):
    """nsd_spatial_apply as an autograd node: backward is nsd_spatial_bwd (dv = W^T . dy serially in fp32; dW in two fixed double stages)."""

    @staticmethod
    def forward(ctx, v, W, sel):
        vc = v.detach().contiguous()
        ctx.save_for_backward(vc, W.detach().contiguous())
        ctx.sel = sel
        return _spatial_apply(vc, W.detach().contiguous(), sel, None)

    @staticmethod
    def backward(ctx, dy):
        v, W = ctx.saved_tensors
        dv, dW, _ = spatial_bwd(v, dy.contiguous().float(), W, sel=ctx.sel, want_dv=ctx.needs_input_grad[0], want_dW=ctx.needs_input_grad[1])
        return dv, (None if dW is None else dW.view(W.shape)), None


def spatial_bwd_scratch_bytes(B: int, T: int, C_: int) -> int:
    """nsd_spatial_bwd_scratch_bytes: stage 1 of dW, B * C * C doubles"""
    d = Dims(int(B), int(T), int(C_), 1, 1, 1, 1)
    n = int(_lib.lib().nsd_spatial_bwd_scratch_bytes(C.byref(d)))
    if n < 0:
        check(n, "nsd_spatial_bwd_scratch_bytes")
    return n


def spatial_bwd(v: torch.Tensor, dy: torch.Tensor, W: torch.Tensor, *, sel: Optional[torch.Tensor] = None, want_dv: bool = True,
                want_dW: bool = True, dv: Optional[torch.Tensor] = None, dW: Optional[torch.Tensor] = None,
                counts: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None):
    """nsd_spatial_bwd, the backward of spatial_apply: v, dy [B,n,C] (or [M,B,n,C]), W [C,C] or [n_mat,C,C], sel as in the apply ->
    (dv [B,n,C] or None, dW [n_mat,C,C] or None, counts int64 [2] {rows used, rows left out} or None).  dv[b,t,j] = sum_i W[i][j]
    dy[b,t,i] serially in fp32; dW[m] = the sum over the rows with sel == m and over t of dy (x) v, one double chain over t per row, then
    one over the rows, rounded once.  dv / dW / counts / scratch (float64, B*C*C elements): caller-owned buffers; nothing is read back."""
    if v.dim() not in (3, 4) or tuple(dy.shape) != tuple(v.shape):
        raise NsdError(f"spatial_bwd: v and dy must be [B,n,C] or [M,B,n,C] of one shape, got {tuple(v.shape)} and {tuple(dy.shape)}")
    T, Cc = int(v.shape[-2]), int(v.shape[-1])
    B = int(v.numel()) // max(T * Cc, 1)
    if W.dim() not in (2, 3) or tuple(W.shape[-2:]) != (Cc, Cc):
        raise NsdError(f"spatial_bwd: W must be [{Cc},{Cc}] or [n_mat,{Cc},{Cc}], got {tuple(W.shape)}")
    n_mat = 1 if W.dim() == 2 else int(W.shape[0])
    if sel is not None and (sel.dtype != torch.int32 or not sel.is_cuda or not sel.is_contiguous() or int(sel.numel()) != B):
        raise NsdError(f"spatial_bwd: sel must be a contiguous int32 tensor of {B} indices on the device")
    want_dv, want_dW = want_dv or dv is not None, want_dW or dW is not None
    if not (want_dv or want_dW):
        return None, None, None
    if want_dv and dv is None:
        dv = torch.empty_like(v)
    if want_dW:
        if dW is None:
            dW = torch.empty((n_mat, Cc, Cc), dtype=torch.float32, device=v.device)
        if counts is None:
            counts = torch.empty(2, dtype=torch.int64, device=v.device)
        if scratch is None:
            scratch = torch.empty(max(B * Cc * Cc, 1), dtype=torch.float64, device=v.device)
        if int(dW.numel()) != n_mat * Cc * Cc:
            raise NsdError(f"spatial_bwd: dW has {int(dW.numel())} elements for [{n_mat},{Cc},{Cc}]")
    else:
        counts = scratch = None
    if want_dv and int(dv.numel()) != int(v.numel()):
        raise NsdError(f"spatial_bwd: dv has {int(dv.numel())} elements for {tuple(v.shape)}")
    d = Dims(B, T, Cc, 1, 1, 1, 1)
    _call("nsd_spatial_bwd", v.device, C.byref(d), _dev_f32(v, "v"), _dev_f32(dy, "dy"), _dev_f32(W, "W"), n_mat,
          None if sel is None else sel.data_ptr(), _dev_f32(dv, "dv"), _dev_f32(dW, "dW"),
          _dev_typed(counts, "spatial_bwd: counts", torch.int64, 2), _dev_typed(scratch, "spatial_bwd: scratch", torch.float64),
          0 if scratch is None else _nbytes(scratch), STREAM)
    return dv, dW, counts


SPATIAL_FIT_NONFINITE = _lib.NSD_SPATIAL_FIT_NONFINITE


def spatial_fit_layout(C_: int) -> "_lib.SpatialFitLayout":
    """Offsets, in bytes, of m, v (float [C,C]), step, skipped (int64) and status (uint32) inside one matrix's slot of a fit state, and the
    slot stride; the int64 call counter follows the last slot."""
    lay = _lib.SpatialFitLayout()
    check(_lib.lib().nsd_spatial_fit_state_layout(int(C_), C.byref(lay)), "nsd_spatial_fit_state_layout")
    return lay


def spatial_fit_state(C_: int, n_mat: int = 1, device="cuda") -> torch.Tensor:
    """A reset fit state of n_mat matrices: zero bytes (uint8 [nsd_spatial_fit_state_bytes]); all-zero is the reset state."""
    n = int(_lib.lib().nsd_spatial_fit_state_bytes(int(C_), int(n_mat)))
    if n < 0:
        check(n, "nsd_spatial_fit_state_bytes")
    return torch.zeros(n // 8, dtype=torch.int64, device=device).view(torch.uint8)       # (8-byte aligned whatever the allocator does)


def spatial_fit_records(C_: int, n_mat: int, state: torch.Tensor) -> List[dict]:
    """Per matrix {step, skipped, status, m [C,C], v [C,C] numpy} of a fit state, and "calls" in every record (one copy; synchronises)."""
    import numpy as np
    lay, Cc = spatial_fit_layout(C_), int(C_)
    raw = state.detach().view(torch.uint8).cpu().numpy()
    calls = int(raw[int(n_mat) * int(lay.stride):][:8].view(np.int64)[0])
    recs = []
    for m in range(int(n_mat)):
        s = raw[m * int(lay.stride):(m + 1) * int(lay.stride)]
        recs.append(dict(step=int(s[int(lay.step):][:8].view(np.int64)[0]), skipped=int(s[int(lay.skipped):][:8].view(np.int64)[0]),
                         status=int(s[int(lay.status):][:4].view(np.uint32)[0]), calls=calls,
                         m=s[int(lay.m):][:4 * Cc * Cc].view(np.float32).reshape(Cc, Cc).copy(),
                         v=s[int(lay.v):][:4 * Cc * Cc].view(np.float32).reshape(Cc, Cc).copy()))
    return recs


def spatial_fit_step(A: torch.Tensor, dW: torch.Tensor, state: torch.Tensor, *, A0: Optional[torch.Tensor] = None, lr: float = 1e-2,
                     beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, decay: float = 0.0,
                     loss_in: Optional[torch.Tensor] = None, loss_out: Optional[torch.Tensor] = None) -> None:
    """nsd_spatial_fit_step: one Adam step on A [C,C] or [n_mat,C,C] in place from dW, with g = dW + decay * (A - A0) (A0 None: no
    pull).  state: ops.spatial_fit_state; its counters advance on the device (the call can be captured).  A matrix whose g is not finite
    stays as it is and records it (spatial_fit_records).  loss_in (device float [1]) is copied to loss_out[call] while call < len(loss_out)."""
    if A.dim() not in (2, 3) or A.shape[-1] != A.shape[-2]:
        raise NsdError(f"spatial_fit_step: A must be [C,C] or [n_mat,C,C], got {tuple(A.shape)}")
    Cc, n_mat = int(A.shape[-1]), (1 if A.dim() == 2 else int(A.shape[0]))
    if int(dW.numel()) != int(A.numel()) or (A0 is not None and int(A0.numel()) != int(A.numel())):
        raise NsdError(f"spatial_fit_step: dW / A0 must hold {int(A.numel())} elements as A does")
    if (loss_in is None) != (loss_out is None):
        raise NsdError("spatial_fit_step: loss_in and loss_out go together")
    fit = _lib.SpatialFitCfg(float(lr), float(beta1), float(beta2), float(eps), float(decay))
    _call("nsd_spatial_fit_step", A.device, Cc, n_mat, _dev_f32(A, "A"), _dev_f32(A0, "A0"), _dev_f32(dW, "dW"), C.byref(fit),
          _dev_typed(state, "spatial_fit_step: state", torch.uint8), _nbytes(state), _dev_f32(loss_in, "loss_in"),
          _dev_f32(loss_out, "loss_out"), 0 if loss_out is None else int(loss_out.numel()), STREAM)


def train_dx(spec: ModelSpec, flat: torch.Tensor, x: torch.Tensor, ws: torch.Tensor, logits: torch.Tensor, dx: torch.Tensor, *,
             labels: Optional[torch.Tensor] = None, targets: Optional[torch.Tensor] = None, scale: Optional[float] = None,
             rrelu_slope: Optional[torch.Tensor] = None, residual: bool = False, loss_out: Optional[torch.Tensor] = None) -> None:
    """The input gradient of the mean loss through a FROZEN model: nsd_lstm_head_train[_soft] -> nsd_lstm_bwd with dx -> nsd_loss_sum
    (where loss_out, a device float [1], is given).  No dropout; rrelu_slope [B,F] are the explicit slopes (the eval slope for an
    eval-mode pass).  The parameter-gradient slabs stay in the workspace unreduced: `flat` is read, never written.  Needs dx_path."""
    B, T, _ = x.shape
    if not dx_path(spec, B, T):
        raise NsdError(f"train_dx: {spec} at batch {B} is outside nsd_dx_path (hidden size 48, 2 layers, <= 8 channels on the fast path)")
    d = spec.dims(B, T)
    flags = _lib.NSD_FLAG_TRAIN | (_lib.NSD_FLAG_RESIDUAL if residual else 0) | _extra_flags
    pp = _dev_f32(flat, "params", (spec.param_count,))
    xp, wsp, wsn, dev = _dev_f32(x, "x", (B, T, spec.C)), _dev_f32(ws, "workspace"), _nbytes(ws), x.device
    sl, lp = _dev_f32(rrelu_slope, "rrelu_slope", (B, spec.F)), _dev_f32(logits, "logits", (B, spec.K))
    scale = (1.0 / max(B, 1)) if scale is None else float(scale)
    if targets is not None:
        _call("nsd_lstm_head_train_soft", dev, C.byref(d), pp, xp, None, sl, None, None, _dev_f32(targets, "targets", (B, spec.K)), scale,
              flags, wsp, wsn, lp, STREAM)
    else:
        _call("nsd_lstm_head_train", dev, C.byref(d), pp, xp, None, sl, None, _labels_ptr(labels), scale, flags, wsp, wsn, lp, STREAM)
    _call("nsd_lstm_bwd", dev, C.byref(d), pp, xp, None, flags, wsp, wsn, _dev_f32(dx, "dx", (B, T, spec.C)), STREAM)
    if loss_out is not None:
        _call("nsd_loss_sum", dev, C.byref(d), wsp, wsn, _dev_f32(loss_out, "loss_out"), STREAM)
