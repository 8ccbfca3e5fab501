"""Drop-in counterpart of the reference's Neuro-Alpha-App/Utilities/lstm_eeg_model.py, running on MI355X.

Same public names, constructor signatures, defaults and state_dict keys as the reference
(`EEG_LSTM` lstm_eeg_model.py:13-39, `SimplePredictor` :42-101, `CLASS_NAMES` :11), so the reference's
checkpoint loads with strict=True and `tester.run_trials` / the Streamlit app can import this module
instead.  The arithmetic is NOT torch's: forward / backward call the hand-written HIP kernels of
libnsd_hip.so through the C ABI (include/nsd.h).  The nn.Linear / nn.LayerNorm sub-modules below only
hold parameters under the reference's names; their own forward() is never used.

There is no CPU implementation: parameters and inputs must be on the GPU, otherwise forward raises.
"""
from __future__ import annotations

import importlib
import importlib.util
import math
import warnings
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import ops, step_recipe as sr
from ._lib import NsdError
from .gate import SignalGate
from .align import SessionAlign
from .prep import CausalPrep
from .resample import Resample

CLASS_NAMES = ["Food", "Water", "BG-Noise"]   # verbatim from lstm_eeg_model.py:11


class _StackedLSTMParams(nn.Module):
    """Parameter container with torch.nn.LSTM's parameter names, shapes and default init."""

    def __init__(self, input_size: int, hidden_size: int, num_layers: int, bidirectional: bool = False):
        super().__init__()
        self.input_size, self.hidden_size, self.num_layers = input_size, hidden_size, num_layers
        self.bidirectional = bool(bidirectional)
        k = 1.0 / math.sqrt(hidden_size)
        D = 2 if bidirectional else 1
        for l in range(num_layers):
            I = input_size if l == 0 else D * hidden_size
            for sfx in (("", "_reverse") if bidirectional else ("",)):         # torch.nn.LSTM's registration order
                for name, shape in ((f"weight_ih_l{l}{sfx}", (4 * hidden_size, I)), (f"weight_hh_l{l}{sfx}", (4 * hidden_size, hidden_size)),
                                    (f"bias_ih_l{l}{sfx}", (4 * hidden_size,)), (f"bias_hh_l{l}{sfx}", (4 * hidden_size,))):
                    self.register_parameter(name, nn.Parameter(torch.empty(shape).uniform_(-k, k)))

    def extra_repr(self) -> str:
        return (f"{self.input_size}, {self.hidden_size}, num_layers={self.num_layers}, batch_first=True"
                + (", bidirectional=True" if self.bidirectional else ""))


def _grad_views(spec, g: torch.Tensor) -> tuple:
    """The flat gradient vector as one view per parameter, in spec.names() order (what an autograd node returns)."""
    offs, shapes = spec.offsets(), spec.shapes()
    return tuple(g[offs[n]:offs[n] + math.prod(shapes[n])].view(shapes[n]) for n in spec.names())


class _EEGFunction(torch.autograd.Function):
    """Whole-model autograd node: x, 16 parameters -> logits.  Backward returns the parameter gradients as
    views of one flat vector produced by the HIP backward kernels."""

    @staticmethod
    def forward(ctx, module: "EEG_LSTM", x: torch.Tensor, masks, *params):
        spec, flat = module.spec, module._flat
        B, T, _ = x.shape
        ws = ops.new_workspace(spec, B, T, x.device)
        drop_lstm, rrelu_slope, drop_head = masks
        logits, _ = ops.train_forward(spec, flat, x, ws, drop_lstm=drop_lstm, rrelu_slope=rrelu_slope,
                                      drop_head=drop_head, residual=module.residual)
        ctx.module, ctx.ws, ctx.masks = module, ws, masks
        ctx.save_for_backward(x, logits)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        module = ctx.module
        spec = module.spec
        x, logits = ctx.saved_tensors
        drop_lstm, rrelu_slope, drop_head = ctx.masks
        # the gradient w.r.t. the EEG window, where somebody asked for it (x.requires_grad): what autograd through self.lstm(x)
        # (lstm_eeg_model.py:34) gives the reference's users; the kernels form it where ops.dx_path says so (H = 48 and the generic
        # path).  Elsewhere the parameter gradients still come back, x gets None, and a warning says why.
        if getattr(ctx, "gates_consumed", False):
            raise NsdError("backward a second time after one that returned the input gradient: the H = 48 kernel forms dx in place of "
                           "layer 0's saved gates -- run the forward pass again")
        B, T, _ = x.shape
        dx = None
        if ctx.needs_input_grad[1]:
            if ops.dx_path(spec, B, T):
                dx = torch.empty_like(x)
            else:
                _warn_no_dx(spec, B)
        g = ops.train_backward(spec, module._flat, x, ctx.ws, logits, dlogits=dlogits.contiguous().float(),
                               drop_lstm=drop_lstm, rrelu_slope=rrelu_slope, drop_head=drop_head,
                               residual=module.residual, dx=dx)
        # (only the H = 48 fast-path kernel overwrites layer 0's saved gates; the generic path keeps them)
        ctx.gates_consumed = dx is not None and spec.fast_path() and spec.H == 48
        grads = _grad_views(spec, g)
        return (None, dx, None) + grads            # (ctx.ws lives as long as the graph does: retain_graph may come back)


_no_dx_warned = set()


def _warn_no_dx(spec, B: int) -> None:
    """One UserWarning per model shape: x.requires_grad where the kernels form no input gradient."""
    if spec in _no_dx_warned:
        return
    _no_dx_warned.add(spec)
    warnings.warn(f"EEG_LSTM: no input gradient for {spec} at batch {B} -- the kernels form dL/dx for hidden size 48 (2 layers, <= 8 "
                  "channels) and on the shape-generic path only (nsd_dx_path); the parameter gradients are returned, x.grad stays None",
                  UserWarning, stacklevel=3)


class _EEGSeqFunction(torch.autograd.Function):
    """Whole-model autograd node on the sequence-batched bf16 path (nsd_seq_*): x, parameters -> logits; backward needs
    d loss / d logits of a mean cross-entropy, which that path fuses into the forward -- so the node takes the labels
    and returns (logits, loss) with loss the mean CE the kernels computed, and only `loss.backward()` (times a scalar) is
    supported.  The Trainer calls the ops directly; this node exists so that the nn.Module surface works too.  dL/dx comes
    back where x requires it (nsd_seq_train_bwd_dx)."""

    @staticmethod
    def forward(ctx, module: "EEG_LSTM", x: torch.Tensor, labels: torch.Tensor, rng, *params):
        spec, flat = module.spec, module._flat
        B, T, _ = x.shape
        ws = ops.seq_workspace(spec, B, T, x.device)
        logits = ops.seq_train_fwd(spec, flat, x, labels, ws, rng=rng)
        loss = ops.seq_loss_sum(spec, ws, B, T) / B
        ctx.module, ctx.ws, ctx.rng, ctx.shape = module, ws, rng, (B, T)
        ctx.mark_non_differentiable(logits)
        return logits, loss.reshape(())

    @staticmethod
    def backward(ctx, _dlogits, dloss):
        module = ctx.module
        spec = module.spec
        B, T = ctx.shape
        dx = torch.empty((B, T, spec.C), dtype=torch.float32, device=dloss.device) if ctx.needs_input_grad[1] else None
        g = ops.seq_train_bwd(spec, module._flat, ctx.ws, B, T, rng=ctx.rng, dx=dx) * dloss
        if dx is not None:
            dx = dx * dloss
        grads = _grad_views(spec, g)
        return (None, dx, None, None) + grads      # (the workspace stays with the graph: a second backward re-runs the scans on it)


class _EEGSeqEvalFunction(torch.autograd.Function):
    """Eval-mode differentiable forward of the sequence-batched bf16 path: x, parameters -> logits, and a backward from ANY
    d loss / d logits (nsd_seq_train_fwd_logits -> nsd_seq_head_bwd -> nsd_seq_train_bwd[_dx]): custom losses, distillation,
    saliency.  No dropout, eval RReLU slope: the logits are those of `with torch.no_grad(): model(x)`, bit for bit."""

    @staticmethod
    def forward(ctx, module: "EEG_LSTM", x: torch.Tensor, *params):
        spec, flat = module.spec, module._flat
        B, T, _ = x.shape
        ws = ops.seq_workspace(spec, B, T, x.device)
        logits = ops.seq_train_fwd_logits(spec, flat, x, ws)
        ctx.module, ctx.ws, ctx.shape = module, ws, (B, T)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        module = ctx.module
        spec = module.spec
        B, T = ctx.shape
        ops.seq_head_bwd(spec, module._flat, ctx.ws, dlogits.contiguous().float(), B, T)
        dx = torch.empty((B, T, spec.C), dtype=torch.float32, device=dlogits.device) if ctx.needs_input_grad[1] else None
        g = ops.seq_train_bwd(spec, module._flat, ctx.ws, B, T, dx=dx)
        grads = _grad_views(spec, g)
        return (None, dx) + grads                  # (head_bwd + bwd recompute from the saved sequence: retain_graph gives the same bits)


class EEG_LSTM(nn.Module):
    """2-layer LSTM -> attention pooling over time -> LayerNorm -> Linear/RReLU/Dropout/Linear.

    Signature and defaults of the reference (lstm_eeg_model.py:14).  Keyword-only extensions, all
    default OFF so that reference checkpoints reproduce reference logits:
      residual       add the layer input to the output of every LSTM layer l>=1 (README's "residual stack")
      normalize      per-channel z-score of the window before the LSTM (Frontend/app.py:166-170 semantics)
      bidirectional  torch.nn.LSTM(bidirectional=True) where lstm_eeg_model.py:16-22 builds the LSTM: `_reverse`
                     parameters in torch's order, the attention pooling / LayerNorm / fc.0 act on 2H columns (BASELINE cfg5)
      precision      "fp32" (default) or "bf16": the sequence-batched path for hidden sizes 64/128/256/512 (BASELINE cfg3 /
                     cfg5) -- bf16 GEMM operands and saved activations, fp32 accumulation and cell state; logits differ
                     from an fp32 run at the 1e-2 level.  bidirectional needs "bf16".
      prep           a CausalPrep: the causal front end (nsd_prep_step, window mode: every trial from a reset state) in front of the
                     LSTM, where normalize runs its z-score -- the model then sees what a StreamDecoder feeds it chunk by chunk.
                     Not together with normalize; no input gradient is offered through it.
      gate           a SignalGate: the signal-quality gate around the front end (gate -> prep -> apply -> LSTM; nsd_gate_step in
                     window mode, nsd_gate_apply): a bad channel is held through the front end and zeroed in front of the LSTM; in
                     eval mode a trial with a rejected step has NaN logits ("no decision"), in train mode nothing is rejected.
                     Not together with normalize; no input gradient is offered through it.
      align          a SessionAlign: session alignment behind the front end (gate -> prep -> apply -> align -> LSTM; nsd_spatial_apply):
                     every step is multiplied by the model's alignment matrix, a non-persistent buffer `align_matrix` [C,C] that is the
                     identity until set (align_matrix=, set_alignment(), SessionAlign.fit, align.SpatialFit).  Not together with
                     normalize.  enable_alignment() gives a model built without one the stage at the identity.
      align_grad     True: x.requires_grad differentiates through the alignment stage (ops.spatial_apply as an autograd node,
                     nsd_spatial_bwd behind it: x.grad = W^T . dL/d(aligned x), where the kernels form dx at all).  False (default):
                     asking for an input gradient through align= is refused, as through gate= and prep=, which stay refused.
      resample       a Resample: rate conversion as stage 0 of the front end (resample -> gate -> prep -> apply -> align -> LSTM;
                     nsd_resample_step in window mode: every trial from rest).  The caller's windows are at the amplifier's rate;
                     everything behind the stage counts samples at the model's rate -- the gate's spans, the sections' corners,
                     window / hop of crops and sliding decoders, quality().  The gate's rail and jump detectors therefore see
                     filtered samples, not the amplifier's.  Not together with normalize (the z-score would be taken over the
                     filter's start-up); no input gradient is offered through it.
      crop           an ops.Crop: the window the model was (or is being) trained on by cropped training (Trainer(crop=)).  It changes
                     nothing in forward(); it travels with the model and its checkpoints so that predict_trials(), SimplePredictor and
                     open_stream() know the trained window.
    """

    def __init__(self, input_size=8, hidden_size=48, num_layers=2, num_classes=3, dropout=0.60, *,
                 residual: bool = False, normalize: bool = False, bidirectional: bool = False, precision: str = "fp32",
                 prep: Optional[CausalPrep] = None, crop: Optional["ops.Crop"] = None, gate: Optional[SignalGate] = None,
                 align: Optional[SessionAlign] = None, align_matrix=None, align_grad: bool = False,
                 resample: Optional[Resample] = None):
        super().__init__()
        if resample is not None and not isinstance(resample, Resample):
            raise ValueError(f"resample={resample!r}: expected a Resample")
        if resample is not None and normalize:
            raise ValueError("resample together with normalize=True: the whole-window z-score would be taken over the filter's start-up "
                             "(CausalPrep.design(zscore_seconds=...) is its running form behind the rate conversion)")
        if resample is not None and not 1 <= input_size <= 64:
            raise ValueError(f"resample: the rate conversion covers 1 .. 64 channels, input_size = {input_size}")
        self.resample = resample
        self.align_grad = bool(align_grad)
        if align is not None and not isinstance(align, SessionAlign):
            raise ValueError(f"align={align!r}: expected a SessionAlign")
        if align is not None and normalize:
            raise ValueError("align together with normalize=True: the whole-window z-score would undo the whitening channel by channel "
                             "(CausalPrep.design(zscore_seconds=...) is its running form in front of the alignment)")
        if align is not None and not 1 <= input_size <= 32:
            raise ValueError(f"align: session alignment covers 1 .. 32 channels, input_size = {input_size}")
        if align is None and align_matrix is not None:
            raise ValueError("align_matrix without align=SessionAlign(...)")
        self.align, self.align_record = align, None         # (the record of the fit the matrix came from, where it came from one)
        if align is not None:
            self.register_buffer("align_matrix", torch.eye(input_size, dtype=torch.float32), persistent=False)
            if align_matrix is not None:
                self.set_alignment(align_matrix)
        if gate is not None and not isinstance(gate, SignalGate):
            raise ValueError(f"gate={gate!r}: expected a SignalGate")
        if gate is not None and normalize:
            raise ValueError("gate together with normalize=True: the whole-window z-score would be taken over held and zeroed channels "
                             "(CausalPrep.design(zscore_seconds=...) is its running form behind the gate)")
        if gate is not None and not 1 <= input_size <= 32:
            raise ValueError(f"gate: the signal-quality gate covers 1 .. 32 channels, input_size = {input_size}")
        self.gate = gate
        if crop is not None and not isinstance(crop, ops.Crop):
            raise ValueError(f"crop={crop!r}: expected an ops.Crop")
        self.crop = crop
        if prep is not None and not isinstance(prep, CausalPrep):
            raise ValueError(f"prep={prep!r}: expected a CausalPrep")
        if prep is not None and normalize:
            raise ValueError("prep together with normalize=True: the whole-window z-score is what the causal front end replaces "
                             "(CausalPrep.design(zscore_seconds=...) is its running form)")
        if prep is not None and not 1 <= input_size <= 64:
            raise ValueError(f"prep: the causal front end covers 1 .. 64 channels, input_size = {input_size}")
        self.prep = prep
        if precision not in ("fp32", "bf16"):
            raise ValueError(f"precision={precision!r}: expected 'fp32' or 'bf16'")
        self.spec = ops.ModelSpec(C=input_size, H=hidden_size, L=num_layers, K=num_classes, F=ops.FC_HIDDEN,
                                  D=2 if bidirectional else 1, residual=bool(residual) and precision == "bf16")
        self.precision = precision
        if bidirectional and precision != "bf16":
            raise ValueError("bidirectional=True is built on the sequence-batched path only: pass precision='bf16'")
        self.dropout_p = float(dropout) if num_layers > 1 else 0.0   # nn.LSTM drops only between layers (:21)
        self.head_dropout_p = float(dropout)
        self.residual, self.normalize = bool(residual), bool(normalize)
        self.lstm = _StackedLSTMParams(input_size, hidden_size, num_layers, bidirectional)
        DH = self.spec.D * hidden_size
        self.ln = nn.LayerNorm(DH)
        self.attn = nn.Linear(DH, 1)
        self.fc = nn.Sequential(
            nn.Linear(DH, ops.FC_HIDDEN),
            nn.RReLU(),
            nn.Dropout(dropout),
            nn.Linear(ops.FC_HIDDEN, num_classes),
        )
        self._flat: Optional[torch.Tensor] = None
        self._seed = int(torch.initial_seed()) & 0x7FFFFFFFFFFFFFFF
        self._step = 0
        self._mask_override = None    # tests inject explicit (drop_lstm, rrelu_slope, drop_head)

    # ---- flat parameter storage: all 16 tensors are views into one contiguous vector -----------------
    def _named_in_order(self):
        byname = dict(self.named_parameters())
        return [(n, byname[n]) for n in self.spec.names()]

    def flatten_parameters(self) -> torch.Tensor:
        """(Re)pack the parameters into one flat fp32 vector in state_dict order; the kernels read it
        directly and the optimizer / gradient all-reduce work on it as a single buffer."""
        named = self._named_in_order()
        dev = named[0][1].device
        flat = torch.empty(self.spec.param_count, dtype=torch.float32, device=dev)
        offs = self.spec.offsets()
        with torch.no_grad():
            for n, p in named:
                seg = flat[offs[n]:offs[n] + p.numel()].view(p.shape)
                seg.copy_(p.detach().to(torch.float32))
                p.data = seg
        self._flat = flat
        return flat

    def _flat_ok(self) -> bool:
        f = self._flat
        if f is None:
            return False
        base, offs = f.data_ptr(), self.spec.offsets()
        return all(p.data_ptr() == base + 4 * offs[n] and p.dtype == torch.float32 for n, p in self._named_in_order())

    def flat_parameters(self) -> torch.Tensor:
        if not self._flat_ok():
            self.flatten_parameters()
        return self._flat

    def view_of(self, row: torch.Tensor) -> "EEG_LSTM":
        """A second EEG_LSTM of this model's shape and options (eval mode) whose parameters are views of `row`, a flat fp32 vector of
        param_count elements in state_dict order -- a trainer's averaged row: the module follows whatever is written there later."""
        sp = self.spec
        if row.dtype != torch.float32 or row.dim() != 1 or row.numel() != sp.param_count or not row.is_contiguous():
            raise NsdError(f"EEG_LSTM.view_of: row must be a contiguous float32 vector of {sp.param_count} elements")
        twin = EEG_LSTM(sp.C, sp.H, sp.L, sp.K, self.head_dropout_p, residual=self.residual, normalize=self.normalize,
                        bidirectional=sp.D == 2, precision=self.precision, prep=self.prep, crop=self.crop, gate=self.gate, align=self.align,
                        align_grad=self.align_grad, resample=self.resample)
        if self.align is not None:
            twin.align_matrix, twin.align_record = self.align_matrix, self.align_record   # (shared: the twin follows a later set_alignment)
        offs = sp.offsets()
        with torch.no_grad():
            for n, p in twin._named_in_order():
                p.data = row[offs[n]:offs[n] + p.numel()].view(p.shape)
                p.requires_grad_(False)                    # nobody trains an average: forward() takes the inference launch
        twin._flat = row
        return twin.eval()

    def _apply(self, fn, *a, **kw):
        out = super()._apply(fn, *a, **kw)
        self._flat = None        # .to()/.cuda() re-created the storages
        return out

    def enable_alignment(self, align: Optional[SessionAlign] = None) -> "EEG_LSTM":
        """Give a model built (or loaded) without align= the alignment stage, at the identity: the start and the prior of a supervised
        fit (align.SpatialFit).  A model that has the stage keeps it, and its matrix, as they are."""
        if self.align is not None:
            return self
        if self.normalize:
            raise ValueError("enable_alignment on a normalize=True model: the whole-window z-score would undo the matrix channel by channel")
        if not 1 <= self.spec.C <= 32:
            raise ValueError(f"enable_alignment: session alignment covers 1 .. 32 channels, the model has {self.spec.C}")
        self.align = align if align is not None else SessionAlign()
        dev = next(self.parameters()).device
        self.register_buffer("align_matrix", torch.eye(self.spec.C, dtype=torch.float32, device=dev), persistent=False)
        return self

    def set_alignment(self, W, record: Optional[dict] = None) -> None:
        """Write the alignment matrix [C,C] (a tensor on any device, or an array) into the model's buffer, in place.  record: the
        nsd_whiten_fit record it came with (ops.whiten_records); it travels in the model's checkpoints."""
        if self.align is None:
            raise NsdError("EEG_LSTM.set_alignment: the model was built without align=SessionAlign(...)")
        W = torch.as_tensor(W, dtype=torch.float32)
        if tuple(W.shape) != tuple(self.align_matrix.shape):
            raise ValueError(f"set_alignment: expected a {list(self.align_matrix.shape)} matrix, got {tuple(W.shape)}")
        with torch.no_grad():
            self.align_matrix.copy_(W)
        self.align_record = None if record is None else dict(record)

    # ---- forward --------------------------------------------------------------------------------------
    def _front_end(self, x: torch.Tensor) -> torch.Tensor:
        """What stands between the caller's window and the LSTM: the z-score (normalize), the signal-quality gate around the causal
        front end (gate -> prep -> apply), or nothing."""
        if self.resample is not None and x.requires_grad and torch.is_grad_enabled():
            raise NsdError("EEG_LSTM(resample=...): dx through the rate conversion is not offered -- x.requires_grad would get no "
                           "gradient; detach x, or differentiate a resample-free model on ops.resample_trials(x, resample)")
        if self.gate is not None and x.requires_grad and torch.is_grad_enabled():
            raise NsdError("EEG_LSTM(gate=...): dx through the signal-quality gate is not offered -- x.requires_grad would get no "
                           "gradient; detach x, or differentiate a gate-free model on the gated windows (ops.gate_step, ops.gate_apply)")
        if self.prep is not None:
            if x.requires_grad and torch.is_grad_enabled():
                raise NsdError("EEG_LSTM(prep=...): dx through the causal front end is not offered -- x.requires_grad would get no "
                               "gradient; detach x, or differentiate a prep-free model on ops.prep_step(x, prep)")
        if self.align is not None and not self.align_grad and x.requires_grad and torch.is_grad_enabled():
            raise NsdError("EEG_LSTM(align=...): dx through the session alignment is not offered -- x.requires_grad would get no "
                           "gradient; detach x, build the model with align_grad=True, or differentiate an align-free model on "
                           "ops.spatial_apply(x, W)")
        if self.resample is not None or self.gate is not None or self.prep is not None or self.align is not None:
            return self._front(x)
        return ops.zscore(x) if self.normalize else x

    def _gate_prep(self, x: torch.Tensor, want_mask: bool = False):
        """gate -> prep -> apply over whole windows, each stage where the model has it.  Train mode never rejects a step.
        want_mask: -> (x, the gate's mask words or None)."""
        mask = None
        if self.gate is not None:
            x, mask = ops.gate_step(x, self.gate)
        if self.prep is not None:
            x = ops.prep_step(x, self.prep, out=x if mask is not None else None)
        if mask is not None:
            x = ops.gate_apply(x, self.gate, mask, out=x, max_bad=self.spec.C if self.training else None)
        return (x, mask) if want_mask else x

    def _front(self, x: torch.Tensor) -> torch.Tensor:
        """resample -> gate -> prep -> apply -> align over whole windows: what stands in front of the (crop and the) LSTM."""
        if self.resample is not None:
            x = ops.resample_trials(x, self.resample)
        y = self._gate_prep(x)
        if self.align is not None:
            y = ops.spatial_apply(y, self.align_matrix, out=y if y is not x else None)   # (in place in a buffer of this call's own)
        return y

    def _train_masks(self, B: int, T: int, device):
        if self._mask_override is not None:
            return self._mask_override
        self._step += 1
        base = sr.base_stream(self._step)                   # (the module's own train-mode calls number their streams as a trainer's steps)
        sp = self.spec
        drop_lstm = (ops.dropout_mask(self._seed, base + sr.SLOT_LSTM_DROPOUT, self.dropout_p, (sp.L - 1, B, T, sp.H), device)
                     if self.dropout_p > 0 and sp.L > 1 else None)
        rrelu = ops.rrelu_noise(self._seed, base + sr.SLOT_RRELU, (B, sp.F), device)
        drop_head = (ops.dropout_mask(self._seed, base + sr.SLOT_HEAD_DROPOUT, self.head_dropout_p, (B, sp.F), device)
                     if self.head_dropout_p > 0 else None)
        return drop_lstm, rrelu, drop_head

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        # x: [B, T, C] -> logits [B, num_classes]  (no softmax, as lstm_eeg_model.py:32-39)
        if x.dim() != 3 or x.shape[-1] != self.spec.C:
            raise ValueError(f"Expected x of shape [B, T, {self.spec.C}], got {tuple(x.shape)}")
        flat = self.flat_parameters()
        if not flat.is_cuda or not x.is_cuda:
            raise NsdError("EEG_LSTM runs only on the MI355X HIP path: move the module and the input to the GPU "
                           f"(module on {flat.device}, input on {x.device}); there is no CPU fallback")
        x = x.contiguous().float()     # predict() hands over a transposed view (preprocessor.py:34)
        x = self._front_end(x)
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if self.precision == "bf16":
            if not self.spec.seq_path(max(x.shape[0], 1), x.shape[1]):
                raise NsdError(f"precision='bf16': model shape {self.spec} is not covered by the sequence-batched path "
                               "(hidden size 64/128/256/512, fc width and classes <= 64)")
            if self.training:
                raise NsdError("precision='bf16': no train-mode forward() -- train through EEG_LSTM.loss(x, labels) or "
                               "nsd_amd.trainer.Trainer (the path draws dropout and fuses the cross-entropy in its kernels); in eval "
                               "mode forward() is differentiable w.r.t. the parameters and x for any loss")
            if torch.is_grad_enabled() and (need_grad or x.requires_grad):
                params = [p for _, p in self._named_in_order()]
                return _EEGSeqEvalFunction.apply(self, x, *params)
            logits, _ = ops.seq_infer(self.spec, flat, x, want_probs=False)
            return logits
        if not self.training and not need_grad:
            logits, _ = ops.infer(self.spec, flat, x, residual=self.residual, want_probs=False)
            return logits
        masks = self._train_masks(x.shape[0], x.shape[1], x.device) if self.training else (None, None, None)
        params = [p for _, p in self._named_in_order()]
        return _EEGFunction.apply(self, x, masks, *params)

    def loss(self, x: torch.Tensor, labels: torch.Tensor):
        """precision='bf16' training surface: (logits, mean cross-entropy) with the loss differentiable w.r.t. the
        parameters -- `model.loss(x, y)[1].backward()` fills `.grad` of all tensors, and `x.grad` where x requires it.  Train
        mode draws the dropout / RReLU streams inside the kernels."""
        if self.precision != "bf16":
            raise NsdError("EEG_LSTM.loss is the bf16 path's training surface; with precision='fp32' use "
                           "torch.nn.functional.cross_entropy(model(x), y)")
        flat = self.flat_parameters()
        x = x.contiguous().float()
        x = self._front_end(x)
        rng = None
        if self.training:
            self._step += 1
            rng = sr.step_rng(self._seed, self._step, self.dropout_p, self.head_dropout_p)
        params = [p for _, p in self._named_in_order()]
        return _EEGSeqFunction.apply(self, x, labels.to(torch.int32).contiguous(), rng, *params)

    @torch.no_grad()
    def predict_proba(self, x: torch.Tensor) -> torch.Tensor:
        """Eval-mode class probabilities with the softmax fused into the head kernel (lstm_eeg_model.py:97)."""
        x = x.contiguous().float()
        x = self._front_end(x)
        if self.precision == "bf16":
            # (the workspace of the evaluation is kept: its status word says whether NaN probabilities are a result or a failure)
            self._last_seq_ws = ops.seq_workspace(self.spec, x.shape[0], x.shape[1], x.device) if x.shape[0] > 0 else None
            return ops.seq_infer(self.spec, self.flat_parameters(), x, ws=self._last_seq_ws, want_probs=True)[1]
        _, probs = ops.infer(self.spec, self.flat_parameters(), x, residual=self.residual, want_probs=True)
        return probs

    @torch.no_grad()
    def predict_trials(self, x: torch.Tensor, hop: Optional[int] = None, window: Optional[int] = None):
        """Trial-level decisions of a model that decides on windows shorter than the trial: x [B,T,C] -> (pooled class probabilities
        [B,K], the windows' probabilities [B,R,K]).  Every whole window of `window` samples (default: the trained one, self.crop's)
        `hop` samples apart (default: half the window) is decided -- the front end over the whole trial first, then the cut, then
        with normalize the z-score of each window, as a cropped training step prepares them (nsd_crop) -- and the trial's decision is
        the mean of its windows' probabilities (nsd_crop_pool).  These are the decisions a sliding decoder with (window, hop) takes on
        the trial."""
        if window is None:
            if self.crop is None:
                raise NsdError("EEG_LSTM.predict_trials: give window=, or a model that carries its trained window (crop=)")
            window = self.crop.window
        hop = max(int(window) // 2, 1) if hop is None else int(hop)
        x = x.contiguous().float()
        if x.dim() != 3 or x.shape[-1] != self.spec.C:
            raise ValueError(f"Expected x of shape [B, T, {self.spec.C}], got {tuple(x.shape)}")
        B, T, _ = x.shape
        if self.resample is not None:
            T = self.resample.out_steps(0, T)               # (window and hop count samples at the model's rate)
        grid = ops.Crop.grid(T, int(window), hop)
        x = self._front(x)
        xc, _, _ = ops.crop(x, grid)
        if self.normalize:
            ops.zscore(xc, out=xc)
        if self.precision == "bf16":
            self._last_seq_ws = ops.seq_workspace(self.spec, xc.shape[0], xc.shape[1], x.device) if B > 0 else None
            probs = ops.seq_infer(self.spec, self.flat_parameters(), xc, ws=self._last_seq_ws, want_probs=True)[1]
        else:
            _, probs = ops.infer(self.spec, self.flat_parameters(), xc, residual=self.residual, want_probs=True)
        probs = probs.view(B, grid.crops, self.spec.K)
        return ops.crop_pool(probs, want_logits=False)[0], probs


# Module names under which the reference's PreProcessor can live, in the reference's own resolution order
# (lstm_eeg_model.py:7-10): package import first (Frontend/app.py:22-28 puts Neuro-Alpha-App/ on sys.path and imports
# Utilities.tester -> Utilities.lstm_eeg_model -> `.preprocessor`), then the script form with Utilities/ itself on the path.
_REFERENCE_PREPROCESSOR_MODULES = ("Utilities.preprocessor", "preprocessor")


def _find_module(name: str) -> bool:
    try:
        return importlib.util.find_spec(name) is not None
    except (ImportError, ValueError):          # parent package missing / half-initialised entry in sys.modules
        return False


def resolve_reference_preprocessor(package: Optional[str] = None):
    """The reference's `PreProcessor` class (preprocessor.py:7-36, the MindsAI filter) as the reference would import
    it at lstm_eeg_model.py:7-10, or None when no such module is importable.  `package`: name of the package the
    re-exporting stub lives in (its `__package__`); tried first as `<package>.preprocessor`.

    Only the *lookup* is guarded: once the module is found, errors raised while importing it (e.g. its own MindsAI
    dependency missing, preprocessor.py:3-6,18-19) propagate, exactly as they would from the reference."""
    names = ([f"{package}.preprocessor"] if package else []) + list(_REFERENCE_PREPROCESSOR_MODULES)
    for name in names:
        if name.split(".")[0] == __name__.split(".")[0]:
            continue                              # never resolve to this package itself
        if _find_module(name):
            return getattr(importlib.import_module(name), "PreProcessor")
    return None


def _default_preprocessor(sr: int, tailoring_lambda: float, package: Optional[str] = None):
    """The reference always filters the window with the third-party MindsAI filter before the model
    (lstm_eeg_model.py:66,91).  The filter is out of scope here (non-commercial licence, host-side numpy) and is never
    restated: the facade uses the reference's own class when it is importable in either of the reference's import
    modes, and otherwise REFUSES to guess -- skipping the filter changes the probabilities (max |delta| ~ 38 uV on a
    real trial), so running without it must be asked for explicitly with `preprocess="identity"`."""
    cls = resolve_reference_preprocessor(package)
    if cls is None:
        raise NsdError(
            "SimplePredictor: the reference's PreProcessor (Utilities/preprocessor.py, MindsAI filter) is not importable "
            f"as any of {list(_REFERENCE_PREPROCESSOR_MODULES)}; the reference applies it to every window "
            "(lstm_eeg_model.py:91).  Put Neuro-Alpha-App/ (or Neuro-Alpha-App/Utilities/) on sys.path, pass "
            "preprocess=<object with .transform([T,C]) -> [T,C]>, or pass preprocess=\"identity\" to run the model "
            "on unfiltered windows on purpose.")
    return cls(sr=sr, tailoring_lambda=tailoring_lambda)


def _raise_on_poison(model: "EEG_LSTM", probs: np.ndarray, what: str) -> None:
    """NaN probabilities are a RESULT wherever the reference produces them (a NaN / Inf window, NaN or diverged weights:
    lstm_eeg_model.py:96-99 returns NaN probabilities and label index 0, and so does this facade on both precisions).  The one case
    that is a failed evaluation instead is the bf16 path's scan time-out (include/nsd.h, 'Failure reporting': the head then poisons
    every output with NaN): decided from the status word of the evaluation's workspace, never inferred from the NaN itself."""
    if model.precision != "bf16" or not np.isnan(probs).any():
        return
    ws = getattr(model, "_last_seq_ws", None)
    if ws is not None:
        ops.seq_raise_on_timeout(ws, what)


class IdentityPreProcessor:
    """Explicit opt-out of the MindsAI filter: same shape / dtype / ValueError contract as the reference's
    PreProcessor.transform (preprocessor.py:21-36), no filtering.  Selected with `preprocess="identity"`."""

    def __init__(self, sr: int = 125, tailoring_lambda: float = 1.25e-29):
        self.sr, self.tailoring_lambda = sr, tailoring_lambda

    def transform(self, chunk_samples_by_channels: np.ndarray) -> np.ndarray:
        x = np.asarray(chunk_samples_by_channels)
        if x.ndim != 2:
            raise ValueError(f"Expected 2D array [samples, channels], got {x.shape}")
        return x.astype(np.float32, copy=False)


class SimplePredictor:
    """Mirror of the reference's SimplePredictor (lstm_eeg_model.py:42-101): preprocess a [T,C] window,
    run the model, softmax, return (probs float32[K], label).

    `device` keeps the reference's keyword and default ("cpu", what tester.py:83 passes) but only names
    where the caller's arrays live: numpy in, numpy out.  The model itself always runs on the GPU
    (`gpu` argument, default "cuda"); if none is available construction fails loudly.

    `preprocess`: None (default) = the reference's own PreProcessor, resolved the way lstm_eeg_model.py:7-10 does
    (`preprocess_package`: the stub's `__package__`); construction FAILS when it cannot be found.
    "identity" = no filtering, on purpose.  Any object with `.transform([T,C]) -> [T,C]` is used as given.
    """

    def __init__(self, pth_path: str, sr: int, channel_order=None, input_size: int = 8, hidden_size: int = 48,
                 num_layers: int = 2, num_classes: int = 3, dropout: float = 0.60, device: str = "cpu",
                 tailoring_lambda: float = 1.25e-29, class_names=None, *, preprocess=None,
                 preprocess_package: Optional[str] = None, gpu: str = "cuda", residual: bool = False,
                 normalize: bool = False, bidirectional: bool = False, precision: str = "fp32", model_rate: Optional[float] = None):
        """A checkpoint written from a model with a causal front end carries it ({"state_dict": ..., "nsd_prep": CausalPrep.to_dict()},
        trainer.save_reference_checkpoint): the predictor's model is rebuilt with that prep.  A signal-quality gate travels the same way
        ("nsd_gate": SignalGate.to_dict()), session alignment as "nsd_align": {config, matrix, record}.  One written from a model trained on
        crops carries "nsd_crop" = {window, crops, hop} beside it: the model is rebuilt with that ops.Crop (predict_trial, open_stream).
        A rate conversion travels as "nsd_resample" = Resample.to_dict(): the model is rebuilt with it, `sr` is then the amplifier's rate
        and self.model_rate = sr * L / M the model's.  model_rate= (default None: the checkpoint's conversion, or none) names the model's
        rate where the checkpoint records no conversion: with sr != model_rate the predictor designs one, Resample.design(sr, model_rate).
        With neither, nothing is converted and model_rate is sr."""
        self.device = torch.device(device)
        self.sr = sr
        self.class_names = class_names or CLASS_NAMES
        if preprocess is None:
            self.pre = _default_preprocessor(sr, tailoring_lambda, preprocess_package)
        elif isinstance(preprocess, str):
            if preprocess != "identity":
                raise ValueError(f"preprocess={preprocess!r}: the only named preprocessor is \"identity\"")
            self.pre = IdentityPreProcessor(sr, tailoring_lambda)
        else:
            self.pre = preprocess
        if not torch.cuda.is_available():
            raise NsdError("SimplePredictor needs an MI355X: torch.cuda.is_available() is False and the HIP path has "
                           "no CPU fallback")
        self.gpu = torch.device(gpu)
        state = torch.load(pth_path, map_location="cpu", weights_only=True)
        prep = crop = gate = align = align_state = resample = None
        if isinstance(state, dict) and "state_dict" in state:     # both forms, as lstm_eeg_model.py:79-80
            align_state = state.get("nsd_align")
            align = SessionAlign.from_dict(align_state["config"]) if align_state is not None else None
            prep = CausalPrep.from_dict(state["nsd_prep"]) if state.get("nsd_prep") is not None else None
            crop = ops.Crop(**{k: int(v) for k, v in state["nsd_crop"].items()}) if state.get("nsd_crop") is not None else None
            gate = SignalGate.from_dict(state["nsd_gate"]) if state.get("nsd_gate") is not None else None
            resample = Resample.from_dict(state["nsd_resample"]) if state.get("nsd_resample") is not None else None
            state = state["state_dict"]
        if resample is None and model_rate is not None and float(model_rate) != float(sr):
            resample = Resample.design(sr, model_rate)
        self.model_rate = float(sr) if resample is None else float(sr) * resample.L / resample.M
        if resample is not None and model_rate is not None and abs(self.model_rate - float(model_rate)) > 1e-6 * float(model_rate):
            raise NsdError(f"SimplePredictor: the checkpoint's rate conversion is L / M = {resample.L} / {resample.M}: sr = {sr} Hz gives the "
                           f"model {self.model_rate} Hz, model_rate = {model_rate}")
        self.model = EEG_LSTM(input_size=input_size, hidden_size=hidden_size, num_layers=num_layers,
                              num_classes=num_classes, dropout=dropout, residual=residual, normalize=normalize,
                              bidirectional=bidirectional, precision=precision, prep=prep, crop=crop, gate=gate, align=align,
                              resample=resample)
        if align_state is not None:
            self.model.set_alignment(align_state["matrix"], record=align_state.get("record"))
        self.model.load_state_dict(state, strict=True)
        self.model.to(self.gpu).eval()
        self.model.flatten_parameters()

    def predict(self, chunk_TxC: np.ndarray):
        """chunk_TxC: [T, C] float32 window -> (probs np.float32[K], label str)."""
        x = self.pre.transform(chunk_TxC)
        x_t = torch.from_numpy(np.ascontiguousarray(x[None, ...], dtype=np.float32)).to(self.gpu, non_blocking=True)
        probs = self.model.predict_proba(x_t)[0].cpu().numpy().astype(np.float32)
        _raise_on_poison(self.model, probs, "SimplePredictor.predict")
        y_idx = int(np.argmax(probs))
        return probs, self.class_names[y_idx]

    def predict_trial(self, trial_TxC: np.ndarray, hop_seconds: Optional[float] = None):
        """The pooled decision of a trial longer than the window the model was trained on (a checkpoint of cropped training):
        trial_TxC [T, C] -> (probs np.float32[K], label str).  Every whole trained window, hop_seconds apart (default: half the
        window), is decided as predict() decides it, and the trial's probabilities are the mean of its windows' (nsd_crop_pool)."""
        crop = getattr(self.model, "crop", None)
        if crop is None:
            raise NsdError("SimplePredictor.predict_trial: the checkpoint carries no trained window (nsd_crop): it was trained on whole "
                           "trials -- use predict()")
        hop = max(crop.window // 2, 1) if hop_seconds is None else int(round(hop_seconds * self.model_rate))
        if hop < 1:
            raise ValueError(f"SimplePredictor.predict_trial: hop_seconds {hop_seconds!r} is less than one sample")
        win_probs, _ = self.predict_windows(trial_TxC, crop.window, hop)
        if win_probs.shape[0] == 0:
            raise ValueError(f"SimplePredictor.predict_trial: the trial has {np.asarray(trial_TxC).shape[0]} samples, the trained window {crop.window}")
        pooled = ops.crop_pool(torch.from_numpy(win_probs[None]).to(self.gpu), want_logits=False)[0][0].cpu().numpy().astype(np.float32)
        return pooled, self.class_names[int(np.argmax(pooled))]

    def predict_windows(self, recording_NxC: np.ndarray, window: int, hop: Optional[int] = None):
        """Batched / streaming mode: classify every `window`-sample window of a longer recording
        [N, C], `hop` samples apart (default: back to back, the live loop of tester.py:52-96 run over a file), in ONE
        launch.  Each window goes through the same preprocess -> model -> softmax as predict(), so
        predict_windows(r, T)[0][k] == predict(r[k*hop : k*hop + T])[0].  Returns (probs float32 [n, K], labels list[str])."""
        rec = np.asarray(recording_NxC)
        if rec.ndim != 2:
            raise ValueError("recording must be 2-D [N, C]")
        hop = int(hop) if hop is not None else int(window)
        if window < 1 or hop < 1:
            raise ValueError("window and hop must be positive")
        starts = list(range(0, rec.shape[0] - window + 1, hop))
        K = len(self.class_names)
        if not starts:
            return np.zeros((0, K), np.float32), []
        # the preprocessor is per window by contract (the MindsAI filter is not shift-invariant): host side, like predict()
        xs = np.stack([np.ascontiguousarray(self.pre.transform(rec[s0:s0 + window]), dtype=np.float32) for s0 in starts])
        x_t = torch.from_numpy(xs).to(self.gpu, non_blocking=True)
        probs = self.model.predict_proba(x_t).cpu().numpy().astype(np.float32)
        _raise_on_poison(self.model, probs, "SimplePredictor.predict_windows")
        return probs, [self.class_names[int(i)] for i in probs.argmax(1)]


    def open_stream(self, streams: int = 1, chunk_transform=None, *, window_seconds: Optional[float] = None,
                    hop_seconds: Optional[float] = None):
        """Resumable decoding (an extension, see stream.py): a PredictorStream whose push(chunk [n,C] or [B,n,C]) advances `streams`
        live streams and returns (probs, labels) of each stream's whole prefix -- predict() on the samples seen so far, without
        waiting for the window to end.  Allowed when the predictor's preprocessor is the identity one, or when the caller passes
        `chunk_transform` ([n,C] -> [n,C], applied to every chunk in place of the preprocessor: a causal filter of the caller's).
        A model with a causal front end (EEG_LSTM(prep=...), rebuilt from its checkpoint) filters and normalises the chunks on the GPU,
        with its state carried from chunk to chunk: what the model is fed is bit for bit what predict() feeds it on the whole window, and
        the probabilities after the last chunk are predict()'s within the resumable path's own bound against nsd_infer (measured 1.5e-7;
        the readout's pooling is updated per step, nsd_infer's per block of steps, so the last bits can differ).
        window_seconds and hop_seconds (both, or neither: the object above, unchanged): a continuous stream without cues -- a
        PredictorSlidingStream whose push returns, per stream, a list of (end_sample, probs float32 [K], label) for the windows the
        chunk completed: every hop_seconds, the decision of the model run from a zero state over the last window_seconds (of an
        EnsemblePredictor: the mean of its members' decisions, all members advanced by one launch per chunk).  With a checkpoint of
        cropped training (nsd_crop), hop_seconds alone is enough: window_seconds defaults to the trained window."""
        from .stream import PredictorSlidingStream, PredictorStream
        crop = getattr(self.model, "crop", None)
        if window_seconds is None and hop_seconds is not None and crop is not None:
            window_seconds = crop.window / float(self.model_rate)   # a model trained on crops: the window it was trained to decide on
        if (window_seconds is None) != (hop_seconds is None):
            raise ValueError("SimplePredictor.open_stream: window_seconds and hop_seconds go together (both, or neither)")
        if chunk_transform is None and not isinstance(self.pre, IdentityPreProcessor):
            raise NsdError("SimplePredictor.open_stream: the reference's window filter (PreProcessor.transform, preprocessor.py:21-36) "
                           "works on a whole window and is not causal, so a stream cannot be filtered with it chunk by chunk; pass "
                           "chunk_transform=<causal [n,C] -> [n,C] callable>, or build the predictor with preprocess=\"identity\"")
        if window_seconds is not None:
            # (window and hop count samples at the model's rate: behind a rate conversion that is not the rate of the pushed chunks)
            return PredictorSlidingStream(self, streams, chunk_transform, int(round(window_seconds * self.model_rate)),
                                          int(round(hop_seconds * self.model_rate)))
        return PredictorStream(self, streams, chunk_transform)

    def calibrate(self, trials, labels, align: bool = True, **fit_kw) -> dict:
        """Session calibration (an extension, see calibrate.py): refit the read-out (LayerNorm, fc.0, fc.3; the LSTM stack and the
        attention stay frozen) on a few cued trials of a new session.  trials [N,T,C] (N <= 256), labels [N] class indices.  The
        trials run through open_stream on reset slots -- preprocessing and a causal front end are exactly what the live stream
        applies -- their pooled features are read and the read-out is fitted by nsd_amd.HeadFit(**fit_kw) in one launch (of an
        EnsemblePredictor: all members together, each on its own features).  chunk_transform=: as open_stream's.  The model is updated
        in place: a decoder that is open keeps its state, and its next read-out uses the fitted head.  Returns a dict with loss and
        accuracy on the calibration trials before and after, the fit's loss curve and its status.
        align (a model with session alignment only): the alignment matrix is refitted from the calibration trials first -- label-free,
        one nsd_whiten_fit over the accumulators of all trials -- and features and the head fit then run on aligned input; decoders
        opened afterwards start from the new matrix.  A fit that kept the identity (too few steps) leaves the matrix as it was.
        spatial=dict(...) (align.SpatialFit's keywords; {} for its defaults): behind that refit and in front of the features, the
        alignment matrix is fitted on the labelled trials by gradient descent through the frozen model; the report gains
        spatial_losses, spatial_status, loss_spatial and acc_spatial.  spatial=None (default): nothing more is launched.  An
        EnsemblePredictor takes spatial=dict(shared=True, ...): ONE matrix is fitted through all members (align.EnsembleSpatialFit)
        and written to each; without the key an ensemble is refused before anything runs."""
        from .calibrate import calibrate_predictor
        return calibrate_predictor(self, trials, labels, align=align, **fit_kw)
