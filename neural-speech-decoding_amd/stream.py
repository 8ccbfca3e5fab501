"""Resumable decoding of live EEG streams on the MI355X: the model advances chunk by chunk while the samples arrive, and a decision
can be read after any chunk (nsd_stream_* of include/nsd.h, csrc/nsd_stream48.hip).

An extension: the reference decodes whole windows (SimplePredictor.predict, lstm_eeg_model.py:86-101).  EEG_LSTM itself is causal
(lstm_eeg_model.py:32-39: forward LSTM layers, a softmax pooling over time), so the probabilities read after t samples are those of
`model.predict_proba` on the first t samples, and they do not depend on how the samples were cut into chunks.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import ops
from ._lib import NsdError


_NORMALIZE_REFUSAL = ("StreamDecoder: normalize=True z-scores over the whole window, which a stream has not seen yet; "
                      "normalise the chunks causally on the caller's side, or train the model with a causal front end "
                      "(EEG_LSTM(prep=CausalPrep.design(zscore_seconds=...)))")


def _check_stream_model(model, streams, who: str, more=None) -> torch.Tensor:
    """The refusals every single-model stream decoder shares -> the model's flat parameters (on the GPU).  more: the decoder's own
    checks of its configuration, made before the model is asked where it lives"""
    from .lstm_eeg_model import EEG_LSTM
    if not isinstance(model, EEG_LSTM):
        raise NsdError(f"{who}: expected an EEG_LSTM, got {type(model).__name__}")
    if model.training:
        raise NsdError(f"{who}: the model must be in eval mode (model.eval()): a stream is decoded without dropout")
    if model.precision != "fp32" or model.spec.D != 1:
        raise NsdError(f"{who}: the bf16 sequence path and bidirectional models are not resumable (a bidirectional model is "
                       "not causal); use an fp32, one-directional EEG_LSTM")
    if model.normalize:
        raise NsdError(_NORMALIZE_REFUSAL.replace("StreamDecoder", who, 1))
    if not ops.stream_path(model.spec):
        raise NsdError(f"{who}: model shape {model.spec} is outside nsd_stream_path (hidden size 48, 2 layers, <= 8 channels, "
                       "fc width and classes <= 64)")
    if int(streams) < 1:
        raise NsdError(f"{who}: streams = {streams}")
    if more is not None:
        more()
    flat = model.flat_parameters()
    if not flat.is_cuda:
        raise NsdError(f"{who} runs only on the MI355X HIP path: move the model to the GPU first; there is no CPU fallback")
    return flat


class StreamDecoder:
    """`streams` independent live streams of one eval-mode EEG_LSTM, each with its own slot of device state.

      push(samples, slots=None, read=True)   samples [n, C] (one stream) or [B, n, C]; slots: the B slot indices (default 0 .. B-1).
                                             Returns class probabilities [B, K] of every pushed stream's whole prefix (device
                                             tensor), or None with read=False (advance only: no readout)
      reset(slots=None)                      restart all streams, or the named ones
      steps                                  samples seen per slot (int64 numpy [streams])
      state_dict() / load_state_dict()       checkpoint / restore the stream state (not the model)

    A model with a causal front end (EEG_LSTM(prep=...)) is decoded through it: the decoder owns a prep state of the same slots, push
    runs nsd_prep_step (stream mode) and then nsd_stream_step, and reset / state_dict / load_state_dict cover both states.
    A model with a signal-quality gate (EEG_LSTM(gate=...)) adds a gate state of the same slots: push runs nsd_gate_step -> (nsd_prep_step)
    -> nsd_gate_apply -> the step; a rejected step is NaN, so this decoder and the ensemble one read NaN until the slot is reset, while the
    sliding decoders lose exactly the windows that contain it.  quality(slots=None) reports what the gate has seen.
    A model with session alignment (EEG_LSTM(align=...)) adds a table of one matrix per slot, each the model's matrix at first, and a
    second-moment accumulator per slot: push ends its front end with nsd_spatial_apply (sel = the slots), and
      align_accumulate(on)                   nsd_cov_step inside push, behind the gate's apply and in front of the spatial apply
      refit_alignment(slots=None)            one nsd_whiten_fit from the accumulators into those slots' matrices; nothing is read back
      alignment(slots=None)                  (matrices [n,C,C] numpy, records) in one copy
      set_alignment(slots, W)                write matrices; reset_alignment(slots): back to the model's matrix, accumulators zero
    reset() restarts a stream, not its session: the matrices and the accumulators stay.
    A model with a rate conversion (EEG_LSTM(resample=...)) is pushed samples at the amplifier's rate: push runs nsd_resample_step
    (stream mode) in front of everything above, on a resample state of the same slots, and the stages behind it -- and `steps` --
    count samples at the model's rate; input_steps counts the amplifier's.  A host mirror of every slot's sample count gives the
    number of steps a push emits without a read-back (slots given as a device tensor are read once).  The mirror follows push / reset /
    load_state_dict only: a caller who replays captured launches on the decoder's states must go through a checkpoint (state_dict ->
    load_state_dict, which reads the counts from the state) before pushing eagerly.  The streams of one push must
    emit the same number of steps: a push whose slots would not is refused before any launch -- push those slots separately.  A push
    that emits no step (a chunk shorter than M / L samples can) advances the rate conversion alone and returns None (a sliding
    decoder: no decisions).
    state_dict() carries the session with the stream: the matrix table, the accumulators and the records of the last fits
    (align_records), so alignment() of a restored decoder returns what the original's returns; a checkpoint written before the records
    travelled loads with all-zero records ("never refitted").  align_accumulate's switch is configuration, not state: it does not
    travel, and a restored decoder accumulates only once it is told to.
    """

    def __init__(self, model, streams: int = 1):
        flat = _check_stream_model(model, streams, "StreamDecoder")
        self.model, self.streams, self.device = model, int(streams), flat.device
        self._layout = ops.stream_layout(model.spec)
        self.state = ops.stream_state(model.spec, self.streams, self.device)
        self._init_front(model)

    def _init_front(self, model) -> None:
        """What runs in front of the model's step, each with a state of the decoder's slots: the signal-quality gate (model.gate) and
        the causal front end (model.prep).  Their outputs go to one set of buffers per chunk shape: push allocates nothing new."""
        C_ = model.spec.C
        self.resample = getattr(model, "resample", None)
        self.resample_state = None if self.resample is None else ops.resample_state(C_, self.resample, self.streams, self.device)
        self._resampled = {}                                # (chunk shape, steps) -> (all rows the call may write, the steps it emitted)
        self._n_in = np.zeros(self.streams, np.int64)       # the host's mirror of every slot's n_in
        self.prep = model.prep
        self.prep_state = None if self.prep is None else ops.prep_state(C_, self.streams, self.device)
        self._prepped = {}
        self.gate = getattr(model, "gate", None)
        self.gate_state = None if self.gate is None else ops.gate_state(C_, self.streams, self.device)
        self._gated = {}                                    # chunk shape -> (held samples, mask words)
        self.align = getattr(model, "align", None)
        if self.align is not None:
            S = self.streams
            self.align_table = model.align_matrix.detach().to(self.device).unsqueeze(0).repeat(S, 1, 1).contiguous()
            self.cov_state = ops.cov_state(C_, S, self.device)
            self.align_records = torch.zeros((S, ops.WHITEN_RECORD_BYTES), dtype=torch.uint8, device=self.device)
            self._all_slots = torch.arange(S, dtype=torch.int32, device=self.device)
            self._accumulate = False
            self._aligned = {}                              # chunk shape -> output (a model without gate and prep: x is the caller's)

    def _front(self, x: torch.Tensor, slots) -> torch.Tensor:
        """gate -> prep -> apply on a chunk, in stream mode: a bad channel is held through the front end and zeroed behind it, a step
        that is bad on too many channels is NaN -- the decoders' poison contract then gives "no decision" where it belongs."""
        mask = None
        if self.gate is not None:
            bufs = self._gated.get(tuple(x.shape))
            if bufs is None:
                bufs = self._gated[tuple(x.shape)] = (torch.empty_like(x), torch.empty(tuple(x.shape[:2]), dtype=torch.int32,
                                                                                         device=x.device))
            x, mask = ops.gate_step(x, self.gate, self.gate_state, slots=slots, out=bufs[0], mask=bufs[1])
        if self.prep is not None:
            out = self._prepped.get(tuple(x.shape))
            if out is None:
                out = self._prepped[tuple(x.shape)] = torch.empty_like(x)
            x = ops.prep_step(x, self.prep, self.prep_state, slots=slots, out=out)
        if mask is not None:
            x = ops.gate_apply(x, self.gate, mask, out=x)
        if self.align is not None:
            if self._accumulate:
                ops.cov_step(x, self.cov_state, mask=mask, slots=slots)
            out = x
            if self.gate is None and self.prep is None:
                out = self._aligned.get(tuple(x.shape))
                if out is None:
                    out = self._aligned[tuple(x.shape)] = torch.empty_like(x)
            x = ops.spatial_apply(x, self.align_table, sel=slots if slots is not None else self._all_slots[:x.shape[0]], out=out)
        return x

    # ---- session alignment ----
    def _need_align(self, who: str) -> None:
        if self.align is None:
            raise NsdError(f"{type(self).__name__}.{who}: the model has no session alignment (EEG_LSTM(align=SessionAlign(...)))")

    def align_accumulate(self, on: bool = True) -> None:
        """Turn the second-moment accumulator inside push on or off (off at first): every pushed step that is finite and clean of
        gate bits is added to its slot's sums."""
        self._need_align("align_accumulate")
        self._accumulate = bool(on)

    @torch.no_grad()
    def refit_alignment(self, slots=None) -> None:
        """One nsd_whiten_fit from the accumulators of all slots, or the named ones, into those slots' matrices and records.  Nothing
        is read back; a slot with fewer than the configuration's min_steps used steps gets the identity (record: few)."""
        self._need_align("refit_alignment")
        C_, S = self.model.spec.C, self.streams
        if slots is None:
            ops.whiten_fit(C_, self.align, state=self.cov_state, group=self._all_slots, G=S, out=self.align_table,
                           records=self.align_records.view(-1))
            return
        idx = self._slots(slots)
        n, at = int(idx.numel()), idx.long()
        group = torch.full((S,), -1, dtype=torch.int32, device=self.device)
        group[at] = self._all_slots[:n]
        W, rec = ops.whiten_fit(C_, self.align, state=self.cov_state, group=group, G=n)
        self.align_table.index_copy_(0, at, W)
        self.align_records.index_copy_(0, at, rec.view(n, -1))

    def alignment(self, slots=None):
        """(matrices float32 numpy [n,C,C], the n records of their last fit as dicts) of all slots or the named ones, in one copy.  A
        slot that was never refitted has an all-zero record."""
        self._need_align("alignment")
        at = self._all_slots.long() if slots is None else self._slots(slots).long()
        n, C_ = int(at.numel()), self.model.spec.C
        raw = torch.cat([self.align_table[at].view(n, -1).view(torch.uint8), self.align_records[at]], dim=1).cpu()
        W = raw[:, :4 * C_ * C_].contiguous().view(torch.float32).view(n, C_, C_).numpy().copy()
        return W, ops.whiten_records(raw[:, 4 * C_ * C_:].contiguous().view(-1), n)

    @torch.no_grad()
    def set_alignment(self, slots, W) -> None:
        """Write W ([C,C] for every named slot, or [n,C,C]) into the named slots' matrices (slots None: all)."""
        self._need_align("set_alignment")
        at = self._all_slots.long() if slots is None else self._slots(slots).long()
        C_ = self.model.spec.C
        W = torch.as_tensor(W, dtype=torch.float32).to(self.device)
        if tuple(W.shape) not in ((C_, C_), (int(at.numel()), C_, C_)):
            raise NsdError(f"{type(self).__name__}.set_alignment: W must be [{C_},{C_}] or [{int(at.numel())},{C_},{C_}], got {tuple(W.shape)}")
        self.align_table[at] = W
        self.align_records[at] = 0

    @torch.no_grad()
    def reset_alignment(self, slots=None) -> None:
        """The named slots (None: all) go back to the model's matrix, their accumulators to zero."""
        self._need_align("reset_alignment")
        self.set_alignment(slots, self.model.align_matrix)
        ops.cov_reset(self.model.spec.C, self.cov_state, self._slots(slots))

    def _resample_push(self, x: torch.Tensor, slots, idx) -> Optional[torch.Tensor]:
        """Stage 0 on a chunk at the amplifier's rate -> the chunk at the model's rate, or None where it emits no step.  idx: the
        pushed slots on the host.  The count comes from the mirror; mixed counts are refused before any launch."""
        r, T = self.resample, int(x.shape[1])
        held = self._n_in[idx]                              # (idx: a slice, or an index array)
        counts = -((-(held + T) * r.L) // r.M) + ((-held * r.L) // r.M)          # ceil((n+T) L / M) - ceil(n L / M), all slots at once
        n = int(counts[0])
        if (counts != n).any():
            raise NsdError(f"{type(self).__name__}.push: the pushed streams hold {held.tolist()} samples and a chunk of {T} would emit "
                           f"{sorted(set(counts.tolist()))} steps at L / M = {r.L} / {r.M}: push those slots separately")
        most = r.out_steps(0, T)                            # ceil(T L / M): the rows the call may write
        key = (tuple(x.shape), n)
        bufs = self._resampled.get(key)
        if bufs is None:
            full = torch.empty((x.shape[0], most, x.shape[2]), dtype=torch.float32, device=x.device)
            bufs = self._resampled[key] = (full, full if n == most else torch.empty((x.shape[0], n, x.shape[2]), dtype=torch.float32,
                                                                                   device=x.device))
        full, cut = bufs
        ops.resample_step(x, r, self.resample_state, slots=slots, out=full)
        self._n_in[idx] += T
        if n == 0:
            return None
        if cut is not full:
            cut.copy_(full[:, :n])                          # (a chunk that emits floor(T L / M) steps: the stages behind want them dense)
        return cut

    def _no_steps(self, x: torch.Tensor):
        """What push returns where the chunk emitted no step at the model's rate."""
        return None

    @property
    def input_steps(self) -> np.ndarray:
        """Samples pushed per slot since its reset, at the rate they were pushed at (int64 numpy [streams]); `steps` counts the
        model's."""
        return self._n_in.copy() if getattr(self, "resample", None) is not None else self.steps

    def _reset_front(self, slots) -> None:
        C_ = self.model.spec.C
        if getattr(self, "resample", None) is not None:
            ops.resample_reset(C_, self.resample, self.resample_state, slots)
            if slots is None:
                self._n_in[:] = 0
            else:
                self._n_in[[int(v) for v in slots.cpu().tolist()]] = 0
        if self.prep is not None:
            ops.prep_reset(C_, self.prep_state, slots)
        if self.gate is not None:
            ops.gate_reset(C_, self.gate_state, slots)

    def _front_state_dict(self, sd: dict) -> dict:
        if getattr(self, "resample", None) is not None:
            sd["resample_state"] = self.resample_state.detach().cpu().clone()
            sd["resample_n_in"] = self._state_n_in(sd["resample_state"]).clone()     # (the state's own words, not the mirror)
        if self.prep is not None:
            sd["prep_state"] = self.prep_state.detach().cpu().clone()
        if self.gate is not None:
            sd["gate_state"] = self.gate_state.detach().cpu().clone()
        if self.align is not None:
            sd["align_table"] = self.align_table.detach().cpu().clone()
            sd["cov_state"] = self.cov_state.detach().cpu().clone()
            sd["align_records"] = self.align_records.detach().cpu().clone()
        return sd

    def _check_front_state(self, sd: dict, who: str):
        rs, mine = sd.get("resample_state"), getattr(self, "resample", None)
        if (rs is None) != (mine is None) or (rs is not None and tuple(rs.shape) != tuple(self.resample_state.shape)):
            raise NsdError(f"{who}: the checkpoint and the decoder differ in their rate conversion's state")
        if rs is not None:
            self._checked_n_in(sd)
        ps, gs = sd.get("prep_state"), sd.get("gate_state")
        if (ps is None) != (self.prep is None) or (ps is not None and tuple(ps.shape) != tuple(self.prep_state.shape)):
            raise NsdError(f"{who}: the checkpoint and the decoder differ in their causal front end's state")
        if (gs is None) != (self.gate is None) or (gs is not None and tuple(gs.shape) != tuple(self.gate_state.shape)):
            raise NsdError(f"{who}: the checkpoint and the decoder differ in their signal-quality gate's state")
        at, cs = sd.get("align_table"), sd.get("cov_state")
        if ((at is None) != (self.align is None) or (cs is None) != (self.align is None)
                or (at is not None and (tuple(at.shape) != tuple(self.align_table.shape) or tuple(cs.shape) != tuple(self.cov_state.shape)))):
            raise NsdError(f"{who}: the checkpoint and the decoder differ in their session alignment's state")
        ar = sd.get("align_records")                        # (a checkpoint from before the records travelled has none: zero records)
        if ar is not None and (at is None or tuple(ar.shape) != tuple(self.align_records.shape)):
            raise NsdError(f"{who}: the checkpoint and the decoder differ in their session alignment's records")
        return ps, gs, at, cs, ar

    def _state_n_in(self, rs: torch.Tensor) -> torch.Tensor:
        """The n_in words of a resample state on the host -> int64 [streams]."""
        col = int(ops.resample_layout(self.model.spec.C, self.resample).n_in) // 2
        return rs.to(torch.float32).contiguous().view(torch.int64)[:, col]

    def _checked_n_in(self, sd: dict) -> np.ndarray:
        """The counts a checkpoint's resample_state holds; a "resample_n_in" beside it that disagrees with them is refused."""
        held = self._state_n_in(sd["resample_state"].detach().cpu()).numpy().astype(np.int64)
        given = sd.get("resample_n_in")
        if given is not None:
            given = np.asarray(given.cpu().numpy() if torch.is_tensor(given) else given, np.int64).reshape(-1)
            if given.shape != held.shape or (given != held).any():
                raise NsdError(f"{type(self).__name__}.load_state_dict: resample_n_in {given.tolist()} disagrees with the counts "
                               f"{held.tolist()} inside resample_state")
        return held

    def _load_resample_state(self, sd: dict) -> None:
        """The rate conversion's state and the host's mirror of its counts (checked by _check_front_state, before anything is
        written).  The mirror is derived from the state's own n_in words, never taken from the checkpoint's copy of a mirror."""
        rs = sd.get("resample_state")
        if rs is None:
            return
        held = self._checked_n_in(sd)
        self.resample_state.copy_(rs.to(self.device, dtype=torch.float32))
        self._n_in[:] = held

    def _load_front_state(self, ps, gs, at=None, cs=None, ar=None) -> None:
        if ps is not None:
            self.prep_state.copy_(ps.to(self.device, dtype=torch.float32))
        if gs is not None:
            self.gate_state.copy_(gs.to(self.device, dtype=torch.float32))
        if at is not None:
            self.align_table.copy_(at.to(self.device, dtype=torch.float32))
            self.cov_state.copy_(cs.to(self.device, dtype=torch.float64))
            if ar is not None:
                self.align_records.copy_(ar.to(self.device, dtype=torch.uint8))
            else:
                self.align_records.zero_()

    def quality(self, slots=None) -> dict:
        """What the signal-quality gate has seen per slot since its reset, read from its state in one copy: {"bad_fraction": [n, C]
        (bad samples / samples, per channel), "rejected_fraction": [n] (rejected steps / samples), "steps": int64 [n]} as numpy
        arrays, for all slots or the named ones."""
        if self.gate is None:
            raise NsdError(f"{type(self).__name__}.quality: the model has no signal-quality gate (EEG_LSTM(gate=SignalGate(...)))")
        if slots is not None:
            slots = [int(v) for v in self._slots(slots).cpu().tolist()]
        return ops.gate_quality(self.model.spec.C, self.gate_state, slots)

    def _slots(self, slots, n: Optional[int] = None) -> Optional[torch.Tensor]:
        if slots is None:
            return None
        if not torch.is_tensor(slots):
            idx = [int(v) for v in np.asarray(slots).reshape(-1)]
            if any(v < 0 or v >= self.streams for v in idx) or len(set(idx)) != len(idx):
                raise NsdError(f"{type(self).__name__}: slots {idx} must be distinct indices in [0, {self.streams})")
            slots = torch.tensor(idx, dtype=torch.int32)
        slots = slots.to(device=self.device, dtype=torch.int32).contiguous().reshape(-1)
        if n is not None and int(slots.numel()) != n:
            raise NsdError(f"{type(self).__name__}: {int(slots.numel())} slots for {n} streams")
        return slots

    @torch.no_grad()
    def push(self, samples, slots=None, read: bool = True) -> Optional[torch.Tensor]:
        x = samples if torch.is_tensor(samples) else torch.from_numpy(np.ascontiguousarray(samples, dtype=np.float32))
        if x.dim() == 2:
            x = x[None]
        if x.dim() != 3 or x.shape[-1] != self.model.spec.C or x.shape[1] < 1:
            raise NsdError(f"StreamDecoder.push: samples must be [n, {self.model.spec.C}] or [B, n, {self.model.spec.C}] with n >= 1, "
                           f"got {tuple(x.shape)}")
        if x.shape[0] > self.streams:
            raise NsdError(f"StreamDecoder.push: {x.shape[0]} streams pushed, the decoder has {self.streams}")
        x = x.to(self.device, non_blocking=True).contiguous().float()
        if getattr(self, "resample", None) is not None:
            idx = (slice(0, int(x.shape[0])) if slots is None
                   else np.asarray(slots.cpu().tolist() if torch.is_tensor(slots) else slots, dtype=np.int64).reshape(-1))
            slots = self._slots(slots, int(x.shape[0]))
            xr = self._resample_push(x, slots, idx)
            if xr is None:
                return self._no_steps(x)
            x = xr
        else:
            slots = self._slots(slots, int(x.shape[0]))
        return self._step(self._front(x, slots), slots, read)

    def _step(self, x: torch.Tensor, slots, read: bool) -> Optional[torch.Tensor]:
        _, probs = ops.stream_step(self.model.spec, self.model.flat_parameters(), x, self.state, slots=slots,
                                   residual=self.model.residual, read=read)
        return probs

    def features(self, slots=None) -> torch.Tensor:
        """The pooled vector each slot holds, [n, H] (device tensor; all slots, or the named ones): the vector whose read-out the slot's
        decision is -- what nsd_amd.HeadFit calibrates the read-out on.  A slot that was never pushed gives a NaN row."""
        return ops.stream_features(self.model.spec, self.state, slots=self._slots(slots))

    def reset(self, slots=None) -> None:
        slots = self._slots(slots)
        ops.stream_reset(self.model.spec, self.state, slots)
        self._reset_front(slots)

    @property
    def steps(self) -> np.ndarray:
        col = int(self._layout.steps) // 2
        return self.state.view(torch.int64)[:, col].cpu().numpy().copy()

    def state_dict(self) -> dict:
        return self._front_state_dict({"state": self.state.detach().cpu().clone(), "stride": int(self._layout.stride)})

    def load_state_dict(self, sd: dict) -> None:
        who = f"{type(self).__name__}.load_state_dict"
        st = sd["state"]
        if tuple(st.shape) != tuple(self.state.shape) or int(sd.get("stride", st.shape[-1])) != int(self._layout.stride):
            raise NsdError(f"{who}: state of shape {tuple(st.shape)} for a decoder of {tuple(self.state.shape)}")
        front = self._check_front_state(sd, who)
        self.state.copy_(st.to(self.device, dtype=torch.float32))
        self._load_front_state(*front)
        self._load_resample_state(sd)


def _check_ensemble(dec, models, streams, who: str, path):
    """The refusals every ensemble stream decoder shares, and the members' stacked parameters: sets dec.members / model (member 0) /
    streams / params [M,P] / device -> (members, first).  models: a sequence of EEG_LSTM, or the ensemble an EnsemblePredictor holds
    (its stacked parameter buffer is then used, not a copy).  path(first, M): the decoder's own check of shape and configuration"""
    from .lstm_eeg_model import EEG_LSTM
    from .multimodel import _check_models
    params = getattr(models, "params", None)
    members = list(getattr(models, "models", models))
    for m in members:
        if not isinstance(m, EEG_LSTM):
            raise NsdError(f"{who}: expected EEG_LSTM members, got {type(m).__name__}")
    _check_models(members, who)
    first = members[0]
    if any(m.training for m in members):
        raise NsdError(f"{who}: the models must be in eval mode (model.eval()): a stream is decoded without dropout")
    if first.normalize:
        raise NsdError(_NORMALIZE_REFUSAL.replace("StreamDecoder", who, 1))
    path(first, len(members))
    if int(streams) < 1:
        raise NsdError(f"{who}: streams = {streams}")
    if not all(m.flat_parameters().is_cuda for m in members):
        raise NsdError(f"{who} runs only on the MI355X HIP path: move the models to the GPU first; there is no CPU fallback")
    dec.members, dec.model, dec.streams = members, first, int(streams)
    dec.params = params if params is not None else torch.stack([m.flat_parameters() for m in members]).contiguous()
    dec.device = dec.params.device
    return members, first


class EnsembleStreamDecoder(StreamDecoder):
    """`streams` independent live streams decoded by an ensemble of M eval-mode EEG_LSTM models of one shape: every push advances all
    M models in one launch (nsd_multi_stream_step) and returns the mean of their class probabilities.  StreamDecoder's surface:

      push(samples, slots=None, read=True)   -> mean probabilities [B, K] (device tensor; a serial fp32 sum over the models divided by
                                             M), or None with read=False
      member_probs                           the models' own probabilities [M, B, K] of the last read: bit for bit what M StreamDecoders
                                             return (None before the first read)
      reset(slots=None), steps               as StreamDecoder's (a slot is reset in every model; the models' step counts agree)
      state_dict() / load_state_dict()       the [M, S, stride] state (+ the front end's)

    models: a sequence of EEG_LSTM (checked as EnsemblePredictor checks them: one shape and options, fp32, one direction), or the
    ensemble an EnsemblePredictor holds (its stacked [M, P] parameter buffer is then used, not a copy).  The members share one causal
    front end (equal `prep`): one prep state of S slots, nsd_prep_step once per push, its output read by all models."""

    def __init__(self, models, streams: int = 1):
        who = "EnsembleStreamDecoder"

        def path(first, M):
            if not ops.multi_stream_path(first.spec, M):
                raise NsdError(f"{who}: {M} models of shape {first.spec} are outside nsd_multi_stream_path (nsd_stream_path: hidden "
                               "size 48, 2 layers, <= 8 channels, fc width and classes <= 64; 1 <= M <= 32)")
        members, first = _check_ensemble(self, models, streams, who, path)
        self._layout = ops.stream_layout(first.spec)
        self.state = ops.multi_stream_state(first.spec, len(members), self.streams, self.device)
        self._init_front(first)
        self.member_probs: Optional[torch.Tensor] = None

    def _step(self, x: torch.Tensor, slots, read: bool) -> Optional[torch.Tensor]:
        _, probs, mean = ops.multi_stream_step(self.model.spec, self.params, x, self.state, slots=slots, residual=self.model.residual,
                                               read=read)
        if read:
            self.member_probs = probs
        return mean

    def features(self, slots=None) -> torch.Tensor:
        """The pooled vector of each slot in every model, [M, n, H] (device tensor): the ensemble's state read as M*S flat slots"""
        slots = self._slots(slots)
        M, S = len(self.members), self.streams
        if slots is None:
            return ops.stream_features(self.model.spec, self.state).view(M, S, -1)
        every = (slots[None, :] + S * torch.arange(M, dtype=torch.int32, device=self.device)[:, None]).reshape(-1).contiguous()
        return ops.stream_features(self.model.spec, self.state, slots=every).view(M, int(slots.numel()), -1)

    def reset(self, slots=None) -> None:
        slots = self._slots(slots)
        M, S = len(self.members), self.streams
        flat = self.state.view(M * S, -1)
        if slots is None:
            ops.stream_reset(self.model.spec, flat)
        else:                                               # slot s of every model: m*S + s of the flat state
            every = (slots[None, :] + S * torch.arange(M, dtype=torch.int32, device=self.device)[:, None]).reshape(-1).contiguous()
            ops.stream_reset(self.model.spec, flat, every)
        self._reset_front(slots)

    @property
    def steps(self) -> np.ndarray:
        col = int(self._layout.steps) // 2
        return self.state[0].view(torch.int64)[:, col].cpu().numpy().copy()


class SlidingStreamDecoder(StreamDecoder):
    """`streams` continuous (uncued) streams of one eval-mode EEG_LSTM: every `hop` samples, the decision of the model run from a zero
    state over the last `window` samples -- nsd_window_step, one launch per chunk whatever the chunk's place against the hops.
    window and hop in samples: 1 <= hop <= window, window % hop == 0, window / hop <= 128.

      push(samples, slots=None)      samples [n, C] or [B, n, C] -> (probs [B, D, K], ends int64 [B, D], counts int32 [B]), device tensors,
                                     D = ceil(n / hop), no host synchronisation: rows 0 .. counts[b]-1 of stream b are the windows the
                                     chunk completed, in ascending end (ends[b, i]: samples since the reset at which window i ended);
                                     the other rows are NaN / -1.  The buffers are reused by the next push of the same chunk shape.
                                     Row i is bit for bit what a StreamDecoder returns when it is reset and fed that window.
      latest()                       per slot the most recent completed window's (end, probs float32 [K]), or None before the first
      reset(slots=None), steps       restart streams; samples seen per slot since its reset (int64 numpy [streams])
      state_dict() / load_state_dict()   checkpoint / restore in the middle of a stream; a checkpoint of another (window, hop) is refused

    A model with a causal front end (EEG_LSTM(prep=...)) is decoded through it: ONE prep state of the same slots runs continuously over
    the stream (it is not restarted per window), and the windows are cut from its output."""

    def __init__(self, model, streams: int = 1, *, window: int, hop: int):
        who = "SlidingStreamDecoder"

        def config():
            if not ops.window_path(model.spec, window, hop):
                raise NsdError(f"{who}: window = {window}, hop = {hop} samples are outside nsd_window_path (1 <= hop <= window, "
                               "window % hop == 0, window / hop <= 128)")
        flat = _check_stream_model(model, streams, who, config)
        self.model, self.streams, self.device = model, int(streams), flat.device
        self.window, self.hop = int(window), int(hop)
        self._layout = ops.window_layout(model.spec, self.window, self.hop)
        self.state = ops.window_state(model.spec, self.window, self.hop, self.streams, self.device)
        self._init_front(model)
        self._all = torch.arange(self.streams, dtype=torch.int64, device=self.device)
        self._last_end = torch.full((self.streams,), -1, dtype=torch.int64, device=self.device)
        self._last_probs = torch.full((self.streams, model.spec.K), float("nan"), dtype=torch.float32, device=self.device)

    @torch.no_grad()
    def push(self, samples, slots=None):
        return super().push(samples, slots, True)

    def _step(self, x: torch.Tensor, slots, read: bool):
        _, probs, ends, counts = ops.window_step(self.model.spec, self.model.flat_parameters(), x, self.state, window=self.window,
                                                 hop=self.hop, slots=slots, residual=self.model.residual)
        self._keep_latest(int(x.shape[0]), slots, probs, ends, counts)
        return probs, ends, counts

    def _keep_latest(self, B: int, slots, probs: torch.Tensor, ends: torch.Tensor, counts: torch.Tensor) -> None:
        # the newest completed window of every pushed stream, kept on the device (the output buffers are reused)
        idx = self._all[:B] if slots is None else slots.long()
        has = counts > 0
        row = (counts.long() - 1).clamp_(min=0)
        self._last_end[idx] = torch.where(has, ends.gather(1, row[:, None])[:, 0], self._last_end[idx])
        newest = probs.gather(1, row[:, None, None].expand(-1, 1, probs.shape[2]))[:, 0]
        self._last_probs[idx] = torch.where(has[:, None], newest, self._last_probs[idx])

    def _no_steps(self, x: torch.Tensor):
        B = int(x.shape[0])
        return (torch.empty((B, 0, self.model.spec.K), dtype=torch.float32, device=x.device),
                torch.empty((B, 0), dtype=torch.int64, device=x.device), torch.zeros((B,), dtype=torch.int32, device=x.device))

    def features(self, slots=None):
        raise NsdError(f"{type(self).__name__}.features: a sliding decoder's phase slots are in the middle of their windows; read the "
                       "pooled features of cued trials from a StreamDecoder (open_stream without window_seconds)")

    def latest(self) -> list:
        ends, probs = self._last_end.cpu().numpy(), self._last_probs.cpu().numpy()
        return [None if int(e) < 0 else (int(e), probs[s].copy()) for s, e in enumerate(ends)]

    def reset(self, slots=None) -> None:
        slots = self._slots(slots)
        ops.window_reset(self.model.spec, self.window, self.hop, self.state, slots)
        self._reset_front(slots)
        idx = self._all if slots is None else slots.long()
        self._last_end[idx] = -1
        self._last_probs[idx] = float("nan")

    @property
    def steps(self) -> np.ndarray:
        col = int(self._layout.count) // 2
        return self.state.view(torch.int64)[:, col].cpu().numpy().copy()

    def state_dict(self) -> dict:
        sd = {"state": self.state.detach().cpu().clone(), "window": self.window, "hop": self.hop,
              "last_end": self._last_end.cpu().clone(), "last_probs": self._last_probs.cpu().clone()}
        return self._front_state_dict(sd)

    def load_state_dict(self, sd: dict) -> None:
        who = f"{type(self).__name__}.load_state_dict"
        if (int(sd.get("window", -1)), int(sd.get("hop", -1))) != (self.window, self.hop):
            raise NsdError(f"{who}: a checkpoint of window = {sd.get('window')}, hop = {sd.get('hop')} for a decoder of window = "
                           f"{self.window}, hop = {self.hop}")
        st = sd["state"]
        if tuple(st.shape) != tuple(self.state.shape):
            raise NsdError(f"{who}: state of shape {tuple(st.shape)} for a decoder of {tuple(self.state.shape)}")
        front = self._check_front_state(sd, who)
        self.state.copy_(st.to(self.device, dtype=torch.float32))
        self._load_front_state(*front)
        self._load_resample_state(sd)
        self._last_end.copy_(sd["last_end"].to(self.device))
        self._last_probs.copy_(sd["last_probs"].to(self.device))


class EnsembleSlidingStreamDecoder(SlidingStreamDecoder):
    """`streams` continuous (uncued) streams decoded by an ensemble of M eval-mode EEG_LSTM models of one shape: every `hop` samples the
    mean of the M decisions over the last `window` samples -- nsd_multi_window_step, one launch per chunk for all models (and one small
    launch for the mean).  SlidingStreamDecoder's surface:

      push(samples, slots=None)      -> (mean probs [B, D, K], ends int64 [B, D], counts int32 [B]), device tensors, no host
                                     synchronisation.  A mean row is the serial fp32 sum of the members' rows divided by M, and NaN
                                     where any member's row is (an unused row, a poisoned window, a skipped member); ends / counts are
                                     model 0's.  The buffers are reused by the next push of the same chunk shape.
      member_probs                   the models' own probabilities [M, B, D, K] of the last push: bit for bit what M
                                     SlidingStreamDecoders return (None before the first push)
      latest()                       per slot the most recent completed window's (end, mean probs float32 [K]), or None
      reset(slots=None), steps       a stream is reset in every model (m*S + s of the flat state) and in the front end; the samples
                                     seen per slot (the models' counts agree)
      state_dict() / load_state_dict()   the [M, S, stream_stride] state, window, hop, the last decisions (+ the front end's state); a
                                     checkpoint of another shape, M, window or hop is refused

    models: as EnsembleStreamDecoder's -- a sequence of EEG_LSTM of one shape and options, or the ensemble an EnsemblePredictor holds
    (its stacked [M, P] parameter buffer is then used, not a copy).  The members share one causal front end (equal `prep`): one prep
    state of S slots runs continuously over the stream, nsd_prep_step once per push, its output read by all models."""

    def __init__(self, models, streams: int = 1, *, window: int, hop: int):
        who = "EnsembleSlidingStreamDecoder"

        def path(first, M):
            if not ops.multi_window_path(first.spec, window, hop, M):
                raise NsdError(f"{who}: {M} models of shape {first.spec} with window = {window}, hop = {hop} samples are outside "
                               "nsd_multi_window_path (nsd_stream_path: hidden size 48, 2 layers, <= 8 channels, fc width and classes "
                               "<= 64; nsd_window_path: 1 <= hop <= window, window % hop == 0, window / hop <= 128; 1 <= M <= 32)")
        members, first = _check_ensemble(self, models, streams, who, path)
        self.window, self.hop = int(window), int(hop)
        self._layout = ops.window_layout(first.spec, self.window, self.hop)
        self.state = ops.multi_window_state(first.spec, self.window, self.hop, len(members), self.streams, self.device)
        self._init_front(first)
        self._all = torch.arange(self.streams, dtype=torch.int64, device=self.device)
        self._last_end = torch.full((self.streams,), -1, dtype=torch.int64, device=self.device)
        self._last_probs = torch.full((self.streams, first.spec.K), float("nan"), dtype=torch.float32, device=self.device)
        self.member_probs: Optional[torch.Tensor] = None

    def _step(self, x: torch.Tensor, slots, read: bool):
        _, probs, mean, ends, counts = ops.multi_window_step(self.model.spec, self.params, x, self.state, window=self.window, hop=self.hop,
                                                             slots=slots, residual=self.model.residual)
        self.member_probs = probs
        self._keep_latest(int(x.shape[0]), slots, mean, ends[0], counts[0])
        return mean, ends[0], counts[0]

    def reset(self, slots=None) -> None:
        slots = self._slots(slots)
        M, S = len(self.members), self.streams
        flat = self.state.view(M * S, -1)
        if slots is None:
            ops.window_reset(self.model.spec, self.window, self.hop, flat)
        else:                                               # stream s of every model: m*S + s of the flat state
            every = (slots[None, :] + S * torch.arange(M, dtype=torch.int32, device=self.device)[:, None]).reshape(-1).contiguous()
            ops.window_reset(self.model.spec, self.window, self.hop, flat, every)
        self._reset_front(slots)
        idx = self._all if slots is None else slots.long()
        self._last_end[idx] = -1
        self._last_probs[idx] = float("nan")

    @property
    def steps(self) -> np.ndarray:
        col = int(self._layout.count) // 2
        return self.state[0].view(torch.int64)[:, col].cpu().numpy().copy()


class PredictorStream:
    """What SimplePredictor.open_stream returns: numpy chunks in, (probs float32 [B, K], labels) out -- predict(), chunk by chunk.
    A predictor with `members` (EnsemblePredictor) is decoded by all of them: an EnsembleStreamDecoder, the probabilities are their mean."""

    def __init__(self, predictor, streams: int, chunk_transform=None):
        self.predictor, self.chunk_transform = predictor, chunk_transform
        ensemble = getattr(predictor, "members", None) is not None
        self.decoder = EnsembleStreamDecoder(predictor.model, streams) if ensemble else StreamDecoder(predictor.model, streams)

    def push(self, chunk: np.ndarray, slots=None, read: bool = True):
        x = np.asarray(chunk)
        if x.ndim == 2:
            x = x[None]
        if x.ndim != 3:
            raise ValueError(f"Expected [n, C] or [B, n, C] samples, got {x.shape}")
        f = self.chunk_transform or self.predictor.pre.transform
        x = np.stack([np.ascontiguousarray(f(c), dtype=np.float32) for c in x])
        probs = self.decoder.push(x, slots=slots, read=read)
        if probs is None:
            return None
        p = probs.cpu().numpy().astype(np.float32)
        return p, [self.predictor.class_names[int(i)] for i in p.argmax(1)]

    def reset(self, slots=None) -> None:
        self.decoder.reset(slots)

    @property
    def steps(self) -> np.ndarray:
        return self.decoder.steps


class PredictorSlidingStream:
    """What SimplePredictor.open_stream(window_seconds=, hop_seconds=) returns: numpy chunks of a continuous stream in; per stream a
    list of (end_sample, probs float32 [K], label) out, one entry per window the chunk completed (a SlidingStreamDecoder of `window`
    and `hop` samples).  A predictor with `members` (EnsemblePredictor) is decoded by all of them: an EnsembleSlidingStreamDecoder, the
    probabilities are their mean."""

    def __init__(self, predictor, streams: int, chunk_transform, window: int, hop: int):
        self.predictor, self.chunk_transform = predictor, chunk_transform
        ensemble = getattr(predictor, "members", None) is not None
        self.decoder = (EnsembleSlidingStreamDecoder if ensemble else SlidingStreamDecoder)(predictor.model, streams, window=window, hop=hop)

    def push(self, chunk: np.ndarray, slots=None) -> list:
        x = np.asarray(chunk)
        if x.ndim == 2:
            x = x[None]
        if x.ndim != 3:
            raise ValueError(f"Expected [n, C] or [B, n, C] samples, got {x.shape}")
        f = self.chunk_transform or self.predictor.pre.transform
        x = np.stack([np.ascontiguousarray(f(c), dtype=np.float32) for c in x])
        probs, ends, counts = (t.cpu().numpy() for t in self.decoder.push(x, slots=slots))
        names = self.predictor.class_names
        return [[(int(ends[b, i]), probs[b, i].astype(np.float32), names[int(probs[b, i].argmax())]) for i in range(max(int(counts[b]), 0))]
                for b in range(x.shape[0])]

    def reset(self, slots=None) -> None:
        self.decoder.reset(slots)

    @property
    def steps(self) -> np.ndarray:
        return self.decoder.steps
