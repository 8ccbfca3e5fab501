"""The composed reference of the SERVING front end, and the table of rows the serve-pipeline tests run.

ServeRef states what a stream decoder's step must see, chunk by chunk and slot by slot, for the four decoders of nsd_amd/stream.py
(StreamDecoder, EnsembleStreamDecoder, SlidingStreamDecoder, EnsembleSlidingStreamDecoder).  It is built ONLY from the per-stage
restatements under tests/ -- gate_ref.State / gate_ref / apply_ref, prep_ref.State / prep_ref, align_ref.cov_ref (sums= / counts= carried)
and align_ref.apply_ref (sel=), window_ref.completed -- in the order the StreamDecoder docstring states,

    gate -> prep -> gate-apply -> (second-moment accumulator) -> spatial apply (sel = the slots) -> the decoder's step,

on four per-slot states (gate, prep, accumulator, matrix table) and the sample count of the slot.  The rules it encodes are the
documented ones: outside training the apply stage rejects with the gate's own max_bad; the accumulator sees what stands behind the
gate's apply, under the gate's mask; reset(slots) restarts gate, prep and the sample count and leaves matrices, records and
accumulators; set_alignment writes matrices and zeroes their records; reset_alignment goes back to the model's matrix and zeroes the
accumulators; a state_dict carries all of it, and not the accumulate switch.

The whitening link.  nsd_whiten_fit has no bitwise restatement (tests/test_gpu_align.py holds it to FIT_BOUND of a float64 eigh), so a
refit in the chain is THE KERNEL ITSELF, as the z-score is in tests/pipeline_ref.py: ServeRef.refit(slots, W) takes the matrices; the GPU
tests read them back from the decoder (and hold them to align_ref.whiten_ref of the reference's own accumulators at FIT_BOUND), the
CPU tests pass whiten_ref's float64 result rounded to float32 (host_fit).

window_ref_windows(x) is the same chain from fresh states over whole trials: what EEG_LSTM.forward (eval), predict_proba and
predict_trials must feed the model.

CASES is the table: two full-chain blocks (gate + prep + align in each of the four decoders, once pushed eagerly and once replayed
from a captured graph), a pairwise cover of FACTORS over the allowed combinations (tests/test_serve_pipeline_cpu.py proves the cover
by enumeration) and one row beyond the pairs: a reset with gate, prep, align and the accumulators all present.  Imports without a GPU.
"""
import copy
from collections import namedtuple

import numpy as np

from tests import align_ref, gate_ref, prep_ref, window_ref
from tests.pipeline_ref import GATE, PREP

F32 = np.float32
STAGES = ("gate", "prep", "apply", "cov", "align")       # the documented order


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _differs(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape != b.shape or not np.array_equal(_bits(a), _bits(b))


def _take(state, idx):
    """the slots idx of a restatement's State as a State of len(idx) streams (copies)"""
    sub = copy.copy(state)
    for k, v in vars(state).items():
        setattr(sub, k, v[idx].copy())
    return sub


def _put(state, idx, sub):
    for k, v in vars(sub).items():
        getattr(state, k)[idx] = v


ZERO_RECORD = dict(steps=0, skipped=0, status=0)


class ServeRef:
    """Per-slot state machine of a decoder's front end.  S slots of C channels; gate: the gate's fields (SignalGate.to_dict()) or
    None; prep: prep_ref's keywords or None; align: the model's matrix [C,C] or None; window, hop: of a sliding decoder, else None.
    accumulate: the switch align_accumulate sets (configuration: snapshot / restore do not carry it)."""

    def __init__(self, S, C, *, gate=None, prep=None, align=None, window=None, hop=None, accumulate=False):
        self.S, self.C, self.gate, self.prep, self.window, self.hop = int(S), int(C), gate, prep, window, hop
        self.accumulate = bool(accumulate)
        self.g = gate_ref.State(S, C) if gate is not None else None
        self.p = prep_ref.State(S, C) if prep is not None else None
        self.W0 = None if align is None else np.array(align, F32)
        if self.W0 is not None:
            assert self.W0.shape == (C, C)
            self.table = np.repeat(self.W0[None], S, axis=0)
            self.sums, self.counts = np.zeros((S, C, C), np.float64), np.zeros((S, 2), np.int64)
            self.records = [dict(ZERO_RECORD) for _ in range(S)]
        self.n = np.zeros(S, np.int64)                    # samples since the slot's reset
        self.nan_at = [[] for _ in range(S)]              # ... and which of them reached the decoder's step with a NaN in them
        self.trace = {}                                   # stage -> did it change the bits of its input, in the last push

    def _idx(self, slots, B=None):
        idx = list(range(self.S if B is None else B)) if slots is None else [int(s) for s in np.asarray(slots).reshape(-1)]
        assert len(set(idx)) == len(idx) and all(0 <= s < self.S for s in idx) and (B is None or len(idx) == B)
        return idx

    def push(self, chunk, slots=None):
        """chunk [B,n,C] of the streams in `slots` (None: 0 .. B-1) -> (what the decoder's step must see, float32 [B,n,C]; the gate's
        mask words uint32 [B,n] or None; per stream the [(end, row, poisoned)] of the windows the chunk completes, or None for a decoder
        that is not sliding)"""
        v = np.ascontiguousarray(chunk, dtype=F32)
        B, n, C = v.shape
        assert C == self.C and n >= 1
        idx = self._idx(slots, B)
        self.trace, mask = {}, None
        if self.g is not None:
            sub = _take(self.g, idx)
            w, mask = gate_ref.gate_ref(v, self.gate, sub)
            _put(self.g, idx, sub)
            self.trace["gate"], v = _differs(v, w), w
        if self.p is not None:
            sub = _take(self.p, idx)
            w = prep_ref.prep_ref(v, state=sub, **self.prep)
            _put(self.p, idx, sub)
            self.trace["prep"], v = _differs(v, w), w
        if mask is not None:
            w = gate_ref.apply_ref(v, mask, self.gate)                 # outside training: the gate's own max_bad
            self.trace["apply"], v = _differs(v, w), w
        if self.W0 is not None:
            if self.accumulate:
                s, c = align_ref.cov_ref(v, mask, sums=self.sums[idx], counts=self.counts[idx])
                self.trace["cov"] = bool((c != self.counts[idx]).any())
                self.sums[idx], self.counts[idx] = s, c
            w = align_ref.apply_ref(v, self.table, sel=idx)
            self.trace["align"], v = _differs(v, w), w
        bad = np.isnan(v).any(axis=2)
        windows = None if self.window is None else []
        for b, s in enumerate(idx):
            n0 = int(self.n[s])
            self.nan_at[s] += [n0 + int(t) for t in np.flatnonzero(bad[b])]
            if windows is not None:
                windows.append([(end, row, any(end - self.window <= t < end for t in self.nan_at[s]))
                                for _, end, row in window_ref.completed(n0, n, self.window, self.hop)])
            self.n[s] = n0 + n
        return np.ascontiguousarray(v, dtype=F32), mask, windows

    def poisoned(self, slot):
        """a decoder that is not sliding reads NaN from the first NaN step until the slot's reset"""
        return bool(self.nan_at[int(slot)])

    def reset(self, slots=None):
        """a stream restarts, not its session: gate, prep and the sample count; matrices, records and accumulators stay"""
        idx = self._idx(slots)
        if self.g is not None:
            _put(self.g, idx, gate_ref.State(len(idx), self.C))
        if self.p is not None:
            _put(self.p, idx, prep_ref.State(len(idx), self.C))
        for s in idx:
            self.n[s], self.nan_at[s] = 0, []

    def set_alignment(self, slots, W):
        idx = self._idx(slots)
        self.table[idx] = np.asarray(W, F32)
        for s in idx:
            self.records[s] = dict(ZERO_RECORD)

    def reset_alignment(self, slots=None):
        idx = self._idx(slots)
        self.set_alignment(idx, self.W0)
        self.sums[idx], self.counts[idx] = 0.0, 0

    def refit(self, slots, W):
        """the whitening link (module docstring): W [n,C,C] float32 are the matrices nsd_whiten_fit gave the named slots (None: all)"""
        idx = self._idx(slots)
        W = np.asarray(W, F32)
        assert W.shape == (len(idx), self.C, self.C)
        self.table[idx] = W
        for s in idx:
            self.records[s] = dict(steps=int(self.counts[s, 0]), skipped=int(self.counts[s, 1]), status=None)   # status: the fit's own

    def host_fit(self, slots, align_cfg):
        """what the CPU tests hand to refit(): whiten_ref of the reference's own accumulators, float64 rounded once -> (W, records)"""
        idx = self._idx(slots)
        out = [align_ref.whiten_ref(self.sums[s:s + 1], self.counts[s:s + 1], **align_cfg) for s in idx]
        return np.stack([w[0] for w, _ in out]), [r[0] for _, r in out]

    def snapshot(self):
        """what a state_dict round trip must preserve: everything but the accumulate switch"""
        keep = {k: copy.deepcopy(v) for k, v in vars(self).items() if k not in ("accumulate", "trace")}
        return keep

    def restore(self, snap, accumulate=False):
        """a FRESH reference loaded from a snapshot (the switch is the new decoder's own)"""
        for k, v in snap.items():
            setattr(self, k, copy.deepcopy(v))
        self.accumulate, self.trace = bool(accumulate), {}
        return self

    def quality(self, slots=None):
        q = self.g.quality()
        idx = self._idx(slots)
        return {k: v[idx] for k, v in q.items()}

    def gate_rows(self):
        return self.g.slot_rows()                         # uint32 [S, stride]

    def prep_rows(self):
        return self.p.slot_rows()                         # float32 [S, stride]


def same_snapshot(a, b):
    """two ServeRef.snapshot()s hold the same bits"""
    def eq(u, v):
        if isinstance(u, (gate_ref.State, prep_ref.State)):
            return all(eq(getattr(u, k), getattr(v, k)) for k in vars(u))
        if isinstance(u, np.ndarray):
            return u.shape == v.shape and u.dtype == v.dtype and u.tobytes() == v.tobytes()
        return u == v
    return set(a) == set(b) and all(eq(a[k], b[k]) for k in a)


def window_ref_windows(x, *, gate=None, prep=None, align=None, trace=None):
    """x [B,T,C] whole trials -> what forward (eval) / predict_proba / predict_trials must feed the model: the chain from fresh states;
    outside training the apply stage uses the gate's own max_bad.  trace: receives stage -> changed the bits"""
    v, mask = np.ascontiguousarray(x, dtype=F32), None
    trace = {} if trace is None else trace
    if gate is not None:
        w, mask = gate_ref.gate_ref(v, gate)
        trace["gate"], v = _differs(v, w), w
    if prep is not None:
        w = prep_ref.prep_ref(v, **prep)
        trace["prep"], v = _differs(v, w), w
    if mask is not None:
        w = gate_ref.apply_ref(v, mask, gate)
        trace["apply"], v = _differs(v, w), w
    if align is not None:
        w = align_ref.apply_ref(v, np.asarray(align, F32))
        trace["align"], v = _differs(v, w), w
    return np.ascontiguousarray(v, dtype=F32)


# ------------------------------------------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------------------------------------------
# The smallest shapes at which the composition can go wrong: the reference model (C = 8, H = 48, L = 2, K = 3; the second ensemble
# member is its scale = 0.9 twin), S = 4 slots, B = 3 pushed streams (2 in the partial level), T = 70 samples per stream, windows of 20
# samples every 10.
C, K, S, B, T, M = 8, 3, 4, 3, 70, 2
WINDOW, HOP = 20, 10
SLOT_LIST = [3, 0, 2]                # a permuted subset of the S slots
CUTS = {"7-1-32-30": [7, 1, 32, 30], "13s": [13, 13, 13, 13, 13, 5], "whole": [70], "ones-58": [1] * 12 + [58], "14s": [14] * 5}
# 14s: the one fixed chunk length (off the hop grid) a captured graph can replay; replayed rows run it, and eager rows may.
POISON_AT, POISON_STREAM = 34, 1     # sample 34 (0-based) of pushed stream 1: first or last sample of no chunk of any cut, inside the
                                     # windows that end at 40 and 50 (counted from a reset behind 12 samples: those ending at 30 and 40);
                                     # the windows ending at 20 and 30 are whole before it, so even a stream that stays poisoned (a NaN
                                     # through prep without a gate) has two finite decisions
RAIL_AT = (18, 21, 27)               # stream i rails channel i at sample RAIL_AT[i]: the gate fires in every stream
EVENT_STREAM, SET_STREAM = 1, 0      # reset / refit / reset_alignment name the slot of pushed stream 1, set_alignment that of stream 0
EVENT_AFTER = 35                     # an event stands at the first chunk boundary at or after this many samples, else at the last one
                                     # in front of the final chunk ("ones-58": after 12 samples)
ALIGN = dict(shrinkage=0.1, floor=1e-4, min_steps=10)          # SessionAlign's fields: a refit after 12 samples is a fit, not "few", and
                                     # behind PREP's common average reference (a covariance one direction short of singular) the
                                     # shrinkage keeps every eigenvalue above the floor: status 0, nothing clipped

FACTORS = dict(
    decoder=("stream", "ens-stream", "sliding", "ens-sliding"),
    gate=(0, 1), prep=(0, 1), align=(0, 1),
    slots=("default", "list", "tensor", "partial"),      # 0 .. B-1; SLOT_LIST as a Python list; as an int32 device tensor; B = 2 of S = 4
    cut=tuple(CUTS),
    event=("none", "reset", "state_dict", "refit", "set-reset"),
    # reset: of the slot of pushed stream 1;  state_dict: state_dict() -> a FRESH decoder of the same model -> go on with it (with align:
    # behind a refit of stream 0's slot);  refit: refit_alignment of stream 1's slot;  set-reset: set_alignment of stream 0's slot, then
    # reset_alignment of stream 1's
    poison=("none", "nan", "pop"),
    drive=("eager", "replay"))
# Rows with align and an event accumulate from the start (align_accumulate(True)), so that the accumulators are there for reset, state_dict
# and reset_alignment to keep, carry or clear; rows without an event run with the switch off (no nsd_cov_step is launched).


def refused(c):
    """Why a combination of levels is no row (None: it is one)."""
    if c["event"] in ("refit", "set-reset") and not c["align"]:
        return "StreamDecoder._need_align: the model has no session alignment"
    if c["poison"] == "pop" and not c["gate"]:
        return "a three-channel pop is a rejected step only where a gate counts bad channels"
    if c["event"] != "none" and c["cut"] == "whole":
        return "an event stands between two chunks; one chunk has no such place"
    if c["drive"] == "replay" and c["cut"] != "14s":
        return "a captured graph replays one chunk shape: the cut is one fixed length"
    return None


Case = namedtuple("Case", "id decoder gate prep align slots cut event poison drive")
_ROWS = [
    # gate + prep + align in each of the four decoders, pushed eagerly: a permuted slot list, a refit between chunks, a rejected step
    (0,  "stream",      1, 1, 1, "list",    "7-1-32-30", "refit",      "pop",  "eager"),
    (1,  "ens-stream",  1, 1, 1, "list",    "7-1-32-30", "refit",      "pop",  "eager"),
    (2,  "sliding",     1, 1, 1, "list",    "7-1-32-30", "refit",      "pop",  "eager"),
    (3,  "ens-sliding", 1, 1, 1, "list",    "7-1-32-30", "refit",      "pop",  "eager"),
    # ... and replayed from a captured graph: the slots as a device tensor, a state_dict into a fresh decoder, a NaN sample
    (4,  "stream",      1, 1, 1, "tensor",  "14s",       "state_dict", "nan",  "replay"),
    (5,  "ens-stream",  1, 1, 1, "tensor",  "14s",       "state_dict", "nan",  "replay"),
    (6,  "sliding",     1, 1, 1, "tensor",  "14s",       "state_dict", "nan",  "replay"),
    (7,  "ens-sliding", 1, 1, 1, "tensor",  "14s",       "state_dict", "nan",  "replay"),
    # the pairwise cover
    (8,  "ens-stream",  0, 0, 0, "partial", "ones-58",   "none",       "none", "eager"),
    (9,  "sliding",     0, 1, 0, "default", "13s",       "reset",      "nan",  "eager"),
    (10, "ens-sliding", 0, 0, 1, "list",    "14s",       "set-reset",  "none", "replay"),
    (11, "stream",      1, 0, 0, "default", "whole",     "none",       "pop",  "eager"),
    (12, "sliding",     0, 0, 0, "tensor",  "7-1-32-30", "state_dict", "none", "eager"),
    (13, "stream",      1, 1, 1, "partial", "13s",       "set-reset",  "none", "eager"),
    (14, "sliding",     1, 0, 0, "partial", "14s",       "reset",      "pop",  "replay"),
    (15, "ens-sliding", 0, 0, 1, "default", "ones-58",   "refit",      "nan",  "eager"),
    (16, "ens-sliding", 0, 1, 1, "partial", "whole",     "none",       "nan",  "eager"),
    (17, "sliding",     1, 1, 1, "tensor",  "ones-58",   "set-reset",  "pop",  "eager"),
    (18, "stream",      0, 1, 1, "list",    "ones-58",   "reset",      "none", "eager"),
    (19, "ens-sliding", 1, 0, 0, "list",    "13s",       "state_dict", "pop",  "eager"),
    (20, "ens-stream",  0, 0, 1, "default", "7-1-32-30", "set-reset",  "nan",  "eager"),
    (21, "sliding",     0, 1, 0, "default", "14s",       "none",       "none", "replay"),
    (22, "ens-stream",  1, 1, 1, "tensor",  "13s",       "refit",      "none", "eager"),
    (23, "ens-stream",  0, 1, 0, "tensor",  "whole",     "none",       "none", "eager"),
    (24, "sliding",     0, 1, 0, "list",    "whole",     "none",       "nan",  "eager"),
    (25, "ens-stream",  0, 1, 0, "partial", "7-1-32-30", "reset",      "none", "eager"),
    (26, "ens-sliding", 0, 1, 0, "tensor",  "14s",       "reset",      "nan",  "eager"),
    (27, "ens-stream",  0, 1, 1, "partial", "14s",       "refit",      "nan",  "replay"),
    (28, "sliding",     1, 1, 1, "default", "ones-58",   "state_dict", "none", "eager"),
    (29, "stream",      1, 1, 0, "partial", "13s",       "state_dict", "pop",  "eager"),
    (30, "ens-stream",  0, 0, 0, "tensor",  "13s",       "none",       "nan",  "eager"),
    (31, "ens-sliding", 1, 0, 0, "default", "7-1-32-30", "none",       "none", "eager"),
    # beyond the pairs: reset(slot) with gate, prep, align and the accumulators all present -- it must restart the first two and the
    # decoder's state and leave the matrices and accumulators; the rejected step lies before it, so the reset slot decides again
    (32, "stream",      1, 1, 1, "list",    "13s",       "reset",      "pop",  "eager"),
]
CASES = [Case(*r) for r in _ROWS]
FULL_CHAIN_IDS = (0, 1, 2, 3, 4, 5, 6, 7)


def case_id(c):
    on = "".join(ch for ch, f in zip("GPL", (c.gate, c.prep, c.align)) if f) or "none"
    return f"{c.id:02d}-{c.decoder}-{on}-{c.slots}-{c.cut}-{c.event}-{c.poison}-{c.drive}"


def sliding(c):
    return c.decoder in ("sliding", "ens-sliding")


def ensemble(c):
    return c.decoder in ("ens-stream", "ens-sliding")


def poison_reaches_the_step(c):
    """a pop is a rejected step (NaN behind the gate's apply); a NaN sample is one bad channel to a gate, which holds it, and a NaN
    step to a front end without one"""
    return c.poison == "pop" or (c.poison == "nan" and not c.gate)


def nan_by_position(c):
    """the rows in which a NaN is COMPUTED from a NaN input: a NaN sample reaches nsd_prep_step (no gate holds it), whose arithmetic
    spreads it over the channels and its states.  For such a NaN the project's rule is prep_ref.same_bits': finite values bitwise, NaNs
    by position (the sign of a NaN result is open in IEEE 754, and host and GPU differ in it).  Every other row compares every word."""
    return bool(c.prep) and not c.gate and c.poison == "nan"


def pushed(c):
    """-> (B, the slots argument as the level states it: None, or the list -- the GPU tests make the tensor of it)"""
    if c.slots == "partial":
        return 2, None
    return B, (None if c.slots == "default" else list(SLOT_LIST))


def slot_of(c, stream):
    _, slots = pushed(c)
    return stream if slots is None else slots[stream]


def event_chunk(c):
    """the event stands behind this chunk of the cut (None: no event)"""
    if c.event == "none":
        return None
    ends = np.cumsum(CUTS[c.cut])[:-1]
    late = [k for k, e in enumerate(ends) if e >= EVENT_AFTER]
    return int(late[0]) if late else len(ends) - 1


def accumulates(c):
    return bool(c.align) and c.event != "none"


# ------------------------------------------------------------------------------------------------------------------------------------
# the settings and inputs of a row
# ------------------------------------------------------------------------------------------------------------------------------------
def settings(c):
    """-> dict(model: EEG_LSTM's front-end keywords (without the matrix), ref: ServeRef's keywords (without align=))"""
    import nsd_amd
    gate = nsd_amd.SignalGate(**GATE) if c.gate else None
    prep = nsd_amd.CausalPrep.design(**PREP) if c.prep else None
    return dict(model=dict(gate=gate, prep=prep, align=nsd_amd.SessionAlign(**ALIGN) if c.align else None),
                ref=ref_settings(gate, prep, WINDOW if sliding(c) else None))


def ref_settings(gate, prep, window=None):
    return dict(gate=gate.to_dict() if gate else None,
                prep=dict(sections=prep.sections, alpha=prep.alpha, var0=prep.var0, baseline=prep.baseline, car=prep.car) if prep else None,
                window=window, hop=HOP if window else None)


def signal(n, rs, poison="none"):
    """n streams of T samples as pipeline_ref._trials makes them: clean noise of 10 units, and stream i rails channel i at RAIL_AT[i];
    the poison (one NaN sample, or a pop on three channels: more than the gate's max_bad) at sample POISON_AT of POISON_STREAM"""
    x = np.clip(10.0 * rs.standard_normal((n, T, C)), -40, 40).astype(F32)
    for i in range(n):
        x[i, RAIL_AT[i], i] = 300.0 if i % 2 == 0 else -300.0
    if poison == "nan":
        x[POISON_STREAM, POISON_AT, 5] = np.nan
    elif poison == "pop":
        x[POISON_STREAM, POISON_AT, 1:4] = 500.0
    return x


def matrices(n, rs):
    """non-symmetric alignment matrices near the identity [n,C,C]"""
    return (np.eye(C) + 0.15 * rs.standard_normal((n, C, C))).astype(F32)


def inputs(c):
    """-> dict(x [B,T,C], W0: the model's matrix (or None), Wset: what set_alignment writes)"""
    rs = np.random.RandomState(2000 + c.id)
    n, _ = pushed(c)
    x = signal(n, rs, c.poison)
    W = matrices(2, rs)
    return dict(x=x, W0=W[0] if c.align else None, Wset=W[1] if c.align else None)


def new_ref(c, inp=None, st=None):
    inp, st = inp or inputs(c), st or settings(c)
    return ServeRef(S, C, align=inp["W0"], accumulate=accumulates(c), **st["ref"])


def apply_event(c, ref, inp, fit=None):
    """the row's event on the reference.  fit(slots) -> the matrices of the refit (the whitening link).  -> the reference to go on with
    (a fresh one behind a state_dict)"""
    _, slots = pushed(c)
    one, other = slot_of(c, EVENT_STREAM), slot_of(c, SET_STREAM)
    if c.event == "reset":
        ref.reset([one])
    elif c.event == "state_dict":
        if c.align:                                       # behind a refit, so that the records the checkpoint must carry are not all zero
            ref.refit([other], fit([other]))
        ref = new_ref(c, inp).restore(ref.snapshot(), accumulate=accumulates(c))
    elif c.event == "refit":
        ref.refit([one], fit([one]))
    elif c.event == "set-reset":
        ref.set_alignment([other], inp["Wset"])
        ref.reset_alignment([one])
    return ref


def run_ref(c, cut=None, fit=None, inp=None):
    """the whole row on the reference -> (ref, [(out, mask, windows, trace) per chunk]).  fit: as apply_event's; None: host_fit"""
    inp, st = inp or inputs(c), settings(c)
    ref = new_ref(c, inp, st)
    _, slots = pushed(c)
    cut = CUTS[c.cut] if cut is None else cut
    at = event_chunk(c) if cut == CUTS[c.cut] else None
    out, t = [], 0
    for k, n in enumerate(cut):
        o, m, w = ref.push(inp["x"][:, t:t + n], slots)
        out.append((o, m, w, dict(ref.trace)))
        t += n
        if at is not None and k == at:
            ref = apply_event(c, ref, inp, fit or (lambda sl, r=ref: r.host_fit(sl, ALIGN)[0]))
    return ref, out


def expected_stages(c):
    on = dict(gate=c.gate, prep=c.prep, apply=c.gate, cov=accumulates(c), align=c.align)
    return [s for s in STAGES if on[s]]
