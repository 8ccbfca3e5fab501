"""The serving front end -- gate -> prep -> gate-apply -> (second-moment accumulator) -> spatial apply -> the decoder's step -- held to ONE
composed reference (tests/serve_ref.py) on the MI355X, in each of the four decoders of nsd_amd/stream.py and on the whole-window
surfaces of EEG_LSTM, with and without the rate conversion (stage 0) in front.

Two layers per row of serve_ref.CASES, both BIT FOR BIT (uint32 / uint64 words: a NaN in the right place with the right payload
passes, anywhere else fails; the file holds no tolerance of its own -- the one bound it uses, FIT_BOUND of the whitening link, is
imported from tests/test_gpu_align.py):
  A  dec._front(chunk, slots) chunk by chunk against ServeRef.push, with the row's event between two chunks: the output chunk, the gate's
     mask words, the gate and prep states of ALL slots against the restatements' slot_rows() (unpushed rows keep their bits), the
     accumulators (float64 words) and their counts, the matrix table, quality(); the caller's chunk checked unchanged;
  B  push on the decoder under test against a PLAIN decoder of the same class -- same weights, no front end -- pushed layer A's REFERENCE
     chunks with the same slots and events (alignment events do not apply to it): probabilities (ensemble: mean and member_probs), ends /
     counts / latest() of the sliding ones, steps and the whole state tensor after every chunk.  Replayed rows capture
     dec._step(dec._front(x_static, slots), slots, True) once in a graph on a side stream, after a warm-up on a throw-away decoder, and
     replay it per chunk; an eager decoder under test runs beside it and must give the same bits.
A state_dict event continues on a FRESH decoder (in a replayed row: with a capture of its own); with alignment the checkpoint is taken
behind a refit, so that the records it must carry are not all zero, and a copy of it without "align_records" must load with zero
records.  A refit is the kernel itself in the chain (serve_ref's docstring) and is held to whiten_ref of the reference's accumulators.
Per row the decisions are counted: every stream the reference calls unpoisoned ends with a finite decision (sliding: at least two
finite windows), and a decision is NaN exactly where ServeRef says.
One test outside the table holds model(x) in eval mode, predict_proba and predict_trials of all eight stage subsets to the plain model on
window_ref_windows(x), and the streamed front end to the same windows.

NaNs.  Every NaN the chain WRITES or CARRIES is held to its bits: the rejected step of nsd_gate_apply, the NaNs through
nsd_spatial_apply and the decoders' steps, in every row.  A NaN COMPUTED from a NaN input compares by position, as everywhere in this
project (prep_ref.same_bits: "the quiet-NaN pattern differs between the host and the GPU" -- a subtraction with a NaN operand gives
0xffc00000 on the device and keeps 0x7fc00000 on the host; IEEE 754 leaves that sign open).  That can occur only where a NaN sample
reaches nsd_prep_step, so the rule is applied only in the rows with prep on, the gate off and the NaN poison
(serve_ref.nan_by_position); there such words are counted and printed.  Every other row asserts exact words.

Behind a rate conversion (the rows with rate 1/2 and 5/8: stage 0, nsd_resample_step, in front of the chain) the chunks are at the
amplifier's rate.  Layer A then runs the front end through push itself with the step taken out -- the count from the host mirror, the
dense copy and the buffer cache are host logic of push -- and adds stage 0's output (every row the call may write, NaN behind the emitted
ones: the count), the resample state of all slots word for word and input_steps against the reference's counts.  A chunk that emits no
step must return None (a sliding decoder: empty decisions) and move nothing but stage 0; layer B skips it.  Behind a reset at a count
with n L mod M != 0 the slots emit different counts: once per such row the streams are pushed together and the documented refusal is
asserted with every word of every state unchanged, then the chunk goes by ServeRef.groups().  Replayed rows capture
ops.resample_step(x_static, r, dec.resample_state, slots, out=buf) in front of the same unit.  A replayed decoder's mirror never moves,
and the mirror is never trusted over the state: its checkpoint's resample_n_in must equal the n_in words of the resample_state it
carries, a disagreeing key is refused with nothing written, and a fresh decoder loaded from it goes on eagerly with a chunk of 3 samples
bit for bit.  (A fixed replayed length is a multiple of M, so a stale mirror stays in phase and cuts the right rows; what it gets wrong
is the count itself -- tests/test_resample_cpu.py shows the wrong cut with a stand-in launch of another length.)

Measured on one MI355X, the file against nothing but itself: 51 rows, 106 tests, 2.7 s from import to the last test (pytest: 5.0 s with
start-up); at the parent commit 33 rows, 68 tests, 1.8 s (3.7 s): 1.5 times the time for 1.55 times the rows.  7503 tensor comparisons
of 2 487 692 words; 34 093 of them are NaN in the reference, 987 of those with the other sign on the device, all in layer A or B of the
by-position rows 09 16 24 26 27 (in the rate rows 37 and 40 the device's NaNs had the host's bits in this run; the rule stays).

That the rows bite: nine Python-only mutants of stream.py / lstm_eeg_model.py, each computing something else through the same launches,
each run once against this file and once against the older GPU files of the touched feature, never committed.  Rows by their number
in serve_ref.CASES (A, B: the layers); "W": the whole-window test.
  mutant                                              this file                                          the older GPU files
  (a) spatial_apply in front of gate_apply            A+B 00-07 13 17 22 28 32 (every gate+align row), W test_gpu_align: 1 fails; test_gpu_gate: passes
  (b) cov_step behind spatial_apply                   A 00-07 10 13 15 17 18 20 22 27 28 32 (every       test_gpu_align: 3 fail
                                                      accumulating row); B where a refit follows
  (c) cov_step without the mask                       A 00-07 13 17 22 28 32; B 00-07 22                 test_gpu_align: 1 fails; test_gpu_gate: passes
  (d) sel always _all_slots[:B]                       A+B 00-07 10 17 22 (listed slots whose matrices    align, stream, window, multi_*: all 261 pass
                                                      differ: behind a refit or set_alignment)
  (e) _reset_front skipping the gate state            A 14 32 (the reset rows with a gate)               test_gpu_gate: 2 fail
  (f) reset also zeroing cov_state                    A 18 32 (the reset rows with align)                test_gpu_align: 1 fails
  (g) ensemble reset of flat slot s, not m*S + s      B 25 26 (against the single decoders per member)   test_gpu_multi_stream: 1, test_gpu_multi_window: 2 fail
  (h) _load_front_state not restoring prep_state      A+B 04-07 28 29 (every state_dict row with prep)   test_gpu_prep: 1, test_gpu_gate: 1 fail
  (i) predict_trials cutting before the front end     W                                                  test_gpu_align: 1, test_gpu_gate: 2 fail
None is equivalent on the device.  tests/test_serve_pipeline_cpu.py fails under (a)-(g) by its order, selection and reset checks; (h)
and (i) need the device.  (e) and (f) show in layer A only: with a rail-only gate a stale gate state changes counters, not samples,
and nothing reads the accumulators behind that reset.

Ten more for stage 0, Python-only mutants of stream.py / align.py, tried the same way on a scratch copy and never committed.  "S":
tests/test_gpu_resample_surfaces.py; "W0": test_whole_window_surfaces_convert_the_rate_first; "R": the 8 decoder cases of
tests/test_gpu_resample.py (the older file); "cpu": the stand-in tests of tests/test_resample_cpu.py, test_serve_pipeline_cpu.py,
test_resample_surfaces_cpu.py.
  mutant                                              this file                                          elsewhere
   1 the mirror is not advanced on a zero-step push   A+B 33 35 38 40 41 45 47 48 (every row with such   S streams; R 8 fail; cpu
                                                      a push), W0
   2 reset(slots) leaves the mirror                   A+B 37 40-44 47 50 (every reset row)               R 8 fail; cpu
   3 the dense copy takes `most` rows, not n          A+B 33 35 37 38 40 41 43-45 47 48 50 (every row    S streams; R 4 fail; cpu
                                                      with a floor push), W0
   4 the count uses floor for both terms              A 33 35 37 38 40 41 43-45 47 48 50; B those and    S streams; R 8 fail; cpu
                                                      34 36; W0
   5 stage 0 runs behind the gate                     A+B 33-36 39 41-43 45 47 48 50 (every gate row),   R passes; cpu
                                                      W0
   6 state_dict drops resample_state                  A+B 34 36 48 (the state_dict rows)                 R 8 fail; cpu
   7 load_state_dict keeps a disagreeing              A+B 34 36 48                                       R passes; cpu
     resample_n_in
   8 no resample_trials line in SessionAlign.fit      passes                                             S session_align_fit, both; cpu
   9 ... in EnsembleSpatialFit.fit                    passes                                             S ensemble_spatial_fit; cpu
  10 the buffer cache keyed by the shape alone        A 33-50 (the lookup by (shape, n)); B 33 37 41 43  S streams; R passes; cpu
                                                      44 50; W0 at 1/2
Every one fails at least one test on the device and one on the host.
"""
import time

import numpy as np
import pytest
import torch

from tests import align_ref as ar
from tests import resample_ref as rr
from tests import serve_ref as sv
from tests.buffer_contract import snapshot
from tests.gpu_harness import dev, nsd, sync_at_the_end, to_dev  # noqa: F401  (fixtures)
from tests.test_gpu_align import FIT_BOUND

pytestmark = pytest.mark.gpu

IDS = [sv.case_id(c) for c in sv.CASES]
_T0 = time.perf_counter()
_SEEN = {"tensors": 0, "words": 0, "nan words": 0, "nan payloads": 0}


def _words(a):
    """-> (the array as uint32 / uint64 words, where it holds a NaN)"""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    a = np.ascontiguousarray(a)
    nan = np.isnan(a) if a.dtype.kind == "f" else np.zeros(a.shape, bool)
    return (a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind in "fiu" and a.dtype.itemsize in (4, 8) else a), nan


def _same_words(c, tag, what, got, want, by_position=False):
    """every word of got equals the word of want, NaNs included.  c: the row (None: no row).  In the rows where a NaN is computed from
    a NaN input (serve_ref.nan_by_position: no gate, a NaN sample, and prep or the rate conversion to compute with it) the project's
    rule for such a NaN holds -- finite values bitwise, NaNs by position (prep_ref.same_bits) -- and the words that differ in sign or
    payload are counted and printed.  by_position: the same rule for this tensor in any row (stage 0's own output, resample_ref.same_bits)."""
    (g, gn), (w, wn) = _words(got), _words(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (tag, what, g.shape, w.shape, g.dtype, w.dtype)
    differ = g != w
    payload = differ & gn & wn
    bad = np.argwhere(differ & ~payload if by_position or (c is not None and sv.nan_by_position(c)) else differ)
    _SEEN["tensors"] += 1
    _SEEN["words"] += int(g.size)
    _SEEN["nan words"] += int(wn.sum())
    _SEEN["nan payloads"] += int(payload.sum())
    if payload.any():
        i = tuple(np.argwhere(payload)[0])
        print(f"[{tag}] {what}: {int(payload.sum())} of {int(wn.sum())} NaN words differ in sign or payload; first at {tuple(int(v) for v in i)}: "
              f"got {int(g[i]):#x}, want {int(w[i]):#x}")
    if len(bad):
        i = tuple(bad[0])
        print(f"[{tag}] {what}: {g.size} words, {len(bad)} differ; first at {tuple(int(v) for v in i)}: got {int(g[i]):#x}, want {int(w[i]):#x}")
    assert len(bad) == 0, (tag, what)


# ---- the row's decoders ---------------------------------------------------------------------------------------------------------------
def _eval_model(nsd, dev, ref_state, scale=1.0, **kw):
    m = nsd.EEG_LSTM(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v) * np.float32(scale)) for k, v in ref_state.items()}, strict=True)
    return m.to(dev).eval()


def _factories(nsd, dev, ref_state, c, inp):
    """-> (make, plain makers): make() is a new decoder of the row's class on the row's model(s) with their front end; the plain makers
    give one of the same class on plain twins of the same weights (the second ensemble member: the scale = 0.9 twin) and, for an
    ensemble, one single-model decoder per member"""
    kw = dict(sv.settings(c)["model"])
    if c.align:
        kw["align_matrix"] = to_dev(inp["W0"], dev)
    scales = (1.0, 0.9) if sv.ensemble(c) else (1.0,)
    mine = [_eval_model(nsd, dev, ref_state, s, **kw) for s in scales]
    plain = [_eval_model(nsd, dev, ref_state, s) for s in scales]
    cls = {"stream": nsd.StreamDecoder, "ens-stream": nsd.EnsembleStreamDecoder, "sliding": nsd.SlidingStreamDecoder,
           "ens-sliding": nsd.EnsembleSlidingStreamDecoder}[c.decoder]
    more = dict(window=sv.WINDOW, hop=sv.HOP) if sv.sliding(c) else {}

    def maker(models, front):
        def make():
            dec = cls(models if sv.ensemble(c) else models[0], streams=sv.S, **more)
            if front and sv.accumulates(c):
                dec.align_accumulate(True)
            return dec
        return make
    single = {"ens-stream": nsd.StreamDecoder, "ens-sliding": nsd.SlidingStreamDecoder}.get(c.decoder)
    singles = [(lambda m=m: single(m, streams=sv.S, **more)) for m in plain] if single else []
    return maker(mine, True), [maker(plain, False)] + singles


def _slots_arg(c, dev):
    _, slots = sv.pushed(c)
    return torch.tensor(slots, dtype=torch.int32, device=dev) if c.slots == "tensor" else slots


def _refit(tag, c, dec, ref, slots):
    """refit_alignment(slots) on the decoder; its matrices go into the reference (the whitening link) and are held to whiten_ref of the
    reference's own accumulators; the other slots keep matrices and records"""
    W0, r0 = dec.alignment()
    dec.refit_alignment(slots)
    W1, r1 = dec.alignment()
    W, recs = dec.alignment(slots)
    for i, s in enumerate(slots):
        Wr, rr = ar.whiten_ref(ref.sums[s:s + 1], ref.used[s:s + 1], **sv.ALIGN)
        err, bound = float(np.abs(W[i].astype(np.float64) - Wr[0]).max()), FIT_BOUND * float(np.abs(Wr[0]).max())
        print(f"[{tag}] refit of slot {s}: steps {recs[i]['steps']} (reference {int(ref.used[s, 0])}), status {recs[i]['status']}, "
              f"|W - whiten_ref| {err:.3e} (bound {bound:.3e})")
        assert recs[i]["steps"] == int(ref.used[s, 0]) == rr[0]["steps"] and recs[i]["skipped"] == int(ref.used[s, 1])
        assert recs[i]["status"] == 0 == rr[0]["status"] and err <= bound
        assert np.array_equal(W1[s], W[i]) and r1[s] == recs[i] and not np.array_equal(W[i], W0[s])
    for s in range(sv.S):
        if s not in slots:
            _same_words(c, tag, f"matrix of slot {s} behind a refit of {slots}", W1[s], W0[s])
            assert r1[s] == r0[s], (tag, s)
    ref.refit(slots, W)


def _resample_words(dec):
    """(the word of n_in, the stride) of a slot of the decoder's resample state"""
    from nsd_amd import ops
    lay = ops.resample_layout(sv.C, dec.resample)
    return int(lay.n_in), int(lay.stride)


def _stage0_state_equals(tag, c, dec, ref, mirror=True):
    """the resample state of ALL slots, word for word (histories carry an input NaN as it came), and the host's mirror"""
    n_in, stride = _resample_words(dec)
    _same_words(c, tag, "resample state, all slots", dec.resample_state.cpu().numpy().view(np.uint32), ref.resample_rows(n_in, stride))
    if mirror:
        assert dec.input_steps.tolist() == ref.rn.tolist(), (tag, dec.input_steps, ref.rn)


def _checkpoint_counts(tag, c, dec, sd, make, ref):
    """the mirror is never trusted over the state: the checkpoint's counts are the n_in words of the state it carries (also where
    the decoder's launches were replayed and its mirror never moved), and a resample_n_in that disagrees is refused, nothing written"""
    n_in, _ = _resample_words(dec)
    words = sd["resample_state"].contiguous().view(torch.int64)[:, n_in // 2]
    assert sd["resample_n_in"].tolist() == words.tolist() == ref.rn.tolist(), (tag, sd["resample_n_in"], words, ref.rn)
    other = make()
    before = [t.clone() for t in (other.resample_state, other.state)]
    from nsd_amd import NsdError
    with pytest.raises(NsdError, match="disagrees with the counts"):
        other.load_state_dict(dict(sd, resample_n_in=sd["resample_n_in"] + 1))
    assert torch.equal(other.resample_state, before[0]) and torch.equal(other.state, before[1]) and not other.input_steps.any(), tag
    other.load_state_dict({k: v for k, v in sd.items() if k != "resample_n_in"})          # without the key: the state's own words
    assert other.input_steps.tolist() == ref.rn.tolist(), tag


def _checkpoint(tag, c, dec, make, ref=None):
    """state_dict() into a fresh decoder: it returns the same alignment, records included, and a checkpoint from before the records
    travelled loads with zero records"""
    sd = dec.state_dict()
    fresh = make()
    if c.rate != "none":
        _checkpoint_counts(tag, c, dec, sd, make, ref)
    if not c.align:
        fresh.load_state_dict(sd)
        return fresh, sd
    assert "align_records" in sd
    old = make()
    old.refit_alignment()                                 # (records that are not zero: "few" from empty accumulators)
    assert old.align_records.any().item()
    old.load_state_dict({k: v for k, v in sd.items() if k != "align_records"})
    (Wa, ra), (Wo, ro) = dec.alignment(), old.alignment()
    _same_words(c, tag, "matrices from a checkpoint without records", Wo, Wa)
    assert not old.align_records.any().item() and all(r["steps"] == 0 and r["status"] == 0 for r in ro), tag
    fresh.load_state_dict(sd)
    Wf, rf = fresh.alignment()
    _same_words(c, tag, "matrices of the restored decoder", Wf, Wa)
    _same_words(c, tag, "records of the restored decoder", fresh.align_records, dec.align_records)
    assert rf == ra and any(r["steps"] > 0 for r in rf), (tag, rf)          # (taken behind a refit: not all zero)
    return fresh, sd


def _event(tag, c, dec, ref, inp, make, plains=(), plain_makers=(), others=()):
    """the row's event on the decoder under test, on the reference, on the plain decoders (reset and state_dict only) and on `others`
    (further decoders under test) -> (dec, ref, plains, others); state_dict: fresh ones"""
    one, other = sv.slot_of(c, sv.EVENT_STREAM), sv.slot_of(c, sv.SET_STREAM)
    if c.event == "reset":
        for d in (dec,) + tuple(plains) + tuple(others):
            d.reset([one])
        ref.reset([one])
    elif c.event == "state_dict":
        if c.align:
            _refit(tag, c, dec, ref, [other])
            for d in others:
                d.refit_alignment([other])
        dec, _ = _checkpoint(tag, c, dec, make, ref)
        if c.rate != "none":
            _stage0_state_equals(tag + " restored", c, dec, ref)
        fresh = []
        for d in others:
            f = make()
            f.load_state_dict(d.state_dict())
            fresh.append(f)
        others = tuple(fresh)
        fresh = []
        for d, mk in zip(plains, plain_makers):
            f = mk()
            f.load_state_dict(d.state_dict())
            fresh.append(f)
        plains = tuple(fresh)
        ref = sv.new_ref(c, inp).restore(ref.snapshot(), accumulate=sv.accumulates(c))
    elif c.event == "refit":
        _refit(tag, c, dec, ref, [one])
        for d in others:
            d.refit_alignment([one])
    elif c.event == "set-reset":
        for d in (dec,) + tuple(others):
            d.set_alignment([other], inp["Wset"])
            d.reset_alignment([one])
        ref.set_alignment([other], inp["Wset"])
        ref.reset_alignment([one])
    return dec, ref, tuple(plains), others


# ---- layer A ------------------------------------------------------------------------------------------------------------------------
def _front_state_equals(tag, c, dec, ref, shape=None, mask=None):
    if c.gate:
        if mask is not None:
            _same_words(c, tag, "mask words", dec._gated[tuple(shape)][1], mask)
        _same_words(c, tag, "gate state, all slots", dec.gate_state, ref.gate_rows())
        for slots in (None, [2, 0]):
            got, want = dec.quality(slots), ref.quality(slots)
            assert set(got) == set(want) == {"bad_fraction", "rejected_fraction", "steps"}
            for k in want:
                _same_words(c, tag, f"quality({slots})[{k}]", np.asarray(got[k], want[k].dtype), want[k])
    if c.prep:
        _same_words(c, tag, "prep state, all slots", dec.prep_state, ref.prep_rows())
    if c.align:
        cov = dec.cov_state.cpu().numpy()
        n = sv.C * sv.C
        _same_words(c, tag, "accumulator sums", cov[:, :n], ref.sums.reshape(sv.S, n))
        _same_words(c, tag, "accumulator counts", cov[:, n:].view(np.int64), ref.used)
        _same_words(c, tag, "matrix table", dec.align_table, ref.table)
        assert bool(ref.used.any()) == sv.accumulates(c)


def _sub_arg(c, dev, subs, sl, arg):
    """the slot argument of one push: the row's own where the streams go together, else the group's slots in the row's form"""
    if len(subs) == 1:
        return arg
    return torch.tensor(sl, dtype=torch.int32, device=dev) if c.slots == "tensor" else list(sl)


def _every_word(dec):
    """every word a push may move: the states of the front end, the decoder's own, the mirror, what a sliding decoder keeps"""
    ts = [dec.state] + [getattr(dec, k, None) for k in ("resample_state", "gate_state", "prep_state", "cov_state", "align_table", "align_records",
                                                        "_last_end", "_last_probs")]
    return [None if t is None else t.detach().cpu().numpy().copy() for t in ts] + [dec.input_steps.copy(), dec.steps.copy()]


def _refused_together(tag, c, dec, chunk, arg):
    """slots at different phases pushed together: the documented refusal, and no word of any state changed"""
    from nsd_amd import NsdError
    before = _every_word(dec)
    with pytest.raises(NsdError, match="push those slots separately"):
        dec.push(chunk, arg)
    torch.cuda.synchronize()
    for a, b in zip(before, _every_word(dec)):
        assert (a is None and b is None) or a.tobytes() == b.tobytes(), tag


def _fed(dec, c, chunk, arg, nB):
    """what the decoder's step is fed for a pushed chunk.  Behind a rate conversion: through push itself -- the mirror, the count, the
    dense copy and the buffer cache are host logic of push -- with the step taken out; None where the chunk emits no step"""
    if c.rate == "none":
        return dec._front(chunk, dec._slots(arg, nB))
    seen = []
    dec._step = lambda x, slots, read: seen.append(x)
    try:
        back = dec.push(chunk, arg)
    finally:
        del dec._step
    if not seen:                                          # the documented return of a push that emits no step
        assert back is None if not sv.sliding(c) else (tuple(back[0].shape) == (nB, 0, sv.K) and tuple(back[1].shape) == (nB, 0)
                                                       and back[2].tolist() == [0] * nB)
    return seen[0] if seen else None


@pytest.mark.parametrize("c", sv.CASES, ids=IDS)
def test_the_front_end_equals_the_composed_reference(nsd, dev, ref_state, c):
    inp = sv.inputs(c)
    make, _ = _factories(nsd, dev, ref_state, c, inp)
    dec, ref = make(), sv.new_ref(c, inp)
    nB, slots = sv.pushed(c)
    arg = _slots_arg(c, dev)
    x = to_dev(inp["x"], dev)
    at, t = sv.event_chunk(c), 0
    acted, refused = {}, 0
    for k, n in enumerate(sv.cuts_of(c)):
        subs = sv.sub_pushes(c, ref, n)
        if len(subs) > 1 and not refused:                 # once per row: the streams together, in front of the pushes by groups
            _refused_together(f"{sv.case_id(c)} chunk {k}", c, dec, x[:, t:t + n].contiguous(), arg)
            _stage0_state_equals(f"{sv.case_id(c)} chunk {k} refused", c, dec, ref)
            refused += 1
        for pos, sl in subs:
            tag = f"{sv.case_id(c)} chunk {k}" + (f" streams {pos}" if len(subs) > 1 else "")
            chunk = x[pos, t:t + n].contiguous()
            snap = snapshot(chunk)
            before = None if c.rate == "none" else _every_word(dec)
            out = _fed(dec, c, chunk, _sub_arg(c, dev, subs, sl, arg), len(pos))
            torch.cuda.synchronize()
            want, mask, _ = ref.push(inp["x"][pos, t:t + n], sl)
            for s, did in ref.trace.items():
                acted[s] = acted.get(s, False) or did
            if c.rate != "none":                          # stage 0: every row the call may write (NaN behind the emitted ones: the count), its state
                full, cnt = ref.stage0
                _same_words(c, tag, "stage 0: the rows the call may write", dec._resampled[(tuple(chunk.shape), int(cnt[0]))][0], full,
                            by_position=True)
                assert (out is None) == (want is None) and (out is None or int(out.shape[1]) == int(cnt[0])), (tag, cnt)
                _stage0_state_equals(tag, c, dec, ref)
            if want is None:                              # no step: nothing behind stage 0 moved
                _front_state_equals(tag + " (no step)", c, dec, ref)
                for i, (a, b) in enumerate(zip(before, _every_word(dec))):
                    assert i in (1, len(before) - 2) or (a is None and b is None) or a.tobytes() == b.tobytes(), (tag, i)      # (1: the resample state; the mirror)
                continue
            _same_words(c, tag, "the chunk the step is fed", out, want)
            _front_state_equals(tag, c, dec, ref, want.shape, mask)
            assert snap.changed() == [], tag
            assert (out is chunk) == (not (c.gate or c.prep or c.align or c.rate != "none"))
        t += n
        if k == at:
            dec, ref, _, _ = _event(tag, c, dec, ref, inp, make)
            _front_state_equals(tag + " behind the event", c, dec, ref)
            if c.rate != "none":
                _stage0_state_equals(tag + " behind the event", c, dec, ref)
    print(f"[{sv.case_id(c)}] stages that acted: {[s for s in sv.STAGES if acted.get(s)]}; refused together: {refused}")
    assert [s for s in sv.STAGES if acted.get(s)] == sv.expected_stages(c)
    assert refused == (c.rate != "none" and c.event == "reset" and c.cut != "14s")


# ---- layer B ------------------------------------------------------------------------------------------------------------------------
class _Replayed:
    """dec._step(dec._front(x_static, slots), slots, True) captured once on a side stream and replayed per chunk.  Behind a rate
    conversion the captured unit is ops.resample_step(x_static, r, dec.resample_state, slots, out=buf) and the same on buf: the fixed
    chunk is a multiple of M, so every replay emits the ceil(n L / M) rows of buf, dense as they stand.  The decoder's host mirror
    never moves under replays (StreamDecoder's docstring: such a decoder goes through a checkpoint before it is pushed eagerly)."""

    def __init__(self, dev, nB, n, throw_away, slots_t):
        self.dev, self.slots_t = dev, slots_t
        self.x = torch.zeros((nB, n, sv.C), device=dev)
        r = throw_away.resample
        self.buf = None if r is None else torch.zeros((nB, r.out_steps(0, n), sv.C), device=dev)
        assert r is None or r.out_steps(0, n) * r.M == n * r.L
        self.side = torch.cuda.Stream(device=dev)
        self._unit(throw_away)                            # the warm-up: nothing is loaded inside a capture
        torch.cuda.synchronize(dev)

    def _unit(self, dec):
        x = self.x
        if dec.resample is not None:
            from nsd_amd import ops
            x = ops.resample_step(self.x, dec.resample, dec.resample_state, slots=self.slots_t, out=self.buf)
        return dec._step(dec._front(x, self.slots_t), self.slots_t, True)

    def capture(self, dec):
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=self.side):
            self.out = self._unit(dec)
        torch.cuda.synchronize(self.dev)

    def __call__(self, chunk):
        torch.cuda.synchronize(self.dev)                  # resets, events and checkpoints ran on the default stream: the side stream waits for none of it
        with torch.cuda.stream(self.side):
            self.x.copy_(chunk)
            self.graph.replay()
        self.side.synchronize()
        return self.out


def _decisions(dec, out):
    """what a push returned, and what the decoder holds behind it, as named host arrays -- copied at once: the output buffers of a
    chunk shape are shared by every decoder of the process and reused by the next push"""
    host = lambda t: t.detach().cpu().numpy().copy()
    got = {}
    if isinstance(out, tuple):
        got["probs"], got["ends"], got["counts"] = (host(t) for t in out)
        latest = dec.latest()
        got["latest ends"] = np.array([-1 if v is None else v[0] for v in latest], np.int64)
        got["latest probs"] = np.stack([np.full(sv.K, np.nan, np.float32) if v is None else v[1] for v in latest])
    else:
        got["probs"] = host(out)
    if getattr(dec, "member_probs", None) is not None:
        got["member_probs"] = host(dec.member_probs)
    got["steps"] = dec.steps
    got["state"] = host(dec.state)
    return got


def _no_step_return(tag, c, out, nB):
    """the documented return of a push that emits no step: None, or empty decisions from a sliding decoder"""
    if sv.sliding(c):
        probs, ends, counts = out
        assert tuple(probs.shape) == (nB, 0, sv.K) and tuple(ends.shape) == (nB, 0) and counts.tolist() == [0] * nB, tag
    else:
        assert out is None, tag


def _continues_with_an_odd_chunk(tag, c, sd, make, plain, plain_maker, ref, chunk_np, arg, dev):
    """a FRESH decoder loaded from the checkpoint `sd` -- taken from a decoder whose launches were replayed -- goes on eagerly with a
    chunk that is no multiple of M, bit for bit: the count it cuts by comes from the state"""
    import copy
    probe, twin, ref = make(), plain_maker(), copy.deepcopy(ref)
    probe.load_state_dict(sd)
    twin.load_state_dict(plain.state_dict())
    got = _decisions(probe, probe.push(to_dev(chunk_np, dev), arg))
    want, _, _ = ref.push(chunk_np, sv.pushed(c)[1])
    assert want is not None and want.shape[1] == ref.stage0[1][0] > 0
    theirs = _decisions(twin, twin.push(to_dev(want, dev), arg))
    for name in theirs:
        _same_words(c, tag, f"{name} of a restored decoder behind an odd chunk", got[name], theirs[name])
    _stage0_state_equals(tag + " odd chunk", c, probe, ref)
    print(f"[{tag}] a restored decoder cut {want.shape[1]} steps from {chunk_np.shape[1]} samples at counts {ref.rn.tolist()}")


@pytest.mark.parametrize("c", sv.CASES, ids=IDS)
def test_the_decoder_equals_a_plain_decoder_on_the_reference_chunks(nsd, dev, ref_state, c):
    inp = sv.inputs(c)
    make, plain_makers = _factories(nsd, dev, ref_state, c, inp)
    dec, plains, ref = make(), tuple(mk() for mk in plain_makers), sv.new_ref(c, inp)
    nB, slots = sv.pushed(c)
    arg = _slots_arg(c, dev)
    x = to_dev(inp["x"], dev)
    cut = sv.cuts_of(c)
    replay, others = None, ()
    if c.drive == "replay":
        assert len(set(cut)) == 1
        others = (dec,)                                   # the eager decoder under test runs beside the replayed one
        dec = make()
        replay = _Replayed(dev, nB, cut[0], make(), dec._slots(arg, nB))
        replay.capture(dec)
        dec.reset()                                       # (whatever the capture ran)
        if c.align:
            dec.reset_alignment()
    at, t = sv.event_chunk(c), 0
    finite = np.zeros(nB, np.int64)
    snap = snapshot(x)
    for k, n in enumerate(cut):
        subs = sv.sub_pushes(c, ref, n)
        assert replay is None or len(subs) == 1
        for pos, sl in subs:
            tag = f"{sv.case_id(c)} chunk {k}" + (f" streams {pos}" if len(subs) > 1 else "")
            a = _sub_arg(c, dev, subs, sl, arg)
            chunk = x[:, t:t + n] if len(subs) == 1 else x[pos, t:t + n]
            held = _every_word(dec) if c.rate != "none" else None
            out = replay(chunk) if replay is not None else dec.push(chunk, a)
            want, _, wins = ref.push(inp["x"][pos, t:t + n], sl)
            if want is None:                              # no step: the documented return, and neither the decoder's state nor its front end moved
                _no_step_return(tag, c, out, len(pos))
                for i, (u, v) in enumerate(zip(held, _every_word(dec))):
                    assert i in (1, len(held) - 2) or (u is None and v is None) or u.tobytes() == v.tobytes(), (tag, i)
                _stage0_state_equals(tag, c, dec, ref)
                continue
            got = _decisions(dec, out)
            wd = to_dev(want, dev)
            theirs = _decisions(plains[0], plains[0].push(wd, a))
            assert set(got) == set(theirs) and ("member_probs" in got) == sv.ensemble(c) and ("ends" in got) == sv.sliding(c)
            for name in theirs:
                _same_words(c, tag, name, got[name], theirs[name])
            for d in others:
                eager = _decisions(d, d.push(chunk, a))
                for name in theirs:
                    _same_words(c, tag, f"{name} of the eager decoder beside the replayed one", eager[name], theirs[name])
            if c.rate != "none":                          # stage 0's state, the replayed decoder's too; the mirror of those that were pushed
                _stage0_state_equals(tag, c, dec, ref, mirror=replay is None)
                for d in others:
                    _stage0_state_equals(tag + " (eager beside replayed)", c, d, ref)
            for m, single in enumerate(plains[1:]):       # an ensemble: member m is bit for bit a single decoder of model m
                alone = _decisions(single, single.push(wd, a))
                _same_words(c, tag, f"member_probs[{m}] against a single decoder", got["member_probs"][m], alone["probs"])
                _same_words(c, tag, f"state[{m}] against a single decoder", got["state"][m], alone["state"])
                _same_words(c, tag, f"steps against single decoder {m}", got["steps"], alone["steps"])
                if sv.sliding(c):
                    _same_words(c, tag, f"ends against single decoder {m}", got["ends"], alone["ends"])
                    _same_words(c, tag, f"counts against single decoder {m}", got["counts"], alone["counts"])
            # the decisions against the reference's word: NaN exactly where it says, finite everywhere else
            probs = got["probs"]
            assert got["steps"].tolist() == ref.n.tolist(), tag
            if sv.sliding(c):
                ends, counts = got["ends"], got["counts"]
                for i, b in enumerate(pos):
                    assert int(counts[i]) == len(wins[i]) and [int(e) for e in ends[i, :counts[i]]] == [e for e, _, _ in wins[i]], (tag, b)
                    assert [r for _, r, _ in wins[i]] == list(range(len(wins[i]))) and (ends[i, counts[i]:] == -1).all(), (tag, b)
                    for e, r, poisoned in wins[i]:
                        assert np.isnan(probs[i, r]).all() if poisoned else np.isfinite(probs[i, r]).all(), (tag, b, e, poisoned)
                        finite[b] += not poisoned
                    assert np.isnan(probs[i, counts[i]:]).all(), (tag, b)
            else:
                for i, b in enumerate(pos):
                    poisoned = ref.poisoned(sv.slot_of(c, b))
                    assert np.isnan(probs[i]).all() if poisoned else np.isfinite(probs[i]).all(), (tag, b, poisoned)
                    finite[b] = not poisoned              # (of the last chunk)
        t += n
        if k == at:
            was = dec
            dec, ref, plains, others = _event(tag, c, dec, ref, inp, make, plains, plain_makers, others)
            if replay is not None and c.event == "state_dict":         # a fresh decoder: a capture of its own, then the checkpoint again
                sd = dec.state_dict()
                if c.rate != "none":                      # ... taken from the REPLAYED decoder, whose mirror never moved
                    assert not was.input_steps.any() and ref.rn.any()
                    _continues_with_an_odd_chunk(tag, c, was.state_dict(), make, plains[0], plain_makers[0], ref, inp["x"][:, t:t + 3], arg, dev)
                replay.capture(dec)
                dec.load_state_dict(sd)
    assert snap.changed() == []
    hit = sv.poison_reaches_the_step(c)
    print(f"[{sv.case_id(c)}] finite decisions per stream: {finite.tolist()} (poison reaches the step: {hit})")
    for b in range(nB):
        if sv.sliding(c):
            assert finite[b] >= 2, (b, finite)
        elif not ref.poisoned(sv.slot_of(c, b)):
            assert finite[b] >= 1, (b, finite)


# ---- the whole-window surfaces --------------------------------------------------------------------------------------------------------
def test_whole_window_surfaces_feed_the_model_the_reference_windows(nsd, dev, ref_state):
    rs = np.random.RandomState(77)
    xn = sv.signal(sv.B, rs)
    W = sv.matrices(1, rs)[0]
    x = to_dev(xn, dev)
    plain = _eval_model(nsd, dev, ref_state)
    for gate in (0, 1):
        for prep in (0, 1):
            for align in (0, 1):
                tag = "whole windows " + ("G" * gate + "P" * prep + "L" * align or "none")
                G = nsd.SignalGate(**sv.GATE) if gate else None
                P = nsd.CausalPrep.design(**sv.PREP) if prep else None
                kw = dict(gate=G, prep=P, align=nsd.SessionAlign(**sv.ALIGN) if align else None)
                if align:
                    kw["align_matrix"] = to_dev(W, dev)
                cfg = sv.ref_settings(G, P)
                want = sv.window_ref_windows(xn, gate=cfg["gate"], prep=cfg["prep"], align=W if align else None)
                assert np.isfinite(want).all()
                wd = to_dev(want, dev)
                m = _eval_model(nsd, dev, ref_state, **kw)
                snap = snapshot(x)
                with torch.no_grad():
                    _same_words(None, tag, "model(x) in eval mode", m(x), plain(wd))
                _same_words(None, tag, "predict_proba", m.predict_proba(x), plain.predict_proba(wd))
                (ta, wa), (tb, wb) = m.predict_trials(x, window=sv.WINDOW, hop=sv.HOP), plain.predict_trials(wd, window=sv.WINDOW, hop=sv.HOP)
                _same_words(None, tag, "predict_trials: trials", ta, tb)
                _same_words(None, tag, "predict_trials: windows", wa, wb)
                assert bool(torch.isfinite(ta).all()) and tuple(wa.shape) == (sv.B, (sv.T - sv.WINDOW) // sv.HOP + 1, sv.K)
                # a streamed model is fed exactly what predict feeds it: the reference's claim (tests/test_serve_pipeline_cpu.py), on the device
                dec = nsd.StreamDecoder(m, streams=sv.S)
                t = 0
                for n in sv.CUTS["7-1-32-30"]:
                    out = dec._front(x[:, t:t + n].contiguous(), None)
                    _same_words(None, tag, f"streamed front end, samples {t} .. {t + n}", out, want[:, t:t + n])
                    t += n
                assert snap.changed() == [], tag


@pytest.mark.parametrize("rate", ["1/2", "5/8"])
def test_whole_window_surfaces_convert_the_rate_first(nsd, dev, ref_state, rate):
    """the same surfaces behind a rate conversion, against the plain model on window_ref_windows(resample=): the reference's conversion
    of the trials, not ops.resample_trials', so a wrong stage 0 cannot cancel"""
    c = next(c for c in sv.CASES if c.rate == rate and c.id != sv.DESIGN_ID)
    r = sv.converter(c)
    R = nsd.Resample(L=r["L"], M=r["M"], P=r["taps"].shape[1], taps=r["taps"])
    rs = np.random.RandomState(78)
    xn = sv.signal_in(sv.B, rs, rate)
    W = sv.matrices(1, rs)[0]
    x = to_dev(xn, dev)
    plain = _eval_model(nsd, dev, ref_state)
    for gate, prep, align in ((0, 0, 0), (1, 1, 1), (0, 1, 0), (1, 0, 1)):
        tag = f"whole windows at {rate} " + ("G" * gate + "P" * prep + "L" * align or "none")
        G = nsd.SignalGate(**sv.GATE) if gate else None
        P = nsd.CausalPrep.design(**sv.PREP) if prep else None
        kw = dict(gate=G, prep=P, align=nsd.SessionAlign(**sv.ALIGN) if align else None, resample=R)
        if align:
            kw["align_matrix"] = to_dev(W, dev)
        cfg = sv.ref_settings(G, P)
        want = sv.window_ref_windows(xn, gate=cfg["gate"], prep=cfg["prep"], align=W if align else None, resample=r)
        assert np.isfinite(want).all() and want.shape == (sv.B, sv.T, sv.C)
        wd = to_dev(want, dev)
        m = _eval_model(nsd, dev, ref_state, **kw)
        snap = snapshot(x)
        with torch.no_grad():
            _same_words(None, tag, "model(x) in eval mode", m(x), plain(wd))
        _same_words(None, tag, "predict_proba", m.predict_proba(x), plain.predict_proba(wd))
        (ta, wa), (tb, wb) = m.predict_trials(x, window=sv.WINDOW, hop=sv.HOP), plain.predict_trials(wd, window=sv.WINDOW, hop=sv.HOP)
        _same_words(None, tag, "predict_trials: trials", ta, tb)
        _same_words(None, tag, "predict_trials: windows", wa, wb)
        assert bool(torch.isfinite(ta).all()) and tuple(wa.shape) == (sv.B, (sv.T - sv.WINDOW) // sv.HOP + 1, sv.K)
        # streamed through push, the model is fed the same windows
        dec = nsd.StreamDecoder(m, streams=sv.S)
        t, outs = 0, []
        for n in sv.CUTS_IN[rate]["7-1-32-30"]:
            out = _fed(dec, c._replace(decoder="stream"), x[:, t:t + n].contiguous(), None, sv.B)
            if out is not None:
                outs.append(out.clone())
            t += n
        _same_words(None, tag, "streamed front end", torch.cat(outs, 1), want)
        assert snap.changed() == [], tag


def test_wall_time_of_this_file():
    """(the last test) -- the figures the docstring records"""
    print(f"tests/test_gpu_serve_pipeline.py: {len(sv.CASES)} rows, two layers each, {_SEEN['tensors']} tensor comparisons of "
          f"{_SEEN['words']} words ({_SEEN['nan words']} of them NaN in the reference, {_SEEN['nan payloads']} of those with another sign or "
          f"payload on the device), {time.perf_counter() - _T0:.1f} s since the file was imported")
