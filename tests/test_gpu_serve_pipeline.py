"""The serving front end -- gate -> prep -> gate-apply -> (second-moment accumulator) -> spatial apply -> the decoder's step -- held to ONE
composed reference (tests/serve_ref.py) on the MI355X, in each of the four decoders of nsd_amd/stream.py and on the whole-window
surfaces of EEG_LSTM.

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

Measured on one MI355X, the file against nothing but itself: 33 rows, 68 tests, 1.8 s from import to the last test (pytest: 3.7 s with
start-up); the slowest test 0.4 s (the first, which loads the kernels).  3854 tensor comparisons of 1 305 182 words; 26 561 of them
are NaN in the reference, 795 of those with the other sign on the device, all in layer A of the five by-position rows (09 16 24 26 27).

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
"""
import time

import numpy as np
import pytest
import torch

from tests import align_ref as ar
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


def _same_words(c, tag, what, got, want):
    """every word of got equals the word of want, NaNs included.  c: the row (None: no row).  In the rows where a NaN is computed from
    a NaN input (serve_ref.nan_by_position: prep on, gate off, a NaN sample) the project's rule for such a NaN holds -- finite values
    bitwise, NaNs by position (prep_ref.same_bits) -- and the words that differ in sign or payload are counted and printed."""
    (g, gn), (w, wn) = _words(got), _words(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (tag, what, g.shape, w.shape, g.dtype, w.dtype)
    differ = g != w
    payload = differ & gn & wn
    bad = np.argwhere(differ & ~payload if c is not None and sv.nan_by_position(c) else differ)
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
        Wr, rr = ar.whiten_ref(ref.sums[s:s + 1], ref.counts[s:s + 1], **sv.ALIGN)
        err, bound = float(np.abs(W[i].astype(np.float64) - Wr[0]).max()), FIT_BOUND * float(np.abs(Wr[0]).max())
        print(f"[{tag}] refit of slot {s}: steps {recs[i]['steps']} (reference {int(ref.counts[s, 0])}), status {recs[i]['status']}, "
              f"|W - whiten_ref| {err:.3e} (bound {bound:.3e})")
        assert recs[i]["steps"] == int(ref.counts[s, 0]) == rr[0]["steps"] and recs[i]["skipped"] == int(ref.counts[s, 1])
        assert recs[i]["status"] == 0 == rr[0]["status"] and err <= bound
        assert np.array_equal(W1[s], W[i]) and r1[s] == recs[i] and not np.array_equal(W[i], W0[s])
    for s in range(sv.S):
        if s not in slots:
            _same_words(c, tag, f"matrix of slot {s} behind a refit of {slots}", W1[s], W0[s])
            assert r1[s] == r0[s], (tag, s)
    ref.refit(slots, W)


def _checkpoint(tag, c, dec, make):
    """state_dict() into a fresh decoder: it returns the same alignment, records included, and a checkpoint from before the records
    travelled loads with zero records"""
    sd = dec.state_dict()
    fresh = make()
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
        dec, _ = _checkpoint(tag, c, dec, make)
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
        _same_words(c, tag, "accumulator counts", cov[:, n:].view(np.int64), ref.counts)
        _same_words(c, tag, "matrix table", dec.align_table, ref.table)
        assert bool(ref.counts.any()) == sv.accumulates(c)


@pytest.mark.parametrize("c", sv.CASES, ids=IDS)
def test_the_front_end_equals_the_composed_reference(nsd, dev, ref_state, c):
    inp = sv.inputs(c)
    make, _ = _factories(nsd, dev, ref_state, c, inp)
    dec, ref = make(), sv.new_ref(c, inp)
    nB, slots = sv.pushed(c)
    arg = _slots_arg(c, dev)
    x = to_dev(inp["x"], dev)
    at, t = sv.event_chunk(c), 0
    acted = {}
    for k, n in enumerate(sv.CUTS[c.cut]):
        tag = f"{sv.case_id(c)} chunk {k}"
        chunk = x[:, t:t + n].contiguous()
        snap = snapshot(chunk)
        out = dec._front(chunk, dec._slots(arg, nB))
        torch.cuda.synchronize()
        want, mask, _ = ref.push(inp["x"][:, t:t + n], slots)
        for s, did in ref.trace.items():
            acted[s] = acted.get(s, False) or did
        _same_words(c, tag, "the chunk the step is fed", out, want)
        _front_state_equals(tag, c, dec, ref, chunk.shape, mask)
        assert snap.changed() == [], tag
        assert (out is chunk) == (not (c.gate or c.prep or c.align))
        t += n
        if k == at:
            dec, ref, _, _ = _event(tag, c, dec, ref, inp, make)
            _front_state_equals(tag + " behind the event", c, dec, ref)
    print(f"[{sv.case_id(c)}] stages that acted: {[s for s in sv.STAGES if acted.get(s)]}")
    assert [s for s in sv.STAGES if acted.get(s)] == sv.expected_stages(c)


# ---- layer B ------------------------------------------------------------------------------------------------------------------------
class _Replayed:
    """dec._step(dec._front(x_static, slots), slots, True) captured once on a side stream and replayed per chunk"""

    def __init__(self, dev, nB, n, throw_away, slots_t):
        self.dev, self.slots_t = dev, slots_t
        self.x = torch.zeros((nB, n, sv.C), device=dev)
        self.side = torch.cuda.Stream(device=dev)
        throw_away._step(throw_away._front(self.x, slots_t), slots_t, True)        # the warm-up: nothing is loaded inside a capture
        torch.cuda.synchronize(dev)

    def capture(self, dec):
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=self.side):
            self.out = dec._step(dec._front(self.x, self.slots_t), self.slots_t, True)
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


@pytest.mark.parametrize("c", sv.CASES, ids=IDS)
def test_the_decoder_equals_a_plain_decoder_on_the_reference_chunks(nsd, dev, ref_state, c):
    inp = sv.inputs(c)
    make, plain_makers = _factories(nsd, dev, ref_state, c, inp)
    dec, plains, ref = make(), tuple(mk() for mk in plain_makers), sv.new_ref(c, inp)
    nB, slots = sv.pushed(c)
    arg = _slots_arg(c, dev)
    x = to_dev(inp["x"], dev)
    cut = sv.CUTS[c.cut]
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
        tag = f"{sv.case_id(c)} chunk {k}"
        chunk = x[:, t:t + n]
        got = _decisions(dec, replay(chunk) if replay is not None else dec.push(chunk, arg))
        want, _, wins = ref.push(inp["x"][:, t:t + n], slots)
        wd = to_dev(want, dev)
        theirs = _decisions(plains[0], plains[0].push(wd, arg))
        assert set(got) == set(theirs) and ("member_probs" in got) == sv.ensemble(c) and ("ends" in got) == sv.sliding(c)
        for name in theirs:
            _same_words(c, tag, name, got[name], theirs[name])
        for d in others:
            eager = _decisions(d, d.push(chunk, arg))
            for name in theirs:
                _same_words(c, tag, f"{name} of the eager decoder beside the replayed one", eager[name], theirs[name])
        for m, single in enumerate(plains[1:]):           # an ensemble: member m is bit for bit a single decoder of model m
            alone = _decisions(single, single.push(wd, arg))
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
            for b in range(nB):
                assert int(counts[b]) == len(wins[b]) and [int(e) for e in ends[b, :counts[b]]] == [e for e, _, _ in wins[b]], (tag, b)
                assert [r for _, r, _ in wins[b]] == list(range(len(wins[b]))) and (ends[b, counts[b]:] == -1).all(), (tag, b)
                for e, r, poisoned in wins[b]:
                    assert np.isnan(probs[b, r]).all() if poisoned else np.isfinite(probs[b, r]).all(), (tag, b, e, poisoned)
                    finite[b] += not poisoned
                assert np.isnan(probs[b, counts[b]:]).all(), (tag, b)
        else:
            for b in range(nB):
                poisoned = ref.poisoned(sv.slot_of(c, b))
                assert np.isnan(probs[b]).all() if poisoned else np.isfinite(probs[b]).all(), (tag, b, poisoned)
                finite[b] = not poisoned                  # (of the last chunk)
        t += n
        if k == at:
            dec, ref, plains, others = _event(tag, c, dec, ref, inp, make, plains, plain_makers, others)
            if replay is not None and c.event == "state_dict":         # a fresh decoder: a capture of its own, then the checkpoint again
                sd = dec.state_dict()
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


def test_wall_time_of_this_file():
    """(the last test) -- the figures the docstring records"""
    print(f"tests/test_gpu_serve_pipeline.py: {len(sv.CASES)} rows, two layers each, {_SEEN['tensors']} tensor comparisons of "
          f"{_SEEN['words']} words ({_SEEN['nan words']} of them NaN in the reference, {_SEEN['nan payloads']} of those with another sign or "
          f"payload on the device), {time.perf_counter() - _T0:.1f} s since the file was imported")
