"""numpy restatement of the signal-quality gate (nsd_gate_* of include/nsd.h), sample by sample in np.float32 on the state a slot
holds -- the ring included: vectorised over (stream, channel), looped over time.  The GPU tests compare bits with it; the CPU tests hold
it to hand-worked cases and to SignalGate.reference, which is written the other way round (whole windows, no ring)."""
import numpy as np

F = np.float32
SPAN = 64                        # NSD_GATE_MAX_SPAN: rows of the ring
OFF = dict(rail=0.0, jump=0.0, flat_eps=0.0, flat_samples=0, pp=0.0, pp_samples=0, hold_samples=0, max_bad=32, zero=True)


def config(**kw):
    """the fields of nsd_gate, everything off unless named"""
    assert set(kw) <= set(OFF), kw
    return dict(OFF, **kw)


def layout(C):
    """Offsets inside a slot in 4-byte words, as nsd_gate_state_layout reports them."""
    bad = ((4 + SPAN) * C + 1) & ~1
    steps = bad + 2 * C + 2
    return dict(prev=0, held=C, run=2 * C, hang=3 * C, ring=4 * C, bad=bad, rejected=bad + 2 * C, steps=steps, stride=(steps + 2 + 3) & ~3)


class State:
    """The state of B streams: what a slot holds."""

    def __init__(self, B, C):
        self.prev, self.held = np.zeros((B, C), F), np.zeros((B, C), F)
        self.run, self.hang = np.zeros((B, C), np.int32), np.zeros((B, C), np.int32)
        self.ring = np.zeros((B, SPAN, C), F)
        self.bad = np.zeros((B, C), np.int64)
        self.rejected, self.n = np.zeros(B, np.int64), np.zeros(B, np.int64)

    def slot_rows(self):
        """[B, stride] uint32: the bytes of the slots"""
        B, C = self.prev.shape
        lay = layout(C)
        out = np.zeros((B, lay["stride"]), np.uint32)
        out[:, :C] = self.prev.view(np.uint32)
        out[:, lay["held"]:lay["held"] + C] = self.held.view(np.uint32)
        out[:, lay["run"]:lay["run"] + C] = self.run.view(np.uint32)
        out[:, lay["hang"]:lay["hang"] + C] = self.hang.view(np.uint32)
        out[:, lay["ring"]:lay["ring"] + SPAN * C] = self.ring.reshape(B, -1).view(np.uint32)
        out[:, lay["bad"]:lay["bad"] + 2 * C] = self.bad.astype("<i8").view(np.uint32).reshape(B, 2 * C)
        out[:, lay["rejected"]:lay["rejected"] + 2] = self.rejected.astype("<i8").view(np.uint32).reshape(B, 2)
        out[:, lay["steps"]:lay["steps"] + 2] = self.n.astype("<i8").view(np.uint32).reshape(B, 2)
        return out

    def quality(self):
        """what StreamDecoder.quality reports: bad_fraction [B,C], rejected_fraction [B], steps [B]"""
        n = np.maximum(self.n, 1).astype(np.float64)
        return dict(bad_fraction=self.bad / n[:, None], rejected_fraction=self.rejected / n, steps=self.n.copy())


def popcount(mask):
    mask = np.asarray(mask).astype(np.uint32)
    return sum(((mask >> np.uint32(c)) & 1).astype(np.int64) for c in range(32))


def gate_ref(x, cfg, state=None):
    """x [B,T,C] float32 -> (y [B,T,C] float32, mask [B,T] uint32).  state: a State that is advanced (stream mode), or None (window
    mode: from reset)."""
    x = np.asarray(x, F)
    B, T, C = x.shape
    st = State(B, C) if state is None else state
    rows = np.arange(B)
    y, mask = np.empty_like(x), np.zeros((B, T), np.uint32)
    rail, jump, eps, pp = F(cfg["rail"]), F(cfg["jump"]), F(cfg["flat_eps"]), F(cfg["pp"])
    fs, ps, hold = int(cfg["flat_samples"]), int(cfg["pp_samples"]), int(cfg["hold_samples"])
    with np.errstate(all="ignore"):
        for t in range(T):
            v = x[:, t, :]
            some = (st.n > 0)[:, None]                       # there is a previous sample
            fin = np.isfinite(v)
            pair = some & fin & np.isfinite(st.prev)
            d = np.abs(v - st.prev)
            assert d.dtype == F
            raw = ~fin
            if rail > 0:
                raw = raw | (np.abs(v) >= rail)
            if jump > 0:
                raw = raw | (pair & (d >= jump))
            st.ring[rows, st.n % SPAN] = v
            if ps > 0:
                hi, lo = np.full((B, C), -np.inf, F), np.full((B, C), np.inf, F)
                for k in range(ps):
                    m = st.n - k                              # the sample k steps back, where the stream has one
                    w = st.ring[rows, m % SPAN]
                    use = (m >= 0)[:, None] & np.isfinite(w)
                    hi, lo = np.where(use, np.maximum(hi, w), hi), np.where(use, np.minimum(lo, w), lo)
                diff = hi - lo
                assert diff.dtype == F
                raw = raw | ((hi >= lo) & (diff >= pp))
            if fs > 0:
                flat = pair & (d <= eps)
                st.run = np.where(flat, np.minimum(st.run + 1, fs), 0).astype(np.int32)
                raw = raw | (st.run >= fs - 1)
            else:
                st.run = np.zeros_like(st.run)
            bad = raw | (st.hang > 0)
            st.hang = np.where(raw, hold, np.maximum(st.hang - 1, 0)).astype(np.int32)
            st.held = np.where(bad, st.held, v)
            y[:, t, :] = np.where(bad, st.held, v)
            word = np.zeros(B, np.uint32)
            for c in range(C):
                word |= bad[:, c].astype(np.uint32) << np.uint32(c)
            mask[:, t] = word
            st.prev = v.copy()
            st.bad += bad
            st.rejected += popcount(word) > int(cfg["max_bad"])
            st.n = st.n + 1
    return y, mask


def apply_ref(v, mask, cfg):
    """the apply stage: v [B,T,C], mask [B,T] -> out [B,T,C]"""
    v = np.asarray(v, F)
    out = v.copy()
    C = v.shape[-1]
    for c in range(C):
        if cfg["zero"]:
            out[..., c][((np.asarray(mask).astype(np.uint32) >> np.uint32(c)) & 1).astype(bool)] = F(0.0)
    out[popcount(mask) > int(cfg["max_bad"])] = np.nan
    return out


def same_bits(got, want):
    """Finite values bitwise, NaNs by position (the quiet-NaN pattern differs between the host and the GPU)."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]))


def _spike(T, at, value):
    x = np.zeros(T, F)
    x[at] = value
    return x


_B100, _B60 = np.nextafter(F(100.0), F(0.0)), np.nextafter(F(60.0), F(0.0))
# hand-worked cases on one channel: (the fields that are on, the samples, bit 0 of the mask of every sample)
HAND_CASES = [
    # |x| == rail fires, the float just below it does not
    (dict(rail=100.0), [100.0, _B100, -100.0, -_B100, 99.0], [1, 0, 1, 0, 0]),
    # |x - prev| == jump fires, the float just below it does not, and n == 0 has no previous sample
    (dict(jump=60.0), [500.0, 0.0, _B60, 0.0, 60.0, 0.0], [0, 1, 0, 0, 1, 1]),
    # flat_samples = 4: a run of exactly 3 equal samples passes; of 4, the fourth is bad, and every further one
    (dict(flat_samples=4), [1, 2, 5, 5, 5, 7, 8, 8, 8, 8, 8, 9, 9], [0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0]),
    # ... within flat_eps
    (dict(flat_samples=3, flat_eps=0.5), [0.0, 0.5, 1.0, 1.75, 2.0, 2.0], [0, 0, 1, 0, 0, 1]),
    # pp_samples = 5: an extreme sample is seen while it is at most 4 steps old
    (dict(pp=50.0, pp_samples=5), _spike(20, 10, 60.0), [0] * 10 + [1] * 5 + [0] * 5),
    # hi - lo == pp fires
    (dict(pp=50.0, pp_samples=2), [0.0, 50.0, 50.0, 1.0, -49.0, -49.0], [0, 1, 0, 0, 1, 0]),
    # the longest span, across two tiles of the kernel
    (dict(pp=50.0, pp_samples=64), _spike(140, 3, 60.0), [0] * 3 + [1] * 64 + [0] * 73),
    # non-finite samples are bad and are left out of the peak-to-peak span
    (dict(pp=50.0, pp_samples=4), [0.0, np.inf, 10.0, np.nan, 70.0, 0.0], [0, 1, 0, 1, 1, 1]),
    # the hang-over: hold_samples further samples; a raw-bad sample inside it starts it again
    (dict(rail=100.0, hold_samples=3), _spike(12, 4, 200.0), [0] * 4 + [1] * 4 + [0] * 4),
    (dict(rail=100.0, hold_samples=2), [0, 200, 0, 200, 0, 0, 0], [0, 1, 1, 1, 1, 1, 0]),
]
