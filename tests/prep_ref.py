"""numpy restatement of the causal front end (nsd_prep_* of include/nsd.h), operation for operation in np.float32: vectorised over
(stream, channel), looped over time and sections.  The GPU tests compare bits with it."""
import numpy as np

F = np.float32
MAX_SECTIONS = 4


def layout(C):
    """Float offsets inside a slot, as nsd_prep_state_layout reports them."""
    steps = ((3 + 2 * MAX_SECTIONS) * C + 1) & ~1
    return dict(x0=0, z=C, mu=(1 + 2 * MAX_SECTIONS) * C, var=(2 + 2 * MAX_SECTIONS) * C, steps=steps, stride=(steps + 2 + 3) & ~3)


class State:
    """The state of B streams: what a slot holds, as arrays [B, C] (z: [B, MAX_SECTIONS, 2, C]) and the sample count n [B]."""

    def __init__(self, B, C):
        self.x0, self.mu, self.var = (np.zeros((B, C), F) for _ in range(3))
        self.z = np.zeros((B, MAX_SECTIONS, 2, C), F)
        self.n = np.zeros(B, np.int64)

    def slot_rows(self):
        """[B, stride] float32: the bytes of the slots (the int64 count viewed as two floats)."""
        B, C = self.x0.shape
        lay = layout(C)
        out = np.zeros((B, lay["stride"]), F)
        out[:, :C] = self.x0
        out[:, lay["z"]:lay["mu"]] = self.z.reshape(B, -1)
        out[:, lay["mu"]:lay["mu"] + C] = self.mu
        out[:, lay["var"]:lay["var"] + C] = self.var
        out[:, lay["steps"]:lay["steps"] + 2] = self.n.astype("<i8").view(F).reshape(B, 2)
        return out


def prep_ref(x, *, sections=(), alpha=0.0, var0=1.0, baseline=True, car=False, state=None):
    """x [B, T, C] float32 -> y [B, T, C] float32.  state: a State that is advanced (stream mode), or None (window mode: from reset)."""
    x = np.asarray(x, F)
    B, T, C = x.shape
    st = State(B, C) if state is None else state
    sos = np.asarray(sections, F).reshape(-1, 5)
    alpha, var0 = F(alpha), F(var0)
    oma = F(1.0) - alpha
    fC = F(C)
    y = np.empty_like(x)
    with np.errstate(all="ignore"):
        for t in range(T):
            v = x[:, t, :].copy()
            first = (st.n == 0)[:, None]
            if baseline:
                st.x0 = np.where(first, v, st.x0)
                v = v - st.x0
            if car:
                m = v[:, 0].copy()
                for c in range(1, C):
                    m = m + v[:, c]
                v = v - (m / fC)[:, None]
            for s in range(len(sos)):
                b0, b1, b2, a1, a2 = sos[s]
                out = b0 * v + st.z[:, s, 0]
                st.z[:, s, 0] = (b1 * v - a1 * out) + st.z[:, s, 1]
                st.z[:, s, 1] = b2 * v - a2 * out
                v = out
            if alpha > 0:
                d = v - st.mu
                ad = alpha * d
                mu = st.mu + ad
                var = oma * (st.var + ad * d)
                st.mu = np.where(first, v, mu)
                st.var = np.where(first, var0, var).astype(F)
                v = (v - st.mu) / (np.sqrt(st.var) + F(1e-6))
            assert v.dtype == F
            y[:, t, :] = v
            st.n = st.n + 1
    return y


def same_bits(got, want):
    """Finite values bitwise, NaNs by position (the quiet-NaN pattern differs between the host and the GPU)."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]))
