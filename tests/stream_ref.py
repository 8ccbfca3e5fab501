"""numpy reference of the resumable inference's attention pooling, shared by tests/test_stream_cpu.py and tests/test_gpu_stream.py.

The oracle pools a whole window: scores, their max, exp, the denominator, then the alpha-weighted sum.  A stream cannot: it has seen a
prefix.  `OnlinePool` restates what csrc/nsd_stream48.hip keeps per stream -- a running max m, a denominator and a weighted sum, updated
ONCE PER STEP, in fp32:
    s = attn.bias + top_t . attn.weight;  m' = max(m, s);  a = exp(m - m');  p = exp(s - m')
    den = den * a + p;  acc = acc * a + p * top_t;  m = m'
so that pooled(prefix t) = acc / den after any t, whatever chunks the steps arrived in.  tests/test_stream_cpu.py holds it to the
oracle's `pooled` on prefixes; the GPU tests compare the kernel's pool_acc / pool_den with the oracle directly.
"""
import numpy as np

from oracle import nsd_oracle as orc

CUTS_41 = ([1] * 41, [1, 2, 3, 5, 8, 13, 9], [40, 1], [41])


class OnlinePool:
    def __init__(self, attn_w, attn_b, H=48):
        self.w, self.b = np.asarray(attn_w, np.float32).reshape(-1), np.float32(np.asarray(attn_b).reshape(-1)[0])
        self.m, self.den, self.acc, self.steps = np.float32(-np.inf), np.float32(0), np.zeros(H, np.float32), 0

    def step(self, top_t):
        top_t = np.asarray(top_t, np.float32)
        s = np.float32(self.b + np.float32(np.dot(top_t, self.w)))
        m2 = np.float32(max(self.m, s))
        a, p = np.exp(np.float32(self.m - m2), dtype=np.float32), np.exp(np.float32(s - m2), dtype=np.float32)
        self.den = np.float32(self.den * a + p)
        self.acc = (self.acc * a + p * top_t).astype(np.float32)
        self.m, self.steps = m2, self.steps + 1

    @property
    def pooled(self):
        return (self.acc / self.den).astype(np.float32)


def top_sequence(flat, x, d, residual=False):
    """[B,T,H]: what the attention pooling reads -- the top layer's h, plus layer 0's with the residual extension (L = 2)"""
    fw = orc.forward(flat, x, d, residual=residual, saves=True)
    return fw["hseq"][1] + (fw["hseq"][0] if residual else 0.0), fw


def prefix_refs(flat, x, d, ts, residual=False):
    """{t: oracle forward (with saves) of x[:, :t]} for the prefix lengths ts"""
    return {int(t): orc.forward(flat, np.ascontiguousarray(x[:, :t]), d, residual=residual, saves=True) for t in sorted(set(ts))}


def cut_points(cut):
    return list(np.cumsum(cut))
