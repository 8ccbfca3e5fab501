"""np.float32 restatement of nsd_multi_stream_step's mean_probs (include/nsd.h), shared by tests/test_multi_stream_cpu.py and
tests/test_gpu_multi_stream.py:  mean[b,k] = (((p_0 + p_1) + p_2) + ... + p_{M-1}) / float32(M),  p_m = probs[m,b,k] -- a serial sum
in m, every addition rounded to fp32 on its own, then one correctly rounded fp32 division.  Nothing else lives here: the per-model
reference is the single-model call and tests/stream_ref.py.
"""
import numpy as np


def mean_probs(probs):
    """probs [M, ...] float32 -> [...] float32"""
    p = np.asarray(probs)
    assert p.dtype == np.float32 and p.ndim >= 1 and p.shape[0] >= 1
    s = p[0].copy()
    for m in range(1, p.shape[0]):
        s = (s + p[m]).astype(np.float32)
    return (s / np.float32(p.shape[0])).astype(np.float32)
