"""Pure-integer schedule of the sliding-window decoder (nsd_window_* of include/nsd.h), shared by tests/test_window_cpu.py and
tests/test_gpu_window.py.

window = W, hop = Hp, R = W // Hp.  A stream's samples are numbered from its reset.  Window k covers [k Hp, k Hp + W) and ends at
e_k = k Hp + W; phase r = k mod R decodes the windows k = r (mod R), back to back from sample r Hp on.  A call of T samples on a stream
that has seen n0 completes the windows with n0 < e_k <= n0 + T, in ascending e_k, in rows 0, 1, ... of its D = ceil(T / Hp) rows.
"""


def rows(T, Hp):
    """D: the decisions a call of T samples can complete per stream"""
    return -(-T // Hp)


def completed(n0, T, W, Hp):
    """[(k, end, row)] of the windows a call of T samples completes on a stream that has seen n0 samples, in row order.
    The ends are the multiples of Hp from W on: closed form, no enumeration of windows."""
    R = W // Hp
    first, last = max(n0 // Hp + 1, R), (n0 + T) // Hp
    return [(j - R, j * Hp, j - first) for j in range(first, last + 1)]


def phases(n, W, Hp):
    """[(start, p)] per phase after n samples: its current window began at sample `start` and has consumed p in [0, W) samples;
    start is None while the phase idles (n <= r Hp: nothing consumed yet, p = 0)."""
    out = []
    for r in range(W // Hp):
        s0 = r * Hp
        if n <= s0:
            out.append((None, 0))
        else:
            p = (n - s0) % W
            out.append((n - p, p))
    return out
