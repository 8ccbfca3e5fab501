"""References and case tables of tests/test_gpu_small_kernels.py (the kernels of csrc/nsd_misc.hip), importable without a GPU:
tests/test_small_kernels_cpu.py pins them on the host.  Nothing here launches anything.

A batch written (m, a) stands for m * cus + a trials, cus = the device's CU count (the GPU file takes it from the fixture; the CPU
file restates the tables at several counts)."""
import functools
import math

import numpy as np

from oracle import nsd_oracle as orc
from tests.golden.make_goldens import synth_x

ZS_NT = 256                      # threads of zscore_kernel, rows of a dx_kernel workgroup, steps of an att_close_kernel chunk
MASK_GRID_CAP = 4096 * 256       # threads of the counter-stream kernels' capped grid: a grid-stride loop from one element more
GR_COLS, GR_GROUPS, GR_UNROLL = 32, 8, 8           # grad_reduce_kernel: columns per workgroup, slab groups, loads in flight per group


def n_trials(mb, cus):
    return mb[0] * cus + mb[1]


def align4(n):
    return (n + 3) // 4 * 4


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. z-score
# ---------------------------------------------------------------------------------------------------------------------------------
ZSCORE_TOL = 2e-5                # test_gpu_parity.py::test_zscore's own bound, absolute, on synth_x-like input
ZSCORE_EPS = 1e-6


def zscore_rows(C):
    """time steps zscore_kernel covers per sweep: 256 // C (the other 256 % C threads idle)"""
    return ZS_NT // C


# ((m, a): B = m * cus + a, T, C): T around rows at C = 1 (rows = 256) and C = 8 (rows = 32); one step; fewer steps than rows with
# idle threads (C = 3: 85 rows, 255 threads); C > 128: one row per sweep and up to 127 idle threads whose tid % C is still read;
# C = 256: the widest accepted; and more trials than the grid of 8 * cus workgroups
ZSCORE_CASES = ([((0, 3), T, 1) for T in (255, 256, 257)] + [((0, 3), T, 8) for T in (31, 32, 33)]
                + [((0, 2), 1, 8), ((0, 2), 2, 3), ((0, 3), 7, 100), ((0, 2), 5, 129), ((0, 2), 3, 256), ((8, 3), 5, 8)])
ZSCORE_GRID_LOOP = ((8, 3), 5, 8)                  # the case run in place too
ZSCORE_OFFSET_SHAPE, ZSCORE_OFFSET = (4, 250, 8), 1000.0


def zscore_ref(x):
    """(x - mean_T) / (sqrt(mean_T d^2) + 1e-6) in float64 on the fp32 input; exactly 0 where a channel of a trial is constant"""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    d = x64 - x64.mean(axis=1, keepdims=True)
    return d / (np.sqrt((d * d).mean(axis=1, keepdims=True)) + ZSCORE_EPS)


def zscore_input(B, T, C):
    return synth_x(B, T, C=C, seed=1000 * C + T)


def zscore_offset_input():
    B, T, C = ZSCORE_OFFSET_SHAPE
    return (ZSCORE_OFFSET + np.random.RandomState(250).standard_normal((B, T, C))).astype(np.float32)


def zscore_offset_bound(x):
    """The bound of the DC-offset case, derived and not tuned.  A sequential fp32 sum of n terms is within (n - 1) 2^-24 sum|x| of
    the exact one.  A thread of zscore_kernel adds ceil(T / rows) samples of its channel, thread tid < C then the `rows` partials:
    |mean error| <= (ceil(T / rows) + rows) 2^-24 max|x|.  y = (x - mean) / (std + eps): the output moves by the mean's error over the
    deviation (the smallest float64 deviation of any trial and channel), on top of ZSCORE_TOL of the centred case.  (The wrong mean
    adds its square to the variance: 1e-6 of it here.)  -> (bound, mean-error term, smallest deviation)"""
    _, T, C = x.shape
    rows = zscore_rows(C)
    x64 = x.astype(np.float64)
    dev = float(np.sqrt(((x64 - x64.mean(axis=1, keepdims=True)) ** 2).mean(axis=1)).min())
    mean_err = (math.ceil(T / rows) + rows) * 2.0 ** -24 * float(np.abs(x64).max())
    return mean_err / dev + ZSCORE_TOL, mean_err, dev


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. counter streams
# ---------------------------------------------------------------------------------------------------------------------------------
STREAM_SIZES = (1, 255, 256, 257, MASK_GRID_CAP, MASK_GRID_CAP + 1, 256 * 250 * 48)       # the last: cfg2's drop_lstm
STREAM_SEEDS = ((0, 0), (12345678901234, 3), (2 ** 63 + 5, 4000000000))                    # test_counter_streams_bit_exact's
P_LARGEST = float(np.nextafter(np.float32(1), np.float32(0)))                              # 1 - 2^-24: accepted (p < 1), keeps one value in 2^24
STREAM_PS = (0.0, 0.25, 0.6, P_LARGEST)
# None of the three seeds above keeps a value of its first 3 072 000 at the largest p; stream 6 of seed 7 keeps exactly one, in the
# grid-stride loop's second pass: (seed, stream, index), the one place where keep = 1 / (1 - p) = 2^24 is seen
P_LARGEST_KEPT = (7, 6, 1679464)
# nsd_train_masks (n_lstm, n_head): cfg2's LSTM mask with a head of 256 trials (the loop runs three times); an L = 1 model -- no layer
# has a successor, its drop_lstm holds (L - 1) * B * T * H = 0 elements; and one where thread 0 of the capped grid, stride
# MASK_GRID_CAP, writes index 0 of drop_lstm, MASK_GRID_CAP - n_lstm of rrelu and 2 * MASK_GRID_CAP - n_lstm - n_head of drop_head
MASK_CASES = ((256 * 250 * 48, 256 * 32), (0, 96), (MASK_GRID_CAP - 5, MASK_GRID_CAP - 3))
MASK_SEED, MASK_BASE, MASK_P = 99, 40, (0.6, 0.25)                                          # test_fused_train_masks_bit_exact's
MASKS_DEV_STEPS = (1, 7, 2 ** 30 + 3)


def masks_dev_base(step):
    """the host base stream that train_masks_kernel's (uint32)(step & 0x3FFFFFFF) * 4 stands for"""
    return ((step & 0x3FFFFFFF) * 4) & 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def _stream(kind, seed, stream, p):
    """the oracle's stream at the largest size any case asks for (value(seed, stream, i) does not depend on n); read-only"""
    n = max(max(STREAM_SIZES), max(max(c) for c in MASK_CASES))
    a = orc.rrelu_noise(seed, stream, (n,)) if kind == "rrelu" else orc.dropout_mask(seed, stream, p, (n,))
    a.setflags(write=False)
    return a


def dropout_ref(seed, stream, p, n):
    return _stream("drop", seed, stream & 0xFFFFFFFF, float(p))[:n]


def rrelu_ref(seed, stream, n):
    return _stream("rrelu", seed, stream & 0xFFFFFFFF, None)[:n]


def train_masks_ref(seed, base, p_lstm, p_head, n_lstm, n_head):
    """(drop_lstm, rrelu, drop_head) from the oracle's streams base, base + 1, base + 2"""
    return dropout_ref(seed, base, p_lstm, n_lstm), rrelu_ref(seed, base + 1, n_head), dropout_ref(seed, base + 2, p_head, n_head)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. reduction and loss sum
# ---------------------------------------------------------------------------------------------------------------------------------
INT_MAX = 8                      # slab, old-gradient and loss entries: integers in [-8, 8]
# head-slab counts B at T = 2 on the default model; the LSTM slab count follows the layout (B up to one trial per CU on the H = 48 path)
REDUCE_B = [(0, b) for b in (1, 7, 8, 9, 56, 57, 63, 64, 65, 120, 121, 128, 129)] + [(1, 44), (2, 5)]
REDUCE_T = 2
REDUCE_STRADDLE = dict(C=3, H=30, L=1, K=3, F=32, B=65)          # P_lstm % 32 != 0: one workgroup reads both slab kinds
REDUCE_ODD_HEAD = dict(C=8, H=48, L=2, K=5, F=7, B=9)            # P % 32 != 0: the last workgroup is partly idle
REDUCE_ACC_B, MULTI_M, MULTI_B = 65, 3, 9
LOSS_B = (1, 63, 64, 65, 255, 256, 257, 1025)
MULTI_LOSS = (3, 65)


def int_pattern(shape, seed):
    """integer-valued floats in [-8, 8]: every partial sum of fewer than 2^24 / 8 of them is an exact fp32 integer in any order"""
    return np.random.RandomState(seed).randint(-INT_MAX, INT_MAX + 1, size=shape).astype(np.float32)


def reduce_ref(slabs, hslabs, p_lstm, old=None):
    """what nsd_grad_reduce must give bit for bit: slabs [n, stride >= p_lstm] and hslabs [B, ph] of integers -> the float64 column
    sums (+ old where it accumulates), which must be fp32 integers"""
    s = np.concatenate([slabs[:, :p_lstm].astype(np.float64).sum(0), hslabs.astype(np.float64).sum(0)])
    if old is not None:
        s = s + old.astype(np.float64)
    assert np.abs(s).max() < 2 ** 24 and np.array_equal(s, np.round(s))
    return s.astype(np.float32)


def largest_partial_sum(n_terms):
    """the largest |partial sum| the exact cases can meet: every entry at +-8"""
    return INT_MAX * n_terms


def reduce_loop_trips(n):
    """(passes of the unrolled loop, passes of the remainder loop) of slab group 0 of grad_reduce_kernel over n slabs"""
    q = unrolled = 0
    while q + (GR_UNROLL - 1) * GR_GROUPS < n:
        q, unrolled = q + GR_UNROLL * GR_GROUPS, unrolled + 1
    return unrolled, len(range(q, n, GR_GROUPS))


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. dx_kernel beyond eight channels (the generic path), 5. att_close_kernel across a chunk
# ---------------------------------------------------------------------------------------------------------------------------------
DX_K, DX_F = 3, 32
# (C, H, L, B, T): one channel (rows = 255: the last thread of the only workgroup idles); a second channel pass of one channel at
# rows = 256; a second pass of four at L = 1 and rows = 257 (a second workgroup of one row); a second pass of five; eight full passes;
# and the largest weight matrix nsd_dx_ok admits, 4H * C * 4 == 65536 bytes of dynamic LDS
DX_ROWS = [(1, 40, 2, 3, 85), (9, 40, 2, 4, 64), (12, 40, 1, 1, 257), (13, 24, 2, 5, 9), (64, 40, 2, 3, 7), (64, 64, 2, 3, 5)]
DX_LDS_LIMIT = 64 * 1024
# (B, T, force) added to test_gpu_parity.py::test_input_gradient_after_the_fused_head_vs_oracle: one full chunk of 256 steps, a second
# chunk of one step, a third (d attn.weight and d attn.bias carried over two chunk changes); B % 4 != 0 keeps a padding trial
ATT_CLOSE_ROWS = [(5, 256, 4), (5, 257, 4), (6, 513, 4)]
