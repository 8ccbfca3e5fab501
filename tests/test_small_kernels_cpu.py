"""What tests/test_gpu_small_kernels.py rests on, pinned on the host (no GPU): the references and case tables of
tests/small_kernels_ref.py, the refusals of nsd_zscore_fwd (its checks precede any launch), the condition under which the reduction
and loss-sum cases are exact, and the kink margin of every dx_kernel row from the oracle alone.

  - zscore_ref (float64) against the fp32 oracle's z-score (1e-5: the oracle's own rounding; measured 1.4e-7) and exactly zero at T = 1
    and on constant channels; the case table reaches every loop edge it names at 64, 256 and 304 CUs.
  - the DC-offset bound: its value ((8 + 32) 2^-24 max|x| / deviation + 2e-5 = 2.635e-3 at 4 x 250 x 8, x = 1000 + N(0, 1)), and a
    restatement of zscore_kernel's summation order in numpy fp32 stays inside it (measured 1.43e-4: what the kernel itself gives).
  - the oracle's counter streams: a shorter stream is a prefix of a longer one (what dropout_ref / rrelu_ref slice), the mask at
    p = 1 - 2^-24 is finite with values 0 and 2^24 only, masks_dev_base, the sizes around the capped grid, the case whose stride
    crosses both segment boundaries.
  - reduction: the largest possible partial sum of every case is below 2^24 (8 x 1025 losses = 8200; 8 x (2 x 304 + 5 slabs + 1) = 4912 in the reduction), the slab counts of
    the table take every pair of (unrolled passes, remainder passes) of grad_reduce_kernel's two loops, the straddling and the odd
    layouts are what they claim (nsd_param_layout).
  - dx rows: generic path, nsd_dx_path, 4H * C * 4 == 65536 for the last, kink margin > KINK_MARGIN (measured >= 2.2).
"""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import nsd_oracle as orc
from tests import small_kernels_ref as sk
from tests.gpu_harness import KINK_MARGIN, head_inputs, kink_margin, oracle_step, spec_of

CUS = (64, 256, 304)             # the tables hold at any CU count; restated at three


def _lib():
    from nsd_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. z-score
# ---------------------------------------------------------------------------------------------------------------------------------
def test_zscore_table_reaches_the_loop_edges_it_names():
    cases = sk.ZSCORE_CASES
    assert len(cases) == len(set(cases)) == 12 and sk.ZSCORE_GRID_LOOP in cases
    for C_, edge in ((1, 256), (8, 32)):
        assert sk.zscore_rows(C_) == edge
        assert sorted(T for mb, T, c in cases if c == C_ and mb == (0, 3)) == [edge - 1, edge, edge + 1]
    assert any(T == 1 for _, T, _ in cases)
    idle = {c: sk.ZS_NT - sk.zscore_rows(c) * c for _, _, c in cases}
    assert idle[3] == 1 and idle[100] == 56 and idle[129] == 127 and idle[256] == 0 and idle[8] == 0
    assert all(sk.zscore_rows(c) == 1 for c in (129, 256)) and sk.zscore_rows(100) == 2
    assert any(T < sk.zscore_rows(c) for _, T, c in cases) and any(T > sk.zscore_rows(c) for _, T, c in cases)
    for cus in CUS:
        assert sk.n_trials(sk.ZSCORE_GRID_LOOP[0], cus) > 8 * cus                       # the grid of 8 * cus workgroups loops
        assert all(sk.n_trials(mb, cus) <= 8 * cus for mb, T, c in cases if (mb, T, c) != sk.ZSCORE_GRID_LOOP)


@pytest.mark.parametrize("mb,T,Cc", sk.ZSCORE_CASES)
def test_zscore_ref_against_the_fp32_oracle(mb, T, Cc):
    x = sk.zscore_input(sk.n_trials(mb, 2), T, Cc)
    ref = sk.zscore_ref(x)
    err = float(np.abs(orc.zscore(x) - ref).max())
    print(f"zscore_ref vs oracle B={x.shape[0]} T={T} C={Cc}: {err:.2e}")
    assert err < 1e-5
    if T == 1:
        assert not ref.any()
    else:
        assert abs(float((ref ** 2).mean(axis=1).max()) - 1.0) < 1e-4 and np.abs(ref.mean(axis=1)).max() < 1e-12


def test_zscore_ref_is_zero_on_constant_channels():
    x = sk.zscore_input(3, 33, 8)
    x[1, :, 2], x[2, :, 7] = 3.25, -1e-3
    ref = sk.zscore_ref(x)
    assert not ref[1, :, 2].any() and not ref[2, :, 7].any() and ref[0].all()


def _kernel_order_zscore(x):
    """zscore_kernel's arithmetic restated in numpy fp32, in its order: per-thread sequential sums over t = tid / C, += rows, the
    `rows` partials added sequentially, fmaf replaced by a float64 product rounded once"""
    B, T, Cc = x.shape
    rows, f32 = sk.zscore_rows(Cc), np.float32
    y = np.empty_like(x)
    for b in range(B):
        for c in range(Cc):
            col = x[b, :, c]
            m = f32(0)
            for r in range(rows):
                s = f32(0)
                for t in range(r, T, rows):
                    s = f32(s + col[t])
                m = f32(m + s)
            mu = f32(m / f32(T))
            vs = f32(0)
            for r in range(rows):
                v = f32(0)
                for t in range(r, T, rows):
                    d = f32(col[t] - mu)
                    v = f32(np.float64(d) * np.float64(d) + np.float64(v))
                vs = f32(vs + v)
            rs = f32(f32(1) / f32(np.sqrt(f32(vs / f32(T))) + f32(1e-6)))
            y[b, :, c] = (col - mu) * rs
    return y


def test_zscore_offset_bound_is_the_derived_one_and_holds_for_the_kernels_order():
    x = sk.zscore_offset_input()
    assert x.shape == (4, 250, 8) and abs(float(x.mean()) - 1000.0) < 0.1
    bound, mean_err, dev = sk.zscore_offset_bound(x)
    assert mean_err == (math.ceil(250 / 32) + 32) * 2.0 ** -24 * float(np.abs(x.astype(np.float64)).max())
    assert 0.85 < dev < 1.0 and 2.3e-3 < bound < 2.7e-3
    err = float(np.abs(_kernel_order_zscore(x) - sk.zscore_ref(x)).max())
    print(f"offset case: bound {bound:.3e} (mean error {mean_err:.3e} / deviation {dev:.3f} + {sk.ZSCORE_TOL}); "
          f"the kernel's order in numpy fp32: {err:.2e}")
    assert err <= bound


def test_zscore_refusals_precede_any_launch():
    """C = 257 and T = 0 return NSD_E_INVALID, B = 0 returns NSD_OK: on a machine without a GPU, so nothing was launched"""
    L = _lib().lib()
    buf = np.zeros(8 * 257, np.float32)
    p = buf.ctypes.data
    assert L.nsd_zscore_fwd(p, p, 2, 3, 257, None) == -1 and b"zscore" in L.nsd_last_error()
    assert L.nsd_zscore_fwd(p, p, 2, 0, 8, None) == -1
    assert L.nsd_zscore_fwd(p, p, 2, 3, 0, None) == -1
    assert L.nsd_zscore_fwd(p, p, 0, 3, 8, None) == 0
    assert L.nsd_zscore_fwd(p, p, 0, 0, 257, None) == 0                 # (the empty batch is accepted before the shape is looked at)
    assert not buf.any()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. counter streams
# ---------------------------------------------------------------------------------------------------------------------------------
def test_stream_tables():
    cap = sk.MASK_GRID_CAP
    assert cap == 1048576 and {1, 255, 256, 257, cap, cap + 1, 3072000} == set(sk.STREAM_SIZES)
    p = np.float32(sk.P_LARGEST)
    assert p < np.float32(1) and float(p) == sk.P_LARGEST == 1.0 - 2.0 ** -24 and np.float32(1) / (np.float32(1) - p) == 2.0 ** 24
    assert sk.STREAM_PS[0] == 0.0 and all(0.0 <= q < 1.0 for q in sk.STREAM_PS)
    assert [sk.masks_dev_base(s) for s in sk.MASKS_DEV_STEPS] == [4, 28, 12]
    assert sk.masks_dev_base(2 ** 30 - 1) == 2 ** 32 - 4
    assert sk.MASK_CASES[0] == (3072000, 8192) and sk.MASK_CASES[1] == (0, 96)
    n_lstm, n_head = sk.MASK_CASES[2]
    hits = [i for i in range(0, n_lstm + 2 * n_head, cap)]              # thread 0 of the capped grid
    assert len(hits) == 3 and hits[0] < n_lstm <= hits[1] < n_lstm + n_head <= hits[2]
    assert all(n_lstm + 2 * n_head > cap or (n_lstm, n_head) == (0, 96) for n_lstm, n_head in sk.MASK_CASES)


def test_oracle_streams_are_prefixes_and_the_largest_p_is_finite():
    seed, stream = sk.STREAM_SEEDS[1]
    for n in (1, 257, 5000):
        assert np.array_equal(orc.dropout_mask(seed, stream, 0.6, (n,)), sk.dropout_ref(seed, stream, 0.6, n))
        assert np.array_equal(orc.rrelu_noise(seed, stream, (n,)), sk.rrelu_ref(seed, stream, n))
    kept = 0
    for seed, stream in sk.STREAM_SEEDS:
        m = sk.dropout_ref(seed, stream, sk.P_LARGEST, max(sk.STREAM_SIZES))
        assert np.isfinite(m).all() and set(np.unique(m)) <= {0.0, 2.0 ** 24}
        kept += int((m != 0).sum())
        z = sk.dropout_ref(seed, stream, 0.0, 4096)
        assert np.array_equal(z, np.ones_like(z))                       # p = 0 keeps everything, unscaled
    print(f"p = 1 - 2^-24: {kept} of 3 x 3 072 000 values kept")
    seed, stream, at = sk.P_LARGEST_KEPT
    m = sk.dropout_ref(seed, stream, sk.P_LARGEST, max(sk.STREAM_SIZES))
    assert np.flatnonzero(m).tolist() == [at] and m[at] == 2.0 ** 24 and at > sk.MASK_GRID_CAP
    r = sk.rrelu_ref(0, 0, 100000)
    assert r.min() >= 0.125 and r.max() <= np.float32(1.0 / 3.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. reduction and loss sum
# ---------------------------------------------------------------------------------------------------------------------------------
def _layout(C_, H, L, K, F):
    offs = (C.c_int64 * (4 * L + 8))()
    assert _lib().lib().nsd_param_layout(C_, H, L, K, F, offs) == 0
    p_lstm, total = int(offs[4 * L]), int(_lib().lib().nsd_param_count(C_, H, L, K, F))
    assert p_lstm == orc.layout(orc.Dims(C_, H, L, K, F))["ln.weight"] and total == orc.param_count(orc.Dims(C_, H, L, K, F))
    return p_lstm, total


def test_exact_means_exact_every_partial_sum_stays_below_2_to_24():
    worst = 0
    for cus in CUS:
        for mb in sk.REDUCE_B:
            B = sk.n_trials(mb, cus)
            worst = max(worst, sk.largest_partial_sum(max(B, min(B, cus)) + 1))        # head slabs / LSTM slabs (+ an old gradient)
    worst = max(worst, sk.largest_partial_sum(max(sk.LOSS_B)), sk.largest_partial_sum(sk.MULTI_LOSS[1]),
                sk.largest_partial_sum(sk.REDUCE_STRADDLE["B"] + 1), sk.largest_partial_sum(sk.MULTI_B))
    print(f"largest possible partial sum of any exact case: {worst}")
    assert worst < 2 ** 24 and sk.INT_MAX == 8
    a = sk.int_pattern((1000, 7), 3)
    assert a.dtype == np.float32 and np.array_equal(a, np.round(a)) and a.min() == -8 and a.max() == 8


def test_reduce_table_takes_both_loops_of_the_kernel_through_every_edge():
    """at 256 CUs the slab count is B up to 129 and cus beyond: (unrolled passes, remainder passes) of slab group 0"""
    trips = {b: sk.reduce_loop_trips(b) for b in (1, 7, 8, 9, 56, 57, 63, 64, 65, 120, 121, 128, 129, 256)}
    assert trips[1] == (0, 1) and trips[8] == (0, 1) and trips[9] == (0, 2) and trips[56] == (0, 7)
    assert trips[57] == (1, 0) and trips[64] == (1, 0) and trips[65] == (1, 1) and trips[120] == (1, 7)
    assert trips[121] == (2, 0) and trips[128] == (2, 0) and trips[129] == (2, 1) and trips[256] == (4, 0)
    assert [b for _, b in sk.REDUCE_B[:13]] == [1, 7, 8, 9, 56, 57, 63, 64, 65, 120, 121, 128, 129]
    assert sk.REDUCE_B[13:] == [(1, 44), (2, 5)]


def test_reduce_ref_and_the_layouts_of_the_odd_cases():
    slabs, hslabs = sk.int_pattern((5, 12), 1), sk.int_pattern((3, 4), 2)
    ref = sk.reduce_ref(slabs, hslabs, 10)
    assert ref.shape == (14,) and ref[0] == slabs[:, 0].sum() and ref[9] == slabs[:, 9].sum() and ref[10] == hslabs[:, 0].sum()
    old = sk.int_pattern((14,), 3)
    assert np.array_equal(sk.reduce_ref(slabs, hslabs, 10, old), ref + old)
    s = sk.REDUCE_STRADDLE
    p_lstm, total = _layout(s["C"], s["H"], s["L"], s["K"], s["F"])
    assert p_lstm % sk.GR_COLS != 0 and total - p_lstm > sk.GR_COLS            # a workgroup of 32 columns holds both slab kinds
    o = sk.REDUCE_ODD_HEAD
    p_lstm, total = _layout(o["C"], o["H"], o["L"], o["K"], o["F"])
    assert total % sk.GR_COLS != 0
    p_lstm, total = _layout(8, 48, 2, 3, 32)
    assert p_lstm % sk.GR_COLS == 0                                             # the default model never straddles


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. dx_kernel rows, 5. att_close rows
# ---------------------------------------------------------------------------------------------------------------------------------
def test_dx_table():
    rows = sk.DX_ROWS
    assert [B * T for _, _, _, B, T in rows[:3]] == [255, 256, 257]
    assert {Cc % 8 for Cc, *_ in rows} >= {0, 1, 4, 5} and any(L == 1 for _, _, L, _, _ in rows)
    Cc, H, L, B, T = rows[-1]
    assert 4 * H * Cc * 4 == sk.DX_LDS_LIMIT and B < 16
    assert all(4 * H * Cc * 4 < sk.DX_LDS_LIMIT for Cc, H, *_ in rows[:-1])
    assert [T for _, T, _ in sk.ATT_CLOSE_ROWS] == [256, 257, 513] and all(f == 4 and B % 4 for B, _, f in sk.ATT_CLOSE_ROWS)


@pytest.mark.parametrize("Cc,H,L,B,T", sk.DX_ROWS)
def test_dx_rows_take_the_generic_path_and_keep_the_kink_margin(Cc, H, L, B, T):
    d, flat, x, y, masks = head_inputs(Cc, H, sk.DX_K, sk.DX_F, B, T, L=L, safe=True)
    dd = spec_of(d).dims(B, T)
    L_ = _lib().lib()
    assert L_.nsd_fast_path(C.byref(dd)) == 0 and L_.nsd_dx_path(C.byref(dd)) == 1
    ref = oracle_step(d, flat, x, labels=y, masks=masks, want_dx=True, kink=KINK_MARGIN)
    print(f"dx row C={Cc} H={H} L={L} B={B} T={T}: kink margin {kink_margin(ref['fw']):.2f}  largest |dx| {np.abs(ref['dx']).max():.2e}")
    assert np.isfinite(ref["dx"]).all() and np.abs(ref["dx"]).max() > 0 and ref["dx"].shape == (B, T, Cc)
    assert all(np.abs(ref["dx"][..., c]).max() > 0 for c in range(Cc))        # every channel carries a gradient to miss
