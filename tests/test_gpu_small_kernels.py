"""The small fp32 kernels of csrc/nsd_misc.hip -- zscore_kernel, the counter-stream kernels, grad_reduce_kernel, loss_sum_kernel,
dx_kernel -- each against a plain reference of its own operation at every edge of its loops.  (att_close_kernel's chunk boundary:
the rows ATT_CLOSE_ROWS in tests/test_gpu_parity.py::test_input_gradient_after_the_fused_head_vs_oracle.)  Needs a real MI355X: run
with `pytest -m gpu -s` (every comparison prints its error before it asserts, the last test of the file the worst per class).
References and case tables: tests/small_kernels_ref.py, pinned on the host by tests/test_small_kernels_cpu.py.  cus = the device's
CU count, from the fixture; (m, a) stands for m * cus + a trials.

  1. z-score against numpy float64 on the same fp32 input.  (B, T, C): (3, 255|256|257, 1) and (3, 31|32|33, 8) -- T on either side
     of the rows = 256 / C steps of a sweep --, (2, 1, 8), (2, 2, 3), (3, 7, 100), (2, 5, 129), (2, 3, 256) -- rows = 1, up to 127
     idle threads --, (8 cus + 3, 5, 8) -- the grid loops -- and that one in place.  2e-5 absolute (test_zscore's bound); exactly
     zero at T = 1 and on a constant channel (3.25 on the last channel of trial 1 of every case).
     x = 1000 + N(0, 1) at (4, 250, 8): a sequential fp32 sum of n terms is within (n - 1) 2^-24 sum|x|; a thread adds
     ceil(T / rows) = 8 samples, then one thread the rows = 32 partials, so |mean error| <= 40 x 2^-24 x max|x| = 2.39e-3; the
     output moves by that over the smallest deviation (0.915), plus 2e-5: bound 2.635e-3.
  2. counter streams bit for bit against the oracle: n in {1, 255, 256, 257, 2^20, 2^20 + 1, 3 072 000} (4096 workgroups of 256
     threads: a grid-stride loop from 2^20 + 1 on), the three (seed, stream) pairs of test_counter_streams_bit_exact, p in
     {0, 0.25, 0.6, 1 - 2^-24}; at the largest p one more stream that keeps a value (2^24) in the loop's second pass.
     nsd_train_masks at (n_lstm, n_head) = (3 072 000, 8192), (0, 96) -- an L = 1 model: through the ABI with a null drop_lstm, with
     an empty tensor, and as ops.train_masks(drop_lstm=None) -- and (2^20 - 5, 2^20 - 3), where thread 0's stride crosses both
     segment boundaries.  nsd_train_masks_dev at device counters 1, 7, 2^30 + 3 == nsd_train_masks at host bases 4, 28, 12.
  3. nsd_grad_reduce bit for bit against float64 column sums of integer-valued slabs (|.| <= 8: every partial sum is an exact fp32
     integer in any order, a slab left out or taken twice is an integer error): B in {1, 7, 8, 9, 56, 57, 63, 64, 65, 120, 121, 128,
     129, cus + 44, 2 cus + 5} head slabs at T = 2 on the default model (LSTM slabs: B up to cus; every count of passes of the
     unrolled and the remainder loop), (C, H, L) = (3, 30, 1) at B = 65 (P_lstm % 32 = 8: one workgroup sums both slab kinds),
     (K, F) = (5, 7) (P % 32 != 0), accumulate = 1 at B = 65, nsd_multi_grad_reduce at M = 3, B = 9.  The rest of the workspace is NaN.
     ops.loss_sum exact at B in {1, 63, 64, 65, 255, 256, 257, 1025}, ops.multi_loss_sum at M = 3, B = 65.
  4. dx_kernel beyond eight channels, on the generic path (fast_path == 0, dx_path, one slab): (C, H, L, B, T) = (1, 40, 2, 3, 85),
     (9, 40, 2, 4, 64), (12, 40, 1, 1, 257), (13, 24, 2, 5, 9), (64, 40, 2, 3, 7), (64, 64, 2, 3, 5) -- the last with
     4H * C * 4 == 65536 bytes of dynamic LDS, the most nsd_dx_ok admits.  train_step(want_dx=True) against
     oracle_step(want_dx=True, kink=KINK_MARGIN), head_inputs(safe=True), all masks on: dx within DX_TOL of its largest element,
     logits / loss / gradients through assert_step_vs_oracle with FP32_EXACT.

Measured on one MI355X (256 CUs):
  z-score          worst 4.05e-6 of 2e-5 (2 x 3 x 256: three samples per channel), every other case <= 9.5e-7; the entries that are
                   zero in float64 exactly 0; in place bit for bit the out-of-place result
  z-score, offset  1.43e-4 of the derived 2.635e-3 (the kernel's summation order restated in numpy fp32 gives the same 1.43e-4)
  streams, masks   every comparison bit for bit; p = 1 - 2^-24: the one kept value is 2^24, at index 1 679 464
  reduction, loss  every comparison bit for bit; LSTM slab counts = B up to 129, then 256, 256
  dx / largest     5.1e-7 of DX_TOL = 2e-5 (C = 13, H = 24); the 64 KB row launches and measures 5.0e-7
  dx rows          logits 1.2e-6, mean loss 3.2e-7, LSTM weight gradients 7.0e-7 / largest, other tensors 8.7e-7 / largest
  the three att_close rows of test_gpu_parity.py: dx 8.6e-7 / largest, LSTM weight gradients 5.4e-6, other tensors 1.3e-6
Kernels made to do less, each built once and run once against this file and the three att_close rows (never committed):
  grad_reduce remainder loop `q < n - 1`          14 reduction tests fail (every slab count with a remainder pass), and the whole steps
  zscore variance pass from `tid / C + rows`      every z-score test but T = 1
  att_close `n = T - t0 - 1` in a partial chunk   the rows T = 257 and 513 (T = 256 has no partial chunk)
  dx store `c0 + i < C - 1`                       all six dx rows
  train_masks stride doubled                      test_train_masks_bit_exact[cfg2] and [stride-crosses-both]
  zscore without its grid loop, dx with its first channel pass only, att_close with its first chunk only (one library):
                                                  the two grid-loop z-score tests, the five dx rows with C > 8, the rows T = 257 and 513
The suite as it stood before this file passes, all 1904 GPU tests, with the doubled mask stride and with the last library.
Wall time of the file on the MI355X: 3 s (60 tests), the CPU references included; the slowest test takes 0.2 s.
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from tests import small_kernels_ref as sk
from tests.gpu_harness import (DX_TOL, FP32_EXACT, KINK_MARGIN, LOGIT_TOL, LOSS_TOL, assert_step_vs_oracle, cus, dev, grad_errors, head_inputs,  # noqa: F401
                               nsd, oracle_step, spec_of, sync_at_the_end, to_dev, train_step)

pytestmark = pytest.mark.gpu

WORST = {}                       # class of number -> (worst value seen in this run, where): printed by the last test
T_START = time.time()
NAN = float("nan")


def _note(key, value, where):
    v = float(value)
    if v != v or v >= WORST.get(key, (0.0, ""))[0]:          # (a NaN is noted, and stays)
        WORST[key] = (v, where)


def _bits_equal(tag, got, ref):
    """bit for bit (np.array_equal: a NaN on either side fails it); prints the number of differing entries first"""
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    same = got.shape == ref.shape and np.array_equal(got, ref)
    n_bad = int((got != ref).sum()) if got.shape == ref.shape else -1
    print(f"[{tag}] n={ref.size}: {'bit for bit' if same else f'{n_bad} entries differ'}")
    _note("entries that differ where bits must match", max(n_bad, 0) if not same else 0, tag)
    return same


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. z-score
# ---------------------------------------------------------------------------------------------------------------------------------
def _zscore_case(mb, T, Cc, cus):
    """synth_x-like input with a constant channel (3.25 on the last channel of trial 1: every partial sum of it is exact)"""
    x = sk.zscore_input(sk.n_trials(mb, cus), T, Cc)
    if x.shape[0] > 1:
        x[1, :, Cc - 1] = 3.25
    return x


def _zscore_vs_float64(tag, got, x):
    ref = sk.zscore_ref(x)
    err = float(np.abs(got - ref).max())
    zero = (ref == 0.0)
    zerr = float(np.abs(got[zero]).max()) if zero.any() else 0.0
    print(f"[{tag}] B={x.shape[0]} T={x.shape[1]} C={x.shape[2]}: max error {err:.2e} (bound {sk.ZSCORE_TOL})  "
          f"{int(zero.sum())} entries exactly zero in float64: largest |kernel| {zerr:.1e}")
    _note("zscore (abs)", err, tag)
    _note("zscore where float64 is exactly zero (abs)", zerr, tag)
    assert np.isfinite(got).all(), tag
    assert err < sk.ZSCORE_TOL, (tag, err)
    assert zerr == 0.0, (tag, zerr)
    return zero


@pytest.mark.parametrize("mb,T,Cc", sk.ZSCORE_CASES, ids=[f"B{f'{m}cus+{a}' if m else a}-T{T}-C{c}" for (m, a), T, c in sk.ZSCORE_CASES])
def test_zscore_vs_float64(nsd, dev, cus, mb, T, Cc):
    from nsd_amd import ops
    x = _zscore_case(mb, T, Cc, cus)
    B = x.shape[0]
    assert ((mb, T, Cc) == sk.ZSCORE_GRID_LOOP) == (B > 8 * cus)
    out = torch.full((B, T, Cc), NAN, device=dev)
    got = ops.zscore(to_dev(x, dev), out=out).cpu().numpy()
    zero = _zscore_vs_float64(f"1 zscore {B} x {T} x {Cc}", got, x)
    assert zero.all() if T == 1 else (B > 1 and zero[1, :, Cc - 1].all() and int(zero.sum()) == T)


def test_zscore_in_place_where_the_grid_loops(nsd, dev, cus):
    from nsd_amd import ops
    mb, T, Cc = sk.ZSCORE_GRID_LOOP
    x = _zscore_case(mb, T, Cc, cus)
    xt = to_dev(x, dev)
    apart = ops.zscore(xt)
    assert ops.zscore(xt, out=xt) is xt
    _zscore_vs_float64("1 zscore in place", xt.cpu().numpy(), x)
    assert _bits_equal("1 zscore in place == out of place", xt, apart.cpu().numpy())


def test_zscore_with_a_dc_offset_much_larger_than_the_deviation(nsd, dev):
    from nsd_amd import ops
    x = sk.zscore_offset_input()
    bound, mean_err, deviation = sk.zscore_offset_bound(x)
    got = ops.zscore(to_dev(x, dev)).cpu().numpy()
    err = float(np.abs(got - sk.zscore_ref(x)).max())
    print(f"[1 zscore offset] x = {sk.ZSCORE_OFFSET} + N(0, 1) at {x.shape}: max error {err:.3e}  derived bound {bound:.3e} "
          f"(mean error {mean_err:.3e} / deviation {deviation:.3f} + {sk.ZSCORE_TOL})")
    _note("zscore, DC offset 1000 (abs)", err, f"bound {bound:.3e}")
    assert np.isfinite(got).all() and err <= bound, (err, bound)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. counter streams
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", sk.STREAM_PS, ids=["p0", "p0.25", "p0.6", "p1-2^-24"])
def test_dropout_stream_bit_exact_at_every_size(nsd, dev, p):
    from nsd_amd import ops
    pairs = sk.STREAM_SEEDS + ((sk.P_LARGEST_KEPT[:2],) if p == sk.P_LARGEST else ())
    for seed, stream in pairs:
        full = sk.dropout_ref(seed, stream, p, max(sk.STREAM_SIZES))
        assert np.isfinite(full).all()                     # the host oracle itself, before it serves as the reference
        for n in sk.STREAM_SIZES:
            got = ops.dropout_mask(seed, stream, p, (n,), dev)
            assert _bits_equal(f"2 dropout p={p:.8g} seed={seed} stream={stream}", got, full[:n]), (seed, stream, p, n)
    if p == sk.P_LARGEST:
        seed, stream, at = sk.P_LARGEST_KEPT
        got = ops.dropout_mask(seed, stream, p, (max(sk.STREAM_SIZES),), dev).cpu().numpy()
        print(f"[2 dropout p=1-2^-24] kept: index {np.flatnonzero(got).tolist()} value {got[at]}")
        assert np.flatnonzero(got).tolist() == [at] and got[at] == 2.0 ** 24


def test_rrelu_stream_bit_exact_at_every_size(nsd, dev):
    from nsd_amd import ops
    for seed, stream in sk.STREAM_SEEDS:
        for n in sk.STREAM_SIZES:
            got = ops.rrelu_noise(seed, stream, (n,), dev)
            assert _bits_equal(f"2 rrelu seed={seed} stream={stream}", got, sk.rrelu_ref(seed, stream, n)), (seed, stream, n)


def _masks_vs_oracle(tag, got, seed, base, p_lstm, p_head):
    a, b, c = got
    ref = sk.train_masks_ref(seed, base, p_lstm, p_head, a.numel(), b.numel())
    ok = [_bits_equal(f"{tag} {name} (stream base+{i})", t, r) for i, (name, t, r) in enumerate(zip(("drop_lstm", "rrelu", "drop_head"), got, ref))]
    assert all(ok), (tag, ok)


@pytest.mark.parametrize("n_lstm,n_head", sk.MASK_CASES, ids=["cfg2", "L1", "stride-crosses-both"])
def test_train_masks_bit_exact(nsd, dev, n_lstm, n_head):
    from nsd_amd import _lib, ops
    seed, base, (p_lstm, p_head) = sk.MASK_SEED, sk.MASK_BASE, sk.MASK_P
    new = lambda n: torch.full((n,), NAN, device=dev)      # noqa: E731
    a, b, c = new(n_lstm), new(n_head), new(n_head)
    if n_lstm:
        assert n_lstm + 2 * n_head > sk.MASK_GRID_CAP       # the loop runs
        ops.train_masks(seed, base, p_lstm, p_head, a, b, c)
        _masks_vs_oracle("2 train_masks", (a, b, c), seed, base, p_lstm, p_head)
        return
    # an L = 1 model has no inter-layer dropout: include/nsd.h sizes drop_lstm [L-1, B, T, H] = 0 elements and nsd_train_masks accepts
    # a null pointer with n_lstm = 0; ...
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib().nsd_train_masks(seed, base, p_lstm, p_head, 0, None, n_head, b.data_ptr(), c.data_ptr(), st), "train_masks")
    _masks_vs_oracle("2 train_masks n_lstm=0, null", (a, b, c), seed, base, p_lstm, p_head)
    # ... an empty tensor goes the same way through ops.train_masks ...
    b2, c2 = new(n_head), new(n_head)
    ops.train_masks(seed, base, p_lstm, p_head, a, b2, c2)
    _masks_vs_oracle("2 train_masks n_lstm=0, empty tensor", (a, b2, c2), seed, base, p_lstm, p_head)
    # ... and the trainer of such a model keeps no drop_lstm buffer: ops.train_masks(drop_lstm=None) fills the other two, one launch each
    b3, c3 = new(n_head), new(n_head)
    ops.train_masks(seed, base, p_lstm, p_head, None, b3, c3)
    _masks_vs_oracle("2 train_masks drop_lstm=None", (a, b3, c3), seed, base, p_lstm, p_head)


@pytest.mark.parametrize("step", sk.MASKS_DEV_STEPS)
def test_train_masks_dev_is_train_masks_at_the_base_the_counter_stands_for(nsd, dev, step):
    from nsd_amd import ops
    seed, (p_lstm, p_head), n_lstm, n_head = sk.MASK_SEED, sk.MASK_P, 3 * 17 * 48, 3 * 32
    base = sk.masks_dev_base(step)
    step_dev = torch.tensor([step], dtype=torch.int64, device=dev)
    on_dev = [torch.full((n,), NAN, device=dev) for n in (n_lstm, n_head, n_head)]
    on_host = [torch.full((n,), NAN, device=dev) for n in (n_lstm, n_head, n_head)]
    ops.train_masks(seed, step_dev, p_lstm, p_head, *on_dev)
    ops.train_masks(seed, base, p_lstm, p_head, *on_host)
    print(f"[2 train_masks_dev] counter {step} -> base {base}")
    assert int(step_dev.item()) == step                    # read, never written
    for t_dev, t_host in zip(on_dev, on_host):
        assert _bits_equal(f"2 train_masks_dev step={step} == host base {base}", t_dev, t_host.cpu().numpy())
    _masks_vs_oracle(f"2 train_masks_dev step={step}", on_dev, seed, base, p_lstm, p_head)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. reduction and loss sum
# ---------------------------------------------------------------------------------------------------------------------------------
def _slab_workspace(dev, spec, lay, nbytes, n_slabs, B, seed, models=1):
    """a workspace of NaN whose LSTM slabs ([models * n_slabs, align4(P_lstm)], the padding columns NaN too) and head slabs
    ([models * B, P_head]) hold integers -> (workspace, [(slabs, hslabs) per model], P_lstm)"""
    p_lstm, P = spec.offsets()["ln.weight"], spec.param_count
    stride, ph = sk.align4(p_lstm), P - p_lstm
    ws = torch.full((nbytes // 4,), NAN, device=dev)
    per_model = []
    for m in range(models):
        slabs = np.full((n_slabs, stride), NAN, np.float32)
        slabs[:, :p_lstm] = sk.int_pattern((n_slabs, p_lstm), seed + 10 * m)
        hslabs = sk.int_pattern((B, ph), seed + 10 * m + 1)
        at, hat = lay.slabs + m * n_slabs * stride, lay.hslabs + m * B * ph
        ws[at:at + n_slabs * stride] = to_dev(slabs.ravel(), dev)
        ws[hat:hat + B * ph] = to_dev(hslabs.ravel(), dev)
        per_model.append((slabs, hslabs))
    assert lay.slabs + models * n_slabs * stride <= lay.hslabs and lay.hslabs + models * B * ph <= nbytes // 4
    return ws, per_model, p_lstm


def _reduce(dev, d_model, B, T, seed, accumulate=False):
    """nsd_grad_reduce on integer slabs of one model -> (gradient tensor, reference, slab count)"""
    from nsd_amd import ops
    spec = ops.ModelSpec(**d_model)
    nbytes, lay = ops.workspace_layout(spec, B, T)
    n_slabs = int(lay.n_slabs)
    ws, [(slabs, hslabs)], p_lstm = _slab_workspace(dev, spec, lay, nbytes, n_slabs, B, seed)
    old = sk.int_pattern((spec.param_count,), seed + 2) if accumulate else None
    g = to_dev(old, dev) if accumulate else torch.full((spec.param_count,), NAN, device=dev)
    dd = spec.dims(B, T)
    ops._call("nsd_grad_reduce", dev, C.byref(dd), ws.data_ptr(), nbytes, g.data_ptr(), int(accumulate), ops.STREAM)
    return g, sk.reduce_ref(slabs, hslabs, p_lstm, old), n_slabs


DEFAULT = dict(C=8, H=48, L=2, K=3, F=32)


@pytest.mark.parametrize("mb", sk.REDUCE_B, ids=[f"B{f'{m}cus+{a}' if m else a}" for m, a in sk.REDUCE_B])
def test_grad_reduce_is_exact_on_integer_slabs(nsd, dev, cus, mb):
    B = sk.n_trials(mb, cus)
    g, ref, n_slabs = _reduce(dev, DEFAULT, B, sk.REDUCE_T, seed=B)
    print(f"[3 reduce B={B}] head slabs {B} (loops {sk.reduce_loop_trips(B)})  n_slabs {n_slabs} (loops {sk.reduce_loop_trips(n_slabs)})  cus {cus}")
    assert n_slabs == (min(B, cus) if B <= 2 * cus else min(-(-B // 2), cus))          # the H = 48 backward's plan: one slab per workgroup
    assert sk.largest_partial_sum(max(B, n_slabs)) < 2 ** 24
    assert _bits_equal(f"3 reduce B={B}", g, ref)


def test_grad_reduce_where_one_workgroup_sums_both_slab_kinds(nsd, dev):
    from nsd_amd import ops
    s = dict(sk.REDUCE_STRADDLE)
    B = s.pop("B")
    p_lstm = ops.ModelSpec(**s).offsets()["ln.weight"]
    assert p_lstm % sk.GR_COLS != 0                        # from nsd_param_layout
    g, ref, n_slabs = _reduce(dev, s, B, sk.REDUCE_T, seed=5)
    print(f"[3 reduce straddle] P_lstm {p_lstm} = {p_lstm // sk.GR_COLS} x 32 + {p_lstm % sk.GR_COLS}  n_slabs {n_slabs}  head slabs {B}")
    assert n_slabs == 1                                    # the generic path: one LSTM slab beside 65 head slabs in one workgroup
    assert _bits_equal("3 reduce straddle", g, ref)


def test_grad_reduce_with_a_partly_idle_last_workgroup(nsd, dev):
    from nsd_amd import ops
    o = dict(sk.REDUCE_ODD_HEAD)
    B = o.pop("B")
    P = ops.ModelSpec(**o).param_count
    assert P % sk.GR_COLS != 0
    g, ref, n_slabs = _reduce(dev, o, B, sk.REDUCE_T, seed=6)
    print(f"[3 reduce odd head] P {P} = {P // sk.GR_COLS} x 32 + {P % sk.GR_COLS}  n_slabs {n_slabs}")
    assert _bits_equal("3 reduce odd head", g, ref)


def test_grad_reduce_accumulates_onto_integer_gradients(nsd, dev):
    g, ref, n_slabs = _reduce(dev, DEFAULT, sk.REDUCE_ACC_B, sk.REDUCE_T, seed=7, accumulate=True)
    assert _bits_equal(f"3 reduce accumulate B={sk.REDUCE_ACC_B}", g, ref)


def test_multi_grad_reduce_gives_each_model_its_own_sums(nsd, dev):
    from nsd_amd import _lib, ops
    M, B, T = sk.MULTI_M, sk.MULTI_B, sk.REDUCE_T
    spec, lay = ops.ModelSpec(**DEFAULT), _lib.WsLayout()
    dd = spec.dims(B, T)
    nbytes = int(_lib.lib().nsd_multi_workspace_bytes(C.byref(dd), M, C.byref(lay)))
    assert nbytes > 0 and int(lay.n_slabs) == M * B        # one LSTM slab per trial and model: model m's B slabs lie behind those of 0 .. m-1
    ws, per_model, p_lstm = _slab_workspace(dev, spec, lay, nbytes, B, B, seed=8, models=M)
    g = torch.full((M, spec.param_count), NAN, device=dev)
    ops._call("nsd_multi_grad_reduce", dev, C.byref(dd), M, ws.data_ptr(), nbytes, g.data_ptr(), ops.STREAM)
    refs = [sk.reduce_ref(s, h, p_lstm) for s, h in per_model]
    assert not np.array_equal(refs[0], refs[1]) and not np.array_equal(refs[1], refs[2])
    for m in range(M):
        assert _bits_equal(f"3 multi reduce model {m}", g[m], refs[m])


@pytest.mark.parametrize("B", sk.LOSS_B)
def test_loss_sum_is_exact_on_integer_losses(nsd, dev, B):
    from nsd_amd import ops
    spec = ops.ModelSpec(**DEFAULT)
    ws = ops.new_workspace(spec, B, 1, dev).fill_(NAN)
    loss = sk.int_pattern((B,), 100 + B)
    ops.ws_view(ws, spec, B, 1, "loss").copy_(to_dev(loss, dev))
    got, ref = float(ops.loss_sum(spec, ws, B, 1).item()), float(loss.astype(np.float64).sum())
    print(f"[3 loss_sum B={B}] {got} vs {ref}")
    _note("loss sum of integers (abs)", abs(got - ref) if got == got else NAN, f"B={B}")
    assert got == ref


def test_multi_loss_sum_is_exact_per_model(nsd, dev):
    from nsd_amd import _lib, ops
    M, B = sk.MULTI_LOSS
    spec, lay = ops.ModelSpec(**DEFAULT), _lib.WsLayout()
    dd = spec.dims(B, 1)
    assert _lib.lib().nsd_multi_workspace_bytes(C.byref(dd), M, C.byref(lay)) > 0
    ws = ops.multi_workspace(spec, M, B, 1, dev).fill_(NAN)
    loss = sk.int_pattern((M, B), 9)
    ws[lay.loss:lay.loss + M * B] = to_dev(loss.ravel(), dev)
    got, ref = ops.multi_loss_sum(spec, ws, M, B, 1).cpu().numpy().astype(np.float64), loss.astype(np.float64).sum(1)
    print(f"[3 multi_loss_sum M={M} B={B}] {got} vs {ref}")
    assert len(set(ref.tolist())) == M and np.array_equal(got, ref)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. dx_kernel beyond eight channels
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc,H,L,B,T", sk.DX_ROWS, ids=[f"C{r[0]}-H{r[1]}-L{r[2]}-rows{r[3] * r[4]}" for r in sk.DX_ROWS])
def test_dx_beyond_eight_channels_vs_oracle(nsd, dev, Cc, H, L, B, T):
    from nsd_amd import _lib, ops
    d, flat, x, y, masks = head_inputs(Cc, H, sk.DX_K, sk.DX_F, B, T, L=L, safe=True)
    spec = spec_of(d)
    dd = spec.dims(B, T)
    assert int(_lib.lib().nsd_fast_path(C.byref(dd))) == 0 and ops.dx_path(spec, B, T)
    assert ops.workspace_layout(spec, B, T)[1].n_slabs == 1 and ("drop_lstm" in masks) == (L > 1)
    if (Cc, H) == (64, 64):
        assert B < 16 and 4 * H * Cc * 4 == sk.DX_LDS_LIMIT       # the generic path (the batched path starts at 16 trials); the largest W_ih0 admitted
    tag = f"4 dx C={Cc} H={H} L={L} rows={B * T}"
    ref = oracle_step(d, flat, x, labels=y, masks=masks, want_dx=True, kink=KINK_MARGIN)
    out = train_step(dev, spec, flat, x, labels=y, masks=masks, want_dx=True)
    finite = bool(np.isfinite(out["dx"]).all() and np.isfinite(out["grads"]).all())
    if finite:
        per_channel = [float(np.abs(out["dx"][..., c] - ref["dx"][..., c]).max()) for c in range(Cc)]
        print(f"[{tag}] dx error per channel / largest element: " + " ".join(f"{e / np.abs(ref['dx']).max():.1e}" for e in per_channel))
        w = grad_errors(out["grads"], ref["grads"], d)[1]
        _note("dx rows: grad lstm.weight / max", w["lstm.weight"], tag)
        _note("dx rows: grad other / max", w["other"], tag)
    errs = assert_step_vs_oracle(out, ref, d, FP32_EXACT, tag=tag)
    for k, name in (("dx", "dx / max"), ("logits", "dx rows: logits (abs)"), ("loss", "dx rows: loss (abs)")):
        _note(name, errs[k], tag)
    assert errs["dx"] <= DX_TOL and errs["logits"] < LOGIT_TOL and errs["loss"] < LOSS_TOL


# ---------------------------------------------------------------------------------------------------------------------------------
def test_zz_worst_errors_of_this_file(nsd, dev):
    """prints the worst value of every class of number compared above (run the whole file with -s) and the file's wall time"""
    torch.cuda.synchronize()
    print("\nworst errors of tests/test_gpu_small_kernels.py:")
    for k in sorted(WORST):
        print(f"  {k:48s} {WORST[k][0]:.2e}   {WORST[k][1]}")
    print(f"  bounds: zscore {sk.ZSCORE_TOL}  DX_TOL {DX_TOL}  FP32_EXACT {FP32_EXACT}")
    print(f"  wall time since import: {time.time() - T_START:.0f} s")
