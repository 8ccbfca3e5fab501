"""Early stopping for model batches on the MI355X (nsd_multi_eval of include/nsd.h, csrc/nsd_eval.hip) against the float64 restatement
tests/eval_ref.py, through ctypes with scripted logits: the entry point takes logits, so any metric trajectory is written down
directly and no model is needed.  The last sections run ModelBatchTrainer.evaluate / track_best / restore_best on three small models
and the two drivers (nsd_amd.train --kfold K --concurrent, nsd_amd.grid) with the early-stopping options on synthetic trials.

Bounds (none comes from the kernel):
  counts     n, correct, nonfinite and the confusion matrix are integers: exact
  loss_sum   within 1e-12 relative of the restatement.  Both form (log(sum_k exp(l_k - max)) + max) - l_y per row in double and add the
             rows in the same order; they differ only where the device's exp / log differ from numpy's in the last place, by about
             an ulp of |max| + loss per row: B * a few 2^-52 of the sum for the logits used here (|l| < 16, every term positive).  At
             B = 1025 that leaves three orders of margin.
  selection  records and snapshots bit for bit: the rule is run by the restatement on the eval records the device wrote (each held
             to the bounds above), and once more on the float64 records -- every trajectory keeps 1e-3 from every threshold, so no
             ulp decides, and both give the same decisions
Every launch works on kilobytes; each case takes well under a second."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import nsd_oracle as orc
from tests import buffer_contract as bc
from tests import eval_ref as er
from tests.buffer_contract import guarded, snapshot
from tests.golden.make_goldens import synth_params
from tests.gpu_harness import dev, nsd, sync_at_the_end, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-12
GAP = 1e-3


# ---------------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------------
def _lib():
    from nsd_amd import _lib as lib
    return lib


def scripted(M, B, K, seed, scale=3.0):
    rs = np.random.RandomState(seed)
    return (scale * rs.standard_normal((M, B, K))).astype(np.float32), rs.randint(0, K, (M, B)).astype(np.int32)


def call(nsd, logits, labels, out, counts=None, sel=None, params=None, state=None, P=None, M=None, B=None, K=None, nbytes=None, stream=None):
    """nsd_multi_eval through ctypes on device tensors (None stays NULL); sel: (metric, patience, min_delta) -> the return code"""
    lib = _lib()
    m, b, k = (int(v) for v in logits.shape) if logits is not None else (M, B, K)
    cp = (C.c_int32 * len(counts))(*counts) if counts is not None else None
    s = C.byref(lib.Select(*sel)) if sel is not None else None
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    ptr = lambda t: None if t is None else t.data_ptr()                                   # noqa: E731
    return lib.lib().nsd_multi_eval(m if M is None else M, b if B is None else B, k if K is None else K, ptr(logits), ptr(labels), cp, ptr(out), s,
                                    ptr(params), (int(params.shape[-1]) if params is not None else 0) if P is None else P, ptr(state),
                                    (state.numel() if state is not None else 0) if nbytes is None else nbytes, st)


def new_state(nsd, M, P, dev, fill="ones"):
    """a guarded select state of exactly nsd_select_state_bytes, pre-filled, then initialised by the library -> (bytes tensor, check)"""
    lib = _lib().lib()
    n = int(lib.nsd_select_state_bytes(M, P))
    st, check = guarded((n,), torch.uint8, dev, fill)
    assert lib.nsd_select_state_init(st.data_ptr(), n, M, P, torch.cuda.current_stream().cuda_stream) == 0
    return st, check


def new_out(M, dev, fill="nan32"):
    return guarded((M * er.EVAL_BYTES,), torch.uint8, dev, fill)


def eval_bytes(out, m):
    return bytes(out.cpu().numpy().tobytes()[m * er.EVAL_BYTES:(m + 1) * er.EVAL_BYTES])


def select_bytes(state, m):
    return bytes(state[:er.SELECT_BYTES * (m + 1)].cpu().numpy().tobytes()[m * er.SELECT_BYTES:])


def snapshot_words(state, M, P):
    from nsd_amd import ops
    off = ops.select_records_bytes(M)
    return state[off:off + 4 * M * P].cpu().numpy().view(np.uint32).reshape(M, P)


def close(got, want):
    return got == want or abs(got - want) <= LOSS_RTOL * abs(want)


def check_record(got: dict, want: dict, what):
    assert (got["n"], got["correct"], got["nonfinite"]) == (want["n"], want["correct"], want["nonfinite"]), what
    assert np.array_equal(got["confusion"], want["confusion"]), what
    if np.isnan(want["loss_sum"]):
        assert np.isnan(got["loss_sum"]), what
    else:
        rel = abs(got["loss_sum"] - want["loss_sum"]) / max(abs(want["loss_sum"]), 1e-300)
        print(f"{what}: loss_sum {got['loss_sum']!r} vs float64 {want['loss_sum']!r}  rel {rel:.2e} (bound {LOSS_RTOL:.0e})")
        assert close(got["loss_sum"], want["loss_sum"]), (what, got["loss_sum"], want["loss_sum"])


# ---------------------------------------------------------------------------------------------------------------------------------
# metrics
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("B", [1, 2, 255, 256, 257, 1025])
def test_metrics_against_float64(nsd, dev, B, K):
    """one row, the workgroup's stride edge (255 / 256 / 257) and the second and fifth trip; two models, so two workgroups"""
    lg, y = scripted(2, B, K, seed=100 * B + K)
    if K > 1:
        lg[1, ::5, K - 1] = lg[1, ::5, 0] = np.abs(lg[1, ::5]).max(axis=1) + 0.5           # exact ties at the maximum: index 0 is predicted
    out, check = new_out(2, dev)
    inputs = (to_dev(lg, dev), to_dev(y, dev))
    snap = snapshot(*inputs)
    assert call(nsd, *inputs, out) == 0
    torch.cuda.synchronize()
    check("out")
    assert snap.unchanged()
    for m in range(2):
        got, want = er.unpack_eval(eval_bytes(out, m)), er.eval_record(lg[m], y[m])
        assert want["n"] == B and got["n"] == B
        check_record(got, want, f"B={B} K={K} model {m}")
    if K > 1:
        tied = er.unpack_eval(eval_bytes(out, 1))["confusion"]
        assert tied[:, K - 1].sum() <= B - len(range(0, B, 5))                             # no tied row went to the last index


def test_logits_of_magnitude_80_do_not_overflow(nsd, dev):
    lg = np.array([[[80.0, -80.0, 3.0], [-80.0, 80.0, 79.5], [80.0, 80.0, 80.0], [-80.0, -80.0, -79.0]]], dtype=np.float32)
    y = np.array([[1, 0, 2, 0]], dtype=np.int32)                                           # losses 160, 160.47, log 3, 1.55: no cancellation
    out, check = new_out(1, dev)
    assert call(nsd, to_dev(lg, dev), to_dev(y, dev), out) == 0
    got, want = er.unpack_eval(eval_bytes(out, 0)), er.eval_record(lg[0], y[0])
    check()
    assert np.isfinite(got["loss_sum"]) and got["loss_sum"] > 320 and got["nonfinite"] == 0
    check_record(got, want, "magnitude 80")
    assert got["confusion"][2, 0] == 1                                                     # three equal logits predict index 0


def test_padding_may_hold_anything(nsd, dev):
    M, B, K = 3, 300, 3
    counts = [300, 257, 1]
    lg, y = scripted(M, B, K, seed=7)
    clean_out, _ = new_out(M, dev)
    assert call(nsd, to_dev(lg, dev), to_dev(y, dev), clean_out, counts=counts) == 0
    lg2, y2 = lg.copy(), y.copy()
    for m, c in enumerate(counts):
        lg2[m, c:] = np.nan
        lg2[m, c + 1::2] = np.inf
        y2[m, c::2], y2[m, c + 1::2] = -7, 99
    out, check = new_out(M, dev, "ones")
    assert call(nsd, to_dev(lg2, dev), to_dev(y2, dev), out, counts=counts) == 0
    check()
    for m, c in enumerate(counts):
        assert eval_bytes(out, m) == eval_bytes(clean_out, m), m                           # the padding changes no bit
        got = er.unpack_eval(eval_bytes(out, m))
        check_record(got, er.eval_record(lg[m], y[m], count=c), f"counts[{m}] = {c}")
        assert got["n"] == c and got["confusion"].sum() == c
        one, _ = new_out(1, dev)                                                           # ... and is the record of a call with B = count
        assert call(nsd, to_dev(lg[m:m + 1, :c], dev), to_dev(y[m:m + 1, :c], dev), one) == 0
        assert eval_bytes(one, 0) == eval_bytes(out, m)


@pytest.mark.parametrize("what", ["nan", "inf", "label"])
def test_a_nonfinite_counted_row_poisons_its_model_alone(nsd, dev, what):
    M, B, K = 3, 260, 4
    lg, y = scripted(M, B, K, seed=11)
    base, _ = new_out(M, dev)
    assert call(nsd, to_dev(lg, dev), to_dev(y, dev), base) == 0
    lg2, y2 = lg.copy(), y.copy()
    if what == "label":
        y2[1, 258] = K                                                                      # a label outside [0, K) among the counted rows
    else:
        lg2[1, 258, 2] = np.nan if what == "nan" else -np.inf
    out, check = new_out(M, dev)
    assert call(nsd, to_dev(lg2, dev), to_dev(y2, dev), out) == 0
    check()
    got, clean = er.unpack_eval(eval_bytes(out, 1)), er.unpack_eval(eval_bytes(base, 1))
    assert got["nonfinite"] == 1 and np.isnan(got["loss_sum"]) and got["n"] == B - 1
    check_record(got, er.eval_record(lg2[1], y2[1]), what)
    assert clean["confusion"].sum() - got["confusion"].sum() == 1
    assert eval_bytes(out, 0) == eval_bytes(base, 0) and eval_bytes(out, 2) == eval_bytes(base, 2)


# ---------------------------------------------------------------------------------------------------------------------------------
# independence of M and of the neighbours
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_models_records_do_not_depend_on_m_or_its_neighbours(nsd, dev):
    B, K, P = 270, 3, 5
    lg_me, y_me = scripted(1, B, K, seed=21)
    p_me = np.random.RandomState(22).standard_normal((1, P)).astype(np.float32)
    want = None
    for M, place, seed in ((1, 0, 0), (3, 1, 31), (3, 2, 32), (32, 0, 33), (32, 17, 34), (32, 31, 35)):
        lg, y = scripted(M, B, K, seed=seed, scale=5.0)
        p = np.random.RandomState(seed).standard_normal((M, P)).astype(np.float32)
        lg[place], y[place], p[place] = lg_me[0], y_me[0], p_me[0]
        counts = [B - (m % 3) for m in range(M)]
        counts[place] = B - 1
        out, ocheck = new_out(M, dev)
        state, scheck = new_state(nsd, M, P, dev)
        for _ in range(2):                                                                  # two evaluations: best at 1, one bad
            assert call(nsd, to_dev(lg, dev), to_dev(y, dev), out, counts=counts, sel=(0, 0, 0.0), params=to_dev(p, dev), state=state) == 0
        ocheck(), scheck()
        got = (eval_bytes(out, place), select_bytes(state, place), snapshot_words(state, M, P)[place].tobytes())
        want = want or got
        assert got == want, (M, place)
    assert er.unpack_select(want[1])["evals"] == 2 and er.unpack_select(want[1])["best_eval"] == 1 and want[2] == p_me.tobytes()


# ---------------------------------------------------------------------------------------------------------------------------------
# selection: the rule, against the restatement, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
ROWS = 20


def rows_for(correct: int, loss_correct: float, loss_wrong: float = 1.2):
    """ROWS two-class rows, label 0: `correct` of them predicted right with per-row loss loss_correct (< log 2), the rest wrong with
    loss_wrong (> log 2) -> logits [ROWS, 2].  A row (a, 0) with label 0 has loss log(1 + exp(-a))."""
    assert 0 < loss_correct < np.log(2) < loss_wrong
    a = np.where(np.arange(ROWS) < correct, -np.log(np.expm1(loss_correct)), -np.log(np.expm1(loss_wrong)))
    return np.stack([a, np.zeros(ROWS)], axis=1).astype(np.float32)


NANROW = "nan"
# per case: the rule and, per model, one (correct, loss of a correct row) per evaluation (NANROW: a non-finite evaluation).
# The mean loss of an evaluation is (correct * loss_correct + (ROWS - correct) * 1.2) / ROWS.
ALL_RIGHT = lambda *means: [(ROWS, m) for m in means]                                      # noqa: E731
# final: per model (best_eval, evals, bad, stopped, status, the 0-based evaluation whose parameters the snapshot holds) -- what the
# trajectory was written to show
CASES = {
    # improve, plateau, stop at patience = 2; then a much better evaluation that the stopped model must ignore
    "loss-stop": dict(sel=(0, 2, 0.0), models=[ALL_RIGHT(0.60, 0.50, 0.40, 0.45, 0.42, 0.05, 0.04),
                                               ALL_RIGHT(0.60, 0.61, 0.50, 0.51, 0.40, 0.41, 0.30),      # never two bad in a row
                                               ALL_RIGHT(0.30, 0.35, 0.36, 0.10, 0.09, 0.08, 0.07)],     # stopped after three evaluations
                      final=[(3, 5, 2, 1, 0, 2), (7, 7, 0, 0, 0, 6), (1, 3, 2, 1, 0, 0)]),
    # patience 0 tracks the best and never stops
    "loss-patience0": dict(sel=(0, 0, 0.0), models=[ALL_RIGHT(0.30, 0.40, 0.45, 0.50, 0.55, 0.60, 0.20),
                                                    ALL_RIGHT(0.50, 0.40, 0.30, 0.20, 0.10, 0.05, 0.02)],
                           final=[(7, 7, 0, 0, 0, 6), (7, 7, 0, 0, 0, 6)]),
    # min_delta = 0.05: 0.40 -> 0.36 is just not enough (0.01 short), 0.40 -> 0.30 clearly is
    "loss-min-delta": dict(sel=(0, 3, 0.05), models=[ALL_RIGHT(0.40, 0.36, 0.353, 0.355), ALL_RIGHT(0.40, 0.30, 0.26, 0.20)],
                           final=[(1, 4, 3, 1, 0, 0), (4, 4, 0, 0, 0, 3)]),
    # a non-finite evaluation in the middle: status bit, one bad evaluation, the snapshot stays
    "loss-nonfinite": dict(sel=(0, 2, 0.0), models=[[(ROWS, 0.5), (ROWS, 0.4), NANROW, (ROWS, 0.3), NANROW, NANROW, (ROWS, 0.1)],
                                                    [NANROW, NANROW, (ROWS, 0.5), (ROWS, 0.4)],           # stopped before any finite one
                                                    ALL_RIGHT(0.5, 0.4, 0.3, 0.2, 0.1, 0.05, 0.02)],
                           final=[(4, 6, 2, 1, 1, 3), (0, 2, 2, 1, 1, None), (7, 7, 0, 0, 0, 6)]),
    # accuracy: 15/20, again 15/20 with a lower loss (an exact tie decided by loss: better), 15/20 with a higher loss (bad), 16/20 with
    # a higher loss (better), 14/20 (bad), 16/20 with a higher loss (the tie lost: bad, stopped), then 18/20 that comes too late
    "acc-tie": dict(sel=(1, 2, 0.0), models=[[(15, 0.40), (15, 0.30), (15, 0.35), (16, 0.50), (14, 0.05), (16, 0.52), (18, 0.6)]],
                    final=[(4, 6, 2, 1, 0, 3)]),
    # min_delta = 0.12 on the accuracy: 16/20 and 17/20 are not enough above 15/20, 18/20 is; 18/20 again with a lower loss; 20/20 is not
    # enough above 18/20
    "acc-min-delta": dict(sel=(1, 0, 0.12), models=[[(15, 0.40), (16, 0.10), (17, 0.60), (18, 0.05), (18, 0.01), (20, 0.3)]],
                          final=[(5, 6, 1, 0, 0, 4)]),
}


def _designed_gaps(case):
    """the thresholds every evaluation is compared with, from the designed means: each keeps GAP from them"""
    metric, patience, min_delta = case["sel"]
    for traj in case["models"]:
        best = None
        for step in traj:
            if step == NANROW:
                continue
            c, lc = step
            mean, acc = (c * lc + (ROWS - c) * 1.2) / ROWS, c / ROWS
            if best is not None:
                if metric == 0:
                    assert abs(mean - (best[0] - min_delta)) >= GAP, (traj, step)
                else:
                    assert acc == best[1] or abs(acc - (best[1] + min_delta)) >= GAP, (traj, step)
                    assert acc != best[1] or abs(mean - best[0]) >= GAP, (traj, step)
                better = mean < best[0] - min_delta if metric == 0 else (acc > best[1] + min_delta or (acc == best[1] and mean < best[0]))
            if best is None or better:
                best = (mean, acc)


@pytest.mark.parametrize("name", list(CASES))
def test_selection_follows_the_rule_bit_for_bit(nsd, dev, name):
    case = CASES[name]
    _designed_gaps(case)
    metric, patience, min_delta = case["sel"]
    M, P = len(case["models"]), 37
    steps = max(len(t) for t in case["models"])
    state, scheck = new_state(nsd, M, P, dev)
    prefill = snapshot_words(state, M, P).copy()
    assert (prefill == 0xFFFFFFFF).all() and state[:er.SELECT_BYTES * M].sum().item() == 0     # init zeroes the records, nothing else
    on_device = er.Selector(M, ("loss", "acc")[metric], patience, min_delta)                # fed the records the device wrote
    in_double = er.Selector(M, ("loss", "acc")[metric], patience, min_delta)                # fed the float64 records
    params_at = []
    y = np.zeros((M, ROWS), dtype=np.int32)
    for t in range(steps):
        lg = np.zeros((M, ROWS, 2), dtype=np.float32)
        for m, traj in enumerate(case["models"]):
            step = traj[min(t, len(traj) - 1)]
            lg[m] = rows_for(ROWS, 0.5) if step == NANROW else rows_for(*step)
            if step == NANROW:
                lg[m, 3, 1] = np.nan
        params = np.random.RandomState(1000 + t).standard_normal((M, P)).astype(np.float32)
        params_at.append(params)
        out, ocheck = new_out(M, dev)
        assert call(nsd, to_dev(lg, dev), to_dev(y, dev), out, sel=case["sel"], params=to_dev(params, dev), state=state) == 0
        ocheck(), scheck()
        dev_recs = [er.unpack_eval(eval_bytes(out, m)) for m in range(M)]
        ref_recs = [er.eval_record(lg[m], y[m]) for m in range(M)]
        for m in range(M):
            check_record(dev_recs[m], ref_recs[m], f"{name} t={t} model {m}")
        on_device.offer(dev_recs)
        in_double.offer(ref_recs)
        snap = snapshot_words(state, M, P)
        for m in range(M):
            assert select_bytes(state, m)[:er.SELECT_BYTES] == er.pack_select(on_device.records[m]), (name, t, m, er.unpack_select(select_bytes(state, m)[:40]),
                                                                                                      on_device.records[m])
            a, b = on_device.records[m], in_double.records[m]
            assert all(a[k] == b[k] for k in ("best_correct", "best_n", "best_eval", "evals", "bad", "stopped", "status")), (name, t, m, a, b)
            assert close(a["best_loss"], b["best_loss"])
            held = on_device.held[m]
            want = prefill[m] if held is None else params_at[held][m].view(np.uint32)
            assert np.array_equal(snap[m], want), (name, t, m, held)
    got = [(r["best_eval"], r["evals"], r["bad"], r["stopped"], r["status"], h) for r, h in zip(on_device.records, on_device.held)]
    assert got == case["final"], (name, got)


# ---------------------------------------------------------------------------------------------------------------------------------
# the snapshot copy
# ---------------------------------------------------------------------------------------------------------------------------------
def odd_words(M, P, salt):
    """distinct 32-bit words: NaNs with payloads, -0.0, denormals, infinities and ordinary numbers"""
    i = np.arange(M * P, dtype=np.uint64) + np.uint64(salt * 7919)
    kinds = np.stack([0x7F800001 + i, 0xFFC00000 + i, 0x00000001 + i, 0x80000001 + i, 0x3F800000 + 3 * i, 0xC0490FDB + i]).astype(np.uint64)
    w = kinds[i % 6, np.arange(M * P)].astype(np.uint32)
    w[::11] = 0x80000000                                                                    # -0.0
    return w.reshape(M, P)


def _real_p():
    from nsd_amd import ops
    return ops.ModelSpec(C=8, H=48, L=2, K=3, F=32).param_count


@pytest.mark.parametrize("P", [1, 3, 4, 5, 7, 1024 + 2, "real"])
@pytest.mark.parametrize("shifted", [False, True])
def test_snapshot_is_the_row_bit_for_bit_and_nothing_else_is_written(nsd, dev, P, shifted):
    """M = 3: rows 1 and 2 start at m * P floats, misaligned for 16-byte accesses unless m * P % 4 == 0.  shifted: the parameters start
    one float past a 16-byte boundary, so source and destination rows are misaligned differently (the word-by-word route)."""
    P = _real_p() if P == "real" else P
    M, B = 3, 6
    good, bad = rows_for(ROWS, 0.3)[:B], rows_for(ROWS, 0.6)[:B]
    y = to_dev(np.zeros((M, B), dtype=np.int32), dev)
    state, scheck = new_state(nsd, M, P, dev)
    out, ocheck = new_out(M, dev)

    def offer(words, quality):
        store = torch.zeros(M * P + 1, dtype=torch.int32, device=dev)
        p = store[1:] if shifted else store[:-1]
        p.copy_(torch.from_numpy(words.view(np.int32).reshape(-1)))
        p = p.view(torch.float32).view(M, P)
        lg = np.stack([dict(g=good, b=bad, n=np.full_like(good, np.nan))[q] for q in quality])
        snap = snapshot(p)
        assert call(nsd, to_dev(lg, dev), y, out, sel=(0, 0, 0.0), params=p, state=state) == 0
        torch.cuda.synchronize()
        assert snap.unchanged()
        ocheck(), scheck()
        return snapshot_words(state, M, P)

    w1, w2, w3 = odd_words(M, P, 1), odd_words(M, P, 2), odd_words(M, P, 3)
    s = offer(w1, "bng")                        # model 0: first finite, model 1: non-finite, model 2: first finite
    assert np.array_equal(s[0], w1[0]) and np.array_equal(s[2], w1[2])
    assert (s[1] == 0xFFFFFFFF).all()                                                       # every word as pre-filled
    s = offer(w2, "ggb")                        # model 0 improves, model 1 has its first finite one, model 2 gets worse
    assert np.array_equal(s[0], w2[0]) and np.array_equal(s[1], w2[1]) and np.array_equal(s[2], w1[2])
    s = offer(w3, "bbn")                        # nobody improves: no word changes
    assert np.array_equal(s[0], w2[0]) and np.array_equal(s[1], w2[1]) and np.array_equal(s[2], w1[2])
    recs = [er.unpack_select(select_bytes(state, m)[:er.SELECT_BYTES]) for m in range(M)]
    assert [(r["best_eval"], r["evals"], r["bad"], r["status"]) for r in recs] == [(2, 3, 1, 0), (2, 3, 1, 1), (1, 3, 2, 1)]


# ---------------------------------------------------------------------------------------------------------------------------------
# buffer contract, streams and graph replay
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", ["zeros", "ones", "nan32", "side"])
def test_buffer_and_stream_contract(nsd, dev, fill):
    """out and sel_state of exactly the stated sizes between guards, whatever they held before; inputs unchanged; a side stream gives
    the bits of the current one"""
    M, B, K, P = 5, 300, 3, 1026
    lg, y = scripted(M, B, K, seed=41)
    params = np.random.RandomState(42).standard_normal((M, P)).astype(np.float32)
    counts = [300, 299, 257, 256, 1]

    def run(fill):
        pre = "nan32" if fill == "side" else fill
        inputs = (to_dev(lg, dev), to_dev(y, dev), to_dev(params, dev))
        snap = snapshot(*inputs)
        out, ocheck = new_out(M, dev, pre)
        state, scheck = new_state(nsd, M, P, dev, pre)
        for _ in range(2):
            assert call(nsd, inputs[0], inputs[1], out, counts=counts, sel=(1, 1, 0.0), params=inputs[2], state=state) == 0
        torch.cuda.current_stream().synchronize()
        ocheck("out"), scheck("sel_state")
        assert snap.unchanged()
        return bytes(out.cpu().numpy().tobytes()), bytes(state.cpu().numpy().tobytes())

    want = run("zeros")
    if fill == "side":
        cur, side = torch.cuda.current_stream(dev), torch.cuda.Stream(dev)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            got = run("side")
    else:
        got = run(fill)
    assert got[0] == want[0] and got[1] == want[1]                                          # every model improved once: no pre-fill is left to differ
    recs = [er.unpack_select(want[1][m * 40:(m + 1) * 40]) for m in range(M)]
    assert all((r["best_eval"], r["evals"], r["bad"], r["stopped"]) == (1, 2, 1, 1) for r in recs)


def test_graph_replay_of_infer_and_eval_counts_three_evaluations(nsd, dev):
    from nsd_amd import ops
    spec = ops.ModelSpec(C=8, H=48, L=2, K=3, F=32)
    M, B, T, P = 3, 5, 6, spec.param_count
    d = orc.Dims(C=8, H=48, L=2, K=3, F=32)
    params = to_dev(np.stack([orc.flatten_state(synth_params(8, 48, 2, 3, F=32, seed=50 + m), d) for m in range(M)]), dev)
    rs = np.random.RandomState(51)
    x = to_dev((2.7 * rs.standard_normal((M, B, T, 8))).astype(np.float32), dev)
    y = to_dev(rs.randint(0, 3, (M, B)).astype(np.int32), dev)
    logits = torch.empty((M, B, 3), dtype=torch.float32, device=dev)
    scratch = torch.empty(max(bc.multi_infer_scratch_bytes(spec, M, B, T), 4), dtype=torch.uint8, device=dev)
    counts, rule = [5, 4, 3], dict(metric="loss", patience=0, min_delta=0.0)

    def pair(out, state):
        ops.multi_infer(spec, params, x, want_probs=False, logits=logits, scratch=scratch)
        ops.multi_eval(logits, y, counts=counts, out=out, select=rule, params=params, state=state)

    out_e, state_e = ops.eval_buffer(M, dev), ops.select_state(M, P, dev)
    for _ in range(3):
        pair(out_e, state_e)
    torch.cuda.synchronize()

    out_g, state_g = ops.eval_buffer(M, dev), ops.select_state(M, P, dev)
    cur, side = torch.cuda.current_stream(dev), torch.cuda.Stream(dev)
    side.wait_stream(cur)
    with torch.cuda.stream(side):                                                           # eager warm-up on a side stream
        pair(out_g, state_g)
    cur.wait_stream(side)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pair(out_g, state_g)
    state_g.copy_(ops.select_state(M, P, dev))                                              # forget the warm-up; the snapshot rows keep what they hold
    out_g.fill_(0xFF)
    snap = snapshot(params, x, y)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize(dev)
    assert snap.unchanged()
    recs = ops.select_records(state_g, M)
    assert [(r["evals"], r["best_eval"], r["bad"]) for r in recs] == [(3, 1, 2)] * M
    assert torch.equal(out_g, out_e) and torch.equal(state_g, state_e)
    assert torch.equal(ops.select_snapshot(state_g, M, P), params)
    ev = ops.eval_records(out_g, M, 3)
    lg = logits.cpu().numpy()
    for m in range(M):
        check_record(dict(ev[m], confusion=np.pad(ev[m]["confusion"], ((0, 5), (0, 5)))), er.eval_record(lg[m], y[m].cpu().numpy(), counts[m]), f"graph model {m}")


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals launch nothing
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_output_as_it_was(nsd, dev):
    M, B, K, P = 3, 16, 3, 10
    lg, y = (to_dev(a, dev) for a in scripted(M, B, K, seed=61))
    params = to_dev(np.ones((M, P), dtype=np.float32), dev)
    out, ocheck = new_out(M, dev, "nan32")
    state, scheck = new_state(nsd, M, P, dev, "ones")
    before = snapshot(out, state)
    L = _lib().lib()
    good = (0, 2, 0.0)
    base = dict(logits=lg, labels=y, out=out, sel=good, params=params, state=state)
    nan = float("nan")
    cases = [dict(M=0), dict(M=33), dict(K=0), dict(K=9), dict(B=0), dict(counts=[16, 0, 16]), dict(counts=[16, 16, 17]),
             dict(M=32, B=2 ** 31 // 64, K=8), dict(logits=None, M=M, B=B, K=K), dict(labels=None), dict(sel=(2, 0, 0.0)), dict(sel=(0, -1, 0.0)),
             dict(sel=(1, 0, -1e-3)), dict(sel=(1, 0, nan)), dict(params=None, P=P), dict(state=None, nbytes=state.numel()), dict(P=0)]
    for kw in cases:
        assert call(nsd, **{**base, **kw}) == -1, kw
        assert L.nsd_last_error().decode().startswith("multi_eval:"), kw
    assert call(nsd, **{**base, "out": None}) == -1
    assert call(nsd, **{**base, "nbytes": state.numel() - 1}) == -3 and "nsd_select_state_bytes" in L.nsd_last_error().decode()
    assert L.nsd_select_state_init(state.data_ptr(), state.numel() - 1, M, P, None) == -3
    torch.cuda.synchronize()
    ocheck(), scheck()
    assert before.unchanged()
    assert call(nsd, **base) == 0                                                           # ... and the same buffers are fine to use
    torch.cuda.synchronize()
    assert before.changed() == [0, 1]


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end: ModelBatchTrainer.evaluate / track_best / restore_best
# ---------------------------------------------------------------------------------------------------------------------------------
def separable(n, T, seed, K=3):
    """nsd_amd.grid's synthetic data: class-dependent mean shift on one channel"""
    rs = np.random.RandomState(seed)
    y = rs.randint(0, K, n).astype(np.int32)
    x = (2.7 * rs.standard_normal((n, T, 8))).astype(np.float32)
    x[np.arange(n), :, y % 8] += 1.5
    return x, y


def trainer_of(nsd, dev, lrs=(1e-3, 3e-2, 0.3)):
    models = []
    for m in range(len(lrs)):
        torch.manual_seed(70 + m)
        models.append(nsd.EEG_LSTM(8, 48, 2, 3, 0.6).to(dev).train())
    return nsd.ModelBatchTrainer(models, lr=list(lrs), seeds=[5, 6, 7])


@pytest.fixture(scope="module")
def e2e_data(dev):
    x, y = separable(16 * 4 + 19, 12, seed=71)
    return to_dev(x, dev), to_dev(y, dev)


def test_evaluate_is_the_metrics_of_the_logits_multi_infer_returns(nsd, dev, e2e_data):
    from nsd_amd import ops
    x, y = e2e_data
    mbt = trainer_of(nsd, dev)
    for s in range(12):
        lo = 16 * (s % 4)
        mbt.step(x[lo:lo + 16], y[lo:lo + 16])
    held_x = torch.stack([x[64:83], x[60:79], x[40:59]])                                    # per-model windows, 19 each
    held_y = torch.stack([y[64:83], y[60:79], y[40:59]])
    counts = [19, 18, 1]
    got = mbt.evaluate(held_x, held_y, counts)
    assert mbt._sel_state is None                                                           # metrics only: nothing is allocated for selection
    logits, _ = ops.multi_infer(mbt.spec, mbt.params, held_x, want_probs=False)
    lg, yy = logits.cpu().numpy(), held_y.cpu().numpy()
    for m in range(3):
        want = er.eval_record(lg[m], yy[m], counts[m])
        assert (got[m]["n"], got[m]["nonfinite"]) == (counts[m], 0) and got[m]["confusion"].shape == (3, 3)
        assert np.array_equal(got[m]["confusion"], want["confusion"][:3, :3]) and got[m]["acc"] == want["correct"] / want["n"]
        print(f"model {m}: loss {got[m]['loss']!r} vs float64 {want['loss_sum'] / want['n']!r}, acc {got[m]['acc']:.3f}")
        assert close(got[m]["loss"] * counts[m], want["loss_sum"]) or close(got[m]["loss"], want["loss_sum"] / want["n"])
    shared = mbt.evaluate(x[64:83], y[64:83])                                               # shared windows, counts None
    assert shared[0]["n"] == 19 and shared[0]["confusion"].tolist() == got[0]["confusion"].tolist() and shared[0]["loss"] == got[0]["loss"]


def test_track_best_and_restore_best_give_each_model_its_best_epoch(nsd, dev, e2e_data):
    x, y = e2e_data
    mbt = trainer_of(nsd, dev)
    ptrs = [[p.data_ptr() for p in mdl.parameters()] for mdl in mbt.models]
    held, at_epoch, seen = (x[64:83], y[64:83]), [], []
    for epoch in range(6):
        for s in range(2):
            lo = 16 * ((2 * epoch + s) % 4)
            mbt.step(x[lo:lo + 16], y[lo:lo + 16])
        at_epoch.append(mbt.params.clone())
        seen.append(mbt.track_best(*held, metric="loss", patience=2))
    best = mbt.best_evals()
    print("best evaluations", best, "stopped", mbt.stopped(), "inner losses", [[round(r[m]["loss"], 4) for r in seen] for m in range(3)])
    ref = er.Selector(3, "loss", 2, 0.0)
    for r in seen:                                                                          # the host-visible trajectory decides the same
        ref.offer([dict(loss_sum=e["loss"] * e["n"], n=e["n"], correct=round(e["acc"] * e["n"])) for e in r])
    assert best == [r["best_eval"] for r in ref.records] and mbt.stopped() == [bool(r["stopped"]) for r in ref.records]
    assert [e["best_eval"] for e in seen[-1]] == best and mbt.all_stopped() == all(mbt.stopped())
    assert all(1 <= b <= 6 for b in best)
    before = [mbt.best_state_dict(m) for m in range(3)]
    with pytest.raises(nsd.NsdError, match="one rule per trainer"):
        mbt.track_best(*held, metric="acc", patience=2)
    assert mbt.restore_best() == best
    for m, mdl in enumerate(mbt.models):
        want = at_epoch[best[m] - 1][m]
        assert torch.equal(mbt.params[m].view(torch.int32), want.view(torch.int32))
        offs = mbt.spec.offsets()
        assert set(mdl.state_dict()) == set(offs)
        for n, p in mdl.state_dict().items():                                               # state_dict() sees the restored model, bit for bit
            assert torch.equal(p.reshape(-1).view(torch.int32), want[offs[n]:offs[n] + p.numel()].view(torch.int32)), (m, n)
            assert torch.equal(before[m][n], p)
        assert [p.data_ptr() for p in mdl.parameters()] == ptrs[m]                          # the modules are still views into trainer.params
        assert mdl.flat_parameters().data_ptr() == mbt.params[m].data_ptr()
        assert not mbt.m[m].any() and not mbt.v[m].any()                                    # a restored model restarts its moments
    mbt.step(x[:16], y[:16])                                                                # ... and trains on


def test_a_trainer_that_never_asks_issues_the_calls_it_always_issued(nsd, dev, e2e_data):
    from nsd_amd import ops
    x, y = e2e_data
    names = []

    class Hook:
        def __init__(self, name):
            names.append(name)

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

    plain, asking = trainer_of(nsd, dev), trainer_of(nsd, dev)
    ops.set_launch_hook(Hook)
    try:
        for s in range(4):
            plain.step(x[16 * s:16 * s + 16], y[16 * s:16 * s + 16])
    finally:
        ops.set_launch_hook(None)
    assert names == ["nsd_multi_train_fwd", "nsd_multi_train_bwd", "nsd_multi_grad_reduce_clip_adam_each"] * 4, names
    assert plain._sel_state is None and plain._sel_rule is None and plain.best_evals() == [0, 0, 0] and not plain.all_stopped()
    for s in range(4):                                                                      # evaluating between the steps changes no step
        asking.step(x[16 * s:16 * s + 16], y[16 * s:16 * s + 16])
        asking.evaluate(x[64:83], y[64:83])
        asking.track_best(x[64:83], y[64:83], patience=1)
    assert torch.equal(plain.params.view(torch.int32), asking.params.view(torch.int32))
    assert torch.equal(plain.m.view(torch.int32), asking.m.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------------
# the drivers
# ---------------------------------------------------------------------------------------------------------------------------------
def _json_lines(capsys):
    import json
    return [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]


def test_train_concurrent_with_early_stopping_scores_the_best_epoch_models(nsd, dev, tmp_path, capsys):
    from nsd_amd import train
    out = str(tmp_path / "m.pth")
    argv = ["--synthetic", "120", "--T", "12", "--kfold", "3", "--concurrent", "--epochs", "6", "--batch", "14", "--lr", "0.01", "--seed", "3",
            "--out", out, "--save-folds", "--early-stop-patience", "2", "--early-stop-metric", "acc", "--inner-fraction", "0.25"]
    assert train.main(argv) == 0
    recs = _json_lines(capsys)
    done = [r for r in recs if r.get("done")][0]
    folds = [r for r in recs if "fold" in r and "n_val" in r]
    assert done["selection"] == "inner split: early stopping on acc, patience 2" and len(folds) == 3
    assert done["best_epochs"] == [f["best_epoch"] for f in folds] and all(0 <= b < done["epochs_run"] <= 6 for b in done["best_epochs"])
    assert done["args"]["early_stop_patience"] == 2 and "early_stop_min_delta" not in done["args"]
    for f, acc, path in zip(folds, done["acc_val_folds"], done["fold_checkpoints"]):
        conf = np.array(f["confusion_val"])
        assert conf.shape == (3, 3) and conf.sum() == f["n_val"] and f["n_train"] + f["n_inner"] + f["n_val"] == 120
        assert acc == f["acc_val_best_epoch"] == round(np.trace(conf) / f["n_val"], 4)
        assert set(torch.load(path)) == set(nsd.EEG_LSTM(8, 48, 2, 3, 0.6).state_dict())
    logged = [r for r in recs if r.get("concurrent") and "epoch" in r]
    assert logged and all({"loss_inner", "acc_inner", "best_epoch", "stopped", "acc_train", "acc_val"} <= set(r) for r in logged)
    # nothing asked for: the lines of before, field for field
    assert train.main(argv[:argv.index("--early-stop-patience")] + ["--epochs", "2"]) == 0
    recs = _json_lines(capsys)
    done = [r for r in recs if r.get("done")][0]
    assert done["selection"] == "none: fixed epoch count, last-epoch model" and "best_epochs" not in done
    assert not any(k.startswith("early_stop") or k == "inner_fraction" for k in done["args"])
    assert all("loss_inner" not in r and "n_inner" not in r for r in recs)


def test_grid_with_early_stopping_reports_the_rule_and_the_chosen_epochs(nsd, dev, capsys):
    from nsd_amd import grid
    assert grid.main(["--synthetic", "120", "--T", "12", "--kfold", "3", "--epochs", "4", "--batch", "14", "--seed", "3", "--grid", "lr=1e-3,1e-2",
                      "--early-stop-patience", "0", "--log-every", "100"]) == 0
    recs = _json_lines(capsys)
    summaries = [r for r in recs if r.get("summary")]
    assert len(summaries) == 2
    for s in summaries:
        assert s["selection"] == "inner split: early stopping on loss, patience 0" and len(s["best_epochs"]) == 3 == len(s["confusion_val"])
        assert all(0 <= b < 4 for b in s["best_epochs"])
        accs = [round(np.trace(np.array(c)) / np.array(c).sum(), 4) for c in s["confusion_val"]]
        assert accs == s["acc_val_folds"]
