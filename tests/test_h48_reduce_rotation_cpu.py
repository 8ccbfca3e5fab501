"""The select-free quad reduction of the H = 48 chain roles (quad_reduce_scatter, nsd_common.h).  No GPU needed.

Host replay: a quad of lanes in float32 numpy.  The form the kernels had -- every lane keeps gate g in slot g and picks by lane with
selects -- and the form they have -- lane s keeps gate i ^ s in slot i, no select -- return the same bits per lane, for the forward's
gate sums and for the backward's unit sums followed by its two row rotations over 16 lanes.

Compiled form: nsd_lstm2_fwd48.hip and nsd_lstm2_bwd48.hip as assembly (the Makefile's flags, --cuda-device-only -S, as
tests/code_object.py compiles); a step body is what stands between two s_barrier.  In the steady-state bodies of the one-trial kernels
the reduction holds no v_cndmask_b32, and every body is at least 6 instructions shorter than the counts of the form with selects
(profiles/h48_step_census.md: layer 0 76, layer 1 82, projection 48, backward recurrences 59-63).
"""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.code_object import CSRC, ROCM

F32 = np.float32


# ---------------------------------------------------------------------------------------------------
# host replay
# ---------------------------------------------------------------------------------------------------
def _partials(rs, lanes):
    """pair accumulators [lane, value, 2] of mixed sign and magnitude (1e-6 .. 1e6), float32"""
    mag = 10.0 ** rs.uniform(-6, 6, (lanes, 4, 2))
    return (mag * rs.choice([-1.0, 1.0], (lanes, 4, 2))).astype(F32)


def _select_form(acc, q):
    """the form with selects on value-major slots: acc [4 lanes, 4 values, 2] of one quad -> per lane s the sum of value s"""
    r = (acc[:, :, 0] + acc[:, :, 1]).astype(F32)                     # r[lane, value]
    odd, hi = (q & 1) != 0, (q & 2) != 0
    send1 = np.where(odd[:, None], r[:, [0, 0, 2, 2]], r[:, [1, 1, 3, 3]])          # columns 0 / 2: what the lane sends for ra / rb
    keep1 = np.where(odd[:, None], r[:, [1, 1, 3, 3]], r[:, [0, 0, 2, 2]])
    ra = (keep1[:, 0] + send1[q ^ 1, 0]).astype(F32)
    rb = (keep1[:, 2] + send1[q ^ 1, 2]).astype(F32)
    send2, keep2 = np.where(hi, ra, rb), np.where(hi, rb, ra)
    return (keep2 + send2[q ^ 2]).astype(F32)


def _rotated_form(acc, q):
    """quad_reduce_scatter on rotated slots: slot i of lane s holds value i ^ s"""
    rot = np.stack([acc[s, np.arange(4) ^ s] for s in range(4)])      # the weights are loaded that way: same products, other slot
    r = (rot[:, :, 0] + rot[:, :, 1]).astype(F32)
    ra = (r[:, 0] + r[q ^ 1, 1]).astype(F32)
    rb = (r[:, 2] + r[q ^ 1, 3]).astype(F32)
    return (ra + rb[q ^ 2]).astype(F32)


def test_host_replay_forward_gate_sums_are_the_same_bits():
    rs, q = np.random.RandomState(4801), np.arange(4)
    for _ in range(2000):
        acc = _partials(rs, 4)
        old, new = _select_form(acc, q), _rotated_form(acc, q)
        assert old.tobytes() == new.tobytes()
        want = [F32(F32(F32(acc[s, s, 0] + acc[s, s, 1]) + F32(acc[s ^ 1, s, 0] + acc[s ^ 1, s, 1]))
                    + F32(F32(acc[s ^ 2, s, 0] + acc[s ^ 2, s, 1]) + F32(acc[s ^ 3, s, 0] + acc[s ^ 3, s, 1]))) for s in range(4)]
        assert new.tobytes() == np.array(want, F32).tobytes()          # lane s: (own + lane s^1) + (lane s^2 + lane s^3) of value s


def test_host_replay_backward_unit_sums_over_sixteen_lanes_are_the_same_bits():
    """slice_dot_t: the quad reduction per quad of the row, then v += row_ror<4>(v), v += row_ror<8>(v)"""
    rs, q, lane = np.random.RandomState(4802), np.arange(4), np.arange(16)
    for _ in range(2000):
        acc = _partials(rs, 16)
        out = []
        for form in (_select_form, _rotated_form):
            v = np.concatenate([form(acc[4 * k:4 * k + 4], q) for k in range(4)])
            v = (v + v[(lane + 4) % 16]).astype(F32)
            v = (v + v[(lane + 8) % 16]).astype(F32)
            out.append(v)
        assert out[0].tobytes() == out[1].tobytes()


# ---------------------------------------------------------------------------------------------------
# compiled form
# ---------------------------------------------------------------------------------------------------
def _bodies(name, kernel):
    """the step bodies (instruction lists between two s_barrier, (op, has a label or branch)) of one kernel of csrc/<name>.hip"""
    make = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^FLAGS\s*\?=\s*(.*)$", make, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    asm = subprocess.run([os.path.join(ROCM, "bin", "hipcc"), *flags, "--cuda-device-only", "-S", name + ".hip", "-o", "-"], check=True,
                         capture_output=True, text=True, cwd=CSRC).stdout
    bodies, body, on = [], None, False
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            on, body = kernel in m.group(1), None
            continue
        t = line.strip()
        if not on or not t:
            continue
        if re.match(r"^\.LBB\w+:", t):
            if body is not None:
                body["tested"] = True
            continue
        if t[0] in ".;" or line[0] not in "\t ":
            continue
        op = t.split()[0]
        if op == "s_endpgm":                                  # the end of one role's branch, not of the kernel
            body = None
        elif op == "s_barrier":
            if body is not None and body["ops"]:
                bodies.append(body)
            body = {"ops": [], "tested": False}
        elif body is not None:
            body["ops"].append(op)
    return bodies


def _count(ops, *prefix):
    return sum(o.startswith(prefix) for o in ops)


def _selects_in_reduction(ops, until):
    """v_cndmask_b32 between the last packed product and the first exponential (until="exp") or the last DPP add (until="dpp")"""
    last_pk = max(i for i, o in enumerate(ops) if o.startswith(("v_pk_fma_f32", "v_pk_mul_f32")))
    if until == "exp":
        end = min(i for i, o in enumerate(ops) if o.startswith("v_exp_f32") and i > last_pk)
    else:
        end = max(i for i, o in enumerate(ops) if o.startswith("v_add_f32_dpp"))
    assert end > last_pk
    return _count(ops[last_pk:end], "v_cndmask_b32")


@pytest.fixture(scope="module")
def fwd_bodies():
    return _bodies("nsd_lstm2_fwd48", "lstm2_fwd48_kernelILi1ELb0E")


@pytest.fixture(scope="module")
def bwd_bodies():
    return _bodies("nsd_lstm2_bwd48", "lstm2_bwd48_kernelILi1E")


def test_forward_steady_state_bodies_have_no_select_in_the_reduction(fwd_bodies):
    straight = [b["ops"] for b in fwd_bodies if not b["tested"] and _count(b["ops"], "s_cbranch", "s_branch") == 0]
    l0 = [o for o in straight if _count(o, "v_pk_fma_f32", "v_pk_mul_f32") == 28 and _count(o, "v_exp_f32")]
    p = [o for o in straight if _count(o, "v_pk_fma_f32", "v_pk_mul_f32") == 24 and not _count(o, "v_exp_f32")]
    # layer 1's steady-state body holds the residual's `s == 2` lane test (one branch over one LDS read), and nothing else tested
    l1 = [b["ops"] for b in fwd_bodies if _count(b["ops"], "v_pk_fma_f32", "v_pk_mul_f32") == 24 and _count(b["ops"], "v_exp_f32")
          and _count(b["ops"], "s_cbranch", "s_branch") == 1]
    print("layer 0", [len(o) for o in l0], "layer 1", [len(o) for o in l1], "projection", [len(o) for o in p])
    assert len(l0) >= 8 and len(l1) >= 8 and len(p) >= 8, (len(l0), len(l1), len(p))
    assert all(_selects_in_reduction(o, "exp") == 0 for o in l0 + l1)
    assert all(_selects_in_reduction(o, "dpp") == 0 for o in p)
    assert max(len(o) for o in l0) <= 76 - 6 and max(len(o) for o in l1) <= 82 - 6 and max(len(o) for o in p) <= 48 - 6


def test_backward_recurrence_bodies_have_no_select_in_the_reduction(bwd_bodies):
    rec = [b["ops"] for b in bwd_bodies if not b["tested"] and _count(b["ops"], "s_cbranch", "s_branch") == 0
           and _count(b["ops"], "v_pk_fma_f32", "v_pk_mul_f32") == 24 and not _count(b["ops"], "v_mfma", "v_cvt_pk_bf16_f32", "global_load_lds")]
    print("recurrences", sorted(len(o) for o in rec))
    assert len(rec) >= 8, len(rec)
    assert all(_selects_in_reduction(o, "dpp") == 0 for o in rec)
    assert min(len(o) for o in rec) <= 59 - 6 and max(len(o) for o in rec) <= 63 - 6
