"""What the tests of the bf16 sequence path share: the bounds against the float64 emulation of oracle/seq_bf16_ref.py with their
derivations, the table of cases, and the machinery of one comparison (inputs, emulation, GPU run, compare); the any-loss sequence with
its two bounds.  A bound family of its own, apart from the fp32 paths' (tests/gpu_harness.py).  Imports without a GPU:
tests/test_seq_bf16_ref_cpu.py pins the emulation at these cases on the host."""
import math
import time

import numpy as np
import torch

from oracle import nsd_oracle as orc
from oracle import seq_bf16_ref as sr
from oracle.seq_bf16_ref import bf16_round_f32
from tests.golden.make_goldens import synth_labels, synth_params, synth_x

# Bounds: about 3x the worst value measured on one MI355X with tests/test_gpu_seqpath_bf16ref.py run with -s (measured values beside
# them).  Gradients:
# relative to each tensor's largest element, per shape class; logits / probs: absolute.  The fp32-oracle bounds of the same classes
# (tests/test_gpu_seqpath.py) are SEQ_GRAD_RTOL = 6e-2 (batches of tens to hundreds of trials, with or without dropout streams),
# 0.15 (T <= 5), SEQ_GRAD_RTOL_CLEAN = 1.5e-2 (cfg5's kernels at T = 1000) and SEQ_LOGIT_TOL = 2e-2.  What is left is noise: the
# kernels' fp32 order and fast transcendentals flip single bf16 roundings, and the recurrence carries each flip on (rounding two
# intermediates of the emulation to fp32 instead moves lstm.weight_ih_l0 of fused_h256 by 3.8e-4).  The worst tensor is nearly
# always lstm.weight_ih_l0, a sum over B*T with heavy cancellation; larger batches average the noise down.
REF_LOGIT_TOL = 2e-3             # measured 1.03e-3 (cfg5_t64), 8.9e-4 (bidir_h128): 1.9x, held at 1/10 of 2e-2
REF_LOSS_TOL = 2e-5              # measured 9.1e-6 (bidir_h128), 7.7e-6 (general_l1)
REF_GRAD_RTOL_CLEAN = 2.6e-3     # measured 8.6e-4 (wide_c80), 7.8e-4 (fused_h256)                      -- 1/23 of 6e-2
REF_GRAD_RTOL_STREAMS = 4e-3     # measured 1.30e-3 (general_l3, attn.weight), 1.07e-3 (streams_h64)    -- 1/15 of 6e-2
REF_GRAD_RTOL_SHORT = 2.5e-3     # measured 9.7e-4 (H256 L2 T2), 5.8e-4 (H64 L2 T3, attn.weight)        -- 1/60 of 0.15
REF_GRAD_RTOL_LARGE = 6e-4       # measured 2.0e-4 (cfg5 T1000, B = 192), 1.2e-4 (cfg3 full)            -- 1/25 of 1.5e-2
KINK_MARGIN = 1e-3
CPU_THREADS = 16


def bound_of(kind: str) -> float:
    return {"clean": REF_GRAD_RTOL_CLEAN, "streams": REF_GRAD_RTOL_STREAMS, "short": REF_GRAD_RTOL_SHORT, "large": REF_GRAD_RTOL_LARGE}[kind]


# name -> (C, H, L, K, D, B, T, p (dropout / RReLU / head-dropout streams, None = off), route, bound kind, diag no-fused flag
#          [, F: width of fc.0, 32 where it is left out])
CASES = {
    "fused_h64":        (8, 64, 2, 5, 1, 40, 24, None, "fused2", "clean", False),
    "fused_h128":       (8, 128, 2, 3, 1, 64, 20, None, "fused2", "clean", False),
    "fused_h256":       (8, 256, 2, 5, 1, 96, 30, None, "fused2", "clean", False),
    "tiles64_h256":     (8, 256, 2, 5, 1, 1030, 3, None, "general", "clean", False),
    "general_l2_nofuse": (8, 128, 2, 5, 1, 100, 30, 0.4, "general", "streams", True),
    "fused_l2_streams": (8, 128, 2, 5, 1, 100, 30, 0.4, "fused2", "streams", False),
    "general_l1":       (8, 128, 1, 3, 1, 33, 17, None, "general", "clean", False),
    "general_l3":       (8, 64, 3, 3, 1, 70, 9, 0.4, "general", "streams", False),
    "wide_c40":         (40, 64, 2, 3, 1, 200, 7, None, "fused2", "clean", False),
    "wide_c64":         (64, 64, 2, 3, 1, 200, 7, None, "fused2", "clean", False),
    "wide_c80":         (80, 128, 2, 3, 1, 64, 10, None, "general", "clean", False),
    "streams_h64":      (8, 64, 2, 3, 1, 37, 15, 0.5, "fused2", "streams", False),
    "bidir_h128":       (24, 128, 2, 3, 2, 96, 9, 0.5, "general", "streams", False),
    "cfg5_t64":         (64, 512, 2, 5, 2, 264, 64, 0.5, "general", "streams", False),
}
SHORT_SHAPES = [(64, 2), (128, 1), (256, 2)]
SHORT_T = [1, 2, 3, 5]
# the long / full-size comparisons (seconds of the float64 emulation on 16 threads are written at the tests)
CFG5_LONG = (64, 512, 2, 5, 2, 192, 1000, None, "general", "large", False)
CFG3_FULL = (8, 256, 2, 5, 1, 1024, 250, None, "fused2", "large", False)
RNG_SEED, RNG_BASE = 0x5EEDBF16, 24


def case_F(case) -> int:
    """width of fc.0 of a case: its twelfth field, 32 (the reference's) where the case has eleven"""
    return case[11] if len(case) > 11 else 32


def kink_safe(st, F=32):
    """fc.0.bias = +-4 (alternating): the fc.0 pre-activations (spread 0.6 .. 0.8) stay far from the RReLU kink"""
    st = dict(st)
    st["fc.0.bias"] = np.where(np.arange(F) % 2 == 0, 4.0, -4.0).astype(np.float32)
    return st


def case_inputs(case, seed=0):
    """(flat params, x, labels, masks for the emulation, rng dict for the kernels) of a case"""
    C, H, L, K, D, B, T, p = case[:8]
    F = case_F(case)
    st = kink_safe(synth_params(C, H, L, K, F=F, seed=1000 + 7 * H + L + 3 * C + seed, D=D), F)
    flat = np.concatenate([st[k].ravel() for k in sr.param_layout(C, H, L, K, F, D)]).astype(np.float32)
    x, y = synth_x(B, T, C=C, seed=B + T + seed), synth_labels(B, K, seed=B + seed)
    masks, rng = {}, None
    if p is not None:
        masks = dict(drop_lstm=orc.dropout_mask(RNG_SEED, RNG_BASE, p, (L - 1, B, T, D * H)) if L > 1 else None,
                     rrelu_slope=orc.rrelu_noise(RNG_SEED, RNG_BASE + 1, (B, F)),
                     drop_head=orc.dropout_mask(RNG_SEED, RNG_BASE + 2, p, (B, F)))
        rng = dict(seed=RNG_SEED, base_stream=RNG_BASE, p_lstm=p, p_head=p)
    return flat, x, y, masks, rng


def emulate(case, flat, x, y, masks, **kw):
    C, H, L, K, D = case[:5]
    return sr.seq_bf16_ref(flat, x, y, C=C, H=H, L=L, K=K, F=case_F(case), D=D, route=case[8], threads=CPU_THREADS, **masks, **kw)


def compare(tag, case, got_logits, got_grads, ref, got_loss=None, got_probs=None, rtol=None):
    """every tensor against the emulation; prints the worst errors (pytest -s) before asserting"""
    C, H, L, K, D, B = case[:6]
    F = case_F(case)
    rtol = bound_of(case[9]) if rtol is None else rtol
    margin = sr.kink_margin(ref["fc0_pre"])
    lerr = float(np.abs(got_logits - ref["logits"]).max())
    msg = f"[{tag}] logits {lerr:.2e}"
    if got_probs is not None:
        msg += f"  probs {float(np.abs(got_probs - ref['probs']).max()):.2e}"
    if got_loss is not None:
        msg += f"  loss {abs(got_loss - ref['loss']):.2e}"
    errs = {}
    if got_grads is not None:
        errs = sr.rel_errors(got_grads, ref["grads"], C, H, L, K, F, D)
        lstm = {k: v for k, v in errs.items() if k.startswith("lstm.")}
        head = {k: v for k, v in errs.items() if not k.startswith("lstm.") and k != "attn.bias"}
        wl, wh = max(lstm.items(), key=lambda kv: kv[1]), max(head.items(), key=lambda kv: kv[1])
        msg += f"  grad/max: lstm {wl[1]:.2e} ({wl[0]})  head {wh[1]:.2e} ({wh[0]})"
    print(msg + f"  kink margin {margin:.1e}")
    assert margin > KINK_MARGIN, margin
    assert np.isfinite(got_logits).all()
    assert lerr < REF_LOGIT_TOL, lerr
    if got_probs is not None:
        assert np.abs(got_probs - ref["probs"]).max() < REF_LOGIT_TOL
    if got_loss is not None:
        assert abs(got_loss - ref["loss"]) < REF_LOSS_TOL
    # argmax agrees wherever the emulation's margin exceeds the logit bound
    if K > 1:
        srt = np.sort(ref["logits"], axis=1)
        clear = (srt[:, -1] - srt[:, -2]) > 2 * REF_LOGIT_TOL
        assert np.array_equal(got_logits.argmax(1)[clear], ref["logits"].argmax(1)[clear])
    if got_grads is not None:
        ga = sr.unflatten(got_grads, C, H, L, K, F, D)
        assert abs(float(ga["attn.bias"][0])) < 1e-4                       # analytically zero
        for k, v in errs.items():
            if k != "attn.bias":
                assert v <= rtol, (tag, k, v, rtol)
    return errs


def n_scan_launches(case, route):
    """scan groups the status word counts for one forward + one backward: one skewed launch each (fused), or per layer and
    direction (general)"""
    C, H, L, K, D, B = case[:6]
    P = H // 32
    MG = 32 if (B + 31) // 32 <= 256 // (P * D) else 64
    groups = (B + MG - 1) // MG
    return 2 * groups if route == "fused2" else 2 * L * D * groups


def run_gpu(case, flat, x, y, rng, dev, ws=None):
    from nsd_amd import ops
    C, H, L, K, D, B, T = case[:7]
    spec = ops.ModelSpec(C=C, H=H, L=L, K=K, F=case_F(case), D=D)
    assert spec.seq_path(B, T)
    ft = torch.from_numpy(flat).to(dev)
    xt, yt = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    ws = ops.seq_workspace(spec, B, T, dev) if ws is None else ws
    logits = ops.seq_train_fwd(spec, ft, xt, yt, ws, rng=rng)
    g = ops.seq_train_bwd(spec, ft, ws, B, T, rng=rng)
    loss = float(ops.seq_loss_sum(spec, ws, B, T).item()) / B
    st, one_xcd, spread = ops.seq_status(ws, detail=True)
    assert st == 0, st
    assert one_xcd + spread == n_scan_launches(case, case[8]), (one_xcd, spread, case[8])     # the route the emulation takes
    lg_inf, probs = ops.seq_infer(spec, ft, xt)
    return dict(logits=logits.cpu().numpy(), grads=g.cpu().numpy(), loss=loss, infer=lg_inf.cpu().numpy(), probs=probs.cpu().numpy(), ws=ws)


def check_case(tag, case, dev, seed=0):
    from nsd_amd import _lib, ops
    flat, x, y, masks, rng = case_inputs(case, seed)
    assert sr.product_route(case[1], case[2], case[4], case[5], case[0]) == ("fused2" if case[10] else case[8])   # (the flag forces general)
    t0 = time.time()
    ref = emulate(case, flat, x, y, masks)
    ev = emulate(case, flat, x, None, {}) if rng is not None else ref       # inference: eval head, no streams
    cpu_s = time.time() - t0
    if case[10]:                                                             # the general route of a shape the product fuses
        with _lib.diagnostic_library():
            ops.set_seq_diag_flags(fused_layers=False)
            try:
                out = run_gpu(case, flat, x, y, rng, dev)
            finally:
                ops.set_seq_diag_flags()
    else:
        out = run_gpu(case, flat, x, y, rng, dev)
    print(f"  (emulation {cpu_s:.1f} s)")
    errs = compare(tag, case, out["logits"], out["grads"], ref, got_loss=out["loss"])
    compare(tag + " infer", case, out["infer"], None, ev, got_probs=out["probs"])
    return errs, out, ref


# ---------------------------------------------------------------------------------------------------------------------------
# the any-loss sequence (tests/test_gpu_seq_autograd.py).  Bounds: about 3x the worst value measured on one MI355X.
EQUIV_RTOL = 3.5e-3              # measured 1.18e-3 (cfg5_t64, lstm.weight_ih_l0), 9.3e-4 (module x.grad): single bf16 roundings of
                                 # da flip with the last-ulp difference between the fused head's (p - onehot) * scale and torch's
DUAL_RTOL = 1e-5                 # measured 1.5e-8 (general_l3_res): fp32 accumulation order only


def rel(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-30))


def per_tensor(spec, g, ref):
    """per tensor: max |g - ref| / max |ref|.  attn.bias is left out: softmax over time is shift-invariant, so its true gradient is
    0 and both sides are fp32 round-off (it is checked against attn.weight's scale instead)"""
    offs, shapes = spec.offsets(), spec.shapes()
    out = {n: rel(g[offs[n]:offs[n] + math.prod(shapes[n])], ref[offs[n]:offs[n] + math.prod(shapes[n])]) for n in spec.names() if n != "attn.bias"}
    o, w = offs["attn.bias"], offs["attn.weight"]
    out["attn.bias/|d attn.weight|"] = float((g[o].double() - ref[o].double()).abs() / ref[w:w + spec.D * spec.H].double().abs().max())
    return out


def any_loss(spec, flat, x, ws, dlogits_of, rng, want_dx=True):
    """train_fwd_logits -> dlogits_of(logits) -> head_bwd -> train_bwd_dx: (logits, dlogits, grads, dx)"""
    from nsd_amd import ops
    B, T, _ = x.shape
    logits = ops.seq_train_fwd_logits(spec, flat, x, ws, rng=rng)
    dl = dlogits_of(logits).contiguous()
    ops.seq_head_bwd(spec, flat, ws, dl, B, T, rng=rng)
    dx = torch.empty_like(x) if want_dx else None
    g = ops.seq_train_bwd(spec, flat, ws, B, T, rng=rng, dx=dx)
    return logits, dl, g, dx


def duality(spec, flat, x, g, dx):
    """(|sum_d <bf16(W_ih0_d), dW_ih0_d> - <bf16(x), dx>|, sum |W| |dW|)"""
    offs, shapes = spec.offsets(), spec.shapes()
    lhs, scale = 0.0, 0.0
    for sfx in ("", "_reverse")[:spec.D]:
        n = f"lstm.weight_ih_l0{sfx}"
        w = bf16_round_f32(flat[offs[n]:offs[n] + math.prod(shapes[n])].contiguous()).double()
        dw = g[offs[n]:offs[n] + math.prod(shapes[n])].double()
        lhs += float((w * dw).sum())
        scale += float((w.abs() * dw.abs()).sum())
    rhs = float((bf16_round_f32(x.contiguous()).double() * dx.double()).sum())
    return abs(lhs - rhs), scale
