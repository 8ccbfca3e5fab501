"""Float64 emulation of the bf16 sequence path -- TEST INFRASTRUCTURE ONLY.

Only tests/ may import this module; the product package never does.

The bf16 sequence path (csrc/nsd_seq.hip, nsd_scan.hip, nsd_scan2.hip, nsd_gemm_bf16.hip, nsd_head_tm.hip) rounds to
bf16 at fixed points and accumulates in fp32 everywhere else.  The fp32 oracles (oracle/nsd_oracle.c, torch) differ from it by
percents, which is more than a wrong term in a gradient.  This module computes the SAME operation in float64 and rounds to bf16
(round to nearest even, as pack_bf16x2 in csrc/nsd_bf16.h) exactly where the kernels round, and nowhere else.  What is left
between it and the kernels is fp32 accumulation order, the ulps of the fast transcendental functions, and the rare bf16 rounding
flip those cause.

The backward pass is an explicit BPTT: it rounds da, the exchanged partial sums of dh and the input-gradient tiles, which autograd
cannot express.  The head (attention pooling, LayerNorm, fc, CE) has no rounding point on the path (it reads the bf16 top sequence
and computes in fp32), so it is differentiated with float64 autograd.

Not emulated: the residual extension (its fp32-oracle tests in tests/test_gpu_seqpath.py stay the check).

Rounding points (name: where the kernels round; `rounding_off` turns single points off for the sensitivity table):
  x      the EEG windows as bf16 (seq_xbf_kernel, nsd_scan.hip:91-99)
  w      GEMM / scan weight operands W_ih, W_hh as bf16 (seq_prep_kernel, nsd_scan.hip:53-89); biases stay fp32
  wscale fused route: the dropout scale folded into W_ih1, rounded once more (nsd_scan2.hip:58-65)
  h      h_t as bf16: exchange ring, hs rows, the head's input (nsd_scan2.hip:290-291, nsd_scan.hip:294-295)
  lk     the linked output bf16(bf16(h) * multiplier) (nsd_scan2.hip:292-294, nsd_scan.hip:320-327)
  xproj  general route: input projection + bias stored as bf16 accumulator tiles (nsd_seq.h:19, nsd_gemm_bf16.hip:89-96)
  c      saved cell state as bf16 (nsd_scan2.hip:315, nsd_scan.hip:330); the running c stays fp32
  gates  saved activated gates as bf16 (nsd_scan2.hip:316-331, nsd_scan.hip:333-337)
  da     gate pre-activation gradients as bf16 (cell_apply, nsd_scan_common.h:264-275); the bias sums use the fp32 da
  psum   partial sums of dh, one per member, as bf16, added in fp32 in member order (nsd_scan2.hip:535-537 / 628-633,
         nsd_scan.hip:500-525 / 580-592)
  din    general route: input gradient of a lower layer as bf16 tiles (GEMM_EPI_TILE_WAVE_BF16, nsd_seq.hip:419-425)
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, Optional

import numpy as np
import torch

ROUNDING_POINTS = ("x", "w", "wscale", "h", "lk", "xproj", "c", "gates", "da", "psum", "din")

# Mutants: switches that reproduce plausible kernel bugs (tests/test_seq_bf16_ref_cpu.py shows that each one moves the result by
# several times the GPU bounds), plus two "moved" rounding points for the sensitivity table.
MUTANTS = ("dwhh_first_step",    # dW_hh sees a nonzero h_{t-1} at a batch tile's first step (b_shift / b_period wrap)
           "stale_member",       # one member's partial sum of dh is taken from the step before (stale for one step)
           "forget_c_edge",      # the forget-gate term uses c_t instead of c_{t-1} = 0 at the sequence edge
           "reverse_init",       # the reverse-direction scan starts from the forward direction's final state, not zero
           "dscore_last",        # the attention-score term of d out is dropped at the last step
           "keep_bit_lost",      # unit 0's dropout keep bit reads as dropped in the backward pass
           "psum_once",          # moved rounding point: the member partial sums are added first and rounded once
           "lk_unrounded_h")     # moved rounding point: the multiplier acts on the fp32 h instead of the bf16 h

RRELU_EVAL_SLOPE = float(np.float32((0.125 + 1.0 / 3.0) / 2.0))


def bf16_round_f32(a: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16, round to nearest even (pack_bf16x2, csrc/nsd_bf16.h:30-35), returned as fp32 holding the bf16 value.
    NaN stays NaN (quiet), +-Inf stay, overflow rounds to Inf, signed zeros keep their sign."""
    assert a.dtype == torch.float32
    u = a.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    r = torch.where(torch.isnan(a), (u | 0x00400000) & 0xFFFF0000, r)
    r = torch.where(r >= 0x80000000, r - 0x100000000, r)
    return r.to(torch.int32).view(torch.float32)


def param_layout(C: int, H: int, L: int, K: int, F: int = 32, D: int = 1) -> Dict[str, tuple]:
    """name -> (offset, shape) in nsd_seq_param_layout order (torch's state_dict order, `_reverse` after each layer's forward)."""
    out, p, DH = {}, 0, D * H
    for l in range(L):
        I = C if l == 0 else DH
        for d in range(D):
            sfx = "_reverse" if d else ""
            for nm, shp in (("weight_ih", (4 * H, I)), ("weight_hh", (4 * H, H)), ("bias_ih", (4 * H,)), ("bias_hh", (4 * H,))):
                out[f"lstm.{nm}_l{l}{sfx}"] = (p, shp)
                p += int(np.prod(shp))
    for nm, shp in (("ln.weight", (DH,)), ("ln.bias", (DH,)), ("attn.weight", (1, DH)), ("attn.bias", (1,)),
                    ("fc.0.weight", (F, DH)), ("fc.0.bias", (F,)), ("fc.3.weight", (K, F)), ("fc.3.bias", (K,))):
        out[nm] = (p, shp)
        p += int(np.prod(shp))
    return out


def param_count(C, H, L, K, F=32, D=1) -> int:
    lo = param_layout(C, H, L, K, F, D)
    o, s = list(lo.values())[-1]
    return o + int(np.prod(s))


def unflatten(flat: np.ndarray, C, H, L, K, F=32, D=1) -> Dict[str, np.ndarray]:
    return {k: np.asarray(flat[o:o + int(np.prod(s))]).reshape(s) for k, (o, s) in param_layout(C, H, L, K, F, D).items()}


def product_route(H: int, L: int, D: int, B: int, C: int, cus: int = 256, residual: bool = False) -> str:
    """The route nsd_seq.hip:57-61 (derive) takes on a device with `cus` CUs: "fused2" or "general"."""
    P = H // 32
    cap = cus // (P * D)
    MG = 32 if (B + 31) // 32 <= cap else 64
    CP = (C + 15) // 16 * 16
    ok2 = H in (64, 128, 256) and MG == 32
    return "fused2" if (D == 1 and L == 2 and not residual and CP <= 64 and ok2) else "general"


class _Rounder:
    def __init__(self, rounding, rounding_off: Iterable[str]):
        off = set(rounding_off)
        bad = off - set(ROUNDING_POINTS)
        assert not bad, bad
        self.on = {p: bool(rounding) and p not in off for p in ROUNDING_POINTS}

    def __call__(self, point: str, v: torch.Tensor) -> torch.Tensor:
        if not self.on[point]:
            return v
        return bf16_round_f32(v.to(torch.float32)).to(torch.float64)

    def store(self, point: str, v: torch.Tensor) -> torch.Tensor:
        """a saved sequence: rounded values are exact in bf16 storage (a quarter of the memory at full size)"""
        return bf16_round_f32(v.to(torch.float32)).to(torch.bfloat16) if self.on[point] else v.clone()


def _gate_cols(H: int, P: int) -> torch.Tensor:
    """gate rows of member q's 32 units, in [q][g][u] order: torch row g*H + 32q + u"""
    g = torch.arange(4).view(1, 4, 1)
    u = torch.arange(32).view(1, 1, 32)
    q = torch.arange(P).view(P, 1, 1)
    return (g * H + 32 * q + u).reshape(P, 128)


def seq_bf16_ref(params: np.ndarray, x: np.ndarray, labels: Optional[np.ndarray], *, C: int, H: int, L: int, K: int, F: int = 32,
                 D: int = 1, route: str, members: Optional[int] = None, rounding=True, rounding_off: Iterable[str] = (),
                 drop_lstm: Optional[np.ndarray] = None, rrelu_slope: Optional[np.ndarray] = None, drop_head: Optional[np.ndarray] = None,
                 mutants: Iterable[str] = (), threads: Optional[int] = None) -> Dict[str, np.ndarray]:
    """One evaluation of the bf16 sequence path in float64.

    params: flat fp32 vector in nsd_seq_param_layout order; x [B, T, C] fp32; labels [B] (None: inference, no gradient).
    route: "fused2" (the skewed two-layer launch, nsd_scan2.hip) or "general" (a scan and GEMMs per layer, nsd_scan.hip).
    members: P = H / 32 workgroups per group (the partial-sum partition); default H / 32.
    rounding: False turns every rounding point off (then this is the fp64 model itself); rounding_off: names of single points.
    drop_lstm [L-1, B, T, D*H] multipliers {0, keep} of the inter-layer dropout (orc.dropout_mask), rrelu_slope / drop_head [B, F]
    (orc.rrelu_noise / orc.dropout_mask): the tensors the kernels' counter streams give; None = off / eval slope.
    Returns logits, probs, fc0_pre (for the RReLU-kink check) and, with labels, loss (mean CE) and grads (flat, float64)."""
    assert route in ("fused2", "general"), route
    assert route == "general" or (D == 1 and L == 2 and (C + 15) // 16 * 16 <= 64), "the fused route is two unidirectional layers, C <= 64"
    mut = set(mutants)
    assert not (mut - set(MUTANTS)), mut - set(MUTANTS)
    P = members if members is not None else H // 32
    assert H == 32 * P, (H, P)
    old_threads = torch.get_num_threads()
    if threads:
        torch.set_num_threads(threads)
    try:
        with torch.no_grad():
            return _run(params, x, labels, C, H, L, K, F, D, route, P, _Rounder(rounding, rounding_off), drop_lstm, rrelu_slope,
                        drop_head, mut)
    finally:
        torch.set_num_threads(old_threads)


def _run(params, x, labels, C, H, L, K, F, D, route, P, R, drop_lstm, rrelu_slope, drop_head, mut):
    f64 = torch.float64
    B, T, Cx = x.shape
    assert Cx == C and params.size == param_count(C, H, L, K, F, D)
    DH, G = D * H, 4 * H
    lo = param_layout(C, H, L, K, F, D)
    W = {k: torch.from_numpy(np.ascontiguousarray(params[o:o + int(np.prod(s))], np.float32).reshape(s)) for k, (o, s) in lo.items()}
    sfx = ("", "_reverse")
    train = labels is not None
    masked = drop_lstm is not None and L > 1
    if masked:
        mask = torch.from_numpy(np.ascontiguousarray(drop_lstm, np.float32)).permute(0, 2, 1, 3).to(f64)   # [L-1, T, B, DH]
        keep32 = float(np.float32(np.max(drop_lstm))) if np.any(drop_lstm) else 1.0
    cols = _gate_cols(H, P)

    def wb(name):                                   # a weight operand as the kernels hold it
        return R("w", W[name].to(f64))

    def bsum(l, d):                                 # b_ih + b_hh, fp32 on the device (seq_prep_kernel)
        return W[f"lstm.bias_ih_l{l}{sfx[d]}"].to(f64) + W[f"lstm.bias_hh_l{l}{sfx[d]}"].to(f64)

    xb = R("x", torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(f64).permute(1, 0, 2).contiguous())    # [T, B, C]

    # ------------------------------------------------------------------ forward
    def scan_fwd(gx, whh, reverse, init=None):
        """gx [T, B, 4H]: input term incl. bias (per step, fp64), whh [4H, H]: the recurrent weights as held.
        The running c is fp32 in the kernels (never rounded); h is rounded once (ring, hs) and that bf16 h is what every
        consumer reads."""
        h = torch.zeros(B, H, dtype=f64) if init is None else init[0]
        c = torch.zeros(B, H, dtype=f64) if init is None else init[1]
        hb_seq = torch.empty(T, B, H, dtype=f64)
        hraw = torch.empty(T, B, H, dtype=f64) if "lk_unrounded_h" in mut else None
        cs = [None] * T
        ga = [None] * T
        whh_t = whh.t().contiguous()
        for t in (range(T - 1, -1, -1) if reverse else range(T)):
            a = gx[t] + h @ whh_t
            i, f, g, o = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H]), torch.tanh(a[:, 2 * H:3 * H]), torch.sigmoid(a[:, 3 * H:])
            c = f * c + i * g                                                  # fp32 cell state (nsd_scan2.hip:274)
            hr = o * torch.tanh(c)
            h = R("h", hr)                                                     # nsd_scan2.hip:290-291
            hb_seq[t] = h
            if hraw is not None:
                hraw[t] = hr
            if train:
                cs[t] = R.store("c", c)                                        # nsd_scan2.hip:315
                ga[t] = R.store("gates", torch.cat([i, f, g, o], 1))           # nsd_scan2.hip:316-331
        return hb_seq, (torch.stack(cs) if train else None), (torch.stack(ga) if train else None), (h, c), hraw

    def linked(hb, l, hraw=None):
        """lk = bf16(bf16(h) * multiplier): the multiplier acts on the value the next layer reads (nsd_scan.hip:320-327)"""
        src = hraw if ("lk_unrounded_h" in mut and hraw is not None) else hb
        return R("lk", src * mask[l])

    layers = []                                      # per layer: dict(hb [T,B,DH], inp [T,B,I] (weight-gradient operand), cs, ga per d)
    if route == "fused2":
        # layer 0: W_ih0 . x_t rides in the scan, fp32 accumulation, no rounding of the projection (nsd_scan2.hip:221-227)
        gx0 = xb @ wb("lstm.weight_ih_l0").t() + bsum(0, 0)
        hb0, cs0, ga0, _, hraw0 = scan_fwd(gx0, wb("lstm.weight_hh_l0"), False)
        if masked:
            # the consumers rebuild h0 (x) m from keep bits; the scale keep sits in W_ih1, rounded once more (nsd_scan2.hip:58-65)
            w_ih1 = R("wscale", wb("lstm.weight_ih_l1") * keep32)
            in1 = hb0 * (mask[0] != 0).to(f64)
            lk0 = linked(hb0, 0, hraw0)                                        # row-major copy for dW_ih1 (nsd_scan2.hip:292-294)
        else:
            w_ih1, in1, lk0 = wb("lstm.weight_ih_l1"), hb0, hb0
        gx1 = in1 @ w_ih1.t() + bsum(1, 0)                                     # W_ih1 . in1 rides in the scan: not rounded
        hb1, cs1, ga1, _, _ = scan_fwd(gx1, wb("lstm.weight_hh_l1"), False)
        layers = [dict(hb=hb0, inp=xb, cs=[cs0], ga=[ga0]), dict(hb=hb1, inp=lk0, cs=[cs1], ga=[ga1])]
    else:
        inp = xb
        for l in range(L):
            hbs, css, gas, finals = [], [], [], []
            for d in range(D):
                w_ih = wb(f"lstm.weight_ih_l{l}{sfx[d]}")
                gx = inp @ w_ih.t() + bsum(l, d)
                if not (l == 0 and (C + 15) // 16 * 16 <= 64):
                    gx = R("xproj", gx)                                        # accumulator tiles + bias as bf16 (nsd_seq.h:19)
                init = None
                if d == 1 and "reverse_init" in mut:
                    init = finals[0]
                hb, cs_, ga_, fin, _ = scan_fwd(gx, wb(f"lstm.weight_hh_l{l}{sfx[d]}"), d == 1, init)
                hbs.append(hb); css.append(cs_); gas.append(ga_); finals.append(fin)
            hb = torch.cat(hbs, 2)
            layers.append(dict(hb=hb, inp=inp, cs=css, ga=gas))
            if l < L - 1:
                inp = linked(hb, l) if masked else hb
    top = layers[-1]["hb"]                                                     # [T, B, DH]: the head reads the bf16 top sequence

    # ------------------------------------------------------------------ head (no rounding point: fp32 on the bf16 sequence)
    hp = {k: W[k].to(f64).clone().requires_grad_(train) for k in ("ln.weight", "ln.bias", "attn.weight", "attn.bias",
                                                                     "fc.0.weight", "fc.0.bias", "fc.3.weight", "fc.3.bias")}
    with torch.enable_grad():
        top_l = top.permute(1, 0, 2).contiguous().requires_grad_(train)      # [B, T, DH]
        score = top_l @ hp["attn.weight"][0] + hp["attn.bias"][0]            # [B, T]
        if train:
            score.retain_grad()
        alpha = torch.softmax(score, 1)
        pooled = torch.einsum("bt,bth->bh", alpha, top_l)
        ln = torch.nn.functional.layer_norm(pooled, (DH,), hp["ln.weight"], hp["ln.bias"], 1e-5)
        pre = ln @ hp["fc.0.weight"].t() + hp["fc.0.bias"]
        slope = torch.from_numpy(np.ascontiguousarray(rrelu_slope, np.float32)).to(f64) if rrelu_slope is not None else RRELU_EVAL_SLOPE
        z = torch.where(pre >= 0, pre, pre * slope)
        if drop_head is not None:
            z = z * torch.from_numpy(np.ascontiguousarray(drop_head, np.float32)).to(f64)
        logits = z @ hp["fc.3.weight"].t() + hp["fc.3.bias"]
        out = dict(logits=logits.detach().numpy().copy(), probs=torch.softmax(logits, 1).detach().numpy().copy(),
                   fc0_pre=pre.detach().numpy().copy())
        if not train:
            return out
        lab = torch.from_numpy(np.asarray(labels, np.int64))
        loss = torch.nn.functional.cross_entropy(logits, lab)
        loss.backward()
    out["loss"] = float(loss.item())
    grads = np.zeros(param_count(C, H, L, K, F, D), np.float64)

    def put(name, v):
        o, s = lo[name]
        grads[o:o + int(np.prod(s))] = v.reshape(-1).numpy()

    for k, v in hp.items():
        put(k, v.grad)
    dtop = top_l.grad.permute(1, 0, 2).contiguous()                           # [T, B, DH] = alpha_t dpooled + dscore_t attn_w
    if "dscore_last" in mut:
        dtop[T - 1] -= score.grad[:, T - 1:T] * hp["attn.weight"][0].detach()

    # ------------------------------------------------------------------ backward (explicit BPTT)
    def psums(dab, w_t):
        """dh rows from da (bf16) through a [4H, N] weight: member q multiplies its own 128 gate columns, rounds its partial sum to
        bf16, and the consumer adds the P partials in fp32 in member order (nsd_scan2.hip:535-537, 628-633).  dab [..., 4H]."""
        sh = dab.shape[:-1]
        part = torch.einsum("nqk,qkj->qnj", dab.reshape(-1, G)[:, cols], w_t[cols])      # [P, n, N]
        if "psum_once" in mut:
            return R("psum", part.sum(0)).reshape(*sh, -1)
        return R("psum", part).sum(0).reshape(*sh, -1)

    def scan_bwd(dup, cs, ga, whh, reverse):
        """dup [T, B, H]: d(out) from above; cs / ga: the saved (bf16) c and gates.  Returns da as stored (bf16) [T, B, 4H] and the
        bias gradient, summed from the fp32 da (cell_apply, nsd_scan_common.h:264-275)."""
        dc = torch.zeros(B, H, dtype=f64)
        drec = torch.zeros(B, H, dtype=f64)
        dab_seq = torch.empty(T, B, G, dtype=torch.bfloat16 if R.on["da"] else f64)
        dbias = torch.zeros(G, dtype=f64)
        stale = None
        whh_t = whh                                  # [4H, H]: dh = da . W_hh
        sq = P - 1                                   # the stale member of the mutant
        order = range(T) if reverse else range(T - 1, -1, -1)
        first_t = T - 1 if reverse else 0            # first step in forward time: c_{t-1} = 0
        for t in order:
            gts = ga[t].to(f64)
            i, f, g, o = gts[:, :H], gts[:, H:2 * H], gts[:, 2 * H:3 * H], gts[:, 3 * H:]
            cb = cs[t].to(f64)
            if t == first_t:
                cp = cb if "forget_c_edge" in mut else torch.zeros_like(cb)
            else:
                cp = cs[t + 1 if reverse else t - 1].to(f64)
            tc = torch.tanh(cb)
            dh = dup[t] + drec
            dct = dh * o * (1 - tc * tc) + dc
            dc = dct * f
            da = torch.cat([dct * g * i * (1 - i), dct * cp * f * (1 - f), dct * i * (1 - g * g), dh * tc * o * (1 - o)], 1)
            dbias += da.sum(0)
            dab = R("da", da)
            dab_seq[t] = dab
            if "stale_member" in mut and P > 1:
                part = torch.einsum("nqk,qkj->qnj", dab[:, cols], whh_t[cols])
                cur = part.clone()
                if stale is not None:
                    part[sq] = stale
                else:
                    part[sq] = 0
                stale = cur[sq]
                drec = R("psum", part).sum(0)
            else:
                drec = psums(dab, whh_t)
        return dab_seq, dbias

    def wgrad(dab_seq, opnd, shift):
        """sum over (t, b) of da_t^T . opnd_{t + shift} (0 outside the tile's steps): bf16 operands, fp32 accumulation"""
        acc = torch.zeros(G, opnd.shape[-1], dtype=f64)
        for t0 in range(0, T, 64):
            t1 = min(T, t0 + 64)
            a = dab_seq[t0:t1].to(f64)
            idx = torch.arange(t0, t1) + shift
            ok = (idx >= 0) & (idx < T)
            if "dwhh_first_step" in mut and shift != 0:
                idx = idx % T
                ok = torch.ones_like(ok)
            b = torch.zeros(t1 - t0, B, opnd.shape[-1], dtype=f64)
            b[ok] = opnd[idx[ok]].to(f64)
            acc += a.reshape(-1, G).t() @ b.reshape(-1, opnd.shape[-1])
        return acc

    def m_of(l):                                     # the multipliers behind layer l, as the saved keep bits give them
        m = mask[l].clone()
        if "keep_bit_lost" in mut:
            m[..., 0] = 0.0
        return m

    if route == "fused2":
        L1, L0 = layers[1], layers[0]
        da1, db1 = scan_bwd(dtop, L1["cs"][0], L1["ga"][0], wb("lstm.weight_hh_l1"), False)
        # layer 0's upstream gradient: W_ih1^T da1 as per-member bf16 partial sums, times the multiplier (nsd_scan2.hip:545-547)
        dinx = psums(da1.to(f64), wb("lstm.weight_ih_l1"))
        dup0 = dinx * m_of(0) if masked else dinx
        da0, db0 = scan_bwd(dup0, L0["cs"][0], L0["ga"][0], wb("lstm.weight_hh_l0"), False)
        for l, (da, db, lay) in enumerate(((da0, db0, L0), (da1, db1, L1))):
            put(f"lstm.weight_hh_l{l}", wgrad(da, lay["hb"], -1))
            put(f"lstm.weight_ih_l{l}", wgrad(da, lay["inp"], 0)[:, :lay["inp"].shape[-1]])
            put(f"lstm.bias_ih_l{l}", db)
            put(f"lstm.bias_hh_l{l}", db)
        return dict(out, grads=grads)

    dout = dtop
    for l in range(L - 1, -1, -1):
        lay = layers[l]
        das = []
        for d in range(D):
            da, db = scan_bwd(dout[..., d * H:(d + 1) * H], lay["cs"][d], lay["ga"][d], wb(f"lstm.weight_hh_l{l}{sfx[d]}"), d == 1)
            das.append(da)
            put(f"lstm.weight_hh_l{l}{sfx[d]}", wgrad(da, lay["hb"][..., d * H:(d + 1) * H], -1 if d == 0 else 1))
            put(f"lstm.weight_ih_l{l}{sfx[d]}", wgrad(da, lay["inp"], 0))
            put(f"lstm.bias_ih_l{l}{sfx[d]}", db)
            put(f"lstm.bias_hh_l{l}{sfx[d]}", db)
        if l > 0:
            # d in = da . W_ih over both directions in ONE contraction, fp32 accumulation, stored as bf16 tiles (nsd_seq.hip:419-425)
            w_ih = torch.cat([wb(f"lstm.weight_ih_l{l}{sfx[d]}") for d in range(D)], 0)      # [D*4H, DH]
            din = torch.empty(T, B, DH, dtype=f64)
            for t in range(T):
                din[t] = R("din", torch.cat([da[t].to(f64) for da in das], 1) @ w_ih)
            dout = din * m_of(l - 1) if masked else din
    return dict(out, grads=grads)


def rel_errors(got: np.ndarray, ref: np.ndarray, C, H, L, K, F=32, D=1) -> Dict[str, float]:
    """per tensor: max |got - ref| / max |ref|"""
    g, r = unflatten(got, C, H, L, K, F, D), unflatten(ref, C, H, L, K, F, D)
    return {k: float(np.abs(g[k] - r[k]).max() / max(np.abs(r[k]).max(), 1e-30)) for k in g}


def kink_margin(fc0_pre: np.ndarray) -> float:
    """smallest |fc.0 pre-activation|: a value closer to 0 than the path's error may take the other RReLU slope"""
    return float(np.abs(fc0_pre).min()) if fc0_pre.size else math.inf
