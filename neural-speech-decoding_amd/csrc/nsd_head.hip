// nsd_head.hip -- attention pooling over time + LayerNorm + dense head (+ softmax / CE), forward and backward.
//
// Replaces lines 35-39 of EEG_LSTM.forward (Neuro-Alpha-App/Utilities/lstm_eeg_model.py):
//   scores = attn(out).squeeze(-1); weights = softmax(scores, dim=1); out = (out*weights[...,None]).sum(1)
//   out = ln(out); return fc(out)          fc = Linear(H,F) -> RReLU -> Dropout -> Linear(F,K)
// and the class softmax of SimplePredictor.predict (lstm_eeg_model.py:97).
//
// One 256-thread workgroup per trial (grid-strided over trials).  The [T,H] sequence of a trial (48 KB at
// T=250,H=48) is read twice per pass (scores, weighted sum); rows are contiguous so every wave reads whole
// 128-B lines.  Reductions over T / H use wave shuffles + one LDS hop.  Shape-generic in T,H,F,K.
//
// Three kernels -- head_fwd_kernel, head_bwd_kernel and the fused head_train_kernel -- are assembled from ONE set of
// phases (stage_seq .. attn_bwd below).  A phase takes plain pointers and sizes and does not know its caller: the
// parameters it reads are in global memory for the first two kernels and in head_train_kernel's LDS copy for the third,
// the sequence is staged or in place.  Every floating-point expression is written once, so the three kernels agree
// bit for bit wherever they compute the same quantity.  One phase has a second form, for head_train_kernel's time: the
// attention backward of the kernel that holds alpha in LDS (attn_bwd_resident).
#include "nsd_args.h"

#define HEAD_NT 256

__device__ __forceinline__ float block_sum(float v, float *red) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}
__device__ __forceinline__ float block_max(float v, float *red) {
    v = wave_max(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// dynamic LDS layout (floats): sc[T] | vecH[4][H] | vecF[2][F] | vecK[K] | part[max(H,256)... see below] | red[8]
__device__ __forceinline__ void weighted_rowsum(const float *seq, int rs, const float *w_t, int T, int H, float *part,
                                                float *out /*LDS [H]*/) {
    // out[j] = sum_t w_t[t] * seq[t][j].  Lanes run along j (coalesced rows), parts run along t.
    const int HL = H < HEAD_NT ? H : HEAD_NT;
    const int nparts = HEAD_NT / HL;
    const int lane_j = threadIdx.x % HL, p = threadIdx.x / HL;
    for (int j0 = 0; j0 < H; j0 += HL) {
        const int j = j0 + lane_j;
        float acc = 0.f;
        if (p < nparts && j < H)
            for (int t = p; t < T; t += nparts) acc = fmaf(w_t[t], seq[(size_t)t * rs + j], acc);
        __syncthreads();
        if (p < nparts) part[p * HL + lane_j] = acc;
        __syncthreads();
        if (threadIdx.x < HL && j0 + threadIdx.x < H) {
            float s = 0.f;
            for (int q = 0; q < nparts; ++q) s += part[q * HL + threadIdx.x];
            out[j0 + threadIdx.x] = s;
        }
    }
    __syncthreads();
}

// a trial's gradient slab: the eight vectors of the head at the offsets o_* of HeadArgs
struct HeadGrad { float *ln_w, *ln_b, *attn_w, *attn_b, *fc0_w, *fc0_b, *fc3_w, *fc3_b; };
__device__ __forceinline__ HeadGrad slab_of(const HeadArgs &a, int b) {
    float *s = a.hslabs + (size_t)b * a.Ph;
    return {s + a.o_ln_w, s + a.o_ln_b, s + a.o_attn_w, s + a.o_attn_b, s + a.o_fc0_w, s + a.o_fc0_b, s + a.o_fc3_w, s + a.o_fc3_b};
}
// row b of an optional [B, n] array
template <class P>
__device__ __forceinline__ P *row_of(P *p, int b, int n) { return p ? p + (size_t)b * n : nullptr; }

// ---------------------------------------------------------------------------------------------
// the phases.  Loops over t, j, f, k give element e to thread e % HEAD_NT, in every phase.
// ---------------------------------------------------------------------------------------------
// a trial's [T,H] sequence -> LDS rows of stride rs with 16-byte loads (H % 4 == 0; rows padded so that a lane-per-row
// ds_read_b128 sweep is bank-conflict free).  The caller's barrier publishes it.
__device__ __forceinline__ void stage_seq(const float *gseq, float *sseq, int T, int H, int rs) {
    const int h4 = H >> 2;
    for (int e = threadIdx.x; e < T * h4; e += HEAD_NT) {
        const int t = e / h4, q = e - t * h4;
        *reinterpret_cast<float4 *>(sseq + (size_t)t * rs + 4 * q) = *reinterpret_cast<const float4 *>(gseq + (size_t)t * H + 4 * q);
    }
}

// init + row . v, the terms added in the order of j (16-byte loads of the row when H % 4 == 0: the same sums)
__device__ __forceinline__ float row_dot(const float *row, const float *v, int H, float init) {
    float s = init;
    if ((H & 3) == 0) {
        for (int j = 0; j < H; j += 4) {
            const float4 r = *reinterpret_cast<const float4 *>(row + j);
            s = fmaf(r.x, v[j], s); s = fmaf(r.y, v[j + 1], s);
            s = fmaf(r.z, v[j + 2], s); s = fmaf(r.w, v[j + 3], s);
        }
    } else {
        for (int j = 0; j < H; ++j) s = fmaf(row[j], v[j], s);
    }
    return s;
}

// attention forward (lstm_eeg_model.py:35-37): scores, softmax over TIME, weighted sum.  sc[t] = alpha_t (also to
// alpha_out when it is not null), pooled[j] = sum_t alpha_t seq[t][j]
__device__ __forceinline__ void attn_fwd(const float *seq, int rs, int T, int H, const float *aw, float ab, float *sc, float *alpha_out,
                                         float *part, float *red, float *pooled) {
    const int tid = threadIdx.x;
    float lmax = -INFINITY;
    for (int t = tid; t < T; t += HEAD_NT) {
        const float s = row_dot(seq + (size_t)t * rs, aw, H, ab);
        sc[t] = s;
        lmax = fmaxf(lmax, s);
    }
    const float mx = block_max(lmax, red);
    float lsum = 0.f;
    for (int t = tid; t < T; t += HEAD_NT) { const float e = __expf(sc[t] - mx); sc[t] = e; lsum += e; }
    const float den = block_sum(lsum, red);
    const float rden = 1.0f / den;
    for (int t = tid; t < T; t += HEAD_NT) {
        const float al = sc[t] * rden;
        sc[t] = al;
        if (alpha_out) alpha_out[t] = al;
    }
    __syncthreads();
    weighted_rowsum(seq, rs, sc, T, H, part, pooled);
}

// LayerNorm forward (lstm_eeg_model.py:38) of x[H]: biased variance, eps inside the sqrt.  out = xhat * w + bias, xhat is kept
// when asked for; returns 1 / std.  A thread reads x[j] of its own j only.
__device__ __forceinline__ float ln_fwd(const float *x, const float *w, const float *bias, int H, float *red, float *xhat, float *out) {
    const int tid = threadIdx.x;
    float ls = 0.f;
    for (int j = tid; j < H; j += HEAD_NT) ls += x[j];
    const float mu = block_sum(ls, red) / (float)H;
    float lv = 0.f;
    for (int j = tid; j < H; j += HEAD_NT) { const float d = x[j] - mu; lv += d * d; }
    const float var = block_sum(lv, red) / (float)H;
    const float rstd = 1.0f / sqrtf(var + 1e-5f);
    for (int j = tid; j < H; j += HEAD_NT) {
        const float xh = (x[j] - mu) * rstd;
        if (xhat) xhat[j] = xh;
        out[j] = xh * w[j] + bias[j];
    }
    return rstd;
}

// RReLU with the unit's slope, then its dropout multiplier (lstm_eeg_model.py:27-28)
__device__ __forceinline__ float rrelu_drop(float pre, float sl, float mk) { return (pre >= 0.f ? pre : pre * sl) * mk; }

// (the dot products of the dense phases ask for the unrolling by 8 that hipcc gives such a loop unasked where no loop over units
// surrounds it)
// dense forward (lstm_eeg_model.py:26-29) of ln[H]: fc.0 (pre-activation also to pre_lds / pre_out when not null) -> RReLU ->
// dropout = z[F], fc.3 = lg[K] (also to logits_out), and the class softmax (lstm_eeg_model.py:97) to probs_out when not null.
// slope / mask: the trial's rows, or null for eval_slope / no dropout.
__device__ __forceinline__ void dense_fwd(const float *w0, const float *b0, const float *w3, const float *b3, const float *ln,
                                          const float *slope, float eval_slope, const float *mask, int H, int F, int K,
                                          float *pre_lds, float *pre_out, float *z, float *lg, float *logits_out, float *probs_out) {
    const int tid = threadIdx.x;
    for (int f = tid; f < F; f += HEAD_NT) {
        float acc = b0[f];
        const float *w = w0 + (size_t)f * H;
#pragma unroll 8
        for (int j = 0; j < H; ++j) acc = fmaf(w[j], ln[j], acc);
        if (pre_lds) pre_lds[f] = acc;
        if (pre_out) pre_out[f] = acc;
        z[f] = rrelu_drop(acc, slope ? slope[f] : eval_slope, mask ? mask[f] : 1.f);
    }
    __syncthreads();
    for (int k = tid; k < K; k += HEAD_NT) {
        float acc = b3[k];
        const float *w = w3 + (size_t)k * F;
#pragma unroll 8
        for (int f = 0; f < F; ++f) acc = fmaf(w[f], z[f], acc);
        lg[k] = acc;
        logits_out[k] = acc;
    }
    __syncthreads();
    if (probs_out && tid == 0) {
        float m2 = lg[0];
        for (int k = 1; k < K; ++k) m2 = fmaxf(m2, lg[k]);
        float d = 0.f;
        for (int k = 0; k < K; ++k) d += __expf(lg[k] - m2);
        for (int k = 0; k < K; ++k) probs_out[k] = __expf(lg[k] - m2) / d;
    }
}

// dense backward from dl[K] (published by the caller's barrier, as are z and ln): dz[F] through fc.3 / dropout / RReLU, and
// d fc.0.bias, d fc.3.weight, d fc.3.bias, d fc.0.weight into the slab
__device__ __forceinline__ void dense_bwd(const float *w3, const float *pre, const float *slope, float eval_slope, const float *mask,
                                          const float *dl, const float *z, const float *ln, int H, int F, int K, float *dz,
                                          const HeadGrad &g) {
    const int tid = threadIdx.x;
    for (int f = tid; f < F; f += HEAD_NT) {
        float d = 0.f;
#pragma unroll 8
        for (int k = 0; k < K; ++k) d = fmaf(w3[(size_t)k * F + f], dl[k], d);
        if (mask) d *= mask[f];
        d = pre[f] >= 0.f ? d : d * (slope ? slope[f] : eval_slope);
        dz[f] = d;
        g.fc0_b[f] = d;
    }
    for (int e = tid; e < K * F; e += HEAD_NT) g.fc3_w[e] = dl[e / F] * z[e % F];
    for (int k = tid; k < K; k += HEAD_NT) g.fc3_b[k] = dl[k];
    __syncthreads();
    for (int e = tid; e < F * H; e += HEAD_NT) g.fc0_w[e] = dz[e / H] * ln[e % H];
}

// d ln_out = fc.0.weight^T dz, d ln.weight and d ln.bias into the slab, and the LayerNorm backward: dp[H] = d pooled (also to dpooled_out)
__device__ __forceinline__ void ln_bwd(const float *w0, const float *lnw, const float *dz, const float *xhat, float rstd, int H, int F,
                                       float *red, float *dp, const HeadGrad &g, float *dpooled_out) {
    const int tid = threadIdx.x;
    float l1 = 0.f, l2 = 0.f;
    for (int j = tid; j < H; j += HEAD_NT) {
        float d = 0.f;
        for (int f = 0; f < F; ++f) d = fmaf(w0[(size_t)f * H + j], dz[f], d);
        g.ln_w[j] = d * xhat[j];
        g.ln_b[j] = d;
        const float dxh = d * lnw[j];
        dp[j] = dxh;
        l1 += dxh; l2 += dxh * xhat[j];
    }
    const float m1 = block_sum(l1, red) / (float)H;
    const float m2 = block_sum(l2, red) / (float)H;
    for (int j = tid; j < H; j += HEAD_NT) {
        const float d = rstd * (dp[j] - m1 - xhat[j] * m2);
        dp[j] = d;
        dpooled_out[j] = d;
    }
    __syncthreads();
}

// the end of the attention backward, from sc[t] = dscore_t and the thread's sum lb of them: d attn.bias = sum_t dscore_t,
// d attn.weight[j] = sum_t dscore_t seq[t][j] (through tmp[H], free LDS)
__device__ __forceinline__ void attn_bwd_params(const float *seq, int rs, int T, int H, const float *sc, float lb, float *part, float *red,
                                                float *tmp, const HeadGrad &g) {
    const int tid = threadIdx.x;
    const float dab = block_sum(lb, red);
    if (tid == 0) g.attn_b[0] = dab;
    weighted_rowsum(seq, rs, sc, T, H, part, tmp);
    for (int j = tid; j < H; j += HEAD_NT) g.attn_w[j] = tmp[j];
    __syncthreads();
}

// attention backward: dalpha_t = dp . seq_t ; dscore_t = alpha_t (dalpha_t - sum_s alpha_s dalpha_s), to dscore_out and as
// {alpha, dscore, 0, 0} records to adpack_out when not null; d attn.bias = sum_t dscore_t, d attn.weight[j] = sum_t dscore_t seq[t][j].
// alpha: the trial's row as the forward wrote it (the thread that reads alpha[t] here is the one that wrote it there);
// sc[T] holds dalpha, then dscore; tmp[H] is free LDS.
__device__ __forceinline__ void attn_bwd(const float *seq, int rs, int T, int H, const float *alpha, const float *dp, float *sc,
                                         float *part, float *red, float *tmp, float *dscore_out, float *adpack_out, const HeadGrad &g) {
    const int tid = threadIdx.x;
    float lsd = 0.f;
    for (int t = tid; t < T; t += HEAD_NT) {
        const float al = alpha[t];
        const float d = row_dot(seq + (size_t)t * rs, dp, H, 0.f);
        sc[t] = d;
        lsd = fmaf(al, d, lsd);
    }
    const float sdot = block_sum(lsd, red);
    float lb = 0.f;
    for (int t = tid; t < T; t += HEAD_NT) {
        const float al = alpha[t];
        const float ds = al * (sc[t] - sdot);
        sc[t] = ds;
        dscore_out[t] = ds;
        if (adpack_out) *reinterpret_cast<float4 *>(adpack_out + (size_t)t * 4) = make_float4(al, ds, 0.f, 0.f);
        lb += ds;
    }
    attn_bwd_params(seq, rs, T, H, sc, lb, part, red, tmp, g);
}
// the same with alpha_t in sc[] and dalpha_t in up to four registers per thread (T <= 4 * HEAD_NT), for the kernel that has
// just formed alpha: no way back to memory for it.  Same sums, same bits.
__device__ __forceinline__ void attn_bwd_resident(const float *seq, int rs, int T, int H, const float *dp, float *sc, float *part,
                                                  float *red, float *tmp, float *dscore_out, float *adpack_out, const HeadGrad &g) {
    const int tid = threadIdx.x;
    float lsd = 0.f;
    float dal[4];
    int nt = 0;
    for (int t = tid; t < T; t += HEAD_NT, ++nt) {
        const float d = row_dot(seq + (size_t)t * rs, dp, H, 0.f);
        if (nt < 4) dal[nt] = d;
        lsd = fmaf(sc[t], d, lsd);
    }
    const float sdot = block_sum(lsd, red);
    float lb = 0.f;
    nt = 0;
    for (int t = tid; t < T; t += HEAD_NT, ++nt) {
        const float al = sc[t];
        const float ds = al * (dal[nt < 4 ? nt : 3] - sdot);
        sc[t] = ds;
        dscore_out[t] = ds;
        *reinterpret_cast<float4 *>(adpack_out + (size_t)t * 4) = make_float4(al, ds, 0.f, 0.f);
        lb += ds;
    }
    attn_bwd_params(seq, rs, T, H, sc, lb, part, red, tmp, g);
}

// ---------------------------------------------------------------------------------------------
// the kernels.  Dynamic LDS (floats): [T][stage_stride] staged sequence (16-byte aligned; empty when not staging), then the
// vectors each kernel names below.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HEAD_NT) void head_fwd_kernel(HeadArgs a) {
    extern __shared__ __align__(16) float lds[];
    const int T = a.T, H = a.H, F = a.F, K = a.K;
    float *sseq = lds;
    float *sc = lds + (size_t)T * a.stage_stride;   // [T]
    float *vaw = sc + T;              // [H] attn weights
    float *vp = vaw + H;              // [H] pooled
    float *vln = vp + H;              // [H] ln out
    float *vz = vln + H;              // [F]
    float *vlg = vz + F;              // [K]
    float *part = vlg + K;            // [256]
    float *red = part + HEAD_NT;      // [8]
    const int tid = threadIdx.x;

    for (int j = tid; j < H; j += HEAD_NT) vaw[j] = a.attn_w[j];
    const float ab = a.attn_b[0];
    __syncthreads();

    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const float *seq = a.top + (size_t)b * T * H;
        int rs = H;
        if (a.stage_stride) {
            stage_seq(seq, sseq, T, H, a.stage_stride);
            __syncthreads();
            seq = sseq; rs = a.stage_stride;
        }
        attn_fwd(seq, rs, T, H, vaw, ab, sc, row_of(a.alpha, b, T), part, red, vp);
        if (a.pooled)
            for (int j = tid; j < H; j += HEAD_NT) a.pooled[(size_t)b * H + j] = vp[j];
        ln_fwd(vp, a.ln_w, a.ln_b, H, red, nullptr, vln);
        __syncthreads();
        dense_fwd(a.fc0_w, a.fc0_b, a.fc3_w, a.fc3_b, vln, row_of(a.rrelu_slope, b, F), a.eval_slope, row_of(a.drop_head, b, F), H, F, K, nullptr, row_of(a.fc0_pre, b, F), vz, vlg, a.logits + (size_t)b * K, row_of(a.probs, b, K));
        __syncthreads();
    }
}

__global__ __launch_bounds__(HEAD_NT) void head_bwd_kernel(HeadArgs a) {
    extern __shared__ __align__(16) float lds[];
    const int T = a.T, H = a.H, F = a.F, K = a.K;
    float *sseq = lds;
    float *sc = lds + (size_t)T * a.stage_stride;   // [T]  d alpha, later dscore
    float *vx = sc + T + H;           // [H] xhat, behind an [H] slot that is no longer used (nsd_head_launch sizes four)
    float *vln = vx + H;              // [H] ln out
    float *vdp = vln + H;             // [H] d pooled
    float *vz = vdp + H;              // [F] activated fc0 output
    float *vdz = vz + F;              // [F]
    float *vdl = vdz + F;             // [K]
    float *part = vdl + K;            // [256]
    float *red = part + HEAD_NT;      // [8]
    const int tid = threadIdx.x;

    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const float *seq = a.top + (size_t)b * T * H;
        int rs = H;
        if (a.stage_stride) {
            stage_seq(seq, sseq, T, H, a.stage_stride);
            __syncthreads();
            seq = sseq; rs = a.stage_stride;
        }
        const HeadGrad g = slab_of(a, b);
        // dlogits: given, or those of the mean CE against soft targets / labels
        if (tid == 0) {
            if (a.dlogits) {
                for (int k = 0; k < K; ++k) vdl[k] = a.dlogits[(size_t)b * K + k];
            } else {
                const float *lg = a.logits_in + (size_t)b * K;
                const float ls = a.targets ? soft_ce_thread(a.targets + (size_t)b * K, lg, K, a.scale, vdl)
                                           : hard_ce_thread(a.labels[b], lg, K, a.scale, vdl);
                if (a.loss) a.loss[b] = ls;
            }
        }
        // LayerNorm again from the saved pooled vector, and the activated fc.0 output from its saved pre-activation
        for (int j = tid; j < H; j += HEAD_NT) vdp[j] = a.pooled[(size_t)b * H + j];
        const float rstd = ln_fwd(vdp, a.ln_w, a.ln_b, H, red, vx, vln);
        const float *pre = a.fc0_pre + (size_t)b * F, *slope = row_of(a.rrelu_slope, b, F), *mask = row_of(a.drop_head, b, F);
        for (int f = tid; f < F; f += HEAD_NT) vz[f] = rrelu_drop(pre[f], slope ? slope[f] : a.eval_slope, mask ? mask[f] : 1.f);
        __syncthreads();
        dense_bwd(a.fc3_w, pre, slope, a.eval_slope, mask, vdl, vz, vln, H, F, K, vdz, g);
        ln_bwd(a.fc0_w, a.ln_w, vdz, vx, rstd, H, F, red, vdp, g, a.dpooled + (size_t)b * H);
        attn_bwd(seq, rs, T, H, a.alpha + (size_t)b * T, vdp, sc, part, red, vx, a.dscore + (size_t)b * T, row_of(a.adpack, b, 4 * T), g);
    }
}

// ---------------------------------------------------------------------------------------------
// Fused train-step head: forward, mean-CE and backward of one trial in ONE pass of one workgroup.
// Everything lives in LDS: the trial's [T,H] sequence (read from HBM exactly once), the head's
// parameters (staged once per workgroup), and every intermediate.  The only HBM latencies left on
// the kernel's critical path are those two staging loads.
// ---------------------------------------------------------------------------------------------
// (bounded to four waves per SIMD, the occupancy the kernel had before its phases were shared: with all of them inlined hipcc took
// 132 VGPRs, one resident workgroup per CU less)
__global__ __launch_bounds__(HEAD_NT, 4) void head_train_kernel(HeadArgs a) {
    extern __shared__ __align__(16) float lds[];
    const int T = a.T, H = a.H, F = a.F, K = a.K, rs = a.stage_stride;
    float *sseq = lds;                                   // [T][rs]
    float *hp = sseq + (size_t)T * rs;                   // [Ph] parameters, same offsets as a head slab
    float *sc = hp + ((a.Ph + 3) & ~3L);                 // [T]
    float *vp = sc + T;                                  // [H] pooled
    float *vx = vp + H;                                  // [H] xhat
    float *vln = vx + H;                                 // [H] LayerNorm output
    float *vdp = vln + H;                                // [H] d pooled
    float *vpre = vdp + H;                               // [F] fc.0 pre-activation
    float *vz = vpre + F;                                // [F] activated
    float *vdz = vz + F;                                 // [F]
    float *vlg = vdz + F;                                // [K]
    float *vdl = vlg + K;                                // [K]
    float *part = vdl + K;                               // [256]
    float *red = part + HEAD_NT;                         // [8]
    const int tid = threadIdx.x;
    const float *p_lnw = hp + a.o_ln_w, *p_lnb = hp + a.o_ln_b, *p_aw = hp + a.o_attn_w;
    const float *p_w0 = hp + a.o_fc0_w, *p_b0 = hp + a.o_fc0_b, *p_w3 = hp + a.o_fc3_w, *p_b3 = hp + a.o_fc3_b;

    for (long e = tid; e < a.Ph; e += HEAD_NT) hp[e] = a.ln_w[e];     // head parameters are contiguous from ln.weight on
    __syncthreads();
    const float ab = hp[a.o_attn_b];

    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        stage_seq(a.top + (size_t)b * T * H, sseq, T, H, rs);
        const HeadGrad g = slab_of(a, b);
        const float *slope = row_of(a.rrelu_slope, b, F), *mask = row_of(a.drop_head, b, F);
        // per-trial small inputs, fetched while the sequence lands
        float sl_f = a.eval_slope, mk_f = 1.f;
        if (tid < F) {
            if (slope) sl_f = slope[tid];
            if (mask) mk_f = mask[tid];
        }
        const int label = a.targets ? 0 : a.labels[b];
        __syncthreads();
        // ---- forward ----
        attn_fwd(sseq, rs, T, H, p_aw, ab, sc, a.alpha + (size_t)b * T, part, red, vp);
        // LayerNorm and dense forward stay written out here (one unit per thread, F <= HEAD_NT; slope and multiplier from registers):
        // through ln_fwd / dense_fwd this kernel took 21.6 us for 19.4 us at H = 32 and 32.5 for 29.6 at H = 64 (profiles/head_phases.md)
        float ls = 0.f;
        for (int j = tid; j < H; j += HEAD_NT) { ls += vp[j]; a.pooled[(size_t)b * H + j] = vp[j]; }
        const float mu = block_sum(ls, red) / (float)H;
        float lv = 0.f;
        for (int j = tid; j < H; j += HEAD_NT) { const float d = vp[j] - mu; lv += d * d; }
        const float rstd = 1.0f / sqrtf(block_sum(lv, red) / (float)H + 1e-5f);
        for (int j = tid; j < H; j += HEAD_NT) { const float xh = (vp[j] - mu) * rstd; vx[j] = xh; vln[j] = xh * p_lnw[j] + p_lnb[j]; }
        __syncthreads();
        if (tid < F) {
            float acc = p_b0[tid];
            const float *w = p_w0 + (size_t)tid * H;
            for (int j = 0; j < H; ++j) acc = fmaf(w[j], vln[j], acc);
            vpre[tid] = acc;
            a.fc0_pre[(size_t)b * F + tid] = acc;
            vz[tid] = rrelu_drop(acc, sl_f, mk_f);
        }
        __syncthreads();
        if (tid < K) {
            float acc = p_b3[tid];
            for (int f = 0; f < F; ++f) acc = fmaf(p_w3[(size_t)tid * F + f], vz[f], acc);
            vlg[tid] = acc;
            a.logits[(size_t)b * K + tid] = acc;
        }
        __syncthreads();
        // ---- mean cross-entropy: dlogits = (softmax - onehot) * scale, or its soft-target form ----
        if (tid == 0)
            a.loss[b] = a.targets ? soft_ce_thread(a.targets + (size_t)b * K, vlg, K, a.scale, vdl) : hard_ce_thread(label, vlg, K, a.scale, vdl);
        __syncthreads();
        // ---- backward ----
        dense_bwd(p_w3, vpre, slope, a.eval_slope, mask, vdl, vz, vln, H, F, K, vdz, g);
        ln_bwd(p_w0, p_lnw, vdz, vx, rstd, H, F, red, vdp, g, a.dpooled + (size_t)b * H);
        attn_bwd_resident(sseq, rs, T, H, vdp, sc, part, red, vx, a.dscore + (size_t)b * T, a.adpack + (size_t)b * T * 4, g);
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// LDS bytes of a launch with `vec` floats of vectors: when H % 4 == 0 and both stay within stage_max bytes, the trial's sequence
// goes in front of them in rows of *stride floats (H rounded up to 4 (mod 8)); otherwise *stride = 0 and the vectors are alone.
static size_t head_lds_plan(const HeadArgs &a, size_t vec, size_t stage_max, int *stride) {
    size_t lds = vec * sizeof(float);
    *stride = 0;
    if ((a.H & 3) == 0) {
        int s = a.H + 4;
        if (((s >> 2) & 1) == 0) s += 4;
        const size_t need = lds + (size_t)a.T * s * sizeof(float);
        if (need <= stage_max) { *stride = s; lds = need; }
    }
    return lds;
}
// a launch with more dynamic LDS than the default 64 KB lifts the kernel's limit first
static void head_lds_allow(const void *kernel, size_t lds) {
    if (lds > 64 * 1024) (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

// the fused head is used when everything fits in LDS (<= 150 KB) and T <= 4*256
// returns 1 if launched, 0 if the shape does not fit (caller falls back to head_fwd + head_bwd), <0 on error
int nsd_head_train_launch(const HeadArgs &a_in, hipStream_t st) {
    HeadArgs a = a_in;
    if (a.T > 4 * HEAD_NT || a.F > HEAD_NT || a.K > HEAD_NT) return 0;
    const size_t vec = ((a.Ph + 3) & ~3L) + a.T + 4 * (size_t)a.H + 3 * (size_t)a.F + 2 * (size_t)a.K + HEAD_NT + 8;
    const size_t lds = head_lds_plan(a, vec, 150 * 1024, &a.stage_stride);
    if (!a.stage_stride) return 0;
    if (a.B <= 0) return 1;
    const int cap = 8 * nsd_num_cus();
    head_lds_allow((const void *)head_train_kernel, lds);
    hipLaunchKernelGGL(head_train_kernel, dim3(a.B < cap ? a.B : cap), dim3(HEAD_NT), lds, st, a);
    NSD_CHECK_LAUNCH("head_train");
    return 1;
}

int nsd_head_launch(const HeadArgs &a_in, bool bwd, hipStream_t st) {
    HeadArgs a = a_in;
    if (a.B <= 0) return NSD_OK;
    // the sequence is staged when it fits next to the small vectors (<= 144 KB); the backward's fourth [H] is no longer used
    const size_t vec = (size_t)a.T + (bwd ? 4 : 3) * (size_t)a.H + (bwd ? 2 : 1) * (size_t)a.F + a.K + HEAD_NT + 8;
    const size_t lds = head_lds_plan(a, vec, 144 * 1024, &a.stage_stride);
    if (lds > 160 * 1024 || a.H > HEAD_NT * 8) {
        nsd_set_error("head: T=%d H=%d needs %zu B of LDS (max 163840)", a.T, a.H, lds);
        return NSD_E_INVALID;
    }
    const int cap = 8 * nsd_num_cus();
    const int grid = a.B < cap ? a.B : cap;
    head_lds_allow(bwd ? (const void *)head_bwd_kernel : (const void *)head_fwd_kernel, lds);
    if (bwd) hipLaunchKernelGGL(head_bwd_kernel, dim3(grid), dim3(HEAD_NT), lds, st, a);
    else hipLaunchKernelGGL(head_fwd_kernel, dim3(grid), dim3(HEAD_NT), lds, st, a);
    NSD_CHECK_LAUNCH(bwd ? "head_bwd" : "head_fwd");
    return NSD_OK;
}
