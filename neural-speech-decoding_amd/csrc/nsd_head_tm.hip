// nsd_head_tm.hip -- attention pooling over time, LayerNorm and the dense head (Neuro-Alpha-App/Utilities/lstm_eeg_model.py:35-39,
// class softmax :97) on the TIME-MAJOR bf16 sequence the scan kernels leave: top[t][b][DH], DH = D*H.
//
// One wave per trial, 4 trials per workgroup, no LDS: lane l owns the DH/64 adjacent columns l*VPL.. of the sequence.
//   pass 1  online softmax over t: running max / denominator / weighted sum (the sequence is read once); the raw scores go
//           to alpha[] when training
//   dense   LayerNorm (biased variance, eps 1e-5), fc.0, RReLU (eval slope, explicit slopes or the counter stream), dropout,
//           fc.3, softmax / mean cross-entropy; lane f holds fc.0 unit f, lane k class k
//   train   dense backward in the same wave -> dpooled; alpha_t = exp(s_t - m) / l; pass 2 over t:
//           dscore_t = alpha_t (dpooled . h_t - dpooled . pooled)   (sum_s alpha_s dpooled . h_s == dpooled . pooled)
//           and the trial's share of d attn.weight = sum_t dscore_t h_t
//   The parameter gradients are reductions over trials of per-trial vectors: the wave writes its row of `hb`
//   (nsd_head_tm_row_floats) and head_tm_grads_kernel sums them in a fixed order (deterministic, no atomics).
#include "nsd_seq.h"

namespace {

template <int VPL>
__device__ __forceinline__ void load_bf16_vals(const bf16_t *p, float (&v)[VPL]) {
    if constexpr (VPL == 1) {
        v[0] = __uint_as_float((unsigned)(*reinterpret_cast<const unsigned short *>(p)) << 16);
    } else if constexpr (VPL == 2) {
        const unsigned w = *reinterpret_cast<const unsigned *>(p);
        v[0] = bf16_lo(w); v[1] = bf16_hi(w);
    } else if constexpr (VPL == 4) {
        const u32x2 w = *reinterpret_cast<const u32x2 *>(p);
        v[0] = bf16_lo(w[0]); v[1] = bf16_hi(w[0]); v[2] = bf16_lo(w[1]); v[3] = bf16_hi(w[1]);
    } else {
#pragma unroll
        for (int q = 0; q < VPL / 8; ++q) {
            const u32x4 w = *reinterpret_cast<const u32x4 *>(p + 8 * q);
#pragma unroll
            for (int i = 0; i < 4; ++i) { v[8 * q + 2 * i] = bf16_lo(w[i]); v[8 * q + 2 * i + 1] = bf16_hi(w[i]); }
        }
    }
}
__device__ __forceinline__ float lane_bcast(const float v, const int src) { return __shfl(v, src, 64); }

// (the modes HEAD_EVAL / HEAD_TRAIN / HEAD_LOGITS / HEAD_DLOG: nsd_seq.h)

template <int VPL, bool TRAIN_>
__global__ __launch_bounds__(256) void head_tm_kernel(const HeadTmArgs a) {
    constexpr int MODE = TRAIN_ ? HEAD_TRAIN : HEAD_EVAL;
    const float *const dlogits = nullptr;
#include "nsd_head_tm_body.h"
}
template <int VPL>
__global__ __launch_bounds__(256) void head_tm_logits_kernel(const HeadTmArgs a) {
    constexpr int MODE = HEAD_LOGITS;
    const float *const dlogits = nullptr;
#include "nsd_head_tm_body.h"
}
template <int VPL>
__global__ __launch_bounds__(256) void head_tm_dlog_kernel(const HeadTmArgs a, const float *dlogits) {
    constexpr int MODE = HEAD_DLOG;
#include "nsd_head_tm_body.h"
}

// Head parameter gradients, two stages (fixed order -> deterministic): stage 1, one thread per (gradient element, slice of the
// batch): partial sums over the slice's trials; stage 2 adds the slices and scatters into the flat gradient vector.
// Element order: d ln.weight[DH] | d ln.bias[DH] | d attn.weight[DH] | d fc.0.weight[F*DH] | d fc.0.bias[F] | d fc.3.weight[K*F] |
// d fc.3.bias[K] | d attn.bias[1]
__device__ __forceinline__ long head_grad_count(int DH, int F, int K) { return 3L * DH + (long)F * DH + F + (long)K * F + K + 1; }

__global__ __launch_bounds__(256) void head_tm_grads_part_kernel(const float *hb, long stride, int B, int DH, int F, int K, float *part) {
    const long total = head_grad_count(DH, F, K);
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int per = (B + gridDim.y - 1) / gridDim.y;
    const int b_lo = blockIdx.y * per, b_hi = b_lo + per < B ? b_lo + per : B;
    const long o_dpre = 4L * DH, o_act = o_dpre + F, o_dlog = o_act + F, o_ds = o_dlog + K;
    const long n_vec = 3L * DH, n_fc0 = (long)F * DH, n_fc3 = (long)K * F;
    long oa, ob = -1;                                           // element = sum_b hb[b][oa] (* hb[b][ob])
    long i = e;
    if (i < n_vec) { const int which = (int)(i / DH); oa = (which + 1L) * DH + (i - (long)which * DH); }
    else if ((i -= n_vec) < n_fc0) { const int f = (int)(i / DH); oa = o_dpre + f; ob = i - (long)f * DH; }
    else if ((i -= n_fc0) < F) { oa = o_dpre + i; }
    else if ((i -= F) < n_fc3) { const int k = (int)(i / F); oa = o_dlog + k; ob = o_act + (i - (long)k * F); }
    else if ((i -= n_fc3) < K) { oa = o_dlog + i; }
    else { oa = o_ds; }
    float s0 = 0.f, s1 = 0.f;
    int b = b_lo;
    if (ob < 0) {
        for (; b + 1 < b_hi; b += 2) { s0 += hb[(long)b * stride + oa]; s1 += hb[(long)(b + 1) * stride + oa]; }
        if (b < b_hi) s0 += hb[(long)b * stride + oa];
    } else {
        for (; b + 1 < b_hi; b += 2) {
            s0 = fmaf(hb[(long)b * stride + oa], hb[(long)b * stride + ob], s0);
            s1 = fmaf(hb[(long)(b + 1) * stride + oa], hb[(long)(b + 1) * stride + ob], s1);
        }
        if (b < b_hi) s0 = fmaf(hb[(long)b * stride + oa], hb[(long)b * stride + ob], s0);
    }
    part[(long)blockIdx.y * total + e] = s0 + s1;
}
__global__ __launch_bounds__(256) void head_tm_grads_sum_kernel(const float *part, int nparts, int DH, int F, int K, float *g_ln_w, float *g_ln_b,
                                                                float *g_attn_w, float *g_attn_b, float *g_fc0_w, float *g_fc0_b, float *g_fc3_w,
                                                                float *g_fc3_b) {
    const long total = head_grad_count(DH, F, K);
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    float s = 0.f;
    for (int z = 0; z < nparts; ++z) s += part[(long)z * total + e];
    const long n_fc0 = (long)F * DH, n_fc3 = (long)K * F;
    long i = e;
    if (i < DH) { g_ln_w[i] = s; return; }
    if ((i -= DH) < DH) { g_ln_b[i] = s; return; }
    if ((i -= DH) < DH) { g_attn_w[i] = s; return; }
    if ((i -= DH) < n_fc0) { g_fc0_w[i] = s; return; }
    if ((i -= n_fc0) < F) { g_fc0_b[i] = s; return; }
    if ((i -= F) < n_fc3) { g_fc3_w[i] = s; return; }
    if ((i -= n_fc3) < K) { g_fc3_b[i] = s; return; }
    g_attn_b[0] = s;
}

// the four kernels of a sequence width share one grid
template <int VPL>
int launch_vpl(const HeadTmArgs &a, int mode, const float *dlogits, hipStream_t st) {
    // the passes over the sequence are latency-bound, one wave per trial: with few trials (cfg5: 512 per GPU) four waves per workgroup
    // put them on half of the CUs -- spread the waves over as many CUs as there are trials
    const int cus = nsd_num_cus();
    const int wpw = a.B >= 4 * cus ? 4 : (a.B >= 2 * cus ? 2 : 1);
    const dim3 grid((a.B + wpw - 1) / wpw), wg(64 * wpw);
    switch (mode) {
    case HEAD_EVAL: hipLaunchKernelGGL((head_tm_kernel<VPL, false>), grid, wg, 0, st, a); break;
    case HEAD_TRAIN: hipLaunchKernelGGL((head_tm_kernel<VPL, true>), grid, wg, 0, st, a); break;
    case HEAD_LOGITS: hipLaunchKernelGGL((head_tm_logits_kernel<VPL>), grid, wg, 0, st, a); break;
    case HEAD_DLOG: hipLaunchKernelGGL((head_tm_dlog_kernel<VPL>), grid, wg, 0, st, a, dlogits); break;
    default: nsd_set_error("head_tm: unknown mode %d", mode); return NSD_E_INVALID;
    }
    NSD_CHECK_LAUNCH(mode == HEAD_DLOG ? "head_tm_dlog_kernel" : mode == HEAD_LOGITS ? "head_tm_logits_kernel" : "head_tm_kernel");
    return NSD_OK;
}

}  // namespace

int nsd_head_tm_launch(const HeadTmArgs &a, int mode, const float *dlogits, hipStream_t st) {
    if (a.B < 1) return NSD_OK;
    if (a.F > 64 || a.K > 64) { nsd_set_error("head_tm: F=%d K=%d exceed 64 (one lane per unit / class)", a.F, a.K); return NSD_E_INVALID; }
    switch (a.DH) {
    case 64: return launch_vpl<1>(a, mode, dlogits, st);
    case 128: return launch_vpl<2>(a, mode, dlogits, st);
    case 256: return launch_vpl<4>(a, mode, dlogits, st);
    case 512: return launch_vpl<8>(a, mode, dlogits, st);
    case 1024: return launch_vpl<16>(a, mode, dlogits, st);
    default: nsd_set_error("head_tm: sequence width %d not covered (64, 128, 256, 512, 1024)", a.DH); return NSD_E_INVALID;
    }
}

int nsd_head_tm_grads_launch(const float *hb, long hb_stride, int B, int DH, int F, int K, float *scratch, float *g_ln_w, float *g_ln_b,
                             float *g_attn_w, float *g_attn_b, float *g_fc0_w, float *g_fc0_b, float *g_fc3_w, float *g_fc3_b, hipStream_t st) {
    const long total = 3L * DH + (long)F * DH + F + (long)K * F + K + 1;
    const int NB = B >= 512 ? 16 : (B >= 64 ? 4 : 1);           // scratch: NB * total floats
    const unsigned gx = (unsigned)((total + 255) / 256);
    hipLaunchKernelGGL(head_tm_grads_part_kernel, dim3(gx, NB), dim3(256), 0, st, hb, hb_stride, B, DH, F, K, scratch);
    hipLaunchKernelGGL(head_tm_grads_sum_kernel, dim3(gx), dim3(256), 0, st, scratch, NB, DH, F, K, g_ln_w, g_ln_b, g_attn_w, g_attn_b, g_fc0_w,
                       g_fc0_b, g_fc3_w, g_fc3_b);
    NSD_CHECK_LAUNCH("head_tm_grads");
    return NSD_OK;
}
