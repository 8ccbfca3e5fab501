// nsd_head_fit.hip -- session calibration (nsd_stream_features / nsd_head_fit of include/nsd.h): the read-out of lstm_eeg_model.py:38-39
// (LayerNorm -> fc.0 -> RReLU -> dropout -> fc.3) refitted on frozen pooled features, E full-batch Adam epochs in ONE launch.
//
// One 256-thread workgroup per model; nothing leaves the CU between the first epoch and the last.  LDS map (fit_lds_floats of nsd_args.h):
//   xhat [N][48]     the features behind LayerNorm's normalisation: they are frozen, so mean, rstd and xhat are formed once
//   dln  [N][48]     d loss / d LayerNorm output of the epoch in flight
//   zd   [N][F]      z (fc.0 -> RReLU -> dropout) until fc.3's gradients are formed, d loss / d fc.0 pre-activation after that
//   dl   [N][K]      dlogits;  loss [N];  sgn [N][2]: the wave ballot of (pre-activation >= 0), all the backward needs of it
//   img              the trainable tail (FIT_H + 1 and F | 1 floats between rows);  grad [Pt];  two 64-float vectors per wave
// Adam's moments of a tail element live in the registers of the thread that owns it (element e: thread e % 256), for all epochs.
// An epoch: P1 forward + loss + dlogits, a wave per trial | P2 fc.3 gradients, a thread per element, n ascending; the loss sum | P3 the
// trial's backward, a wave per trial | P4 fc.0 and LayerNorm gradients, a thread per element, n ascending | P5 Adam.  A parameter's
// gradient is therefore one fmaf chain over n = 0 .. N-1 whatever M, the grid or the stream.
#include "nsd_args.h"

namespace {

constexpr int HH = FIT_H, NT = FIT_NT, W0S = FIT_H + 1;

__device__ __forceinline__ bool not_finite(const float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// feats[i][j] = pool_acc[j] / pool_den of slot slots[i]: the division nsd_stream48.hip hands to prefix_readout.  A wave per row.
__global__ __launch_bounds__(NT) void stream_features_kernel(const float *state, const int S, const int32_t *slots, const int n, float *feats) {
    const int i = blockIdx.x * (NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n || lane >= HH) return;
    const int slot = slots ? slots[i] : i;
    float v = __uint_as_float(0x7fc00000u);
    if ((unsigned)slot < (unsigned)S) {
        const float *st = state + (size_t)slot * STREAM_STRIDE;
        v = st[STREAM_ACC + lane] / st[STREAM_DEN];
    }
    feats[(size_t)i * HH + lane] = v;
}

// element e of the tail (ln.weight, ln.bias, fc.0.weight, fc.0.bias, fc.3.weight, fc.3.bias): its NSD_FIT_* group, its place in the LDS
// image and in the flat parameter vector
struct Elem { unsigned group; int img; long flat; };
__device__ __forceinline__ Elem tail_elem(const FitArgs &a, int e) {
    const int F = a.F, K = a.K, W3S = fit_w3s(F);
    if (e < HH) return Elem{NSD_FIT_LN, e, a.o_ln_w + e};
    e -= HH;
    if (e < HH) return Elem{NSD_FIT_LN, HH + e, a.o_ln_b + e};
    e -= HH;
    if (e < F * HH) { const int f = e / HH; return Elem{NSD_FIT_FC0, 2 * HH + f * W0S + (e - f * HH), a.o_fc0_w + e}; }
    e -= F * HH;
    const int i_b0 = 2 * HH + F * W0S;
    if (e < F) return Elem{NSD_FIT_FC0, i_b0 + e, a.o_fc0_b + e};
    e -= F;
    if (e < K * F) { const int k = e / F; return Elem{NSD_FIT_FC3, i_b0 + F + k * W3S + (e - k * F), a.o_fc3_w + e}; }
    e -= K * F;
    return Elem{NSD_FIT_FC3, i_b0 + F + K * W3S + e, a.o_fc3_b + e};
}

// b^s by squaring, in double: a function of s alone, so a run cut into several calls forms the bias corrections of one uncut run
__device__ __forceinline__ double pow_int(double b, long long s) {
    double r = 1.0;
    while (s) { if (s & 1) r *= b; b *= b; s >>= 1; }
    return r;
}

// RReLU slope and head-dropout multiplier of (trial n, unit f): the values nsd_train_masks writes for a batch of N trials
struct Noise { uint64_t seed; uint32_t thr; float keep; };
__device__ __forceinline__ void noise_of(const Noise &r, const uint32_t base, const int F, const int n, const int f, float *slope, float *dmul) {
    const uint64_t idx = (uint64_t)((long)n * F + f);
    const float u = (float)(nsd_rand_u32(r.seed, base + 1u, idx) >> 8) * (1.0f / 16777216.0f);
    *slope = 0.125f + ((float)(1.0 / 3.0) - 0.125f) * u;
    *dmul = nsd_rand_u32(r.seed, base + 2u, idx) >= r.thr ? r.keep : 0.f;
}

template <int OWN>
__global__ __launch_bounds__(NT) void head_fit_kernel(const FitArgs a) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, mo = blockIdx.x;
    const int N = a.N, F = a.F, K = a.K, W3S = fit_w3s(F), Pt = fit_tail(F, K);
    const int i_lnw = 0, i_lnb = HH, i_w0 = 2 * HH, i_b0 = i_w0 + F * W0S, i_w3 = i_b0 + F, i_b3 = i_w3 + K * W3S;
    float *xhat = lds, *dln = xhat + (size_t)N * HH, *zd = dln + (size_t)N * HH, *dl = zd + (size_t)N * F, *lossn = dl + (size_t)N * K;
    unsigned *sgn = reinterpret_cast<unsigned *>(lossn + N);
    float *img = reinterpret_cast<float *>(sgn + 2 * N), *grad = img + fit_image(F, K), *vecs = grad + Pt, *misc = vecs + (NT / 64) * 128;
    int *flag = reinterpret_cast<int *>(misc);                 // flag[1]: a non-finite input, flag[3]: a non-finite loss; misc[0] = 1, misc[2]: the loss
    float *vln = vecs + wave * 128, *vz = vln + 64;

    float *params = a.params + (size_t)mo * a.P;
    const float *feats = a.feats + (size_t)mo * a.feats_stride, *targets = a.targets + (size_t)mo * N * K;
    float *st = a.state + (size_t)mo * fit_stride(F, K);
    long long *count = reinterpret_cast<long long *>(st + fit_epochs_off(F, K));
    int *status = reinterpret_cast<int *>(st + fit_status_off(F, K));
    float *loss_out = a.loss_out ? a.loss_out + (size_t)mo * a.epochs : nullptr;
    const float nan = __uint_as_float(0x7fc00000u);
    const Noise noise{a.seed[mo], a.thr[mo], a.keep[mo]};       // this model's entries, once: the arrays stay in the argument block
    const uint32_t base0 = a.base[mo];

    if (tid == 0) { misc[0] = 1.0f; flag[1] = 0; flag[3] = 0; }
    __syncthreads();
    const int status0 = status[0];
    const long long s0 = count[0];
    // ---- once: LayerNorm's normalisation of the frozen features (prefix_readout's expressions), the finite check, the tail -> LDS ----
    for (int n = wave; n < N; n += NT / 64) {
        const float x = lane < HH ? feats[(size_t)n * HH + lane] : 0.f;
        const float q = lane < K ? targets[(size_t)n * K + lane] : 0.f;
        if (not_finite(x) || not_finite(q)) flag[1] = 1;
        const float mu = wave_sum(x) * (1.0f / HH);
        const float dlt = lane < HH ? x - mu : 0.f;
        const float rstd = 1.0f / sqrtf(wave_sum(dlt * dlt) * (1.0f / HH) + 1e-5f);
        if (lane < HH) xhat[n * HH + lane] = dlt * rstd;
    }
    for (int e = tid; e < Pt; e += NT) { const Elem el = tail_elem(a, e); img[el.img] = params[el.flat]; }
    float mreg[OWN], vreg[OWN];
#pragma unroll
    for (int i = 0; i < OWN; ++i) {
        const int e = tid + NT * i;
        mreg[i] = e < Pt ? st[e] : 0.f;
        vreg[i] = e < Pt ? st[Pt + e] : 0.f;
    }
    __syncthreads();
    if (status0 != 0 || flag[1] != 0) {                        // refused on the device: nothing of the model changes but its status word
        if (loss_out) for (int e = tid; e < a.epochs; e += NT) loss_out[e] = nan;
        if (tid == 0) status[0] = 1;
        return;
    }

    int done = 0;
    for (; done < a.epochs; ++done) {
        const long long s = s0 + done;                         // 0-based global epoch
        const uint32_t base = base0 + 4u * (uint32_t)s;
        // ---- P1: forward, loss and dlogits of trial n by one wave ----
        for (int n = wave; n < N; n += NT / 64) {
            if (lane < HH) vln[lane] = xhat[n * HH + lane] * img[i_lnw + lane] + img[i_lnb + lane];
            float pre = 0.f, act = 0.f;
            if (lane < F) {
                float acc = img[i_b0 + lane];
                const float *w = img + i_w0 + lane * W0S;
#pragma unroll 8
                for (int j = 0; j < HH; ++j) acc = fmaf(w[j], vln[j], acc);
                pre = acc;
                float slope = a.eval_slope, dmul = 1.f;
                if (a.rng_on) noise_of(noise, base, F, n, lane, &slope, &dmul);
                act = (pre >= 0.f ? pre : pre * slope) * dmul;
                zd[n * F + lane] = act;
                vz[lane] = act;
            }
            const unsigned long long pos = __ballot(lane < F && pre >= 0.f);
            if (lane == 0) { sgn[2 * n] = (unsigned)pos; sgn[2 * n + 1] = (unsigned)(pos >> 32); }
            float lg = -INFINITY;
            if (lane < K) {
                float acc = img[i_b3 + lane];
                const float *w = img + i_w3 + lane * W3S;
#pragma unroll 8
                for (int f = 0; f < F; ++f) acc = fmaf(w[f], vz[f], acc);
                lg = acc;
            }
            const float mx = wave_max(lg);
            const float ex = lane < K ? expf(lg - mx) : 0.f;
            const float den = wave_sum(ex);
            const float q = lane < K ? targets[(size_t)n * K + lane] : 0.f;
            float ls;
            const float dq = soft_ce_wave(q, lg, mx, ex, den, logf(den), lane, K, &ls);
            if (lane < K) dl[n * K + lane] = dq * a.scale;
            if (lane == 0) lossn[n] = ls;
        }
        __syncthreads();
        // ---- P2: the epoch's loss (serial in n) and fc.3's gradients, a thread per element, n ascending ----
        if (tid == NT - 1) {
            float sum = 0.f;
#pragma unroll 8
            for (int n = 0; n < N; ++n) sum = sum + lossn[n];
            const float L = sum * a.scale;
            misc[2] = L;
            flag[3] = not_finite(L) ? 1 : 0;
        }
        if (a.train & NSD_FIT_FC3) {
            for (int e = tid; e < K * F + K; e += NT) {
                const bool bias = e >= K * F;
                const int k = bias ? e - K * F : e / F;
                const float *pa = dl + k, *pb = bias ? misc : zd + (e - k * F);
                const int sb = bias ? 0 : F;
                float acc = 0.f;
#pragma unroll 8
                for (int n = 0; n < N; ++n) acc = fmaf(pa[n * K], pb[n * sb], acc);
                grad[Pt - (K * F + K) + e] = acc;
            }
        }
        __syncthreads();
        if (flag[3]) break;                                    // the parameters and moments keep the values they had before this epoch
        // ---- P3: the trial's backward by one wave: d pre-activation over z, d LayerNorm output ----
        if (a.train & (NSD_FIT_LN | NSD_FIT_FC0)) {
            for (int n = wave; n < N; n += NT / 64) {
                if (lane < F) {
                    float dact = 0.f;
#pragma unroll 4
                    for (int k = 0; k < K; ++k) dact = fmaf(dl[n * K + k], img[i_w3 + k * W3S + lane], dact);
                    float slope = a.eval_slope, dmul = 1.f;
                    if (a.rng_on) noise_of(noise, base, F, n, lane, &slope, &dmul);
                    const bool pos = (sgn[2 * n + (lane >> 5)] >> (lane & 31)) & 1u;
                    zd[n * F + lane] = dact * dmul * (pos ? 1.f : slope);
                }
                if ((a.train & NSD_FIT_LN) && lane < HH) {
                    float acc = 0.f;
                    const float *dp = zd + n * F, *w = img + i_w0 + lane;
#pragma unroll 8
                    for (int f = 0; f < F; ++f) acc = fmaf(dp[f], w[f * W0S], acc);
                    dln[n * HH + lane] = acc;
                }
            }
        }
        __syncthreads();
        // ---- P4: LayerNorm's and fc.0's gradients, a thread per element, n ascending ----
        for (int e = tid; e < 2 * HH + F * HH + F; e += NT) {
            float acc = 0.f;
            if (e < 2 * HH) {
                if (!(a.train & NSD_FIT_LN)) continue;
                const int j = e < HH ? e : e - HH;
                const float *pa = dln + j, *pb = e < HH ? xhat + j : misc;
                const int sb = e < HH ? HH : 0;
#pragma unroll 8
                for (int n = 0; n < N; ++n) acc = fmaf(pa[n * HH], pb[n * sb], acc);
            } else {
                if (!(a.train & NSD_FIT_FC0)) continue;
                const int r = e - 2 * HH;
                if (r < F * HH) {
                    const int f = r / HH, j = r - f * HH;
                    const float gw = img[i_lnw + j], gb = img[i_lnb + j];
                    const float *pa = zd + f, *px = xhat + j;
#pragma unroll 8
                    for (int n = 0; n < N; ++n) acc = fmaf(pa[n * F], px[n * HH] * gw + gb, acc);
                } else {
                    const float *pa = zd + (r - F * HH);
#pragma unroll 8
                    for (int n = 0; n < N; ++n) acc = fmaf(pa[n * F], 1.0f, acc);
                }
            }
            grad[e] = acc;
        }
        __syncthreads();
        // ---- P5: Adam (adam_kernel's arithmetic, in its order) on the elements this thread owns ----
        const double bc1 = 1.0 - pow_int((double)a.b1, s + 1), bc2 = 1.0 - pow_int((double)a.b2, s + 1);
        const float lr_over_bc1 = (float)((double)a.lr / bc1), rsqrt_bc2 = (float)(1.0 / sqrt(bc2));
#pragma unroll
        for (int i = 0; i < OWN; ++i) {
            const int e = tid + NT * i;
            if (e < Pt) {
                const Elem el = tail_elem(a, e);
                if (a.train & el.group) {
                    const float pi = img[el.img];
                    const float gi = fmaf(a.wd, pi, grad[e] * 1.0f);
                    const float mi = a.b1 * mreg[i] + (1.f - a.b1) * gi;
                    const float vi = a.b2 * vreg[i] + (1.f - a.b2) * gi * gi;
                    mreg[i] = mi; vreg[i] = vi;
                    const float denom = sqrtf(vi) * rsqrt_bc2 + a.eps;
                    img[el.img] = pi - lr_over_bc1 * (mi / denom);
                }
            }
        }
        if (tid == 0 && loss_out) loss_out[done] = misc[2];
        __syncthreads();
    }

    // ---- out: the trained tensors, their moments, the epoch count; a non-finite loss leaves the state of the last good epoch ----
    const bool broke = done < a.epochs;
    if (broke && loss_out) for (int e = done + tid; e < a.epochs; e += NT) loss_out[e] = nan;
#pragma unroll
    for (int i = 0; i < OWN; ++i) {
        const int e = tid + NT * i;
        if (e < Pt) {
            const Elem el = tail_elem(a, e);
            if (a.train & el.group) { params[el.flat] = img[el.img]; st[e] = mreg[i]; st[Pt + e] = vreg[i]; }
        }
    }
    if (tid == 0) {
        count[0] = s0 + done;
        if (broke) status[0] = 1;
    }
}

template <int OWN>
int fit_launch(const FitArgs &a, int M, size_t lds, hipStream_t st) {
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void *)head_fit_kernel<OWN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(head_fit_kernel<OWN>, dim3(M), dim3(NT), lds, st, a);
    NSD_CHECK_LAUNCH("head_fit");
    return NSD_OK;
}

}  // namespace

int nsd_head_fit_launch(const FitArgs &a, int M, hipStream_t st) {
    const size_t lds = (size_t)fit_lds_floats(a.N, a.F, a.K) * sizeof(float);
    const int own = (fit_tail(a.F, a.K) + NT - 1) / NT;
    if (own <= 8) return fit_launch<8>(a, M, lds, st);
    if (own <= 16) return fit_launch<16>(a, M, lds, st);
    return fit_launch<FIT_MAX_OWN>(a, M, lds, st);
}

int nsd_stream_features_launch(const float *state, int S, const int32_t *slots, int n, float *feats, hipStream_t st) {
    hipLaunchKernelGGL(stream_features_kernel, dim3((n + NT / 64 - 1) / (NT / 64)), dim3(NT), 0, st, state, S, slots, n, feats);
    NSD_CHECK_LAUNCH("stream_features");
    return NSD_OK;
}
