// nsd_mixup.hip -- soft targets from labels and mixed windows for the trainers (nsd_mixup of include/nsd.h; an extension, the reference
// neither smooths, weights nor mixes): per trial b of a model's batch the target row
//     targets[b, k] = lambda_b * base(label_b)[k] + mu_b * base(label_p(b))[k],   base(j)[k] = w_k * (k == j ? (1 - eps) + eps / K : eps / K)
// and the window y[b] = lambda_b * x[b] + mu_b * x[p(b)], in ONE launch for all models of a model-batched step.  Every draw is
// nsd_rand_u32(seed, base_stream + 3, index) on index slots nsd_augment leaves alone, so a test restates a launch in numpy and an
// augmented step's draws do not move.  The mixing is a launch of its own and not a part of nsd_augment's because a trial needs its
// PARTNER's augmented (and z-scored) window, which another workgroup of that launch produces.
//
// One 256-thread workgroup per (model, trial), grid-stride, as augment_kernel; element e of the window belongs to thread e % 256 (the
// 16-byte path: float4 e to thread e % 256).  The per-trial draws are formed by every thread (two hashes): no LDS, no barrier.  Every fp32
// operation is an explicit _rn intrinsic, one rounding each whatever the contraction setting; the order is the one written in nsd.h.
// Memory-bound: two windows read, one written (3 * T*C*4 bytes per trial); 16-byte loads and stores where T*C and the pointers allow.
#include "nsd_args.h"

#define MIX_NT 256
constexpr uint32_t MIX_STREAM = 3u;                                // base_stream + 3, shared with nsd_augment (other index slots)
constexpr uint64_t MIX_TRIAL_BIT = 0x8000000000000000ull;          // P(b, slot) = 2^63 | b << 16 | slot
constexpr uint64_t MIX_ROT_INDEX = 0xC000000000000000ull;          // 2^63 | 2^62: the rotation of a model's batch
constexpr uint64_t MIX_LAMBDA_SLOT = 1024ull;

template <bool VEC>
__global__ __launch_bounds__(MIX_NT) void mixup_kernel(const MixArgs a) {
    const int tid = threadIdx.x;
    const int B = a.B, K = a.K;
    const long n_el = a.n_el;
    const uint32_t base_dev = a.step_dev ? (uint32_t)(a.step_dev[0] & 0x3FFFFFFF) * 4u : 0u;
    const long total = (long)a.M * B;
    for (long g = blockIdx.x; g < total; g += gridDim.x) {
        const int m = (int)(g / B), b = (int)(g - (long)m * B);
        const float mix = a.mix[m], eps = a.eps[m];                // the model's nsd_mix: workgroup-uniform
        const bool mixing = mix != 0.f && B >= 2;
        const float eps_k = __fdiv_rn(eps, (float)K);
        const float on = __fadd_rn(__fsub_rn(1.0f, eps), eps_k);
        int p = b;
        float lam = 1.0f, mu = 0.f;
        if (mixing) {
            const uint64_t seed = a.seed[m];
            const uint32_t stream = (a.step_dev ? base_dev : a.base[m]) + MIX_STREAM;
            const uint32_t r = 1u + nsd_rand_u32(seed, stream, MIX_ROT_INDEX) % (uint32_t)(B - 1);
            p = (int)(((uint32_t)b + r) % (uint32_t)B);
            const float u = (float)(nsd_rand_u32(seed, stream, MIX_TRIAL_BIT | ((uint64_t)b << 16) | MIX_LAMBDA_SLOT) >> 8) * (1.0f / 16777216.0f);
            lam = __fsub_rn(1.0f, __fmul_rn(mix, u));
            mu = __fsub_rn(1.0f, lam);
        }
        if (tid < K) {
            const int lb = a.labels[g], lp = a.labels[(long)m * B + p];
            float tb = tid == lb ? on : eps_k, tp = tid == lp ? on : eps_k;
            if (a.w) { const float w = a.w[(long)m * a.w_stride + tid]; tb = __fmul_rn(w, tb); tp = __fmul_rn(w, tp); }
            a.targets[g * K + tid] = mixing ? __fadd_rn(__fmul_rn(lam, tb), __fmul_rn(mu, tp)) : tb;
        }
        if (!a.y) continue;                                        // (workgroup-uniform: a targets-only launch)
        const float *xb = a.x + (size_t)m * a.x_stride + (size_t)b * n_el;
        const float *xp = a.x + (size_t)m * a.x_stride + (size_t)p * n_el;
        float *yb = a.y + (size_t)g * n_el;
        if constexpr (VEC) {
            const long n4 = n_el >> 2;
            for (long e = tid; e < n4; e += MIX_NT) {
                float4 v = reinterpret_cast<const float4 *>(xb)[e];
                if (mixing) {
                    const float4 o = reinterpret_cast<const float4 *>(xp)[e];
                    v.x = __fadd_rn(__fmul_rn(lam, v.x), __fmul_rn(mu, o.x)); v.y = __fadd_rn(__fmul_rn(lam, v.y), __fmul_rn(mu, o.y));
                    v.z = __fadd_rn(__fmul_rn(lam, v.z), __fmul_rn(mu, o.z)); v.w = __fadd_rn(__fmul_rn(lam, v.w), __fmul_rn(mu, o.w));
                }
                reinterpret_cast<float4 *>(yb)[e] = v;
            }
        } else {
            for (long e = tid; e < n_el; e += MIX_NT) {
                float v = xb[e];
                if (mixing) v = __fadd_rn(__fmul_rn(lam, v), __fmul_rn(mu, xp[e]));
                yb[e] = v;
            }
        }
    }
}

int nsd_mixup_launch(const MixArgs &a, hipStream_t st) {
    const long total = (long)a.M * a.B;
    if (total <= 0) return NSD_OK;
    if (a.K < 1 || a.K > 64 || a.n_el < 0) { nsd_set_error("mixup: bad shape K=%d T*C=%ld", a.K, a.n_el); return NSD_E_INVALID; }
    const long cap = 8L * nsd_num_cus();
    const dim3 grid((unsigned)(total < cap ? total : cap)), block(MIX_NT);
    // 16-byte accesses: every trial's window starts on a 16-byte boundary
    const bool vec = a.y && (a.n_el & 3) == 0 && (a.x_stride & 3) == 0 && (((uintptr_t)a.x | (uintptr_t)a.y) & 15) == 0;
    if (vec) hipLaunchKernelGGL((mixup_kernel<true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((mixup_kernel<false>), grid, block, 0, st, a);
    NSD_CHECK_LAUNCH("mixup");
    return NSD_OK;
}
