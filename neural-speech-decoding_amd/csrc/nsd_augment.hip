// nsd_augment.hip -- trial augmentation for the trainers (nsd_augment of include/nsd.h; an extension, the reference has none):
// time shift, amplitude scale, additive noise, channel dropout, optionally followed by the per-channel z-score, in ONE launch for
// all models of a model-batched step.  Every draw is nsd_rand_u32(seed, base_stream + 3, index), so a test restates a launch in numpy.
//
// One 256-thread workgroup per (model, trial), grid-stride; lanes run along the contiguous [t][c] axis with the thread <-> element
// mapping of zscore_kernel (nsd_misc.hip): thread tid owns channel tid % C and the elements tid + k * act, act = (256 / C) * C.  That
// mapping makes the fused z-score the sums of zscore_kernel in the same order (bitwise nsd_zscore_fwd of the unfused output), and it
// keeps what depends on the channel alone -- the drop bit -- in a register.  The per-trial draws (shift, scale, C drop bits) are
// formed once per workgroup by a few threads and broadcast through LDS; the element loop holds one hash (the noise) and no division.
// Every fp32 operation of the augmentation is an explicit _rn intrinsic: one rounding each whatever the contraction setting.
//
// Memory-bound: x read once, y written once (2 * B*T*C*4 bytes per model).  With the z-score, a window of up to 64 KB is staged in
// LDS by the first statistic pass and the other two passes read it there; larger windows recompute the augmented value per pass.
// Loads are one dword per lane (256 B per wave-instruction): wider loads would give a thread several channels and change the
// order of the z-score's sums.
#include "nsd_args.h"

#define AUG_NT 256
constexpr uint32_t AUG_STREAM = 3u;                        // base_stream + 3: the trainers use + {0, 1, 2}
constexpr uint64_t AUG_TRIAL_BIT = 0x8000000000000000ull;   // per-trial index space (the per-element indices keep the top bit clear)

struct AugTrial {                                          // what one workgroup knows about its trial
    const float *xb;
    uint64_t seed, ebase;                                  // ebase = b * T * C: index of the trial's first element
    uint32_t stream;
    int shift;
    float scale;
    bool dropped;                                          // this thread's channel
};

// (am: the parameters of the trial's model, AugArgs::mod[m]; workgroup-uniform)
__device__ __forceinline__ float aug_value(const AugArgs &a, const AugArgs::Model &am, const AugTrial &tr, const int t, const int ch, const int e) {
    int ts = t;
    if (am.max_shift) { ts = t - tr.shift; ts = ts < 0 ? 0 : (ts > a.T - 1 ? a.T - 1 : ts); }
    float v = tr.xb[(size_t)ts * a.C + ch];
    if (am.scale_on) v = __fmul_rn(tr.scale, v);
    if (am.noise_on) {
        const uint32_t q = nsd_rand_u32(tr.seed, tr.stream, tr.ebase + (uint64_t)e);
        const int n = (int)__builtin_amdgcn_sad_u8(q, 0u, 0u) - 510;          // sum of the four bytes, one instruction
        v = __fadd_rn(v, __fmul_rn(am.noise_k, (float)n));
    }
    return tr.dropped ? 0.f : v;
}

// ZS: the fused z-score; STAGE (with ZS): the augmented window is kept in LDS between the passes
template <bool ZS, bool STAGE>
__global__ __launch_bounds__(AUG_NT) void augment_kernel(const AugArgs a) {
    extern __shared__ __attribute__((aligned(16))) float al[];   // [AUG_NT] partials, [2C] stats, [2 + C] draws, (16-byte aligned) [T*C] window
    float *stat = al + AUG_NT;
    uint32_t *draw = reinterpret_cast<uint32_t *>(stat + 2 * a.C);
    float *win = al + ((AUG_NT + 3 * a.C + 2 + 3) & ~3);
    const int tid = threadIdx.x;
    const int C = a.C, T = a.T;
    const int act = (AUG_NT / C) * C;                      // as zscore_kernel: threads taking part, each keeps one channel
    const int ch = tid % C, t0 = tid / C, rows = act / C;
    const int n_el = T * C;
    const uint32_t base_dev = a.step_dev ? (uint32_t)(a.step_dev[0] & 0x3FFFFFFF) * 4u : 0u;
    const long total = (long)a.M * a.B;
    for (long g = blockIdx.x; g < total; g += gridDim.x) {
        const int m = (int)(g / a.B), b = (int)(g - (long)m * a.B);
        const AugArgs::Model am = a.mod[m];
        AugTrial tr;
        tr.xb = a.x + (size_t)m * a.x_stride + (size_t)b * n_el;
        tr.seed = a.seed[m];
        tr.stream = (a.step_dev ? base_dev : a.base[m]) + AUG_STREAM;
        tr.ebase = (uint64_t)b * (uint64_t)n_el;
        float *yb = a.y + (size_t)g * n_el;
        // ---- per-trial draws, once per workgroup ----
        const uint64_t pidx = AUG_TRIAL_BIT | ((uint64_t)b << 16);
        if (am.drop_on && tid < C) draw[2 + tid] = nsd_rand_u32(tr.seed, tr.stream, pidx | (uint64_t)(256 + tid)) < am.thr_channel ? 1u : 0u;
        if (am.max_shift && tid == AUG_NT - 64)
            draw[0] = (uint32_t)((int)(nsd_rand_u32(tr.seed, tr.stream, pidx) % (uint32_t)(2 * am.max_shift + 1)) - am.max_shift);
        if (am.scale_on && tid == AUG_NT - 63) {
            const float u = (float)(nsd_rand_u32(tr.seed, tr.stream, pidx | 1ull) >> 8) * (1.0f / 16777216.0f);
            const float w = __fadd_rn(__fmul_rn(2.0f, u), -1.0f);                 // exact
            draw[1] = __float_as_uint(__fadd_rn(1.0f, __fmul_rn(am.scale_range, w)));
        }
        __syncthreads();
        tr.shift = am.max_shift ? (int)draw[0] : 0;
        tr.scale = am.scale_on ? __uint_as_float(draw[1]) : 1.0f;
        tr.dropped = am.drop_on ? draw[2 + ch] != 0u : false;
        if constexpr (!ZS) {
            if (tid < act) for (int t = t0, e = tid; t < T; t += rows, e += act) yb[e] = aug_value(a, am, tr, t, ch, e);
        } else {
            // the three passes of zscore_kernel on the augmented window v (same partial sums, same order)
            float s = 0.f;
            if (tid < act) for (int t = t0, e = tid; t < T; t += rows, e += act) {
                const float v = aug_value(a, am, tr, t, ch, e);
                if constexpr (STAGE) win[e] = v;
                s += v;
            }
            al[tid] = s;
            __syncthreads();
            if (tid < C) { float mm = 0.f; for (int q = 0; q < rows; ++q) mm += al[q * C + tid]; stat[tid] = mm / (float)T; }
            __syncthreads();
            const float mu = stat[ch];
            float var = 0.f;
            if (tid < act) for (int t = t0, e = tid; t < T; t += rows, e += act) {
                const float d = (STAGE ? win[e] : aug_value(a, am, tr, t, ch, e)) - mu;
                var = fmaf(d, d, var);
            }
            __syncthreads();
            al[tid] = var;
            __syncthreads();
            if (tid < C) { float mm = 0.f; for (int q = 0; q < rows; ++q) mm += al[q * C + tid]; stat[C + tid] = 1.0f / (sqrtf(mm / (float)T) + 1e-6f); }
            __syncthreads();
            const float rs = stat[C + ch];
            if (tid < act) for (int t = t0, e = tid; t < T; t += rows, e += act)
                yb[e] = ((STAGE ? win[e] : aug_value(a, am, tr, t, ch, e)) - mu) * rs;
        }
        __syncthreads();                                   // (draws, partials and the staged window are reused by the next trial)
    }
}

// the fused z-score stages windows of up to 64 KB in LDS
static bool aug_staged(const AugArgs &a) { return (size_t)a.T * a.C * sizeof(float) <= 64 * 1024; }

int nsd_augment_launch(const AugArgs &a, hipStream_t st) {
    const long total = (long)a.M * a.B;
    if (total <= 0) return NSD_OK;
    if (a.C < 1 || a.C > AUG_NT || a.T < 1) { nsd_set_error("augment: bad shape T=%d C=%d", a.T, a.C); return NSD_E_INVALID; }
    const long cap = 8L * nsd_num_cus();
    const dim3 grid((unsigned)(total < cap ? total : cap)), block(AUG_NT);
    const size_t head = (size_t)((AUG_NT + 3 * a.C + 2 + 3) & ~3) * sizeof(float);
    if (!a.zscore) {
        hipLaunchKernelGGL((augment_kernel<false, false>), grid, block, head, st, a);
    } else if (aug_staged(a)) {
        const size_t lds = head + (size_t)a.T * a.C * sizeof(float);
        if (lds > 64 * 1024)
            (void)hipFuncSetAttribute((const void *)augment_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((augment_kernel<true, true>), grid, block, lds, st, a);
    } else {
        hipLaunchKernelGGL((augment_kernel<true, false>), grid, block, head, st, a);
    }
    NSD_CHECK_LAUNCH("augment");
    return NSD_OK;
}
