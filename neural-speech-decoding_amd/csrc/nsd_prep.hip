// nsd_prep.hip -- causal per-channel front end for live streams and their training (nsd_prep_* of include/nsd.h; an extension, the
// reference filters whole windows on the host): baseline removal, common-average reference, up to four IIR sections (direct form II
// transposed) and a running z-score, with the state carried from chunk to chunk in a caller-owned slot, as nsd_stream_step carries the
// model's.  Window mode (no state) runs the same transform over whole trials from a reset state: what the trainers and predict use.
//
// One lane carries one (stream, channel): the first wave of a workgroup holds 64 / C streams and runs their recurrences; three helper
// waves share what is not a recurrence -- the staging, the common average and the z-score's division.
// The time loop is serial, as the definition demands: a step is a dependent chain of a few dozen fp32 operations, each an explicit _rn
// intrinsic (one rounding each whatever the contraction setting; sqrtf and / are the correctly rounded ones), and every sample runs
// the same sequence wherever it falls in a chunk -- state and outputs are bit for bit a function of the samples alone.
//
// x and y never meet the dependent chain: a trial's [tile][C] block is contiguous, so the wave stages PREP_TT steps of its streams
// through LDS with coalesced loads (16 bytes per lane where T*C and the pointers allow it, dwords otherwise), the lanes run their
// PREP_TT steps on LDS in place, and the tile goes back the same way.  A stream's tile is padded by one step, which puts lane i on bank
// i mod 32 where C divides 32 (elsewhere: fewer conflicts than the unpadded power-of-two stride, not none).  The common average needs all C channels of a step: before the serial part the wave forms m / C of every (stream, step) of the
// tile in parallel, summing the C baseline-corrected values serially from the staged tile -- the order the definition fixes.
// Everything a lane keeps lives in registers (constant indices after unrolling): there is no private segment.
#include "nsd_args.h"

namespace {

constexpr int PREP_NT = 64;                                // lanes that carry a (stream, channel): one wave
constexpr int PREP_BLOCK = 256;                            // threads of a workgroup: that wave and three helpers
constexpr int PREP_PAD = PREP_TT + 1;                      // steps per stream in the LDS tile (one of padding)

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }

// global <-> LDS for the `gl` streams of the group, steps [t0, t0 + nt): element i of stream gi is x[(b0 + gi) * T * C + t0 * C + i]
template <bool VEC, bool STORE>
__device__ __forceinline__ void prep_move(const float *src, float *dst, float *tile, const long b0, const int gl, const int t0, const int nt,
                                          const int T, const int C, const int tid) {
    constexpr int W = VEC ? 4 : 1;
    const int nq = nt * C / W;                             // (VEC: T * C and PREP_TT * C are multiples of 4, so every tile's count is)
    const int total = gl * nq;
    for (int idx = tid; idx < total; idx += PREP_BLOCK) {
        const int gi = idx / nq, i = (idx - gi * nq) * W;
        const size_t gofs = ((size_t)(b0 + gi) * T + t0) * C + i;
        float *l = tile + gi * PREP_PAD * C + i;
        if constexpr (STORE) {
            if constexpr (VEC) *reinterpret_cast<float4 *>(dst + gofs) = make_float4(l[0], l[1], l[2], l[3]);
            else dst[gofs] = l[0];
        } else {
            if constexpr (VEC) { const float4 q = ld4(src + gofs); l[0] = q.x; l[1] = q.y; l[2] = q.z; l[3] = q.w; }
            else l[0] = src[gofs];
        }
    }
}

// NS, ZS: the number of sections and the z-score switch as compile-time constants -- the serial loop has no branch on them
template <int NS, bool ZS, bool VEC>
__global__ __launch_bounds__(PREP_BLOCK) void prep_kernel(const CausalPrepArgs a) {
    __shared__ __attribute__((aligned(16))) float tile[PREP_NT * PREP_PAD];   // [stream][PREP_PAD][C]
    __shared__ float vart[PREP_NT * PREP_PAD];                                // the same layout: the running variance of each element
    __shared__ float mean[PREP_NT * PREP_PAD];                                // [stream][PREP_PAD]: m / C of the step (64 / C streams)
    __shared__ float x0s[PREP_NT];                                            // [stream][C]
    const int C = a.C, T = a.T, tid = threadIdx.x;
    const int G = PREP_NT / C;                             // streams per wave
    const int g = tid < PREP_NT ? tid / C : PREP_NT, ch = tid - g * C;        // (a helper thread carries nothing: g is past every stream)
    const long groups = ((long)a.B + G - 1) / G;
    for (long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const long b0 = grp * G, b = b0 + g;
        const int gl = (int)(a.B - b0 < G ? a.B - b0 : G);
        const bool mine = g < gl;                          // this lane carries a (stream, channel) of the call
        // ---- the lane's state: from its slot, or a reset one (window mode) ----
        long slot = b;
        if (mine && a.state && a.slots) slot = a.slots[b];
        const bool bad = mine && a.state && (unsigned long)slot >= (unsigned long)a.S;   // skipped: its rows of y are NaN
        const bool run = mine && !bad;
        float *sp = a.state ? a.state + (size_t)(run ? slot : 0) * prep_stride(C) : nullptr;
        float x0 = 0.f, mu = 0.f, var = 0.f, z1[NSD_PREP_MAX_SECTIONS], z2[NSD_PREP_MAX_SECTIONS];
        long long n = 0;
#pragma unroll
        for (int s = 0; s < NSD_PREP_MAX_SECTIONS; ++s) z1[s] = z2[s] = 0.f;
        if (run && sp) {
            x0 = sp[PREP_X0 + ch]; mu = sp[prep_mu(C) + ch]; var = sp[prep_var(C) + ch];
#pragma unroll
            for (int s = 0; s < NSD_PREP_MAX_SECTIONS; ++s) { z1[s] = sp[prep_z(C, s, 0) + ch]; z2[s] = sp[prep_z(C, s, 1) + ch]; }
            n = *reinterpret_cast<const long long *>(sp + prep_steps(C));
        }
        float *mt = tile + g * PREP_PAD * C + ch;          // this lane's column of its stream's tile
        float *vt = vart + g * PREP_PAD * C + ch;
        const float *mm = mean + g * PREP_PAD;
        for (int t0 = 0; t0 < T; t0 += PREP_TT) {
            const int nt = T - t0 < PREP_TT ? T - t0 : PREP_TT;
            prep_move<VEC, false>(a.x, nullptr, tile, b0, gl, t0, nt, T, C, tid);
            __syncthreads();
            if (a.car) {
                // ---- the step's common average, all (stream, step) pairs of the tile in parallel ----
                if (a.baseline) {
                    if (mine) x0s[tid] = n == 0 ? mt[0] : x0;          // (n == 0: this tile's first sample is the baseline)
                    __syncthreads();
                }
                for (int idx = tid; idx < gl * nt; idx += PREP_BLOCK) {
                    const int gi = idx / nt, t = idx - gi * nt;
                    const float *row = tile + gi * PREP_PAD * C + t * C;
                    float m = 0.f;
                    for (int c = 0; c < C; ++c) {
                        const float v = a.baseline ? __fsub_rn(row[c], x0s[gi * C + c]) : row[c];
                        m = c == 0 ? v : __fadd_rn(m, v);
                    }
                    mean[gi * PREP_PAD + t] = m / (float)C;
                }
                __syncthreads();
            }
            // ---- the serial part: nt steps of this lane's channel, in place in LDS ----
            if (run) {
                bool first = n == 0;                       // the slot's first sample: only ever a tile's first
                float xnext = mt[0];
                for (int t = 0; t < nt; ++t) {
                    const float xv = xnext;
                    xnext = mt[(t + 1) * C];               // (read a step ahead, off the chain; the last one reads the tile's padding)
                    float v = xv;
                    if (a.baseline) { x0 = first ? xv : x0; v = __fsub_rn(xv, x0); }
                    if (a.car) v = __fsub_rn(v, mm[t]);
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const float y = __fadd_rn(__fmul_rn(a.sos[s][0], v), z1[s]);
                        z1[s] = __fadd_rn(__fsub_rn(__fmul_rn(a.sos[s][1], v), __fmul_rn(a.sos[s][3], y)), z2[s]);
                        z2[s] = __fsub_rn(__fmul_rn(a.sos[s][2], v), __fmul_rn(a.sos[s][4], y));
                        v = y;
                    }
                    if constexpr (ZS) {
                        const float d = __fsub_rn(v, mu), ad = __fmul_rn(a.alpha, d);
                        const float mu1 = __fadd_rn(mu, ad), var1 = __fmul_rn(a.oma, __fadd_rn(var, __fmul_rn(ad, d)));
                        mu = first ? v : mu1; var = first ? a.var0 : var1;
                        v = __fsub_rn(v, mu);                  // the numerator; the division follows below, off the chain
                        vt[t * C] = var;
                    }
                    mt[t * C] = v;
                    first = false;
                }
                n += nt;
            } else if (bad) {
                for (int t = 0; t < nt; ++t) { mt[t * C] = __builtin_nanf(""); vt[t * C] = 1.f; }
            }
            __syncthreads();
            if constexpr (ZS) {
                // ---- the z-score's division: no sample's depends on another's, so the whole workgroup shares the tile's ----
                const int ne = nt * C;
                for (int idx = tid; idx < gl * ne; idx += PREP_BLOCK) {
                    const int gi = idx / ne, e = gi * PREP_PAD * C + (idx - gi * ne);
                    tile[e] = tile[e] / __fadd_rn(sqrtf(vart[e]), 1e-6f);
                }
                __syncthreads();
            }
            prep_move<VEC, true>(nullptr, a.y, tile, b0, gl, t0, nt, T, C, tid);
            __syncthreads();                               // (the next tile, or the next group, is staged over this one)
        }
        if (run && sp) {
            sp[PREP_X0 + ch] = x0; sp[prep_mu(C) + ch] = mu; sp[prep_var(C) + ch] = var;
#pragma unroll
            for (int s = 0; s < NSD_PREP_MAX_SECTIONS; ++s) { sp[prep_z(C, s, 0) + ch] = z1[s]; sp[prep_z(C, s, 1) + ch] = z2[s]; }
            if (ch == 0) *reinterpret_cast<long long *>(sp + prep_steps(C)) = n;
        }
    }
}

// a reset slot is all zero: filters at rest, step count 0 (x0, mu and var are set by the slot's first sample)
__global__ __launch_bounds__(256) void prep_reset_kernel(float *state, const int stride, const int S, const int32_t *slots, const int n) {
    const int i = blockIdx.x;
    if (i >= n) return;
    const int slot = slots ? slots[i] : i;
    if ((unsigned)slot >= (unsigned)S) return;
    for (int e = threadIdx.x; e < stride; e += 256) state[(size_t)slot * stride + e] = 0.f;
}

}  // namespace

int nsd_prep_launch(const CausalPrepArgs &a, hipStream_t st) {
    const int G = PREP_NT / a.C;
    const long groups = ((long)a.B + G - 1) / G;
    const dim3 grid((unsigned)(groups < PREP_GRID_CAP ? groups : PREP_GRID_CAP)), block(PREP_BLOCK);
    const bool vec = ((long)a.T * a.C) % 4 == 0 && ((uintptr_t)a.x | (uintptr_t)a.y) % 16 == 0;
    using kernel_t = void (*)(CausalPrepArgs);
#define PREP_K(NS) {{prep_kernel<NS, false, false>, prep_kernel<NS, false, true>}, {prep_kernel<NS, true, false>, prep_kernel<NS, true, true>}}
    static const kernel_t table[NSD_PREP_MAX_SECTIONS + 1][2][2] = {PREP_K(0), PREP_K(1), PREP_K(2), PREP_K(3), PREP_K(4)};
#undef PREP_K
    hipLaunchKernelGGL(table[a.ns][a.zs ? 1 : 0][vec ? 1 : 0], grid, block, 0, st, a);
    NSD_CHECK_LAUNCH("prep_step");
    return NSD_OK;
}

int nsd_prep_reset_launch(float *state, int C, int S, const int32_t *slots, int n, hipStream_t st) {
    hipLaunchKernelGGL(prep_reset_kernel, dim3(n), dim3(256), 0, st, state, prep_stride(C), S, slots, n);
    NSD_CHECK_LAUNCH("prep_reset");
    return NSD_OK;
}
