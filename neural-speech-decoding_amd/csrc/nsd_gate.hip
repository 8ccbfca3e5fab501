// nsd_gate.hip -- signal-quality gate for live streams and their training (nsd_gate_* of include/nsd.h; an extension): a causal
// per-channel detector of railed, jumping, flat and high-amplitude spans with sample-and-hold of a bad channel (gate_kernel, in front of
// nsd_prep_step), and the stateless stage behind the front end that zeroes a bad channel and turns a step that is bad on too many
// channels into NaN (gate_apply_kernel).  Cut from the pattern of nsd_prep.hip: one lane carries one (stream, channel), the first wave
// of a workgroup holds 64 / C streams and runs what is a recurrence; three helper waves share everything else.
//
// What is a recurrence: the flat run, the hang-over and the held value -- a few integer operations per step, run serially by the carrying
// wave on flags the whole workgroup prepared.  What is not: the rail test, the jump and flat-pair tests (x[n] against x[n-1]) and the
// peak-to-peak test (a sliding min / max over the last pp_samples raw samples).  For those the raw samples of a stream live in a circular
// LDS window of GATE_ROWS = 128 steps: a tile of PREP_TT steps is staged behind the 64 steps before it (at the first tile: the slot's
// ring, or NaN where the stream has no such sample yet -- a NaN is "not finite", which every test skips, so n == 0 needs no case of its
// own), and every (stream, step, channel) of the tile is tested in parallel.  A tile never wraps (128 and the tile start are multiples
// of PREP_TT) and the next tile overwrites rows that lie at least 64 steps behind its own first step.
//
// A stream's window is padded by one step: its stride of 129 * C words puts lane i of the carrying wave on bank i mod 32 where C divides
// 32, as the prep kernel's tile does; the parallel phases walk elements in address order.  y and the per-element flags go through tiles
// of the prep kernel's [stream][PREP_TT + 1][C] layout, x and y move 16 bytes per lane where T * C and the pointers allow it.  The mask word
// of a step is an OR over the C flags of its step in LDS.  No atomics, no private segment, vector stores only.
#include "nsd_args.h"

namespace {

constexpr int GATE_NT = 64;                                // lanes that carry a (stream, channel): one wave
constexpr int GATE_BLOCK = 256;                            // threads of a workgroup: that wave and three helpers
constexpr int GATE_ROWS = 128;                             // steps of a stream's circular window of raw samples
constexpr int GATE_WIN = GATE_ROWS + 1;                    // its stride in steps (one of padding)
constexpr int GATE_PAD = PREP_TT + 1;                      // steps per stream in the y / flag tiles (one of padding)
constexpr unsigned F_RAW = 1u, F_FLAT = 2u;                // flags of the parallel phase: raw-bad without the flat test; a flat pair

__device__ __forceinline__ bool finite_f(const float v) { return fabsf(v) < __builtin_inff(); }   // (false for NaN)

// global -> window rows [row0, row0 + nt) / y tile -> global, for the `gl` streams of the group, steps [t0, t0 + nt)
template <bool VEC, bool STORE>
__device__ __forceinline__ void gate_move(const float *src, float *dst, float *lds, const int lstride, const long b0, const int gl,
                                          const int t0, const int nt, const int T, const int C, const int tid) {
    constexpr int W = VEC ? 4 : 1;
    const int nq = nt * C / W;                             // (VEC: T * C and PREP_TT * C are multiples of 4, so every tile's count is)
    const int total = gl * nq;
    for (int idx = tid; idx < total; idx += GATE_BLOCK) {
        const int gi = idx / nq, i = (idx - gi * nq) * W;
        const size_t gofs = ((size_t)(b0 + gi) * T + t0) * C + i;
        float *l = lds + gi * lstride + i;
        if constexpr (STORE) {
            if constexpr (VEC) *reinterpret_cast<float4 *>(dst + gofs) = make_float4(l[0], l[1], l[2], l[3]);
            else dst[gofs] = l[0];
        } else {
            if constexpr (VEC) { const float4 q = *reinterpret_cast<const float4 *>(src + gofs); l[0] = q.x; l[1] = q.y; l[2] = q.z; l[3] = q.w; }
            else l[0] = src[gofs];
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(GATE_BLOCK) void gate_kernel(const GateArgs a) {
    __shared__ __attribute__((aligned(16))) float win[GATE_NT * GATE_WIN];    // [stream][GATE_WIN][C]: raw samples, circular in the step
    __shared__ __attribute__((aligned(16))) float ytile[GATE_NT * GATE_PAD];  // [stream][GATE_PAD][C]
    __shared__ unsigned flag[GATE_NT * GATE_PAD];                             // the same layout: F_* of the element, then its bad bit
    __shared__ unsigned mrow[GATE_NT * GATE_PAD];                             // [stream][GATE_PAD]: the mask word of the step
    __shared__ long slot_s[GATE_NT];                                          // [stream]: its slot, -1: skipped (stream mode)
    __shared__ long long n_s[GATE_NT];                                        // [stream]: samples before this call
    const int C = a.C, T = a.T, tid = threadIdx.x;
    const int G = GATE_NT / C;                             // streams per wave
    const int g = tid < GATE_NT ? tid / C : GATE_NT, ch = tid - g * C;        // (a helper thread carries nothing: g is past every stream)
    const int wstride = GATE_WIN * C, tstride = GATE_PAD * C;
    const float NANF = __builtin_nanf("");
    const long groups = ((long)a.B + G - 1) / G;
    for (long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const long b0 = grp * G, b = b0 + g;
        const int gl = (int)(a.B - b0 < G ? a.B - b0 : G);
        const bool mine = g < gl;                          // this lane carries a (stream, channel) of the call
        // ---- the lane's state: from its slot, or a reset one (window mode) ----
        long slot = b;
        if (mine && a.state && a.slots) slot = a.slots[b];
        const bool skip = mine && a.state && (unsigned long)slot >= (unsigned long)a.S;   // skipped: NaN rows, an all-ones mask
        const bool live = mine && !skip;
        float *sp = a.state && live ? a.state + (size_t)slot * gate_stride(C) : nullptr;
        float held = 0.f;
        int run = 0, hang = 0;
        long long n = 0, nbad = 0, nrej = 0;
        if (sp) {
            held = sp[gate_held(C) + ch];
            run = reinterpret_cast<const int *>(sp)[gate_run(C) + ch];
            hang = reinterpret_cast<const int *>(sp)[gate_hang(C) + ch];
            nbad = reinterpret_cast<const long long *>(sp + gate_bad(C))[ch];
            nrej = *reinterpret_cast<const long long *>(sp + gate_rejected(C));
            n = *reinterpret_cast<const long long *>(sp + gate_steps(C));
        }
        if (mine && ch == 0) { slot_s[g] = skip ? -1 : slot; n_s[g] = n; }
        __syncthreads();
        // ---- window rows 64 - back .. 63: the samples before the call that a test can reach (the previous one, the peak-to-peak
        // span), from the ring; NaN where there is none ----
        const int back = a.pp_samples > 1 ? a.pp_samples - 1 : 1;
        for (int idx = tid; idx < gl * back * C; idx += GATE_BLOCK) {
            const int gi = idx / (back * C), r = idx - gi * back * C, j = GATE_SPAN - back + r / C, c = r % C;
            const long long m = n_s[gi] - GATE_SPAN + j;   // the sample's index in its stream
            float v = NANF;
            if (a.state && slot_s[gi] >= 0 && m >= 0)
                v = a.state[(size_t)slot_s[gi] * gate_stride(C) + gate_ring(C) + (int)(m & (GATE_SPAN - 1)) * C + c];
            win[gi * wstride + j * C + c] = v;
        }
        unsigned *ft = flag + g * tstride + ch;            // this lane's column of its stream's tiles
        float *yt = ytile + g * tstride + ch;
        for (int t0 = 0; t0 < T; t0 += PREP_TT) {
            const int nt = T - t0 < PREP_TT ? T - t0 : PREP_TT;
            const int row0 = (GATE_SPAN + t0) & (GATE_ROWS - 1);               // the tile's first row of the window
            gate_move<VEC, false>(a.x, nullptr, win + row0 * C, wstride, b0, gl, t0, nt, T, C, tid);
            __syncthreads();
            // ---- the tests that are no recurrence, all (stream, step, channel) of the tile in parallel ----
            const int ne = nt * C;
            for (int idx = tid; idx < gl * ne; idx += GATE_BLOCK) {
                const int gi = idx / ne, r = idx - gi * ne, t = r / C, c = r - t * C;
                const float *col = win + gi * wstride + c;
                const int row = row0 + t;
                const float xv = col[row * C], pv = col[((row - 1) & (GATE_ROWS - 1)) * C];
                const bool fx = finite_f(xv), pair = fx && finite_f(pv);
                const float dj = fabsf(__fsub_rn(xv, pv));
                bool raw = !fx;
                if (a.rail > 0.f) raw |= fabsf(xv) >= a.rail;
                if (a.jump > 0.f) raw |= pair && dj >= a.jump;
                if (a.pp_samples > 0) {
                    // (max and min of the finite samples do not depend on the order: eight loads in flight, then the compares)
                    float hi = -__builtin_inff(), lo = __builtin_inff();
                    int k = 0;
                    for (; k + 8 <= a.pp_samples; k += 8) {
                        float v[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) v[u] = col[((row - k - u) & (GATE_ROWS - 1)) * C];
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            const bool f = finite_f(v[u]);
                            hi = f ? fmaxf(hi, v[u]) : hi;
                            lo = f ? fminf(lo, v[u]) : lo;
                        }
                    }
                    for (; k < a.pp_samples; ++k) {
                        const float v = col[((row - k) & (GATE_ROWS - 1)) * C];
                        const bool f = finite_f(v);
                        hi = f ? fmaxf(hi, v) : hi;
                        lo = f ? fminf(lo, v) : lo;
                    }
                    raw |= hi >= lo && __fsub_rn(hi, lo) >= a.pp;
                }
                const bool flat = a.flat_samples > 0 && pair && dj <= a.flat_eps;
                flag[gi * tstride + r] = (raw ? F_RAW : 0u) | (flat ? F_FLAT : 0u);
            }
            __syncthreads();
            // ---- the serial part: nt steps of this lane's channel ----
            if (live) {
                const float *xc = win + g * wstride + row0 * C + ch;
                for (int t = 0; t < nt; ++t) {
                    const unsigned f = ft[t * C];
                    const float xv = xc[t * C];
                    run = (f & F_FLAT) ? (run + 1 < a.flat_samples ? run + 1 : a.flat_samples) : 0;
                    const bool raw = (f & F_RAW) || (a.flat_samples > 0 && run >= a.flat_samples - 1);
                    const bool bad = raw || hang > 0;
                    hang = raw ? a.hold_samples : (hang > 0 ? hang - 1 : 0);
                    held = bad ? held : xv;
                    yt[t * C] = bad ? held : xv;
                    ft[t * C] = bad ? 1u : 0u;
                    nbad += bad ? 1 : 0;
                }
                n += nt;
            } else if (skip) {
                for (int t = 0; t < nt; ++t) { yt[t * C] = NANF; ft[t * C] = 1u; }
            }
            __syncthreads();
            // ---- the mask word of every (stream, step) of the tile; y and the mask go out ----
            for (int idx = tid; idx < gl * nt; idx += GATE_BLOCK) {
                const int gi = idx / nt, t = idx - gi * nt;
                const unsigned *row = flag + gi * tstride + t * C;
                unsigned m = 0u;
                for (int c = 0; c < C; ++c) m |= row[c] << c;
                if (a.state && slot_s[gi] < 0) m = 0xFFFFFFFFu;
                mrow[gi * GATE_PAD + t] = m;
                a.mask[(size_t)(b0 + gi) * T + t0 + t] = m;
            }
            gate_move<VEC, true>(nullptr, a.y, ytile, tstride, b0, gl, t0, nt, T, C, tid);
            __syncthreads();                               // (the next tile is tested into these flags, the next group staged over all)
            if (live && ch == 0)
                for (int t = 0; t < nt; ++t) nrej += __popc(mrow[g * GATE_PAD + t]) > a.max_bad ? 1 : 0;
        }
        // ---- the state: the lane's recurrences and counts, and the last min(T, 64) raw samples into the ring ----
        if (sp) {
            const int last = (GATE_SPAN + T - 1) & (GATE_ROWS - 1);
            sp[GATE_PREV + ch] = win[g * wstride + last * C + ch];
            sp[gate_held(C) + ch] = held;
            reinterpret_cast<int *>(sp)[gate_run(C) + ch] = run;
            reinterpret_cast<int *>(sp)[gate_hang(C) + ch] = hang;
            reinterpret_cast<long long *>(sp + gate_bad(C))[ch] = nbad;
            if (ch == 0) {
                *reinterpret_cast<long long *>(sp + gate_rejected(C)) = nrej;
                *reinterpret_cast<long long *>(sp + gate_steps(C)) = n;
            }
        }
        if (a.state) {
            const int keep = T < GATE_SPAN ? T : GATE_SPAN;
            for (int idx = tid; idx < gl * keep * C; idx += GATE_BLOCK) {
                const int gi = idx / (keep * C), r = idx - gi * keep * C, j = r / C, c = r - j * C;
                if (slot_s[gi] < 0) continue;
                const int t = T - keep + j;                // the call's step
                const long long m = n_s[gi] + t;
                a.state[(size_t)slot_s[gi] * gate_stride(C) + gate_ring(C) + (int)(m & (GATE_SPAN - 1)) * C + c] =
                    win[gi * wstride + ((GATE_SPAN + t) & (GATE_ROWS - 1)) * C + c];
            }
        }
        __syncthreads();                                   // (slot_s, n_s and the window belong to the next group from here)
    }
}

// out = rejected step ? NaN : (bad channel && zero ? 0 : v); W values of one step per thread
template <bool VEC>
__global__ __launch_bounds__(256) void gate_apply_kernel(const GateApplyArgs a) {
    constexpr int W = VEC ? 4 : 1;
    const int C = a.C;
    const long total = a.steps * C / W;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long e = idx * W, s = e / C;
        const int c = (int)(e - s * C);
        const unsigned m = a.mask[s];
        const bool rej = __popc(m) > a.max_bad;
        float v[W];
        if constexpr (VEC) { const float4 q = *reinterpret_cast<const float4 *>(a.v + e); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
        else v[0] = a.v[e];
#pragma unroll
        for (int k = 0; k < W; ++k) v[k] = rej ? __builtin_nanf("") : (a.zero && ((m >> (c + k)) & 1u) ? 0.f : v[k]);
        if constexpr (VEC) *reinterpret_cast<float4 *>(a.out + e) = make_float4(v[0], v[1], v[2], v[3]);
        else a.out[e] = v[0];
    }
}

// a reset slot is all zero
__global__ __launch_bounds__(256) void gate_reset_kernel(float *state, const int stride, const int S, const int32_t *slots, const int n) {
    const int i = blockIdx.x;
    if (i >= n) return;
    const int slot = slots ? slots[i] : i;
    if ((unsigned)slot >= (unsigned)S) return;
    for (int e = threadIdx.x; e < stride; e += 256) state[(size_t)slot * stride + e] = 0.f;
}

}  // namespace

int nsd_gate_launch(const GateArgs &a, hipStream_t st) {
    const int G = GATE_NT / a.C;
    const long groups = ((long)a.B + G - 1) / G;
    const dim3 grid((unsigned)(groups < PREP_GRID_CAP ? groups : PREP_GRID_CAP)), block(GATE_BLOCK);
    const bool vec = ((long)a.T * a.C) % 4 == 0 && ((uintptr_t)a.x | (uintptr_t)a.y) % 16 == 0;
    hipLaunchKernelGGL(vec ? gate_kernel<true> : gate_kernel<false>, grid, block, 0, st, a);
    NSD_CHECK_LAUNCH("gate_step");
    return NSD_OK;
}

int nsd_gate_reset_launch(float *state, int C, int S, const int32_t *slots, int n, hipStream_t st) {
    hipLaunchKernelGGL(gate_reset_kernel, dim3(n), dim3(256), 0, st, state, gate_stride(C), S, slots, n);
    NSD_CHECK_LAUNCH("gate_reset");
    return NSD_OK;
}

int nsd_gate_apply_launch(const GateApplyArgs &a, hipStream_t st) {
    // 4 values of one step per thread where C is a multiple of 4 (a quad never straddles two steps) and the pointers allow it
    const bool vec = a.C % 4 == 0 && ((uintptr_t)a.v | (uintptr_t)a.out) % 16 == 0;
    const long total = a.steps * a.C / (vec ? 4 : 1);
    const long blocks = (total + 255) / 256;
    const dim3 grid((unsigned)(blocks < 4 * PREP_GRID_CAP ? blocks : 4 * PREP_GRID_CAP)), block(256);
    hipLaunchKernelGGL(vec ? gate_apply_kernel<true> : gate_apply_kernel<false>, grid, block, 0, st, a);
    NSD_CHECK_LAUNCH("gate_apply");
    return NSD_OK;
}
