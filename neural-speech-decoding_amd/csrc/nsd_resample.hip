// nsd_resample.hip -- rate conversion, stage 0 of the front end (nsd_resample_* of include/nsd.h; an extension, the reference's board
// and trials run at the models' 125 Hz): a causal rational-ratio polyphase FIR, out / in rate = L / M, P taps per phase, with the last
// P - 1 samples of a stream carried from chunk to chunk in a caller-owned slot, as nsd_prep_step carries its filters'.  Window mode (no
// state) runs whole trials from rest: what the trainers and predict use.
//
// An FIR output depends on inputs alone, so the parallel unit is an output element (j, c), not a serial chain.  A workgroup stages RS_TI
// input samples of one stream and the P - 1 in front of them -- the slot's history at the stream's first samples, zeros in window mode --
// through LDS with coalesced loads (16 bytes per lane where T*C and the pointer allow it, dwords otherwise), then every thread forms
// outputs of the tile: the P products of one output in ascending tap order, each an explicit _rn multiply and _rn add, so an output is
// bit for bit a function of the samples whatever tile, chunk or slot it falls in.  Where C is a multiple of 4 (and y is 16-byte aligned)
// a thread forms the four neighbouring channels of one j: one tap read (the lanes of one j share the address), one 16-byte LDS read,
// four independent chains, one 16-byte store; elsewhere a thread forms one element and stores a dword.  The taps of a phase are
// contiguous; the table lives in LDS up to RS_TAPS_LDS floats (every decimator: L = 1, P <= 256) and is read through the caches beyond.
//
// Stream mode gives a slot to ONE workgroup, which walks the chunk's tiles in order: every read of hist / n_in -- n_in at the top, hist
// while a tile is staged, the rows that stay when the chunk is shorter than the history -- precedes the barrier behind which the new
// hist and n_in are written.  Window mode has no state and spreads (trial, tile) units over the grid.
#include "nsd_args.h"

namespace {

constexpr int RS_BLOCK = 256;
constexpr int RS_PAD = 4;                                  // floats in front of and behind the staged rows: an aligned 16-byte load may
                                                           // start up to 3 floats early and end up to 3 late
__host__ __device__ constexpr int rs_rows(int T, int P) { return P - 1 + (T < RS_TI ? T : RS_TI); }
__host__ __device__ constexpr int rs_x_floats(int T, int C, int P) { return (RS_PAD + rs_rows(T, P) * C + RS_PAD + 3) & ~3; }

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }

template <bool VECIN, bool QUAD, bool TLDS>
__global__ __launch_bounds__(RS_BLOCK) void resample_kernel(const ResampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) float rl[];
    const int C = a.C, T = a.T, L = a.L, M = a.M, P = a.P, H = a.P - 1, tid = threadIdx.x;
    float *xs = rl + RS_PAD;                               // xs[r * C + c]: row r of the tile is sample t0 - H + r of the chunk
    const float *tp = a.taps;
    if constexpr (TLDS) {
        float *tl = rl + rs_x_floats(T, C, P);
        for (int i = tid; i < L * P; i += RS_BLOCK) tl[i] = a.taps[i];
        tp = tl;                                           // (first read behind the first tile's barrier)
    }
    const float nan = __builtin_nanf("");
    const int tiles = (T + RS_TI - 1) / RS_TI;
    const int tpu = a.state ? tiles : 1;                   // tiles of a work unit: a stream's slot has one owner
    const long long units = a.state ? (long long)a.B : (long long)a.B * tiles;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const long long b = a.state ? u : u / tiles;
        const int k0 = a.state ? 0 : (int)(u - b * tiles);
        long long slot = b;
        if (a.state && a.slots) slot = a.slots[b];
        bool bad = a.state && (unsigned long long)slot >= (unsigned long long)a.S;
        float *sp = a.state && !bad ? a.state + (size_t)slot * rs_stride(C, P) : nullptr;
        long long n0 = sp ? *reinterpret_cast<const long long *>(sp + rs_n_in(C, P)) : 0;
        if (n0 < 0 || n0 > RS_MAX_N_IN) { bad = true; sp = nullptr; n0 = 0; }
        const long long j0 = rs_ceil_div(n0 * L, M);
        const long long cntb = bad ? 0 : rs_ceil_div((n0 + T) * L, M) - j0;
        const float *xb = a.x + (size_t)b * T * C;
        float *yb = a.y + (size_t)b * a.To * C;
        if (k0 == 0) {
            // ---- behind the row's outputs: NaN ----
            const long long lo = cntb * C, hi = a.To * C;
            if constexpr (QUAD) {
                for (long long e = lo + 4 * tid; e < hi; e += 4 * RS_BLOCK) *reinterpret_cast<float4 *>(yb + e) = make_float4(nan, nan, nan, nan);
            } else {
                for (long long e = lo + tid; e < hi; e += RS_BLOCK) yb[e] = nan;
            }
            if (tid == 0 && a.cnt) a.cnt[b] = (int32_t)cntb;
        }
        if (bad) continue;                                 // (uniform over the workgroup)
        for (int k = k0; k < k0 + tpu; ++k) {
            const int t0 = k * RS_TI, nt = T - t0 < RS_TI ? T - t0 : RS_TI;
            // ---- stage rows [0, H + nt): samples t0 - H .. t0 + nt - 1; the ones before the chunk from hist (or rest) ----
            const int nA = H > t0 ? H - t0 : 0;            // rows before the chunk: hist rows t0 .. H - 1
            for (int i = tid; i < nA * C; i += RS_BLOCK) xs[i] = sp ? sp[RS_HIST + t0 * C + i] : 0.f;
            const int s_lo = t0 > H ? t0 - H : 0;          // first sample of the chunk in the tile, at row nA
            const int g_lo = s_lo * C, g_hi = (t0 + nt) * C;
            float *xl = xs + nA * C - g_lo;                // element e of the chunk's row-major [T][C] sits at xl[e]
            if constexpr (VECIN) {
                for (int e = (g_lo & ~3) + 4 * tid; e < g_hi; e += 4 * RS_BLOCK) {      // (g_lo is aligned unless s_lo > 0, where nA = 0:
                    const float4 q = ld4(xb + e);                                      // the early floats land in the front padding)
                    xl[e] = q.x; xl[e + 1] = q.y; xl[e + 2] = q.z; xl[e + 3] = q.w;
                }
            } else {
                for (int e = g_lo + tid; e < g_hi; e += RS_BLOCK) xl[e] = xb[e];
            }
            __syncthreads();
            // ---- the tile's outputs: q in [n0 + t0, n0 + t0 + nt) ----
            const long long jl = rs_ceil_div((n0 + t0) * L, M), jh = rs_ceil_div((n0 + t0 + nt) * L, M);
            const long long nel = (jh - jl) * C;
            constexpr int W = QUAD ? 4 : 1;
            for (long long e = (long long)W * tid; e < nel; e += W * RS_BLOCK) {
                const long long jj = e / C;
                const int c = (int)(e - jj * C);
                const long long j = jl + jj, p = j * M, q = p / L;
                const int ph = (int)(p - q * L);
                const float *xr = xs + (H + (int)(q - n0) - t0) * C + c;   // xa[q], channel c; xa[q - i] is i rows up
                const float *tr = tp + ph * P;
                float *yo = yb + (j - j0) * C + c;
                if constexpr (QUAD) {
                    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
                    for (int i = 0; i < P; ++i) {
                        const float w = tr[i];
                        const float4 v = ld4(xr - i * C);
                        acc.x = __fadd_rn(acc.x, __fmul_rn(w, v.x)); acc.y = __fadd_rn(acc.y, __fmul_rn(w, v.y));
                        acc.z = __fadd_rn(acc.z, __fmul_rn(w, v.z)); acc.w = __fadd_rn(acc.w, __fmul_rn(w, v.w));
                    }
                    *reinterpret_cast<float4 *>(yo) = acc;
                } else {
                    float acc = 0.f;
#pragma unroll 4
                    for (int i = 0; i < P; ++i) acc = __fadd_rn(acc, __fmul_rn(tr[i], xr[-i * C]));
                    *yo = acc;
                }
            }
            __syncthreads();                               // (the next tile, or the next unit, is staged over this one)
        }
        if (sp) {
            // ---- the slot's new history: the last H samples of (old history, chunk).  Rows of the old one that stay go through LDS:
            // every read of the slot precedes the barrier, every write follows it ----
            const int keep = H > T ? H - T : 0;            // old rows [T, H) become rows [0, keep)
            for (int i = tid; i < keep * C; i += RS_BLOCK) xs[i] = sp[RS_HIST + T * C + i];
            __syncthreads();
            for (int i = tid; i < keep * C; i += RS_BLOCK) sp[RS_HIST + i] = xs[i];
            const float *src = xb + (size_t)(T > H ? T - H : 0) * C;
            for (int i = tid; i < (H - keep) * C; i += RS_BLOCK) sp[RS_HIST + keep * C + i] = src[i];
            if (tid == 0) *reinterpret_cast<long long *>(sp + rs_n_in(C, P)) = n0 + T;
            __syncthreads();                               // (the next unit stages over xs)
        }
    }
}

// a reset slot is all zero: a silent history, no samples yet
__global__ __launch_bounds__(256) void resample_reset_kernel(float *state, const int stride, const int S, const int32_t *slots, const int n) {
    const int i = blockIdx.x;
    if (i >= n) return;
    const int slot = slots ? slots[i] : i;
    if ((unsigned)slot >= (unsigned)S) return;
    for (int e = threadIdx.x; e < stride; e += 256) state[(size_t)slot * stride + e] = 0.f;
}

}  // namespace

int nsd_resample_launch(const ResampleArgs &a, hipStream_t st) {
    const int tiles = (a.T + RS_TI - 1) / RS_TI;
    const long long units = a.state ? (long long)a.B : (long long)a.B * tiles;
    const dim3 grid((unsigned)(units < RS_GRID_CAP ? units : RS_GRID_CAP)), block(RS_BLOCK);
    const bool vecin = ((long long)a.T * a.C) % 4 == 0 && (uintptr_t)a.x % 16 == 0;
    const bool quad = a.C % 4 == 0 && (uintptr_t)a.y % 16 == 0;
    const bool tlds = a.L * a.P <= RS_TAPS_LDS;
    const size_t lds = ((size_t)rs_x_floats(a.T, a.C, a.P) + (tlds ? (size_t)a.L * a.P : 0)) * sizeof(float);
    using kernel_t = void (*)(ResampleArgs);
#define RS_K(V, Q) {resample_kernel<V, Q, false>, resample_kernel<V, Q, true>}
    static const kernel_t table[2][2][2] = {{RS_K(false, false), RS_K(false, true)}, {RS_K(true, false), RS_K(true, true)}};
#undef RS_K
    const kernel_t kernel = table[vecin ? 1 : 0][quad ? 1 : 0][tlds ? 1 : 0];
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kernel, grid, block, lds, st, a);
    NSD_CHECK_LAUNCH("resample_step");
    return NSD_OK;
}

int nsd_resample_reset_launch(float *state, int stride, int S, const int32_t *slots, int n, hipStream_t st) {
    hipLaunchKernelGGL(resample_reset_kernel, dim3(n), dim3(256), 0, st, state, stride, S, slots, n);
    NSD_CHECK_LAUNCH("resample_reset");
    return NSD_OK;
}
