// nsd_align.hip -- session alignment (nsd_cov_* / nsd_whiten_fit / nsd_spatial_apply of include/nsd.h; an extension): the second moment
// of the channels accumulated beside a stream (cov_kernel), its inverse square root formed on the device (whiten_kernel) and the C x C
// matrix applied in front of the model (spatial_kernel).  Cut from the pattern of nsd_gate.hip: tiles of steps go through LDS, what is a
// recurrence runs serially, everything else in parallel.
//
// cov_kernel: one workgroup per stream.  Every (i, j) of the matrix is one serial chain over time in double, so the parallelism is the
// C * C entries (up to four per thread) times the streams, never a split of T: the state after n samples does not depend on the cut.  A
// tile of COV_TT steps is staged into LDS with an odd row stride; the first wave tests one step per lane (all C values finite, mask word
// 0) and its ballot is the tile's `used` word; every thread then walks the tile and adds the exact double product of its two channels
// for the used steps.  In that walk the lanes of a wave read one or two values of i (a broadcast) and consecutive j: no bank conflict.
//
// whiten_kernel: one wave per group.  The group's matrices are summed in registers (16 entries per lane at C = 32) in ascending
// accumulator order, R' is formed in LDS (row stride 33 doubles: lane k's row k falls on its own bank pair), and a cyclic Jacobi
// eigen-solve rotates pair after pair: every lane forms the same (c, s) from three broadcast reads, lanes 0 .. C-1 then update row and
// column k of A, lanes 32 .. 32+C-1 row k of V.  A lane reads and writes only its own row's two elements and the mirror elements of
// rows p and q that no other lane reads, so a rotation has no hazard inside itself; barriers separate the rotations.
//
// spatial_kernel: one workgroup per (row b, tile of SP_TS steps): the row's matrix and the tile are staged into LDS (odd row strides),
// then a thread forms one output -- or four outputs of one step and one 16-byte store where C % 4 == 0 and the pointers allow -- by
// the serial sum over j.  A workgroup reads its whole tile before it writes, and no other workgroup reads it: out == v is safe.
//
// The supervised fit of that matrix (nsd_spatial_bwd / nsd_spatial_fit_step): dv is spatial_kernel with the matrix staged transposed;
// dW is spatial_dw_kernel (cov_kernel's shape over two operands: one serial double chain over t per row and entry) and
// spatial_dw_sum_kernel (a second small launch: one serial double chain over the rows per matrix); spatial_fit_kernel is one Adam step
// per matrix with its counters in the caller's state.
// No atomics, no private segment, vector stores only.
#include "nsd_args.h"

namespace {

constexpr int COV_BLOCK = 256;                             // threads of a workgroup: up to COV_ENT entries of the matrix each
constexpr int COV_ENT = 4;                                 // 4 * 256 = 32 * 32
constexpr int COV_TT = 64;                                 // steps staged at once: one per lane of the testing wave
constexpr int ALIGN_MAXC = 32;
constexpr int ALIGN_LD = ALIGN_MAXC + 1;                   // the widest padded row

__device__ __forceinline__ bool finite_f(const float v) { return fabsf(v) < __builtin_inff(); }   // (false for NaN)
__device__ __forceinline__ bool finite_d(const double v) { return fabs(v) < __builtin_inf(); }

// global [nt][C] at src -> LDS rows of stride CP
template <bool VEC>
__device__ __forceinline__ void stage_rows(const float *src, float *lds, const int nt, const int C, const int CP, const int tid, const int nthreads) {
    constexpr int W = VEC ? 4 : 1;
    const int nq = nt * C / W;                             // (VEC: the caller made sure nt * C is a multiple of 4)
    for (int idx = tid; idx < nq; idx += nthreads) {
        const int e = idx * W;
        if constexpr (VEC) {
            const float4 q = *reinterpret_cast<const float4 *>(src + e);
            const float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) { const int t = (e + u) / C; lds[t * CP + (e + u - t * C)] = v[u]; }
        } else {
            const int t = e / C;
            lds[t * CP + (e - t * C)] = src[e];
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(COV_BLOCK) void cov_kernel(const CovArgs a) {
    __shared__ float tile[COV_TT * ALIGN_LD];              // [COV_TT][CP]
    __shared__ unsigned long long used_s;                  // bit t: step t of the tile is used
    const int C = a.C, T = a.T, tid = threadIdx.x, CC = C * C, CP = C | 1;
    int ei[COV_ENT], ej[COV_ENT];
#pragma unroll
    for (int k = 0; k < COV_ENT; ++k) {
        const int e = tid + k * COV_BLOCK;
        ei[k] = e < CC ? e / C : 0;
        ej[k] = e < CC ? e - ei[k] * C : 0;
    }
    for (long b = blockIdx.x; b < a.B; b += gridDim.x) {
        long slot = b;
        if (a.state && a.slots) slot = a.slots[b];
        if (a.state && (unsigned long)slot >= (unsigned long)a.S) continue;   // (the whole workgroup: nothing is touched)
        double *sp = a.state ? a.state + (size_t)slot * cov_stride(C) : nullptr;
        double acc[COV_ENT];
#pragma unroll
        for (int k = 0; k < COV_ENT; ++k) {
            const int e = tid + k * COV_BLOCK;
            acc[k] = sp && e < CC ? sp[COV_SUM + e] : 0.0;
        }
        long long count = 0, skipped = 0;                  // (thread 0's)
        if (sp && tid == 0) {
            count = reinterpret_cast<const long long *>(sp)[cov_count(C)];
            skipped = reinterpret_cast<const long long *>(sp)[cov_skipped(C)];
        }
        for (int t0 = 0; t0 < T; t0 += COV_TT) {
            const int nt = T - t0 < COV_TT ? T - t0 : COV_TT;
            stage_rows<VEC>(a.v + ((size_t)b * T + t0) * C, tile, nt, C, CP, tid, COV_BLOCK);
            __syncthreads();
            if (tid < 64) {                                // the first wave: one step per lane
                bool u = tid < nt;
                if (u) {
                    const float *row = tile + tid * CP;
                    for (int c = 0; c < C; ++c) u &= finite_f(row[c]);
                    if (a.mask) u &= a.mask[(size_t)b * T + t0 + tid] == 0u;
                }
                const unsigned long long m = __ballot(u);
                if (tid == 0) {
                    used_s = m;
                    const int n = __popcll(m);
                    count += n;
                    skipped += nt - n;
                }
            }
            __syncthreads();
            const unsigned long long um = used_s;
            for (int t = 0; t < nt; ++t) {
                if (!((um >> t) & 1ull)) continue;
                const float *row = tile + t * CP;
#pragma unroll
                for (int k = 0; k < COV_ENT; ++k)
                    if (tid + k * COV_BLOCK < CC) acc[k] = acc[k] + (double)row[ei[k]] * (double)row[ej[k]];
            }
            __syncthreads();                               // (the next tile is staged over this one)
        }
        double *dst = sp ? sp + COV_SUM : a.sums + (size_t)b * CC;
#pragma unroll
        for (int k = 0; k < COV_ENT; ++k) {
            const int e = tid + k * COV_BLOCK;
            if (e < CC) dst[e] = acc[k];
        }
        if (tid == 0) {
            long long *cnt = sp ? reinterpret_cast<long long *>(sp) + cov_count(C) : a.counts + 2 * b;
            cnt[0] = count;
            cnt[1] = skipped;
        }
    }
}

// a reset slot is all zero
__global__ __launch_bounds__(256) void cov_reset_kernel(double *state, const int stride, const int S, const int32_t *slots, const int n) {
    const int i = blockIdx.x;
    if (i >= n) return;
    const int slot = slots ? slots[i] : i;
    if ((unsigned)slot >= (unsigned)S) return;
    for (int e = threadIdx.x; e < stride; e += 256) state[(size_t)slot * stride + e] = 0.0;
}

constexpr int WH_ENT = ALIGN_MAXC * ALIGN_MAXC / 64;       // entries of the matrix per lane

__global__ __launch_bounds__(64) void whiten_kernel(const WhitenArgs a) {
    __shared__ double A[ALIGN_MAXC * ALIGN_LD], V[ALIGN_MAXC * ALIGN_LD];
    __shared__ double dl[ALIGN_MAXC];                      // lambda, then lambda^(-1/2)
    const int g = blockIdx.x, C = a.C, CC = C * C, lane = threadIdx.x;
    // ---- S and n of the group, in ascending accumulator order ----
    double s[WH_ENT];
#pragma unroll
    for (int m = 0; m < WH_ENT; ++m) s[m] = 0.0;
    long long n = 0, skipped = 0;
    int nacc = 0, ignored = 0;
    for (int i = 0; i < a.N; ++i) {
        const int gi = a.group ? a.group[i] : 0;
        if ((unsigned)gi >= (unsigned)a.G) ++ignored;
        if (gi != g) continue;
        const double *src = a.sums + (size_t)i * a.sum_stride;
#pragma unroll
        for (int m = 0; m < WH_ENT; ++m) {
            const int e = lane + 64 * m;
            if (e < CC) s[m] = s[m] + src[e];
        }
        n += a.counts[(size_t)i * a.count_stride];
        skipped += a.counts[(size_t)i * a.count_stride + 1];
        ++nacc;
    }
    bool fin = true;
#pragma unroll
    for (int m = 0; m < WH_ENT; ++m) {
        const int e = lane + 64 * m;
        if (e < CC) { const int i = e / C; A[i * ALIGN_LD + (e - i * C)] = s[m]; fin &= finite_d(s[m]); }
    }
    const bool all_fin = __ballot(!fin) == 0ull;
    __syncthreads();
    double trS = 0.0;
    for (int i = 0; i < C; ++i) trS = trS + A[i * ALIGN_LD + i];
    unsigned status = 0u;
    if (n < a.min_steps) status = NSD_WHITEN_FEW;
    else if (!all_fin || !(trS > 0.0)) status = NSD_WHITEN_NONFINITE;
    double tm = 0.0, lmin = 0.0, lmax = 0.0;
    int sweeps = 0;
    if (!status) {
        // ---- R' = (1 - shrinkage) * S / n + shrinkage * (tr R / C) * I;  V = I ----
        const double dn = (double)n, keep = 1.0 - a.shrinkage;
        __syncthreads();
        for (int e = lane; e < CC; e += 64) {
            const int i = e / C, j = e - i * C;
            A[i * ALIGN_LD + j] = A[i * ALIGN_LD + j] / dn;
            V[i * ALIGN_LD + j] = i == j ? 1.0 : 0.0;
        }
        __syncthreads();
        for (int i = 0; i < C; ++i) tm = tm + A[i * ALIGN_LD + i];
        tm = tm / (double)C;
        __syncthreads();
        for (int e = lane; e < CC; e += 64) {
            const int i = e / C, j = e - i * C;
            const double r = keep * A[i * ALIGN_LD + j];
            A[i * ALIGN_LD + j] = i == j ? r + a.shrinkage * tm : r;
        }
        __syncthreads();
        // ---- cyclic Jacobi: lanes 0 .. C-1 carry row / column k of A, lanes 32 .. 32+C-1 row k of V ----
        const int k = lane & 31;
        const bool isV = lane >= 32;
        double *Mk = (isV ? V : A) + k * ALIGN_LD;
        bool conv = false;
        while (sweeps < NSD_WHITEN_MAX_SWEEPS && !conv) {
            int rotated = 0;
            for (int p = 0; p < C - 1; ++p)
                for (int q = p + 1; q < C; ++q) {
                    const double app = A[p * ALIGN_LD + p], aqq = A[q * ALIGN_LD + q], apq = A[p * ALIGN_LD + q];
                    if (!(fabs(apq) > 0x1p-53 * sqrt(fabs(app * aqq)))) continue;   // (the same for every lane)
                    ++rotated;
                    const double theta = (aqq - app) / (2.0 * apq);
                    const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                    __syncthreads();                       // (every lane holds app, aqq, apq)
                    if (k < C) {
                        if (isV || (k != p && k != q)) {
                            const double mp = Mk[p], mq = Mk[q];
                            const double np_ = c * mp - sn * mq, nq_ = sn * mp + c * mq;
                            Mk[p] = np_;
                            Mk[q] = nq_;
                            if (!isV) { A[p * ALIGN_LD + k] = np_; A[q * ALIGN_LD + k] = nq_; }
                        } else if (k == p) {
                            A[p * ALIGN_LD + p] = app - t * apq;
                            A[p * ALIGN_LD + q] = 0.0;
                            A[q * ALIGN_LD + p] = 0.0;
                        } else {
                            A[q * ALIGN_LD + q] = aqq + t * apq;
                        }
                    }
                    __syncthreads();
                }
            ++sweeps;
            conv = rotated == 0;
        }
        if (!conv) status |= NSD_WHITEN_NOT_CONVERGED;
        // ---- the clip and lambda^(-1/2) ----
        lmin = lmax = A[0];
        for (int i = 1; i < C; ++i) { const double l = A[i * ALIGN_LD + i]; lmin = l < lmin ? l : lmin; lmax = l > lmax ? l : lmax; }
        if (!(lmax > 0.0) || !finite_d(lmax) || !finite_d(lmin)) {
            status = NSD_WHITEN_NONFINITE;                 // (a matrix that was not positive semi-definite to begin with)
        } else {
            const double thr = a.floor * lmax;
            if (lmin < thr) status |= NSD_WHITEN_CLIPPED;
            if (lane < C) { const double l = A[lane * ALIGN_LD + lane]; dl[lane] = 1.0 / sqrt(l < thr ? thr : l); }
        }
        __syncthreads();
    }
    float *W = a.W + (size_t)g * CC;
    if (status & (NSD_WHITEN_FEW | NSD_WHITEN_NONFINITE)) {
        for (int e = lane; e < CC; e += 64) W[e] = e / C == e % C ? 1.f : 0.f;
        tm = lmin = lmax = 0.0;
        sweeps = 0;
    } else {
        // W[i][j] = sum_k (V[i][k] * V[j][k]) * d[k]: the product of the two V's first, so (i, j) and (j, i) are the same bits
        for (int e = lane; e < CC; e += 64) {
            const int i = e / C, j = e - i * C;
            double w = 0.0;
            for (int kk = 0; kk < C; ++kk) w = w + (V[i * ALIGN_LD + kk] * V[j * ALIGN_LD + kk]) * dl[kk];
            W[e] = (float)w;
        }
    }
    if (lane == 0) {
        nsd_whiten_record r;
        r.steps = n; r.skipped = skipped; r.trace_mean = tm; r.eig_min = lmin; r.eig_max = lmax;
        r.sweeps = sweeps; r.status = status; r.accumulators = nacc; r.ignored = ignored; r.reserved = 0;
        a.records[g] = r;
    }
}

constexpr int SP_BLOCK = 256;
constexpr int SP_TS = 64;                                  // steps of a tile

// TR: the matrix is staged transposed -- out[b,t,j] = sum_i W[i][j] * v[b,t,i], the input gradient of the apply (nsd_spatial_bwd's dv)
template <bool VEC, bool TR = false>
__global__ __launch_bounds__(SP_BLOCK) void spatial_kernel(const SpatialArgs a) {
    constexpr int Q = VEC ? 4 : 1;
    __shared__ float wt[ALIGN_MAXC * ALIGN_LD];            // [C][CP]: the row's matrix
    __shared__ float vt[SP_TS * ALIGN_LD];                 // [SP_TS][CP]: the tile's steps
    const int C = a.C, T = a.T, tid = threadIdx.x, CP = C | 1;
    const int tiles = (T + SP_TS - 1) / SP_TS;
    const long units = (long)a.B * tiles;
    for (long u = blockIdx.x; u < units; u += gridDim.x) {
        const long b = u / tiles;
        const int t0 = (int)(u - b * tiles) * SP_TS;
        const int nt = T - t0 < SP_TS ? T - t0 : SP_TS;
        const size_t base = ((size_t)b * T + t0) * C;
        const int m = a.sel ? a.sel[b] : 0;
        const int nq = nt * C / Q;
        if ((unsigned)m >= (unsigned)a.n_mat) {            // (the whole workgroup) a selection outside the table: NaN rows
            const float NANF = __builtin_nanf("");
            for (int idx = tid; idx < nq; idx += SP_BLOCK) {
                if constexpr (VEC) *reinterpret_cast<float4 *>(a.out + base + idx * 4) = make_float4(NANF, NANF, NANF, NANF);
                else a.out[base + idx] = NANF;
            }
            continue;
        }
        if constexpr (TR) {
            const float *Wm = a.W + (size_t)m * C * C;
            for (int e = tid; e < C * C; e += SP_BLOCK) { const int i = e / C, j = e - i * C; wt[j * CP + i] = Wm[e]; }
        } else {
            stage_rows<false>(a.W + (size_t)m * C * C, wt, C, C, CP, tid, SP_BLOCK);
        }
        stage_rows<VEC>(a.v + base, vt, nt, C, CP, tid, SP_BLOCK);
        __syncthreads();
        for (int idx = tid; idx < nq; idx += SP_BLOCK) {
            const int e = idx * Q, s = e / C, i0 = e - s * C;
            const float *vr = vt + s * CP, *wr = wt + i0 * CP;
            float acc[Q];
#pragma unroll
            for (int k = 0; k < Q; ++k) acc[k] = __fmul_rn(wr[k * CP], vr[0]);
            for (int j = 1; j < C; ++j) {
                const float vv = vr[j];
#pragma unroll
                for (int k = 0; k < Q; ++k) acc[k] = __fadd_rn(acc[k], __fmul_rn(wr[k * CP + j], vv));
            }
            if constexpr (VEC) *reinterpret_cast<float4 *>(a.out + base + e) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            else a.out[base + e] = acc[0];
        }
        __syncthreads();                                   // (the next unit is staged over both tiles)
    }
}

// ---- nsd_spatial_bwd's dW, stage 1: p[b][i][j] = the serial chain over t of (double)dy[b,t,i] * (double)v[b,t,j].  cov_kernel's shape: one
// workgroup per row, tiles of DW_TT steps of both operands through LDS, up to COV_ENT entries per thread.  Nothing is masked: a
// non-finite value reaches the entries of its row and column.  A row whose selection lies outside the table is skipped whole (stage 2
// never reads its p).
constexpr int DW_UN = 8;                                   // steps whose operands are in flight at once
constexpr int DW_TT = 128;                                 // steps staged at once (two operands: 33 KB of LDS)
// NE: the entries a thread walks, 1 up to C = 16 (C * C <= COV_BLOCK), else COV_ENT -- a compile-time count keeps the walk free of branches
template <bool VEC, int NE>
__global__ __launch_bounds__(COV_BLOCK) void spatial_dw_kernel(const SpatialBwdArgs a) {
    __shared__ float yt[DW_TT * ALIGN_LD], xt[DW_TT * ALIGN_LD];   // [DW_TT][CP]: dy and v
    const int C = a.C, T = a.T, tid = threadIdx.x, CC = C * C, CP = C | 1;
    int ei[COV_ENT], ej[COV_ENT];
#pragma unroll
    for (int k = 0; k < COV_ENT; ++k) {
        const int e = tid + k * COV_BLOCK;
        ei[k] = e < CC ? e / C : 0;
        ej[k] = e < CC ? e - ei[k] * C : 0;
    }
    for (long b = blockIdx.x; b < a.B; b += gridDim.x) {
        const int m = a.sel ? a.sel[b] : 0;
        if ((unsigned)m >= (unsigned)a.n_mat) continue;    // (the whole workgroup)
        double acc[COV_ENT];
#pragma unroll
        for (int k = 0; k < COV_ENT; ++k) acc[k] = 0.0;
        for (int t0 = 0; t0 < T; t0 += DW_TT) {
            const int nt = T - t0 < DW_TT ? T - t0 : DW_TT;
            const size_t base = ((size_t)b * T + t0) * C;
            stage_rows<VEC>(a.dy + base, yt, nt, C, CP, tid, COV_BLOCK);
            stage_rows<VEC>(a.v + base, xt, nt, C, CP, tid, COV_BLOCK);
            __syncthreads();
            // the chain is serial, its operands are not: DW_UN steps' LDS reads are issued before their DW_UN dependent additions
            // (an entry beyond C * C reads (0, 0) and is never stored; a whole wave beyond it skips the walk)
            if (tid - (tid & 63) < CC) {
                int t = 0;
                for (; t + DW_UN <= nt; t += DW_UN) {
                    float yv[DW_UN][NE], xv[DW_UN][NE];
#pragma unroll
                    for (int u = 0; u < DW_UN; ++u)
#pragma unroll
                        for (int k = 0; k < NE; ++k) { yv[u][k] = yt[(t + u) * CP + ei[k]]; xv[u][k] = xt[(t + u) * CP + ej[k]]; }
#pragma unroll
                    for (int u = 0; u < DW_UN; ++u)
#pragma unroll
                        for (int k = 0; k < NE; ++k) acc[k] = acc[k] + (double)yv[u][k] * (double)xv[u][k];
                }
                for (; t < nt; ++t) {
                    const float *yr = yt + t * CP, *xr = xt + t * CP;
#pragma unroll
                    for (int k = 0; k < NE; ++k) acc[k] = acc[k] + (double)yr[ei[k]] * (double)xr[ej[k]];
                }
            }
            __syncthreads();                               // (the next tile is staged over this one)
        }
        double *dst = a.p + (size_t)b * CC;
#pragma unroll
        for (int k = 0; k < COV_ENT; ++k) {
            const int e = tid + k * COV_BLOCK;
            if (e < CC) dst[e] = acc[k];
        }
    }
}

// stage 2, a second launch behind stage 1 on the stream: one workgroup per matrix sums the p of its rows in ascending b, in double, and
// rounds once.  Workgroup 0 also counts the rows.
__global__ __launch_bounds__(COV_BLOCK) void spatial_dw_sum_kernel(const SpatialBwdArgs a) {
    const int m = blockIdx.x, CC = a.C * a.C, tid = threadIdx.x;
    double acc[COV_ENT];
#pragma unroll
    for (int k = 0; k < COV_ENT; ++k) acc[k] = 0.0;
    long long used = 0, left = 0;
    for (int b = 0; b < a.B; ++b) {
        const int mb = a.sel ? a.sel[b] : 0;
        if ((unsigned)mb >= (unsigned)a.n_mat) { ++left; continue; }
        ++used;
        if (mb != m) continue;
        const double *src = a.p + (size_t)b * CC;
#pragma unroll
        for (int k = 0; k < COV_ENT; ++k) {
            const int e = tid + k * COV_BLOCK;
            if (e < CC) acc[k] = acc[k] + src[e];
        }
    }
    float *dst = a.dW + (size_t)m * CC;
#pragma unroll
    for (int k = 0; k < COV_ENT; ++k) {
        const int e = tid + k * COV_BLOCK;
        if (e < CC) dst[e] = (float)acc[k];
    }
    if (m == 0 && tid == 0 && a.counts) { a.counts[0] = used; a.counts[1] = left; }
}

// b^s by squaring: the same products on the host restatement (pow() differs from libm's in the last place)
__device__ __forceinline__ double sfit_pow(double b, long long s) {
    double r = 1.0;
    while (s) { if (s & 1) r *= b; b *= b; s >>= 1; }
    return r;
}

// ---- nsd_spatial_fit_step: one workgroup per matrix, up to COV_ENT entries per thread.  g = dW + decay * (A - A0), tested whole; a
// matrix with a g that is not finite only records it.  The update is adam_kernel's arithmetic in its order (weight decay 0, scale 1),
// the bias corrections formed in double from the slot's own counter, which advances here: the call replays from a graph.
__global__ __launch_bounds__(COV_BLOCK) void spatial_fit_kernel(const SpatialFitArgs a) {
    const int m = blockIdx.x, C = a.C, CC = C * C, tid = threadIdx.x;
    unsigned char *slot = a.state + (size_t)m * sfit_stride(C);
    float *mom = reinterpret_cast<float *>(slot + sfit_m(C)), *var = reinterpret_cast<float *>(slot + sfit_v(C));
    long long *step = reinterpret_cast<long long *>(slot + sfit_step(C)), *skipped = reinterpret_cast<long long *>(slot + sfit_skipped(C));
    unsigned *status = reinterpret_cast<unsigned *>(slot + sfit_status(C));
    if (m == 0 && tid == 0) {                              // the loss of this call, by the call counter behind the last slot
        long long *calls = reinterpret_cast<long long *>(a.state + (size_t)a.n_mat * sfit_stride(C));
        const long long n = calls[0];
        if (a.loss_in && n >= 0 && n < (long long)a.loss_cap) a.loss_out[n] = a.loss_in[0];   // (n < 0: a state nobody reset)
        calls[0] = n + 1;
    }
    float *A = a.A + (size_t)m * CC;
    float g[COV_ENT], pi[COV_ENT];
    bool fin = true;
#pragma unroll
    for (int k = 0; k < COV_ENT; ++k) {
        const int e = tid + k * COV_BLOCK;
        g[k] = pi[k] = 0.f;
        if (e < CC) {
            pi[k] = A[e];
            const float d = a.dW[(size_t)m * CC + e];
            g[k] = a.A0 ? __fadd_rn(d, __fmul_rn(a.decay, __fsub_rn(pi[k], a.A0[(size_t)m * CC + e]))) : d;
            fin &= finite_f(g[k]);
        }
    }
    const long long s = step[0];                           // (read by every thread above the barrier, written by thread 0 below it)
    const bool bad = __syncthreads_or(!fin) != 0;
    if (bad) {
        if (tid == 0) { status[0] |= NSD_SPATIAL_FIT_NONFINITE; skipped[0] += 1; }
        return;
    }
    const double bc1 = 1.0 - sfit_pow((double)a.b1, s + 1), bc2 = 1.0 - sfit_pow((double)a.b2, s + 1);
    const float lr_over_bc1 = (float)((double)a.lr / bc1), rsqrt_bc2 = (float)(1.0 / sqrt(bc2));
#pragma unroll
    for (int k = 0; k < COV_ENT; ++k) {
        const int e = tid + k * COV_BLOCK;
        if (e < CC) {
            const float gi = g[k];
            const float mi = a.b1 * mom[e] + (1.f - a.b1) * gi;
            const float vi = a.b2 * var[e] + (1.f - a.b2) * gi * gi;
            mom[e] = mi; var[e] = vi;
            const float denom = sqrtf(vi) * rsqrt_bc2 + a.eps;
            A[e] = pi[k] - lr_over_bc1 * (mi / denom);
        }
    }
    if (tid == 0) step[0] = s + 1;
}

}  // namespace

int nsd_spatial_bwd_launch(const SpatialBwdArgs &a, hipStream_t st) {
    if (a.dv && a.B > 0) {                                 // the apply's kernel on dy with the matrix transposed
        SpatialArgs s;
        s.v = a.dy; s.W = a.W; s.sel = a.sel; s.out = a.dv; s.B = a.B; s.T = a.T; s.C = a.C; s.n_mat = a.n_mat;
        const bool vec = a.C % 4 == 0 && ((uintptr_t)a.dy | (uintptr_t)a.dv) % 16 == 0;
        const long units = (long)a.B * ((a.T + SP_TS - 1) / SP_TS);
        const dim3 grid((unsigned)(units < 4 * PREP_GRID_CAP ? units : 4 * PREP_GRID_CAP)), block(SP_BLOCK);
        if (vec) hipLaunchKernelGGL((spatial_kernel<true, true>), grid, block, 0, st, s);
        else hipLaunchKernelGGL((spatial_kernel<false, true>), grid, block, 0, st, s);
        NSD_CHECK_LAUNCH("spatial_bwd (dv)");
    }
    if (a.dW) {
        if (a.B > 0) {
            const dim3 grid((unsigned)(a.B < PREP_GRID_CAP ? a.B : PREP_GRID_CAP)), block(COV_BLOCK);
            const bool vec = ((long)a.T * a.C) % 4 == 0 && ((uintptr_t)a.v | (uintptr_t)a.dy) % 16 == 0;
            const bool one = a.C * a.C <= COV_BLOCK;
            hipLaunchKernelGGL(vec ? (one ? spatial_dw_kernel<true, 1> : spatial_dw_kernel<true, COV_ENT>)
                                   : (one ? spatial_dw_kernel<false, 1> : spatial_dw_kernel<false, COV_ENT>), grid, block, 0, st, a);
            NSD_CHECK_LAUNCH("spatial_bwd (dW, stage 1)");
        }
        hipLaunchKernelGGL(spatial_dw_sum_kernel, dim3(a.n_mat), dim3(COV_BLOCK), 0, st, a);
        NSD_CHECK_LAUNCH("spatial_bwd (dW, stage 2)");
    }
    return NSD_OK;
}

int nsd_spatial_fit_launch(const SpatialFitArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(spatial_fit_kernel, dim3(a.n_mat), dim3(COV_BLOCK), 0, st, a);
    NSD_CHECK_LAUNCH("spatial_fit_step");
    return NSD_OK;
}

int nsd_cov_launch(const CovArgs &a, hipStream_t st) {
    const dim3 grid((unsigned)(a.B < PREP_GRID_CAP ? a.B : PREP_GRID_CAP)), block(COV_BLOCK);
    // 16 bytes per lane where every tile of every stream starts on a 16-byte boundary (COV_TT * C is a multiple of 4)
    const bool vec = ((long)a.T * a.C) % 4 == 0 && (uintptr_t)a.v % 16 == 0;
    hipLaunchKernelGGL(vec ? cov_kernel<true> : cov_kernel<false>, grid, block, 0, st, a);
    NSD_CHECK_LAUNCH("cov_step");
    return NSD_OK;
}

int nsd_cov_reset_launch(double *state, int C, int S, const int32_t *slots, int n, hipStream_t st) {
    hipLaunchKernelGGL(cov_reset_kernel, dim3(n), dim3(256), 0, st, state, cov_stride(C), S, slots, n);
    NSD_CHECK_LAUNCH("cov_reset");
    return NSD_OK;
}

int nsd_whiten_launch(const WhitenArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(whiten_kernel, dim3(a.G), dim3(64), 0, st, a);
    NSD_CHECK_LAUNCH("whiten_fit");
    return NSD_OK;
}

int nsd_spatial_launch(const SpatialArgs &a, hipStream_t st) {
    // 4 outputs of one step per thread where C is a multiple of 4 (a quad never straddles two steps) and the pointers allow it
    const bool vec = a.C % 4 == 0 && ((uintptr_t)a.v | (uintptr_t)a.out) % 16 == 0;
    const long units = (long)a.B * ((a.T + SP_TS - 1) / SP_TS);
    const dim3 grid((unsigned)(units < 4 * PREP_GRID_CAP ? units : 4 * PREP_GRID_CAP)), block(SP_BLOCK);
    hipLaunchKernelGGL(vec ? spatial_kernel<true> : spatial_kernel<false>, grid, block, 0, st, a);
    NSD_CHECK_LAUNCH("spatial_apply");
    return NSD_OK;
}
