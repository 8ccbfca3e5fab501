// nsd_optim.hip -- global-norm gradient clipping and learning-rate schedules in the step tail (nsd_opt of include/nsd.h).
//
// The clipped tail is TWO launches with no signalling between workgroups:
//   1. a reduction that also leaves, per workgroup, the double sum of its squared scaled gradients (reduce_norm_kernel for the slabs of the
//      fused tail, norm_flat_kernel for a flat vector) in the scratch part of opt_state;
//   2. adam_clip_kernel, the one update kernel of every route: each workgroup first sums those partials in the same fixed order (the
//      sums, and with them the skip decision, are identical in every workgroup), forms coef, the schedule factor and the bias
//      corrections in double, then updates its elements; workgroup 0 of a model writes the model's record.
// A ticket counter whose last reduction workgroup finishes the update alone was weighed and not built.
// Weight averaging (nsd_avg of include/nsd.h) rides in launch 2: adam_clip_avg_kernel is the same update body with the averaged row formed
// in the iteration that stores p[i].  Every workgroup of a model reads n_avg before it works and then adds 1 to `arrive`; the one that
// sees gridDim.x - 1 is the last and alone writes n_avg + 1 and arrive = 0.  Nobody waits.  All four accesses are relaxed device-scope
// atomics and there is NO device-scope fence per workgroup: no workgroup publishes data to another inside the launch, the only order
// needed is "my read of n_avg, then my arrival", and thread 0 holds the read's value (it has handed it round through LDS, behind a
// barrier) before it issues the add.  A __threadfence() in front of every add was measured at +72 us on the update of 25 models (an L2
// write-back per workgroup), and 3125 arrivals on one cache line at +16 us, hence the smaller grid (profiles/weight_averaging.md).
#include <math.h>
#include <float.h>
#include <string.h>
#include <type_traits>
#include "nsd_args.h"

// ---- schedule factor f(s), double: the same expression on the host (nsd_lr_factor, host-step launches) and on the device (step_dev) ----
__host__ __device__ static inline double lr_factor_of(int sched, int W, int total, int step_size, float min_ratio, float gamma, long long s) {
    const long long e = s - 1;
    if (e < W) return (double)(e + 1) / (double)W;
    const long long ep = e - W;
    if (sched == NSD_SCHED_COSINE) {
        const long long np = (long long)total - W;
        const double r = (double)min_ratio;
        const long long q = ep < np ? ep : np;
        return r + (1.0 - r) * 0.5 * (1.0 + cos(3.14159265358979323846 * (double)q / (double)np));
    }
    if (sched == NSD_SCHED_STEP) return pow((double)gamma, (double)(ep / step_size));
    return 1.0;
}

// nsd_opt's fields: 0, or the NSD_E_INVALID refusal with the field named (who: the entry point)
int nsd_opt_check(const nsd_opt *o, const char *who) {
    if (!o) { nsd_set_error("%s: opt is NULL", who); return NSD_E_INVALID; }
    if (!(o->max_norm >= 0.f)) { nsd_set_error("%s: max_norm %g negative or NaN", who, o->max_norm); return NSD_E_INVALID; }
    if (o->sched != NSD_SCHED_CONSTANT && o->sched != NSD_SCHED_COSINE && o->sched != NSD_SCHED_STEP) {
        nsd_set_error("%s: sched %d unknown (NSD_SCHED_CONSTANT / _COSINE / _STEP)", who, o->sched); return NSD_E_INVALID;
    }
    if (o->warmup_steps < 0) { nsd_set_error("%s: warmup_steps %d negative", who, o->warmup_steps); return NSD_E_INVALID; }
    if (o->sched == NSD_SCHED_COSINE && o->total_steps <= o->warmup_steps) {
        nsd_set_error("%s: total_steps %d must exceed warmup_steps %d for the cosine schedule", who, o->total_steps, o->warmup_steps); return NSD_E_INVALID;
    }
    if (o->step_size < 1) { nsd_set_error("%s: step_size %d must be >= 1", who, o->step_size); return NSD_E_INVALID; }
    if (!(o->gamma > 0.f && o->gamma <= 1.f)) { nsd_set_error("%s: gamma %g outside (0, 1]", who, o->gamma); return NSD_E_INVALID; }
    if (!(o->min_ratio >= 0.f && o->min_ratio <= 1.f)) { nsd_set_error("%s: min_ratio %g outside [0, 1]", who, o->min_ratio); return NSD_E_INVALID; }
    return NSD_OK;
}

double nsd_lr_factor_host(const nsd_opt *o, long long step) {
    return lr_factor_of(o->sched, o->warmup_steps, o->total_steps, o->step_size, o->min_ratio, o->gamma, step);
}

// ---- opt_state: M records, then per model the workgroups' partial sums (doubles) ------------------------------------------------------
// fused tail: one partial per 32 columns; flat route: one per workgroup of norm_flat_kernel (never more than that: 256 >= 32)
constexpr int ON_COLS = 32, ON_GROUPS = 8, ON_UNROLL = 8;     // the tiling of grad_reduce_kernel (nsd_misc.hip), whose sums these must equal
constexpr int FLAT_NT = 256, FLAT_MAX_PARTS = 2048;
static inline long col_parts(long P) { return (P + ON_COLS - 1) / ON_COLS; }
static inline long flat_parts(long n) { const long b = (n + FLAT_NT - 1) / FLAT_NT; return b < FLAT_MAX_PARTS ? b : FLAT_MAX_PARTS; }
int64_t nsd_opt_state_need(int64_t n, int M) { return (int64_t)M * (int64_t)sizeof(nsd_opt_record) + (int64_t)M * col_parts(n) * (int64_t)sizeof(double); }
static inline double *parts_of(void *state, int M) { return reinterpret_cast<double *>(static_cast<char *>(state) + (size_t)M * sizeof(nsd_opt_record)); }

__global__ void opt_state_init_kernel(uint32_t *w, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) w[i] = 0u;
}
int nsd_opt_state_init_launch(void *state, int64_t bytes, hipStream_t st) {
    const long words = (long)(bytes / 4);
    if (words <= 0) return NSD_OK;
    long blocks = (words + 255) / 256; if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(opt_state_init_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (uint32_t *)state, words);
    NSD_CHECK_LAUNCH("opt_state_init");
    return NSD_OK;
}

// ---- launch 1, fused tail: grad_reduce_kernel's column sums (same tiling, same association order: grads is nsd_grad_reduce's bit for
// bit) and the workgroup's double sum of (fp32(grads[e] * gscale))^2, lanes in order; lanes past P add exactly 0 ----------------------
// gscale: one float, or for M models one per model by value in the launch arguments (nsd_opt::grad_scale of each model's entry; the
// uniform entry point fills M equal ones): blockIdx.y is workgroup-uniform, so model mo's is a scalar load from the kernel arguments
template <bool MODELS> struct GScale { float g; __device__ __forceinline__ float of(long) const { return g; } };
template <> struct GScale<true> { float g[NSD_MAX_MODELS]; __device__ __forceinline__ float of(long mo) const { return g[mo]; } };
template <bool MODELS>
__global__ __launch_bounds__(ON_COLS * ON_GROUPS) void reduce_norm_kernel(
        const float *slabs, long slab_stride, int n_slabs, long p_lstm, const float *hslabs, long ph, int n_hslabs,
        float *grads, GScale<MODELS> gs, double *parts) {
    const float gscale = gs.of(MODELS ? (long)blockIdx.y : 0);
    if constexpr (MODELS) {
        const long mo = blockIdx.y;
        slabs += mo * n_slabs * slab_stride; hslabs += mo * n_hslabs * ph; grads += mo * (p_lstm + ph);
        parts += mo * gridDim.x;
    }
    __shared__ float part[ON_GROUPS][ON_COLS];
    __shared__ double sq[ON_COLS];
    const int c = threadIdx.x & (ON_COLS - 1), grp = threadIdx.x / ON_COLS;
    const long e = (long)blockIdx.x * ON_COLS + c;
    float s0 = 0.f;
    if (e < p_lstm + ph) {
        const float *p; long stride; int n;
        if (e < p_lstm) { p = slabs + e; stride = slab_stride; n = n_slabs; }
        else { p = hslabs + (e - p_lstm); stride = ph; n = n_hslabs; }
        int q = grp;
        float acc[ON_UNROLL];
#pragma unroll
        for (int u = 0; u < ON_UNROLL; ++u) acc[u] = 0.f;
        for (; q + (ON_UNROLL - 1) * ON_GROUPS < n; q += ON_UNROLL * ON_GROUPS) {
            float vload[ON_UNROLL];
#pragma unroll
            for (int u = 0; u < ON_UNROLL; ++u) vload[u] = p[(size_t)(q + u * ON_GROUPS) * stride];
#pragma unroll
            for (int u = 0; u < ON_UNROLL; ++u) acc[u] += vload[u];
        }
        for (; q < n; q += ON_GROUPS) acc[0] += p[(size_t)q * stride];
#pragma unroll
        for (int w = ON_UNROLL / 2; w >= 1; w >>= 1)
#pragma unroll
            for (int u = 0; u < w; ++u) acc[u] += acc[u + w];
        s0 = acc[0];
    }
    part[grp][c] = s0 + 0.f;
    __syncthreads();
    if (grp == 0) {
        double q2 = 0.0;
        if (e < p_lstm + ph) {
            float s = 0.f;
#pragma unroll
            for (int g = 0; g < ON_GROUPS; ++g) s += part[g][c];
            grads[e] = s;
            const float gt = s * gscale;
            q2 = (double)gt * (double)gt;
        }
        sq[c] = q2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < ON_COLS; ++i) t += sq[i];
        parts[blockIdx.x] = t;
    }
}

// ---- launch 1, flat route: workgroup b's double sum of (fp32(g[i] * gscale))^2 over its grid-stride elements (each thread in index
// order, then a fixed tree over the threads) ------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum_256(double v, double *red) {      // every thread returns the total; fixed association
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int w = FLAT_NT / 2; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}
__global__ __launch_bounds__(FLAT_NT) void norm_flat_kernel(long n, const float *g, float gscale, double *parts) {
    __shared__ double red[FLAT_NT];
    double s = 0.0;
    for (long i = (long)blockIdx.x * FLAT_NT + threadIdx.x; i < n; i += (long)gridDim.x * FLAT_NT) {
        const float gt = g[i] * gscale;
        s += (double)gt * (double)gt;
    }
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) parts[blockIdx.x] = s;
}

// ---- launch 2: the Adam update of every route ---------------------------------------------------------------------------------------
// Host step (step_dev == null): lr_eff, lr / bc1 and 1 / sqrt(bc2) arrive formed on the host, as nsd_adam_step forms them -- an unclipped
// constant-schedule step is that entry point's bit for bit.  Device step: formed here from the counter, as adam_dev_kernel does.
struct OptK {
    float lr, b1, b2, eps, wd, gscale, max_norm;
    int sched, warmup, total, step_size;
    float min_ratio, gamma;
    float lr_eff, lr_over_bc1, rsqrt_bc2;       // host step only
    const long long *step_dev;
};
// M models: an OptK per model by value in the launch arguments, indexed by blockIdx.y (workgroup-uniform: scalar loads).  The uniform
// model-batched entry point fills M equal entries, so a model's workgroups run the same instructions on either route.
struct OptKSet { OptK k[NSD_MAX_MODELS]; };
static_assert(sizeof(OptKSet) <= 2560, "the per-model optimizer block stays well inside the 4 KB kernarg segment");
__device__ __forceinline__ const OptK &opt_of(const OptK &k, long) { return k; }
__device__ __forceinline__ const OptK &opt_of(const OptKSet &k, long mo) { return k.k[mo]; }
// weight averaging (nsd_avg): per model by value next to OptK.  NoAvg: the plain update, whose instructions the averaging twin leaves alone
struct AvgK { int mode; float w; int start, every; };                 // w = 1.0f - decay, formed once on the host in fp32
struct AvgKSet { AvgK k[NSD_MAX_MODELS]; };
static_assert(sizeof(OptKSet) + sizeof(AvgKSet) <= 3072, "optimizer and averaging blocks together stay inside the 4 KB kernarg segment");
struct NoAvg {};
struct AvgArgs1 { AvgK k; int step; nsd_avg_record *rec; float *rows; };        // step: the host step (ignored with step_dev)
struct AvgArgsM { AvgKSet k; int step; nsd_avg_record *rec; float *rows; };
__device__ __forceinline__ const AvgK &avg_of(const AvgArgs1 &a, long) { return a.k; }
__device__ __forceinline__ const AvgK &avg_of(const AvgArgsM &a, long mo) { return a.k.k[mo]; }

template <class OK, class AV>
__device__ __forceinline__ void adam_clip_body(long n, float *p, const float *g, float *m, float *v, const OK &ok, const double *parts,
                                               int n_parts, nsd_opt_record *rec, const float *skip, const AV &av) {
    constexpr bool AVG = !std::is_same<AV, NoAvg>::value;
    if (skip != nullptr && skip[0] != 0.f) return;                    // the caller's guard: nothing is written, the record included
    const long mo = blockIdx.y;
    const OptK &o = opt_of(ok, mo);
    p += mo * n; g += mo * n; m += mo * n; v += mo * n; parts += mo * n_parts; rec += mo;
    __shared__ double red[FLAT_NT];
    double s = 0.0;
    for (int i = threadIdx.x; i < n_parts; i += FLAT_NT) s += parts[i];
    const double S = block_sum_256(s, red);
    const double nrm = sqrt(S);
    const bool finite = fabs(S) <= DBL_MAX;                            // false for Inf and NaN
    float lr_eff = o.lr_eff, lr_over_bc1 = o.lr_over_bc1, rsqrt_bc2 = o.rsqrt_bc2;
    if (o.step_dev != nullptr) {
        const long long sn = o.step_dev[0];
        const double st = (double)sn;
        const double bc1 = 1.0 - pow((double)o.b1, st), bc2 = 1.0 - pow((double)o.b2, st);
        lr_eff = (float)((double)o.lr * lr_factor_of(o.sched, o.warmup, o.total, o.step_size, o.min_ratio, o.gamma, sn));
        lr_over_bc1 = (float)((double)lr_eff / bc1);
        rsqrt_bc2 = (float)(1.0 / sqrt(bc2));
    }
    float coef = 1.f;
    if (o.max_norm > 0.f) { const double c = (double)o.max_norm / (nrm + 1e-6); coef = (float)(c < 1.0 ? c : 1.0); }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        rec->norm = (float)nrm; rec->coef = finite ? coef : 0.f; rec->lr = lr_eff;
        if (!finite) rec->skipped += 1u;                               // one writer per model: no atomic
    }
    if (!finite) return;                                               // uniform over the grid: every workgroup formed the same S
    // averaging: does this step average (uniform over the model's workgroups: s and the settings are), and n_avg as it stood before
    // the launch.  Thread 0 reads the word and hands it round through LDS, so it holds the value before this workgroup arrives.
    bool averaging = false;
    unsigned n0 = 0u;
    float *row = nullptr;
    nsd_avg_record *arec = nullptr;
    if constexpr (AVG) {
        const AvgK &a = avg_of(av, mo);
        const long long s = o.step_dev != nullptr ? o.step_dev[0] : (long long)av.step;
        averaging = a.mode != 0 && s >= a.start && (s - a.start) % a.every == 0;
        if (averaging) {
            __shared__ unsigned n_sh;
            arec = av.rec + mo; row = av.rows + mo * n;
            if (threadIdx.x == 0) n_sh = __hip_atomic_load(&arec->n_avg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            n0 = n_sh;
        }
    }
    for (long i = (long)blockIdx.x * FLAT_NT + threadIdx.x; i < n; i += (long)gridDim.x * FLAT_NT) {
        const float pi = p[i];                                         // the arithmetic of adam_kernel, in its order
        const float gi = fmaf(o.wd, pi, (g[i] * o.gscale) * coef);
        const float mi = o.b1 * m[i] + (1.f - o.b1) * gi;
        const float vi = o.b2 * v[i] + (1.f - o.b2) * gi * gi;
        m[i] = mi; v[i] = vi;
        const float denom = sqrtf(vi) * rsqrt_bc2 + o.eps;
        const float pn = pi - lr_over_bc1 * (mi / denom);
        p[i] = pn;
        if constexpr (AVG) {
            if (averaging) {
                if (n0 == 0u) row[i] = pn;                             // the first averaged step copies the word
                else {
                    const AvgK &a = avg_of(av, mo);
                    const float ai = row[i], dlt = pn - ai;            // each operation rounded once (-ffp-contract=off)
                    row[i] = a.mode == NSD_AVG_EMA ? ai + a.w * dlt : ai + dlt / (float)(n0 + 1u);
                }
            }
        }
    }
    if constexpr (AVG) {
        // last arriver: no workgroup waits for another.  (The rows are nobody's input in this launch: the arrival says "I have read
        // n_avg", not "I have written my elements".)
        if (averaging && threadIdx.x == 0 &&
            __hip_atomic_fetch_add(&arec->arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u) {
            __hip_atomic_store(&arec->n_avg, n0 + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&arec->arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}
template <class OK>
__global__ __launch_bounds__(FLAT_NT) void adam_clip_kernel(long n, float *p, const float *g, float *m, float *v, OK ok,
                                                            const double *parts, int n_parts, nsd_opt_record *rec, const float *skip) {
    adam_clip_body(n, p, g, m, v, ok, parts, n_parts, rec, skip, NoAvg{});
}
template <class OK, class AV>
__global__ __launch_bounds__(FLAT_NT) void adam_clip_avg_kernel(long n, float *p, const float *g, float *m, float *v, OK ok,
                                                                const double *parts, int n_parts, nsd_opt_record *rec, const float *skip, AV av) {
    adam_clip_body(n, p, g, m, v, ok, parts, n_parts, rec, skip, av);
}

static OptK opt_kernel_args(const nsd_opt *o, int step, const long long *step_dev) {
    OptK k;
    memset(&k, 0, sizeof(k));
    k.lr = o->lr; k.b1 = o->beta1; k.b2 = o->beta2; k.eps = o->eps; k.wd = o->weight_decay; k.gscale = o->grad_scale; k.max_norm = o->max_norm;
    k.sched = o->sched; k.warmup = o->warmup_steps; k.total = o->total_steps; k.step_size = o->step_size;
    k.min_ratio = o->min_ratio; k.gamma = o->gamma; k.step_dev = step_dev;
    if (!step_dev) {
        const double bc1 = 1.0 - pow((double)o->beta1, step), bc2 = 1.0 - pow((double)o->beta2, step);
        k.lr_eff = (float)((double)o->lr * nsd_lr_factor_host(o, step));
        k.lr_over_bc1 = (float)(k.lr_eff / bc1);
        k.rsqrt_bc2 = (float)(1.0 / sqrt(bc2));
    }
    return k;
}

static AvgK avg_kernel_args(const nsd_avg *a) {
    AvgK k;
    memset(&k, 0, sizeof(k));
    k.mode = a->mode; k.w = a->mode == NSD_AVG_EMA ? 1.0f - a->decay : 0.f; k.start = a->start_step; k.every = a->every;
    if (k.mode == 0) { k.start = 1; k.every = 1; }
    return k;
}
template <class AV> static void avg_fill(AV *av, int M, const NsdAvgSpec *as, int step) {
    memset(av, 0, sizeof(*av));
    av->step = step; av->rec = (nsd_avg_record *)as->state;
    av->rows = reinterpret_cast<float *>(static_cast<char *>(as->state) + (size_t)M * sizeof(nsd_avg_record));
}

// as: null -- the plain update kernel, as before averaging existed; else its averaging twin with the model's (models') settings
template <class OK>
static int adam_clip_launch(long n, int M, float *p, const float *g, float *m, float *v, const OK &k, long n_parts, void *state,
                            const float *skip, const char *who, hipStream_t st, const NsdAvgSpec *as = nullptr, int step = 0) {
    long blocks = (n + FLAT_NT - 1) / FLAT_NT; if (blocks > 2048) blocks = 2048;
    // averaging: every workgroup arrives once on its model's record, and the records of all models share a few cache lines, so the
    // arrivals of a launch queue up behind each other: a grid-stride loop over fewer workgroups per model, about one per CU in all,
    // more only where a thread would otherwise take more than 8 elements (large flat vectors: there the memory traffic dominates).
    // The results do not depend on the grid: the update is element-wise and the partials are summed in the order of their index.
    if (as) {
        long cap = 256 / M > 32 ? 256 / M : 32;
        const long by_work = (n + 8 * FLAT_NT - 1) / (8 * FLAT_NT);
        if (by_work > cap) cap = by_work;
        if (blocks > cap) blocks = cap;
    }
    const dim3 grid((unsigned)blocks, (unsigned)M);
    const double *parts = parts_of(state, M);
    if (!as) {
        hipLaunchKernelGGL(adam_clip_kernel<OK>, grid, dim3(FLAT_NT), 0, st, n, p, g, m, v, k, parts, (int)n_parts, (nsd_opt_record *)state, skip);
    } else if constexpr (std::is_same<OK, OptK>::value) {
        AvgArgs1 av;
        avg_fill(&av, M, as, step);
        av.k = avg_kernel_args(as->avg);
        hipLaunchKernelGGL((adam_clip_avg_kernel<OK, AvgArgs1>), grid, dim3(FLAT_NT), 0, st, n, p, g, m, v, k, parts, (int)n_parts,
                           (nsd_opt_record *)state, skip, av);
    } else {
        AvgArgsM av;
        avg_fill(&av, M, as, step);
        for (int mo = 0; mo < M; ++mo) av.k.k[mo] = avg_kernel_args(as->each ? as->avg + mo : as->avg);
        hipLaunchKernelGGL((adam_clip_avg_kernel<OK, AvgArgsM>), grid, dim3(FLAT_NT), 0, st, n, p, g, m, v, k, parts, (int)n_parts,
                           (nsd_opt_record *)state, skip, av);
    }
    NSD_CHECK_LAUNCH(who);
    return NSD_OK;
}

// nsd_avg's fields: 0, or the NSD_E_INVALID refusal with the field named.  allow_off: mode 0 passes (an entry of the `_each` twin)
int nsd_avg_check(const nsd_avg *a, const char *who, int allow_off) {
    if (!a) { nsd_set_error("%s: avg is NULL", who); return NSD_E_INVALID; }
    if (a->mode == 0 && allow_off) return NSD_OK;
    if (a->mode != NSD_AVG_EMA && a->mode != NSD_AVG_SWA) { nsd_set_error("%s: mode %d unknown (NSD_AVG_EMA / NSD_AVG_SWA)", who, a->mode); return NSD_E_INVALID; }
    if (a->mode == NSD_AVG_EMA && !(a->decay >= 0.f && a->decay < 1.f)) { nsd_set_error("%s: decay %g outside [0, 1) or NaN", who, a->decay); return NSD_E_INVALID; }
    if (a->start_step < 1) { nsd_set_error("%s: start_step %d must be >= 1", who, a->start_step); return NSD_E_INVALID; }
    if (a->every < 1) { nsd_set_error("%s: every %d must be >= 1", who, a->every); return NSD_E_INVALID; }
    return NSD_OK;
}
int64_t nsd_avg_state_need(int64_t n, int M) { return (int64_t)M * (int64_t)sizeof(nsd_avg_record) + (int64_t)M * n * (int64_t)sizeof(float); }

// the fused tail of M models (M = 1: the single-model entry point): reduction with norm, then the update.  o: one nsd_opt for all
// models, or with each != 0 (M > 1) one per model
int nsd_reduce_clip_adam_launch(const SlabSet &s, int M, float *grads, float *p, float *m, float *v, const nsd_opt *o, int each, int step,
                                const long long *step_dev, void *state, const char *who, hipStream_t st, const NsdAvgSpec *as) {
    const long P = s.p_lstm + s.ph, cols = col_parts(P);
    const dim3 wg(ON_COLS * ON_GROUPS);
    if (M == 1) {
        hipLaunchKernelGGL(reduce_norm_kernel<false>, dim3((unsigned)cols), wg, 0, st, s.slabs, s.stride, s.n, s.p_lstm, s.hslabs, s.ph, s.n_h, grads,
                           GScale<false>{o->grad_scale}, parts_of(state, M));
        NSD_CHECK_LAUNCH(who);
        return adam_clip_launch(P, M, p, grads, m, v, opt_kernel_args(o, step, step_dev), cols, state, nullptr, who, st, as, step);
    }
    GScale<true> gs;
    OptKSet ks;
    memset(&gs, 0, sizeof(gs));
    memset(&ks, 0, sizeof(ks));
    for (int mo = 0; mo < M; ++mo) {
        const nsd_opt *om = each ? o + mo : o;
        gs.g[mo] = om->grad_scale;
        ks.k[mo] = opt_kernel_args(om, step, step_dev);
    }
    hipLaunchKernelGGL(reduce_norm_kernel<true>, dim3((unsigned)cols, (unsigned)M), wg, 0, st, s.slabs, s.stride, s.n, s.p_lstm, s.hslabs, s.ph, s.n_h,
                       grads, gs, parts_of(state, M));
    NSD_CHECK_LAUNCH(who);
    return adam_clip_launch(P, M, p, grads, m, v, ks, cols, state, nullptr, who, st, as, step);
}

int nsd_grad_norm_launch(long n, const float *g, float gscale, void *state, hipStream_t st) {
    if (n <= 0) return NSD_OK;
    hipLaunchKernelGGL(norm_flat_kernel, dim3((unsigned)flat_parts(n)), dim3(FLAT_NT), 0, st, n, g, gscale, parts_of(state, 1));
    NSD_CHECK_LAUNCH("grad_norm");
    return NSD_OK;
}

int nsd_adam_clip_flat_launch(long n, float *p, const float *g, float *m, float *v, const nsd_opt *o, int step, const long long *step_dev,
                              const float *skip, void *state, hipStream_t st, const NsdAvgSpec *as) {
    if (n <= 0) return NSD_OK;
    return adam_clip_launch(n, 1, p, g, m, v, opt_kernel_args(o, step, step_dev), flat_parts(n), state, skip, as ? "adam_step_clip_avg" : "adam_step_clip", st,
                            as, step);
}

// ---- sharpness-aware minimisation: the ascent (nsd_sam of include/nsd.h) -------------------------------------------------------------
// Two launches with no signalling between workgroups, as the clipped tail: launch 1 is the tail's own (reduce_norm_kernel for the slabs,
// norm_flat_kernel for a flat gradient) and leaves grads and the partial sums in opt_state's scratch; launch 2, sam_ascend_kernel, sums
// the partials in the tail's fixed order in every workgroup, forms the step length in double and writes its grid-stride share of the
// model's perturbed row.  p and grads are inputs only; rho and grad_scale arrive per model by value (blockIdx.y is workgroup-uniform).
struct SamK { float rho, gscale; };
struct SamKSet { SamK k[NSD_MAX_MODELS]; };
__device__ __forceinline__ const SamK &sam_of(const SamK &k, long) { return k; }
__device__ __forceinline__ const SamK &sam_of(const SamKSet &k, long mo) { return k.k[mo]; }

template <class SK>
__global__ __launch_bounds__(FLAT_NT) void sam_ascend_kernel(long n, const float *p, const float *g, SK sk, const double *parts, int n_parts,
                                                             nsd_sam_record *rec, float *rows) {
    const long mo = blockIdx.y;
    const SamK &k = sam_of(sk, mo);
    p += mo * n; g += mo * n; rows += mo * n; parts += mo * n_parts; rec += mo;
    __shared__ double red[FLAT_NT];
    double s = 0.0;
    for (int i = threadIdx.x; i < n_parts; i += FLAT_NT) s += parts[i];
    const double S = block_sum_256(s, red);
    const double nrm = sqrt(S);
    const bool finite = fabs(S) <= DBL_MAX;                            // false for Inf and NaN
    const bool move = finite && k.rho != 0.f;                          // uniform over the model's workgroups: every one formed the same S
    const float es = move ? (float)((double)k.rho / (nrm + 1e-12)) : 0.f;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        rec->norm = (float)nrm; rec->scale = es;
        if (!finite) rec->nonfinite += 1u;                             // one writer per model: no atomic
    }
    const long i0 = (long)blockIdx.x * FLAT_NT + threadIdx.x, stride = (long)gridDim.x * FLAT_NT;
    if (!move) {                                                       // a copy of the words: signed zeros survive
        for (long i = i0; i < n; i += stride) rows[i] = p[i];
        return;
    }
    for (long i = i0; i < n; i += stride) {
        const float gt = g[i] * k.gscale;                              // each operation rounded once (-ffp-contract=off)
        const float up = es * gt;
        rows[i] = p[i] + up;
    }
}

int nsd_sam_check(const nsd_sam *s, const char *who) {
    if (!s) { nsd_set_error("%s: sam is NULL", who); return NSD_E_INVALID; }
    if (!(s->rho >= 0.f)) { nsd_set_error("%s: rho %g negative or NaN", who, s->rho); return NSD_E_INVALID; }
    return NSD_OK;
}
int64_t nsd_sam_state_need(int64_t n, int M) { return (int64_t)M * (int64_t)sizeof(nsd_sam_record) + (int64_t)M * n * (int64_t)sizeof(float); }

// rho, gscale: M entries each
static int sam_ascend_launch(long n, int M, const float *p, const float *g, const float *rho, const float *gscale, long n_parts, void *opt_state,
                             void *sam_state, const char *who, hipStream_t st) {
    long blocks = (n + FLAT_NT - 1) / FLAT_NT; if (blocks > 2048) blocks = 2048; if (blocks < 1) blocks = 1;
    const dim3 grid((unsigned)blocks, (unsigned)M);
    const double *parts = parts_of(opt_state, M);
    nsd_sam_record *rec = (nsd_sam_record *)sam_state;
    float *rows = reinterpret_cast<float *>(static_cast<char *>(sam_state) + (size_t)M * sizeof(nsd_sam_record));
    if (M == 1) {
        hipLaunchKernelGGL(sam_ascend_kernel<SamK>, grid, dim3(FLAT_NT), 0, st, n, p, g, SamK{rho[0], gscale[0]}, parts, (int)n_parts, rec, rows);
    } else {
        SamKSet ks;
        memset(&ks, 0, sizeof(ks));
        for (int mo = 0; mo < M; ++mo) ks.k[mo] = SamK{rho[mo], gscale[mo]};
        hipLaunchKernelGGL(sam_ascend_kernel<SamKSet>, grid, dim3(FLAT_NT), 0, st, n, p, g, ks, parts, (int)n_parts, rec, rows);
    }
    NSD_CHECK_LAUNCH(who);
    return NSD_OK;
}

// from the slabs of M models (M = 1: the single-model entry point): the tail's reduction with norm, then the ascent
int nsd_sam_ascend_slabs_launch(const SlabSet &s, int M, float *grads, const float *p, const float *rho, const float *gscale, void *opt_state,
                                void *sam_state, const char *who, hipStream_t st) {
    const long P = s.p_lstm + s.ph, cols = col_parts(P);
    const dim3 wg(ON_COLS * ON_GROUPS);
    if (M == 1) {
        hipLaunchKernelGGL(reduce_norm_kernel<false>, dim3((unsigned)cols), wg, 0, st, s.slabs, s.stride, s.n, s.p_lstm, s.hslabs, s.ph, s.n_h, grads,
                           GScale<false>{gscale[0]}, parts_of(opt_state, M));
    } else {
        GScale<true> gs;
        memset(&gs, 0, sizeof(gs));
        for (int mo = 0; mo < M; ++mo) gs.g[mo] = gscale[mo];
        hipLaunchKernelGGL(reduce_norm_kernel<true>, dim3((unsigned)cols, (unsigned)M), wg, 0, st, s.slabs, s.stride, s.n, s.p_lstm, s.hslabs, s.ph, s.n_h,
                           grads, gs, parts_of(opt_state, M));
    }
    NSD_CHECK_LAUNCH(who);
    return sam_ascend_launch(P, M, p, grads, rho, gscale, cols, opt_state, sam_state, who, st);
}

int nsd_sam_ascend_flat_launch(long n, const float *p, const float *g, float rho, float gscale, void *opt_state, void *sam_state, hipStream_t st) {
    if (n <= 0) return NSD_OK;
    if (const int rc = nsd_grad_norm_launch(n, g, gscale, opt_state, st)) return rc;
    return sam_ascend_launch(n, 1, p, g, &rho, &gscale, flat_parts(n), opt_state, sam_state, "sam_ascend_flat", st);
}
