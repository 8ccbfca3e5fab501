// nsd_gather.hip -- the step's batch formed on the device (nsd_gather of include/nsd.h; an extension, the reference has no trainer):
// the trials x_all [N][T][C] stay resident with the run's index schedule table [M][S][B]; row r = (c - step_base) mod S of the table,
// c the host's step or the device step counter, names model m's B trials, and x [M][B][T][C] (with labels / target rows) is their copy,
// in ONE launch for all models.  The first stage of a step: gather -> augment -> prep -> crop -> mixup (StepRecipe).
//
// gather_kernel: one 256-thread workgroup per output row (model, trial of its batch), grid-stride, as crop_kernel.  The counter and the
// row's index are workgroup-uniform loads; lanes run along the row's T*C contiguous floats.  Memory-bound: T*C floats read and written
// per row; 16 bytes per lane where T*C % 4 == 0 and both base pointers are 16-byte aligned (every row then starts on a 16-byte
// boundary), one word per lane otherwise, chosen per launch.  Words travel as uint32: a NaN keeps its payload.  An index outside
// [0, N) reads nothing: the row becomes quiet NaNs, its label 0 (the head kernels index by it), its target row NaN, and bit 0 of
// status[m] is set with a vector atomic; the NaNs make the step's guarded tail skip and count it.
#include "nsd_args.h"

#define GATHER_NT 256
constexpr uint32_t GATHER_NAN = 0x7FC00000u;

template <bool VEC>
__global__ __launch_bounds__(GATHER_NT) void gather_kernel(const GatherArgs a) {
    const int tid = threadIdx.x;
    const int B = a.B, K = a.K;
    const long n_el = a.n_el;
    const long long c = a.step_dev ? a.step_dev[0] : a.step;
    long long r = (c - a.step_base) % (long long)a.S;
    if (r < 0) r += a.S;
    const long total = (long)a.M * B;
    for (long g = blockIdx.x; g < total; g += gridDim.x) {         // g = m * B + b: the output row
        const int m = (int)(g / B);
        const int b = (int)(g - (long)m * B);
        const int i = a.table[((long)m * a.S + r) * B + b];
        const bool ok = i >= 0 && i < a.N;
        if (tid == 0) {
            if (a.labels) a.labels[g] = ok ? a.labels_all[i] : 0;
            if (!ok && a.status) atomicOr(&a.status[m], 1);
        }
        if (a.targets)
            for (int k = tid; k < K; k += GATHER_NT)
                reinterpret_cast<uint32_t *>(a.targets)[g * K + k] =
                    ok ? reinterpret_cast<const uint32_t *>(a.targets_all)[(long)i * K + k] : GATHER_NAN;
        const uint32_t *src = reinterpret_cast<const uint32_t *>(a.x_all) + (size_t)(ok ? i : 0) * n_el;
        uint32_t *dst = reinterpret_cast<uint32_t *>(a.x) + (size_t)g * n_el;
        if constexpr (VEC) {                                       // (ok is workgroup-uniform: a branch, not a select per element)
            const long n4 = n_el >> 2;
            if (ok) {
                for (long e = tid; e < n4; e += GATHER_NT) reinterpret_cast<uint4 *>(dst)[e] = reinterpret_cast<const uint4 *>(src)[e];
            } else {
                for (long e = tid; e < n4; e += GATHER_NT)
                    reinterpret_cast<uint4 *>(dst)[e] = make_uint4(GATHER_NAN, GATHER_NAN, GATHER_NAN, GATHER_NAN);
            }
        } else if (ok) {
            for (long e = tid; e < n_el; e += GATHER_NT) dst[e] = src[e];
        } else {
            for (long e = tid; e < n_el; e += GATHER_NT) dst[e] = GATHER_NAN;
        }
    }
}

int nsd_gather_launch(const GatherArgs &a, hipStream_t st) {
    const long total = (long)a.M * a.B;
    if (total <= 0) return NSD_OK;
    const long cap = 32L * nsd_num_cus();
    const dim3 grid((unsigned)(total < cap ? total : cap)), block(GATHER_NT);
    // 16-byte accesses: every trial and every output row start on a 16-byte boundary
    const bool vec = (a.n_el & 3) == 0 && (((uintptr_t)a.x_all | (uintptr_t)a.x) & 15) == 0;
    if (vec) hipLaunchKernelGGL((gather_kernel<true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((gather_kernel<false>), grid, block, 0, st, a);
    NSD_CHECK_LAUNCH("gather");
    return NSD_OK;
}
