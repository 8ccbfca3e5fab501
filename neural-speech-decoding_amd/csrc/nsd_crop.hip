// nsd_crop.hip -- cropped training (nsd_crop / nsd_crop_pool of include/nsd.h; an extension, the reference trains on whole trials):
// R windows of W samples cut from every trial of a step, x [B,T,C] -> y [B*R][W][C] per model, with the trial's label / target row
// repeated for its crops, in ONE launch for all models of a model-batched step; and the trial-level decision from window decisions.
//
// crop_kernel: one 256-thread workgroup per output row (model, trial, crop), grid-stride, as mixup_kernel; lanes run along the row's
// contiguous span of W*C floats, which starts at float o*C of the trial.  Random offsets are nsd_rand_u32(seed, base_stream + 3, index)
// on index slots 2048.. that nsd_augment and nsd_mixup leave alone; every thread forms its row's draw itself (one hash): no LDS, no
// barrier.  Memory-bound: W*C floats read and written per row; 16 bytes per lane where C % 4 == 0 (then o*C and W*C are multiples of
// four floats) and the pointers and the model stride allow, one word per lane otherwise.  Words travel as uint32: a NaN keeps its payload.
//
// crop_pool_kernel: one thread per (trial, class); the serial fp32 sum over the trial's counted windows in ascending order, the
// division by float(count), and the logarithm in double.  No thread reads what another writes.
#include <math.h>
#include "nsd_args.h"

#define CROP_NT 256
constexpr uint32_t CROP_STREAM = 3u;                               // base_stream + 3, shared with nsd_augment and nsd_mixup (other slots)
constexpr uint64_t CROP_TRIAL_BIT = 0x8000000000000000ull;         // P(b, slot) = 2^63 | b << 16 | slot
constexpr uint64_t CROP_SLOT0 = 2048ull;                           // crop r draws slot 2048 + r (r < NSD_CROP_MAX)

template <bool VEC>
__global__ __launch_bounds__(CROP_NT) void crop_kernel(const CropArgs a) {
    const int tid = threadIdx.x;
    const int B = a.B, R = a.R, K = a.K;
    const long span = (long)a.W * a.C, n_el = (long)a.T * a.C;
    const uint32_t base_dev = a.step_dev ? (uint32_t)(a.step_dev[0] & 0x3FFFFFFF) * 4u : 0u;
    const uint32_t range = (uint32_t)(a.T - a.W + 1);
    const long per_model = (long)B * R, total = (long)a.M * per_model;
    for (long g = blockIdx.x; g < total; g += gridDim.x) {         // g = (m * B + b) * R + r: the output row
        const int m = (int)(g / per_model);
        const long br = g - (long)m * per_model;
        const int b = (int)(br / R), r = (int)(br - (long)b * R);
        int o;
        if (a.hop > 0) o = r * a.hop;
        else {
            const uint32_t stream = (a.step_dev ? base_dev : a.base[m]) + CROP_STREAM;
            o = (int)(nsd_rand_u32(a.seed[m], stream, CROP_TRIAL_BIT | ((uint64_t)b << 16) | (CROP_SLOT0 + (uint64_t)r)) % range);
        }
        const long t = (long)m * B + b;                            // the trial among all models'
        if (tid == 0) {
            if (a.offsets_out) a.offsets_out[g] = o;
            if (a.labels_out) a.labels_out[g] = a.labels[t];
        }
        if (a.targets_out)
            for (int k = tid; k < K; k += CROP_NT)
                reinterpret_cast<uint32_t *>(a.targets_out)[g * K + k] = reinterpret_cast<const uint32_t *>(a.targets)[t * K + k];
        const uint32_t *src = reinterpret_cast<const uint32_t *>(a.x) + (size_t)m * a.x_stride + (size_t)b * n_el + (size_t)o * a.C;
        uint32_t *dst = reinterpret_cast<uint32_t *>(a.y) + (size_t)g * span;
        if constexpr (VEC) {
            const long n4 = span >> 2;
            for (long e = tid; e < n4; e += CROP_NT) reinterpret_cast<uint4 *>(dst)[e] = reinterpret_cast<const uint4 *>(src)[e];
        } else {
            for (long e = tid; e < span; e += CROP_NT) dst[e] = src[e];
        }
    }
}

int nsd_crop_launch(const CropArgs &a, hipStream_t st) {
    const long total = (long)a.M * a.B * a.R;
    if (total <= 0) return NSD_OK;
    const long cap = 8L * nsd_num_cus();
    const dim3 grid((unsigned)(total < cap ? total : cap)), block(CROP_NT);
    // 16-byte accesses: every trial, every crop (o * C floats into it) and every output row start on a 16-byte boundary
    const bool vec = (a.C & 3) == 0 && (a.x_stride & 3) == 0 && (((uintptr_t)a.x | (uintptr_t)a.y) & 15) == 0;
    if (vec) hipLaunchKernelGGL((crop_kernel<true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((crop_kernel<false>), grid, block, 0, st, a);
    NSD_CHECK_LAUNCH("crop");
    return NSD_OK;
}

__device__ __forceinline__ bool crop_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

__global__ __launch_bounds__(CROP_NT) void crop_pool_kernel(const CropPoolArgs a) {
    const long total = (long)a.N * a.K;
    for (long i = (long)blockIdx.x * CROP_NT + threadIdx.x; i < total; i += (long)gridDim.x * CROP_NT) {
        const int n = (int)(i / a.K), k = (int)(i - (long)n * a.K);
        const int cnt = a.counts ? a.counts[n] : a.R;
        float mean = __uint_as_float(0x7FC00000u);
        if (cnt >= 1 && cnt <= a.R) {
            const float *p = a.probs + (size_t)n * a.R * a.K;
            float s = 0.f;
            bool ok = true;
            for (int r = 0; r < cnt; ++r)
                for (int j = 0; j < a.K; ++j) {                    // a non-finite value anywhere in the trial's counted rows spoils the row
                    const float v = p[(size_t)r * a.K + j];
                    ok = ok && crop_finite(v);
                    if (j == k) s = __fadd_rn(s, v);
                }
            if (ok) mean = __fdiv_rn(s, (float)cnt);
        }
        a.probs_out[i] = mean;
        if (a.logits_out) a.logits_out[i] = (float)log((double)mean);
    }
}

int nsd_crop_pool_launch(const CropPoolArgs &a, hipStream_t st) {
    const long total = (long)a.N * a.K;
    if (total <= 0) return NSD_OK;
    const long blocks = (total + CROP_NT - 1) / CROP_NT, cap = 8L * nsd_num_cus();
    hipLaunchKernelGGL(crop_pool_kernel, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(CROP_NT), 0, st, a);
    NSD_CHECK_LAUNCH("crop_pool");
    return NSD_OK;
}
