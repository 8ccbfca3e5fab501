// nsd_eval.hip -- early stopping for model batches (nsd_multi_eval of include/nsd.h): held-out metrics, the best-evaluation decision,
// the patience count and the parameter snapshot of M models in ONE launch, one 256-thread workgroup per model.
//
//   1. metrics: lane i takes rows i, i + 256, ... of its model's counted rows in ascending order; per row the loss, the first maximal
//      index and the finiteness test in double from the fp32 logits.  The counts (n, correct, nonfinite, confusion) are integers in LDS,
//      so their order does not matter; the loss is a double per lane, combined by a halving tree over the 256 lanes: an order that
//      depends on the workgroup size alone.
//   2. lane 0 writes the eval record, reads the model's select record, decides (the rule of nsd.h), writes the record back and leaves
//      the decision in LDS.
//   3. after the barrier every lane of an improved model copies the parameter row into the snapshot row: single words up to the first
//      16-byte boundary of the destination, 16 bytes per lane in the body, single words in the tail.  Source and destination rows
//      start at the same float offset m * P of their 16-byte aligned bases, so they share the misalignment; where a caller's bases do
//      not, the whole row goes word by word.  A model that did not improve stores nothing.
// No workgroup reads what another writes; the select record is read and written by its own workgroup's lane 0 only, so launches on one
// stream (and the replays of a captured one) see it in order.
#include <math.h>
#include "nsd_args.h"

__device__ __forceinline__ bool finite_f32(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

__global__ __launch_bounds__(EVAL_NT) void multi_eval_kernel(EvalArgs a) {
    const int mo = blockIdx.x, tid = threadIdx.x;
    const int K = a.K, count = a.counts[mo];
    const float *lg = a.logits + (size_t)mo * a.B * K;
    const int32_t *lab = a.labels + (size_t)mo * a.B;

    __shared__ double lane_sum[EVAL_NT];
    __shared__ int conf[NSD_EVAL_MAX_K * NSD_EVAL_MAX_K];
    __shared__ int cnt[3];                       // n, correct, nonfinite
    __shared__ int improved;
    if (tid < NSD_EVAL_MAX_K * NSD_EVAL_MAX_K) conf[tid] = 0;
    if (tid < 3) cnt[tid] = 0;
    if (tid == 0) improved = 0;
    __syncthreads();

    double s = 0.0;
    int n = 0, correct = 0, bad = 0;
    for (int r = tid; r < count; r += EVAL_NT) {
        float l[NSD_EVAL_MAX_K];
        bool ok = true;
#pragma unroll
        for (int k = 0; k < NSD_EVAL_MAX_K; ++k) {
            l[k] = k < K ? lg[(size_t)r * K + k] : 0.f;
            ok = ok && finite_f32(l[k]);
        }
        const int y = lab[r];
        if (!ok || y < 0 || y >= K) { ++bad; continue; }
        int pred = 0;
        float mx = l[0], ly = l[0];
#pragma unroll
        for (int k = 1; k < NSD_EVAL_MAX_K; ++k) {
            if (k < K && l[k] > mx) { mx = l[k]; pred = k; }
            if (k == y) ly = l[k];
        }
        double e = 0.0;
#pragma unroll
        for (int k = 0; k < NSD_EVAL_MAX_K; ++k)
            if (k < K) e += exp((double)l[k] - (double)mx);
        s += (log(e) + (double)mx) - (double)ly;
        ++n;
        correct += pred == y ? 1 : 0;
        atomicAdd(&conf[y * NSD_EVAL_MAX_K + pred], 1);
    }
    lane_sum[tid] = s;
    if (n) atomicAdd(&cnt[0], n);
    if (correct) atomicAdd(&cnt[1], correct);
    if (bad) atomicAdd(&cnt[2], bad);
    __syncthreads();
    for (int w = EVAL_NT / 2; w >= 1; w >>= 1) {
        if (tid < w) lane_sum[tid] += lane_sum[tid + w];
        __syncthreads();
    }

    nsd_eval_record *out = a.out + mo;
    if (tid < NSD_EVAL_MAX_K * NSD_EVAL_MAX_K) out->confusion[tid / NSD_EVAL_MAX_K][tid % NSD_EVAL_MAX_K] = conf[tid];
    if (tid == 0) {
        const int nn = cnt[0], cc = cnt[1], nf = cnt[2];
        const double loss_sum = nf > 0 ? (double)NAN : lane_sum[0];
        out->loss_sum = loss_sum; out->n = nn; out->correct = cc; out->nonfinite = nf; out->pad = 0;
        if (a.select) {
            nsd_select_record r = a.recs[mo];
            if (r.stopped == 0u) {
                r.evals += 1;
                const double mean = loss_sum / (double)nn;           // 0 / 0 with no counted row left: NaN, "not improved"
                const bool fin = nn > 0 && isfinite(mean);
                bool better = false;
                if (!fin) r.status |= 1u;
                else if (r.best_eval == 0) better = true;
                else if (a.metric == NSD_SELECT_LOSS) better = mean < r.best_loss - (double)a.min_delta;
                else {
                    const double acc = (double)cc / (double)nn, best_acc = (double)r.best_correct / (double)r.best_n;
                    better = acc > best_acc + (double)a.min_delta || (acc == best_acc && mean < r.best_loss);
                }
                if (better) {
                    r.best_loss = mean; r.best_correct = cc; r.best_n = nn; r.best_eval = r.evals; r.bad = 0;
                    improved = 1;
                } else {
                    r.bad += 1;
                    if (a.patience > 0 && r.bad >= a.patience) r.stopped = 1u;
                }
                a.recs[mo] = r;
            }
        }
    }
    __syncthreads();
    if (!improved) return;

    // the snapshot: best[mo] = params[mo], bit for bit (words, not floats: a NaN keeps its payload)
    const long P = a.P;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(a.params) + (size_t)mo * P;
    uint32_t *dst = reinterpret_cast<uint32_t *>(a.best) + (size_t)mo * P;
    long head = (long)(((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u) >> 2);
    if (((uintptr_t)src & 15u) != ((uintptr_t)dst & 15u) || head > P) head = P;
    const long body = (P - head) >> 2, tail = head + (body << 2);
    for (long i = tid; i < head; i += EVAL_NT) dst[i] = src[i];
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src + head);
    uint4 *d4 = reinterpret_cast<uint4 *>(dst + head);
    for (long i = tid; i < body; i += EVAL_NT) d4[i] = s4[i];
    for (long i = tail + tid; i < P; i += EVAL_NT) dst[i] = src[i];
}

int nsd_multi_eval_launch(const EvalArgs &a, int M, hipStream_t st) {
    hipLaunchKernelGGL(multi_eval_kernel, dim3((unsigned)M), dim3(EVAL_NT), 0, st, a);
    NSD_CHECK_LAUNCH("multi_eval");
    return NSD_OK;
}
