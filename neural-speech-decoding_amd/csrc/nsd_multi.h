// nsd_multi.h -- model-batched H = 48 launches (nsd_multi_* of include/nsd.h): M models of one shape in the launches one model uses.
//
// Layout: one batch of M*B trials, partitioned by model.  Model m's trial b is global trial m*B + b of every per-trial workspace region
// (so those regions keep their indexing), its parameters are params + m*P, its windows x + m*x_stride (0: one window set for all).
// The grid is partitioned the same way: workgroups m*G .. m*G + G - 1 take model m's trials and nothing else -- the kernels load the
// recurrent weights into registers once, before the trial loop, so a workgroup never changes model -- and the backward slab of a
// workgroup is the workspace slab of its global index.  The kernels see a "model view": the argument block with every pointer moved to
// model m, B = the trials of one model, and the workgroup index / count inside the model (wg_id / wg_count below).  The single-model
// kernels pass their argument block itself: wg_id / wg_count are blockIdx.x / gridDim.x there and nothing else changes.
#pragma once
#include "nsd_args.h"

struct ModelSplit {
    int G;                                   // workgroups per model
    int rng_on;
    long long x_stride;                      // floats between two models' windows
    long long P;                             // floats per model (nsd_param_count)
    uint64_t seed[NSD_MAX_MODELS];           // model m's random streams: seed[m], base[m]
    uint32_t base[NSD_MAX_MODELS];
    // model m's dropout thresholds and keep factors (nsd_drop_threshold(p), 1 / (1 - p) of rng[m], as nsd_rng_args forms them; equal for
    // all models without NSD_FLAG_MODEL_P).  Workgroup-uniform: a workgroup never changes model, so the view's values are scalar loads
    // from the kernel arguments -- one 16-byte record per model, so that one address and one load serve the four.
    struct Drop { uint32_t thr_lstm; float keep_lstm; uint32_t thr_head; float keep_head; } drop[NSD_MAX_MODELS];
};
static_assert(sizeof(ModelSplit) <= 1088, "ModelSplit + the largest argument block stay well inside the 4 KB kernarg segment");

template <class A>
struct ModelView : A {
    unsigned wg, nwg;
};

// (unsigned, as blockIdx.x / gridDim.x: `(size_t)wg_id(a) * stride` then zero-extends, and the single-model kernels' ISA is unchanged)
template <class A> __device__ __forceinline__ unsigned wg_id(const A &) { return blockIdx.x; }
template <class A> __device__ __forceinline__ unsigned wg_count(const A &) { return gridDim.x; }
template <class A> __device__ __forceinline__ unsigned wg_id(const ModelView<A> &a) { return a.wg; }
template <class A> __device__ __forceinline__ unsigned wg_count(const ModelView<A> &a) { return a.nwg; }

namespace nsd_multi_detail {
template <class T> __device__ __forceinline__ T *mv(T *p, const size_t off) { return p ? p + off : p; }   // (null stays null)
__device__ __forceinline__ int model_of_block(const ModelSplit &s) { return __builtin_amdgcn_readfirstlane((int)blockIdx.x / s.G); }
}  // namespace nsd_multi_detail

template <bool PIN = false>
__device__ __forceinline__ ModelView<Lstm2FwdArgs> model_view(const Lstm2FwdArgs &a, const ModelSplit &s) {
    using nsd_multi_detail::mv;
    const int m = nsd_multi_detail::model_of_block(s);
    ModelView<Lstm2FwdArgs> v;
    static_cast<Lstm2FwdArgs &>(v) = a;
    v.wg = (int)blockIdx.x - m * s.G;
    v.nwg = s.G;
    const size_t P = (size_t)s.P * m, b = (size_t)m * a.B, bt = b * a.T, bth = bt * 48;
    v.x = mv(a.x, (size_t)s.x_stride * m);
    v.w_ih0 = mv(a.w_ih0, P); v.w_hh0 = mv(a.w_hh0, P); v.b_ih0 = mv(a.b_ih0, P); v.b_hh0 = mv(a.b_hh0, P);
    v.w_ih1 = mv(a.w_ih1, P); v.w_hh1 = mv(a.w_hh1, P); v.b_ih1 = mv(a.b_ih1, P); v.b_hh1 = mv(a.b_hh1, P);
    v.attn_w = mv(a.attn_w, P); v.attn_b = mv(a.attn_b, P); v.ln_w = mv(a.ln_w, P); v.ln_b = mv(a.ln_b, P);
    v.fc0_w = mv(a.fc0_w, P); v.fc0_b = mv(a.fc0_b, P); v.fc3_w = mv(a.fc3_w, P); v.fc3_b = mv(a.fc3_b, P);
    v.mask = mv(a.mask, bth);
    v.hseq0 = mv(a.hseq0, bth); v.hseq1 = mv(a.hseq1, bth); v.cseq0 = mv(a.cseq0, bth); v.cseq1 = mv(a.cseq1, bth);
    v.gact0 = mv(a.gact0, 4 * bth); v.gact1 = mv(a.gact1, 4 * bth); v.inseq = mv(a.inseq, bth); v.top = mv(a.top, bth);
    v.logits_out = mv(a.logits_out, b * a.K); v.probs_out = mv(a.probs_out, b * a.K);
    if (a.head_train == HEAD_TRAIN_SOFT) v.targets = mv(a.targets, b * a.K); else v.labels = mv(a.labels, b);
    v.rrelu_slope = mv(a.rrelu_slope, b * a.F); v.drop_head = mv(a.drop_head, b * a.F);
    v.logits = mv(a.logits, b * a.K); v.loss = mv(a.loss, b); v.alpha = mv(a.alpha, bt); v.pooled = mv(a.pooled, b * 48);
    v.fc0_pre = mv(a.fc0_pre, b * a.F); v.dscore = mv(a.dscore, bt); v.dpooled = mv(a.dpooled, b * 48);
    v.adpack = mv(a.adpack, 4 * bt); v.hslabs = mv(a.hslabs, b * a.Ph);
    if (s.rng_on) {
        // PIN (set by the two-trial instantiations of nsd_lstm2_fwd48.hip's kernel): the record's index passes through an empty volatile
        // asm, so its loads stay in the role that reads them and are not hoisted to the kernel's entry.  Each instantiation takes the
        // form with which its VGPR count, spills and private segment are those it had before the record existed
        // (profiles/hyper_grid.md): the values are scalar either way, what differs is where the SGPR spills fall.
        int md = m;
        if constexpr (PIN) asm volatile("" : "+s"(md));
        const ModelSplit::Drop &r = s.drop[md];
        v.rng.seed = s.seed[m]; v.rng.base = s.base[m];
        v.rng.thr_lstm = r.thr_lstm; v.rng.thr_head = r.thr_head; v.rng.keep_lstm = r.keep_lstm; v.rng.keep_head = r.keep_head;
    }
    return v;
}

// DX (false in the four-trial kernel, which writes no da0: its code object stays what it was): the view moves da0_out as well
template <bool DX = true>
__device__ __forceinline__ ModelView<Lstm2BwdArgs> model_view(const Lstm2BwdArgs &a, const ModelSplit &s) {
    const int m = nsd_multi_detail::model_of_block(s);
    ModelView<Lstm2BwdArgs> v;
    static_cast<Lstm2BwdArgs &>(v) = a;
    v.wg = (int)blockIdx.x - m * s.G;
    v.nwg = s.G;
    const size_t P = (size_t)s.P * m, b = (size_t)m * a.B, bt = b * a.T, bth = bt * 48;
    // (every pointer but mask -- null on the model-batched path -- and da0_out -- null unless nsd_multi_train_bwd_dx asks for the input
    // gradient -- is set by the host launcher)
    v.x = a.x + (size_t)s.x_stride * m;
    v.w_hh0 = a.w_hh0 + P; v.w_ih1 = a.w_ih1 + P; v.w_hh1 = a.w_hh1 + P; v.attn_w = a.attn_w + P;
    v.hseq0 = a.hseq0 + bth; v.hseq1 = a.hseq1 + bth; v.cseq0 = a.cseq0 + bth; v.cseq1 = a.cseq1 + bth;
    v.gact0 = a.gact0 + 4 * bth; v.gact1 = a.gact1 + 4 * bth; v.in1seq = a.in1seq + bth;
    v.alpha = a.alpha + bt; v.dscore = a.dscore + bt; v.dpooled = a.dpooled + b * 48;
    v.dsc_pack = a.dsc_pack + 4 * bt; v.pooled = a.pooled + b * 48; v.dscore_out = a.dscore_out + bt;
    v.hslabs = a.hslabs + b * a.Ph;
    v.slabs = a.slabs + (size_t)m * s.G * a.slab_stride;
    if constexpr (DX) v.da0_out = nsd_multi_detail::mv(a.da0_out, 4 * bth);
    if (s.rng_on) {
        const ModelSplit::Drop &r = s.drop[m];
        v.rng.seed = s.seed[m]; v.rng.base = s.base[m];
        v.rng.thr_lstm = r.thr_lstm; v.rng.thr_head = r.thr_head; v.rng.keep_lstm = r.keep_lstm; v.rng.keep_head = r.keep_head;
    }
    return v;
}

// host side: the four H = 48 kernels' model-batched launches (grid = M * s.G workgroups; a.B = trials per model)
int nsd_lstm2_fwd48_multi_launch(const Lstm2FwdArgs &a, const ModelSplit &s, int M, int nb, hipStream_t st);
int nsd_lstm2_fwd48x4_multi_launch(const Lstm2FwdArgs &a, const ModelSplit &s, int M, hipStream_t st);
int nsd_lstm2_bwd48_multi_launch(const Lstm2BwdArgs &a, const ModelSplit &s, int M, int nb, hipStream_t st);
int nsd_lstm2_bwd48x4_multi_launch(const Lstm2BwdArgs &a, const ModelSplit &s, int M, hipStream_t st);
// dispatch by the launch plan of the M*B trials of the launch (plan48, nsd_lstm2.hip)
int nsd_lstm2_multi_fwd_launch(const Lstm2FwdArgs &a, ModelSplit s, int M, hipStream_t st);
int nsd_lstm2_multi_bwd_launch(const Lstm2BwdArgs &a, ModelSplit s, int M, hipStream_t st);
// resumable inference of M models (nsd_multi_stream_step; nsd_multi_stream48.hip): a.B streams and a.S slots per model, s.G is set here;
// mean: null or [B,K], the mean of a.probs over the models, by a second launch
int nsd_multi_stream48_launch(const StreamArgs &a, ModelSplit s, int M, float *mean, hipStream_t st);
// sliding-window decisions of M models (nsd_multi_window_step; nsd_multi_window48.hip): a.B streams and a.S streams of state per model,
// logits / probs [M,B,D,K], ends [M,B,D], counts [M,B]; s.G is set here; mean: null or [B,D,K], the mean of a.probs over the models
int nsd_multi_window48_launch(const WindowArgs &a, ModelSplit s, int M, float *mean, hipStream_t st);
