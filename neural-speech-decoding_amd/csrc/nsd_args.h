// nsd_args.h -- kernel argument blocks and host launchers shared by the .hip files of libnsd_hip.so.
#pragma once
#include "nsd_common.h"

constexpr int HEAD_TRAIN_SOFT = 2;
struct Lstm2FwdArgs {
    const float *x;
    const float *w_ih0, *w_hh0, *b_ih0, *b_hh0, *w_ih1, *w_hh1, *b_ih1, *b_hh1;
    const float *mask;
    float *hseq0, *hseq1, *cseq0, *cseq1, *gact0, *gact1, *inseq, *top;
    long long *dbg;                          // diagnostic build only (see nsd_prof.h)
    // fused inference tail (lstm2_fwd48 only; logits_out != null): attention pooling over time as an online softmax,
    // LayerNorm, dense head and class softmax inside the LSTM kernel -- the [B,T,H] sequence never leaves the chip
    const float *attn_w, *attn_b, *ln_w, *ln_b, *fc0_w, *fc0_b, *fc3_w, *fc3_b;
    float *logits_out, *probs_out;
    float eval_slope;
    int K, F;
    int B, T, C, residual;
    int ablate;                              // timing experiments only (env NSD_ABLATE); 0 in production
    // fused TRAIN head (lstm2_fwd48 only; head_train != 0): attention pooling rides along the recurrence (wave 10), then
    // LayerNorm, dense head, mean-CE and the head's backward run in the kernel's tail -- what nsd_head_train does in a
    // second launch.  Outputs and per-trial gradient slabs are those of HeadArgs.
    // head_train == HEAD_TRAIN_SOFT: the loss is formed from fp32 target rows [B,K] instead of labels (the `_soft` entry points of nsd.h);
    // the two pointers share their place in the block, so the hard-label kernels' argument block is what it was
    int head_train;
    // lstm2_fwd48x4 only, set by the launcher when the backward pass of this batch runs lstm2_bwd48x4_kernel: the per-step part of the
    // attention's backward (dL/dscore_t, d attn.weight, d attn.bias) is left to that kernel, which reads the top rows anyway; the
    // forward writes alpha_t and marks the {alpha, dscore} records as open ({alpha_t, 0, 1, 0}: see Lstm2BwdArgs::dsc_pack)
    int defer_att;
    union { const int32_t *labels; const float *targets; };   // head_train == 1: labels [B]; == HEAD_TRAIN_SOFT: targets [B,K]
    const float *rrelu_slope, *drop_head;
    float scale;
    float *logits, *loss, *alpha, *pooled, *fc0_pre, *dscore, *dpooled, *adpack, *hslabs;
    long o_ln_w, o_ln_b, o_attn_w, o_attn_b, o_fc0_w, o_fc0_b, o_fc3_w, o_fc3_b, Ph;
    RngArgs rng;                             // rng.on: dropout multipliers / RReLU slopes are generated in the kernel
};
struct Lstm2BwdArgs {
    const float *x;
    const float *w_hh0, *w_ih1, *w_hh1, *attn_w;
    const float *mask;
    const float *hseq0, *hseq1, *cseq0, *cseq1, *gact0, *gact1;
    const float *in1seq;
    const float *alpha, *dscore, *dpooled;
    const float *dsc_pack;                   // [B,T,4] {alpha, dscore, 0, 0}: 16-byte records for LDS-DMA
                                             // lstm2_bwd48x4: a record {alpha, -, 1, -} is OPEN (left by lstm2_fwd48x4 with defer_att): the kernel
                                             // forms dscore_t = alpha_t dpooled . (top_t - pooled) itself, writes it to dscore_out and adds
                                             // d attn.weight / d attn.bias of the trial to its head slab
    const float *pooled;                     // [B,H] (open records only)
    float *dscore_out;                       // [B,T]
    float *da0_out;                          // null, or [B,T,4H]: the layer-0 pre-activation gradients da0[b][t][gate * H + unit] for the input
                                             // gradient dx = da0 . W_ih0 (lstm2_bwd48_kernel<1> only; may alias gact0: a step's saved gates
                                             // have been staged a chunk earlier)
    float *hslabs;                           // per-trial head-gradient slabs (stride Ph), offsets of attn.weight / attn.bias in them
    long Ph, o_attn_w, o_attn_b;
    float *slabs;
    long slab_stride;
    long o_w_ih0, o_w_hh0, o_b_ih0, o_b_hh0, o_w_ih1, o_w_hh1, o_b_ih1, o_b_hh1;
    long long *dbg;                          // diagnostic build of the schedule: per-wave {work, wait} cycle sums of workgroup 0 (null = off)
    int B, T, C, residual;
    int ablate;                              // timing experiments only (env NSD_ABLATE); 0 in production
    RngArgs rng;                             // rng.on: the inter-layer dropout multipliers are generated in the kernel
};
struct HeadArgs {
    const float *top;
    const float *ln_w, *ln_b, *attn_w, *attn_b, *fc0_w, *fc0_b, *fc3_w, *fc3_b;
    const float *rrelu_slope, *drop_head;
    float eval_slope;
    float *logits, *probs;
    float *alpha, *pooled, *fc0_pre;
    const float *logits_in, *dlogits;
    const int32_t *labels;
    const float *targets;                    // null, or [B,K] soft targets in place of the labels
    float scale;
    float *loss, *dscore, *dpooled;
    float *adpack;                           // [B,T,4] {alpha, dscore, 0, 0} (backward only, may be null)
    float *hslabs;
    long o_ln_w, o_ln_b, o_attn_w, o_attn_b, o_fc0_w, o_fc0_b, o_fc3_w, o_fc3_b;
    long Ph;
    int stage_stride;                        // set by the launcher: LDS row stride of the staged sequence (0 = read from HBM)
    int B, T, H, F, K;
};
int nsd_lstm2_fwd_launch(const Lstm2FwdArgs &a, int H, hipStream_t st);
int nsd_lstm2_bwd_launch(const Lstm2BwdArgs &a, int H, hipStream_t st);
int nsd_lstm2_bwd_groups(int B, int M);     // workgroups (= slabs) per model of the backward launch: M models of B trials each (plan48, nsd_lstm2.hip)
int nsd_lstm2_bwd48_launch(const Lstm2BwdArgs &a, int nb, int grid, hipStream_t st);
int nsd_lstm2_fwd48_launch(const Lstm2FwdArgs &a, int nb, int grid, hipStream_t st);
bool nsd_lstm2_fwd48_head_train_fits(int T, int F, int K);
// four trials per workgroup, gate products on the matrix pipe (nsd_lstm2_fwd48x4.hip): training launches of the plain stack
bool nsd_lstm2_fwd48x4_ok(const Lstm2FwdArgs &a);
int nsd_lstm2_fwd48x4_launch(const Lstm2FwdArgs &a, int grid, hipStream_t st);
// EXPERIMENTAL one-wave-per-layer forward (nsd_lstm2_fwd48w.hip): diagnostic twin only (nsd_diag_force_fwd48(8))
bool nsd_lstm2_fwd48w_ok(const Lstm2FwdArgs &a);
int nsd_lstm2_fwd48w_launch(const Lstm2FwdArgs &a, int grid, hipStream_t st);
bool nsd_lstm2_bwd48x4_ok(const Lstm2BwdArgs &a);
int nsd_lstm2_bwd48x4_launch(const Lstm2BwdArgs &a, int grid, hipStream_t st);
// The layer-by-layer stacks (nsd_lstm_generic.hip, nsd_lstm_batched.hip): one argument block for their four drivers, built by stack_args()
// of nsd_abi.hip.  Training binds the saved regions of the workspace; inference leaves them null and ping-pongs between top_out and scratch2.
struct StackArgs {
    nsd_dims d;
    ParamLayout pl;
    const float *params, *x;
    const float *drop_lstm;                  // null, or the inter-layer multipliers [L-1][B,T,H]
    int residual;
    float *hseq, *cseq, *gact, *inseq;       // saved per layer: h, c [L][B,T,H], gates [L][B,T,4H], layer outputs [L-1][B,T,H]
    float *top_out;                          // [B,T,H]: the last layer's output
    const float *alpha, *dscore, *dpooled;   // the head's gradient inputs
    float *da_seq;                           // generic: [B,T,4H], the layer in flight; batched: [L][B,T,4H]
    float *din_a, *din_b;                    // [B,T,H] ping-pong for d(layer input)
    float *state;                            // batched backward: [L][3][B,H] (dhrec, dc, dho) + split-K partials 8 * 4H * max(C,H)
    float *slab;                             // weight / bias gradients [P_lstm]
    bool bf16;                               // batched: bf16 GEMM operands
    float *scratch2, *cstate;                // inference: [B,T,H] ping-pong; batched: cell-state ping-pong [L][2][B,H]

    int64_t BTH() const { return (int64_t)d.B * d.T * d.H; }
    int I(int l) const { return l == 0 ? d.C : d.H; }
    const float *w_ih(int l) const { return params + pl.w_ih[l]; }
    const float *w_hh(int l) const { return params + pl.w_hh[l]; }
    const float *b_ih(int l) const { return params + pl.b_ih[l]; }
    const float *b_hh(int l) const { return params + pl.b_hh[l]; }
    const float *mask(int l) const { return (l < d.L - 1 && drop_lstm) ? drop_lstm + (int64_t)l * BTH() : nullptr; }
    float *out(int l) const {                // (inference ping-pong: the last layer lands in top_out)
        if (l == d.L - 1) return top_out;
        if (inseq) return inseq + (int64_t)l * BTH();
        return ((d.L - 1 - l) & 1) ? scratch2 : top_out;
    }
    const float *in(int l) const { return l == 0 ? x : out(l - 1); }
    float *din(int l) const { return (l & 1) ? din_a : din_b; }       // written by layer l's backward, read by layer l - 1's
    float *h(int l) const { return hseq + (int64_t)l * BTH(); }
    float *c(int l) const { return cseq + (int64_t)l * BTH(); }
    float *gates(int l) const { return gact + (int64_t)l * 4 * BTH(); }
};
int nsd_lstm_generic_fwd(const StackArgs &s, hipStream_t st);
int nsd_lstm_generic_bwd(const StackArgs &s, hipStream_t st);
bool nsd_lstm_batched_ok(const nsd_dims *d, bool training);
int nsd_lstm_batched_fwd(const StackArgs &s, hipStream_t st);
int nsd_lstm_batched_bwd(const StackArgs &s, hipStream_t st);
int nsd_head_launch(const HeadArgs &a, bool bwd, hipStream_t st);
int nsd_head_train_launch(const HeadArgs &a, hipStream_t st);   // 1 launched, 0 shape does not fit, <0 error
int nsd_zscore_launch(const float *x, float *y, int B, int T, int C, hipStream_t st);
// trial augmentation (nsd_augment of nsd.h; nsd_augment.hip): thresholds and the noise factor are formed on the host
struct AugArgs {
    const float *x; float *y;
    long long x_stride;                      // floats between two models' windows (0: shared)
    const long long *step_dev;               // null, or the device step counter the stream id is formed from
    int B, T, C, M;
    int zscore;                              // per launch (it selects the kernel)
    struct Model {                           // model m's nsd_aug (nsd_augment: M equal entries; nsd_augment_each: its own), read with the
        int max_shift;                       // workgroup's m: scalar loads from the kernel arguments.  0: off
        float scale_range, noise_k;          // noise_k = float(double(noise_std) / sqrt(21845))
        uint32_t thr_channel;                // a channel is dropped when its draw is below this
        int scale_on, noise_on, drop_on;     // an operation is on when its parameter is not 0 (noise_k may round to 0 while noise_std is not)
    } mod[NSD_MAX_MODELS];
    uint64_t seed[NSD_MAX_MODELS];
    uint32_t base[NSD_MAX_MODELS];
};
static_assert(sizeof(AugArgs) <= 2048, "AugArgs stays well inside the 4 KB kernarg segment");
int nsd_augment_launch(const AugArgs &a, hipStream_t st);
// soft targets and mixed windows (nsd_mixup of nsd.h; nsd_mixup.hip)
struct MixArgs {
    const float *x; float *y;                // null together: the launch only builds targets
    long long x_stride;                      // floats between two models' windows (0: shared)
    const long long *step_dev;               // null, or the device step counter the stream id is formed from
    const int32_t *labels;                   // [M*B]
    const float *w;                          // null, or the class weights: model m's row is w + m * w_stride
    long w_stride;                           // 0 (one row [K] for all models: nsd_mixup) or K ([M][K]: nsd_mixup_each)
    float *targets;                          // [M*B][K]
    long n_el;                               // T * C
    int B, K, M;
    float mix[NSD_MAX_MODELS], eps[NSD_MAX_MODELS];   // model m's nsd_mix (nsd_mixup: M equal entries), read with the workgroup's m
    uint64_t seed[NSD_MAX_MODELS];
    uint32_t base[NSD_MAX_MODELS];
};
int nsd_mixup_launch(const MixArgs &a, hipStream_t st);
// cropped training (nsd_crop / nsd_crop_pool of nsd.h; nsd_crop.hip)
struct CropArgs {
    const float *x; float *y;                // [B,T,C] per model -> [M][B*R][W][C]
    long long x_stride;                      // floats between two models' trials (0: shared)
    const long long *step_dev;               // null, or the device step counter the stream id is formed from
    const int32_t *labels; int32_t *labels_out;      // null together, or [M*B] -> [M*B*R]
    const float *targets; float *targets_out;        // null together, or [M*B][K] -> [M*B*R][K]
    int32_t *offsets_out;                    // null, or [M*B*R]
    int B, T, C, K, M;
    int W, R, hop;                           // hop 0: drawn offsets; > 0: offset r * hop
    uint64_t seed[NSD_MAX_MODELS];
    uint32_t base[NSD_MAX_MODELS];
};
int nsd_crop_launch(const CropArgs &a, hipStream_t st);
struct CropPoolArgs {
    const float *probs;                      // [N][R][K]
    const int32_t *counts;                   // null (every trial counts R windows), or [N]
    float *probs_out, *logits_out;           // [N][K]; logits_out may be null
    int N, R, K;
};
int nsd_crop_pool_launch(const CropPoolArgs &a, hipStream_t st);
// the step's batch gathered from the resident trials (nsd_gather of nsd.h; nsd_gather.hip)
struct GatherArgs {
    const float *x_all; float *x;            // [N][T][C] -> [M][B][T][C]
    const int32_t *labels_all; int32_t *labels;      // null together, or [N] -> [M*B]
    const float *targets_all; float *targets;        // null together, or [N][K] -> [M*B][K]
    const int32_t *table;                    // [M][S][B] trial indices
    const long long *step_dev;               // null, or the device step counter the row is formed from
    long long step, step_base;               // row = (counter or step - step_base) mod S, non-negative
    int32_t *status;                         // null, or [M]: bit 0 = an index outside [0, N)
    long n_el;                               // T * C
    int B, K, M, N, S;
};
int nsd_gather_launch(const GatherArgs &a, hipStream_t st);
// gradient slabs of M models in one workspace: per model n LSTM slabs (one per backward workgroup) and n_h head slabs (one per trial)
struct SlabSet {
    const float *slabs; long stride; int n; long p_lstm;
    const float *hslabs; long ph; int n_h;
};
struct AdamStep { float *p, *m, *v; float lr, b1, b2, eps, wd, gscale; int step; };
// grads + m*P (+)= model m's slabs; adam != null: and the Adam update of p / m / v + m*P in the same launch (who: the entry point, for the texts)
int nsd_grad_reduce_launch(const SlabSet &s, int M, float *grads, int accumulate, const AdamStep *adam, const char *who, hipStream_t st);
int nsd_adam_launch(long n, float *p, const float *g, float *m, float *v, float lr, float b1, float b2, float eps,
                    float wd, float gscale, int step, const float *skip, hipStream_t st);
// global-norm clipping and learning-rate schedules (nsd_opt of nsd.h; nsd_optim.hip).  state: the caller's opt_state, already checked
// against nsd_opt_state_need(n or P, M); o: already through nsd_opt_check
int nsd_opt_check(const nsd_opt *o, const char *who);
double nsd_lr_factor_host(const nsd_opt *o, long long step);
int64_t nsd_opt_state_need(int64_t n, int M);
int nsd_opt_state_init_launch(void *state, int64_t bytes, hipStream_t st);
// weight averaging in the update launch (nsd_avg of nsd.h): avg already through nsd_avg_check, state against nsd_avg_state_need.
// each: avg has M entries.  A null NsdAvgSpec is the launch without averaging
struct NsdAvgSpec { const nsd_avg *avg; int each; void *state; };
int nsd_avg_check(const nsd_avg *a, const char *who, int allow_off);
int64_t nsd_avg_state_need(int64_t n, int M);
int nsd_reduce_clip_adam_launch(const SlabSet &s, int M, float *grads, float *p, float *m, float *v, const nsd_opt *o, int each, int step,
                                const long long *step_dev, void *state, const char *who, hipStream_t st,
                                const NsdAvgSpec *as = nullptr);   // each: o has M entries
int nsd_grad_norm_launch(long n, const float *g, float gscale, void *state, hipStream_t st);
int nsd_adam_clip_flat_launch(long n, float *p, const float *g, float *m, float *v, const nsd_opt *o, int step, const long long *step_dev,
                              const float *skip, void *state, hipStream_t st, const NsdAvgSpec *as = nullptr);
// sharpness-aware minimisation, the ascent (nsd_sam of nsd.h; nsd_optim.hip): the tail's first launch, then sam_ascend_kernel.  rho and
// gscale: M entries each, already checked; opt_state against nsd_opt_state_need, sam_state against nsd_sam_state_need
int nsd_sam_check(const nsd_sam *s, const char *who);
int64_t nsd_sam_state_need(int64_t n, int M);
int nsd_sam_ascend_slabs_launch(const SlabSet &s, int M, float *grads, const float *p, const float *rho, const float *gscale, void *opt_state,
                                void *sam_state, const char *who, hipStream_t st);
int nsd_sam_ascend_flat_launch(long n, const float *p, const float *g, float rho, float gscale, void *opt_state, void *sam_state, hipStream_t st);
int nsd_seq_guard_launch(const int *header, int status_word, float *flag_out, hipStream_t st);
int nsd_dropout_mask_launch(uint64_t seed, uint32_t stream_id, float p, long n, float *out, hipStream_t st);
int nsd_train_masks_launch(uint64_t seed, uint32_t base, const long long *step_dev, float p_lstm, float p_head, long n_lstm,
                           float *drop_lstm, long n_head, float *rrelu, float *drop_head, hipStream_t st);
int nsd_adam_dev_launch(long n, float *p, const float *g, float *m, float *v, float lr, float b1, float b2, float eps,
                        float wd, float gscale, const long long *step_dev, hipStream_t st);
int nsd_step_inc_launch(long long *step_dev, hipStream_t st);
int nsd_rrelu_noise_launch(uint64_t seed, uint32_t stream_id, long n, float *out, hipStream_t st);
// out[m] = sum of model m's B losses (per_model: the model-batched instantiation, nsd_multi_loss_sum's at M = 1 too)
int nsd_loss_sum_launch(const float *loss, int B, int M, bool per_model, float *out, const char *who, hipStream_t st);
// dx[r][c] = sum_k da0[r][k] * w_ih0[k][c]: r = (trial, step), k = gate * H + unit (nn.LSTM weight_ih_l0 is [4H][C] row-major)
int nsd_dx_launch(const float *da0, const float *w_ih0, float *dx, long rows, int G4, int C, hipStream_t st);
bool nsd_dx_ok(int G4, int C);            // the dx kernel's domain (C channels, 4H gate rows: W_ih0 staged in 64 KB of LDS)
// the same for M models in one launch: da0 [M][rows][G4], model m's matrix at w_ih0 + m * P, C <= 8.  mean: dx [rows][C], the serial fp32
// sum over m ascending / (float)M; else dx [M][rows][C], each model's rows bit for bit those of nsd_dx_launch
int nsd_multi_dx_launch(const float *da0, const float *w_ih0, long P, float *dx, long rows, int M, bool mean, int G4, int C, hipStream_t st);
// out[0] = the serial fp32 sum over m ascending of nsd_loss_sum_launch(per_model)'s M values / (float)M
int nsd_loss_mean_launch(const float *loss, int B, int M, float *out, const char *who, hipStream_t st);
// H = 48, input gradient requested: closes OPEN attention records (left by lstm2_fwd48x4 with defer_att) in front of lstm2_bwd48_kernel<1>
int nsd_att_close_launch(const float *hseq1, const float *pooled, const float *dpooled, float *adpack, float *dscore, float *hslabs,
                         long Ph, long o_attn_w, long o_attn_b, int B, int T, int H, hipStream_t st);

// resumable H = 48 inference (nsd_stream_* of nsd.h; nsd_stream48.hip).  One slot of the caller's state, in floats: the public layout
// nsd_stream_state_layout reports
constexpr int STREAM_H0 = 0, STREAM_H1 = 48, STREAM_C0 = 96, STREAM_C1 = 144, STREAM_ACC = 192, STREAM_MAX = 240, STREAM_DEN = 241,
              STREAM_STEPS = 242 /* int64: 8-byte aligned */, STREAM_STRIDE = 256;
struct StreamArgs {
    const float *x;                          // [B,T,C]: the chunk
    const float *w_ih0, *w_hh0, *b_ih0, *b_hh0, *w_ih1, *w_hh1, *b_ih1, *b_hh1;
    const float *attn_w, *attn_b, *ln_w, *ln_b, *fc0_w, *fc0_b, *fc3_w, *fc3_b;
    const int32_t *slots;                    // null: stream b lives in slot b
    float *state;                            // [S][STREAM_STRIDE]
    float *logits, *probs;                   // null: advance only / no class softmax
    float eval_slope;
    int B, T, C, K, F, S, residual;
};
int nsd_stream48_launch(const StreamArgs &a, hipStream_t st);
int nsd_stream_reset_launch(float *state, int S, const int32_t *slots, int n, hipStream_t st);

// session calibration (nsd_stream_features / nsd_head_fit of nsd.h; nsd_head_fit.hip).  The trainable tail of a model, in the flat order
// without the attention: ln.weight[H] ln.bias[H] fc.0.weight[F,H] fc.0.bias[F] fc.3.weight[K,F] fc.3.bias[K] -- Pt floats.  One model's
// fit state, in floats: m[Pt], v[Pt], the int64 epoch count (8-byte aligned), the int32 status word; the public nsd_fit_layout.
constexpr int FIT_H = 48, FIT_NT = 256;
constexpr int FIT_MAX_OWN = 29;              // tail elements per thread at F = K = 64: ceil(7392 / 256)
__host__ __device__ constexpr int fit_tail(int F, int K) { return 2 * FIT_H + F * FIT_H + F + K * F + K; }
__host__ __device__ constexpr int fit_epochs_off(int F, int K) { return (2 * fit_tail(F, K) + 1) & ~1; }
__host__ __device__ constexpr int fit_status_off(int F, int K) { return fit_epochs_off(F, K) + 2; }
__host__ __device__ constexpr int fit_stride(int F, int K) { return (fit_status_off(F, K) + 1 + 3) & ~3; }
// LDS image of the tail: fc.0's rows are FIT_H + 1 floats apart and fc.3's F | 1 (odd strides: a lane per row sweeps without conflicts)
__host__ __device__ constexpr int fit_w3s(int F) { return F | 1; }
__host__ __device__ constexpr int fit_image(int F, int K) { return 2 * FIT_H + F * (FIT_H + 1) + F + K * fit_w3s(F) + K; }
// floats of LDS of one workgroup: xhat[N][H], dln[N][H], z / dpre [N][F], dlogits [N][K], loss[N], sign bits [N][2], the tail's image,
// its gradient [Pt], two 64-float vectors per wave, and 8 words of flags and constants
__host__ __device__ constexpr long fit_lds_floats(int N, int F, int K) {
    return (long)N * (2 * FIT_H + F + K + 3) + fit_image(F, K) + fit_tail(F, K) + (FIT_NT / 64) * 128 + 8;
}
constexpr long FIT_LDS_MAX = 160 * 1024;     // bytes of LDS one workgroup may hold on gfx950
struct FitArgs {
    float *params; long P;                   // model m's flat vector at params + m * P
    long o_ln_w, o_ln_b, o_fc0_w, o_fc0_b, o_fc3_w, o_fc3_b;
    const float *feats; long feats_stride;   // [N][H] per model; 0: one set for all
    const float *targets;                    // [M*N][K]
    float *state;                            // [M][fit_stride]
    float *loss_out;                         // [M][epochs] or null
    int N, F, K, epochs;
    unsigned train;
    float lr, b1, b2, eps, wd, scale, eval_slope;
    int rng_on;
    uint64_t seed[NSD_MAX_MODELS];
    uint32_t base[NSD_MAX_MODELS], thr[NSD_MAX_MODELS];
    float keep[NSD_MAX_MODELS];
};
int nsd_head_fit_launch(const FitArgs &a, int M, hipStream_t st);
int nsd_stream_features_launch(const float *state, int S, const int32_t *slots, int n, float *feats, hipStream_t st);

// early stopping for model batches (nsd_multi_eval of nsd.h; nsd_eval.hip).  sel_state: M nsd_select_record, padded to 16 bytes, then the
// snapshot rows [M][P].  The counts travel by value, so a captured launch carries them.
constexpr int EVAL_NT = 256;
__host__ __device__ constexpr long eval_records_bytes(int M) { return ((long)M * (long)sizeof(nsd_select_record) + 15) & ~15L; }
struct EvalArgs {
    const float *logits;                     // [M*B][K]
    const int32_t *labels;                   // [M*B]
    nsd_eval_record *out;                    // [M]
    int B, K;
    int select, metric, patience;            // select 0: metrics only
    float min_delta;
    const float *params; long P;             // model m's row at params + m * P
    nsd_select_record *recs;                 // [M]
    float *best;                             // [M][P]
    int32_t counts[NSD_MAX_MODELS];
};
int nsd_multi_eval_launch(const EvalArgs &a, int M, hipStream_t st);

// sliding-window decisions (nsd_window_* of nsd.h; nsd_window48.hip).  One stream of the caller's state, in floats: R = window / hop PHASE
// SLOTS of STREAM_STRIDE floats in the layout above, then a header: the recorded window and hop (int32), two zero words, and one int64
// sample count PER PHASE.  Phase r's workgroup reads and writes its own copy only, so no workgroup of a launch reads a word that another
// one writes; between calls all copies are equal and phase 0's is the public one (nsd_window_layout.count).
constexpr int WINDOW_HDR_W = 0, WINDOW_HDR_HOP = 1, WINDOW_HDR_COUNT = 4 /* int64[R]: 8-byte aligned */;
__host__ __device__ constexpr int window_hdr_floats(int R) { return (WINDOW_HDR_COUNT + 2 * R + 3) & ~3; }
__host__ __device__ constexpr int window_stream_stride(int R) { return R * STREAM_STRIDE + window_hdr_floats(R); }
struct WindowArgs : StreamArgs {             // T: the chunk; logits / probs [B,D,K]
    long long *ends;                         // [B,D]
    int32_t *counts;                         // [B]
    int W, Hp, R, D;
};
int nsd_window48_launch(const WindowArgs &a, hipStream_t st);
int nsd_window_reset_launch(float *state, int S, const int32_t *slots, int n, int W, int Hp, hipStream_t st);

// causal front end (nsd_prep_* of nsd.h; nsd_prep.hip).  One slot of the caller's state, in floats -- the public layout
// nsd_prep_state_layout reports; it holds room for NSD_PREP_MAX_SECTIONS sections and depends on C alone
constexpr int PREP_X0 = 0;
constexpr int PREP_TT = 32;                  // time steps staged through LDS at once
constexpr int PREP_GRID_CAP = 1024;          // workgroups of a launch; larger calls walk their stream groups grid-stride
__host__ __device__ constexpr int prep_z(int C, int s, int k) { return C + (2 * s + k) * C; }   // z[s][k][C], k = 0: z1, 1: z2
__host__ __device__ constexpr int prep_mu(int C) { return (1 + 2 * NSD_PREP_MAX_SECTIONS) * C; }
__host__ __device__ constexpr int prep_var(int C) { return (2 + 2 * NSD_PREP_MAX_SECTIONS) * C; }
__host__ __device__ constexpr int prep_steps(int C) { return ((3 + 2 * NSD_PREP_MAX_SECTIONS) * C + 1) & ~1; }   // int64: 8-byte aligned
__host__ __device__ constexpr int prep_stride(int C) { return (prep_steps(C) + 2 + 3) & ~3; }
struct CausalPrepArgs {
    const float *x; float *y;                // [B,T,C]; y == x allowed
    const int32_t *slots;                    // null: stream b lives in slot b
    float *state;                            // null: window mode (every trial from a reset state, nothing stored)
    int B, T, C, S;
    int baseline, car, ns, zs;               // zs: alpha > 0
    float sos[NSD_PREP_MAX_SECTIONS][5];     // b0 b1 b2 a1 a2
    float alpha, oma, var0;                  // oma = 1.0f - alpha
};
int nsd_prep_launch(const CausalPrepArgs &a, hipStream_t st);
int nsd_prep_reset_launch(float *state, int C, int S, const int32_t *slots, int n, hipStream_t st);

// rate conversion (nsd_resample_* of nsd.h; nsd_resample.hip).  One slot of the caller's state in 4-byte words -- the public layout
// nsd_resample_state_layout reports; it depends on (C, P): hist[P-1][C] fp32, then the int64 n_in
constexpr int RS_HIST = 0;
constexpr int RS_TI = 256;                   // input samples staged through LDS at once (with the P - 1 in front of them)
constexpr int RS_GRID_CAP = 1024;            // workgroups of a launch; larger calls walk their work units grid-stride
constexpr int RS_TAPS_LDS = 768;             // the tap table [L][P] lives in LDS up to this many floats, else it is read through the caches
constexpr long long RS_MAX_N_IN = 1LL << 40; // a slot's n_in beyond it (or below 0) was never reset: the slot is skipped
__host__ __device__ constexpr int rs_n_in(int C, int P) { return ((P - 1) * C + 1) & ~1; }   // int64: 8-byte aligned
__host__ __device__ constexpr int rs_stride(int C, int P) { return (rs_n_in(C, P) + 2 + 3) & ~3; }
__host__ __device__ constexpr long long rs_ceil_div(long long a, long long b) { return (a + b - 1) / b; }   // a >= 0, b > 0
struct ResampleArgs {
    const float *x; float *y;                // [B,T,C], [B,To,C]; no overlap
    const float *taps;                       // [L][P]
    const int32_t *slots;                    // null: stream b lives in slot b
    float *state;                            // null: window mode (every trial from rest, nothing stored)
    int32_t *cnt;                            // null, or [B]
    long long To;
    int B, T, C, S;
    int L, M, P;
};
int nsd_resample_launch(const ResampleArgs &a, hipStream_t st);
int nsd_resample_reset_launch(float *state, int stride, int S, const int32_t *slots, int n, hipStream_t st);

// signal-quality gate (nsd_gate_* of nsd.h; nsd_gate.hip).  One slot of the caller's state in 4-byte words -- the public layout
// nsd_gate_state_layout reports; it depends on C alone.  prev / held / ring are fp32, run / hang int32, bad / rejected / steps int64
constexpr int GATE_SPAN = NSD_GATE_MAX_SPAN;                          // rows of the ring, the longest peak-to-peak span
constexpr int GATE_PREV = 0;
__host__ __device__ constexpr int gate_held(int C) { return C; }
__host__ __device__ constexpr int gate_run(int C) { return 2 * C; }
__host__ __device__ constexpr int gate_hang(int C) { return 3 * C; }
__host__ __device__ constexpr int gate_ring(int C) { return 4 * C; }   // ring[GATE_SPAN][C]
__host__ __device__ constexpr int gate_bad(int C) { return ((4 + GATE_SPAN) * C + 1) & ~1; }   // int64[C]: 8-byte aligned
__host__ __device__ constexpr int gate_rejected(int C) { return gate_bad(C) + 2 * C; }
__host__ __device__ constexpr int gate_steps(int C) { return gate_rejected(C) + 2; }
__host__ __device__ constexpr int gate_stride(int C) { return (gate_steps(C) + 2 + 3) & ~3; }
struct GateArgs {
    const float *x; float *y;                // [B,T,C]; y == x allowed
    uint32_t *mask;                          // [B,T]: bit c set where channel c is bad
    const int32_t *slots;                    // null: stream b lives in slot b
    float *state;                            // null: window mode (every trial from a reset state, nothing stored)
    int B, T, C, S;
    float rail, jump, flat_eps, pp;
    int flat_samples, pp_samples, hold_samples, max_bad;
};
int nsd_gate_launch(const GateArgs &a, hipStream_t st);
int nsd_gate_reset_launch(float *state, int C, int S, const int32_t *slots, int n, hipStream_t st);
struct GateApplyArgs {
    const float *v; const uint32_t *mask; float *out;   // v, out [B,T,C] (out == v allowed), mask [B,T]
    long steps;                              // B * T
    int C, max_bad, zero;
};
int nsd_gate_apply_launch(const GateApplyArgs &a, hipStream_t st);

// session alignment (nsd_cov_* / nsd_whiten_fit / nsd_spatial_apply of nsd.h; nsd_align.hip).  One slot of a cov state in 8-byte words --
// the public layout nsd_cov_state_layout reports: sum[C][C] double, then count and skipped (int64)
constexpr int COV_SUM = 0;
__host__ __device__ constexpr int cov_count(int C) { return C * C; }
__host__ __device__ constexpr int cov_skipped(int C) { return C * C + 1; }
__host__ __device__ constexpr int cov_stride(int C) { return C * C + 2; }
struct CovArgs {
    const float *v; const uint32_t *mask;    // [B,T,C]; null, or [B,T]
    const int32_t *slots;                    // null: stream b lives in slot b
    double *state;                           // null: window mode (every trial from zero, results to sums / counts)
    double *sums; long long *counts;         // window mode: [B][C][C], [B][2]
    int B, T, C, S;
};
int nsd_cov_launch(const CovArgs &a, hipStream_t st);
int nsd_cov_reset_launch(double *state, int C, int S, const int32_t *slots, int n, hipStream_t st);
struct WhitenArgs {
    const double *sums; const long long *counts; long sum_stride, count_stride;
    const int32_t *group;                    // null: every accumulator in group 0
    float *W; nsd_whiten_record *records;    // [G][C][C], [G]
    int C, N, G, min_steps;
    double shrinkage, floor;
};
int nsd_whiten_launch(const WhitenArgs &a, hipStream_t st);
struct SpatialArgs {
    const float *v; const float *W; const int32_t *sel; float *out;   // v, out [B,T,C] (out == v allowed), W [n_mat][C][C], sel null or [B]
    int B, T, C, n_mat;
};
int nsd_spatial_launch(const SpatialArgs &a, hipStream_t st);

// supervised session alignment (nsd_spatial_bwd / nsd_spatial_fit_step of nsd.h; nsd_align.hip).  One matrix's slot of a fit state in
// BYTES -- the public layout nsd_spatial_fit_state_layout reports: m[C][C], v[C][C] (float), step, skipped (int64), status, reserved
// (uint32); the int64 call counter follows the last slot
__host__ __device__ constexpr long sfit_m(int) { return 0; }
__host__ __device__ constexpr long sfit_v(int C) { return 4L * C * C; }
__host__ __device__ constexpr long sfit_step(int C) { return 8L * C * C; }
__host__ __device__ constexpr long sfit_skipped(int C) { return 8L * C * C + 8; }
__host__ __device__ constexpr long sfit_status(int C) { return 8L * C * C + 16; }
__host__ __device__ constexpr long sfit_stride(int C) { return 8L * C * C + 24; }
struct SpatialBwdArgs {
    const float *v, *dy, *W; const int32_t *sel;   // v, dy [B,T,C]; W [n_mat][C][C]; sel null or [B]
    float *dv, *dW;                          // null, or [B,T,C]; null, or [n_mat][C][C]
    long long *counts;                       // null, or {rows used, rows left out} (written with dW)
    double *p;                               // scratch [B][C][C]: stage 1 of dW
    int B, T, C, n_mat;
};
int nsd_spatial_bwd_launch(const SpatialBwdArgs &a, hipStream_t st);
struct SpatialFitArgs {
    float *A; const float *A0, *dW;          // [n_mat][C][C]; A0 null: no pull
    unsigned char *state;                    // n_mat slots, then the call counter
    const float *loss_in; float *loss_out; int loss_cap;
    int C, n_mat;
    float lr, b1, b2, eps, decay;
};
int nsd_spatial_fit_launch(const SpatialFitArgs &a, hipStream_t st);
