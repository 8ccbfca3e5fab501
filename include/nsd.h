/*
 * nsd.h -- C ABI of libnsd_hip.so: the MI355X (gfx950) implementation of the
 * EEG_LSTM hot path of aa217/Neural-Speech-Decoding.
 *
 * The reference has NO native interface: its hot path is a torch nn.Module
 * (Neuro-Alpha-App/Utilities/lstm_eeg_model.py:13-39) called through
 * SimplePredictor.predict (lstm_eeg_model.py:86-101).  Each entry point below
 * names the reference lines whose arithmetic it replaces; the Python facade in
 * neural-speech-decoding_amd/ binds them with ctypes (INTEGRATION.md shows the
 * stub a reference maintainer would add).
 *
 * Conventions
 *   - plain C symbols, no C++/torch types; every function returns int:
 *     0 = ok, <0 = error (NSD_E_*); nsd_last_error() gives thread-local text.
 *   - every entry point that reads or writes the training workspace takes `workspace_bytes`, the size of the
 *     caller's buffer, and returns NSD_E_WORKSPACE (launching nothing) when it is smaller than
 *     nsd_workspace_bytes(d) -- a C caller cannot be overrun.
 *   - the CALLER owns every buffer.  All pointers are DEVICE pointers (fp32
 *     unless stated) valid on the current HIP device; the library allocates
 *     nothing and never synchronises: work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the legacy default stream).
 *   - buffer contents before a call are never read unless documented (an output, a workspace or a scratch buffer may hold
 *     arbitrary bytes, NaN patterns and the leftovers of another shape included; a training workspace carries one
 *     evaluation from its forward call to the calls that follow it, and the sequence workspace keeps its header), nothing
 *     outside the stated extents is written (a workspace or scratch buffer of exactly the size its *_bytes function returns
 *     is enough), inputs are never written.
 *   - re-entrant per stream; kernels are deterministic (no float atomics).
 *   - shapes: B trials, T time steps, C channels, H hidden, L layers,
 *     K classes, F = width of the first dense layer (32 in the reference).
 *
 * Flat parameter vector (same order as the reference state_dict, so the
 * reference .pth maps 1:1; see nsd_param_layout):
 *   for l in 0..L-1: lstm.weight_ih_l{l}[4H,I_l] lstm.weight_hh_l{l}[4H,H]
 *                    lstm.bias_ih_l{l}[4H] lstm.bias_hh_l{l}[4H]   (I_0=C, I_l=H)
 *   ln.weight[H] ln.bias[H] attn.weight[H] attn.bias[1]
 *   fc.0.weight[F,H] fc.0.bias[F] fc.3.weight[K,F] fc.3.bias[K]
 */
#ifndef NSD_H
#define NSD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NSD_VERSION 301          /* 0.3.1: nsd_lstm_bwd's dx is right after every forward of the batch (the fused head's open
                                    attention records included), refused before any launch outside its domain; nsd_dx_path.
                                    0.3.0: sequence-batched path: persistent workspace header (nsd_seq_workspace_init), sticky
                                    status, nsd_seq_guard / nsd_adam_step_guarded; diagnostics left the shipped library */
#define NSD_MAX_LAYERS 8
#define NSD_MAX_MODELS 32        /* nsd_multi_*: models per launch.  The model-batched entry points are additive and leave NSD_VERSION
                                    at 301: a caller detects them with nsd_multi_path (a library without them lacks the symbol) */

#define NSD_OK            0
#define NSD_E_INVALID    -1      /* bad argument / unsupported shape */
#define NSD_E_LAUNCH     -2      /* HIP launch or runtime error */
#define NSD_E_WORKSPACE  -3      /* workspace_bytes < nsd_workspace_bytes(d): nothing was launched */

/* flags */
#define NSD_FLAG_RESIDUAL   1u   /* extension (not in the reference): out_l = LSTM_l(in_l) + in_l, l>=1 */
#define NSD_FLAG_TRAIN      2u   /* keep activations in the workspace for nsd_*_bwd */
#define NSD_FLAG_BIDIR      8u   /* nsd_seq_* entry points only: bidirectional LSTM (torch.nn.LSTM(bidirectional=True)); the
                                    sequence fed to the attention pooling and the head is 2H wide */
#define NSD_FLAG_BF16       4u   /* large-H batched path only (H % 16 == 0, H >= 64, B >= 16; ignored elsewhere): GEMM operands
                                    rounded to bf16 at the matrix pipe (fp32 accumulate, fp32 storage and cell arithmetic) --
                                    BASELINE cfg3's precision; results differ from fp32 at the 1e-2 level */

typedef struct nsd_dims {
    int32_t B, T, C, H, L, K, F;
} nsd_dims;

/* word offsets (units of float) of the regions inside the training workspace */
typedef struct nsd_ws_layout {
    int64_t hseq;      /* [L,B,T,H]   h_t of every layer (LSTM's own output)          */
    int64_t cseq;      /* [L,B,T,H]   c_t                                              */
    int64_t gact;      /* [L,B,T,H,4] activated gates, unit-major: (i,f,g,o) per unit  */
    int64_t inseq;     /* [L-1,B,T,H] input fed to layer l+1 (after residual+dropout)  */
    int64_t top;       /* [B,T,H]     sequence fed to attention (== hseq[L-1] unless residual) */
    int64_t alpha;     /* [B,T]       attention weights                                */
    int64_t pooled;    /* [B,H]                                                        */
    int64_t fc0_pre;   /* [B,F]       pre-activation of fc.0                           */
    int64_t dscore;    /* [B,T]       d loss / d attention score  (head_bwd -> lstm_bwd) */
    int64_t dpooled;   /* [B,H]       d loss / d pooled           (head_bwd -> lstm_bwd) */
    int64_t loss;      /* [B]         per-trial CE loss                                */
    int64_t adpack;    /* [B,T,4]     {alpha, dscore, 0, 0} per step: 16-byte records for the LSTM backward's LDS-DMA */
    int64_t slabs;     /* [n_slabs,P_lstm] per-workgroup partial gradients of the LSTM stack */
    int64_t n_slabs;
    int64_t hslabs;    /* [B,P_head]  per-trial gradients of ln/attn/fc                  */
    int64_t da_seq;    /* [B,T,4H]    generic path only: pre-activation gradients of the layer in flight */
    int64_t din;       /* [2,B,T,H]   generic path only: gradient w.r.t. a layer's input (ping-pong)      */
    int64_t total;     /* floats */
} nsd_ws_layout;

int         nsd_version(void);
const char *nsd_last_error(void);

/* number of floats in the flat parameter vector; <0 on bad dims */
int64_t nsd_param_count(int32_t C, int32_t H, int32_t L, int32_t K, int32_t F);
/* offsets[4L+8]: per layer w_ih,w_hh,b_ih,b_hh; then ln.w ln.b attn.w attn.b fc0.w fc0.b fc3.w fc3.b */
int     nsd_param_layout(int32_t C, int32_t H, int32_t L, int32_t K, int32_t F, int64_t *offsets);

/* workspace needed by the train-mode calls for these dims, in BYTES; layout optional */
int64_t nsd_workspace_bytes(const nsd_dims *d, nsd_ws_layout *layout_out);

/* 1 if the fused register-resident kernels cover these dims (H in {32,48,64}, L==2, C<=8), else 0: the shape-generic
 * per-layer kernels (nsd_lstm_generic.hip) are used -- same results, not tuned */
int     nsd_fast_path(const nsd_dims *d);

/*
 * Per-channel z-score over time, y = (x - mean_T) / (std_T(ddof=0) + 1e-6).
 * Replaces normalize_eeg, Neuro-Alpha-App/Frontend/app.py:166-170.  x,y [B,T,C]; in-place allowed.
 */
int nsd_zscore_fwd(const float *x, float *y, int32_t B, int32_t T, int32_t C, void *stream);

/*
 * Inference: x[B,T,C] -> logits[B,K] (+ probs[B,K] if non-NULL).
 * Replaces EEG_LSTM.forward in eval mode (lstm_eeg_model.py:32-39) and the class
 * softmax of SimplePredictor.predict (lstm_eeg_model.py:97).
 * scratch: device buffer of nsd_infer_scratch_bytes(d) bytes.
 */
int64_t nsd_infer_scratch_bytes(const nsd_dims *d);
int nsd_infer(const nsd_dims *d, const float *params, const float *x, uint32_t flags,
              float *logits, float *probs, void *scratch, void *stream);

/*
 * Stacked LSTM forward (lstm_eeg_model.py:34, self.lstm(x)), train mode.
 * drop_lstm: NULL, or multiplier masks [L-1,B,T,H] (0 or 1/(1-p)) applied to the output of every
 *            layer but the last (nn.LSTM(dropout=p), lstm_eeg_model.py:21).
 * Fills hseq/cseq/gact/inseq/top of the workspace.
 */
int nsd_lstm_fwd(const nsd_dims *d, const float *params, const float *x, const float *drop_lstm,
                 uint32_t flags, float *workspace, int64_t workspace_bytes, void *stream);

/*
 * Head forward: attention pooling over time, LayerNorm, fc (lstm_eeg_model.py:35-39),
 * optional class softmax (lstm_eeg_model.py:97).  Reads `top` from the workspace.
 * rrelu_slope: NULL -> eval slope (lower+upper)/2, else per-element slopes [B,F] (train-mode RReLU noise)
 * drop_head:   NULL or multiplier mask [B,F] (nn.Dropout, lstm_eeg_model.py:28)
 */
int nsd_head_fwd(const nsd_dims *d, const float *params, const float *rrelu_slope, const float *drop_head,
                 float *workspace, int64_t workspace_bytes, float *logits, float *probs, void *stream);

/*
 * Head backward.  Either dlogits[B,K] is given, or labels[B] (int32) with `scale`:
 * then dlogits = (softmax(logits) - onehot(label)) * scale (mean CE when scale = 1/B_global) and the
 * per-trial CE loss is written to the workspace's `loss` region.  Writes dscore/dpooled for
 * nsd_lstm_bwd and the head's partial gradients into the slabs.
 */
int nsd_head_bwd(const nsd_dims *d, const float *params, const float *rrelu_slope, const float *drop_head,
                 const float *logits, const float *dlogits, const int32_t *labels, float scale,
                 float *workspace, int64_t workspace_bytes, void *stream);

/*
 * Train-step head: nsd_head_fwd + mean cross-entropy + nsd_head_bwd of every trial in ONE launch (sequence and head
 * parameters staged in LDS once).  Same workspace outputs as the two separate calls; logits[B,K] is written too.
 */
int nsd_head_train(const nsd_dims *d, const float *params, const float *rrelu_slope, const float *drop_head,
                   const int32_t *labels, float scale, float *workspace, int64_t workspace_bytes, float *logits, void *stream);

/*
 * nsd_lstm_fwd + nsd_head_train in ONE launch where the shape allows (H = 48, L = 2, T <= 1024, F <= 64, K <= 8: the
 * attention pooling rides along the recurrence and the dense head, loss and head backward run in the kernel's tail);
 * other shapes run the two launches it replaces.  Same outputs, workspace contents and gradient slabs either way --
 * except that the single launch does not write the workspace's `top` region when the residual extension is off (it
 * would duplicate the last layer's hseq, which nsd_lstm_bwd and the kernel's own tail read instead).
 */
int nsd_lstm_head_train(const nsd_dims *d, const float *params, const float *x, const float *drop_lstm,
                        const float *rrelu_slope, const float *drop_head, const int32_t *labels, float scale, uint32_t flags,
                        float *workspace, int64_t workspace_bytes, float *logits, void *stream);

/*
 * Train-mode random streams generated INSIDE the kernels (no mask tensors in HBM): the three streams of one step are
 * value(seed, base_stream + {0: LSTM inter-layer dropout [B,T,H], 1: RReLU slope [B,F], 2: head dropout [B,F]}, index),
 * the same pure function as nsd_train_masks / oracle -- a step run this way is bit-identical to the same step run with
 * the masks of nsd_train_masks passed explicitly.  Only where nsd_rng_path(d) != 0 (the single-launch H = 48 shape: L = 2, C <= 8,
 * T <= 1024, F <= 64, K <= 8); elsewhere both entry points return NSD_E_INVALID before any launch and nsd_last_error names these limits.
 */
typedef struct nsd_rng {
    uint64_t seed;
    uint32_t base_stream;
    float p_lstm, p_head;
} nsd_rng;
int nsd_rng_path(const nsd_dims *d);
int nsd_lstm_head_train_rng(const nsd_dims *d, const float *params, const float *x, const nsd_rng *rng, const int32_t *labels,
                            float scale, uint32_t flags, float *workspace, int64_t workspace_bytes, float *logits, void *stream);
int nsd_lstm_bwd_rng(const nsd_dims *d, const float *params, const float *x, const nsd_rng *rng, uint32_t flags,
                     float *workspace, int64_t workspace_bytes, void *stream);

/*
 * Stacked LSTM backward (BPTT) through lstm_eeg_model.py:34 with the activations kept by nsd_lstm_fwd.
 * Partial gradients go to the slabs.  dx (optional, may be NULL): dL/dx [B,T,C], what autograd through self.lstm(x)
 * (lstm_eeg_model.py:34) returns for the EEG window -- formed as da0 . W_ih0 behind the backward pass, for H = 48 (L = 2, C <= 8; the
 * one-trial kernel then runs whatever the batch and leaves da0 IN PLACE of layer 0's saved gates: one backward per forward) and on the
 * shape-generic path with C <= 64 and 4H * C * 4 <= 64 KB.  With H = 48 it follows either forward, nsd_lstm_fwd + a head or
 * nsd_lstm_head_train at any batch: where the fused head left the attention's per-step backward to the four-trial backward kernel (from
 * 513 trials), a small kernel forms it first (dL/dscore, d attn.weight, d attn.bias), and every gradient is the one dx = NULL gives.
 * Where nsd_dx_path(d) == 0 a non-NULL dx returns NSD_E_INVALID and launches nothing.  The parameter gradients never need it.
 */
int nsd_dx_path(const nsd_dims *d);       /* 1 where nsd_lstm_bwd forms dx for these dims, 0 elsewhere (and for invalid dims) */
int nsd_lstm_bwd(const nsd_dims *d, const float *params, const float *x, const float *drop_lstm,
                 uint32_t flags, float *workspace, int64_t workspace_bytes, float *dx, void *stream);

/* grads[P] (=|+=) sum over slabs.  accumulate: 0 overwrite, 1 add to existing. */
int nsd_grad_reduce(const nsd_dims *d, const float *workspace, int64_t workspace_bytes, float *grads, int32_t accumulate, void *stream);

/* Single-rank train step tail: nsd_grad_reduce (grads[] is still written) followed, in the same launch, by
 * nsd_adam_step on the reduced gradient -- same arithmetic in the same order as the two separate calls.  With more
 * than one rank the all-reduce sits between the two and the separate entry points are used. */
int nsd_grad_reduce_adam(const nsd_dims *d, const float *workspace, int64_t workspace_bytes, float *grads, float *p, float *m, float *v, float lr,
                         float beta1, float beta2, float eps, float weight_decay, float grad_scale, int32_t step, void *stream);

/* sum of the per-trial losses written by nsd_head_bwd -> out[0] (device) */
int nsd_loss_sum(const nsd_dims *d, const float *workspace, int64_t workspace_bytes, float *out, void *stream);

/* torch.optim.Adam semantics (no amsgrad); step counted from 1; all vectors length n */
int nsd_adam_step(int64_t n, float *p, const float *g, float *m, float *v, float lr, float beta1, float beta2,
                  float eps, float weight_decay, float grad_scale, int32_t step, void *stream);
/* the same update, skipped entirely (p, m, v untouched) when the device flag skip[0] != 0: see nsd_seq_guard */
int nsd_adam_step_guarded(int64_t n, float *p, const float *g, float *m, float *v, float lr, float beta1, float beta2,
                          float eps, float weight_decay, float grad_scale, int32_t step, const float *skip, void *stream);

/*
 * Counter-based random streams of the trainer (the reference's training RNG is torch's and is not
 * portable): value(seed, stream, index) is a pure function, identical in oracle/nsd_oracle.c.
 *   nsd_dropout_mask: out[i] = keep ? 1/(1-p) : 0       nsd_rrelu_noise: out[i] ~ U(1/8, 1/3)
 */
int nsd_dropout_mask(uint64_t seed, uint32_t stream_id, float p, int64_t n, float *out, void *stream);
/* the three streams of one train step in one launch: drop_lstm[n_lstm] = stream base, rrelu_slope[n_head] = base+1,
 * drop_head[n_head] = base+2 (bit-identical to the three separate calls) */
int nsd_train_masks(uint64_t seed, uint32_t base_stream, float p_lstm, float p_head, int64_t n_lstm, float *drop_lstm,
                    int64_t n_head, float *rrelu_slope, float *drop_head, void *stream);
int nsd_rrelu_noise(uint64_t seed, uint32_t stream_id, int64_t n, float *out, void *stream);

/*
 * hipGraph-friendly variants: whatever changes from step to step (the Adam step number, the random-stream ids) is read
 * from a device-side counter instead of being a kernel argument, so that one captured graph can be replayed.
 *   nsd_step_counter_inc  step_dev[0] += 1 (int64, device); call it first in the captured step
 *   nsd_train_masks_dev   like nsd_train_masks with base_stream = 4 * (step_dev[0] & 0x3fffffff)
 *   nsd_adam_step_dev     like nsd_adam_step with step = step_dev[0]
 */
int nsd_step_counter_inc(int64_t *step_dev, void *stream);
int nsd_train_masks_dev(uint64_t seed, const int64_t *step_dev, float p_lstm, float p_head, int64_t n_lstm, float *drop_lstm,
                        int64_t n_head, float *rrelu_slope, float *drop_head, void *stream);
int nsd_adam_step_dev(int64_t n, float *p, const float *g, float *m, float *v, float lr, float beta1, float beta2, float eps,
                      float weight_decay, float grad_scale, const int64_t *step_dev, void *stream);

/*
 * ---- trial augmentation for the trainers (an EXTENSION: the reference's training notebook is missing and has none) ----
 *
 * x[B,T,C] -> y[B,T,C] (fp32) per model, every draw a pure function of (seed, stream, index) like the dropout streams, so a test can
 * restate a launch bit for bit.  Stream: rng[m].base_stream + 3 (the trainers number a step's streams 4 * step + {0, 1, 2}; + 3 is this
 * one), seed rng[m].seed; p_lstm / p_head are ignored.  With R(i) = value(seed, base_stream + 3, i) and U(r) = float(r >> 8) * 2^-24:
 *   per-trial draws    index P(b, slot) = 2^63 | (uint64(b) << 16) | slot
 *   per-element draws  index E(b, t, c) = (b * T + t) * C + c                       (top bit clear: the two never collide)
 * b is the trial's index inside ITS model's batch, so model m draws what a single-model call with rng[m] draws.  Four operations, in this
 * order, each SKIPPED when its parameter is 0 (all four off: y is a bitwise copy of x):
 *   max_shift S    s_b = int(R(P(b, 0)) % (2S + 1)) - S;  v = x[b, clamp(t - s_b, 0, T - 1), c]   (edge sample repeated)
 *   scale_range r  a_b = 1 + r * (2 U(R(P(b, 1))) - 1);   v = a_b * v                              (one factor per trial)
 *   noise_std s    q = R(E(b, t, c)), n = float(sum of the four bytes of q - 510);  v = v + sk * n, sk = float(double(s) / sqrt(21845))
 *                  (the byte sum has mean 510 and variance 21845: unit-variance Irwin-Hall(4) noise, bounded by +-3.45 s)
 *   p_channel p    channel c of trial b is dropped when R(P(b, 256 + c)) < floor(p * 2^32):  v = 0 for its whole window (no rescaling)
 * Every fp32 operation rounds on its own (no FMA contraction).  NSD_AUG_ZSCORE: y = the per-channel z-score of the augmented window,
 * bitwise what nsd_zscore_fwd gives on the unfused output.
 *   x_model_stride  floats between two models' windows; 0: every model augments the same windows with its own draws
 *   step_dev        NULL, or a device step counter: base_stream = 4 * (step_dev[0] & 0x3fffffff) for every model, as nsd_train_masks_dev
 * NSD_E_INVALID before any launch: M outside [1, NSD_MAX_MODELS]; NULL x / y / aug / rng; max_shift < 0 or >= T; scale_range or
 * p_channel outside [0, 1); noise_std negative or not finite; C outside [1, 256]; T < 1; a negative x_model_stride or one in
 * (0, B*T*C); y overlapping x.  B = 0 launches nothing.  Only d->B, T, C are read.  Additive: NSD_VERSION stays 301, a caller detects
 * the feature by the symbol.
 */
typedef struct nsd_aug {
    int32_t max_shift;
    float scale_range, p_channel, noise_std;
} nsd_aug;
#define NSD_AUG_ZSCORE 1u
int nsd_augment_path(const nsd_dims *d);       /* 1 where nsd_augment covers d->B / T / C, else 0 */
int nsd_augment(const nsd_dims *d, int32_t M, const float *x, int64_t x_model_stride, const nsd_aug *aug, const nsd_rng *rng,
                const int64_t *step_dev, uint32_t flags, float *y, void *stream);

/*
 * ---- soft targets: label smoothing, class weights, mixup, distillation in the fused train step (an EXTENSION) ----
 *
 * Every fused head forms its loss either from int32 labels (the entry points above and below) or, through the `_soft` twins, from a
 * per-trial target row q[b, 0..K) (device fp32, finite, q >= 0, any row sum s_b = sum_k q[b,k]):
 *   loss_b     = - sum_k q[b,k] * log softmax(logits_b)[k]
 *   dlogits_bk = scale * (s_b * p_bk - q[b,k])
 * which is torch.nn.functional.cross_entropy(logits, target_probs, weight=w, label_smoothing=eps) when q holds
 * w_k * ((1 - eps) * target_k + eps / K) -- up to the normalisation: `scale` stays the caller's (1 / B_global in the trainers), where
 * torch's weighted `mean` divides by the sum of the weights instead.  A zero row is a trial that contributes nothing.  s p_k - q_k is
 * formed as (sum_{j != k} (q_j e_k - q_k e_j)) / d, e = exp(logits - max), d = sum e: like the hard path's p_y - 1 = -(sum of the others) / d
 * it has no O(1) - O(1) difference; the loss is sum_k q_k ((max - logit_k) + log d).  One-hot rows reproduce the hard-label entry point
 * (same logits bit for bit, same gradients up to the order of a K-term sum).
 * Each `_soft` entry point is its hard-label twin with `targets` ([B,K]; [M*B][K] for nsd_multi_*) in place of `labels`: same domain,
 * fallbacks, workspace contents, refusals and NSD_E_WORKSPACE behaviour; the backward calls that follow are the existing ones
 * (nsd_lstm_bwd[_rng], nsd_multi_train_bwd, nsd_seq_train_bwd[_dx]) and nsd_loss_sum / nsd_multi_loss_sum / nsd_seq_loss_sum read the
 * soft loss.  nsd_lstm_head_train_soft is the twin of nsd_lstm_head_train (rng == NULL: explicit mask tensors, each may be NULL) AND of
 * nsd_lstm_head_train_rng (rng != NULL: the three mask pointers must be NULL; NSD_E_INVALID where nsd_rng_path(d) == 0); outside the
 * single-launch shape it runs nsd_lstm_fwd + nsd_head_train_soft.  Additive: NSD_VERSION stays 301, a caller detects the feature by
 * the symbols.
 */
int nsd_head_train_soft(const nsd_dims *d, const float *params, const float *rrelu_slope, const float *drop_head,
                        const float *targets, float scale, float *workspace, int64_t workspace_bytes, float *logits, void *stream);
int nsd_lstm_head_train_soft(const nsd_dims *d, const float *params, const float *x, const float *drop_lstm, const float *rrelu_slope,
                             const float *drop_head, const nsd_rng *rng, const float *targets, float scale, uint32_t flags,
                             float *workspace, int64_t workspace_bytes, float *logits, void *stream);

/*
 * nsd_mixup: the target rows of a step from its labels -- label smoothing, class weights -- and, with mix > 0, mixed windows, in ONE
 * launch for all models.  Per model, with b the trial's index inside ITS model's batch, R(i) = value(seed, base_stream + 3, i),
 * U(r) = float(r >> 8) * 2^-24 and P(b, slot) as for nsd_augment (the slots used here are ones nsd_augment leaves alone: an augmented
 * step's draws do not move):
 *   partner   r = 1 + R(2^63 | 2^62) mod (B - 1)  (B >= 2),  p(b) = (b + r) mod B: a rotation of the batch, a bijection, never b itself
 *   weights   lambda_b = 1 - mix * U(R(P(b, 1024))),  mu_b = 1 - lambda_b      (mix in [0, 1]; mix = 1: lambda uniform, Beta(1, 1) mixup)
 *   base(j)[k] = w_k * (k == j ? (1 - eps) + eps / K : eps / K)                 (class_weight == NULL: no multiply)
 *   y[b]         = lambda_b * x[b] + mu_b * x[p(b)]
 *   targets[b,k] = lambda_b * base(label_b)[k] + mu_b * base(label_p(b))[k]
 * Every fp32 operation rounds on its own (no FMA contraction), in this order: ek = eps / float(K); on = (1 - eps) + ek;
 * base = k == j ? on : ek, then w_k * base; m = mix * U; lambda = 1 - m; mu = 1 - lambda; out = (lambda * a) + (mu * b) for the
 * windows and the targets alike.  mix == 0 or B == 1: nothing is mixed -- y is a bitwise copy of x and targets[b] = base(label_b)
 * exactly (no multiplication by lambda = 1); with mix == 0, x and y may both be NULL and the launch only builds targets.  eps == 0,
 * class_weight == NULL, mix == 0: one-hot rows.  A label outside [0, K) gives the row of no class (eps / K everywhere).
 *   x_model_stride, rng[m], step_dev   as for nsd_augment (p_lstm / p_head are ignored); labels [M*B], y [M*B][T*C], targets [M*B][K]
 * NSD_E_INVALID before any launch: M outside [1, NSD_MAX_MODELS]; NULL labels / targets / mix / rng; smoothing outside [0, 1); mix
 * outside [0, 1]; K outside [1, 64]; T or C < 1; x / y NULL with mix > 0, or only one of the two given; a negative x_model_stride or
 * one in (0, B*T*C); y overlapping x.  B = 0 launches nothing.  Only d->B, T, C, K are read.  Additive, detected by the symbol.
 */
typedef struct nsd_mix {
    float mix, smoothing;
} nsd_mix;
int nsd_mixup(const nsd_dims *d, int32_t M, const float *x, int64_t x_model_stride, const int32_t *labels,
              const float *class_weight /* NULL or [K] device */, const nsd_mix *mix, const nsd_rng *rng, const int64_t *step_dev,
              float *y, float *targets /* [M*B][K] */, void *stream);

/*
 * ---- cropped training: random or regular windows cut from the trials of a step, and the trial's decision pooled from its windows'
 * (an EXTENSION: the reference trains and decides on whole trials) ----
 *
 * nsd_crop: x [B,T,C] per model -> y [M][B*R][W][C], row b * R + r of model m = crop r of that model's trial b, in ONE launch for all
 * models.  W = c->window, R = c->crops.  The offset o(b, r) of a crop, in samples:
 *   c->hop == 0   o(b, r) = R(P(b, 2048 + r)) mod (T - W + 1)   with R(i) = value(seed, base_stream + 3, i) and P(b, slot) as for
 *                 nsd_augment, b the trial's index inside ITS model's batch.  Slots 2048 .. 2048 + NSD_CROP_MAX - 1 are ones
 *                 nsd_augment (0, 1, 256..511) and nsd_mixup (1024, and the index 2^63 | 2^62) leave alone: a cropped step does not move
 *                 an augmented or mixed step's draws.  W == T: every offset is 0.
 *   c->hop > 0    o(b, r) = r * hop, no draws (rng may be NULL); (R - 1) * hop + W <= T.  These are the windows k = 0 .. R - 1 that
 *                 nsd_window_step with {W, hop} decides on the trial from a reset state.
 * y[row] is a bitwise copy of x[b, o : o + W, :]; labels_out[row] = labels[b]; targets_out[row, :] is a bitwise copy of targets[b, :]
 * (K = d->K floats); offsets_out[row] = o.  labels / labels_out, targets / targets_out: [M*B] -> [M*B*R] and [M*B][K] -> [M*B*R][K], each
 * pair optional (an input without its output is ignored); offsets_out: NULL or [M*B*R].
 *   x_model_stride, rng[m], step_dev   as for nsd_augment (p_lstm / p_head are ignored): with x_model_stride == 0, M models draw apart
 *                                      from shared trials
 * NSD_E_INVALID before any launch: M outside [1, NSD_MAX_MODELS]; NULL x / y / c; B < 0, T or C < 1; window outside [1, T]; crops
 * outside [1, NSD_CROP_MAX]; hop < 0; a regular grid that leaves the trial; NULL rng with hop == 0; labels_out without labels,
 * targets_out without targets (or with K < 1); a negative x_model_stride or one in (0, B*T*C); y overlapping x; M * B * R above 2^31 - 1.
 * B = 0 launches nothing.  Only d->B, T, C (and K with targets) are read.  nsd_crop_path: 1 where d and c pass these checks.
 *
 * nsd_crop_pool: the trial-level decision from window decisions.  probs [N][R][K] -> probs_out [N][K]:
 *   probs_out[n, k] = (((0 + probs[n, 0, k]) + probs[n, 1, k]) + ... + probs[n, cnt - 1, k]) / float(cnt)   (fp32, one rounding each)
 * cnt = R, or counts[n] with counts given.  A count <= 0 or > R, or a non-finite value anywhere in the trial's cnt counted rows, gives
 * a NaN row.  logits_out (NULL, or [N][K]) = float(log(double(probs_out))): the nsd_multi_eval loss of these "logits" is -log of the
 * pooled probability of the label (a row of probabilities sums to 1 up to rounding) and their argmax the pooled decision; a NaN row
 * counts as non-finite there.  The layout is that of nsd_window_step's probs [B,D,K] and counts [B] (N = B, R = D): a sliding decoder's
 * output pools without a repack.  NSD_E_INVALID before any launch: N < 0, R < 1, K < 1, N * R * K above 2^31 - 1, NULL probs /
 * probs_out.  N = 0 launches nothing.  Additive: NSD_VERSION stays 301, a caller detects the feature by the symbols.
 */
typedef struct nsd_crop_cfg {
    int32_t window, crops, hop;
} nsd_crop_cfg;
#define NSD_CROP_MAX 64
int nsd_crop_path(const nsd_dims *d, const nsd_crop_cfg *c);
int nsd_crop(const nsd_dims *d, int32_t M, const float *x, int64_t x_model_stride, const nsd_crop_cfg *c, const nsd_rng *rng,
             const int64_t *step_dev, const int32_t *labels, const float *targets, float *y, int32_t *labels_out, float *targets_out,
             int32_t *offsets_out, void *stream);
int nsd_crop_pool(int32_t N, int32_t R, int32_t K, const float *probs /* [N][R][K] */, const int32_t *counts /* NULL or [N] */,
                  float *probs_out /* [N][K] */, float *logits_out /* NULL or [N][K] */, void *stream);

/*
 * ---- the step's batch gathered on the device from resident trials (an EXTENSION: the reference has no trainer) ----
 *
 * nsd_gather: the trials x_all [N][T][C] (with labels_all [N] and / or target rows targets_all [N][K]) stay on the device for the whole
 * run, with the run's index schedule table [M][S][B]: row r of model m holds the B trial indices of one step's batch.  One launch forms
 * the batch of all M models, as the first stage of a step (gather -> augment -> prep -> crop -> mixup):
 *   c = *step_dev as the kernel reads it when step_dev is non-NULL (hipGraph replay: the step's device counter), else `step`
 *   r = (c - step_base) mod S, taken non-negative
 *   i = table[m][r][b]:  x[m][b] is a bitwise copy of x_all[i]; labels[m*B + b] = labels_all[i]; targets[m*B + b, :] is a bitwise copy
 *   of targets_all[i, :] (K = d->K floats).  labels_all / labels and targets_all / targets: each pair optional (an input without its
 *   output is ignored).  Duplicate indices within a batch are legal.
 * An index outside [0, N) reads nothing: every word of that row of x is the quiet NaN 0x7FC00000, its target row likewise, its label 0
 * (not -1: the head kernels index by it), and bit 0 of status[m] (NULL, or int32 [M], which the caller zeroes) is set; every other row is
 * what it would have been.  The step's non-finite handling then skips and counts the step.
 * NSD_E_INVALID before any launch: M outside [1, NSD_MAX_MODELS]; N < 1, S < 1, B < 0, T or C < 1; NULL x_all / table / x; labels
 * without labels_all, targets without targets_all (or with K < 1); x overlapping x_all; M * B * T * C or M * S * B above 2^31 - 1.
 * B = 0 launches nothing.  Only d->B, T, C (and K with targets) are read.  nsd_gather_path: 1 where d, M, N, S pass these checks.
 * Additive: NSD_VERSION stays as it is, a caller detects the feature by the symbols.
 */
int nsd_gather_path(const nsd_dims *d, int32_t M, int32_t N, int32_t S);
int nsd_gather(const nsd_dims *d, int32_t M, int32_t N, const float *x_all /* [N][T][C] */, const int32_t *labels_all /* NULL or [N] */,
               const float *targets_all /* NULL or [N][K] */, const int32_t *table /* [M][S][B] trial indices */, int32_t S,
               int64_t step, const int64_t *step_dev, int64_t step_base, float *x /* [M][B][T][C] */, int32_t *labels /* NULL or [M*B] */,
               float *targets /* NULL or [M*B][K] */, int32_t *status /* NULL or [M] */, void *stream);

/*
 * ---- global-norm gradient clipping and learning-rate schedules in the step tail (an EXTENSION: the reference's recipe is missing) ----
 *
 * Step indexing: s is the 1-based Adam step, e = s - 1.
 * Schedule factor f(s), formed in double:
 *   warm-up             W = warmup_steps >= 0;  e < W: f = (e + 1) / W;  otherwise e' = e - W and
 *   NSD_SCHED_CONSTANT  f = 1
 *   NSD_SCHED_COSINE    N' = total_steps - W >= 1, r = min_ratio in [0, 1]:  f = r + (1 - r) * 0.5 * (1 + cos(pi * min(e', N') / N'))
 *                       (past N' it holds at r)
 *   NSD_SCHED_STEP      f = gamma ^ floor(e' / step_size),  step_size >= 1, gamma in (0, 1]
 *   lr_eff = (float)((double)lr * f),  lr_over_bc1 = (float)((double)lr_eff / bc1)
 * With W = 0 the last two are torch's CosineAnnealingLR(T_max = N', eta_min = lr * r) closed form up to T_max, and StepLR.
 * Clipping, torch.nn.utils.clip_grad_norm_ with norm_type = 2:
 *   g~_e = fp32(grads[e] * grad_scale)             (the fp32 product Adam forms anyway)
 *   S    = sum_e (double)g~_e^2                    (the squares are exact in double; the sum is taken in a FIXED order: per reduction
 *                                                   workgroup over its lanes, then a fixed tree over the workgroups' partials)
 *   norm = (float)sqrt(S)
 *   coef = max_norm > 0 ? (float)min(1.0, max_norm / (sqrt(S) + 1e-6)) : 1
 *   Adam takes gi = fmaf(weight_decay, p, g~_e * coef): decay after clipping, as in torch, where decay lives in the optimizer.
 * Bitwise: when nothing is clipped coef is exactly 1.0f and g~ * coef == g~; a constant schedule gives lr_eff == lr.  An unclipped,
 * constant-schedule step with a host `step` leaves grads, p, m, v bitwise what nsd_grad_reduce_adam / nsd_adam_step leave (the Adam
 * arithmetic is adam_kernel's, in its order; the host forms bc1, bc2 and f with libm as there).  With step_dev they are formed on the
 * device, as nsd_adam_step_dev does (its pow / cos differ from libm's in the last place).
 * Non-finite: when S is Inf or NaN the update is skipped entirely -- p, m, v untouched, the model's sticky `skipped` counter + 1, `norm`
 * records the non-finite value, coef reads 0.  Also with max_norm = 0, which means: report the norm and guard, do not clip.
 *
 * opt_state (device, caller-owned, nsd_opt_state_bytes(n_or_P, M) bytes; n_or_P: the flat route's n, or a model's parameter count):
 * M records nsd_opt_record, then private scratch (the workgroups' partial sums, doubles).  nsd_opt_state_init zeroes the buffer once
 * after allocation (the records' sticky counter needs one initialisation); the scratch may hold anything, before and after it: every
 * call writes all of it that it reads.  norm, coef, lr are overwritten by every update; skipped is only ever incremented.
 *   nsd_lr_factor              HOST only: f(step); negative for invalid fields or step < 1
 *   nsd_grad_reduce_clip_adam  the single-rank fp32 tail: nsd_grad_reduce (grads bit for bit) + norm, then the update: two launches.
 *                              step_dev != NULL: s is read from the device counter and `step` is ignored (hipGraph replay: the
 *                              graph replays the schedule with no host argument changing)
 *   nsd_multi_grad_reduce_clip_adam  the same for M models: one norm, one record, one skip decision per model; model m is bitwise a
 *                              single-model call (domain and refusals of nsd_multi_grad_reduce_adam)
 *   nsd_grad_norm              flat route, launch 1: the partial sums of g[0..n) * grad_scale -> opt_state's scratch
 *   nsd_adam_step_clip         flat route, launch 2: the update from what nsd_grad_norm(n, g, opt->grad_scale) left (after the all-reduce
 *                              at world > 1, on the bf16 sequence path, in graph segment B).  skip: NULL, or the device flag of
 *                              nsd_adam_step_guarded -- non-zero: nothing is written, the record included
 * NSD_E_INVALID before any launch: NULL opt / pointers; max_norm negative or NaN; unknown sched; warmup_steps < 0; cosine with
 * total_steps <= warmup_steps; step_size < 1; gamma outside (0, 1]; min_ratio outside [0, 1]; step < 1 without step_dev; n < 0.
 * NSD_E_WORKSPACE: opt_state_bytes < nsd_opt_state_bytes, or a short workspace.  Additive: NSD_VERSION stays 301, detected by the symbols.
 */
#define NSD_SCHED_CONSTANT 0
#define NSD_SCHED_COSINE   1
#define NSD_SCHED_STEP     2
typedef struct nsd_opt {
    float lr, beta1, beta2, eps, weight_decay, grad_scale, max_norm;
    int32_t sched, warmup_steps, total_steps, step_size;
    float min_ratio, gamma;
} nsd_opt;
typedef struct nsd_opt_record { float norm, coef, lr; uint32_t skipped; } nsd_opt_record;   /* 16 B per model, first bytes of opt_state */
double  nsd_lr_factor(const nsd_opt *opt, int64_t step);
int64_t nsd_opt_state_bytes(int64_t n_or_P, int32_t M);
int nsd_opt_state_init(void *opt_state, int64_t opt_state_bytes, void *stream);
int nsd_grad_reduce_clip_adam(const nsd_dims *d, const float *workspace, int64_t workspace_bytes, float *grads, float *p, float *m, float *v,
                              const nsd_opt *opt, int32_t step, const int64_t *step_dev, void *opt_state, int64_t opt_state_bytes, void *stream);
int nsd_grad_norm(int64_t n, const float *g, float grad_scale, void *opt_state, int64_t opt_state_bytes, void *stream);
int nsd_adam_step_clip(int64_t n, float *p, const float *g, float *m, float *v, const nsd_opt *opt, int32_t step, const int64_t *step_dev,
                       const float *skip, void *opt_state, int64_t opt_state_bytes, void *stream);

/*
 * ---- model-batched H = 48 path: M models of one shape trained / evaluated in the launches one model uses ----
 *
 * Folds, seeds and ensembles of EEG_LSTM (lstm_eeg_model.py:13-39): each model has its own parameters, windows, labels and random
 * streams; a launch covers all of them.  Layout ("one batch of M*B trials, partitioned by model", d->B = trials PER MODEL):
 *   params   [M][P]       P = nsd_param_count; each block in the flat order above
 *   x        model m reads x + m * x_model_stride floats ([B,T,C] each); x_model_stride = 0: every model reads the same windows
 *   labels   [M*B]  logits / probs [M*B][K]  grads [M][P]
 *   workspace  the regions of a batch of M*B trials (model m's trial b is trial m*B + b); nsd_multi_workspace_bytes
 *   rng      NULL (no dropout, eval RReLU slope) or M entries: model m's streams are exactly those of a single-model call with rng[m]
 *            at batch B (nsd_lstm_head_train_rng).  All entries share p_lstm / p_head (per-model ones: NSD_FLAG_MODEL_P, below).
 * Each model's step is that of nsd_lstm_head_train_rng (scale 1/B: mean CE per model, lstm_eeg_model.py:32-39) + nsd_lstm_bwd_rng +
 * nsd_grad_reduce(_adam) on its own; the kernels dispatch on the M*B trials of the launch as the single-model entry points do on B.
 * Where nsd_multi_path(d, M) == 0 every entry point returns NSD_E_INVALID before any launch (nsd_last_error says why), as it does for
 * M outside [1, NSD_MAX_MODELS], NULL pointers, mismatched rng probabilities, NSD_FLAG_RESIDUAL or a negative / overlapping
 * x_model_stride; a workspace smaller than nsd_multi_workspace_bytes gives NSD_E_WORKSPACE.  The residual extension is not offered
 * here; dx is, for frozen models (nsd_multi_train_bwd_dx, below).
 *   nsd_multi_path            1 for H = 48, L = 2, C <= 8, T <= 1024, F <= 64, K <= 8 and 1 <= M <= NSD_MAX_MODELS, else 0
 *   nsd_multi_train_fwd       forward + head + mean CE per model + head backward; logits [M*B][K]
 *   nsd_multi_train_bwd       BPTT into the per-workgroup slabs (same rng as the forward call)
 *   nsd_multi_grad_reduce     grads[m] = model m's slabs summed (overwritten), all models in one launch
 *   nsd_multi_grad_reduce_adam  the same + torch.optim.Adam on p / m / v [M][P] in that launch (= reduce, then nsd_adam_step(n = M*P))
 *   nsd_multi_loss_sum        out[m] = sum of model m's per-trial CE losses (device)
 *   nsd_multi_infer           eval-mode forward + class softmax (lstm_eeg_model.py:32-39, :97) of every model on its windows;
 *                             scratch: nsd_multi_infer_scratch_bytes(d, M) bytes (0: may be NULL)
 */
int     nsd_multi_path(const nsd_dims *d, int32_t M);
int64_t nsd_multi_workspace_bytes(const nsd_dims *d, int32_t M, nsd_ws_layout *layout_out);
int nsd_multi_train_fwd(const nsd_dims *d, int32_t M, const float *params, const float *x, int64_t x_model_stride, const nsd_rng *rng,
                        const int32_t *labels, uint32_t flags, float *workspace, int64_t workspace_bytes, float *logits, void *stream);
/* nsd_multi_train_fwd with targets [M*B][K] in place of the labels (soft targets, above) */
int nsd_multi_train_fwd_soft(const nsd_dims *d, int32_t M, const float *params, const float *x, int64_t x_model_stride, const nsd_rng *rng,
                             const float *targets, uint32_t flags, float *workspace, int64_t workspace_bytes, float *logits, void *stream);
int nsd_multi_train_bwd(const nsd_dims *d, int32_t M, const float *params, const float *x, int64_t x_model_stride, const nsd_rng *rng,
                        uint32_t flags, float *workspace, int64_t workspace_bytes, void *stream);
int nsd_multi_grad_reduce(const nsd_dims *d, int32_t M, const float *workspace, int64_t workspace_bytes, float *grads, void *stream);
int nsd_multi_grad_reduce_adam(const nsd_dims *d, int32_t M, const float *workspace, int64_t workspace_bytes, float *grads, float *p,
                               float *m, float *v, float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                               int32_t step, void *stream);
/* nsd_grad_reduce_clip_adam for M models (clipping and schedules, above): grads / p / m / v [M][P], opt_state of nsd_opt_state_bytes(P, M) */
int nsd_multi_grad_reduce_clip_adam(const nsd_dims *d, int32_t M, const float *workspace, int64_t workspace_bytes, float *grads, float *p,
                                    float *m, float *v, const nsd_opt *opt, int32_t step, const int64_t *step_dev, void *opt_state,
                                    int64_t opt_state_bytes, void *stream);
int nsd_multi_loss_sum(const nsd_dims *d, int32_t M, const float *workspace, int64_t workspace_bytes, float *out, void *stream);
int64_t nsd_multi_infer_scratch_bytes(const nsd_dims *d, int32_t M);
int nsd_multi_infer(const nsd_dims *d, int32_t M, const float *params, const float *x, int64_t x_model_stride, uint32_t flags,
                    float *logits, float *probs, void *scratch, void *stream);

/*
 * ---- input gradients of M frozen models: dL/dx through an ensemble ----
 *
 * Additive (NSD_VERSION stays 301; callers detect the feature by the symbol nsd_multi_dx_path).  The backward that follows
 * nsd_multi_train_fwd[_soft] called with rng == NULL (eval-mode noise: no dropout, the eval RReLU slope), with dL/dx formed behind it.
 * There is no rng parameter: the single-model nsd_lstm_bwd_rng forms no dx either, and the use is a frozen model (saliency, fitting an
 * input-side matrix through the models: nsd_spatial_bwd).
 *   nsd_multi_dx_path         1 where nsd_multi_path(d, M) and nsd_dx_path(d) both hold, else 0
 *   nsd_multi_train_bwd_dx    nsd_multi_train_bwd(rng = NULL) + dx.  The parameter-gradient slabs are written exactly as
 *                             nsd_multi_train_bwd writes them (the reduce entry points that follow stay valid).  Layer 0's saved gates are
 *                             consumed -- da0 lands in their place: ONE backward per forward, as for nsd_lstm_bwd's dx.  The one-trial
 *                             backward kernel runs whatever the batch; open attention records (the fused forward leaves them from 513
 *                             trials in the launch on) are closed first, over all M*B trials.
 *       reduce = NSD_DX_PER_MODEL   dx [M*B][T][C]: model m's rows hold the gradient of ITS mean loss with respect to ITS windows.  Every
 *                             element is one fmaf chain over the 4H gate rows ascending, as nsd_lstm_bwd's dx.  Below 513 trials in
 *                             the launch (M*B: the one- and two-trial forward kernels, which save the same bits) model m's rows are bit
 *                             for bit nsd_lstm_bwd's dx for that model alone on the same windows.  From 513 trials the four-trial forward
 *                             forms the gate products on the matrix pipe; a single model of B < 513 trials does not, the saved
 *                             activations differ in their last bits and so does dx (both within the dx bound against the oracle).
 *       reduce = NSD_DX_MEAN  dx [B][T][C], dx[r,c] = (((d_0 + d_1) + ...) + d_{M-1}) / (float)M with d_m model m's per-model value: a
 *                             serial fp32 sum over m ascending, every addition rounded on its own, then one correctly rounded division
 *                             (the convention of nsd_multi_stream_step's mean).  Requires x_model_stride == 0 (every model saw the same
 *                             windows).  At M = 1 it is the per-model value, bitwise.
 *                             M = 1 runs nsd_lstm_bwd with dx.
 *   nsd_multi_loss_mean       out[0] (device) = the serial fp32 sum over m ascending of the values nsd_multi_loss_sum writes, divided by
 *                             (float)M: the ensemble objective's numerator, e.g. nsd_spatial_fit_step's loss_in without a host read
 * NSD_E_INVALID before any launch (nsd_last_error names the cause): NULL d / params / x / workspace / dx; a shape outside
 * nsd_multi_dx_path; reduce outside {0, 1}; NSD_DX_MEAN with a non-zero x_model_stride; the refusals of the entry points above (residual
 * flag, x_model_stride in (0, B*T*C)); B * T * H * 4 bytes per model reaching 2 GB (the one-trial kernel's 32-bit offsets).
 * NSD_E_WORKSPACE as for nsd_multi_train_bwd.  B = 0 launches nothing.  No host synchronisation, no allocation: capturable on one stream.
 */
#define NSD_DX_PER_MODEL 0
#define NSD_DX_MEAN      1
int nsd_multi_dx_path(const nsd_dims *d, int32_t M);
int nsd_multi_train_bwd_dx(const nsd_dims *d, int32_t M, const float *params, const float *x, int64_t x_model_stride, uint32_t flags,
                           float *workspace, int64_t workspace_bytes, float *dx, int32_t reduce, void *stream);
int nsd_multi_loss_mean(const nsd_dims *d, int32_t M, const float *workspace, int64_t workspace_bytes, float *out, void *stream);

/*
 * ---- per-model step settings: a hyper-parameter grid (configurations x folds) in the launches one model uses ----
 *
 * Additive (NSD_VERSION stays 301; callers detect the feature by the symbol nsd_multi_hyper_path).  The model axis of the entry points
 * above holds folds and seeds; with these it also holds configurations: every scalar of a train step is per model.
 *   nsd_multi_hyper_path      1 where the entry points below are offered (the domain of nsd_multi_path), else 0
 *   NSD_FLAG_MODEL_P          accepted by nsd_multi_train_fwd, nsd_multi_train_fwd_soft and nsd_multi_train_bwd only: rng[m].p_lstm /
 *                             rng[m].p_head may differ from model to model (each in [0, 1), 0 included).  The same flag and the same
 *                             rng array go to the forward and the backward call of a step.  Without the flag mixed probabilities are
 *                             refused as before; with the flag and equal probabilities the call is bit for bit the unflagged one;
 *                             M = 1 strips the bit and runs the single-model entry point.  Model m's workgroups run the instructions
 *                             of a launch of the same M and B in which every model has rng[m]'s probabilities, on the same data.
 *   nsd_augment_each          nsd_augment with aug pointing to M entries; each operation is skipped per model where that model's
 *                             parameter is 0; NSD_AUG_ZSCORE stays per launch
 *   nsd_mixup_each            nsd_mixup with mix pointing to M entries and class_weight NULL or [M][K]; with any mix[m].mix > 0, x and y
 *                             are required, and a model with mix == 0 gets a bitwise copy of its windows and un-multiplied target rows
 *   nsd_multi_grad_reduce_clip_adam_each
 *                             nsd_multi_grad_reduce_clip_adam with opt pointing to M entries: every field per model, grad_scale
 *                             included; opt_state, records, step / step_dev and the two launches are unchanged
 * Each entry of aug / mix / opt is validated as the twin validates its one, before any launch; the refusal names the entry
 * ("augment_each: aug[2]: max_shift ...").  Model m's result is bit for bit that of the twin called with entry m for all models.
 */
#define NSD_FLAG_MODEL_P    16u
int nsd_multi_hyper_path(const nsd_dims *d, int32_t M);
int nsd_augment_each(const nsd_dims *d, int32_t M, const float *x, int64_t x_model_stride, const nsd_aug *aug, const nsd_rng *rng,
                     const int64_t *step_dev, uint32_t flags, float *y, void *stream);
int nsd_mixup_each(const nsd_dims *d, int32_t M, const float *x, int64_t x_model_stride, const int32_t *labels, const float *class_weight,
                   const nsd_mix *mix, const nsd_rng *rng, const int64_t *step_dev, float *y, float *targets, void *stream);
int nsd_multi_grad_reduce_clip_adam_each(const nsd_dims *d, int32_t M, const float *workspace, int64_t workspace_bytes, float *grads,
                                         float *p, float *m, float *v, const nsd_opt *opt, int32_t step, const int64_t *step_dev,
                                         void *opt_state, int64_t opt_state_bytes, void *stream);

/*
 * ---- weight averaging in the step tail: EMA / SWA of the parameters, formed by the update launch (an EXTENSION) ----
 *
 * Additive (NSD_VERSION stays 301; callers detect the feature by the symbol nsd_avg_state_bytes).  Each `_avg` entry point is the twin of
 * the one it is named after, with `avg, avg_state, avg_state_bytes` appended; its launch count is the twin's (two for the fused tails,
 * one for the flat update): the average is formed by the update kernel in the iteration that stores p[i].  p, m, v, grads and the
 * nsd_opt_record are bit for bit what the twin leaves.  No existing entry point changes its launches or its bits.
 * avg_state (device, caller-owned, nsd_avg_state_bytes(n_or_P, M) bytes): M records nsd_avg_record, then the averaged rows [M][n_or_P]
 * (fp32) from byte 16 * M.  nsd_avg_state_init zeroes the M records and nothing else; a row may hold anything until its model's first
 * averaged step, which overwrites all of it.
 * The rule, per model, at Adam step s (1-based; the host `step`, or step_dev's value where that is given, as the schedule reads it):
 *   a skipped update (non-finite norm, or the caller's skip flag)           row and n_avg untouched
 *   s < start_step, or (s - start_step) % every != 0                        row and n_avg untouched
 *   otherwise, n = n_avg as it stood before the launch and p' the new parameter:
 *     n == 0          a = p'  (a copy of the word)
 *     NSD_AVG_EMA     a' = a + w * (p' - a),  w = 1.0f - decay in fp32
 *     NSD_AVG_SWA     a' = a + (p' - a) / (float)(n + 1)                     (torch.optim.swa_utils.AveragedModel's default)
 *     then n_avg = n + 1
 * Every fp32 operation is rounded once (no contraction); the division is IEEE.
 * The counter.  The launch has no order between workgroups, and every workgroup of a model needs n as it stood BEFORE the launch.  So
 * every workgroup reads n_avg first and then adds 1 to `arrive`; the workgroup that sees gridDim.x - 1 is the last one, and it alone
 * writes n_avg = n + 1 and arrive = 0.  Nobody waits for anybody.  The four accesses are relaxed device-scope atomics; there is no
 * device-scope fence per workgroup (nothing is published from one workgroup to another inside the launch; a workgroup holds the value
 * of its read before it arrives).  `arrive` reads 0 between launches.  The `_avg` twins may launch fewer workgroups per model than
 * their twins (every workgroup arrives once): the results do not depend on the grid.
 *   nsd_multi_grad_reduce_clip_adam_avg       one nsd_avg for all M models
 *   nsd_multi_grad_reduce_clip_adam_avg_each  opt AND avg point to M entries; avg[m].mode == 0: model m does not average (its row and
 *                                             record are never touched)
 *   nsd_adam_step_clip_avg                    the flat route (world > 1 after the all-reduce; the bf16 sequence path with its skip flag)
 * NSD_E_INVALID before any launch (the `_each` twin names the entry, "...: avg[2]: decay ..."): the twin's refusals; NULL avg or avg_state;
 * mode outside {NSD_AVG_EMA, NSD_AVG_SWA} (0 also allowed inside `_each`); for EMA decay outside [0, 1) or NaN (ignored for SWA);
 * start_step < 1; every < 1.  NSD_E_WORKSPACE: avg_state_bytes < nsd_avg_state_bytes.
 */
#define NSD_AVG_EMA 1
#define NSD_AVG_SWA 2
typedef struct nsd_avg { int32_t mode; float decay; int32_t start_step; int32_t every; } nsd_avg;
typedef struct nsd_avg_record { uint32_t n_avg; uint32_t arrive; uint32_t pad[2]; } nsd_avg_record;   /* 16 B per model, first bytes of avg_state */
int64_t nsd_avg_state_bytes(int64_t n_or_P, int32_t M);
int nsd_avg_state_init(void *avg_state, int64_t avg_state_bytes, int32_t M, void *stream);
int nsd_grad_reduce_clip_adam_avg(const nsd_dims *d, const float *workspace, int64_t workspace_bytes, float *grads, float *p, float *m, float *v,
                                  const nsd_opt *opt, int32_t step, const int64_t *step_dev, void *opt_state, int64_t opt_state_bytes, void *stream,
                                  const nsd_avg *avg, void *avg_state, int64_t avg_state_bytes);
int nsd_multi_grad_reduce_clip_adam_avg(const nsd_dims *d, int32_t M, const float *workspace, int64_t workspace_bytes, float *grads, float *p,
                                        float *m, float *v, const nsd_opt *opt, int32_t step, const int64_t *step_dev, void *opt_state,
                                        int64_t opt_state_bytes, void *stream, const nsd_avg *avg, void *avg_state, int64_t avg_state_bytes);
int nsd_multi_grad_reduce_clip_adam_avg_each(const nsd_dims *d, int32_t M, const float *workspace, int64_t workspace_bytes, float *grads,
                                             float *p, float *m, float *v, const nsd_opt *opt, int32_t step, const int64_t *step_dev,
                                             void *opt_state, int64_t opt_state_bytes, void *stream, const nsd_avg *avg, void *avg_state,
                                             int64_t avg_state_bytes);
int nsd_adam_step_clip_avg(int64_t n, float *p, const float *g, float *m, float *v, const nsd_opt *opt, int32_t step, const int64_t *step_dev,
                           const float *skip, void *opt_state, int64_t opt_state_bytes, void *stream, const nsd_avg *avg, void *avg_state,
                           int64_t avg_state_bytes);

/*
 * ---- sharpness-aware minimisation (SAM, Foret et al. 2021): the ascent between two forward/backward passes (an EXTENSION) ----
 *
 * Additive (NSD_VERSION stays 301; callers detect the feature by the symbol nsd_sam_state_bytes).  SAM updates the parameters with the
 * gradient taken at the parameters moved a distance rho uphill along the normalised gradient.  These entry points form that perturbed
 * copy on the device; no existing entry point changes its launches or its bits, and THE STEP'S TAIL IS UNCHANGED.  The sequence a
 * caller issues for one step:
 *   1. pass 1: the training forward/backward with params = p;
 *   2. the ascent (below): grads of pass 1, and p_adv in sam_state;
 *   3. pass 2: the same forward/backward calls with params = the model's row in sam_state and the same x / targets / rng (or mask
 *      tensors) / flags and the same workspace -- the random streams are counter-based, so pass 2 sees pass 1's draws;
 *   4. any existing tail on p (nsd_grad_reduce, _adam, _clip_adam, their `_avg` and `multi` forms, or the flat route).
 * The ascent, per model, with g~_e = fp32(grads[e] * grad_scale) and S = sum_e (double)g~_e^2 exactly as the clipped tail defines
 * and orders them ("global-norm gradient clipping" above):
 *   es       = (float)((double)rho / (sqrt(S) + 1e-12))
 *   p_adv[e] = p[e] + es * g~_e                 every fp32 operation rounded once (no contraction), as the averaged row
 *   rho == 0, or S not finite:  p_adv[e] = p[e], a copy of the word (signed zeros and NaN payloads survive); the branch is uniform
 *                               over a model's workgroups.  S not finite: the record's sticky `nonfinite` counter + 1.
 *   record: norm = (float)sqrt(S), scale = es (0 where the row is a copy)
 * Launches: two, with no signalling between workgroups, no atomics and no fences.  Launch 1 is the clipped tail's own first launch
 * (from the slabs: grads is nsd_grad_reduce's bit for bit; flat: nsd_grad_norm's) and leaves the partial sums in opt_state's scratch;
 * launch 2 sums them in the tail's fixed order in every workgroup and writes the rows; workgroup 0 of a model writes its record.
 * p and grads (flat: g) are inputs of launch 2 only; m and v are not touched.  opt_state's records are not touched either.
 * sam_state (device, caller-owned, nsd_sam_state_bytes(n_or_P, M) bytes): M records nsd_sam_record, then the rows p_adv [M][n_or_P]
 * (fp32) from byte 16 * M.  nsd_sam_state_init zeroes the buffer once after allocation (the sticky counter needs it); the rows are
 * scratch: every ascent writes all of a model's row.
 *   nsd_sam_ascend        single-rank fp32 route from the slabs of pass 1
 *   nsd_multi_sam_ascend  M models in the same two launches.  each != 0: sam and grad_scale point to M entries; each == 0: to one
 *                         entry for all.  Model m is bit for bit the single-model call.  Domain and refusals of
 *                         nsd_multi_grad_reduce_clip_adam (M = 1 runs nsd_sam_ascend)
 *   nsd_sam_ascend_flat   from a flat gradient g[0..n): world > 1 after nsd_grad_reduce (each rank along its own shard's gradient),
 *                         the bf16 sequence path after nsd_seq_train_bwd.  n == 0 launches nothing.
 * NSD_E_INVALID before any launch: NULL pointers; rho negative or NaN; n < 0; the rows of sam_state overlapping p or grads.
 * NSD_E_WORKSPACE: opt_state_bytes < nsd_opt_state_bytes, sam_state_bytes < nsd_sam_state_bytes, or a short workspace.
 */
typedef struct nsd_sam { float rho; } nsd_sam;
typedef struct nsd_sam_record { float norm, scale; uint32_t nonfinite, pad; } nsd_sam_record;   /* 16 B per model, first bytes of sam_state */
int64_t nsd_sam_state_bytes(int64_t n_or_P, int32_t M);
int nsd_sam_state_init(void *sam_state, int64_t sam_state_bytes, void *stream);
int nsd_sam_ascend(const nsd_dims *d, const float *workspace, int64_t workspace_bytes, float *grads, const float *p, const nsd_sam *sam,
                   float grad_scale, void *opt_state, int64_t opt_state_bytes, void *sam_state, int64_t sam_state_bytes, void *stream);
int nsd_multi_sam_ascend(const nsd_dims *d, int32_t M, const float *workspace, int64_t workspace_bytes, float *grads, const float *p,
                         const nsd_sam *sam, int32_t each, const float *grad_scale /* HOST: M entries (each != 0) or one */,
                         void *opt_state, int64_t opt_state_bytes, void *sam_state, int64_t sam_state_bytes, void *stream);
int nsd_sam_ascend_flat(int64_t n, const float *p, const float *g, const nsd_sam *sam, float grad_scale, void *opt_state,
                        int64_t opt_state_bytes, void *sam_state, int64_t sam_state_bytes, void *stream);

/*
 * ---- early stopping for model batches: held-out metrics, the best-evaluation decision and the snapshot in ONE launch (an EXTENSION) ----
 *
 * Additive (NSD_VERSION stays 301; callers detect the feature by the symbol nsd_multi_eval_path).  nsd_multi_eval reads the logits of M
 * models -- what nsd_multi_infer wrote for each model's held-out windows, or any other path's -- and their parameter rows; it is not
 * H = 48 specific.  One launch, one 256-thread workgroup per model.
 * Rows that count.  Only the first counts[m] rows of model m count (counts: a HOST array of M entries, validated before the launch and
 * passed by value, so a captured call replays; NULL: B each).  The rest is padding (folds differ in size by one, nsd_multi_infer wants
 * one B) and may hold anything, NaN logits and labels outside [0, K) included.
 * Per counted row, from the fp32 logits in double:  loss = log(sum_k exp(l_k - max)) + max - l_y, k ascending; the prediction is the
 * first maximal index; confusion[y][pred] += 1, correct += (pred == y), n += 1.  A counted row with a non-finite logit, or with a label
 * outside [0, K), counts in `nonfinite` ONLY (not in n, correct or confusion) and makes the model's loss_sum NaN, explicitly and not by
 * what the arithmetic would yield.
 * Summation order.  loss_sum is formed in an order fixed by the workgroup size alone: lane i of 256 sums rows i, i + 256, ... in
 * ascending order, then a halving tree combines the lanes (lane i += lane i + s for s = 128, 64, ..., 1).  Model m's record therefore
 * does not depend on M or on the other models' data.
 * Selection, with sel != NULL, per model, on the record in sel_state:
 *   stopped != 0          the select record and the snapshot keep their bytes (the eval record is still written)
 *   otherwise             evals += 1; mean = loss_sum / n; acc = (double)correct / n.  A non-finite mean sets status bit 0 and counts as
 *                         "not improved".  Improved, NSD_SELECT_LOSS: no best yet (best_eval == 0), or mean < best_loss - min_delta.
 *                         Improved, NSD_SELECT_ACC: no best yet, or acc > best_acc + min_delta, or acc == best_acc and mean < best_loss
 *                         (best_acc = (double)best_correct / best_n; every comparison in double, min_delta widened exactly).
 *   on improvement        best_loss = mean, best_correct = correct, best_n = n, best_eval = evals, bad = 0, and best_params[m] becomes
 *                         a byte copy of params[m] (16-byte accesses in the body, single words at the misaligned head and tail of a row;
 *                         the decision reaches the workgroup through LDS first)
 *   without               bad += 1; with patience > 0 and bad >= patience: stopped = 1.  No word of the snapshot is written.
 * sel_state (device, caller-owned, nsd_select_state_bytes(M, P) bytes): M nsd_select_record, padded to a multiple of 16 bytes, then
 * best_params [M][P].  nsd_select_state_init zeroes the records (and the padding); the snapshot rows may hold anything until their
 * model's first improvement.  `evals` lives in the record, so a captured call replays: three replays are three evaluations.
 *   nsd_multi_eval_path   1 where 1 <= M <= NSD_MAX_MODELS, 1 <= K <= 8, B >= 1, M * B * K <= 2^31 - 1 and P >= 0 (P = 0: metrics only)
 * Failure behaviour.  Every refusal happens before any launch.  NSD_E_INVALID: M outside [1, NSD_MAX_MODELS]; K outside [1, 8]; B < 1;
 * M * B * K > 2^31 - 1; a counts[m] outside [1, B]; NULL logits, labels or out; sel with a metric other than NSD_SELECT_LOSS / _ACC, with
 * patience < 0, with a negative or NaN min_delta; sel without params or sel_state, or with P < 1.  NSD_E_WORKSPACE: sel_state_bytes <
 * nsd_select_state_bytes(M, P).  Writes: out[M] and, with sel, the records and the improved models' snapshot rows; nothing else.  No
 * host synchronisation, no allocation.
 */
#define NSD_SELECT_LOSS 0
#define NSD_SELECT_ACC  1
#define NSD_EVAL_MAX_K  8
typedef struct nsd_select {
    int32_t metric;                 /* NSD_SELECT_LOSS | NSD_SELECT_ACC */
    int32_t patience;               /* >= 0; 0: track the best, never stop */
    float   min_delta;              /* >= 0 */
} nsd_select;
typedef struct nsd_eval_record {    /* 280 B per model */
    double  loss_sum;               /* over the n rows, NaN where nonfinite > 0 */
    int32_t n, correct, nonfinite, pad;
    int32_t confusion[NSD_EVAL_MAX_K][NSD_EVAL_MAX_K];   /* [label][prediction] */
} nsd_eval_record;
typedef struct nsd_select_record {  /* 40 B per model, first bytes of sel_state */
    double   best_loss;             /* mean loss of the best evaluation */
    int32_t  best_correct, best_n, best_eval /* 1-based, 0: none yet */, evals, bad;
    uint32_t stopped, status /* bit 0: a non-finite evaluation was seen */, pad;
} nsd_select_record;
int     nsd_multi_eval_path(int32_t M, int32_t B, int32_t K, int64_t P);
int64_t nsd_select_state_bytes(int32_t M, int64_t P);
int     nsd_select_state_init(void *sel_state, int64_t sel_state_bytes, int32_t M, int64_t P, void *stream);
int     nsd_multi_eval(int32_t M, int32_t B, int32_t K, const float *logits /* [M*B][K] */, const int32_t *labels /* [M*B] */,
                       const int32_t *counts /* HOST, [M] or NULL = B each */, nsd_eval_record *out /* device, [M] */,
                       const nsd_select *sel /* NULL: metrics only */, const float *params /* [M][P] */, int64_t P,
                       void *sel_state, int64_t sel_state_bytes, void *stream);

/*
 * ---- resumable H = 48 inference: decode live streams chunk by chunk (an EXTENSION: the reference decodes whole windows only) ----
 *
 * EEG_LSTM (lstm_eeg_model.py:13-39) is causal: two forward LSTM layers and a softmax pooling over time that can be formed online.  The
 * state of a stream after t samples is h and c of both layers plus the pooling's running max, denominator and weighted sum: one SLOT of
 * nsd_stream_layout.stride floats in a caller-owned device buffer of S slots.  nsd_stream_step advances B streams by a chunk of d->T
 * samples each and, when asked, reads the decision of the prefix seen so far: row b of logits / probs is what nsd_infer returns for the
 * first t samples of that stream (t = the slot's step count after the call; there is no upper limit on t).  The pooling is updated once
 * per step in a fixed order that does not depend on where a chunk begins, so the state after t samples, and every output read from it,
 * is bit for bit a function of the samples alone -- not of how they were cut into chunks, of the slot, or of the other streams of a call.
 *   nsd_stream_path          1 for H = 48, L = 2, C <= 8, F <= 64, K <= 64, else 0 (and for invalid dims).  Only the model dims are read.
 *   nsd_stream_state_bytes   bytes of a state of S >= 1 slots (S * stride * 4); <0 outside nsd_stream_path
 *   nsd_stream_state_layout  float offsets inside a slot: h[l][H], c[l][H], pool_max, pool_den, pool_acc[H]; `steps`: the float offset of
 *                            the slot's int64 step count (8-byte aligned); `stride`: floats per slot.  The layout is public: a slot can be
 *                            checkpointed and restored by copying its stride floats.  h[1] is the top LSTM layer's own output (without
 *                            the residual extension's sum); pool_acc / pool_den is the pooled vector of the prefix.
 *   nsd_stream_reset         slots == NULL: all S slots; else the n slots of the DEVICE array slots[n] (indices outside [0, S) are
 *                            skipped).  A reset slot has zero h and c, an empty pooling state (max -inf, denominator 0) and step count
 *                            0.  A state must be reset once before its first nsd_stream_step; it may hold anything before that.
 *   nsd_stream_step          d->B streams, chunk length d->T >= 1, x [B,T,C]; slots: DEVICE int32[B] of distinct indices in [0, S), or
 *                            NULL for 0 .. B-1; flags: NSD_FLAG_RESIDUAL (the same on every call of a stream); logits [B,K] or NULL
 *                            (advance only: no readout); probs [B,K] or NULL.
 * Failure behaviour.  Every refusal happens before any launch: NSD_E_INVALID for NULL d / params / x / state, probs without logits,
 * S < 1, n < 0 or n > S (reset), B > S, a shape outside nsd_stream_path, flags other than NSD_FLAG_RESIDUAL; NSD_E_WORKSPACE when
 * state_bytes < nsd_stream_state_bytes(d, S).  B = 0 (n = 0) launches nothing.  A slot index outside [0, S) can only be seen on the
 * device: that stream is skipped, its rows of logits / probs are NaN, no memory outside the state is touched.  Duplicate slots in one call
 * are undefined (two workgroups would race on one slot).  A sample that is not finite (NaN or +-Inf) makes that stream's state, and every
 * output read from it, NaN until the slot is reset; the other streams are unaffected.  No host synchronisation, no allocation: the call
 * can be captured in a single-stream graph and replayed -- the step count lives in the state, nothing in the arguments changes per call.
 * Additive: NSD_VERSION stays 301, a caller detects the feature by the symbols.
 */
typedef struct nsd_stream_layout {
    int64_t h[NSD_MAX_LAYERS], c[NSD_MAX_LAYERS];   /* [H] each, entries 0 .. L-1 */
    int64_t pool_max, pool_den, pool_acc;           /* 1, 1, [H] */
    int64_t steps;                                  /* int64 step count: float offset, even */
    int64_t stride;                                 /* floats per slot */
} nsd_stream_layout;
int     nsd_stream_path(const nsd_dims *d);
int64_t nsd_stream_state_bytes(const nsd_dims *d, int32_t S);
int     nsd_stream_state_layout(const nsd_dims *d, nsd_stream_layout *out);
int nsd_stream_reset(const nsd_dims *d, void *state, int64_t state_bytes, int32_t S, const int32_t *slots, int32_t n, void *stream);
int nsd_stream_step(const nsd_dims *d, const float *params, const float *x, const int32_t *slots, uint32_t flags, void *state,
                    int64_t state_bytes, int32_t S, float *logits, float *probs, void *stream);

/*
 * ---- resumable inference of an ensemble: M models per stream in one launch (an EXTENSION, of the two above: nsd_multi_*, nsd_stream_*) ----
 *
 * nsd_multi_stream_step advances the B streams of a call in each of M models of one shape -- params [M,P], P = nsd_param_count(d) -- by
 * one launch of the step nsd_stream_step runs (the same source, csrc/nsd_stream48.hip, compiled with a model view), and can return the
 * ensemble's mean probabilities.
 * State: [M][S][stride] floats.  Model m's part starts at float m * S * stride and is an ordinary single-model state of S slots in the
 * public nsd_stream_layout: it can be handed to nsd_stream_step as it is (with params + m*P).  The whole buffer is a flat state of M*S
 * slots to nsd_stream_reset -- slot m*S + s is stream s of model m, slots == NULL resets everything -- so there is no reset entry of its
 * own, and the state must be reset once before its first step.
 *   nsd_multi_stream_path         1 where nsd_stream_path(d) and 1 <= M <= NSD_MAX_MODELS, else 0
 *   nsd_multi_stream_state_bytes  M * nsd_stream_state_bytes(d, S); <0 outside the path or for S < 1
 *   nsd_multi_stream_step         d->B streams, chunk length d->T >= 1.  x: model m reads the chunk [B,T,C] at x + m * x_model_stride
 *                                 floats; 0: one chunk for all models, else >= B*T*C.  slots: DEVICE int32[B] of distinct indices in
 *                                 [0, S) or NULL for 0 .. B-1, shared by the models: stream b lives in slot slots[b] of every model's
 *                                 part.  logits [M,B,K] or NULL (advance only), probs [M,B,K] or NULL, mean_probs [B,K] or NULL.
 * Contract.  Model m's slots after the call, and its rows of logits / probs, are bit for bit what
 *   nsd_stream_step(d, params + m*P, x + m*x_model_stride, slots, flags, state + m*S*stride, S*stride*4, S, logits + m*B*K, probs + m*B*K)
 * leaves and writes, for any M, B, cut of the stream and placement in the grid.
 * mean_probs[b,k] = (((p_0 + p_1) + p_2) + ... + p_{M-1}) / (float)M with p_m = probs[m,b,k]: a serial fp32 sum in m, every addition
 * rounded on its own, then one correctly rounded division.  It is formed from the probs buffer by a second small launch that the
 * same call enqueues behind the step.
 * Failure behaviour.  As nsd_stream_step, every refusal before any launch: NSD_E_INVALID for all that call refuses, for M outside
 * [1, NSD_MAX_MODELS], mean_probs without probs, x_model_stride negative or positive and below B*T*C, M*B*K above 2^31 - 1;
 * NSD_E_WORKSPACE when state_bytes < nsd_multi_stream_state_bytes(d, M, S).  B = 0 launches nothing.  A slot index outside [0, S) is
 * skipped in every model: its rows of logits, probs and mean_probs are NaN, no state is touched.  A sample that is not finite poisons
 * that stream in every model that reads it until those slots (m*S + s) are reset; its mean row is NaN, other streams are unaffected.
 * No host synchronisation, no allocation: the call can be captured in a single-stream graph, with nsd_prep_step in front of it.
 * Additive: NSD_VERSION stays 301, a caller detects the feature by the symbols.
 */
int     nsd_multi_stream_path(const nsd_dims *d, int32_t M);
int64_t nsd_multi_stream_state_bytes(const nsd_dims *d, int32_t M, int32_t S);
int nsd_multi_stream_step(const nsd_dims *d, int32_t M, const float *params, const float *x, int64_t x_model_stride, const int32_t *slots,
                          uint32_t flags, void *state, int64_t state_bytes, int32_t S, float *logits, float *probs, float *mean_probs,
                          void *stream);

/*
 * ---- session calibration: refit the read-out on frozen pooled features in ONE launch (an EXTENSION, of nsd_stream_*) ----
 *
 * A model trained on earlier sessions meets a new one: a few cued trials are pushed through a stream, the pooled vector each slot holds is
 * read out (nsd_stream_features), and the trainable tail of the model -- LayerNorm, fc.0, fc.3 of lstm_eeg_model.py:38-39; the LSTM stack
 * and the attention stay frozen -- is refitted on those vectors by E full-batch Adam epochs in one launch (nsd_head_fit), one 256-thread
 * workgroup per model, M models (the folds of an ensemble) per launch, no host in the loop.
 *   nsd_stream_features   feats[i, j] = pool_acc[j] / pool_den of slot slots[i] (DEVICE int32[n], or NULL for 0 .. n-1), j < H: the one
 *                         correctly rounded fp32 division whose result nsd_stream_step's read-out is formed from, so the row is exactly
 *                         the vector whose read-out the slot's decision is.  A slot that was never stepped gives a NaN row (0 / 0), a slot
 *                         index outside [0, S) a NaN row too; nothing outside feats[n,H] is written.  The state of an ensemble is read
 *                         as a flat state of M*S slots, as nsd_stream_reset reads it.  Refusals before any launch, as nsd_stream_step:
 *                         NSD_E_INVALID for NULL d / state / feats, a shape outside nsd_stream_path, S < 1, n < 0, n > S with slots ==
 *                         NULL; NSD_E_WORKSPACE for state_bytes < nsd_stream_state_bytes(d, S).  n = 0 launches nothing.
 * nsd_head_fit.  Per model m: theta = params + m*P (the whole flat vector; only its tail is touched), N = d->B trials, features
 * feats + m*feats_model_stride [N,H], target rows targets[m*N + n][K].  One epoch is one full-batch Adam step on
 *   LayerNorm (biased variance, eps 1e-5 inside the square root) -> fc.0 -> RReLU -> dropout -> fc.3,
 *   loss_n = - sum_k q log softmax,  dlogits = scale (s p - q): the soft-target convention above (nsd_head_train_soft), formed without
 *   the O(1) - O(1) difference.
 * The gradient of a parameter is the sum over the trials in ascending n, one fmaf chain per parameter: a fixed order that does not depend
 * on M, on the model's place in the grid, or on the stream.  The update is nsd_adam_step's arithmetic (gi = fmaf(weight_decay, p, g):
 * coupled L2), every fp32 operation rounded on its own; the bias corrections are formed in double on the device from the 1-based GLOBAL
 * epoch number s (beta^s by repeated squaring, a function of s alone), lr / bc1 and 1 / sqrt(bc2) rounded to fp32 as there.
 * Only the tensors named in fit->train change (NSD_FIT_LN: ln.weight, ln.bias; NSD_FIT_FC0: fc.0.*; NSD_FIT_FC3: fc.3.*); every other
 * float of params -- always all LSTM tensors, attn.weight, attn.bias -- is bit for bit what it was.  The gradient flows through an
 * untrained tensor unchanged.
 * Noise.  rng == NULL: the eval slope and no dropout.  Otherwise global epoch e (0-based, from the state) of model m draws what a
 * trainer's step e draws for a batch of N trials: RReLU slopes [N,F] and head-dropout multipliers [N,F] are the values nsd_train_masks
 * writes for seed = rng[m].seed, base_stream = rng[m].base_stream + 4e (uint32 wrap), p_head = rng[m].p_head.  p_lstm is ignored.
 * State (device, caller-owned, nsd_head_fit_state_bytes(d, M) bytes): per model `stride` floats -- m[Pt] at `m`, v[Pt] at `v`, the int64
 * global epoch count at `epochs` (8-byte aligned), the int32 status word at `status` -- with Pt = 2H + FH + F + KF + K and the tail in
 * the flat order without the attention: ln.weight ln.bias fc.0.weight fc.0.bias fc.3.weight fc.3.bias.  All-zero bytes is the reset
 * state (hipMemsetAsync is enough; there is no reset entry point).  The state and the parameters after e1 + e2 epochs are the same bits
 * whether the epochs ran in one call or in two, and so is row e of loss_out.  loss_out[m, e] = scale * sum_n loss_n before that epoch's
 * update, the sum serial in n.
 *   nsd_head_fit_path     1 where nsd_stream_path(d), 1 <= M <= NSD_MAX_MODELS, 1 <= N = d->B <= NSD_FIT_MAX_TRIALS and the workgroup's
 *                         LDS need, 4 * (N * (2H + F + K + 3) + 2H + F(H+1) + F + K(F|1) + K + Pt + 520) bytes, is at most 160 KiB.  At the
 *                         reference head (F = 32, K <= 8) that holds up to N = 256; at F = 64, K = 8 up to N = 192, at F = K = 64 up to
 *                         N = 112.  The limit does not depend on M or on fit->train.
 * Failure behaviour.  Every refusal happens before any launch.  NSD_E_INVALID: NULL d / params / feats / targets / fit / fit_state; a shape
 * outside nsd_head_fit_path; epochs outside [1, NSD_FIT_MAX_EPOCHS]; an empty or unknown train mask; lr negative or not finite, a beta
 * outside [0, 1), eps not positive or not finite, weight_decay negative or not finite, scale not finite (nsd_adam_step itself checks
 * none of these); a negative feats_model_stride or one in (0, N*H); rng with a p_head outside [0, 1).  NSD_E_WORKSPACE: fit_state_bytes <
 * nsd_head_fit_state_bytes(d, M).  Seen on the device only, and never silent: when a feature or a target of a model is not finite, or its
 * status word is already set, the model's parameters, moments and epoch count keep their bits, its row of loss_out is NaN and its status
 * word becomes (stays) 1 until the state is zeroed; when an epoch's loss is not finite, parameters, moments and the count keep the values
 * they had before that epoch, that epoch's and the remaining entries of loss_out are NaN and the status word becomes 1.  The other models
 * of the launch are unaffected.  No host synchronisation, no allocation: the call can be captured in a single-stream graph and replayed
 * (the epoch count lives in the state).  Additive: NSD_VERSION stays 301, a caller detects the feature by the symbols.
 */
int nsd_stream_features(const nsd_dims *d, const void *state, int64_t state_bytes, int32_t S,
                        const int32_t *slots /* DEVICE int32[n] or NULL = 0..n-1 */, int32_t n, float *feats /* [n,H] */, void *stream);
#define NSD_FIT_MAX_TRIALS 256
#define NSD_FIT_MAX_EPOCHS 65536
#define NSD_FIT_LN  1u   /* ln.weight, ln.bias     */
#define NSD_FIT_FC0 2u   /* fc.0.weight, fc.0.bias */
#define NSD_FIT_FC3 4u   /* fc.3.weight, fc.3.bias */
typedef struct nsd_fit {
    int32_t epochs;                 /* epochs of THIS call, 1 .. NSD_FIT_MAX_EPOCHS */
    uint32_t train;                 /* non-empty subset of NSD_FIT_* */
    float lr, beta1, beta2, eps, weight_decay, scale;   /* scale: 1/N in the Python layer */
} nsd_fit;
typedef struct nsd_fit_layout { int64_t m, v, epochs, status, stride; } nsd_fit_layout;  /* float offsets per model */
int     nsd_head_fit_path(const nsd_dims *d, int32_t M);      /* d->B = N trials */
int64_t nsd_head_fit_state_bytes(const nsd_dims *d, int32_t M);
int     nsd_head_fit_state_layout(const nsd_dims *d, nsd_fit_layout *out);
int nsd_head_fit(const nsd_dims *d, int32_t M, float *params /* [M,P] in/out */,
                 const float *feats, int64_t feats_model_stride /* 0: one set for all models, else >= N*H */,
                 const float *targets /* [M*N][K] */, const nsd_fit *fit, const nsd_rng *rng /* NULL or [M] */,
                 void *fit_state, int64_t fit_state_bytes, float *loss_out /* [M, fit->epochs] or NULL */, void *stream);

/*
 * ---- sliding-window decisions for continuous streams in one launch per chunk (an EXTENSION, of nsd_stream_*) ----
 *
 * "Every `hop` samples, the decision of the model run from a zero state over the last `window` samples."  window = W >= 1, hop = Hp with
 * 1 <= Hp <= W, W % Hp == 0 and R = W / Hp <= NSD_WINDOW_MAX_PHASES.  A stream's samples are numbered from its last reset, n = 0, 1, ...
 * Window k (k = 0, 1, ...) covers samples [k Hp, k Hp + W); its END is e_k = k Hp + W, and its decision exists once sample e_k - 1 has been
 * pushed.  PHASE r = k mod R decodes the windows k = r (mod R): it idles until sample r Hp, then runs its windows back to back, each from
 * a reset slot.
 * Contract.  The decision of window k is bit for bit what nsd_stream_step writes (logits and probs) when a freshly reset slot is given
 * x[k Hp : k Hp + W] -- whatever the cut of the stream into calls, B, the slot, the placement in the grid, the HIP stream or a graph replay.
 * State: per stream R PHASE SLOTS followed by a header, stream_stride floats in all; S streams.  A phase slot is an ordinary slot of the
 * public nsd_stream_layout (phase_stride = its stride); its step count is the number of samples its current window has consumed, in
 * [0, W), and it can be copied out and handed to nsd_stream_step as it is.  The header records W and Hp (int32 words at the float offsets
 * `window` and `hop` from the stream's start) and the stream's int64 sample count n at `count` (8-byte aligned).  The count is kept once
 * per phase, R consecutive int64 from `count` on, all equal between calls: each phase's workgroup reads and writes its own copy, so that
 * no workgroup of a launch reads a word another one writes.  Everything a call needs is derived on the device from n: nothing in the
 * arguments changes from call to call, and nsd_prep_step + nsd_window_step can be captured once and replayed.
 *   nsd_window_path          1 where nsd_stream_path(d) and the conditions on W and Hp above hold, else 0
 *   nsd_window_rows          D = ceil(T / hop): the decisions a call of T samples can complete per stream; <0 for T < 1 or an invalid w
 *   nsd_window_state_bytes   bytes of a state of S >= 1 streams (S * stream_stride * 4); <0 outside nsd_window_path or for S < 1
 *   nsd_window_state_layout  phases = R, phase_stride, window, hop, count, stream_stride: float offsets from a stream's start
 *   nsd_window_reset         slots == NULL: all S streams; else the n streams of the DEVICE array slots[n] (indices outside [0, S) are
 *                            skipped).  Every phase slot becomes a reset nsd_stream_layout slot, the header records W and Hp, n = 0.  A
 *                            state is reset once before its first nsd_window_step, and again to change W or Hp.
 *   nsd_window_step          d->B streams, chunk length d->T >= 1, x [B,T,C]; slots: DEVICE int32[B] of distinct indices in [0, S), or
 *                            NULL for 0 .. B-1; flags: NSD_FLAG_RESIDUAL.  Outputs, with D = nsd_window_rows(d->T, w) and n0 the
 *                            stream's count before the call: the windows with n0 < e_k <= n0 + T are written in ascending e_k to rows
 *                            0 .. counts[b] - 1 of logits [B,D,K] and probs [B,D,K] (or NULL), ends[b,i] = e_k (int64 [B,D]); rows
 *                            counts[b] .. D-1 are written too, NaN in logits / probs and -1 in ends, so that a call's outputs are a
 *                            function of its inputs.  counts: int32 [B].
 * Failure behaviour.  Every refusal happens before any launch: NSD_E_INVALID for NULL d / w / params / x / state / logits / ends /
 * counts, a shape outside nsd_window_path, T < 1, S < 1, n < 0 or n > S (reset), B > S, flags other than NSD_FLAG_RESIDUAL, B * D * K
 * above 2^31 - 1; NSD_E_WORKSPACE when state_bytes < nsd_window_state_bytes(d, w, S).  B = 0 (n = 0) launches nothing.  Seen on the device
 * only, and never silent: a slot index outside [0, S), or a stream whose header records another (W, Hp) than the call's, is skipped -- all
 * its D rows are NaN / -1, counts[b] = -1, no state is touched.  Duplicate slots in one call are undefined.  A sample that is not finite
 * (NaN or +-Inf) poisons exactly the windows that contain it: their rows are NaN, every other window's rows are the bits of the clean
 * run, and the stream heals on its own once the sample has left every window, because a phase's reset overwrites its state.  No host
 * synchronisation, no allocation.  Additive: NSD_VERSION stays 301, a caller detects the feature by the symbols.
 */
#define NSD_WINDOW_MAX_PHASES 128
typedef struct nsd_window { int32_t window, hop; } nsd_window;
typedef struct nsd_window_layout {
    int64_t phases, phase_stride;                   /* R phase slots of phase_stride floats each, from the stream's start */
    int64_t window, hop;                            /* int32 words: float offsets */
    int64_t count;                                  /* int64 sample count (R copies, one per phase): float offset, even */
    int64_t stream_stride;                          /* floats per stream, a multiple of 4 */
} nsd_window_layout;
int     nsd_window_path(const nsd_dims *d, const nsd_window *w);
int32_t nsd_window_rows(int32_t T, const nsd_window *w);
int64_t nsd_window_state_bytes(const nsd_dims *d, const nsd_window *w, int32_t S);
int     nsd_window_state_layout(const nsd_dims *d, const nsd_window *w, nsd_window_layout *out);
int     nsd_window_reset(const nsd_dims *d, const nsd_window *w, void *state, int64_t state_bytes, int32_t S, const int32_t *slots,
                         int32_t n, void *stream);
int     nsd_window_step(const nsd_dims *d, const nsd_window *w, const float *params, const float *x, const int32_t *slots, uint32_t flags,
                        void *state, int64_t state_bytes, int32_t S, float *logits, float *probs, int64_t *ends, int32_t *counts,
                        void *stream);

/*
 * ---- sliding-window decisions from an ensemble: M models per stream in one launch (an EXTENSION, of the two above: nsd_multi_stream_*,
 * nsd_window_*) ----
 *
 * nsd_multi_window_step is to nsd_window_step what nsd_multi_stream_step is to nsd_stream_step: it advances the B continuous streams of a
 * call in each of M models of one shape -- params [M,P], P = nsd_param_count(d) -- by one launch of the step nsd_window_step runs (the
 * same source, csrc/nsd_window48.hip, compiled with a model view), and can return the ensemble's mean probabilities per window.
 * State: [M][S][stream_stride] floats.  Model m's part starts at float m * S * stream_stride and is an ordinary window state of S streams
 * in the public nsd_window_layout: it can be handed to nsd_window_step as it is (with params + m*P).  The whole buffer is a flat state of
 * M*S streams to nsd_window_reset -- stream m*S + s is stream s of model m, slots == NULL resets everything -- so there is no reset entry
 * of its own, and the state must be reset once before its first step.
 *   nsd_multi_window_path         1 where nsd_window_path(d, w) and 1 <= M <= NSD_MAX_MODELS, else 0
 *   nsd_multi_window_state_bytes  M * nsd_window_state_bytes(d, w, S); <0 outside the path or for S < 1
 *   nsd_multi_window_step         d->B streams, chunk length d->T >= 1.  x: model m reads the chunk [B,T,C] at x + m * x_model_stride
 *                                 floats; 0: one chunk for all models, else >= B*T*C.  slots: DEVICE int32[B] of distinct indices in
 *                                 [0, S) or NULL for 0 .. B-1, shared by the models: stream b lives in stream slots[b] of every model's
 *                                 part.  Outputs, with D = nsd_window_rows(d->T, w): logits [M,B,D,K] (required), probs [M,B,D,K] or
 *                                 NULL, mean_probs [B,D,K] or NULL, ends int64 [M,B,D], counts int32 [M,B].
 * Contract.  Model m's part of the state after the call, and its blocks of logits / probs / ends / counts -- the NaN / -1 rows from
 * counts[m,b] on included -- are bit for bit what
 *   nsd_window_step(d, w, params + m*P, x + m*x_model_stride, slots, flags, state + m*S*stream_stride, S*stream_stride*4, S,
 *                   logits + m*B*D*K, probs + m*B*D*K, ends + m*B*D, counts + m*B)
 * leaves and writes, for any M, B, cut of the stream, slot, placement in the grid, HIP stream or graph replay.  Workgroups m*G ..
 * m*G + G - 1 walk model m's B*R (stream, phase) pairs, G = min(B*R, max(1, CUs / M)).
 * mean_probs[b,i,k] = (((p_0 + p_1) + p_2) + ... + p_{M-1}) / (float)M with p_m = probs[m,b,i,k]: a serial fp32 sum in m, every addition
 * rounded on its own, then one correctly rounded division.  It is formed from the probs buffer by a second small launch that the same
 * call enqueues behind the step.  Where every model's row i is a decision, the mean row is that mean; where any model's row is NaN -- an
 * unused row, a poisoned window, a skipped model -- the mean row is NaN (some NaN: test it with isnan, not by its payload).
 * Failure behaviour.  Every refusal happens before any launch: NSD_E_INVALID for all that nsd_window_step refuses, for M outside
 * [1, NSD_MAX_MODELS], mean_probs without probs, x_model_stride negative or positive and below B*T*C, M * B * D * K above 2^31 - 1;
 * NSD_E_WORKSPACE when state_bytes < nsd_multi_window_state_bytes(d, w, M, S).  B = 0 launches nothing.  Seen on the device only, and never
 * silent: a slot index outside [0, S) is skipped in every model -- counts[m,b] = -1, all its rows NaN / -1, no state touched; a model whose
 * header for that stream records another (W, Hp) than the call's is skipped for that model alone -- its rows are NaN / -1, its counts[m,b]
 * is -1, the stream's mean rows are NaN, and the other models' bits are those of the clean run.  A sample that is not finite poisons
 * exactly the windows that contain it, in every model that reads it, and the stream heals as in nsd_window_step.  No host synchronisation,
 * no allocation: nsd_prep_step + nsd_multi_window_step (the step and the mean launch) can be captured in one single-stream graph and
 * replayed.  Additive: NSD_VERSION stays 301, a caller detects the feature by the symbols.
 */
int     nsd_multi_window_path(const nsd_dims *d, const nsd_window *w, int32_t M);
int64_t nsd_multi_window_state_bytes(const nsd_dims *d, const nsd_window *w, int32_t M, int32_t S);
int     nsd_multi_window_step(const nsd_dims *d, const nsd_window *w, int32_t M, const float *params, const float *x, int64_t x_model_stride,
                              const int32_t *slots, uint32_t flags, void *state, int64_t state_bytes, int32_t S, float *logits, float *probs,
                              float *mean_probs, int64_t *ends, int32_t *counts, void *stream);

/*
 * ---- causal front end for live streams and their training (an EXTENSION: the reference filters whole windows on the host) ----
 *
 * A per-channel transform that can run chunk by chunk in front of nsd_stream_step, and over whole windows in a training step, so that a
 * model is trained on what a live stream can deliver.  For one stream, n = samples since the slot's reset (it lives in the state), c the
 * channel, x[n,c] the raw sample.  Every fp32 operation rounds on its own (no FMA contraction); sqrt and / are the correctly rounded
 * ones.  Four steps, in this order, each SKIPPED when it is off (all off: y is a bitwise copy of x):
 *   NSD_PREP_BASELINE  at n == 0: x0[c] = x[0,c] (kept in the state);  v = x[n,c] - x0[c]                  (without the flag v = x[n,c])
 *   NSD_PREP_CAR       m = (((v[0] + v[1]) + v[2]) + ...) over c = 0 .. C-1, serially;  v = v - m / float(C)
 *   sections           n_sections in [0, NSD_PREP_MAX_SECTIONS], sos[s] = {b0, b1, b2, a1, a2} (a0 = 1), the same for all channels;
 *                      direct form II transposed from rest, in order:  y = b0*v + z1;  z1 = (b1*v - a1*y) + z2;  z2 = b2*v - a2*y;  v = y
 *   running z-score    alpha > 0, oma = 1.0f - alpha.  At n == 0: mu = v, var = var0; otherwise d = v - mu, mu = mu + alpha*d,
 *                      var = oma * (var + (alpha*d)*d).  Output (v - mu) / (sqrt(var) + 1e-6f) with the updated mu and var.
 * The baseline comes first because the sections lose the signal under a DC offset of raw amplifier size (fp32 against float64 on a
 * 1-40 Hz band-pass + notch with offsets up to 2e5: 1.3e-2 of the largest output without it, 3.7e-3 with it behind the common average,
 * below 1e-5 in this order).  Every sample runs the same operations wherever it falls in a chunk: the state after n samples, and every
 * output, is bit for bit a function of the samples alone -- not of the cut, the slot, the other streams of the call, the HIP stream or a
 * graph replay.  Non-finite samples propagate by the arithmetic: a poisoned channel stays NaN until its slot is reset, and with the
 * common average every channel of that stream is poisoned; other streams are unaffected.
 *   nsd_prep_path          1 where nsd_prep_step covers C channels with the configuration p (p == NULL: C alone), else 0
 *   nsd_prep_state_bytes   bytes of a state of S >= 1 slots (S * stride * 4); <0 for C outside [1, 64] or S < 1
 *   nsd_prep_state_layout  float offsets inside a slot: x0[C], z[NSD_PREP_MAX_SECTIONS][2][C] (z1 then z2 of each section), mu[C],
 *                          var[C]; `steps`: the float offset of the slot's int64 sample count (8-byte aligned); `stride`: floats per
 *                          slot.  The layout holds room for the maximum number of sections and depends on C only: a slot can be
 *                          checkpointed and restored by copying its stride floats.
 *   nsd_prep_reset         slots == NULL: all S slots; else the n slots of the DEVICE array slots[n] (indices outside [0, S) are
 *                          skipped).  A reset slot is all zero.  A state is reset once before its first nsd_prep_step.
 *   nsd_prep_step          x, y [B,T,C] (of d only B, T, C are read); y == x (in place) is allowed, a partial overlap is refused.
 *     stream mode (state != NULL): d->B streams advance by d->T samples; slots: DEVICE int32[B] of distinct indices, or NULL for
 *       0 .. B-1.  A slot index outside [0, S) is skipped and its rows of y are NaN.  No host synchronisation, no allocation; nothing in
 *       the arguments changes from call to call, so the call can be captured and replayed in front of nsd_stream_step.
 *     window mode (state == NULL, slots == NULL, S ignored): every trial starts from a reset state and nothing is stored.
 * NSD_E_INVALID before any launch: NULL d / p / x / y; C outside [1, 64]; T < 1; B < 0; B > S or S < 1 (stream mode); slots without a
 * state; unknown flag bits; n_sections outside [0, NSD_PREP_MAX_SECTIONS]; a coefficient that is not finite; an unstable section (stable:
 * |a2| < 1 and |a1| < 1 + a2); alpha outside [0, 1); var0 not finite, or var0 <= 0 while alpha > 0; partially overlapping x / y.
 * NSD_E_WORKSPACE: state_bytes < nsd_prep_state_bytes(C, S).  B = 0 (n = 0) launches nothing.  Additive: NSD_VERSION stays 301, a caller
 * detects the feature by the symbols.
 */
#define NSD_PREP_MAX_SECTIONS 4
#define NSD_PREP_BASELINE 1u
#define NSD_PREP_CAR      2u
typedef struct nsd_prep { uint32_t flags; int32_t n_sections; float sos[NSD_PREP_MAX_SECTIONS][5]; float alpha, var0; } nsd_prep;
typedef struct nsd_prep_layout { int64_t x0, z, mu, var, steps, stride; } nsd_prep_layout;   /* float offsets in a slot; depends on C only */
int     nsd_prep_path(int32_t C, const nsd_prep *p);
int64_t nsd_prep_state_bytes(int32_t C, int32_t S);
int     nsd_prep_state_layout(int32_t C, nsd_prep_layout *out);
int     nsd_prep_reset(int32_t C, void *state, int64_t state_bytes, int32_t S, const int32_t *slots, int32_t n, void *stream);
int     nsd_prep_step(const nsd_dims *d, const nsd_prep *p, const float *x, const int32_t *slots,
                      void *state, int64_t state_bytes, int32_t S, float *y, void *stream);

/*
 * ---- signal-quality gate for live streams (an EXTENSION: the reference has no notion of a bad channel or an artefact) ----
 *
 * A causal detector of flat, railed, jumping and high-amplitude spans per channel, in two stages around the front end above:
 *   nsd_gate_step (stateful)  raw samples -> y (a bad channel holds its last good value, so the sections and the common average behind
 *                             it stay finite and calm) and one mask word per step;
 *   nsd_gate_apply (stateless) behind the front end: a bad channel is zeroed in front of the model, a step that is bad on too many
 *                             channels becomes NaN -- which the window decoders' poison contract turns into "no decision" for exactly
 *                             the windows that contain it.
 * For one stream, n = samples since the slot's reset, c the channel, x[n,c] the raw sample, prev = x[n-1,c].  Every fp32 operation
 * rounds on its own (a - b is one correctly rounded subtraction); everything else is fabsf and comparisons, so the outputs and the state
 * after n samples are bit for bit a function of the samples alone -- not of the cut, the slot, the other streams of the call, the HIP
 * stream or a graph replay.  The detectors of nsd_gate, each off at 0:
 *   rail          bad if |x| >= rail
 *   jump          bad if n > 0, prev finite and |x - prev| >= jump
 *   flat_samples  a pair is flat if n > 0, both samples are finite and |x - prev| <= flat_eps;
 *                 run = flat pair ? min(run + 1, flat_samples) : 0;  bad if run >= flat_samples - 1 (flat_samples equal samples in a row)
 *   pp_samples    hi, lo over the FINITE raw samples max(0, n - pp_samples + 1) .. n;  bad if there is one and hi - lo >= pp
 *   raw_bad = !isfinite(x) | rail | jump | flat | pp.   raw_bad: hang = hold_samples, the sample is bad;  else if hang > 0: the sample
 *   is bad, hang -= 1;  else the sample is good and held = x.   y[n,c] = bad ? held[c] : x[n,c] (held is 0 after a reset);  mask[n] has
 *   bit c set where channel c is bad, which bounds C to [1, 32].  A step with more than max_bad bits set is REJECTED.
 *   nsd_gate_path          1 where nsd_gate_step covers C channels with the configuration g (g == NULL: C alone), else 0
 *   nsd_gate_state_bytes   bytes of a state of S >= 1 slots (S * stride * 4); <0 for C outside [1, 32] or S < 1
 *   nsd_gate_state_layout  offsets inside a slot in 4-byte words: prev[C], held[C] (fp32), run[C], hang[C] (int32), ring[64][C] (fp32,
 *                          ring[n mod 64][c] = x[n,c]), bad[C] (int64 counts of bad samples, 8-byte aligned), rejected (int64 count of
 *                          rejected steps), steps (int64), and the stride.  The layout depends on C only: a slot can be checkpointed
 *                          and restored by copying its stride words.
 *   nsd_gate_reset         as nsd_prep_reset: slots == NULL: all S slots; else the n slots of the DEVICE array slots[n] (indices outside
 *                          [0, S) are skipped).  A reset slot is all zero.
 *   nsd_gate_step          x, y [B,T,C], mask [B,T] uint32 (of d only B, T, C are read); y == x is allowed, a partial overlap is refused.
 *     stream mode (state != NULL): slots as in nsd_prep_step; a slot index outside [0, S) is skipped: its rows of y are NaN, its mask
 *       rows are all ones (0xFFFFFFFF) and no state is touched.  No host synchronisation, no allocation: the call can be captured.
 *     window mode (state == NULL, slots == NULL, S ignored): every trial starts from a reset state and nothing is stored.
 *   nsd_gate_apply         v, out [B,T,C], mask [B,T] (of g only max_bad and flags are read).  popcount(mask) > max_bad: all C values of
 *                          the step are NaN.  Otherwise a bad channel is 0.0f with NSD_GATE_ZERO and left as it is without the flag; a
 *                          good one is a bitwise copy.  out == v is allowed, a partial overlap is refused.
 * NSD_E_INVALID before any launch: NULL d / g / x / y / mask (v / out); C outside [1, 32]; T < 1; B < 0; B > S or S < 1 (stream mode);
 * slots without a state; a threshold (rail, jump, flat_eps, pp) that is negative or not finite; flat_samples < 0; pp_samples outside
 * [0, NSD_GATE_MAX_SPAN]; hold_samples < 0; max_bad < 0; unknown flag bits; partially overlapping x / y (v / out).
 * NSD_E_WORKSPACE: state_bytes < nsd_gate_state_bytes(C, S).  B = 0 (n = 0) launches nothing.  Additive: NSD_VERSION stays as it is, a
 * caller detects the feature by the symbols.
 */
#define NSD_GATE_MAX_SPAN 64
#define NSD_GATE_ZERO 1u
typedef struct nsd_gate {
    float   rail;          /* 0 = off.  bad if |x| >= rail */
    float   jump;          /* 0 = off.  bad if n > 0, prev finite and |x - prev| >= jump */
    float   flat_eps;      /* with flat_samples > 0: a pair is flat if both finite and |x - prev| <= flat_eps */
    int32_t flat_samples;  /* 0 = off */
    float   pp;            /* with pp_samples > 0: bad if hi - lo >= pp over the finite raw samples of the span */
    int32_t pp_samples;    /* 0 = off, else 1 .. NSD_GATE_MAX_SPAN */
    int32_t hold_samples;  /* >= 0: after a raw-bad sample the channel stays bad for this many further samples */
    int32_t max_bad;       /* a step with more than max_bad bad channels is rejected; max_bad >= C: never */
    uint32_t flags;        /* NSD_GATE_ZERO */
} nsd_gate;
typedef struct nsd_gate_layout { int64_t prev, held, run, hang, ring, bad, rejected, steps, stride; } nsd_gate_layout;   /* 4-byte words */
int     nsd_gate_path(int32_t C, const nsd_gate *g);
int64_t nsd_gate_state_bytes(int32_t C, int32_t S);
int     nsd_gate_state_layout(int32_t C, nsd_gate_layout *out);
int     nsd_gate_reset(int32_t C, void *state, int64_t state_bytes, int32_t S, const int32_t *slots, int32_t n, void *stream);
int     nsd_gate_step(const nsd_dims *d, const nsd_gate *g, const float *x, const int32_t *slots,
                      void *state, int64_t state_bytes, int32_t S, float *y, uint32_t *mask, void *stream);
int     nsd_gate_apply(const nsd_dims *d, const nsd_gate *g, const float *v, const uint32_t *mask, float *out, void *stream);

/*
 * ---- session alignment: channel covariance and whitening (an EXTENSION: the reference never mixes channels) ----
 *
 * Euclidean alignment: a session is whitened by the inverse square root of its mean channel second moment, y = R^(-1/2) x, a fixed
 * C x C matrix at serve time.  Three stages behind nsd_gate_apply, C in [1, 32] (the gate's range):
 *   nsd_cov_step (stateful)     accumulates sum[i][j] += (double)v[i] * (double)v[j] over the USED steps of a stream, beside the stream;
 *   nsd_whiten_fit              forms W = R'^(-1/2) per group of accumulators, on the device;
 *   nsd_spatial_apply (stateless)  out[b,t,:] = W[sel[b]] . v[b,t,:] in front of the model.
 * The formula is the RAW second moment R = (1/n) sum_t v[t] v[t]^T, not a centred covariance: the signal behind a high-pass or baseline
 * stage is near zero-mean, and a raw moment composes over chunks and sessions by adding sums and counts.
 *
 * nsd_cov_step.  v [B,T,C] fp32, mask NULL or [B,T] uint32 (the words of nsd_gate_step).  The samples of a stream are taken in ascending
 * order.  A step is USED if all its C values are finite and, where a mask is given, its word is 0; a used step does, for all i, j,
 * sum[i][j] = sum[i][j] + (double)v[i] * (double)v[j] (the product of two fp32 values is exact in double, so contraction cannot change
 * a bit) and count += 1; any other step does skipped += 1 and adds nothing.  The full matrix is stored and is symmetric bit for bit.
 * Every (i, j) is one serial chain over time: the state after n samples is bit for bit a function of the samples alone -- not of the
 * cut, the slot, the other streams of the call, the HIP stream or a graph replay.
 *   stream mode (state != NULL, sums == counts == NULL): one slot is sum[C][C] (double), count, skipped (int64): C*C + 2 8-byte words.
 *     slots as in nsd_prep_step; a slot index outside [0, S) touches nothing.
 *   window mode (state == NULL, slots == NULL, S ignored): every trial starts from zero; trial b's matrix goes to sums[b] ([B][C][C]
 *     double) and its {count, skipped} to counts[b] ([B][2] int64).
 *   nsd_cov_state_bytes / nsd_cov_state_layout (offsets in 8-byte words) / nsd_cov_reset: as the prep functions of those names; a reset
 *   slot is all zero.
 *
 * nsd_whiten_fit.  N accumulators: accumulator a's matrix is sums + a * sum_stride (doubles), its {count, skipped} counts + a *
 * count_stride (int64 words) -- window-mode outputs (strides C*C and 2) or a stream state read in place (sums = state, counts =
 * (int64 *)state + C*C, both strides C*C + 2).  group: DEVICE int32[N] or NULL (every accumulator in group 0); an index outside [0, G) is
 * ignored and counted in every record.  One workgroup per group, all in double:
 *   S = sum of the group's matrices in ascending accumulator order, n = sum of their counts;  R = S / n;
 *   R' = (1 - shrinkage) * R + shrinkage * (tr R / C) * I;
 *   a cyclic Jacobi eigen-solve of R' (pairs (p, q) row by row; a pair is rotated unless |a_pq| <= 2^-53 * sqrt(|a_pp * a_qq|)); it stops
 *   after the first sweep that rotates nothing, or after NSD_WHITEN_MAX_SWEEPS sweeps;
 *   eigenvalues are clipped from below at floor * lambda_max;  W = V diag(lambda^(-1/2)) V^T, symmetric bit for bit, rounded once to fp32.
 * Record per group (nsd_whiten_record, 64 bytes): steps used and skipped, tr R / C, the smallest and largest eigenvalue before the clip,
 * sweeps taken, accumulators of the group, ignored accumulators, and a status word:
 *   NSD_WHITEN_FEW            n < min_steps: W is the identity (a group without accumulators has n = 0)
 *   NSD_WHITEN_NONFINITE      a sum that is not finite, or tr R <= 0 (tested where FEW is not set): W is the identity
 *   NSD_WHITEN_CLIPPED        at least one eigenvalue was floored
 *   NSD_WHITEN_NOT_CONVERGED  the sweep cap was reached; W is written all the same
 * Where W is the identity the record's trace, eigenvalues and sweeps are 0.  A bad group never touches another group's output.
 *
 * nsd_spatial_apply.  v, out [B,T,C], W [n_mat][C][C] fp32, sel: DEVICE int32[B] or NULL (matrix 0 for every row b).
 *   out[b,t,i] = ((W[i][0]*v[0] + W[i][1]*v[1]) + ...) serially over j, every fp32 operation rounding on its own.  A NaN anywhere in a
 *   step makes the whole step NaN by the arithmetic (0 * NaN is NaN).  A sel entry outside [0, n_mat) gives NaN rows.  out == v is
 *   allowed (a workgroup reads all its steps before it writes one), a partial overlap is refused.
 *
 * NSD_E_INVALID before any launch: a NULL d / v / out / W / sums / counts / records where one is needed; C outside [1, 32]; T < 1; B < 0;
 * B > S or S < 1 (stream mode); slots without a state; sums or counts with a state; a state that is not 8-byte aligned; N < 0, G < 1,
 * n_mat < 1; a stride below its row (sum_stride < C*C, count_stride < 2); shrinkage outside [0, 1]; floor outside (0, 1]; min_steps < 1;
 * partially overlapping v / out.  NSD_E_WORKSPACE: state_bytes < nsd_cov_state_bytes(C, S).  B = 0 (n = 0) launches nothing; N = 0
 * still writes G identities.  No allocation, no host synchronisation: every call can be captured.  Additive: NSD_VERSION stays as it
 * is, a caller detects the feature by the symbols.
 */
#define NSD_WHITEN_MAX_SWEEPS 40
#define NSD_WHITEN_FEW           1u
#define NSD_WHITEN_NONFINITE     2u
#define NSD_WHITEN_CLIPPED       4u
#define NSD_WHITEN_NOT_CONVERGED 8u
typedef struct nsd_whiten { float shrinkage; float floor; int32_t min_steps; } nsd_whiten;
typedef struct nsd_whiten_record {
    int64_t steps, skipped;                  /* used and skipped steps of the group's accumulators */
    double  trace_mean, eig_min, eig_max;    /* tr R / C; the eigenvalues of R' before the clip */
    int32_t sweeps; uint32_t status;
    int32_t accumulators, ignored;           /* accumulators of this group; accumulators of the call with a group index outside [0, G) */
    int64_t reserved;
} nsd_whiten_record;
typedef struct nsd_cov_layout { int64_t sum, count, skipped, stride; } nsd_cov_layout;   /* 8-byte words in a slot; depends on C only */
int64_t nsd_cov_state_bytes(int32_t C, int32_t S);
int     nsd_cov_state_layout(int32_t C, nsd_cov_layout *out);
int     nsd_cov_reset(int32_t C, void *state, int64_t state_bytes, int32_t S, const int32_t *slots, int32_t n, void *stream);
int     nsd_cov_step(const nsd_dims *d, const float *v, const uint32_t *mask, const int32_t *slots,
                     void *state, int64_t state_bytes, int32_t S, double *sums, int64_t *counts, void *stream);
int     nsd_whiten_fit(int32_t C, const nsd_whiten *w, const double *sums, int64_t sum_stride, const int64_t *counts, int64_t count_stride,
                       int32_t N, const int32_t *group, int32_t G, float *W, nsd_whiten_record *records, void *stream);
int     nsd_spatial_apply(const nsd_dims *d, const float *v, const float *W, int32_t n_mat, const int32_t *sel, float *out, void *stream);

/*
 * ---- supervised session alignment: the backward of nsd_spatial_apply and an Adam step on the matrix (an EXTENSION) ----
 *
 * nsd_spatial_apply is the forward of a linear layer in front of the model; with nsd_lstm_bwd's dx (nsd_dx_path) these two calls fit its
 * matrix on labelled trials by gradient descent through the frozen model, everything on the device.
 *
 * nsd_spatial_bwd.  v, dy, dv [B,T,C] fp32, W and dW [n_mat][C][C] fp32, sel as in the apply, C in [1, 32].  d->B, T, C are read.
 *   dv (NULL: not formed): dv[b,t,j] = ((W[0][j]*dy[0] + W[1][j]*dy[1]) + ...) serially over i with W = W[sel[b]], every fp32 operation
 *     rounding on its own -- the apply with the matrix transposed, in the apply's kernel.  A sel entry outside [0, n_mat) gives NaN rows.
 *     dv == dy is allowed, a partial overlap is refused.
 *   dW (NULL: not formed), in two fixed stages:
 *     1. p[b][i][j] is ONE serial chain over t ascending in double, s = s + (double)dy[b,t,i] * (double)v[b,t,j] (an exact product, one
 *        rounding per sum), one workgroup per row b;
 *     2. dW[m][i][j] = (float) of ONE serial double chain over b ascending with sel[b] == m -- a second small launch behind the first.
 *     The bits therefore do not depend on the grid, the tiling, the HIP stream or a graph replay.  A row with sel outside the table is
 *     left out.  counts (NULL, or int64[2], written with dW): {rows used, rows left out}.  Non-finite input is NOT masked: it reaches
 *     the entries of its row i or column j.  A matrix no row selects gets zeros.
 *   p lives in the caller's scratch, needed with dW only: nsd_spatial_bwd_scratch_bytes(d) = B * C * C * 8 bytes, 8-byte aligned.
 *   NSD_E_INVALID before any launch: NULL d / v / dy / W; dv and dW both NULL; C outside [1, 32]; T < 1; B < 0; n_mat < 1; dW without a
 *   scratch, or a scratch that is not 8-byte aligned; dv overlapping dy partially.  NSD_E_WORKSPACE: scratch_bytes below the size.
 *   B = 0 launches stage 2 alone (dW is zero).
 *
 * nsd_spatial_fit_step.  One Adam step on A [n_mat][C][C] fp32 from dW, one workgroup per matrix:
 *   g = dW + decay * (A - A0), each operation rounded in fp32 (A0 [n_mat][C][C]: the prior the fit is pulled towards; NULL: g = dW);
 *   then nsd_adam_step's arithmetic in its order with weight_decay 0 and grad_scale 1, at step = the matrix's own counter + 1:
 *     m = b1*m + (1-b1)*g;  v = b2*v + ((1-b2)*g)*g;  A = A - (float)(lr / bc1) * (m / (sqrtf(v) * (float)(1 / sqrt(bc2)) + eps)),
 *     bc = 1 - beta^step in double, the power by repeated squaring (exact products: a host restatement gives the same bits).
 *   State (nsd_spatial_fit_state_bytes(C, n_mat); nsd_spatial_fit_state_layout, offsets in BYTES): per matrix m[C][C], v[C][C] (float),
 *   step, skipped (int64), status (uint32); behind the last matrix one int64 counter of calls.  A reset state is all zero.  The
 *   counters advance on the device: the call can be captured and replayed.
 *   If any g of a matrix is not finite, that matrix, its moments and its step stay bitwise as they were, NSD_SPATIAL_FIT_NONFINITE is
 *   set in its status and its skipped counter advances; the other matrices proceed.
 *   loss_in (NULL, or a device float, what nsd_loss_sum wrote) is copied to loss_out[calls] while calls < loss_cap: the per-epoch losses
 *   need no host read.
 *   NSD_E_INVALID before any launch, naming the field: NULL A / dW / fit / state; C outside [1, 32]; n_mat < 1; lr or decay negative or
 *   not finite; a beta outside [0, 1); eps not positive or not finite; a state that is not 8-byte aligned or smaller than
 *   nsd_spatial_fit_state_bytes(); loss_in without loss_out, or loss_cap < 0.
 */
#define NSD_SPATIAL_FIT_NONFINITE 1u
typedef struct nsd_spatial_fit { float lr, beta1, beta2, eps, decay; } nsd_spatial_fit;
typedef struct nsd_spatial_fit_layout { int64_t m, v, step, skipped, status, stride; } nsd_spatial_fit_layout;   /* bytes in a slot; depends on C only */
int64_t nsd_spatial_bwd_scratch_bytes(const nsd_dims *d);
int     nsd_spatial_bwd(const nsd_dims *d, const float *v, const float *dy, const float *W, int32_t n_mat, const int32_t *sel,
                        float *dv, float *dW, int64_t *counts, void *scratch, int64_t scratch_bytes, void *stream);
int64_t nsd_spatial_fit_state_bytes(int32_t C, int32_t n_mat);
int     nsd_spatial_fit_state_layout(int32_t C, nsd_spatial_fit_layout *out);
int     nsd_spatial_fit_step(int32_t C, int32_t n_mat, float *A, const float *A0, const float *dW, const nsd_spatial_fit *fit,
                             void *state, int64_t state_bytes, const float *loss_in, float *loss_out, int32_t loss_cap, void *stream);

/*
 * ---- rate conversion: stage 0 of the front end (an EXTENSION: the reference's board and every recorded trial run at 125 Hz) ----
 *
 * A causal rational-ratio polyphase FIR resampler in front of nsd_gate_step / nsd_prep_step, so that a stream at any amplifier rate
 * reaches the models at theirs without leaving the device.  out / in rate = L / M with gcd(L, M) = 1, P taps per phase; `taps` is a
 * DEVICE table [L][P], caller-owned, taps[ph*P + i] = h[ph + i*L] of the prototype filter h (never read on the host: non-finite taps
 * give non-finite outputs by the arithmetic).  For one stream, xa[k] = the k-th sample since the slot's reset and xa[k] = 0 for
 * k < 0, c the channel.  Output j:
 *   p = j*M (int64),  ph = p mod L,  q = p div L
 *   acc = +0.0f;  for i = 0 .. P-1 ascending:  acc = acc + taps[ph*P + i] * xa[q - i]      (one rounded product, one rounded sum)
 *   y[j] = acc
 * Every fp32 operation rounds on its own (no FMA contraction).  Output j exists once q <= n_in - 1: a call that adds T samples to a
 * slot holding n_in emits the outputs j in [ceil(n_in*L/M), ceil((n_in+T)*L/M)) -- floor(T*L/M) or ceil(T*L/M) of them, possibly none.
 * Outputs and state are bit for bit a function of the samples alone -- not of the cut, the slot, the other streams of the call, the
 * HIP stream or a graph replay.  A non-finite sample at index n makes exactly the outputs with q in [n, n+P-1] non-finite and nothing
 * after them: unlike the IIR sections the stage heals itself.
 *   nsd_resample_path          1 where nsd_resample_step covers C channels with r (r == NULL: C alone), else 0
 *   nsd_resample_out_steps     ceil((n_in+T)*L/M) - ceil(n_in*L/M); <0 for a refused r, n_in < 0 or T < 0
 *   nsd_resample_state_bytes   bytes of a state of S >= 1 slots (S * stride * 4); <0 for a refused C / r or S < 1
 *   nsd_resample_state_layout  offsets inside a slot in 4-byte words: hist[P-1][C] (fp32, hist[k][c] = xa[n_in - (P-1) + k] -- linear
 *                              and chronological, not a ring, so the state is a function of the samples alone), n_in (int64, 8-byte
 *                              aligned), and the stride.  The layout depends on (C, P); P = 1 has no history.  A slot can be
 *                              checkpointed and restored by copying its stride words.
 *   nsd_resample_reset         as nsd_prep_reset: slots == NULL: all S slots; else the n slots of the DEVICE array slots[n] (indices
 *                              outside [0, S) are skipped).  A reset slot is all zero.
 *   nsd_resample_step          x [B,T,C], y [B,To,C] (of d only B, T, C are read).  y is written completely: row b holds its cnt[b]
 *                              outputs and NaN behind them; cnt: DEVICE int32[B], or NULL.  y must not overlap x.
 *     stream mode (state != NULL): To >= ceil(T*L/M); slots as in nsd_prep_step.  A slot index outside [0, S) is skipped: its row
 *       of y is NaN, its cnt 0 and no state is touched; so is a slot whose n_in lies outside [0, 2^40] (one that was never reset).
 *       No host synchronisation, no allocation: the call can be captured (the counts of a replay are those of the capture only
 *       where M divides T*L -- L/M = 1/2 with even T, say; the kernel itself reads n_in from the slot on every run).
 *     window mode (state == NULL, slots == NULL, S ignored): every trial starts from rest, To == ceil(T*L/M), nothing is stored.
 * NSD_E_INVALID before any launch: NULL d / r / taps / x / y; C outside [1, 64]; T < 1; B < 0; L or M outside [1, 1024]; gcd(L, M)
 * != 1; P outside [1, 256]; L*P > 65536; B > S or S < 1, a state that is not 8-byte aligned (stream mode); slots without a state; To
 * below ceil(T*L/M) (stream mode) or different from it (window mode); T*C or To*64 beyond 2^31 - 1; y overlapping x.  NSD_E_WORKSPACE: state_bytes <
 * nsd_resample_state_bytes(C, r, S).  B = 0 (n = 0) launches nothing.  Additive: NSD_VERSION stays 301, a caller detects the feature
 * by the symbols.
 */
typedef struct nsd_resample { int32_t L, M, P; } nsd_resample;   /* out/in rate = L/M, gcd(L,M)=1; P taps per phase */
typedef struct nsd_resample_layout { int64_t hist, n_in, stride; } nsd_resample_layout;  /* 4-byte words in a slot; depends on (C, P) */
int     nsd_resample_path(int32_t C, const nsd_resample *r);
int64_t nsd_resample_out_steps(const nsd_resample *r, int64_t n_in, int64_t T);
int64_t nsd_resample_state_bytes(int32_t C, const nsd_resample *r, int32_t S);
int     nsd_resample_state_layout(int32_t C, const nsd_resample *r, nsd_resample_layout *out);
int     nsd_resample_reset(int32_t C, const nsd_resample *r, void *state, int64_t state_bytes, int32_t S,
                           const int32_t *slots, int32_t n, void *stream);
int     nsd_resample_step(const nsd_dims *d, const nsd_resample *r, const float *taps, const float *x, const int32_t *slots,
                          void *state, int64_t state_bytes, int32_t S, float *y, int64_t To, int32_t *cnt, void *stream);

/*
 * ---- sequence-batched path for large hidden sizes (BASELINE cfg3: H=256, K=5, B=1024 bf16; cfg5: bidirectional H=512) ----
 *
 * Building block, exported so that it can be tested and timed on its own: C[M,N] = A . B with bf16 operands (device
 * pointers to bf16 bit patterns) and fp32 accumulation on v_mfma_f32_32x32x16_bf16.
 *   a_kmajor == 0: A is [M][lda], k contiguous;  != 0: A is [K][lda], m contiguous
 *   b_kmajor == 0: B is [N][ldb], k contiguous;  != 0: B is [K][ldb], n contiguous; row k is then taken from row
 *                  k + b_shift, rows outside [0, K) read as zero (h_{t-1} for the recurrent weight gradient)
 *   epilogue 0: C fp32 [M][ldc]; splits > 1 writes split z to C + z*M*ldc (the caller sums the parts)
 *            1: C bf16 [M][ldc]
 *            2: C bf16 as 32x32 accumulator tiles [N/32][M/32][64][16] (+ bias[m]): the layout the scan kernels' lanes load
 *            3: the same tiles with the register group first, [N/32][M/32][4][64][4]: element (g, lane, e) is tile row
 *               8 g + 4 (lane >> 5) + e, column lane & 31 (what lane `lane` of wave g of a backward scan owns, 8 contiguous bytes)
 * Contiguous dimensions and leading dimensions must be multiples of 8 elements.
 */
int nsd_gemm_bf16(const void *A, int64_t lda, int32_t a_kmajor, const void *B, int64_t ldb, int32_t b_kmajor, int64_t b_shift,
                  void *C, int64_t ldc, int32_t epilogue, const float *bias, int32_t M, int32_t N, int64_t K, int32_t splits,
                  void *stream);

/*
 * The path itself.  Same model as above -- EEG_LSTM, lstm_eeg_model.py:13-39, with the ctor kwargs of :14 -- for hidden sizes
 * 64, 128, 256, 512 (L <= 8, F, K <= 64), optionally bidirectional (NSD_FLAG_BIDIR; where lstm_eeg_model.py:16-22 would take
 * torch's `bidirectional=True`), computed with bf16 GEMM operands, bf16 saved activations, fp32 accumulation and fp32 cell
 * state / gate arithmetic (BASELINE cfg3 / cfg5 precision; differs from an fp32 run at the 1e-2 level on logits).
 * Per layer: input projection over the whole sequence (one GEMM) -> persistent scan (recurrent weights resident in
 * registers, groups of H/32 workgroups exchanging h_t through the saved sequence) ; backward: persistent scan -> weight /
 * input gradient GEMMs.  x is the same [B,T,C] fp32 tensor as everywhere else; everything in between lives in `workspace`.
 *
 * Flat parameter vector: torch's state_dict order, i.e. per layer the four tensors of the forward direction, then (D = 2)
 * the four `_reverse` tensors; layer l > 0 has input width D*H; ln / attn / fc.0 act on D*H columns.
 *   nsd_seq_param_layout: offsets[4*L*D + 8]
 * Train-mode randomness: counter streams of `rng` as in nsd_lstm_head_train_rng (inter-layer dropout index
 * ((l*B + b)*T + t)*D*H + column, RReLU / head dropout index b*F + f); rng == NULL: no dropout, eval RReLU slope.
 *   nsd_seq_train_fwd   forward + head + mean CE (scale = 1/B_global) + head backward; logits[B,K] written
 *   nsd_seq_train_bwd   BPTT + all parameter gradients -> grads[P] (overwritten), same rng as the forward call
 *   nsd_seq_loss_sum    sum of the per-trial CE losses of the last nsd_seq_train_fwd -> out[0] (device); neither
 *                       nsd_seq_train_fwd_logits nor nsd_seq_head_bwd writes them
 * Two call sequences train or differentiate the model (one workspace, one rng for every call of a sequence):
 *   fused mean CE:  nsd_seq_train_fwd -> nsd_seq_train_bwd[_dx]
 *   any loss:       nsd_seq_train_fwd_logits -> (the caller forms dL/dlogits) -> nsd_seq_head_bwd -> nsd_seq_train_bwd[_dx]
 *   nsd_seq_train_fwd_logits  the training forward of nsd_seq_train_fwd (same scans, same saved activations, same streams) and a
 *                       head that writes logits[B,K] only: no labels, no loss, no head backward.  The logits are nsd_seq_train_fwd's
 *                       bit for bit; time-outs and non-finite values are reported as there.
 *   nsd_seq_head_bwd    dlogits[B,K] (device fp32, the caller's dL/dlogits at any scale) -> the head backward, recomputed from the
 *                       saved top-layer sequence with the same rng: it leaves in the workspace what nsd_seq_train_fwd's fused head
 *                       backward leaves, so nsd_seq_train_bwd[_dx] then returns the gradients of that loss.  Valid after either
 *                       forward; a second call with other dlogits replaces the first.
 *   nsd_seq_train_bwd_dx  nsd_seq_train_bwd (grads bit-identical to it) and, with dx != NULL, dL/dx -> dx[B,T,C] (fp32, the layout of
 *                       x), formed from layer 0's gate gradients and the bf16 W_ih of layer 0 (both directions in one
 *                       contraction, fp32 accumulation).  dx == NULL: exactly nsd_seq_train_bwd.  No extra workspace: the
 *                       nsd_seq_workspace_bytes of the forward covers it.
 * Failure reporting (the persistent scan kernels assume that all workgroups of a scan group are resident at once -- true on an
 * MI355X this process has to itself; a CU mask, another process or a partition mode can break it -- and bound every wait: a group
 * that cannot assemble gives up after ~1-2 s).  A time-out is never silent:
 *   - the workspace starts with a persistent header whose first word is a STICKY status (OR of every time-out code; bit 0 a
 *     forward, bit 1 a backward scan).  nsd_seq_workspace_init zeroes it: call it once after allocating the workspace (an
 *     uninitialised header reads as a failure).  No forward / backward call ever clears it.  The header is all the workspace
 *     needs before first use: the rest may hold arbitrary bytes, before nsd_seq_workspace_init and after it (every ring slot,
 *     rendezvous word and padded row an evaluation reads is set by that evaluation), and a workspace that served another
 *     shape serves the next one without a second nsd_seq_workspace_init.
 *   - logits, probs and the per-trial loss of an evaluation on a workspace that reports a time-out are NaN.
 * Non-finite values (a NaN / Inf window, NaN / Inf or diverged weights) propagate as in the reference's torch.nn.LSTM
 * (lstm_eeg_model.py:34): the logits / probs / loss of the affected trials are NaN, the other trials of the batch are
 * untouched, gradients of a batch with such a trial are NaN.  They are reported as status bit 2 (value 4) of the evaluation
 * -- NOT sticky, no time-out, no waiting -- and nsd_seq_guard raises its flag for that step, so the guarded Adam update
 * does not write NaN into the parameters.
 *   nsd_seq_status      BLOCKING: status_out[4] = {code of the last evaluation OR the sticky word (0 = ok; bits 0 / 1 time-outs,
 *                       bit 2 non-finite activations in the last evaluation), the sticky word alone,
 *                       scan groups (over all scan launches since the last nsd_seq_train_fwd / nsd_seq_infer) whose workgroups
 *                       all reported ONE XCD, groups spread over several}
 *   nsd_seq_guard       enqueued: flag_out[0] (device fp32) = 1 if the workspace reports a time-out or non-finite activations, else 0.  Append it to the
 *                       gradient vector that is all-reduced and hand it to nsd_adam_step_guarded: every rank then skips the
 *                       update when any rank's gradient is garbage.
 */
int64_t nsd_seq_param_count(int32_t C, int32_t H, int32_t L, int32_t K, int32_t F, int32_t D);
int     nsd_seq_param_layout(int32_t C, int32_t H, int32_t L, int32_t K, int32_t F, int32_t D, int64_t *offsets);
int     nsd_seq_supported(const nsd_dims *d, uint32_t flags);
int64_t nsd_seq_workspace_bytes(const nsd_dims *d, uint32_t flags);
int nsd_seq_infer(const nsd_dims *d, const float *params, const float *x, uint32_t flags, float *logits, float *probs,
                  void *workspace, int64_t workspace_bytes, void *stream);
int nsd_seq_train_fwd(const nsd_dims *d, const float *params, const float *x, const nsd_rng *rng, const int32_t *labels,
                      float scale, uint32_t flags, void *workspace, int64_t workspace_bytes, float *logits, void *stream);
/* nsd_seq_train_fwd with targets [B][K] in place of the labels (soft targets, above); its logits are nsd_seq_train_fwd's bit for bit */
int nsd_seq_train_fwd_soft(const nsd_dims *d, const float *params, const float *x, const nsd_rng *rng, const float *targets,
                           float scale, uint32_t flags, void *workspace, int64_t workspace_bytes, float *logits, void *stream);
int nsd_seq_train_bwd(const nsd_dims *d, const float *params, const nsd_rng *rng, uint32_t flags, void *workspace,
                      int64_t workspace_bytes, float *grads, void *stream);
int nsd_seq_train_fwd_logits(const nsd_dims *d, const float *params, const float *x, const nsd_rng *rng, uint32_t flags,
                             void *workspace, int64_t workspace_bytes, float *logits, void *stream);
int nsd_seq_head_bwd(const nsd_dims *d, const float *params, const nsd_rng *rng, const float *dlogits, uint32_t flags,
                     void *workspace, int64_t workspace_bytes, void *stream);
int nsd_seq_train_bwd_dx(const nsd_dims *d, const float *params, const nsd_rng *rng, uint32_t flags, void *workspace,
                         int64_t workspace_bytes, float *grads, float *dx, void *stream);
int nsd_seq_loss_sum(const nsd_dims *d, uint32_t flags, const void *workspace, int64_t workspace_bytes, float *out, void *stream);
int nsd_seq_workspace_init(void *workspace, int64_t workspace_bytes, void *stream);
int nsd_seq_status(const void *workspace, int32_t *status_out, void *stream);
int nsd_seq_guard(const void *workspace, float *flag_out, void *stream);
#ifdef __cplusplus
}
#endif
#endif /* NSD_H */
