// nsd_abi.hip -- extern "C" entry points of libnsd_hip.so (declared in include/nsd.h).
// Argument validation, parameter / workspace layout, kernel dispatch.  No allocation, no synchronisation.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <math.h>
#include "nsd_args.h"
#include "nsd_multi.h"
#include "nsd_bf16.h"

// ---- error text -------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void nsd_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int nsd_num_cus() {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
            cus = prop.multiProcessorCount;
        else
            cus = 256;   // MI355X
    }
    return cus;
}

ParamLayout nsd_make_layout(int C, int H, int L, int K, int F) {
    ParamLayout o;
    memset(&o, 0, sizeof(o));
    int64_t p = 0;
    for (int l = 0; l < L; ++l) {
        const int I = l == 0 ? C : H;
        o.w_ih[l] = p; p += 4LL * H * I;
        o.w_hh[l] = p; p += 4LL * H * H;
        o.b_ih[l] = p; p += 4LL * H;
        o.b_hh[l] = p; p += 4LL * H;
    }
    o.lstm_total = p;
    o.ln_w = p; p += H;   o.ln_b = p; p += H;
    o.attn_w = p; p += H; o.attn_b = p; p += 1;
    o.fc0_w = p; p += (int64_t)F * H; o.fc0_b = p; p += F;
    o.fc3_w = p; p += (int64_t)K * F; o.fc3_b = p; p += K;
    o.total = p;
    return o;
}

static int check_model(int C, int H, int L, int K, int F) {
    if (C < 1 || H < 1 || L < 1 || L > NSD_MAX_LAYERS || K < 1 || F < 1) {
        nsd_set_error("bad model dims C=%d H=%d L=%d K=%d F=%d", C, H, L, K, F);
        return NSD_E_INVALID;
    }
    return NSD_OK;
}
int nsd_check_dims(const nsd_dims *d) {
    if (!d) { nsd_set_error("dims is NULL"); return NSD_E_INVALID; }
    if (d->B < 0 || d->T < 1) { nsd_set_error("bad batch dims B=%d T=%d", d->B, d->T); return NSD_E_INVALID; }
    return check_model(d->C, d->H, d->L, d->K, d->F);
}

static inline int64_t align4(int64_t v) { return (v + 3) & ~(int64_t)3; }

static int fast_path_ok(const nsd_dims *d) {
    // H = 64: the first-generation fused kernels win for small batches, the batched MFMA path from ~400 trials on
    // (measured B=256: 6.9 vs 8.2 ms/step, B=1024: 27.5 vs 13.4 ms/step)
    if (d->H == 64 && d->B >= 384 && nsd_lstm_batched_ok(d, true)) return 0;
    return d->L == 2 && (d->H == 32 || d->H == 48 || d->H == 64) && d->C <= 8;
}

static inline ParamLayout layout_of(const nsd_dims *d) { return nsd_make_layout(d->C, d->H, d->L, d->K, d->F); }
static inline int residual_of(uint32_t flags) { return (flags & NSD_FLAG_RESIDUAL) ? 1 : 0; }

// workspace of M models of d->B trials each: one batch of M*B trials, partitioned by model (nsd_multi.h); M = 1 is one model's workspace
static nsd_ws_layout ws_layout(const nsd_dims *d, int M, bool have_device) {
    nsd_ws_layout w;
    memset(&w, 0, sizeof(w));
    const ParamLayout pl = layout_of(d);
    nsd_dims all = *d;
    all.B = M * d->B;
    const int64_t B = all.B, T = d->T, H = d->H, L = d->L, F = d->F;
    int64_t p = 0;
    w.hseq = p;    p = align4(p + L * B * T * H);
    w.cseq = p;    p = align4(p + L * B * T * H);
    w.gact = p;    p = align4(p + L * B * T * H * 4);
    w.inseq = p;   p = align4(p + (L - 1) * B * T * H);
    w.top = p;     p = align4(p + B * T * H);
    w.alpha = p;   p = align4(p + B * T);
    w.pooled = p;  p = align4(p + B * H);
    w.fc0_pre = p; p = align4(p + B * F);
    w.dscore = p;  p = align4(p + B * T);
    w.dpooled = p; p = align4(p + B * H);
    w.loss = p;    p = align4(p + B);
    w.adpack = p;  p = align4(p + B * T * 4);
    // LSTM slabs: one per backward workgroup (<= #CUs); head slabs: one per trial, stored behind them.
    // Without a device (symbol / layout checks on CPU) assume the MI355X's 256 CUs.
    const bool fast = fast_path_ok(&all) != 0;
    int64_t nsl = B < 256 ? B : 256;
    if (have_device) nsl = nsd_lstm2_bwd_groups((int)B, 1);
    if (nsl < 1 || !fast) nsl = 1;       // generic path: the weight-gradient GEMMs write one slab
    // several models: each writes the slabs of its own G workgroups, so there is room for M * G
    const int64_t own = M > 1 ? (int64_t)M * nsd_lstm2_bwd_groups(d->B > 0 ? d->B : 1, M) : 0;
    if (nsl < own) nsl = own;
    w.n_slabs = nsl;
    w.slabs = p;   p = align4(p + nsl * align4(pl.lstm_total));
    w.hslabs = p;  p = align4(p + B * (pl.total - pl.lstm_total));
    w.da_seq = p;  if (!fast) p = align4(p + L * B * T * 4 * H);      // one per layer: the batched path keeps all layers in flight
    // din: two [B,T,H] ping-pong buffers + the batched path's per-step state [L,3,B,H] and split-K partials [4][4H x max(C,H)]
    w.din = p;     if (!fast) p = align4(p + 2 * B * T * H + L * 3 * B * H + 8 * 4 * H * (H > d->C ? H : (int64_t)d->C));
    w.total = p;
    return w;
}

// Diagnostic build only (make prof -> libnsd_hip_prof.so, or -DNSD_ABLATE_HOOKS=1): the cycle-stamp buffer and the
// NSD_ABLATE timing switches.  The shipped library has neither the symbol nor the getenv.
#if NSD_PROFILE || NSD_ABLATE_HOOKS
static long long *g_dbg = nullptr;
static int ablate_mask() { const char *e = getenv("NSD_ABLATE"); return e ? atoi(e) : 0; }     // (read per launch: tools/kbench.py sweeps it)
extern "C" int nsd_debug_profile_buffer(void *p) { g_dbg = (long long *)p; return NSD_OK; }
#else
static long long *const g_dbg = nullptr;
static int ablate_mask() { return 0; }
#endif

// ---- what an entry point works on once its arguments are accepted -----------------------------------------------------------------
struct Ctx {
    const nsd_dims *d;
    int M;                                   // models in the workspace (1: the single-model entry points)
    ParamLayout pl;
    nsd_ws_layout w;
    float *ws;
    hipStream_t st;
    float *at(int64_t region) const { return ws + region; }
};
constexpr int EMPTY_BATCH = 1;               // accepted, nothing to launch
static int leave(int rc) { return rc == EMPTY_BATCH ? NSD_OK : rc; }

// The workspace binder of every entry point that touches the training workspace of M models (nsd_workspace_bytes() is M = 1): refuses a
// null or short workspace, fills the context, reports the empty batch.  (who: "multi_..." names nsd_multi_workspace_bytes() in the text)
static int bind_ws(Ctx *c, const nsd_dims *d, int M, const void *workspace, int64_t bytes, const char *who, void *stream) {
    if (!workspace) { nsd_set_error("%s: workspace is NULL", who); return NSD_E_INVALID; }
    c->w = ws_layout(d, M, true);
    const int64_t need = c->w.total * (int64_t)sizeof(float);
    if (bytes < need) {
        nsd_set_error("%s: workspace of %lld bytes is smaller than %s() = %lld", who, (long long)bytes,
                      strncmp(who, "multi_", 6) ? "nsd_workspace_bytes" : "nsd_multi_workspace_bytes", (long long)need);
        return NSD_E_WORKSPACE;
    }
    c->d = d; c->M = M; c->pl = layout_of(d); c->ws = (float *)workspace; c->st = (hipStream_t)stream;
    return d->B == 0 ? EMPTY_BATCH : NSD_OK;
}

// The preamble of the single-model fp32 workspace entry points.  Refusals, in this order: dims; ptrs_ok (the entry's null-pointer set, the
// workspace among them); the entry's own refusal (its text, or null); the workspace size; then the empty batch (EMPTY_BATCH: leave(rc)).
static int enter(Ctx *c, const char *who, const nsd_dims *d, bool ptrs_ok, const char *refusal, const void *workspace, int64_t bytes, void *stream) {
    if (nsd_check_dims(d) != NSD_OK) return NSD_E_INVALID;
    if (!ptrs_ok) { nsd_set_error("%s: null pointer", who); return NSD_E_INVALID; }
    if (refusal) { nsd_set_error("%s", refusal); return NSD_E_INVALID; }
    return bind_ws(c, d, 1, workspace, bytes, who, stream);
}

static bool device_present() {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}


extern "C" {

int nsd_version(void) { return NSD_VERSION; }
const char *nsd_last_error(void) { return g_err; }

int64_t nsd_param_count(int32_t C, int32_t H, int32_t L, int32_t K, int32_t F) {
    if (check_model(C, H, L, K, F) != NSD_OK) return NSD_E_INVALID;
    return nsd_make_layout(C, H, L, K, F).total;
}

int nsd_param_layout(int32_t C, int32_t H, int32_t L, int32_t K, int32_t F, int64_t *offsets) {
    if (check_model(C, H, L, K, F) != NSD_OK || !offsets) return NSD_E_INVALID;
    const ParamLayout o = nsd_make_layout(C, H, L, K, F);
    for (int l = 0; l < L; ++l) {
        offsets[4 * l + 0] = o.w_ih[l]; offsets[4 * l + 1] = o.w_hh[l];
        offsets[4 * l + 2] = o.b_ih[l]; offsets[4 * l + 3] = o.b_hh[l];
    }
    int64_t *q = offsets + 4 * L;
    q[0] = o.ln_w; q[1] = o.ln_b; q[2] = o.attn_w; q[3] = o.attn_b;
    q[4] = o.fc0_w; q[5] = o.fc0_b; q[6] = o.fc3_w; q[7] = o.fc3_b;
    return NSD_OK;
}

int64_t nsd_workspace_bytes(const nsd_dims *d, nsd_ws_layout *layout_out) {
    if (nsd_check_dims(d) != NSD_OK) return NSD_E_INVALID;
    const nsd_ws_layout w = ws_layout(d, 1, device_present());
    if (layout_out) *layout_out = w;
    return w.total * (int64_t)sizeof(float);
}

int nsd_fast_path(const nsd_dims *d) {
    if (nsd_check_dims(d) != NSD_OK) return 0;
    return fast_path_ok(d);
}

int nsd_zscore_fwd(const float *x, float *y, int32_t B, int32_t T, int32_t C, void *stream) {
    if (!x || !y || B < 0) { nsd_set_error("zscore: null pointer or B<0"); return NSD_E_INVALID; }
    return nsd_zscore_launch(x, y, B, T, C, (hipStream_t)stream);
}

// ---- shared argument builders -----------------------------------------------------------------------------
// (c: the bound training workspace -- c->M models: the per-layer stride of its saved [L, M*B, T, H] regions -- or null: inference into top_only)
static Lstm2FwdArgs build_lstm_fwd(const nsd_dims *d, const float *params, const float *x, const float *drop_lstm, uint32_t flags,
                                   const Ctx *c, float *top_only) {
    const ParamLayout pl = layout_of(d);
    Lstm2FwdArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x;
    a.w_ih0 = params + pl.w_ih[0]; a.w_hh0 = params + pl.w_hh[0]; a.b_ih0 = params + pl.b_ih[0]; a.b_hh0 = params + pl.b_hh[0];
    a.w_ih1 = params + pl.w_ih[1]; a.w_hh1 = params + pl.w_hh[1]; a.b_ih1 = params + pl.b_ih[1]; a.b_hh1 = params + pl.b_hh[1];
    a.mask = drop_lstm;
    a.dbg = g_dbg;
    a.B = d->B; a.T = d->T; a.C = d->C;
    a.residual = residual_of(flags);
    a.ablate = ablate_mask();
    if (c) {
        const int64_t BTH = (int64_t)c->M * d->B * d->T * d->H;
        a.hseq0 = c->at(c->w.hseq); a.hseq1 = a.hseq0 + BTH;
        a.cseq0 = c->at(c->w.cseq); a.cseq1 = a.cseq0 + BTH;
        a.gact0 = c->at(c->w.gact); a.gact1 = a.gact0 + 4 * BTH;
        a.inseq = c->at(c->w.inseq);
        a.top = c->at(c->w.top);
    } else {
        a.top = top_only;
    }
    return a;
}

// the head's parameters (c == null: inference) and, with them, the head's regions of the bound workspace: the one region -> field map
static HeadArgs build_head(const nsd_dims *d, const float *params, const Ctx *c = nullptr) {
    const ParamLayout pl = layout_of(d);
    HeadArgs h;
    memset(&h, 0, sizeof(h));
    h.ln_w = params + pl.ln_w; h.ln_b = params + pl.ln_b; h.attn_w = params + pl.attn_w; h.attn_b = params + pl.attn_b;
    h.fc0_w = params + pl.fc0_w; h.fc0_b = params + pl.fc0_b; h.fc3_w = params + pl.fc3_w; h.fc3_b = params + pl.fc3_b;
    h.eval_slope = (float)((0.125 + 1.0 / 3.0) / 2.0);   // nn.RReLU eval slope, lstm_eeg_model.py:27
    h.o_ln_w = pl.ln_w - pl.lstm_total; h.o_ln_b = pl.ln_b - pl.lstm_total;
    h.o_attn_w = pl.attn_w - pl.lstm_total; h.o_attn_b = pl.attn_b - pl.lstm_total;
    h.o_fc0_w = pl.fc0_w - pl.lstm_total; h.o_fc0_b = pl.fc0_b - pl.lstm_total;
    h.o_fc3_w = pl.fc3_w - pl.lstm_total; h.o_fc3_b = pl.fc3_b - pl.lstm_total;
    h.Ph = pl.total - pl.lstm_total;
    h.B = d->B; h.T = d->T; h.H = d->H; h.F = d->F; h.K = d->K;
    if (c) {
        h.top = c->at(c->w.top); h.alpha = c->at(c->w.alpha); h.pooled = c->at(c->w.pooled); h.fc0_pre = c->at(c->w.fc0_pre);
        h.loss = c->at(c->w.loss); h.dscore = c->at(c->w.dscore); h.dpooled = c->at(c->w.dpooled);
        h.hslabs = c->at(c->w.hslabs); h.adpack = c->at(c->w.adpack);
    }
    return h;
}

// the head in the tail of the H = 48 forward kernels: its parameters and the RReLU eval slope (inference adds logits_out / probs_out)
static void attach_head(Lstm2FwdArgs *a, const HeadArgs &h) {
    a->attn_w = h.attn_w; a->attn_b = h.attn_b; a->ln_w = h.ln_w; a->ln_b = h.ln_b;
    a->fc0_w = h.fc0_w; a->fc0_b = h.fc0_b; a->fc3_w = h.fc3_w; a->fc3_b = h.fc3_b;
    a->eval_slope = h.eval_slope; a->K = h.K; a->F = h.F;
}
// the fused training head: forward, loss, and the head's backward up to dscore / dpooled and the per-trial head slabs (h: bound to the workspace)
// What a fused head's loss is formed from: int32 labels [B] (mean CE) or, the `_soft` entry points, fp32 target rows [B,K].  One of the two.
struct Target {
    const int32_t *labels;
    const float *targets;
    bool given() const { return labels || targets; }
};
static inline Target hard(const int32_t *labels) { return Target{labels, nullptr}; }
static inline Target soft(const float *targets) { return Target{nullptr, targets}; }

static void attach_head_train(Lstm2FwdArgs *a, const HeadArgs &h, const Target &tg, float scale, float *logits) {
    attach_head(a, h);
    a->head_train = tg.targets ? HEAD_TRAIN_SOFT : 1;
    if (!a->residual) a->top = nullptr;      // top == layer-1 h: the kernel's tail reads hseq1, the saver skips the duplicate
    if (tg.targets) a->targets = tg.targets; else a->labels = tg.labels;
    a->scale = scale;
    a->logits = logits; a->loss = h.loss; a->alpha = h.alpha; a->pooled = h.pooled;
    a->fc0_pre = h.fc0_pre; a->dscore = h.dscore; a->dpooled = h.dpooled;
    a->adpack = h.adpack; a->hslabs = h.hslabs;
    a->o_ln_w = h.o_ln_w; a->o_ln_b = h.o_ln_b; a->o_attn_w = h.o_attn_w; a->o_attn_b = h.o_attn_b;
    a->o_fc0_w = h.o_fc0_w; a->o_fc0_b = h.o_fc0_b; a->o_fc3_w = h.o_fc3_w; a->o_fc3_b = h.o_fc3_b; a->Ph = h.Ph;
}

// (c.M as in build_lstm_fwd; mask, rng and da0_out are the caller's)
static Lstm2BwdArgs build_lstm_bwd(const Ctx &c, const float *params, const float *x, uint32_t flags) {
    const nsd_dims *d = c.d;
    const ParamLayout &pl = c.pl;
    const int64_t BTH = (int64_t)c.M * d->B * d->T * d->H;
    Lstm2BwdArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x;
    a.w_hh0 = params + pl.w_hh[0]; a.w_ih1 = params + pl.w_ih[1]; a.w_hh1 = params + pl.w_hh[1];
    a.attn_w = params + pl.attn_w;
    a.hseq0 = c.at(c.w.hseq); a.hseq1 = a.hseq0 + BTH;
    a.cseq0 = c.at(c.w.cseq); a.cseq1 = a.cseq0 + BTH;
    a.gact0 = c.at(c.w.gact); a.gact1 = a.gact0 + 4 * BTH;
    a.in1seq = c.at(c.w.inseq);
    const HeadArgs h = build_head(d, params, &c);
    a.alpha = h.alpha; a.dscore = h.dscore; a.dpooled = h.dpooled;
    a.dsc_pack = h.adpack;
    a.pooled = h.pooled; a.dscore_out = h.dscore; a.hslabs = h.hslabs;
    a.Ph = h.Ph; a.o_attn_w = h.o_attn_w; a.o_attn_b = h.o_attn_b;
    a.dbg = g_dbg;
    a.slabs = c.at(c.w.slabs);
    a.slab_stride = align4(pl.lstm_total);
    a.o_w_ih0 = pl.w_ih[0]; a.o_w_hh0 = pl.w_hh[0]; a.o_b_ih0 = pl.b_ih[0]; a.o_b_hh0 = pl.b_hh[0];
    a.o_w_ih1 = pl.w_ih[1]; a.o_w_hh1 = pl.w_hh[1]; a.o_b_ih1 = pl.b_ih[1]; a.o_b_hh1 = pl.b_hh[1];
    a.B = d->B; a.T = d->T; a.C = d->C;
    a.residual = residual_of(flags);
    a.ablate = ablate_mask();
    return a;
}

// the layer-by-layer stacks' argument block (StackArgs, nsd_args.h).  c: the bound training workspace, or null: inference in `scratch`
// (nsd_infer_scratch_bytes(): top_out, the [B,T,H] ping-pong buffer, the batched path's cell state)
static StackArgs stack_args(const nsd_dims *d, const float *params, const float *x, const float *drop_lstm, uint32_t flags, const Ctx *c,
                            float *scratch) {
    StackArgs s;
    memset(&s, 0, sizeof(s));
    s.d = *d; s.pl = layout_of(d);
    s.params = params; s.x = x; s.drop_lstm = drop_lstm;
    s.residual = residual_of(flags);
    s.bf16 = (flags & NSD_FLAG_BF16) != 0;
    if (c) {
        const nsd_ws_layout &w = c->w;
        s.hseq = c->at(w.hseq); s.cseq = c->at(w.cseq); s.gact = c->at(w.gact); s.inseq = c->at(w.inseq); s.top_out = c->at(w.top);
        s.alpha = c->at(w.alpha); s.dscore = c->at(w.dscore); s.dpooled = c->at(w.dpooled);
        s.da_seq = c->at(w.da_seq);
        s.din_a = c->at(w.din); s.din_b = s.din_a + s.BTH(); s.state = s.din_b + s.BTH();
        s.slab = c->at(w.slabs);
    } else {
        const int64_t bth = align4(s.BTH());
        s.top_out = scratch; s.scratch2 = scratch + bth; s.cstate = scratch + 2 * bth;
    }
    return s;
}

// the gradient slabs of the bound workspace (per model: the slabs of its backward workgroups, one head slab per trial)
static SlabSet slab_set(const Ctx &c) {
    const int B = c.d->B;
    const int n = B <= 0 ? 0 : c.M > 1 ? nsd_lstm2_bwd_groups(B, c.M) : (int)c.w.n_slabs;
    return SlabSet{c.at(c.w.slabs), align4(c.pl.lstm_total), n, c.pl.lstm_total, c.at(c.w.hslabs), c.pl.total - c.pl.lstm_total, B};
}

#define REQUIRE_FAST(d, name)                                                                              \
    do {                                                                                                   \
        if (!fast_path_ok(d)) {                                                                            \
            nsd_set_error("%s: dims C=%d H=%d L=%d not covered yet (fast path: L==2, H in {32,48,64}, C<=8)", \
                          name, (d)->C, (d)->H, (d)->L);                                                   \
            return NSD_E_INVALID;                                                                          \
        }                                                                                                  \
    } while (0)

static bool fused_train_shape(const nsd_dims *d) {
    return fast_path_ok(d) && d->H == 48 && nsd_lstm2_fwd48_head_train_fits(d->T, d->F, d->K);
}
static int make_rng(const nsd_rng *r, RngArgs *out) {
    if (!r) { nsd_set_error("rng: null pointer"); return NSD_E_INVALID; }
    return nsd_rng_args(r, out);
}

int64_t nsd_infer_scratch_bytes(const nsd_dims *d) {
    if (nsd_check_dims(d) != NSD_OK) return NSD_E_INVALID;
    if (fast_path_ok(d)) return align4((int64_t)d->B * d->T * d->H) * (int64_t)sizeof(float);
    // two [B,T,H] ping-pong buffers + the batched path's cell-state ping-pong [L][2][B,H]
    return (2 * align4((int64_t)d->B * d->T * d->H) + align4(2 * (int64_t)d->L * d->B * d->H)) * (int64_t)sizeof(float);
}

int nsd_infer(const nsd_dims *d, const float *params, const float *x, uint32_t flags, float *logits, float *probs,
              void *scratch, void *stream) {
    if (nsd_check_dims(d) != NSD_OK) return NSD_E_INVALID;
    if (!params || !x || !logits || !scratch) { nsd_set_error("infer: null pointer"); return NSD_E_INVALID; }
    if (d->B == 0) return NSD_OK;
    int rc;
    if (fast_path_ok(d)) {
        Lstm2FwdArgs a = build_lstm_fwd(d, params, x, nullptr, flags, nullptr, (float *)scratch);
        if (d->H == 48 && d->F <= 64 && d->K <= 64) {
            // single launch: attention pooling (online softmax), LayerNorm, dense head and class softmax run in the
            // LSTM kernel's tail wave; nothing but x, the parameters and the [B,K] outputs touches HBM
            attach_head(&a, build_head(d, params));
            a.top = nullptr;
            a.logits_out = logits; a.probs_out = probs;
            return nsd_lstm2_fwd_launch(a, d->H, (hipStream_t)stream);
        }
        rc = nsd_lstm2_fwd_launch(a, d->H, (hipStream_t)stream);
    } else {
        const StackArgs s = stack_args(d, params, x, nullptr, flags, nullptr, (float *)scratch);
        rc = nsd_lstm_batched_ok(d, false) && !s.residual ? nsd_lstm_batched_fwd(s, (hipStream_t)stream) : nsd_lstm_generic_fwd(s, (hipStream_t)stream);
    }
    if (rc != NSD_OK) return rc;
    HeadArgs h = build_head(d, params);
    h.top = (const float *)scratch;
    h.logits = logits; h.probs = probs;
    return nsd_head_launch(h, false, (hipStream_t)stream);
}

int nsd_lstm_fwd(const nsd_dims *d, const float *params, const float *x, const float *drop_lstm, uint32_t flags,
                 float *workspace, int64_t workspace_bytes, void *stream) {
    Ctx c;
    if (const int rc = enter(&c, "lstm_fwd", d, params && x && workspace, nullptr, workspace, workspace_bytes, stream)) return leave(rc);
    if (!fast_path_ok(d)) {
        const StackArgs s = stack_args(d, params, x, drop_lstm, flags, &c, nullptr);
        // large H: per-step batched gate GEMM on the matrix pipe
        return nsd_lstm_batched_ok(d, true) ? nsd_lstm_batched_fwd(s, c.st) : nsd_lstm_generic_fwd(s, c.st);
    }
    return nsd_lstm2_fwd_launch(build_lstm_fwd(d, params, x, drop_lstm, flags, &c, nullptr), d->H, c.st);
}

int nsd_head_fwd(const nsd_dims *d, const float *params, const float *rrelu_slope, const float *drop_head,
                 float *workspace, int64_t workspace_bytes, float *logits, float *probs, void *stream) {
    Ctx c;
    if (const int rc = enter(&c, "head_fwd", d, params && workspace && logits, nullptr, workspace, workspace_bytes, stream)) return leave(rc);
    HeadArgs h = build_head(d, params, &c);
    h.rrelu_slope = rrelu_slope; h.drop_head = drop_head;
    h.logits = logits; h.probs = probs;
    return nsd_head_launch(h, false, c.st);
}

int nsd_head_bwd(const nsd_dims *d, const float *params, const float *rrelu_slope, const float *drop_head,
                 const float *logits, const float *dlogits, const int32_t *labels, float scale, float *workspace,
                 int64_t workspace_bytes, void *stream) {
    Ctx c;
    const char *refusal = (!dlogits && !(labels && logits)) ? "head_bwd: need dlogits, or labels together with logits" : nullptr;
    if (const int rc = enter(&c, "head_bwd", d, params && workspace, refusal, workspace, workspace_bytes, stream)) return leave(rc);
    HeadArgs h = build_head(d, params, &c);
    h.rrelu_slope = rrelu_slope; h.drop_head = drop_head;
    h.logits_in = logits; h.dlogits = dlogits; h.labels = labels; h.scale = scale;
    return nsd_head_launch(h, true, c.st);
}

static int head_train_impl(const char *who, const nsd_dims *d, const float *params, const float *rrelu_slope, const float *drop_head,
                           const Target &tg, float scale, float *workspace, int64_t workspace_bytes, float *logits, void *stream) {
    Ctx c;
    if (const int rc = enter(&c, who, d, params && workspace && logits && tg.given(), nullptr, workspace, workspace_bytes, stream)) return leave(rc);
    HeadArgs h = build_head(d, params, &c);
    h.rrelu_slope = rrelu_slope; h.drop_head = drop_head;
    h.logits = logits; h.logits_in = logits; h.labels = tg.labels; h.targets = tg.targets; h.scale = scale;
    const int rc = nsd_head_train_launch(h, c.st);
    if (rc != 0) return rc < 0 ? rc : NSD_OK;
    // shape does not fit the fused kernel's LDS budget: two passes
    const int rc2 = nsd_head_launch(h, false, c.st);
    if (rc2 != NSD_OK) return rc2;
    return nsd_head_launch(h, true, c.st);
}

int nsd_head_train(const nsd_dims *d, const float *params, const float *rrelu_slope, const float *drop_head,
                   const int32_t *labels, float scale, float *workspace, int64_t workspace_bytes, float *logits, void *stream) {
    return head_train_impl("head_train", d, params, rrelu_slope, drop_head, hard(labels), scale, workspace, workspace_bytes, logits, stream);
}

int nsd_head_train_soft(const nsd_dims *d, const float *params, const float *rrelu_slope, const float *drop_head,
                        const float *targets, float scale, float *workspace, int64_t workspace_bytes, float *logits, void *stream) {
    return head_train_impl("head_train_soft", d, params, rrelu_slope, drop_head, soft(targets), scale, workspace, workspace_bytes, logits, stream);
}

int nsd_rng_path(const nsd_dims *d) {
    if (nsd_check_dims(d) != NSD_OK) return 0;
    return fused_train_shape(d) ? 1 : 0;
}

static int lstm_head_train_impl(const nsd_dims *d, const float *params, const float *x, const float *drop_lstm,
                                const float *rrelu_slope, const float *drop_head, const RngArgs *rng, const Target &tg,
                                float scale, uint32_t flags, float *workspace, int64_t workspace_bytes, float *logits, void *stream) {
    Ctx c;
    const char *who = tg.targets ? "lstm_head_train_soft" : "lstm_head_train";
    if (const int rc = enter(&c, who, d, params && x && workspace && logits && tg.given(), nullptr, workspace, workspace_bytes, stream))
        return leave(rc);
    if (!fused_train_shape(d)) {
        if (rng) { nsd_set_error("%s: shape outside the single-launch path (nsd_rng_path() == 0: H = 48, L = 2, C <= 8, T <= 1024, F <= 64, K <= 8)", tg.targets ? "lstm_head_train_soft with rng" : "lstm_head_train_rng"); return NSD_E_INVALID; }
        // shapes outside the fused kernel: the two launches it replaces
        const int rc = nsd_lstm_fwd(d, params, x, drop_lstm, flags, workspace, workspace_bytes, stream);
        if (rc != NSD_OK) return rc;
        return head_train_impl(tg.targets ? "head_train_soft" : "head_train", d, params, rrelu_slope, drop_head, tg, scale, workspace, workspace_bytes, logits, stream);
    }
    Lstm2FwdArgs a = build_lstm_fwd(d, params, x, drop_lstm, flags, &c, nullptr);
    attach_head_train(&a, build_head(d, params, &c), tg, scale, logits);
    a.rrelu_slope = rrelu_slope; a.drop_head = drop_head;
    if (rng) a.rng = *rng;
    return nsd_lstm2_fwd_launch(a, d->H, c.st);
}

int nsd_lstm_head_train(const nsd_dims *d, const float *params, const float *x, const float *drop_lstm,
                        const float *rrelu_slope, const float *drop_head, const int32_t *labels, float scale, uint32_t flags,
                        float *workspace, int64_t workspace_bytes, float *logits, void *stream) {
    return lstm_head_train_impl(d, params, x, drop_lstm, rrelu_slope, drop_head, nullptr, hard(labels), scale, flags, workspace, workspace_bytes, logits, stream);
}

int nsd_lstm_head_train_rng(const nsd_dims *d, const float *params, const float *x, const nsd_rng *rng, const int32_t *labels,
                            float scale, uint32_t flags, float *workspace, int64_t workspace_bytes, float *logits, void *stream) {
    RngArgs r;
    if (make_rng(rng, &r) != NSD_OK) return NSD_E_INVALID;
    return lstm_head_train_impl(d, params, x, nullptr, nullptr, nullptr, &r, hard(labels), scale, flags, workspace, workspace_bytes, logits, stream);
}

// the soft-target twin of both: explicit mask tensors (rng == NULL) or the in-kernel streams (rng != NULL, no mask tensors)
int nsd_lstm_head_train_soft(const nsd_dims *d, const float *params, const float *x, const float *drop_lstm, const float *rrelu_slope,
                             const float *drop_head, const nsd_rng *rng, const float *targets, float scale, uint32_t flags,
                             float *workspace, int64_t workspace_bytes, float *logits, void *stream) {
    if (!rng) return lstm_head_train_impl(d, params, x, drop_lstm, rrelu_slope, drop_head, nullptr, soft(targets), scale, flags, workspace, workspace_bytes, logits, stream);
    if (drop_lstm || rrelu_slope || drop_head) { nsd_set_error("lstm_head_train_soft: explicit mask tensors or rng, not both"); return NSD_E_INVALID; }
    RngArgs r;
    if (make_rng(rng, &r) != NSD_OK) return NSD_E_INVALID;
    return lstm_head_train_impl(d, params, x, nullptr, nullptr, nullptr, &r, soft(targets), scale, flags, workspace, workspace_bytes, logits, stream);
}

// where nsd_lstm_bwd forms dx: H = 48 on the fast path (the one-trial kernel leaves da0 in place of layer 0's saved gates: ONE backward per
// forward then) and the generic path (its da_seq holds layer 0 last), within the dx kernel's domain (W_ih0 staged in 64 KB of LDS)
static bool dx_shape(const nsd_dims *d) {
    const bool path = (fast_path_ok(d) && d->H == 48) || (!fast_path_ok(d) && !nsd_lstm_batched_ok(d, true));
    return path && nsd_dx_ok(4 * d->H, d->C);
}

int nsd_dx_path(const nsd_dims *d) {
    if (nsd_check_dims(d) != NSD_OK) return 0;
    return dx_shape(d) ? 1 : 0;
}

static int lstm_bwd_impl(const nsd_dims *d, const float *params, const float *x, const float *drop_lstm, const RngArgs *rng,
                         uint32_t flags, float *workspace, int64_t workspace_bytes, float *dx, void *stream) {
    // dx = dL/dx [B,T,C] (optional): refused before any launch where it is not formed (dx_shape, nsd_dx_path)
    const char *refusal = (dx && !nsd_dx_path(d))
        ? "lstm_bwd: dx is available for H = 48 (L = 2, C <= 8) and on the generic path with C <= 64 and 4H * C * 4 <= 64 KB only (nsd_dx_path, include/nsd.h)"
        : nullptr;
    Ctx c;
    if (const int rc = enter(&c, "lstm_bwd", d, params && x && workspace, refusal, workspace, workspace_bytes, stream)) return leave(rc);
    const long rows = (long)d->B * d->T;
    if (!fast_path_ok(d)) {
        const StackArgs s = stack_args(d, params, x, drop_lstm, flags, &c, nullptr);
        if (nsd_lstm_batched_ok(d, true)) return nsd_lstm_batched_bwd(s, c.st);
        if (const int rc = nsd_lstm_generic_bwd(s, c.st)) return rc;
        return dx ? nsd_dx_launch(s.da_seq, s.w_ih(0), dx, rows, 4 * d->H, d->C, c.st) : NSD_OK;
    }
    Lstm2BwdArgs a = build_lstm_bwd(c, params, x, flags);
    a.mask = drop_lstm;
    if (rng) a.rng = *rng;
    if (dx) {
        a.da0_out = c.at(c.w.gact);                                 // (in place of layer 0's saved gates, 4H floats per step: see Lstm2BwdArgs)
        // the one-trial kernel takes a record's dL/dscore_t as finished: close the records a four-trial forward left open
        if (const int rc = nsd_att_close_launch(a.hseq1, a.pooled, a.dpooled, c.at(c.w.adpack), a.dscore_out, a.hslabs, a.Ph,
                                                a.o_attn_w, a.o_attn_b, d->B, d->T, d->H, c.st)) return rc;
    }
    if (const int rc = nsd_lstm2_bwd_launch(a, d->H, c.st)) return rc;
    return dx ? nsd_dx_launch(a.da0_out, params + c.pl.w_ih[0], dx, rows, 4 * d->H, d->C, c.st) : NSD_OK;
}

int nsd_lstm_bwd(const nsd_dims *d, const float *params, const float *x, const float *drop_lstm, uint32_t flags,
                 float *workspace, int64_t workspace_bytes, float *dx, void *stream) {
    return lstm_bwd_impl(d, params, x, drop_lstm, nullptr, flags, workspace, workspace_bytes, dx, stream);
}

int nsd_lstm_bwd_rng(const nsd_dims *d, const float *params, const float *x, const nsd_rng *rng, uint32_t flags,
                     float *workspace, int64_t workspace_bytes, void *stream) {
    RngArgs r;
    if (make_rng(rng, &r) != NSD_OK) return NSD_E_INVALID;
    if (nsd_check_dims(d) != NSD_OK) return NSD_E_INVALID;
    if (!fused_train_shape(d)) { nsd_set_error("lstm_bwd_rng: shape outside the single-launch path (nsd_rng_path() == 0: H = 48, L = 2, C <= 8, T <= 1024, F <= 64, K <= 8)"); return NSD_E_INVALID; }
    return lstm_bwd_impl(d, params, x, nullptr, &r, flags, workspace, workspace_bytes, nullptr, stream);
}

// (the three below launch for an empty batch too: the gradient is zeroed / the parameters decay, the loss sum is 0)
int nsd_grad_reduce(const nsd_dims *d, const float *workspace, int64_t workspace_bytes, float *grads, int32_t accumulate, void *stream) {
    Ctx c;
    if (const int rc = enter(&c, "grad_reduce", d, workspace && grads, nullptr, workspace, workspace_bytes, stream); rc < 0) return rc;
    return nsd_grad_reduce_launch(slab_set(c), 1, grads, accumulate, nullptr, "grad_reduce", c.st);
}

int nsd_grad_reduce_adam(const nsd_dims *d, const float *workspace, int64_t workspace_bytes, float *grads, float *p, float *m, float *v, float lr,
                         float beta1, float beta2, float eps, float weight_decay, float grad_scale, int32_t step, void *stream) {
    Ctx c;
    if (const int rc = enter(&c, "grad_reduce_adam", d, workspace && grads && p && m && v, nullptr, workspace, workspace_bytes, stream); rc < 0) return rc;
    const AdamStep adam{p, m, v, lr, beta1, beta2, eps, weight_decay, grad_scale, step};
    return nsd_grad_reduce_launch(slab_set(c), 1, grads, 0, &adam, "grad_reduce_adam", c.st);
}

int nsd_loss_sum(const nsd_dims *d, const float *workspace, int64_t workspace_bytes, float *out, void *stream) {
    Ctx c;
    if (const int rc = enter(&c, "loss_sum", d, workspace && out, nullptr, workspace, workspace_bytes, stream); rc < 0) return rc;
    return nsd_loss_sum_launch(c.at(c.w.loss), d->B, 1, false, out, "loss_sum", c.st);
}

int nsd_adam_step(int64_t n, float *p, const float *g, float *m, float *v, float lr, float beta1, float beta2,
                  float eps, float weight_decay, float grad_scale, int32_t step, void *stream) {
    if (n < 0 || !p || !g || !m || !v) { nsd_set_error("adam: null pointer or n<0"); return NSD_E_INVALID; }
    return nsd_adam_launch(n, p, g, m, v, lr, beta1, beta2, eps, weight_decay, grad_scale, step, nullptr, (hipStream_t)stream);
}

int nsd_adam_step_guarded(int64_t n, float *p, const float *g, float *m, float *v, float lr, float beta1, float beta2,
                          float eps, float weight_decay, float grad_scale, int32_t step, const float *skip, void *stream) {
    if (n < 0 || !p || !g || !m || !v || !skip) { nsd_set_error("adam_guarded: null pointer or n<0"); return NSD_E_INVALID; }
    return nsd_adam_launch(n, p, g, m, v, lr, beta1, beta2, eps, weight_decay, grad_scale, step, skip, (hipStream_t)stream);
}

// ---- global-norm clipping and learning-rate schedules (nsd_opt, include/nsd.h; nsd_optim.hip) ---------------------------------------
// refusals shared by the launching entry points, before any launch: the fields of opt, the step, then the size of opt_state
static int opt_enter(const char *who, const nsd_opt *o, int32_t step, const int64_t *step_dev, const void *state, int64_t bytes, int64_t n, int M) {
    if (const int rc = nsd_opt_check(o, who)) return rc;
    if (!step_dev && step < 1) { nsd_set_error("%s: step %d must be >= 1 (or pass step_dev)", who, step); return NSD_E_INVALID; }
    if (!state) { nsd_set_error("%s: opt_state is NULL", who); return NSD_E_INVALID; }
    const int64_t need = nsd_opt_state_need(n, M);
    if (bytes < need) {
        nsd_set_error("%s: opt_state of %lld bytes is smaller than nsd_opt_state_bytes() = %lld", who, (long long)bytes, (long long)need);
        return NSD_E_WORKSPACE;
    }
    return NSD_OK;
}

double nsd_lr_factor(const nsd_opt *opt, int64_t step) {
    if (nsd_opt_check(opt, "lr_factor") != NSD_OK) return -1.0;
    if (step < 1) { nsd_set_error("lr_factor: step %lld must be >= 1", (long long)step); return -1.0; }
    return nsd_lr_factor_host(opt, step);
}

int64_t nsd_opt_state_bytes(int64_t n_or_P, int32_t M) {
    if (n_or_P < 0 || M < 1 || M > NSD_MAX_MODELS) { nsd_set_error("opt_state_bytes: n = %lld, M = %d (n >= 0, 1 <= M <= %d)", (long long)n_or_P, M, NSD_MAX_MODELS); return NSD_E_INVALID; }
    return nsd_opt_state_need(n_or_P, M);
}

int nsd_opt_state_init(void *opt_state, int64_t opt_state_bytes, void *stream) {
    if (!opt_state || opt_state_bytes < (int64_t)sizeof(nsd_opt_record)) { nsd_set_error("opt_state_init: opt_state is NULL or shorter than one record"); return NSD_E_INVALID; }
    return nsd_opt_state_init_launch(opt_state, opt_state_bytes, (hipStream_t)stream);
}

int nsd_grad_reduce_clip_adam(const nsd_dims *d, const float *workspace, int64_t workspace_bytes, float *grads, float *p, float *m, float *v,
                              const nsd_opt *opt, int32_t step, const int64_t *step_dev, void *opt_state, int64_t opt_state_bytes, void *stream) {
    static const char *who = "grad_reduce_clip_adam";
    if (nsd_check_dims(d) != NSD_OK) return NSD_E_INVALID;
    if (!workspace || !grads || !p || !m || !v) { nsd_set_error("%s: null pointer", who); return NSD_E_INVALID; }
    if (const int rc = opt_enter(who, opt, step, step_dev, opt_state, opt_state_bytes, layout_of(d).total, 1)) return rc;
    Ctx c;
    if (const int rc = enter(&c, who, d, true, nullptr, workspace, workspace_bytes, stream); rc < 0) return rc;
    return nsd_reduce_clip_adam_launch(slab_set(c), 1, grads, p, m, v, opt, 0, step, (const long long *)step_dev, opt_state, who, c.st);
}

int nsd_grad_norm(int64_t n, const float *g, float grad_scale, void *opt_state, int64_t opt_state_bytes, void *stream) {
    if (n < 0 || !g || !opt_state) { nsd_set_error("grad_norm: null pointer or n<0"); return NSD_E_INVALID; }
    if (opt_state_bytes < nsd_opt_state_need(n, 1)) {
        nsd_set_error("grad_norm: opt_state of %lld bytes is smaller than nsd_opt_state_bytes() = %lld", (long long)opt_state_bytes, (long long)nsd_opt_state_need(n, 1));
        return NSD_E_WORKSPACE;
    }
    return nsd_grad_norm_launch(n, g, grad_scale, opt_state, (hipStream_t)stream);
}

int nsd_adam_step_clip(int64_t n, float *p, const float *g, float *m, float *v, const nsd_opt *opt, int32_t step, const int64_t *step_dev,
                       const float *skip, void *opt_state, int64_t opt_state_bytes, void *stream) {
    static const char *who = "adam_step_clip";
    if (n < 0 || !p || !g || !m || !v) { nsd_set_error("%s: null pointer or n<0", who); return NSD_E_INVALID; }
    if (const int rc = opt_enter(who, opt, step, step_dev, opt_state, opt_state_bytes, n, 1)) return rc;
    return nsd_adam_clip_flat_launch(n, p, g, m, v, opt, step, (const long long *)step_dev, skip, opt_state, (hipStream_t)stream);
}

// ---- weight averaging in the update launch (nsd_avg, include/nsd.h; nsd_optim.hip) ----------------------------------------------------
// refusals of the `_avg` twins, before any launch: the fields of avg (each: M entries, mode 0 allowed, the entry named), then avg_state
static int avg_enter(const char *who, const nsd_avg *avg, int each, const void *state, int64_t bytes, int64_t n, int M) {
    if (!avg) { nsd_set_error("%s: avg is NULL", who); return NSD_E_INVALID; }
    for (int mo = 0; mo < (each ? M : 1); ++mo) {
        char entry[64];
        snprintf(entry, sizeof(entry), "%s: avg[%d]", who, mo);
        if (const int rc = nsd_avg_check(&avg[mo], each ? entry : who, each)) return rc;
    }
    if (!state) { nsd_set_error("%s: avg_state is NULL", who); return NSD_E_INVALID; }
    const int64_t need = nsd_avg_state_need(n, M);
    if (bytes < need) {
        nsd_set_error("%s: avg_state of %lld bytes is smaller than nsd_avg_state_bytes() = %lld", who, (long long)bytes, (long long)need);
        return NSD_E_WORKSPACE;
    }
    return NSD_OK;
}

int64_t nsd_avg_state_bytes(int64_t n_or_P, int32_t M) {
    if (n_or_P < 0 || M < 1 || M > NSD_MAX_MODELS) { nsd_set_error("avg_state_bytes: n = %lld, M = %d (n >= 0, 1 <= M <= %d)", (long long)n_or_P, M, NSD_MAX_MODELS); return NSD_E_INVALID; }
    return nsd_avg_state_need(n_or_P, M);
}

int nsd_avg_state_init(void *avg_state, int64_t avg_state_bytes, int32_t M, void *stream) {
    if (M < 1 || M > NSD_MAX_MODELS) { nsd_set_error("avg_state_init: M = %d (1 <= M <= %d)", M, NSD_MAX_MODELS); return NSD_E_INVALID; }
    if (!avg_state || avg_state_bytes < (int64_t)M * (int64_t)sizeof(nsd_avg_record)) { nsd_set_error("avg_state_init: avg_state is NULL or shorter than %d records", M); return NSD_E_INVALID; }
    return nsd_opt_state_init_launch(avg_state, (int64_t)M * (int64_t)sizeof(nsd_avg_record), (hipStream_t)stream);    // the records only
}

int nsd_grad_reduce_clip_adam_avg(const nsd_dims *d, const float *workspace, int64_t workspace_bytes, float *grads, float *p, float *m, float *v,
                                  const nsd_opt *opt, int32_t step, const int64_t *step_dev, void *opt_state, int64_t opt_state_bytes, void *stream,
                                  const nsd_avg *avg, void *avg_state, int64_t avg_state_bytes) {
    static const char *who = "grad_reduce_clip_adam_avg";
    if (nsd_check_dims(d) != NSD_OK) return NSD_E_INVALID;
    if (!workspace || !grads || !p || !m || !v) { nsd_set_error("%s: null pointer", who); return NSD_E_INVALID; }
    if (const int rc = opt_enter(who, opt, step, step_dev, opt_state, opt_state_bytes, layout_of(d).total, 1)) return rc;
    if (const int rc = avg_enter(who, avg, 0, avg_state, avg_state_bytes, layout_of(d).total, 1)) return rc;
    Ctx c;
    if (const int rc = enter(&c, who, d, true, nullptr, workspace, workspace_bytes, stream); rc < 0) return rc;
    const NsdAvgSpec as{avg, 0, avg_state};
    return nsd_reduce_clip_adam_launch(slab_set(c), 1, grads, p, m, v, opt, 0, step, (const long long *)step_dev, opt_state, who, c.st, &as);
}

int nsd_adam_step_clip_avg(int64_t n, float *p, const float *g, float *m, float *v, const nsd_opt *opt, int32_t step, const int64_t *step_dev,
                           const float *skip, void *opt_state, int64_t opt_state_bytes, void *stream, const nsd_avg *avg, void *avg_state,
                           int64_t avg_state_bytes) {
    static const char *who = "adam_step_clip_avg";
    if (n < 0 || !p || !g || !m || !v) { nsd_set_error("%s: null pointer or n<0", who); return NSD_E_INVALID; }
    if (const int rc = opt_enter(who, opt, step, step_dev, opt_state, opt_state_bytes, n, 1)) return rc;
    if (const int rc = avg_enter(who, avg, 0, avg_state, avg_state_bytes, n, 1)) return rc;
    const NsdAvgSpec as{avg, 0, avg_state};
    return nsd_adam_clip_flat_launch(n, p, g, m, v, opt, step, (const long long *)step_dev, skip, opt_state, (hipStream_t)stream, &as);
}

int nsd_train_masks(uint64_t seed, uint32_t base_stream, float p_lstm, float p_head, int64_t n_lstm, float *drop_lstm,
                    int64_t n_head, float *rrelu_slope, float *drop_head, void *stream) {
    if (n_lstm < 0 || n_head < 0 || (n_lstm > 0 && !drop_lstm) || (n_head > 0 && (!rrelu_slope || !drop_head))) {
        nsd_set_error("train_masks: null pointer or negative size");
        return NSD_E_INVALID;
    }
    return nsd_train_masks_launch(seed, base_stream, nullptr, p_lstm, p_head, n_lstm, drop_lstm, n_head, rrelu_slope, drop_head,
                                  (hipStream_t)stream);
}

int nsd_train_masks_dev(uint64_t seed, const int64_t *step_dev, float p_lstm, float p_head, int64_t n_lstm, float *drop_lstm,
                        int64_t n_head, float *rrelu_slope, float *drop_head, void *stream) {
    if (!step_dev || n_lstm < 0 || n_head < 0 || (n_lstm > 0 && !drop_lstm) || (n_head > 0 && (!rrelu_slope || !drop_head))) {
        nsd_set_error("train_masks_dev: null pointer or negative size");
        return NSD_E_INVALID;
    }
    return nsd_train_masks_launch(seed, 0, (const long long *)step_dev, p_lstm, p_head, n_lstm, drop_lstm, n_head, rrelu_slope,
                                  drop_head, (hipStream_t)stream);
}

int nsd_adam_step_dev(int64_t n, float *p, const float *g, float *m, float *v, float lr, float beta1, float beta2, float eps,
                      float weight_decay, float grad_scale, const int64_t *step_dev, void *stream) {
    if (n < 0 || !p || !g || !m || !v || !step_dev) { nsd_set_error("adam_dev: null pointer or n<0"); return NSD_E_INVALID; }
    return nsd_adam_dev_launch(n, p, g, m, v, lr, beta1, beta2, eps, weight_decay, grad_scale, (const long long *)step_dev,
                               (hipStream_t)stream);
}

int nsd_step_counter_inc(int64_t *step_dev, void *stream) {
    if (!step_dev) { nsd_set_error("step_counter_inc: null pointer"); return NSD_E_INVALID; }
    return nsd_step_inc_launch((long long *)step_dev, (hipStream_t)stream);
}

int nsd_dropout_mask(uint64_t seed, uint32_t stream_id, float p, int64_t n, float *out, void *stream) {
    if (n < 0 || !out) { nsd_set_error("dropout_mask: null pointer or n<0"); return NSD_E_INVALID; }
    return nsd_dropout_mask_launch(seed, stream_id, p, n, out, (hipStream_t)stream);
}

int nsd_rrelu_noise(uint64_t seed, uint32_t stream_id, int64_t n, float *out, void *stream) {
    if (n < 0 || !out) { nsd_set_error("rrelu_noise: null pointer or n<0"); return NSD_E_INVALID; }
    return nsd_rrelu_noise_launch(seed, stream_id, n, out, (hipStream_t)stream);
}

int nsd_gemm_bf16(const void *A, int64_t lda, int32_t a_kmajor, const void *B, int64_t ldb, int32_t b_kmajor, int64_t b_shift,
                  void *C, int64_t ldc, int32_t epilogue, const float *bias, int32_t M, int32_t N, int64_t K, int32_t splits,
                  void *stream) {
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = (const bf16_t *)A; g.B = (const bf16_t *)B; g.lda = lda; g.ldb = ldb; g.a_kmajor = a_kmajor; g.b_kmajor = b_kmajor;
    g.b_shift = b_shift; g.C = C; g.ldc = ldc; g.bias = bias; g.M = M; g.N = N; g.K = K; g.splits = splits; g.epi = epilogue;
    return nsd_gemm_bf16_launch(g, (hipStream_t)stream);
}

// ---- trial augmentation (nsd_augment, include/nsd.h; nsd_augment.hip) --------------------------------------------------------------
static bool augment_shape(const nsd_dims *d) {
    return d && d->B >= 0 && d->T >= 1 && d->C >= 1 && d->C <= 256 && (int64_t)d->T * d->C <= 0x7fffffff;
}
int nsd_augment_path(const nsd_dims *d) { return augment_shape(d) ? 1 : 0; }

// one nsd_aug's fields (who: "augment", or "augment_each: aug[m]")
static int aug_check(const char *who, const nsd_aug *aug, int T) {
    if (aug->max_shift < 0 || aug->max_shift >= T) { nsd_set_error("%s: max_shift %d outside [0, T = %d)", who, aug->max_shift, T); return NSD_E_INVALID; }
    if (!(aug->scale_range >= 0.f && aug->scale_range < 1.f)) { nsd_set_error("%s: scale_range %g outside [0, 1)", who, aug->scale_range); return NSD_E_INVALID; }
    if (!(aug->p_channel >= 0.f && aug->p_channel < 1.f)) { nsd_set_error("%s: p_channel %g outside [0, 1)", who, aug->p_channel); return NSD_E_INVALID; }
    if (!(aug->noise_std >= 0.f && aug->noise_std <= 3.4028234e38f)) { nsd_set_error("%s: noise_std %g negative or not finite", who, aug->noise_std); return NSD_E_INVALID; }
    return NSD_OK;
}

// each: aug points to M entries (nsd_augment_each), else to one for all models
static int augment_impl(const char *who, bool each, const nsd_dims *d, int32_t M, const float *x, int64_t x_model_stride, const nsd_aug *aug,
                        const nsd_rng *rng, const int64_t *step_dev, uint32_t flags, float *y, void *stream) {
    if (!d) { nsd_set_error("%s: dims is NULL", who); return NSD_E_INVALID; }
    if (M < 1 || M > NSD_MAX_MODELS) { nsd_set_error("%s: M = %d models outside [1, %d]", who, M, NSD_MAX_MODELS); return NSD_E_INVALID; }
    if (!x || !y || !aug || !rng) { nsd_set_error("%s: null pointer (x, y, aug, rng)", who); return NSD_E_INVALID; }
    if (!augment_shape(d)) { nsd_set_error("%s: shape B=%d T=%d C=%d outside nsd_augment_path (B >= 0, T >= 1, 1 <= C <= 256)", who, d->B, d->T, d->C); return NSD_E_INVALID; }
    if (flags & ~NSD_AUG_ZSCORE) { nsd_set_error("%s: unknown flag bits 0x%x", who, flags); return NSD_E_INVALID; }
    for (int m = 0; m < (each ? M : 1); ++m) {
        char entry[48];
        if (each) snprintf(entry, sizeof(entry), "%s: aug[%d]", who, m);
        if (const int rc = aug_check(each ? entry : who, &aug[m], d->T)) return rc;
    }
    const int64_t n = (int64_t)d->B * d->T * d->C;
    if (x_model_stride < 0 || (x_model_stride > 0 && x_model_stride < n)) {
        nsd_set_error("%s: x_model_stride %lld: 0 (one window set for all models) or >= B*T*C = %lld", who, (long long)x_model_stride, (long long)n);
        return NSD_E_INVALID;
    }
    if ((int64_t)M * d->B > 0x7fffffff) { nsd_set_error("%s: M * B = %lld trials in one launch", who, (long long)M * d->B); return NSD_E_INVALID; }
    const float *x_end = x + (M - 1) * x_model_stride + n;
    const float *y_end = y + (int64_t)M * n;
    if (n > 0 && x < y_end && y < x_end) { nsd_set_error("%s: y overlaps x (the shift reads other time steps: no in-place form)", who); return NSD_E_INVALID; }
    if (d->B == 0) return NSD_OK;
    AugArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.y = y; a.x_stride = x_model_stride; a.step_dev = (const long long *)step_dev;
    a.B = d->B; a.T = d->T; a.C = d->C; a.M = M;
    a.zscore = (flags & NSD_AUG_ZSCORE) != 0;
    for (int m = 0; m < M; ++m) {
        const nsd_aug *g = each ? &aug[m] : aug;
        AugArgs::Model &am = a.mod[m];
        am.max_shift = g->max_shift;
        am.scale_range = g->scale_range; am.scale_on = g->scale_range != 0.f;
        am.noise_k = (float)((double)g->noise_std / sqrt(21845.0)); am.noise_on = g->noise_std != 0.f;
        am.thr_channel = nsd_drop_threshold(g->p_channel); am.drop_on = g->p_channel != 0.f;
        a.seed[m] = rng[m].seed; a.base[m] = rng[m].base_stream;
    }
    return nsd_augment_launch(a, (hipStream_t)stream);
}

int nsd_augment(const nsd_dims *d, int32_t M, const float *x, int64_t x_model_stride, const nsd_aug *aug, const nsd_rng *rng,
                const int64_t *step_dev, uint32_t flags, float *y, void *stream) {
    return augment_impl("augment", false, d, M, x, x_model_stride, aug, rng, step_dev, flags, y, stream);
}

int nsd_augment_each(const nsd_dims *d, int32_t M, const float *x, int64_t x_model_stride, const nsd_aug *aug, const nsd_rng *rng,
                     const int64_t *step_dev, uint32_t flags, float *y, void *stream) {
    return augment_impl("augment_each", true, d, M, x, x_model_stride, aug, rng, step_dev, flags, y, stream);
}

// ---- soft targets and mixed windows (nsd_mixup, include/nsd.h; nsd_mixup.hip) ------------------------------------------------------
// each: mix points to M entries and class_weight is NULL or [M][K] (nsd_mixup_each), else one nsd_mix and NULL or [K] for all models
static int mixup_impl(const char *who, bool each, const nsd_dims *d, int32_t M, const float *x, int64_t x_model_stride, const int32_t *labels,
                      const float *class_weight, const nsd_mix *mix, const nsd_rng *rng, const int64_t *step_dev, float *y, float *targets,
                      void *stream) {
    if (!d) { nsd_set_error("%s: dims is NULL", who); return NSD_E_INVALID; }
    if (M < 1 || M > NSD_MAX_MODELS) { nsd_set_error("%s: M = %d models outside [1, %d]", who, M, NSD_MAX_MODELS); return NSD_E_INVALID; }
    if (!labels || !targets || !mix || !rng) { nsd_set_error("%s: null pointer (labels, targets, mix, rng)", who); return NSD_E_INVALID; }
    if (d->B < 0 || d->T < 1 || d->C < 1 || (int64_t)d->T * d->C > 0x7fffffff) { nsd_set_error("%s: shape B=%d T=%d C=%d (B >= 0, T >= 1, C >= 1)", who, d->B, d->T, d->C); return NSD_E_INVALID; }
    if (d->K < 1 || d->K > 64) { nsd_set_error("%s: K = %d classes outside [1, 64]", who, d->K); return NSD_E_INVALID; }
    for (int m = 0; m < (each ? M : 1); ++m) {
        char entry[48];
        if (each) snprintf(entry, sizeof(entry), "%s: mix[%d]", who, m);
        const char *w = each ? entry : who;
        if (!(mix[m].smoothing >= 0.f && mix[m].smoothing < 1.f)) { nsd_set_error("%s: smoothing %g outside [0, 1)", w, mix[m].smoothing); return NSD_E_INVALID; }
        if (!(mix[m].mix >= 0.f && mix[m].mix <= 1.f)) { nsd_set_error("%s: mix %g outside [0, 1]", w, mix[m].mix); return NSD_E_INVALID; }
    }
    if ((x == nullptr) != (y == nullptr)) { nsd_set_error("%s: x and y are given together or not at all", who); return NSD_E_INVALID; }
    for (int m = 0; m < (each ? M : 1); ++m)
        if (mix[m].mix > 0.f && !x) {
            if (each) nsd_set_error("%s: mix[%d]: mix = %g needs the windows x and y", who, m, mix[m].mix);
            else nsd_set_error("%s: mix = %g needs the windows x and y", who, mix[m].mix);
            return NSD_E_INVALID;
        }
    const int64_t n = (int64_t)d->B * d->T * d->C;
    if (x_model_stride < 0 || (x_model_stride > 0 && x_model_stride < n)) {
        nsd_set_error("%s: x_model_stride %lld: 0 (one window set for all models) or >= B*T*C = %lld", who, (long long)x_model_stride, (long long)n);
        return NSD_E_INVALID;
    }
    if ((int64_t)M * d->B > 0x7fffffff) { nsd_set_error("%s: M * B = %lld trials in one launch", who, (long long)M * d->B); return NSD_E_INVALID; }
    if (x) {
        const float *x_end = x + (M - 1) * x_model_stride + n;
        const float *y_end = y + (int64_t)M * n;
        if (n > 0 && x < y_end && y < x_end) { nsd_set_error("%s: y overlaps x (a trial reads its partner's window: no in-place form)", who); return NSD_E_INVALID; }
    }
    if (d->B == 0) return NSD_OK;
    MixArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.y = y; a.x_stride = x_model_stride; a.step_dev = (const long long *)step_dev;
    a.labels = labels; a.w = class_weight; a.w_stride = each ? d->K : 0; a.targets = targets;
    a.n_el = (long)d->T * d->C; a.B = d->B; a.K = d->K; a.M = M;
    for (int m = 0; m < M; ++m) {
        const nsd_mix *g = each ? &mix[m] : mix;
        a.mix[m] = g->mix; a.eps[m] = g->smoothing;
        a.seed[m] = rng[m].seed; a.base[m] = rng[m].base_stream;
    }
    return nsd_mixup_launch(a, (hipStream_t)stream);
}

int nsd_mixup(const nsd_dims *d, int32_t M, const float *x, int64_t x_model_stride, const int32_t *labels, const float *class_weight,
              const nsd_mix *mix, const nsd_rng *rng, const int64_t *step_dev, float *y, float *targets, void *stream) {
    return mixup_impl("mixup", false, d, M, x, x_model_stride, labels, class_weight, mix, rng, step_dev, y, targets, stream);
}

int nsd_mixup_each(const nsd_dims *d, int32_t M, const float *x, int64_t x_model_stride, const int32_t *labels, const float *class_weight,
                   const nsd_mix *mix, const nsd_rng *rng, const int64_t *step_dev, float *y, float *targets, void *stream) {
    return mixup_impl("mixup_each", true, d, M, x, x_model_stride, labels, class_weight, mix, rng, step_dev, y, targets, stream);
}

// ---- cropped training (nsd_crop / nsd_crop_pool, include/nsd.h; nsd_crop.hip) -------------------------------------------------------
static bool crop_shape(const nsd_dims *d) {
    return d && d->B >= 0 && d->T >= 1 && d->C >= 1 && (int64_t)d->T * d->C <= 0x7fffffff;
}
static bool crop_cfg_ok(const nsd_dims *d, const nsd_crop_cfg *c) {
    return c && c->window >= 1 && c->window <= d->T && c->crops >= 1 && c->crops <= NSD_CROP_MAX && c->hop >= 0 &&
           (c->hop == 0 || (int64_t)(c->crops - 1) * c->hop + c->window <= d->T);
}
int nsd_crop_path(const nsd_dims *d, const nsd_crop_cfg *c) { return crop_shape(d) && crop_cfg_ok(d, c) ? 1 : 0; }

int nsd_crop(const nsd_dims *d, int32_t M, const float *x, int64_t x_model_stride, const nsd_crop_cfg *c, const nsd_rng *rng,
             const int64_t *step_dev, const int32_t *labels, const float *targets, float *y, int32_t *labels_out, float *targets_out,
             int32_t *offsets_out, void *stream) {
    static const char *who = "crop";
    if (!d) { nsd_set_error("%s: dims is NULL", who); return NSD_E_INVALID; }
    if (M < 1 || M > NSD_MAX_MODELS) { nsd_set_error("%s: M = %d models outside [1, %d]", who, M, NSD_MAX_MODELS); return NSD_E_INVALID; }
    if (!x || !y || !c) { nsd_set_error("%s: null pointer (x, y, c)", who); return NSD_E_INVALID; }
    if (!crop_shape(d)) { nsd_set_error("%s: shape B=%d T=%d C=%d (B >= 0, T >= 1, C >= 1)", who, d->B, d->T, d->C); return NSD_E_INVALID; }
    if (c->window < 1 || c->window > d->T) { nsd_set_error("%s: window %d outside [1, T = %d]", who, c->window, d->T); return NSD_E_INVALID; }
    if (c->crops < 1 || c->crops > NSD_CROP_MAX) { nsd_set_error("%s: crops %d outside [1, %d]", who, c->crops, NSD_CROP_MAX); return NSD_E_INVALID; }
    if (c->hop < 0) { nsd_set_error("%s: hop %d negative (0: drawn offsets)", who, c->hop); return NSD_E_INVALID; }
    if (c->hop > 0 && (int64_t)(c->crops - 1) * c->hop + c->window > d->T) {
        nsd_set_error("%s: the regular grid leaves the trial: (crops - 1) * hop + window = %lld > T = %d", who,
                      (long long)((int64_t)(c->crops - 1) * c->hop + c->window), d->T);
        return NSD_E_INVALID;
    }
    if (c->hop == 0 && !rng) { nsd_set_error("%s: drawn offsets (hop = 0) need rng", who); return NSD_E_INVALID; }
    if (labels_out && !labels) { nsd_set_error("%s: labels_out without labels", who); return NSD_E_INVALID; }
    if (targets_out && !targets) { nsd_set_error("%s: targets_out without targets", who); return NSD_E_INVALID; }
    if (targets_out && d->K < 1) { nsd_set_error("%s: targets with K = %d classes (K >= 1)", who, d->K); return NSD_E_INVALID; }
    const int64_t n = (int64_t)d->B * d->T * d->C;
    if (x_model_stride < 0 || (x_model_stride > 0 && x_model_stride < n)) {
        nsd_set_error("%s: x_model_stride %lld: 0 (one trial set for all models) or >= B*T*C = %lld", who, (long long)x_model_stride, (long long)n);
        return NSD_E_INVALID;
    }
    const int64_t rows = (int64_t)M * d->B * c->crops;
    if (rows > 0x7fffffff) { nsd_set_error("%s: M * B * crops = %lld rows in one launch exceed 2^31 - 1", who, (long long)rows); return NSD_E_INVALID; }
    const float *x_end = x + (M - 1) * x_model_stride + n;
    const float *y_end = y + rows * c->window * d->C;
    if (n > 0 && x < y_end && y < x_end) { nsd_set_error("%s: y overlaps x (a crop is a copy: no in-place form)", who); return NSD_E_INVALID; }
    if (d->B == 0) return NSD_OK;
    CropArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.y = y; a.x_stride = x_model_stride; a.step_dev = (const long long *)step_dev;
    a.labels = labels_out ? labels : nullptr; a.labels_out = labels_out;
    a.targets = targets_out ? targets : nullptr; a.targets_out = targets_out; a.offsets_out = offsets_out;
    a.B = d->B; a.T = d->T; a.C = d->C; a.K = targets_out ? d->K : 0; a.M = M;
    a.W = c->window; a.R = c->crops; a.hop = c->hop;
    if (c->hop == 0)
        for (int m = 0; m < M; ++m) { a.seed[m] = rng[m].seed; a.base[m] = rng[m].base_stream; }
    return nsd_crop_launch(a, (hipStream_t)stream);
}

int nsd_crop_pool(int32_t N, int32_t R, int32_t K, const float *probs, const int32_t *counts, float *probs_out, float *logits_out,
                  void *stream) {
    static const char *who = "crop_pool";
    if (N < 0 || R < 1 || K < 1) { nsd_set_error("%s: N = %d, R = %d, K = %d (N >= 0, R >= 1, K >= 1)", who, N, R, K); return NSD_E_INVALID; }
    if ((int64_t)N * R * K > 2147483647LL) {
        nsd_set_error("%s: N * R * K = %lld probabilities exceed 2^31 - 1", who, (long long)((int64_t)N * R * K)); return NSD_E_INVALID;
    }
    if (!probs || !probs_out) { nsd_set_error("%s: null pointer (probs, probs_out)", who); return NSD_E_INVALID; }
    if (N == 0) return NSD_OK;
    CropPoolArgs a;
    a.probs = probs; a.counts = counts; a.probs_out = probs_out; a.logits_out = logits_out; a.N = N; a.R = R; a.K = K;
    return nsd_crop_pool_launch(a, (hipStream_t)stream);
}

// ---- the step's batch from the resident trials (nsd_gather, include/nsd.h; nsd_gather.hip) -------------------------------------------
static bool gather_shape(const nsd_dims *d, int32_t M, int32_t N, int32_t S) {
    return d && M >= 1 && M <= NSD_MAX_MODELS && N >= 1 && S >= 1 && d->B >= 0 && d->T >= 1 && d->C >= 1 &&
           (int64_t)d->T * d->C <= 0x7fffffff && (int64_t)M * d->B * d->T * d->C <= 0x7fffffff && (int64_t)M * S * d->B <= 0x7fffffff;
}
int nsd_gather_path(const nsd_dims *d, int32_t M, int32_t N, int32_t S) { return gather_shape(d, M, N, S) ? 1 : 0; }

int nsd_gather(const nsd_dims *d, int32_t M, int32_t N, const float *x_all, const int32_t *labels_all, const float *targets_all,
               const int32_t *table, int32_t S, int64_t step, const int64_t *step_dev, int64_t step_base, float *x, int32_t *labels,
               float *targets, int32_t *status, void *stream) {
    static const char *who = "gather";
    if (!d) { nsd_set_error("%s: dims is NULL", who); return NSD_E_INVALID; }
    if (M < 1 || M > NSD_MAX_MODELS) { nsd_set_error("%s: M = %d models outside [1, %d]", who, M, NSD_MAX_MODELS); return NSD_E_INVALID; }
    if (N < 1 || S < 1) { nsd_set_error("%s: N = %d trials, S = %d schedule rows (both >= 1)", who, N, S); return NSD_E_INVALID; }
    if (d->B < 0 || d->T < 1 || d->C < 1 || (int64_t)d->T * d->C > 0x7fffffff) {
        nsd_set_error("%s: shape B=%d T=%d C=%d (B >= 0, T >= 1, C >= 1)", who, d->B, d->T, d->C); return NSD_E_INVALID;
    }
    if (!x_all || !table || !x) { nsd_set_error("%s: null pointer (x_all, table, x)", who); return NSD_E_INVALID; }
    if (labels && !labels_all) { nsd_set_error("%s: labels without labels_all", who); return NSD_E_INVALID; }
    if (targets && !targets_all) { nsd_set_error("%s: targets without targets_all", who); return NSD_E_INVALID; }
    if (targets && d->K < 1) { nsd_set_error("%s: targets with K = %d classes (K >= 1)", who, d->K); return NSD_E_INVALID; }
    const int64_t n_el = (int64_t)d->T * d->C, out = (int64_t)M * d->B * n_el, cells = (int64_t)M * S * d->B;
    if (out > 0x7fffffff) { nsd_set_error("%s: M * B * T * C = %lld floats in one launch exceed 2^31 - 1", who, (long long)out); return NSD_E_INVALID; }
    if (cells > 0x7fffffff) { nsd_set_error("%s: M * S * B = %lld table entries exceed 2^31 - 1", who, (long long)cells); return NSD_E_INVALID; }
    const float *all_end = x_all + (int64_t)N * n_el;
    if (out > 0 && x_all < x + out && x < all_end) { nsd_set_error("%s: x overlaps x_all (a gather is a copy: no in-place form)", who); return NSD_E_INVALID; }
    if (d->B == 0) return NSD_OK;
    GatherArgs a;
    memset(&a, 0, sizeof(a));
    a.x_all = x_all; a.x = x; a.table = table; a.status = status;
    a.labels_all = labels ? labels_all : nullptr; a.labels = labels;
    a.targets_all = targets ? targets_all : nullptr; a.targets = targets;
    a.step_dev = (const long long *)step_dev; a.step = step; a.step_base = step_base;
    a.n_el = (long)n_el; a.B = d->B; a.K = targets ? d->K : 0; a.M = M; a.N = N; a.S = S;
    return nsd_gather_launch(a, (hipStream_t)stream);
}

// ---- model-batched H = 48 path (nsd_multi_*, include/nsd.h; nsd_multi.h) ----------------------------------------------------------
// M = 1 runs the single-model entry points themselves.  M > 1: the kernels' model-batched twins on a workspace of M*B trials.
static bool multi_shape(const nsd_dims *d, int M) {
    return nsd_check_dims(d) == NSD_OK && M >= 1 && M <= NSD_MAX_MODELS && fused_train_shape(d) && (int64_t)M * d->B <= 0x7fffffff;
}
static int multi_check(const nsd_dims *d, int M, const char *who) {
    if (!d) { nsd_set_error("%s: dims is NULL", who); return NSD_E_INVALID; }
    if (M < 1 || M > NSD_MAX_MODELS) { nsd_set_error("%s: M = %d models outside [1, %d]", who, M, NSD_MAX_MODELS); return NSD_E_INVALID; }
    if (!multi_shape(d, M)) {
        nsd_set_error("%s: shape outside the model-batched path (nsd_multi_path: H = 48, L = 2, C <= 8, T <= 1024, F <= 64, K <= 8)", who);
        return NSD_E_INVALID;
    }
    return NSD_OK;
}
// rng: NULL or M entries with one p_lstm / p_head; with NSD_FLAG_MODEL_P each entry has its own.  Either way the kernels read model m's
// thresholds and keep factors from s (nsd_multi.h), formed per entry as nsd_rng_args forms them.
static int multi_rng(const nsd_rng *rng, int M, uint32_t flags, const char *who, RngArgs *r, ModelSplit *s) {
    memset(r, 0, sizeof(*r));
    if (!rng) return NSD_OK;
    for (int m = 0; m < M && !(flags & NSD_FLAG_MODEL_P); ++m)
        if (rng[m].p_lstm != rng[0].p_lstm || rng[m].p_head != rng[0].p_head) {
            nsd_set_error("%s: rng[%d] has p_lstm / p_head %g / %g, rng[0] %g / %g: all models share the probabilities", who, m,
                          rng[m].p_lstm, rng[m].p_head, rng[0].p_lstm, rng[0].p_head);
            return NSD_E_INVALID;
        }
    if (make_rng(&rng[0], r) != NSD_OK) return NSD_E_INVALID;
    s->rng_on = 1;
    for (int m = 0; m < M; ++m) {
        RngArgs rm;
        if (make_rng(&rng[m], &rm) != NSD_OK) { nsd_set_error("%s: rng[%d]: p_lstm / p_head %g / %g out of [0,1)", who, m, rng[m].p_lstm, rng[m].p_head); return NSD_E_INVALID; }
        s->seed[m] = rm.seed; s->base[m] = rm.base;
        s->drop[m].thr_lstm = rm.thr_lstm; s->drop[m].thr_head = rm.thr_head; s->drop[m].keep_lstm = rm.keep_lstm; s->drop[m].keep_head = rm.keep_head;
    }
    return NSD_OK;
}
static int multi_common(const nsd_dims *d, int M, int64_t x_stride, uint32_t flags, const char *who) {
    if (const int rc = multi_check(d, M, who)) return rc;
    if (flags & (NSD_FLAG_RESIDUAL | NSD_FLAG_BIDIR)) { nsd_set_error("%s: flags 0x%x: no residual extension on the model-batched path", who, flags); return NSD_E_INVALID; }
    if (x_stride != 0 && (M > 1 && x_stride < (int64_t)d->B * d->T * d->C)) {
        nsd_set_error("%s: x_model_stride %lld: 0 (one window set for all models) or >= B*T*C = %lld", who, (long long)x_stride,
                      (long long)d->B * d->T * d->C);
        return NSD_E_INVALID;
    }
    return NSD_OK;
}

int nsd_multi_path(const nsd_dims *d, int32_t M) { return multi_shape(d, M) ? 1 : 0; }
int nsd_multi_hyper_path(const nsd_dims *d, int32_t M) { return nsd_multi_path(d, M); }

int64_t nsd_multi_workspace_bytes(const nsd_dims *d, int32_t M, nsd_ws_layout *layout_out) {
    if (multi_check(d, M, "multi_workspace_bytes") != NSD_OK) return NSD_E_INVALID;
    const nsd_ws_layout w = ws_layout(d, M, device_present());
    if (layout_out) *layout_out = w;
    return w.total * (int64_t)sizeof(float);
}

// (the model-batched preamble keeps its own order: multi_common / multi_check, pointers, random streams, then the workspace binder)
static ModelSplit model_split(const nsd_dims *d, int64_t x_model_stride) {
    ModelSplit s;
    memset(&s, 0, sizeof(s));
    s.x_stride = x_model_stride; s.P = layout_of(d).total;
    return s;
}

static int multi_train_fwd_impl(const char *who, const nsd_dims *d, int32_t M, const float *params, const float *x, int64_t x_model_stride,
                                const nsd_rng *rng, const Target &tg, uint32_t flags, float *workspace, int64_t workspace_bytes, float *logits,
                                void *stream) {
    if (const int rc = multi_common(d, M, x_model_stride, flags, who)) return rc;
    if (!params || !x || !tg.given() || !logits) { nsd_set_error("%s: null pointer", who); return NSD_E_INVALID; }
    ModelSplit s = model_split(d, x_model_stride);
    RngArgs r;
    if (multi_rng(rng, M, flags, who, &r, &s) != NSD_OK) return NSD_E_INVALID;
    flags &= ~NSD_FLAG_MODEL_P;
    Ctx c;
    if (const int rc = bind_ws(&c, d, M, workspace, workspace_bytes, who, stream)) return leave(rc);
    const float scale = 1.0f / (float)d->B;                     // mean CE per model
    if (M == 1) return lstm_head_train_impl(d, params, x, nullptr, nullptr, nullptr, rng ? &r : nullptr, tg, scale, flags, workspace,
                                            workspace_bytes, logits, stream);
    Lstm2FwdArgs a = build_lstm_fwd(d, params, x, nullptr, flags, &c, nullptr);
    attach_head_train(&a, build_head(d, params, &c), tg, scale, logits);
    a.rng = r;
    return nsd_lstm2_multi_fwd_launch(a, s, M, c.st);
}

int nsd_multi_train_fwd(const nsd_dims *d, int32_t M, const float *params, const float *x, int64_t x_model_stride, const nsd_rng *rng,
                        const int32_t *labels, uint32_t flags, float *workspace, int64_t workspace_bytes, float *logits, void *stream) {
    return multi_train_fwd_impl("multi_train_fwd", d, M, params, x, x_model_stride, rng, hard(labels), flags, workspace, workspace_bytes, logits, stream);
}

int nsd_multi_train_fwd_soft(const nsd_dims *d, int32_t M, const float *params, const float *x, int64_t x_model_stride, const nsd_rng *rng,
                             const float *targets, uint32_t flags, float *workspace, int64_t workspace_bytes, float *logits, void *stream) {
    return multi_train_fwd_impl("multi_train_fwd_soft", d, M, params, x, x_model_stride, rng, soft(targets), flags, workspace, workspace_bytes, logits, stream);
}

int nsd_multi_train_bwd(const nsd_dims *d, int32_t M, const float *params, const float *x, int64_t x_model_stride, const nsd_rng *rng,
                        uint32_t flags, float *workspace, int64_t workspace_bytes, void *stream) {
    static const char *who = "multi_train_bwd";
    if (const int rc = multi_common(d, M, x_model_stride, flags, who)) return rc;
    if (!params || !x) { nsd_set_error("%s: null pointer", who); return NSD_E_INVALID; }
    ModelSplit s = model_split(d, x_model_stride);
    RngArgs r;
    if (multi_rng(rng, M, flags, who, &r, &s) != NSD_OK) return NSD_E_INVALID;
    flags &= ~NSD_FLAG_MODEL_P;
    Ctx c;
    if (const int rc = bind_ws(&c, d, M, workspace, workspace_bytes, who, stream)) return leave(rc);
    if (M == 1) return lstm_bwd_impl(d, params, x, nullptr, rng ? &r : nullptr, flags, workspace, workspace_bytes, nullptr, stream);
    Lstm2BwdArgs a = build_lstm_bwd(c, params, x, flags);
    a.rng = r;
    return nsd_lstm2_multi_bwd_launch(a, s, M, c.st);
}

// ---- the input gradient of M frozen models (eval-mode noise: the forward ran with rng == NULL) ----
int nsd_multi_dx_path(const nsd_dims *d, int32_t M) { return nsd_multi_path(d, M) && nsd_dx_path(d) ? 1 : 0; }

int nsd_multi_train_bwd_dx(const nsd_dims *d, int32_t M, const float *params, const float *x, int64_t x_model_stride, uint32_t flags,
                           float *workspace, int64_t workspace_bytes, float *dx, int32_t reduce, void *stream) {
    static const char *who = "multi_train_bwd_dx";
    if (const int rc = multi_common(d, M, x_model_stride, flags, who)) return rc;
    if (!params || !x || !workspace || !dx) { nsd_set_error("%s: null pointer (params, x, workspace and dx are required)", who); return NSD_E_INVALID; }
    if (!nsd_multi_dx_path(d, M)) { nsd_set_error("%s: shape outside nsd_multi_dx_path (nsd_multi_path and nsd_dx_path)", who); return NSD_E_INVALID; }
    if (reduce != NSD_DX_PER_MODEL && reduce != NSD_DX_MEAN) {
        nsd_set_error("%s: reduce = %d: NSD_DX_PER_MODEL (0) or NSD_DX_MEAN (1)", who, reduce);
        return NSD_E_INVALID;
    }
    if (reduce == NSD_DX_MEAN && x_model_stride != 0) {
        nsd_set_error("%s: NSD_DX_MEAN with x_model_stride %lld: the mean over the models is that of ONE window set (x_model_stride = 0)", who,
                      (long long)x_model_stride);
        return NSD_E_INVALID;
    }
    // (only the one-trial backward kernel writes da0, and it addresses a model's saved rows with 32-bit offsets)
    if ((int64_t)d->B * d->T * d->H * 4 >= 0x7fffffffLL) {
        nsd_set_error("%s: B * T * H * 4 = %lld bytes per model reach 2 GB: the input gradient needs the one-trial backward kernel", who,
                      (long long)d->B * d->T * d->H * 4);
        return NSD_E_INVALID;
    }
    flags &= ~NSD_FLAG_MODEL_P;
    Ctx c;
    if (const int rc = bind_ws(&c, d, M, workspace, workspace_bytes, who, stream)) return leave(rc);
    if (M == 1) return lstm_bwd_impl(d, params, x, nullptr, nullptr, flags, workspace, workspace_bytes, dx, stream);
    Lstm2BwdArgs a = build_lstm_bwd(c, params, x, flags);
    a.da0_out = c.at(c.w.gact);                                     // (in place of layer 0's saved gates, as nsd_lstm_bwd's: [M*B][T][4H])
    // the fused forward of >= X4_MIN_B trials left the attention records open: close those of all M*B trials (global trial indices)
    if (const int rc = nsd_att_close_launch(a.hseq1, a.pooled, a.dpooled, c.at(c.w.adpack), a.dscore_out, a.hslabs, a.Ph, a.o_attn_w,
                                            a.o_attn_b, M * d->B, d->T, d->H, c.st)) return rc;
    if (const int rc = nsd_lstm2_multi_bwd_launch(a, model_split(d, x_model_stride), M, c.st)) return rc;
    return nsd_multi_dx_launch(a.da0_out, params + c.pl.w_ih[0], c.pl.total, dx, (long)d->B * d->T, M, reduce == NSD_DX_MEAN, 4 * d->H, d->C, c.st);
}

int nsd_multi_loss_mean(const nsd_dims *d, int32_t M, const float *workspace, int64_t workspace_bytes, float *out, void *stream) {
    static const char *who = "multi_loss_mean";
    if (const int rc = multi_check(d, M, who)) return rc;
    if (!out) { nsd_set_error("%s: null pointer", who); return NSD_E_INVALID; }
    Ctx c;
    if (const int rc = bind_ws(&c, d, M, workspace, workspace_bytes, who, stream); rc < 0) return rc;
    return nsd_loss_mean_launch(c.at(c.w.loss), d->B, M, out, who, c.st);
}

// (M = 1 goes through the single-model entry point, as the two above do)
int nsd_multi_grad_reduce(const nsd_dims *d, int32_t M, const float *workspace, int64_t workspace_bytes, float *grads, void *stream) {
    static const char *who = "multi_grad_reduce";
    if (const int rc = multi_check(d, M, who)) return rc;
    if (!grads) { nsd_set_error("%s: null pointer", who); return NSD_E_INVALID; }
    Ctx c;
    if (const int rc = bind_ws(&c, d, M, workspace, workspace_bytes, who, stream); rc < 0) return rc;
    if (M == 1) return nsd_grad_reduce(d, workspace, workspace_bytes, grads, 0, stream);
    return nsd_grad_reduce_launch(slab_set(c), M, grads, 0, nullptr, who, c.st);
}

int nsd_multi_grad_reduce_adam(const nsd_dims *d, int32_t M, const float *workspace, int64_t workspace_bytes, float *grads, float *p,
                               float *m, float *v, float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                               int32_t step, void *stream) {
    static const char *who = "multi_grad_reduce_adam";
    if (const int rc = multi_check(d, M, who)) return rc;
    if (!grads || !p || !m || !v) { nsd_set_error("%s: null pointer", who); return NSD_E_INVALID; }
    Ctx c;
    if (const int rc = bind_ws(&c, d, M, workspace, workspace_bytes, who, stream); rc < 0) return rc;
    if (M == 1) return nsd_grad_reduce_adam(d, workspace, workspace_bytes, grads, p, m, v, lr, beta1, beta2, eps, weight_decay, grad_scale, step, stream);
    const AdamStep adam{p, m, v, lr, beta1, beta2, eps, weight_decay, grad_scale, step};
    return nsd_grad_reduce_launch(slab_set(c), M, grads, 0, &adam, who, c.st);
}

int nsd_multi_grad_reduce_clip_adam(const nsd_dims *d, int32_t M, const float *workspace, int64_t workspace_bytes, float *grads, float *p,
                                    float *m, float *v, const nsd_opt *opt, int32_t step, const int64_t *step_dev, void *opt_state,
                                    int64_t opt_state_bytes, void *stream) {
    static const char *who = "multi_grad_reduce_clip_adam";
    if (const int rc = multi_check(d, M, who)) return rc;
    if (!grads || !p || !m || !v) { nsd_set_error("%s: null pointer", who); return NSD_E_INVALID; }
    if (const int rc = opt_enter(who, opt, step, step_dev, opt_state, opt_state_bytes, layout_of(d).total, M)) return rc;
    Ctx c;
    if (const int rc = bind_ws(&c, d, M, workspace, workspace_bytes, who, stream); rc < 0) return rc;
    if (M == 1) return nsd_grad_reduce_clip_adam(d, workspace, workspace_bytes, grads, p, m, v, opt, step, step_dev, opt_state, opt_state_bytes, stream);
    return nsd_reduce_clip_adam_launch(slab_set(c), M, grads, p, m, v, opt, 0, step, (const long long *)step_dev, opt_state, who, c.st);
}

// opt: M entries, every field per model (M = 1: the single-model entry point with opt[0])
int nsd_multi_grad_reduce_clip_adam_each(const nsd_dims *d, int32_t M, const float *workspace, int64_t workspace_bytes, float *grads,
                                         float *p, float *m, float *v, const nsd_opt *opt, int32_t step, const int64_t *step_dev,
                                         void *opt_state, int64_t opt_state_bytes, void *stream) {
    static const char *who = "multi_grad_reduce_clip_adam_each";
    if (const int rc = multi_check(d, M, who)) return rc;
    if (!grads || !p || !m || !v) { nsd_set_error("%s: null pointer", who); return NSD_E_INVALID; }
    if (!opt) { nsd_set_error("%s: opt is NULL", who); return NSD_E_INVALID; }
    for (int mo = 0; mo < M; ++mo) {
        char entry[64];
        snprintf(entry, sizeof(entry), "%s: opt[%d]", who, mo);
        if (const int rc = nsd_opt_check(&opt[mo], entry)) return rc;
    }
    if (const int rc = opt_enter(who, opt, step, step_dev, opt_state, opt_state_bytes, layout_of(d).total, M)) return rc;
    Ctx c;
    if (const int rc = bind_ws(&c, d, M, workspace, workspace_bytes, who, stream); rc < 0) return rc;
    if (M == 1) return nsd_grad_reduce_clip_adam(d, workspace, workspace_bytes, grads, p, m, v, opt, step, step_dev, opt_state, opt_state_bytes, stream);
    return nsd_reduce_clip_adam_launch(slab_set(c), M, grads, p, m, v, opt, 1, step, (const long long *)step_dev, opt_state, who, c.st);
}

// the `_avg` twins of the two above (each: opt AND avg have M entries; an entry with mode 0 does not average)
static int multi_clip_adam_avg(const char *who, int each, const nsd_dims *d, int32_t M, const float *workspace, int64_t workspace_bytes, float *grads,
                               float *p, float *m, float *v, const nsd_opt *opt, int32_t step, const int64_t *step_dev, void *opt_state,
                               int64_t opt_state_bytes, void *stream, const nsd_avg *avg, void *avg_state, int64_t avg_state_bytes) {
    if (const int rc = multi_check(d, M, who)) return rc;
    if (!grads || !p || !m || !v) { nsd_set_error("%s: null pointer", who); return NSD_E_INVALID; }
    if (!opt) { nsd_set_error("%s: opt is NULL", who); return NSD_E_INVALID; }
    for (int mo = 0; each && mo < M; ++mo) {
        char entry[64];
        snprintf(entry, sizeof(entry), "%s: opt[%d]", who, mo);
        if (const int rc = nsd_opt_check(&opt[mo], entry)) return rc;
    }
    if (const int rc = opt_enter(who, opt, step, step_dev, opt_state, opt_state_bytes, layout_of(d).total, M)) return rc;
    if (const int rc = avg_enter(who, avg, each, avg_state, avg_state_bytes, layout_of(d).total, M)) return rc;
    Ctx c;
    if (const int rc = bind_ws(&c, d, M, workspace, workspace_bytes, who, stream); rc < 0) return rc;
    if (M == 1) {
        if (avg[0].mode == 0) return nsd_grad_reduce_clip_adam(d, workspace, workspace_bytes, grads, p, m, v, opt, step, step_dev, opt_state, opt_state_bytes, stream);
        return nsd_grad_reduce_clip_adam_avg(d, workspace, workspace_bytes, grads, p, m, v, opt, step, step_dev, opt_state, opt_state_bytes, stream, avg,
                                             avg_state, avg_state_bytes);
    }
    const NsdAvgSpec as{avg, each, avg_state};
    return nsd_reduce_clip_adam_launch(slab_set(c), M, grads, p, m, v, opt, each, step, (const long long *)step_dev, opt_state, who, c.st, &as);
}

int nsd_multi_grad_reduce_clip_adam_avg(const nsd_dims *d, int32_t M, const float *workspace, int64_t workspace_bytes, float *grads, float *p,
                                        float *m, float *v, const nsd_opt *opt, int32_t step, const int64_t *step_dev, void *opt_state,
                                        int64_t opt_state_bytes, void *stream, const nsd_avg *avg, void *avg_state, int64_t avg_state_bytes) {
    return multi_clip_adam_avg("multi_grad_reduce_clip_adam_avg", 0, d, M, workspace, workspace_bytes, grads, p, m, v, opt, step, step_dev, opt_state,
                               opt_state_bytes, stream, avg, avg_state, avg_state_bytes);
}

int nsd_multi_grad_reduce_clip_adam_avg_each(const nsd_dims *d, int32_t M, const float *workspace, int64_t workspace_bytes, float *grads,
                                             float *p, float *m, float *v, const nsd_opt *opt, int32_t step, const int64_t *step_dev,
                                             void *opt_state, int64_t opt_state_bytes, void *stream, const nsd_avg *avg, void *avg_state,
                                             int64_t avg_state_bytes) {
    return multi_clip_adam_avg("multi_grad_reduce_clip_adam_avg_each", 1, d, M, workspace, workspace_bytes, grads, p, m, v, opt, step, step_dev,
                               opt_state, opt_state_bytes, stream, avg, avg_state, avg_state_bytes);
}

// ---- sharpness-aware minimisation: the ascent (nsd_sam, include/nsd.h; nsd_optim.hip) -------------------------------------------------
static bool bytes_overlap(const void *a, int64_t na, const void *b, int64_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return na > 0 && nb > 0 && a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}
// refusals shared by the three entry points, before any launch: sam's fields (each: M entries, the entry named), the two state buffers,
// then the rows of sam_state against p and grads
static int sam_enter(const char *who, const nsd_sam *sam, int each, const void *p, const void *grads, const void *opt_state, int64_t opt_bytes,
                     const void *sam_state, int64_t sam_bytes, int64_t n, int M) {
    if (!sam) { nsd_set_error("%s: sam is NULL", who); return NSD_E_INVALID; }
    for (int mo = 0; mo < (each ? M : 1); ++mo) {
        char entry[64];
        snprintf(entry, sizeof(entry), "%s: sam[%d]", who, mo);
        if (const int rc = nsd_sam_check(&sam[mo], each ? entry : who)) return rc;
    }
    if (!opt_state || !sam_state) { nsd_set_error("%s: opt_state or sam_state is NULL", who); return NSD_E_INVALID; }
    if (opt_bytes < nsd_opt_state_need(n, M)) {
        nsd_set_error("%s: opt_state of %lld bytes is smaller than nsd_opt_state_bytes() = %lld", who, (long long)opt_bytes, (long long)nsd_opt_state_need(n, M));
        return NSD_E_WORKSPACE;
    }
    if (sam_bytes < nsd_sam_state_need(n, M)) {
        nsd_set_error("%s: sam_state of %lld bytes is smaller than nsd_sam_state_bytes() = %lld", who, (long long)sam_bytes, (long long)nsd_sam_state_need(n, M));
        return NSD_E_WORKSPACE;
    }
    const int64_t row_bytes = (int64_t)M * n * (int64_t)sizeof(float);
    const char *rows = static_cast<const char *>(sam_state) + (size_t)M * sizeof(nsd_sam_record);
    if (bytes_overlap(rows, row_bytes, p, row_bytes) || bytes_overlap(rows, row_bytes, grads, row_bytes)) {
        nsd_set_error("%s: the rows of sam_state overlap p or grads", who);
        return NSD_E_INVALID;
    }
    return NSD_OK;
}

int64_t nsd_sam_state_bytes(int64_t n_or_P, int32_t M) {
    if (n_or_P < 0 || M < 1 || M > NSD_MAX_MODELS) { nsd_set_error("sam_state_bytes: n = %lld, M = %d (n >= 0, 1 <= M <= %d)", (long long)n_or_P, M, NSD_MAX_MODELS); return NSD_E_INVALID; }
    return nsd_sam_state_need(n_or_P, M);
}

int nsd_sam_state_init(void *sam_state, int64_t sam_state_bytes, void *stream) {
    if (!sam_state || sam_state_bytes < (int64_t)sizeof(nsd_sam_record)) { nsd_set_error("sam_state_init: sam_state is NULL or shorter than one record"); return NSD_E_INVALID; }
    return nsd_opt_state_init_launch(sam_state, sam_state_bytes, (hipStream_t)stream);
}

int nsd_sam_ascend(const nsd_dims *d, const float *workspace, int64_t workspace_bytes, float *grads, const float *p, const nsd_sam *sam,
                   float grad_scale, void *opt_state, int64_t opt_state_bytes, void *sam_state, int64_t sam_state_bytes, void *stream) {
    static const char *who = "sam_ascend";
    if (nsd_check_dims(d) != NSD_OK) return NSD_E_INVALID;
    if (!workspace || !grads || !p) { nsd_set_error("%s: null pointer", who); return NSD_E_INVALID; }
    if (const int rc = sam_enter(who, sam, 0, p, grads, opt_state, opt_state_bytes, sam_state, sam_state_bytes, layout_of(d).total, 1)) return rc;
    Ctx c;
    if (const int rc = enter(&c, who, d, true, nullptr, workspace, workspace_bytes, stream); rc < 0) return rc;
    return nsd_sam_ascend_slabs_launch(slab_set(c), 1, grads, p, &sam->rho, &grad_scale, opt_state, sam_state, who, c.st);
}

int nsd_multi_sam_ascend(const nsd_dims *d, int32_t M, const float *workspace, int64_t workspace_bytes, float *grads, const float *p,
                         const nsd_sam *sam, int32_t each, const float *grad_scale, void *opt_state, int64_t opt_state_bytes, void *sam_state,
                         int64_t sam_state_bytes, void *stream) {
    static const char *who = "multi_sam_ascend";
    if (const int rc = multi_check(d, M, who)) return rc;
    if (!grads || !p || !grad_scale) { nsd_set_error("%s: null pointer", who); return NSD_E_INVALID; }
    if (const int rc = sam_enter(who, sam, each, p, grads, opt_state, opt_state_bytes, sam_state, sam_state_bytes, layout_of(d).total, M)) return rc;
    Ctx c;
    if (const int rc = bind_ws(&c, d, M, workspace, workspace_bytes, who, stream); rc < 0) return rc;
    if (M == 1) return nsd_sam_ascend(d, workspace, workspace_bytes, grads, p, sam, grad_scale[0], opt_state, opt_state_bytes, sam_state, sam_state_bytes, stream);
    float rho[NSD_MAX_MODELS], gs[NSD_MAX_MODELS];
    for (int mo = 0; mo < M; ++mo) { rho[mo] = sam[each ? mo : 0].rho; gs[mo] = grad_scale[each ? mo : 0]; }
    return nsd_sam_ascend_slabs_launch(slab_set(c), M, grads, p, rho, gs, opt_state, sam_state, who, c.st);
}

int nsd_sam_ascend_flat(int64_t n, const float *p, const float *g, const nsd_sam *sam, float grad_scale, void *opt_state, int64_t opt_state_bytes,
                        void *sam_state, int64_t sam_state_bytes, void *stream) {
    static const char *who = "sam_ascend_flat";
    if (n < 0 || !p || !g) { nsd_set_error("%s: null pointer or n<0", who); return NSD_E_INVALID; }
    if (const int rc = sam_enter(who, sam, 0, p, g, opt_state, opt_state_bytes, sam_state, sam_state_bytes, n, 1)) return rc;
    return nsd_sam_ascend_flat_launch(n, p, g, sam->rho, grad_scale, opt_state, sam_state, (hipStream_t)stream);
}

int nsd_multi_loss_sum(const nsd_dims *d, int32_t M,const float *workspace, int64_t workspace_bytes, float *out, void *stream) {
    static const char *who = "multi_loss_sum";
    if (const int rc = multi_check(d, M, who)) return rc;
    if (!out) { nsd_set_error("%s: null pointer", who); return NSD_E_INVALID; }
    Ctx c;
    if (const int rc = bind_ws(&c, d, M, workspace, workspace_bytes, who, stream); rc < 0) return rc;
    return nsd_loss_sum_launch(c.at(c.w.loss), d->B, M, true, out, who, c.st);
}

int64_t nsd_multi_infer_scratch_bytes(const nsd_dims *d, int32_t M) {
    if (multi_check(d, M, "multi_infer_scratch_bytes") != NSD_OK) return NSD_E_INVALID;
    return 0;                                                    // the fused inference tail keeps nothing outside the chip
}

int nsd_multi_infer(const nsd_dims *d, int32_t M, const float *params, const float *x, int64_t x_model_stride, uint32_t flags,
                    float *logits, float *probs, void *scratch, void *stream) {
    static const char *who = "multi_infer";
    (void)scratch;
    if (const int rc = multi_common(d, M, x_model_stride, flags, who)) return rc;
    if (!params || !x || !logits) { nsd_set_error("%s: null pointer", who); return NSD_E_INVALID; }
    if (d->B == 0) return NSD_OK;
    Lstm2FwdArgs a = build_lstm_fwd(d, params, x, nullptr, 0, nullptr, nullptr);
    attach_head(&a, build_head(d, params));
    a.logits_out = logits; a.probs_out = probs;
    return nsd_lstm2_multi_fwd_launch(a, model_split(d, x_model_stride), M, (hipStream_t)stream);
}

// ---- resumable H = 48 inference (nsd_stream48.hip) ----
// the model dims alone: B and T are the call's (streams advanced, chunk length), not the state's
static bool stream_shape(const nsd_dims *d) {
    return d && check_model(d->C, d->H, d->L, d->K, d->F) == NSD_OK && d->H == 48 && d->L == 2 && d->C <= 8 && d->F <= 64 && d->K <= 64;
}
// the preamble of the entry points that touch a stream state: shape, pointers, slot count, size
static int stream_enter(const nsd_dims *d, const char *who, bool ptrs_ok, const void *state, int64_t state_bytes, int32_t S, int32_t M = 1) {
    if (!stream_shape(d)) {
        nsd_set_error("%s: shape outside the resumable path (nsd_stream_path: H = 48, L = 2, C <= 8, F <= 64, K <= 64)", who);
        return NSD_E_INVALID;
    }
    if (!ptrs_ok || !state) { nsd_set_error("%s: null pointer", who); return NSD_E_INVALID; }
    if (S < 1) { nsd_set_error("%s: S = %d slots", who, S); return NSD_E_INVALID; }
    const int64_t need = (int64_t)M * S * STREAM_STRIDE * (int64_t)sizeof(float);
    if (state_bytes < need) {
        nsd_set_error("%s: state of %lld bytes is smaller than nsd_%sstream_state_bytes() = %lld", who, (long long)state_bytes,
                      M > 1 ? "multi_" : "", (long long)need);
        return NSD_E_WORKSPACE;
    }
    return NSD_OK;
}

int nsd_stream_path(const nsd_dims *d) { return stream_shape(d) ? 1 : 0; }

int64_t nsd_stream_state_bytes(const nsd_dims *d, int32_t S) {
    if (!stream_shape(d) || S < 1) { nsd_set_error("stream_state_bytes: shape outside nsd_stream_path, or S < 1"); return NSD_E_INVALID; }
    return (int64_t)S * STREAM_STRIDE * (int64_t)sizeof(float);
}

int nsd_stream_state_layout(const nsd_dims *d, nsd_stream_layout *out) {
    if (!stream_shape(d) || !out) { nsd_set_error("stream_state_layout: shape outside nsd_stream_path, or null pointer"); return NSD_E_INVALID; }
    memset(out, 0, sizeof(*out));
    out->h[0] = STREAM_H0; out->h[1] = STREAM_H1; out->c[0] = STREAM_C0; out->c[1] = STREAM_C1;
    out->pool_max = STREAM_MAX; out->pool_den = STREAM_DEN; out->pool_acc = STREAM_ACC;
    out->steps = STREAM_STEPS; out->stride = STREAM_STRIDE;
    return NSD_OK;
}

int nsd_stream_reset(const nsd_dims *d, void *state, int64_t state_bytes, int32_t S, const int32_t *slots, int32_t n, void *stream) {
    static const char *who = "stream_reset";
    if (const int rc = stream_enter(d, who, true, state, state_bytes, S)) return rc;
    if (slots && (n < 0 || n > S)) { nsd_set_error("%s: n = %d slots of S = %d", who, n, S); return NSD_E_INVALID; }
    const int count = slots ? n : S;
    if (count == 0) return NSD_OK;
    return nsd_stream_reset_launch((float *)state, S, slots, count, (hipStream_t)stream);
}

// the step's argument block: one model's parameters, state and outputs (the model-batched launch moves them per model)
static StreamArgs build_stream(const nsd_dims *d, const float *params, const float *x, const int32_t *slots, uint32_t flags, void *state,
                               int32_t S, float *logits, float *probs) {
    const HeadArgs h = build_head(d, params);
    const ParamLayout pl = layout_of(d);
    StreamArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x;
    a.w_ih0 = params + pl.w_ih[0]; a.w_hh0 = params + pl.w_hh[0]; a.b_ih0 = params + pl.b_ih[0]; a.b_hh0 = params + pl.b_hh[0];
    a.w_ih1 = params + pl.w_ih[1]; a.w_hh1 = params + pl.w_hh[1]; a.b_ih1 = params + pl.b_ih[1]; a.b_hh1 = params + pl.b_hh[1];
    a.attn_w = h.attn_w; a.attn_b = h.attn_b; a.ln_w = h.ln_w; a.ln_b = h.ln_b;
    a.fc0_w = h.fc0_w; a.fc0_b = h.fc0_b; a.fc3_w = h.fc3_w; a.fc3_b = h.fc3_b;
    a.eval_slope = h.eval_slope;
    a.slots = slots; a.state = (float *)state; a.logits = logits; a.probs = probs;
    a.B = d->B; a.T = d->T; a.C = d->C; a.K = d->K; a.F = d->F; a.S = S; a.residual = residual_of(flags);
    return a;
}

int nsd_stream_step(const nsd_dims *d, const float *params, const float *x, const int32_t *slots, uint32_t flags, void *state,
                    int64_t state_bytes, int32_t S, float *logits, float *probs, void *stream) {
    static const char *who = "stream_step";
    if (nsd_check_dims(d) != NSD_OK) return NSD_E_INVALID;
    if (const int rc = stream_enter(d, who, params && x, state, state_bytes, S)) return rc;
    if (probs && !logits) { nsd_set_error("%s: probs without logits", who); return NSD_E_INVALID; }
    if (flags & ~NSD_FLAG_RESIDUAL) { nsd_set_error("%s: flags 0x%x (only NSD_FLAG_RESIDUAL applies)", who, flags); return NSD_E_INVALID; }
    if (d->B > S) { nsd_set_error("%s: B = %d streams, S = %d slots", who, d->B, S); return NSD_E_INVALID; }
    if (d->B == 0) return NSD_OK;
    return nsd_stream48_launch(build_stream(d, params, x, slots, flags, state, S, logits, probs), (hipStream_t)stream);
}

// ---- resumable inference of M models per launch (nsd_multi_stream48.hip): state [M][S][STREAM_STRIDE] ----
int nsd_multi_stream_path(const nsd_dims *d, int32_t M) { return stream_shape(d) && M >= 1 && M <= NSD_MAX_MODELS ? 1 : 0; }

int64_t nsd_multi_stream_state_bytes(const nsd_dims *d, int32_t M, int32_t S) {
    if (!nsd_multi_stream_path(d, M) || S < 1) {
        nsd_set_error("multi_stream_state_bytes: shape outside nsd_stream_path, M = %d outside [1, %d], or S < 1", M, NSD_MAX_MODELS);
        return NSD_E_INVALID;
    }
    return (int64_t)M * S * STREAM_STRIDE * (int64_t)sizeof(float);
}

int nsd_multi_stream_step(const nsd_dims *d, int32_t M, const float *params, const float *x, int64_t x_model_stride, const int32_t *slots,
                          uint32_t flags, void *state, int64_t state_bytes, int32_t S, float *logits, float *probs, float *mean_probs,
                          void *stream) {
    static const char *who = "multi_stream_step";
    if (nsd_check_dims(d) != NSD_OK) return NSD_E_INVALID;
    if (M < 1 || M > NSD_MAX_MODELS) { nsd_set_error("%s: M = %d models outside [1, %d]", who, M, NSD_MAX_MODELS); return NSD_E_INVALID; }
    if (const int rc = stream_enter(d, who, params && x, state, state_bytes, S, M)) return rc;
    if (probs && !logits) { nsd_set_error("%s: probs without logits", who); return NSD_E_INVALID; }
    if (mean_probs && !probs) { nsd_set_error("%s: mean_probs without probs", who); return NSD_E_INVALID; }
    if (flags & ~NSD_FLAG_RESIDUAL) { nsd_set_error("%s: flags 0x%x (only NSD_FLAG_RESIDUAL applies)", who, flags); return NSD_E_INVALID; }
    if (d->B > S) { nsd_set_error("%s: B = %d streams, S = %d slots", who, d->B, S); return NSD_E_INVALID; }
    const int64_t n = (int64_t)d->B * d->T * d->C;
    if (x_model_stride < 0 || (x_model_stride > 0 && x_model_stride < n)) {
        nsd_set_error("%s: x_model_stride %lld: 0 (one chunk for all models) or >= B*T*C = %lld", who, (long long)x_model_stride, (long long)n);
        return NSD_E_INVALID;
    }
    if ((int64_t)M * d->B * d->K > 0x7fffffff) { nsd_set_error("%s: M * B * K = %lld output values in one launch", who, (long long)M * d->B * d->K); return NSD_E_INVALID; }
    if (d->B == 0) return NSD_OK;
    const StreamArgs a = build_stream(d, params, x, slots, flags, state, S, logits, probs);
    return nsd_multi_stream48_launch(a, model_split(d, x_model_stride), M, mean_probs, (hipStream_t)stream);
}

// ---- session calibration (nsd_head_fit.hip): the pooled vector of stream slots, and the read-out refitted on such vectors ----
int nsd_stream_features(const nsd_dims *d, const void *state, int64_t state_bytes, int32_t S, const int32_t *slots, int32_t n, float *feats,
                        void *stream) {
    static const char *who = "stream_features";
    if (const int rc = stream_enter(d, who, feats != nullptr, state, state_bytes, S)) return rc;
    if (n < 0 || (!slots && n > S)) { nsd_set_error("%s: n = %d rows of S = %d slots", who, n, S); return NSD_E_INVALID; }
    if (n == 0) return NSD_OK;
    return nsd_stream_features_launch((const float *)state, S, slots, n, feats, (hipStream_t)stream);
}

// the model dims, the model count, the trial count d->B and the LDS one workgroup needs for them
static bool fit_shape(const nsd_dims *d, int32_t M) {
    return stream_shape(d) && M >= 1 && M <= NSD_MAX_MODELS && d->B >= 1 && d->B <= NSD_FIT_MAX_TRIALS &&
           fit_lds_floats(d->B, d->F, d->K) * (long)sizeof(float) <= FIT_LDS_MAX;
}
int nsd_head_fit_path(const nsd_dims *d, int32_t M) { return fit_shape(d, M) ? 1 : 0; }

int64_t nsd_head_fit_state_bytes(const nsd_dims *d, int32_t M) {
    if (!stream_shape(d) || M < 1 || M > NSD_MAX_MODELS) {
        nsd_set_error("head_fit_state_bytes: shape outside nsd_stream_path, or M = %d outside [1, %d]", M, NSD_MAX_MODELS);
        return NSD_E_INVALID;
    }
    return (int64_t)M * fit_stride(d->F, d->K) * (int64_t)sizeof(float);
}

int nsd_head_fit_state_layout(const nsd_dims *d, nsd_fit_layout *out) {
    if (!stream_shape(d) || !out) { nsd_set_error("head_fit_state_layout: shape outside nsd_stream_path, or null pointer"); return NSD_E_INVALID; }
    out->m = 0; out->v = fit_tail(d->F, d->K); out->epochs = fit_epochs_off(d->F, d->K); out->status = fit_status_off(d->F, d->K);
    out->stride = fit_stride(d->F, d->K);
    return NSD_OK;
}

int nsd_head_fit(const nsd_dims *d, int32_t M, float *params, const float *feats, int64_t feats_model_stride, const float *targets,
                 const nsd_fit *fit, const nsd_rng *rng, void *fit_state, int64_t fit_state_bytes, float *loss_out, void *stream) {
    static const char *who = "head_fit";
    if (!d || !params || !feats || !targets || !fit || !fit_state) { nsd_set_error("%s: null pointer", who); return NSD_E_INVALID; }
    if (!fit_shape(d, M)) {
        nsd_set_error("%s: outside nsd_head_fit_path (nsd_stream_path, 1 <= M <= %d, 1 <= N <= %d, %ld bytes of LDS for N, F, K): "
                      "M = %d, N = %d, H = %d, F = %d, K = %d", who, NSD_MAX_MODELS, NSD_FIT_MAX_TRIALS, FIT_LDS_MAX, M, d->B, d->H, d->F, d->K);
        return NSD_E_INVALID;
    }
    if (fit->epochs < 1 || fit->epochs > NSD_FIT_MAX_EPOCHS) { nsd_set_error("%s: epochs %d outside [1, %d]", who, fit->epochs, NSD_FIT_MAX_EPOCHS); return NSD_E_INVALID; }
    if (fit->train == 0 || (fit->train & ~(NSD_FIT_LN | NSD_FIT_FC0 | NSD_FIT_FC3))) {
        nsd_set_error("%s: train mask 0x%x (a non-empty subset of NSD_FIT_LN | NSD_FIT_FC0 | NSD_FIT_FC3)", who, fit->train); return NSD_E_INVALID;
    }
    if (!(fit->lr >= 0.f && fit->lr < INFINITY) || !(fit->beta1 >= 0.f && fit->beta1 < 1.f) || !(fit->beta2 >= 0.f && fit->beta2 < 1.f) ||
        !(fit->eps > 0.f && fit->eps < INFINITY) || !(fit->weight_decay >= 0.f && fit->weight_decay < INFINITY) || !(fit->scale == fit->scale) ||
        fit->scale == INFINITY || fit->scale == -INFINITY) {
        nsd_set_error("%s: lr %g (finite, >= 0), betas %g %g (in [0, 1)), eps %g (finite, > 0), weight_decay %g (finite, >= 0), scale %g (finite)",
                      who, fit->lr, fit->beta1, fit->beta2, fit->eps, fit->weight_decay, fit->scale);
        return NSD_E_INVALID;
    }
    const int64_t nh = (int64_t)d->B * d->H;
    if (feats_model_stride < 0 || (feats_model_stride > 0 && feats_model_stride < nh)) {
        nsd_set_error("%s: feats_model_stride %lld: 0 (one set for all models) or >= N*H = %lld", who, (long long)feats_model_stride, (long long)nh);
        return NSD_E_INVALID;
    }
    FitArgs a;
    memset(&a, 0, sizeof(a));
    for (int m = 0; rng && m < M; ++m) {
        if (!(rng[m].p_head >= 0.f && rng[m].p_head < 1.f)) { nsd_set_error("%s: rng[%d].p_head %g outside [0, 1)", who, m, rng[m].p_head); return NSD_E_INVALID; }
        a.seed[m] = rng[m].seed; a.base[m] = rng[m].base_stream;
        a.thr[m] = nsd_drop_threshold(rng[m].p_head); a.keep[m] = 1.0f / (1.0f - rng[m].p_head);
    }
    const int64_t need = (int64_t)M * fit_stride(d->F, d->K) * (int64_t)sizeof(float);
    if (fit_state_bytes < need) {
        nsd_set_error("%s: state of %lld bytes is smaller than nsd_head_fit_state_bytes() = %lld", who, (long long)fit_state_bytes, (long long)need);
        return NSD_E_WORKSPACE;
    }
    const ParamLayout pl = layout_of(d);
    a.params = params; a.P = pl.total;
    a.o_ln_w = pl.ln_w; a.o_ln_b = pl.ln_b; a.o_fc0_w = pl.fc0_w; a.o_fc0_b = pl.fc0_b; a.o_fc3_w = pl.fc3_w; a.o_fc3_b = pl.fc3_b;
    a.feats = feats; a.feats_stride = feats_model_stride; a.targets = targets; a.state = (float *)fit_state; a.loss_out = loss_out;
    a.N = d->B; a.F = d->F; a.K = d->K; a.epochs = fit->epochs; a.train = fit->train;
    a.lr = fit->lr; a.b1 = fit->beta1; a.b2 = fit->beta2; a.eps = fit->eps; a.wd = fit->weight_decay; a.scale = fit->scale;
    a.eval_slope = build_head(d, params).eval_slope;
    a.rng_on = rng ? 1 : 0;
    return nsd_head_fit_launch(a, M, (hipStream_t)stream);
}

// ---- early stopping for model batches (nsd_eval.hip): metrics, the best-evaluation decision and the snapshot of M models ----
// the shape of a call: 0, or the refusal with the field named
static int eval_shape(const char *who, int32_t M, int32_t B, int32_t K) {
    if (M < 1 || M > NSD_MAX_MODELS) { nsd_set_error("%s: M = %d outside [1, %d]", who, M, NSD_MAX_MODELS); return NSD_E_INVALID; }
    if (K < 1 || K > NSD_EVAL_MAX_K) { nsd_set_error("%s: K = %d outside [1, %d]", who, K, NSD_EVAL_MAX_K); return NSD_E_INVALID; }
    if (B < 1) { nsd_set_error("%s: B = %d must be >= 1", who, B); return NSD_E_INVALID; }
    if ((int64_t)M * B * K > 2147483647LL) {
        nsd_set_error("%s: M * B * K = %lld logits exceed 2^31 - 1", who, (long long)((int64_t)M * B * K)); return NSD_E_INVALID;
    }
    return NSD_OK;
}
int nsd_multi_eval_path(int32_t M, int32_t B, int32_t K, int64_t P) {
    return M >= 1 && M <= NSD_MAX_MODELS && K >= 1 && K <= NSD_EVAL_MAX_K && B >= 1 && (int64_t)M * B * K <= 2147483647LL && P >= 0 ? 1 : 0;
}

int64_t nsd_select_state_bytes(int32_t M, int64_t P) {
    if (M < 1 || M > NSD_MAX_MODELS || P < 1) {
        nsd_set_error("select_state_bytes: M = %d, P = %lld (1 <= M <= %d, P >= 1)", M, (long long)P, NSD_MAX_MODELS); return NSD_E_INVALID;
    }
    return (int64_t)eval_records_bytes(M) + (int64_t)M * P * (int64_t)sizeof(float);
}

int nsd_select_state_init(void *sel_state, int64_t sel_state_bytes, int32_t M, int64_t P, void *stream) {
    static const char *who = "select_state_init";
    if (!sel_state) { nsd_set_error("%s: sel_state is NULL", who); return NSD_E_INVALID; }
    const int64_t need = nsd_select_state_bytes(M, P);
    if (need < 0) return NSD_E_INVALID;
    if (sel_state_bytes < need) {
        nsd_set_error("%s: sel_state of %lld bytes is smaller than nsd_select_state_bytes() = %lld", who, (long long)sel_state_bytes, (long long)need);
        return NSD_E_WORKSPACE;
    }
    return nsd_opt_state_init_launch(sel_state, eval_records_bytes(M), (hipStream_t)stream);      // the records; the snapshot rows stay
}

int nsd_multi_eval(int32_t M, int32_t B, int32_t K, const float *logits, const int32_t *labels, const int32_t *counts, nsd_eval_record *out,
                   const nsd_select *sel, const float *params, int64_t P, void *sel_state, int64_t sel_state_bytes, void *stream) {
    static const char *who = "multi_eval";
    if (const int rc = eval_shape(who, M, B, K)) return rc;
    if (!logits) { nsd_set_error("%s: logits is NULL", who); return NSD_E_INVALID; }
    if (!labels) { nsd_set_error("%s: labels is NULL", who); return NSD_E_INVALID; }
    if (!out) { nsd_set_error("%s: out is NULL", who); return NSD_E_INVALID; }
    EvalArgs a;
    memset(&a, 0, sizeof(a));
    for (int m = 0; m < M; ++m) {
        a.counts[m] = counts ? counts[m] : B;
        if (a.counts[m] < 1 || a.counts[m] > B) { nsd_set_error("%s: counts[%d] = %d outside [1, B = %d]", who, m, a.counts[m], B); return NSD_E_INVALID; }
    }
    if (sel) {
        if (sel->metric != NSD_SELECT_LOSS && sel->metric != NSD_SELECT_ACC) {
            nsd_set_error("%s: sel->metric %d unknown (NSD_SELECT_LOSS / NSD_SELECT_ACC)", who, sel->metric); return NSD_E_INVALID;
        }
        if (sel->patience < 0) { nsd_set_error("%s: sel->patience %d negative", who, sel->patience); return NSD_E_INVALID; }
        if (!(sel->min_delta >= 0.f)) { nsd_set_error("%s: sel->min_delta %g negative or NaN", who, sel->min_delta); return NSD_E_INVALID; }
        if (!params) { nsd_set_error("%s: sel without params", who); return NSD_E_INVALID; }
        if (!sel_state) { nsd_set_error("%s: sel without sel_state", who); return NSD_E_INVALID; }
        if (P < 1) { nsd_set_error("%s: sel with P = %lld (P >= 1)", who, (long long)P); return NSD_E_INVALID; }
        const int64_t need = nsd_select_state_bytes(M, P);
        if (sel_state_bytes < need) {
            nsd_set_error("%s: sel_state of %lld bytes is smaller than nsd_select_state_bytes() = %lld", who, (long long)sel_state_bytes, (long long)need);
            return NSD_E_WORKSPACE;
        }
        a.select = 1; a.metric = sel->metric; a.patience = sel->patience; a.min_delta = sel->min_delta;
        a.params = params; a.P = P;
        a.recs = static_cast<nsd_select_record *>(sel_state);
        a.best = reinterpret_cast<float *>(static_cast<char *>(sel_state) + eval_records_bytes(M));
    }
    a.logits = logits; a.labels = labels; a.out = out; a.B = B; a.K = K;
    return nsd_multi_eval_launch(a, M, (hipStream_t)stream);
}

// ---- sliding-window decisions (nsd_window48.hip): state [S][R phase slots + header] ----
static bool window_ok(const nsd_window *w) {
    return w && w->window >= 1 && w->hop >= 1 && w->hop <= w->window && w->window % w->hop == 0 && w->window / w->hop <= NSD_WINDOW_MAX_PHASES;
}
// the preamble of the entry points that touch a window state: shape, pointers, stream count, size
static int window_enter(const nsd_dims *d, const nsd_window *w, const char *who, bool ptrs_ok, const void *state, int64_t state_bytes, int32_t S,
                        int32_t M = 1) {
    if (!d || !w) { nsd_set_error("%s: null pointer", who); return NSD_E_INVALID; }
    if (!stream_shape(d) || !window_ok(w)) {
        nsd_set_error("%s: outside nsd_window_path (nsd_stream_path, 1 <= hop <= window, window %% hop == 0, window / hop <= %d): window %d, hop %d",
                      who, NSD_WINDOW_MAX_PHASES, w->window, w->hop);
        return NSD_E_INVALID;
    }
    if (!ptrs_ok || !state) { nsd_set_error("%s: null pointer", who); return NSD_E_INVALID; }
    if (S < 1) { nsd_set_error("%s: S = %d streams", who, S); return NSD_E_INVALID; }
    const int64_t need = (int64_t)M * S * window_stream_stride(w->window / w->hop) * (int64_t)sizeof(float);
    if (state_bytes < need) {
        nsd_set_error("%s: state of %lld bytes is smaller than nsd_%swindow_state_bytes() = %lld", who, (long long)state_bytes,
                      M > 1 ? "multi_" : "", (long long)need);
        return NSD_E_WORKSPACE;
    }
    return NSD_OK;
}

int nsd_window_path(const nsd_dims *d, const nsd_window *w) { return stream_shape(d) && window_ok(w) ? 1 : 0; }

int32_t nsd_window_rows(int32_t T, const nsd_window *w) {
    if (T < 1 || !window_ok(w)) { nsd_set_error("window_rows: T = %d, or an invalid window / hop", T); return NSD_E_INVALID; }
    return (int32_t)(((int64_t)T + w->hop - 1) / w->hop);
}

int64_t nsd_window_state_bytes(const nsd_dims *d, const nsd_window *w, int32_t S) {
    if (!nsd_window_path(d, w) || S < 1) { nsd_set_error("window_state_bytes: outside nsd_window_path, or S < 1"); return NSD_E_INVALID; }
    return (int64_t)S * window_stream_stride(w->window / w->hop) * (int64_t)sizeof(float);
}

int nsd_window_state_layout(const nsd_dims *d, const nsd_window *w, nsd_window_layout *out) {
    if (!nsd_window_path(d, w) || !out) { nsd_set_error("window_state_layout: outside nsd_window_path, or null pointer"); return NSD_E_INVALID; }
    const int R = w->window / w->hop;
    memset(out, 0, sizeof(*out));
    out->phases = R; out->phase_stride = STREAM_STRIDE;
    out->window = (int64_t)R * STREAM_STRIDE + WINDOW_HDR_W; out->hop = (int64_t)R * STREAM_STRIDE + WINDOW_HDR_HOP;
    out->count = (int64_t)R * STREAM_STRIDE + WINDOW_HDR_COUNT;
    out->stream_stride = window_stream_stride(R);
    return NSD_OK;
}

int nsd_window_reset(const nsd_dims *d, const nsd_window *w, void *state, int64_t state_bytes, int32_t S, const int32_t *slots, int32_t n,
                     void *stream) {
    static const char *who = "window_reset";
    if (const int rc = window_enter(d, w, who, true, state, state_bytes, S)) return rc;
    if (slots && (n < 0 || n > S)) { nsd_set_error("%s: n = %d streams of S = %d", who, n, S); return NSD_E_INVALID; }
    const int count = slots ? n : S;
    if (count == 0) return NSD_OK;
    return nsd_window_reset_launch((float *)state, S, slots, count, w->window, w->hop, (hipStream_t)stream);
}

int nsd_window_step(const nsd_dims *d, const nsd_window *w, const float *params, const float *x, const int32_t *slots, uint32_t flags,
                    void *state, int64_t state_bytes, int32_t S, float *logits, float *probs, int64_t *ends, int32_t *counts, void *stream) {
    static const char *who = "window_step";
    if (!d || !w) { nsd_set_error("%s: null pointer", who); return NSD_E_INVALID; }
    if (nsd_check_dims(d) != NSD_OK) return NSD_E_INVALID;
    if (const int rc = window_enter(d, w, who, params && x && logits && ends && counts, state, state_bytes, S)) return rc;
    if (flags & ~NSD_FLAG_RESIDUAL) { nsd_set_error("%s: flags 0x%x (only NSD_FLAG_RESIDUAL applies)", who, flags); return NSD_E_INVALID; }
    if (d->T < 1) { nsd_set_error("%s: chunk length T = %d", who, d->T); return NSD_E_INVALID; }
    if (d->B > S) { nsd_set_error("%s: B = %d streams, S = %d", who, d->B, S); return NSD_E_INVALID; }
    const int R = w->window / w->hop, D = nsd_window_rows(d->T, w);
    if ((int64_t)d->B * D * d->K > 0x7fffffff || (int64_t)d->B * R > 0x7fffffff) {
        nsd_set_error("%s: B * D * K = %lld output values (B * R = %lld workgroup passes) in one launch", who, (long long)d->B * D * d->K, (long long)d->B * R);
        return NSD_E_INVALID;
    }
    if (d->B == 0) return NSD_OK;
    WindowArgs a;
    memset(&a, 0, sizeof(a));
    static_cast<StreamArgs &>(a) = build_stream(d, params, x, slots, flags, state, S, logits, probs);
    a.ends = (long long *)ends; a.counts = counts;
    a.W = w->window; a.Hp = w->hop; a.R = R; a.D = D;
    return nsd_window48_launch(a, (hipStream_t)stream);
}

// ---- sliding-window decisions of M models per launch (nsd_multi_window48.hip): state [M][S][R phase slots + header] ----
int nsd_multi_window_path(const nsd_dims *d, const nsd_window *w, int32_t M) {
    return nsd_window_path(d, w) && M >= 1 && M <= NSD_MAX_MODELS ? 1 : 0;
}

int64_t nsd_multi_window_state_bytes(const nsd_dims *d, const nsd_window *w, int32_t M, int32_t S) {
    if (!nsd_multi_window_path(d, w, M) || S < 1) {
        nsd_set_error("multi_window_state_bytes: outside nsd_window_path, M = %d outside [1, %d], or S < 1", M, NSD_MAX_MODELS);
        return NSD_E_INVALID;
    }
    return (int64_t)M * S * window_stream_stride(w->window / w->hop) * (int64_t)sizeof(float);
}

int nsd_multi_window_step(const nsd_dims *d, const nsd_window *w, int32_t M, const float *params, const float *x, int64_t x_model_stride,
                          const int32_t *slots, uint32_t flags, void *state, int64_t state_bytes, int32_t S, float *logits, float *probs,
                          float *mean_probs, int64_t *ends, int32_t *counts, void *stream) {
    static const char *who = "multi_window_step";
    if (!d || !w) { nsd_set_error("%s: null pointer", who); return NSD_E_INVALID; }
    if (nsd_check_dims(d) != NSD_OK) return NSD_E_INVALID;
    if (M < 1 || M > NSD_MAX_MODELS) { nsd_set_error("%s: M = %d models outside [1, %d]", who, M, NSD_MAX_MODELS); return NSD_E_INVALID; }
    if (const int rc = window_enter(d, w, who, params && x && logits && ends && counts, state, state_bytes, S, M)) return rc;
    if (mean_probs && !probs) { nsd_set_error("%s: mean_probs without probs", who); return NSD_E_INVALID; }
    if (flags & ~NSD_FLAG_RESIDUAL) { nsd_set_error("%s: flags 0x%x (only NSD_FLAG_RESIDUAL applies)", who, flags); return NSD_E_INVALID; }
    if (d->T < 1) { nsd_set_error("%s: chunk length T = %d", who, d->T); return NSD_E_INVALID; }
    if (d->B > S) { nsd_set_error("%s: B = %d streams, S = %d", who, d->B, S); return NSD_E_INVALID; }
    const int64_t n = (int64_t)d->B * d->T * d->C;
    if (x_model_stride < 0 || (x_model_stride > 0 && x_model_stride < n)) {
        nsd_set_error("%s: x_model_stride %lld: 0 (one chunk for all models) or >= B*T*C = %lld", who, (long long)x_model_stride, (long long)n);
        return NSD_E_INVALID;
    }
    const int R = w->window / w->hop, D = nsd_window_rows(d->T, w);
    if ((int64_t)M * d->B * D * d->K > 0x7fffffff || (int64_t)d->B * R > 0x7fffffff) {
        nsd_set_error("%s: M * B * D * K = %lld output values (B * R = %lld workgroup passes per model) in one launch", who,
                      (long long)M * d->B * D * d->K, (long long)d->B * R);
        return NSD_E_INVALID;
    }
    if (d->B == 0) return NSD_OK;
    WindowArgs a;
    memset(&a, 0, sizeof(a));
    static_cast<StreamArgs &>(a) = build_stream(d, params, x, slots, flags, state, S, logits, probs);
    a.ends = (long long *)ends; a.counts = counts;
    a.W = w->window; a.Hp = w->hop; a.R = R; a.D = D;
    return nsd_multi_window48_launch(a, model_split(d, x_model_stride), M, mean_probs, (hipStream_t)stream);
}

// ---- causal front end (nsd_prep_*, include/nsd.h; nsd_prep.hip) ----
static bool prep_channels(int32_t C) { return C >= 1 && C <= 64; }
static bool prep_finite(float v) { return v - v == 0.f; }
// the configuration alone: flags, sections, z-score (who == NULL: a silent query)
static bool prep_config(const nsd_prep *p, const char *who) {
#define PREP_REFUSE(...) do { if (who) nsd_set_error(__VA_ARGS__); return false; } while (0)
    if (p->flags & ~(NSD_PREP_BASELINE | NSD_PREP_CAR)) PREP_REFUSE("%s: unknown flag bits 0x%x", who, p->flags);
    if (p->n_sections < 0 || p->n_sections > NSD_PREP_MAX_SECTIONS) PREP_REFUSE("%s: n_sections = %d outside [0, %d]", who, p->n_sections, NSD_PREP_MAX_SECTIONS);
    for (int s = 0; s < p->n_sections; ++s) {
        for (int k = 0; k < 5; ++k)
            if (!prep_finite(p->sos[s][k])) PREP_REFUSE("%s: section %d: coefficient %d is not finite", who, s, k);
        const double a1 = p->sos[s][3], a2 = p->sos[s][4];
        if (!(fabs(a2) < 1.0 && fabs(a1) < 1.0 + a2)) PREP_REFUSE("%s: section %d is unstable (a1 = %g, a2 = %g: stable means |a2| < 1 and |a1| < 1 + a2)", who, s, a1, a2);
    }
    if (!(p->alpha >= 0.f && p->alpha < 1.f)) PREP_REFUSE("%s: alpha %g outside [0, 1)", who, p->alpha);
    if (!prep_finite(p->var0) || (p->alpha > 0.f && !(p->var0 > 0.f))) PREP_REFUSE("%s: var0 %g (finite, and > 0 with the running z-score)", who, p->var0);
#undef PREP_REFUSE
    return true;
}
// the preamble of the entry points that touch a prep state: channels, slot count, size
static int prep_enter(int32_t C, const char *who, const void *state, int64_t state_bytes, int32_t S) {
    if (!prep_channels(C)) { nsd_set_error("%s: C = %d channels outside [1, 64]", who, C); return NSD_E_INVALID; }
    if (!state) { nsd_set_error("%s: null state", who); return NSD_E_INVALID; }
    if (S < 1) { nsd_set_error("%s: S = %d slots", who, S); return NSD_E_INVALID; }
    const int64_t need = (int64_t)S * prep_stride(C) * (int64_t)sizeof(float);
    if (state_bytes < need) {
        nsd_set_error("%s: state of %lld bytes is smaller than nsd_prep_state_bytes() = %lld", who, (long long)state_bytes, (long long)need);
        return NSD_E_WORKSPACE;
    }
    return NSD_OK;
}

int nsd_prep_path(int32_t C, const nsd_prep *p) { return prep_channels(C) && (!p || prep_config(p, nullptr)) ? 1 : 0; }

int64_t nsd_prep_state_bytes(int32_t C, int32_t S) {
    if (!prep_channels(C) || S < 1) { nsd_set_error("prep_state_bytes: C outside [1, 64], or S < 1"); return NSD_E_INVALID; }
    return (int64_t)S * prep_stride(C) * (int64_t)sizeof(float);
}

int nsd_prep_state_layout(int32_t C, nsd_prep_layout *out) {
    if (!prep_channels(C) || !out) { nsd_set_error("prep_state_layout: C outside [1, 64], or null pointer"); return NSD_E_INVALID; }
    out->x0 = PREP_X0; out->z = prep_z(C, 0, 0); out->mu = prep_mu(C); out->var = prep_var(C);
    out->steps = prep_steps(C); out->stride = prep_stride(C);
    return NSD_OK;
}

int nsd_prep_reset(int32_t C, void *state, int64_t state_bytes, int32_t S, const int32_t *slots, int32_t n, void *stream) {
    static const char *who = "prep_reset";
    if (const int rc = prep_enter(C, who, state, state_bytes, S)) return rc;
    if (slots && (n < 0 || n > S)) { nsd_set_error("%s: n = %d slots of S = %d", who, n, S); return NSD_E_INVALID; }
    const int count = slots ? n : S;
    if (count == 0) return NSD_OK;
    return nsd_prep_reset_launch((float *)state, C, S, slots, count, (hipStream_t)stream);
}

int nsd_prep_step(const nsd_dims *d, const nsd_prep *p, const float *x, const int32_t *slots, void *state, int64_t state_bytes,
                  int32_t S, float *y, void *stream) {
    static const char *who = "prep_step";
    if (!d || !p || !x || !y) { nsd_set_error("%s: null pointer (d, p, x, y)", who); return NSD_E_INVALID; }
    if (!prep_channels(d->C)) { nsd_set_error("%s: C = %d channels outside [1, 64]", who, d->C); return NSD_E_INVALID; }
    if (d->T < 1 || d->B < 0) { nsd_set_error("%s: shape B=%d T=%d (B >= 0, T >= 1)", who, d->B, d->T); return NSD_E_INVALID; }
    if (!prep_config(p, who)) return NSD_E_INVALID;
    if (slots && !state) { nsd_set_error("%s: slots without a state (window mode takes neither)", who); return NSD_E_INVALID; }
    if (state) {
        if (const int rc = prep_enter(d->C, who, state, state_bytes, S)) return rc;
        if (d->B > S) { nsd_set_error("%s: B = %d streams, S = %d slots", who, d->B, S); return NSD_E_INVALID; }
    }
    const int64_t n = (int64_t)d->B * d->T * d->C;
    if (x != y && x < y + n && y < x + n) { nsd_set_error("%s: y overlaps x partially (in place means y == x)", who); return NSD_E_INVALID; }
    if (d->B == 0) return NSD_OK;
    CausalPrepArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.y = y; a.slots = slots; a.state = (float *)state;
    a.B = d->B; a.T = d->T; a.C = d->C; a.S = state ? S : 0;
    a.baseline = (p->flags & NSD_PREP_BASELINE) != 0; a.car = (p->flags & NSD_PREP_CAR) != 0;
    a.ns = p->n_sections; a.zs = p->alpha > 0.f;
    memcpy(a.sos, p->sos, sizeof(a.sos));
    a.alpha = p->alpha; a.oma = 1.0f - p->alpha; a.var0 = p->var0;
    return nsd_prep_launch(a, (hipStream_t)stream);
}

// ---- rate conversion (nsd_resample_*, include/nsd.h; nsd_resample.hip) ----
static int resample_gcd(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }
// the configuration alone: ratio and taps per phase (who == NULL: a silent query)
static bool resample_config(const nsd_resample *r, const char *who) {
#define RS_REFUSE(...) do { if (who) nsd_set_error(__VA_ARGS__); return false; } while (0)
    if (r->L < 1 || r->L > 1024 || r->M < 1 || r->M > 1024) RS_REFUSE("%s: L / M = %d / %d outside [1, 1024]", who, r->L, r->M);
    if (resample_gcd(r->L, r->M) != 1) RS_REFUSE("%s: L / M = %d / %d is not reduced (gcd %d)", who, r->L, r->M, resample_gcd(r->L, r->M));
    if (r->P < 1 || r->P > 256) RS_REFUSE("%s: P = %d taps per phase outside [1, 256]", who, r->P);
    if ((int64_t)r->L * r->P > 65536) RS_REFUSE("%s: L * P = %lld taps, more than 65536", who, (long long)r->L * r->P);
#undef RS_REFUSE
    return true;
}
// the preamble of the entry points that touch a resample state: channels, configuration, slot count, size
static int resample_enter(int32_t C, const nsd_resample *r, const char *who, const void *state, int64_t state_bytes, int32_t S) {
    if (!prep_channels(C)) { nsd_set_error("%s: C = %d channels outside [1, 64]", who, C); return NSD_E_INVALID; }
    if (!r) { nsd_set_error("%s: null configuration", who); return NSD_E_INVALID; }
    if (!resample_config(r, who)) return NSD_E_INVALID;
    if (!state) { nsd_set_error("%s: null state", who); return NSD_E_INVALID; }
    if ((uintptr_t)state % 8) { nsd_set_error("%s: state is not 8-byte aligned (it holds an int64 count)", who); return NSD_E_INVALID; }
    if (S < 1) { nsd_set_error("%s: S = %d slots", who, S); return NSD_E_INVALID; }
    const int64_t need = (int64_t)S * rs_stride(C, r->P) * (int64_t)sizeof(float);
    if (state_bytes < need) {
        nsd_set_error("%s: state of %lld bytes is smaller than nsd_resample_state_bytes() = %lld", who, (long long)state_bytes, (long long)need);
        return NSD_E_WORKSPACE;
    }
    return NSD_OK;
}

int nsd_resample_path(int32_t C, const nsd_resample *r) { return prep_channels(C) && (!r || resample_config(r, nullptr)) ? 1 : 0; }

int64_t nsd_resample_out_steps(const nsd_resample *r, int64_t n_in, int64_t T) {
    static const char *who = "resample_out_steps";
    if (!r) { nsd_set_error("%s: null configuration", who); return NSD_E_INVALID; }
    if (!resample_config(r, who)) return NSD_E_INVALID;
    if (n_in < 0 || T < 0 || n_in > RS_MAX_N_IN || T > RS_MAX_N_IN) {
        nsd_set_error("%s: n_in = %lld, T = %lld outside [0, 2^40]", who, (long long)n_in, (long long)T);
        return NSD_E_INVALID;
    }
    return rs_ceil_div((n_in + T) * r->L, r->M) - rs_ceil_div(n_in * r->L, r->M);
}

int64_t nsd_resample_state_bytes(int32_t C, const nsd_resample *r, int32_t S) {
    if (!prep_channels(C) || !r || S < 1) { nsd_set_error("resample_state_bytes: C outside [1, 64], null configuration, or S < 1"); return NSD_E_INVALID; }
    if (!resample_config(r, "resample_state_bytes")) return NSD_E_INVALID;
    return (int64_t)S * rs_stride(C, r->P) * (int64_t)sizeof(float);
}

int nsd_resample_state_layout(int32_t C, const nsd_resample *r, nsd_resample_layout *out) {
    if (!prep_channels(C) || !r || !out) { nsd_set_error("resample_state_layout: C outside [1, 64], or null pointer"); return NSD_E_INVALID; }
    if (!resample_config(r, "resample_state_layout")) return NSD_E_INVALID;
    out->hist = RS_HIST; out->n_in = rs_n_in(C, r->P); out->stride = rs_stride(C, r->P);
    return NSD_OK;
}

int nsd_resample_reset(int32_t C, const nsd_resample *r, void *state, int64_t state_bytes, int32_t S, const int32_t *slots, int32_t n,
                       void *stream) {
    static const char *who = "resample_reset";
    if (const int rc = resample_enter(C, r, who, state, state_bytes, S)) return rc;
    if (slots && (n < 0 || n > S)) { nsd_set_error("%s: n = %d slots of S = %d", who, n, S); return NSD_E_INVALID; }
    const int count = slots ? n : S;
    if (count == 0) return NSD_OK;
    return nsd_resample_reset_launch((float *)state, rs_stride(C, r->P), S, slots, count, (hipStream_t)stream);
}

int nsd_resample_step(const nsd_dims *d, const nsd_resample *r, const float *taps, const float *x, const int32_t *slots, void *state,
                      int64_t state_bytes, int32_t S, float *y, int64_t To, int32_t *cnt, void *stream) {
    static const char *who = "resample_step";
    if (!d || !r || !taps || !x || !y) { nsd_set_error("%s: null pointer (d, r, taps, x, y)", who); return NSD_E_INVALID; }
    if (!prep_channels(d->C)) { nsd_set_error("%s: C = %d channels outside [1, 64]", who, d->C); return NSD_E_INVALID; }
    if (d->T < 1 || d->B < 0) { nsd_set_error("%s: shape B=%d T=%d (B >= 0, T >= 1)", who, d->B, d->T); return NSD_E_INVALID; }
    if ((int64_t)d->T * d->C > 0x7fffffff) { nsd_set_error("%s: T * C = %lld values per stream in one call", who, (long long)d->T * d->C); return NSD_E_INVALID; }
    if (!resample_config(r, who)) return NSD_E_INVALID;
    if (slots && !state) { nsd_set_error("%s: slots without a state (window mode takes neither)", who); return NSD_E_INVALID; }
    if (state) {
        if (const int rc = resample_enter(d->C, r, who, state, state_bytes, S)) return rc;
        if (d->B > S) { nsd_set_error("%s: B = %d streams, S = %d slots", who, d->B, S); return NSD_E_INVALID; }
    }
    const int64_t most = rs_ceil_div((int64_t)d->T * r->L, r->M);
    if (state ? To < most : To != most) {
        nsd_set_error("%s: To = %lld rows of y, ceil(T * L / M) = %lld (stream mode: at least; window mode: exactly)", who, (long long)To, (long long)most);
        return NSD_E_INVALID;
    }
    if (To > 0x7fffffff / 64) { nsd_set_error("%s: To = %lld rows of y in one call", who, (long long)To); return NSD_E_INVALID; }
    const int64_t nx = (int64_t)d->B * d->T * d->C, ny = (int64_t)d->B * To * d->C;
    if (x < y + ny && y < x + nx) { nsd_set_error("%s: y overlaps x", who); return NSD_E_INVALID; }
    if (d->B == 0) return NSD_OK;
    ResampleArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.y = y; a.taps = taps; a.slots = slots; a.state = (float *)state; a.cnt = cnt; a.To = To;
    a.B = d->B; a.T = d->T; a.C = d->C; a.S = state ? S : 0;
    a.L = r->L; a.M = r->M; a.P = r->P;
    return nsd_resample_launch(a, (hipStream_t)stream);
}

// ---- signal-quality gate (nsd_gate_*, include/nsd.h; nsd_gate.hip) ----
static bool gate_channels(int32_t C) { return C >= 1 && C <= 32; }
// the configuration alone (who == NULL: a silent query)
static bool gate_config(const nsd_gate *g, const char *who) {
#define GATE_REFUSE(...) do { if (who) nsd_set_error(__VA_ARGS__); return false; } while (0)
    const float thr[4] = {g->rail, g->jump, g->flat_eps, g->pp};
    static const char *const names[4] = {"rail", "jump", "flat_eps", "pp"};
    for (int k = 0; k < 4; ++k)
        if (!prep_finite(thr[k]) || thr[k] < 0.f) GATE_REFUSE("%s: %s = %g (a threshold is finite and >= 0)", who, names[k], thr[k]);
    if (g->flat_samples < 0) GATE_REFUSE("%s: flat_samples = %d < 0", who, g->flat_samples);
    if (g->pp_samples < 0 || g->pp_samples > NSD_GATE_MAX_SPAN) GATE_REFUSE("%s: pp_samples = %d outside [0, %d]", who, g->pp_samples, NSD_GATE_MAX_SPAN);
    if (g->hold_samples < 0) GATE_REFUSE("%s: hold_samples = %d < 0", who, g->hold_samples);
    if (g->max_bad < 0) GATE_REFUSE("%s: max_bad = %d < 0", who, g->max_bad);
    if (g->flags & ~NSD_GATE_ZERO) GATE_REFUSE("%s: unknown flag bits 0x%x", who, g->flags);
#undef GATE_REFUSE
    return true;
}
// the preamble of the entry points that touch a gate state: channels, slot count, size
static int gate_enter(int32_t C, const char *who, const void *state, int64_t state_bytes, int32_t S) {
    if (!gate_channels(C)) { nsd_set_error("%s: C = %d channels outside [1, 32]", who, C); return NSD_E_INVALID; }
    if (!state) { nsd_set_error("%s: null state", who); return NSD_E_INVALID; }
    if ((uintptr_t)state % 8) { nsd_set_error("%s: state is not 8-byte aligned (it holds int64 counts)", who); return NSD_E_INVALID; }
    if (S < 1) { nsd_set_error("%s: S = %d slots", who, S); return NSD_E_INVALID; }
    const int64_t need = (int64_t)S * gate_stride(C) * (int64_t)sizeof(float);
    if (state_bytes < need) {
        nsd_set_error("%s: state of %lld bytes is smaller than nsd_gate_state_bytes() = %lld", who, (long long)state_bytes, (long long)need);
        return NSD_E_WORKSPACE;
    }
    return NSD_OK;
}

int nsd_gate_path(int32_t C, const nsd_gate *g) { return gate_channels(C) && (!g || gate_config(g, nullptr)) ? 1 : 0; }

int64_t nsd_gate_state_bytes(int32_t C, int32_t S) {
    if (!gate_channels(C) || S < 1) { nsd_set_error("gate_state_bytes: C outside [1, 32], or S < 1"); return NSD_E_INVALID; }
    return (int64_t)S * gate_stride(C) * (int64_t)sizeof(float);
}

int nsd_gate_state_layout(int32_t C, nsd_gate_layout *out) {
    if (!gate_channels(C) || !out) { nsd_set_error("gate_state_layout: C outside [1, 32], or null pointer"); return NSD_E_INVALID; }
    out->prev = GATE_PREV; out->held = gate_held(C); out->run = gate_run(C); out->hang = gate_hang(C); out->ring = gate_ring(C);
    out->bad = gate_bad(C); out->rejected = gate_rejected(C); out->steps = gate_steps(C); out->stride = gate_stride(C);
    return NSD_OK;
}

int nsd_gate_reset(int32_t C, void *state, int64_t state_bytes, int32_t S, const int32_t *slots, int32_t n, void *stream) {
    static const char *who = "gate_reset";
    if (const int rc = gate_enter(C, who, state, state_bytes, S)) return rc;
    if (slots && (n < 0 || n > S)) { nsd_set_error("%s: n = %d slots of S = %d", who, n, S); return NSD_E_INVALID; }
    const int count = slots ? n : S;
    if (count == 0) return NSD_OK;
    return nsd_gate_reset_launch((float *)state, C, S, slots, count, (hipStream_t)stream);
}

int nsd_gate_step(const nsd_dims *d, const nsd_gate *g, const float *x, const int32_t *slots, void *state, int64_t state_bytes,
                  int32_t S, float *y, uint32_t *mask, void *stream) {
    static const char *who = "gate_step";
    if (!d || !g || !x || !y || !mask) { nsd_set_error("%s: null pointer (d, g, x, y, mask)", who); return NSD_E_INVALID; }
    if (!gate_channels(d->C)) { nsd_set_error("%s: C = %d channels outside [1, 32]", who, d->C); return NSD_E_INVALID; }
    if (d->T < 1 || d->B < 0) { nsd_set_error("%s: shape B=%d T=%d (B >= 0, T >= 1)", who, d->B, d->T); return NSD_E_INVALID; }
    if (!gate_config(g, who)) return NSD_E_INVALID;
    if (slots && !state) { nsd_set_error("%s: slots without a state (window mode takes neither)", who); return NSD_E_INVALID; }
    if (state) {
        if (const int rc = gate_enter(d->C, who, state, state_bytes, S)) return rc;
        if (d->B > S) { nsd_set_error("%s: B = %d streams, S = %d slots", who, d->B, S); return NSD_E_INVALID; }
    }
    const int64_t n = (int64_t)d->B * d->T * d->C;
    if (x != y && x < y + n && y < x + n) { nsd_set_error("%s: y overlaps x partially (in place means y == x)", who); return NSD_E_INVALID; }
    if (d->B == 0) return NSD_OK;
    GateArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.y = y; a.mask = mask; a.slots = slots; a.state = (float *)state;
    a.B = d->B; a.T = d->T; a.C = d->C; a.S = state ? S : 0;
    a.rail = g->rail; a.jump = g->jump; a.flat_eps = g->flat_eps; a.pp = g->pp;
    a.flat_samples = g->flat_samples; a.pp_samples = g->pp_samples; a.hold_samples = g->hold_samples; a.max_bad = g->max_bad;
    return nsd_gate_launch(a, (hipStream_t)stream);
}

int nsd_gate_apply(const nsd_dims *d, const nsd_gate *g, const float *v, const uint32_t *mask, float *out, void *stream) {
    static const char *who = "gate_apply";
    if (!d || !g || !v || !mask || !out) { nsd_set_error("%s: null pointer (d, g, v, mask, out)", who); return NSD_E_INVALID; }
    if (!gate_channels(d->C)) { nsd_set_error("%s: C = %d channels outside [1, 32]", who, d->C); return NSD_E_INVALID; }
    if (d->T < 1 || d->B < 0) { nsd_set_error("%s: shape B=%d T=%d (B >= 0, T >= 1)", who, d->B, d->T); return NSD_E_INVALID; }
    if (!gate_config(g, who)) return NSD_E_INVALID;
    const int64_t n = (int64_t)d->B * d->T * d->C;
    if (v != out && v < out + n && out < v + n) { nsd_set_error("%s: out overlaps v partially (in place means out == v)", who); return NSD_E_INVALID; }
    if (d->B == 0) return NSD_OK;
    GateApplyArgs a;
    memset(&a, 0, sizeof(a));
    a.v = v; a.mask = mask; a.out = out;
    a.steps = (long)d->B * d->T; a.C = d->C; a.max_bad = g->max_bad; a.zero = (g->flags & NSD_GATE_ZERO) != 0;
    return nsd_gate_apply_launch(a, (hipStream_t)stream);
}

// ---- session alignment (nsd_cov_* / nsd_whiten_fit / nsd_spatial_apply, include/nsd.h; nsd_align.hip) ----
// the preamble of the entry points that touch a cov state: channels, slot count, size
static int cov_enter(int32_t C, const char *who, const void *state, int64_t state_bytes, int32_t S) {
    if (!gate_channels(C)) { nsd_set_error("%s: C = %d channels outside [1, 32]", who, C); return NSD_E_INVALID; }
    if (!state) { nsd_set_error("%s: null state", who); return NSD_E_INVALID; }
    if ((uintptr_t)state % 8) { nsd_set_error("%s: state is not 8-byte aligned (it holds doubles and int64 counts)", who); return NSD_E_INVALID; }
    if (S < 1) { nsd_set_error("%s: S = %d slots", who, S); return NSD_E_INVALID; }
    const int64_t need = (int64_t)S * cov_stride(C) * (int64_t)sizeof(double);
    if (state_bytes < need) {
        nsd_set_error("%s: state of %lld bytes is smaller than nsd_cov_state_bytes() = %lld", who, (long long)state_bytes, (long long)need);
        return NSD_E_WORKSPACE;
    }
    return NSD_OK;
}

int64_t nsd_cov_state_bytes(int32_t C, int32_t S) {
    if (!gate_channels(C) || S < 1) { nsd_set_error("cov_state_bytes: C outside [1, 32], or S < 1"); return NSD_E_INVALID; }
    return (int64_t)S * cov_stride(C) * (int64_t)sizeof(double);
}

int nsd_cov_state_layout(int32_t C, nsd_cov_layout *out) {
    if (!gate_channels(C) || !out) { nsd_set_error("cov_state_layout: C outside [1, 32], or null pointer"); return NSD_E_INVALID; }
    out->sum = COV_SUM; out->count = cov_count(C); out->skipped = cov_skipped(C); out->stride = cov_stride(C);
    return NSD_OK;
}

int nsd_cov_reset(int32_t C, void *state, int64_t state_bytes, int32_t S, const int32_t *slots, int32_t n, void *stream) {
    static const char *who = "cov_reset";
    if (const int rc = cov_enter(C, who, state, state_bytes, S)) return rc;
    if (slots && (n < 0 || n > S)) { nsd_set_error("%s: n = %d slots of S = %d", who, n, S); return NSD_E_INVALID; }
    const int count = slots ? n : S;
    if (count == 0) return NSD_OK;
    return nsd_cov_reset_launch((double *)state, C, S, slots, count, (hipStream_t)stream);
}

int nsd_cov_step(const nsd_dims *d, const float *v, const uint32_t *mask, const int32_t *slots, void *state, int64_t state_bytes,
                 int32_t S, double *sums, int64_t *counts, void *stream) {
    static const char *who = "cov_step";
    if (!d || !v) { nsd_set_error("%s: null pointer (d, v)", who); return NSD_E_INVALID; }
    if (!gate_channels(d->C)) { nsd_set_error("%s: C = %d channels outside [1, 32]", who, d->C); return NSD_E_INVALID; }
    if (d->T < 1 || d->B < 0) { nsd_set_error("%s: shape B=%d T=%d (B >= 0, T >= 1)", who, d->B, d->T); return NSD_E_INVALID; }
    if (slots && !state) { nsd_set_error("%s: slots without a state (window mode takes neither)", who); return NSD_E_INVALID; }
    if (state) {
        if (sums || counts) { nsd_set_error("%s: sums / counts with a state (stream mode keeps them in the state)", who); return NSD_E_INVALID; }
        if (const int rc = cov_enter(d->C, who, state, state_bytes, S)) return rc;
        if (d->B > S) { nsd_set_error("%s: B = %d streams, S = %d slots", who, d->B, S); return NSD_E_INVALID; }
    } else if (!sums || !counts) {
        nsd_set_error("%s: window mode needs sums and counts", who); return NSD_E_INVALID;
    } else if ((uintptr_t)sums % 8 || (uintptr_t)counts % 8) {
        nsd_set_error("%s: sums / counts are not 8-byte aligned", who); return NSD_E_INVALID;
    }
    if (d->B == 0) return NSD_OK;
    CovArgs a;
    memset(&a, 0, sizeof(a));
    a.v = v; a.mask = mask; a.slots = slots; a.state = (double *)state; a.sums = sums; a.counts = (long long *)counts;
    a.B = d->B; a.T = d->T; a.C = d->C; a.S = state ? S : 0;
    return nsd_cov_launch(a, (hipStream_t)stream);
}

int nsd_whiten_fit(int32_t C, const nsd_whiten *w, const double *sums, int64_t sum_stride, const int64_t *counts, int64_t count_stride,
                   int32_t N, const int32_t *group, int32_t G, float *W, nsd_whiten_record *records, void *stream) {
    static const char *who = "whiten_fit";
    if (!w || !W || !records) { nsd_set_error("%s: null pointer (w, W, records)", who); return NSD_E_INVALID; }
    if (!gate_channels(C)) { nsd_set_error("%s: C = %d channels outside [1, 32]", who, C); return NSD_E_INVALID; }
    if (N < 0 || G < 1) { nsd_set_error("%s: N = %d accumulators, G = %d groups (N >= 0, G >= 1)", who, N, G); return NSD_E_INVALID; }
    if (N > 0 && (!sums || !counts)) { nsd_set_error("%s: null pointer (sums, counts)", who); return NSD_E_INVALID; }
    if (N > 0 && ((uintptr_t)sums % 8 || (uintptr_t)counts % 8)) { nsd_set_error("%s: sums / counts are not 8-byte aligned", who); return NSD_E_INVALID; }
    if ((uintptr_t)records % 16) { nsd_set_error("%s: records are not 16-byte aligned", who); return NSD_E_INVALID; }
    if (sum_stride < (int64_t)C * C || count_stride < 2) {
        nsd_set_error("%s: sum_stride = %lld (>= C*C), count_stride = %lld (>= 2)", who, (long long)sum_stride, (long long)count_stride);
        return NSD_E_INVALID;
    }
    if (!(w->shrinkage >= 0.f && w->shrinkage <= 1.f)) { nsd_set_error("%s: shrinkage %g outside [0, 1]", who, w->shrinkage); return NSD_E_INVALID; }
    if (!(w->floor > 0.f && w->floor <= 1.f)) { nsd_set_error("%s: floor %g outside (0, 1]", who, w->floor); return NSD_E_INVALID; }
    if (w->min_steps < 1) { nsd_set_error("%s: min_steps = %d < 1", who, w->min_steps); return NSD_E_INVALID; }
    WhitenArgs a;
    memset(&a, 0, sizeof(a));
    a.sums = sums; a.counts = (const long long *)counts; a.sum_stride = sum_stride; a.count_stride = count_stride; a.group = group;
    a.W = W; a.records = records; a.C = C; a.N = N; a.G = G; a.min_steps = w->min_steps;
    a.shrinkage = (double)w->shrinkage; a.floor = (double)w->floor;
    return nsd_whiten_launch(a, (hipStream_t)stream);
}

int nsd_spatial_apply(const nsd_dims *d, const float *v, const float *W, int32_t n_mat, const int32_t *sel, float *out, void *stream) {
    static const char *who = "spatial_apply";
    if (!d || !v || !W || !out) { nsd_set_error("%s: null pointer (d, v, W, out)", who); return NSD_E_INVALID; }
    if (!gate_channels(d->C)) { nsd_set_error("%s: C = %d channels outside [1, 32]", who, d->C); return NSD_E_INVALID; }
    if (d->T < 1 || d->B < 0) { nsd_set_error("%s: shape B=%d T=%d (B >= 0, T >= 1)", who, d->B, d->T); return NSD_E_INVALID; }
    if (n_mat < 1) { nsd_set_error("%s: n_mat = %d matrices", who, n_mat); return NSD_E_INVALID; }
    const int64_t n = (int64_t)d->B * d->T * d->C;
    if (v != out && v < out + n && out < v + n) { nsd_set_error("%s: out overlaps v partially (in place means out == v)", who); return NSD_E_INVALID; }
    if (d->B == 0) return NSD_OK;
    SpatialArgs a;
    memset(&a, 0, sizeof(a));
    a.v = v; a.W = W; a.sel = sel; a.out = out; a.B = d->B; a.T = d->T; a.C = d->C; a.n_mat = n_mat;
    return nsd_spatial_launch(a, (hipStream_t)stream);
}

// ---- supervised session alignment (nsd_spatial_bwd / nsd_spatial_fit_step, include/nsd.h; nsd_align.hip) ----
int64_t nsd_spatial_bwd_scratch_bytes(const nsd_dims *d) {
    if (!d || !gate_channels(d->C) || d->B < 0) { nsd_set_error("spatial_bwd_scratch_bytes: null d, C outside [1, 32], or B < 0"); return NSD_E_INVALID; }
    return (int64_t)d->B * d->C * d->C * (int64_t)sizeof(double);
}

int nsd_spatial_bwd(const nsd_dims *d, const float *v, const float *dy, const float *W, int32_t n_mat, const int32_t *sel,
                    float *dv, float *dW, int64_t *counts, void *scratch, int64_t scratch_bytes, void *stream) {
    static const char *who = "spatial_bwd";
    if (!d || !v || !dy || !W) { nsd_set_error("%s: null pointer (d, v, dy, W)", who); return NSD_E_INVALID; }
    if (!dv && !dW) { nsd_set_error("%s: neither dv nor dW", who); return NSD_E_INVALID; }
    if (!gate_channels(d->C)) { nsd_set_error("%s: C = %d channels outside [1, 32]", who, d->C); return NSD_E_INVALID; }
    if (d->T < 1 || d->B < 0) { nsd_set_error("%s: shape B=%d T=%d (B >= 0, T >= 1)", who, d->B, d->T); return NSD_E_INVALID; }
    if (n_mat < 1) { nsd_set_error("%s: n_mat = %d matrices", who, n_mat); return NSD_E_INVALID; }
    const int64_t n = (int64_t)d->B * d->T * d->C;
    if (dv && dv != dy && dy < dv + n && dv < dy + n) { nsd_set_error("%s: dv overlaps dy partially (in place means dv == dy)", who); return NSD_E_INVALID; }
    if (dW && d->B > 0) {
        if (!scratch) { nsd_set_error("%s: dW without a scratch", who); return NSD_E_INVALID; }
        if ((uintptr_t)scratch % 8) { nsd_set_error("%s: scratch is not 8-byte aligned (it holds doubles)", who); return NSD_E_INVALID; }
        const int64_t need = (int64_t)d->B * d->C * d->C * (int64_t)sizeof(double);
        if (scratch_bytes < need) {
            nsd_set_error("%s: scratch of %lld bytes is smaller than nsd_spatial_bwd_scratch_bytes() = %lld", who, (long long)scratch_bytes, (long long)need);
            return NSD_E_WORKSPACE;
        }
    }
    if (counts && (uintptr_t)counts % 8) { nsd_set_error("%s: counts are not 8-byte aligned", who); return NSD_E_INVALID; }
    SpatialBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.v = v; a.dy = dy; a.W = W; a.sel = sel; a.dv = dv; a.dW = dW; a.counts = (long long *)counts; a.p = (double *)scratch;
    a.B = d->B; a.T = d->T; a.C = d->C; a.n_mat = n_mat;
    return nsd_spatial_bwd_launch(a, (hipStream_t)stream);
}

int64_t nsd_spatial_fit_state_bytes(int32_t C, int32_t n_mat) {
    if (!gate_channels(C) || n_mat < 1) { nsd_set_error("spatial_fit_state_bytes: C outside [1, 32], or n_mat < 1"); return NSD_E_INVALID; }
    return (int64_t)n_mat * sfit_stride(C) + (int64_t)sizeof(int64_t);
}

int nsd_spatial_fit_state_layout(int32_t C, nsd_spatial_fit_layout *out) {
    if (!gate_channels(C) || !out) { nsd_set_error("spatial_fit_state_layout: C outside [1, 32], or null pointer"); return NSD_E_INVALID; }
    out->m = sfit_m(C); out->v = sfit_v(C); out->step = sfit_step(C); out->skipped = sfit_skipped(C); out->status = sfit_status(C);
    out->stride = sfit_stride(C);
    return NSD_OK;
}

int nsd_spatial_fit_step(int32_t C, int32_t n_mat, float *A, const float *A0, const float *dW, const nsd_spatial_fit *fit,
                         void *state, int64_t state_bytes, const float *loss_in, float *loss_out, int32_t loss_cap, void *stream) {
    static const char *who = "spatial_fit_step";
    if (!A || !dW || !fit || !state) { nsd_set_error("%s: null pointer (A, dW, fit, state)", who); return NSD_E_INVALID; }
    if (!gate_channels(C)) { nsd_set_error("%s: C = %d channels outside [1, 32]", who, C); return NSD_E_INVALID; }
    if (n_mat < 1) { nsd_set_error("%s: n_mat = %d matrices", who, n_mat); return NSD_E_INVALID; }
    if (!(fit->lr >= 0.f) || !std::isfinite(fit->lr)) { nsd_set_error("%s: lr %g negative or not finite", who, fit->lr); return NSD_E_INVALID; }
    if (!(fit->decay >= 0.f) || !std::isfinite(fit->decay)) { nsd_set_error("%s: decay %g negative or not finite", who, fit->decay); return NSD_E_INVALID; }
    if (!(fit->beta1 >= 0.f && fit->beta1 < 1.f)) { nsd_set_error("%s: beta1 %g outside [0, 1)", who, fit->beta1); return NSD_E_INVALID; }
    if (!(fit->beta2 >= 0.f && fit->beta2 < 1.f)) { nsd_set_error("%s: beta2 %g outside [0, 1)", who, fit->beta2); return NSD_E_INVALID; }
    if (!(fit->eps > 0.f) || !std::isfinite(fit->eps)) { nsd_set_error("%s: eps %g not positive or not finite", who, fit->eps); return NSD_E_INVALID; }
    if ((uintptr_t)state % 8) { nsd_set_error("%s: state is not 8-byte aligned (it holds int64 counters)", who); return NSD_E_INVALID; }
    const int64_t need = (int64_t)n_mat * sfit_stride(C) + (int64_t)sizeof(int64_t);
    if (state_bytes < need) {
        nsd_set_error("%s: state of %lld bytes is smaller than nsd_spatial_fit_state_bytes() = %lld", who, (long long)state_bytes, (long long)need);
        return NSD_E_INVALID;
    }
    if (loss_in && (!loss_out || loss_cap < 0)) { nsd_set_error("%s: loss_in without loss_out, or loss_cap = %d < 0", who, loss_cap); return NSD_E_INVALID; }
    SpatialFitArgs a;
    memset(&a, 0, sizeof(a));
    a.A = A; a.A0 = A0; a.dW = dW; a.state = (unsigned char *)state; a.loss_in = loss_in; a.loss_out = loss_out; a.loss_cap = loss_in ? loss_cap : 0;
    a.C = C; a.n_mat = n_mat; a.lr = fit->lr; a.b1 = fit->beta1; a.b2 = fit->beta2; a.eps = fit->eps; a.decay = fit->decay;
    return nsd_spatial_fit_launch(a, (hipStream_t)stream);
}

}  // extern "C"
