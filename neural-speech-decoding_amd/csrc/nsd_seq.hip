// nsd_seq.hip -- orchestration and C ABI of the sequence-batched path (declared in include/nsd.h, "nsd_seq_*"):
// parameter / workspace layout, the per-layer sequence  input-projection GEMM -> persistent scan  (forward) and
// persistent scan -> weight-gradient / input-gradient GEMMs  (backward), head on the time-major sequence.
// Model: EEG_LSTM of Neuro-Alpha-App/Utilities/lstm_eeg_model.py:13-39 (+ bidirectional nn.LSTM where :16-22 would take the
// kwarg); parameter order = torch's state_dict order (…_l{k}, then …_l{k}_reverse per layer).
#include <string.h>
#include <vector>
#include "nsd_seq.h"
#include "nsd_args.h"
#include "nsd_diag.h"

namespace {

// ---- opt-in launch timing: DIAGNOSTIC BUILD ONLY (make diag -> libnsd_hip_diag.so, -DNSD_DIAG=1; declared in nsd_diag.h, not in
// include/nsd.h).  HIP events on the launch stream around the kernels of the path, so that a benchmark can quote the dominant
// kernel's own duration.  The product library has neither the state nor the entry points.
enum { PK_SCAN_FWD = 0, PK_SCAN_BWD = 1, PK_GEMM_XPROJ = 2, PK_GEMM_DW = 3, PK_GEMM_DIN = 4, PK_HEAD = 5, PK_HEAD_GRADS = 6, PK_PREP = 7,
       PK_GEMM_DX = 8, PK_HEAD_BWD = 9, PK_COUNT = 10 };
#if NSD_DIAG
struct ProfRec { hipEvent_t a, b; int kind; };
struct ProfState { bool on = false; std::vector<ProfRec> recs; } g_prof;
struct ProfScope {
    hipStream_t st; int idx = -1;
    ProfScope(int kind, hipStream_t s) : st(s) {
        if (!g_prof.on) return;
        ProfRec r; r.kind = kind;
        if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return;
        (void)hipEventRecord(r.a, st);
        g_prof.recs.push_back(r);
        idx = (int)g_prof.recs.size() - 1;
    }
    ~ProfScope() { if (idx >= 0) (void)hipEventRecord(g_prof.recs[idx].b, st); }
};
#else
struct ProfScope { ProfScope(int, hipStream_t) {} ~ProfScope() {} };
#endif

inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// scan groups that can be resident at once: a group takes P workgroups per direction, one per CU
int scan_cap(const SeqDims &s) { return nsd_num_cus() / (s.P * s.D); }

int derive(const nsd_dims *d, uint32_t flags, SeqDims *o) {
    if (nsd_check_dims(d) != NSD_OK) return NSD_E_INVALID;
    if (flags & ~(uint32_t)(NSD_FLAG_BIDIR | NSD_FLAG_RESIDUAL | NSD_FLAG_TRAIN | (NSD_DIAG ? NSD_DIAG_FLAG_ALL : 0u))) {
        nsd_set_error("seq path: unknown flag bits 0x%x", flags);
        return NSD_E_INVALID;
    }
    SeqDims s;
    s.B = d->B; s.T = d->T; s.C = d->C; s.H = d->H; s.L = d->L; s.K = d->K; s.F = d->F;
    s.D = (flags & NSD_FLAG_BIDIR) ? 2 : 1;
    s.residual = (flags & NSD_FLAG_RESIDUAL) ? 1 : 0;
    if (!nsd_scan_supported(s.H)) { nsd_set_error("seq path: hidden size %d not covered (64, 128, 256, 512)", s.H); return NSD_E_INVALID; }
    if (s.F > 64 || s.K > 64) { nsd_set_error("seq path: F=%d K=%d exceed 64", s.F, s.K); return NSD_E_INVALID; }
    s.P = s.H / 32;
    s.CP = (int)align_up(s.C, 16);
    const int cus = nsd_num_cus(), cap = scan_cap(s);
    if (cap < 1) { nsd_set_error("seq path: H=%d D=%d needs %d workgroups per group, device has %d CUs", s.H, s.D, s.P * s.D, cus); return NSD_E_INVALID; }
    const int g32 = (s.B + 31) / 32;
    s.MG = (g32 <= cap) ? 32 : 64;
    s.Bp = (int)align_up(s.B > 0 ? s.B : 1, s.MG);
    s.groups = s.Bp / s.MG;
    // two unidirectional layers: one launch advances both, layer 1 a step behind layer 0 (nsd_scan2.hip)
    s.fused2 = (s.D == 1 && s.L == 2 && !s.residual && !(NSD_DIAG && (flags & NSD_DIAG_FLAG_NO_FUSED_LAYERS)) && s.CP <= 64 && nsd_scan2_supported(s.H, s.MG)) ? 1 : 0;
    *o = s;
    return NSD_OK;
}

// The flag sets of the scans (NSD_SEQ_GROUP_WORDS rendezvous words per group and direction, nsd_seq.h): forward sets of every layer,
// then the backward sets.  Words in front of the sets of the launch of pass (0 forward, 1 backward), layer l, whose first group is g0;
// chunks of one layer are disjoint.  The fused two-layer route (D = 1) uses layer 0's sets.  (s, 1, 0, 0) is where the backward half
// starts, (s, 2, 0, 0) the size of it all.
int64_t flag_words(const SeqDims &s, int pass, int l, int g0) {
    return (((int64_t)pass * s.L + l) * s.D * s.groups + (int64_t)g0 * s.D) * NSD_SEQ_GROUP_WORDS;
}

constexpr long PARTS_FLOATS = 18L * 1024 * 1024;               // 64 splits of cfg3's 1024 x 256 weight gradient

SeqWs make_ws(const SeqDims &s) {
    SeqWs w;
    memset(&w, 0, sizeof(w));
    const int64_t R = (int64_t)s.T * s.Bp, H = s.H, G = 4 * H, DH = (int64_t)s.D * H;
    int64_t p = 0;
    auto take = [&](int64_t bytes) { const int64_t at = p; p = align_up(p + bytes, 256); return at; };
    (void)take(NSD_SEQ_HEADER_BYTES);                            // persistent header: sticky status (nsd_seq_workspace_init zeroes it)
    w.status = take(NSD_SEQ_STATUS_WORDS * 4);                   // == NSD_SEQ_HEADER_BYTES: nsd_seq_status / nsd_seq_guard rely on it
    w.flags_bytes = flag_words(s, 2, 0, 0) * 4;
    w.flags = take(w.flags_bytes);
    w.xbf = take(R * s.CP * 2);
    for (int l = 0; l < s.L; ++l) {
        const int64_t I = l == 0 ? s.C : DH, Ip = l == 0 ? s.CP : DH;
        (void)I;
        for (int d = 0; d < s.D; ++d) {
            w.wf[l][d] = take(G * H * 2);
            w.wb[l][d] = take(H * G * 2);
            w.wx[l][d] = take(G * Ip * 2);
            w.bsum[l][d] = take(G * 4);
        }
        w.wxt[l] = l > 0 ? take(DH * s.D * G * 2) : 0;
        w.hs[l] = take(R * DH * 2);
        w.lk[l] = (l < s.L - 1 || s.residual) ? take(R * DH * 2) : 0;
        for (int d = 0; d < s.D; ++d) {
            w.cs[l][d] = take(R * H * 2);
            w.ga[l][d] = take(R * G * 2);
        }
    }
    for (int d = 0; d < s.D; ++d) w.xproj[d] = take(R * G * 2);
    w.da = take(R * s.D * G * 2);
    w.da2 = s.fused2 ? take(R * G * 2) : 0;                  // fused two-layer scans: layer 1's da next to layer 0's
    w.din[0] = take(R * DH * (s.residual ? 4 : 2));             // bf16 owner-ordered tiles; row-major fp32 with the residual extension
    w.din[1] = s.residual ? take(R * DH * 4) : 0;           // residual extension: d(linked output) passed around the LSTM
    w.alpha = take(R * 4);
    w.dscore = take(R * 4);
    w.pooled = take((int64_t)s.Bp * DH * 4);
    w.dpooled = take((int64_t)s.Bp * DH * 4);
    w.loss = take((int64_t)s.Bp * 4);
    w.hb_stride = align_up(nsd_head_tm_row_floats((int)DH, s.F, s.K), 4);
    w.hb = take((int64_t)s.Bp * w.hb_stride * 4);
    w.dbp = take((int64_t)(s.D > 2 ? s.D : 2) * s.groups * G * 4);
    {   // exchange rings of the scans, sized for the widest user: h tiles of the forward scans (two slots, step parity) or the
        // partial-sum blocks of the fused backward (nsd_scan2.hip, PartRing: P * P * NT * 4 blocks of 1.5 KB per group, ONE slot)
        const int64_t tiles = 2LL * s.groups * 3 * s.MG * (s.D * 4LL * H) * 2, Pm = H / 32;
        const int64_t parts = 1LL * s.groups * s.D * Pm * Pm * (s.MG / 32) * 4 * 1536;
        w.xch = take(tiles > parts ? tiles : parts);
    }
    w.parts = take(PARTS_FLOATS * 4);                            // split-K partials of the weight-gradient GEMMs
    w.total = p;
    return w;
}

template <class T>
T *at(void *ws, int64_t off) { return reinterpret_cast<T *>(reinterpret_cast<char *>(ws) + off); }

// ---- small reduction kernels of the backward pass -----------------------------------------------------------------------------
// grads rows are torch's (g*H + u); the GEMM's rows are unit-major c = 4u + g.  out[(g*H+u)*I + i] = sum_z part[z][c][i], i < I
__global__ __launch_bounds__(256) void seq_reduce_dw_kernel(const float *part, int nparts, int H, int N, int I, float *out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = 4L * H * I;
    if (e >= total) return;
    const int c = (int)(e / I), i = (int)(e - (long)c * I), u = c >> 2, g = c & 3;
    const long MN = 4L * H * N;
    float s = 0.f;
    for (int z = 0; z < nparts; ++z) s += part[(long)z * MN + (long)c * N + i];
    out[(long)(g * H + u) * I + i] = s;
}
// bias gradients: sum of the per-tile rows the backward scan left
__global__ __launch_bounds__(256) void seq_reduce_db_kernel(const float *part, int nparts, int H, float *b_ih, float *b_hh) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= 4 * H) return;
    float s = 0.f;
    for (int z = 0; z < nparts; ++z) s += part[(long)z * 4 * H + c];
    const int u = c >> 2, g = c & 3;
    b_ih[g * H + u] = s; b_hh[g * H + u] = s;
}

struct Ctx {
    SeqDims s;
    SeqParamLayout pl;
    SeqWs w;
    void *ws;
    const float *params;
    hipStream_t st;
    const char *who;                                             // the entry point, for its error texts
    RngArgs rng;                                                 // the caller's streams (all zero: off)
    bool lstm_drop;                                              // inter-layer dropout is active
    int cap;                                                     // groups per scan launch: what can be resident at once
    int spread;                                                  // NSD_FLAG_SPREAD_GROUPS
    int l2_mode;                                                 // same-XCD exchange shortcut allowed (diagnostic build: NSD_DIAG_FLAG_NO_L2_EXCHANGE clears it)
    int short_grid;                                              // diagnostic build: NSD_DIAG_FLAG_LOSE_MEMBER -> every scan launch misses its last workgroup
};

int split_count(int M, int N, long K) {
    // the 256 x 256 kernel (nsd_gemm_bf16.hip) wants at least one workgroup per CU, the 128 x 128 kernel about two
    const bool big = M >= 256 && N >= 256;
    const int tiles = big ? ((M + 255) / 256) * ((N + 255) / 256) : ((M + 127) / 128) * ((N + 127) / 128);
    int S = big ? (nsd_num_cus() + tiles - 1) / (tiles > 0 ? tiles : 1) : 512 / (tiles > 0 ? tiles : 1);
    if (S < 1) S = 1;
    if (S > 64) S = 64;
    while (S > 1 && K / S < 256) --S;
    while ((long)S * M * N > PARTS_FLOATS && S > 1) --S;
    return S;
}

// a layer writes its LINKED output lk[l] = (h [+ its input]) * multiplier when that differs from h: inter-layer dropout active
// (masked: l < L-1) or the residual extension (l >= 1); readers take lk[l] then, hs[l] otherwise
bool masked(const Ctx &c, int l) { return c.lstm_drop && l < c.s.L - 1; }
bool writes_lk(const Ctx &c, int l) { return masked(c, l) || (c.s.residual && l >= 1); }
const bf16_t *out_of(Ctx &c, int l) { return at<bf16_t>(c.ws, writes_lk(c, l) ? c.w.lk[l] : c.w.hs[l]); }

// The launches of one scan (A: one of the four argument structs of nsd_seq.h) over all groups, at most c.cap of them at a time, each
// chunk on flag sets of its own.  Fills what the four structs share; fill(a) adds the scan's own operands.  bwd: backward pass;
// l: the layer whose output the rng multiplies (0 for the fused two-layer scans).
template <class A, class Fill>
int scan_chunks(Ctx &c, int (*launch)(const A &, int, int, hipStream_t), bool bwd, int l, Fill fill) {
    const SeqDims &s = c.s;
    for (int g0 = 0; g0 < s.groups; g0 += c.cap) {
        A a;
        memset(&a, 0, sizeof(a));
        fill(a);
        a.xch = at<bf16_t>(c.ws, c.w.xch); a.groups_total = s.groups;
        a.flags = at<unsigned>(c.ws, c.w.flags) + flag_words(s, bwd ? 1 : 0, l, g0);
        a.status = at<int>(c.ws, c.w.status);
        a.B = s.B; a.Bp = s.Bp; a.T = s.T; a.groups = s.groups - g0 < c.cap ? s.groups - g0 : c.cap; a.group0 = g0;
        a.rng = c.rng; a.rng.on = masked(c, l) ? 1 : 0;
        a.allow_l2_mode = c.l2_mode; a.spread_groups = c.spread; a.diag_short_grid = c.short_grid;
        ProfScope ps(bwd ? PK_SCAN_BWD : PK_SCAN_FWD, c.st);
        if (const int rc = launch(a, s.H, s.MG, c.st)) return rc;
    }
    return NSD_OK;
}

int forward(Ctx &c, const float *x, bool train) {
    const SeqDims &s = c.s;
    const int H = s.H, G = 4 * H, DH = s.D * H;
    const long R = (long)s.T * s.Bp;
    if (hipMemsetAsync(at<char>(c.ws, c.w.status), 0, (size_t)(c.w.flags + c.w.flags_bytes - c.w.status), c.st) != hipSuccess) {
        nsd_set_error("seq: memset failed"); return NSD_E_LAUNCH;
    }
    {
        ProfScope prep(PK_PREP, c.st);
        if (const int rc = nsd_seq_xbf_launch(x, at<bf16_t>(c.ws, c.w.xbf), s.B, s.Bp, s.T, s.C, s.CP, c.st)) return rc;
        for (int l = 0; l < s.L; ++l)
            for (int d = 0; d < s.D; ++d) {
                PrepArgs p;
                memset(&p, 0, sizeof(p));
                p.w_ih = c.params + c.pl.w_ih[l][d]; p.w_hh = c.params + c.pl.w_hh[l][d];
                p.b_ih = c.params + c.pl.b_ih[l][d]; p.b_hh = c.params + c.pl.b_hh[l][d];
                p.wf = at<bf16_t>(c.ws, c.w.wf[l][d]); p.wb = at<bf16_t>(c.ws, c.w.wb[l][d]); p.wx = at<bf16_t>(c.ws, c.w.wx[l][d]);
                p.wxt = l > 0 ? at<bf16_t>(c.ws, c.w.wxt[l]) : nullptr;
                p.bsum = at<float>(c.ws, c.w.bsum[l][d]);
                p.H = H; p.I = l == 0 ? s.C : DH; p.Ipad = l == 0 ? s.CP : DH; p.wxt_ld = s.D * G; p.wxt_off = d * G;
                if (const int rc = nsd_seq_prep_launch(p, c.st)) return rc;
            }
    }
    if (s.fused2)
        // (no projection GEMM: W_ih0 . x_t is CP / 16 <= 4 MFMAs per step inside the scan -- one launch and a 1-GB tile round trip less)
        return scan_chunks(c, nsd_scan2_fwd_launch, false, 0, [&](Scan2FwdArgs &a) {
            a.wf0 = at<bf16_t>(c.ws, c.w.wf[0][0]); a.wx1 = at<bf16_t>(c.ws, c.w.wx[1][0]); a.wf1 = at<bf16_t>(c.ws, c.w.wf[1][0]);
            a.bsum1 = at<float>(c.ws, c.w.bsum[1][0]);
            a.wx0 = at<bf16_t>(c.ws, c.w.wx[0][0]); a.bsum0 = at<float>(c.ws, c.w.bsum[0][0]); a.xbf = at<bf16_t>(c.ws, c.w.xbf); a.CP = s.CP;
            a.hs0 = at<bf16_t>(c.ws, c.w.hs[0]); a.lk0 = writes_lk(c, 0) ? at<bf16_t>(c.ws, c.w.lk[0]) : nullptr; a.hs1 = at<bf16_t>(c.ws, c.w.hs[1]);
            if (train) {
                a.cs0 = at<bf16_t>(c.ws, c.w.cs[0][0]); a.ga0 = at<bf16_t>(c.ws, c.w.ga[0][0]);
                a.cs1 = at<bf16_t>(c.ws, c.w.cs[1][0]); a.ga1 = at<bf16_t>(c.ws, c.w.ga[1][0]);
            }
        });
    for (int l = 0; l < s.L; ++l) {
        const bf16_t *in = l == 0 ? at<bf16_t>(c.ws, c.w.xbf) : out_of(c, l - 1);
        const int Kin = l == 0 ? s.CP : DH;
        // layer 0 with at most 64 channels: W_ih . x_t is CP / 16 <= 4 MFMAs per step inside the scan (no GEMM, no tile round trip)
        const bool inproj = l == 0 && s.CP <= 64;
        for (int d = 0; d < s.D && !inproj; ++d) {
            GemmArgs g;
            memset(&g, 0, sizeof(g));
            g.A = at<bf16_t>(c.ws, c.w.wx[l][d]); g.lda = Kin; g.B = in; g.ldb = Kin;
            g.C = at<bf16_t>(c.ws, c.w.xproj[d]); g.bias = at<float>(c.ws, c.w.bsum[l][d]);
            g.M = G; g.N = (int)R; g.K = Kin; g.splits = 1; g.epi = GEMM_EPI_TILE_BF16;
            ProfScope ps(PK_GEMM_XPROJ, c.st);
            if (const int rc = nsd_gemm_bf16_launch(g, c.st)) return rc;
        }
        if (const int rc = scan_chunks(c, nsd_scan_fwd_launch, false, l, [&](ScanFwdArgs &a) {
            for (int d = 0; d < s.D; ++d) {
                a.wf[d] = at<bf16_t>(c.ws, c.w.wf[l][d]);
                a.xproj[d] = at<bf16_t>(c.ws, c.w.xproj[d]);
                if (inproj) { a.wx0[d] = at<bf16_t>(c.ws, c.w.wx[0][d]); a.bsum0[d] = at<float>(c.ws, c.w.bsum[0][d]); }
                a.cs[d] = train ? at<bf16_t>(c.ws, c.w.cs[l][d]) : nullptr;
                a.ga[d] = train ? at<bf16_t>(c.ws, c.w.ga[l][d]) : nullptr;
            }
            a.hs = at<bf16_t>(c.ws, c.w.hs[l]);
            a.xbf = at<bf16_t>(c.ws, c.w.xbf); a.CP = s.CP;
            a.lk = writes_lk(c, l) ? at<bf16_t>(c.ws, c.w.lk[l]) : nullptr;
            a.res = (s.residual && l >= 1) ? in : nullptr;
            a.D = s.D; a.ld = DH; a.layer = l;
        })) return rc;
    }
    return NSD_OK;
}

// mode: HEAD_EVAL, or one of the train-mode launches, which draw RReLU slopes and head dropout from c.rng (rng off: eval slope, no dropout)
HeadTmArgs head_args(Ctx &c, int mode, float *logits, float *probs) {
    const SeqDims &s = c.s;
    HeadTmArgs h;
    memset(&h, 0, sizeof(h));
    h.top = out_of(c, s.L - 1);                                  // (the last layer is never multiplied; with the residual extension it is lk)
    h.ln_w = c.params + c.pl.ln_w; h.ln_b = c.params + c.pl.ln_b; h.attn_w = c.params + c.pl.attn_w; h.attn_b = c.params + c.pl.attn_b;
    h.fc0_w = c.params + c.pl.fc0_w; h.fc0_b = c.params + c.pl.fc0_b; h.fc3_w = c.params + c.pl.fc3_w; h.fc3_b = c.params + c.pl.fc3_b;
    h.eval_slope = (float)((0.125 + 1.0 / 3.0) / 2.0);           // nn.RReLU eval slope, lstm_eeg_model.py:27
    h.logits = logits; h.probs = probs;
    h.train = mode != HEAD_EVAL; h.rng = c.rng;
    h.B = s.B; h.Bp = s.Bp; h.T = s.T; h.DH = s.D * s.H; h.F = s.F; h.K = s.K;
    h.status = at<int>(c.ws, c.w.status);
    return h;
}

// The training outputs of the head, which the backward pass reads: alpha, dscore, pooled, dpooled and the per-trial rows.  The
// padding trials' dpooled / dscore are zeroed so that they contribute nothing to any gradient.  (loss, labels and scale stay with
// nsd_seq_train_fwd, the one entry that has them.)
int head_train_outputs(Ctx &c, HeadTmArgs &h) {
    const SeqDims &s = c.s;
    const int DH = s.D * s.H;
    h.alpha = at<float>(c.ws, c.w.alpha); h.dscore = at<float>(c.ws, c.w.dscore);
    h.pooled = at<float>(c.ws, c.w.pooled); h.dpooled = at<float>(c.ws, c.w.dpooled);
    h.hb = at<float>(c.ws, c.w.hb); h.hb_stride = c.w.hb_stride;
    if (s.Bp > s.B &&
        (hipMemsetAsync(h.dpooled + (long)s.B * DH, 0, (size_t)(s.Bp - s.B) * DH * 4, c.st) != hipSuccess ||
         hipMemsetAsync(h.alpha, 0, (size_t)s.T * s.Bp * 4, c.st) != hipSuccess ||
         hipMemsetAsync(h.dscore, 0, (size_t)s.T * s.Bp * 4, c.st) != hipSuccess)) {
        nsd_set_error("%s: memset failed", c.who);
        return NSD_E_LAUNCH;
    }
    return NSD_OK;
}

// dL/dx of the evaluation in `ws` from layer 0's gate gradients (nsd_seq_dx.hip), called once w.da holds them and layer 0's weight
// gradients are formed.  Layer 0 has no residual term (the extension adds the input to the output for l >= 1 only) and no dropout
// on its input, so dx = sum_d da0_d . W_ih0_d and nothing else.
// Scratch: the W_ih0 fragments go to `parts`, the split-K buffer of the weight-gradient GEMMs.  It holds nothing between launches:
// each weight_grads() writes it (GEMM) and consumes it (seq_reduce_dw) before returning, layer 0's is the last of them, and the
// head-gradient reduction that follows overwrites its own scratch there before reading it -- the stream orders all of it.
int input_grad(Ctx &c, float *dx) {
    const SeqDims &s = c.s;
    SeqDx a;
    memset(&a, 0, sizeof(a));
    a.da = at<bf16_t>(c.ws, c.w.da);                             // [T*Bp][D*4H] on both routes (fused: D = 1, layer 0's block)
    for (int d = 0; d < s.D; ++d) a.wx[d] = at<bf16_t>(c.ws, c.w.wx[0][d]);
    a.wfrag = at<bf16_t>(c.ws, c.w.parts);
    a.dx = dx;
    a.B = s.B; a.Bp = s.Bp; a.T = s.T; a.C = s.C; a.CP = s.CP; a.H = s.H; a.D = s.D;
    ProfScope ps(PK_GEMM_DX, c.st);
    return nsd_seq_dx_launch(a, c.st);
}

int backward(Ctx &c, float *grads, float *dx) {
    const SeqDims &s = c.s;
    const int H = s.H, G = 4 * H, DH = s.D * H;
    const long R = (long)s.T * s.Bp;
    float *parts = at<float>(c.ws, c.w.parts);
    // the backward scans' flag sets (rendezvous words, per-wave step counters) start from zero on EVERY backward call: a second
    // nsd_seq_train_bwd on the same forward (retain_graph) would otherwise find last call's counters at T and race through
    const int64_t bwd_sets = flag_words(s, 1, 0, 0) * 4;
    if (hipMemsetAsync(at<char>(c.ws, c.w.flags) + bwd_sets, 0, (size_t)(c.w.flags_bytes - bwd_sets), c.st) != hipSuccess) {
        nsd_set_error("seq: memset failed"); return NSD_E_LAUNCH;
    }
    // contractions over the whole sequence for layer l: dW_hh, dW_ih (split-K, fixed-order reduction), biases from the scan's
    // per-tile sums.  da: [T*Bp][ldda] with direction d in columns d*4H..; dbp: [D][groups][4H]
    auto weight_grads = [&](int l, const bf16_t *da, long ldda, const float *dbp) -> int {
        const bf16_t *in = l == 0 ? at<bf16_t>(c.ws, c.w.xbf) : out_of(c, l - 1);
        const int Kin = l == 0 ? s.CP : DH, I = l == 0 ? s.C : DH;
        for (int d = 0; d < s.D; ++d) {
            ProfScope ps(PK_GEMM_DW, c.st);
            GemmArgs g;
            memset(&g, 0, sizeof(g));
            g.A = da + (long)d * G; g.lda = ldda; g.a_kmajor = 1; g.b_kmajor = 1;
            g.C = parts; g.M = G; g.K = R; g.epi = GEMM_EPI_F32;
            // recurrent weights: operand h_{t-1} of the direction: one time step = 32 rows away inside the batch tile's block of
            // T * 32 rows (tile-major rows); the step before the first of a tile is zero
            g.B = at<bf16_t>(c.ws, c.w.hs[l]) + (long)d * H; g.ldb = DH;
            g.b_shift = d == 0 ? -32 : 32; g.b_period = (long)s.T * 32;
            if (H % 256 == 0 && Kin >= 256 && (G / 256) * ((H + Kin) / 256) <= 16) {
                // ONE pass over da for both gradients: columns [0, H) meet h_{t-1}, columns [H, H + Kin) the layer's input (da does not
                // fit the Infinity Cache: as two launches it is read from HBM twice).  Measured: cfg3's layer 1 (1024 x 512, 8 tiles
                // x 32 slices) 2 x 190 -> 305 us; cfg5's (2048 x 1536: 48 tiles, 5 slices fit the partial-sum buffer) 3.6 -> 4.0 ms,
                // so only where the fused problem still has few tiles and many slices
                g.B2 = in; g.ldb2 = Kin; g.b2_shift = 0; g.n_split = H;
                g.N = H + Kin; g.ldc = H + Kin;
                g.splits = split_count(G, H + Kin, R);
                if (const int rc = nsd_gemm_bf16_launch(g, c.st)) return rc;
                hipLaunchKernelGGL(seq_reduce_dw_kernel, dim3((unsigned)((4L * H * H + 255) / 256)), dim3(256), 0, c.st, parts, g.splits, H, H + Kin, H,
                                   grads + c.pl.w_hh[l][d]);
                hipLaunchKernelGGL(seq_reduce_dw_kernel, dim3((unsigned)((4L * H * I + 255) / 256)), dim3(256), 0, c.st, parts + H, g.splits, H, H + Kin, I,
                                   grads + c.pl.w_ih[l][d]);
            } else {
                g.N = H; g.ldc = H;
                g.splits = split_count(G, H, R);
                if (const int rc = nsd_gemm_bf16_launch(g, c.st)) return rc;
                hipLaunchKernelGGL(seq_reduce_dw_kernel, dim3((unsigned)((4L * H * H + 255) / 256)), dim3(256), 0, c.st, parts, g.splits, H, H, H,
                                   grads + c.pl.w_hh[l][d]);
                // input weights
                g.B = in; g.ldb = Kin; g.N = Kin; g.ldc = Kin; g.b_shift = 0; g.b_period = 0;
                g.splits = split_count(G, Kin, R);
                if (const int rc = nsd_gemm_bf16_launch(g, c.st)) return rc;
                hipLaunchKernelGGL(seq_reduce_dw_kernel, dim3((unsigned)((4L * H * I + 255) / 256)), dim3(256), 0, c.st, parts, g.splits, H, Kin, I,
                                   grads + c.pl.w_ih[l][d]);
            }
            hipLaunchKernelGGL(seq_reduce_db_kernel, dim3((G + 255) / 256), dim3(256), 0, c.st, dbp + (long)d * s.groups * G, s.groups, H,
                               grads + c.pl.b_ih[l][d], grads + c.pl.b_hh[l][d]);
            NSD_CHECK_LAUNCH("seq weight gradients");
        }
        return NSD_OK;
    };
    if (s.fused2) {
        float *dbp0 = at<float>(c.ws, c.w.dbp), *dbp1 = dbp0 + (long)s.groups * G;
        if (const int rc = scan_chunks(c, nsd_scan2_bwd_launch, true, 0, [&](Scan2BwdArgs &a) {
            a.wb0 = at<bf16_t>(c.ws, c.w.wb[0][0]); a.wb1 = at<bf16_t>(c.ws, c.w.wb[1][0]); a.wxt1 = at<bf16_t>(c.ws, c.w.wxt[1]);
            a.cs0 = at<bf16_t>(c.ws, c.w.cs[0][0]); a.ga0 = at<bf16_t>(c.ws, c.w.ga[0][0]);
            a.cs1 = at<bf16_t>(c.ws, c.w.cs[1][0]); a.ga1 = at<bf16_t>(c.ws, c.w.ga[1][0]);
            a.da0 = at<bf16_t>(c.ws, c.w.da); a.da1 = at<bf16_t>(c.ws, c.w.da2); a.dbp0 = dbp0; a.dbp1 = dbp1;
            a.alpha = at<float>(c.ws, c.w.alpha); a.dscore = at<float>(c.ws, c.w.dscore); a.dpooled = at<float>(c.ws, c.w.dpooled);
            a.attn_w = c.params + c.pl.attn_w;
        })) return rc;
        if (const int rc = weight_grads(1, at<bf16_t>(c.ws, c.w.da2), G, dbp1)) return rc;
        if (const int rc = weight_grads(0, at<bf16_t>(c.ws, c.w.da), G, dbp0)) return rc;
        if (dx)
            if (const int rc = input_grad(c, dx)) return rc;
    } else
    for (int l = s.L - 1; l >= 0; --l) {
        if (const int rc = scan_chunks(c, nsd_scan_bwd_launch, true, l, [&](ScanBwdArgs &a) {
            for (int d = 0; d < s.D; ++d) {
                a.wb[d] = at<bf16_t>(c.ws, c.w.wb[l][d]);
                a.cs[d] = at<bf16_t>(c.ws, c.w.cs[l][d]);
                a.ga[d] = at<bf16_t>(c.ws, c.w.ga[l][d]);
            }
            a.da = at<bf16_t>(c.ws, c.w.da);
            // the upstream gradient of a lower layer: bf16 tiles in owner order, or (residual extension) row-major fp32
            a.din = (l == s.L - 1 || !s.residual) ? nullptr : at<float>(c.ws, c.w.din[0]);
            a.din_tiles = (l == s.L - 1 || s.residual) ? nullptr : at<bf16_t>(c.ws, c.w.din[0]);
            a.dres = (s.residual && l >= 1) ? at<float>(c.ws, c.w.din[1]) : nullptr;
            a.alpha = at<float>(c.ws, c.w.alpha); a.dscore = at<float>(c.ws, c.w.dscore); a.dpooled = at<float>(c.ws, c.w.dpooled);
            a.attn_w = c.params + c.pl.attn_w;
            a.dbp = at<float>(c.ws, c.w.dbp);
            a.D = s.D; a.ld = DH; a.layer = l;
        })) return rc;
        if (const int rc = weight_grads(l, at<bf16_t>(c.ws, c.w.da), (long)s.D * G, at<float>(c.ws, c.w.dbp))) return rc;
        if (l == 0 && dx)
            if (const int rc = input_grad(c, dx)) return rc;
        if (l > 0) {                                             // gradient w.r.t. the layer's input, both directions in one contraction
            GemmArgs g;
            memset(&g, 0, sizeof(g));
            if (s.residual) {                                    // row-major fp32 + d(linked output) of this layer (extension)
                g.A = at<bf16_t>(c.ws, c.w.da); g.lda = (long)s.D * G; g.B = at<bf16_t>(c.ws, c.w.wxt[l]); g.ldb = (long)s.D * G;
                g.C = at<float>(c.ws, c.w.din[0]); g.ldc = DH; g.M = (int)R; g.N = DH; g.K = (long)s.D * G; g.splits = 1; g.epi = GEMM_EPI_F32;
                g.add = at<float>(c.ws, c.w.din[1]);
            } else {
                // the TRANSPOSED product d_in^T [D*H, T*Bp] = W_ih^T' . da^T: an accumulator tile is then 32 units x the 32 trials of
                // one (batch tile, step) -- registers 4j..4j+3 of a lane are what lane (trial, half) of wave j of the lower layer's
                // backward scan needs -- written as bf16 in that order (the scan's lanes load 8 contiguous bytes)
                g.A = at<bf16_t>(c.ws, c.w.wxt[l]); g.lda = (long)s.D * G; g.B = at<bf16_t>(c.ws, c.w.da); g.ldb = (long)s.D * G;
                g.C = at<bf16_t>(c.ws, c.w.din[0]); g.ldc = 0; g.M = DH; g.N = (int)R; g.K = (long)s.D * G; g.splits = 1; g.epi = GEMM_EPI_TILE_WAVE_BF16;
            }
            ProfScope ps(PK_GEMM_DIN, c.st);
            if (const int rc = nsd_gemm_bf16_launch(g, c.st)) return rc;
        }
    }
    const long hbs = c.w.hb_stride;
    ProfScope ps(PK_HEAD_GRADS, c.st);
    return nsd_head_tm_grads_launch(at<float>(c.ws, c.w.hb), hbs, s.B, DH, s.F, s.K, parts, grads + c.pl.ln_w, grads + c.pl.ln_b, grads + c.pl.attn_w,
                                    grads + c.pl.attn_b, grads + c.pl.fc0_w, grads + c.pl.fc0_b, grads + c.pl.fc3_w, grads + c.pl.fc3_b, c.st);
}

// Dims and workspace layout of an entry point.  Refusals, in this order: dims and flags; a null workspace or !ptr_ok (the parameters --
// for nsd_seq_loss_sum, which has none, its output); a workspace smaller than nsd_seq_workspace_bytes().
int open_ws(const char *who, const nsd_dims *d, uint32_t flags, const void *ws, int64_t ws_bytes, bool ptr_ok, SeqDims *s, SeqWs *w) {
    if (const int rc = derive(d, flags, s)) return rc;
    *w = make_ws(*s);
    if (!ws || !ptr_ok) { nsd_set_error("%s: null pointer", who); return NSD_E_INVALID; }
    if (ws_bytes < w->total) {
        nsd_set_error("%s: workspace of %lld bytes is smaller than nsd_seq_workspace_bytes() = %lld", who, (long long)ws_bytes, (long long)w->total);
        return NSD_E_WORKSPACE;
    }
    return NSD_OK;
}

// The preamble of every entry point that launches model work.  After open_ws's refusals: the entry's own pointers (own_ptrs), an
// input gradient dx wider than its scratch, the empty batch (EMPTY_BATCH: nothing to launch), the rng (null: streams off).
// An entry leaves with leave(rc) on anything but NSD_OK.
constexpr int EMPTY_BATCH = 1;
int leave(int rc) { return rc == EMPTY_BATCH ? NSD_OK : rc; }
int enter(Ctx *c, const char *who, const nsd_dims *d, uint32_t flags, const float *params, void *ws, int64_t ws_bytes, bool own_ptrs,
          const nsd_rng *rng, void *stream, const float *dx = nullptr) {
    if (const int rc = open_ws(who, d, flags, ws, ws_bytes, params != nullptr, &c->s, &c->w)) return rc;
    if (!own_ptrs) { nsd_set_error("%s: null pointer", who); return NSD_E_INVALID; }
    if (dx && nsd_seq_dx_scratch_bytes(c->s.H, c->s.D, c->s.CP) > PARTS_FLOATS * 4) {
        nsd_set_error("%s: %d input channels exceed the input-gradient scratch", who, c->s.C);
        return NSD_E_INVALID;
    }
    if (d->B == 0) return EMPTY_BATCH;
    memset(&c->rng, 0, sizeof(c->rng));
    if (rng)
        if (const int rc = nsd_rng_args(rng, &c->rng)) return rc;
    c->lstm_drop = c->rng.on && c->rng.thr_lstm != 0;
    c->pl = nsd_seq_make_layout(c->s.C, c->s.H, c->s.L, c->s.K, c->s.F, c->s.D);
    c->ws = ws; c->params = params; c->st = (hipStream_t)stream; c->who = who;
    c->cap = scan_cap(c->s);
    c->l2_mode = (NSD_DIAG && (flags & NSD_DIAG_FLAG_NO_L2_EXCHANGE)) ? 0 : 1;
    c->spread = (NSD_DIAG && (flags & NSD_DIAG_FLAG_SPREAD_GROUPS)) ? 1 : 0;
    c->short_grid = (NSD_DIAG && (flags & NSD_DIAG_FLAG_LOSE_MEMBER)) ? 1 : 0;
    return NSD_OK;
}

// nsd_seq_train_bwd (dx == null) and nsd_seq_train_bwd_dx: the same launches in front of the optional dx contraction, so the same gradients
int train_bwd(const char *who, const nsd_dims *d, const float *params, const nsd_rng *rng, uint32_t flags, void *workspace, int64_t workspace_bytes,
              float *grads, float *dx, void *stream) {
    Ctx c;
    if (const int rc = enter(&c, who, d, flags, params, workspace, workspace_bytes, grads != nullptr, rng, stream, dx)) return leave(rc);
    return backward(c, grads, dx);
}

}  // namespace

SeqParamLayout nsd_seq_make_layout(int C, int H, int L, int K, int F, int D) {
    SeqParamLayout o;
    memset(&o, 0, sizeof(o));
    int64_t p = 0;
    const int DH = D * H;
    for (int l = 0; l < L; ++l) {
        const int I = l == 0 ? C : DH;
        for (int d = 0; d < D; ++d) {                            // torch: all four tensors of a direction, then the _reverse ones
            o.w_ih[l][d] = p; p += 4LL * H * I;
            o.w_hh[l][d] = p; p += 4LL * H * H;
            o.b_ih[l][d] = p; p += 4LL * H;
            o.b_hh[l][d] = p; p += 4LL * H;
        }
    }
    o.lstm_total = p;
    o.ln_w = p; p += DH;   o.ln_b = p; p += DH;
    o.attn_w = p; p += DH; o.attn_b = p; p += 1;
    o.fc0_w = p; p += (int64_t)F * DH; o.fc0_b = p; p += F;
    o.fc3_w = p; p += (int64_t)K * F; o.fc3_b = p; p += K;
    o.total = p;
    return o;
}

extern "C" {

int64_t nsd_seq_param_count(int32_t C, int32_t H, int32_t L, int32_t K, int32_t F, int32_t D) {
    if (C < 1 || H < 1 || L < 1 || L > NSD_MAX_LAYERS || K < 1 || F < 1 || D < 1 || D > NSD_SEQ_MAX_DIRS) {
        nsd_set_error("bad model dims C=%d H=%d L=%d K=%d F=%d D=%d", C, H, L, K, F, D);
        return NSD_E_INVALID;
    }
    return nsd_seq_make_layout(C, H, L, K, F, D).total;
}

int nsd_seq_param_layout(int32_t C, int32_t H, int32_t L, int32_t K, int32_t F, int32_t D, int64_t *offsets) {
    if (nsd_seq_param_count(C, H, L, K, F, D) < 0 || !offsets) return NSD_E_INVALID;
    const SeqParamLayout o = nsd_seq_make_layout(C, H, L, K, F, D);
    int64_t *q = offsets;
    for (int l = 0; l < L; ++l)
        for (int d = 0; d < D; ++d) { *q++ = o.w_ih[l][d]; *q++ = o.w_hh[l][d]; *q++ = o.b_ih[l][d]; *q++ = o.b_hh[l][d]; }
    q[0] = o.ln_w; q[1] = o.ln_b; q[2] = o.attn_w; q[3] = o.attn_b; q[4] = o.fc0_w; q[5] = o.fc0_b; q[6] = o.fc3_w; q[7] = o.fc3_b;
    return NSD_OK;
}

int nsd_seq_supported(const nsd_dims *d, uint32_t flags) {
    SeqDims s;
    return derive(d, flags, &s) == NSD_OK ? 1 : 0;
}

int64_t nsd_seq_workspace_bytes(const nsd_dims *d, uint32_t flags) {
    SeqDims s;
    if (const int rc = derive(d, flags, &s)) return rc;
    return make_ws(s).total;
}

int nsd_seq_infer(const nsd_dims *d, const float *params, const float *x, uint32_t flags, float *logits, float *probs, void *workspace,
                  int64_t workspace_bytes, void *stream) {
    Ctx c;
    if (const int rc = enter(&c, "seq_infer", d, flags, params, workspace, workspace_bytes, x && logits, nullptr, stream)) return leave(rc);
    if (const int rc = forward(c, x, false)) return rc;
    HeadTmArgs h = head_args(c, HEAD_EVAL, logits, probs);
    ProfScope ps(PK_HEAD, c.st);
    return nsd_head_tm_launch(h, HEAD_EVAL, nullptr, c.st);
}

// nsd_seq_train_fwd (labels) and nsd_seq_train_fwd_soft (targets [B][K]): one of the two is given
static int train_fwd(const char *who, const nsd_dims *d, const float *params, const float *x, const nsd_rng *rng, const int32_t *labels,
                     const float *targets, float scale, uint32_t flags, void *workspace, int64_t workspace_bytes, float *logits, void *stream) {
    Ctx c;
    if (const int rc = enter(&c, who, d, flags, params, workspace, workspace_bytes, x && logits && (labels || targets), rng, stream)) return leave(rc);
    if (const int rc = forward(c, x, true)) return rc;
    HeadTmArgs h = head_args(c, HEAD_TRAIN, logits, nullptr);
    h.labels = labels; h.targets = targets; h.scale = scale; h.loss = at<float>(c.ws, c.w.loss);
    if (const int rc = head_train_outputs(c, h)) return rc;
    ProfScope ps(PK_HEAD, c.st);
    return nsd_head_tm_launch(h, HEAD_TRAIN, nullptr, c.st);
}

int nsd_seq_train_fwd(const nsd_dims *d, const float *params, const float *x, const nsd_rng *rng, const int32_t *labels, float scale,
                      uint32_t flags, void *workspace, int64_t workspace_bytes, float *logits, void *stream) {
    return train_fwd("seq_train_fwd", d, params, x, rng, labels, nullptr, scale, flags, workspace, workspace_bytes, logits, stream);
}

int nsd_seq_train_fwd_soft(const nsd_dims *d, const float *params, const float *x, const nsd_rng *rng, const float *targets, float scale,
                           uint32_t flags, void *workspace, int64_t workspace_bytes, float *logits, void *stream) {
    return train_fwd("seq_train_fwd_soft", d, params, x, rng, nullptr, targets, scale, flags, workspace, workspace_bytes, logits, stream);
}

int nsd_seq_train_bwd(const nsd_dims *d, const float *params, const nsd_rng *rng, uint32_t flags, void *workspace, int64_t workspace_bytes,
                      float *grads, void *stream) {
    return train_bwd("seq_train_bwd", d, params, rng, flags, workspace, workspace_bytes, grads, nullptr, stream);
}

// The any-loss sequence: the training forward with activations kept and logits out (no labels, no loss, no head backward) ...
int nsd_seq_train_fwd_logits(const nsd_dims *d, const float *params, const float *x, const nsd_rng *rng, uint32_t flags, void *workspace,
                             int64_t workspace_bytes, float *logits, void *stream) {
    Ctx c;
    if (const int rc = enter(&c, "seq_train_fwd_logits", d, flags, params, workspace, workspace_bytes, x && logits, rng, stream)) return leave(rc);
    if (const int rc = forward(c, x, true)) return rc;
    HeadTmArgs h = head_args(c, HEAD_LOGITS, logits, nullptr);   // the streams of nsd_seq_train_fwd's head: the same logits, bit for bit
    ProfScope ps(PK_HEAD, c.st);
    return nsd_head_tm_launch(h, HEAD_LOGITS, nullptr, c.st);
}

// ... the head backward from the caller's dlogits, recomputed from the saved top-layer sequence with the forward's streams: it leaves
// what nsd_seq_train_fwd's fused head backward leaves (alpha, dscore, pooled, dpooled, the per-trial rows, zeros for padding trials),
// so nsd_seq_train_bwd[_dx] then gives the gradients of that loss.  Valid after either forward.
int nsd_seq_head_bwd(const nsd_dims *d, const float *params, const nsd_rng *rng, const float *dlogits, uint32_t flags, void *workspace,
                     int64_t workspace_bytes, void *stream) {
    Ctx c;
    if (const int rc = enter(&c, "seq_head_bwd", d, flags, params, workspace, workspace_bytes, dlogits != nullptr, rng, stream)) return leave(rc);
    HeadTmArgs h = head_args(c, HEAD_DLOG, nullptr, nullptr);
    if (const int rc = head_train_outputs(c, h)) return rc;
    ProfScope ps(PK_HEAD_BWD, c.st);
    return nsd_head_tm_launch(h, HEAD_DLOG, dlogits, c.st);
}

// nsd_seq_train_bwd plus dx[B][T][C] (fp32) when dx != null; the parameter gradients are nsd_seq_train_bwd's, bit for bit
int nsd_seq_train_bwd_dx(const nsd_dims *d, const float *params, const nsd_rng *rng, uint32_t flags, void *workspace, int64_t workspace_bytes,
                         float *grads, float *dx, void *stream) {
    return train_bwd("seq_train_bwd_dx", d, params, rng, flags, workspace, workspace_bytes, grads, dx, stream);
}

// (reads the workspace only: no parameters, and an empty batch still gets its sum, 0)
int nsd_seq_loss_sum(const nsd_dims *d, uint32_t flags, const void *workspace, int64_t workspace_bytes, float *out, void *stream) {
    SeqDims s;
    SeqWs w;
    if (const int rc = open_ws("seq_loss_sum", d, flags, workspace, workspace_bytes, out != nullptr, &s, &w)) return rc;
    return nsd_loss_sum_launch(reinterpret_cast<const float *>(reinterpret_cast<const char *>(workspace) + w.loss), s.B, 1, false, out, "loss_sum", (hipStream_t)stream);
}

// Zero the persistent header of a freshly allocated workspace (the sticky status word).  Call once per allocation; an
// uninitialised header reads as a failure, never as success.
int nsd_seq_workspace_init(void *workspace, int64_t workspace_bytes, void *stream) {
    if (!workspace) { nsd_set_error("seq_workspace_init: null pointer"); return NSD_E_INVALID; }
    if (workspace_bytes < NSD_SEQ_HEADER_BYTES + NSD_SEQ_STATUS_WORDS * 4) { nsd_set_error("seq_workspace_init: workspace too small"); return NSD_E_WORKSPACE; }
    if (hipMemsetAsync(workspace, 0, NSD_SEQ_HEADER_BYTES + NSD_SEQ_STATUS_WORDS * 4, (hipStream_t)stream) != hipSuccess) {
        nsd_set_error("seq_workspace_init: %s", hipGetErrorString(hipGetLastError()));
        return NSD_E_LAUNCH;
    }
    return NSD_OK;
}

// Blocking read of the path's status: status_out[0] = code of the evaluation in flight OR the sticky word (0 = ok, bit 0 / bit 1 =
// a forward / backward scan group gave up waiting for a member: a workgroup of the group was not resident, or the device was
// lost), [1] = the sticky word alone (every code since nsd_seq_workspace_init), [2] / [3] = scan groups on one XCD / spread.
int nsd_seq_status(const void *workspace, int32_t *status_out, void *stream) {
    if (!workspace || !status_out) { nsd_set_error("seq_status: null pointer"); return NSD_E_INVALID; }
    int32_t sticky = 0, cur[4] = {0, 0, 0, 0};
    const char *base = reinterpret_cast<const char *>(workspace);
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess ||
        hipMemcpy(&sticky, base, sizeof(sticky), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(cur, base + NSD_SEQ_HEADER_BYTES, sizeof(cur), hipMemcpyDeviceToHost) != hipSuccess) {
        nsd_set_error("seq_status: %s", hipGetErrorString(hipGetLastError()));
        return NSD_E_LAUNCH;
    }
    status_out[0] = cur[0] | sticky; status_out[1] = sticky; status_out[2] = cur[2]; status_out[3] = cur[3];
    return NSD_OK;
}

// flag_out[0] (device, fp32) = 1 if the workspace reports a scan time-out (current or sticky), else 0; enqueued, never blocks.
// The trainer appends the flag to the flat gradient it all-reduces, so that EVERY rank skips the update when ANY rank failed.
int nsd_seq_guard(const void *workspace, float *flag_out, void *stream) {
    if (!workspace || !flag_out) { nsd_set_error("seq_guard: null pointer"); return NSD_E_INVALID; }
    return nsd_seq_guard_launch(reinterpret_cast<const int *>(workspace), NSD_SEQ_HEADER_WORDS, flag_out, (hipStream_t)stream);
}

#if NSD_DIAG
// Diagnostic build only (nsd_diag.h).  enable != 0 starts recording HIP events (on the launch stream) around the kernels of
// every following nsd_seq_* call, 0 stops and discards.  nsd_seq_profile_read sums one kind and forgets its records
// (BLOCKING: waits for those events).  kind: 0 forward scan, 1 backward scan, 2 input-projection GEMM, 3 weight-gradient
// GEMMs (+ their reductions), 4 input-gradient GEMM, 5 head, 6 head parameter gradients, 7 operand preparation, 8 dL/dx contraction
// (nsd_seq_train_bwd_dx), 9 head backward from dlogits (nsd_seq_head_bwd).
int nsd_seq_profile(int32_t enable) {
    for (ProfRec &r : g_prof.recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    g_prof.recs.clear();
    g_prof.on = enable != 0;
    return NSD_OK;
}
int nsd_seq_profile_read(int32_t kind, float *total_ms, int32_t *count) {
    if (kind < 0 || kind >= PK_COUNT || !total_ms || !count) { nsd_set_error("seq_profile_read: bad argument"); return NSD_E_INVALID; }
    float tot = 0.f; int n = 0;
    std::vector<ProfRec> keep;
    for (ProfRec &r : g_prof.recs) {
        if (r.kind != kind) { keep.push_back(r); continue; }
        float ms = 0.f;
        if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { tot += ms; ++n; }
        (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b);
    }
    g_prof.recs.swap(keep);
    *total_ms = tot; *count = n;
    return NSD_OK;
}
// The GEMM with every field of GemmArgs and a pinned kernel; the two reductions of weight_grads alone (nsd_diag.h).
int nsd_diag_gemm_bf16(const nsd_diag_gemm *p, void *stream) {
    if (!p) { nsd_set_error("diag_gemm_bf16: null arguments"); return NSD_E_INVALID; }
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = (const bf16_t *)p->A; g.B = (const bf16_t *)p->B; g.lda = p->lda; g.ldb = p->ldb; g.a_kmajor = p->a_kmajor; g.b_kmajor = p->b_kmajor;
    g.b_shift = p->b_shift; g.b_period = p->b_period;
    g.B2 = (const bf16_t *)p->B2; g.ldb2 = p->ldb2; g.b2_shift = p->b2_shift; g.n_split = p->n_split;
    g.C = p->C; g.ldc = p->ldc; g.bias = p->bias; g.add = p->add; g.M = p->M; g.N = p->N; g.K = p->K; g.splits = p->splits; g.epi = p->epilogue;
    return nsd_gemm_bf16_launch(g, (hipStream_t)stream, p->kernel);
}
int nsd_diag_reduce_dw(const float *part, int32_t nparts, int32_t H, int32_t N, int32_t I, float *out, void *stream) {
    if (!part || !out || nparts < 1 || H < 1 || I < 1 || I > N) { nsd_set_error("diag_reduce_dw: null pointer or bad sizes"); return NSD_E_INVALID; }
    hipLaunchKernelGGL(seq_reduce_dw_kernel, dim3((unsigned)((4L * H * I + 255) / 256)), dim3(256), 0, (hipStream_t)stream, part, nparts, H, N, I, out);
    NSD_CHECK_LAUNCH("seq_reduce_dw_kernel");
    return NSD_OK;
}
int nsd_diag_reduce_db(const float *part, int32_t nparts, int32_t H, float *b_ih, float *b_hh, void *stream) {
    if (!part || !b_ih || !b_hh || nparts < 1 || H < 1) { nsd_set_error("diag_reduce_db: null pointer or bad sizes"); return NSD_E_INVALID; }
    hipLaunchKernelGGL(seq_reduce_db_kernel, dim3((unsigned)((4 * H + 255) / 256)), dim3(256), 0, (hipStream_t)stream, part, nparts, H, b_ih, b_hh);
    NSD_CHECK_LAUNCH("seq_reduce_db_kernel");
    return NSD_OK;
}
#endif

}  // extern "C"
