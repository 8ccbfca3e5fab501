// nsd_common.h -- shared host/device helpers of libnsd_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/nsd.h"

// ---------------------------------------------------------------------------------------------
// host side: error text + parameter layout
// ---------------------------------------------------------------------------------------------
void nsd_set_error(const char *fmt, ...);

struct ParamLayout {
    int64_t w_ih[NSD_MAX_LAYERS], w_hh[NSD_MAX_LAYERS], b_ih[NSD_MAX_LAYERS], b_hh[NSD_MAX_LAYERS];
    int64_t ln_w, ln_b, attn_w, attn_b, fc0_w, fc0_b, fc3_w, fc3_b, total;
    int64_t lstm_total;   // floats belonging to the LSTM stack (prefix of the vector)
};
ParamLayout nsd_make_layout(int C, int H, int L, int K, int F);
int nsd_check_dims(const nsd_dims *d);
int nsd_num_cus();

#define NSD_CHECK_LAUNCH(name)                                                        \
    do {                                                                              \
        hipError_t e_ = hipGetLastError();                                            \
        if (e_ != hipSuccess) {                                                       \
            nsd_set_error("%s: launch failed: %s", name, hipGetErrorString(e_));      \
            return NSD_E_LAUNCH;                                                      \
        }                                                                             \
    } while (0)

// ---------------------------------------------------------------------------------------------
// device side
// ---------------------------------------------------------------------------------------------
#define LOG2E_F 1.44269504088896340736f

// quad (4 adjacent lanes) cross-lane moves via DPP quad_perm: no LDS, no latency beyond a VALU op.
template <int CTRL>
__device__ __forceinline__ float dpp_quad(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, true));
}
#define QP(a, b, c, d) ((a) | ((b) << 2) | ((c) << 4) | ((d) << 6))
__device__ __forceinline__ float quad_xor1(float v) { return dpp_quad<QP(1, 0, 3, 2)>(v); }
__device__ __forceinline__ float quad_xor2(float v) { return dpp_quad<QP(2, 3, 0, 1)>(v); }
template <int Q>
__device__ __forceinline__ float quad_bcast(float v) { return dpp_quad<QP(Q, Q, Q, Q)>(v); }
__device__ __forceinline__ float quad_sum(float v) {
    v += quad_xor1(v);
    v += quad_xor2(v);
    return v;
}

// Reduce-scatter of four pair accumulators over a quad: lane s returns the sum, over the quad's four lanes, of the value it OWNS.
// Ownership rule: slot i of lane s holds gate (or output unit) i ^ s -- the weights are loaded that way once, in front of the time
// loop -- so slot 0 is always the lane's own value, and the slot a lane needs from its partner is a fixed one: partner s ^ 1 keeps
// value 1 ^ (s ^ 1) = s in its slot 1 (and 2 ^ s, my slot 2, in its slot 3); after that stage ra is value s and rb is value 2 ^ s
// over lanes {s, s ^ 1}, and partner s ^ 2 keeps value 2 ^ (s ^ 2) = s in its rb.  Four pair sums and three DPP adds, no select by
// lane.  With every lane keeping value g in slot g the same sums take six selects (odd ? r1 : r0 ...); each addition here has the
// two operands it has there -- (own + lane s^1) + (lane s^2 + lane s^3) of the same pair sums -- so the results are the same bits.
typedef float nsd_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float quad_reduce_scatter(const nsd_f32x2 (&acc)[4]) {
    const float r0 = acc[0].x + acc[0].y, r1 = acc[1].x + acc[1].y;
    const float r2 = acc[2].x + acc[2].y, r3 = acc[3].x + acc[3].y;
    const float ra = r0 + quad_xor1(r1);
    const float rb = r2 + quad_xor1(r3);
    return ra + quad_xor2(rb);
}

// rotation inside a row of 16 lanes (DPP row_ror:N): lane i receives the value of lane (i + N) % 16 or (i - N) % 16 --
// only used in sums over all rotations by a multiple of 4, where the direction does not matter
template <int N>
__device__ __forceinline__ float row_ror(float v) { return dpp_quad<0x120 + N>(v); }

// sigma(x) = 1/(1+2^(-x*log2e)); tanh(x) = 2*sigma(2x) - 1.  v_exp_f32 / v_rcp_f32 (1 ulp each).
__device__ __forceinline__ float fast_sigmoid(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-LOG2E_F * x));
}
__device__ __forceinline__ float fast_tanh(float x) {
    return fmaf(2.0f, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-2.0f * LOG2E_F * x)), -1.0f);
}
// unified gate activation: a*rcp(1+exp2(b*x))+c with per-lane constants (sigmoid: 1,-log2e,0; tanh: 2,-2log2e,-1)
__device__ __forceinline__ float gate_act(float x, float a, float b, float c) {
    return fmaf(a, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(b * x)), c);
}

// wave64 reductions (all lanes get the result): DPP inside a row of 16 lanes (quad xor 1/2, half-row mirror, row
// mirror -- each an all-reduce step because both partners end up with the same value), then the four row totals
// through v_readlane.  No LDS crossbar (ds_bpermute) on the way: ~10 short instructions instead of 6 LDS round trips.
__device__ __forceinline__ float rows_combine_sum(float v) {      // v uniform inside each row of 16
    const float a0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float a1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float a2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float a3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return (a0 + a1) + (a2 + a3);
}
__device__ __forceinline__ float rows_combine_max(float v) {
    const float a0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float a1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float a2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float a3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return fmaxf(fmaxf(a0, a1), fmaxf(a2, a3));
}
__device__ __forceinline__ float oct_sum(float v) {               // all-reduce over aligned groups of 8 lanes
    v += quad_xor1(v);
    v += quad_xor2(v);
    v += dpp_quad<0x141>(v);                                      // row_half_mirror: lane i <-> 7 - i
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
    v = oct_sum(v);
    v += dpp_quad<0x140>(v);                                      // row_mirror: lane i <-> 15 - i
    return rows_combine_sum(v);
}
__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, quad_xor1(v));
    v = fmaxf(v, quad_xor2(v));
    v = fmaxf(v, dpp_quad<0x141>(v));
    v = fmaxf(v, dpp_quad<0x140>(v));
    return rows_combine_max(v);
}

// Soft-target cross-entropy of one trial by one wave (the `_soft` entry points of nsd.h): lane k < K holds its class's target q (>= 0),
// logit lg and e = exp(lg - m), d = sum_k e_k; lanes >= K hold q = 0, e = 0.  Returns s p_k - q_k (s = sum_j q_j, p = e / d) formed as
// (sum_{j != k} (q_j e_k - q_k e_j)) / d: with a one-hot q that is the hard path's -(sum of the others) / d for the label and e_k / d for
// the rest -- no O(1) - O(1) difference anywhere.  *loss = sum_k q_k ((m - lg_k) + log d) over the lanes < K (the others hold -inf logits).
__device__ __forceinline__ float soft_ce_wave(const float q, const float lg, const float m, const float e, const float d, const float logd,
                                              const int lane, const int K, float *loss) {
    float num = 0.f;
    for (int j = 0; j < K; ++j) {
        const float qj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q), j));
        const float ej = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e), j));
        const float term = qj * e - q * ej;
        num += j == lane ? 0.f : term;
    }
    *loss = wave_sum(lane < K ? q * ((m - lg) + logd) : 0.f);
    return num / d;
}
// the same for one thread that holds all K classes (the LDS-resident heads of nsd_head.hip): dl[k] = scale (s p_k - q_k), returns the loss
__device__ __forceinline__ float soft_ce_thread(const float *q, const float *lg, const int K, const float scale, float *dl) {
    float m = lg[0];
    for (int k = 1; k < K; ++k) m = fmaxf(m, lg[k]);
    float d = 0.f;
    for (int k = 0; k < K; ++k) d += expf(lg[k] - m);
    const float logd = logf(d);
    float loss = 0.f;
    for (int k = 0; k < K; ++k) {
        const float ek = expf(lg[k] - m), qk = q[k];
        float num = 0.f;
        for (int j = 0; j < K; ++j)
            if (j != k) num += q[j] * ek - qk * expf(lg[j] - m);
        dl[k] = num / d * scale;
        loss += qk * ((m - lg[k]) + logd);
    }
    return loss;
}
// and with the label y in place of the targets: dl[k] = scale (p_k - [k == y]), where for the label class p_y - 1 = -(sum_{k != y} e_k) / d
// (no cancellation); returns the loss -log p_y
__device__ __forceinline__ float hard_ce_thread(const int y, const float *lg, const int K, const float scale, float *dl) {
    float m = lg[0];
    for (int k = 1; k < K; ++k) m = fmaxf(m, lg[k]);
    float d = 0.f, rest = 0.f;
    for (int k = 0; k < K; ++k) { const float e = expf(lg[k] - m); d += e; if (k != y) rest += e; }
    for (int k = 0; k < K; ++k) dl[k] = (k == y ? -rest / d : expf(lg[k] - m) / d) * scale;
    return -((lg[y] - m) - logf(d));
}

// A called function sees the kernel's argument block through a pointer: what it loads from there sits in VGPRs, and hipcc cannot know that
// every lane holds the same value -- buffer descriptors built from such pointers are used inside WATERFALL loops (one pass per distinct
// value, a vmcnt(0) in front), loop bounds become vector compares.  uniform_copy() hands every dword through v_readfirstlane: scalar again.
template <class A>
__device__ __forceinline__ A uniform_copy(const A &in) {
    static_assert(sizeof(A) % 4 == 0, "argument block: whole dwords");
    A out;
    const unsigned *s = reinterpret_cast<const unsigned *>(&in);
    unsigned *d = reinterpret_cast<unsigned *>(&out);
#pragma unroll
    for (unsigned i = 0; i < sizeof(A) / 4; ++i) d[i] = __builtin_amdgcn_readfirstlane(s[i]);
    return out;
}

// The dense head's weights -> LDS once per workgroup (fc.0 [F][H] with row stride W0S, fc.3 [K][F] as it is), by ONE wave, sixteen requests
// of a lane in flight at a time.  (As `for (e = lane; e < n; e += 64) lds[..] = w[e]` hipcc emits one load, a full wait and one LDS
// write per trip: 26 round trips to the L2 in front of the workgroup's first step barrier, ~14 us of a launch.)
template <int HH, int W0S>
__device__ __forceinline__ void stage_head_weights(const float *fc0_w, const float *fc3_w, const int F, const int K, float *w0, float *w3, const int lane) {
    typedef const __attribute__((address_space(1))) float *gw_p;
    const int n0 = F * HH, n3 = K * F;
    for (int e0 = 0; e0 < n0; e0 += 64 * 16) {
        float v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) { const int e = e0 + lane + 64 * i; v[i] = ((gw_p)fc0_w)[e < n0 ? e : 0]; }
#pragma unroll
        for (int i = 0; i < 16; ++i) { const int e = e0 + lane + 64 * i; if (e < n0) { const int f = e / HH; w0[f * W0S + (e - f * HH)] = v[i]; } }
    }
    for (int e0 = 0; e0 < n3; e0 += 64 * 8) {
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) { const int e = e0 + lane + 64 * i; v[i] = ((gw_p)fc3_w)[e < n3 ? e : 0]; }
#pragma unroll
        for (int i = 0; i < 8; ++i) { const int e = e0 + lane + 64 * i; if (e < n3) w3[e] = v[i]; }
    }
}

// The eval-mode readout of a pooled prefix by ONE wave (the inference tail of nsd_lstm2_fwd48.hip, nsd_stream48.hip): LayerNorm (biased
// variance, eps in the sqrt), fc.0 -> RReLU(eval) -> fc.3, and the softmax over classes when probs is not null.  Lane j < HH holds
// p = pooled[j], the others 0; vec: 64 floats of LDS; row b of logits / probs is written when b < B.  A: an argument struct with
// ln_w .. fc3_b, eval_slope, K, F (F, K <= 64).
template <int HH, class A>
__device__ __forceinline__ void prefix_readout(const A &a, const float p, float *vec, float *logits, float *probs, const int b, const int B,
                                               const int lane) {
    const int K = a.K, F = a.F;
    const float mu = wave_sum(p) * (1.0f / HH);
    const float dlt = lane < HH ? p - mu : 0.f;
    const float rstd = 1.0f / sqrtf(wave_sum(dlt * dlt) * (1.0f / HH) + 1e-5f);
    if (lane < HH) vec[lane] = dlt * rstd * a.ln_w[lane] + a.ln_b[lane];
    float z = 0.f;
    if (lane < F) {
        float acc = a.fc0_b[lane];
        const float *w = a.fc0_w + (size_t)lane * HH;
#pragma unroll 8
        for (int j = 0; j < HH; ++j) acc = fmaf(w[j], vec[j], acc);
        z = acc >= 0.f ? acc : acc * a.eval_slope;
    }
    if (lane < F) vec[lane] = z;                              // all reads of the LayerNorm vector are done (same wave, in order)
    float lg = -INFINITY;
    if (lane < K) {
        float acc = a.fc3_b[lane];
        const float *w = a.fc3_w + (size_t)lane * F;
        for (int f = 0; f < F; ++f) acc = fmaf(w[f], vec[f], acc);
        lg = acc;
        if (b < B) logits[(size_t)b * K + lane] = acc;
    }
    if (probs) {
        const float mx = wave_max(lg);
        const float e = lane < K ? __expf(lg - mx) : 0.f;
        const float d = wave_sum(e);
        if (lane < K && b < B) probs[(size_t)b * K + lane] = e / d;
    }
}

// in-kernel train-mode streams (see nsd_rng in nsd.h): thresholds and keep factors precomputed on the host
struct RngArgs {
    uint64_t seed;
    uint32_t base;            // stream ids base, base+1, base+2
    uint32_t thr_lstm, thr_head;
    float keep_lstm, keep_head;
    int on;
};
static inline uint32_t nsd_drop_threshold(float p) {
    double t = (double)p * 4294967296.0;
    if (t > 4294967295.0) t = 4294967295.0;
    return (uint32_t)t;
}
// nsd_rng (nsd.h) -> RngArgs with the streams on.  r is not null: whether a null nsd_rng means "off" or is an error is the caller's decision
static inline int nsd_rng_args(const nsd_rng *r, RngArgs *out) {
    if (!(r->p_lstm >= 0.f && r->p_lstm < 1.f) || !(r->p_head >= 0.f && r->p_head < 1.f)) { nsd_set_error("rng: p out of [0,1)"); return NSD_E_INVALID; }
    out->seed = r->seed; out->base = r->base_stream;
    out->thr_lstm = nsd_drop_threshold(r->p_lstm); out->thr_head = nsd_drop_threshold(r->p_head);
    out->keep_lstm = 1.0f / (1.0f - r->p_lstm); out->keep_head = 1.0f / (1.0f - r->p_head);
    out->on = 1;
    return NSD_OK;
}

// counter-based random stream shared bit-for-bit with oracle/nsd_oracle.c (nsd_oracle_rand_u32)
__host__ __device__ __forceinline__ uint32_t nsd_mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16; return x;
}
__host__ __device__ __forceinline__ uint32_t nsd_rand_u32(uint64_t seed, uint32_t stream, uint64_t index) {
    uint32_t lo = (uint32_t)index, hi = (uint32_t)(index >> 32);
    uint32_t s0 = (uint32_t)seed, s1 = (uint32_t)(seed >> 32);
    uint32_t h = nsd_mix32(lo ^ s0);
    h = nsd_mix32(h + 0x9e3779b9U * (stream + 1u) + hi);
    h = nsd_mix32(h ^ s1);
    return h;
}
