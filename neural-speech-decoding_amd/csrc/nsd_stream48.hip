// nsd_stream48.hip -- resumable inference of the two-layer H=48 model (gfx950): nsd_stream_step / nsd_stream_reset of nsd.h.
//
// EEG_LSTM.forward in eval mode (Neuro-Alpha-App/Utilities/lstm_eeg_model.py:32-39) and the class softmax of SimplePredictor.predict
// (:97), cut along time: a call advances B independent streams by a chunk of T samples each, from and to a small per-stream state
// (h, c of both layers and the attention pooling's running max / denominator / weighted sum: STREAM_* of nsd_args.h), and may read
// the decision of the prefix seen so far.  The model is causal -- two forward LSTM layers, a softmax pooling over time that the
// one-shot inference tail already forms online -- so the prefix decision is what nsd_infer gives on the first t samples.
//
// One workgroup = one stream at a time (it loops when there are more streams than workgroups; the weights stay in VGPRs), ten waves,
// one barrier per macro step, operands through LDS, as in nsd_lstm2_fwd48.hip.  At macro step m of a chunk
//   waves 0..2  "L0"    layer 0, step m       : W_ih0 x + W_hh0 h0, cell update
//   waves 3..5  "P"     layer-1 input projection of step m-1 : W_ih1 h0
//   waves 6..8  "L1"    layer 1, step m-2     : W_hh1 h1 + P, cell update, top = h1 (+ h0 with the residual extension)
//   wave  9     "pool"  attention pooling of step m-3, ONE STEP AT A TIME in a fixed order: a 48-term dot product (fixed reduction
//                       tree), new running max, two exponentials, one scaled accumulate.  It also stages x through LDS, 32 steps
//                       ahead (loads issued at one step, written to LDS sixteen steps later: no wait on the recurrence).
// A chunk of T steps takes T + 3 macro steps: the last three DRAIN the skew between the roles, so that every part of the stored
// state is that of the same step.  Every step's arithmetic is the same instruction sequence whatever its place in the chunk, so the
// state after t samples is a function of the samples alone, not of how they were cut.
// Thread (unit j, k-slice s) in the chain roles: 4 gates x 12 (+2) weights in VGPRs, DPP quad reduction, lane s evaluates gate s.
//
// The step is one source that two kernels are compiled from: stream48_kernel (one model, this file) and multi_stream48_kernel (M
// models of one shape per launch: nsd_multi_stream_step; compiled as nsd_multi_stream48.hip, which includes this file with
// NSD_MULTI_TU set, so that the single-model kernels' module is what it was).  The model-batched kernel works on a model view
// (nsd_multi.h): pointers moved to its model, the workgroup index and count taken inside the model.
#include "nsd_multi.h"

namespace {

constexpr int H = 48;
constexpr int KS = 12;
constexpr int NT = 640;      // 10 waves
constexpr int XCH = 32;
constexpr int SKEW = 3;      // macro steps the pooling runs behind layer 0
typedef float f32x2 __attribute__((ext_vector_type(2)));

struct SSmem {
    float xs[2][XCH][8];     // staged samples, channels zero-padded to 8
    float h0[4][H];          // layer 0's h of step t in row t & 3 (L1 reads it two steps later for the residual)
    float pb[2][4 * H];      // layer-1 input projection, [gate*48 + unit]
    float h1[2][H];
    float top[2][H];         // what the pooling reads
    float vec[64];           // readout: LayerNorm output / activated fc.0 output
};

__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }

__device__ __forceinline__ void load_slice(const float *p, f32x2 (&v)[6]) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const float4 u = *reinterpret_cast<const float4 *>(p + 4 * q);
        v[2 * q] = (f32x2){u.x, u.y};
        v[2 * q + 1] = (f32x2){u.z, u.w};
    }
}

// gate pre-activations of unit j, reduced over the 4 k-slices of the quad: quad_reduce_scatter (nsd_common.h).  Slot g of lane s holds
// gate g ^ s (the weights are loaded that way), lane s returns the sum of gate s

// lane s holds the pre-activation of gate s (i, f, g, o) of its unit; all four lanes of the quad return the same c and h
__device__ __forceinline__ float cell_step(const float pre, float &c, const float ga, const float gb, const float gc) {
    const float act = gate_act(pre, ga, gb, gc);
    const float ig = quad_bcast<0>(act), fg = quad_bcast<1>(act), gg = quad_bcast<2>(act), og = quad_bcast<3>(act);
    c = fg * c + ig * gg;
    return og * fast_tanh(c);
}

// element (tl = lane >> 1, channels 4 (lane & 1) ..) of the 32-step chunk that starts at t0; a sample that is not finite enters as NaN
// (an infinity times a weight can come out finite behind a sigmoid: the stream would look healthy)
__device__ __forceinline__ void chunk_x(const StreamArgs &a, const int b, const int t0, const int lane, float (&v)[4]) {
    const int t = t0 + (lane >> 1), ch0 = 4 * (lane & 1);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        float w = 0.f;
        if (t < a.T && ch0 + u < a.C) {
            w = a.x[((size_t)b * a.T + t) * a.C + ch0 + u];
            if ((__float_as_uint(w) & 0x7f800000u) == 0x7f800000u) w = __uint_as_float(0x7fc00000u);
        }
        v[u] = w;
    }
}

// The step's one source, compiled as two kernels.  STREAM48_KERNEL: the kernel's name and parameters; STREAM48_VIEW: what `a` is --
// the argument block itself (the workgroups of the grid share its B streams: wg_id / wg_count are blockIdx.x / gridDim.x) or the view
// of the workgroup's model (the workgroups of one model share them).  A macro rather than a template body: the single-model kernel
// keeps its text, and with it its machine code (tools/isa_digest.py)
#if !NSD_MULTI_TU
#define STREAM48_KERNEL stream48_kernel(const StreamArgs a)
#define STREAM48_VIEW
#else
// workgroup blockIdx.x runs model blockIdx.x / s.G: params + m*P, x + m*x_stride, state + m*S*STREAM_STRIDE, output rows + m*B*K
__device__ __forceinline__ ModelView<StreamArgs> model_view(const StreamArgs &a, const ModelSplit &s) {
    using nsd_multi_detail::mv;
    const int m = nsd_multi_detail::model_of_block(s);
    ModelView<StreamArgs> v;
    static_cast<StreamArgs &>(v) = a;
    v.wg = (int)blockIdx.x - m * s.G;
    v.nwg = s.G;
    const size_t P = (size_t)s.P * m, bk = (size_t)m * a.B * a.K;
    v.x = a.x + (size_t)s.x_stride * m;
    v.w_ih0 = a.w_ih0 + P; v.w_hh0 = a.w_hh0 + P; v.b_ih0 = a.b_ih0 + P; v.b_hh0 = a.b_hh0 + P;
    v.w_ih1 = a.w_ih1 + P; v.w_hh1 = a.w_hh1 + P; v.b_ih1 = a.b_ih1 + P; v.b_hh1 = a.b_hh1 + P;
    v.attn_w = a.attn_w + P; v.attn_b = a.attn_b + P; v.ln_w = a.ln_w + P; v.ln_b = a.ln_b + P;
    v.fc0_w = a.fc0_w + P; v.fc0_b = a.fc0_b + P; v.fc3_w = a.fc3_w + P; v.fc3_b = a.fc3_b + P;
    v.state = a.state + (size_t)m * a.S * STREAM_STRIDE;
    v.logits = mv(a.logits, bk); v.probs = mv(a.probs, bk);
    return v;
}
#define STREAM48_KERNEL multi_stream48_kernel(const StreamArgs a_in, const ModelSplit ms)
#define STREAM48_VIEW const ModelView<StreamArgs> a = model_view(a_in, ms);
#endif

__global__ __launch_bounds__(NT) void STREAM48_KERNEL {
    STREAM48_VIEW
    __shared__ SSmem sm;
    const int tid = threadIdx.x, lane = tid & 63;
    const int role = tid / 192;              // 0 L0, 1 P, 2 L1, 3 pool (wave-uniform: 192 = 3 waves)
    const int r = tid - role * 192, j = r >> 2, s = r & 3;
    const int T = a.T, C = a.C, K = a.K;

    // ---- weights of this thread's role, once per launch ----
    f32x2 w[4][6], wx[4];
    float bias = 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        wx[g] = (f32x2){0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 6; ++q) w[g][q] = (f32x2){0.f, 0.f};
    }
    if (role < 3) {
        const float *W = role == 0 ? a.w_hh0 : role == 1 ? a.w_ih1 : a.w_hh1;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int row = (g ^ s) * H + j;             // slot g: gate g ^ s
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                w[g][q].x = W[(size_t)row * H + s * KS + 2 * q];
                w[g][q].y = W[(size_t)row * H + s * KS + 2 * q + 1];
            }
            if (role == 0) {
                wx[g].x = (2 * s < C) ? a.w_ih0[(size_t)row * C + 2 * s] : 0.f;
                wx[g].y = (2 * s + 1 < C) ? a.w_ih0[(size_t)row * C + 2 * s + 1] : 0.f;
            }
        }
        if (role == 0) bias = a.b_ih0[s * H + j] + a.b_hh0[s * H + j];
        if (role == 2) bias = a.b_ih1[s * H + j] + a.b_hh1[s * H + j];
    }
    // gate s: sigmoid (i, f, o) or tanh (g) as a * rcp(1 + exp2(b x)) + c
    const float ga = s == 2 ? 2.f : 1.f, gb = s == 2 ? -2.f * LOG2E_F : -LOG2E_F, gc = s == 2 ? -1.f : 0.f;
    const float aw = (role == 3 && lane < H) ? a.attn_w[lane] : 0.f;
    const float ab = a.attn_b[0];
    const bool res = a.residual != 0;

    for (int b = wg_id(a); b < a.B; b += wg_count(a)) {
        const int slot = a.slots ? a.slots[b] : b;
        if ((unsigned)slot >= (unsigned)a.S) {           // (the same for every thread of the workgroup) skipped: NaN outputs, no state touched
            if (a.logits && tid < K) {
                a.logits[(size_t)b * K + tid] = __uint_as_float(0x7fc00000u);
                if (a.probs) a.probs[(size_t)b * K + tid] = __uint_as_float(0x7fc00000u);
            }
            continue;
        }
        float *st = a.state + (size_t)slot * STREAM_STRIDE;

        // ---- state in ----
        float c = 0.f, hlast = 0.f;                      // chain roles: cell state and last h of unit j
        float pm = 0.f, den = 0.f, acc = 0.f;            // pool: running max, denominator, weighted sum (lane j < 48)
        float xr[4] = {0.f, 0.f, 0.f, 0.f};
        if (role == 0) {
            c = st[STREAM_C0 + j];
            if (s == 0) sm.h0[3][j] = st[STREAM_H0 + j];  // h0 of step -1 of the chunk
        } else if (role == 2) {
            c = st[STREAM_C1 + j];
            if (s == 0) sm.h1[1][j] = st[STREAM_H1 + j];
        } else if (role == 3) {
            pm = st[STREAM_MAX]; den = st[STREAM_DEN];
            acc = lane < H ? st[STREAM_ACC + lane] : 0.f;
            chunk_x(a, b, 0, lane, xr);
            *reinterpret_cast<float4 *>(&sm.xs[0][0][0] + 4 * lane) = make_float4(xr[0], xr[1], xr[2], xr[3]);
        }
        __syncthreads();

        const int nm = T + SKEW;
        for (int m = 0; m < nm; ++m) {
            if (role == 0) {
                if (m < T) {
                    const float2 xq = *reinterpret_cast<const float2 *>(&sm.xs[(m >> 5) & 1][m & (XCH - 1)][2 * s]);
                    const f32x2 xv = {xq.x, xq.y};
                    f32x2 hv[6];
                    load_slice(&sm.h0[(m + 3) & 3][s * KS], hv);
                    f32x2 ac[4];
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        ac[g] = pk_fma(wx[g], xv, (f32x2){g == 0 ? bias : 0.f, 0.f});
#pragma unroll
                        for (int q = 0; q < 6; ++q) ac[g] = pk_fma(w[g][q], hv[q], ac[g]);
                    }
                    hlast = cell_step(quad_reduce_scatter(ac), c, ga, gb, gc);
                    if (s == 0) sm.h0[m & 3][j] = hlast;
                }
            } else if (role == 1) {
                if (m >= 1 && m <= T) {
                    f32x2 iv[6];
                    load_slice(&sm.h0[(m + 3) & 3][s * KS], iv);
                    f32x2 ac[4];
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        ac[g] = w[g][0] * iv[0];
#pragma unroll
                        for (int q = 1; q < 6; ++q) ac[g] = pk_fma(w[g][q], iv[q], ac[g]);
                    }
                    sm.pb[(m + 1) & 1][s * H + j] = quad_reduce_scatter(ac);
                }
            } else if (role == 2) {
                if (m >= 2 && m <= T + 1) {
                    const int t = m - 2;
                    const float pjb = sm.pb[t & 1][s * H + j] + bias;
                    f32x2 hv[6];
                    load_slice(&sm.h1[(t + 1) & 1][s * KS], hv);
                    f32x2 ac[4];
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        ac[g] = pk_fma(w[g][0], hv[0], (f32x2){g == 0 ? pjb : 0.f, 0.f});
#pragma unroll
                        for (int q = 1; q < 6; ++q) ac[g] = pk_fma(w[g][q], hv[q], ac[g]);
                    }
                    hlast = cell_step(quad_reduce_scatter(ac), c, ga, gb, gc);
                    if (s == 0) {
                        sm.h1[t & 1][j] = hlast;
                        sm.top[t & 1][j] = res ? hlast + sm.h0[t & 3][j] : hlast;
                    }
                }
            } else {
                if (m >= SKEW) {                         // one step of the online softmax, in this order whatever the chunk
                    const float tv = lane < H ? sm.top[(m - SKEW) & 1][lane] : 0.f;
                    const float sc = wave_sum(tv * aw) + ab;
                    const float mnew = fmaxf(pm, sc);
                    const float scale = __expf(pm - mnew);      // exp(-inf) = 0 on a stream's first step
                    const float p = __expf(sc - mnew);
                    den = den * scale + p;
                    acc = acc * scale + p * tv;
                    pm = mnew;
                }
                // the next 32 samples: loads at the chunk's first step, LDS writes (the wait for them) sixteen steps on
                const int nxt = (m & ~(XCH - 1)) + XCH;
                if (nxt < T) {
                    if ((m & (XCH - 1)) == 0) chunk_x(a, b, nxt, lane, xr);
                    if ((m & (XCH - 1)) == XCH / 2)
                        *reinterpret_cast<float4 *>(&sm.xs[(nxt >> 5) & 1][0][0] + 4 * lane) = make_float4(xr[0], xr[1], xr[2], xr[3]);
                }
            }
            __syncthreads();
        }

        // ---- state out: every part is that of the chunk's last step ----
        if (role == 0 && s == 0) { st[STREAM_H0 + j] = hlast; st[STREAM_C0 + j] = c; }
        if (role == 2 && s == 0) { st[STREAM_H1 + j] = hlast; st[STREAM_C1 + j] = c; }
        if (role == 3) {
            if (lane < H) st[STREAM_ACC + lane] = acc;
            if (lane == 0) {
                st[STREAM_MAX] = pm; st[STREAM_DEN] = den;
                long long *n = reinterpret_cast<long long *>(st + STREAM_STEPS);
                *n = *n + T;
            }
            // the decision of the prefix seen so far
            if (a.logits) prefix_readout<H>(a, lane < H ? acc / den : 0.f, sm.vec, a.logits, a.probs, b, a.B, lane);
        }
        __syncthreads();                                 // the next stream's state goes into the LDS rows this one's tail has read
    }
}

#if !NSD_MULTI_TU
// a reset slot: zero h and c, empty pooling state (running max -inf, denominator and sum 0), step count 0
__global__ __launch_bounds__(256) void stream_reset_kernel(float *state, const int S, const int32_t *slots, const int n) {
    const int i = blockIdx.x;
    if (i >= n) return;
    const int slot = slots ? slots[i] : i;
    if ((unsigned)slot >= (unsigned)S) return;
    const int e = threadIdx.x;
    if (e < STREAM_STRIDE) state[(size_t)slot * STREAM_STRIDE + e] = e == STREAM_MAX ? -INFINITY : 0.f;
}

#else
// mean[i] = (((p_0[i] + p_1[i]) + p_2[i]) + ...) / float(M), p_m = probs + m*n: a serial sum in m, every operation rounded on its own
__global__ __launch_bounds__(256) void multi_stream_mean_kernel(const float *probs, float *mean, const int M, const int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float sum = probs[i];
    for (int m = 1; m < M; ++m) sum = sum + probs[(size_t)m * n + i];
    mean[i] = sum / (float)M;
}
#endif

}  // namespace

#if !NSD_MULTI_TU
int nsd_stream48_launch(const StreamArgs &a, hipStream_t st) {
    const int cus = nsd_num_cus();
    const int grid = a.B < cus ? a.B : cus;
    hipLaunchKernelGGL(stream48_kernel, dim3(grid), dim3(NT), 0, st, a);
    NSD_CHECK_LAUNCH("stream_step");
    return NSD_OK;
}

int nsd_stream_reset_launch(float *state, int S, const int32_t *slots, int n, hipStream_t st) {
    static_assert(STREAM_STRIDE <= 256, "one thread per float of a slot");
    hipLaunchKernelGGL(stream_reset_kernel, dim3(n), dim3(256), 0, st, state, S, slots, n);
    NSD_CHECK_LAUNCH("stream_reset");
    return NSD_OK;
}

#else
// a.B streams of each of M models; G = min(B, max(1, CUs / M)) workgroups per model: one workgroup fits a CU (ten waves), so a larger
// grid would only queue.  mean: null, or [B,K] formed from a.probs by a second launch behind the step
int nsd_multi_stream48_launch(const StreamArgs &a, ModelSplit s, int M, float *mean, hipStream_t st) {
    const int per = nsd_num_cus() / M > 1 ? nsd_num_cus() / M : 1;
    s.G = a.B < per ? a.B : per;
    hipLaunchKernelGGL(multi_stream48_kernel, dim3(M * s.G), dim3(NT), 0, st, a, s);
    NSD_CHECK_LAUNCH("multi_stream_step");
    if (mean) {
        const int n = a.B * a.K;
        hipLaunchKernelGGL(multi_stream_mean_kernel, dim3((n + 255) / 256), dim3(256), 0, st, (const float *)a.probs, mean, M, n);
        NSD_CHECK_LAUNCH("multi_stream_mean");
    }
    return NSD_OK;
}
#endif
