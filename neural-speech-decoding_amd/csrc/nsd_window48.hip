// nsd_window48.hip -- sliding-window decisions for continuous streams (gfx950): nsd_window_step / nsd_window_reset of nsd.h.
//
// "Every `hop` samples, the decision of the model run from a zero state over the last `window` samples."  With R = window / hop, window k
// covers samples [k hop, k hop + window) of a stream and belongs to PHASE k mod R; a phase's windows follow each other back to back, so
// a phase is one resumable stream (nsd_stream48.hip) that is read out and reset every `window` samples.  One workgroup = one (stream,
// phase) at a time (it loops when there are more pairs than workgroups; the weights stay in VGPRs), the same ten waves and roles as
// stream48_kernel, one barrier per macro step.  A workgroup walks its phase through the chunk in SEGMENTS: the idle samples in front of
// the phase's first window are skipped; a segment runs min(T - at, window - p) steps plus the three drain macro steps; when that fills
// the window, the pool wave reads it out into its row (prefix_readout, nsd_common.h) and the phase state is reset in registers / LDS;
// the phase slot is stored once, at the end.  Everything a call needs is derived from the stream's sample count in the state.
//
// THE PER-STEP STATEMENTS OF THE FOUR ROLES ARE THOSE OF stream48_kernel, RESTATED HERE statement for statement (with the segment's
// length and offset where that kernel has the chunk's): sharing the text would have put stream48_kernel's body behind a function or
// macro boundary, and its machine code is pinned (tools/isa_digest.py).  The library is built with -ffp-contract=off,
// so equal source gives equal bits; tests/test_gpu_window.py holds the two together byte for byte.
//
// The step is one source that two kernels are compiled from, as nsd_stream48.hip's is: window48_kernel (one model, this file) and
// multi_window48_kernel (M models of one shape per launch: nsd_multi_window_step; compiled as nsd_multi_window48.hip, which includes this
// file with NSD_MULTI_TU set, so that the single-model kernels' module is what it was).  The model-batched kernel works on a model view
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

// element (tl = lane >> 1, channels 4 (lane & 1) ..) of the 32 steps that start at sample t0 of the chunk, up to the segment's end `lim`
// (<= T); a sample that is not finite enters as NaN (an infinity times a weight can come out finite behind a sigmoid)
__device__ __forceinline__ void chunk_x(const WindowArgs &a, const int b, const int t0, const int lim, const int lane, float (&v)[4]) {
    const int t = t0 + (lane >> 1), ch0 = 4 * (lane & 1);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        float w = 0.f;
        if (t < lim && ch0 + u < a.C) {
            w = a.x[((size_t)b * a.T + t) * a.C + ch0 + u];
            if ((__float_as_uint(w) & 0x7f800000u) == 0x7f800000u) w = __uint_as_float(0x7fc00000u);
        }
        v[u] = w;
    }
}

// phase ph's share of a stream's unused rows (those from `cnt` on, row i belongs to phase i mod R): NaN logits / probs, end -1
__device__ __forceinline__ void void_rows(const WindowArgs &a, const int b, const int ph, const int cnt, const int tid) {
    const int K = a.K, R = a.R;
    int i = cnt + (ph - cnt % R + R) % R;
    for (; i < a.D; i += R) {
        const size_t row = (size_t)b * a.D + i;
        if (tid < K) {
            a.logits[row * K + tid] = __uint_as_float(0x7fc00000u);
            if (a.probs) a.probs[row * K + tid] = __uint_as_float(0x7fc00000u);
        }
        if (tid == 64) a.ends[row] = -1;
    }
}

// WINDOW48_KERNEL: the kernel's name and parameters; WINDOW48_VIEW: what `a` is -- the argument block itself (the workgroups of the grid
// share its B * R pairs: wg_id / wg_count are blockIdx.x / gridDim.x) or the view of the workgroup's model (the workgroups of one model
// share them).  A macro rather than a template body: window48_kernel keeps its machine code (tools/isa_digest.py)
#if !NSD_MULTI_TU
#define WINDOW48_KERNEL window48_kernel(const WindowArgs a)
#define WINDOW48_VIEW
#else
// workgroup blockIdx.x runs model blockIdx.x / s.G: params + m*P, x + m*x_stride, state + m*S*window_stream_stride(R), logits / probs +
// m*B*D*K, ends + m*B*D, counts + m*B
__device__ __forceinline__ ModelView<WindowArgs> model_view(const WindowArgs &a, const ModelSplit &s) {
    using nsd_multi_detail::mv;
    const int m = nsd_multi_detail::model_of_block(s);
    ModelView<WindowArgs> v;
    static_cast<WindowArgs &>(v) = a;
    v.wg = (int)blockIdx.x - m * s.G;
    v.nwg = s.G;
    const size_t P = (size_t)s.P * m, bd = (size_t)m * a.B * a.D, bdk = bd * a.K;
    v.x = a.x + (size_t)s.x_stride * m;
    v.w_ih0 = a.w_ih0 + P; v.w_hh0 = a.w_hh0 + P; v.b_ih0 = a.b_ih0 + P; v.b_hh0 = a.b_hh0 + P;
    v.w_ih1 = a.w_ih1 + P; v.w_hh1 = a.w_hh1 + P; v.b_ih1 = a.b_ih1 + P; v.b_hh1 = a.b_hh1 + P;
    v.attn_w = a.attn_w + P; v.attn_b = a.attn_b + P; v.ln_w = a.ln_w + P; v.ln_b = a.ln_b + P;
    v.fc0_w = a.fc0_w + P; v.fc0_b = a.fc0_b + P; v.fc3_w = a.fc3_w + P; v.fc3_b = a.fc3_b + P;
    v.state = a.state + (size_t)m * a.S * window_stream_stride(a.R);
    v.logits = a.logits + bdk; v.probs = mv(a.probs, bdk);
    v.ends = a.ends + bd; v.counts = a.counts + (size_t)m * a.B;
    return v;
}
#define WINDOW48_KERNEL multi_window48_kernel(const WindowArgs a_in, const ModelSplit ms)
#define WINDOW48_VIEW const ModelView<WindowArgs> a = model_view(a_in, ms);
#endif

__global__ __launch_bounds__(NT) void WINDOW48_KERNEL {
    WINDOW48_VIEW
    __shared__ SSmem sm;
    const int tid = threadIdx.x, lane = tid & 63;
    const int role = tid / 192;              // 0 L0, 1 P, 2 L1, 3 pool (wave-uniform: 192 = 3 waves)
    const int r = tid - role * 192, j = r >> 2, s = r & 3;
    const int T = a.T, C = a.C, W = a.W, Hp = a.Hp, R = a.R;

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
        const float *Wm = role == 0 ? a.w_hh0 : role == 1 ? a.w_ih1 : a.w_hh1;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int row = (g ^ s) * H + j;             // slot g: gate g ^ s
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                w[g][q].x = Wm[(size_t)row * H + s * KS + 2 * q];
                w[g][q].y = Wm[(size_t)row * H + s * KS + 2 * q + 1];
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

    const int items = a.B * R;               // B <= S and the state holds S * R phase slots: below 2^31
    for (int it = wg_id(a); it < items; it += wg_count(a)) {
        const int b = it / R, ph = it - b * R;
        const int slot = a.slots ? a.slots[b] : b;
        // (all the same for every thread of the workgroup) a slot outside the state, or a state reset with another window / hop: skipped
        bool ok = (unsigned)slot < (unsigned)a.S;
        float *hdr = nullptr;
        if (ok) {
            hdr = a.state + (size_t)slot * window_stream_stride(R) + (size_t)R * STREAM_STRIDE;
            const int32_t *hw = reinterpret_cast<const int32_t *>(hdr);
            ok = hw[WINDOW_HDR_W] == W && hw[WINDOW_HDR_HOP] == Hp;
        }
        if (!ok) {                                       // NaN rows, count -1, no state touched
            void_rows(a, b, ph, 0, tid);
            if (ph == 0 && tid == 0) a.counts[b] = -1;
            continue;
        }
        long long *cnt_p = reinterpret_cast<long long *>(hdr + WINDOW_HDR_COUNT) + ph;
        const long long n0 = *cnt_p;                     // this phase's copy of the stream's sample count
        // ends are the multiples of hop from `window` on: those in (n0, n0 + T] complete in this call, in rows 0 .. cnt - 1
        const long long q0 = n0 / Hp + 1, j0 = q0 > R ? q0 : (long long)R, j1 = (n0 + T) / Hp;
        const int cnt = j1 >= j0 ? (int)(j1 - j0 + 1) : 0;
        void_rows(a, b, ph, cnt, tid);
        if (ph == 0 && tid == 0) a.counts[b] = cnt;
        const long long s0 = (long long)ph * Hp;         // the phase's first window begins here
        if (n0 + T <= s0) {                              // idle for the whole call: its count and nothing else
            __syncthreads();                             // every wave has read n0
            if (tid == 0) *cnt_p = n0 + T;
            continue;
        }
        int at = n0 >= s0 ? 0 : (int)(s0 - n0);          // sample of the chunk the next segment begins at
        int p = n0 >= s0 ? (int)((n0 - s0) % W) : 0;     // samples the phase's current window has consumed
        float *st = a.state + (size_t)slot * window_stream_stride(R) + (size_t)ph * STREAM_STRIDE;

        // ---- state in ----
        float c = 0.f, hlast = 0.f;                      // chain roles: cell state and last h of unit j
        float pm = 0.f, den = 0.f, acc = 0.f;            // pool: running max, denominator, weighted sum (lane j < 48)
        float xr[4] = {0.f, 0.f, 0.f, 0.f};
        if (role == 0) {
            c = st[STREAM_C0 + j];
            hlast = st[STREAM_H0 + j];
        } else if (role == 2) {
            c = st[STREAM_C1 + j];
            hlast = st[STREAM_H1 + j];
        } else if (role == 3) {
            pm = st[STREAM_MAX]; den = st[STREAM_DEN];
            acc = lane < H ? st[STREAM_ACC + lane] : 0.f;
        }

        for (;;) {
            // ---- one segment: len steps of the phase's window, from sample `at` of the chunk ----
            const int len = T - at < W - p ? T - at : W - p;
            const int lim = at + len;
            if (role == 0) {
                if (s == 0) sm.h0[3][j] = hlast;         // h0 of step -1 of the segment
            } else if (role == 2) {
                if (s == 0) sm.h1[1][j] = hlast;
            } else if (role == 3) {
                chunk_x(a, b, at, lim, lane, xr);
                *reinterpret_cast<float4 *>(&sm.xs[0][0][0] + 4 * lane) = make_float4(xr[0], xr[1], xr[2], xr[3]);
            }
            __syncthreads();

            const int nm = len + SKEW;
            for (int m = 0; m < nm; ++m) {
                if (role == 0) {
                    if (m < len) {
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
                    if (m >= 1 && m <= len) {
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
                    if (m >= 2 && m <= len + 1) {
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
                    if (m >= SKEW) {                     // one step of the online softmax, in this order whatever the segment
                        const float tv = lane < H ? sm.top[(m - SKEW) & 1][lane] : 0.f;
                        const float sc = wave_sum(tv * aw) + ab;
                        const float mnew = fmaxf(pm, sc);
                        const float scale = __expf(pm - mnew);      // exp(-inf) = 0 on a window's first step
                        const float pe = __expf(sc - mnew);
                        den = den * scale + pe;
                        acc = acc * scale + pe * tv;
                        pm = mnew;
                    }
                    // the segment's next 32 samples: loads at a block's first step, LDS writes (the wait for them) sixteen steps on
                    const int nxt = (m & ~(XCH - 1)) + XCH;
                    if (nxt < len) {
                        if ((m & (XCH - 1)) == 0) chunk_x(a, b, at + nxt, lim, lane, xr);
                        if ((m & (XCH - 1)) == XCH / 2)
                            *reinterpret_cast<float4 *>(&sm.xs[(nxt >> 5) & 1][0][0] + 4 * lane) = make_float4(xr[0], xr[1], xr[2], xr[3]);
                    }
                }
                __syncthreads();
            }
            p += len;
            at = lim;

            if (p == W) {
                // ---- the window is full: its decision into its row, then the phase starts over from a reset slot ----
                if (role == 3) {
                    const long long e = n0 + at;
                    const size_t row = (size_t)b * a.D + (size_t)(e / Hp - j0);
                    prefix_readout<H>(a, lane < H ? acc / den : 0.f, sm.vec, a.logits, a.probs, (int)row, a.B * a.D, lane);
                    if (lane == 0) a.ends[row] = e;
                }
                c = 0.f; hlast = 0.f;
                pm = -INFINITY; den = 0.f; acc = 0.f;
                p = 0;
            }
            if (at >= T) break;
        }

        // ---- state out: every part is that of the chunk's last step ----
        if (role == 0 && s == 0) { st[STREAM_H0 + j] = hlast; st[STREAM_C0 + j] = c; }
        if (role == 2 && s == 0) { st[STREAM_H1 + j] = hlast; st[STREAM_C1 + j] = c; }
        if (role == 3) {
            if (lane < H) st[STREAM_ACC + lane] = acc;
            if (lane == 0) {
                st[STREAM_MAX] = pm; st[STREAM_DEN] = den;
                *reinterpret_cast<long long *>(st + STREAM_STEPS) = (long long)p;
                *cnt_p = n0 + T;
            }
        }
        __syncthreads();                                 // the next pair's state goes into the LDS rows this one's tail has read
    }
}

#if !NSD_MULTI_TU
// every phase slot a reset stream slot (zero h and c, max -inf, denominator and sum 0, step count 0); the header: window, hop, counts 0
__global__ __launch_bounds__(256) void window_reset_kernel(float *state, const int S, const int32_t *slots, const int n, const int W,
                                                           const int Hp, const int R) {
    const int i = blockIdx.x, ph = blockIdx.y;
    if (i >= n) return;
    const int slot = slots ? slots[i] : i;
    if ((unsigned)slot >= (unsigned)S) return;
    float *sb = state + (size_t)slot * window_stream_stride(R) + (size_t)ph * STREAM_STRIDE;
    if (ph < R) {
        const int e = threadIdx.x;
        if (e < STREAM_STRIDE) sb[e] = e == STREAM_MAX ? -INFINITY : 0.f;
        return;
    }
    for (int e = threadIdx.x; e < window_hdr_floats(R); e += 256)
        sb[e] = e == WINDOW_HDR_W ? __int_as_float(W) : e == WINDOW_HDR_HOP ? __int_as_float(Hp) : 0.f;
}

#else
// mean[i] = (((p_0[i] + p_1[i]) + p_2[i]) + ...) / float(M), p_m = probs + m*n: a serial sum in m, every operation rounded on its own (a
// row that is NaN in any model is NaN in the mean)
__global__ __launch_bounds__(256) void multi_window_mean_kernel(const float *probs, float *mean, const int M, const int n) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;      // n <= 2^31 - 1: the last block's index stays below 2^32
    if (i >= (unsigned)n) return;
    float sum = probs[i];
    for (int m = 1; m < M; ++m) sum = sum + probs[(size_t)m * n + i];
    mean[i] = sum / (float)M;
}
#endif

}  // namespace

#if !NSD_MULTI_TU
// B * R (stream, phase) pairs; one workgroup fits a CU (ten waves), so a grid above the CU count would only queue
int nsd_window48_launch(const WindowArgs &a, hipStream_t st) {
    const int cus = nsd_num_cus();
    const long long items = (long long)a.B * a.R;
    const int grid = items < cus ? (int)items : cus;
    hipLaunchKernelGGL(window48_kernel, dim3(grid), dim3(NT), 0, st, a);
    NSD_CHECK_LAUNCH("window_step");
    return NSD_OK;
}

int nsd_window_reset_launch(float *state, int S, const int32_t *slots, int n, int W, int Hp, hipStream_t st) {
    static_assert(STREAM_STRIDE <= 256, "one thread per float of a phase slot");
    const int R = W / Hp;
    hipLaunchKernelGGL(window_reset_kernel, dim3(n, R + 1), dim3(256), 0, st, state, S, slots, n, W, Hp, R);
    NSD_CHECK_LAUNCH("window_reset");
    return NSD_OK;
}

#else
// a.B * a.R (stream, phase) pairs of each of M models; G = min(B * R, max(1, CUs / M)) workgroups per model: one workgroup fits a CU (ten
// waves), so a larger grid would only queue.  mean: null, or [B,D,K] formed from a.probs by a second launch behind the step
int nsd_multi_window48_launch(const WindowArgs &a, ModelSplit s, int M, float *mean, hipStream_t st) {
    const int per = nsd_num_cus() / M > 1 ? nsd_num_cus() / M : 1;
    const long long items = (long long)a.B * a.R;
    s.G = items < per ? (int)items : per;
    hipLaunchKernelGGL(multi_window48_kernel, dim3(M * s.G), dim3(NT), 0, st, a, s);
    NSD_CHECK_LAUNCH("multi_window_step");
    if (mean) {
        const long long n = (long long)a.B * a.D * a.K;      // M * n <= 2^31 - 1 (nsd_multi_window_step)
        hipLaunchKernelGGL(multi_window_mean_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float *)a.probs, mean, M, (int)n);
        NSD_CHECK_LAUNCH("multi_window_mean");
    }
    return NSD_OK;
}
#endif
