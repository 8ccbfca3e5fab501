// nsd_ring_block.h -- the time loop of a recurrence role of the role-split H = 48 kernels (nsd_lstm2_fwd48.hip, nsd_lstm2_bwd48.hip),
// one ring block at a time.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif
#include <type_traits>

// ------------------------------------------------------------------------------------------------
// Block schedule of the one-trial H = 48 backward (nsd_lstm2_bwd48.hip), written once for the device and for the host test
// (tests/test_h48_bwd_schedule_cpu.py compiles this header with a host compiler and replays every role for T = 1 .. 1100).
// A trial is n_steps macro steps m = 0 .. n_steps - 1 in blocks of 8 (the ring length = the staged chunk), one workgroup barrier
// per step and one in front of the first; layer 1 handles time step t = T - 1 - m at macro step m, layer 0 t = T + 1 + DL0 - m.
// `..._inside(T, m0)` says that NO step of the block m0 .. m0 + 7 takes the other side of any test the role's untested block
// leaves out; every other block runs the tested form.
// ------------------------------------------------------------------------------------------------
#ifndef __HIPCC__
#define NSD_SCHED_FN constexpr
#else
#define NSD_SCHED_FN __host__ __device__ constexpr
#endif
namespace h48_bwd_sched {
constexpr int BLOCK = 8;
constexpr int DL0 = 3;                       // macro steps layer 0 runs behind layer 1, minus the 2 of a step-by-step hand-off
NSD_SCHED_FN int n_steps(const int T, const int dl0 = DL0) { return 4 * ((((T + 2 + dl0) / 4 + 1) + 1) & ~1); }
NSD_SCHED_FN int tbase(const int layer, const int T, const int dl0 = DL0) { return layer == 1 ? T - 1 : T + 1 + dl0; }   // t = tbase - m
// recurrences: the step reads da of the previous step and forms its own -- both t and t + 1 inside [0, T)
NSD_SCHED_FN bool chain_inside(const int layer, const int T, const int m0, const int dl0 = DL0) {
    return m0 >= tbase(layer, T, dl0) - T + 2 && m0 + BLOCK - 1 <= tbase(layer, T, dl0);
}
// x1 waves.  Every duty: the four-step hand-off wants m >= 4 (false at m = 0 only).  PREP of layer L at step m forms the factors of
// macro step m + 1: c[t-1] is read where t > 0, and the cell state of a trial's first step (t == T - 1, m + 1 == tbase - T + 1) comes
// from memory.  DX (no prep): da0 of macro step m - 1 leaves where its t0 = T + 2 + DL0 - m lies inside [0, T).
enum X1Duty : int { X1_PREP1 = 0, X1_PREP0 = 1, X1_PLAIN = 2, X1_DX = 3 };
NSD_SCHED_FN bool x1m_inside(const int duty, const int T, const int m0) {
    if (m0 < BLOCK) return false;            // m = 0 (no hand-off yet), layer 0's first step (m + 1 == 5), dx: t0 >= T up to m = 5
    const int mlast = m0 + BLOCK - 1;
    if (duty == X1_PREP1) return tbase(1, T) - (mlast + 1) > 0;
    if (duty == X1_PREP0) return tbase(0, T) - (mlast + 1) > 0;
    if (duty == X1_DX) return T + 2 + DL0 - mlast >= 0;
    return true;
}
// dW waves, da converters: the da of macro step m - 1 (m >= 1) is zero where its t lies outside [0, T)
NSD_SCHED_FN bool dw_conv_inside(const int layer, const int T, const int m0) {
    return m0 >= BLOCK && tbase(layer, T) - (m0 - 1) < T && tbase(layer, T) - (m0 + BLOCK - 2) >= 0;
}
// dW waves, tiles: window W = steps 16 W .. 16 W + 15 is taken at steps 16 W + 17 .. + 21 -- never in the first 16 steps (which
// dw16_role peels as its FIRST half; the host test holds the peeled steps to this)
NSD_SCHED_FN bool dw_tiles(const int m0) { return m0 >= 2 * BLOCK; }
// (the loader tests every piece of every chunk: chunks wholly inside [0, T) without the test measured no gain)
}  // namespace h48_bwd_sched
#undef NSD_SCHED_FN

#ifdef __HIPCC__

// One ring block: N steps, unrolled so that ring slots and LDS offsets are immediates.  body(k, inside) is the step of ring slot k
// and its barrier; `inside` is std::true_type where every step of the block lies inside the role's active window, else
// std::false_type, and the body tests the step index only in the second case.  One trial per workgroup: the ring unrolling left
// the window test as the only non-immediate control of a step, and a wave issues about one instruction per 5 cycles, scalar ones
// included; the blocks that hold an end of the window keep the test, rolled up (they run once or twice per trial and must not
// double the loop's code).  Two trials per workgroup: the loop as it was, every step tested (the split cost the forward's
// two-trial instantiation 4 bytes of scratch).
template <int NB, int N, class Body>
__device__ __forceinline__ void ring_block(const bool inside, Body &&body) {
    if constexpr (NB == 1) {
        if (inside) {
#pragma unroll
            for (int k = 0; k < N; ++k) body(k, std::true_type{});
        } else {
#pragma unroll 1
            for (int k = 0; k < N; ++k) body(k, std::false_type{});
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) body(k, std::false_type{});
    }
}
#endif  // __HIPCC__
