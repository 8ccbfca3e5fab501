// nsd_ring_block.h -- the time loop of a recurrence role of the role-split H = 48 kernels (nsd_lstm2_fwd48.hip, nsd_lstm2_bwd48.hip),
// one ring block at a time.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

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
