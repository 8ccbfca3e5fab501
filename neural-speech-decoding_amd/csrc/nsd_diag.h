// nsd_diag.h -- what only the DIAGNOSTIC build of the library has (make diag -> libnsd_hip_diag.so, compiled with -DNSD_DIAG=1).
// None of this is part of include/nsd.h or of libnsd_hip.so: the product library rejects these flag bits (NSD_E_INVALID) and
// does not export the entry points.  Users: tests/ (exchange-mode agreement, forced time-out, the bf16 GEMM with every argument field
// and a pinned kernel: tests/test_gpu_gemm_bf16_exact.py), bench.py's per-kernel timing
// loop (outside the timed region), tools/.
#pragma once
#include <stdint.h>

#ifndef NSD_DIAG
#define NSD_DIAG 0
#endif

// nsd_seq_* flag bits, honoured by the diagnostic build only
#define NSD_DIAG_FLAG_NO_L2_EXCHANGE  16u   // scan groups always use the write-through exchange, also when all their workgroups report one XCD
#define NSD_DIAG_FLAG_SPREAD_GROUPS   32u   // consecutive block ids per group: every group spread over all XCDs (exercises write-through for real)
#define NSD_DIAG_FLAG_NO_FUSED_LAYERS 64u   // two unidirectional layers as two scans + GEMMs (the general route) instead of the skewed launch
#define NSD_DIAG_FLAG_LOSE_MEMBER    128u   // every scan launch misses its last workgroup: its group must time out (bounded spin) and report it
#define NSD_DIAG_FLAG_ALL (NSD_DIAG_FLAG_NO_L2_EXCHANGE | NSD_DIAG_FLAG_SPREAD_GROUPS | NSD_DIAG_FLAG_NO_FUSED_LAYERS | NSD_DIAG_FLAG_LOSE_MEMBER)

#if NSD_DIAG
extern "C" {
// Opt-in launch timing: nsd_seq_profile(1) records HIP events on the launch stream around the kernels of every following
// nsd_seq_* call, nsd_seq_profile(0) stops and discards; nsd_seq_profile_read sums the records of one kind and forgets them
// (BLOCKING).  kind: 0 forward scan, 1 backward scan, 2 input-projection GEMM, 3 weight-gradient GEMMs, 4 input-gradient GEMM,
// 5 head, 6 head parameter gradients, 7 operand preparation, 8 dL/dx contraction, 9 head backward from dlogits.
int nsd_seq_profile(int32_t enable);
int nsd_seq_profile_read(int32_t kind, float *total_ms, int32_t *count);
// Pin the H = 48 forward instantiation of the fp32 fast path: 1 / 2 / 4 trials per workgroup (4 = nsd_lstm2_fwd48x4.hip where it
// applies), 0 = the product's own choice.  Process-wide; tests compare the instantiations on the same inputs.
int nsd_diag_force_fwd48(int32_t nb);       // 0 = the product's choice, 1 / 2 / 4 trials per workgroup, 8 = the experimental one-wave-per-layer kernel (nsd_lstm2_fwd48w.hip: unfused training launches)
int nsd_diag_force_bwd48(int32_t nb);       // 0 = the product's choice, 2 = nsd_lstm2_bwd48.hip, 4 = nsd_lstm2_bwd48x4.hip where it applies
// The bf16 GEMM of the sequence path with EVERY field of GemmArgs (nsd_bf16.h; the public nsd_gemm_bf16 leaves b_period, the second
// source and the addend at zero) and the kernel pinned: 0 the product's choice, 1 the 128 x 128 kernel, 2 the register-staged
// 256 x 256 kernel, 22 / 23 / 32 the LDS-DMA 256 x 256 kernel with those stages.  Pointers are device pointers; the arguments pass
// the launcher's checks as the path's own calls do, and a selector whose kernel cannot run the problem is NSD_E_INVALID (nothing
// is launched).  Enqueues on `stream`.
typedef struct nsd_diag_gemm {
    const void *A, *B;          // bf16
    int64_t lda, ldb;
    int32_t a_kmajor, b_kmajor;
    int64_t b_shift, b_period;
    const void *B2;             // bf16 or null
    int64_t ldb2, b2_shift;
    int32_t n_split, epilogue;
    void *C;
    int64_t ldc;
    const float *bias, *add;
    int32_t M, N;
    int64_t K;
    int32_t splits, kernel;
} nsd_diag_gemm;
int nsd_diag_gemm_bf16(const nsd_diag_gemm *args, void *stream);
// The reductions that follow the weight-gradient GEMMs, alone: out[(g*H + u)*I + i] = sum_z part[z][4u + g][i] over nparts partials
// of [4H][N] floats, i < I <= N (seq_reduce_dw_kernel); b_ih[g*H + u] = b_hh[g*H + u] = sum_z part[z][4u + g] (seq_reduce_db_kernel).
int nsd_diag_reduce_dw(const float *part, int32_t nparts, int32_t H, int32_t N, int32_t I, float *out, void *stream);
int nsd_diag_reduce_db(const float *part, int32_t nparts, int32_t H, float *b_ih, float *b_hh, void *stream);
// The input-gradient kernels alone on caller-made operands: da0 [M][rows][G4], model m's W_ih0 [G4][C] at w_ih0 + m * P.  mode 0: M calls
// of the single-model launch into dx [M][rows][C]; 1: the model-batched launch, per model, into dx [M][rows][C]; 2: its mean over the
// models (serial fp32 sum over m ascending / (float)M) into dx [rows][C].  tests/ tie 1 to 0 bit for bit; tools/ time the three.
int nsd_diag_dx(const float *da0, const float *w_ih0, int64_t P, float *dx, int64_t rows, int32_t M, int32_t mode, int32_t G4, int32_t C,
                void *stream);
}
#endif
