// nsd_seq_dx.hip -- the input gradient of the sequence-batched path (nsd_seq_train_bwd_dx):
//   dx[b][t][c] = sum_d sum_k da0_d[seq_row(t, b)][k] * W_ih0_d[k][c]
// one contraction over K = D * 4H (both directions at once) of layer 0's gate gradients with its bf16 input weights, fp32
// accumulation, scattered straight into the caller's [B][T][C] layout (padding trials and padding channels dropped).
//
// Shape: M = T * Bp rows (up to 512 k), N = CP = 16..64 columns, K up to 4096.  The kernel is bound by reading da0 once (cfg5:
// 4.3 GB), so it is a streaming kernel: a wave owns 64 rows and walks K in blocks of 64 -- per block a lane loads 32 contiguous
// bytes of each of its 4 rows (16 rows x 128 B per load pair = whole lines), non-temporal, one block ahead of the MFMAs.
// v_mfma_f32_16x16x32_bf16: N = 16 per tile (a 32x32 tile would waste half of every MFMA at CP = 16 or 48).  The 32 k of an
// MFMA step are a PERMUTATION of the block's 64: lane group q = lane >> 4 holds k = 64 kb + 16 q + 8 s + j (j = 0..7) at step s,
// and the B operand is laid out with the same map.  W_ih0 (512 KB at cfg5) does not fit LDS; its fragments are prepared once
// per call into a scratch region (wfrag) and every wave reads them from L2 with 1-KB coalesced loads.
#include "nsd_seq.h"

namespace {

// wfrag[kb][nt][s][lane][8] = W^T[k = 64 kb + 16 (lane >> 4) + 8 s + j][n = 16 nt + (lane & 15)], k over [0, D * 4H) in the
// unit-major gate order of da (c = 4u + g, direction d at k = d * 4H + c).
// CHECKED, not assumed: wx[0][d] (the forward's W_ih0 operand, seq_prep_kernel) is NOT in that order -- its rows are in accumulator-
// tile order, row' = 32 tile + 8 j + 4 hh + g <-> torch row g * H + 8 tile + 4 hh + j (tile_row_to_param_row, nsd_scan.hip).  So
// unit u = 8 tile + 4 hh + j sits at row' = 32 (u >> 3) + 8 (u & 3) + 4 ((u >> 2) & 1) + g.  Columns n >= C are wx's zero padding.
__global__ __launch_bounds__(256) void seq_dx_wprep_kernel(const bf16_t *wx0, const bf16_t *wx1, int H, int CP, long total, bf16_t *wfrag) {
    const int G = 4 * H, NTT = CP / 16;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int j = (int)(e & 7), lane = (int)((e >> 3) & 63), s = (int)((e >> 9) & 1);
        const long r = e >> 10;
        const int nt = (int)(r % NTT), kb = (int)(r / NTT);
        const int k = 64 * kb + 16 * (lane >> 4) + 8 * s + j, n = 16 * nt + (lane & 15);
        const int d = k / G, c = k - d * G, u = c >> 2, g = c & 3;
        const int rowp = 32 * (u >> 3) + 8 * (u & 3) + 4 * ((u >> 2) & 1) + g;
        wfrag[e] = (d ? wx1 : wx0)[(long)rowp * CP + n];
    }
}

// NT column tiles of 16 (columns 16 nt0 .. 16 (nt0 + NT) of CP); a workgroup = 4 waves = 256 rows
template <int NT>
__global__ __launch_bounds__(256) void seq_dx_kernel(const bf16_t *da, const bf16_t *wfrag, int K, int NTT, int nt0, long R, int B, int T,
                                                     int C, float *dx) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, col = lane & 15;
    const long m0 = ((long)blockIdx.x * 4 + wave) * 64;
    if (m0 >= R) return;                                        // (R is a multiple of 32: a 16-row tile is wholly in or out)
    const bf16_t *arow[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const long r = m0 + 16 * mt + col;
        arow[mt] = da + (r < R ? r : R - 1) * K + 16 * q;       // rows past R load row R - 1 and store nothing
    }
    const bf16_t *wl = wfrag + ((long)nt0 * 2 * 64 + lane) * 8;
    const long kb_stride = (long)NTT * 2 * 512;                 // elements per k block of wfrag
    const int KB = K / 64;
    f32x4 acc[4][NT];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[mt][nt][r] = 0.f;
    u32x4 a[4][2], w[NT][2];
    auto load = [&](const int kb) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            a[mt][0] = ld_stream<u32x4>(arow[mt] + 64L * kb);
            a[mt][1] = ld_stream<u32x4>(arow[mt] + 64L * kb + 8);
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            w[nt][0] = *reinterpret_cast<const u32x4 *>(wl + kb * kb_stride + (2L * nt) * 512);
            w[nt][1] = *reinterpret_cast<const u32x4 *>(wl + kb * kb_stride + (2L * nt + 1) * 512);
        }
    };
    load(0);
    for (int kb = 0; kb < KB; ++kb) {
        u32x4 ca[4][2], cw[NT][2];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) { ca[mt][0] = a[mt][0]; ca[mt][1] = a[mt][1]; }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) { cw[nt][0] = w[nt][0]; cw[nt][1] = w[nt][1]; }
        if (kb + 1 < KB) load(kb + 1);
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ca[mt][s]), __builtin_bit_cast(bf16x8, cw[nt][s]),
                                                                         acc[mt][nt], 0, 0, 0);
    }
    // accumulator map (16x16): register r of lane l holds row 4 (l >> 4) + r, column l & 15; row -> (trial, step) by seq_row's inverse
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long row = m0 + 16 * mt + 4 * q + r;
            if (row >= R) continue;
            const long tile = row / (32L * T), rem = row - tile * 32L * T;
            const int t = (int)(rem >> 5), b = (int)(tile * 32 + (rem & 31));
            if (b >= B) continue;                               // padding trials
            float *out = dx + ((long)b * T + t) * C;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int c = 16 * (nt0 + nt) + col;
                if (c < C) out[c] = acc[mt][nt][r];             // padding channels dropped
            }
        }
}

template <int NT>
void launch_nt(const bf16_t *da, const bf16_t *wfrag, int K, int NTT, int nt0, long R, int B, int T, int C, float *dx, hipStream_t st) {
    hipLaunchKernelGGL((seq_dx_kernel<NT>), dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, da, wfrag, K, NTT, nt0, R, B, T, C, dx);
}

}  // namespace

int64_t nsd_seq_dx_scratch_bytes(int H, int D, int CP) { return (int64_t)D * 4 * H * CP * 2; }

int nsd_seq_dx_launch(const SeqDx &a, hipStream_t st) {
    const int K = a.D * 4 * a.H, NTT = a.CP / 16;
    const long R = (long)a.T * a.Bp;
    if (K % 64 || a.CP % 16 || a.Bp % 32) { nsd_set_error("seq dx: K=%d CP=%d Bp=%d not covered", K, a.CP, a.Bp); return NSD_E_INVALID; }
    const long total = (long)K * a.CP;
    const long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(seq_dx_wprep_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, a.wx[0], a.D > 1 ? a.wx[1] : a.wx[0],
                       a.H, a.CP, total, a.wfrag);
    for (int nt0 = 0; nt0 < NTT; nt0 += 4) {                    // CP > 64: one pass over da per 64 columns
        switch (NTT - nt0 < 4 ? NTT - nt0 : 4) {
        case 1: launch_nt<1>(a.da, a.wfrag, K, NTT, nt0, R, a.B, a.T, a.C, a.dx, st); break;
        case 2: launch_nt<2>(a.da, a.wfrag, K, NTT, nt0, R, a.B, a.T, a.C, a.dx, st); break;
        case 3: launch_nt<3>(a.da, a.wfrag, K, NTT, nt0, R, a.B, a.T, a.C, a.dx, st); break;
        default: launch_nt<4>(a.da, a.wfrag, K, NTT, nt0, R, a.B, a.T, a.C, a.dx, st); break;
        }
    }
    NSD_CHECK_LAUNCH("seq_dx_kernel");
    return NSD_OK;
}
