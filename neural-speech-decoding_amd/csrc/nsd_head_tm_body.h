// nsd_head_tm_body.h -- the body of the head kernels of nsd_head_tm.hip, included INSIDE each kernel's braces (no include guard:
// it is not a header).  The including kernel defines `constexpr int MODE` (HEAD_EVAL, HEAD_TRAIN, HEAD_LOGITS, HEAD_DLOG), the
// template parameter VPL, the argument block `a` and `dlogits` (null except in HEAD_DLOG).
// Why an include and not an inlined function: hipcc compiles a kernel that calls an always-inline body differently from the same
// body written in the kernel (measured: head_tm_kernel<VPL, false / true> moved by 1-50 instructions and 2 VGPRs); textual
// inclusion leaves the code objects of the original two instantiations bit for bit what they were before the two new modes.
    constexpr bool STREAMS = MODE != HEAD_EVAL;                // RReLU slopes / head dropout of the training forward
    constexpr bool TRAIN = MODE == HEAD_TRAIN || MODE == HEAD_DLOG;   // dense backward, pass 2
    // U rows of the trial in flight per lane: the passes over the sequence are latency-bound (one wave per trial, 4 waves per CU at
    // B = 1024), so the bytes in flight set the rate -- 4 rows gave 1.3 TB/s
    constexpr int DH = 64 * VPL, U = VPL >= 16 ? 8 : (VPL >= 8 ? 8 : 16);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * (blockDim.x >> 6) + wave;        // one wave per trial; 4, 2 or 1 waves per workgroup (see launch_vpl)
    if (b >= a.B) return;                                       // whole waves leave; nothing below needs the workgroup
    const int c0 = lane * VPL, T = a.T, F = a.F, K = a.K;
    // a scan group of this evaluation (or of an earlier one on this workspace) timed out: the sequence below is garbage
    const bool bad = a.status != nullptr && ((a.status[0] | a.status[-NSD_SEQ_HEADER_WORDS]) & NSD_SEQ_ST_TIMEOUT_MASK) != 0;
    float aw[VPL];
#pragma unroll
    for (int v = 0; v < VPL; ++v) aw[v] = a.attn_w[c0 + v];
    const float ab = a.attn_b[0];
    const long arow = seq_row(0, b, T);                          // tile-major rows: step t of the trial is row arow + 32 t
    const bf16_t *seq = a.top + arow * DH + c0;

    // ---- pass 1: online softmax over time ------------------------------------------------------------------------------
    float m = -3.0e38f, l = 0.f, acc[VPL];
#pragma unroll
    for (int v = 0; v < VPL; ++v) acc[v] = 0.f;
    for (int t0 = 0; t0 < T; t0 += U) {
        float hv[U][VPL];
#pragma unroll
        for (int q = 0; q < U; ++q) {
            const int t = t0 + q < T ? t0 + q : T - 1;
            load_bf16_vals<VPL>(seq + (long)t * 32 * DH, hv[q]);
        }
#pragma unroll
        for (int q = 0; q < U; ++q) {
            if (t0 + q < T) {                                   // (a guard, not a break: the loop must unroll for hv[q] to stay in registers)
                float part = 0.f;
#pragma unroll
                for (int v = 0; v < VPL; ++v) part = fmaf(hv[q][v], aw[v], part);
                const float s = wave_sum(part) + ab;
                if (TRAIN && lane == 0) a.alpha[arow + 32L * (t0 + q)] = s;          // raw score; normalised below
                const float mn = fmaxf(m, s);
                const float sc = __expf(m - mn), e = __expf(s - mn);
                l = fmaf(l, sc, e);
#pragma unroll
                for (int v = 0; v < VPL; ++v) acc[v] = fmaf(acc[v], sc, e * hv[q][v]);
                m = mn;
            }
        }
    }
    const float inv_l = 1.f / l;
    float pooled[VPL];
#pragma unroll
    for (int v = 0; v < VPL; ++v) pooled[v] = acc[v] * inv_l;

    // ---- LayerNorm ------------------------------------------------------------------------------------------------------
    float sum = 0.f;
#pragma unroll
    for (int v = 0; v < VPL; ++v) sum += pooled[v];
    const float mu = wave_sum(sum) * (1.f / DH);
    float sq = 0.f;
#pragma unroll
    for (int v = 0; v < VPL; ++v) { const float d = pooled[v] - mu; sq = fmaf(d, d, sq); }
    const float rstd = rsqrtf(wave_sum(sq) * (1.f / DH) + 1e-5f);
    float xhat[VPL], ln[VPL], gam[VPL];
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
        gam[v] = a.ln_w[c0 + v];
        xhat[v] = (pooled[v] - mu) * rstd;
        ln[v] = fmaf(xhat[v], gam[v], a.ln_b[c0 + v]);
    }
    // ---- fc.0 -> RReLU -> dropout: lane f holds unit f ---------------------------------------------------------------------
    float pre = 0.f;
    for (int f = 0; f < F; ++f) {
        const float *wr = a.fc0_w + (long)f * DH + c0;
        float part = 0.f;
#pragma unroll
        for (int v = 0; v < VPL; ++v) part = fmaf(ln[v], wr[v], part);
        const float tot = wave_sum(part);
        if (lane == f) pre = tot + a.fc0_b[f];
    }
    float slope = a.eval_slope, dmul = 1.f;
    if (STREAMS && lane < F) {
        const long hi = (long)b * F + lane;
        if (a.rng.on) {
            const float u = (float)(nsd_rand_u32(a.rng.seed, a.rng.base + 1u, (uint64_t)hi) >> 8) * (1.0f / 16777216.0f);
            slope = 0.125f + ((float)(1.0 / 3.0) - 0.125f) * u;
            dmul = nsd_rand_u32(a.rng.seed, a.rng.base + 2u, (uint64_t)hi) >= a.rng.thr_head ? a.rng.keep_head : 0.f;
        } else {
            if (a.rrelu_slope) slope = a.rrelu_slope[hi];
            if (a.drop_head) dmul = a.drop_head[hi];
        }
    }
    const float act = lane < F ? (pre >= 0.f ? pre : pre * slope) * dmul : 0.f;
    // ---- fc.3: lane k holds class k ---------------------------------------------------------------------------------------
    float logit = -3.0e38f;
    for (int k = 0; k < K; ++k) {
        const float tot = wave_sum(lane < F ? act * a.fc3_w[(long)k * F + lane] : 0.f);
        if (lane == k) logit = tot + a.fc3_b[k];
    }
    if (bad) logit = __uint_as_float(0x7fc00000u);              // NaN: logits, probabilities and the loss all carry it
    float dlog;
    if constexpr (MODE == HEAD_DLOG) {
        // the caller's d loss / d logits (any loss, any scale); a timed-out evaluation poisons it as HEAD_TRAIN's NaN logits would
        dlog = lane < K ? (bad ? __uint_as_float(0x7fc00000u) : dlogits[(long)b * K + lane]) : 0.f;
    } else {
        if (lane < K) a.logits[(long)b * K + lane] = logit;
        const float lmax = wave_max(logit);
        const float ex = lane < K ? __expf(logit - lmax) : 0.f;
        const float den = wave_sum(ex);
        const float prob = ex / den;
        if (a.probs && lane < K) a.probs[(long)b * K + lane] = prob;
        if constexpr (!TRAIN) return;

        // ---- mean cross-entropy ------------------------------------------------------------------------------------------
        if (a.targets) {
            // soft targets (wave-uniform): loss = sum_k q_k ((lmax - logit_k) + log den), dlogits = scale (s p - q) without cancellation
            float ls;
            const float q = lane < K ? a.targets[(long)b * K + lane] : 0.f;
            const float dq = soft_ce_wave(q, logit, lmax, ex, den, __logf(den), lane, K, &ls);
            if (lane == 0) a.loss[b] = ls;
            dlog = lane < K ? dq * a.scale : 0.f;
        } else {
            const int y = a.labels[b];
            const float ly = lane_bcast(logit, y);
            if (lane == 0) a.loss[b] = (lmax - ly) + __logf(den);
            // p_y - 1 without cancellation: -(sum of the other classes' probabilities)
            const float others = wave_sum((lane < K && lane != y) ? ex : 0.f) / den;
            dlog = lane < K ? (lane == y ? -others : prob) * a.scale : 0.f;
        }
    }

    // ---- dense backward ---------------------------------------------------------------------------------------------------
    float dact = 0.f;
    for (int k = 0; k < K; ++k) {
        const float dk = lane_bcast(dlog, k);
        if (lane < F) dact = fmaf(dk, a.fc3_w[(long)k * F + lane], dact);
    }
    const float dpre = lane < F ? dact * dmul * (pre >= 0.f ? 1.f : slope) : 0.f;
    float dln[VPL];
#pragma unroll
    for (int v = 0; v < VPL; ++v) dln[v] = 0.f;
    for (int f = 0; f < F; ++f) {
        const float df = lane_bcast(dpre, f);
        const float *wr = a.fc0_w + (long)f * DH + c0;
#pragma unroll
        for (int v = 0; v < VPL; ++v) dln[v] = fmaf(df, wr[v], dln[v]);
    }
    // LayerNorm backward: dx = rstd * (dxhat - mean(dxhat) - xhat * mean(dxhat * xhat))
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int v = 0; v < VPL; ++v) { const float dx = dln[v] * gam[v]; s1 += dx; s2 = fmaf(dx, xhat[v], s2); }
    const float m1 = wave_sum(s1) * (1.f / DH), m2 = wave_sum(s2) * (1.f / DH);
    float dpool[VPL];
#pragma unroll
    for (int v = 0; v < VPL; ++v) dpool[v] = rstd * (dln[v] * gam[v] - m1 - xhat[v] * m2);
    // per-trial row for the parameter-gradient reductions
    float *row = a.hb + (long)b * a.hb_stride;
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
        row[c0 + v] = ln[v];
        row[DH + c0 + v] = dln[v] * xhat[v];
        row[2 * DH + c0 + v] = dln[v];
        a.pooled[(long)b * DH + c0 + v] = pooled[v];
        a.dpooled[(long)b * DH + c0 + v] = dpool[v];
    }
    if (lane < F) { row[4 * DH + lane] = dpre; row[4 * DH + F + lane] = act; }
    if (lane < K) row[4 * DH + 2 * F + lane] = dlog;

    // ---- pass 2: alpha_t, dscore_t, d attn.weight ----------------------------------------------------------------------------
    float dp_pooled = 0.f;
#pragma unroll
    for (int v = 0; v < VPL; ++v) dp_pooled = fmaf(dpool[v], pooled[v], dp_pooled);
    dp_pooled = wave_sum(dp_pooled);
    float dattn[VPL], dsum = 0.f;
#pragma unroll
    for (int v = 0; v < VPL; ++v) dattn[v] = 0.f;
    for (int t0 = 0; t0 < T; t0 += U) {
        float hv[U][VPL], sraw[U];
#pragma unroll
        for (int q = 0; q < U; ++q) {
            const int t = t0 + q < T ? t0 + q : T - 1;
            load_bf16_vals<VPL>(seq + (long)t * 32 * DH, hv[q]);
            sraw[q] = a.alpha[arow + 32L * t];                 // written by this wave's lane 0 in pass 1
        }
#pragma unroll
        for (int q = 0; q < U; ++q) {
            if (t0 + q < T) {
                float part = 0.f;
#pragma unroll
                for (int v = 0; v < VPL; ++v) part = fmaf(hv[q][v], dpool[v], part);
                const float qd = wave_sum(part);
                const float al = __expf(sraw[q] - m) * inv_l;
                const float ds = al * (qd - dp_pooled);
                if (lane == 0) {
                    a.alpha[arow + 32L * (t0 + q)] = al;
                    a.dscore[arow + 32L * (t0 + q)] = ds;
                }
                dsum += ds;
#pragma unroll
                for (int v = 0; v < VPL; ++v) dattn[v] = fmaf(ds, hv[q][v], dattn[v]);
            }
        }
    }
#pragma unroll
    for (int v = 0; v < VPL; ++v) row[3 * DH + c0 + v] = dattn[v];
    if (lane == 0) row[4 * DH + 2 * F + K] = dsum;
