// The body of k_gemm_dual (weighted.hip.h) behind its stop test: one block's 64 x 64 output tiles of the TWO products that share
// an operand, over contraction chunk blockIdx.z, handed to the epilogue `epi` as (C1, C2).  NOT a header of its own: it is included
// INSIDE a kernel that has the names M, N, K, A, ars, acs, B, brs, bcs, X2, kchunk, epi and the template parameters T, SHARE_B in
// scope and defines KL_GEMM_DUAL_ROW_TILE, the block's row tile -- blockIdx.y in k_gemm_dual; in k_gemm_dual_batch (batch.hip.h),
// whose blockIdx.y carries the problem index as well, the row tile within the problem.  Text inclusion, not a __device__ function,
// for gemm_body.hip.h's reason: k_gemm_dual's instruction stream stays the one it was, and the batched kernel sums in its order by
// construction.
    __shared__ T As[GK][GT + 4];
    __shared__ T Bs[GK][GT + 4];
    __shared__ T Xs[GK][GT + 4];
    const int tid = threadIdx.x;
    const int m0 = KL_GEMM_DUAL_ROW_TILE * GT, n0 = blockIdx.x * GT;
    const int kbeg = blockIdx.z * kchunk;
    const int kend = min(K, kbeg + kchunk);
    typedef typename Acc4<T>::type acc_t;
    acc_t acc1[4], acc2[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) { acc1[t] = acc_t{T(0), T(0), T(0), T(0)}; acc2[t] = acc_t{T(0), T(0), T(0), T(0)}; }

    const bool a_k_contig = (acs == 1);
    const bool b_n_contig = (bcs == 1);
    const bool m_inside = m0 + GT <= M, n_inside = n0 + GT <= N;
    constexpr int PER = GT * GK / 256;
    T ra[PER], rb[PER], rx[PER];
    auto fetch = [&](int k0) {
        const bool k_inside = k0 + GK <= kend;
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int e = tid + 256 * u;
            int m, kk;
            if (a_k_contig) { kk = e % GK; m = e / GK; } else { m = e % GT; kk = e / GT; }
            const int gm = m0 + m, gk = k0 + kk;
            const int64_t o = (int64_t)gm * ars + (int64_t)gk * acs;
            const bool ok = (m_inside && k_inside) || (gm < M && gk < kend);
            ra[u] = ok ? A[o] : T(0);
            if constexpr (SHARE_B) rx[u] = ok ? X2[o] : T(0);
        }
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int e = tid + 256 * u;
            int n, kk;
            if (b_n_contig) { n = e % GT; kk = e / GT; } else { kk = e % GK; n = e / GK; }
            const int gn = n0 + n, gk = k0 + kk;
            const int64_t o = (int64_t)gk * brs + (int64_t)gn * bcs;
            const bool ok = (n_inside && k_inside) || (gn < N && gk < kend);
            rb[u] = ok ? B[o] : T(0);
            if constexpr (!SHARE_B) rx[u] = ok ? X2[o] : T(0);
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int e = tid + 256 * u;
            int m, kk;
            if (a_k_contig) { kk = e % GK; m = e / GK; } else { m = e % GT; kk = e / GT; }
            As[kk][m] = ra[u];
            if constexpr (SHARE_B) Xs[kk][m] = rx[u];
        }
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int e = tid + 256 * u;
            int n, kk;
            if (b_n_contig) { n = e % GT; kk = e / GT; } else { kk = e % GK; n = e / GK; }
            Bs[kk][n] = rb[u];
            if constexpr (!SHARE_B) Xs[kk][n] = rx[u];
        }
    };
    const int lane = tid & 63, wv = tid >> 6;
    if (kbeg < kend) { fetch(kbeg); commit(); }
    __syncthreads();
    for (int k0 = kbeg; k0 < kend; k0 += GK) {
        const bool more = k0 + GK < kend;
        if (more) fetch(k0 + GK);
#pragma unroll
        for (int k4 = 0; k4 < GK / 4; ++k4) {
            const int kr = 4 * k4 + (lane >> 4), ac = 16 * wv + (lane & 15);
            const T av = As[kr][ac];
            if constexpr (SHARE_B) {
                const T xv = Xs[kr][ac];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const T bv = Bs[kr][16 * t + (lane & 15)];
                    acc1[t] = mfma_16x16x4(av, bv, acc1[t]);
                    acc2[t] = mfma_16x16x4(xv, bv, acc2[t]);
                }
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const T bv = Bs[kr][16 * t + (lane & 15)];
                    const T xv = Xs[kr][16 * t + (lane & 15)];
                    acc1[t] = mfma_16x16x4(av, bv, acc1[t]);
                    acc2[t] = mfma_16x16x4(av, xv, acc2[t]);
                }
            }
        }
        __syncthreads();
        if (more) {
            commit();
            __syncthreads();
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int r = m0 + 16 * wv + (MfmaRow<T>::kLane * (lane >> 4) + MfmaRow<T>::kReg * rr), c = n0 + 16 * t + (lane & 15);
            if (r < M && c < N) epi.apply(r, c, acc1[t][rr], acc2[t][rr]);
        }
