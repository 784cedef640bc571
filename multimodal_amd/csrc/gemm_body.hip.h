// The body of k_gemm (exact.hip.h) behind its stop test: one block's 64 x 64 output tile of C = A . B over contraction chunk
// blockIdx.z, handed to the epilogue `epi`.  NOT a header of its own: it is included INSIDE a kernel that has the names M, N, K, A,
// ars, acs, B, brs, bcs, kchunk, epi and the template parameters T, TT, MF in scope and defines KL_GEMM_ROW_TILE, the block's row
// tile -- blockIdx.y in k_gemm; in k_gemm_batch (batch.hip.h), whose blockIdx.y carries the problem index as well, the row tile
// within the problem.  Text inclusion, not a __device__ function: k_gemm's instruction stream stays the one it was (a function
// call, inlined, came out with another register assignment), and the batched kernel sums in k_gemm's order by construction.
    static_assert(TT == 4, "64 x 64 tiles");
    constexpr int TL = 16 * TT;             // tile edge
    __shared__ T As[GK][TL + 4];
    __shared__ T Bs[GK][TL + 4];
    __shared__ double red[16];
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
    const int m0 = KL_GEMM_ROW_TILE * TL, n0 = blockIdx.x * TL;
    const int kbeg = blockIdx.z * kchunk;
    const int kend = min(K, kbeg + kchunk);
    T acc[TT][TT];
#pragma unroll
    for (int i = 0; i < TT; ++i)
#pragma unroll
        for (int j = 0; j < TT; ++j) acc[i][j] = T(0);
    typedef typename Acc4<T>::type acc_t;
    acc_t accm[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) accm[t] = acc_t{T(0), T(0), T(0), T(0)};

    const bool a_k_contig = (acs == 1);   // consecutive threads walk the contiguous axis
    const bool b_n_contig = (bcs == 1);
    const bool m_inside = m0 + TL <= M, n_inside = n0 + TL <= N;      // (uniform) this tile's rows of A / columns of B all exist
    // The next contraction step's operands are requested into registers BEFORE this step's arithmetic and written to LDS
    // behind it: the global latency runs under 16 x TT x TT multiply-adds per thread instead of in front of them (rounds
    // 1-3: load -> LDS -> barrier -> compute -> barrier, the latency exposed at every step).
    constexpr int PER = TL * GK / 256;      // elements of A (and of B) per thread and step
    T ra[PER], rb[PER];
    auto fetch = [&](int k0) {
        const bool k_inside = k0 + GK <= kend;
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int e = tid + 256 * u;
            int m, kk;
            if (a_k_contig) { kk = e % GK; m = e / GK; } else { m = e % TL; kk = e / TL; }
            const int gm = m0 + m, gk = k0 + kk;
            if (m_inside && k_inside) ra[u] = A[(int64_t)gm * ars + (int64_t)gk * acs];
            else ra[u] = (gm < M && gk < kend) ? A[(int64_t)gm * ars + (int64_t)gk * acs] : T(0);
        }
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int e = tid + 256 * u;
            int n, kk;
            if (b_n_contig) { n = e % TL; kk = e / TL; } else { kk = e % GK; n = e / GK; }
            const int gn = n0 + n, gk = k0 + kk;
            if (n_inside && k_inside) rb[u] = B[(int64_t)gk * brs + (int64_t)gn * bcs];
            else rb[u] = (gn < N && gk < kend) ? B[(int64_t)gk * brs + (int64_t)gn * bcs] : T(0);
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int e = tid + 256 * u;
            int m, kk;
            if (a_k_contig) { kk = e % GK; m = e / GK; } else { m = e % TL; kk = e / TL; }
            As[kk][m] = ra[u];
        }
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int e = tid + 256 * u;
            int n, kk;
            if (b_n_contig) { n = e % TL; kk = e / TL; } else { kk = e % GK; n = e / GK; }
            Bs[kk][n] = rb[u];
        }
    };
    if (kbeg < kend) { fetch(kbeg); commit(); }
    __syncthreads();
    for (int k0 = kbeg; k0 < kend; k0 += GK) {
        const bool more = k0 + GK < kend;
        if (more) fetch(k0 + GK);
        if constexpr (MF) {
            const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
            for (int k4 = 0; k4 < GK / 4; ++k4) {
                const T av = As[4 * k4 + (lane >> 4)][16 * wv + (lane & 15)];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const T bv = Bs[4 * k4 + (lane >> 4)][16 * t + (lane & 15)];
                    accm[t] = mfma_16x16x4(av, bv, accm[t]);
                }
            }
        } else {
#pragma unroll 4
        for (int kk = 0; kk < GK; ++kk) {
            T a[TT], b[TT];
#pragma unroll
            for (int i = 0; i < TT; ++i) a[i] = As[kk][ty * TT + i];
#pragma unroll
            for (int j = 0; j < TT; ++j) b[j] = Bs[kk][tx * TT + j];
#pragma unroll
            for (int i = 0; i < TT; ++i)
#pragma unroll
                for (int j = 0; j < TT; ++j) acc[i][j] += a[i] * b[j];
        }
        }
        __syncthreads();
        if (more) {
            commit();
            __syncthreads();
        }
    }
    if constexpr (MF) {
        const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int r = m0 + 16 * wv + (MfmaRow<T>::kLane * (lane >> 4) + MfmaRow<T>::kReg * rr), c = n0 + 16 * t + (lane & 15);
                if (r < M && c < N) epi.apply(r, c, (T)accm[t][rr]);
            }
    } else {
#pragma unroll
    for (int i = 0; i < TT; ++i)
#pragma unroll
        for (int j = 0; j < TT; ++j) {
            const int r = m0 + ty * TT + i, c = n0 + tx * TT + j;
            if (r < M && c < N) epi.apply(r, c, acc[i][j]);
        }
    }
    epi.finish(red);
