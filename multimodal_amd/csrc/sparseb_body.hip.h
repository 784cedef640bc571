// The bodies of k_spb_qw, k_spb_wrule, k_spb_n and k_spb_numer behind their stop test, included as text by those kernels
// (sparseb.hip.h) and by their batched forms (batch_sparse.hip.h), which first move the per-problem pointers to problem p's part
// of each buffer: what is gathered and summed is gathered and summed by one text, in one order, and each kernel's instruction
// stream is its own (gemm_body.hip.h's scheme).  No include guard: one section per inclusion, chosen by the macro the includer
// defines.  In scope at the inclusion:
//   KL_SPB_BODY_QW      T, KC, MODE, KEEP, NB, blkptr, indices, data, W, HT, q, loss_part, G, n, k, nb, eps    wave (b, i) = blockIdx.x
//   KL_SPB_BODY_WRULE   T, G, nb, Wold, Wnew, n, k, multiply                             elements over (blockIdx.x, gridDim.x)
//   KL_SPB_BODY_N       T, KC, cblkptr, csc_rows, csc_perm, q, W, NT, k, f, nrb                                wave (rb, j) = blockIdx.x
//   KL_SPB_BODY_NUMER   T, NT, nrb, numer, k, f; KL_SPB_NUMER_ATILE: the block's tile of 32 components         32 columns = blockIdx.x
#if defined(KL_SPB_BODY_QW)
    const int64_t i = blockIdx.x % n;
    const int b = (int)(blockIdx.x / n);
    const int lane = threadIdx.x, el = lane & (NB - 1);
    const int64_t p0 = blkptr[i * (nb + 1) + b], p1 = blkptr[i * (nb + 1) + b + 1];
    T w[KC], acc[KC];
    bool live[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) {
        live[c] = 64 * c + lane < k;
        w[c] = (MODE != SPB_INIT && live[c]) ? W[i * k + 64 * c + lane] : T(0);
        acc[c] = T(0);
    }
    double local = 0;
    for (int64_t p = p0; p < p1; p += NB) {
        const bool mine = lane < NB && p + lane < p1;
        const bool have = p + el < p1;
        const int my_j = have ? __builtin_nontemporal_load(indices + p + el) : __builtin_nontemporal_load(indices + p0);      // (past the end: a row of this block, unused)
        const T x = mine ? __builtin_nontemporal_load(data + p + lane) : T(0);
        const int cnt = (int)min((int64_t)NB, p1 - p);
        T qq = x;                                              // SPB_INIT: the W rule multiplies the entry itself
        T hv[KEEP ? NB : 1][KEEP ? KC : 1];
        if (KEEP) {
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                const T *h = HT + (int64_t)__builtin_amdgcn_readlane(my_j, u) * k;
#pragma unroll
                for (int c = 0; c < KC; ++c) hv[KEEP ? u : 0][KEEP ? c : 0] = live[c] ? h[64 * c + lane] : T(0);
            }
        }
        if (MODE != SPB_INIT) {
            T part[NB];
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                part[u] = T(0);
                if (KEEP) {
#pragma unroll
                    for (int c = 0; c < KC; ++c) part[u] += w[c] * hv[KEEP ? u : 0][KEEP ? c : 0];
                } else {
                    const T *h = HT + (int64_t)__builtin_amdgcn_readlane(my_j, u) * k;
#pragma unroll
                    for (int c = 0; c < KC; ++c)
                        if (live[c]) part[u] += w[c] * h[64 * c + lane];
                }
            }
            T wh = LaneTransposeSum<T, NB>::run(part, lane);
#pragma unroll
            for (int o = NB; o < 64; o <<= 1) wh += __shfl_xor(wh, o);      // every group of NB lanes summed its own lanes
            qq = T(0);
            if (mine) {
                qq = (x + eps) / (wh + eps);
                if (MODE == SPB_UPDATE) __builtin_nontemporal_store(qq, q + p + lane);
                local += (double)(x * log(qq)) - (double)x;
            }
        }
        if (MODE != SPB_LOSS) {
            if (KEEP) {                    // (entries past the end carry qq = 0)
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const T qu = lane_value(qq, u);
#pragma unroll
                    for (int c = 0; c < KC; ++c) acc[c] += qu * hv[KEEP ? u : 0][KEEP ? c : 0];
                }
            } else if (cnt == NB) {
                // k > 128: the rows are gathered a second time, all 32 loads of a component block issued before the first multiply-add
#pragma unroll
                for (int c = 0; c < KC; ++c) {
                    if (live[c]) {
                        T hr[NB];
#pragma unroll
                        for (int u = 0; u < NB; ++u) hr[u] = HT[(int64_t)__builtin_amdgcn_readlane(my_j, u) * k + 64 * c + lane];
#pragma unroll
                        for (int u = 0; u < NB; ++u) acc[c] += lane_value(qq, u) * hr[u];
                    }
                }
            } else {
                for (int u = 0; u < cnt; ++u) {                // (wave-uniform trip count)
                    const T *h = HT + (int64_t)__shfl(my_j, u) * k;
                    const T qu = __shfl(qq, u);
#pragma unroll
                    for (int c = 0; c < KC; ++c)
                        if (live[c]) acc[c] += qu * h[64 * c + lane];
                }
            }
        }
    }
    if (MODE != SPB_INIT) {
        local = wave_sum(local);
        if (lane == 0) loss_part[(int64_t)b * n + i] = local;
    }
    if (MODE != SPB_LOSS) {
        T *g = G + ((int64_t)b * n + i) * k;
#pragma unroll
        for (int c = 0; c < KC; ++c)
            if (live[c]) g[64 * c + lane] = acc[c];
    }
#elif defined(KL_SPB_BODY_WRULE)
    const int64_t total = n * k;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        T s = G[e];
        for (int b = 1; b < nb; ++b) s += G[(int64_t)b * total + e];
        Wnew[e] = multiply ? Wold[e] * s : s;
    }
#elif defined(KL_SPB_BODY_N)
    const int64_t j = blockIdx.x % f;
    const int rb = (int)(blockIdx.x / f);
    const int lane = threadIdx.x;
    const int64_t p0 = cblkptr[j * (nrb + 1) + rb], p1 = cblkptr[j * (nrb + 1) + rb + 1];
    T acc[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) acc[c] = T(0);
    for (int64_t p = p0; p < p1; p += 64) {
        const bool mine = p + lane < p1;
        const int my_i = mine ? __builtin_nontemporal_load(csc_rows + p + lane) : 0;
        const T my_q = mine ? q[__builtin_nontemporal_load(csc_perm + p + lane)] : T(0);
        const int cnt = (int)min((int64_t)64, p1 - p);
        // groups of 16 entries, all 16 gathers of a component block issued before the first multiply-add (entries past the end
        // carry q = 0 and row 0: no divergence; one dependent load per entry was a chain of L2 latencies)
#pragma unroll
        for (int u0 = 0; u0 < 64; u0 += 16) {
            if (u0 < cnt) {
#pragma unroll
                for (int c = 0; c < KC; ++c) {
                    if (64 * c + lane < k) {
                        T wv[16];
#pragma unroll
                        for (int u = 0; u < 16; ++u) wv[u] = W[(int64_t)__builtin_amdgcn_readlane(my_i, u0 + u) * k + 64 * c + lane];
#pragma unroll
                        for (int u = 0; u < 16; ++u) acc[c] += wv[u] * lane_value(my_q, u0 + u);
                    }
                }
            }
        }
    }
    T *o = NT + ((int64_t)rb * f + j) * k;
#pragma unroll
    for (int c = 0; c < KC; ++c)
        if (64 * c + lane < k) o[64 * c + lane] = acc[c];
#elif defined(KL_SPB_BODY_NUMER)
    __shared__ T tile[32][33];
    const int64_t j0 = (int64_t)blockIdx.x * 32, a0 = (int64_t)KL_SPB_NUMER_ATILE * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;           // 32 x 8 threads
    for (int r = ty; r < 32; r += 8) {
        const int64_t j = j0 + r, a = a0 + tx;
        T s = T(0);
        if (j < f && a < k)
            for (int rb = 0; rb < nrb; ++rb) s += NT[((int64_t)rb * f + j) * k + a];
        tile[r][tx] = s;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int64_t a = a0 + r, j = j0 + tx;
        if (a < k && j < f) numer[a * f + j] = tile[tx][r];
    }
#else
#error "sparseb_body.hip.h: define one of KL_SPB_BODY_QW / _WRULE / _N / _NUMER"
#endif
