// Codebooks by k-means on the device: what the reference's `build_codebook` and `iterative_kmeans` do with scipy's
// vq, kmeans2 and an SVD of the largest cluster's members (features/hac.py:68-107), as a fixed number of launches per iteration.
//
//   k_km_assign<T>   one workgroup per GROUP of kKmGroup = 4096 consecutive frames, walked as 16 tiles of kKmTile = 256 frames.
//                    Per tile: a thread per frame forms its label with vq.hip.h's code (features.hac.quantize's rule), stores
//                    it, and leaves it in LDS; then the tile's frames are added, frame by frame in ascending order, to the
//                    group's K * d fp64 accumulators and K int32 counts, which stay in LDS across the group's tiles.  At the
//                    end the group's partial sums and counts go to the workspace.
//   k_km_update<T>   a thread per codebook element: the groups' partials added in ascending group order, the count likewise
//                    (integers), the new element = sum / count.
//   k_km_gram<T>     one workgroup per group: sum over the group's member frames (label == cluster, or all with cluster = -1),
//                    ascending, of x_i * x_j for i <= j, and of x_j; the accumulators are registers (a thread owns up to 9 of
//                    the <= 2080 pairs), the frames pass through LDS promoted to fp64, 64 at a time.
//   k_km_gram_reduce the groups' partials added in ascending group order; the upper triangle stored and mirrored.
//
// THE ORDER RULE (the numpy twin, multimodal_amd/features/codebook.py, restates it).  Every sum over frames -- a cluster's
// column sum, an entry of the Gram matrix, a column sum of the Gram call -- is formed as
//     group g = frames [4096 g, min(T, 4096 (g + 1))):  p_g = (((0 + v_a) + v_b) + ...), the group's contributing frames in
//                                                       ascending order, each addition rounded to fp64;
//     total = (((0 + p_0) + p_1) + ...), the groups in ascending order (a group without a contributing frame adds its +0).
// v is the frame's value promoted to fp64 exactly (a sum) or the fp64 product x_i * x_j rounded on its own (the Gram matrix).
// The order is a function of T alone; no floating-point atomic exists in this file.  The tile (256 frames) is how a group is
// walked and is not part of the rule.  The mean is one fp64 division, sum / (double)count -- the count is below 2^31 and converts
// exactly -- rounded once more to f32 where the call's type is f32.  A cluster without a member keeps its row bit for bit.
//
// Who adds what (no two threads ever touch one accumulator): with d < 256 the K clusters are cut into nr = 256 / d contiguous
// ranges of per = ceil(K / nr); thread r * d + j owns column j of the clusters of range r, and the thread of column 0 their
// counts.  With d >= 256 thread j owns the columns j, j + 256, ... of every cluster.  Each walks the tile's 256 labels in LDS.
//
// LDS of k_km_assign: K * d doubles + K + 256 ints, at most kKmMaxKd * 8 + kKmMaxKd * 4 + 1024 = 160768 of the CU's 163840
// bytes at the bound K * d <= kKmMaxKd = 13312 (150 x 39 = 5850 and 1000 x 13 = 13000 fit).  Where more room is left the host
// stages the codebook and then the tile's frames (vq_staging; k_hac_vq does the same).
// Every store to global memory is a plain vector store by exactly one thread.
//
// Contraction.  "Rounded on its own" needs the compiler's contraction of a product and a sum into a fused multiply-add off:
// vq.hip.h, included before this header, says why the _rn intrinsics do not give that; the pragma below restates vq.hip.h's.
#pragma once
#pragma clang fp contract(off)

namespace klnmf {

constexpr int kKmThreads = 256;
constexpr int kKmTile = 256;                        // frames per tile: one per thread
constexpr int kKmGroupTiles = 16;
constexpr int kKmGroup = kKmTile * kKmGroupTiles;   // frames per group = per workgroup: the unit of the order rule
constexpr int kKmMaxKd = 13312;                     // K * d of a Lloyd call: 104 KiB of fp64 accumulators
constexpr int kKmLds = 160 * 1024;                  // the CU's LDS
constexpr int kKmGramMaxD = 64;
constexpr int kKmGramTile = 64;                     // frames staged per step of k_km_gram: 64 x 64 doubles = 32 KiB
constexpr int kKmGramPairs = (kKmGramMaxD * (kKmGramMaxD + 1) / 2 + kKmThreads - 1) / kKmThreads;   // 9 pairs per thread

static_assert(kKmThreads == kVqTile && kKmTile == kVqTile, "k_km_assign: vq.hip.h's tile, a thread per frame");

__host__ __device__ inline int64_t km_groups(int64_t T) { return T > 0 ? (T + kKmGroup - 1) / kKmGroup : 1; }

struct KmCall {                                     // one Lloyd call; device pointers, strides in elements
    const void *x;
    void *cb;
    int64_t ldx, ldc;
    int32_t T, d, K;
    int32_t stage;                                  // VQ_STAGE_*: what the host found room for in LDS
    int32_t sums;                                   // 0: labels and counts alone (n_iter = 0)
};

// psum [groups][K * d], pcnt [groups][K]: the groups' partials.  labels [T].
template <typename T>
__global__ __launch_bounds__(kKmThreads) void k_km_assign(KmCall c, int32_t *labels, double *psum, int32_t *pcnt) {
    extern __shared__ double km_lds[];
    const int d = c.d, K = c.K, Kd = K * d;
    const int tid = threadIdx.x;
    const T *x = (const T *)c.x, *cb = (const T *)c.cb;
    double *acc = km_lds;
    T *cbs = (T *)(acc + Kd);
    T *xs = cbs + ((c.stage & VQ_STAGE_CODEBOOK) ? Kd : 0);
    int32_t *cnt = (int32_t *)(xs + ((c.stage & VQ_STAGE_FRAMES) ? kVqFrameStride * d : 0));
    int32_t *lab = cnt + K;
    for (int e = tid; e < Kd; e += kKmThreads) acc[e] = 0.0;
    for (int k = tid; k < K; k += kKmThreads) cnt[k] = 0;
    if (c.stage & VQ_STAGE_CODEBOOK) vq_stage_codebook<T>(cbs, cb, c.ldc, Kd, d);
    // the accumulators of this thread: column j0 (+ 256, ...) of the clusters [k_lo, k_hi)
    const bool wide = d >= kKmThreads;
    const int nr = wide ? 1 : kKmThreads / d;
    const int per = (K + nr - 1) / nr;
    const int r = wide ? 0 : tid / d;
    const int j0 = wide ? tid : tid % d;
    const int k_lo = r < nr ? r * per : K;
    const int k_hi = min(K, k_lo + per);
    const int64_t group0 = (int64_t)blockIdx.x * kKmGroup;
    for (int tile = 0; tile < kKmGroupTiles; ++tile) {
        const int64_t frame0 = group0 + (int64_t)tile * kKmTile;
        if (frame0 >= c.T) break;                   // (block-uniform)
        const int n = (int)min((int64_t)kKmTile, (int64_t)c.T - frame0);
        if (c.stage & VQ_STAGE_FRAMES) vq_stage_frames<T>(xs, x, c.ldx, frame0, n, d);
        __syncthreads();                            // (the staged tile; the first time also the zeros and the codebook)
        if (tid < n) {
            const int64_t t = frame0 + tid;
            const int q = vq_code<T>(c.stage, x, c.ldx, t, xs, cb, c.ldc, cbs, K, d);
            labels[t] = q;
            lab[tid] = q;
        }
        __syncthreads();
        for (int f = 0; f < n; ++f) {
            const int l = lab[f];
            if (l >= k_lo && l < k_hi) {
                if (c.sums)
                    for (int j = j0; j < d; j += kKmThreads) {
                        const double v = (c.stage & VQ_STAGE_FRAMES) ? (double)xs[j * kVqFrameStride + f]
                                                                     : (double)x[(frame0 + f) * c.ldx + j];
                        acc[l * d + j] = acc[l * d + j] + v;
                    }
                if (j0 == 0) cnt[l] += 1;
            }
        }
        __syncthreads();                            // (the next tile overwrites the frames and the labels)
    }
    __syncthreads();
    if (c.sums)
        for (int e = tid; e < Kd; e += kKmThreads) psum[(int64_t)blockIdx.x * Kd + e] = acc[e];
    for (int k = tid; k < K; k += kKmThreads) pcnt[(int64_t)blockIdx.x * K + k] = cnt[k];
}

// A thread per codebook element: the new row where the cluster has members (c.sums), and counts[k] (int64) from the thread of
// column 0.
template <typename T>
__global__ __launch_bounds__(kKmThreads) void k_km_update(KmCall c, int groups, const double *psum, const int32_t *pcnt,
                                                          int64_t *counts) {
    const int e = blockIdx.x * kKmThreads + threadIdx.x;
    const int Kd = c.K * c.d;
    if (e >= Kd) return;
    const int k = e / c.d, j = e % c.d;
    int64_t n = 0;
    for (int g = 0; g < groups; ++g) n += pcnt[(int64_t)g * c.K + k];
    if (j == 0) counts[k] = n;
    if (!c.sums || n == 0) return;
    double s = 0.0;
    for (int g = 0; g < groups; ++g) s = s + psum[(int64_t)g * Kd + e];
    ((T *)c.cb)[(int64_t)k * c.ldc + j] = (T)(s / (double)n);
}

struct KmGramCall {
    const void *x;
    const int32_t *labels;                          // may be null with cluster = -1
    int64_t ldx;
    int32_t T, d, cluster;
};

// The pair p of the upper triangle, rows ascending: (0,0) (0,1) ... (0,d-1) (1,1) ...
__device__ __forceinline__ void km_pair(int p, int d, int *i, int *j) {
    int row = 0, left = p;
    while (left >= d - row) { left -= d - row; ++row; }
    *i = row;
    *j = row + left;
}

// pg [groups][npairs + d]: the pairs' partial sums, then the columns' ; pn [groups]: the group's members.
template <typename T>
__global__ __launch_bounds__(kKmThreads) void k_km_gram(KmGramCall c, double *pg, int32_t *pn) {
    __shared__ double xs[kKmGramTile * kKmGramMaxD];
    __shared__ int32_t member[kKmGramTile];
    const int d = c.d, tid = threadIdx.x;
    const int npairs = d * (d + 1) / 2;
    const T *x = (const T *)c.x;
    int pi[kKmGramPairs], pj[kKmGramPairs];
    double a[kKmGramPairs];
#pragma unroll
    for (int u = 0; u < kKmGramPairs; ++u) {
        const int p = tid + u * kKmThreads;
        pi[u] = 0;
        pj[u] = 0;
        if (p < npairs) km_pair(p, d, &pi[u], &pj[u]);
        a[u] = 0.0;
    }
    double colsum = 0.0;
    int members = 0;
    const int64_t group0 = (int64_t)blockIdx.x * kKmGroup;
    const int64_t group1 = min((int64_t)c.T, group0 + kKmGroup);
    for (int64_t frame0 = group0; frame0 < group1; frame0 += kKmGramTile) {
        const int n = (int)min((int64_t)kKmGramTile, group1 - frame0);
        __syncthreads();                            // (the previous step's readers are done)
        if (tid < n) member[tid] = c.cluster < 0 || c.labels[frame0 + tid] == c.cluster;
        for (int e = tid; e < n * d; e += kKmThreads) xs[e] = (double)x[(frame0 + e / d) * c.ldx + e % d];
        __syncthreads();
        for (int f = 0; f < n; ++f) {
            if (!member[f]) continue;               // (block-uniform)
            const double *row = xs + f * d;
#pragma unroll
            for (int u = 0; u < kKmGramPairs; ++u) a[u] = a[u] + row[pi[u]] * row[pj[u]];
            if (tid < d) colsum = colsum + row[tid];
            ++members;
        }
    }
    double *out = pg + (int64_t)blockIdx.x * (npairs + d);
#pragma unroll
    for (int u = 0; u < kKmGramPairs; ++u) {
        const int p = tid + u * kKmThreads;
        if (p < npairs) out[p] = a[u];
    }
    if (tid < d) out[npairs + tid] = colsum;
    if (tid == 0) pn[blockIdx.x] = members;
}

// gram [d * d] (the upper triangle and its mirror image), colsum [d], count [1].
KL_GLOBAL __launch_bounds__(kKmThreads) void k_km_gram_reduce(int d, int groups, const double *pg, const int32_t *pn, double *gram,
                                                              double *colsum, int64_t *count) {
    const int npairs = d * (d + 1) / 2;
    const int e = blockIdx.x * kKmThreads + threadIdx.x;
    if (e >= npairs + d + 1) return;
    if (e == npairs + d) {
        int64_t n = 0;
        for (int g = 0; g < groups; ++g) n += pn[g];
        *count = n;
        return;
    }
    double s = 0.0;
    for (int g = 0; g < groups; ++g) s = s + pg[(int64_t)g * (npairs + d) + e];
    if (e >= npairs) {
        colsum[e - npairs] = s;
        return;
    }
    int i, j;
    km_pair(e, d, &i, &j);
    gram[i * d + j] = s;
    if (i != j) gram[j * d + i] = s;
}

}  // namespace klnmf
