// Fused nearest-example search: for every row of A the index of its nearest row of B under each selected measure,
// for a table of (A, B) jobs in ONE launch -- what evaluation.py:103-116 `classify_NN` does with `all_distances` + np.argmin per
// measure (metrics.py:58-86), without the [na, nb] matrices.
//
// Contract.  The value compared for (i, j, measure) is bit for bit what k_all_distances<T> stores in out[i * nb + j]: the terms
// and the closing expression are exact.hip.h's dist_term_* / dist_close (the text both kernels are compiled from), summed
// in its order -- lane-strided fp64 partial sums over e = lane, lane + 64, ..., wave_sum -- and rounded to T before they are
// compared.  The measures of a pair are formed in one pass over the two rows (one logarithm serves the three KL measures);
// each keeps the accumulators it has in the single-measure kernel, so no sum changes its order.
// Selection: np.argmin's -- the lowest index among equal minima; a NaN counts as smaller than every number, the lowest NaN wins.
//
// Decomposition.  One workgroup of kNearestWaves waves per row of A (block -> job through `row_job`; the row within the job by
// the job's row offset).  The row is staged once in LDS where d <= kNearestRowLds and read from global / L2 beyond that.
// Wave w takes the examples j = w, w + kNearestWaves, ...: one wave per pair as in k_all_distances, its lane 0 keeping the
// wave's best (value, index) per measure; the waves' candidates meet in LDS and thread m < 5 picks among them under the same
// rule and writes the one output element (job row, measure): one writer each, no atomics.
#pragma once

namespace klnmf {

constexpr int kNearestWaves = 4;          // waves that share one row of A
constexpr int kNearestRowLds = 2048;      // elements of T of the A row kept in LDS (16 KiB in fp64)
constexpr int kNearestMetrics = 5;        // DIST_KL .. DIST_COSINE_DIFF
constexpr int kNearestAllMetrics = (1 << kNearestMetrics) - 1;

struct NearestJob {                        // one (A, B) pair; device pointers, row strides in elements
    const void *A, *B;
    int64_t lda, ldb;
    int64_t row0;                          // offset of the job's rows in the outputs: the sum of na of the jobs before it
    int32_t na, nb;
    int32_t d, pad;
};

// np.argmin's order on (value, index): is (v, j) ahead of (bv, bj)?  An index < 0: no candidate.
template <typename T>
__device__ __forceinline__ bool nearest_ahead(T v, int j, T bv, int bj) {
    const bool vn = v != v, bn = bv != bv;
    const bool lower = vn ? (!bn || j < bj) : (!bn && (v < bv || (v == bv && j < bj)));
    return j >= 0 && (bj < 0 || lower);
}

template <typename T>
__device__ __forceinline__ void nearest_offer(T v, int j, T &bv, int &bj) {
    const bool ahead = nearest_ahead(v, j, bv, bj);
    bv = ahead ? v : bv;
    bj = ahead ? j : bj;
}

template <typename T>
struct NearestBest {                       // a wave's candidates, one per measure (named members: registers)
    T v0, v1, v2, v3, v4;
    int j0, j1, j2, j3, j4;
};

// The examples of wave `wave` (wave-uniform) against the row `a` (LDS or global): candidates in lane 0.
template <typename T>
__device__ __forceinline__ NearestBest<T> nearest_scan(const T *a, const T *B, int64_t ldb, int nb, int d, int metrics, double eps,
                                                       int wave, int lane) {
    NearestBest<T> best{(T)0, (T)0, (T)0, (T)0, (T)0, -1, -1, -1, -1, -1};
    const bool kl = (metrics & 7) != 0, fro = (metrics >> DIST_FROBENIUS & 1) != 0, cosd = (metrics >> DIST_COSINE_DIFF & 1) != 0;
    for (int j = wave; j < nb; j += kNearestWaves) {
        const T *b = B + (int64_t)j * ldb;
        double k0 = 0, k1 = 0, f0 = 0, c0 = 0, c1 = 0, c2 = 0;
        for (int e = lane; e < d; e += 64) {
            const double x = (double)a[e], y = (double)b[e];
            if (kl) dist_term_kl(x, y, eps, k0, k1);
            if (fro) dist_term_frobenius(x, y, f0);
            if (cosd) dist_term_cosine(x, y, c0, c1, c2);
        }
        if (kl) { k0 = wave_sum(k0); k1 = wave_sum(k1); }
        if (fro) f0 = wave_sum(f0);
        if (cosd) { c0 = wave_sum(c0); c1 = wave_sum(c1); c2 = wave_sum(c2); }
        if (metrics >> DIST_KL & 1) nearest_offer((T)dist_close(DIST_KL, k0, k1, 0.0), j, best.v0, best.j0);
        if (metrics >> DIST_REV_KL & 1) nearest_offer((T)dist_close(DIST_REV_KL, k0, k1, 0.0), j, best.v1, best.j1);
        if (metrics >> DIST_SYM_KL & 1) nearest_offer((T)dist_close(DIST_SYM_KL, k0, k1, 0.0), j, best.v2, best.j2);
        if (fro) nearest_offer((T)dist_close(DIST_FROBENIUS, f0, 0.0, 0.0), j, best.v3, best.j3);
        if (cosd) nearest_offer((T)dist_close(DIST_COSINE_DIFF, c0, c1, c2), j, best.v4, best.j4);
    }
    return best;
}

template <typename T>
__global__ __launch_bounds__(64 * kNearestWaves) void k_nearest(const NearestJob *jobs, const int32_t *row_job, int metrics,
                                                                 double eps, int32_t *idx, T *dist) {
    __shared__ T arow[kNearestRowLds];
    __shared__ T cand_v[kNearestWaves][kNearestMetrics];
    __shared__ int cand_j[kNearestWaves][kNearestMetrics];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const NearestJob job = jobs[row_job[blockIdx.x]];
    const int64_t row = (int64_t)blockIdx.x;                     // the output row: jobs lie behind one another
    const T *a = (const T *)job.A + (row - job.row0) * job.lda;
    const T *B = (const T *)job.B;
    NearestBest<T> best;
    if (job.d <= kNearestRowLds) {
        for (int e = threadIdx.x; e < job.d; e += 64 * kNearestWaves) arow[e] = a[e];
        __syncthreads();
        best = nearest_scan<T>(arow, B, job.ldb, job.nb, job.d, metrics, eps, wave, lane);
    } else {
        best = nearest_scan<T>(a, B, job.ldb, job.nb, job.d, metrics, eps, wave, lane);
    }
    if (lane == 0) {
        cand_v[wave][0] = best.v0; cand_j[wave][0] = best.j0;
        cand_v[wave][1] = best.v1; cand_j[wave][1] = best.j1;
        cand_v[wave][2] = best.v2; cand_j[wave][2] = best.j2;
        cand_v[wave][3] = best.v3; cand_j[wave][3] = best.j3;
        cand_v[wave][4] = best.v4; cand_j[wave][4] = best.j4;
    }
    __syncthreads();
    if (threadIdx.x < kNearestMetrics && (metrics >> threadIdx.x & 1)) {
        const int m = threadIdx.x;
        T bv = cand_v[0][m];
        int bj = cand_j[0][m];
        for (int w = 1; w < kNearestWaves; ++w) nearest_offer(cand_v[w][m], cand_j[w][m], bv, bj);
        const int count = __popc(metrics & kNearestAllMetrics), slot = __popc(metrics & ((1 << m) - 1));
        idx[row * count + slot] = bj;
        if (dist) dist[row * count + slot] = bv;
    }
}

}  // namespace klnmf
