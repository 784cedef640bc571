// The motion modality on the device: what the reference's `db_to_VQ_hist_matrix` does with one Python call per
// frame and joint, scipy's whiten / kmeans per degree of freedom and lib/vector_quantization's get_histos
// (features/angle_histograms.py:171-223), as a fixed number of launches per stage.
//
//   k_mo_angles<T>      a thread per (frame, marker pair): q = q_src^-1 * q_dst, quaternion_matrix, euler_from_matrix('sxyz'),
//                       the operations in the reference's order (lib/transformations.py:1031-1097, 1174-1193, 1228-1267).
//   k_mo_velocities<T>  a thread per (frame, column): the delayed difference inside the frame's example (lib/utils.py:103-123),
//                       the example found by bisection of the offsets; the optional clip.
//   k_mo_clip<T>        the clip of the angles, after the velocities were taken from the unclipped ones.
//   k_mo_moments<T>     one workgroup per (group of 4096 frames, 32 columns): the group's partial sum of x or of (x - mean)^2
//                       per column, a thread per column adding the frames in ascending order out of LDS tiles of 128 frames.
//   k_mo_moments_reduce a thread per column: the groups' partials in ascending order; the mean, or the deviation (0 becomes 1).
//   k_mo_scale<T>       x / std.
//   k_mo_km_init        the state of the P problems: every row alive, no iteration, previous distortion +inf, not stopped.
//   k_mo_assign<T>      one workgroup per (group, problem); returns at once where the problem has stopped.  kmeans.hip.h's
//                       k_km_assign with three differences: rows that are not alive are skipped, the frame's distance
//                       sqrt(least squared distance) is left in LDS and added up by one thread in ascending order, and the
//                       tile of points and the codebook are always staged in LDS as fp64.  Where K * d <= 256 a thread owns
//                       exactly one accumulator and keeps it in a register: its loop over the tile's labels then holds no
//                       store, the LDS loads run ahead of the additions, and the order of the additions is the same.
//   k_mo_update<T>      one workgroup per problem: the groups' partials in ascending order, row = sum / count, a live row
//                       without members dropped; then one thread forms the distortion and the stop decision.
//   k_mo_hist<T>        one workgroup per (example, point set): per tile of 256 frames a thread per frame forms the least squared
//                       distance, the code and (soft) the sum of the weights; then a thread per bin adds the tile's frames in
//                       ascending order, forming its own weight again from the same operands (the same bits).
//   k_mo_hist_norm<T>   one workgroup per example: the row's sum by one thread, columns ascending; then the divisions.
//
// THE ORDER RULE is kmeans.hip.h's: groups of kMoGroup = 4096 consecutive frames, a group's contributing frames ascending from
// +0, the groups ascending from +0.  The numpy twin (multimodal_amd/features/angle_histograms.py) restates it.
// No two threads ever touch one accumulator (the ownership of k_km_assign); no floating-point atomic exists in this file; every
// store to global memory is a plain vector store by exactly one thread; no array is indexed dynamically outside LDS and global
// memory, so nothing goes to scratch.  Everything below is compiled with contraction off (vq.hip.h says why).
#pragma once
#pragma clang fp contract(off)

namespace klnmf {

constexpr int kMoThreads = 256;
constexpr int kMoTile = 256;
constexpr int kMoGroup = 4096;
constexpr int kMoGroupTiles = kMoGroup / kMoTile;
constexpr int kMoMaxK = 256;
constexpr int kMoMaxD = 16;
constexpr int kMoMaxKd = 1024;
constexpr int kMoMaxPairs = 32;
constexpr int kMoMaxGridY = 65535;
constexpr int kMoXStride = kMoTile + 1;             // doubles between the coordinates j, j + 1 of a staged point (bank spread)
constexpr int kMoMomCols = 32;                      // columns of one k_mo_moments workgroup
constexpr int kMoMomTile = 128;                     // frames of one of its LDS tiles
constexpr double kMoEps = 8.881784197001252e-16;    // 4 * eps(float64): lib/transformations.py's _EPS

__host__ __device__ inline int64_t mo_groups(int64_t T) { return T > 0 ? (T + kMoGroup - 1) / kMoGroup : 1; }

__device__ __forceinline__ double mo_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

// pairs: DEVICE int32 [n_pairs][2].  ang [T, 3 n_pairs].
template <typename T>
__global__ __launch_bounds__(kMoThreads) void k_mo_angles(const T *rec, int32_t frames, int32_t markers, const int32_t *pairs,
                                                          int32_t n_pairs, T *ang, int64_t lda) {
    const int64_t idx = (int64_t)blockIdx.x * kMoThreads + threadIdx.x;
    if (idx >= (int64_t)frames * n_pairs) return;
    const int64_t t = idx / n_pairs;
    const int p = (int)(idx % n_pairs);
    const T *qs = rec + (t * markers + pairs[2 * p]) * 7 + 3;
    const T *qd = rec + (t * markers + pairs[2 * p + 1]) * 7 + 3;
    const double sx = (double)qs[0], sy = (double)qs[1], sz = (double)qs[2], sw = (double)qs[3];
    const double x0 = (double)qd[0], y0 = (double)qd[1], z0 = (double)qd[2], w0 = (double)qd[3];
    // quaternion_inverse: the conjugate over dot(q, q)
    const double ns = ((sx * sx + sy * sy) + sz * sz) + sw * sw;
    const double x1 = -sx / ns, y1 = -sy / ns, z1 = -sz / ns, w1 = sw / ns;
    // quaternion_multiply(q1 = inverse, q0 = dest), left to right
    double q0 = ((x1 * w0 + y1 * z0) - z1 * y0) + w1 * x0;
    double q1 = ((-x1 * z0 + y1 * w0) + z1 * x0) + w1 * y0;
    double q2 = ((x1 * y0 - y1 * x0) + z1 * w0) + w1 * z0;
    double q3 = ((-x1 * x0 - y1 * y0) - z1 * z0) + w1 * w0;
    // quaternion_matrix
    const double nq = ((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3;
    double m00 = 1.0, m10 = 0.0, m20 = 0.0, m11 = 1.0, m12 = 0.0, m21 = 0.0, m22 = 1.0;
    if (!(nq < kMoEps)) {
        const double s = sqrt(2.0 / nq);
        q0 = q0 * s;
        q1 = q1 * s;
        q2 = q2 * s;
        q3 = q3 * s;
        const double q00 = q0 * q0, q01 = q0 * q1, q02 = q0 * q2, q03 = q0 * q3, q11 = q1 * q1, q12 = q1 * q2, q13 = q1 * q3,
                     q22 = q2 * q2, q23 = q2 * q3;
        m00 = (1.0 - q11) - q22;
        m10 = q01 + q23;
        m20 = q02 - q13;
        m11 = (1.0 - q00) - q22;
        m12 = q12 - q03;
        m21 = q12 + q03;
        m22 = (1.0 - q00) - q11;
    }
    // euler_from_matrix, axes 'sxyz': i, j, k = 0, 1, 2, no parity, no repetition, static frame
    const double cy = sqrt(m00 * m00 + m10 * m10);
    double ax, ay, az;
    if (cy > kMoEps) {
        ax = atan2(m21, m22);
        ay = atan2(-m20, cy);
        az = atan2(m10, m00);
    } else {
        ax = atan2(-m12, m11);
        ay = atan2(-m20, cy);
        az = 0.0;
    }
    T *o = ang + t * lda + 3 * p;
    o[0] = (T)ax;
    o[1] = (T)ay;
    o[2] = (T)az;
}

__device__ __forceinline__ double mo_clip(double x, double lo, double hi) {     // maximum(minimum(x, hi), lo); a NaN stays
    const double y = x > hi ? hi : x;
    return y < lo ? lo : y;
}

// offsets: DEVICE int64 [E + 1], checked by the host: 0 = offsets[0] <= ... <= offsets[E] = frames.
template <typename T>
__global__ __launch_bounds__(kMoThreads) void k_mo_velocities(const T *ang, int64_t lda, int32_t frames, int32_t cols,
                                                              const int64_t *offsets, int32_t E, int64_t delay, int circular,
                                                              int clip, double lo, double hi, T *vel, int64_t ldv) {
    const int64_t idx = (int64_t)blockIdx.x * kMoThreads + threadIdx.x;
    if (idx >= (int64_t)frames * cols) return;
    const int64_t t = idx / cols;
    const int c = (int)(idx % cols);
    int a = 0, b = E;                               // the example e with offsets[e] <= t < offsets[e + 1]: the last e whose start
    while (b - a > 1) {                             // is <= t (examples without a frame share a start with the one that has t)
        const int mid = (a + b) >> 1;
        if (offsets[mid] <= t) a = mid; else b = mid;
    }
    const int64_t start = offsets[a], n = offsets[a + 1] - start, local = t - start;
    const int64_t dl = delay < n ? delay : n;
    double prev = 0.0;
    if (local >= dl) prev = (double)ang[(t - dl) * lda + c];
    else if (circular) prev = (double)ang[(start + n - dl + local) * lda + c];
    double v = (double)ang[t * lda + c] - prev;
    if (clip) v = mo_clip(v, lo, hi);
    vel[t * ldv + c] = (T)v;
}

template <typename T>
__global__ __launch_bounds__(kMoThreads) void k_mo_clip(T *x, int64_t ld, int32_t frames, int32_t cols, double lo, double hi) {
    const int64_t idx = (int64_t)blockIdx.x * kMoThreads + threadIdx.x;
    if (idx >= (int64_t)frames * cols) return;
    T *p = x + (idx / cols) * ld + idx % cols;
    *p = (T)mo_clip((double)*p, lo, hi);
}

// part [groups][C].  mode 0: the sum of x; mode 1: of (x - mean)^2.
template <typename T>
__global__ __launch_bounds__(kMoThreads) void k_mo_moments(const T *x, int64_t ld, int32_t frames, int32_t C, int mode,
                                                           const double *mean, double *part) {
    __shared__ double tile[kMoMomTile * (kMoMomCols + 1)];
    const int tid = threadIdx.x;
    const int c0 = blockIdx.y * kMoMomCols;
    const int nc = min(kMoMomCols, C - c0);
    const int64_t group0 = (int64_t)blockIdx.x * kMoGroup;
    const int64_t group1 = min((int64_t)frames, group0 + kMoGroup);
    const double mu = (mode && tid < nc) ? mean[c0 + tid] : 0.0;
    double acc = 0.0;
    for (int64_t frame0 = group0; frame0 < group1; frame0 += kMoMomTile) {
        const int n = (int)min((int64_t)kMoMomTile, group1 - frame0);
        __syncthreads();                            // (the previous tile's readers are done)
        for (int e = tid; e < n * kMoMomCols; e += kMoThreads) {
            const int f = e / kMoMomCols, c = e % kMoMomCols;
            if (c < nc) tile[f * (kMoMomCols + 1) + c] = (double)x[(frame0 + f) * ld + c0 + c];
        }
        __syncthreads();
        if (tid < nc)
            for (int f = 0; f < n; ++f) {
                const double v = tile[f * (kMoMomCols + 1) + tid];
                if (mode) {
                    const double dv = v - mu;
                    acc = acc + dv * dv;
                } else {
                    acc = acc + v;
                }
            }
    }
    if (tid < nc) part[(int64_t)blockIdx.x * C + c0 + tid] = acc;
}

KL_GLOBAL __launch_bounds__(kMoThreads) void k_mo_moments_reduce(const double *part, int groups, int32_t frames, int32_t C, int mode,
                                                                 double *mean, double *std) {
    const int c = blockIdx.x * kMoThreads + threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (int g = 0; g < groups; ++g) s = s + part[(int64_t)g * C + c];
    if (!mode) {
        mean[c] = s / (double)frames;
    } else {
        const double sd = sqrt(s / (double)frames);
        std[c] = sd == 0.0 ? 1.0 : sd;
    }
}

template <typename T>
__global__ __launch_bounds__(kMoThreads) void k_mo_scale(const T *x, int64_t ld, int32_t frames, int32_t C, const double *std, T *out,
                                                         int64_t ldo) {
    const int64_t idx = (int64_t)blockIdx.x * kMoThreads + threadIdx.x;
    if (idx >= (int64_t)frames * C) return;
    const int64_t t = idx / C;
    const int c = (int)(idx % C);
    out[t * ldo + c] = (T)((double)x[t * ld + c] / std[c]);
}

struct MoKm {                                       // the P problems of one call; device pointers, strides in elements
    const void *pts;
    void *cbs;                                      // [P, K, d]
    int64_t set_stride, ld;
    int32_t T, d, K, P;
    const int32_t *set_of;                          // [P]
    int32_t *alive;                                 // [P, K]
    int32_t *done;                                  // [P]
    double *prev;                                   // [P]
};

KL_GLOBAL __launch_bounds__(kMoThreads) void k_mo_km_init(MoKm c, int32_t *iters, double *distortion) {
    const int idx = blockIdx.x * kMoThreads + threadIdx.x;
    if (idx < c.P * c.K) c.alive[idx] = 1;
    if (idx < c.P) {
        c.done[idx] = 0;
        c.prev[idx] = mo_inf();
        iters[idx] = 0;
        distortion[idx] = mo_inf();
    }
}

// The staged tile of points: dynamic, d * kMoXStride doubles (d = 2 leaves room for six workgroups on a CU, d = 16 for two).
extern __shared__ double mo_xs[];

// Stage n <= 256 points, `first` on, of a set as fp64: coordinate j of point f at xs[j * kMoXStride + f].
template <typename T>
__device__ __forceinline__ void mo_stage_points(const T *x, int64_t ld, int64_t first, int n, int d, double *xs) {
    for (int e = threadIdx.x; e < n * d; e += kMoThreads) {
        const int f = e / d, j = e % d;
        xs[j * kMoXStride + f] = (double)x[(first + f) * ld + j];
    }
}

// vq.hip.h's rule (vq_nearest_code) over the live rows of the staged codebook cbs [K, d]: the squared distance of staged point f
// to row k, j ascending, every operation rounded on its own.
__device__ __forceinline__ double mo_dist2(const double *xs, int f, const double *row, int d) {
    double acc = 0.0;
    for (int j = 0; j < d; ++j) {
        const double df = xs[j * kMoXStride + f] - row[j];
        acc = acc + df * df;
    }
    return acc;
}

// psum [P][groups][K * d], pcnt [P][groups][K], pdist [P][groups]; labels [P][T] or null.
template <typename T>
__global__ __launch_bounds__(kMoThreads) void k_mo_assign(MoKm c, int32_t *labels, double *psum, int32_t *pcnt, double *pdist) {
    __shared__ double acc[kMoMaxKd];
    __shared__ double cbs[kMoMaxKd];
    double *xs = mo_xs;                             // d * kMoXStride doubles
    __shared__ double dist[kMoTile];
    __shared__ int32_t cnt[kMoMaxK];
    __shared__ int32_t al[kMoMaxK];
    __shared__ int32_t lab[kMoTile];
    const int p = blockIdx.y;
    if (c.done[p]) return;                          // (block-uniform; nothing of a stopped problem is written again)
    const int d = c.d, K = c.K, Kd = K * d, tid = threadIdx.x;
    const T *x = (const T *)c.pts + (int64_t)c.set_of[p] * c.set_stride;
    const T *cb = (const T *)c.cbs + (int64_t)p * Kd;
    for (int e = tid; e < Kd; e += kMoThreads) {
        acc[e] = 0.0;
        cbs[e] = (double)cb[e];
    }
    for (int k = tid; k < K; k += kMoThreads) {
        cnt[k] = 0;
        al[k] = c.alive[(int64_t)p * K + k];
    }
    // the accumulators of this thread: column j0 of the clusters [k_lo, k_hi) (d <= 16 < 256: k_km_assign's narrow case)
    const int nr = kMoThreads / d;
    const int per = (K + nr - 1) / nr;
    const int r = tid / d, j0 = tid % d;
    const int k_lo = r < nr ? r * per : K;
    const int k_hi = min(K, k_lo + per);
    // K * d <= 256 (d = 2 up to K = 128): per = 1, a thread owns one accumulator and keeps it, and its count, in registers
    const bool own_one = per == 1;
    double ra = 0.0;
    int rn = 0;
    double dsum = 0.0;                              // thread kMoThreads - 1: the group's sum of distances
    const int64_t group0 = (int64_t)blockIdx.x * kMoGroup;
    for (int tile = 0; tile < kMoGroupTiles; ++tile) {
        const int64_t frame0 = group0 + (int64_t)tile * kMoTile;
        if (frame0 >= c.T) break;                   // (block-uniform)
        const int n = (int)min((int64_t)kMoTile, (int64_t)c.T - frame0);
        mo_stage_points<T>(x, c.ld, frame0, n, d, xs);
        __syncthreads();                            // (the staged tile; the first time also the zeros, codebook and mask)
        if (tid < n) {
            double best = mo_inf();
            int q = -1;
            for (int k = 0; k < K; ++k) {
                if (!al[k]) continue;
                const double a = mo_dist2(xs, tid, cbs + k * d, d);
                if (a < best || q < 0) {            // strict: the lowest live index keeps a tie
                    best = a;
                    q = k;
                }
            }
            lab[tid] = q;
            dist[tid] = sqrt(best);
            if (labels) labels[(int64_t)p * c.T + frame0 + tid] = q;
        }
        __syncthreads();
        if (own_one) {                              // (block-uniform) no store in the loop: the loads run ahead of the additions
            if (k_lo < k_hi) {
                const double *col = xs + j0 * kMoXStride;
#pragma unroll 8
                for (int f = 0; f < n; ++f) {
                    const bool mine = lab[f] == k_lo;
                    ra = mine ? ra + col[f] : ra;
                    rn += mine ? 1 : 0;
                }
            }
        } else {
            for (int f = 0; f < n; ++f) {
                const int l = lab[f];
                if (l >= k_lo && l < k_hi) {
                    acc[l * d + j0] = acc[l * d + j0] + xs[j0 * kMoXStride + f];
                    if (j0 == 0) cnt[l] += 1;
                }
            }
        }
        if (tid == kMoThreads - 1)
            for (int f = 0; f < n; ++f) dsum = dsum + dist[f];
        __syncthreads();                            // (the next tile overwrites the points, the labels and the distances)
    }
    const int64_t slot = (int64_t)p * gridDim.x + blockIdx.x;
    if (own_one) {
        if (k_lo < k_hi) {
            psum[slot * Kd + k_lo * d + j0] = ra;
            if (j0 == 0) pcnt[slot * K + k_lo] = rn;
        }
    } else {
        for (int e = tid; e < Kd; e += kMoThreads) psum[slot * Kd + e] = acc[e];
        for (int k = tid; k < K; k += kMoThreads) pcnt[slot * K + k] = cnt[k];
    }
    if (tid == kMoThreads - 1) pdist[slot] = dsum;
}

template <typename T>
__global__ __launch_bounds__(kMoThreads) void k_mo_update(MoKm c, int groups, double thresh, const double *psum, const int32_t *pcnt,
                                                          const double *pdist, int32_t *iters, double *distortion) {
    const int p = blockIdx.x;
    if (c.done[p]) return;                          // (block-uniform: every thread reads it before the barrier below)
    const int d = c.d, K = c.K, Kd = K * d, tid = threadIdx.x;
    const int64_t slot0 = (int64_t)p * groups;
    T *cb = (T *)c.cbs + (int64_t)p * Kd;
    int32_t *alive = c.alive + (int64_t)p * K;
    for (int e = tid; e < Kd; e += kMoThreads) {
        const int k = e / d;
        if (!alive[k]) continue;
        int64_t n = 0;
        for (int g = 0; g < groups; ++g) n += pcnt[(slot0 + g) * K + k];
        if (n == 0) continue;
        double s = 0.0;
        for (int g = 0; g < groups; ++g) s = s + psum[(slot0 + g) * Kd + e];
        cb[e] = (T)(s / (double)n);
    }
    __syncthreads();                                // (every read of the mask and of the stop flag is done)
    for (int k = tid; k < K; k += kMoThreads) {
        if (!alive[k]) continue;
        int64_t n = 0;
        for (int g = 0; g < groups; ++g) n += pcnt[(slot0 + g) * K + k];
        if (n == 0) alive[k] = 0;                   // dropped for good: code_book[has_members]
    }
    if (tid == 0) {
        double s = 0.0;
        for (int g = 0; g < groups; ++g) s = s + pdist[slot0 + g];
        const double now = s / (double)c.T;
        const double diff = fabs(c.prev[p] - now);
        c.prev[p] = now;
        distortion[p] = now;
        iters[p] += 1;
        if (diff <= thresh) c.done[p] = 1;
    }
}

struct MoHist {
    const void *pts;
    const void *cbs;                                // [D, K, d]
    int64_t set_stride, ld;
    int32_t d, K, D, soft;
    double alpha;
    const int64_t *offsets;                         // [E + 1]
};

// raw fp64 [E][D * K]: the sums of the associations over each example's frames.
template <typename T>
__global__ __launch_bounds__(kMoThreads) void k_mo_hist(MoHist c, double *raw) {
    __shared__ double cbs[kMoMaxKd];
    double *xs = mo_xs;                             // d * kMoXStride doubles
    __shared__ double least[kMoTile];
    __shared__ double wsum[kMoTile];
    __shared__ int32_t lab[kMoTile];
    const int e = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    const int d = c.d, K = c.K, Kd = K * d;
    const T *x = (const T *)c.pts + (int64_t)s * c.set_stride;
    const T *cb = (const T *)c.cbs + (int64_t)s * Kd;
    for (int i = tid; i < Kd; i += kMoThreads) cbs[i] = (double)cb[i];
    const int64_t first = c.offsets[e], last = c.offsets[e + 1];
    const double na = -c.alpha;
    double acc = 0.0;                               // thread k < K: bin k
    for (int64_t frame0 = first; frame0 < last; frame0 += kMoTile) {
        const int n = (int)min((int64_t)kMoTile, last - frame0);
        mo_stage_points<T>(x, c.ld, frame0, n, d, xs);
        __syncthreads();                            // (the staged tile; the first time also the codebook)
        if (tid < n) {
            double best = mo_inf();
            int q = 0;
            for (int k = 0; k < K; ++k) {
                const double a = mo_dist2(xs, tid, cbs + k * d, d);
                if (a < best) {
                    best = a;
                    q = k;
                }
            }
            lab[tid] = q;
            least[tid] = best;
            if (c.soft) {
                const double den = 1e-9 + best;
                double sw = 0.0;
                for (int k = 0; k < K; ++k) sw = sw + exp(na * mo_dist2(xs, tid, cbs + k * d, d) / den);
                wsum[tid] = sw;
            }
        }
        __syncthreads();
        if (tid < K)
            for (int f = 0; f < n; ++f) {
                if (c.soft) {
                    const double w = exp(na * mo_dist2(xs, f, cbs + tid * d, d) / (1e-9 + least[f]));
                    acc = acc + w / wsum[f];
                } else {
                    acc = acc + (lab[f] == tid ? 1.0 : 0.0);
                }
            }
        __syncthreads();                            // (the next tile overwrites the points and the frames' values)
    }
    if (tid < K) raw[((int64_t)e * c.D + s) * K + tid] = acc;
}

template <typename T>
__global__ __launch_bounds__(kMoThreads) void k_mo_hist_norm(const double *raw, int32_t W, T *out, int64_t ldo) {
    __shared__ double total;
    const double *row = raw + (int64_t)blockIdx.x * W;
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int c = 0; c < W; ++c) s = s + row[c];
        total = s;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < W; c += kMoThreads) out[(int64_t)blockIdx.x * ldo + c] = (T)(row[c] / total);
}

}  // namespace klnmf
