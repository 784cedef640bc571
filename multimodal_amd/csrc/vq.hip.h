// The vector quantiser of the feature units, once: k_hac_vq (hac.hip.h) and k_km_assign (kmeans.hip.h) label a
// frame with it, and motion.hip.h's own loop (an alive mask, fp64 staging, the distance returned) obeys the same rule.
//
// THE RULE (features.hac.quantize's, scipy's vq): the label of a frame is the index of the nearest codebook row by the squared
// distance formed in fp64, j ascending, every difference, product and sum rounded on its own; strict `<`, so the lowest index keeps
// a tie and a NaN distance never gets ahead.
//
// "Rounded on its own" needs the compiler's contraction of a product and a sum into a fused multiply-add off; device code has it
// on by default.  __dsub_rn / __dmul_rn / __dadd_rn do not help: under hipcc they are the plain operators inside a compiler header
// parsed with the default, so a loop written with them still compiles to fused multiply-adds.  Hence plain operators under the
// pragma below.  At file scope it lasts to the end of the including unit: each feature unit includes only its own kernels after
// this header, all of which want the same (k_hac_pass and k_hac_scan are integer work).
//
// A workgroup is kVqTile = 256 threads, a thread per frame of a tile.  Where the host found room in LDS (vq_staging) the codebook
// is staged as it lies, [K, d], and the tile's frames transposed (element j of frame f at j * kVqFrameStride + f: lanes read
// neighbouring words).
#pragma once
#pragma clang fp contract(off)

namespace klnmf {

constexpr int kVqTile = 256;                        // frames per tile = threads per workgroup
constexpr int kVqFrameStride = kVqTile + 1;         // words between the elements j, j + 1 of a staged frame (bank spread)

enum { VQ_STAGE_CODEBOOK = 1, VQ_STAGE_FRAMES = 2 };

// What a launch stages beside the `used` bytes of LDS it needs anyway, within `budget`: the codebook first, then the frame tile.
// Returns the VQ_STAGE_* bits; `used` becomes the dynamic LDS of the launch.
inline int vq_staging(size_t el, int64_t K, int64_t d, size_t budget, size_t *used) {
    const size_t cb_bytes = (size_t)K * d * el, x_bytes = (size_t)kVqFrameStride * d * el;
    int stage = 0;
    if (*used + cb_bytes <= budget) { stage |= VQ_STAGE_CODEBOOK; *used += cb_bytes; }
    if (*used + x_bytes <= budget) { stage |= VQ_STAGE_FRAMES; *used += x_bytes; }
    return stage;
}

// The code of one frame `xp[j * sx]` (j < d) against the codebook rows cb + k * ldc.
template <typename T>
__device__ __forceinline__ int vq_nearest_code(const T *xp, int64_t sx, const T *cb, int64_t ldc, int K, int d) {
    double best = __longlong_as_double(0x7ff0000000000000LL);
    int q = 0, k = 0;
    // four rows at a time: the frame's element is read once for the four, and four independent sums are in flight (a workgroup
    // with its accumulators in LDS is often alone on its CU, one wave per SIMD).  Each row's sum is formed exactly as below.
    for (; k + 4 <= K; k += 4) {
        const T *c0 = cb + (int64_t)k * ldc, *c1 = c0 + ldc, *c2 = c1 + ldc, *c3 = c2 + ldc;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        for (int j = 0; j < d; ++j) {
            const double xv = (double)xp[(int64_t)j * sx];
            const double d0 = xv - (double)c0[j], d1 = xv - (double)c1[j], d2 = xv - (double)c2[j], d3 = xv - (double)c3[j];
            a0 = a0 + d0 * d0;
            a1 = a1 + d1 * d1;
            a2 = a2 + d2 * d2;
            a3 = a3 + d3 * d3;
        }
        if (a0 < best) { best = a0; q = k; }    // in ascending order, strict: as below
        if (a1 < best) { best = a1; q = k + 1; }
        if (a2 < best) { best = a2; q = k + 2; }
        if (a3 < best) { best = a3; q = k + 3; }
    }
    for (; k < K; ++k) {
        const T *c = cb + (int64_t)k * ldc;
        double acc = 0.0;
        for (int j = 0; j < d; ++j) {
            const double df = (double)xp[(int64_t)j * sx] - (double)c[j];
            acc = acc + df * df;
        }
        const bool ahead = acc < best;          // strict: the lowest index keeps a tie, a NaN never wins
        best = ahead ? acc : best;
        q = ahead ? k : q;
    }
    return q;
}

// The codebook [K, d] (rows ldc apart) into cbs, by the whole workgroup; the caller synchronises.
template <typename T>
__device__ __forceinline__ void vq_stage_codebook(T *cbs, const T *cb, int64_t ldc, int Kd, int d) {
    for (int e = threadIdx.x; e < Kd; e += kVqTile) cbs[e] = cb[(int64_t)(e / d) * ldc + e % d];
}

// The tile's n <= 256 frames from frame0 on into xs, transposed, the frames beyond n as zeros; the caller synchronises.
template <typename T>
__device__ __forceinline__ void vq_stage_frames(T *xs, const T *x, int64_t ldx, int64_t frame0, int n, int d) {
    for (int e = threadIdx.x; e < kVqTile * d; e += kVqTile) {
        const int f = e / d, j = e % d;
        xs[j * kVqFrameStride + f] = f < n ? x[(frame0 + f) * ldx + j] : (T)0;
    }
}

// The code of this thread's frame t = frame0 + threadIdx.x, read from wherever `stage` says the frames and the codebook are.
template <typename T>
__device__ __forceinline__ int vq_code(int stage, const T *x, int64_t ldx, int64_t t, const T *xs, const T *cb, int64_t ldc,
                                       const T *cbs, int K, int d) {
    if (stage & VQ_STAGE_FRAMES) {
        if (stage & VQ_STAGE_CODEBOOK) return vq_nearest_code<T>(xs + threadIdx.x, kVqFrameStride, cbs, d, K, d);
        return vq_nearest_code<T>(xs + threadIdx.x, kVqFrameStride, cb, ldc, K, d);
    }
    if (stage & VQ_STAGE_CODEBOOK) return vq_nearest_code<T>(x + t * ldx, 1, cbs, d, K, d);
    return vq_nearest_code<T>(x + t * ldx, 1, cb, ldc, K, d);
}

}  // namespace klnmf
