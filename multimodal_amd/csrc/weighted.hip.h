// Weighted / masked KL-NMF on the exact kernels (KLNMF_PREC_F64 / F32, dense): the multiplicative update of
// sum Om o d(V | W.H) with Om >= 0 an n x f buffer beside V (klnmf_upload_weights; nmf.py:159-175 documents `weights` and never
// reads it).  With Y = W.H, Q = (V + eps) / (Y + eps) and R = Om o Q:
//   k_gemm<.., EpiQ<T, ElemWeight>>      W.H -> R, loss partials of Om o (V log Q - V + Y)   (Om = 0: R = 0, a loss term of exactly 0)
//   k_gemm_dual<.., EpiW<T, FacDen>, A>   (R.H^T, Om.H^T) -> W * num / den                   the B tile H^T is shared
//   k_gemm_dual<.., EpiN<T, 2>, B>        (W^T.R, W^T.Om) split over row chunks -> two slab sets   the A tile W^T is shared
//   k_sum_partials<T, 2>, k_update_H / k_update_H_part / k_wrule_exact under FacDen           the rules: factor = den > 0 ? num / den : 1
// The kernels of the rules and the epilogues are the one family of exact.hip.h under the policies ElemWeight (here) and FacDen; this
// file holds what only a weighted problem runs: k_gemm_dual, ElemWeight and k_fill.
// The denominators Om.H^T and W^T.Om do not collapse to the constants they are in the reference's rule (H's row sums 1, W's
// column sums cancelling in the normalisation), so an iteration has five contractions of n f k instead of three; the two that
// share an operand are formed in ONE pass over its LDS image.  Slabs, chunks and segments are the unweighted plan's
// (plan.hip.h): each route has a numerator and a denominator slab set, summed in the same fixed order.
#pragma once
#include "exact.hip.h"

namespace klnmf {

// the weight of element (r, c) = offset o of the n x f buffers
template <typename T>
struct ElemWeight {
    const T *Om;
    __device__ T at(int, int, int64_t o) const { return Om[o]; }
};

// the factor of both rules: the denominator beside the numerator; den = 0 (nothing observed) keeps the old value
template <typename T>
__device__ __forceinline__ T w_factor(T num, T den) { return den > T(0) ? num / den : T(1); }

struct FacDen {
    static constexpr int S = 2;
    __device__ bool on() const { return true; }
    template <typename V> __device__ auto of(const V &v, int64_t, int64_t) const { return w_factor(v[0], v[1]); }
};

// Two products that share one operand, 64 x 64 output tiles of both, the inner product on v_mfma_f64_16x16x4_f64 /
// v_mfma_f32_16x16x4_f32 in k_gemm's MF lane layout (exact.hip.h: wave w owns rows 16 w .. 16 w + 15 and the four 16-column
// blocks; A[i][k] in lane i + 16 k, B[k][j] in lane j + 16 k).
//   SHARE_B  C1 = A.B, C2 = X2.B   X2 indexed as A (form A: A = R, X2 = Om, B = H^T)
//   else     C1 = A.B, C2 = A.X2   X2 indexed as B (form B: A = W^T, B = R, X2 = Om)
// Three LDS images per contraction step (26 KiB in fp64), two accumulator sets per wave (2 x 16 registers per lane), the
// next step's three operands prefetched into registers (12 values per lane) under the current step's 32 MFMAs; per four
// contraction steps 6 (form A) or 9 (form B) LDS reads feed 8 MFMAs, where two k_gemm launches read 10 and stage the shared
// operand twice.  Staging, edge handling, chunking over blockIdx.z and the summation order of an output element are k_gemm's.
template <typename T, typename Epi, bool SHARE_B>
__global__ __launch_bounds__(256, 2) void k_gemm_dual(int M, int N, int K, const T *A, int64_t ars, int64_t acs,
                                                      const T *B, int64_t brs, int64_t bcs, const T *X2, int kchunk,
                                                      const DevState *st, Epi epi) {
    if (st && st->stop) return;
#define KL_GEMM_DUAL_ROW_TILE blockIdx.y
#include "gemm_dual_body.hip.h"      // (the tile loop and the epilogue calls: shared with k_gemm_dual_batch)
#undef KL_GEMM_DUAL_ROW_TILE
}

// the weight buffer before its first block: all ones
template <typename T>
__global__ void k_fill(T *dst, int64_t count, T value) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < count; e += (int64_t)gridDim.x * blockDim.x) dst[e] = value;
}

}  // namespace klnmf
