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
    __shared__ T As[GK][GT + 4];
    __shared__ T Bs[GK][GT + 4];
    __shared__ T Xs[GK][GT + 4];
    const int tid = threadIdx.x;
    const int m0 = blockIdx.y * GT, n0 = blockIdx.x * GT;
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
}

// the weight buffer before its first block: all ones
template <typename T>
__global__ void k_fill(T *dst, int64_t count, T value) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < count; e += (int64_t)gridDim.x * blockDim.x) dst[e] = value;
}

}  // namespace klnmf
