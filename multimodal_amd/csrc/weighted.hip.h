// Weighted / masked KL-NMF on the exact kernels (KLNMF_PREC_F64 / F32, dense): the multiplicative update of
// sum Om o d(V | W.H) with Om >= 0 an n x f buffer beside V (klnmf_upload_weights; nmf.py:159-175 documents `weights` and never
// reads it).  With Y = W.H, Q = (V + eps) / (Y + eps) and R = Om o Q:
//   k_gemm<.., EpiQw>        W.H -> R, loss partials of Om o (V log Q - V + Y)        (Om = 0: R = 0, a loss term of exactly 0)
//   k_gemm_dual<.., form A>  (R.H^T, Om.H^T) -> W * num / den                         the B tile H^T is shared
//   k_gemm_dual<.., form B>  (W^T.R, W^T.Om) split over row chunks -> two slab sets   the A tile W^T is shared
//   k_sum_partials_w / k_update_H_w / _part_w / _slabs_w, k_wrule_exact_w              the rules: factor = den > 0 ? num / den : 1
// The denominators Om.H^T and W^T.Om do not collapse to the constants they are in the reference's rule (H's row sums 1, W's
// column sums cancelling in the normalisation), so an iteration has five contractions of n f k instead of three; the two that
// share an operand are formed in ONE pass over its LDS image.  Slabs, chunks and segments are the unweighted plan's
// (plan.hip.h): each route has a numerator and a denominator slab set, summed in the same fixed order.
#pragma once
#include "exact.hip.h"

namespace klnmf {

template <typename T>
__device__ __forceinline__ T w_factor(T num, T den) { return den > T(0) ? num / den : T(1); }

// R = Om * (V+eps)/(WH+eps) and the loss terms Om * (x*log(q) - x + y).
template <typename T>
struct EpiQw {
    const T *V; const T *Om; T *R; int64_t f; double *loss_part; int write_q; double local; T eps;
    __device__ void apply(int r, int c, T y) {
        const int64_t o = (int64_t)r * f + c;
        const T x = V[o], om = Om[o];
        const T q = (x + eps) / (y + eps);
        if (write_q) R[o] = om * q;
        if (om != T(0)) local += (double)(om * (x * log(q) - x + y));
    }
    __device__ void finish(double *red) {
        const double t = block_sum(local, red);
        if (threadIdx.x == 0) loss_part[blockIdx.y * gridDim.x + blockIdx.x] = t;
    }
};

template <typename T> struct Acc4;
template <> struct Acc4<double> { typedef __attribute__((ext_vector_type(4))) double type; };
template <> struct Acc4<float> { typedef __attribute__((ext_vector_type(4))) float type; };
__device__ __forceinline__ Acc4<double>::type mfma_16x16x4(double a, double b, Acc4<double>::type c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ Acc4<float>::type mfma_16x16x4(float a, float b, Acc4<float>::type c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

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
            // result register rr of lane l: fp64 D[(l >> 4) + 4 rr][l & 15]; fp32 D[4 (l >> 4) + rr][l & 15] (exact.hip.h)
            const int r = m0 + 16 * wv + (sizeof(T) == 8 ? (lane >> 4) + 4 * rr : 4 * (lane >> 4) + rr), c = n0 + 16 * t + (lane & 15);
            if (r < M && c < N) epi.apply(r, c, acc1[t][rr], acc2[t][rr]);
        }
}

// W_new = W_old * (R.H^T) / (Om.H^T); a sample with no observed entry (denominator 0) keeps its coefficients.
template <typename T>
struct EpiW2 {
    const T *Wold; T *Wnew; int64_t k;
    __device__ void apply(int r, int c, T num, T den) {
        const int64_t o = (int64_t)r * k + c;
        Wnew[o] = Wold[o] * w_factor(num, den);
    }
};

// Split contraction of the weighted W rule (EpiWpart's layout, twice): slab z of the numerator and of the denominator.
template <typename T>
struct EpiW2part {
    T *P; T *D; int64_t k; int64_t slab;      // slab = n*k
    __device__ void apply(int r, int c, T num, T den) {
        const int64_t o = blockIdx.z * slab + (int64_t)r * k + c;
        P[o] = num; D[o] = den;
    }
};
template <typename T>
__global__ void k_wrule_exact_w(const T *part, const T *dpart, int nslab, int64_t count, const T *Wold, T *Wnew,
                                const DevState *st) {
    if (st && st->stop) return;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < count; e += (int64_t)gridDim.x * blockDim.x) {
        T g = T(0), d = T(0);
        for (int z = 0; z < nslab; ++z) { g += part[z * count + e]; d += dpart[z * count + e]; }
        Wnew[e] = Wold[e] * w_factor(g, d);
    }
}

// Partial numerator and denominator of the weighted H rule for one row chunk (EpiN's layout, twice).
template <typename T>
struct EpiN2 {
    T *Npart; T *Dpart; int64_t f; int64_t slab;   // slab = k*f
    __device__ void apply(int r, int c, T num, T den) {
        const int64_t o = blockIdx.z * slab + (int64_t)r * f + c;
        Npart[o] = num; Dpart[o] = den;
    }
};

// both slab sets in k_sum_partials' order
template <typename T>
__global__ void k_sum_partials_w(const T *part, const T *dpart, T *out, T *dout, int64_t count, int nslab, const DevState *st) {
    if (st && st->stop) return;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < count; e += (int64_t)gridDim.x * blockDim.x) {
        T s = T(0), d = T(0);
        for (int z = 0; z < nslab; ++z) { s += part[z * count + e]; d += dpart[z * count + e]; }
        out[e] = s; dout[e] = d;
    }
}

// H <- H * num / den (factor 1 where den = 0), rows divided by (1e-16 + row sum): k_update_H with the weighted factor.
template <typename T>
__global__ __launch_bounds__(256) void k_update_H_w(T *H, const T *num, const T *den, int64_t f, const DevState *st) {
    if (st && st->stop) return;
    __shared__ double red[16];
    __shared__ double total;
    T *row = H + blockIdx.x * f;
    const T *nrow = num + blockIdx.x * f, *drow = den + blockIdx.x * f;
    double s = 0;
    for (int64_t j = threadIdx.x; j < f; j += blockDim.x) {
        const T v = row[j] * w_factor(nrow[j], drow[j]);
        row[j] = v;
        s += (double)v;
    }
    const double t = block_sum(s, red);
    if (threadIdx.x == 0) total = t;
    __syncthreads();
    const T d = (T)(kEpsNorm + total);
    for (int64_t j = threadIdx.x; j < f; j += blockDim.x) row[j] = row[j] / d;
}

// ... for long rows: the segment's product and partial sum (k_update_H_part); k_update_H_norm follows unchanged.
template <typename T>
__global__ __launch_bounds__(256) void k_update_H_part_w(T *H, const T *num, const T *den, int64_t f, int64_t seg, double *part,
                                                         const DevState *st) {
    if (st && st->stop) return;
    __shared__ double red[16];
    const int64_t a = blockIdx.y, j0 = blockIdx.x * seg, j1 = min(f, j0 + seg);
    T *row = H + a * f;
    const T *nrow = num + a * f, *drow = den + a * f;
    double s = 0;
    for (int64_t j = j0 + threadIdx.x; j < j1; j += blockDim.x) {
        const T v = row[j] * w_factor(nrow[j], drow[j]);
        row[j] = v;
        s += (double)v;
    }
    const double t = block_sum(s, red);
    if (threadIdx.x == 0) part[a * gridDim.x + blockIdx.x] = t;
}

// ... straight from the row chunks' two slab sets (k_update_H_slabs): the bits of k_sum_partials_w + k_update_H_w.
template <typename T>
__global__ __launch_bounds__(256) void k_update_H_slabs_w(T *H, const T *part, const T *dpart, int nslab, int64_t slab, int64_t f,
                                                          const DevState *st) {
    if (st && st->stop) return;
    __shared__ double red[16];
    __shared__ double total;
    T *row = H + blockIdx.x * f;
    const T *prow = part + blockIdx.x * f, *qrow = dpart + blockIdx.x * f;
    double s = 0;
    for (int64_t j = threadIdx.x; j < f; j += blockDim.x) {
        T nj = T(0), dj = T(0);
        for (int z = 0; z < nslab; ++z) { nj += prow[z * slab + j]; dj += qrow[z * slab + j]; }
        const T v = row[j] * w_factor(nj, dj);
        row[j] = v;
        s += (double)v;
    }
    const double t = block_sum(s, red);
    if (threadIdx.x == 0) total = t;
    __syncthreads();
    const T d = (T)(kEpsNorm + total);
    for (int64_t j = threadIdx.x; j < f; j += blockDim.x) row[j] = row[j] / d;
}

// the weight buffer before its first block: all ones
template <typename T>
__global__ void k_fill(T *dst, int64_t count, T value) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < count; e += (int64_t)gridDim.x * blockDim.x) dst[e] = value;
}

}  // namespace klnmf
