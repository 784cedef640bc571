// Exact-arithmetic kernels (fp64 = the reference's arithmetic, or fp32): the
// four dense contractions of one multiplicative update as LDS-tiled VALU GEMMs
// with the element-wise work fused into their epilogues.  This is the mode the
// tight parity tests run; the throughput path is mfma.hip.h.
//
//   k_gemm<.., EpiQ<T, Weight>>   W.H -> Q=(V+eps)/(WH+eps) [* weight], loss partials   nmf.py:325-336, 297-310
//   k_gemm<.., EpiW<T, Fac>>      Q.H^T -> W*factor                                     nmf.py:338-343 (and :156 for W0)
//   k_gemm<.., EpiWpart<T, S>> + k_wrule_exact<T, Fac>   the same over feature chunks: slabs, then the rule from them
//   k_gemm<.., EpiN<T, S>>        W^T.Q split over row chunks -> partials               nmf.py:349
//   k_sum_partials<T, S> / k_update_H<T, Num, Fac> / k_update_H_part<T, Fac> + k_update_H_norm   nmf.py:349-350, array_utils.py:19-22
// ONE family for the unweighted cost function and for the two others, whose policies the headers that include this one bring: see
// "policies" below.
#pragma once
#include <type_traits>
#include "common.hip.h"

namespace klnmf {

constexpr int GT = 64;   // output tile edge
constexpr int GK = 16;   // contraction step

// MFMA accumulators and the 16 x 16 x 4 product in fp64 / fp32 (same operand layout: A[i][k] in lane i + 16 k, B[k][j] in lane
// j + 16 k; probed, experiments/micro/mfma_f64_probe.hip)
template <typename T> struct Acc4;
template <> struct Acc4<double> { typedef __attribute__((ext_vector_type(4))) double type; };
template <> struct Acc4<float> { typedef __attribute__((ext_vector_type(4))) float type; };
__device__ __forceinline__ Acc4<double>::type mfma_16x16x4(double a, double b, Acc4<double>::type c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ Acc4<float>::type mfma_16x16x4(float a, float b, Acc4<float>::type c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// row of the 16 x 16 result held in register rr of lane l (its column is l & 15): kLane (l >> 4) + kReg rr -- fp64 (l >> 4) + 4 rr,
// fp32 4 (l >> 4) + rr
template <typename T>
struct MfmaRow { static constexpr int kLane = sizeof(T) == 8 ? 1 : 4, kReg = sizeof(T) == 8 ? 4 : 1; };

// C[M,N] = A[M,K] . B[K,N]; element (r,c) of A is A[r*ars + c*acs] (so a
// transposed operand is a stride swap).  256 threads, TT x TT outputs each: tiles of 64 x 64 (TT = 4).
// blockIdx.z selects a contraction chunk [z*kchunk, (z+1)*kchunk).
// Round 4: with 4 x 4 outputs per thread every contraction step reads 8 operands from LDS for 16 multiply-adds -- in fp64
// that is 128 LDS cycles for 64 VALU cycles per step and workgroup: LDS-bound at a quarter of the fp64 peak (18 TFLOP/s
// measured), with element-wise bounds-checked staging on top.  Since: tiles that do not touch a matrix edge load without bounds
// checks; the next step's operands are prefetched into registers under the current step's arithmetic.  (8 x 8 outputs per thread,
// 128 x 128 tiles, balanced LDS and VALU time in that form; tried in round 4, instantiated nowhere since MF, and removed.)
// MF (64 x 64 tiles): the inner product on v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32 -- wave w owns rows 16 w .. 16 w + 15 of the tile and
// its four 16-column blocks; per 4 contraction steps one double of A and four of B per lane from the SAME LDS images (A[i][k]
// in lane i + 16 k, B[k][j] in lane j + 16 k; result register r of lane l: MfmaRow).  Same fp64 peak as the vector pipe on this
// part, a sixth of the LDS reads and a sixteenth of the instructions: the VALU form is LDS-bound at a quarter of that peak.  Round 1 had tried it and found no
// gain (526 vs 540 us at 2000 x 4096, k = 200) because the bounds-checked synchronous staging bound the kernel then.
template <typename T, typename Epi, int TT = 4, bool MF = false>
__global__ __launch_bounds__(256, 3) void k_gemm(int M, int N, int K, const T *A, int64_t ars,
                                              int64_t acs, const T *B, int64_t brs, int64_t bcs,
                                              int kchunk, const DevState *st, Epi epi) {
    if (st && st->stop) return;
#define KL_GEMM_ROW_TILE blockIdx.y
#include "gemm_body.hip.h"      // (the tile loop and the epilogue calls: shared with k_gemm_batch)
#undef KL_GEMM_ROW_TILE
}

// ---- the policies of the one family ---------------------------------------------------------------------------------------
// The unweighted, the weighted (an n x f buffer of weights: ElemWeight, FacDen) and the masked (weights of the form P[i][m(j)]:
// PresenceWeight, FacPresW, FacPresH) cost functions run the SAME kernels; what differs is named by three small policies, and the
// policies of the last two are defined beside the kernels only they run, not here.
//   element weight   of the ratio epilogue: NoWeight | ElemWeight (one per element) | PresenceWeight (one per row and column range)
//   numerator source of a rule: NumArray (summed before) | NumSlabs (summed here: T(0) + slab 0 + slab 1 ..., z ascending);
//                    either holds Fac::S buffer sets side by side -- the numerator, and the denominator where the factor wants one
//   rule factor      what multiplies the old value: FacNum / FacW0 (num) | FacDen (num / den) | FacPresW, FacPresH (num / the
//                    mask's collapsed denominator); den = 0 gives the factor 1 (w_factor)
// An unweighted instantiation holds no weight load, no multiplication by 1 and no test the others need.
struct NoWeight {
    __device__ NoWeight at(int, int, int64_t) const { return NoWeight{}; }
};

template <typename T, int S>
struct NumArray {
    const T *p[S];
    __device__ NumArray at(int64_t o) const {
        NumArray r;
#pragma unroll
        for (int s = 0; s < S; ++s) r.p[s] = p[s] + o;
        return r;
    }
    struct At {      // element j of each set, read where the factor uses it
        const NumArray &a; int64_t j;
        __device__ T operator[](int s) const { return a.p[s][j]; }
    };
    __device__ At get(int64_t j) const { return At{*this, j}; }
};
template <typename T, int S>
struct Sums {
    T v[S];
    __device__ T operator[](int s) const { return v[s]; }
};
template <typename T, int S>
struct NumSlabs {
    NumArray<T, S> first; int nslab; int64_t slab;      // slab 0 of each set, the number of slabs, elements per slab
    __device__ NumSlabs at(int64_t o) const { return NumSlabs{first.at(o), nslab, slab}; }
    __device__ Sums<T, S> get(int64_t j) const {
        static_assert(S <= 2, "numerator, denominator");
        T g = T(0), d = T(0);
        for (int z = 0; z < nslab; ++z) {
            g += first.p[0][z * slab + j];
            if constexpr (S == 2) d += first.p[1][z * slab + j];
        }
        if constexpr (S == 2) return Sums<T, 2>{{g, d}};
        else return Sums<T, 1>{{g}};
    }
};
// a rule's inputs as ONE kernel argument: an empty factor takes no room in it
template <typename Num, typename Fac>
struct RuleIn { Num num; [[no_unique_address]] Fac fac; };

// of(v, r, c): the factor of element (r, c) -- (sample, component) in the W rule, (component, column) in the H rule -- from its S sums
struct FacNum {
    static constexpr int S = 1;
    template <typename V> __device__ auto of(const V &v, int64_t, int64_t) const { return v[0]; }
};
struct FacW0 : FacNum {      // the unweighted W rule, which is also the start W0 = V.H0^T (multiply = 0: the numerator itself)
    int multiply;
    __device__ bool on() const { return multiply != 0; }
};

// Q = w * (V+eps)/(WH+eps) and the loss terms w * (x*log(q) - x + y) (metrics.py:18-20); NoWeight: no w at all.
template <typename T, typename Weight = NoWeight>
struct EpiQ {
    const T *V; [[no_unique_address]] Weight wt; T *Q; int64_t f; double *loss_part; int write_q; double local; T eps;
    __device__ void apply(int r, int c, T y) {
        const int64_t o = (int64_t)r * f + c;
        const T x = V[o];
        const auto w = wt.at(r, c, o);      // (NoWeight: nothing is read)
        const T q = (x + eps) / (y + eps);
        if constexpr (std::is_same<Weight, NoWeight>::value) {
            if (write_q) Q[o] = q;
            local += (double)(x * log(q) - x + y);
        } else {
            if (write_q) Q[o] = w * q;
            if (w != T(0)) local += (double)(w * (x * log(q) - x + y));      // (w = 0: a loss term of exactly 0)
        }
    }
    __device__ void finish(double *red) {
        const double t = block_sum(local, red);
        if (threadIdx.x == 0) loss_part[blockIdx.y * gridDim.x + blockIdx.x] = t;
    }
};

// W_new = W_old * factor (fac.on(); FacW0 with multiply = 0: W_new = the numerator).  Epilogue of the whole contraction -- one
// accumulator, or two from k_gemm_dual -- and the rule of k_wrule_exact behind a split one.
template <typename T, typename Fac>
struct EpiW {
    static constexpr int sets = Fac::S;
    const T *Wold; T *Wnew; int64_t k; [[no_unique_address]] Fac fac;
    template <typename V>
    __device__ void rule(int64_t o, int64_t r, int64_t c, const V &v) {
        Wnew[o] = fac.on() ? Wold[o] * fac.of(v, r, c) : fac.of(v, r, c);
    }
    __device__ void apply(int r, int c, T g) { rule((int64_t)r * k + c, r, c, Sums<T, 1>{{g}}); }
    __device__ void apply(int r, int c, T num, T den) { rule((int64_t)r * k + c, r, c, Sums<T, 2>{{num, den}}); }
    __device__ void finish(double *) {}
};

// Split contraction of the W rule (few rows: n*k/4096 output tiles would leave the chip idle while each walks all of
// f): blockIdx.z = chunk of the feature axis, partial Q.H^T into slab z of each of the S sets; k_wrule_exact sums the slabs
// in a fixed order.
template <typename T, int S = 1>
struct EpiWpart {
    static constexpr int sets = S;
    T *P[S]; int64_t k; int64_t slab;      // slab = n*k
    __device__ void apply(int r, int c, T g) { P[0][blockIdx.z * slab + (int64_t)r * k + c] = g; }
    __device__ void apply(int r, int c, T num, T den) {
        const int64_t o = blockIdx.z * slab + (int64_t)r * k + c;
        P[0][o] = num; P[1][o] = den;
    }
    __device__ void finish(double *) {}
};
template <typename T, typename Fac>
__global__ void k_wrule_exact(NumSlabs<T, Fac::S> part, const DevState *st, EpiW<T, Fac> epi) {
    if (st && st->stop) return;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < part.slab; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = e / epi.k;
        epi.rule(e, r, e - r * epi.k, part.get(e));
    }
}

// Plain store C[r][c] = acc (reconstruction GEMM, learner.py:80-84).
template <typename T>
struct EpiStore {
    T *C; int64_t ldc;
    __device__ void apply(int r, int c, T v) { C[(int64_t)r * ldc + c] = v; }
    __device__ void finish(double *) {}
};

// Partial numerator (S = 2: and denominator) of the H rule for one row chunk.
template <typename T, int S = 1>
struct EpiN {
    T *Npart[S]; int64_t f; int64_t slab;   // slab = k*f
    __device__ void apply(int r, int c, T v) { Npart[0][blockIdx.z * slab + (int64_t)r * f + c] = v; }
    __device__ void apply(int r, int c, T num, T den) {
        const int64_t o = blockIdx.z * slab + (int64_t)r * f + c;
        Npart[0][o] = num; Npart[1][o] = den;
    }
    __device__ void finish(double *) {}
};

template <typename T, int S>
struct OutSets { T *p[S]; };
template <typename T, int S>
__global__ void k_sum_partials(NumArray<T, S> part, OutSets<T, S> out, int64_t count, int nslab, const DevState *st) {
    if (st && st->stop) return;
    const NumSlabs<T, S> slabs{part, nslab, count};
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < count;
         e += (int64_t)gridDim.x * blockDim.x) {
        const Sums<T, S> v = slabs.get(e);
#pragma unroll
        for (int s = 0; s < S; ++s) out.p[s][e] = v[s];
    }
}

// The product of the H rule, written once: row[j] <- row[j] * factor over j0 + tid, + 256, ... < j1; returns the thread's fp64
// sum of the products.
template <typename T, typename Num, typename Fac>
__device__ __forceinline__ double h_product(T *row, const Num &num, const Fac &fac, int64_t a, int64_t j0, int64_t j1) {
    double s = 0;
    for (int64_t j = j0 + threadIdx.x; j < j1; j += blockDim.x) {
        const auto nv = num.get(j);      // (slabs: summed here, in front of the read of row[j])
        const T v = row[j] * fac.of(nv, a, j);
        row[j] = v;
        s += (double)v;
    }
    return s;
}

// H <- H*factor, rows divided by (1e-16 + row sum).  One block per component row.  Num = NumSlabs (single-context loops): the
// rule straight from the row chunks' slabs, summed in k_sum_partials' order -- one launch instead of two, the same bits.
template <typename T, typename Num, typename Fac>
__global__ __launch_bounds__(256) void k_update_H(T *H, RuleIn<Num, Fac> in, int64_t f, const DevState *st) {
    if (st && st->stop) return;
    __shared__ double red[16];
    __shared__ double total;
    T *row = H + blockIdx.x * f;
    const double s = h_product(row, in.num.at(blockIdx.x * f), in.fac, (int64_t)blockIdx.x, 0, f);
    const double t = block_sum(s, red);
    if (threadIdx.x == 0) total = t;
    __syncthreads();
    const T d = (T)(kEpsNorm + total);
    for (int64_t j = threadIdx.x; j < f; j += blockDim.x) row[j] = row[j] / d;
}

// The same rule for long rows (round 4: the CSR problems have f = 110 000 columns and k = 50 components -- 50 blocks walked
// 880 KB each, three dependent passes: 0.33 ms of a 3.3 ms iteration): the row in S segments, two launches, no communication
// inside a launch.  k_update_H_part: H * factor written back + the segment's fp64 partial sum; k_update_H_norm: every block adds
// the row's S partial sums in the same fixed order and divides its segment.
template <typename T, typename Fac>
__global__ __launch_bounds__(256) void k_update_H_part(T *H, RuleIn<NumArray<T, Fac::S>, Fac> in, int64_t f, int64_t seg,
                                                       double *part, const DevState *st) {
    if (st && st->stop) return;
    __shared__ double red[16];
    const int64_t a = blockIdx.y, j0 = blockIdx.x * seg, j1 = min(f, j0 + seg);
    const double s = h_product(H + a * f, in.num.at(a * f), in.fac, a, j0, j1);
    const double t = block_sum(s, red);
    if (threadIdx.x == 0) part[a * gridDim.x + blockIdx.x] = t;
}
template <typename T>
__global__ __launch_bounds__(256) void k_update_H_norm(T *H, int64_t f, int64_t seg, const double *part, const DevState *st) {
    if (st && st->stop) return;
    const int64_t a = blockIdx.y, j0 = blockIdx.x * seg, j1 = min(f, j0 + seg);
    double total = 0;
    for (unsigned z = 0; z < gridDim.x; ++z) total += part[a * gridDim.x + z];      // (every thread: the same order, the same bits)
    const T d = (T)(kEpsNorm + total);
    T *row = H + a * f;
    for (int64_t j = j0 + threadIdx.x; j < j1; j += blockDim.x) row[j] = row[j] / d;
}

// The stop rule of nmf.py:214-220 behind a one-block loss reduction (single-context loops of the exact modes: k_decide as a
// launch of its own is a seventh of a small problem's iteration).
struct DecideArgs {
    int on;                   // 0: the loss only (it is exchanged or read by the caller; the rule follows elsewhere)
    DevState *st_rw;
    double tol_abs;
    double *errors;
    int64_t cap;
};
__device__ __forceinline__ void decide_here(const DecideArgs &d, double err) {
    if (!d.on) return;
    if (d.st_rw->prev_err - err < d.tol_abs) {
        d.st_rw->stop = 1;
        return;
    }
    d.st_rw->prev_err = err;
    d.st_rw->prev2[0] = err; d.st_rw->prev2[1] = err;
    if (d.st_rw->n_done < d.cap) d.errors[d.st_rw->n_done] = err;
    d.st_rw->n_done += 1;
}

// Sum of `count` doubles in a fixed order (deterministic), one block.
KL_GLOBAL __launch_bounds__(1024) void k_sum_doubles(const double *part, int64_t count,
                                                      double *out, const DevState *st,
                                                      DecideArgs dec = DecideArgs{0, nullptr, 0.0, nullptr, 0}) {
    if (st && st->stop) return;
    __shared__ double red[16];
    double s = 0;
    for (int64_t e = threadIdx.x; e < count; e += blockDim.x) s += part[e];
    const double t = block_sum(s, red);
    if (threadIdx.x == 0) { out[0] = t; out[1] = 0; decide_here(dec, t); }
}

// V[row0+i, col0+j] = scale * src[i, j]  (learner.py:53-56 fused into the upload).
template <typename T, typename S>
__global__ void k_place_V(T *V, int64_t f, const S *src, int64_t rows, int64_t cols, int64_t ld,
                          int64_t row0, int64_t col0, double scale, const int64_t *row_idx = nullptr) {
    const int64_t total = rows * cols;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e / cols, j = e % cols;
        V[(row0 + i) * f + col0 + j] = (T)(scale * (double)src[(row_idx ? row_idx[i] : i) * ld + j]);
    }
}

template <typename D, typename S>
__global__ void k_convert(D *dst, const S *src, int64_t count) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < count;
         e += (int64_t)gridDim.x * blockDim.x)
        dst[e] = (D)src[e];
}

// generalized_KL of two flat arrays (metrics.py:18-20), partial per block.
template <typename T>
__global__ __launch_bounds__(256) void k_gkl(const T *x, const T *y, int64_t count, double eps,
                                             double *part) {
    __shared__ double red[16];
    double s = 0;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < count;
         e += (int64_t)gridDim.x * blockDim.x) {
        const double xv = (double)x[e], yv = (double)y[e];
        s += xv * log((xv + eps) / (yv + eps)) - xv + yv;
    }
    const double t = block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// ---- pairwise distances for the nearest-neighbour evaluation (next-row N4) --------------------------
// out[i][j] = measure(A[i, :], B[j, :]) for the measures of metrics.py:58-86 (as used by
// evaluation.py:103-116 `all_distances`, which broadcasts [n_a,1,d] x [1,n_b,d]).  One wave per pair.
enum DistMetric { DIST_KL = 0, DIST_REV_KL = 1, DIST_SYM_KL = 2, DIST_FROBENIUS = 3, DIST_COSINE_DIFF = 4 };

// The terms of one element and the closing expression of a pair: the one text k_all_distances and k_nearest (nearest.hip.h) are
// both compiled from, so that the two agree bit for bit.  Where the compiler's contraction decides by the code AROUND a
// statement, the rounding is written out (fma / dist_mul_rounded): k_all_distances adds the term of every measure to s0 in one
// shared instruction, so its Frobenius and x.y products are rounded before that add, while its x.x and y.y sums are fused --
// those are the roundings it has always had.  A KL term has one product and its own subtraction behind it: fused in any context.
__device__ __forceinline__ double dist_mul_rounded(double x, double y) {
#pragma clang fp contract(off)
    return x * y;
}
__device__ __forceinline__ void dist_term_kl(double x, double y, double eps, double &s0, double &s1) {
    const double l = log((x + eps) / (y + eps));
    s0 += x * l - x + y;                    // generalized_KL(a, b)
    s1 += -y * l - y + x;                   // generalized_KL(b, a): log((y+eps)/(x+eps)) = -l
}
__device__ __forceinline__ void dist_term_frobenius(double x, double y, double &s0) { s0 += dist_mul_rounded(x - y, x - y); }
__device__ __forceinline__ void dist_term_cosine(double x, double y, double &s0, double &s1, double &s2) {
    s0 += dist_mul_rounded(x, y); s1 = fma(x, x, s1); s2 = fma(y, y, s2);
}
__device__ __forceinline__ double dist_close(int metric, double s0, double s1, double s2) {
    switch (metric) {
        case DIST_KL: return s0;
        case DIST_REV_KL: return s1;
        case DIST_SYM_KL: return 0.5 * (s0 + s1);
        case DIST_FROBENIUS: return sqrt(s0);
        default: return -(s0 / (sqrt(s1 * s2) + (s0 == 0.0 ? 1.0 : 0.0)));     // metrics.py:71-77
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_all_distances(const T *A, const T *B, T *out, int64_t na, int64_t nb,
                                                        int64_t d, int metric, double eps, int64_t lda = -1, int64_t ldb = -1) {
    if (lda < 0) lda = d;
    if (ldb < 0) ldb = d;
    const int lane = threadIdx.x & 63;
    const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= na * nb) return;
    const int64_t i = pair / nb, j = pair % nb;
    const T *a = A + i * lda, *b = B + j * ldb;
    double s0 = 0, s1 = 0, s2 = 0;
    for (int64_t e = lane; e < d; e += 64) {
        const double x = (double)a[e], y = (double)b[e];
        if (metric <= DIST_SYM_KL) dist_term_kl(x, y, eps, s0, s1);
        else if (metric == DIST_FROBENIUS) dist_term_frobenius(x, y, s0);
        else dist_term_cosine(x, y, s0, s1, s2);
    }
    s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2);
    if (lane != 0) return;
    out[pair] = (T)dist_close(metric, s0, s1, s2);
}

}  // namespace klnmf
