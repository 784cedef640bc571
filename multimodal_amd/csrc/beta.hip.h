// Beta-divergence NMF on the exact kernels (KLNMF_PREC_F64 / F32, dense): the majorise-minimise multiplicative update of
// sum Om o d_beta(x | y), x = V + eps, y = W.H + eps, beta != 1 (nmf.py:293 announces "Helpers for beta divergence and related
// updates" and holds none: the reference has no counterpart).  With
//   A = Om o x o y^(beta-2)      B = Om o y^(beta-1)
// the rules are W <- W o ((A.H^T) / (B.H^T))^gamma and H <- H o ((W^T.A) / (W^T.B))^gamma, gamma = 1/(2-beta) below beta = 1,
// 1 up to beta = 2, 1/(beta-1) above: the shape of the weighted KL rules (weighted.hip.h) with B where those pass Om.
//   k_gemm<.., EpiBeta<T, Weight, LOSS, KIND>>   W.H -> A (the Q buffer), B (its own n x f buffer), loss partials of Om o d_beta
//   k_gemm_dual<.., EpiW<T, FacBeta<T>>, A>       (A.H^T, B.H^T) -> W * (num / den)^gamma          the tile of H^T shared
//   k_gemm_dual<.., EpiN<T, 2>, B>                (W^T.A, W^T.B) split over row chunks               the tile of W^T shared
//   k_wrule_exact / k_update_H_part under FacBeta; k_update_H_sums: k_update_H that also leaves every row's sum
//   k_scale_W_cols                                W[:, a] *= sum[a]: the normalisation of H's rows leaves W.H as it was
// The policies of the one family (exact.hip.h) that only a beta problem runs: the ratio epilogue EpiBeta and the factor FacBeta.
// Powers are exp(c * log(y)): one log per element serves y^(beta-2) and, times y, y^(beta-1); beta = 2 and beta = 0 need none.
#pragma once
#include "exact.hip.h"
#include "weighted.hip.h"

namespace klnmf {

enum BetaKind { BETA_TWO = 0, BETA_ZERO = 1, BETA_GEN = 2 };

// d_beta(x | y) and the two factors of the rules' matrices, a = x y^(beta-2) and b = y^(beta-1); x, y > 0
template <typename T, int KIND, bool LOSS>
__device__ __forceinline__ void beta_terms(T x, T y, T beta, T &a, T &b, T &d) {
    if constexpr (KIND == BETA_TWO) {
        a = x; b = y;
        if constexpr (LOSS) { const T r = x - y; d = T(0.5) * r * r; }
    } else if constexpr (KIND == BETA_ZERO) {
        const T inv = T(1) / y;
        b = inv; a = x * inv * inv;
        if constexpr (LOSS) { const T q = x * inv; d = q - log(q) - T(1); }
    } else {
        const T p2 = exp((beta - T(2)) * log(y));      // y^(beta-2)
        a = x * p2; b = p2 * y;                          // y^(beta-1) = y^(beta-2) y
        if constexpr (LOSS) {
            const T xb = exp(beta * log(x));             // x^beta;  y^beta = b y
            d = (xb + (beta - T(1)) * (b * y) - beta * (x * b)) / (beta * (beta - T(1)));
        }
    }
}

// The ratio epilogue of a beta problem: A into the Q buffer, B beside it, the loss partials in fp64 as EpiQ leaves them.
// Om = 0: A = B = 0 and a loss term of exactly 0, whatever V holds there.
template <typename T, typename Weight, bool LOSS, int KIND>
struct EpiBeta {
    const T *V; [[no_unique_address]] Weight wt; T *A; T *Bm; int64_t f; double *loss_part; double local; T eps; T beta;
    __device__ void apply(int r, int c, T wh) {
        const int64_t o = (int64_t)r * f + c;
        T a, b, d = T(0);
        if constexpr (std::is_same<Weight, NoWeight>::value) {
            beta_terms<T, KIND, LOSS>(V[o] + eps, wh + eps, beta, a, b, d);
            A[o] = a; Bm[o] = b;
            if constexpr (LOSS) local += (double)d;
        } else {
            const T w = wt.at(r, c, o);
            if (w != T(0)) {
                beta_terms<T, KIND, LOSS>(V[o] + eps, wh + eps, beta, a, b, d);
                A[o] = w * a; Bm[o] = w * b;
                if constexpr (LOSS) local += (double)(w * d);
            } else {
                A[o] = T(0); Bm[o] = T(0);
            }
        }
    }
    __device__ void finish(double *red) {
        if constexpr (LOSS) {
            const double t = block_sum(local, red);
            if (threadIdx.x == 0) loss_part[blockIdx.y * gridDim.x + blockIdx.x] = t;
        }
    }
};

// the factor of both rules: (num / den)^gamma, gamma <= 1; den = 0 (nothing observed) keeps the old value; gamma = 1: no power
template <typename T>
struct FacBeta {
    static constexpr int S = 2;
    T gamma;
    __device__ bool on() const { return true; }
    template <typename V> __device__ T of(const V &v, int64_t, int64_t) const {
        const T num = v[0], den = v[1];
        if (!(den > T(0))) return T(1);
        const T q = num / den;
        return gamma == T(1) ? q : exp(gamma * log(q));      // (q = 0: exp(-inf) = 0)
    }
};

// k_update_H (exact.hip.h: H <- H * factor, rows divided by 1e-16 + row sum) that also leaves each row's sum in sums[a]
template <typename T, typename Num, typename Fac>
__global__ __launch_bounds__(256) void k_update_H_sums(T *H, RuleIn<Num, Fac> in, int64_t f, double *sums, const DevState *st) {
    if (st && st->stop) return;
    __shared__ double red[16];
    __shared__ double total;
    T *row = H + blockIdx.x * f;
    const double s = h_product(row, in.num.at(blockIdx.x * f), in.fac, (int64_t)blockIdx.x, 0, f);
    const double t = block_sum(s, red);
    if (threadIdx.x == 0) { total = t; sums[blockIdx.x] = t; }
    __syncthreads();
    const T d = (T)(kEpsNorm + total);
    for (int64_t j = threadIdx.x; j < f; j += blockDim.x) row[j] = row[j] / d;
}

// W[:, a] *= the sum of row a of H before its normalisation: part[a * nseg + z], z ascending (k_update_H_norm's order; nseg = 1:
// k_update_H_sums' sums)
template <typename T>
__global__ __launch_bounds__(256) void k_scale_W_cols(T *W, int64_t count, int64_t k, const double *part, int nseg, const DevState *st) {
    if (st && st->stop) return;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < count; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t a = e % k;
        double total = 0;
        for (int z = 0; z < nseg; ++z) total += part[a * nseg + z];
        W[e] = W[e] * (T)total;
    }
}

}  // namespace klnmf
