// Row x modality presence masks on the exact kernels (KLNMF_PREC_F64 / F32, dense): weighted KL-NMF for weights of the form
// Om[i, j] = P[i, m(j)] -- P an n x M matrix (klnmf_upload_presence), m(j) the modality of column j, modalities contiguous
// column ranges, M <= KLNMF_MAX_MODALITIES -- without the n x f buffer Om.  With R = Om o Q the update is weighted.hip.h's, and
// its two denominators collapse:
//   Om.H^T      = P.S    S[m][a] = sum of H[a][j] over the columns j of modality m   (M x k; n M k work)
//   (W^T.Om)[a][j] = D[a][m(j)]    D = W^T.P                                         (k x M; n k M work)
// so an iteration is the unweighted loop's three contractions of n f k plus these, and V and R are its only n x f streams:
//   k_gemm<.., EpiQ<T, PresenceWeight>>   W.H -> R = p * Q, loss partials of p * (V log Q - V + Y)   (p = 0: R = 0, a loss term of exactly 0)
//   k_presence_S                           S from the current H, once per W rule
//   k_gemm<.., EpiW<T, FacPresW>>          R.H^T -> W * num / (P.S)   (feature chunks: EpiWpart's slabs, summed by k_wrule_exact<T, FacPresW>)
//   k_gemm<.., EpiN<T>>                    W_new^T.R: the unweighted H numerator, unchanged
//   k_presence_D_part / k_presence_D_sum   D = W_new^T.P over row chunks, slabs in double summed in a fixed order
//   k_update_H / k_update_H_part under FacPresH   the H rule: factor = D > 0 ? num / D : 1
// The ratio epilogue and the rules are the one family of exact.hip.h under the policies PresenceWeight, FacPresW and FacPresH; this
// file holds them and what only a masked problem runs: k_presence_S, k_presence_D_part, k_presence_D_sum -- their bodies in
// presence_body.hip.h, included as text here and in their batched forms (batch.hip.h), as gemm_body.hip.h is.
// The mask itself comes from the host (klnmf_upload_presence: k_place_V on the n x M matrix) or from a mask resident in device
// memory, gathered by row index and source column (klnmf_upload_presence_device_rows: k_presence_rows_check, k_presence_gather).
// S and D are accumulated in double in a fixed order and rounded once to T (as the H rule's row sums are): two runs give the
// same bits.  The routes (row chunks, feature chunks, segments, rule from the slabs) are the unweighted plan's.
#pragma once
#include "weighted.hip.h"

namespace klnmf {

constexpr int kMaxMod = 16;          // KLNMF_MAX_MODALITIES (klnmf.h)
constexpr int kPresDRows = 128;      // rows per chunk of D's reduction, at least (presence_d_chunks)
constexpr int kPresDMaxChunks = 64;
constexpr int kPresGatherMaxBlocks = 512;      // the gather's grid: 256 rows per block, more rows than 131 072 go round its loop

// row chunks of D = W^T.P: a function of n alone (the bits of D do not depend on the device's size)
inline int presence_d_chunks(int64_t n) {
    const int64_t c = (n + kPresDRows - 1) / kPresDRows;
    return (int)(c < 1 ? 1 : (c > kPresDMaxChunks ? kPresDMaxChunks : c));
}

// the weight of element (r, c): p = P[r][m(c)], looked up per element (a 64-column tile may hold several modalities)
template <typename T>
struct PresenceWeight {
    const T *P; const unsigned char *mod; int nmod;
    __device__ T at(int r, int c, int64_t) const { return P[(int64_t)r * nmod + mod[c]]; }
};

// S[m][a] = sum over modality m's columns of H[a][j]: one block per (a, m), fp64 partial sums per thread (stride 256), the
// block's fixed-order sum, rounded once.
template <typename T>
__global__ __launch_bounds__(256) void k_presence_S(const T *H, const int64_t *bounds, T *S, int64_t f, int64_t k, const DevState *st) {
    if (st && st->stop) return;
#define KL_PRESENCE_BODY_S
#include "presence_body.hip.h"      // (the block's work: shared with k_presence_S_batch)
#undef KL_PRESENCE_BODY_S
}

// den = sum_m P[r][m] * S[m][c], m ascending, in T
template <typename T>
__device__ __forceinline__ T presence_den(const T *prow, const T *S, int64_t k, int c, int nmod) {
    T den = T(0);
    for (int m = 0; m < nmod; ++m) den += prow[m] * S[(int64_t)m * k + c];
    return den;
}

// W rule: num / (P.S)[r][c]; a sample with no present modality (denominator 0) keeps its coefficients.  No denominator slabs.
template <typename T>
struct FacPresW {
    static constexpr int S = 1;
    const T *P; const T *Sm; int64_t k; int nmod;
    __device__ bool on() const { return true; }
    template <typename V>
    __device__ T of(const V &v, int64_t r, int64_t c) const { return w_factor(v[0], presence_den(P + r * nmod, Sm, k, (int)c, nmod)); }
};
// H rule: num / D[a][m(j)]
template <typename T>
struct FacPresH {
    static constexpr int S = 1;
    const T *D; const unsigned char *mod; int nmod;
    template <typename V>
    __device__ T of(const V &v, int64_t a, int64_t j) const { return w_factor(v[0], (D + a * nmod)[mod[j]]); }
};

// D = W^T.P over one row chunk: block (x, z) takes components 64 x .. 64 x + 63 and rows [z * chunk, (z + 1) * chunk); wave w
// walks the chunk's rows w, w + 4, ... (64 consecutive components of a row of W per load), every lane holds M fp64 sums; the
// four waves' sums are added in wave order and stored to slab z ([k][M] doubles).
template <typename T>
__global__ __launch_bounds__(256) void k_presence_D_part(const T *W, const T *P, double *slab, int64_t n, int64_t k, int nmod,
                                                         int64_t chunk, const DevState *st) {
    if (st && st->stop) return;
#define KL_PRESENCE_BODY_D_PART
#include "presence_body.hip.h"      // (the block's work: shared with k_presence_D_part_batch)
#undef KL_PRESENCE_BODY_D_PART
}

// D[a][m] = the slabs' sum, chunk 0 first, rounded once to T
template <typename T>
__global__ void k_presence_D_sum(const double *slab, int nslab, int64_t count, T *D, const DevState *st) {
    if (st && st->stop) return;
#define KL_PRESENCE_BODY_D_SUM
#include "presence_body.hip.h"      // (shared with k_presence_D_sum_batch)
#undef KL_PRESENCE_BODY_D_SUM
}

// The source column of every modality of one gather, passed by value (read through the kernel-argument segment: uniform loads, no
// table in device memory); -1: the modality has no column, its weight is 1
struct PresenceCols {
    int col[kMaxMod];
};

// bad[0] = 1 if a row index lies outside [0, src_rows): reads idx alone, nothing through it.  The gather is launched only after the
// host has read bad[0] == 0.
KL_GLOBAL __launch_bounds__(256) void k_presence_rows_check(const int64_t *idx, int64_t rows, int64_t src_rows, int64_t *bad) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < rows; r += stride) {
        const int64_t i = idx[r];
        if (i < 0 || i >= src_rows) bad[0] = 1;
    }
}

// P[row0 + r, m] = src[idx[r], cols[m]] (idx null: src[r, cols[m]]), 1 where cols[m] < 0, cast to T as k_place_V casts an upload.  One
// thread per output row: one index load, M gathered loads, M contiguous stores (consecutive threads write consecutive rows of P).
// In range by the caller's checks: every idx[r] in [0, src_rows), every cols[m] in [-1, ld), row0 + rows <= n.
template <typename T, typename S>
__global__ __launch_bounds__(256) void k_presence_gather(T *P, int nmod, const S *src, int64_t ld, const int64_t *idx, int64_t rows,
                                                         int64_t row0, PresenceCols cols) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < rows; r += stride) {
        const S *srow = src + (idx ? idx[r] : r) * ld;
        T *prow = P + (row0 + r) * nmod;
#pragma unroll
        for (int m = 0; m < kMaxMod; ++m)
            if (m < nmod) prow[m] = cols.col[m] >= 0 ? (T)(double)srow[cols.col[m]] : T(1);
    }
}

}  // namespace klnmf
