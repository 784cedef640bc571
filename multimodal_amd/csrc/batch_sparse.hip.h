// Batched forms of the CSR loop's kernels in the blocked regime (sparseb.hip.h, and the small launches of sparse.hip.h around them):
// B unweighted CSR problems of one shape (n, f, k), each with its own stored entries (nnz[p] of them), advance through the sparse
// branch of nmf.py:52-70, 301-308, 331-334 together, every stage ONE launch with the problem index on the grid.
//
//   k_sp_transpose_H_batch                            H^T of every problem                          grid (.., B)
//   k_spb_qw_batch<T, KC, MODE>                       ratio + loss partials + G (SDDMM and SpMM)    grid (cb x n, B)
//   k_sp_colsum_part_batch / k_sp_hsum_part_batch     the loss term's column sums of W, row sums of H
//   k_sp_dots_batch / k_sp_loss_batch                 ... their products, and the loss with the stop rule riding in it, block p for problem p
//   k_spb_wrule_batch                                 the W rule from the column blocks' slabs      grid (.., B)
//   k_spb_n_batch<T, KC> / k_spb_numer_batch          the H numerator over the CSC order            grid (rb x f, B) / (.., .., B)
// (the H rule is batch.hip.h's k_update_H_batch / _part_batch / _norm_batch from `numer`)
// Each is the single problem's kernel's own text (sparseb_body.hip.h, sparse_body.hip.h) behind a prologue that moves the
// per-problem pointers: the gathered rows stay in registers from the dot products to the W rule, and 32 / 16 gathers are issued
// before the first multiply-add, exactly as sparseb.hip.h says and for its reasons.
//
// Layout.  Per problem, p x (the single problem's element count) apart: W[2] [B][n][k], H [B][k][f], H^T [B][f][k], the block pointers
// [B][n][cb + 1] and [B][f][rb + 1], G [B][cb][n][k], NT [B][rb][f][k], the loss partials [B][cb x n], the column-sum partials
// [B][nblk][k], prod [B][k], hpart [B][k][S], DevState [B], the loss records [B][cap].  Per entry, the B problems' arrays one
// behind another (problem p's entries at off[p] = nnz[0] + .. + nnz[p - 1]): int32 column indices, values, q, and the CSC order's
// int32 rows and permutation.  The block pointers and the permutation's targets hold positions in those CONCATENATED arrays
// (k_spb_shift / k_spb_shift32 add off[p] once, at upload), so the entry loops index them as the single kernels do and no kernel
// knows off[p].  One pair of block counts (cb, rb) serves every problem.
// Summation order: the bodies' -- a problem in a CSR batch has the bits of the same problem alone in a context with equal block counts.
// Stop state: one DevState per problem; the blocks of a stopped problem return at their first instruction.
#pragma once
#include "sparseb.hip.h"

namespace klnmf {

// positions of problem p's own arrays -> positions in the batch's concatenated arrays
KL_GLOBAL void k_spb_shift(int64_t *a, int64_t count, int64_t off) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < count; e += (int64_t)gridDim.x * blockDim.x) a[e] += off;
}
KL_GLOBAL void k_spb_shift32(int *a, int64_t count, int off) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < count; e += (int64_t)gridDim.x * blockDim.x) a[e] += off;
}

// k_sp_transpose_H, grid (.., B)
template <typename T>
__global__ void k_sp_transpose_H_batch(const T *H0, T *HT0, int64_t k, int64_t f, const DevState *st) {
    const int pb = blockIdx.y;
    if (st[pb].stop) return;
    const T *H = H0 + pb * k * f;
    T *HT = HT0 + pb * k * f;
#define KL_SP_BODY_TRANSPOSE
#include "sparse_body.hip.h"
#undef KL_SP_BODY_TRANSPOSE
}

// k_spb_qw, grid (cb x n, B): indices / data / q are the concatenated arrays, blkptr0 [B][n][nb + 1] holds positions in them
template <typename T, int KC, int MODE>
__global__ __launch_bounds__(64) void k_spb_qw_batch(const int64_t *blkptr0, const int *indices, const T *data, const T *W0, const T *HT0,
                                                     T *q, double *loss_part0, T *G0, int64_t n, int64_t k, int64_t f, int nb, T eps,
                                                     const DevState *st) {
    constexpr bool KEEP = KC <= 2;
    constexpr int NB = KC == 1 ? 32 : (KC == 2 ? 16 : 32);
    const int pb = blockIdx.y;
    if (st[pb].stop) return;
    const int64_t *blkptr = blkptr0 + pb * n * (nb + 1);
    const T *W = W0 + pb * n * k, *HT = HT0 + pb * f * k;
    double *loss_part = loss_part0 + (int64_t)pb * nb * n;
    T *G = G0 + (int64_t)pb * nb * n * k;
#define KL_SPB_BODY_QW
#include "sparseb_body.hip.h"
#undef KL_SPB_BODY_QW
}

// k_spb_wrule, grid (.., B)
template <typename T>
__global__ __launch_bounds__(256) void k_spb_wrule_batch(const T *G0, int nb, const T *Wold0, T *Wnew0, int64_t n, int64_t k, int multiply,
                                                         const DevState *st) {
    const int pb = blockIdx.y;
    if (st[pb].stop) return;
    const T *G = G0 + (int64_t)pb * nb * n * k, *Wold = Wold0 + pb * n * k;
    T *Wnew = Wnew0 + pb * n * k;
#define KL_SPB_BODY_WRULE
#include "sparseb_body.hip.h"
#undef KL_SPB_BODY_WRULE
}

// k_spb_n, grid (rb x f, B): csc_rows / csc_perm / q are the concatenated arrays (csc_perm's targets: positions in q)
template <typename T, int KC>
__global__ __launch_bounds__(64) void k_spb_n_batch(const int64_t *cblkptr0, const int *csc_rows, const int *csc_perm, const T *q,
                                                    const T *W0, T *NT0, int64_t n, int64_t k, int64_t f, int nrb, const DevState *st) {
    const int pb = blockIdx.y;
    if (st[pb].stop) return;
    const int64_t *cblkptr = cblkptr0 + pb * f * (nrb + 1);
    const T *W = W0 + pb * n * k;
    T *NT = NT0 + (int64_t)pb * nrb * f * k;
#define KL_SPB_BODY_N
#include "sparseb_body.hip.h"
#undef KL_SPB_BODY_N
}

// k_spb_numer, grid (32-column tiles, 32-component tiles, B)
template <typename T>
__global__ __launch_bounds__(256) void k_spb_numer_batch(const T *NT0, int nrb, T *numer0, int64_t k, int64_t f, const DevState *st) {
    const int pb = blockIdx.z;
    if (st[pb].stop) return;
    const T *NT = NT0 + (int64_t)pb * nrb * f * k;
    T *numer = numer0 + pb * k * f;
#define KL_SPB_BODY_NUMER
#define KL_SPB_NUMER_ATILE blockIdx.y
#include "sparseb_body.hip.h"
#undef KL_SPB_NUMER_ATILE
#undef KL_SPB_BODY_NUMER
}

// k_sp_colsum_part, grid (row blocks, B); part [B][row blocks][k]
template <typename T>
__global__ __launch_bounds__(256) void k_sp_colsum_part_batch(const T *W0, double *part0, int64_t n, int64_t k, const DevState *st) {
    const int pb = blockIdx.y;
    if (st[pb].stop) return;
    const T *W = W0 + pb * n * k;
    double *part = part0 + (int64_t)pb * gridDim.x * k;
#define KL_SP_BODY_COLSUM
#include "sparse_body.hip.h"
#undef KL_SP_BODY_COLSUM
}

// k_sp_hsum_part, grid (segments, k, B); hpart [B][k][segments]
template <typename T>
__global__ __launch_bounds__(256) void k_sp_hsum_part_batch(const T *H0, int64_t f, int64_t seg, double *hpart0, const DevState *st) {
    const int pb = blockIdx.z;
    if (st[pb].stop) return;
    const T *H = H0 + (int64_t)pb * gridDim.y * f;
    double *hpart = hpart0 + (int64_t)pb * gridDim.y * gridDim.x;
#define KL_SP_BODY_HSUM
#include "sparse_body.hip.h"
#undef KL_SP_BODY_HSUM
}

// k_sp_dots, grid (k, B); hpart0 != nullptr: [B][k][S]
template <typename T>
__global__ __launch_bounds__(256) void k_sp_dots_batch(const double *wpart0, int64_t nblk, const T *H0, int64_t k, int64_t f, double *prod0,
                                                       const DevState *st, const double *hpart0, int S) {
    const int pb = blockIdx.y;
    if (st[pb].stop) return;
    const double *wpart = wpart0 + pb * nblk * k, *hpart = hpart0 != nullptr ? hpart0 + pb * k * S : nullptr;
    const T *H = H0 + pb * k * f;
    double *prod = prod0 + pb * k;
#define KL_SP_BODY_DOTS
#include "sparse_body.hip.h"
#undef KL_SP_BODY_DOTS
}

// k_sp_loss with the stop rule, block p for problem p: `n` loss partials and k products each, the loss into out0[2 p] and -- decide
// -- into problem p's record
KL_GLOBAL __launch_bounds__(1024) void k_sp_loss_batch(const double *row_loss0, int64_t n, const double *prod0, int64_t k, double *out0,
                                                        DevState *st, int decide, double tol_abs, double *errors, int64_t cap) {
    const int pb = blockIdx.x;
    if (st[pb].stop) return;
    const double *row_loss = row_loss0 + pb * n, *prod = prod0 + pb * k;
    double *out = out0 + 2 * pb;
    const DecideArgs dec{decide, st + pb, tol_abs, errors + pb * cap, cap};
#define KL_SP_BODY_LOSS
#include "sparse_body.hip.h"
#undef KL_SP_BODY_LOSS
}

}  // namespace klnmf
