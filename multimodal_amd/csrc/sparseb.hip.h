// CSR input, blocked for the L2 (round 5): the reference's sparse branch (nmf.py:52-70, 301-308, 331-334, 342, 349) as
//   ONE pass over the stored entries for ratio + loss + W rule (SDDMM and SpMM fused), column-blocked, and
//   one pass over the same entries in CSC order for the H numerator, row-blocked.
//
// Why blocks.  Per stored entry the passes gather a k-vector of H^T (ratio, W rule) or of W (H numerator): 3 x nnz x k x es
// bytes per iteration against nnz x (index + value) compulsory ones -- 13.2 GB against 1.04 GB at 20 000 x 110 000, 0.5 %
// stored, k = 50, fp64.  Round 4 served them from the Infinity Cache (H^T is 44 MB): 3.7 .. 6.5 TB/s, 2.75 ms per iteration,
// 0.047 of the HBM roof on compulsory bytes.  An XCD's 4 MiB L2 delivers gathered rows at twice the Infinity Cache's rate
// (MI355X_MICROARCH.md, "Indexed rows"), so the entries are walked block by block:
//   * column blocks of `cb_cols` columns with cb_cols x k x es <= 3 MiB -- the block's rows of H^T stay in every XCD's L2
//     while ALL workgroups work on that block (blockIdx = block x rows: dispatch order keeps the chip on one block);
//   * the ratio needs the whole dot product W_i . H_:,j, which a column block has -- one entry, one column; the W rule
//     sums over ALL entries of a row: per (row, block) partial sums G[b][i][:] (fp64 / fp32 slabs, summed in block order by
//     k_spb_wrule: fixed order, no atomics), and the second gather of an entry's row of H^T -- for the W rule, right behind
//     the dot product -- hits the L1 it was just loaded into: the two products cost ONE pass of gathers;
//   * row blocks of `rb_rows` rows (rb_rows x k x es <= 3 MiB of W) for the H numerator over the CSC order, partial sums
//     per row block in TRANSPOSED layout [rb][column][k] (one coalesced k-vector per wave), summed and transposed by
//     k_spb_numer.
// Block pointers are built on the device at upload from the sorted CSR / CSC arrays (binary search per row and block);
// indices are kept as int32 (half the index bytes).  Results equal the unblocked kernels' to summation order: tests/test_sparse_gpu.py
// checks every component chunk, 1 to 7 column and row blocks (forced and by the size rule) and the unblocked kernels against
// the fp64 reference, and a blocked run against the same problem in one block of each kind (1e-12 in fp64).
#pragma once
#include "sparse.hip.h"

namespace klnmf {

constexpr int64_t kSpBlockBytes = (int64_t)3 << 20;       // of H^T (column block) / of W (row block): fits a 4 MiB L2 beside the streams

// blkptr[r][b] = first position in [ptr[r], ptr[r+1]) whose index is >= b * width (b = 0 .. nb; blkptr[r][nb] = ptr[r+1]);
// idx sorted ascending inside every row.  bad: set when a row is not sorted.
KL_GLOBAL void k_spb_blkptr(const int64_t *ptr, const int64_t *idx, int64_t rows, int nb, int64_t width, int64_t *blkptr, int *bad) {
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e >= rows * (nb + 1)) return;
    const int64_t r = e / (nb + 1);
    const int b = (int)(e % (nb + 1));
    const int64_t p0 = ptr[r], p1 = ptr[r + 1];
    const int64_t key = (int64_t)b * width;
    int64_t lo = p0, hi = p1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (idx[mid] < key) lo = mid + 1; else hi = mid;
    }
    blkptr[e] = b == nb ? p1 : lo;
    if (b == 0)
        for (int64_t p = p0 + 1; p < p1; ++p)
            if (idx[p] < idx[p - 1]) { *bad = 1; break; }
}
KL_GLOBAL void k_spb_narrow(const int64_t *src, int *dst, int64_t count) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < count; e += (int64_t)gridDim.x * blockDim.x) dst[e] = (int)src[e];
}

enum SpbMode { SPB_LOSS = 0, SPB_UPDATE = 1, SPB_INIT = 2 };

// One wave per (row i, column block b); blockIdx.x = b * n + i.  Lane l holds components l, l + 64, ... of W_i.
//   SPB_UPDATE  q_p = (x_p + eps) / (W_i . H_:,j_p + eps) -> q (CSR order), loss partial, G[b][i][a] = sum_p q_p H[a][j_p]
//   SPB_LOSS    the loss partial only (klnmf_error)
//   SPB_INIT    G[b][i][a] = sum_p x_p H[a][j_p]                       (W0 = X . H0^T, nmf.py:156)
// 32 entries per trip: 32 gathers of a k-vector at wave-uniform addresses in flight, LaneTransposeSum turns the 32 vectors of
// per-lane partial products into the 32 dot products (both lane halves; the lower one takes division and logarithm), then
// the same 32 rows of H^T -- now in L1 -- are multiplied by their ratios into the W rule's partial sums.
template <typename T, int KC, int MODE>
__global__ __launch_bounds__(64) void k_spb_qw(const int64_t *blkptr, const int *indices, const T *data, const T *W, const T *HT,
                                               T *q, double *loss_part, T *G, int64_t n, int64_t k, int nb, T eps, const DevState *st) {
    // KEEP (k <= 128): the gathered rows stay in registers from the dot products to the W rule -- ONE pass of gathers.  (Reloading
    // them "from L1" was an illusion: 16 waves x 32 rows x 400 B per CU are 200 KB against 32 KB of L1, the second pass missed it
    // and the kernel sat on the gather roof -- 8.5 TB/s -- with twice the bytes: 1.37 ms instead of 0.8 at the bench's shape.)
    constexpr bool KEEP = KC <= 2;
    constexpr int NB = KC == 1 ? 32 : (KC == 2 ? 16 : 32);            // entries per trip (NB x KC rows of registers in the KEEP form)
    if (st && st->stop) return;
#define KL_SPB_BODY_QW
#include "sparseb_body.hip.h"
#undef KL_SPB_BODY_QW
}

// W_new[i][a] = (multiply ? W[i][a] : 1) * sum_b G[b][i][a]        (fixed block order)
template <typename T>
__global__ __launch_bounds__(256) void k_spb_wrule(const T *G, int nb, const T *Wold, T *Wnew, int64_t n, int64_t k, int multiply,
                                                   const DevState *st) {
    if (st && st->stop) return;
#define KL_SPB_BODY_WRULE
#include "sparseb_body.hip.h"
#undef KL_SPB_BODY_WRULE
}

// One wave per (column j, row block rb); blockIdx.x = rb * f + j.  NT[rb][j][a] = sum_{p in column j, row block rb} W[row_p][a] q[perm_p]
template <typename T, int KC>
__global__ __launch_bounds__(64) void k_spb_n(const int64_t *cblkptr, const int *csc_rows, const int *csc_perm, const T *q, const T *W,
                                              T *NT, int64_t k, int64_t f, int nrb, const DevState *st) {
    if (st && st->stop) return;
#define KL_SPB_BODY_N
#include "sparseb_body.hip.h"
#undef KL_SPB_BODY_N
}

// numer[a][j] = sum_rb NT[rb][j][a]: summed in row-block order and transposed through LDS (32 columns x 32 components per step:
// coalesced on both sides)
template <typename T>
__global__ __launch_bounds__(256) void k_spb_numer(const T *NT, int nrb, T *numer, int64_t k, int64_t f, const DevState *st) {
    if (st && st->stop) return;
#define KL_SPB_BODY_NUMER
#define KL_SPB_NUMER_ATILE blockIdx.y
#include "sparseb_body.hip.h"
#undef KL_SPB_NUMER_ATILE
#undef KL_SPB_BODY_NUMER
}

}  // namespace klnmf
