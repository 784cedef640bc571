/* klnmf_batch_csr.h -- C-ABI of CSR batches: many SPARSE KL-NMF problems of one shape in one launch sequence.
 *
 * An interface of its own beside klnmf_batch.h (whose type, conventions and queries it uses) and klnmf.h (whose
 * klnmf_set_problem_sparse / klnmf_upload_csr_rows / klnmf_upload_csr_device_rows it mirrors for a problem of a batch): int status
 * returns, klnmf_last_error(), every entry point naming the reference interface it replaces.  The same library, libklnmf.so,
 * exports the four headers' symbols.
 */
#ifndef KLNMF_BATCH_CSR_H
#define KLNMF_BATCH_CSR_H

#include "klnmf_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A CSR batch: `count` UNWEIGHTED problems of one shape (n, f, k) whose X are scipy-style CSR matrices, each with its OWN stored
 * entries (nnz[p] of them), in KLNMF_PREC_F64 / KLNMF_PREC_F32.  They advance through the reference's sparse branch (nmf.py:52-70
 * `_special_sparse_dot`, 301-308, 331-334, 342, 349) together: every stage of an iteration -- H^T, ratio + loss partials + the W
 * rule's partial sums, the loss term's sums, the loss with the stop rule, the W rule, and in a fit the H numerator over the CSC
 * order and the H rule -- is one launch for all problems (csrc/batch_sparse.hip.h), in the order klnmf_run takes for one blocked
 * CSR problem.  Each problem keeps its own W, H, loss record and stop state.
 *
 * Contract.  A problem in a CSR batch has, bit for bit, the losses, W and H of the same problem alone in a context
 * (klnmf_set_problem_sparse + klnmf_upload_csr_rows) whose KLNMF_Q_SP_COL_BLOCKS, KLNMF_Q_SP_ROW_BLOCKS and KLNMF_Q_EX_H_SEGMENTS
 * equal the batch's.  One pair of block counts serves the whole batch: the single context's size rule on the batch's MEAN stored
 * entries per problem; KLNMF_SP_CB / KLNMF_SP_RB force it as they force a context's.  klnmf_batch_query answers
 * KLNMF_Q_SP_COL_BLOCKS / _ROW_BLOCKS for a CSR batch (0 for a dense one).
 *
 * On a CSR batch klnmf_batch_set_H, _set_H_device, _set_W, _init_W (W0 = X.H0^T over the stored entries, nmf.py:156), _run,
 * _result, _get_W, _get_H and _get_W_device work as on a dense one.  klnmf_batch_upload_V* return KLNMF_ERR_ARG (the problems hold no
 * dense V), klnmf_batch_upload_presence* KLNMF_ERR_UNSUPP (CSR problems have no masked kernels, as in a context).
 * klnmf_batch_set_problem after klnmf_batch_set_problem_sparse, and the reverse, releases the other kind's state. */

/* klnmf_set_problem_sparse for every problem of the batch: the shape, the capacity of each loss record and nnz[p], p < count.
 * KLNMF_ERR_UNSUPP for what has no blocked regime -- k > 512, an nnz[p] == 0, 2^31 or more stored entries in the whole batch -- and
 * for count x blocks beyond the grid; KLNMF_ERR_ARG for a null or negative nnz and non-positive dimensions.  Every refusal comes
 * before anything is freed: the previous problem stays.  Replaces nothing of the reference (nmf.py:196-199 reads the shape). */
int klnmf_batch_set_problem_sparse(klnmf_batch *b, int64_t n, int64_t f, int64_t k, int64_t max_iter_capacity, const int64_t *nnz);
/* klnmf_upload_csr_rows for problem p (learner.py:53-56 `safe_hstack` of CSR modalities; experiment.py:163-164): host CSR arrays,
 * indptr[n + 1] with indptr[0] == 0 and indptr[n] == nnz[p] (else KLNMF_ERR_ARG), int64 column indices sorted within every row,
 * values of `dtype`.  The structure is checked on the device (row pointers, index range, order) and the CSC order built there.  A
 * refused upload leaves problem p without an X: klnmf_batch_run refuses until a good one follows. */
int klnmf_batch_upload_csr_rows(klnmf_batch *b, int p, int dtype, const int64_t *indptr, const int64_t *indices, const void *data);
/* klnmf_upload_csr_device_rows for problem p: X_p = hstack([scale[m] * X_m[drow_idx] ...]) gathered from device-resident CSR
 * modalities, same arguments, same checks -- the gathered total must equal nnz[p] before anything is copied (KLNMF_ERR_ARG).
 * Synchronous: the sources and drow_idx are free to go on return.  Replaces the per-run host slices of experiment.py:163-164. */
int klnmf_batch_upload_csr_device_rows(klnmf_batch *b, int p, int n_mod, const int64_t *const *indptr, const int32_t *const *indices,
                                       const void *const *data, const int *dtype, const int64_t *col_bounds, const double *scale,
                                       int64_t src_rows, const int64_t *drow_idx, int64_t rows);

#ifdef __cplusplus
}
#endif
#endif /* KLNMF_BATCH_CSR_H */
