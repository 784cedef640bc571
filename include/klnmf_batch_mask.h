/* klnmf_batch_mask.h -- C-ABI of presence masks on batches: many MASKED KL-NMF problems of one shape in one launch sequence.
 *
 * An interface of its own beside klnmf_batch.h (whose type, conventions and queries it uses) and klnmf.h (whose
 * klnmf_upload_presence* it mirrors for a problem of a batch): int status returns, klnmf_last_error(), every entry point naming
 * the reference interface it replaces.  The same library, libklnmf.so, exports the three headers' symbols.
 */
#ifndef KLNMF_BATCH_MASK_H
#define KLNMF_BATCH_MASK_H

#include "klnmf_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A masked batch: `count` dense problems of one shape (n, f, k) that share ONE set of column bounds (n_mod <= KLNMF_MAX_MODALITIES
 * modalities, klnmf_upload_presence's col_bounds) and have each their OWN n x n_mod presence matrix P.  The weights of problem p are
 * Om_p[i, j] = P_p[i, m(j)]; every stage of the masked iteration -- ratio + loss, S and the W rule, and in a fit D, the H numerator
 * and the H rule -- is one launch for all problems (csrc/batch.hip.h).  A problem in a masked batch has, bit for bit, the results
 * of the same masked problem alone in a context (klnmf_upload_presence) whose chunk counts equal the batch's.
 *
 * State.  The first mask upload on a batch fixes the bounds for the whole batch and takes EVERY problem's P filled with 1: from
 * then on the batch is masked as a whole (klnmf_batch_query KLNMF_Q_PRESENCE = n_mod, 0 without a mask or a problem), and a
 * problem that never gets an upload runs the masked kernels on a mask of ones.  A later upload with other bounds returns
 * KLNMF_ERR_ARG.  klnmf_batch_clear_presence and klnmf_batch_set_problem drop the mask.  klnmf_batch_init_W stays W0 = V.H0^T,
 * unmasked, as klnmf_init_W on a masked context.
 *
 * Refusals, KLNMF_ERR_ARG, each leaving the batch exactly as it was and usable: no problem set, p outside [0, count), a null
 * source, an unknown dtype, n_mod outside 1 .. KLNMF_MAX_MODALITIES, bounds that do not run from 0 to f or do not increase
 * strictly, rows out of range (rows < 0, row0 < 0, row0 + rows > n, ld < n_mod), and for the device form a source column outside
 * [-1, ld) and a row index outside [0, src_rows). */

/* klnmf_upload_presence for problem p: rows row0 .. row0 + rows - 1 of P_p from src[rows][n_mod] (host memory, leading dimension
 * ld >= n_mod).  The reference has no counterpart (it has no mask; learner.py:53-56 stacks the modalities as contiguous column
 * ranges). */
int klnmf_batch_upload_presence(klnmf_batch *b, int p, const void *src, int dtype, int64_t rows, int64_t ld, int64_t row0,
                                const int64_t *col_bounds, int n_mod);
/* klnmf_upload_presence_device_rows for problem p: a mask in DEVICE memory of the batch's device, gathered by row index and source
 * column in one launch,
 *     P_p[row0 + i, m] = src_cols[m] >= 0 ? dP[drow_idx[i] * ld + src_cols[m]] : 1          i < rows, m < n_mod
 * (drow_idx null: rows 0 .. rows - 1 of dP; indices in any order, repeats allowed).  The indices are checked on the device before
 * anything is read through them: a bad one is reported through a flag and never dereferenced, and nothing is taken or written.
 * Synchronous: dP and drow_idx are free to go on return.  Replaces the per-run host slices of experiment.py:163-164 for the mask
 * of a device-resident dataset; the reference has no mask. */
int klnmf_batch_upload_presence_device_rows(klnmf_batch *b, int p, const void *dP, int dtype, int64_t src_rows, int64_t ld,
                                            const int64_t *drow_idx, int64_t rows, int64_t row0, const int *src_cols,
                                            const int64_t *col_bounds, int n_mod);
/* klnmf_clear_weights for a batch: the batch runs the unmasked kernels again, with the bits of a batch that never held a mask.
 * Nothing happens on a batch without a mask.  The reference has no counterpart. */
int klnmf_batch_clear_presence(klnmf_batch *b);

#ifdef __cplusplus
}
#endif
#endif /* KLNMF_BATCH_MASK_H */
