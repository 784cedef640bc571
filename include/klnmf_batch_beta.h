/* klnmf_batch_beta.h -- C-ABI of the beta-divergence cost on batches: many beta-NMF problems of one shape in one launch sequence.
 *
 * An interface of its own beside klnmf_batch.h (whose type, conventions and queries it uses) and klnmf_beta.h (whose
 * klnmf_set_divergence / klnmf_get_divergence it mirrors for a batch) and klnmf.h (whose klnmf_upload_weights it mirrors for a
 * problem of a batch): int status returns, klnmf_last_error(), every entry point naming the reference interface it replaces.  The
 * same library, libklnmf.so, exports the symbols of all the headers.
 */
#ifndef KLNMF_BATCH_BETA_H
#define KLNMF_BATCH_BETA_H

#include "klnmf_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A beta batch: `count` dense problems of one shape (n, f, k) under ONE beta != 1 (klnmf_beta.h has the cost and the rules), each
 * with its own V, W, H and -- where uploaded -- weights Om.  klnmf_batch_run then runs the beta iteration for all of them, every
 * stage one launch (csrc/batch.hip.h): the ratio pass with the loss, the per-problem loss sum with the stop rule, the W rule, the
 * second ratio pass, the H numerator and denominator, the H rule that leaves the rows' sums, the column scale of W; a transform
 * (fit = 0) is the first ratio pass and the W rule.  A problem in a beta batch has, bit for bit, the losses, W and H of the same
 * problem alone in a context with klnmf_set_divergence(beta) whose chunk counts equal the batch's.  klnmf_batch_init_W stays
 * W0 = V.H0^T, unweighted, as klnmf_init_W on a beta context.
 *
 * The reference has no counterpart to any entry below: nmf.py:293 announces "Helpers for beta divergence and related updates" and
 * holds none, and its `weights` (nmf.py:159-175) is never read. */

/* klnmf_set_divergence for a batch, behind klnmf_batch_set_problem and in front of a run.  beta != 1 takes the second buffer B
 * [count][n][f], the denominators' slab sets and the rows' sums; beta = 1 hands them (and the weights) back and the batch runs
 * the Kullback-Leibler loop again, bit for bit; klnmf_batch_set_problem* returns a batch to beta = 1.
 * KLNMF_ERR_UNSUPP, the batch unchanged and usable: a CSR batch, a batch that holds a presence mask (and on a batch with
 * beta != 1 klnmf_batch_upload_presence* is refused in turn).  KLNMF_ERR_ARG: no problem set, a beta that is not finite, and in
 * KLNMF_PREC_F32 a beta that fp32 rounds to 1 or to 0 without being it (klnmf_set_divergence's rule). */
int klnmf_batch_set_divergence(klnmf_batch *b, double beta);
/* klnmf_get_divergence for a batch: the beta its loop runs (1 behind klnmf_batch_set_problem*). */
int klnmf_batch_get_divergence(klnmf_batch *b, double *beta);
/* klnmf_upload_weights for problem p of a batch with beta != 1: Om_p[row0 + i, col0 + j] = src[i * ld + j] >= 0 (host memory).
 * The first call on a batch takes Om [count][n][f] filled with 1: a problem without an upload is weighted by ones.  The weights go
 * with the problem and with klnmf_batch_set_divergence(b, 1).  KLNMF_ERR_UNSUPP on a batch with beta = 1 (there are no weighted
 * Kullback-Leibler batches); KLNMF_ERR_ARG: p outside [0, count), a null source, an unknown dtype, a block out of range. */
int klnmf_batch_upload_weights(klnmf_batch *b, int p, const void *src, int dtype, int64_t rows, int64_t cols, int64_t ld, int64_t row0,
                               int64_t col0);

#ifdef __cplusplus
}
#endif
#endif /* KLNMF_BATCH_BETA_H */
