/* klnmf_batch.h -- C-ABI of batches: many KL-NMF problems of one shape in one launch sequence.
 *
 * An interface of its own beside klnmf.h (whose status codes, precisions, element types and conventions it uses: int status
 * returns, klnmf_last_error(), every entry point naming the reference interface it replaces).  A batch is neither a mode of
 * klnmf_ctx nor a klnmf_group; the same library, libklnmf.so, exports both headers' symbols.
 */
#ifndef KLNMF_BATCH_H
#define KLNMF_BATCH_H

#include "klnmf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The reference's launcher runs Ks x N_RUN independent experiments (samples/launcher.py:68-69, 82), each one fit and a few dozen
 * transforms (experiment.py:158-180, 235-238) of a few hundred rows: one such problem leaves the GPU idle between its launches.  A
 * batch is `count` DENSE, UNWEIGHTED problems of identical (n, f, k) in KLNMF_PREC_F64 / KLNMF_PREC_F32 on one device that advance
 * through the loop of nmf.py:212-222 together -- every stage of an iteration one launch for all of them (csrc/batch.hip.h), each
 * problem with its own V, W, H, loss record and stop state (nmf.py:214-220: a problem whose stop rule fired is frozen while the
 * others go on).  A problem in a batch has, bit for bit, the results of the same problem alone in a context whose chunk counts
 * (KLNMF_Q_EX_ROW_CHUNKS / _W_CHUNKS) equal the batch's.  The batch's counts are the single problem's plan for
 * max(1, cu_count / count) compute units: klnmf_plan_query(precision, n, f, k, -1, max(1, cu_count / count), ...); the
 * development switches KLNMF_EX_ROW_CHUNKS / _W_CHUNKS / _H_SEG force them as they force a context's.  A batch is a type of its
 * own: neither a mode of klnmf_ctx nor a klnmf_group.  Used from one thread at a time; it owns its stream.  (Row x modality
 * presence masks on the problems of a batch: klnmf_batch_mask.h; CSR problems on a batch: klnmf_batch_csr.h.) */
typedef struct klnmf_batch klnmf_batch;
#define KLNMF_BATCH_MAX 256
/* KLNMF_ERR_UNSUPP for every precision but KLNMF_PREC_F64 / F32 (nothing is created), KLNMF_ERR_ARG unless 1 <= count <=
 * KLNMF_BATCH_MAX.  Replaces constructing `count` KLdivNMF objects (nmf.py:136-145). */
int klnmf_batch_create(klnmf_batch **out, int device, int precision, int count);
int klnmf_batch_destroy(klnmf_batch *b);
/* The shape every problem of the batch has (nmf.py:196-199) and the capacity of each loss record.  Refuses what
 * klnmf_set_problem refuses in these modes (dimensions, the row limit) and a shape whose count x row tiles (or component
 * tiles) of 64 exceed the 65535 of gridDim.y -- before anything is freed or allocated: the previous problem stays. */
int klnmf_batch_set_problem(klnmf_batch *b, int64_t n, int64_t f, int64_t k, int64_t max_iter_capacity);
/* klnmf_upload_V / klnmf_upload_V_device_rows_dt for problem p (learner.py:53-56; experiment.py:163-164): KLNMF_ERR_ARG for p
 * outside [0, count). */
int klnmf_batch_upload_V(klnmf_batch *b, int p, const void *src, int dtype, int64_t rows, int64_t cols, int64_t ld,
                         int64_t row0, int64_t col0, double scale);
int klnmf_batch_upload_V_device_rows_dt(klnmf_batch *b, int p, const void *dsrc, int dtype, const int64_t *drow_idx, int64_t rows,
                                        int64_t cols, int64_t ld, int64_t row0, int64_t col0, double scale);
/* klnmf_set_H / klnmf_set_H_device / klnmf_set_W for problem p (nmf.py:147-157 `_init`; nmf.py:251-253) */
int klnmf_batch_set_H(klnmf_batch *b, int p, const void *src, int dtype);
int klnmf_batch_set_H_device(klnmf_batch *b, int p, const void *dsrc, int dtype, int64_t ld, int64_t col0, int64_t ncols, int last);
int klnmf_batch_set_W(klnmf_batch *b, int p, const void *src, int dtype);
/* W0 = V.H0^T of every problem (nmf.py:156), one launch sequence */
int klnmf_batch_init_W(klnmf_batch *b);
/* The loop of nmf.py:212-222 for every problem at once: whole iterations are enqueued without draining the stream; with
 * tol_abs > 0 "has every problem stopped?" is asked every 16th iteration (klnmf_run's cadence).  Synchronous on return.
 * KLNMF_ERR_ARG before every problem has a V and an H, and for max_iter beyond the capacity. */
int klnmf_batch_run(klnmf_batch *b, int64_t max_iter, int fit, double tol_abs);
/* problem p's loss record of the last klnmf_batch_run (nmf.py:221 `errors`), its length and whether its stop rule fired */
int klnmf_batch_result(klnmf_batch *b, int p, double *errors_out, int64_t *n_done, int *stopped);
/* klnmf_get_W / klnmf_get_H / klnmf_get_W_device for problem p */
int klnmf_batch_get_W(klnmf_batch *b, int p, void *dst, int dtype);
int klnmf_batch_get_H(klnmf_batch *b, int p, void *dst, int dtype);
int klnmf_batch_get_W_device(klnmf_batch *b, int p, void *ddst, int dtype, int64_t ld);
/* KLNMF_Q_EX_ROW_CHUNKS / _W_CHUNKS / _H_SEGMENTS / _H_FROM_SLABS of the batch's plan (0 with no problem),
 * KLNMF_Q_BATCH_COUNT: the count the batch was created with, and KLNMF_Q_PRESENCE: the modalities of the batch's presence masks
 * (klnmf_batch_mask.h), 0 without one.  Replaces nothing of the reference. */
#define KLNMF_Q_BATCH_COUNT       22
int klnmf_batch_query(klnmf_batch *b, int what, int64_t *value);

#ifdef __cplusplus
}
#endif
#endif /* KLNMF_BATCH_H */
