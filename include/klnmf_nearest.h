/* klnmf_nearest.h -- C-ABI of the fused nearest-example search: for every row of A the index of its nearest row of B under
 * each selected measure, for many (A, B) pairs in one launch; only the indices (and, on request, the distances) are written.
 *
 * An interface of its own beside klnmf.h (whose conventions, error codes and measure numbers it uses): int status returns,
 * klnmf_last_error(), every entry point naming the reference interface it stands in for.  The same library, libklnmf.so, exports
 * the symbols of every header.
 *
 * What it computes.  The reference classifies by `np.argmin(all_distances(reco, ex, measure), axis=1)` (evaluation.py:74-77,
 * 103-116), once per measure of metrics.py:58-86.  Here the value of a pair (i, j) under a measure is bit for bit the value
 * klnmf_all_distances_device stores in out[i * nb + j] for that measure and dtype (the final rounding to the dtype included), and
 * the index chosen is np.argmin's: the lowest index among equal minima; a NaN counts as smaller than every number, and among
 * NaNs the lowest index wins.  d = 0 gives index 0.
 *
 * metrics: a bit mask, bit i = measure i of klnmf.h (KLNMF_DIST_KL .. KLNMF_DIST_COSINE_DIFF); M = the number of set bits.
 * Outputs: the jobs' rows lie behind one another -- the row offset of job q is the sum of na of the jobs before it -- and a
 * row holds its M results in ascending bit order: idx[row * M + slot] (int32), dist[row * M + slot] (the dtype).
 * Limits: na, nb <= 2^24 and d <= 2^30 per job, the sum of na <= 2^24, count <= KLNMF_NEAREST_MAX_JOBS. */
#ifndef KLNMF_NEAREST_H
#define KLNMF_NEAREST_H

#include "klnmf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KLNMF_NEAREST_MAX_JOBS (1 << 20)
#define KLNMF_DIST_MASK_ALL 31

/* One search: A [na, d] against B [nb, d], DEVICE pointers of the call's dtype, row strides in elements (>= d).  Jobs are of
 * independent shape; na = 0 contributes no rows; a pointer may be null where its matrix holds no element. */
typedef struct klnmf_nearest_job {
    const void *A;
    int64_t lda;
    const void *B;
    int64_t ldb;
    int64_t na, nb, d;
} klnmf_nearest_job;

/* The bytes of device workspace a klnmf_nearest_many_device call of `count` jobs with `total_rows` = sum of na needs (the job
 * table and the map from output rows to jobs).  KLNMF_ERR_ARG: a null `bytes`, a negative count or total, one beyond the limits.
 * Stands in for nothing of the reference: evaluation.py:103-116 allocates its [na, nb, d] broadcast per call. */
int klnmf_nearest_work_bytes(int64_t count, int64_t total_rows, uint64_t *bytes);

/* The searches jobs[0 .. count) (a HOST array of device pointers) in ONE launch on `device`'s null stream: uploads the job table
 * into the caller's workspace d_work (device memory, work_bytes >= klnmf_nearest_work_bytes), launches, and synchronises as
 * klnmf_all_distances_device does; no allocation per call.  d_idx: int32 [sum na][M]; d_dist: the distances of the chosen
 * examples, `dtype` [sum na][M], or null.  count = 0 or sum na = 0: KLNMF_OK, nothing done.
 * KLNMF_ERR_ARG, nothing launched and nothing written: a null pointer where data is needed (jobs, d_idx, d_work; A or B of a
 * job that has elements), a stride below d, an empty or unknown measure mask, a dtype other than KLNMF_DT_F32 / KLNMF_DT_F64,
 * nb = 0 with na > 0 (np.argmin of nothing raises), negative counts, a shape beyond the limits above, a workspace smaller than
 * klnmf_nearest_work_bytes says.
 * Replaces `classify_NN` = `dists_to_found_labels(all_distances(reco_data, ex_data, measure), ...)` (evaluation.py:103-116, with
 * np.argmin of evaluation.py:74-77) for every measure of metrics.py:58-86 at once: 48 calls of a two-modality evaluation
 * (experiment.py:233-257), 48 of a three-modality one (experiment.py:332-350), are 12 jobs of one call. */
int klnmf_nearest_many_device(int device, int dtype, int metrics, const klnmf_nearest_job *jobs, int64_t count, int32_t *d_idx,
                              void *d_dist, void *d_work, uint64_t work_bytes);

/* One job on HOST arrays: A [na x d], B [nb x d] row-major of `dtype`; idx int32 [na x M], dist `dtype` [na x M] or null.  The
 * counterpart of klnmf_all_distances for callers without device tensors (allocates, uploads, searches, downloads).  Refusals
 * as above.  Replaces `np.argmin(all_distances(reco_data, ex_data, measure), axis=1)` (evaluation.py:103-116; metrics.py:58-86)
 * for the selected measures. */
int klnmf_nearest(int device, int dtype, int metrics, int64_t na, int64_t nb, int64_t d, const void *A, const void *B,
                  int32_t *idx, void *dist);

#ifdef __cplusplus
}
#endif
#endif /* KLNMF_NEAREST_H */
