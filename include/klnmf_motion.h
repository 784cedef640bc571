/* klnmf_motion.h -- C-ABI of the motion modality's device half: Kinect records to joint angles and delayed velocities, per-column
 * whitening, scipy's `kmeans` (Lloyd iterations to convergence, empty clusters dropped) for many problems at once, and the hard /
 * soft vector-quantisation histograms per example -- the stages of the reference's `db_to_VQ_hist_matrix`
 * (features/angle_histograms.py:171-223).
 *
 * An interface of its own beside klnmf.h (whose conventions, error codes and dtype numbers it uses): int status returns,
 * klnmf_last_error(), every entry point naming the reference lines it stands in for.  The same library, libklnmf.so, exports
 * the symbols of every header.
 *
 * Storage is KLNMF_DT_F32 or KLNMF_DT_F64; every operation is fp64 (f32 values promoted exactly), each rounded on its own -- no
 * fused multiply-add -- and a result is rounded once more where it is stored as f32.  No floating-point atomics.
 *
 * The order rule (klnmf_kmeans.h's).  Every sum over frames -- a column's sum and sum of squared deviations, a cluster's column
 * sum, the sum of the frames' distances to their codes -- is formed per group of KLNMF_MOTION_GROUP = 4096 consecutive frames,
 * the group's contributing frames added in ascending order starting from +0, and the groups' partial sums are then added in
 * ascending group order starting from +0.  A histogram bin is the sum over its example's frames, ascending from +0 (no groups:
 * an example is one chain).  The order depends on the shape alone: two calls on the same data give the same bits.
 *
 * Point sets.  The k-means and histogram calls read D point sets of T points of d coordinates from one buffer: coordinate j of
 * point t of set s is points[s * set_stride + t * ld + j].  The whitened [T, 2 D] matrix of interleaved (angle, velocity)
 * columns is D sets with set_stride = 2, ld = 2 D, d = 2.
 *
 * Limits: K <= KLNMF_MOTION_MAX_K, d <= KLNMF_MOTION_MAX_D, K * d <= KLNMF_MOTION_MAX_KD (a workgroup's accumulators, its copy
 * of the codebook and a tile of points live in LDS), pairs <= KLNMF_MOTION_MAX_PAIRS, problems and point sets
 * <= KLNMF_MOTION_MAX_P each (a grid dimension); beyond them KLNMF_ERR_UNSUPP before anything is launched.  T < 2^31 - 1. */
#ifndef KLNMF_MOTION_H
#define KLNMF_MOTION_H

#include "klnmf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KLNMF_MOTION_TILE 256
#define KLNMF_MOTION_GROUP 4096
#define KLNMF_MOTION_MAX_K 256
#define KLNMF_MOTION_MAX_D 16
#define KLNMF_MOTION_MAX_KD 1024
#define KLNMF_MOTION_MAX_PAIRS 32
#define KLNMF_MOTION_MAX_P 65535
#define KLNMF_MOTION_POLL 4
#define KLNMF_MOTION_PAD_ZEROS 0
#define KLNMF_MOTION_PAD_CIRCULAR 1

/* The bytes of device workspace any call of this header on these sizes needs: with G = max(1, ceil(T / 4096)) groups, the
 * largest of  G * C doubles (whitening of C columns),  G * P * K * d doubles + G * P doubles + G * P * K int32 + P doubles +
 * 2 P int32 (k-means: the groups' partial sums, distances and counts; a problem's previous distortion, stop flag and set),
 * E * D * K doubles (histograms),  each part rounded up to 16 bytes, plus (E + 1) int64 rounded up to 16 bytes and 256 bytes
 * (the offsets and the pairs, which a call that takes them copies there).  Sizes a call does not use are given as 0 (C, P, E)
 * with K = d = D = 1.  Host arithmetic only.
 * KLNMF_ERR_ARG: null `bytes`, T < 0 or T >= 2^31 - 1, C, P or E < 0, K, d or D < 1.  KLNMF_ERR_UNSUPP: beyond the limits.
 * Stands in for nothing of the reference: features/angle_histograms.py:199-221 allocates lists of arrays per stage. */
int klnmf_motion_work_bytes(int64_t T, int64_t C, int64_t d, int64_t K, int64_t P, int64_t D, int64_t E, uint64_t *bytes);

/* Angles and delayed velocities.  records: DEVICE [T, n_markers, 7] of `dtype`, contiguous (translation, then the quaternion
 * x y z w); pairs: HOST int32 [n_pairs][2], (source, dest) marker indices; offsets: HOST int64 [E + 1], offsets[0] = 0,
 * non-decreasing, offsets[E] = T: example e is the frames [offsets[e], offsets[e + 1]).  angles, vels: DEVICE [T, 3 n_pairs],
 * rows lda / ldv elements apart.  Per frame and pair: q = q_src^-1 * q_dst, its rotation matrix (the identity where
 * dot(q, q) < 4 eps), the Euler angles of axes 'sxyz' (cy > 4 eps, else the gimbal case with az = 0).  Velocities per example
 * with n frames and D = min(delay, n): vel[t] = angle[t] - angle[t - D] for t >= D within the example, else angle[t] - 0
 * (KLNMF_MOTION_PAD_ZEROS) or angle[t] - angle[n - D + t] (KLNMF_MOTION_PAD_CIRCULAR); never across an offset.  bounds /
 * vel_bounds: HOST double [2] (min, max) or null: angles (after the velocities were taken) and velocities are cut to
 * max(min(x, hi), lo).  Two launches (three with bounds) behind two small uploads (the offsets, the pairs).
 * KLNMF_ERR_ARG, nothing launched and nothing written: a null records, pairs, offsets, angles, vels or d_work, a stride below
 * 3 n_pairs, T < 1 or T >= 2^31 - 1, E < 1, n_markers < 1, n_pairs < 1, a pair index outside [0, n_markers), offsets that do
 * not start at 0, decrease, or do not end at T, delay < 1, an unknown padding, bounds with min > max or a NaN, a bad dtype, a
 * workspace below klnmf_motion_work_bytes(T, 0, 1, 1, 0, 1, E).  KLNMF_ERR_UNSUPP: n_pairs > KLNMF_MOTION_MAX_PAIRS.
 * Replaces `db_to_angles_and_vels` and `filter_values` (features/angle_histograms.py:45-94, 192-198: `get_angles` once per
 * frame and pair on lib/transformations.py:1031-1097, 1174-1193, 1228-1267; `delayed_velocities`, lib/utils.py:103-123). */
int klnmf_motion_angles_device(int device, int dtype, const void *records, int64_t T, int64_t n_markers, const int32_t *pairs,
                               int64_t n_pairs, const int64_t *offsets, int64_t E, int64_t delay, int padding,
                               const double *bounds, const double *vel_bounds, void *d_work, uint64_t work_bytes, void *angles,
                               int64_t lda, void *vels, int64_t ldv);

/* Whitening.  x: DEVICE [T, C] of `dtype`, rows ld apart; out: the same shape, rows ldo apart (may be x itself);
 * d_mean, d_std: DEVICE fp64 [C].  Per column: mean = sum / T, std = sqrt(sum((x - mean)^2) / T), both sums under the order
 * rule; a std of 0 is stored as 1; out = x / std, one division.  Five launches; no synchronisation.
 * KLNMF_ERR_ARG, nothing launched and nothing written: a null pointer, a stride below C, T < 1 or T >= 2^31 - 1, C < 1, a bad
 * dtype, a workspace below klnmf_motion_work_bytes(T, C, 1, 1, 0, 1, 0).
 * Replaces `whiten(d)` per degree of freedom (features/angle_histograms.py:209). */
int klnmf_motion_whiten_device(int device, int dtype, const void *x, int64_t ld, int64_t T, int64_t C, void *d_work,
                               uint64_t work_bytes, void *out, int64_t ldo, double *d_mean, double *d_std);

/* P k-means problems to convergence, scipy's `kmeans(obs, guess)`.  Problem p reads point set set_of[p] (HOST int32 [P], each
 * in [0, D)) and owns codebooks[p] (DEVICE [P, K, d] of `dtype`, contiguous, in/out).  One iteration of a problem: every point's
 * code among the problem's live rows (klnmf_kmeans.h's rule: fp64 squared distance, j ascending, the lowest index among equal
 * minima); the distortion = (sum over points of sqrt(least squared distance)) / T under the order rule; every live row with
 * members becomes their mean (sum under the order rule, one division); a live row without members is dropped for good
 * (d_alive[p][k] = 0, its values stay); the problem stops when |previous distortion - distortion| <= thresh, the first
 * iteration comparing against +inf.  All problems advance through two launches per iteration, the workgroups of a stopped
 * problem returning at once; every KLNMF_MOTION_POLL = 4 iterations the P stop flags are downloaded, and the call returns when
 * all are set.  On return: the codebooks after the last update, d_alive (DEVICE int32 [P, K]: code_book[has_members] is the live
 * rows in order), d_distortion (DEVICE fp64 [P]: the last one measured), d_iters (DEVICE int32 [P]), d_labels (DEVICE int32
 * [P, T] or null: the codes of a problem's last assignment), *unfinished (HOST) = -1, or the lowest problem that had not
 * stopped after max_iter iterations (the state is then that of max_iter iterations).
 * KLNMF_ERR_ARG, nothing launched and nothing written: a null points, set_of, codebooks, d_alive, d_distortion, d_iters, d_work
 * or unfinished, ld < d, set_stride < 0, T < 1 or T >= 2^31 - 1, d, K, D or P < 1, a set_of entry outside [0, D), a thresh
 * that is negative or NaN, max_iter < 1, a bad dtype, a workspace below klnmf_motion_work_bytes(T, 0, d, K, P, D, 0).
 * KLNMF_ERR_UNSUPP: K, d or K * d beyond the limits.
 * Replaces `kmeans(d, nb_bins, iter=20)` for every degree of freedom (features/angle_histograms.py:212) from the drawn rows
 * on: scipy's `_kmeans` loop of `vq` and `update_cluster_means`, restart after restart. */
int klnmf_motion_kmeans_device(int device, int dtype, const void *points, int64_t set_stride, int64_t ld, int64_t T, int64_t d,
                               int64_t D, const int32_t *set_of, int64_t P, void *codebooks, int64_t K, double thresh,
                               int max_iter, void *d_work, uint64_t work_bytes, int32_t *d_alive, double *d_distortion,
                               int32_t *d_iters, int32_t *d_labels, int *unfinished);

/* The examples' histograms.  Set s is quantised against codebooks[s] (DEVICE [D, K, d] of `dtype`, contiguous, all K rows
 * live).  soft = 0: a frame adds 1 to the bin of its code.  soft = 1: it adds h_c = w_c / sum_c w_c (c ascending from +0) with
 * w_c = exp(-alpha * d2_c / (1e-9 + min_c d2_c)), d2 the squared distance as above.  out: DEVICE [E, D * K] of `dtype`, rows
 * ldo apart, laid out [example][set][bin]: the sums over the example's frames, ascending from +0, each row then divided by its
 * sum over the columns ascending from +0 (an example without a frame: 0 / 0).  Two launches behind the upload of the offsets.
 * KLNMF_ERR_ARG, nothing launched and nothing written: a null pointer, ld < d, ldo < D * K, set_stride < 0, T < 1 or
 * T >= 2^31 - 1, d, K, D or E < 1, offsets as klnmf_motion_angles_device refuses them, soft outside {0, 1}, an alpha that is
 * not finite, a bad dtype, a workspace below klnmf_motion_work_bytes(T, 0, d, K, 0, D, E).  KLNMF_ERR_UNSUPP: the limits.
 * Replaces `get_histos` and the sums per example (features/angle_histograms.py:214-222; lib/vector_quantization.py:15-60). */
int klnmf_motion_hist_device(int device, int dtype, const void *points, int64_t set_stride, int64_t ld, int64_t T, int64_t d,
                             int64_t D, const void *codebooks, int64_t K, const int64_t *offsets, int64_t E, int soft,
                             double alpha, void *d_work, uint64_t work_bytes, void *out, int64_t ldo);

#ifdef __cplusplus
}
#endif
#endif /* KLNMF_MOTION_H */
