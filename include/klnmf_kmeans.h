/* klnmf_kmeans.h -- C-ABI of the codebook builders' device half: Lloyd iterations (scipy's kmeans2 with minit='matrix') and the
 * Gram matrix of one cluster's members, the two pieces the reference's `build_codebook` and `iterative_kmeans`
 * (features/hac.py:68-107) spend their time in.
 *
 * An interface of its own beside klnmf.h (whose conventions, error codes and dtype numbers it uses): int status returns,
 * klnmf_last_error(), every entry point naming the reference lines it stands in for.  The same library, libklnmf.so, exports
 * the symbols of every header.
 *
 * One Lloyd iteration.  label[t] = the index of the codebook row nearest to frame t, klnmf_hac.h's rule: the squared distance
 * sum_j (x_j - c_j)^2 in fp64 (f32 inputs promoted), j ascending, every difference, product and sum rounded on its own, the
 * lowest index among equal minima; a NaN distance never wins.  Then row k of the codebook becomes the mean of the frames with
 * label k: their sum in fp64 under the order rule below, divided once by their count (converted exactly), stored in the call's
 * dtype (rounded once more for f32).  A cluster without a member keeps its row bit for bit (kmeans2's missing='warn').  Exactly
 * n_iter iterations run -- kmeans2 has no stop rule inside its loop -- and the labels and counts returned are those of the LAST
 * assignment, taken before the last update, as kmeans2 returns them.
 *
 * The order rule.  Every sum over frames is formed per group of KLNMF_KMEANS_GROUP = 4096 consecutive frames, the group's
 * contributing frames added in ascending order starting from +0, and the groups' partial sums are then added in ascending
 * group order starting from +0; every addition is rounded to fp64.  The order depends on T alone, never on scheduling: two
 * calls on the same data give the same bits.  The Gram matrix adds the fp64 products x_i * x_j, each rounded on its own, under
 * the same rule, computes the upper triangle and mirrors it.
 *
 * Limits: K * d <= KLNMF_KMEANS_MAX_KD (the fp64 accumulators of a workgroup live in LDS: 104 KiB of the CU's 160) for the
 * Lloyd calls, d <= KLNMF_KMEANS_GRAM_MAX_D for the Gram call; beyond them KLNMF_ERR_UNSUPP before anything is launched.
 * T < 2^31. */
#ifndef KLNMF_KMEANS_H
#define KLNMF_KMEANS_H

#include "klnmf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KLNMF_KMEANS_TILE 256
#define KLNMF_KMEANS_GROUP 4096
#define KLNMF_KMEANS_MAX_KD 13312
#define KLNMF_KMEANS_GRAM_MAX_D 64

/* The bytes of device workspace a klnmf_kmeans_device or klnmf_kmeans_gram_device call on T frames of d columns and K units
 * needs: with G = max(1, ceil(T / 4096)) groups, the larger of G * K * d doubles + G * K int32 (the groups' partial sums and
 * counts) and, where d <= 64, G * (d (d + 1) / 2 + d) doubles + G int32 + one int64 (the Gram call's), each part rounded up to
 * 16 bytes.  Host arithmetic only.  KLNMF_ERR_ARG: a null `bytes`, T < 0 or T >= 2^31, d < 1, K < 1.  KLNMF_ERR_UNSUPP:
 * K * d > KLNMF_KMEANS_MAX_KD.
 * Stands in for nothing of the reference: scipy's kmeans2 allocates per iteration (features/hac.py:96). */
int klnmf_kmeans_work_bytes(int64_t T, int64_t d, int64_t K, uint64_t *bytes);

/* n_iter Lloyd iterations on `device`'s null stream.  frames: DEVICE [T, d] of `dtype` (f32 / f64), rows `ld` elements apart;
 * codebook: DEVICE [K, d] of the same type, rows `ldc` apart, in/out; d_labels: DEVICE int32 [T]; d_counts: DEVICE int64 [K].
 * Two launches per iteration whatever T and K are, no allocation, no host synchronisation: the results are ordered on the null
 * stream like any other work.  n_iter = 0: the labels and counts against the given codebook, two launches, nothing written to
 * the codebook.  T = 0: KLNMF_OK, the codebook untouched, the counts 0.
 * KLNMF_ERR_ARG, nothing launched and nothing written: a null pointer where data is needed (codebook, d_work, d_counts; frames
 * and d_labels with T > 0), a stride below d, d < 1, K < 1, T < 0, T >= 2^31, n_iter < 0, a dtype other than KLNMF_DT_F32 /
 * KLNMF_DT_F64, a workspace smaller than klnmf_kmeans_work_bytes says.  KLNMF_ERR_UNSUPP, nothing launched and nothing written:
 * K * d > KLNMF_KMEANS_MAX_KD.
 * Replaces `kmeans2(data, centroids, minit='matrix')` (features/hac.py:96; with the random draw made by the caller also
 * `kmeans2(data, k)`, :102) and, with n_iter = 0, `vq(data, centroids)` and `np.bincount(quantized, minlength=...)`
 * (features/hac.py:80-81). */
int klnmf_kmeans_device(int device, int dtype, const void *frames, int64_t ld, int64_t T, int64_t d, void *codebook, int64_t ldc,
                        int64_t K, int n_iter, void *d_work, uint64_t work_bytes, int32_t *d_labels, int64_t *d_counts);

/* The Gram matrix of the frames with d_labels[t] == cluster (cluster = -1: of every frame; d_labels may then be null):
 * d_gram (DEVICE fp64 [d * d]) = sum x x^T, d_colsum (DEVICE fp64 [d]) = sum x, *count (HOST) = their number (one
 * synchronisation).  Two launches.  A cluster without a member, or T = 0: zeros and *count = 0.  d_labels are a
 * klnmf_kmeans_device call's; a cluster that no label names (at or beyond that call's K) has no member.
 * KLNMF_ERR_ARG, nothing launched and nothing written: null d_gram, d_colsum, count or d_work; null frames with T > 0; null
 * d_labels with cluster >= 0 and T > 0; a stride below d; d < 1; T < 0 or T >= 2^31; cluster < -1; a bad dtype; a workspace
 * smaller than klnmf_kmeans_work_bytes(T, d, 1) says.  KLNMF_ERR_UNSUPP: d > KLNMF_KMEANS_GRAM_MAX_D.
 * Replaces the O(T d^2) half of `np.linalg.svd(data[associated, :])` (features/hac.py:84-85): the top right singular pair of
 * the members is the top eigenpair of this matrix (s_0^2 = lambda), which the caller takes from a d x d problem; and, with
 * cluster = -1, the mean and covariance of kmeans2's 'random' initialisation (features/hac.py:102). */
int klnmf_kmeans_gram_device(int device, int dtype, const void *frames, int64_t ld, int64_t T, int64_t d, const int32_t *d_labels,
                             int64_t cluster, void *d_work, uint64_t work_bytes, double *d_gram, double *d_colsum, int64_t *count);

/* The whole Lloyd call from HOST arrays: frames [T, d] and codebook [K, d] (in/out) of `dtype` with their strides, labels int32
 * [T], counts int64 [K].  Allocates, uploads, runs klnmf_kmeans_device, downloads.  Refusals as there.
 * Replaces `kmeans2(data, centroids, minit='matrix')` (features/hac.py:96) for callers without device tensors. */
int klnmf_kmeans(int device, int dtype, const void *frames, int64_t ld, int64_t T, int64_t d, void *codebook, int64_t ldc, int64_t K,
                 int n_iter, int32_t *labels, int64_t *counts);

#ifdef __cplusplus
}
#endif
#endif /* KLNMF_KMEANS_H */
