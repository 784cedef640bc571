/* klnmf_hac.h -- C-ABI of the windowed histograms of acoustic co-occurrences (HAC): the frames of up to 8 streams are vector
 * quantised once, and every window [t0, t1) of a host list becomes one row of a CSR matrix of lagged pair counts, built on the
 * device in a fixed number of launches.
 *
 * An interface of its own beside klnmf.h (whose conventions, error codes and dtype numbers it uses): int status returns,
 * klnmf_last_error(), every entry point naming the reference lines it stands in for.  The same library, libklnmf.so, exports
 * the symbols of every header.
 *
 * What it computes.  q_s[t] = the index of the codebook row nearest to frame t of stream s (scipy.cluster.vq.vq's label): the
 * squared distance sum_j (x_j - c_j)^2 in fp64 (f32 inputs promoted), j ascending, every product and sum rounded on its own, the
 * lowest index among equal minima; a NaN distance never wins.  Row w of the result is, streams outer and lags inner in the
 * caller's order, np.bincount(q[t0 + lag : t1] * K + q[t0 : t1 - lag], minlength = K * K) -- the reference's `coocurrences` on the
 * window's slice (features/hac.py:152-175), the later frame the high digit.  A window no longer than a lag contributes nothing
 * for that lag.  F = sum_s n_lags * K_s^2 columns.
 *
 * The result is CSR: int64 row pointers [n_windows + 1], int32 column indices ascending within a row, the counts as values of the
 * requested dtype; no explicit zeros, no duplicates -- what klnmf_upload_csr_device_rows reads.
 *
 * Routes.  A segment is a (window, stream, lag) triple of n_codes = t1 - t0 - lag pair codes.  n_codes <= KLNMF_HAC_SORT_MAX:
 * sorted in LDS.  Beyond that, K <= KLNMF_HAC_DENSE_MAX_K: counted in K^2 LDS counters.  A longer segment over a larger codebook
 * is refused with KLNMF_ERR_UNSUPP before anything is launched.
 * Limits: n_streams, n_lags in [1, 8]; T < 2^31; d, K >= 1, K^2 < 2^31; F < 2^31; n_windows * n_streams * n_lags < 2^31. */
#ifndef KLNMF_HAC_H
#define KLNMF_HAC_H

#include "klnmf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KLNMF_HAC_MAX_STREAMS 8
#define KLNMF_HAC_MAX_LAGS 8
#define KLNMF_HAC_SORT_MAX 4096
#define KLNMF_HAC_DENSE_MAX_K 192

/* One stream: frames [T, d] and its codebook [K, d], pointers of the call's dtype, row strides in elements (>= d).  T is the
 * call's: every stream has as many frames. */
typedef struct klnmf_hac_stream {
    const void *frames;
    int64_t ld;
    const void *codebook;
    int64_t ldc;
    int64_t d, K;
} klnmf_hac_stream;

/* The bytes of device workspace a klnmf_hac_count_device / klnmf_hac_fill_device pair needs: the codes int32 [n_streams, T], the
 * windows, the segment counts and offsets.  KLNMF_ERR_ARG: a null `bytes`, a count outside the limits above.
 * Stands in for nothing of the reference: each of its pool workers allocates what np.bincount returns (features/hac.py:169). */
int klnmf_hac_work_bytes(int n_streams, int64_t T, int n_lags, int64_t n_windows, uint64_t *bytes);

/* Quantises the streams (a HOST table of DEVICE pointers, `dtype` f32 / f64), counts the distinct pair codes of every segment and
 * scans them, on `device`'s null stream: d_indptr (device, int64 [n_windows + 1]) receives the row pointers, *nnz the stored
 * entries of the matrix (one synchronisation).  lags: HOST int32 [n_lags]; windows: HOST int64 [n_windows][2] = (t0, t1).  The
 * workspace then holds what klnmf_hac_fill_device needs.  Three launches and one copy of the windows, whatever n_windows is; no
 * allocation.  n_windows = 0: KLNMF_OK, d_indptr[0] = 0, *nnz = 0.  T = 0 (every window is then empty): KLNMF_OK, row pointers all 0.
 * KLNMF_ERR_ARG, nothing launched and nothing written: a null pointer where data is needed (streams, lags, nnz, d_indptr, d_work;
 * windows with n_windows > 0; frames with T > 0; a codebook), a stride below d, d < 1 or K < 1, a window outside [0, T] or with
 * t1 < t0, a lag < 1, more than 8 streams or lags (or none), F >= 2^31, a dtype other than KLNMF_DT_F32 / KLNMF_DT_F64, a
 * workspace smaller than klnmf_hac_work_bytes says.  KLNMF_ERR_UNSUPP, nothing launched and nothing written: a segment that fits
 * neither route; the message names the window and the stream.
 * Replaces, for all windows at once: `vq(data, centroids)` and `coocurrences(quantized, K, l) for l in lags` of
 * compute_coocurrences (features/hac.py:172-175, 152-169) as `hac` applies them per stream (features/hac.py:193-196) in every
 * `process_win` of the pool (samples/image_sound_eval_sliding.py:97-107), and the row pointers of `sp.vstack(vectors)` (:113). */
int klnmf_hac_count_device(int device, int dtype, const klnmf_hac_stream *streams, int n_streams, int64_t T, const int32_t *lags,
                           int n_lags, const int64_t *windows, int64_t n_windows, void *d_work, uint64_t work_bytes,
                           int64_t *d_indptr, int64_t *nnz);

/* The column indices (device, int32 [nnz]) and the counts (device, `value_dtype` [nnz]) of the matrix whose row pointers the
 * preceding klnmf_hac_count_device call with the same K (HOST int64 [n_streams]), T, lags and windows wrote, from the same
 * workspace left untouched since; nnz: what that call returned.  One launch.  nnz = 0: KLNMF_OK, nothing done.
 * KLNMF_ERR_ARG / KLNMF_ERR_UNSUPP as above, nothing launched and nothing written; also nnz < 0, null d_indices / d_values with
 * nnz > 0.
 * Replaces the indices and data of `sp.csc_matrix(win_hac)` per window and of `sp.vstack(vectors)`
 * (samples/image_sound_eval_sliding.py:100, 113), as CSR. */
int klnmf_hac_fill_device(int device, int value_dtype, const int64_t *K, int n_streams, int64_t T, const int32_t *lags, int n_lags,
                          const int64_t *windows, int64_t n_windows, const void *d_work, uint64_t work_bytes, int64_t nnz,
                          int32_t *d_indices, void *d_values);

/* The whole matrix from HOST arrays: the streams' pointers are host pointers here (frames [T x d] and codebooks [K x d] with
 * their strides); indptr int64 [n_windows + 1], indices int32 [capacity], values `value_dtype` [capacity], *nnz the entries
 * stored.  Allocates, uploads, counts, fills, downloads.  capacity < nnz: KLNMF_ERR_ARG with *nnz and indptr written and indices
 * and values untouched (sum over the segments of min(n_codes, K^2) is always enough).  Other refusals as above.
 * Replaces lines 97-113 of samples/image_sound_eval_sliding.py behind the MFCC front end, for callers without device tensors. */
int klnmf_hac(int device, int dtype, int value_dtype, const klnmf_hac_stream *streams, int n_streams, int64_t T,
              const int32_t *lags, int n_lags, const int64_t *windows, int64_t n_windows, int64_t *indptr, int64_t capacity,
              int32_t *indices, void *values, int64_t *nnz);

#ifdef __cplusplus
}
#endif
#endif /* KLNMF_HAC_H */
