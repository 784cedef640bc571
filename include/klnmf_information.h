/* klnmf_information.h -- C-ABI of the atom x label information matrix: for every column ("atom") of a coefficient matrix and
 * every label, the mutual information between the atom's binned value and the presence of the label, for many matrices in one
 * fixed sequence of launches.
 *
 * An interface of its own beside klnmf.h (whose conventions, error codes and element types it uses): int status returns,
 * klnmf_last_error(), every entry point naming the reference interface it stands in for.  The same library, libklnmf.so, exports
 * the symbols of every header.
 *
 * What it computes (samples/plot_info_matrix.py:66-90, 126-136 on lib/metrics.py:33-55), for a job A [n, k], labels [n], L labels
 * and B bins; all arithmetic in fp64, an f32 value widened first:
 *   range   lo = min_i A[i, a], hi = max_i A[i, a]; lo == hi: lo -= 0.5, hi += 0.5 (np.histogram's rule for an empty range)
 *   edges   np.linspace(lo, hi, B + 1): step = (hi - lo) / B, e_b = fl(fl(b * step) + lo) for b < B, e_B = hi (step == 0:
 *           e_b = fl(fl(fl(b / B) * (hi - lo)) + lo))
 *   bin     of v: the b with e_b <= v < e_(b+1); v == hi lies in bin B - 1   (np.histogram(v, bins=B, range=(lo, hi)))
 *   counts  counts[a][l][b] = the rows with label l whose value of atom a lies in bin b (int32: exact, whatever the scheduling)
 *   table   for (a, l): t0[b] = counts[a][l][b], t1[b] = sum over l' of counts[a][l'][b] - t0[b]; p = t / n; the row marginals
 *           (sum_b t_c[b]) / n and the column marginals (t0[b] + t1[b]) / n are integer sums and one division
 *   info    I = sum_c sum_b p * log(p / (pr_c * pc_b)) over the cells with t > 0, c-major, b ascending -- metrics.py:37-43 on the
 *           table of plot_info_matrix.py:88-90.  L = 1 gives 0.
 * Outputs: job q writes behind the jobs before it, at the atom offset o_q = the sum of k of the jobs before it:
 *   info[o_q * L + l * k_q + a]  (fp64 for either dtype: per job the reference's (n_labels, K) matrix, plot_info_matrix.py:133-136)
 *   counts[(o_q * L + a * L + l) * B + b]  (int32)
 * Limits: n <= 2^30, k <= 2^20, L <= 65536, 1 <= B <= 256, (sum of k) * L * B <= 2^28, count <= 2^16. */
#ifndef KLNMF_INFORMATION_H
#define KLNMF_INFORMATION_H

#include "klnmf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KLNMF_INFORMATION_MAX_JOBS (1 << 16)
#define KLNMF_INFORMATION_MAX_BINS 256
#define KLNMF_INFORMATION_MAX_LABELS 65536
#define KLNMF_INFORMATION_MAX_CELLS (1 << 28)

/* One analysis: A [n, k], DEVICE pointer of the call's dtype, rows lda elements apart (lda >= k); labels: DEVICE int32 [n], every
 * one in [0, n_labels). */
typedef struct klnmf_information_job {
    const void *A;
    int64_t lda;
    const int32_t *labels;
    int64_t n, k;
} klnmf_information_job;

/* The bytes of device workspace a klnmf_information_many_device call of `count` jobs with `total_atoms` = the sum of k needs: the
 * job table, the jobs' flags, the per-atom ranges, the slabs of partial minima and maxima, and the counts (used where the caller
 * passes no d_counts).  A function of its four arguments alone.  KLNMF_ERR_ARG: a null `bytes`, an argument outside the limits.
 * Stands in for nothing of the reference: plot_info_matrix.py:66-72 allocates per histogram. */
int klnmf_information_work_bytes(int64_t count, int64_t total_atoms, int n_labels, int bins, uint64_t *bytes);

/* The analyses jobs[0 .. count) (a HOST array of device pointers) on `device`'s null stream in a fixed number of launches whatever
 * `count` is -- the ranges (two launches: partial minima / maxima, their combination), the histograms, the information -- and
 * synchronises.  No allocation per call: the job table, ranges, flags and (with d_counts null) the counts live in the caller's
 * workspace d_work (device memory, work_bytes >= klnmf_information_work_bytes).  d_info: fp64 [sum k][L] as laid out above;
 * d_counts: int32 [sum k][L][B] or null.  count = 0: KLNMF_OK, nothing done.
 * KLNMF_ERR_ARG, nothing launched and nothing written: a null pointer where data is needed (jobs, d_info, d_work; A or labels of
 * a job), lda < k, a dtype other than KLNMF_DT_F32 / KLNMF_DT_F64, n < 1 or k < 1, n_labels < 1, bins outside [1, 256], a shape
 * beyond the limits above, a workspace smaller than klnmf_information_work_bytes says.
 * KLNMF_ERR_ARG after the launches, the outputs of the named job unspecified (klnmf_last_error names the first such job): a label
 * outside [0, n_labels), a range that is not finite (a NaN or an infinity among the coefficients: np.histogram refuses it).
 * Replaces the body of the loop over runs of samples/plot_info_matrix.py:126-136: `mutual_information_by_label(internal[:, i],
 * by_label)` for every atom i (plot_info_matrix.py:66-90: K * n_labels calls of np.histogram and of metrics.mutual_information,
 * lib/metrics.py:37-43), for all runs in one call. */
int klnmf_information_many_device(int device, int dtype, int n_labels, int bins, const klnmf_information_job *jobs, int64_t count,
                                  double *d_info, int32_t *d_counts, void *d_work, uint64_t work_bytes);

/* One job on HOST arrays: A [n x k] row-major of `dtype`, labels int32 [n]; info fp64 [n_labels x k], counts int32
 * [k x n_labels x bins] or null.  The counterpart of klnmf_nearest for callers without device tensors (allocates, uploads, runs,
 * downloads).  Refusals as above.  Replaces `np.array([mutual_information_by_label(internal[:, i], by_label) for i in
 * range(K)]).T` (samples/plot_info_matrix.py:133-136; lib/metrics.py:37-43). */
int klnmf_information(int device, int dtype, int n_labels, int bins, int64_t n, int64_t k, const void *A, const int32_t *labels,
                      double *info, int32_t *counts);

/* The counter route of the histogram launch is a function of (n_labels, bins) alone: a workgroup keeps the counters of
 * T = min(64, floor(KLNMF_INFORMATION_LDS_BYTES / (4 * n_labels * bins))) atoms in LDS -- 64: the full tile; fewer: a shrunk tile;
 * T = 0: not even one atom's counters fit and the launch counts straight into device memory.  Every route gives the same
 * integers. */
#define KLNMF_INFORMATION_LDS_BYTES 32768

#ifdef __cplusplus
}
#endif
#endif /* KLNMF_INFORMATION_H */
