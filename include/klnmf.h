/* klnmf.h -- C-ABI of the MI355X-native KL-divergence NMF hot path.
 *
 * This is the drop-in boundary for the multiplicative-update loop of
 * omangin/multimodal (`multimodal/lib/nmf.py`).  Every entry point below names
 * the reference interface it replaces (file:line, relative to the reference
 * root).  Plain pointers and sizes only; no exceptions cross the boundary:
 * every function returns an int status (0 = ok, <0 = error class) and the
 * message for the calling thread is available from klnmf_last_error().
 *
 * One context = one GPU (one process per GPU in the multi-GPU case).  The
 * collective between row shards is issued INSIDE the library on the native path
 * (klnmf_comm_init + klnmf_run_sharded / klnmf_run_more: RCCL over xGMI), or by
 * the caller between the klnmf_iter_* pieces (e.g. torch.distributed); see
 * INTEGRATION.md.  A context is used from one thread at a time; different
 * contexts may be used from different threads.  All calls are asynchronous on
 * the context's stream unless they return data to the host.
 *
 * Matrices named as in the reference: V/X [n,f] data (rows = samples),
 * W [n,k] coefficients, H [k,f] dictionary (`components_`), Q [n,f] ratio.
 */
#ifndef KLNMF_H
#define KLNMF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KLNMF_VERSION 100            /* 0.1.0 */

/* status codes */
#define KLNMF_OK            0
#define KLNMF_ERR_ARG      -1        /* bad argument / wrong state        */
#define KLNMF_ERR_ALLOC    -2        /* device or host allocation failed  */
#define KLNMF_ERR_HIP      -3        /* HIP runtime error                 */
#define KLNMF_ERR_UNSUPP   -4        /* shape not supported by this mode  */
#define KLNMF_ERR_RCCL     -5        /* an RCCL call failed, or librccl could not be opened */
#define KLNMF_ERR_REPLICA  -6        /* the dictionaries of a group's contexts differ after a loop (klnmf_group_run) */

/* arithmetic modes */
#define KLNMF_PREC_F64      0        /* fp64 everywhere (reference arithmetic)      */
#define KLNMF_PREC_F32      1        /* fp32 everywhere                              */
#define KLNMF_PREC_F16      2        /* fp16 MFMA operands (power-of-two-scaled images, saturating conversion), fp32
                                      * accumulate and masters, V stored 16-bit (scaled fp16): the throughput mode */
#define KLNMF_PREC_BF16     KLNMF_PREC_F16      /* round-1 name of the mode (its operands were bf16 then) */
/* (3 was KLNMF_PREC_F16_V32 -- the same kernels on fp32-stored V -- until round 5: retired, it missed the 1e-4 bar on a
 *  BASELINE shape and kept the generation-1 kernels in the library for no measured benefit) */
#define KLNMF_PREC_BF16X3   4        /* the fp32 mode (fp32 storage, loop, loss partials in fp64, every shape, any k, CSR on the
                                      * fp32 sparse kernels, any eps) with its three dense contractions on the bf16 matrix
                                      * cores: each fp32 operand x split into hi = bf16(x) and lo = bf16(x - hi), products
                                      * hi.hi + hi.lo + lo.hi accumulated in fp32 -- each product within ~2^-16 of a.b
                                      * (relative), no scaling (bf16 has fp32's exponent range; operands below 3.39e38) */
#define KLNMF_PREC_F16X3    5        /* fp32 storage (V, Q, W, H), loss partials in fp64, any eps, with every operand of the three
                                      * dense contractions split into two fp16 parts under a power-of-two scale: hi = f16(x s),
                                      * lo = f16(x s - hi), products hi.hi + hi.lo + lo.hi accumulated in fp32.  k <= 256: the
                                      * loop's row pass (loss + ratio + W rule) and column pass are fused split-fp16 kernels;
                                      * k > 256, the single steps and CSR input: the KLNMF_PREC_BF16X3 / fp32 kernels */

/* host element types for uploads / downloads */
#define KLNMF_DT_F32        0
#define KLNMF_DT_F64        1

typedef struct klnmf_ctx klnmf_ctx;
typedef struct klnmf_group klnmf_group;

/* ---- library / device -------------------------------------------------- */
int         klnmf_version(void);
const char *klnmf_last_error(void);
/* arch string (e.g. "gfx950"), CU count, HBM bytes: roofline constants for bench.py */
int         klnmf_device_info(int device, char *arch, int arch_len,
                              int *cu_count, uint64_t *hbm_bytes);

/* ---- context ----------------------------------------------------------- */
/* stream: a hipStream_t to run on (e.g. torch's current stream), NULL for an own (non-blocking)
 * stream, or KLNMF_STREAM_DEFAULT for the device's default (null) stream -- whose handle is 0 and
 * could not be told from "no stream" otherwise; it is what torch reports as its current stream unless
 * the caller switched streams, and collectives issued through torch are ordered against it.  Replaces constructing KLdivNMF (nmf.py:136-145) + the implicit
 * "everything lives in host numpy arrays" of the reference. */
#define KLNMF_STREAM_DEFAULT ((void *)(intptr_t)-1)
int klnmf_create(klnmf_ctx **out, int device, int precision, void *stream);
int klnmf_destroy(klnmf_ctx *ctx);

/* Declare the local problem: n rows held by this context, f features, k
 * components, and the capacity of the per-iteration loss record.
 * (nmf.py:196-199: shapes taken from X and n_components.) */
int klnmf_set_problem(klnmf_ctx *ctx, int64_t n, int64_t f, int64_t k,
                      int64_t max_iter_capacity);

/* ---- data in ------------------------------------------------------------ */
/* KLNMF_PREC_BF16 stores V as fp16 of c*V with c the power of two that puts
 * c*vmax in [2^14, 2^15); call this with vmax >= max(scale * src) over ALL
 * blocks (and all ranks: the factor must be common) before the first upload.
 * Without it c = 1 (fine for data in fp16's range).  No-op in the other modes. */
int klnmf_set_v_max(klnmf_ctx *ctx, double vmax);
/* Give the problem's device memory back (to the library's block cache) and keep the context -- its stream, its
 * communicator -- for a later klnmf_set_problem.  Hosts that run many short fits in sequence (experiment.py:158-180)
 * keep a few contexts alive this way instead of creating one per fit. */
int klnmf_release_problem(klnmf_ctx *ctx);
/* Forget the uploaded matrix: zero V and the sums the upload kernels accumulate (sum of V as stored, the
 * storage-rounding correction of the loss, the count of values beyond the announced maximum), so that the same
 * context can take another matrix of the same shape; klnmf_set_v_max may be called again afterwards.  (Uploading
 * a block twice without this counts it twice in the reported loss.) */
int klnmf_reset_V(klnmf_ctx *ctx);
/* Upload the sub-block V[row0:row0+rows, col0:col0+cols] = scale * src, src a
 * host array with leading dimension ld (elements).  One call per modality
 * block replaces learner.py:53-56 (`safe_hstack([c * m ...])`): the scale,
 * cast and column placement are fused into the upload (K6). */
int klnmf_upload_V(klnmf_ctx *ctx, const void *src, int dtype,
                   int64_t rows, int64_t cols, int64_t ld,
                   int64_t row0, int64_t col0, double scale);
/* Same from a device-resident fp32 block (bench / device-side pipelines). */
int klnmf_upload_V_device(klnmf_ctx *ctx, const float *dsrc,
                          int64_t rows, int64_t cols, int64_t ld,
                          int64_t row0, int64_t col0, double scale);
/* Same with a row gather: row i of the block is row drow_idx[i] (device array) of the device-resident
 * matrix dsrc.  Replaces the per-run `x[train, :]` / `x[test, :]` copies of experiment.py:163-164 and the
 * re-upload that follows them (next-row N2: the stacked data stays on the device across runs). */
int klnmf_upload_V_device_rows(klnmf_ctx *ctx, const float *dsrc, const int64_t *drow_idx,
                               int64_t rows, int64_t cols, int64_t ld,
                               int64_t row0, int64_t col0, double scale);
/* Weights on the cost function (nmf.py:159-175: `weights`, "used as coefficients on each element of the data"; the
 * reference ignores the argument): the sub-block Om[row0:row0+rows, col0:col0+cols] = src of an n x f buffer of the
 * context's element type beside V, arguments as klnmf_upload_V without the scale.  The first upload of a problem takes
 * the buffer filled with 1, so a caller uploads only the blocks that carry weights.  From then on the problem is
 * weighted (klnmf_query KLNMF_Q_WEIGHTED): klnmf_run / klnmf_run_more, the loop in pieces, klnmf_update, klnmf_step_Q / _W /
 * _H and klnmf_error minimise sum Om o d(V | W.H) (csrc/weighted.hip.h) -- the loss and the stop rule are the weighted
 * ones, klnmf_step_Q leaves R = Om o Q, a rule's factor is 1 where its denominator (Om.H^T, W^T.Om) is 0, and the H rule
 * normalises the rows as ever; klnmf_init_W stays W0 = V.H0^T.  Om >= 0 is the caller's contract.  Dense problems in
 * KLNMF_PREC_F64 / KLNMF_PREC_F32 only: KLNMF_ERR_UNSUPP on a CSR problem and in every other precision, and where a
 * weighted context enters a loop on a communicator or a group (klnmf_run_sharded, klnmf_loop_begin*_sharded / _agreed,
 * klnmf_group_create / _run), whose exchange carries no denominator, and where weights are uploaded while such a loop is
 * open (until klnmf_loop_end).  The weighted loss is available through klnmf_error (and the loops' records) only:
 * klnmf_loss_terms stays refused in the exact modes, weighted or not.  klnmf_set_problem* and klnmf_release_problem drop
 * the weights with the problem. */
int klnmf_upload_weights(klnmf_ctx *ctx, const void *src, int dtype,
                         int64_t rows, int64_t cols, int64_t ld,
                         int64_t row0, int64_t col0);
/* Drop the weights (nmf.py:159-175: back to the reference's unweighted cost) -- or the presence mask of
 * klnmf_upload_presence: the problem runs the unweighted kernels again. */
int klnmf_clear_weights(klnmf_ctx *ctx);
/* Weights of the form Om[i, j] = P[i, m(j)] (a modality absent from some samples: learner.py:53-56 stacks the modalities as
 * contiguous column ranges; the reference has no counterpart): P is n x n_mod, m(j) the modality whose column range
 * [col_bounds[m], col_bounds[m + 1]) holds column j.  Sets rows row0 .. row0 + rows - 1 of P from src[rows][n_mod] (leading
 * dimension ld >= n_mod).  col_bounds has n_mod + 1 entries, 0 = b_0 < b_1 < ... < b_M = f, 1 <= n_mod <=
 * KLNMF_MAX_MODALITIES.  The first call of a problem fixes the bounds and takes P filled with 1; a later call with other bounds
 * returns KLNMF_ERR_ARG.  From then on the problem is masked (klnmf_query KLNMF_Q_PRESENCE = n_mod; KLNMF_Q_WEIGHTED stays 0:
 * there is no n x f buffer): every call that minimises the weighted cost on a weighted problem minimises it on this one, to
 * the same rules, with the denominators Om.H^T = P.S (S the dictionary's row sums per modality) and W^T.Om = D[., m(j)]
 * (D = W^T.P) formed in n k n_mod operations each (csrc/presence.hip.h); results agree with the same weights uploaded through
 * klnmf_upload_weights within the exact modes' rounding, not bit for bit.  P >= 0 is the caller's contract.  Refusals, each
 * leaving the context and the problem as they were: KLNMF_ERR_UNSUPP on a CSR problem, outside KLNMF_PREC_F64 / F32 and while a
 * loop over row shards is open; KLNMF_ERR_ARG for bad bounds, n_mod out of range, rows out of range, and on a problem that
 * holds weights (as klnmf_upload_weights on a problem that holds a mask); a masked context is refused (KLNMF_ERR_UNSUPP)
 * wherever a weighted one is.  klnmf_clear_weights, klnmf_set_problem* and klnmf_release_problem drop the mask. */
#define KLNMF_MAX_MODALITIES 16
int klnmf_upload_presence(klnmf_ctx *ctx, const void *src, int dtype,
                          int64_t rows, int64_t ld, int64_t row0,
                          const int64_t *col_bounds, int n_mod);
/* klnmf_upload_presence for a mask that lives in DEVICE memory of the context's device, gathered there by row index and by source
 * column in one launch (the reference has no counterpart: it has no mask, and experiment.py:163-164 slices every per-sample array
 * of a run on the host):
 *     P[row0 + i, m] = src_cols[m] >= 0 ? dP[drow_idx[i] * ld + src_cols[m]] : 1          i < rows, m < n_mod
 * dP: src_rows rows, ld elements apart, KLNMF_DT_F32 or KLNMF_DT_F64, cast to the context's type as klnmf_upload_presence casts a
 * host upload (a float64 source in KLNMF_PREC_F64 gives P the bits of the host path).  drow_idx: `rows` int64 indices in device
 * memory, any order, repeats allowed; null: rows 0 .. rows - 1 of the source (as klnmf_upload_V_device_rows_dt reads it).
 * src_cols: n_mod source columns, each in [0, ld) or -1 (the modality has no column: its weight is 1).  col_bounds, n_mod, row0:
 * as in klnmf_upload_presence.  State and refusals are klnmf_upload_presence's -- the first mask upload of a problem fixes the
 * bounds and takes P filled with 1; KLNMF_ERR_UNSUPP on a CSR problem, outside KLNMF_PREC_F64 / F32 and while a loop over row
 * shards is open; KLNMF_ERR_ARG for bad bounds, n_mod out of range, rows out of range, a problem that holds weights -- and
 * KLNMF_ERR_ARG as well for a source column outside [-1, ld) and for a row index outside [0, src_rows): the indices are checked
 * on the device before anything is read through them, the host reads the flag back, and only then is the mask taken and the
 * gather launched.  A refused call leaves the problem exactly as it was.  Synchronous: dP and drow_idx are free to go on return. */
int klnmf_upload_presence_device_rows(klnmf_ctx *ctx, const void *dP, int dtype, int64_t src_rows, int64_t ld,
                                      const int64_t *drow_idx, int64_t rows, int64_t row0,
                                      const int *src_cols, const int64_t *col_bounds, int n_mod);
/* Dictionary [k,f], C order (nmf.py:149-155 `_init_dictionary`, learner.py:13
 * `components_ = dictionary`). */
int klnmf_set_H(klnmf_ctx *ctx, const void *src, int dtype);
/* Coefficients [n,k], C order (tests call `_update(X, W)` with their own W). */
int klnmf_set_W(klnmf_ctx *ctx, const void *src, int dtype);
/* Ratio [n,f] given by the caller (nmf.py:338-351: the `Q=` argument).
 * F64/F32 modes only. */
int klnmf_set_Q(klnmf_ctx *ctx, const void *src, int dtype);

/* ---- the path ----------------------------------------------------------- */
/* W0 = V . H^T  (nmf.py:156). */
int klnmf_init_W(klnmf_ctx *ctx);

/* The whole loop of nmf.py:212-222 on the device, single GPU:
 *   for it in 1..max_iter: err = error(); if prev - err < tol_abs: break;
 *                          errors.append(err); W (and H if fit) = update
 * errors_out receives n_done losses (each recorded before its update);
 * *stopped = 1 when the stop rule fired (the break), 0 when the limit ended
 * the loop.  Synchronous. */
int klnmf_run(klnmf_ctx *ctx, int64_t max_iter, int fit, double tol_abs,
              double *errors_out, int64_t *n_done, int *stopped);

/* The same loop in pieces, for the row-sharded multi-GPU case: the host issues
 * the collective between the pieces (sum of the exchange buffers over ranks).
 *   klnmf_loop_begin                          reset prev_error / counters
 *   per iteration:
 *     klnmf_iter_rowpass   loss partial + W update        -> loss exchange [0]
 *     [all-reduce loss[0]: may run while the column pass computes]
 *     klnmf_iter_colpass   H numerator W_new^T . Q_old    -> numerator exchange; its last launch writes loss[1], the count of
 *                          fp8-monitor trips and unfixable ratio entries of this iteration
 *     [all-reduce numerator exchange]
 *     [all-reduce loss[1] -- BEHIND klnmf_iter_colpass, never together with loss[0] in front of it -- on the iterations for
 *      which klnmf_query(KLNMF_Q_FP8_POLL_DUE) answers 1: the klnmf_iter_advance below then polls the sum, and every rank
 *      leaves the fp8 regime in the same iteration]
 *     klnmf_iter_decide    stop rule (nmf.py:214-220) on loss[0]
 *     klnmf_iter_update_H  H * num, row-normalise (nmf.py:349-350)
 *     klnmf_iter_advance   swap the W_old / W_new buffers
 *   klnmf_loop_end         sync, fetch errors / counters
 * After the stop rule fires every later piece is a no-op on the device, so the
 * host may enqueue all max_iter iterations without synchronising. */
int klnmf_loop_begin(klnmf_ctx *ctx);
/* The same for one rank of a row-sharded problem: the fp8 decision of the loop (16-bit modes) is taken from the sums over
 * ALL shards -- sum of V (klnmf_query_f64 KLNMF_QF_SUM_V, all-reduced) and its element count -- so that every rank runs
 * the same kernels and the result does not depend on the partition beyond summation order. */
int klnmf_loop_begin_sharded(klnmf_ctx *ctx, double sum_v_all, double cells_all);
/* ... and with the number of entries of V that are > 0 over all shards (klnmf_query_f64 KLNMF_QF_NNZ_V, all-reduced): fp8 ratio
 * tiles need enough of them per column, not enough rows (sparse data stored densely).  nnz_all < 0: as the call above (dense). */
int klnmf_loop_begin_sharded_nnz(klnmf_ctx *ctx, double sum_v_all, double cells_all, double nnz_all);
/* ... and with the conjunction over all ranks of "this shard's SHAPE allows fp8 ratio tiles" (klnmf_query
 * KLNMF_Q_RATIO_TILE_BYTES == 1, all-reduced as a minimum): shards differ by a row tile and the last one takes the remainder,
 * so they can straddle the row threshold -- ranks must not mix tile formats (the numerators of the two differ by sqrt(2)).
 * fp8_shape_all < 0: this rank's own shape decides (the calls above).  klnmf_loop_begin on a communicator agrees it itself. */
int klnmf_loop_begin_agreed(klnmf_ctx *ctx, double sum_v_all, double cells_all, double nnz_all, int fp8_shape_all);
/* `iters` whole iterations of the open loop at once, enqueued exactly as klnmf_run enqueues them (callers that fence between
 * two parts of one loop: warm-up | timed iterations of bench.py).
 * On a context that holds an RCCL communicator of more than one rank (klnmf_comm_init below) klnmf_loop_begin and
 * klnmf_run_more are klnmf_run_sharded in parts: the entry agrees the refusals and the fp8 decision over the communicator,
 * every iteration carries the ONE grouped all-reduce (numerator + loss) between column pass and stop rule; tol_abs is then
 * tol x n_total x f of the GLOBAL shape (nmf.py:207). */
int klnmf_run_more(klnmf_ctx *ctx, int64_t iters, int fit, double tol_abs);
int klnmf_iter_rowpass(klnmf_ctx *ctx, int fit);
int klnmf_iter_decide(klnmf_ctx *ctx, double tol_abs);
int klnmf_iter_colpass(klnmf_ctx *ctx);
int klnmf_iter_update_H(klnmf_ctx *ctx);
/* advance the W ping-pong after one iteration's pieces have been enqueued */
int klnmf_iter_advance(klnmf_ctx *ctx);
int klnmf_loop_end(klnmf_ctx *ctx, double *errors_out, int64_t *n_done,
                   int *stopped);
/* ---- Row shards over the GPUs of one node: the native collective path -----------------------------
 * One process (or thread) per GPU, each with its own context holding n_local rows of V and W; the dictionary is
 * replicated.  The reference has no counterpart (it is a single process); what is exchanged per fit iteration is
 * exactly what the algebra needs: the k x f numerator W_new^T.Q of the H rule (nmf.py:349) and the scalar loss
 * (nmf.py:214), summed over the ranks by ONE grouped RCCL all-reduce on the context's stream (xGMI inside a node).
 * The W rule and a transform exchange only the loss.  librccl is opened at run time on the first klnmf_comm_* call.
 *
 *   rank 0:  klnmf_comm_unique_id(id)  -> send the 128 bytes to every rank (any channel: MPI, a file, torch.distributed)
 *   each:    klnmf_comm_init(ctx, id, rank, nranks)
 *            klnmf_comm_max(ctx, &vmax) -> klnmf_set_v_max(ctx, vmax)      (the storage factor must be common)
 *            uploads, klnmf_set_H (same H on every rank), klnmf_init_W
 *            klnmf_run_sharded(ctx, n_total, ...)                           (errors / n_done / stopped identical on all ranks)
 */
#define KLNMF_COMM_ID_BYTES 128
int klnmf_comm_unique_id(void *id_out /* KLNMF_COMM_ID_BYTES */);
int klnmf_comm_init(klnmf_ctx *ctx, const void *id, int rank, int nranks);
int klnmf_comm_destroy(klnmf_ctx *ctx);
/* all-reduce(max) of one host double over the communicator (no-op without one) */
int klnmf_comm_max(klnmf_ctx *ctx, double *value);
/* klnmf_run over row shards: tol is the RELATIVE tolerance of nmf.py:207 (x n_total x f inside, the global shape).
 * Without a communicator (or with one of size 1) it is klnmf_run on the local rows. */
int klnmf_run_sharded(klnmf_ctx *ctx, int64_t n_total, int64_t max_iter, int fit, double tol,
                      double *errors_out, int64_t *n_done, int *stopped);

/* Device pointers of the two exchange buffers (what the collective sums):
 * loss: 2 doubles ([0] the loss partial, [1] this rank's count of fp8 ratio entries beyond the exact fix-up's list: the
 * summed value tells every rank when a loop gives fp8 tiles up); numerator: *numer_count elements of fp32 (BF16 modes,
 * F32) or fp64 (F64).  The buffers are owned by the context. */
int klnmf_exchange_buffers(klnmf_ctx *ctx, void **loss_ptr, void **numer_ptr,
                           int64_t *numer_count, int *numer_is_f64);
/* Layout of the numerator buffer: component rows of *row_stride elements, of which the first k rows
 * (*valid_count elements from the start) carry data -- what a collective has to move; the rest is padding. */
int klnmf_exchange_layout(klnmf_ctx *ctx, int64_t *row_stride, int64_t *valid_count);
/* Column-range form of the numerator exchange (round 4): with KLNMF_COMM_PARTS = P > 1 (read by klnmf_set_problem; 16-bit
 * modes, fused tail) the H numerator of nmf.py:349 can be produced and exchanged in P column parts, so that the all-reduce of
 * part p runs while the column pass of part p + 1 computes.  Part p = columns [col0[p], col0[p] + ncols[p]) of all k
 * components, stored as ONE contiguous block of counts[p] = k x (padded part width) elements at element offset offsets[p]
 * of the numerator buffer (klnmf_exchange_buffers: *numer_count covers this layout too).  Arrays of KLNMF_MAX_PARTS entries;
 * *nparts = 1 when the problem is not split: the one part is the whole-matrix layout of klnmf_exchange_layout.
 *   per iteration:  klnmf_iter_rowpass | for p in 0 .. P-1: klnmf_iter_colpass_part(p) -> [all-reduce part p] |
 *                   klnmf_iter_decide | klnmf_iter_update_H (applies the parts) | klnmf_iter_advance
 * klnmf_run_sharded / klnmf_run_more on a communicator do the same natively (part all-reduces on a second stream). */
#define KLNMF_MAX_PARTS 4
int klnmf_exchange_parts(klnmf_ctx *ctx, int *nparts, int64_t *offsets, int64_t *counts, int64_t *col0, int64_t *ncols);
int klnmf_iter_colpass_part(klnmf_ctx *ctx, int part);
/* (Round 4: the collective of the native path -- klnmf_run_sharded -- is issued INSIDE the library; these entry points serve
 * callers that sequence the loop's pieces around their own collective, e.g. torch.distributed.)
 * Use caller-owned device buffers as the exchange buffers instead (e.g. torch
 * tensors handed to torch.distributed.all_reduce): loss_ptr >= 2 doubles,
 * numer_ptr >= numer_count elements.  NULL keeps the current buffer. */
int klnmf_bind_exchange(klnmf_ctx *ctx, void *loss_ptr, void *numer_ptr);

/* ---- Row shards driven from ONE host thread: a group of contexts (SURVEY.md 8e's ctx_create(device_ids[], n_dev)) ---------
 * One ordinary context per row shard, each on one device; a device may repeat (several shards on one GPU).  What travels per fit
 * iteration is what the RCCL path exchanges -- the numerator of the H rule (nmf.py:349) and the two loss doubles (nmf.py:214) --
 * summed by two launches per context that read the peers' buffers directly (peer access; fine-grained device memory where the
 * members are on distinct devices), ordered by HIP events only: no flags, no spinning, no graphs.
 * Every element is summed in shard order, so every replica of H holds the same bits.
 *   each shard:  klnmf_create(device_i) -> klnmf_set_problem(n_i, f, k, cap) -> klnmf_set_v_max(max over ALL shards) -> uploads ->
 *                klnmf_set_H (the same H) -> klnmf_init_W
 *                (CSR: klnmf_set_problem_sparse(n_i, f, k, cap, nnz_i) -> klnmf_upload_csr_rows of the shard's rows -> klnmf_set_H ->
 *                klnmf_init_W; a shard may hold no stored entry)
 *   klnmf_group_create(&g, ctxs, n) -> klnmf_group_run(g, n_total, ...) (as often as wanted) -> klnmf_group_destroy(g)
 *
 * klnmf_group_create  contexts whose problems are set, in row order; they must share f, k, precision and capacity, and be all
 *                     dense or all CSR (KLNMF_ERR_ARG otherwise: the contexts stay as they were).  Enables peer access between every pair of distinct devices (KLNMF_ERR_UNSUPP naming
 *                     the pair where hipDeviceCanAccessPeer says no), allocates the exchange buffers and binds them to the
 *                     contexts (klnmf_bind_exchange).  A context belongs to one group at a time. */
int klnmf_group_create(klnmf_group **out, klnmf_ctx *const *ctxs, int n);
/* klnmf_group_run  the whole loop of nmf.py:212-222 over the group's shards, fit (H rule) or transform (fit = 0: the loss
 *                  alone is exchanged); tol is the RELATIVE tolerance of nmf.py:207 (x n_total x f inside).  The loop's entry is
 *                  agreed on the host: if any shard is refused (V beyond the announced maximum, factors beyond the fp16 operand
 *                  range) every shard fails together before anything is enqueued, and the fp8 decision is taken from the sums
 *                  over all shards (klnmf_loop_begin_agreed on each).  Per iteration: row pass, column pass, exchange, stop rule,
 *                  H rule; the stop rule is polled every 16 iterations.  errors_out / n_done / stopped: shard 0's (identical on
 *                  every shard).  After a fit the dictionaries of all shards are compared bit for bit: KLNMF_ERR_REPLICA if
 *                  they differ.  Synchronous. */
int klnmf_group_run(klnmf_group *g, int64_t n_total, int64_t max_iter, int fit, double tol,
                    double *errors_out, int64_t *n_done, int *stopped);
/* klnmf_group_destroy  frees the exchange buffers and gives every context its own back (destroy the group before the
 *                      contexts' problems are released or re-set). */
int klnmf_group_destroy(klnmf_group *g);
/* klnmf_group_enqueue_time  the host's time to enqueue one iteration of the last klnmf_group_run on this thread (every member's
 *                           pieces, waits and exchange launches; the stop rule's polls every 16 iterations excluded): the
 *                           iterations timed, the median and the largest, in milliseconds.  The median of a loop that keeps the
 *                           GPU busy is what one host thread costs per iteration (scripts/group_timing.py). */
int klnmf_group_enqueue_time(klnmf_group *g, int64_t *iterations, double *median_ms, double *max_ms);
/* klnmf_group_selftest  the exchange alone on buffers of its own: n buffers of `count` elements (dtype KLNMF_DT_F32 /
 *                       KLNMF_DT_F64) on devices[0 .. n) filled with values whose sum depends on the order of summation,
 *                       both phases run, every buffer and loss pair compared bit for bit with the host's sum in shard order;
 *                       *failed = mismatching elements (0 = pass). */
int klnmf_group_selftest(const int *devices, int n, int64_t count, int dtype, int *failed);

/* Step-granular entry points (unit parity with the reference's private
 * methods).  Synchronous. */
/* error(X, W, H)                      nmf.py:297-310 + metrics.py:18-20 */
int klnmf_error(klnmf_ctx *ctx, double *loss);
/* Diagnostic: the terms klnmf_error assembles in the 16-bit modes, in the caller's units:
 * terms[0] = sum x~ ln((x~+eps)/(W.H+eps)), [1] = sum W.H, [2] = sum x~ (V as stored),
 * [3] = the storage-rounding correction C = KL(x~ || x); loss = [0] + [1] - [2] - [3]
 * (metrics.py:18-20 split into its three sums).  KLNMF_ERR_UNSUPP in the exact modes. */
int klnmf_loss_terms(klnmf_ctx *ctx, double *terms);
/* one _update(X, W, _fit) without stop rule: nmf.py:232-257 */
int klnmf_update(klnmf_ctx *ctx, int fit);
/* eps of klnmf_step_Q (the `eps=` argument of _Q, nmf.py:325; default 1e-8).
 * The loop itself always uses 1e-8, as the reference does (nmf.py:232,251). */
int klnmf_set_ratio_eps(klnmf_ctx *ctx, double eps);
/* Q = (V+eps)/(W.H+eps) into the context's Q buffer (F64/F32 modes): nmf.py:325-336 */
int klnmf_step_Q(klnmf_ctx *ctx);
/* W <- W * (Q . H^T) with the Q buffer: nmf.py:338-343 */
int klnmf_step_W(klnmf_ctx *ctx);
/* H <- normalize_rows(H * (W^T . Q)) with the Q buffer: nmf.py:345-351 */
int klnmf_step_H(klnmf_ctx *ctx);
/* generalized_KL(x, y) of two host arrays of `count` elements: metrics.py:18-20 */
int klnmf_generalized_kl(klnmf_ctx *ctx, const void *x, const void *y, int dtype,
                         int64_t count, double eps, double *out);

/* ---- data out ----------------------------------------------------------- */
int klnmf_get_W(klnmf_ctx *ctx, void *dst, int dtype);   /* [n,k] */
int klnmf_get_H(klnmf_ctx *ctx, void *dst, int dtype);   /* [k,f] */
int klnmf_get_Q(klnmf_ctx *ctx, void *dst, int dtype);   /* [n,f], F64/F32 modes */

/* ---- device-resident operands (next-row N1) -------------------------------
 * The evaluation of an experiment (experiment.py:233-277, 332-371) runs 2 M .. 12 transforms per run on a fixed dictionary,
 * reconstructs modalities from the coefficients (learner.py:80-84) and compares in every space (evaluation.py:103-116).
 * With these the dictionary, the coefficients and the reconstructions never leave the GPU: pointers are DEVICE memory on the
 * context's device (e.g. torch tensors), row strides in elements.
 *   klnmf_set_H_device           a column block of `components_` (nmf.py:283-284; get_dico / get_stacked_dicos,
 *                                learner.py:43-51) from a device-resident dictionary: H[:, col0 : col0 + ncols] <- src
 *                                ([k, ncols], rows `ld` apart); `last` != 0 on the block that completes the dictionary
 *   klnmf_get_W_device           the coefficients of the last loop (what transform returns, nmf.py:291) -> [n, k], rows `ld` apart
 *                                (both on dense and on CSR problems)
 *   klnmf_upload_V_device_rows_dt klnmf_upload_V_device_rows for float32 or float64 device-resident modalities
 *   klnmf_matmul_device          reconstruct_modalit{y,ies} (learner.py:80-84): C[m,n] = A[m,kk] . B[kk,n]
 *   klnmf_all_distances_device   all_distances (metrics.py:80-86) of two device matrices -> [na, nb] on the device */
int klnmf_set_H_device(klnmf_ctx *ctx, const void *dsrc, int dtype, int64_t ld, int64_t col0, int64_t ncols, int last);
int klnmf_get_W_device(klnmf_ctx *ctx, void *ddst, int dtype, int64_t ld);
int klnmf_upload_V_device_rows_dt(klnmf_ctx *ctx, const void *dsrc, int dtype, const int64_t *drow_idx, int64_t rows,
                                  int64_t cols, int64_t ld, int64_t row0, int64_t col0, double scale);
int klnmf_matmul_device(int device, int dtype, int64_t m, int64_t n, int64_t kk, const void *dA, int64_t lda,
                        const void *dB, int64_t ldb, void *dC, int64_t ldc);
int klnmf_all_distances_device(int device, int dtype, int metric, int64_t na, int64_t nb, int64_t d, const void *dA,
                               int64_t lda, const void *dB, int64_t ldb, void *dout);

/* ---- introspection ------------------------------------------------------ */
/* What a context decided and what its last loop actually ran -- no reference counterpart (the reference has one
 * arithmetic); bench.py and the parity tests read it instead of mirroring the library's rules on the host.
 *   KLNMF_Q_FP8_LOOP          1 if the current / last loop was allowed fp8 ratio tiles (shape and range rules at the loop's entry;
 *                             what the tiles' rounding noise does to this data is measured while the loop runs: the monitor below)
 *   KLNMF_Q_FP8_TILE_ITERS    iterations of that loop whose ratio tiles were fp8 (e4m3 of ratio x sqrt(2) / 8, stochastically rounded)
 *   KLNMF_Q_FP8_COL_ITERS     iterations whose H-numerator product ran on e4m3 operands on both sides
 *   KLNMF_Q_RATIO_TILE_BYTES  bytes per element of V the stored ratio tiles take in an fp8 iteration (1), else 2; 0: none stored
 *   KLNMF_Q_COMM_RANKS        ranks RCCL reports for the context's communicator (ncclCommCount); 1 without one */
#define KLNMF_Q_FP8_LOOP          0
#define KLNMF_Q_FP8_TILE_ITERS    1
#define KLNMF_Q_FP8_COL_ITERS     2
#define KLNMF_Q_RATIO_TILE_BYTES  3
#define KLNMF_Q_COMM_RANKS        4
/* e4m3 saturation in the last loop -- counted, and kept out of the result:
 *   KLNMF_Q_W8_SATURATED     entries of the e4m3 W image beyond 448 x their component's scale (a column that more than doubled
 *                            in one update), KLNMF_Q_W8_FALLBACKS the iterations whose H-numerator product therefore ran on the
 *                            f16 W image instead;
 *   KLNMF_Q_RATIO_SATURATED  ratio-tile entries at the tiles' maximum (ratio >= 3584 / sqrt(2)): each is recomputed exactly and its excess
 *                            added to the H numerator; KLNMF_Q_RATIO_UNFIXED those beyond the correction list's capacity (8192 per
 *                            iteration) -- non-zero means H numerators of this loop were clipped; the loop then drops fp8 tiles */
#define KLNMF_Q_W8_SATURATED      5
#define KLNMF_Q_W8_FALLBACKS      6
#define KLNMF_Q_RATIO_SATURATED   7
#define KLNMF_Q_RATIO_UNFIXED     8
/*   KLNMF_Q_NO_NUM_EPS       1 if that loop's update passes on fp8 tiles formed the ratio as x / (W.H + eps) instead of the
 *                            reference's (x + eps) / (W.H + eps) (nmf.py:332-336): taken at the loop's entry where eps / mean(V)
 *                            <= 1e-5 (k <= 224), V keeps true zeros (2^-100 addend in the ratio), the loss corrected exactly; KLNMF_NE=0 turns it off */
#define KLNMF_Q_NO_NUM_EPS        9
/* The fp8 monitor of the last loop (csrc/monitor.hip.h): on the loop's first iteration (a dry run, before any fp8 tile is
 * taken), on fp8 iterations 1, 2, 4, 8, 16 and every 32nd after them the library recomputes, for one column tile and a sample
 * of rows, the H numerator (nmf.py:349) the 16-bit ratio tiles would have given and compares it with what the fp8 regime
 * produced -- a measured bound on the noise the (unbiased) e4m3 rounding puts into this data's numerator.
 *   KLNMF_Q_MON_CHECKS       monitored iterations;  KLNMF_Q_MON_TRIPS  component rows whose statistic exceeded the threshold;
 *   KLNMF_Q_MON_GAVE_UP      1 if the loop therefore (or after bulk saturation) continued on 16-bit tiles;
 *   klnmf_query_f64: KLNMF_QF_MON_STAT the largest statistic of the loop (estimated relative error of a numerator entry),
 *                    KLNMF_QF_MON_THRESHOLD the threshold it is compared with */
#define KLNMF_Q_MON_CHECKS        10
#define KLNMF_Q_MON_TRIPS         11
#define KLNMF_Q_MON_GAVE_UP       12
/*   KLNMF_Q_FP8_POLL_DUE     loops sequenced in pieces on row shards (klnmf_iter_*): 1 if the klnmf_iter_advance that follows the
 *                            column pass just enqueued reads the all-reduced count in loss[1] (monitor trips + unfixable ratio entries,
 *                            written by that column pass's last launch).  The caller then all-reduces loss[1] BEHIND
 *                            klnmf_iter_colpass and before klnmf_iter_advance; loss[0] alone may be exchanged earlier, while the
 *                            column pass computes.  The loop state behind the answer is the same on every rank. */
#define KLNMF_Q_FP8_POLL_DUE      13
/* The CSR kernels a problem given by klnmf_set_problem_sparse runs on (csrc/sparseb.hip.h):
 *   KLNMF_Q_SP_COL_BLOCKS    column blocks of the fused ratio / W-rule pass;  KLNMF_Q_SP_ROW_BLOCKS  row blocks of the
 *                            H-numerator pass.  0 (both): the unblocked kernels (k > 512, or no stored entries), or the
 *                            problem is dense */
#define KLNMF_Q_SP_COL_BLOCKS     14
#define KLNMF_Q_SP_ROW_BLOCKS     15
/* The dense kernel routes a problem given by klnmf_set_problem runs on in KLNMF_PREC_F64 / F32 / BF16X3 / F16X3 (csrc/exact.hip.h;
 * 0 for a 16-bit-mode problem, a CSR problem or no problem):
 *   KLNMF_Q_EX_ROW_CHUNKS    row chunks of the H numerator W^T.Q (its slabs);  KLNMF_Q_EX_W_CHUNKS  feature chunks of the W rule's
 *                            Q.H^T (1: one piece);  KLNMF_Q_EX_H_SEGMENTS  segments per dictionary row of the H rule (1: one block
 *                            per row);  KLNMF_Q_EX_H_FROM_SLABS  1: a single-context klnmf_run applies the H rule straight from the
 *                            row chunks' slabs (k_update_H_slabs), 0: from their sum (the step API and the loop in pieces always) */
#define KLNMF_Q_EX_ROW_CHUNKS     16
#define KLNMF_Q_EX_W_CHUNKS       17
#define KLNMF_Q_EX_H_SEGMENTS     18
#define KLNMF_Q_EX_H_FROM_SLABS   19
/*   KLNMF_Q_WEIGHTED         1 if the current problem holds weights (klnmf_upload_weights), 0 otherwise or with no problem */
#define KLNMF_Q_WEIGHTED          20
/*   KLNMF_Q_PRESENCE         modalities of the current problem's presence mask (klnmf_upload_presence), 0 without one or with no problem */
#define KLNMF_Q_PRESENCE          21
int klnmf_query(klnmf_ctx *ctx, int what, int64_t *value);
/* The launch plan of a problem without a context or a device (replaces nothing of the reference): what klnmf_query would answer
 * right after klnmf_set_problem(n, f, k) -- with nnz >= 0 after klnmf_set_problem_sparse(n, f, k, nnz) -- on a context of `precision`
 * whose device has `cu_count` compute units, for the items of the plan: KLNMF_Q_RATIO_TILE_BYTES, KLNMF_Q_SP_COL_BLOCKS / _ROW_BLOCKS,
 * KLNMF_Q_EX_ROW_CHUNKS / _W_CHUNKS / _H_SEGMENTS / _H_FROM_SLABS.  Returns the refusal where that call would refuse the shape.  It
 * reads the development switches as that call does, makes no HIP call, and runs on a machine without a GPU. */
int klnmf_plan_query(int precision, int64_t n, int64_t f, int64_t k, int64_t nnz, int cu_count, int what, int64_t *value);
/*   KLNMF_QF_SUM_V  the sum of the uploaded V as stored (16-bit modes; 0 in the exact modes), in the data's own units */
#define KLNMF_QF_SUM_V            0
/*   KLNMF_QF_NNZ_V  how many entries of the uploaded V are > 0 as stored (16-bit modes) */
#define KLNMF_QF_NNZ_V            1
#define KLNMF_QF_MON_STAT         2
#define KLNMF_QF_MON_THRESHOLD    3
/*   KLNMF_QF_MON_PART0 + 0 / 1 / 2: the statistic's ingredients, largest of the loop each (diagnostics: uncentred bias, noise
 *   term scaled to the full row count, |common factor of a component row over the monitored tile|) */
#define KLNMF_QF_MON_PART0        4
/*   KLNMF_QF_MON_SPREAD the smallest relative spread std(q) / mean(q) of a monitored column's ratios in the loop (the e4m3
 *   rounding only averages out over the rows if the ratios are spread over its cells), KLNMF_QF_MON_MIN_SPREAD its threshold */
#define KLNMF_QF_MON_SPREAD       7
#define KLNMF_QF_MON_MIN_SPREAD   8
/*   KLNMF_QF_KL_OVER_SUM_V  the last loop's final recorded loss over the sum of V (all shards), 16-bit modes; -1: none.  Below
 *   about 2e-3 the f16 operands' own rounding noise can exceed 1e-4 of the loss (nmf.py:214 has no
 *   counterpart: the reference has one arithmetic) -- the host layer says so once on stderr */
#define KLNMF_QF_KL_OVER_SUM_V    9
int klnmf_query_f64(klnmf_ctx *ctx, int what, double *value);

/* ---- measurement -------------------------------------------------------- */
/* When enabled, row-pass / column-pass launches are bracketed by HIP events on the context's stream: on = 1 every
 * iteration's, on = N > 1 those of every N-th iteration of a loop (an event record is a stream packet of its own, about
 * 5 us of dispatch gap: four per fit iteration are 3.5 % of a 0.65 ms iteration, so a measurement that must not
 * disturb what it times samples).  klnmf_profile_read returns the bracketed launches' count and summed milliseconds
 * since the last reset (synchronises). */
int klnmf_profile_enable(klnmf_ctx *ctx, int on);
int klnmf_profile_read(klnmf_ctx *ctx, int64_t *rowpass_launches,
                       double *rowpass_ms, int64_t *colpass_launches,
                       double *colpass_ms, int reset);
/* The part of the row-pass time klnmf_profile_read reports that the column-split last partial round of workgroups and its
 * slab W rule took (hybrid update pass: DESIGN.md section 4.1), the launches it was measured over and the (padded) rows
 * that part covers; 0 launches when the context runs whole rows everywhere. */
int klnmf_profile_read_tail(klnmf_ctx *ctx, int64_t *tail_n, double *tail_ms, int64_t *tail_rows, int reset);
int klnmf_synchronize(klnmf_ctx *ctx);

/* ---- CSR input (next-row N3): the reference's sparse branch ----------------------------------- */
/* With scipy-sparse X the reference evaluates W.H and the ratio only on the stored entries of X
 * (nmf.py:52-70, 301-308, 331-334).  Exact modes only.  klnmf_set_problem_sparse replaces
 * klnmf_set_problem; klnmf_upload_csr takes X in CSR (indptr[n+1], indices[nnz], data[nnz]; no explicit
 * zeros, `eliminate_zeros` of nmf.py:66) and the same entries in CSC order (csc_indptr[f+1], csc_rows[nnz],
 * csc_perm[nnz] = position of the entry in the CSR arrays).  Every loop / step / error entry point then
 * works on the stored entries; klnmf_get_Q_values returns the ratio in CSR order (the data of the sparse
 * matrix `_Q` returns, nmf.py:333-334). */
int klnmf_set_problem_sparse(klnmf_ctx *ctx, int64_t n, int64_t f, int64_t k, int64_t max_iter_capacity, int64_t nnz);
int klnmf_upload_csr(klnmf_ctx *ctx, int dtype, const int64_t *indptr, const int64_t *indices, const void *data,
                     const int64_t *csc_indptr, const int64_t *csc_rows, const int64_t *csc_perm);
/* klnmf_upload_csr_rows  X in CSR only (indptr[n+1], indices[nnz], data[nnz]); the library builds the CSC order on the device
 * (csrc/csc.hip.h: a stable radix sort of the entries by column), bit for bit what klnmf_upload_csr is given by a caller that
 * sorts on the host (np.argsort(indices, kind='stable')).  It replaces the host side of nmf.py:52-70 and 331-351 -- the
 * transposed access to X's structure that `_special_sparse_dot` and the H rule's W^T.Q need.  The structure is checked on the
 * device first: row pointers that decrease, a column index outside [0, f) or indices of a row that are not sorted are refused
 * (KLNMF_ERR_ARG) before anything is reordered, and leave the problem with no stored entry until the next upload. */
int klnmf_upload_csr_rows(klnmf_ctx *ctx, int dtype, const int64_t *indptr, const int64_t *indices, const void *data);
int klnmf_get_Q_values(klnmf_ctx *ctx, void *dst, int dtype);
/* klnmf_upload_csr_device_rows  X = hstack([scale[m] * X_m[rows] for m in 0 .. n_mod)]) in CSR, gathered ON THE DEVICE from
 * device-resident CSR modalities: replaces the per-run host slices `x[train, :]` / `x[test, :]` of experiment.py:163-164 and the
 * sparse stack of learner.py:53-56 (`safe_hstack` keeps the stack sparse if any block is) for data that stays on the GPU across
 * runs; nothing of nnz length is sliced on the host or crosses the bus.  Called on a problem set by
 * klnmf_set_problem_sparse(n = rows, f, k, cap, nnz) with nnz the stored entries of the selected rows (the caller knows it from
 * the sources' row pointers).  Source m (device memory of the context's device): indptr[m] int64 [src_rows + 1], indices[m] INT32
 * [nnz_m] sorted within every row and in [0, col_bounds[m + 1] - col_bounds[m]) (a modality has fewer than 2^31 columns; half the
 * resident bytes of int64 -- the problem's own indices stay int64), data[m] [nnz_m] float32 / float64 (dtype[m] = KLNMF_DT_*), no
 * explicit zeros.  col_bounds has n_mod + 1 entries, 0 = b_0 <= b_1 <= ... <= b_M = f: modality m takes the columns
 * [b_m, b_(m+1)), 1 <= n_mod <= KLNMF_MAX_MODALITIES.  drow_idx: `rows` int64 row indices in device memory, any order, repeats
 * allowed.  The product x * scale[m] is formed in the SOURCE's element type with scale[m] rounded to it (scipy's `csr * float(c)`),
 * then cast to the context's type: the problem is bit for bit the one klnmf_upload_csr_rows uploads from the host's slices.  The
 * caller keeps products that round to zero out (a scale of 0, or one that underflows the smallest stored value: the reference
 * drops such entries, nmf.py:66, and a device gather cannot after nnz is fixed).  Then the device tail of klnmf_upload_csr_rows
 * (structure check, CSC order).  KLNMF_ERR_ARG, the problem as it was: a dense problem, rows != n, n_mod out of range, a null
 * pointer, bounds that do not run from 0 to f or decrease, an unknown dtype.  KLNMF_ERR_ARG, the problem left with no stored
 * entry until the next upload (as a refused klnmf_upload_csr_rows leaves it): a row index outside [0, src_rows) -- found on the
 * device, reported through a flag, never dereferenced -- and a gathered total that differs from the problem's nnz (read back
 * with the flag, before anything is copied).  Synchronous. */
int klnmf_upload_csr_device_rows(klnmf_ctx *ctx, int n_mod, const int64_t *const *indptr, const int32_t *const *indices,
                                 const void *const *data, const int *dtype, const int64_t *col_bounds, const double *scale,
                                 int64_t src_rows, const int64_t *drow_idx, int64_t rows);
/* klnmf_csr_rows_to_dense_device  rows drow_idx[0 .. rows) of ONE device-resident CSR matrix (arrays as a source above, d columns)
 * as a dense float64 device matrix dout [rows, d], rows `ld` apart, zero where nothing is stored: the raw rows `x[test, :]` of a
 * sparse modality (experiment.py:163-164) that the evaluation compares reconstructions with (experiment.py:266), for
 * klnmf_all_distances_device; learner.py:53-56 has no part in it (no scale, no stacking).  A row index outside [0, src_rows)
 * leaves its row zero.  On `device`'s null stream, synchronous (the pattern of klnmf_matmul_device). */
int klnmf_csr_rows_to_dense_device(int device, int dtype, const int64_t *indptr, const int32_t *indices, const void *data,
                                   int64_t src_rows, const int64_t *drow_idx, int64_t rows, int64_t d, void *dout, int64_t ld);

/* ---- reconstruction (next-row K7) ---------------------------------------- */
/* C[m x n] = A[m x kk] . B[kk x n], row-major host arrays of `dtype`, computed on `device` in that
 * arithmetic.  Replaces `internal.dot(self.get_dico(dest_mod))` / `internal.dot(self.get_stacked_dicos(..))`
 * of MultimodalLearner.reconstruct_modality / reconstruct_modalities (learner.py:80-84). */
int klnmf_matmul(int device, int dtype, int64_t m, int64_t n, int64_t kk,
                 const void *A, const void *B, void *C);

/* ---- nearest-neighbour evaluation (next-row N4) ------------------------------------------------- */
/* out[na x nb] (row-major) = measure(A[i, :], B[j, :]) for all pairs; A [na x d], B [nb x d] row-major host
 * arrays of `dtype`.  Replaces `all_distances(reco_data, ex_data, measure)` (evaluation.py:103-106: a
 * [na,1,d] x [1,nb,d] broadcast of one of the measures of metrics.py:58-86).  metric: 0 kl_div(a, b),
 * 1 rev_kl_div, 2 sym_kl_div, 3 frobenius, 4 cosine_diff; eps = 1e-8 (metrics.py:15). */
#define KLNMF_DIST_KL 0
#define KLNMF_DIST_REV_KL 1
#define KLNMF_DIST_SYM_KL 2
#define KLNMF_DIST_FROBENIUS 3
#define KLNMF_DIST_COSINE_DIFF 4
int klnmf_all_distances(int device, int dtype, int metric, int64_t na, int64_t nb, int64_t d,
                        const void *A, const void *B, void *out);

/* ---- hardware probes (tests) -------------------------------------------- */
/* Runs the MFMA / LDS-transpose layout self-checks the fused kernels rely on;
 * *failed = bitmask of failing probes (0 = all good). */
int klnmf_selftest(int device, int *failed);

#ifdef __cplusplus
}
#endif
#endif /* KLNMF_H */
