// libklnmf.so, unit 6 of 6: klnmf_batch_* -- B dense problems of one shape in KLNMF_PREC_F64 / F32, unweighted or (all of them)
// under row x modality presence masks (klnmf_batch_mask.h), that run the loop of nmf.py:212-222 together, one launch per stage
// for all of them (batch.hip.h has the kernels and the layout; ctx.hip.h lists the other units).  The plan is the single problem's (plan_dense_exact) for max(1, cu_count / B) compute units; the launch
// sequence of an iteration is local_iteration's for a dense unweighted problem of the exact modes (api_loop.hip: exact_Q, exact_W,
// exact_N, exact_H), stage for stage -- with a mask: for a dense masked problem (presence_S in front of the W rule, presence_D in
// front of the H numerator).
// A CSR batch (klnmf_batch_csr.h; batch_sparse.hip.h has the kernels and the layout): B unweighted CSR problems of one shape, each
// with its own stored entries, on the blocked sparse kernels; the plan is plan_csr's for the batch's mean entries per problem, the
// launch sequence local_iteration's for a blocked CSR problem (sparse_Q, the blocked arms of exact_W and exact_N, exact_H).
// A beta batch (klnmf_batch_beta.h): B dense problems under one beta != 1, weighted where klnmf_batch_upload_weights placed an Om;
// the launch sequence is local_iteration's for a beta context (beta_ratio with the loss, the beta arm of exact_W, beta_ratio without
// the loss, the dual arm of exact_N, the beta arm of exact_H with its column scale of W), stage for stage.
#include "ctx.hip.h"
#include "../../include/klnmf_batch.h"
#include "../../include/klnmf_batch_mask.h"
#include "../../include/klnmf_batch_csr.h"
#include "../../include/klnmf_batch_beta.h"
#include "batch.hip.h"

struct klnmf_batch : DeviceBlocks, PresenceState {
    int prec = KLNMF_PREC_F64, cu_count = 256, count = 1;
    // ---- the current problem
    bool have_problem = false;
    ProblemPlan plan;
    int64_t n = 0, f = 0, k = 0, cap = 0;
    int cur = 0;                                        // index of the W buffer every problem's current W is in (outside a loop)
    std::vector<char> has_V, has_H;
    std::vector<DevState> last;                         // the last loop's DevStates as klnmf_batch_run read them
    DevState *st = nullptr, *st_init = nullptr;         // [B]; st_init: the state every loop starts from
    double *errors = nullptr, *loss_xchg = nullptr, *loss_part = nullptr, *hpart = nullptr;
    void *V = nullptr, *Q = nullptr, *W[2] = {nullptr, nullptr}, *H = nullptr, *Npart = nullptr, *numer = nullptr, *Wpart = nullptr;
    // ---- a CSR batch (sparse): per problem H^T, the block pointers, the slabs G / NT and the loss term's sums; per entry the
    // problems' arrays one behind another, problem p's at off[p]; and the arrays ONE upload works in (u_*: a problem's own positions)
    bool sparse = false;
    std::vector<int64_t> nnz, off;                      // [B], [B + 1]
    void *HT = nullptr, *sp_data = nullptr, *sp_q = nullptr, *sp_G = nullptr, *sp_NT = nullptr;
    int *sp_idx32 = nullptr, *csc_rows32 = nullptr, *csc_perm32 = nullptr, *sp_bad = nullptr;
    int64_t *sp_blkptr = nullptr, *csc_blkptr = nullptr;
    double *sp_loss_part = nullptr, *sp_wpart = nullptr, *sp_prod = nullptr;
    int64_t *u_indptr = nullptr, *u_indices = nullptr, *u_csc_indptr = nullptr, *u_csc_rows = nullptr, *u_csc_perm = nullptr, *u_work = nullptr;
    // (a masked batch: PresenceState, every problem's P, S, D and D's slabs and once per batch the bounds and the modality bytes --
    // taken by the first klnmf_batch_upload_presence*, dropped by klnmf_batch_clear_presence and with the problem)
    // ---- a beta batch (klnmf_batch_beta.h; beta != 1): B [B][n][f] beside Q (= A), the denominators' slab sets and sums beside
    // the numerators', the rows' sums of the H rule in hpart ([B][k] where the plan holds no segments: own_hpart) -- taken by
    // klnmf_batch_set_divergence; Om [B][n][f] by the first klnmf_batch_upload_weights.  All go with the problem and at beta = 1
    double beta = 1.0;
    bool own_hpart = false;
    void *Bt = nullptr, *Om = nullptr, *Dpart = nullptr, *denom = nullptr, *WDpart = nullptr;

    size_t esize() const { return prec_esize(prec); }
    MaskDims mask_dims() const { return {n, f, k, count, prec}; }
    bool beta_on() const { return beta != 1.0; }
    double beta_gamma() const { return beta < 1.0 ? 1.0 / (2.0 - beta) : (beta <= 2.0 ? 1.0 : 1.0 / (beta - 1.0)); }
    void forget_beta() {      // (the blocks are released, or about to be)
        beta = 1.0;
        own_hpart = false;
        Bt = Om = Dpart = denom = WDpart = nullptr;
    }
    void free_all() {      // (callers have synchronised the stream)
        release_all();
        forget_presence();
        forget_beta();
        have_problem = false;
        sparse = false;
    }
};

namespace {

void use(klnmf_batch *b) {
    if (!b) fail(KLNMF_ERR_ARG, "null batch");
    HIPCHK(hipSetDevice(b->device));
}
void need_problem(klnmf_batch *b) {
    use(b);
    if (!b->have_problem) fail(KLNMF_ERR_ARG, "klnmf_batch_set_problem has not been called");
}
void need_p(klnmf_batch *b, int p) {
    need_problem(b);
    if (p < 0 || p >= b->count) fail(KLNMF_ERR_ARG, "problem index " + std::to_string(p) + " outside the batch of " + std::to_string(b->count));
}

// fn<T>(b, ...) in the batch's element type
#define BATCH_CALL(b, fn, ...)                                         \
    do {                                                               \
        if ((b)->prec == KLNMF_PREC_F64) fn<double>(b, ##__VA_ARGS__); \
        else fn<float>(b, ##__VA_ARGS__);                              \
    } while (0)

// a host matrix [rows, cols] into a device matrix of the batch's type, and back (klnmf_set_H / klnmf_get_W of a context)
void set_matrix(klnmf_batch *b, void *dst, const void *src, int dtype, int64_t rows, int64_t cols) {
    const size_t bytes = (size_t)rows * cols * (dtype == KLNMF_DT_F64 ? 8 : 4);
    void *d = nullptr;
    HIPCHK(hipMalloc(&d, bytes ? bytes : 16));
    try {
        HIPCHK(hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, b->stream));
        copy_2d_any(b->stream, dst, b->prec == KLNMF_PREC_F64, cols, d, dtype == KLNMF_DT_F64, cols, rows, cols);
        HIPCHK(hipStreamSynchronize(b->stream));
    } catch (...) {
        (void)hipFree(d);
        throw;
    }
    (void)hipFree(d);
}
void get_matrix(klnmf_batch *b, void *dst, int dtype, const void *src, int64_t rows, int64_t cols) {
    const size_t bytes = (size_t)rows * cols * (dtype == KLNMF_DT_F64 ? 8 : 4);
    void *d = nullptr;
    HIPCHK(hipMalloc(&d, bytes ? bytes : 16));
    try {
        copy_2d_any(b->stream, d, dtype == KLNMF_DT_F64, cols, src, b->prec == KLNMF_PREC_F64, cols, rows, cols);
        HIPCHK(hipMemcpyAsync(dst, d, bytes, hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
    } catch (...) {
        (void)hipFree(d);
        throw;
    }
    (void)hipFree(d);
}

void *problem_ptr(const klnmf_batch *b, void *base, int p, int64_t elems) { return (char *)base + (size_t)p * elems * b->esize(); }

// V of problem p [row0 + i, col0 + j] = scale * src[row_idx ? row_idx[i] : i, j], src on the device
void place_block(klnmf_batch *b, int p, const void *dsrc, int dtype, const int64_t *row_idx, int64_t rows, int64_t cols, int64_t ld,
                 int64_t row0, int64_t col0, double scale) {
    if (rows * cols == 0) return;
    place_rows(b->stream, problem_ptr(b, b->V, p, b->n * b->f), b->prec == KLNMF_PREC_F64, b->f, dsrc, dtype == KLNMF_DT_F64, rows, cols, ld,
               row0, col0, scale, row_idx);
    b->has_V[(size_t)p] = 1;
}

void reset_states(klnmf_batch *b) {
    HIPCHK(hipMemcpyAsync(b->st, b->st_init, sizeof(DevState) * (size_t)b->count, hipMemcpyDeviceToDevice, b->stream));
}

// ---- the stages of an iteration: api_loop.hip's exact_Q / exact_W / exact_N / exact_H for B problems ----------------------------
template <typename T>
void batch_Q(klnmf_batch *b, int decide, double tol_abs) {
    const ProblemPlan &pl = b->plan;
    const int ytiles = (int)((b->n + GT - 1) / GT);
    const dim3 grid((unsigned)((b->f + GT - 1) / GT), (unsigned)(b->count * ytiles), 1);
#define KL_BQ_ARGS (int)b->n, (int)b->f, (int)b->k, (const T *)b->W[b->cur], (int64_t)b->k, (int64_t)1, b->n * b->k, (const T *)b->H, \
                   (int64_t)b->f, (int64_t)1, b->k * b->f, (int)b->k + GK, (const DevState *)b->st, ytiles
    if (b->presence()) {
        typedef EpiQ<T, PresenceWeight<T>> Epi;
        hipLaunchKernelGGL((k_gemm_batch<T, Epi>), grid, dim3(256), 0, b->stream, KL_BQ_ARGS,
                           Epi{(const T *)b->V, {(const T *)b->Pm, (const unsigned char *)b->pres_mod, b->pres_M}, (T *)b->Q, b->f,
                               b->loss_part, 1, 0.0, (T)kEpsRatio});
    } else {
        hipLaunchKernelGGL((k_gemm_batch<T, EpiQ<T>>), grid, dim3(256), 0, b->stream, KL_BQ_ARGS,
                           EpiQ<T>{(const T *)b->V, {}, (T *)b->Q, b->f, b->loss_part, 1, 0.0, (T)kEpsRatio});
    }
#undef KL_BQ_ARGS
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_sum_doubles_batch, dim3((unsigned)b->count), dim3(1024), 0, b->stream, (const double *)b->loss_part,
                       pl.loss_part_count, b->loss_xchg, b->st, decide, tol_abs, b->errors, b->cap);
    HIPCHK(hipGetLastError());
}

// S of every problem's masked W rule, from its current H (presence_S of api_loop.hip)
template <typename T>
void batch_presence_S(klnmf_batch *b) {
    hipLaunchKernelGGL((k_presence_S_batch<T>), dim3((unsigned)b->k, (unsigned)b->pres_M, (unsigned)b->count), dim3(256), 0, b->stream,
                       (const T *)b->H, (const int64_t *)b->pres_dbounds, (T *)b->pres_S, b->f, b->k, (const DevState *)b->st);
    HIPCHK(hipGetLastError());
}

// D = W[widx]^T.P of every problem: the row chunks' slabs in double, then their fixed-order sum (presence_D of api_loop.hip)
template <typename T>
void batch_presence_D(klnmf_batch *b, int widx) {
    const int64_t chunk = (b->n + b->pres_dchunks - 1) / b->pres_dchunks;
    hipLaunchKernelGGL((k_presence_D_part_batch<T>), dim3((unsigned)((b->k + 63) / 64), (unsigned)b->pres_dchunks, (unsigned)b->count),
                       dim3(256), 0, b->stream, (const T *)b->W[widx], (const T *)b->Pm, (double *)b->pres_Dslab, b->n, b->k, b->pres_M,
                       chunk, (const DevState *)b->st);
    HIPCHK(hipGetLastError());
    const int64_t count = b->k * b->pres_M;
    hipLaunchKernelGGL((k_presence_D_sum_batch<T>), dim3(grid_for(count), (unsigned)b->count), dim3(256), 0, b->stream,
                       (const double *)b->pres_Dslab, b->pres_dchunks, count, (T *)b->pres_D, (const DevState *)b->st);
    HIPCHK(hipGetLastError());
}

// W_new = W * factor under the policy `fac`: the whole contraction with the rule in its epilogue, or over feature chunks and the
// rule from their slabs
template <typename T, typename Fac>
void batch_W_rule(klnmf_batch *b, const void *qsrc, Fac fac) {
    const ProblemPlan &pl = b->plan;
    const bool split = pl.wsplit > 1;
    const int ytiles = (int)((b->n + GT - 1) / GT);
    const dim3 grid((unsigned)((b->k + GT - 1) / GT), (unsigned)(b->count * ytiles), (unsigned)(split ? pl.wsplit : 1));
    const int chunk = split ? pl.wchunk : (int)b->f + GK;
    const int64_t count = b->n * b->k;
    const EpiW<T, Fac> epi{(const T *)b->W[b->cur], (T *)b->W[b->cur ^ 1], b->k, fac};
#define KL_BW_ARGS (int)b->n, (int)b->k, (int)b->f, (const T *)qsrc, (int64_t)b->f, (int64_t)1, b->n * b->f, (const T *)b->H, (int64_t)1, \
                   (int64_t)b->f, b->k * b->f, chunk, (const DevState *)b->st, ytiles
    if (!split) {
        hipLaunchKernelGGL((k_gemm_batch<T, EpiW<T, Fac>>), grid, dim3(256), 0, b->stream, KL_BW_ARGS, epi);
        HIPCHK(hipGetLastError());
        return;
    }
    hipLaunchKernelGGL((k_gemm_batch<T, EpiWpart<T, 1>>), grid, dim3(256), 0, b->stream, KL_BW_ARGS, EpiWpart<T, 1>{{(T *)b->Wpart}, b->k, count});
#undef KL_BW_ARGS
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL((k_wrule_batch<T, Fac>), dim3(grid_for(count), (unsigned)b->count), dim3(256), 0, b->stream,
                       NumSlabs<T, 1>{{{(const T *)b->Wpart}}, pl.wsplit, count}, (const DevState *)b->st, epi);
    HIPCHK(hipGetLastError());
}

// W_new = W * (Qsrc . H^T)   (multiply = 0: W_new = Qsrc . H^T, W0 with Qsrc = V -- unweighted under a mask too, as in a context)
template <typename T>
void batch_W(klnmf_batch *b, const void *qsrc, int multiply) {
    if (b->presence() && multiply) {
        batch_presence_S<T>(b);
        batch_W_rule<T>(b, qsrc, FacPresW<T>{(const T *)b->Pm, (const T *)b->pres_S, b->k, b->pres_M});
    } else {
        batch_W_rule<T>(b, qsrc, FacW0{{}, multiply});
    }
}

// the H numerator's slabs from W[widx]^T . Q per row chunk (sum_slabs: and their sum)
template <typename T>
void batch_N(klnmf_batch *b, int widx, bool sum_slabs) {
    const ProblemPlan &pl = b->plan;
    if (b->presence()) batch_presence_D<T>(b, widx);      // (the numerator below is the unweighted one, on R)
    const int ytiles = (int)((b->k + GT - 1) / GT);
    const dim3 grid((unsigned)((b->f + GT - 1) / GT), (unsigned)(b->count * ytiles), (unsigned)pl.nsplit);
    const int64_t count = b->k * b->f;
    hipLaunchKernelGGL((k_gemm_batch<T, EpiN<T, 1>>), grid, dim3(256), 0, b->stream, (int)b->k, (int)b->f, (int)b->n,
                       (const T *)b->W[widx], (int64_t)1, (int64_t)b->k, b->n * b->k, (const T *)b->Q, (int64_t)b->f, (int64_t)1,
                       b->n * b->f, pl.kchunk, (const DevState *)b->st, ytiles, EpiN<T, 1>{{(T *)b->Npart}, b->f, count});
    HIPCHK(hipGetLastError());
    if (!sum_slabs) return;
    hipLaunchKernelGGL((k_sum_partials_batch<T>), dim3(grid_for(count), (unsigned)b->count), dim3(256), 0, b->stream,
                       NumArray<T, 1>{{(const T *)b->Npart}}, (T *)b->numer, count, pl.nsplit, (const DevState *)b->st);
    HIPCHK(hipGetLastError());
}

template <typename T, typename Fac>
void batch_H_rule(klnmf_batch *b, bool from_slabs, Fac fac) {
    const ProblemPlan &pl = b->plan;
    typedef NumArray<T, 1> Arr;
    typedef NumSlabs<T, 1> Slabs;
    const Arr sums{{(const T *)b->numer}}, slab0{{(const T *)b->Npart}};
    const dim3 rows((unsigned)b->k, (unsigned)b->count), segs((unsigned)pl.hseg_n, (unsigned)b->k, (unsigned)b->count);
    if (from_slabs) {
        hipLaunchKernelGGL((k_update_H_batch<T, Slabs, Fac>), rows, dim3(256), 0, b->stream, (T *)b->H,
                           RuleIn<Slabs, Fac>{Slabs{slab0, pl.nsplit, b->k * b->f}, fac}, b->f, (const DevState *)b->st);
    } else if (pl.hseg_n > 1) {
        hipLaunchKernelGGL((k_update_H_part_batch<T, Fac>), segs, dim3(256), 0, b->stream, (T *)b->H, RuleIn<Arr, Fac>{sums, fac},
                           b->f, pl.hseg, b->hpart, (const DevState *)b->st);
        hipLaunchKernelGGL((k_update_H_norm_batch<T>), segs, dim3(256), 0, b->stream, (T *)b->H, b->f, pl.hseg,
                           (const double *)b->hpart, (const DevState *)b->st);
    } else {
        hipLaunchKernelGGL((k_update_H_batch<T, Arr, Fac>), rows, dim3(256), 0, b->stream, (T *)b->H, RuleIn<Arr, Fac>{sums, fac},
                           b->f, (const DevState *)b->st);
    }
    HIPCHK(hipGetLastError());
}

template <typename T>
void batch_H(klnmf_batch *b, bool from_slabs) {
    if (b->presence()) batch_H_rule<T>(b, from_slabs, FacPresH<T>{(const T *)b->pres_D, (const unsigned char *)b->pres_mod, b->pres_M});
    else batch_H_rule<T>(b, from_slabs, FacNum{});
}

// ---- a beta batch's stages: api_loop.hip's beta_AB and the beta arms of exact_W / exact_N / exact_H for B problems ----------------
// A = Om o x o y^(beta-2) into Q and B = Om o y^(beta-1) into Bt at (W[widx], H) of every problem; `loss`: the cost's partials, their
// per-problem sum and the stop rule
template <typename T>
void beta_AB(klnmf_batch *b, int widx, bool loss, double tol_abs) {
    const ProblemPlan &pl = b->plan;
    const int ytiles = (int)((b->n + GT - 1) / GT);
    const dim3 grid((unsigned)((b->f + GT - 1) / GT), (unsigned)(b->count * ytiles), 1);
    auto launch = [&](auto epi) {
        typedef decltype(epi) Epi;
        hipLaunchKernelGGL((k_gemm_batch<T, Epi>), grid, dim3(256), 0, b->stream, (int)b->n, (int)b->f, (int)b->k, (const T *)b->W[widx],
                           (int64_t)b->k, (int64_t)1, b->n * b->k, (const T *)b->H, (int64_t)b->f, (int64_t)1, b->k * b->f, (int)b->k + GK,
                           (const DevState *)b->st, ytiles, epi);
    };
    auto with_kind = [&](auto weight, auto with_loss) {
        typedef decltype(weight) Weight;
        constexpr bool L = decltype(with_loss)::value;
#define KL_BETA_EPI(KIND) launch(EpiBeta<T, Weight, L, KIND>{(const T *)b->V, weight, (T *)b->Q, (T *)b->Bt, b->f, b->loss_part, 0.0, \
                                                              (T)kEpsRatio, (T)b->beta})
        if (b->beta == 2.0) KL_BETA_EPI(BETA_TWO);
        else if (b->beta == 0.0) KL_BETA_EPI(BETA_ZERO);
        else KL_BETA_EPI(BETA_GEN);
#undef KL_BETA_EPI
    };
    auto with_weight = [&](auto with_loss) {
        if (b->Om) with_kind(ElemWeight<T>{(const T *)b->Om}, with_loss);
        else with_kind(NoWeight{}, with_loss);
    };
    if (loss) with_weight(std::true_type{}); else with_weight(std::false_type{});
    HIPCHK(hipGetLastError());
    if (!loss) return;
    hipLaunchKernelGGL(k_sum_doubles_batch, dim3((unsigned)b->count), dim3(1024), 0, b->stream, (const double *)b->loss_part,
                       pl.loss_part_count, b->loss_xchg, b->st, 1, tol_abs, b->errors, b->cap);
    HIPCHK(hipGetLastError());
}

// W_new = W * ((A.H^T) / (B.H^T))^gamma: form A of k_gemm_dual_batch (the tile of H^T shared) with the rule in its epilogue, or over
// feature chunks into two slab sets and the rule from them
template <typename T>
void beta_W(klnmf_batch *b) {
    const ProblemPlan &pl = b->plan;
    typedef FacBeta<T> Fac;
    const bool split = pl.wsplit > 1;
    const int ytiles = (int)((b->n + GT - 1) / GT);
    const dim3 grid((unsigned)((b->k + GT - 1) / GT), (unsigned)(b->count * ytiles), (unsigned)(split ? pl.wsplit : 1));
    const int chunk = split ? pl.wchunk : (int)b->f + GK;
    const int64_t count = b->n * b->k;
    const EpiW<T, Fac> epi{(const T *)b->W[b->cur], (T *)b->W[b->cur ^ 1], b->k, Fac{(T)b->beta_gamma()}};
#define KL_BBW_ARGS (int)b->n, (int)b->k, (int)b->f, (const T *)b->Q, (int64_t)b->f, (int64_t)1, b->n * b->f, (const T *)b->H, (int64_t)1, \
                    (int64_t)b->f, b->k * b->f, (const T *)b->Bt, b->n * b->f, chunk, (const DevState *)b->st, ytiles
    if (!split) {
        hipLaunchKernelGGL((k_gemm_dual_batch<T, EpiW<T, Fac>, true>), grid, dim3(256), 0, b->stream, KL_BBW_ARGS, epi);
        HIPCHK(hipGetLastError());
        return;
    }
    hipLaunchKernelGGL((k_gemm_dual_batch<T, EpiWpart<T, 2>, true>), grid, dim3(256), 0, b->stream, KL_BBW_ARGS,
                       EpiWpart<T, 2>{{(T *)b->Wpart, (T *)b->WDpart}, b->k, count});
#undef KL_BBW_ARGS
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL((k_wrule_batch<T, Fac>), dim3(grid_for(count), (unsigned)b->count), dim3(256), 0, b->stream,
                       NumSlabs<T, 2>{{{(const T *)b->Wpart, (const T *)b->WDpart}}, pl.wsplit, count}, (const DevState *)b->st, epi);
    HIPCHK(hipGetLastError());
}

// the H numerator's and denominator's slabs (W[widx]^T.A, W[widx]^T.B) per row chunk: form B of k_gemm_dual_batch (the tile of
// W^T shared); sum_slabs: and their sums
template <typename T>
void beta_N(klnmf_batch *b, int widx, bool sum_slabs) {
    const ProblemPlan &pl = b->plan;
    const int ytiles = (int)((b->k + GT - 1) / GT);
    const dim3 grid((unsigned)((b->f + GT - 1) / GT), (unsigned)(b->count * ytiles), (unsigned)pl.nsplit);
    const int64_t count = b->k * b->f;
    hipLaunchKernelGGL((k_gemm_dual_batch<T, EpiN<T, 2>, false>), grid, dim3(256), 0, b->stream, (int)b->k, (int)b->f, (int)b->n,
                       (const T *)b->W[widx], (int64_t)1, (int64_t)b->k, b->n * b->k, (const T *)b->Q, (int64_t)b->f, (int64_t)1,
                       b->n * b->f, (const T *)b->Bt, b->n * b->f, pl.kchunk, (const DevState *)b->st, ytiles,
                       EpiN<T, 2>{{(T *)b->Npart, (T *)b->Dpart}, b->f, count});
    HIPCHK(hipGetLastError());
    if (!sum_slabs) return;
    hipLaunchKernelGGL((k_sum_partials_sets_batch<T, 2>), dim3(grid_for(count), (unsigned)b->count), dim3(256), 0, b->stream,
                       NumArray<T, 2>{{(const T *)b->Npart, (const T *)b->Dpart}}, OutSets<T, 2>{{(T *)b->numer, (T *)b->denom}}, count,
                       pl.nsplit, (const DevState *)b->st);
    HIPCHK(hipGetLastError());
}

// the H rule under FacBeta on its three routes, each leaving the rows' sums (one per segment) in hpart, and behind it the
// compensation W[widx][:, a] *= sum[a]
template <typename T>
void beta_H(klnmf_batch *b, bool from_slabs, int widx) {
    const ProblemPlan &pl = b->plan;
    typedef FacBeta<T> Fac;
    typedef NumArray<T, 2> Arr;
    typedef NumSlabs<T, 2> Slabs;
    const Fac fac{(T)b->beta_gamma()};
    const Arr sums{{(const T *)b->numer, (const T *)b->denom}}, slab0{{(const T *)b->Npart, (const T *)b->Dpart}};
    const dim3 rows((unsigned)b->k, (unsigned)b->count), segs((unsigned)pl.hseg_n, (unsigned)b->k, (unsigned)b->count);
    const int nseg = (!from_slabs && pl.hseg_n > 1) ? pl.hseg_n : 1;
    if (from_slabs) {
        hipLaunchKernelGGL((k_update_H_sums_batch<T, Slabs, Fac>), rows, dim3(256), 0, b->stream, (T *)b->H,
                           RuleIn<Slabs, Fac>{Slabs{slab0, pl.nsplit, b->k * b->f}, fac}, b->f, b->hpart, (const DevState *)b->st);
    } else if (nseg > 1) {
        hipLaunchKernelGGL((k_update_H_part_batch<T, Fac>), segs, dim3(256), 0, b->stream, (T *)b->H, RuleIn<Arr, Fac>{sums, fac}, b->f,
                           pl.hseg, b->hpart, (const DevState *)b->st);
        hipLaunchKernelGGL((k_update_H_norm_batch<T>), segs, dim3(256), 0, b->stream, (T *)b->H, b->f, pl.hseg, (const double *)b->hpart,
                           (const DevState *)b->st);
    } else {
        hipLaunchKernelGGL((k_update_H_sums_batch<T, Arr, Fac>), rows, dim3(256), 0, b->stream, (T *)b->H, RuleIn<Arr, Fac>{sums, fac},
                           b->f, b->hpart, (const DevState *)b->st);
    }
    HIPCHK(hipGetLastError());
    const int64_t count = b->n * b->k;
    hipLaunchKernelGGL((k_scale_W_cols_batch<T>), dim3(grid_for(count), (unsigned)b->count), dim3(256), 0, b->stream, (T *)b->W[widx], count,
                       b->k, (const double *)b->hpart, nseg, (const DevState *)b->st);
    HIPCHK(hipGetLastError());
}

// ---- a CSR batch's stages: api_loop.hip's sparse_Q and the blocked arms of exact_W / exact_N for B problems ----------------------
// k_spb_*<T, KC, ..>: KC = 1, 2, 4, 8 component chunks of 64 by k, as a context picks them
#define KL_BATCH_KC(b, LAUNCH)                                   \
    do {                                                         \
        const int kcb_ = (int)(((b)->k + 63) / 64);              \
        if (kcb_ <= 1) LAUNCH(1); else if (kcb_ == 2) LAUNCH(2); \
        else if (kcb_ <= 4) LAUNCH(4); else LAUNCH(8);           \
    } while (0)

template <typename T>
void csr_transpose_H(klnmf_batch *b) {
    hipLaunchKernelGGL((k_sp_transpose_H_batch<T>), dim3(grid_for(b->k * b->f), (unsigned)b->count), dim3(256), 0, b->stream,
                       (const T *)b->H, (T *)b->HT, b->k, b->f, (const DevState *)b->st);
    HIPCHK(hipGetLastError());
}

// the fused pass over the stored entries: SPB_UPDATE (ratio, loss partials, G) or SPB_INIT (G from the entries' values themselves)
template <typename T, int MODE>
void csr_qw(klnmf_batch *b) {
    const ProblemPlan &pl = b->plan;
    const dim3 grid((unsigned)((int64_t)pl.sp_cb * b->n), (unsigned)b->count);
#define KL_BQW(KCV) hipLaunchKernelGGL((k_spb_qw_batch<T, KCV, MODE>), grid, dim3(64), 0, b->stream, (const int64_t *)b->sp_blkptr,        \
        (const int *)b->sp_idx32, (const T *)b->sp_data, (const T *)b->W[b->cur], (const T *)b->HT, (T *)b->sp_q, b->sp_loss_part, (T *)b->sp_G, \
        b->n, b->k, b->f, pl.sp_cb, (T)(MODE == SPB_INIT ? 0.0 : kEpsRatio), (const DevState *)b->st)
    KL_BATCH_KC(b, KL_BQW);
#undef KL_BQW
    HIPCHK(hipGetLastError());
}

// ratio on the stored entries + loss + stop rule (sparse_Q)
template <typename T>
void csr_Q(klnmf_batch *b, int decide, double tol_abs) {
    const ProblemPlan &pl = b->plan;
    const unsigned B = (unsigned)b->count;
    csr_transpose_H<T>(b);
    csr_qw<T, SPB_UPDATE>(b);
    hipLaunchKernelGGL((k_sp_colsum_part_batch<T>), dim3((unsigned)pl.sp_nblk, B), dim3(256), 0, b->stream, (const T *)b->W[b->cur],
                       b->sp_wpart, b->n, b->k, (const DevState *)b->st);
    if (pl.hseg_n > 1)
        hipLaunchKernelGGL((k_sp_hsum_part_batch<T>), dim3((unsigned)pl.hseg_n, (unsigned)b->k, B), dim3(256), 0, b->stream, (const T *)b->H,
                           b->f, pl.hseg, b->hpart, (const DevState *)b->st);
    hipLaunchKernelGGL((k_sp_dots_batch<T>), dim3((unsigned)b->k, B), dim3(256), 0, b->stream, (const double *)b->sp_wpart, pl.sp_nblk,
                       (const T *)b->H, b->k, b->f, b->sp_prod, (const DevState *)b->st,
                       (const double *)(pl.hseg_n > 1 ? b->hpart : nullptr), pl.hseg_n > 1 ? pl.hseg_n : 0);
    hipLaunchKernelGGL(k_sp_loss_batch, dim3(B), dim3(1024), 0, b->stream, (const double *)b->sp_loss_part, (int64_t)pl.sp_cb * b->n,
                       (const double *)b->sp_prod, b->k, b->loss_xchg, b->st, decide, tol_abs, b->errors, b->cap);
    HIPCHK(hipGetLastError());
}

// W_new = (multiply ? W : 1) * sum over the column blocks' slabs G -- which csr_Q left (multiply), or the SPB_INIT pass fills here
template <typename T>
void csr_W(klnmf_batch *b, int multiply) {
    if (!multiply) csr_qw<T, SPB_INIT>(b);
    hipLaunchKernelGGL((k_spb_wrule_batch<T>), dim3(grid_for(b->n * b->k, 256, 8192), (unsigned)b->count), dim3(256), 0, b->stream,
                       (const T *)b->sp_G, b->plan.sp_cb, (const T *)b->W[b->cur], (T *)b->W[b->cur ^ 1], b->n, b->k, multiply,
                       (const DevState *)b->st);
    HIPCHK(hipGetLastError());
}

// numer = W[widx]^T . Q over the CSC order, row block by row block
template <typename T>
void csr_N(klnmf_batch *b, int widx) {
    const ProblemPlan &pl = b->plan;
    const dim3 grid((unsigned)((int64_t)pl.sp_rb * b->f), (unsigned)b->count);
#define KL_BN(KCV) hipLaunchKernelGGL((k_spb_n_batch<T, KCV>), grid, dim3(64), 0, b->stream, (const int64_t *)b->csc_blkptr, (const int *)b->csc_rows32, \
        (const int *)b->csc_perm32, (const T *)b->sp_q, (const T *)b->W[widx], (T *)b->sp_NT, b->n, b->k, b->f, pl.sp_rb, (const DevState *)b->st)
    KL_BATCH_KC(b, KL_BN);
#undef KL_BN
    hipLaunchKernelGGL((k_spb_numer_batch<T>), dim3((unsigned)((b->f + 31) / 32), (unsigned)((b->k + 31) / 32), (unsigned)b->count), dim3(256),
                       0, b->stream, (const T *)b->sp_NT, pl.sp_rb, (T *)b->numer, b->k, b->f, (const DevState *)b->st);
    HIPCHK(hipGetLastError());
}

// one iteration for every problem (local_iteration of api_loop.hip): ratio + loss, stop rule, W rule, and in a fit the H rule;
// masked: Q, then S and the W rule, and in a fit D, N and the H rule
void batch_iteration(klnmf_batch *b, int fit, double tol_abs) {
    if (b->sparse) {
        BATCH_CALL(b, csr_Q, 1, tol_abs);
        BATCH_CALL(b, csr_W, 1);
        if (fit) {
            BATCH_CALL(b, csr_N, b->cur ^ 1);
            BATCH_CALL(b, batch_H, false);
        }
        b->cur ^= 1;
        return;
    }
    if (b->beta_on()) {      // the beta cost: A, B and the loss at (W, H), the W rule from them; a fit: A, B at (W_new, H), the H rule
        BATCH_CALL(b, beta_AB, b->cur, true, tol_abs);
        BATCH_CALL(b, beta_W);
        if (fit) {
            const bool slabs = h_from_slabs(&b->plan);
            BATCH_CALL(b, beta_AB, b->cur ^ 1, false, 0.0);
            BATCH_CALL(b, beta_N, b->cur ^ 1, !slabs);
            BATCH_CALL(b, beta_H, slabs, b->cur ^ 1);
        }
        b->cur ^= 1;
        return;
    }
    BATCH_CALL(b, batch_Q, 1, tol_abs);
    BATCH_CALL(b, batch_W, b->Q, 1);
    if (fit) {
        const bool slabs = h_from_slabs(&b->plan);
        BATCH_CALL(b, batch_N, b->cur ^ 1, !slabs);
        BATCH_CALL(b, batch_H, slabs);
    }
    b->cur ^= 1;
}

// the problems' DevStates as they stand (one copy, one synchronisation); true: every stop rule has fired
bool read_states(klnmf_batch *b) {
    b->last.resize((size_t)b->count);
    HIPCHK(hipMemcpyAsync(b->last.data(), b->st, sizeof(DevState) * (size_t)b->count, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return std::all_of(b->last.begin(), b->last.end(), [](const DevState &s) { return s.stop != 0; });
}

void start_states(klnmf_batch *b);

// what both kinds of problem hold: shape, plan, the problems' states, loss records and flags
void take_common(klnmf_batch *b, const ProblemPlan &plan, int64_t n, int64_t f, int64_t k, int64_t cap) {
    b->plan = plan;
    b->n = n; b->f = f; b->k = k; b->cap = cap;
    b->cur = 0;
    const size_t B = (size_t)b->count;
    b->has_V.assign(B, 0); b->has_H.assign(B, 0);
    b->last.assign(B, DevState{});
    b->st = (DevState *)b->dalloc(sizeof(DevState) * B);
    b->st_init = (DevState *)b->dalloc(sizeof(DevState) * B);
    b->errors = (double *)b->dalloc(sizeof(double) * B * (size_t)cap);
    b->loss_xchg = (double *)b->dalloc(sizeof(double) * 2 * B);
}

void set_problem(klnmf_batch *b, int64_t n, int64_t f, int64_t k, int64_t cap) {
    const DevSwitches sw = problem_switches();
    const ProblemPlan plan = plan_dense_exact(n, f, k, b->prec, std::max(1, b->cu_count / b->count), sw);
    if (plan.refuse != KLNMF_OK) fail(plan.refuse, plan.refuse_msg);
    // the problem index shares gridDim.y with the row tiles (ratio, W rule) and with the component tiles (H numerator)
    if ((int64_t)b->count * ((std::max(n, k) + GT - 1) / GT) > 65535)
        fail(KLNMF_ERR_UNSUPP, "klnmf_batch_set_problem: count x row tiles of 64 exceed the 65535 of gridDim.y; use a smaller batch");
    if (plan.nsplit > 65535 || plan.wsplit > 65535 || k > 65535)
        fail(KLNMF_ERR_UNSUPP, "klnmf_batch_set_problem: more than 65535 chunks or components (gridDim.z, gridDim.y)");
    HIPCHK(hipStreamSynchronize(b->stream));
    b->free_all();
    take_common(b, plan, n, f, k, cap);
    const size_t B = (size_t)b->count, es = b->esize(), un = (size_t)n, uf = (size_t)f, uk = (size_t)k;
    b->V = b->dalloc(B * un * uf * es);
    b->Q = b->dalloc(B * un * uf * es);
    for (void *&w : b->W) w = b->dalloc(B * un * uk * es);
    b->H = b->dalloc(B * uk * uf * es);
    b->Npart = b->dalloc(B * (size_t)plan.nsplit * uk * uf * es);
    b->hpart = plan.hseg_n > 1 ? (double *)b->dalloc(sizeof(double) * B * uk * (size_t)plan.hseg_n) : nullptr;
    b->numer = b->dalloc(B * uk * uf * es);
    b->Wpart = plan.wsplit > 1 ? b->dalloc(B * (size_t)plan.wsplit * un * uk * es) : nullptr;
    b->loss_part = (double *)b->dalloc(sizeof(double) * B * (size_t)plan.loss_part_count);
    start_states(b);
}

// what klnmf_batch_set_problem_sparse does: the refusals, then -- the previous problem released -- the CSR layout of batch_sparse.hip.h
void set_problem_sparse(klnmf_batch *b, int64_t n, int64_t f, int64_t k, int64_t cap, const int64_t *nnz) {
    const std::string who = "klnmf_batch_set_problem_sparse";
    if (!nnz) fail(KLNMF_ERR_ARG, who + ": null nnz");
    int64_t total = 0, most = 0;
    bool empty = false;
    for (int p = 0; p < b->count; ++p) {
        if (nnz[p] < 0) fail(KLNMF_ERR_ARG, "n, f, k must be positive, nnz >= 0");
        if (nnz[p] >= (int64_t)1 << 31) fail(KLNMF_ERR_UNSUPP, who + ": 2^31 or more stored entries in the batch (int32 positions)");      // (and the total cannot overflow)
        empty = empty || nnz[p] == 0;
        total += nnz[p];
        most = std::max(most, nnz[p]);
    }
    const DevSwitches sw = problem_switches();
    // one pair of block counts for every problem: the context's rule on the batch's mean entries per problem
    const ProblemPlan plan = plan_csr(n, f, k, total / b->count, b->prec, b->cu_count, sw);
    if (plan.refuse != KLNMF_OK) fail(plan.refuse, plan.refuse_msg);
    if (k > 512) fail(KLNMF_ERR_UNSUPP, who + ": k > 512 has no blocked CSR kernels; run such problems one context each");
    if (empty) fail(KLNMF_ERR_UNSUPP, who + ": a problem without stored entries has no blocked CSR kernels; run it in a context");
    if (total >= (int64_t)1 << 31) fail(KLNMF_ERR_UNSUPP, who + ": 2^31 or more stored entries in the batch (int32 positions)");
    if (!plan.sp_blocked) fail(KLNMF_ERR_UNSUPP, who + ": the shape has no blocked CSR regime");
    HIPCHK(hipStreamSynchronize(b->stream));
    b->free_all();
    take_common(b, plan, n, f, k, cap);
    b->sparse = true;
    const size_t B = (size_t)b->count, es = b->esize(), un = (size_t)n, uf = (size_t)f, uk = (size_t)k, nz = (size_t)total, mz = (size_t)most;
    b->nnz.assign(nnz, nnz + b->count);
    b->off.assign(B + 1, 0);
    for (size_t p = 0; p < B; ++p) b->off[p + 1] = b->off[p] + nnz[p];
    for (void *&w : b->W) w = b->dalloc(B * un * uk * es);
    b->H = b->dalloc(B * uk * uf * es);
    b->HT = b->dalloc(B * uk * uf * es);
    b->numer = b->dalloc(B * uk * uf * es);
    b->hpart = plan.hseg_n > 1 ? (double *)b->dalloc(sizeof(double) * B * uk * (size_t)plan.hseg_n) : nullptr;
    b->sp_data = b->dalloc(nz * es);
    b->sp_q = b->dalloc(nz * es);
    b->sp_idx32 = (int *)b->dalloc(sizeof(int) * nz);
    b->csc_rows32 = (int *)b->dalloc(sizeof(int) * nz);
    b->csc_perm32 = (int *)b->dalloc(sizeof(int) * nz);
    b->sp_blkptr = (int64_t *)b->dalloc(sizeof(int64_t) * B * un * (size_t)(plan.sp_cb + 1));
    b->csc_blkptr = (int64_t *)b->dalloc(sizeof(int64_t) * B * uf * (size_t)(plan.sp_rb + 1));
    b->sp_loss_part = (double *)b->dalloc(sizeof(double) * B * (size_t)plan.sp_cb * un);
    b->sp_G = b->dalloc(B * (size_t)plan.sp_cb * un * uk * es);
    b->sp_NT = b->dalloc(B * (size_t)plan.sp_rb * uf * uk * es);
    b->sp_wpart = (double *)b->dalloc(sizeof(double) * B * (size_t)plan.sp_nblk * uk);
    b->sp_prod = (double *)b->dalloc(sizeof(double) * B * uk);
    b->sp_bad = (int *)b->dalloc(sizeof(int));
    b->u_indptr = (int64_t *)b->dalloc(sizeof(int64_t) * (un + 1));
    b->u_indices = (int64_t *)b->dalloc(sizeof(int64_t) * mz);
    b->u_csc_indptr = (int64_t *)b->dalloc(sizeof(int64_t) * (uf + 1));
    b->u_csc_rows = (int64_t *)b->dalloc(sizeof(int64_t) * mz);
    b->u_csc_perm = (int64_t *)b->dalloc(sizeof(int64_t) * mz);
    int64_t work = 0;
    for (int p = 0; p < b->count; ++p) work = std::max(work, csr_csc_work_elems(nnz[p]));
    b->u_work = (int64_t *)b->dalloc(sizeof(int64_t) * (size_t)work);
    start_states(b);
}

// problem p of a CSR batch as the shared upload steps see it: the upload's own arrays, and p's part of the batch's
CsrParts csr_parts(klnmf_batch *b, int p) {
    const ProblemPlan &pl = b->plan;
    const int64_t o = b->off[(size_t)p];
    return CsrParts{b->n, b->f, b->nnz[(size_t)p], b->prec, b->u_indptr, b->u_indices, b->u_csc_indptr, b->u_csc_rows, b->u_csc_perm, b->u_work,
                    (char *)b->sp_data + (size_t)o * b->esize(), pl.sp_cb, pl.sp_rb, pl.sp_cb_cols, pl.sp_rb_rows,
                    b->sp_blkptr + (int64_t)p * b->n * (pl.sp_cb + 1), b->csc_blkptr + (int64_t)p * b->f * (pl.sp_rb + 1), b->sp_idx32 + o,
                    b->csc_rows32 + o, b->csc_perm32 + o, b->sp_bad};
}

void need_sparse(klnmf_batch *b, int p, const char *who) {
    need_p(b, p);
    if (!b->sparse) fail(KLNMF_ERR_ARG, std::string(who) + " needs klnmf_batch_set_problem_sparse");
}

// the device tail of an upload into problem p: CSC order, block pointers and int32 copies by the context's steps on the problem's
// own positions, then the positions moved to the concatenated arrays
void csr_finish_upload(klnmf_batch *b, int p, const CsrParts &v, const std::string &msg) {
    csr_csc_build(b->stream, v);
    csr_blocked_setup(b->stream, v, msg);
    const int64_t o = b->off[(size_t)p], nb = b->n * (v.cb + 1), ncb = b->f * (v.rb + 1);
    if (o > 0) {
        hipLaunchKernelGGL(k_spb_shift, dim3(grid_for(nb, 256, 8192)), dim3(256), 0, b->stream, v.blkptr, nb, o);
        hipLaunchKernelGGL(k_spb_shift, dim3(grid_for(ncb, 256, 8192)), dim3(256), 0, b->stream, v.cblkptr, ncb, o);
        hipLaunchKernelGGL(k_spb_shift32, dim3(grid_for(v.nnz, 256, 8192)), dim3(256), 0, b->stream, v.perm32, v.nnz, (int)o);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(b->stream));
    b->has_V[(size_t)p] = 1;
}

// the state every loop starts from, and the problems' states set to it
void start_states(klnmf_batch *b) {
    const size_t B = (size_t)b->count;
    // what k_reset_state leaves (common.hip.h), once: a loop's entry copies it over the problems' states
    DevState init{};
    init.prev_err = std::numeric_limits<double>::infinity();
    init.prev2[0] = init.prev2[1] = init.prev_err;
    init.mon_spread_bits = 0x3f800000u;
    const std::vector<DevState> inits(B, init);
    HIPCHK(hipMemcpyAsync(b->st_init, inits.data(), sizeof(DevState) * B, hipMemcpyHostToDevice, b->stream));
    reset_states(b);
    HIPCHK(hipStreamSynchronize(b->stream));
    b->have_problem = true;
}

// the shared argument checks of a mask upload (a batch holds no weights)
void presence_check_all(klnmf_batch *b, const std::string &who, int64_t rows, int64_t row0, bool rows_ok, const int64_t *col_bounds, int n_mod) {
    if (b->sparse) fail(KLNMF_ERR_UNSUPP, who + ": CSR problems have no masked kernels (the ratio lives on the stored entries only)");
    presence_check_args(who, b->mask_dims(), rows, row0, rows_ok, col_bounds, n_mod);
    if (b->beta_on())
        fail(KLNMF_ERR_UNSUPP, who + ": the batch runs a beta divergence (klnmf_batch_set_divergence), which has no masked form; upload the "
                                     "mask as weights (klnmf_batch_upload_weights) or klnmf_batch_set_divergence(b, 1.0) first");
    presence_check_bounds(*b, who, "batch", col_bounds, n_mod);
}

}  // namespace

extern "C" {

int klnmf_batch_create(klnmf_batch **out, int device, int precision, int count) {
    return guarded([&] {
        if (!out) fail(KLNMF_ERR_ARG, "null out pointer");
        if (precision != KLNMF_PREC_F64 && precision != KLNMF_PREC_F32)
            fail(KLNMF_ERR_UNSUPP, "klnmf_batch_create: a batch runs in KLNMF_PREC_F64 / KLNMF_PREC_F32 (dense, unweighted problems on the "
                                   "exact kernels); run the other modes one context per problem");
        if (count < 1 || count > KLNMF_BATCH_MAX)
            fail(KLNMF_ERR_ARG, "klnmf_batch_create: count must be in 1 .. " + std::to_string(KLNMF_BATCH_MAX));
        int ndev = 0;
        HIPCHK(hipGetDeviceCount(&ndev));
        if (device < 0 || device >= ndev) fail(KLNMF_ERR_ARG, "no such device");
        HIPCHK(hipSetDevice(device));
        hipDeviceProp_t p;
        HIPCHK(hipGetDeviceProperties(&p, device));
        if (std::strncmp(p.gcnArchName, "gfx950", 6) != 0)
            fail(KLNMF_ERR_UNSUPP, std::string("this library is built for gfx950 only, device is ") + p.gcnArchName);
        klnmf_batch *b = new klnmf_batch();
        b->device = device; b->prec = precision; b->count = count; b->cu_count = p.multiProcessorCount;
        const hipError_t e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete b;
            HIPCHK(e);
        }
        *out = b;
    });
}

int klnmf_batch_destroy(klnmf_batch *b) {
    return guarded([&] {
        if (!b) return;
        (void)hipSetDevice(b->device);
        (void)hipStreamSynchronize(b->stream);
        b->free_all();
        (void)hipStreamDestroy(b->stream);
        delete b;
    });
}

int klnmf_batch_set_problem(klnmf_batch *b, int64_t n, int64_t f, int64_t k, int64_t cap) {
    return guarded([&] {
        use(b);      // (a CSR problem before it goes with free_all, as a dense one before klnmf_batch_set_problem_sparse)
        if (cap < 0) fail(KLNMF_ERR_ARG, "n, f, k must be positive");
        set_problem(b, n, f, k, cap > 0 ? cap : 1);
    });
}

int klnmf_batch_upload_V(klnmf_batch *b, int p, const void *src, int dtype, int64_t rows, int64_t cols, int64_t ld, int64_t row0,
                         int64_t col0, double scale) {
    return guarded([&] {
        need_p(b, p);
        if (b->sparse) fail(KLNMF_ERR_ARG, "klnmf_batch_upload_V: a CSR batch holds no dense V (klnmf_batch_upload_csr_rows)");
        if (!src) fail(KLNMF_ERR_ARG, "null source");
        check_dtype(dtype);
        check_block(b->n, b->f, rows, cols, ld, row0, col0);
        if (rows * cols == 0) return;
        staged_upload(b->stream, src, dt_size(dtype), rows, cols, ld, [&](const void *d, int64_t r0, int64_t rr) {
            place_block(b, p, d, dtype, nullptr, rr, cols, ld, row0 + r0, col0, scale);
        });
    });
}

int klnmf_batch_upload_V_device_rows_dt(klnmf_batch *b, int p, const void *dsrc, int dtype, const int64_t *drow_idx, int64_t rows,
                                        int64_t cols, int64_t ld, int64_t row0, int64_t col0, double scale) {
    return guarded([&] {
        need_p(b, p);
        if (b->sparse) fail(KLNMF_ERR_ARG, "klnmf_batch_upload_V_device_rows_dt: a CSR batch holds no dense V (klnmf_batch_upload_csr_device_rows)");
        if (!dsrc) fail(KLNMF_ERR_ARG, "null source");
        check_dtype(dtype);
        check_block(b->n, b->f, rows, cols, ld, row0, col0);
        place_block(b, p, dsrc, dtype, drow_idx, rows, cols, ld, row0, col0, scale);
    });
}

int klnmf_batch_set_H(klnmf_batch *b, int p, const void *src, int dtype) {
    return guarded([&] {
        need_p(b, p);
        if (!src) fail(KLNMF_ERR_ARG, "null source");
        check_dtype(dtype);
        set_matrix(b, problem_ptr(b, b->H, p, b->k * b->f), src, dtype, b->k, b->f);
        b->has_H[(size_t)p] = 1;
    });
}

int klnmf_batch_set_H_device(klnmf_batch *b, int p, const void *dsrc, int dtype, int64_t ld, int64_t col0, int64_t ncols, int last) {
    return guarded([&] {
        need_p(b, p);
        if (!dsrc) fail(KLNMF_ERR_ARG, "null source");
        check_dtype(dtype);
        if (col0 < 0 || ncols < 0 || col0 + ncols > b->f || ld < ncols) fail(KLNMF_ERR_ARG, "klnmf_batch_set_H_device: column block out of range");
        char *H = (char *)problem_ptr(b, b->H, p, b->k * b->f) + (size_t)col0 * b->esize();
        copy_2d_any(b->stream, H, b->prec == KLNMF_PREC_F64, b->f, dsrc, dtype == KLNMF_DT_F64, ld, b->k, ncols);
        if (last) {
            HIPCHK(hipStreamSynchronize(b->stream));      // the caller's buffer may go away
            b->has_H[(size_t)p] = 1;
        }
    });
}

int klnmf_batch_set_W(klnmf_batch *b, int p, const void *src, int dtype) {
    return guarded([&] {
        need_p(b, p);
        if (!src) fail(KLNMF_ERR_ARG, "null source");
        check_dtype(dtype);
        set_matrix(b, problem_ptr(b, b->W[b->cur], p, b->n * b->k), src, dtype, b->n, b->k);
    });
}

int klnmf_batch_init_W(klnmf_batch *b) {
    return guarded([&] {
        need_problem(b);
        reset_states(b);
        if (b->sparse) {      // W0 = X . H0^T over the stored entries (klnmf_init_W on a CSR context): H^T, the SPB_INIT pass, the W rule
            BATCH_CALL(b, csr_transpose_H);
            BATCH_CALL(b, csr_W, 0);
        } else BATCH_CALL(b, batch_W, b->V, 0);
        b->cur ^= 1;
    });
}

int klnmf_batch_run(klnmf_batch *b, int64_t max_iter, int fit, double tol_abs) {
    return guarded([&] {
        need_problem(b);
        if (max_iter < 0) fail(KLNMF_ERR_ARG, "max_iter < 0");
        if (max_iter > b->cap) fail(KLNMF_ERR_ARG, "max_iter exceeds the capacity given to klnmf_batch_set_problem");
        for (int p = 0; p < b->count; ++p)
            if (!b->has_V[(size_t)p] || !b->has_H[(size_t)p])
                fail(KLNMF_ERR_ARG, "klnmf_batch_run: problem " + std::to_string(p) + " has no " + (b->has_V[(size_t)p] ? "H" : "V") + " yet");
        reset_states(b);
        const int start = b->cur;
        for (int64_t it = 0; it < max_iter; ++it) {
            batch_iteration(b, fit, tol_abs);
            if (tol_abs > 0 && (it & 15) == 15 && read_states(b)) break;
        }
        read_states(b);
        // problem p's current W is the one its last EXECUTED update wrote: buffer start ^ (n_done & 1).  Outside a loop all of them
        // live in one buffer, problem 0's; the others' are copied there where their parity differs
        auto where = [&](int p) { return (start + (b->last[(size_t)p].n_done & 1)) & 1; };
        b->cur = where(0);
        const size_t wbytes = (size_t)b->n * b->k * b->esize();
        for (int p = 1; p < b->count; ++p)
            if (where(p) != b->cur)
                HIPCHK(hipMemcpyAsync(problem_ptr(b, b->W[b->cur], p, b->n * b->k), problem_ptr(b, b->W[b->cur ^ 1], p, b->n * b->k), wbytes,
                                      hipMemcpyDeviceToDevice, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
    });
}

int klnmf_batch_result(klnmf_batch *b, int p, double *errors_out, int64_t *n_done, int *stopped) {
    return guarded([&] {
        need_p(b, p);
        const DevState &s = b->last[(size_t)p];
        const int64_t nd = std::min<int64_t>(s.n_done, b->cap);
        if (errors_out && nd > 0) HIPCHK(hipMemcpy(errors_out, b->errors + (size_t)p * b->cap, sizeof(double) * (size_t)nd, hipMemcpyDeviceToHost));
        if (n_done) *n_done = s.n_done;
        if (stopped) *stopped = s.stop;
    });
}

int klnmf_batch_get_W(klnmf_batch *b, int p, void *dst, int dtype) {
    return guarded([&] {
        need_p(b, p);
        if (!dst) fail(KLNMF_ERR_ARG, "null destination");
        check_dtype(dtype);
        get_matrix(b, dst, dtype, problem_ptr(b, b->W[b->cur], p, b->n * b->k), b->n, b->k);
    });
}

int klnmf_batch_get_H(klnmf_batch *b, int p, void *dst, int dtype) {
    return guarded([&] {
        need_p(b, p);
        if (!dst) fail(KLNMF_ERR_ARG, "null destination");
        check_dtype(dtype);
        get_matrix(b, dst, dtype, problem_ptr(b, b->H, p, b->k * b->f), b->k, b->f);
    });
}

int klnmf_batch_get_W_device(klnmf_batch *b, int p, void *ddst, int dtype, int64_t ld) {
    return guarded([&] {
        need_p(b, p);
        if (!ddst) fail(KLNMF_ERR_ARG, "null destination");
        check_dtype(dtype);
        if (ld < b->k) fail(KLNMF_ERR_ARG, "klnmf_batch_get_W_device: row stride shorter than k");
        copy_2d_any(b->stream, ddst, dtype == KLNMF_DT_F64, ld, problem_ptr(b, b->W[b->cur], p, b->n * b->k), b->prec == KLNMF_PREC_F64, b->k, b->n, b->k);
        HIPCHK(hipStreamSynchronize(b->stream));
    });
}

int klnmf_batch_query(klnmf_batch *b, int what, int64_t *value) {
    return guarded([&] {
        use(b);
        if (!value) fail(KLNMF_ERR_ARG, "null destination");
        if (what == KLNMF_Q_BATCH_COUNT) { *value = b->count; return; }
        if (what == KLNMF_Q_PRESENCE) { *value = (b->have_problem && b->presence()) ? b->pres_M : 0; return; }
        if (what == KLNMF_Q_SP_COL_BLOCKS || what == KLNMF_Q_SP_ROW_BLOCKS) {
            *value = 0;
            if (b->have_problem) plan_answer(b->plan, what, value);
            return;
        }
        if (what != KLNMF_Q_EX_ROW_CHUNKS && what != KLNMF_Q_EX_W_CHUNKS && what != KLNMF_Q_EX_H_SEGMENTS && what != KLNMF_Q_EX_H_FROM_SLABS)
            fail(KLNMF_ERR_ARG, "klnmf_batch_query: unknown item");
        if (!b->have_problem) { *value = 0; return; }
        plan_answer(b->plan, what, value);
    });
}

// ---- klnmf_batch_csr.h ---------------------------------------------------------------------------------------------------------
int klnmf_batch_set_problem_sparse(klnmf_batch *b, int64_t n, int64_t f, int64_t k, int64_t cap, const int64_t *nnz) {
    return guarded([&] {
        use(b);
        if (cap < 0) fail(KLNMF_ERR_ARG, "n, f, k must be positive, nnz >= 0");
        set_problem_sparse(b, n, f, k, cap > 0 ? cap : 1, nnz);
    });
}

// klnmf_upload_csr_rows for problem p
int klnmf_batch_upload_csr_rows(klnmf_batch *b, int p, int dtype, const int64_t *indptr, const int64_t *indices, const void *data) {
    return guarded([&] {
        need_sparse(b, p, "klnmf_batch_upload_csr_rows");
        if (!indptr || !indices || !data) fail(KLNMF_ERR_ARG, "null pointer");
        check_dtype(dtype);
        const CsrParts v = csr_parts(b, p);
        if (indptr[0] != 0 || indptr[b->n] != v.nnz) fail(KLNMF_ERR_ARG, "klnmf_batch_upload_csr_rows: the row pointers do not match n, nnz[p]");
        b->has_V[(size_t)p] = 0;
        HIPCHK(hipMemcpyAsync(v.indptr, indptr, sizeof(int64_t) * (b->n + 1), hipMemcpyHostToDevice, b->stream));
        HIPCHK(hipMemcpyAsync(v.indices, indices, sizeof(int64_t) * v.nnz, hipMemcpyHostToDevice, b->stream));
        set_matrix(b, v.data, data, dtype, 1, v.nnz);      // (the values: a 1 x nnz matrix through the dtype conversion)
        csr_finish_upload(b, p, v, "klnmf_batch_upload_csr_rows: the column indices of every row must be sorted");
    });
}

// klnmf_upload_csr_device_rows for problem p
int klnmf_batch_upload_csr_device_rows(klnmf_batch *b, int p, int n_mod, const int64_t *const *indptr, const int32_t *const *indices,
                                       const void *const *data, const int *dtype, const int64_t *col_bounds, const double *scale,
                                       int64_t src_rows, const int64_t *drow_idx, int64_t rows) {
    return guarded([&] {
        need_sparse(b, p, "klnmf_batch_upload_csr_device_rows");
        const CsrParts v = csr_parts(b, p);
        csr_gather_rows(*b, v, "klnmf_batch_upload_csr_device_rows", n_mod, indptr, indices, data, dtype, col_bounds, scale, src_rows,
                        drow_idx, rows, [&] { b->has_V[(size_t)p] = 0; });
        csr_finish_upload(b, p, v, "klnmf_batch_upload_csr_device_rows: the column indices of every source row must be sorted");
    });
}

// ---- klnmf_batch_mask.h --------------------------------------------------------------------------------------------------------
// klnmf_upload_presence for problem p: P_p[row0 + i, m] = src[i, m]
int klnmf_batch_upload_presence(klnmf_batch *b, int p, const void *src, int dtype, int64_t rows, int64_t ld, int64_t row0,
                                const int64_t *col_bounds, int n_mod) {
    return guarded([&] {
        need_p(b, p);
        const std::string who = "klnmf_batch_upload_presence";
        if (!src) fail(KLNMF_ERR_ARG, "null source");
        check_dtype(dtype);
        presence_check_all(b, who, rows, row0, ld >= n_mod, col_bounds, n_mod);
        presence_take(*b, *b, b->mask_dims(), col_bounds, n_mod);
        if (rows == 0) return;
        presence_upload(*b, *b, b->mask_dims(), p, src, dtype, rows, ld, row0);
    });
}

// klnmf_upload_presence_device_rows for problem p: only clean row indices take the mask (a first upload) and launch the gather into
// problem p's P
int klnmf_batch_upload_presence_device_rows(klnmf_batch *b, int p, const void *dP, int dtype, int64_t src_rows, int64_t ld,
                                            const int64_t *drow_idx, int64_t rows, int64_t row0, const int *src_cols,
                                            const int64_t *col_bounds, int n_mod) {
    return guarded([&] {
        need_p(b, p);
        const std::string who = "klnmf_batch_upload_presence_device_rows";
        if (!dP) fail(KLNMF_ERR_ARG, "null source");
        check_dtype(dtype);
        presence_check_all(b, who, rows, row0, ld >= 0 && src_rows >= 0 && (drow_idx || rows <= src_rows), col_bounds, n_mod);
        if (!src_cols) fail(KLNMF_ERR_ARG, who + ": null source columns");
        PresenceCols cols{};
        for (int m = 0; m < n_mod; ++m) {
            if (src_cols[m] < -1 || src_cols[m] >= ld) fail(KLNMF_ERR_ARG, who + ": a source column outside [-1, ld)");
            cols.col[m] = src_cols[m];
        }
        if (rows > 0 && drow_idx) presence_rows_check(*b, who, drow_idx, rows, src_rows);
        presence_take(*b, *b, b->mask_dims(), col_bounds, n_mod);
        if (rows == 0) return;
        presence_gather(*b, *b, b->mask_dims(), p, dP, dtype, ld, drow_idx, rows, row0, cols);
    });
}

// the batch runs the unmasked kernels again
int klnmf_batch_clear_presence(klnmf_batch *b) {
    return guarded([&] {
        need_problem(b);
        presence_drop(*b, *b);
    });
}

// ---- klnmf_batch_beta.h --------------------------------------------------------------------------------------------------------
// klnmf_set_divergence for a batch: the refusals, then -- all or nothing -- what only the beta loop holds
int klnmf_batch_set_divergence(klnmf_batch *b, double beta) {
    return guarded([&] {
        need_problem(b);
        const std::string who = "klnmf_batch_set_divergence";
        if (!std::isfinite(beta)) fail(KLNMF_ERR_ARG, who + ": beta must be finite");
        if (beta == 1.0) {      // the KL loop again: nothing of the beta cost stays, the weights neither
            if (!b->beta_on()) return;
            HIPCHK(hipStreamSynchronize(b->stream));
            b->dfree(b->Bt); b->dfree(b->Om); b->dfree(b->Dpart); b->dfree(b->denom); b->dfree(b->WDpart);
            if (b->own_hpart) { void *h = b->hpart; b->dfree(h); b->hpart = nullptr; }
            b->forget_beta();
            return;
        }
        if (b->sparse) fail(KLNMF_ERR_UNSUPP, who + ": CSR problems have no beta kernels (the ratio lives on the stored entries only)");
        if (b->prec == KLNMF_PREC_F32 && beta != 0.0 && ((float)beta == 1.0f || (float)beta == 0.0f))
            fail(KLNMF_ERR_ARG, who + ": in KLNMF_PREC_F32 the kernels see beta rounded to fp32, and this beta rounds to 1 or to 0 "
                                      "without being it (the general cost divides by beta (beta - 1)); give 1 or 0 itself");
        if (b->presence())
            fail(KLNMF_ERR_UNSUPP, who + ": the batch holds a presence mask (klnmf_batch_upload_presence), and the beta rules have no masked "
                                         "form; klnmf_batch_clear_presence first and upload the mask as weights");
        if (b->beta_on()) { b->beta = beta; return; }      // (the buffers are there)
        HIPCHK(hipStreamSynchronize(b->stream));
        const ProblemPlan &pl = b->plan;
        const size_t B = (size_t)b->count, es = b->esize(), n = (size_t)b->n, f = (size_t)b->f, k = (size_t)b->k;
        const bool have_sums = b->hpart != nullptr;         // (long rows: the problem holds [B][k][hseg_n] already)
        void *bt = nullptr, *sums = nullptr, *dpart = nullptr, *denom = nullptr, *wdpart = nullptr;
        try {
            bt = b->dalloc(B * n * f * es);
            if (!have_sums) sums = b->dalloc(sizeof(double) * B * k);
            dpart = b->dalloc(B * (size_t)pl.nsplit * k * f * es);
            denom = b->dalloc(B * k * f * es);
            if (pl.wsplit > 1) wdpart = b->dalloc(B * (size_t)pl.wsplit * n * k * es);
        } catch (...) {                                     // all or nothing: a failed call leaves the batch at beta = 1
            (void)hipStreamSynchronize(b->stream);
            b->dfree(bt); b->dfree(sums); b->dfree(dpart); b->dfree(denom); b->dfree(wdpart);
            throw;
        }
        b->Bt = bt; b->Dpart = dpart; b->denom = denom; b->WDpart = wdpart;
        if (!have_sums) { b->hpart = (double *)sums; b->own_hpart = true; }
        b->beta = beta;
    });
}

int klnmf_batch_get_divergence(klnmf_batch *b, double *beta) {
    return guarded([&] {
        need_problem(b);
        if (!beta) fail(KLNMF_ERR_ARG, "klnmf_batch_get_divergence: null destination");
        *beta = b->beta;
    });
}

// klnmf_upload_weights for problem p of a beta batch: Om_p[row0 + i, col0 + j] = src[i, j]; the first call takes every problem's Om
// filled with 1
int klnmf_batch_upload_weights(klnmf_batch *b, int p, const void *src, int dtype, int64_t rows, int64_t cols, int64_t ld, int64_t row0,
                               int64_t col0) {
    return guarded([&] {
        need_p(b, p);
        if (!b->beta_on())
            fail(KLNMF_ERR_UNSUPP, "klnmf_batch_upload_weights: the batch runs the Kullback-Leibler loop (beta = 1), which has no weighted "
                                   "batch kernels; klnmf_batch_set_divergence first, or klnmf_batch_upload_presence for a mask");
        if (!src) fail(KLNMF_ERR_ARG, "null source");
        check_dtype(dtype);
        check_block(b->n, b->f, rows, cols, ld, row0, col0);
        if (!b->Om) {
            HIPCHK(hipStreamSynchronize(b->stream));
            void *om = b->dalloc((size_t)b->count * (size_t)b->n * (size_t)b->f * b->esize(), false);
            try {
                fill_ones(b->stream, om, b->prec == KLNMF_PREC_F64, (int64_t)b->count * b->n * b->f);
                HIPCHK(hipStreamSynchronize(b->stream));
            } catch (...) {
                (void)hipStreamSynchronize(b->stream);
                b->dfree(om);
                throw;
            }
            b->Om = om;
        }
        if (rows * cols == 0) return;
        staged_upload(b->stream, src, dt_size(dtype), rows, cols, ld, [&](const void *d, int64_t r0, int64_t rr) {
            place_rows(b->stream, problem_ptr(b, b->Om, p, b->n * b->f), b->prec == KLNMF_PREC_F64, b->f, d, dtype == KLNMF_DT_F64, rr, cols, ld,
                       row0 + r0, col0, 1.0, nullptr);
        });
    });
}

}  // extern "C"
