// libklnmf.so, unit 6 of 6: klnmf_batch_* -- B dense problems of one shape in KLNMF_PREC_F64 / F32, unweighted or (all of them)
// under row x modality presence masks (klnmf_batch_mask.h), that run the loop of nmf.py:212-222 together, one launch per stage
// for all of them (batch.hip.h has the kernels and the layout; ctx.hip.h lists the other units).  The plan is the single problem's (plan_dense_exact) for max(1, cu_count / B) compute units; the launch
// sequence of an iteration is local_iteration's for a dense unweighted problem of the exact modes (api_loop.hip: exact_Q, exact_W,
// exact_N, exact_H), stage for stage -- with a mask: for a dense masked problem (presence_S in front of the W rule, presence_D in
// front of the H numerator).
#include "ctx.hip.h"
#include "../../include/klnmf_batch.h"
#include "../../include/klnmf_batch_mask.h"
#include "batch.hip.h"

struct klnmf_batch {
    int device = 0, prec = KLNMF_PREC_F64, cu_count = 256, count = 1;
    hipStream_t stream = nullptr;
    std::vector<std::pair<void *, size_t>> allocs;      // (block, size class) of the current problem's device blocks
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
    // ---- a masked batch (klnmf_batch_upload_presence*; batch.hip.h has the layout): every problem's P -- taken filled with 1 by the
    // first upload --, S, D and D's slabs, and once per batch the bounds (host and device) and the per-column modality bytes.
    // Dropped by klnmf_batch_clear_presence and with the problem
    int pres_M = 0, pres_dchunks = 0;
    int64_t pres_bounds[kMaxMod + 1] = {};
    void *Pm = nullptr, *pres_S = nullptr, *pres_D = nullptr, *pres_Dslab = nullptr, *pres_dbounds = nullptr, *pres_mod = nullptr;
    bool presence() const { return pres_M > 0; }

    size_t esize() const { return prec_esize(prec); }
    void *dalloc(size_t bytes) {      // (klnmf_ctx::dalloc: the block cache of api_context.hip, zero-filled blocks)
        if (bytes == 0) bytes = 16;
        const size_t cls = DevBlockCache::size_class(bytes);
        void *p = g_block_cache.take(device, cls);
        if (!p) {
            hipError_t e = hipMalloc(&p, cls);
            if (e == hipErrorOutOfMemory) {
                (void)hipGetLastError();
                g_block_cache.flush(device);
                e = hipMalloc(&p, cls);
            }
            HIPCHK(e);
        }
        allocs.push_back({p, cls});
        HIPCHK(hipMemsetAsync(p, 0, bytes, stream));
        return p;
    }
    void dfree(void *&p) {      // one block back (callers have synchronised the stream)
        for (size_t i = 0; p && i < allocs.size(); ++i)
            if (allocs[i].first == p) {
                if (!g_block_cache.give(device, allocs[i].second, p)) (void)hipFree(p);
                allocs.erase(allocs.begin() + (std::ptrdiff_t)i);
                break;
            }
        p = nullptr;
    }
    void forget_presence() {      // (the blocks are gone or go with `allocs`)
        Pm = pres_S = pres_D = pres_Dslab = pres_dbounds = pres_mod = nullptr;
        pres_M = 0; pres_dchunks = 0;
        std::fill(pres_bounds, pres_bounds + kMaxMod + 1, (int64_t)0);
    }
    void free_all() {      // (callers have synchronised the stream)
        for (auto &a : allocs)
            if (!g_block_cache.give(device, a.second, a.first)) (void)hipFree(a.first);
        allocs.clear();
        forget_presence();
        have_problem = false;
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
void check_dtype(int dtype) {
    if (dtype != KLNMF_DT_F32 && dtype != KLNMF_DT_F64) fail(KLNMF_ERR_ARG, "dtype must be KLNMF_DT_F32 or KLNMF_DT_F64");
}

// fn<T>(b, ...) in the batch's element type
#define BATCH_CALL(b, fn, ...)                                         \
    do {                                                               \
        if ((b)->prec == KLNMF_PREC_F64) fn<double>(b, ##__VA_ARGS__); \
        else fn<float>(b, ##__VA_ARGS__);                              \
    } while (0)

// dst[rows, cols] (rows dld apart, type D by `d64`) = src[rows, cols] (rows sld apart, type by `s64`), on the device
void copy_2d_any(klnmf_batch *b, void *dst, bool d64, int64_t dld, const void *src, bool s64, int64_t sld, int64_t rows, int64_t cols) {
    if (rows * cols == 0) return;
    const dim3 grid(grid_for(rows * cols, 256, 8192));
#define KL_COPY(D, S) hipLaunchKernelGGL((k_copy_2d<D, S>), grid, dim3(256), 0, b->stream, (D *)dst, dld, (const S *)src, sld, rows, cols, 1.0)
    if (d64) { if (s64) KL_COPY(double, double); else KL_COPY(double, float); }
    else { if (s64) KL_COPY(float, double); else KL_COPY(float, float); }
#undef KL_COPY
    HIPCHK(hipGetLastError());
}

// a host matrix [rows, cols] into a device matrix of the batch's type, and back (klnmf_set_H / klnmf_get_W of a context)
void set_matrix(klnmf_batch *b, void *dst, const void *src, int dtype, int64_t rows, int64_t cols) {
    const size_t bytes = (size_t)rows * cols * (dtype == KLNMF_DT_F64 ? 8 : 4);
    void *d = nullptr;
    HIPCHK(hipMalloc(&d, bytes ? bytes : 16));
    try {
        HIPCHK(hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, b->stream));
        copy_2d_any(b, dst, b->prec == KLNMF_PREC_F64, cols, d, dtype == KLNMF_DT_F64, cols, rows, cols);
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
        copy_2d_any(b, d, dtype == KLNMF_DT_F64, cols, src, b->prec == KLNMF_PREC_F64, cols, rows, cols);
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
    void *V = problem_ptr(b, b->V, p, b->n * b->f);
    const dim3 grid(grid_for(rows * cols, 256, 8192));
#define KL_PLACE(T, S) hipLaunchKernelGGL((k_place_V<T, S>), grid, dim3(256), 0, b->stream, (T *)V, b->f, (const S *)dsrc, rows, cols, ld, row0, col0, scale, row_idx)
    if (b->prec == KLNMF_PREC_F64) { if (dtype == KLNMF_DT_F64) KL_PLACE(double, double); else KL_PLACE(double, float); }
    else { if (dtype == KLNMF_DT_F64) KL_PLACE(float, double); else KL_PLACE(float, float); }
#undef KL_PLACE
    HIPCHK(hipGetLastError());
    b->has_V[(size_t)p] = 1;
}

void check_block(const klnmf_batch *b, int64_t rows, int64_t cols, int64_t ld, int64_t row0, int64_t col0) {
    if (rows < 0 || cols < 0 || row0 < 0 || col0 < 0 || row0 + rows > b->n || col0 + cols > b->f || ld < cols)
        fail(KLNMF_ERR_ARG, "V block out of range");
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

// one iteration for every problem (local_iteration of api_loop.hip): ratio + loss, stop rule, W rule, and in a fit the H rule;
// masked: Q, then S and the W rule, and in a fit D, N and the H rule
void batch_iteration(klnmf_batch *b, int fit, double tol_abs) {
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
    b->plan = plan;
    b->n = n; b->f = f; b->k = k; b->cap = cap;
    b->cur = 0;
    const size_t B = (size_t)b->count, es = b->esize(), un = (size_t)n, uf = (size_t)f, uk = (size_t)k;
    b->has_V.assign(B, 0); b->has_H.assign(B, 0);
    b->last.assign(B, DevState{});
    b->st = (DevState *)b->dalloc(sizeof(DevState) * B);
    b->st_init = (DevState *)b->dalloc(sizeof(DevState) * B);
    b->errors = (double *)b->dalloc(sizeof(double) * B * (size_t)cap);
    b->loss_xchg = (double *)b->dalloc(sizeof(double) * 2 * B);
    b->V = b->dalloc(B * un * uf * es);
    b->Q = b->dalloc(B * un * uf * es);
    for (void *&w : b->W) w = b->dalloc(B * un * uk * es);
    b->H = b->dalloc(B * uk * uf * es);
    b->Npart = b->dalloc(B * (size_t)plan.nsplit * uk * uf * es);
    b->hpart = plan.hseg_n > 1 ? (double *)b->dalloc(sizeof(double) * B * uk * (size_t)plan.hseg_n) : nullptr;
    b->numer = b->dalloc(B * uk * uf * es);
    b->Wpart = plan.wsplit > 1 ? b->dalloc(B * (size_t)plan.wsplit * un * uk * es) : nullptr;
    b->loss_part = (double *)b->dalloc(sizeof(double) * B * (size_t)plan.loss_part_count);
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

// ---- presence masks (klnmf_batch_mask.h): presence_check_args / presence_take of api_context.hip for a batch -------------------
// `rows_ok`: the caller's own part of "rows out of range" (the source's leading dimension).  Everything here is checked before
// anything is taken or written: a refused call leaves the batch as it was.
void batch_presence_check(klnmf_batch *b, const std::string &who, int64_t rows, int64_t row0, bool rows_ok, const int64_t *col_bounds,
                          int n_mod) {
    if (n_mod < 1 || n_mod > KLNMF_MAX_MODALITIES)
        fail(KLNMF_ERR_ARG, who + ": 1 <= n_mod <= KLNMF_MAX_MODALITIES (" + std::to_string(KLNMF_MAX_MODALITIES) + ")");
    if (!col_bounds) fail(KLNMF_ERR_ARG, who + ": null column bounds");
    if (col_bounds[0] != 0 || col_bounds[n_mod] != b->f) fail(KLNMF_ERR_ARG, who + ": the column bounds must run from 0 to f");
    for (int m = 0; m < n_mod; ++m)
        if (col_bounds[m] >= col_bounds[m + 1]) fail(KLNMF_ERR_ARG, who + ": the column bounds must increase strictly");
    if (rows < 0 || row0 < 0 || row0 + rows > b->n || !rows_ok) fail(KLNMF_ERR_ARG, who + ": rows out of range");
    if (b->presence() && (n_mod != b->pres_M || !std::equal(col_bounds, col_bounds + n_mod + 1, b->pres_bounds)))
        fail(KLNMF_ERR_ARG, who + ": the column bounds differ from the ones the batch's first upload fixed");
}

// The first mask upload of a batch: every problem's P filled with 1, S, D, D's slabs, and once for all the bounds and the
// per-column modality bytes.  All or nothing; a batch that holds a mask already is left alone.
void batch_presence_take(klnmf_batch *b, const int64_t *col_bounds, int n_mod) {
    if (b->presence()) return;
    const size_t es = b->esize(), B = (size_t)b->count;
    const int64_t M = n_mod;
    HIPCHK(hipStreamSynchronize(b->stream));
    void *pm = nullptr, *S = nullptr, *D = nullptr, *Dslab = nullptr, *dbounds = nullptr, *mod = nullptr;
    try {
        const int dch = presence_d_chunks(b->n);
        pm = b->dalloc(B * (size_t)(b->n * M) * es);
        S = b->dalloc(B * (size_t)(M * b->k) * es);
        D = b->dalloc(B * (size_t)(b->k * M) * es);
        Dslab = b->dalloc(B * (size_t)dch * (size_t)(b->k * M) * sizeof(double));
        dbounds = b->dalloc((size_t)(M + 1) * sizeof(int64_t));
        mod = b->dalloc((size_t)b->f);
        std::vector<unsigned char> modv((size_t)b->f);
        for (int m = 0; m < n_mod; ++m) std::fill(modv.begin() + col_bounds[m], modv.begin() + col_bounds[m + 1], (unsigned char)m);
        HIPCHK(hipMemcpyAsync(mod, modv.data(), modv.size(), hipMemcpyHostToDevice, b->stream));
        HIPCHK(hipMemcpyAsync(dbounds, col_bounds, (size_t)(M + 1) * sizeof(int64_t), hipMemcpyHostToDevice, b->stream));
        const int64_t count = (int64_t)B * b->n * M;
        if (b->prec == KLNMF_PREC_F64)
            hipLaunchKernelGGL((k_fill<double>), dim3(grid_for(count, 256, 8192)), dim3(256), 0, b->stream, (double *)pm, count, 1.0);
        else
            hipLaunchKernelGGL((k_fill<float>), dim3(grid_for(count, 256, 8192)), dim3(256), 0, b->stream, (float *)pm, count, 1.0f);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(b->stream));      // (the host images above are read by the copies until here)
        b->pres_dchunks = dch;
    } catch (...) {                     // all or nothing: a failed first upload leaves the batch without a mask
        (void)hipStreamSynchronize(b->stream);
        b->dfree(pm); b->dfree(S); b->dfree(D); b->dfree(Dslab); b->dfree(dbounds); b->dfree(mod);
        throw;
    }
    b->Pm = pm; b->pres_S = S; b->pres_D = D; b->pres_Dslab = Dslab; b->pres_dbounds = dbounds; b->pres_mod = mod;
    std::copy(col_bounds, col_bounds + n_mod + 1, b->pres_bounds);
    b->pres_M = n_mod;
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
        use(b);
        if (cap < 0) fail(KLNMF_ERR_ARG, "n, f, k must be positive");
        set_problem(b, n, f, k, cap > 0 ? cap : 1);
    });
}

int klnmf_batch_upload_V(klnmf_batch *b, int p, const void *src, int dtype, int64_t rows, int64_t cols, int64_t ld, int64_t row0,
                         int64_t col0, double scale) {
    return guarded([&] {
        need_p(b, p);
        if (!src) fail(KLNMF_ERR_ARG, "null source");
        check_dtype(dtype);
        check_block(b, rows, cols, ld, row0, col0);
        if (rows * cols == 0) return;
        // through a bounded device staging buffer, as klnmf_upload_V
        const size_t es = dtype == KLNMF_DT_F64 ? 8 : 4;
        const int64_t rows_per = std::min(rows, std::max<int64_t>(1, (int64_t)((256ull << 20) / (es * (size_t)ld))));
        void *d = nullptr;
        HIPCHK(hipMalloc(&d, (size_t)rows_per * ld * es + 16));
        try {
            for (int64_t r0 = 0; r0 < rows; r0 += rows_per) {
                const int64_t rr = std::min(rows_per, rows - r0);
                HIPCHK(hipMemcpyAsync(d, (const char *)src + (size_t)r0 * ld * es, ((size_t)(rr - 1) * ld + cols) * es,
                                      hipMemcpyHostToDevice, b->stream));
                place_block(b, p, d, dtype, nullptr, rr, cols, ld, row0 + r0, col0, scale);
                HIPCHK(hipStreamSynchronize(b->stream));
            }
        } catch (...) {
            (void)hipFree(d);
            throw;
        }
        (void)hipFree(d);
    });
}

int klnmf_batch_upload_V_device_rows_dt(klnmf_batch *b, int p, const void *dsrc, int dtype, const int64_t *drow_idx, int64_t rows,
                                        int64_t cols, int64_t ld, int64_t row0, int64_t col0, double scale) {
    return guarded([&] {
        need_p(b, p);
        if (!dsrc) fail(KLNMF_ERR_ARG, "null source");
        check_dtype(dtype);
        check_block(b, rows, cols, ld, row0, col0);
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
        copy_2d_any(b, H, b->prec == KLNMF_PREC_F64, b->f, dsrc, dtype == KLNMF_DT_F64, ld, b->k, ncols);
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
        BATCH_CALL(b, batch_W, b->V, 0);
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
        copy_2d_any(b, ddst, dtype == KLNMF_DT_F64, ld, problem_ptr(b, b->W[b->cur], p, b->n * b->k), b->prec == KLNMF_PREC_F64, b->k, b->n, b->k);
        HIPCHK(hipStreamSynchronize(b->stream));
    });
}

int klnmf_batch_query(klnmf_batch *b, int what, int64_t *value) {
    return guarded([&] {
        use(b);
        if (!value) fail(KLNMF_ERR_ARG, "null destination");
        if (what == KLNMF_Q_BATCH_COUNT) { *value = b->count; return; }
        if (what == KLNMF_Q_PRESENCE) { *value = (b->have_problem && b->presence()) ? b->pres_M : 0; return; }
        if (what != KLNMF_Q_EX_ROW_CHUNKS && what != KLNMF_Q_EX_W_CHUNKS && what != KLNMF_Q_EX_H_SEGMENTS && what != KLNMF_Q_EX_H_FROM_SLABS)
            fail(KLNMF_ERR_ARG, "klnmf_batch_query: unknown item");
        if (!b->have_problem) { *value = 0; return; }
        plan_answer(b->plan, what, value);
    });
}

// ---- klnmf_batch_mask.h --------------------------------------------------------------------------------------------------------
// klnmf_upload_presence for problem p: P_p[row0 + i, m] = src[i, m], cast and placed by k_place_V on problem p's n x M matrix
int klnmf_batch_upload_presence(klnmf_batch *b, int p, const void *src, int dtype, int64_t rows, int64_t ld, int64_t row0,
                                const int64_t *col_bounds, int n_mod) {
    return guarded([&] {
        need_p(b, p);
        const std::string who = "klnmf_batch_upload_presence";
        if (!src) fail(KLNMF_ERR_ARG, "null source");
        check_dtype(dtype);
        batch_presence_check(b, who, rows, row0, ld >= n_mod, col_bounds, n_mod);
        const int64_t M = n_mod;
        batch_presence_take(b, col_bounds, n_mod);
        if (rows == 0) return;
        const size_t ses = dtype == KLNMF_DT_F64 ? 8 : 4;
        int64_t rows_per = (int64_t)((256ull << 20) / (ses * (size_t)ld));
        rows_per = std::max<int64_t>(1, std::min(rows_per, rows));
        void *P = problem_ptr(b, b->Pm, p, b->n * M);
        void *d = nullptr;
        HIPCHK(hipMalloc(&d, (size_t)rows_per * ld * ses + 16));
        try {
            for (int64_t r0 = 0; r0 < rows; r0 += rows_per) {
                const int64_t rr = std::min(rows_per, rows - r0);
                HIPCHK(hipMemcpyAsync(d, (const char *)src + (size_t)r0 * ld * ses, ((size_t)(rr - 1) * ld + M) * ses,
                                      hipMemcpyHostToDevice, b->stream));
                const int grid = grid_for(rr * M, 256, 8192);
                const int64_t *no_idx = nullptr;
#define KL_PLACE_P(T, S) hipLaunchKernelGGL((k_place_V<T, S>), dim3(grid), dim3(256), 0, b->stream, (T *)P, M, (const S *)d, rr, M, ld, \
                                            row0 + r0, (int64_t)0, 1.0, no_idx)
                if (b->prec == KLNMF_PREC_F64) { if (dtype == KLNMF_DT_F64) KL_PLACE_P(double, double); else KL_PLACE_P(double, float); }
                else { if (dtype == KLNMF_DT_F64) KL_PLACE_P(float, double); else KL_PLACE_P(float, float); }
#undef KL_PLACE_P
                HIPCHK(hipGetLastError());
                HIPCHK(hipStreamSynchronize(b->stream));
            }
        } catch (...) {
            (void)hipFree(d);
            throw;
        }
        (void)hipFree(d);
    });
}

// klnmf_upload_presence_device_rows for problem p: the row indices are checked on the device first (k_presence_rows_check); the host
// reads the flag back, and only a clean flag takes the mask (a first upload) and launches the gather into problem p's P
int klnmf_batch_upload_presence_device_rows(klnmf_batch *b, int p, const void *dP, int dtype, int64_t src_rows, int64_t ld,
                                            const int64_t *drow_idx, int64_t rows, int64_t row0, const int *src_cols,
                                            const int64_t *col_bounds, int n_mod) {
    return guarded([&] {
        need_p(b, p);
        const std::string who = "klnmf_batch_upload_presence_device_rows";
        if (!dP) fail(KLNMF_ERR_ARG, "null source");
        check_dtype(dtype);
        batch_presence_check(b, who, rows, row0, ld >= 0 && src_rows >= 0 && (drow_idx || rows <= src_rows), col_bounds, n_mod);
        if (!src_cols) fail(KLNMF_ERR_ARG, who + ": null source columns");
        PresenceCols cols{};
        for (int m = 0; m < n_mod; ++m) {
            if (src_cols[m] < -1 || src_cols[m] >= ld) fail(KLNMF_ERR_ARG, who + ": a source column outside [-1, ld)");
            cols.col[m] = src_cols[m];
        }
        if (rows > 0 && drow_idx) {
            void *flag = b->dalloc(sizeof(int64_t));      // (zero-filled)
            int64_t bad = 0;
            try {
                hipLaunchKernelGGL(k_presence_rows_check, dim3(grid_for(rows, 256, kPresGatherMaxBlocks)), dim3(256), 0, b->stream, drow_idx,
                                   rows, src_rows, (int64_t *)flag);
                HIPCHK(hipGetLastError());
                HIPCHK(hipMemcpyAsync(&bad, flag, sizeof(int64_t), hipMemcpyDeviceToHost, b->stream));
                HIPCHK(hipStreamSynchronize(b->stream));
            } catch (...) {
                (void)hipStreamSynchronize(b->stream);
                b->dfree(flag);
                throw;
            }
            b->dfree(flag);
            if (bad) fail(KLNMF_ERR_ARG, who + ": a row index outside [0, src_rows)");
        }
        batch_presence_take(b, col_bounds, n_mod);
        if (rows == 0) return;
        // every index is a source row, every column one of its ld, and row0 + rows <= n: the gather reads and writes in range
        void *P = problem_ptr(b, b->Pm, p, b->n * n_mod);
        const int grid = grid_for(rows, 256, kPresGatherMaxBlocks);
#define KL_GATHER_P(T, S) hipLaunchKernelGGL((k_presence_gather<T, S>), dim3(grid), dim3(256), 0, b->stream, (T *)P, n_mod, (const S *)dP, ld, \
                                             drow_idx, rows, row0, cols)
        if (b->prec == KLNMF_PREC_F64) { if (dtype == KLNMF_DT_F64) KL_GATHER_P(double, double); else KL_GATHER_P(double, float); }
        else { if (dtype == KLNMF_DT_F64) KL_GATHER_P(float, double); else KL_GATHER_P(float, float); }
#undef KL_GATHER_P
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(b->stream));      // (dP and drow_idx are the caller's: free to go from here)
    });
}

// the batch runs the unmasked kernels again
int klnmf_batch_clear_presence(klnmf_batch *b) {
    return guarded([&] {
        need_problem(b);
        if (!b->presence()) return;
        HIPCHK(hipStreamSynchronize(b->stream));
        b->dfree(b->Pm); b->dfree(b->pres_S); b->dfree(b->pres_D); b->dfree(b->pres_Dslab); b->dfree(b->pres_dbounds); b->dfree(b->pres_mod);
        b->forget_presence();
    });
}

}  // extern "C"
