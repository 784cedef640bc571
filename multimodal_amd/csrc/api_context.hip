// libklnmf.so, unit 1 of 6: contexts, problems, uploads and downloads (ctx.hip.h lists the units).
#include "ctx.hip.h"
#include "csc.hip.h"
#include "csrgather.hip.h"

DevBlockCache g_block_cache;

namespace {

void fast_pack_W(klnmf_ctx *c) {
    hipLaunchKernelGGL(k_pack_W, dim3(grid_for(c->n_pad * c->KP, 256, 8192)), dim3(256), 0,
                       c->stream, (const float *)c->W32[c->cur], c->Wb[c->cur], c->n_pad, c->KP,
                       w_ld(c->KP), c->kc, (const float *)c->tcur);
    HIPCHK(hipGetLastError());
}

// Both images of the current (W, H) with scales MEASURED from W's column maxima (a W that no W rule produced: W0 = V.H0^T,
// klnmf_set_W -- see opnd_t in mfma.hip.h).  They are valid for one update; the update's W rule packs the next W image
// with the hs-based / row-normalised scale again.
// eps through the matrix product (kc >= 0, k_update_pack_H) is the pair "W image column kc = 2^-10, dictionary image row kc =
// eps x c x 2^10" (c = the storage factor of V, a power of two fixed by klnmf_set_v_max).  Both must be fp16 numbers: with
// max(V) below 5e-6 the row value passes 65504 (round 4's data fuzz: V x 1e-6, k = 40 -- eps came out 25 % small, the losses
// 4 % off), with max(V) above ~1e7 it underflows to 0 and the padded rows of the last row tile divide 0 by 0 (V x 1e6,
// 70 000 rows: NaN).  Outside [2^-20, 2^15] -- max(V) outside about [1e-5, 3e5] -- the carrier is dropped and the kernels add
// eps in their fp32 epilogue (the EP = 0 instantiations every shape has; one more VALU instruction per element).  Below
// 2^-14 the row value is a subnormal half (at 2^-20: 16 steps, eps good to 3 %): V is then 1e11 times eps and more, and all
// that is asked of eps is to keep 0 / 0 out of the empty rows.
void choose_eps_carrier(klnmf_ctx *c) {
    const double ev = kEpsRatio * c->v_scale / (double)kCarrierW;
    const bool fits = ev >= 9.5367431640625e-07 && ev <= 32768.0;
    c->kc = (c->kc_shape >= 0 && fits) ? c->kc_shape : -1;
}

// ------------------------------------------------------------- loop pieces ---
// Empty V tile buffers: true zeros (padding rows and columns are inert; an all-zero row of V gives an exactly zero row of W,
// as in the reference -- also under the update pass without the numerator's eps, whose ratio carries a 2^-100 addend instead
// of relying on a stored "zero class": mfma4.hip.h, NE).
void fill_v_tiles(klnmf_ctx *c, void *tiles, size_t bytes) {
    HIPCHK(hipMemsetAsync(tiles, 0, bytes, c->stream));
}

// ---------------------------------------------------------------- uploads ---
// `om` (a weighted problem's weights, exact modes): the block goes to Om instead of V, and V's upload state is left alone
void place_block(klnmf_ctx *c, const void *dsrc, bool s64, int64_t rows, int64_t cols, int64_t ld, int64_t row0, int64_t col0,
                 double scale, const int64_t *row_idx = nullptr, bool om = false) {
    if (c->is_exact()) {
        place_rows(c->stream, om ? c->Om : c->V, c->prec == KLNMF_PREC_F64, c->f, dsrc, s64, rows, cols, ld, row0, col0, scale, row_idx);
    } else {
        dispatch_type(s64, [&](auto st) {
            typedef tag_t<decltype(st)> S;
            hipLaunchKernelGGL((k_tile_V<S>), dim3(grid_for(rows * cols, 256, 8192)), dim3(256), 0, c->stream, (_Float16 *)c->VtA, c->nrt,
                               c->nct, (const S *)dsrc, rows, cols, ld, row0, col0, scale * c->v_scale, c->st, row_idx,
                               kEpsRatio * c->v_scale);
        });
        HIPCHK(hipGetLastError());
    }
    if (om) return;
    c->v_uploaded = true;
    c->refusals_dirty = true;
}

// a host block [rows, cols] (leading dimension ld) into V (or Om) through the bounded staging buffer
void upload_block(klnmf_ctx *c, const void *src, int dtype, int64_t rows, int64_t cols, int64_t ld, int64_t row0, int64_t col0,
                  double scale, bool om) {
    staged_upload(c->stream, src, dt_size(dtype), rows, cols, ld, [&](const void *d, int64_t r0, int64_t rr) {
        place_block(c, d, dtype == KLNMF_DT_F64, rr, cols, ld, row0 + r0, col0, scale, nullptr, om);
    });
}

// dense [rows,cols] host array -> device array of the context's element type / padded fp32
void set_matrix(klnmf_ctx *c, const void *src, int dtype, int64_t rows, int64_t cols, void *exact_dst,
                float *fast_dst, int64_t fast_ld, double mul = 1.0) {
    const int64_t count = rows * cols;
    void *d = stage_to_device(c, src, dtype, count);
    const dim3 grid(grid_for(count, 256, 8192));
    if (c->is_exact()) {
        dispatch_types(c->prec == KLNMF_PREC_F64, dtype == KLNMF_DT_F64, [&](auto dt, auto st) {
            typedef tag_t<decltype(dt)> D;
            typedef tag_t<decltype(st)> S;
            hipLaunchKernelGGL((k_convert<D, S>), grid, dim3(256), 0, c->stream, (D *)exact_dst, (const S *)d, count);
        });
    } else {
        dispatch_type(dtype == KLNMF_DT_F64, [&](auto st) {
            typedef tag_t<decltype(st)> S;
            hipLaunchKernelGGL((k_place_padded<S>), grid, dim3(256), 0, c->stream, fast_dst, fast_ld, (const S *)d, rows, cols, mul);
        });
    }
    hipError_t e = hipGetLastError();
    HIPCHK(hipStreamSynchronize(c->stream));
    (void)hipFree(d);
    HIPCHK(e);
}

void get_matrix(klnmf_ctx *c, void *dst, int dtype, int64_t rows, int64_t cols, const void *exact_src,
                const float *fast_src, int64_t fast_ld, double mul = 1.0) {
    const int64_t count = rows * cols;
    void *d = nullptr;
    const size_t bytes = (size_t)count * dt_size(dtype);
    HIPCHK(hipMalloc(&d, bytes ? bytes : 16));
    const dim3 grid(grid_for(count, 256, 8192));
    if (c->is_exact()) {
        dispatch_types(dtype == KLNMF_DT_F64, c->prec == KLNMF_PREC_F64, [&](auto dt, auto st) {
            typedef tag_t<decltype(dt)> D;
            typedef tag_t<decltype(st)> S;
            hipLaunchKernelGGL((k_convert<D, S>), grid, dim3(256), 0, c->stream, (D *)d, (const S *)exact_src, count);
        });
    } else {
        dispatch_type(dtype == KLNMF_DT_F64, [&](auto dt) {
            typedef tag_t<decltype(dt)> D;
            hipLaunchKernelGGL((k_gather_padded<D>), grid, dim3(256), 0, c->stream, (D *)d, fast_src, fast_ld, rows, cols, mul);
        });
    }
    hipError_t e = hipGetLastError();
    hipError_t e2 = hipMemcpyAsync(dst, d, bytes, hipMemcpyDeviceToHost, c->stream);
    hipError_t e3 = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    HIPCHK(e);
    HIPCHK(e2);
    HIPCHK(e3);
}

// ------------------------------------------------------------ a new problem ---
// [count] floats `value` into each of `dsts`
void fill_floats(klnmf_ctx *c, std::initializer_list<float *> dsts, int count, float value) {
    const std::vector<float> v((size_t)count, value);
    for (float *d : dsts) HIPCHK(hipMemcpyAsync(d, v.data(), v.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
}

// The buffers of a dense problem in the exact modes, as the plan sizes them.  (The order of the dalloc calls is kept in all three
// functions: the block cache hands blocks out by size class.)
void alloc_dense_exact(klnmf_ctx *c) {
    const size_t es = c->esize(), n = (size_t)c->n, f = (size_t)c->f, k = (size_t)c->k;
    c->loss_red = (double2 *)c->dalloc(sizeof(double2) * kLossRedMax);
    c->V = c->dalloc(n * f * es);
    c->Q = c->dalloc(n * f * es);
    for (void *&w : c->W) w = c->dalloc(n * k * es);
    c->H = c->dalloc(k * f * es);
    c->Npart = c->dalloc((size_t)c->nsplit * k * f * es);
    if (c->hseg_n > 1) c->hpart = (double *)c->dalloc(sizeof(double) * k * c->hseg_n);
    c->numer = c->dalloc(k * f * es);
    if (c->wsplit > 1) c->Wpart = c->dalloc((size_t)c->wsplit * n * k * es);
    c->loss_part = (double *)c->dalloc(sizeof(double) * c->loss_part_count);
    if (c->x3_fused()) {
        c->x3_hs = (float *)c->dalloc(sizeof(float) * F3_KMAX);
        c->x3_xmax = (unsigned *)c->dalloc(sizeof(unsigned) * F3_KMAX);
        c->x3_qr = (float *)c->dalloc(sizeof(float) * n);
        c->x3_loss = (double *)c->dalloc(sizeof(double) * ((n + F3_TR - 1) / F3_TR));
    }
}

// ... in the 16-bit mode, with unit scales until a dictionary is packed / an e4m3 image is measured
void alloc_dense_16(klnmf_ctx *c) {
    const size_t kp4 = (size_t)c->KP * 4;
    c->loss_red = (double2 *)c->dalloc(sizeof(double2) * kLossRedMax);
    c->VtA = c->dalloc(c->v_bytes);      // (true zeros: fill_v_tiles)
    c->Qt = (unsigned char *)c->dalloc(c->qt_bytes);
    if (c->q8_ok) c->q8_list = (uint2 *)c->dalloc(sizeof(uint2) * kQ8ListCap);
    if (c->w8) {
        c->W8 = (unsigned char *)c->dalloc(c->w8_bytes);
        c->w8s = (float *)c->dalloc(kp4);
        fill_floats(c, {c->w8s}, c->KP, 256.f);
    }
    for (int i = 0; i < 2; ++i) {
        c->W32[i] = (float *)c->dalloc(c->w32_bytes);
        c->Wb[i] = (opnd_t *)c->dalloc(c->wb_bytes);
    }
    c->H32 = (float *)c->dalloc(c->h32_bytes);
    c->Ht4 = (opnd_t *)c->dalloc(c->ht4_bytes);
    choose_eps_carrier(c);
    c->hsum = (double *)c->dalloc((size_t)c->KP * 8);
    for (float **t : {&c->tcur, &c->t_hs, &c->t_unit}) *t = (float *)c->dalloc(kp4);
    c->wmax = (unsigned *)c->dalloc(kp4);
    fill_floats(c, {c->tcur, c->t_hs, c->t_unit}, c->KP, kOpScaleW);      // until a dictionary is packed (k_update_pack_H)
    c->NpartF = (float *)c->dalloc(c->npartF_bytes);
    c->numerF = (float *)c->dalloc(c->numerF_bytes);
    c->H32alt = (float *)c->dalloc(c->h32_bytes);
    if (c->W8) {
        c->w8tab = (unsigned *)c->dalloc((size_t)kW8TabRows * kp4);      // (zero-filled)
        c->w8s_next = (float *)c->dalloc(kp4);
        HIPCHK(hipMemcpyAsync(c->w8s_next, c->w8s, kp4, hipMemcpyDeviceToDevice, c->stream));
    }
    if (c->q8_ok) {      // the fp8 monitor (monitor.hip.h)
        c->mon_part = (float *)c->dalloc((size_t)kMonBlocks * 2 * 2 * c->KP * 32 * 4);
        c->mon_spread = (float *)c->dalloc((size_t)2 * kMonBlocks * 96 * 4);
    }
    if (c->gpart_bytes) c->Gpart = (float *)c->dalloc(c->gpart_bytes);
    c->loss_part2 = (double2 *)c->dalloc(c->loss_part2_bytes);
}

// ... of a CSR problem
void alloc_csr(klnmf_ctx *c) {
    const size_t es = c->esize(), n = (size_t)c->n, f = (size_t)c->f, k = (size_t)c->k, nnz = (size_t)c->nnz, nz1 = nnz > 0 ? nnz : 1;
    for (void *&w : c->W) w = c->dalloc(n * k * es);
    c->H = c->dalloc(k * f * es);
    c->HT = c->dalloc(k * f * es);
    c->numer = c->dalloc(k * f * es);
    c->sp_indptr = (int64_t *)c->dalloc(sizeof(int64_t) * (n + 1));
    c->sp_indices = (int64_t *)c->dalloc(sizeof(int64_t) * nz1);
    c->csc_indptr = (int64_t *)c->dalloc(sizeof(int64_t) * (f + 1));
    c->csc_rows = (int64_t *)c->dalloc(sizeof(int64_t) * nz1);
    c->csc_perm = (int64_t *)c->dalloc(sizeof(int64_t) * nz1);
    c->csc_work = (int64_t *)c->dalloc(sizeof(int64_t) * CscWork(c->nnz).elems);
    c->sp_data = c->dalloc(nz1 * es);
    c->sp_q = c->dalloc(nz1 * es);
    c->sp_row_loss = (double *)c->dalloc(sizeof(double) * n);
    if (c->hseg_n > 1) c->hpart = (double *)c->dalloc(sizeof(double) * k * c->hseg_n);
    c->sp_wpart = (double *)c->dalloc(sizeof(double) * c->sp_nblk * k);
    c->sp_prod = (double *)c->dalloc(sizeof(double) * k);
    if (!c->sp_blocked) return;
    c->sp_idx32 = (int *)c->dalloc(sizeof(int) * nnz);
    c->csc_rows32 = (int *)c->dalloc(sizeof(int) * nnz);
    c->csc_perm32 = (int *)c->dalloc(sizeof(int) * nnz);
    c->sp_blkptr = (int64_t *)c->dalloc(sizeof(int64_t) * n * (c->sp_cb + 1));
    c->csc_blkptr = (int64_t *)c->dalloc(sizeof(int64_t) * f * (c->sp_rb + 1));
    c->sp_loss_part = (double *)c->dalloc(sizeof(double) * (size_t)c->sp_cb * n);
    c->sp_G = c->dalloc((size_t)c->sp_cb * n * k * es);
    c->sp_NT = c->dalloc((size_t)c->sp_rb * f * k * es);
    c->sp_bad = (int *)c->dalloc(sizeof(int));
}

// What klnmf_set_problem and klnmf_set_problem_sparse (nnz >= 0) do.  The plan of the shape first (plan.hip.h): what it refuses is
// refused before anything is touched -- except where it says that the previous problem goes first.  Then the previous problem
// is released (free_all: ProblemState back to its defaults), the plan and the switches it was made with are stored, and the
// buffers it sizes are taken.
void set_problem(klnmf_ctx *c, int64_t n, int64_t f, int64_t k, int64_t cap, int64_t nnz) {
    const DevSwitches sw = problem_switches();
    const ProblemPlan plan = plan_problem(c->prec, n, f, k, nnz, c->cu_count, sw);
    if (plan.refuse != KLNMF_OK && !plan.refuse_releases) fail(plan.refuse, plan.refuse_msg);
    HIPCHK(hipStreamSynchronize(c->stream));
    c->free_all();
    if (plan.refuse != KLNMF_OK) fail(plan.refuse, plan.refuse_msg);
    static_cast<ProblemPlan &>(*c) = plan;
    c->sw = sw;
    c->cap = cap;
    c->st = (DevState *)c->dalloc(sizeof(DevState));
    c->errors = (double *)c->dalloc(sizeof(double) * (cap > 0 ? cap : 1));
    c->loss_xchg = (double *)c->dalloc(sizeof(double) * 2);
    if (c->sparse) alloc_csr(c);
    else if (c->is_exact()) alloc_dense_exact(c);
    else alloc_dense_16(c);
    reset_state(c);
    HIPCHK(hipStreamSynchronize(c->stream));
    c->have_problem = true;
}

}  // namespace

namespace klnmf_host {

// the development switches as a new problem reads them (klnmf_set_problem*, klnmf_batch_set_problem)
DevSwitches problem_switches() { return DevSwitches::read(); }

void reset_state(klnmf_ctx *c) {
    hipLaunchKernelGGL(k_reset_state, dim3(1), dim3(1), 0, c->stream, c->st);
    HIPCHK(hipGetLastError());
}

void fast_pack_H(klnmf_ctx *c, const unsigned *wmax) {
    // the dictionary's fp16 tile images, row sums and image scales from its fp32 master (no update: the H rule of a loop runs in
    // k_post).  One block per component row; its passes over the row are a chain of memory round trips, so a long row gets more
    // threads (fewer elements per thread and pass)
    const int hthreads = c->f_pad >= 4096 ? 1024 : (c->f_pad >= 2048 ? 512 : 256);
    hipLaunchKernelGGL(k_update_pack_H, dim3((unsigned)c->k), dim3(hthreads), 0, c->stream, c->H32, (const float *)c->numerF,
                       c->Ht4, c->hsum, c->tcur, c->t_hs, wmax, &c->st->op_range, c->f, c->f_pad, c->KP, 0,
                       (const DevState *)nullptr, c->kc, (float)(kEpsRatio * c->v_scale), 0, (int64_t)c->KP * c->f_pad,
                       wmax ? (const DevState *)c->st : (const DevState *)nullptr);      // measured images carry DevState.cq_e
    HIPCHK(hipGetLastError());
    c->images_measured = wmax != nullptr;
}

// from_init: W is W0 = V.H0^T of klnmf_init_W -- the first update's ratios are about f / k times 1, and the dictionary image
// then carries the ratio scale k_ratio_scale derives (mfma.hip.h; KLNMF_RATIO_SCALE=0: never); any other W: scale 1.
void measure_and_pack(klnmf_ctx *c, bool from_init) {
    c->refusals_dirty = true;
    const bool cq_ok = c->sw.ratio_scale;
    // (the eps row of the image is scaled too: it must stay an fp16 number)
    int e_cap = 12;
    if (c->kc >= 0) {
        const double ev = kEpsRatio * c->v_scale / (double)kCarrierW;
        int ex = 0;
        (void)std::frexp(32768.0 / ev, &ex);
        e_cap = std::min(12, std::max(0, ex - 1));
    }
    hipLaunchKernelGGL(k_ratio_scale, dim3(1), dim3(256), 0, c->stream, (const double *)c->hsum, (const float *)c->tcur, (int)c->k, c->f,
                       c->st, from_init && cq_ok ? 1 : 0, e_cap);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(c->wmax, 0, (size_t)c->KP * 4, c->stream));
    HIPCHK(hipMemsetAsync(&c->st->op_range, 0, sizeof(int), c->stream));
    const int rows_grid = (int)std::min<int64_t>(c->n_pad, 1024);
    hipLaunchKernelGGL(k_colmax_W, dim3(rows_grid, (c->KP + 255) / 256), dim3(256), 0, c->stream,
                       (const float *)c->W32[c->cur], c->n_pad, c->KP, c->wmax);
    HIPCHK(hipGetLastError());
    fast_pack_H(c, c->wmax);
    fast_pack_W(c);
}

size_t dt_size(int dtype) {
    check_dtype(dtype, "unknown dtype");
    return dtype == KLNMF_DT_F64 ? 8 : 4;
}

// host [rows,cols] (dtype) -> device staging buffer; returns device pointer (freed by caller)
void *stage_to_device(klnmf_ctx *c, const void *src, int dtype, int64_t count) {
    void *d = nullptr;
    const size_t bytes = (size_t)count * dt_size(dtype);
    HIPCHK(hipMalloc(&d, bytes ? bytes : 16));
    hipError_t e = hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) {
        (void)hipFree(d);
        fail(KLNMF_ERR_HIP, std::string("hipMemcpyAsync H2D: ") + hipGetErrorString(e));
    }
    return d;
}

// ---- what contexts and batches share (ctx.hip.h) -------------------------------------------------------------------------------
void place_rows(hipStream_t stream, void *dst, bool d64, int64_t dld, const void *dsrc, bool s64, int64_t rows, int64_t cols, int64_t ld,
                int64_t row0, int64_t col0, double scale, const int64_t *row_idx) {
    const dim3 grid(grid_for(rows * cols, 256, 8192));
    dispatch_types(d64, s64, [&](auto dt, auto st) {
        typedef tag_t<decltype(dt)> T;
        typedef tag_t<decltype(st)> S;
        hipLaunchKernelGGL((k_place_V<T, S>), grid, dim3(256), 0, stream, (T *)dst, dld, (const S *)dsrc, rows, cols, ld, row0, col0, scale,
                           row_idx);
    });
    HIPCHK(hipGetLastError());
}

void copy_2d_any(hipStream_t stream, void *dst, bool d64, int64_t dld, const void *src, bool s64, int64_t sld, int64_t rows, int64_t cols,
                 double mul) {
    if (rows * cols == 0) return;
    const dim3 grid(grid_for(rows * cols, 256, 8192));
    dispatch_types(d64, s64, [&](auto dt, auto st) {
        typedef tag_t<decltype(dt)> D;
        typedef tag_t<decltype(st)> S;
        hipLaunchKernelGGL((k_copy_2d<D, S>), grid, dim3(256), 0, stream, (D *)dst, dld, (const S *)src, sld, rows, cols, mul);
    });
    HIPCHK(hipGetLastError());
}

void fill_ones(hipStream_t stream, void *dst, bool f64, int64_t count) {
    dispatch_type(f64, [&](auto t) {
        typedef tag_t<decltype(t)> T;
        hipLaunchKernelGGL((k_fill<T>), dim3(grid_for(count, 256, 8192)), dim3(256), 0, stream, (T *)dst, count, (T)1);
    });
    HIPCHK(hipGetLastError());
}

// `rows_ok`: the caller's own part of "rows out of range" (the source's leading dimension)
void presence_check_args(const std::string &who, const MaskDims &d, int64_t rows, int64_t row0, bool rows_ok, const int64_t *col_bounds,
                         int n_mod) {
    if (n_mod < 1 || n_mod > KLNMF_MAX_MODALITIES)
        fail(KLNMF_ERR_ARG, who + ": 1 <= n_mod <= KLNMF_MAX_MODALITIES (" + std::to_string(KLNMF_MAX_MODALITIES) + ")");
    if (!col_bounds) fail(KLNMF_ERR_ARG, who + ": null column bounds");
    if (col_bounds[0] != 0 || col_bounds[n_mod] != d.f) fail(KLNMF_ERR_ARG, who + ": the column bounds must run from 0 to f");
    for (int m = 0; m < n_mod; ++m)
        if (col_bounds[m] >= col_bounds[m + 1]) fail(KLNMF_ERR_ARG, who + ": the column bounds must increase strictly");
    if (rows < 0 || row0 < 0 || row0 + rows > d.n || !rows_ok) fail(KLNMF_ERR_ARG, who + ": rows out of range");
}
// ... and, last of the checks, against a mask that is held: `owner` is "problem" or "batch"
void presence_check_bounds(const PresenceState &ps, const std::string &who, const char *owner, const int64_t *col_bounds, int n_mod) {
    if (ps.presence() && (n_mod != ps.pres_M || !std::equal(col_bounds, col_bounds + n_mod + 1, ps.pres_bounds)))
        fail(KLNMF_ERR_ARG, who + ": the column bounds differ from the ones the " + owner + "'s first upload fixed");
}

// The first mask upload: every problem's P filled with 1 (taken without the zero-fill: k_fill writes all of it), S, D, D's slabs, and
// once for all the bounds and the per-column modality bytes.  All or nothing; an owner that holds a mask already is left alone.
void presence_take(DeviceBlocks &a, PresenceState &ps, const MaskDims &d, const int64_t *col_bounds, int n_mod) {
    if (ps.presence()) return;
    const size_t es = prec_esize(d.prec), B = (size_t)d.B;
    const int64_t M = n_mod;
    HIPCHK(hipStreamSynchronize(a.stream));
    PresenceState t;
    try {
        t.pres_dchunks = presence_d_chunks(d.n);
        t.Pm = a.dalloc(B * (size_t)(d.n * M) * es, false);
        t.pres_S = a.dalloc(B * (size_t)(M * d.k) * es);
        t.pres_D = a.dalloc(B * (size_t)(d.k * M) * es);
        t.pres_Dslab = a.dalloc(B * (size_t)t.pres_dchunks * (size_t)(d.k * M) * sizeof(double));
        t.pres_dbounds = a.dalloc((size_t)(M + 1) * sizeof(int64_t));
        t.pres_mod = a.dalloc((size_t)d.f);
        std::vector<unsigned char> mod((size_t)d.f);
        for (int m = 0; m < n_mod; ++m) std::fill(mod.begin() + col_bounds[m], mod.begin() + col_bounds[m + 1], (unsigned char)m);
        HIPCHK(hipMemcpyAsync(t.pres_mod, mod.data(), mod.size(), hipMemcpyHostToDevice, a.stream));
        HIPCHK(hipMemcpyAsync(t.pres_dbounds, col_bounds, (size_t)(M + 1) * sizeof(int64_t), hipMemcpyHostToDevice, a.stream));
        fill_ones(a.stream, t.Pm, d.prec == KLNMF_PREC_F64, (int64_t)B * d.n * M);
        HIPCHK(hipStreamSynchronize(a.stream));      // (the host images above are read by the copies until here)
    } catch (...) {                     // all or nothing: a failed first upload leaves the owner without a mask
        (void)hipStreamSynchronize(a.stream);
        for (void **b : {&t.Pm, &t.pres_S, &t.pres_D, &t.pres_Dslab, &t.pres_dbounds, &t.pres_mod}) a.dfree(*b);
        throw;
    }
    std::copy(col_bounds, col_bounds + n_mod + 1, t.pres_bounds);
    t.pres_M = n_mod;
    ps = t;
}

static void *presence_of(const PresenceState &ps, const MaskDims &d, int p) {
    return (char *)ps.Pm + (size_t)p * (size_t)(d.n * ps.pres_M) * prec_esize(d.prec);
}

// P_p[row0 + i, m] = src[i, m] from the host: the rows through the bounded staging buffer, cast and placed by k_place_V on problem
// p's n x M matrix
void presence_upload(DeviceBlocks &a, PresenceState &ps, const MaskDims &d, int p, const void *src, int dtype, int64_t rows, int64_t ld,
                     int64_t row0) {
    const int64_t M = ps.pres_M;
    staged_upload(a.stream, src, dt_size(dtype), rows, M, ld, [&](const void *chunk, int64_t r0, int64_t rr) {
        place_rows(a.stream, presence_of(ps, d, p), d.prec == KLNMF_PREC_F64, M, chunk, dtype == KLNMF_DT_F64, rr, M, ld, row0 + r0, 0, 1.0,
                   nullptr);
    });
}

// The row indices of a device-side upload, checked on the device (k_presence_rows_check; the pattern of k_csrg_len): the host reads
// the flag back and refuses before anything is taken or written.
void presence_rows_check(DeviceBlocks &a, const std::string &who, const int64_t *drow_idx, int64_t rows, int64_t src_rows) {
    void *flag = a.dalloc(sizeof(int64_t));      // (zero-filled)
    int64_t bad = 0;
    try {
        hipLaunchKernelGGL(k_presence_rows_check, dim3(grid_for(rows, 256, kPresGatherMaxBlocks)), dim3(256), 0, a.stream, drow_idx, rows,
                           src_rows, (int64_t *)flag);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&bad, flag, sizeof(int64_t), hipMemcpyDeviceToHost, a.stream));
        HIPCHK(hipStreamSynchronize(a.stream));
    } catch (...) {
        (void)hipStreamSynchronize(a.stream);
        a.dfree(flag);
        throw;
    }
    a.dfree(flag);
    if (bad) fail(KLNMF_ERR_ARG, who + ": a row index outside [0, src_rows)");
}

// P_p[row0 + i, m] = dP[drow_idx[i], cols.col[m]] (1 where the column is -1), gathered by k_presence_gather.  Callers have checked
// that every index is a source row, every column one of its ld, and row0 + rows <= n: the gather reads and writes in range
void presence_gather(DeviceBlocks &a, PresenceState &ps, const MaskDims &d, int p, const void *dP, int dtype, int64_t ld,
                     const int64_t *drow_idx, int64_t rows, int64_t row0, const PresenceCols &cols) {
    const dim3 grid(grid_for(rows, 256, kPresGatherMaxBlocks));
    dispatch_types(d.prec == KLNMF_PREC_F64, dtype == KLNMF_DT_F64, [&](auto dt, auto st) {
        typedef tag_t<decltype(dt)> T;
        typedef tag_t<decltype(st)> S;
        hipLaunchKernelGGL((k_presence_gather<T, S>), grid, dim3(256), 0, a.stream, (T *)presence_of(ps, d, p), ps.pres_M, (const S *)dP, ld,
                           drow_idx, rows, row0, cols);
    });
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(a.stream));      // (dP and drow_idx are the caller's: free to go from here)
}

// the owner runs the unmasked kernels again
void presence_drop(DeviceBlocks &a, PresenceState &ps) {
    if (!ps.presence()) return;
    HIPCHK(hipStreamSynchronize(a.stream));
    for (void **b : {&ps.Pm, &ps.pres_S, &ps.pres_D, &ps.pres_Dslab, &ps.pres_dbounds, &ps.pres_mod}) a.dfree(*b);
    ps.forget_presence();
}

}  // namespace klnmf_host

extern "C" {

int klnmf_create(klnmf_ctx **out, int device, int precision, void *stream) {
    return guarded([&] {
        if (!out) fail(KLNMF_ERR_ARG, "null out pointer");
        if (precision != KLNMF_PREC_F64 && precision != KLNMF_PREC_F32 && precision != KLNMF_PREC_F16 && precision != KLNMF_PREC_BF16X3 &&
            precision != KLNMF_PREC_F16X3)
            fail(KLNMF_ERR_ARG, "unknown precision mode");
        int ndev = 0;
        HIPCHK(hipGetDeviceCount(&ndev));
        if (device < 0 || device >= ndev) fail(KLNMF_ERR_ARG, "no such device");
        HIPCHK(hipSetDevice(device));
        hipDeviceProp_t p;
        HIPCHK(hipGetDeviceProperties(&p, device));
        if (std::strncmp(p.gcnArchName, "gfx950", 6) != 0)
            fail(KLNMF_ERR_UNSUPP, std::string("this library is built for gfx950 only, device is ") + p.gcnArchName);
        klnmf_ctx *c = new klnmf_ctx();
        c->device = device;
        c->prec = precision;
        c->cu_count = p.multiProcessorCount;
        if (stream == KLNMF_STREAM_DEFAULT) {
            c->stream = nullptr;                    // the default (null) stream
        } else if (stream) {
            c->stream = (hipStream_t)stream;
        } else {
            hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
            if (e != hipSuccess) {
                delete c;
                HIPCHK(e);
            }
            c->own_stream = true;
        }
        *out = c;
    });
}

int klnmf_destroy(klnmf_ctx *c) {
    return guarded([&] {
        if (!c) return;
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        c->free_all();
        if (c->comm || c->comm_scratch) {
            try { comm_release(c); } catch (...) {}
        }
        if (c->poll_ev) (void)hipEventDestroy(c->poll_ev);
        if (c->poll_host) (void)hipHostFree(c->poll_host);
        if (c->own_stream) (void)hipStreamDestroy(c->stream);
        delete c;
    });
}

int klnmf_set_problem(klnmf_ctx *c, int64_t n, int64_t f, int64_t k, int64_t cap) {
    return guarded([&] {
        use(c);
        if (cap < 0) fail(KLNMF_ERR_ARG, "n, f, k must be positive");
        set_problem(c, n, f, k, cap, -1);
    });
}

int klnmf_release_problem(klnmf_ctx *c) {
    return guarded([&] {
        use(c);
        HIPCHK(hipStreamSynchronize(c->stream));
        c->free_all();              // device blocks back to the per-process cache (large ones to the driver), ProblemState to its defaults
        c->profiling = false;       // (the two settings of ContextState that end with a problem: ctx.hip.h)
        c->ratio_eps = kEpsRatio;
    });
}

}  // extern "C"

namespace klnmf_host {

// The blocked regime's structures of an uploaded CSR problem (sparseb.hip.h): block pointers by binary search in the sorted rows /
// columns, int32 copies of the indices.  Refuses (`msg`) unsorted rows or columns.
void csr_blocked_setup(hipStream_t stream, const CsrParts &v, const std::string &msg) {
    if (!v.blkptr) return;
    HIPCHK(hipMemsetAsync(v.bad, 0, sizeof(int), stream));
    hipLaunchKernelGGL(k_spb_blkptr, dim3(grid_for(v.n * (v.cb + 1), 256, 1 << 20)), dim3(256), 0, stream,
                       (const int64_t *)v.indptr, (const int64_t *)v.indices, v.n, v.cb, v.cb_cols, v.blkptr, v.bad);
    hipLaunchKernelGGL(k_spb_blkptr, dim3(grid_for(v.f * (v.rb + 1), 256, 1 << 20)), dim3(256), 0, stream,
                       (const int64_t *)v.csc_indptr, (const int64_t *)v.csc_rows, v.f, v.rb, v.rb_rows, v.cblkptr, v.bad);
    hipLaunchKernelGGL(k_spb_narrow, dim3(grid_for(v.nnz, 256, 8192)), dim3(256), 0, stream, (const int64_t *)v.indices, v.idx32, v.nnz);
    hipLaunchKernelGGL(k_spb_narrow, dim3(grid_for(v.nnz, 256, 8192)), dim3(256), 0, stream, (const int64_t *)v.csc_rows, v.rows32, v.nnz);
    hipLaunchKernelGGL(k_spb_narrow, dim3(grid_for(v.nnz, 256, 8192)), dim3(256), 0, stream, (const int64_t *)v.csc_perm, v.perm32, v.nnz);
    HIPCHK(hipGetLastError());
    int bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, v.bad, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (bad) fail(KLNMF_ERR_ARG, msg);
}

int64_t csr_csc_work_elems(int64_t nnz) { return CscWork(nnz).elems; }

// A refused upload leaves every row and column of the problem empty: no kernel reads the refused indices.
void csr_leave_empty(hipStream_t stream, const CsrParts &v) {
    HIPCHK(hipMemsetAsync(v.indptr, 0, sizeof(int64_t) * (v.n + 1), stream));
    HIPCHK(hipMemsetAsync(v.csc_indptr, 0, sizeof(int64_t) * (v.f + 1), stream));
    if (v.blkptr) {
        HIPCHK(hipMemsetAsync(v.blkptr, 0, sizeof(int64_t) * v.n * (v.cb + 1), stream));
        HIPCHK(hipMemsetAsync(v.cblkptr, 0, sizeof(int64_t) * v.f * (v.rb + 1), stream));
    }
    HIPCHK(hipStreamSynchronize(stream));
}

// csc_indptr / csc_rows / csc_perm from the CSR structure already on the device (csc.hip.h), after checking it there.  Bad input is
// refused before any pass runs, and leaves every row and column of the problem empty (no kernel reads the refused indices).
void csr_csc_build(hipStream_t stream, const CsrParts &v) {
    const CscWork wk(v.nnz);
    int64_t *counts = v.csc_work, *parts = v.csc_work + wk.m, *flag = v.csc_work + wk.flag_at();
    HIPCHK(hipMemsetAsync(flag, 0, sizeof(int64_t), stream));
    hipLaunchKernelGGL(k_csc_check, dim3(grid_for(std::max(v.n, v.nnz), 256, 8192)), dim3(256), 0, stream,
                       (const int64_t *)v.indptr, (const int64_t *)v.indices, v.n, v.f, v.nnz, flag);
    HIPCHK(hipGetLastError());
    int64_t bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, flag, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (bad) {
        csr_leave_empty(stream, v);
        fail(KLNMF_ERR_ARG, "klnmf_upload_csr_rows: the row pointers must not decrease, and the column indices of every row must be "
                            "sorted and lie in [0, f)");
    }
    if (v.nnz > 0) {
        int bits = 0;
        while (bits < 62 && ((v.f - 1) >> bits) != 0) ++bits;
        const int passes = std::max(1, (bits + kCscBits - 1) / kCscBits);
        const int64_t *src = nullptr;
        for (int p = 0; p < passes; ++p) {
            // the last pass writes csc_perm; csc_rows is the other buffer until k_csc_rows fills it
            int64_t *dst = ((passes - 1 - p) & 1) == 0 ? v.csc_perm : v.csc_rows;
            const int shift = p * kCscBits;
            hipLaunchKernelGGL(k_csc_hist, dim3((unsigned)wk.tiles), dim3(kCscThreads), 0, stream, src,
                               (const int64_t *)v.indices, v.nnz, shift, wk.tiles, counts);
            hipLaunchKernelGGL(k_csc_scan_tiles, dim3((unsigned)wk.nparts), dim3(kCscThreads), 0, stream, counts, wk.m, parts);
            hipLaunchKernelGGL(k_csc_scan_part, dim3(1), dim3(kCscThreads), 0, stream, parts, wk.nparts);
            hipLaunchKernelGGL(k_csc_scan_add, dim3(grid_for(wk.m, 256, 8192)), dim3(256), 0, stream, counts, wk.m, (const int64_t *)parts);
            hipLaunchKernelGGL(k_csc_scatter, dim3((unsigned)wk.tiles), dim3(kCscThreads), 0, stream, src,
                               (const int64_t *)v.indices, v.nnz, shift, wk.tiles, (const int64_t *)counts, dst);
            HIPCHK(hipGetLastError());
            src = dst;
        }
        hipLaunchKernelGGL(k_csc_rows, dim3(grid_for(v.nnz, 256, 8192)), dim3(256), 0, stream, (const int64_t *)v.csc_perm,
                           (const int64_t *)v.indptr, v.n, v.nnz, v.csc_rows);
    }
    hipLaunchKernelGGL(k_csc_indptr, dim3(grid_for(v.f + 1, 256, 8192)), dim3(256), 0, stream, (const int64_t *)v.csc_perm,
                       (const int64_t *)v.indices, v.nnz, v.f, v.csc_indptr);
    HIPCHK(hipGetLastError());
}

// The CSR of hstack([scale[m] * X_m[rows] ...]) gathered on the device from device-resident CSR modalities (csrgather.hip.h) into
// v.indptr / v.indices / v.data.  Nothing of nnz length crosses the bus: the host reads back two words (the gathered total and the
// flag) -- before the copy kernel runs, because its stores are in range only if the total is the problem's nnz.
void csr_gather_rows(DeviceBlocks &a, const CsrParts &v, const std::string &who, int n_mod, const int64_t *const *indptr,
                     const int32_t *const *indices, const void *const *data, const int *dtype, const int64_t *col_bounds,
                     const double *scale, int64_t src_rows, const int64_t *drow_idx, int64_t rows,
                     const std::function<void()> &before_write) {
    if (n_mod < 1 || n_mod > KLNMF_MAX_MODALITIES)
        fail(KLNMF_ERR_ARG, who + ": 1 <= n_mod <= KLNMF_MAX_MODALITIES (" + std::to_string(KLNMF_MAX_MODALITIES) + ")");
    if (rows != v.n) fail(KLNMF_ERR_ARG, who + ": `rows` must be the problem's n");
    if (src_rows < 0) fail(KLNMF_ERR_ARG, who + ": src_rows < 0");
    if (!indptr || !indices || !data || !dtype || !col_bounds || !scale || !drow_idx) fail(KLNMF_ERR_ARG, who + ": null pointer");
    if (col_bounds[0] != 0 || col_bounds[n_mod] != v.f) fail(KLNMF_ERR_ARG, who + ": the column bounds must run from 0 to f");
    CsrSources S{};
    S.src_rows = src_rows;
    S.n_mod = n_mod;
    for (int m = 0; m < n_mod; ++m) {
        if (col_bounds[m] > col_bounds[m + 1]) fail(KLNMF_ERR_ARG, who + ": the column bounds must not decrease");
        if (col_bounds[m + 1] - col_bounds[m] > (int64_t)std::numeric_limits<int32_t>::max())
            fail(KLNMF_ERR_ARG, who + ": a modality of 2^31 columns or more (int32 source indices)");
        check_dtype(dtype[m], who + ": " + kDtypeMsg);
        if (!indptr[m] || (v.nnz > 0 && (!indices[m] || !data[m]))) fail(KLNMF_ERR_ARG, who + ": null pointer");
        S.indptr[m] = indptr[m];
        S.indices[m] = indices[m];
        S.data[m] = data[m];
        S.col0[m] = col_bounds[m];
        S.scale[m] = scale[m];
        if (dtype[m] == KLNMF_DT_F64) S.f64_mask |= 1u << m;
    }
    before_write();      // (every argument check is behind us: from here the problem's arrays change)
    // row lengths -> exclusive scan in place (csc.hip.h's scan: fixed order, exact integers) -> indptr
    const int64_t m1 = v.n + 1, nparts = (m1 + kCscScanTile - 1) / kCscScanTile;
    void *tmp = a.dalloc(sizeof(int64_t) * (size_t)(nparts + 1));      // the scan's tile sums, then the flag (zero-filled)
    int64_t *parts = (int64_t *)tmp, *flag = parts + nparts;
    hipLaunchKernelGGL(k_csrg_len, dim3(grid_for(m1, kCsrgThreads, 8192)), dim3(kCsrgThreads), 0, a.stream, S, drow_idx, rows,
                       v.indptr, flag);
    hipLaunchKernelGGL(k_csc_scan_tiles, dim3((unsigned)nparts), dim3(kCscThreads), 0, a.stream, v.indptr, m1, parts);
    hipLaunchKernelGGL(k_csc_scan_part, dim3(1), dim3(kCscThreads), 0, a.stream, parts, nparts);
    hipLaunchKernelGGL(k_csc_scan_add, dim3(grid_for(m1, 256, 8192)), dim3(256), 0, a.stream, v.indptr, m1, (const int64_t *)parts);
    HIPCHK(hipGetLastError());
    int64_t bad = 0, total = -1;
    HIPCHK(hipMemcpyAsync(&bad, flag, sizeof(int64_t), hipMemcpyDeviceToHost, a.stream));
    HIPCHK(hipMemcpyAsync(&total, v.indptr + v.n, sizeof(int64_t), hipMemcpyDeviceToHost, a.stream));
    HIPCHK(hipStreamSynchronize(a.stream));
    a.dfree(tmp);
    if (bad || total != v.nnz) {
        csr_leave_empty(a.stream, v);
        if (bad) fail(KLNMF_ERR_ARG, who + ": a row index outside [0, src_rows), or source row pointers that decrease");
        fail(KLNMF_ERR_ARG, who + ": the rows hold " + std::to_string(total) + " stored entries, the problem was set for " +
                            std::to_string(v.nnz));
    }
    if (v.nnz > 0) {
        const int grid = grid_for(rows * kCsrgTrip, kCsrgThreads, 1 << 16);
        if (v.prec == KLNMF_PREC_F64)
            hipLaunchKernelGGL((k_csrg_copy<double>), dim3(grid), dim3(kCsrgThreads), 0, a.stream, S, drow_idx, rows,
                               (const int64_t *)v.indptr, v.indices, (double *)v.data);
        else
            hipLaunchKernelGGL((k_csrg_copy<float>), dim3(grid), dim3(kCsrgThreads), 0, a.stream, S, drow_idx, rows,
                               (const int64_t *)v.indptr, v.indices, (float *)v.data);
        HIPCHK(hipGetLastError());
    }
}

}  // namespace klnmf_host

namespace {

// a context's CSR problem as the shared upload steps see it
CsrParts csr_parts(klnmf_ctx *c) {
    return CsrParts{c->n, c->f, c->nnz, c->prec, c->sp_indptr, c->sp_indices, c->csc_indptr, c->csc_rows, c->csc_perm, c->csc_work,
                    c->sp_data, c->sp_cb, c->sp_rb, c->sp_cb_cols, c->sp_rb_rows, c->sp_blocked ? c->sp_blkptr : nullptr, c->csc_blkptr,
                    c->sp_idx32, c->csc_rows32, c->csc_perm32, c->sp_bad};
}
void csr_blocked_setup(klnmf_ctx *c, const char *msg) { csr_blocked_setup(c->stream, csr_parts(c), msg); }
void csc_build(klnmf_ctx *c) { csr_csc_build(c->stream, csr_parts(c)); }

}  // namespace

extern "C" {

int klnmf_set_problem_sparse(klnmf_ctx *c, int64_t n, int64_t f, int64_t k, int64_t cap, int64_t nnz) {
    return guarded([&] {
        use(c);
        if (!c->is_exact()) fail(KLNMF_ERR_UNSUPP, kCsrNeedsExact);
        if (cap < 0 || nnz < 0) fail(KLNMF_ERR_ARG, "n, f, k must be positive, nnz >= 0");
        set_problem(c, n, f, k, cap, nnz);
    });
}

int klnmf_upload_csr(klnmf_ctx *c, int dtype, const int64_t *indptr, const int64_t *indices, const void *data,
                     const int64_t *csc_indptr, const int64_t *csc_rows, const int64_t *csc_perm) {
    return guarded([&] {
        need_problem(c);
        if (!c->sparse) fail(KLNMF_ERR_ARG, "klnmf_upload_csr needs klnmf_set_problem_sparse");
        if (!indptr || !csc_indptr || (c->nnz > 0 && (!indices || !data || !csc_rows || !csc_perm)))
            fail(KLNMF_ERR_ARG, "null pointer");
        check_dtype(dtype);
        if (indptr[0] != 0 || indptr[c->n] != c->nnz || csc_indptr[0] != 0 || csc_indptr[c->f] != c->nnz)
            fail(KLNMF_ERR_ARG, "index pointers do not match n, f, nnz");
        HIPCHK(hipMemcpyAsync(c->sp_indptr, indptr, sizeof(int64_t) * (c->n + 1), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->csc_indptr, csc_indptr, sizeof(int64_t) * (c->f + 1), hipMemcpyHostToDevice, c->stream));
        if (c->nnz > 0) {
            HIPCHK(hipMemcpyAsync(c->sp_indices, indices, sizeof(int64_t) * c->nnz, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(c->csc_rows, csc_rows, sizeof(int64_t) * c->nnz, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(c->csc_perm, csc_perm, sizeof(int64_t) * c->nnz, hipMemcpyHostToDevice, c->stream));
            // values: through the dense setter (dtype conversion) as a 1 x nnz matrix
            set_matrix(c, data, dtype, 1, c->nnz, c->sp_data, nullptr, 0);
        }
        csr_blocked_setup(c, "klnmf_upload_csr: the column indices of every row (and the rows of every column in the CSC arrays) must be sorted");
        HIPCHK(hipStreamSynchronize(c->stream));
        c->v_uploaded = true;
        c->refusals_dirty = true;
    });
}

int klnmf_upload_csr_rows(klnmf_ctx *c, int dtype, const int64_t *indptr, const int64_t *indices, const void *data) {
    return guarded([&] {
        need_problem(c);
        if (!c->sparse) fail(KLNMF_ERR_ARG, "klnmf_upload_csr_rows needs klnmf_set_problem_sparse");
        if (!indptr || (c->nnz > 0 && (!indices || !data))) fail(KLNMF_ERR_ARG, "null pointer");
        check_dtype(dtype);
        if (indptr[0] != 0 || indptr[c->n] != c->nnz) fail(KLNMF_ERR_ARG, "the row pointers do not match n, nnz");
        c->v_uploaded = false;
        HIPCHK(hipMemcpyAsync(c->sp_indptr, indptr, sizeof(int64_t) * (c->n + 1), hipMemcpyHostToDevice, c->stream));
        if (c->nnz > 0)
            HIPCHK(hipMemcpyAsync(c->sp_indices, indices, sizeof(int64_t) * c->nnz, hipMemcpyHostToDevice, c->stream));
        csc_build(c);
        if (c->nnz > 0) set_matrix(c, data, dtype, 1, c->nnz, c->sp_data, nullptr, 0);
        csr_blocked_setup(c, "klnmf_upload_csr_rows: the column indices of every row must be sorted");
        HIPCHK(hipStreamSynchronize(c->stream));
        c->v_uploaded = true;
        c->refusals_dirty = true;
    });
}

// The CSR of hstack([scale[m] * X_m[rows] ...]) gathered on the device from device-resident CSR modalities (csr_gather_rows), then
// the device tail of klnmf_upload_csr_rows.
int klnmf_upload_csr_device_rows(klnmf_ctx *c, int n_mod, const int64_t *const *indptr, const int32_t *const *indices,
                                 const void *const *data, const int *dtype, const int64_t *col_bounds, const double *scale,
                                 int64_t src_rows, const int64_t *drow_idx, int64_t rows) {
    return guarded([&] {
        need_problem(c);
        if (!c->sparse) fail(KLNMF_ERR_ARG, "klnmf_upload_csr_device_rows needs klnmf_set_problem_sparse");
        csr_gather_rows(*c, csr_parts(c), "klnmf_upload_csr_device_rows", n_mod, indptr, indices, data, dtype, col_bounds, scale, src_rows,
                        drow_idx, rows, [&] { c->v_uploaded = false; });
        csc_build(c);
        csr_blocked_setup(c, "klnmf_upload_csr_device_rows: the column indices of every source row must be sorted");
        HIPCHK(hipStreamSynchronize(c->stream));      // (drow_idx and the sources are the caller's: free to go from here)
        c->v_uploaded = true;
        c->refusals_dirty = true;
    });
}

// Rows drow_idx[0 .. rows) of one device-resident CSR matrix as a dense float64 device matrix (the pattern of klnmf_matmul_device:
// the device's null stream, synchronous)
int klnmf_csr_rows_to_dense_device(int device, int dtype, const int64_t *indptr, const int32_t *indices, const void *data,
                                   int64_t src_rows, const int64_t *drow_idx, int64_t rows, int64_t d, void *dout, int64_t ld) {
    return guarded([&] {
        if (rows < 0 || d < 0 || src_rows < 0 || rows > (1LL << 40) || d > (int64_t)std::numeric_limits<int32_t>::max())
            fail(KLNMF_ERR_ARG, "klnmf_csr_rows_to_dense_device: bad shape");
        check_dtype(dtype, std::string("klnmf_csr_rows_to_dense_device: ") + kDtypeMsg);
        if (rows == 0 || d == 0) return;
        if (!indptr || !drow_idx || !dout || ld < d) fail(KLNMF_ERR_ARG, "klnmf_csr_rows_to_dense_device: null pointer or short stride");
        HIPCHK(hipSetDevice(device));
        HIPCHK(hipMemset2DAsync(dout, (size_t)ld * sizeof(double), 0, (size_t)d * sizeof(double), (size_t)rows, 0));
        if (indices && data) {      // (a matrix without stored entries may come without them: the zeros are the answer)
            const int grid = grid_for(rows * kCsrgTrip, kCsrgThreads, 1 << 16);
            if (dtype == KLNMF_DT_F64)
                hipLaunchKernelGGL((k_csrg_dense<double>), dim3(grid), dim3(kCsrgThreads), 0, 0, indptr, indices, (const double *)data, src_rows,
                                   drow_idx, rows, d, (double *)dout, ld);
            else
                hipLaunchKernelGGL((k_csrg_dense<float>), dim3(grid), dim3(kCsrgThreads), 0, 0, indptr, indices, (const float *)data, src_rows,
                                   drow_idx, rows, d, (double *)dout, ld);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipStreamSynchronize(0));
    });
}

int klnmf_get_Q_values(klnmf_ctx *c, void *dst, int dtype) {
    return guarded([&] {
        need_problem(c);
        if (!c->sparse) fail(KLNMF_ERR_ARG, "klnmf_get_Q_values needs a CSR problem");
        if (!dst && c->nnz > 0) fail(KLNMF_ERR_ARG, "null destination");
        if (c->nnz > 0) get_matrix(c, dst, dtype, 1, c->nnz, c->sp_q, nullptr, 0);
    });
}

int klnmf_set_v_max(klnmf_ctx *c, double vmax) {
    return guarded([&] {
        need_problem(c);
        if (!(vmax >= 0) || !std::isfinite(vmax)) fail(KLNMF_ERR_ARG, "vmax must be finite and >= 0");
        if (c->v_uploaded) fail(KLNMF_ERR_ARG, "klnmf_set_v_max must precede the first upload");
        if (c->is_exact() || vmax == 0) {
            c->v_scale = 1.0;
            if (!c->is_exact()) choose_eps_carrier(c);
            return;
        }
        int e = 0;
        (void)std::frexp(vmax, &e);             // vmax = m * 2^e, m in [0.5, 1)
        c->v_scale = std::ldexp(1.0, 15 - e);   // c * vmax in [2^14, 2^15)
        c->v_max = vmax;
        choose_eps_carrier(c);
        if (c->kc >= 0) fast_pack_H(c);      // the eps row of the dictionary images is in scaled units
    });
}

int klnmf_reset_V(klnmf_ctx *c) {
    return guarded([&] {
        need_problem(c);
        if (c->sparse) fail(KLNMF_ERR_ARG, "klnmf_reset_V: CSR problems are re-uploaded whole (klnmf_upload_csr)");
        // the upload kernels ACCUMULATE sum(V as stored), the storage-rounding correction and the overflow count: a second
        // upload into a live context would count a block twice.  Clear the matrix and the three counters.
        if (c->is_exact()) {
            HIPCHK(hipMemsetAsync(c->V, 0, (size_t)c->n * c->f * c->esize(), c->stream));
        } else {
            fill_v_tiles(c, c->VtA, (size_t)c->nrt * c->nct * 1024 * 2);
        }
        HIPCHK(hipMemsetAsync(&c->st->sum_x, 0, sizeof(double) * 4, c->stream));         // sum_x, corr_c, corr_eps, nnz_x
        HIPCHK(hipMemsetAsync(&c->st->v_overflow, 0, sizeof(int), c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        c->v_uploaded = false;
        c->refusals_dirty = true;
    });
}

int klnmf_upload_V(klnmf_ctx *c, const void *src, int dtype, int64_t rows, int64_t cols, int64_t ld,
                   int64_t row0, int64_t col0, double scale) {
    return guarded([&] {
        need_problem(c);
        if (!src) fail(KLNMF_ERR_ARG, "null source");
        check_block(c->n, c->f, rows, cols, ld, row0, col0);
        upload_block(c, src, dtype, rows, cols, ld, row0, col0, scale, false);
    });
}

// Om[row0 + i, col0 + j] = src[i, j] (nmf.py:159-175: `weights`, which the reference documents and ignores).  The first upload
// of a problem takes the buffer filled with 1 -- a caller uploads only the blocks that carry weights -- and the denominators'
// slabs beside it; klnmf_set_problem* / klnmf_release_problem drop them with the problem (ProblemState).
int klnmf_upload_weights(klnmf_ctx *c, const void *src, int dtype, int64_t rows, int64_t cols, int64_t ld,
                         int64_t row0, int64_t col0) {
    return guarded([&] {
        need_problem(c);
        if (c->sparse) fail(KLNMF_ERR_UNSUPP, "klnmf_upload_weights: CSR problems have no weighted kernels (the ratio lives on the stored entries only)");
        if (c->prec != KLNMF_PREC_F64 && c->prec != KLNMF_PREC_F32)
            fail(KLNMF_ERR_UNSUPP, "klnmf_upload_weights: the weighted kernels exist in KLNMF_PREC_F64 and KLNMF_PREC_F32 only");
        if (!src) fail(KLNMF_ERR_ARG, "null source");
        check_dtype(dtype, "unknown dtype");
        if (c->sharded_loop)
            fail(KLNMF_ERR_UNSUPP, "klnmf_upload_weights: a loop over row shards is open on this context (klnmf_loop_begin on a communicator, "
                                   "klnmf_loop_begin_sharded / _agreed) and its exchange carries no denominator; klnmf_loop_end first");
        check_block(c->n, c->f, rows, cols, ld, row0, col0);
        if (c->presence())
            fail(KLNMF_ERR_ARG, "klnmf_upload_weights: the problem holds a presence mask (klnmf_upload_presence); klnmf_clear_weights first");
        const size_t es = c->esize(), n = (size_t)c->n, f = (size_t)c->f, k = (size_t)c->k;
        if (!c->weighted()) {
            HIPCHK(hipStreamSynchronize(c->stream));
            void *om = nullptr;
            const bool have_den = c->beta_on();      // (klnmf_set_divergence took the denominators' slabs and sums: they stay its)
            try {
                om = c->dalloc(n * f * es, false);
                if (!have_den) {
                    c->Dpart = c->dalloc((size_t)c->nsplit * k * f * es);
                    c->denom = c->dalloc(k * f * es);
                    if (c->wsplit > 1) c->WDpart = c->dalloc((size_t)c->wsplit * n * k * es);
                }
                fill_ones(c->stream, om, c->prec == KLNMF_PREC_F64, c->n * c->f);
            } catch (...) {                     // all or nothing: a failed first upload leaves the problem unweighted
                (void)hipStreamSynchronize(c->stream);
                if (!have_den) { c->dfree(c->Dpart); c->dfree(c->denom); c->dfree(c->WDpart); }
                c->dfree(om);
                throw;
            }
            c->Om = om;
        }
        if (rows == 0 || cols == 0) return;
        upload_block(c, src, dtype, rows, cols, ld, row0, col0, 1.0, true);
    });
}

// What klnmf_upload_presence and klnmf_upload_presence_device_rows refuse alike and a batch never meets, in this order around their
// own argument checks.
static void presence_check_supported(klnmf_ctx *c, const std::string &who) {
    if (c->sparse) fail(KLNMF_ERR_UNSUPP, who + ": CSR problems have no masked kernels (the ratio lives on the stored entries only)");
    if (c->prec != KLNMF_PREC_F64 && c->prec != KLNMF_PREC_F32)
        fail(KLNMF_ERR_UNSUPP, who + ": the masked kernels exist in KLNMF_PREC_F64 and KLNMF_PREC_F32 only");
    if (c->sharded_loop)
        fail(KLNMF_ERR_UNSUPP, who + ": a loop over row shards is open on this context (klnmf_loop_begin on a communicator, "
                                     "klnmf_loop_begin_sharded / _agreed) and its exchange carries no W^T.P; klnmf_loop_end first");
}

// the shared argument checks around the one refusal that is a context's own
static MaskDims mask_dims(const klnmf_ctx *c) { return {c->n, c->f, c->k, 1, c->prec}; }
static void presence_check_all(klnmf_ctx *c, const std::string &who, int64_t rows, int64_t row0, bool rows_ok, const int64_t *col_bounds,
                               int n_mod) {
    presence_check_args(who, mask_dims(c), rows, row0, rows_ok, col_bounds, n_mod);
    if (c->weighted()) fail(KLNMF_ERR_ARG, who + ": the problem holds weights (klnmf_upload_weights); klnmf_clear_weights first");
    if (c->beta_on()) fail(KLNMF_ERR_UNSUPP, who + ": the problem runs a beta divergence (klnmf_set_divergence), which has no masked form; "
                                                   "upload the mask as weights (klnmf_upload_weights) or klnmf_set_divergence(ctx, 1.0) first");
    presence_check_bounds(*c, who, "problem", col_bounds, n_mod);
}

// P[row0 + i, m] = src[i, m] for the M = n_mod modalities whose columns are [col_bounds[m], col_bounds[m + 1]) (presence.hip.h).  The
// first upload of a problem fixes the bounds, builds the per-column modality index and takes P filled with 1, with S, D and D's
// slabs beside it; klnmf_set_problem* / klnmf_release_problem drop them with the problem (ProblemState).
int klnmf_upload_presence(klnmf_ctx *c, const void *src, int dtype, int64_t rows, int64_t ld, int64_t row0,
                          const int64_t *col_bounds, int n_mod) {
    return guarded([&] {
        need_problem(c);
        const std::string who = "klnmf_upload_presence";
        presence_check_supported(c, who);
        if (!src && rows > 0) fail(KLNMF_ERR_ARG, "null source");
        check_dtype(dtype, "unknown dtype");
        presence_check_all(c, who, rows, row0, ld >= n_mod, col_bounds, n_mod);
        presence_take(*c, *c, mask_dims(c), col_bounds, n_mod);
        if (rows == 0) return;
        presence_upload(*c, *c, mask_dims(c), 0, src, dtype, rows, ld, row0);
    });
}

// klnmf_upload_presence for a mask in device memory: P[row0 + i, m] = dP[drow_idx[i], src_cols[m]], 1 where src_cols[m] is -1.  The row
// indices are checked on the device first, and only a clean flag takes the mask (a first upload) and launches the gather -- a
// refused call leaves the problem as it was.
int klnmf_upload_presence_device_rows(klnmf_ctx *c, const void *dP, int dtype, int64_t src_rows, int64_t ld, const int64_t *drow_idx,
                                      int64_t rows, int64_t row0, const int *src_cols, const int64_t *col_bounds, int n_mod) {
    return guarded([&] {
        need_problem(c);
        const std::string who = "klnmf_upload_presence_device_rows";
        presence_check_supported(c, who);
        if (!dP && rows > 0) fail(KLNMF_ERR_ARG, "null source");
        check_dtype(dtype, "unknown dtype");
        presence_check_all(c, who, rows, row0, ld >= 0 && src_rows >= 0 && (drow_idx || rows <= src_rows), col_bounds, n_mod);
        if (!src_cols) fail(KLNMF_ERR_ARG, who + ": null source columns");
        PresenceCols cols{};
        for (int m = 0; m < n_mod; ++m) {
            if (src_cols[m] < -1 || src_cols[m] >= ld) fail(KLNMF_ERR_ARG, who + ": a source column outside [-1, ld)");
            cols.col[m] = src_cols[m];
        }
        if (rows > 0 && drow_idx) presence_rows_check(*c, who, drow_idx, rows, src_rows);
        presence_take(*c, *c, mask_dims(c), col_bounds, n_mod);
        if (rows == 0) return;
        presence_gather(*c, *c, mask_dims(c), 0, dP, dtype, ld, drow_idx, rows, row0, cols);
    });
}

// weights and a presence mask alike: the problem runs the unweighted kernels again
int klnmf_clear_weights(klnmf_ctx *c) {
    return guarded([&] {
        need_problem(c);
        if (c->presence()) {
            presence_drop(*c, *c);
            return;
        }
        if (!c->weighted()) return;
        HIPCHK(hipStreamSynchronize(c->stream));
        c->dfree(c->Om);
        if (!c->beta_on()) { c->dfree(c->Dpart); c->dfree(c->denom); c->dfree(c->WDpart); }      // (a beta problem keeps its denominators)
    });
}

int klnmf_upload_V_device(klnmf_ctx *c, const float *dsrc, int64_t rows, int64_t cols, int64_t ld,
                          int64_t row0, int64_t col0, double scale) {
    return guarded([&] {
        need_problem(c);
        if (!dsrc) fail(KLNMF_ERR_ARG, "null source");
        check_block(c->n, c->f, rows, cols, ld, row0, col0);
        place_block(c, dsrc, false, rows, cols, ld, row0, col0, scale);
    });
}

int klnmf_upload_V_device_rows(klnmf_ctx *c, const float *dsrc, const int64_t *drow_idx, int64_t rows,
                               int64_t cols, int64_t ld, int64_t row0, int64_t col0, double scale) {
    return guarded([&] {
        need_problem(c);
        if (!dsrc || !drow_idx) fail(KLNMF_ERR_ARG, "null source");
        check_block(c->n, c->f, rows, cols, ld, row0, col0);
        place_block(c, dsrc, false, rows, cols, ld, row0, col0, scale, drow_idx);
    });
}

int klnmf_set_H(klnmf_ctx *c, const void *src, int dtype) {
    return guarded([&] {
        need_problem(c);
        if (!src) fail(KLNMF_ERR_ARG, "null source");
        if (!c->is_exact()) HIPCHK(hipMemsetAsync(c->H32, 0, (size_t)c->KP * c->f_pad * 4, c->stream));
        set_matrix(c, src, dtype, c->k, c->f, c->H, c->H32, c->f_pad);
        if (!c->is_exact()) {
            fast_pack_H(c);          // hs-based scales (also leaves them in t_hs)
            // the W that is there (zeros, a klnmf_set_W, W0 = V.H_init^T of klnmf_init_W) goes with it; behind klnmf_init_W the
            // first update still starts from W0 -- about f / k too small whatever dictionary is set now (transform with
            // components_ != _init_dictionary: nmf.py:159-230) --, so the first update's ratio scale stays on
            measure_and_pack(c, c->w_is_init);
        }
    });
}

// ---- device-resident operands (next-row N1: the transforms of an evaluation keep dictionary, coefficients and
// reconstructions on the GPU).  Pointers are DEVICE memory of the context's device; row strides in elements.
int klnmf_set_H_device(klnmf_ctx *c, const void *dsrc, int dtype, int64_t ld, int64_t col0, int64_t ncols, int last) {
    return guarded([&] {
        need_problem(c);
        if (!dsrc) fail(KLNMF_ERR_ARG, "null source");
        check_dtype(dtype);
        if (col0 < 0 || ncols < 0 || col0 + ncols > c->f || ld < ncols) fail(KLNMF_ERR_ARG, "klnmf_set_H_device: column block out of range");
        // the first block of a dictionary (col0 = 0) starts from zeros, as klnmf_set_H does: a pooled or re-used context
        // must not keep padding rows / columns of the previous dictionary in its images
        if (col0 == 0 && !c->is_exact()) HIPCHK(hipMemsetAsync(c->H32, 0, (size_t)c->KP * c->f_pad * 4, c->stream));
        if (c->is_exact())
            copy_2d_any(c->stream, (char *)c->H + (size_t)col0 * c->esize(), c->prec == KLNMF_PREC_F64, c->f, dsrc, dtype == KLNMF_DT_F64, ld,
                        c->k, ncols);
        else
            copy_2d_any(c->stream, c->H32 + col0, false, c->f_pad, dsrc, dtype == KLNMF_DT_F64, ld, c->k, ncols);
        if (last) {
            if (!c->is_exact()) {
                fast_pack_H(c);
                measure_and_pack(c, c->w_is_init);
            }
            HIPCHK(hipStreamSynchronize(c->stream));      // the caller's buffer may go away
        }
    });
}

int klnmf_get_W_device(klnmf_ctx *c, void *ddst, int dtype, int64_t ld) {
    return guarded([&] {
        need_problem(c);
        if (!ddst) fail(KLNMF_ERR_ARG, "null destination");
        check_dtype(dtype);
        if (ld < c->k) fail(KLNMF_ERR_ARG, "klnmf_get_W_device: row stride shorter than k");
        if (c->is_exact())
            copy_2d_any(c->stream, ddst, dtype == KLNMF_DT_F64, ld, c->W[c->cur], c->prec == KLNMF_PREC_F64, c->k, c->n, c->k);
        else
            copy_2d_any(c->stream, ddst, dtype == KLNMF_DT_F64, ld, c->W32[c->cur], false, c->KP, c->n, c->k, 1.0 / c->v_scale);
        HIPCHK(hipStreamSynchronize(c->stream));
    });
}

int klnmf_upload_V_device_rows_dt(klnmf_ctx *c, const void *dsrc, int dtype, const int64_t *drow_idx, int64_t rows,
                                  int64_t cols, int64_t ld, int64_t row0, int64_t col0, double scale) {
    return guarded([&] {
        need_problem(c);
        if (!dsrc) fail(KLNMF_ERR_ARG, "null source");
        check_dtype(dtype);
        check_block(c->n, c->f, rows, cols, ld, row0, col0);
        place_block(c, dsrc, dtype == KLNMF_DT_F64, rows, cols, ld, row0, col0, scale, drow_idx);
    });
}

int klnmf_set_W(klnmf_ctx *c, const void *src, int dtype) {
    return guarded([&] {
        need_problem(c);
        if (!src) fail(KLNMF_ERR_ARG, "null source");
        set_matrix(c, src, dtype, c->n, c->k, c->W[c->cur], c->W32[c->cur], c->KP, c->v_scale);
        c->w_is_init = false;
        if (!c->is_exact()) measure_and_pack(c);     // (all padded rows too: the eps carrier column in every row a tile can contain)
    });
}

int klnmf_set_Q(klnmf_ctx *c, const void *src, int dtype) {
    return guarded([&] {
        need_problem(c);
        if (!c->is_exact()) fail(KLNMF_ERR_UNSUPP, "the ratio Q is never materialised in the bf16 modes");
        if (!src) fail(KLNMF_ERR_ARG, "null source");
        if (c->sparse) fail(KLNMF_ERR_UNSUPP, "klnmf_set_Q: the ratio of a CSR problem lives on X's structure");
        set_matrix(c, src, dtype, c->n, c->f, c->Q, nullptr, 0);
        c->x3_ready = false;      // (the fused row pass's qr no longer bounds these ratios: the column pass takes the fp32 kernel)
    });
}

int klnmf_set_ratio_eps(klnmf_ctx *c, double eps) {
    return guarded([&] {
        use(c);
        if (!(eps >= 0)) fail(KLNMF_ERR_ARG, "eps must be >= 0");
        if (!c->is_exact() && eps != kEpsRatio)
            fail(KLNMF_ERR_UNSUPP, "the bf16 kernels use the reference's fixed eps = 1e-8");
        c->ratio_eps = eps;
    });
}

int klnmf_get_W(klnmf_ctx *c, void *dst, int dtype) {
    return guarded([&] {
        need_problem(c);
        if (!dst) fail(KLNMF_ERR_ARG, "null destination");
        get_matrix(c, dst, dtype, c->n, c->k, c->W[c->cur], c->W32[c->cur], c->KP, 1.0 / c->v_scale);
    });
}

int klnmf_get_H(klnmf_ctx *c, void *dst, int dtype) {
    return guarded([&] {
        need_problem(c);
        if (!dst) fail(KLNMF_ERR_ARG, "null destination");
        get_matrix(c, dst, dtype, c->k, c->f, c->H, c->H32, c->f_pad);
    });
}

int klnmf_get_Q(klnmf_ctx *c, void *dst, int dtype) {
    return guarded([&] {
        need_problem(c);
        if (!c->is_exact()) fail(KLNMF_ERR_UNSUPP, "the ratio Q is never materialised in the bf16 modes");
        if (!dst) fail(KLNMF_ERR_ARG, "null destination");
        if (c->sparse) fail(KLNMF_ERR_UNSUPP, "klnmf_get_Q: use klnmf_get_Q_values for a CSR problem");
        get_matrix(c, dst, dtype, c->n, c->f, c->Q, nullptr, 0);
    });
}

}  // extern "C"
