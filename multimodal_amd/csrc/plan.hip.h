// The launch plan of a problem as a value: every count klnmf_set_problem* derive from the shape, the precision, the device's CU
// count and the development switches, computed BEFORE anything is allocated by three pure functions (plan_dense_exact,
// plan_dense_16, plan_csr: no HIP runtime call, no context).  ProblemState (ctx.hip.h) derives from ProblemPlan, so c->nsplit,
// c->KP, ... are the stored plan's fields; klnmf_query answers from it and klnmf_plan_query from a fresh one (plan_answer).
// Included by ctx.hip.h behind the kernel headers (their tile constants) and DevSwitches.
#pragma once

namespace klnmf_host {

inline bool prec_is_exact(int prec) {
    return prec == KLNMF_PREC_F64 || prec == KLNMF_PREC_F32 || prec == KLNMF_PREC_BF16X3 || prec == KLNMF_PREC_F16X3;
}
inline size_t prec_esize(int prec) { return prec == KLNMF_PREC_F64 ? 8 : 4; }

struct ProblemPlan {
    enum Mode { NONE = 0, DENSE_EXACT, DENSE_16, CSR };
    int mode = NONE;
    // a refusal that depends on the shape alone; refuse_releases: the previous problem is released first (k > 512 in the 16-bit mode)
    int refuse = KLNMF_OK;
    const char *refuse_msg = "";
    bool refuse_releases = false;

    int64_t n = 0, f = 0, k = 0, nnz = 0;
    bool sparse = false;          // CSR input in the exact modes (sparse.hip.h)

    // ---- exact modes, dense
    int64_t loss_part_count = 0;
    int nsplit = 1, kchunk = 0;       // row chunks of the H numerator's contraction, slabs in Npart
    int wsplit = 1, wchunk = 0;       // feature chunks of the W rule's contraction (few rows), slabs in Wpart
    bool x3 = false;                  // KLNMF_PREC_F16X3 on dense input with k <= 256: the fused loop kernels (f16x3.hip.h)
    int hseg_n = 1; int64_t hseg = 0; // segments per dictionary row and their length (1: the one-block-per-row kernels)
    int64_t sp_nblk = 0;              // ---- CSR
    bool sp_blocked = false;          // blocked for the L2 (sparseb.hip.h; k <= 512):
    int sp_cb = 1, sp_rb = 1;         // column blocks of the CSR order, row blocks of the CSC order
    int64_t sp_cb_cols = 0, sp_rb_rows = 0;

    // ---- 16-bit mode
    int KT = 0, KP = 0, ks = 0;
    bool big = false;                 // 224 < k <= 512: 4-wave workgroups of the ping-pong row pass (mfma4.hip.h)
    int64_t n_pad = 0, f_pad = 0, w_rows = 0;
    int nrt = 0, nct = 0, nct_used = 0, ncb = 0, nchunks = 0, stages_per_chunk = 0;
    bool q8_ok = false;               // the shape allows fp8 ratio tiles (q8_loop of LoopState: a loop's data do)
    bool ne_ok = false;               // the problem's shape has NE kernels (fp16 V, k <= 224, enough rows for fp8 ratio tiles)
    bool w8 = false;                  // the e4m3 image of W_new for the fp8 x fp8 column pass is kept (colq8x.hip.h; KLNMF_COL8=0: off)
    int kc_shape = -1;                // eps-carrying pad component as the shape allows it (kc: choose_eps_carrier)
    int row_chunks = 1, row_ct_chunk = 0;     // column-split update pass (few rows): chunks, column tiles per chunk
    int tail_wg = 0, tail_chunks = 1, tail_ct_chunk = 0;      // hybrid update pass (many rows); tail_wg = 0: none
    // Column parts of the H numerator.  `whole`: all columns as one part (layout [KP][f_pad], what every single-context loop
    // and the exchange API use).  `parts[0 .. nparts_cfg)`: the split layout of loops on a communicator -- part p = a range of
    // column blocks with its own slabs [nchunks][KP][ld] and numerator [KP][ld] (contiguous: one ncclAllReduce each), so that
    // the all-reduce of part p overlaps the column pass of part p + 1 (KLNMF_COMM_PARTS, default 1 = no split)
    struct PartCfg { int cb0, ncb, ct0, nct, col0, ncols, ld, nchunks, spc; int64_t numer_off, slab_off; };
    PartCfg whole{}, parts[kPostMaxParts]{};
    int nparts_cfg = 1;
    // buffer sizes in bytes (0: the buffer is not allocated)
    size_t v_bytes = 0, qt_bytes = 0, w8_bytes = 0, w32_bytes = 0, wb_bytes = 0, h32_bytes = 0, ht4_bytes = 0;
    size_t npartF_bytes = 0, numerF_bytes = 0, gpart_bytes = 0, loss_part2_bytes = 0;

    int64_t loss_parts() const {               // entries of loss_part2 an update pass writes
        if (tail_wg > 0) return (int64_t)nrt + (int64_t)(tail_chunks - 1) * (nrt - tail_rt0());
        return (int64_t)nrt * row_chunks;
    }
    int tail_rt0() const { return (((nrt + 7) / 8) - tail_wg) * 8; }
    // fp8 ratio tiles from how many rows per context?  Their e4m3 rounding only enters the H numerator, a sum over all rows
    // (relative error ~ 0.036 sqrt(2 / n)); measured against the fp64 oracle (scripts/fp8_rows_survey.py,
    // profiles/r03_fp8_rows_survey.txt): final-KL deviation 1.7e-5 .. 3.5e-5 from 4096 to 50 000 rows at k = 50, 6.7e-6 .. 1.5e-5
    // at k = 200 -- a floor that does not depend on n, a fifth of the 1e-4 budget.  k <= 224: from 32 769 rows, where the
    // column-split update pass of small problems no longer runs (round 2: 65 536; C2 = 50 000 rows now qualifies).
    // 256 < k <= 512: 65 536, the size fixture G14 pins.
    static bool row_chunks_possible_q8(int64_t n, bool big_k) { return big_k ? n >= 65536 : n > 32768; }
};

// A single-context fit loop (piece_fit_tail) applies the H rule straight from the row chunks' slabs (k_update_H on NumSlabs) where that
// is a few thousand loads per row; beyond, and in segments, the slabs are summed first (k_sum_partials).  KLNMF_Q_EX_H_FROM_SLABS.
inline bool h_from_slabs(const ProblemPlan *p) {
    return !p->sparse && p->hseg_n == 1 && (int64_t)p->nsplit * p->f <= 8192;
}

constexpr const char *kCsrNeedsExact =
    "CSR input runs in the exact modes (KLNMF_PREC_F64 / F32 / BF16X3 / F16X3); densify for the bf16 kernels";

inline bool plan_refuses_shape(ProblemPlan &p, bool args_ok, const char *args_msg) {
    if (!args_ok) { p.refuse = KLNMF_ERR_ARG; p.refuse_msg = args_msg; }
    else if (p.n > (1LL << 30) || p.f > (1LL << 30) || p.k > (1LL << 20)) {
        p.refuse = KLNMF_ERR_UNSUPP; p.refuse_msg = "dimension too large";
    }
    return p.refuse != KLNMF_OK;
}

// Dictionary rows of 16 384 columns and more: the H rule (exact_H) -- and a CSR problem's loss term's row sums -- in segments
// of 4096.  `forced`: KLNMF_EX_H_SEG = L, the H rule in segments of L columns at any f > L (dense problems; klnmf_set_problem_sparse
// passes 0: the CSR path never honoured the switch).
inline void plan_h_segments(ProblemPlan &p, int64_t forced) {
    p.hseg = 4096;
    p.hseg_n = p.f >= 16384 ? (int)((p.f + p.hseg - 1) / p.hseg) : 1;
    if (forced > 0) {
        p.hseg = forced;
        p.hseg_n = p.f > p.hseg ? (int)((p.f + p.hseg - 1) / p.hseg) : 1;
    }
}

// ---- dense problems of the exact modes ------------------------------------------------------------------------------------------
inline ProblemPlan plan_dense_exact(int64_t n, int64_t f, int64_t k, int prec, int cu_count, const DevSwitches &sw) {
    ProblemPlan p;
    p.mode = ProblemPlan::DENSE_EXACT;
    p.n = n; p.f = f; p.k = k;
    if (plan_refuses_shape(p, n > 0 && f > 0 && k > 0, "n, f, k must be positive")) return p;
    if (n > (int64_t)65535 * GT) {
        p.refuse = KLNMF_ERR_UNSUPP;
        p.refuse_msg = "KLNMF_PREC_F64 / F32 / BF16X3 / F16X3: more than 65535 x 64 rows per context (row tiles ride on gridDim.y); "
                       "shard the rows or use the 16-bit mode";
        return p;
    }
    const int64_t es = (int64_t)prec_esize(prec);
    // 64 x 64 output tiles (k_gemm).  Measured (profiles/r04_exact_modes.txt): with the register prefetch they win over
    // 128 x 128 tiles at every shape tried (2000 x 4096, k = 200, fp64: 440 us per iteration against 455, 537 before):
    // four waves per SIMD hide more than the halved LDS traffic gains.
    auto tiles_of = [](int64_t M, int64_t N) { return ((M + GT - 1) / GT) * ((N + GT - 1) / GT); };
    int64_t s = sw.ex_rc;                                 // (KLNMF_EX_ROW_CHUNKS: ctx.hip.h)
    if (s <= 0) {
        const int64_t tiles = tiles_of(k, f);
        s = (4 * (int64_t)cu_count + tiles - 1) / tiles;
        s = std::max<int64_t>(1, std::min<int64_t>(s, (n + 63) / 64));      // at least four contraction steps per chunk
    }
    int64_t chunk = (n + s - 1) / s;
    chunk = (chunk + GK - 1) / GK * GK;
    p.nsplit = (int)((n + chunk - 1) / chunk);
    p.kchunk = (int)chunk;
    plan_h_segments(p, sw.ex_hseg);
    // W rule: n*k/4096 output tiles, each contracting over all of f.  With fewer tiles than CUs split f so that
    // the grid covers the chip about twice.
    const int64_t wt = tiles_of(k, n);
    int64_t ws = wt < cu_count ? (2 * (int64_t)cu_count + wt - 1) / wt : 1;
    ws = std::min<int64_t>(ws, (f + 4 * GK - 1) / (4 * GK));
    if (sw.ex_wc > 0) ws = sw.ex_wc;                      // (KLNMF_EX_W_CHUNKS)
    while (ws > 1 && ws * n * k * es > ((int64_t)256 << 20)) --ws;
    int64_t wch = (f + ws - 1) / ws;
    wch = (wch + GK - 1) / GK * GK;
    p.wsplit = (int)((f + wch - 1) / wch);
    p.wchunk = (int)wch;
    p.loss_part_count = ((f + GT - 1) / GT) * ((n + GT - 1) / GT);
    p.x3 = prec == KLNMF_PREC_F16X3 && k <= F3_KMAX;
    return p;
}

// ---- dense problems of the 16-bit mode ------------------------------------------------------------------------------------------
inline ProblemPlan plan_dense_16(int64_t n, int64_t f, int64_t k, int cu_count, const DevSwitches &sw) {
    ProblemPlan p;
    p.mode = ProblemPlan::DENSE_16;
    p.n = n; p.f = f; p.k = k;
    if (plan_refuses_shape(p, n > 0 && f > 0 && k > 0, "n, f, k must be positive")) return p;
    if (k > 512) {
        p.refuse = KLNMF_ERR_UNSUPP;
        p.refuse_msg = "k > 512 runs in KLNMF_PREC_F32 / F64 / BF16X3 / F16X3 (the 16-bit MFMA kernels cover k <= 512)";
        p.refuse_releases = true;
        return p;
    }
    p.KT = (int)((k + 31) / 32);
    p.ks = (int)((k + 15) / 16);
    if (p.KT >= 8) {
        // 224 < k <= 512: 4-wave workgroups of the row pass (whole register file per wave, FUSED order) and the
        // component-split column passes; component tiles in pairs, the W.H contraction over all of them
        p.big = true;
        p.KT = 2 * (int)((k + 63) / 64);
        p.ks = 2 * p.KT;
    }
    p.KP = 32 * p.KT;
    // both passes work on 64-row / 64-column stages: pad to 64 (zero padding is inert)
    p.n_pad = (n + 63) / 64 * 64;
    p.f_pad = (f + 127) / 128 * 128;            // the row pass walks 4 column tiles per loop body
    p.nrt = (int)(p.n_pad / 32);
    p.nct = (int)(p.f_pad / 32);
    p.nct_used = (int)((f + 63) / 64 * 2);      // column tiles that hold data (column pass)
    const int total_stages = p.nrt / kStageRowTiles;
    // the fp16 W images are streamed by global_load_lds in whole 8 KiB rounds, i.e. a stage's copy reads on into the rows
    // behind it: pad the tail by what ONE copy covers.  (64 rows until round 4: at KP = 32 a row is 64 bytes and a copy 128
    // rows -- the last stage read 2 KiB past the image; found by scripts/shape_fuzz.py as a memory access fault at
    // 16 305 x 28, k = 8, where the image is exactly 1 MiB and ends on a mapping boundary.)
    const int64_t copy_rows = (colq_w_area(p.KP) + (int64_t)w_ld(p.KP) * 2 - 1) / ((int64_t)w_ld(p.KP) * 2);
    p.w_rows = (int64_t)total_stages * 32 * kStageRowTiles + std::max<int64_t>(64, copy_rows);
    p.v_bytes = (size_t)p.nrt * p.nct * 1024 * 2;
    // fp8 ratio tiles: only the H numerator -- a sum over all rows -- sees their 3-bit significands; its relative
    // error falls like 0.036 sqrt(2 / n), so they are used from 32 769 / 65 536 rows per context on (row_chunks_possible_q8;
    // KLNMF_QTILE = 8 / 16 forces either), where the bytes matter
    const bool col8_off = sw.col8 == 0;
    const bool q8_kt = !p.big || !col8_off;      // (k > 224: fp8 tiles only with the fp8 x fp8 column pass)
    // ... and from one column tile of data on: below that the tiles are mostly padding (nothing to gain), and a handful of
    // columns is fitted so exactly that the loss itself goes to 0 (the 16-bit mode's own operand rounding then shows)
    p.q8_ok = q8_kt && f >= 32 && ProblemPlan::row_chunks_possible_q8(n, p.big);
    if (sw.qtile != 0) p.q8_ok = q8_kt && sw.qtile == 8;
    p.ne_ok = p.q8_ok && !p.big;      // (q8_ok: enough rows for fp8 ratio tiles -- where the NE kernels exist)
    p.qt_bytes = (size_t)p.nrt * p.nct * kQTile;      // (fp8 tiles use the first half of the buffer)
    // fp8 x fp8 column pass (e4m3 image of W_new): where the H-numerator product is worth the conversion launch --
    // k > 96 and 65 536 rows or more; below that the f16-operand column pass reads the fp8 tiles (C2, k = 50: 0.053 ms
    // against 0.050 + 0.03 ms of conversions; profiles/r03_c2_schedules.txt)
    const bool col8_size = p.big || (p.KT >= 4 && n >= 65536) || sw.col8 >= 1;
    p.w8 = p.q8_ok && !col8_off && col8_size;
    if (p.w8) p.w8_bytes = (size_t)(p.n_pad + 64) * w8_ld(p.KP) + 65536;
    p.w32_bytes = (size_t)p.n_pad * p.KP * 4;
    p.wb_bytes = (size_t)p.w_rows * w_ld(p.KP) * 2;
    p.h32_bytes = (size_t)p.KP * p.f_pad * 4;
    p.ht4_bytes = (size_t)p.nct * h4_tile_bytes(p.KP) + kObj4;
    // eps through a pad component (k_update_pack_H): the row pass's W epilogue keeps the carrier column at 2^-10; needs
    // a spare component inside the MFMA-1 contraction range
    p.kc_shape = (k < 16 * p.ks && sw.eps_pad) ? (int)k : -1;
    // column pass decomposition: column blocks of 8 tiles x row chunks; keep the grid a
    // multiple of 8 (XCD remap) and close to a multiple of the CU count
    const int ctw = p.big ? kWavesPerWG / 2 : kWavesPerWG;      // column tiles per workgroup (colq.hip.h, KSPLIT)
    p.ncb = (p.nct_used + ctw - 1) / ctw;
    auto chunks_for = [&](int ncb) {      // row chunks of a column pass over `ncb` column blocks: the grid fills the chip once
        int nch = 8;                      // (one workgroup is resident per CU; two per CU measured 1-3 % slower)
        while ((int64_t)nch * ncb < cu_count && nch * 2 <= total_stages) nch += 8;
        while (nch > 8 && ((int64_t)nch * ncb) % cu_count != 0 &&
               (int64_t)(nch - 8) * ncb >= cu_count) nch -= 8;
        if (nch > total_stages) nch = total_stages > 0 ? ((total_stages + 7) / 8) * 8 : 8;
        return nch;
    };
    p.nchunks = chunks_for(p.ncb);
    p.stages_per_chunk = (total_stages + p.nchunks - 1) / p.nchunks;
    p.whole = ProblemPlan::PartCfg{0, p.ncb, 0, p.nct_used, 0, (int)f, (int)p.f_pad, p.nchunks, p.stages_per_chunk, 0, 0};
    // column parts for loops on a communicator (overlap of the numerator's all-reduce with the column pass)
    p.nparts_cfg = std::min(std::min(kPostMaxParts, std::max(1, sw.comm_parts)), p.ncb);
    int64_t split_numer = 0, split_slabs = 0;
    if (p.nparts_cfg > 1) {
        for (int i = 0; i < p.nparts_cfg; ++i) {
            ProblemPlan::PartCfg &q = p.parts[i];
            q.cb0 = (int)((int64_t)p.ncb * i / p.nparts_cfg);
            q.ncb = (int)((int64_t)p.ncb * (i + 1) / p.nparts_cfg) - q.cb0;
            q.ct0 = q.cb0 * ctw;
            q.nct = std::min(p.nct_used - q.ct0, q.ncb * ctw);
            q.col0 = q.ct0 * 32;
            q.ld = q.ncb * ctw * 32;
            q.ncols = (int)std::min<int64_t>(f - q.col0, q.ld);
            q.nchunks = chunks_for(q.ncb);
            q.spc = (total_stages + q.nchunks - 1) / q.nchunks;
            q.numer_off = split_numer;
            q.slab_off = split_slabs;
            split_numer += (int64_t)p.KP * q.ld;
            split_slabs += (int64_t)q.nchunks * p.KP * q.ld;
        }
    }
    p.npartF_bytes = (size_t)std::max<int64_t>((int64_t)p.nchunks * p.KP * p.f_pad, split_slabs) * 4;
    p.numerF_bytes = (size_t)std::max<int64_t>((int64_t)p.KP * p.f_pad, split_numer) * 4;
    // Column-split update pass: with fewer than half as many 8-wave workgroups as CUs (n < ~32 000 rows; the
    // reference's own data sets have 10^2..10^3) split every row block's columns over blockIdx.y so that the grid
    // fills the chip once.  KLNMF_ROW_SPLIT = 0 / N (development switch) forces it off / to N chunks.
    // (row_chunks and tail_wg below: only under !big -- the column-split kernels exist for the 8-wave workgroups alone,
    // and fast_rowpass refuses a big problem that carries either)
    p.row_ct_chunk = p.nct;
    const int nwg = (p.nrt + kWaves4 - 1) / kWaves4;
    if (!p.big && !p.q8_ok) {
        int want = (2 * nwg <= cu_count) ? cu_count / nwg : 1;
        if (sw.row_split >= 0) want = std::max(1, sw.row_split);
        want = std::min(want, p.nct / 4);
        const int64_t slab_bytes = (int64_t)p.nrt * 32 * p.KP * 4;
        while (want > 1 && want * slab_bytes > (int64_t)256 << 20) --want;
        if (want > 1) {
            p.row_ct_chunk = 4 * ((p.nct / 4 + want - 1) / want);
            p.row_chunks = (p.nct + p.row_ct_chunk - 1) / p.row_ct_chunk;
        }
        if (p.row_chunks > 1) p.gpart_bytes = (size_t)p.row_chunks * slab_bytes;
    }
    // Hybrid update pass: more workgroups than CUs, and a last partial round of at most half the CUs (one
    // workgroup per CU: 254 registers).  Its workgroups are split into as many column chunks as fill the chip
    // once (n = 10^6: 67 workgroups x 3 chunks; 90 000 rows: 96 x 2).  KLNMF_ROW_TAIL = 0 (development switch): off.
    p.tail_ct_chunk = p.nct;
    if (!p.big && p.row_chunks == 1) {
        const int rem = nwg % cu_count;
        int want = (nwg > cu_count && rem > 0) ? cu_count / rem : 1;
        if (sw.row_tail >= 0) want = std::min(want, std::max(1, sw.row_tail));
        want = std::min(std::min(want, 4), p.nct / 4);
        if (want > 1) {
            p.tail_ct_chunk = 4 * ((p.nct / 4 + want - 1) / want);
            p.tail_chunks = (p.nct + p.tail_ct_chunk - 1) / p.tail_ct_chunk;
            if (p.tail_chunks > 1) {
                p.tail_wg = rem;
                p.gpart_bytes = (size_t)p.tail_chunks * (p.nrt - p.tail_rt0()) * 32 * p.KP * 4;
            }
        }
    }
    p.loss_part2_bytes = sizeof(double2) * (size_t)std::max<int64_t>(p.loss_parts(), (int64_t)p.nrt * p.row_chunks);
    return p;
}

// ---- CSR problems (exact modes) -------------------------------------------------------------------------------------------------
inline ProblemPlan plan_csr(int64_t n, int64_t f, int64_t k, int64_t nnz, int prec, int cu_count, const DevSwitches &sw) {
    (void)cu_count;                   // (no CSR rule depends on it)
    ProblemPlan p;
    p.mode = ProblemPlan::CSR;
    p.n = n; p.f = f; p.k = k; p.nnz = nnz;
    p.sparse = true;
    if (plan_refuses_shape(p, n > 0 && f > 0 && k > 0 && nnz >= 0, "n, f, k must be positive, nnz >= 0")) return p;
    const int64_t es = (int64_t)prec_esize(prec);
    p.sp_nblk = (n + kSpColsumRows - 1) / kSpColsumRows;
    plan_h_segments(p, 0);
    // blocks for the L2 (sparseb.hip.h): kSpBlockBytes of H^T per column block / of W per row block, as many blocks as the
    // slabs of partial sums allow (1 GiB each)
    p.sp_blocked = k <= 512 && nnz > 0 && n < ((int64_t)1 << 31) && f < ((int64_t)1 << 31) && nnz < ((int64_t)1 << 31);
    if (!p.sp_blocked) return p;
    const int64_t per = std::max<int64_t>(64, (kSpBlockBytes / (int64_t)(k * es)) / 64 * 64);
    const int64_t slab_cap = (int64_t)1 << 30;
    // How many blocks: as many as make a block's gathered rows fit the L2 (`per` rows of k x es bytes) -- but a (row, block)
    // cell must still fill the kernels' trips, or the gather slots of its last trip run empty.  Measured (round 5, 20 000 x
    // 110 000, 0.5 %, k = 50, fp64; profiles/r05_sparse_blocks.txt): 15 column blocks (37 entries per cell) cut the fused
    // pass's fabric traffic from 4.5 to 1.1 GB and cost it 0.87 instead of 0.66 ms; 4 blocks (137 per cell): 0.62 ms; 3 row
    // blocks (33 per cell, groups of 16) take the H-side pass from 0.61 to 0.51 ms, 6 (17 per cell) back to 0.63.  So: at
    // least 128 entries per cell of the CSR order, 32 of the CSC order.  KLNMF_SP_CB / KLNMF_SP_RB (development) override.
    int64_t cb = std::min<int64_t>((f + per - 1) / per, std::max<int64_t>(1, nnz / std::max<int64_t>(1, n) / 128));
    int64_t rb = std::min<int64_t>((n + per - 1) / per, std::max<int64_t>(1, nnz / std::max<int64_t>(1, f) / 32));
    if (sw.sp_cb > 0) cb = std::min<int64_t>(sw.sp_cb, (f + 63) / 64);
    if (sw.sp_rb > 0) rb = std::min<int64_t>(sw.sp_rb, (n + 63) / 64);
    cb = std::max<int64_t>(1, std::min(cb, slab_cap / std::max<int64_t>(1, n * k * es)));
    rb = std::max<int64_t>(1, std::min(rb, slab_cap / std::max<int64_t>(1, f * k * es)));
    cb = std::min<int64_t>(cb, ((int64_t)1 << 31) / std::max<int64_t>(1, n) - 1);      // (blocks x rows ride on gridDim.x)
    rb = std::min<int64_t>(rb, ((int64_t)1 << 31) / std::max<int64_t>(1, f) - 1);
    if (cb < 1 || rb < 1) p.sp_blocked = false;
    p.sp_cb = (int)cb; p.sp_rb = (int)rb;
    p.sp_cb_cols = (f + cb - 1) / cb; p.sp_rb_rows = (n + rb - 1) / rb;
    return p;
}

// The plan of (precision, shape): nnz < 0 a dense problem (klnmf_set_problem), nnz >= 0 a CSR one (klnmf_set_problem_sparse).
inline ProblemPlan plan_problem(int prec, int64_t n, int64_t f, int64_t k, int64_t nnz, int cu_count, const DevSwitches &sw) {
    if (nnz >= 0) {
        if (prec_is_exact(prec)) return plan_csr(n, f, k, nnz, prec, cu_count, sw);
        ProblemPlan p;
        p.refuse = KLNMF_ERR_UNSUPP; p.refuse_msg = kCsrNeedsExact;
        return p;
    }
    return prec_is_exact(prec) ? plan_dense_exact(n, f, k, prec, cu_count, sw) : plan_dense_16(n, f, k, cu_count, sw);
}

// The plan items of klnmf_query / klnmf_plan_query; false: `what` is not one of them.
inline bool plan_answer(const ProblemPlan &p, int what, int64_t *value) {
    const bool dense_exact = p.mode == ProblemPlan::DENSE_EXACT, blocked = p.mode == ProblemPlan::CSR && p.sp_blocked;
    switch (what) {
        case KLNMF_Q_RATIO_TILE_BYTES:          // per element of V: 0 = no stored ratio tiles, 2 = 16-bit, 1 = fp8 once a loop allows them
            *value = p.mode == ProblemPlan::DENSE_16 ? (p.q8_ok ? 1 : 2) : 0;
            return true;
        case KLNMF_Q_SP_COL_BLOCKS: *value = blocked ? p.sp_cb : 0; return true;
        case KLNMF_Q_SP_ROW_BLOCKS: *value = blocked ? p.sp_rb : 0; return true;
        case KLNMF_Q_EX_ROW_CHUNKS: *value = dense_exact ? p.nsplit : 0; return true;
        case KLNMF_Q_EX_W_CHUNKS: *value = dense_exact ? p.wsplit : 0; return true;
        case KLNMF_Q_EX_H_SEGMENTS: *value = dense_exact ? p.hseg_n : 0; return true;
        case KLNMF_Q_EX_H_FROM_SLABS: *value = (dense_exact && h_from_slabs(&p)) ? 1 : 0; return true;
        default: return false;
    }
}

}  // namespace klnmf_host
