// Host side of libklnmf.so, shared by its translation units (include/klnmf.h has the contract and the reference interfaces each
// entry point replaces):
//   api_context.hip  contexts, problems, uploads and downloads (K6: learner.py:53-56 stack_data; nmf.py:147-157 _init)
//   api_loop.hip     the loop of nmf.py:212-222 and its pieces: launch sequencing (the row pass's kernel looked up in the table
//                    built from rowpass4_list.hip.h), stop rule, fp8 regime and its monitor; the loop driver every loop of
//                    every unit runs on (loop_open, local_iteration, loop_advance, stop_fired)
//   api_comm.hip     row shards over the GPUs of a node: the RCCL communicator, the agreed loop entry, the exchange (nmf.py:349)
//   api_eval.hip     evaluation and introspection: reconstruction products (learner.py:80-84), distances, the fused nearest-example
//                    search of include/klnmf_nearest.h (nearest.hip.h, included by this unit alone), queries, profiling
//   api_group.hip    a group of contexts (row shards, one device each, a device may repeat) driven from one host thread: the
//                    exchange of group.hip.h between their streams, the loop of klnmf_group_run
//   api_batch.hip    a batch of dense problems of one shape in KLNMF_PREC_F64 / F32, unweighted or all under presence masks
//                    (klnmf_batch_*): the [B] layout, the loop's stages as one launch each for all of them (batch.hip.h), the plan
//                    of one problem for its share of the CUs; and of CSR problems of one shape, each with its own stored entries
//                    (klnmf_batch_csr.h, batch_sparse.hip.h)
//   api_beta.hip     the beta-divergence cost of a context's problem (include/klnmf_beta.h): its buffers and refusals, its loss and
//                    single steps; the loop's pieces branch on it in api_loop.hip, on the policies of beta.hip.h
//   api_info.hip     the atom x label information matrix of include/klnmf_information.h (samples/plot_info_matrix.py:66-90,
//                    126-136): checks, workspace layout and the launches of information.hip.h, included by that unit alone
//   api_hac.hip      the windowed co-occurrence histograms of include/klnmf_hac.h (features/hac.py:152-196 behind its MFCCs, for the
//                    windows of samples/image_sound_eval_sliding.py:97-113): checks, workspace layout and the launches of
//                    hac.hip.h behind the quantiser of vq.hip.h
//   api_kmeans.hip   the codebook builders' device half of include/klnmf_kmeans.h (features/hac.py:68-107: Lloyd iterations and
//                    the Gram matrix of a cluster's members): checks, workspace layout and the launches of kmeans.hip.h, included
//                    by that unit alone behind vq.hip.h
//   api_motion.hip   the motion modality's device half of include/klnmf_motion.h: checks, workspace layout and the launches of
//                    motion.hip.h, included by that unit alone
//   api_mfcc.hip     the MFCC front end of include/features/klnmf_mfcc.h (features/hac.py:44-65 and the deltas of :190-192):
//                    checks, workspace layout, the table of twiddles and the launches of mfcc.hip.h, included by that unit alone
// The feature units (the nearest part of api_eval.hip, api_info.hip, api_hac.hip, api_kmeans.hip, api_motion.hip, api_mfcc.hip) word their
// refusals, cut up their workspaces, own their scratch and pick their element type through feature_host.hip.h; the quantiser of
// api_hac.hip and api_kmeans.hip is vq.hip.h's.
// This header: error handling, the type dispatch of the host-facing kernels, the device block cache and the arena over it
// (DeviceBlocks), the staged host upload, the development switches, the mask state (PresenceState) and the context itself -- its
// state in four groups, one per lifetime (ContextState, ProblemState, LoopState, LoopRecord) -- and what contexts and batches share
// (defined once, in api_context.hip: the mask helpers, the steps of a CSR upload, place_rows, copy_2d_any, fill_ones).  plan.hip.h: the launch plan of a
// problem, the value ProblemState is built on; stage_chunks.h: the chunk arithmetic of staged_upload, free of HIP.
#pragma once
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>       // types and enums only: the library itself is opened at run time (no link-time dependency)

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/klnmf.h"
#include "stage_chunks.h"
#include "common.hip.h"
#include "exact.hip.h"
#include "weighted.hip.h"
#include "presence.hip.h"
#include "beta.hip.h"
#include "split3.hip.h"
#include "f16x3.hip.h"
#include "sparseb.hip.h"
#include "mfma.hip.h"
#include "mfma4.hip.h"
// the k_rowpass4 instantiations live in rowpass4_inst_{1,2,3}.hip (built in parallel); here they are only declared, and
// launch_rowpass4_kt (api_loop.hip) takes their addresses: no host unit carries device code for them
#include "rowpass4_list.hip.h"
namespace klnmf {
KL_RP4_LIST_1(KL_RP4_DECLARE) KL_RP4_LIST_2(KL_RP4_DECLARE) KL_RP4_LIST_3(KL_RP4_DECLARE)
}  // namespace klnmf
#include "colq.hip.h"
#include "colq8x.hip.h"
#include "post.hip.h"

using namespace klnmf;

namespace klnmf_host {

extern thread_local std::string g_err;      // (api_eval.hip: klnmf_last_error)

struct ApiError {
    int code;
    std::string msg;
};

[[noreturn]] inline void fail(int code, const std::string &m) { throw ApiError{code, m}; }

#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            fail(e_ == hipErrorOutOfMemory ? KLNMF_ERR_ALLOC : KLNMF_ERR_HIP,              \
                 std::string(#expr) + ": " + hipGetErrorString(e_));                       \
    } while (0)

template <typename F>
int guarded(F &&f) {
    try {
        f();
        return KLNMF_OK;
    } catch (const ApiError &e) {
        g_err = e.msg;
        return e.code;
    } catch (const std::exception &e) {
        g_err = e.what();
        return KLNMF_ERR_HIP;
    } catch (...) {
        g_err = "unknown error";
        return KLNMF_ERR_HIP;
    }
}

inline int grid_for(int64_t count, int block = 256, int cap = 4096) {
    int64_t g = (count + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

// The host-facing kernels (placing, copying, converting, filling) exist for double and float on either side; a dtype or precision
// known at run time picks the instantiation: f(TypeTag<T>{}) for `f64`, f(TypeTag<D>{}, TypeTag<S>{}) for (`d64`, `s64`).
template <typename T> struct TypeTag { using type = T; };
template <typename Tag> using tag_t = typename Tag::type;
template <typename F>
void dispatch_type(bool f64, F &&f) {
    if (f64) f(TypeTag<double>{}); else f(TypeTag<float>{});
}
template <typename F>
void dispatch_types(bool d64, bool s64, F &&f) {
    dispatch_type(d64, [&](auto d) { dispatch_type(s64, [&](auto s) { f(d, s); }); });
}

constexpr const char *kDtypeMsg = "dtype must be KLNMF_DT_F32 or KLNMF_DT_F64";
inline void check_dtype(int dtype, const std::string &msg = kDtypeMsg) {
    if (dtype != KLNMF_DT_F32 && dtype != KLNMF_DT_F64) fail(KLNMF_ERR_ARG, msg);
}
// a block [rows, cols] (leading dimension ld) at (row0, col0) of an n x f matrix
inline void check_block(int64_t n, int64_t f, int64_t rows, int64_t cols, int64_t ld, int64_t row0, int64_t col0) {
    if (rows < 0 || cols < 0 || row0 < 0 || col0 < 0 || row0 + rows > n || col0 + cols > f || ld < cols)
        fail(KLNMF_ERR_ARG, "V block out of range");
}

constexpr int kW8Blocks = 1024;             // conversion kernel's grid: per-block column maxima [kW8Blocks][KP]

struct EventPair {
    hipEvent_t a, b;
};

// RCCL entry points, resolved on first use: a process that never shards needs no librccl.
struct RcclApi {
    void *lib = nullptr;
    std::string err;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclCommCount) CommCount = nullptr;
};
RcclApi &rccl();              // (api_comm.hip: resolved on first use)
#define RCCLCHK(expr)                                                                              \
    do {                                                                                           \
        ncclResult_t r_ = (expr);                                                                  \
        if (r_ != ncclSuccess) fail(KLNMF_ERR_RCCL, std::string(#expr) + ": " + rccl().GetErrorString(r_)); \
    } while (0)

}  // namespace klnmf_host
using namespace klnmf_host;

// Device blocks of destroyed / re-shaped contexts are kept for the next one (per process, per device, by size class).
// At the reference's data sizes a fit is a few milliseconds of kernels, and ~25 hipMalloc + hipFree per context cost as
// much again (experiment.py and samples/launcher.py run many small fits and transforms in sequence).  Blocks are handed
// back only after the owning stream has been synchronised (klnmf_destroy, klnmf_set_problem), and every block is
// zero-filled on hand-out as a fresh one is.  KLNMF_ALLOC_CACHE_MB (default 1024; 0 = off) bounds what is kept;
// blocks above 64 MiB are never kept.
struct DevBlockCache {
    std::mutex mu;
    std::map<std::pair<int, size_t>, std::vector<void *>> free_blocks;
    size_t held = 0;
    static size_t limit() {
        static const size_t v = [] {
            const char *e = std::getenv("KLNMF_ALLOC_CACHE_MB");
            return (size_t)(e ? std::max(0, std::atoi(e)) : 1024) << 20;
        }();
        return v;
    }
    static size_t size_class(size_t bytes) {          // next power of two up to 1 MiB, then multiples of 1 MiB
        if (bytes <= 256) return 256;
        if (bytes <= ((size_t)1 << 20)) { size_t c = 256; while (c < bytes) c <<= 1; return c; }
        return (bytes + ((size_t)1 << 20) - 1) >> 20 << 20;
    }
    void *take(int device, size_t cls) {
        std::lock_guard<std::mutex> g(mu);
        auto it = free_blocks.find({device, cls});
        if (it == free_blocks.end() || it->second.empty()) return nullptr;
        void *p = it->second.back();
        it->second.pop_back();
        held -= cls;
        return p;
    }
    void flush(int device) {
        std::lock_guard<std::mutex> g(mu);
        for (auto &kv : free_blocks) {
            if (kv.first.first != device) continue;
            for (void *p : kv.second) { (void)hipFree(p); held -= kv.first.second; }
            kv.second.clear();
        }
    }
    bool give(int device, size_t cls, void *p) {
        if (cls > ((size_t)64 << 20)) return false;
        std::lock_guard<std::mutex> g(mu);
        if (held + cls > limit()) return false;
        free_blocks[{device, cls}].push_back(p);
        held += cls;
        return true;
    }
};
extern DevBlockCache g_block_cache;      // (api_context.hip)

// The device blocks of one owner (a context, a batch) on its device and stream: taken from the cache or the driver, handed back
// one by one or all at once.  Callers of dfree / release_all have synchronised the stream: no kernel still touches the blocks.
struct DeviceBlocks {
    int device = 0;
    hipStream_t stream = nullptr;
    std::vector<std::pair<void *, size_t>> allocs;      // (block, size class) of the current problem's device blocks
    void *dalloc(size_t bytes, bool zero = true) {
        if (bytes == 0) bytes = 16;
        const size_t cls = DevBlockCache::size_class(bytes);
        void *p = g_block_cache.take(device, cls);
        if (!p) {
            hipError_t e = hipMalloc(&p, cls);
            if (e == hipErrorOutOfMemory) {        // the cache may be what is in the way: give its blocks back and retry once
                (void)hipGetLastError();
                g_block_cache.flush(device);
                e = hipMalloc(&p, cls);
            }
            HIPCHK(e);
        }
        allocs.push_back({p, cls});
        if (zero) HIPCHK(hipMemsetAsync(p, 0, bytes, stream));
        return p;
    }
    void dfree(void *&p) {
        for (size_t i = 0; i < allocs.size(); ++i) {
            if (allocs[i].first != p) continue;
            if (!g_block_cache.give(device, allocs[i].second, p)) (void)hipFree(p);
            allocs.erase(allocs.begin() + (std::ptrdiff_t)i);
            break;
        }
        p = nullptr;
    }
    void release_all() {
        for (auto &b : allocs)
            if (!g_block_cache.give(device, b.second, b.first)) (void)hipFree(b.first);
        allocs.clear();
    }
};

// A host block [rows, cols] (rows `ld` elements of `es` bytes apart) through a bounded device staging buffer (stage_chunks.h):
// place(device_chunk, r0, rr) enqueues what puts rows [r0, r0 + rr) where they belong; the stream is synchronised behind every
// chunk, and the buffer is released on the normal and on the throwing path.
template <typename Place>
void staged_upload(hipStream_t stream, const void *src, size_t es, int64_t rows, int64_t cols, int64_t ld, Place &&place) {
    const int64_t rows_per = stage_rows_per(rows, ld, es);
    void *d = nullptr;
    HIPCHK(hipMalloc(&d, stage_alloc_bytes(rows_per, ld, es)));
    try {
        stage_walk(rows, cols, ld, es, rows_per, [&](const StageChunk &ch) {
            HIPCHK(hipMemcpyAsync(d, (const char *)src + ch.offset, ch.bytes, hipMemcpyHostToDevice, stream));
            place((const void *)d, ch.r0, ch.rr);
            HIPCHK(hipStreamSynchronize(stream));
        });
    } catch (...) {
        (void)hipFree(d);
        throw;
    }
    (void)hipFree(d);
}

// Development switches: what only measurements and tests need.  Read in ONE place (here), afresh at every klnmf_set_problem and
// loop entry, and honoured only under KLNMF_DEV=1 -- a production process cannot change the library's arithmetic by accident.
// (User-facing environment: KLNMF_QTILE=16 -- never fp8 ratio tiles -- and KLNMF_ALLOC_CACHE_MB, plus the host layer's
// KLNMF_PRECISION / KLNMF_DEVICE / KLNMF_LIB / KLNMF_NO_POOL: INTEGRATION.md section 1.)
struct DevSwitches {
    int qtile = 0;              // KLNMF_QTILE = 8 / 16: fp8 ratio tiles forced on (from a loop's third iteration) / off      [16: also without KLNMF_DEV]
    int col8 = -1;              // KLNMF_COL8 = 0: no fp8 x fp8 column pass; 1: at any size
    int ne = -1;                // KLNMF_NE = 0 / 1: the update pass without the numerator's eps never / in every fp8 loop
    bool q8_fixup = true;       // KLNMF_Q8_FIXUP=0: no exact correction of large ratio entries (the tests' control run)
    bool q8_monitor = true;     // KLNMF_Q8_MONITOR=0: no monitor
    float mon_threshold = 0.f, mon_min_spread = -1.f;      // KLNMF_MON_THRESHOLD / KLNMF_MON_MIN_SPREAD: the monitor's two thresholds (calibration runs)
    bool ratio_scale = true;    // KLNMF_RATIO_SCALE=0: no ratio scale of the first update
    bool eps_pad = true;        // KLNMF_NO_EPS_PAD=1: eps added in the epilogue instead of riding through MFMA-1
    int row_split = -1;         // KLNMF_ROW_SPLIT = 0 / N: column-split update pass off / N chunks
    int row_tail = -1;          // KLNMF_ROW_TAIL = 0: no column-split last partial round
    int comm_parts = 1;         // KLNMF_COMM_PARTS = P: the numerator in P column parts on a communicator (experimental: one-rank runs only)
    bool comm_overlap = true;   // KLNMF_COMM_OVERLAP=0: the parts' all-reduces on the loop's own stream
    bool comm_single = false;   // KLNMF_COMM_SINGLE=1: a one-rank communicator takes the collective path (tests)
    int sp_cb = 0, sp_rb = 0;   // KLNMF_SP_CB / KLNMF_SP_RB: column / row blocks of the CSR kernels (sparseb.hip.h; 0: by the L2's size)
    // dense problems of the exact modes (klnmf_set_problem; 0: the size rules).  KLNMF_EX_ROW_CHUNKS / KLNMF_EX_W_CHUNKS = N: the H
    // numerator's row chunks / the W rule's feature chunks computed from N instead of the CU count (each chunk still rounded up to
    // GK, so the count may come out below N; 1: the one-piece W rule); KLNMF_EX_H_SEG = L: the H rule in segments of L columns
    // at any f > L.  Buffers are sized for what these force; klnmf_query (KLNMF_Q_EX_*) reports the effective values.
    int ex_rc = 0, ex_wc = 0;
    int64_t ex_hseg = 0;
    static DevSwitches read() {
        DevSwitches d;
        auto num = [](const char *name, int dflt) { const char *e = std::getenv(name); return e ? std::atoi(e) : dflt; };
        if (num("KLNMF_QTILE", 0) == 16) d.qtile = 16;
        if (num("KLNMF_DEV", 0) == 0) return d;
        d.qtile = num("KLNMF_QTILE", 0);
        d.col8 = num("KLNMF_COL8", -1);
        d.ne = num("KLNMF_NE", -1);
        d.q8_fixup = num("KLNMF_Q8_FIXUP", 1) != 0;
        d.q8_monitor = num("KLNMF_Q8_MONITOR", 1) != 0;
        if (const char *e = std::getenv("KLNMF_MON_THRESHOLD")) d.mon_threshold = (float)std::atof(e);
        if (const char *e = std::getenv("KLNMF_MON_MIN_SPREAD")) d.mon_min_spread = (float)std::atof(e);
        d.ratio_scale = num("KLNMF_RATIO_SCALE", 1) != 0;
        d.eps_pad = num("KLNMF_NO_EPS_PAD", 0) == 0;
        d.row_split = num("KLNMF_ROW_SPLIT", -1);
        d.row_tail = num("KLNMF_ROW_TAIL", -1);
        d.comm_parts = num("KLNMF_COMM_PARTS", 1);
        d.comm_overlap = num("KLNMF_COMM_OVERLAP", 1) != 0;
        d.comm_single = num("KLNMF_COMM_SINGLE", 0) != 0;
        d.sp_cb = num("KLNMF_SP_CB", 0);
        d.sp_rb = num("KLNMF_SP_RB", 0);
        d.ex_rc = std::max(0, num("KLNMF_EX_ROW_CHUNKS", 0));
        d.ex_wc = std::max(0, num("KLNMF_EX_W_CHUNKS", 0));
        d.ex_hseg = std::max(0, num("KLNMF_EX_H_SEG", 0));
        return d;
    }
};

#include "plan.hip.h"

namespace klnmf_host {

// The context's state in four groups, one per lifetime.  klnmf_ctx derives from all four (c->field everywhere); a reset is the
// assignment of a default-constructed group, never a list of fields.
// ---- as long as the context: untouched by klnmf_set_problem*
//   * ratio_eps survives klnmf_set_problem* and is reset by klnmf_release_problem;
//   * profile_every and profile_seq survive both calls; profiling survives klnmf_set_problem* and is cleared by
//     klnmf_release_problem;
//   * the communicator (comm, its stream, events and scratch) survives both.
struct ContextState : DeviceBlocks {
    int prec = KLNMF_PREC_F64;
    bool own_stream = false;
    int cu_count = 256;
    double ratio_eps = kEpsRatio;   // only the step API honours a non-default value
    // polls of the monitor's verdict (poll_fp8_overflow).  The dry run's poll synchronises (its answer decides the NEXT iteration's
    // kernels); every later one is deferred: the counts are copied to pinned host memory behind the monitored iteration, an event
    // marks the copy, and the answer is read one iteration later, when the event has long passed -- the stream never drains
    // (a synchronising poll cost a pipeline bubble plus a pageable read-back per check: 5 checks in bench.py's 40 timed iterations)
    void *poll_host = nullptr;                // pinned: a DevState or the two doubles of the loss exchange
    hipEvent_t poll_ev = nullptr;

    bool profiling = false;
    // every `profile_every`-th iteration of a loop has its row-pass / column-pass launches bracketed by HIP events (1: every one).
    // An event record is a packet of its own in the stream: about 5-6 us of dispatch gap each -- four of them per fit iteration
    // were 3.5 % of one rank's 0.65 ms shard iteration (profiles/r06_timelines_shard.txt), so bench.py samples every 4th
    int profile_every = 1;
    int64_t profile_seq = 0;
    std::vector<EventPair> ev_row, ev_col, ev_tail;      // ev_tail: the column-split tail + slabs part of a hybrid row pass

    // row shards over the GPUs of a node (klnmf_comm_*, klnmf_run_sharded): this rank's RCCL communicator
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_size = 1;
    double *comm_scratch = nullptr;       // 8 doubles on the device, owned by the communicator (not by a problem)
    hipStream_t comm_stream = nullptr;        // all-reduces of the parts before the last one (overlap)
    hipEvent_t ev_part[kPostMaxParts] = {}, ev_ar[kPostMaxParts] = {};
};

// A mask (presence.hip.h; dense, KLNMF_PREC_F64 / F32) of a context's problem or of all B problems of a batch (batch.hip.h has the
// [B] layout): the presence matrices P [B][n][M] -- taken filled with 1 by the first upload --, S [B][M][k] and D [B][k][M] of the two
// collapsed denominators, D's row-chunk slabs, and once for all B the modalities' column bounds (host and device) and the per-column
// modality index.  pres_M > 0 IS "a mask is held" (KLNMF_Q_PRESENCE).  The blocks are the owner's (DeviceBlocks): they go with
// presence_drop or with the problem.
struct PresenceState {
    int pres_M = 0, pres_dchunks = 0;
    int64_t pres_bounds[kMaxMod + 1] = {};
    void *Pm = nullptr, *pres_S = nullptr, *pres_D = nullptr;
    void *pres_dbounds = nullptr, *pres_mod = nullptr, *pres_Dslab = nullptr;      // int64 [M + 1]; bytes [f]; double [B][chunks][k][M]
    bool presence() const { return pres_M > 0; }
    void forget_presence() { *this = PresenceState(); }      // (the blocks are gone or go with the owner's)
};

// ---- as long as a problem: the plan (plan.hip.h: every shape-derived count), every device buffer, and what uploads and setters
// leave on them.  Default-constructed by klnmf_set_problem* (behind free_all, before the new plan is stored) and by
// klnmf_release_problem.
struct ProblemState : ProblemPlan, PresenceState {
    DevSwitches sw;               // as klnmf_set_problem* read them; read afresh at every loop entry
    int64_t cap = 0;
    bool have_problem = false;
    int cur = 0;          // index of the current W buffer
    // where W and the dictionary master stood at the loop's entry (loop_open; fetch_results): they point into THIS problem's buffers
    int loop_start_cur = 0;
    int64_t loop_hswaps = 0;                  // H rules enqueued since the loop's entry (how many the device executed: n_done -- fetch_results)
    float *loop_h0 = nullptr, *loop_h1 = nullptr;      // H32 / H32alt as the loop found them

    // common device state
    DevState *st = nullptr;
    double *errors = nullptr;
    double *loss_xchg = nullptr;
    double2 *loss_red = nullptr;              // [kLossRedMax] pairs of the loss slices (k_slab_sum -> k_post; 16-bit modes)

    // exact modes (T = double or float)
    void *V = nullptr, *W[2] = {nullptr, nullptr}, *H = nullptr, *Q = nullptr;
    void *Npart = nullptr, *numer = nullptr;
    double *loss_part = nullptr;
    void *Wpart = nullptr;
    // a weighted problem (weighted.hip.h; dense, KLNMF_PREC_F64 / F32): the n x f weights Om beside V -- allocated filled with 1
    // by the first klnmf_upload_weights, dropped by klnmf_clear_weights -- and the denominators' slabs and sums, laid out as
    // Npart / numer / Wpart are.  Om != nullptr IS "the current problem is weighted" (klnmf_query KLNMF_Q_WEIGHTED).
    void *Om = nullptr, *Dpart = nullptr, *denom = nullptr, *WDpart = nullptr;
    // a beta-divergence problem (beta.hip.h; dense, KLNMF_PREC_F64 / F32; klnmf_set_divergence): beta != 1 IS "the loop runs the
    // beta rules"; B is the second n x f matrix of the ratio pass (A lives in Q); the sums of H's rows before their
    // normalisation go to hpart [k][hseg_n] (taken by klnmf_set_divergence where the problem has one segment and holds none).  The denominators' slabs and sums are the weighted problem's (Dpart, denom, WDpart): taken by whichever
    // of klnmf_upload_weights and klnmf_set_divergence comes first, dropped when neither needs them.
    double beta = 1.0;
    void *Bt = nullptr;
    // the exchange buffers (loss_xchg, numer / numerF) are a caller's: klnmf_bind_exchange -- a group's member, a loop sequenced
    // over torch.distributed -- until the group's end or the next klnmf_set_problem*
    bool exchange_bound = false;
    // a masked problem: PresenceState, taken by the first klnmf_upload_presence*, dropped by klnmf_clear_weights; a problem holds
    // Om or P, never both
    float *x3_hs = nullptr, *x3_qr = nullptr;     // per-component H scales; per-row ratio scales of the column pass
    unsigned *x3_xmax = nullptr;                  // per-component maxima of W_new qr (bit patterns of non-negative floats)
    double *x3_loss = nullptr;                    // one loss partial per 64 rows

    // CSR input in the exact modes (sparse.hip.h): structure of X in CSR and CSC order, ratio values, H^T
    int64_t *sp_indptr = nullptr, *sp_indices = nullptr, *csc_indptr = nullptr, *csc_rows = nullptr, *csc_perm = nullptr;
    void *sp_data = nullptr, *sp_q = nullptr, *HT = nullptr;
    double *sp_row_loss = nullptr, *sp_wpart = nullptr, *sp_prod = nullptr;
    // ... blocked for the L2 (sparseb.hip.h; k <= 512): int32 copies of the indices, column blocks of the CSR order and row blocks
    // of the CSC order with their pointers, the slabs of partial sums
    int *sp_idx32 = nullptr, *csc_rows32 = nullptr, *csc_perm32 = nullptr;
    int64_t *sp_blkptr = nullptr, *csc_blkptr = nullptr;      // [n][cb + 1], [f][rb + 1]
    double *sp_loss_part = nullptr;           // [cb][n]
    void *sp_G = nullptr, *sp_NT = nullptr;   // [cb][n][k], [rb][f][k]
    int *sp_bad = nullptr;
    int64_t *csc_work = nullptr;      // workspace of the device-side CSC build (csc.hip.h, CscWork: klnmf_upload_csr_rows)
    double *hpart = nullptr;          // exact modes, long rows: [k][hseg_n] partial row sums of the H rule / of the CSR loss term

    // 16-bit mode
    float *Gpart = nullptr;                   // [row_chunks][nrt * 32][KP] partial Q.H^T (hybrid update pass: the tail's slabs)
    unsigned char *W8 = nullptr;              // e4m3 image of W_new for the fp8 x fp8 column pass (colq8x.hip.h; plan: w8)
    float *w8s = nullptr;                     // [KP] power-of-two scales of the e4m3 image
    void *VtA = nullptr;          // V as 32 x 32 fp16 tiles in the row pass's accumulator order (k_tile_V)
    unsigned char *Qt = nullptr;  // ratio tiles the row pass leaves for the column pass
    uint2 *q8_list = nullptr;                 // [kQ8ListCap] saturated ratio entries of the current iteration (colq.hip.h)
    float *mon_part = nullptr, *mon_spread = nullptr;      // the fp8 monitor (monitor.hip.h): partial sums of the monitored iteration
    float *W32[2] = {nullptr, nullptr};
    opnd_t *Wb[2] = {nullptr, nullptr};
    float *H32 = nullptr;
    // ---- one launch behind the column pass (post.hip.h) ----
    float *H32alt = nullptr;                  // the dictionary master is ping-pong there: k_post reads H32, writes H32alt, then they swap
    unsigned *w8tab = nullptr;                // [kW8TabRows][KP] maxima of the conversion kernel (k_post: -> w8s_next, emptied)
    float *w8s_next = nullptr;                // [KP] scales of the NEXT image: k_post writes them, then w8s / w8s_next swap
    opnd_t *Ht4 = nullptr;
    int kc = -1;                 // eps-carrying pad component of the ping-pong path (k_update_pack_H), -1: none; kc = kc_shape only
                                 // while the carrier pair fits fp16 (choose_eps_carrier)
    double *hsum = nullptr;
    // per-component power-of-two scales of the fp16 operand images (mfma.hip.h, opnd_t), [KP] each: of the current images;
    // hs-based (from the dictionary's row sums); the constant 2^-13 of a row-normalised dictionary; measured from a W
    float *tcur = nullptr, *t_hs = nullptr, *t_unit = nullptr;
    unsigned *wmax = nullptr;
    float *NpartF = nullptr, *numerF = nullptr;
    double2 *loss_part2 = nullptr;

    double v_scale = 1.0;           // storage factor c of the 16-bit V (power of two)
    double v_max = 0.0;          // the maximum announced with klnmf_set_v_max (0: none)
    bool v_uploaded = false;
    bool images_measured = false;    // the current images carry measured scales: valid for one update (see opnd_t)
    bool w_is_init = false;          // the current W is W0 = V.H0^T of klnmf_init_W, untouched since: a dictionary set NOW still meets
                                     // ratios of about f / k on its first update (the ratio scale of k_ratio_scale must stay on)
    // the refusal counters of DevState (v_overflow, op_range) change only on uploads and image measurements: they are read
    // back (one copy + synchronisation) only when one of those happened since the last check
    bool refusals_dirty = true;
};

// ---- as long as a loop: default-constructed at every loop entry (begin_fp8_loop), and nowhere else -- q8_loop, ne_loop and the
// iteration counts below answer klnmf_query on a context whose problem has been released or replaced, until the next loop entry.
struct LoopState {
    // fp8 ratio tiles: q8_loop: this loop's data allow them (decided at the loop's entry; q8_ok of the plan: the shape does); they
    // are used from the loop's third iteration on (the first updates from W0 = V.H0^T can carry ratios far beyond fp8's range).
    bool q8_loop = false;
    int64_t iter_in_loop = 0;
    // what the loop actually ran (klnmf_query): iterations whose ratio tiles were fp8, whose column pass was fp8 x fp8
    int64_t stat_q8_tiles = 0, stat_col8 = 0;
    bool stat_mon_gave_up = false;
    bool w8_meas = false;                     // the maxima table holds a measurement of this loop
    bool ne_loop = false;                     // this loop's fp8-tile update passes drop the numerator's eps (NE kernels; begin_fp8_loop)
    bool last_row_ne = false;                 // ... and the update pass just launched was one of them (its loss needs DevState.corr_eps)
    // the fp8 monitor (monitor.hip.h): what k_post is to do with the monitored iteration's partial sums
    bool mon_pending = false;                 // this iteration's first summing launch turns the partial sums into the statistic
    bool mon_dry_pending = false;             // ... and it was the dry run of the loop's second iteration: poll before the third
    int mon_ncols = 0; float mon_noise_scale = 0.f;
    int64_t mon_checks = 0;
    bool poll_inflight = false, poll_agreed = false;
    // the 16-bit mode's data condition (below KL / sum(V) of about 2e-3 the f16 operands' own noise can pass 1e-4
    // of the loss): sum of V over ALL shards as the loop's entry was given it (stored units; < 0: this context's own)
    double loop_sum_x_all = -1.0;
    // single-context fit loops: the loss reduction + stop decision of an iteration ride in the slab-sum launch behind the
    // column pass (k_sum_partials_f32) instead of a launch of their own behind the row pass; set by piece_rowpass,
    // consumed by the next fast_colpass.  KLNMF_LOSS_DEFER=0: off.
    LossArgs pending_loss{nullptr, 0, 0.0, nullptr, 0, nullptr, 0.0, nullptr, 0};
    bool conv_ran = false;                    // this iteration's conversion ran: k_post derives the next scales
    bool piece_split = false, piece_use8 = false;      // loop in pieces: the numerator was produced in parts (klnmf_iter_colpass_part)
    unsigned sr_launches = 0;        // row pass launches of the current loop (the seeds of the tiles' stochastic rounding)
    bool x3_ready = false;           // Q, x3_qr and x3_xmax are the last fused row pass's (its column pass may run)
    bool prof_now = false;           // this iteration's launches are bracketed (set by piece_rowpass)
    bool pieces_open = false;        // klnmf_loop_begin* has opened a loop whose pieces the caller enqueues; until klnmf_loop_end,
                                     // the problem's end (free_all) or the next loop entry; never behind klnmf_group_run
    bool sharded_loop = false;       // the open loop's pieces are exchanged between row shards by the caller (klnmf_loop_begin on a
                                     // communicator, klnmf_loop_begin_sharded / _agreed; until klnmf_loop_end): no weights may arrive
};

// ---- the last loop's record as fetch_results wrote it (klnmf_query / klnmf_query_f64): never reset, overwritten whole by the next
// fetch_results -- readable on a context whose problem has been released or replaced.  (DevState, where the counters come from,
// is emptied by the next entry point.)
struct LoopRecord {
    int64_t stat_w8_sat = 0, stat_w8_fallbacks = 0, stat_q8_sat = 0, stat_q8_unfixed = 0;
    int64_t stat_mon_checks = 0, stat_mon_trips = 0;
    double stat_mon_max = 0.0, stat_mon_dbg[3] = {0, 0, 0}, stat_mon_spread = 1.0;
    double stat_kl_over_sumv = -1.0;          // the final KL / sum(V) (KLNMF_QF_KL_OVER_SUM_V; < 0: no loop yet / exact mode)
};

}  // namespace klnmf_host

struct klnmf_ctx : ContextState, ProblemState, LoopState, LoopRecord {
    // fp8 ratio tiles in this iteration?  k > 256 (FUSED row pass, KSPLIT = 2 column pass) has only the fp8 x fp8 column pass
    // for them: there the W image's scales must have been measured (the loop's second iteration does that)
    bool q8() const { return q8_loop && iter_in_loop >= 2 && (!big || (W8 != nullptr && w8_meas)); }
    // the exact modes' storage, loop and kernels; KLNMF_PREC_BF16X3 is the fp32 side of them with the dense contractions on
    // the split-operand bf16 kernel (split3.hip.h); KLNMF_PREC_F16X3 the same storage and step kernels, its fit and transform
    // loop on the fused split-fp16 kernels where x3_fused() (f16x3.hip.h)
    bool is_exact() const { return prec_is_exact(prec); }
    // fp32 storage (the exact modes other than f64)
    bool is_f32() const { return prec == KLNMF_PREC_F32 || prec == KLNMF_PREC_BF16X3 || prec == KLNMF_PREC_F16X3; }
    // KLNMF_PREC_F16X3 on dense input with k <= 256: the loop's row pass is k_rowpass_x3 and its column pass k_colpass_x3
    // (k > 256 and CSR input: the bf16x3 kernels / the fp32 sparse kernels)
    bool x3_fused() const { return x3; }
    size_t esize() const { return prec_esize(prec); }
    bool weighted() const { return Om != nullptr; }
    bool beta_on() const { return beta != 1.0; }
    // both rules contract a numerator and a denominator matrix (k_gemm_dual): the weights, or B of a beta problem
    bool dual() const { return weighted() || beta_on(); }
    const void *den_matrix() const { return beta_on() ? Bt : Om; }
    // the exponent of the beta rules' factor (majorise-minimise: <= 1)
    double beta_gamma() const { return beta < 1.0 ? 1.0 / (2.0 - beta) : (beta <= 2.0 ? 1.0 : 1.0 / (beta - 1.0)); }

    // The problem ends: its blocks go back to the cache and its state to the defaults.  Callers have synchronised the stream: no
    // kernel of this context still touches the blocks.
    void free_all() {
        release_all();
        for (auto *v : {&ev_row, &ev_col, &ev_tail}) {
            for (auto &e : *v) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
            v->clear();
        }
        static_cast<ProblemState &>(*this) = ProblemState();
        sharded_loop = false;      // (a loop that was left open went with its problem)
        pieces_open = false;
    }
};

namespace klnmf_host {

inline void use(klnmf_ctx *c) {
    if (!c) fail(KLNMF_ERR_ARG, "null context");
    HIPCHK(hipSetDevice(c->device));
}
inline void comm_release(klnmf_ctx *c) {
    if (c->comm) { (void)rccl().CommDestroy(c->comm); c->comm = nullptr; }
    if (c->comm_stream) { (void)hipStreamDestroy(c->comm_stream); c->comm_stream = nullptr; }
    for (int p = 0; p < kPostMaxParts; ++p) {
        if (c->ev_part[p]) { (void)hipEventDestroy(c->ev_part[p]); c->ev_part[p] = nullptr; }
        if (c->ev_ar[p]) { (void)hipEventDestroy(c->ev_ar[p]); c->ev_ar[p] = nullptr; }
    }
    if (c->comm_scratch) { (void)hipFree(c->comm_scratch); c->comm_scratch = nullptr; }
    c->comm_rank = 0; c->comm_size = 1;
}
inline void need_problem(klnmf_ctx *c) {
    use(c);
    if (!c->have_problem) fail(KLNMF_ERR_ARG, "klnmf_set_problem has not been called");
}

inline EventPair begin_event(klnmf_ctx *c, std::vector<EventPair> &v) {
    EventPair e{};
    HIPCHK(hipEventCreate(&e.a));
    HIPCHK(hipEventCreate(&e.b));
    HIPCHK(hipEventRecord(e.a, c->stream));
    v.push_back(e);
    return e;
}

// ---- what the units call across each other (default arguments live here) ---------------------------------------------------------
enum PostMode { POST_FULL = 0, POST_SUM = 1, POST_RULE = 2 };
static const LossArgs kNoLoss{nullptr, 0, 0.0, nullptr, 0, nullptr, 0.0, nullptr, 0, 0};
struct Refusals { int v_overflow = 0, op_range = 0; };
// api_context.hip
DevSwitches problem_switches();
// ... what contexts and batches share.  dst[row0 + i, col0 + j] = scale * src[row_idx ? row_idx[i] : i, j] on a matrix of row
// length dld (k_place_V); dst[rows, cols] = mul * src[rows, cols] (k_copy_2d); `count` ones (k_fill) -- types by d64 / s64
void place_rows(hipStream_t stream, void *dst, bool d64, int64_t dld, const void *dsrc, bool s64, int64_t rows, int64_t cols, int64_t ld,
                int64_t row0, int64_t col0, double scale, const int64_t *row_idx);
void copy_2d_any(hipStream_t stream, void *dst, bool d64, int64_t dld, const void *src, bool s64, int64_t sld, int64_t rows, int64_t cols,
                 double mul = 1.0);
void fill_ones(hipStream_t stream, void *dst, bool f64, int64_t count);
// ... the mask of B problems of the shape n x f x k in `prec` (a context: B = 1, problem 0), blocks from `a`, state in `ps`.  Every
// check comes before anything is taken or written: a refused call leaves the owner as it was.
struct MaskDims { int64_t n, f, k; int B, prec; };
void presence_check_args(const std::string &who, const MaskDims &d, int64_t rows, int64_t row0, bool rows_ok, const int64_t *col_bounds,
                         int n_mod);
void presence_check_bounds(const PresenceState &ps, const std::string &who, const char *owner, const int64_t *col_bounds, int n_mod);
void presence_take(DeviceBlocks &a, PresenceState &ps, const MaskDims &d, const int64_t *col_bounds, int n_mod);
void presence_upload(DeviceBlocks &a, PresenceState &ps, const MaskDims &d, int p, const void *src, int dtype, int64_t rows, int64_t ld,
                     int64_t row0);
void presence_rows_check(DeviceBlocks &a, const std::string &who, const int64_t *drow_idx, int64_t rows, int64_t src_rows);
void presence_gather(DeviceBlocks &a, PresenceState &ps, const MaskDims &d, int p, const void *dP, int dtype, int64_t ld,
                     const int64_t *drow_idx, int64_t rows, int64_t row0, const PresenceCols &cols);
void presence_drop(DeviceBlocks &a, PresenceState &ps);
// ... the upload of ONE CSR problem (a context's, or problem p of a CSR batch): its arrays on the device and the steps both owners
// run on them.  indptr .. csc_work hold the problem's own positions 0 .. nnz; blkptr == nullptr: no blocked regime.  A batch points
// idx32 / rows32 / perm32 and the block pointers at problem p's part of its concatenated arrays and moves the positions afterwards.
struct CsrParts {
    int64_t n, f, nnz;
    int prec;
    int64_t *indptr, *indices, *csc_indptr, *csc_rows, *csc_perm, *csc_work;
    void *data;
    int cb, rb;
    int64_t cb_cols, rb_rows;
    int64_t *blkptr, *cblkptr;
    int *idx32, *rows32, *perm32, *bad;
};
int64_t csr_csc_work_elems(int64_t nnz);      // int64 elements of csc_work for a problem of nnz stored entries (csc.hip.h, CscWork)
void csr_leave_empty(hipStream_t stream, const CsrParts &v);
void csr_csc_build(hipStream_t stream, const CsrParts &v);
void csr_blocked_setup(hipStream_t stream, const CsrParts &v, const std::string &msg);
void csr_gather_rows(DeviceBlocks &a, const CsrParts &v, const std::string &who, int n_mod, const int64_t *const *indptr,
                     const int32_t *const *indices, const void *const *data, const int *dtype, const int64_t *col_bounds,
                     const double *scale, int64_t src_rows, const int64_t *drow_idx, int64_t rows,
                     const std::function<void()> &before_write);
void reset_state(klnmf_ctx *c);
void fast_pack_H(klnmf_ctx *c, const unsigned *wmax = nullptr);
void measure_and_pack(klnmf_ctx *c, bool from_init = false);
size_t dt_size(int dtype);
void *stage_to_device(klnmf_ctx *c, const void *src, int dtype, int64_t count);
// api_loop.hip
void piece_rowpass(klnmf_ctx *c, int fit, const double *fused_tol = nullptr, bool defer_to_post = false);
void piece_decide(klnmf_ctx *c, double tol_abs);
void piece_colpass(klnmf_ctx *c);
void piece_update_H(klnmf_ctx *c);
void piece_fit_tail(klnmf_ctx *c);
void fetch_results(klnmf_ctx *c, double *errors_out, int64_t *n_done, int *stopped);
void loop_open(klnmf_ctx *c);
void loop_advance(klnmf_ctx *c, bool poll, bool agreed);
void local_iteration(klnmf_ctx *c, int fit, double tol_abs);
bool stop_fired(klnmf_ctx *c);
bool fp8_poll_due(const klnmf_ctx *c);
bool fused_w8_stage(klnmf_ctx *c);
void launch_monitor(klnmf_ctx *c, bool use8);
void fused_colpass_part(klnmf_ctx *c, const klnmf_ctx::PartCfg &p, bool use8);
void launch_post(klnmf_ctx *c, PostMode mode, const klnmf_ctx::PartCfg *parts, int nparts, const LossArgs &la, bool decide, bool use8,
                 bool last_sum);
Refusals read_refusals(klnmf_ctx *c);
void raise_refusals(klnmf_ctx *c, const Refusals &r);
void check_v_overflow(klnmf_ctx *c);
void begin_fp8_loop(klnmf_ctx *c, double sum_x_global = -1.0, double cells_global = -1.0, double nnz_global = -1.0, int ok_all = -1);
void refuse_weighted(const klnmf_ctx *c, const char *who);
// ... the pieces of a beta iteration (api_beta.hip runs its entry points on them): A, B (and with `loss` the cost, into loss_xchg;
// fused_tol: with the stop rule) at (W[widx], H); the W rule from them; the H rule with W[widx], its normalisation and the
// compensation on W[widx]'s columns (from_slabs: as piece_fit_tail chooses)
void beta_ratio(klnmf_ctx *c, int widx, bool loss, const double *fused_tol = nullptr);
void beta_rule_W(klnmf_ctx *c);
void beta_rule_H(klnmf_ctx *c, int widx, bool from_slabs);
// api_comm.hip
bool comm_multi(const klnmf_ctx *c);
void comm_loop_entry(klnmf_ctx *c);
void comm_iteration(klnmf_ctx *c, int fit, double tol_abs);

}  // namespace klnmf_host
