// libklnmf.so, unit 5 of 6: a group of contexts -- one per row shard, on one device each (a device may repeat) -- driven from ONE
// host thread (klnmf_group_*).  The numerator of the H rule and the loss are exchanged by the two launches of group.hip.h, which
// read the peers' buffers directly; the streams are ordered by events only.  DESIGN.md section 8 has the design and its argument.
#include <chrono>

#include "ctx.hip.h"
#include "group.hip.h"

struct klnmf_group {
    int n = 0;
    std::vector<klnmf_ctx *> ctxs;       // rank order = row order of the shards
    std::vector<int> dev;
    std::vector<hipStream_t> streams;    // the contexts' streams (selftest: streams of its own)
    bool f64 = false;                    // numerator type: double (KLNMF_PREC_F64) or float
    bool fine = false;                   // the buffers are fine-grained device memory (some pair of members on distinct devices)
    int64_t valid = 0;                   // elements of the numerator that carry data (klnmf_exchange_layout)
    std::vector<void *> numer, loss, slot, tab;   // per member, on its device: numerator, loss pair, private loss slot, pointer table
    std::vector<void *> own_numer, own_loss;      // the contexts' own exchange buffers (re-bound by klnmf_group_destroy)
    std::vector<hipEvent_t> ev_col, ev_a, ev_b;   // per member: column pass done, phase A done, phase B done
    std::vector<double> enqueue_ms;               // host time of each iteration's enqueue in the last klnmf_group_run
};

namespace klnmf_host {

static void group_free(klnmf_group *g) {
    for (int r = 0; r < (int)g->dev.size(); ++r) {
        (void)hipSetDevice(g->dev[r]);
        for (auto *v : {&g->numer, &g->loss, &g->slot, &g->tab})
            if (r < (int)v->size() && (*v)[r]) (void)hipFree((*v)[r]);
        for (auto *v : {&g->ev_col, &g->ev_a, &g->ev_b})
            if (r < (int)v->size() && (*v)[r]) (void)hipEventDestroy((*v)[r]);
    }
    g->numer.clear(); g->loss.clear(); g->slot.clear(); g->tab.clear();
    g->ev_col.clear(); g->ev_a.clear(); g->ev_b.clear();
}

// Peer access for every pair of distinct devices (refused, naming the pair, where the hardware has none)
static void group_enable_peers(const std::vector<int> &dev) {
    for (size_t a = 0; a < dev.size(); ++a)
        for (size_t b = 0; b < dev.size(); ++b) {
            if (dev[a] == dev[b]) continue;
            int can = 0;
            HIPCHK(hipDeviceCanAccessPeer(&can, dev[a], dev[b]));
            if (!can)
                fail(KLNMF_ERR_UNSUPP, "klnmf_group: device " + std::to_string(dev[a]) + " cannot access device " +
                                           std::to_string(dev[b]) + " (hipDeviceCanAccessPeer)");
            HIPCHK(hipSetDevice(dev[a]));
            const hipError_t e = hipDeviceEnablePeerAccess(dev[b], 0);
            if (e == hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
            else HIPCHK(e);
        }
}

// Buffers (numerator of `alloc_count` elements, loss pair, private slot), pointer tables and events of every member.  The
// numerator and loss buffers are what the peers read: fine-grained device memory when some member sits on another device.
static void group_alloc(klnmf_group *g, int64_t alloc_count) {
    const int N = g->n;
    std::vector<int> d = g->dev;
    std::sort(d.begin(), d.end());
    g->fine = std::unique(d.begin(), d.end()) - d.begin() > 1;
    if (g->fine) group_enable_peers(g->dev);
    const size_t es = g->f64 ? 8 : 4;
    const size_t nbytes = (size_t)std::max<int64_t>(alloc_count, 4) * es;
    g->numer.assign(N, nullptr); g->loss.assign(N, nullptr); g->slot.assign(N, nullptr); g->tab.assign(N, nullptr);
    g->ev_col.assign(N, nullptr); g->ev_a.assign(N, nullptr); g->ev_b.assign(N, nullptr);
    for (int r = 0; r < N; ++r) {
        HIPCHK(hipSetDevice(g->dev[r]));
        if (g->fine) {
            HIPCHK(hipExtMallocWithFlags(&g->numer[r], nbytes, hipDeviceMallocFinegrained));
            HIPCHK(hipExtMallocWithFlags(&g->loss[r], 2 * sizeof(double), hipDeviceMallocFinegrained));
        } else {
            HIPCHK(hipMalloc(&g->numer[r], nbytes));
            HIPCHK(hipMalloc(&g->loss[r], 2 * sizeof(double)));
        }
        HIPCHK(hipMemset(g->numer[r], 0, nbytes));
        HIPCHK(hipMemset(g->loss[r], 0, 2 * sizeof(double)));
        HIPCHK(hipMalloc(&g->slot[r], 2 * sizeof(double)));
        HIPCHK(hipMalloc(&g->tab[r], 2 * (size_t)N * sizeof(void *)));
        HIPCHK(hipEventCreateWithFlags(&g->ev_col[r], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&g->ev_a[r], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&g->ev_b[r], hipEventDisableTiming));
    }
    std::vector<void *> t(2 * (size_t)N);
    for (int q = 0; q < N; ++q) { t[q] = g->numer[q]; t[N + q] = g->loss[q]; }
    for (int r = 0; r < N; ++r) {
        HIPCHK(hipSetDevice(g->dev[r]));
        HIPCHK(hipMemcpy(g->tab[r], t.data(), t.size() * sizeof(void *), hipMemcpyHostToDevice));
    }
}

static void wait_peers(klnmf_group *g, int r, const std::vector<hipEvent_t> &ev) {
    for (int q = 0; q < g->n; ++q)
        if (q != r) HIPCHK(hipStreamWaitEvent(g->streams[r], ev[q], 0));
}

// Phase A / B of member r (the caller has made r's device current and enqueued the waits)
static void group_phase_a(klnmf_group *g, int r, int64_t count, const DevState *st) {
    const int N = g->n;
    const int vec = g->f64 ? 2 : 4;
    const int64_t sl = (count / vec + N - 1) / N + 1;                // vectors of the longest slice (bound)
    const dim3 grid((unsigned)grid_for(sl, kGroupThreads, 1024));
    void **tab = (void **)g->tab[r];
    if (g->f64)
        hipLaunchKernelGGL(k_group_reduce<double>, grid, dim3(kGroupThreads), 0, g->streams[r], (double *const *)tab,
                           (double *const *)(tab + N), N, r, count, (double *)g->slot[r], st);
    else
        hipLaunchKernelGGL(k_group_reduce<float>, grid, dim3(kGroupThreads), 0, g->streams[r], (float *const *)tab,
                           (double *const *)(tab + N), N, r, count, (double *)g->slot[r], st);
    HIPCHK(hipGetLastError());
}

static void group_phase_b(klnmf_group *g, int r, int64_t count, const DevState *st) {
    const int N = g->n;
    const int vec = g->f64 ? 2 : 4;
    const int64_t sl = (count / vec + N - 1) / N + 1;
    const dim3 grid((unsigned)grid_for(sl, kGroupThreads, 512), (unsigned)N);
    void **tab = (void **)g->tab[r];
    if (g->f64)
        hipLaunchKernelGGL(k_group_gather<double>, grid, dim3(kGroupThreads), 0, g->streams[r], (double *const *)tab,
                           (double *)g->loss[r], N, r, count, (const double *)g->slot[r], st);
    else
        hipLaunchKernelGGL(k_group_gather<float>, grid, dim3(kGroupThreads), 0, g->streams[r], (float *const *)tab,
                           (double *)g->loss[r], N, r, count, (const double *)g->slot[r], st);
    HIPCHK(hipGetLastError());
}

// Every member's phase A behind every peer's ev_col, then every member's phase B behind every peer's phase A.  `tail(r)` is
// enqueued on member r's stream right behind its phase B (the stop rule, the H rule, the advance of the loop).  Host order is
// a topological order of the dependencies: every event is recorded before any wait on it is enqueued (streams of one device
// share its hardware queues -- GPU_MAX_HW_QUEUES -- so a wait ahead of its record in a shared queue would never be satisfied).
template <typename Tail>
static void group_exchange(klnmf_group *g, int64_t count, const std::vector<const DevState *> &st, Tail &&tail) {
    for (int r = 0; r < g->n; ++r) {
        HIPCHK(hipSetDevice(g->dev[r]));
        wait_peers(g, r, g->ev_col);
        group_phase_a(g, r, count, st[r]);
        HIPCHK(hipEventRecord(g->ev_a[r], g->streams[r]));
    }
    for (int r = 0; r < g->n; ++r) {
        HIPCHK(hipSetDevice(g->dev[r]));
        wait_peers(g, r, g->ev_a);
        group_phase_b(g, r, count, st[r]);
        HIPCHK(hipEventRecord(g->ev_b[r], g->streams[r]));
        tail(r);
    }
}

static void group_check(klnmf_group *g) {
    if (!g || g->n < 1) fail(KLNMF_ERR_ARG, "null or empty group");
}

// Loop entry, agreed on the host before anything is enqueued: every member's refusals are read first, and if any member is
// refused every member fails together; the fp8 decision is taken from the sums over all shards (ShardedKLNMF.begin's decision).
static void group_loop_entry(klnmf_group *g) {
    const int N = g->n;
    double sum_v = 0.0, cells = 0.0, nnz = 0.0;
    int shape_all = 1;
    std::vector<Refusals> refs(N);
    for (int r = 0; r < N; ++r) {
        klnmf_ctx *c = g->ctxs[r];
        need_problem(c);
        if (!c->is_exact() && c->v_scale != g->ctxs[0]->v_scale)
            fail(KLNMF_ERR_ARG, "klnmf_group_run: shard " + std::to_string(r) + " stores V with another factor than shard 0: "
                                "klnmf_set_v_max must be given the maximum over all shards");
        c->refusals_dirty = true;
        refs[r] = read_refusals(c);
        DevState ds{};
        HIPCHK(hipMemcpyAsync(&ds, c->st, sizeof(DevState), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        sum_v += ds.sum_x / c->v_scale;
        cells += (double)c->n * (double)c->f;
        nnz += ds.nnz_x;
        if (!c->q8_ok) shape_all = 0;
    }
    for (int r = 0; r < N; ++r) {
        if (refs[r].v_overflow == 0 && refs[r].op_range == 0) continue;
        try {
            raise_refusals(g->ctxs[r], refs[r]);
        } catch (const ApiError &e) {
            fail(e.code, "shard " + std::to_string(r) + " of the group: " + e.msg + " -- the group's loop is refused on every shard");
        }
    }
    for (int r = 0; r < N; ++r) {
        raise_refusals(g->ctxs[r], refs[r]);          // (passes: the state is clean, the entry below reads nothing back)
        const int rc = klnmf_loop_begin_agreed(g->ctxs[r], sum_v, cells, nnz, shape_all);
        if (rc != KLNMF_OK) fail(rc, "shard " + std::to_string(r) + ": " + g_err);
        g->ctxs[r]->pieces_open = false;       // (the pieces are klnmf_group_run's own, not a caller's: nothing stays open behind
                                               // it, whichever way it ends)
    }
}

}  // namespace klnmf_host

extern "C" {

int klnmf_group_create(klnmf_group **out, klnmf_ctx *const *ctxs, int n) {
    return guarded([&] {
        if (!out) fail(KLNMF_ERR_ARG, "klnmf_group_create: null out");
        *out = nullptr;
        if (!ctxs || n < 1) fail(KLNMF_ERR_ARG, "klnmf_group_create: no contexts");
        for (int r = 0; r < n; ++r) {
            need_problem(ctxs[r]);
            for (int q = 0; q < r; ++q)
                if (ctxs[q] == ctxs[r]) fail(KLNMF_ERR_ARG, "klnmf_group_create: a context appears twice");
        }
        const klnmf_ctx *c0 = ctxs[0];
        for (int r = 0; r < n; ++r) {
            const klnmf_ctx *c = ctxs[r];
            if (c->sparse != c0->sparse)
                fail(KLNMF_ERR_ARG, "klnmf_group_create: shard " + std::to_string(r) + " holds a " + (c->sparse ? "CSR" : "dense") +
                                        " problem, shard 0 a " + (c0->sparse ? "CSR" : "dense") + " one: the members must be all dense or all CSR");
            if (c->f != c0->f || c->k != c0->k || c->prec != c0->prec || c->cap != c0->cap)
                fail(KLNMF_ERR_ARG, "klnmf_group_create: shard " + std::to_string(r) + " differs from shard 0 in f, k, precision or capacity");
            if (c->comm != nullptr) fail(KLNMF_ERR_ARG, "klnmf_group_create: shard " + std::to_string(r) + " holds an RCCL communicator");
            refuse_weighted(c, "klnmf_group_create");
        }
        klnmf_group *g = new klnmf_group();
        try {
            g->n = n;
            g->ctxs.assign(ctxs, ctxs + n);
            g->f64 = c0->prec == KLNMF_PREC_F64;
            int64_t stride = 0, alloc_count = 0;
            void *lp = nullptr, *np = nullptr;
            int is64 = 0;
            for (int r = 0; r < n; ++r) {
                g->dev.push_back(ctxs[r]->device);
                g->streams.push_back(ctxs[r]->stream);
                HIPCHK(hipSetDevice(ctxs[r]->device));
                HIPCHK(hipStreamSynchronize(ctxs[r]->stream));
                if (klnmf_exchange_buffers(ctxs[r], &lp, &np, &alloc_count, &is64) != KLNMF_OK ||
                    klnmf_exchange_layout(ctxs[r], &stride, &g->valid) != KLNMF_OK)
                    fail(KLNMF_ERR_ARG, g_err);
                g->own_loss.push_back(lp);
                g->own_numer.push_back(np);
            }
            group_alloc(g, alloc_count);
            for (int r = 0; r < n; ++r)
                if (klnmf_bind_exchange(ctxs[r], g->loss[r], g->numer[r]) != KLNMF_OK) fail(KLNMF_ERR_ARG, g_err);
        } catch (...) {
            for (int r = 0; r < (int)g->own_loss.size(); ++r) {
                ctxs[r]->loss_xchg = (double *)g->own_loss[r];
                ctxs[r]->exchange_bound = false;
                if (ctxs[r]->is_exact()) ctxs[r]->numer = g->own_numer[r]; else ctxs[r]->numerF = (float *)g->own_numer[r];
            }
            group_free(g);
            delete g;
            throw;
        }
        *out = g;
    });
}

int klnmf_group_destroy(klnmf_group *g) {
    return guarded([&] {
        if (!g) return;
        // the contexts go back to their own exchange buffers (unless a klnmf_set_problem has given them new ones since)
        for (int r = 0; r < g->n; ++r) {
            klnmf_ctx *c = g->ctxs[r];
            (void)hipSetDevice(c->device);
            (void)hipStreamSynchronize(c->stream);
            if (c->loss_xchg == g->loss[r]) { c->loss_xchg = (double *)g->own_loss[r]; c->exchange_bound = false; }
            if (c->is_exact() && c->numer == g->numer[r]) c->numer = g->own_numer[r];
            if (!c->is_exact() && c->numerF == g->numer[r]) c->numerF = (float *)g->own_numer[r];
        }
        group_free(g);
        delete g;
    });
}

int klnmf_group_run(klnmf_group *g, int64_t n_total, int64_t max_iter, int fit, double tol, double *errors_out,
                    int64_t *n_done, int *stopped) {
    return guarded([&] {
        group_check(g);
        const int N = g->n;
        int64_t rows = 0;
        for (int r = 0; r < N; ++r) {
            need_problem(g->ctxs[r]);
            refuse_weighted(g->ctxs[r], "klnmf_group_run");
            rows += g->ctxs[r]->n;
            if (g->ctxs[r]->loss_xchg != g->loss[r])
                fail(KLNMF_ERR_ARG, "klnmf_group_run: shard " + std::to_string(r) + " was given another problem since klnmf_group_create");
        }
        if (max_iter < 0 || max_iter > g->ctxs[0]->cap) fail(KLNMF_ERR_ARG, "max_iter out of range");
        if (n_total < rows) fail(KLNMF_ERR_ARG, "n_total smaller than the group's rows");
        group_loop_entry(g);
        const double tol_abs = tol * (double)n_total * (double)g->ctxs[0]->f;      // nmf.py:207 on the GLOBAL shape
        std::vector<const DevState *> st(N);
        for (int r = 0; r < N; ++r) st[r] = g->ctxs[r]->st;
        const int64_t count = fit ? g->valid : 0;                                     // a transform exchanges the loss only
        g->enqueue_ms.clear();
        for (int64_t it = 0; it < max_iter; ++it) {
            const auto t0 = std::chrono::steady_clock::now();
            // row pass | (fit) wait for every peer's phase B of the last iteration -- their reads of this member's numerator --
            // then the column pass.  The row pass is not held back: it writes the loss pair only behind this member's own
            // phase B, which came after every peer's phase A, the only reader of a peer's loss pair.
            for (int r = 0; r < N; ++r) {
                klnmf_ctx *c = g->ctxs[r];
                HIPCHK(hipSetDevice(c->device));
                piece_rowpass(c, fit);
                if (fit) {
                    if (it > 0) wait_peers(g, r, g->ev_b);
                    piece_colpass(c);
                }
                HIPCHK(hipEventRecord(g->ev_col[r], c->stream));
            }
            group_exchange(g, count, st, [&](int r) {
                klnmf_ctx *c = g->ctxs[r];
                piece_decide(c, tol_abs);              // identical inputs on every member -> identical decisions
                if (fit) piece_update_H(c);
                loop_advance(c, true, true);           // (as klnmf_iter_advance)
            });
            g->enqueue_ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            if (tol_abs > 0 && (it & 15) == 15) {
                HIPCHK(hipSetDevice(g->ctxs[0]->device));
                if (stop_fired(g->ctxs[0])) break;
            }
        }
        // results: every member's; shard 0's are reported, and every replica must agree with them bit for bit
        int64_t nd0 = 0;
        int st0 = 0;
        for (int r = 0; r < N; ++r) {
            klnmf_ctx *c = g->ctxs[r];
            HIPCHK(hipSetDevice(c->device));
            int64_t nd = 0;
            int sp = 0;
            fetch_results(c, r == 0 ? errors_out : nullptr, &nd, &sp);
            c->sharded_loop = false;               // (as klnmf_loop_end: the loop klnmf_loop_begin_agreed opened has ended)
            if (r == 0) { nd0 = nd; st0 = sp; }
            else if (nd != nd0 || sp != st0)
                fail(KLNMF_ERR_REPLICA, "klnmf_group_run: shard " + std::to_string(r) + " ran " + std::to_string(nd) +
                                            " updates, shard 0 " + std::to_string(nd0));
        }
        if (n_done) *n_done = nd0;
        if (stopped) *stopped = st0;
        if (fit) {
            const klnmf_ctx *c0 = g->ctxs[0];
            const int dt = g->f64 ? KLNMF_DT_F64 : KLNMF_DT_F32;
            const size_t bytes = (size_t)c0->k * (size_t)c0->f * (g->f64 ? 8 : 4);
            std::vector<unsigned char> h0(bytes), h(bytes);
            if (klnmf_get_H(g->ctxs[0], h0.data(), dt) != KLNMF_OK) fail(KLNMF_ERR_HIP, g_err);
            for (int r = 1; r < N; ++r) {
                if (klnmf_get_H(g->ctxs[r], h.data(), dt) != KLNMF_OK) fail(KLNMF_ERR_HIP, g_err);
                if (std::memcmp(h0.data(), h.data(), bytes) != 0)
                    fail(KLNMF_ERR_REPLICA, "klnmf_group_run: the dictionary of shard " + std::to_string(r) +
                                                " differs from shard 0's (device " + std::to_string(g->dev[r]) + " vs " +
                                                std::to_string(g->dev[0]) + "): the exchange did not deliver the same bits");
            }
        }
    });
}

int klnmf_group_enqueue_time(klnmf_group *g, int64_t *iterations, double *median_ms, double *max_ms) {
    return guarded([&] {
        group_check(g);
        std::vector<double> t = g->enqueue_ms;
        if (iterations) *iterations = (int64_t)t.size();
        std::sort(t.begin(), t.end());
        if (median_ms) *median_ms = t.empty() ? 0.0 : t[t.size() / 2];
        if (max_ms) *max_ms = t.empty() ? 0.0 : t.back();
    });
}

int klnmf_group_selftest(const int *devices, int n, int64_t count, int dtype, int *failed) {
    return guarded([&] {
        if (!devices || n < 1 || count < 0 || !failed || (dtype != KLNMF_DT_F32 && dtype != KLNMF_DT_F64))
            fail(KLNMF_ERR_ARG, "klnmf_group_selftest: bad arguments");
        *failed = 0;
        klnmf_group g;
        g.n = n;
        g.f64 = dtype == KLNMF_DT_F64;
        g.dev.assign(devices, devices + n);
        struct Streams {
            std::vector<int> dev; std::vector<hipStream_t> s;
            ~Streams() { for (size_t i = 0; i < s.size(); ++i) { (void)hipSetDevice(dev[i]); (void)hipStreamDestroy(s[i]); } }
        } own;
        try {
            for (int r = 0; r < n; ++r) {
                HIPCHK(hipSetDevice(devices[r]));
                hipStream_t s = nullptr;
                HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
                own.dev.push_back(devices[r]);
                own.s.push_back(s);
            }
            g.streams = own.s;
            group_alloc(&g, count);
            // values whose sum depends on the order of summation: large terms that cancel, small ones they swallow, subnormals
            const double pat64[] = {1e8, 1.0, -1e8, 4.9406564584124654e-324, 3.0e-310, 1e-8, -1.0, 0.1, 1e16, -1e16, 0.3, 2.5e-300};
            const float pat32[] = {1e8f, 1.0f, -1e8f, 1.4e-45f, 3.0e-39f, 1e-8f, -1.0f, 0.1f, 1e16f, -1e16f, 0.3f, 2.5e-38f};
            const int P = 12;
            auto val64 = [&](int q, int64_t i) { return pat64[(i * 7 + q * 5 + (i >> 3)) % P]; };
            auto val32 = [&](int q, int64_t i) { return pat32[(i * 7 + q * 5 + (i >> 3)) % P]; };
            const size_t es = g.f64 ? 8 : 4;
            std::vector<std::vector<unsigned char>> host(n, std::vector<unsigned char>((size_t)count * es + 16));
            std::vector<double> lossv(2 * (size_t)n);
            for (int q = 0; q < n; ++q) {
                for (int64_t i = 0; i < count; ++i) {
                    if (g.f64) ((double *)host[q].data())[i] = val64(q, i);
                    else ((float *)host[q].data())[i] = val32(q, i);
                }
                lossv[2 * q] = pat64[(q * 3) % P];
                lossv[2 * q + 1] = pat64[(q * 3 + 1) % P];
                HIPCHK(hipSetDevice(devices[q]));
                HIPCHK(hipMemcpyAsync(g.numer[q], host[q].data(), (size_t)count * es, hipMemcpyHostToDevice, g.streams[q]));
                HIPCHK(hipMemcpyAsync(g.loss[q], &lossv[2 * q], 2 * sizeof(double), hipMemcpyHostToDevice, g.streams[q]));
                HIPCHK(hipEventRecord(g.ev_col[q], g.streams[q]));
            }
            const std::vector<const DevState *> st(n, nullptr);
            group_exchange(&g, count, st, [](int) {});
            for (int r = 0; r < n; ++r) {
                HIPCHK(hipSetDevice(devices[r]));
                HIPCHK(hipStreamSynchronize(g.streams[r]));
            }
            // expected: every element summed in rank order on the host, in the buffer's own type
            std::vector<unsigned char> want((size_t)count * es + 16), got((size_t)count * es + 16);
            for (int64_t i = 0; i < count; ++i) {
                if (g.f64) {
                    double a = val64(0, i);
                    for (int q = 1; q < n; ++q) a += val64(q, i);
                    ((double *)want.data())[i] = a;
                } else {
                    float a = val32(0, i);
                    for (int q = 1; q < n; ++q) a += val32(q, i);
                    ((float *)want.data())[i] = a;
                }
            }
            double lw[2] = {lossv[0], lossv[1]};
            for (int q = 1; q < n; ++q) { lw[0] += lossv[2 * q]; lw[1] += lossv[2 * q + 1]; }
            int bad = 0;
            for (int r = 0; r < n; ++r) {
                HIPCHK(hipSetDevice(devices[r]));
                HIPCHK(hipMemcpy(got.data(), g.numer[r], (size_t)count * es, hipMemcpyDeviceToHost));
                double lg[2];
                HIPCHK(hipMemcpy(lg, g.loss[r], sizeof(lg), hipMemcpyDeviceToHost));
                for (int64_t i = 0; i < count; ++i)
                    if (std::memcmp(got.data() + i * es, want.data() + i * es, es) != 0) ++bad;
                if (std::memcmp(lg, lw, sizeof(lw)) != 0) ++bad;
            }
            *failed = bad;
        } catch (...) {
            group_free(&g);
            throw;
        }
        group_free(&g);
    });
}

}  // extern "C"
