// libklnmf.so, the feature unit: the windowed co-occurrence histograms of include/klnmf_hac.h -- argument checks, the workspace
// layout, the launches of hac.hip.h (included by this unit alone, behind the quantiser of vq.hip.h) and the host-array wrapper
// (ctx.hip.h lists the units).
#include "ctx.hip.h"
#include "feature_host.hip.h"
#include "../../include/klnmf_hac.h"
#include "vq.hip.h"
#include "hac.hip.h"

static_assert(sizeof(klnmf_hac_stream) == 48, "klnmf_hac_stream: two pointers, two strides, two sizes");
static_assert(kHacMaxStreams == KLNMF_HAC_MAX_STREAMS && kHacMaxLags == KLNMF_HAC_MAX_LAGS && kHacSortMax == KLNMF_HAC_SORT_MAX
              && kHacDenseBins == KLNMF_HAC_DENSE_MAX_K * KLNMF_HAC_DENSE_MAX_K, "the header's route rule");

namespace klnmf_host {
namespace {

// The caller's workspace: the codes, the windows, the segment counts, the segment offsets (byte offsets; the codes lie at 0).
struct HacLayout {
    size_t windows, counts, offsets, total;
    HacLayout(int S, int64_t T, int L, int64_t N) {
        const size_t segs = (size_t)N * S * L;
        WorkLayout w;
        w.take((size_t)S * (size_t)T * sizeof(int32_t));
        windows = w.take((size_t)N * 2 * sizeof(int32_t));
        counts = w.take(segs * sizeof(int32_t));
        offsets = w.take((segs + 1) * sizeof(int64_t));
        total = w.end;
    }
};

void hac_check_sizes(const Who &w, int S, int64_t T, int L, int64_t N) {
    if (S < 1 || S > KLNMF_HAC_MAX_STREAMS) w.bad("n_streams outside [1, 8]");
    if (L < 1 || L > KLNMF_HAC_MAX_LAGS) w.bad("n_lags outside [1, 8]");
    if (T < 0 || T >= kMaxInt) w.bad("T negative or not below 2^31 - 1");
    if (N < 0 || N * S * L >= kMaxInt) w.bad("n_windows negative, or n_windows * n_streams * n_lags not below 2^31 - 1");
}

// What the passes need of a call, from host arithmetic alone: the table, the LDS of the launch.  fail() on the first bad
// argument: nothing has been touched then.
struct HacCall {
    HacPlan plan;
    int64_t segs;
    size_t lds;
};

HacCall hac_check(const Who &w, const int64_t *K, int S, int64_t T, const int32_t *lags, int L, const int64_t *windows, int64_t N) {
    hac_check_sizes(w, S, T, L, N);
    if (!K || !lags) w.bad("null stream sizes or lags");
    if (N > 0 && !windows) w.bad("null windows");
    HacCall call{};
    call.plan.S = S;
    call.plan.L = L;
    call.plan.T = (int32_t)T;
    int64_t F = 0;
    for (int l = 0; l < L; ++l) {
        if (lags[l] < 1) w.bad("a lag below 1");
        call.plan.lag[l] = lags[l];
    }
    for (int s = 0; s < S; ++s) {
        if (K[s] < 1 || K[s] > 46340) w.bad("a codebook of no unit, or of K with K^2 not below 2^31");
        call.plan.K[s] = (int32_t)K[s];
        for (int l = 0; l < L; ++l) {
            if (F >= kMaxInt) w.bad("the number of columns F = sum n_lags * K^2 is not below 2^31");
            call.plan.colbase[s * L + l] = (int32_t)F;
            F += K[s] * K[s];
        }
    }
    if (F >= kMaxInt) w.bad("the number of columns F = sum n_lags * K^2 is not below 2^31");
    int64_t sort_p = 0, dense_bins = 0;
    for (int64_t i = 0; i < N; ++i) {
        const int64_t t0 = windows[2 * i], t1 = windows[2 * i + 1];
        if (t0 < 0 || t1 < t0 || t1 > T) w.bad("window " + std::to_string(i) + " outside [0, T] or with t1 < t0");
        for (int l = 0; l < L; ++l) {
            const int64_t n = t1 - t0 - lags[l];
            for (int s = 0; s < S; ++s) {
                const int route = hac_route(n, K[s]);
                if (route == HAC_ROUTE_UNFIT)
                    w.unsupp("window " + std::to_string(i) + ", stream " + std::to_string(s) + ": " + std::to_string(n)
                             + " pair codes (above " + std::to_string(kHacSortMax) + ") over a codebook of " + std::to_string(K[s])
                             + " units (above " + std::to_string(KLNMF_HAC_DENSE_MAX_K) + ") fit neither route");
                if (route == HAC_ROUTE_SORT) {
                    int64_t P = 64;
                    while (P < n) P <<= 1;
                    sort_p = std::max(sort_p, P);
                } else if (route == HAC_ROUTE_DENSE) {
                    dense_bins = std::max(dense_bins, K[s] * K[s]);
                }
            }
        }
    }
    call.segs = N * S * L;
    call.lds = sizeof(int32_t) * (size_t)std::max(sort_p > 0 ? 2 * sort_p + 1 : 0, dense_bins);
    return call;
}

template <typename T, bool kFill>
void hac_launch_pass(const HacCall &call, const int32_t *codes, const int32_t *windows, int32_t *counts, const int64_t *offsets,
                     int64_t nnz, int32_t *indices, T *values) {
    if (call.lds > 64 * 1024)       // (the dense route's counters: beyond the default dynamic LDS of a launch)
        (void)hipFuncSetAttribute((const void *)k_hac_pass<T, kFill>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)call.lds);
    hipLaunchKernelGGL((k_hac_pass<T, kFill>), dim3((unsigned)call.segs), dim3(kHacThreads), call.lds, 0, call.plan, codes, windows,
                       counts, offsets, nnz, indices, values);
}

// The quantisation table of a call: staging decided per stream, the grid.
HacStreams hac_streams(const Who &w, int dtype, const klnmf_hac_stream *streams, int S, int64_t T, size_t *lds, int64_t *blocks) {
    const size_t el = dtype_bytes(dtype);
    HacStreams tab{};
    tab.count = S;
    tab.T = (int32_t)T;
    const int64_t tiles = (T + kHacThreads - 1) / kHacThreads;
    size_t need = 0;
    int64_t block0 = 0;
    for (int s = 0; s < S; ++s) {
        const klnmf_hac_stream &in = streams[s];
        if (in.d < 1 || in.d > (1 << 20) || in.K < 1) w.bad("d outside [1, 2^20] or K < 1");
        if (in.ld < in.d || in.ldc < in.d) w.bad("a stride below d");
        if (!in.codebook || (T > 0 && !in.frames)) w.bad("null frames or codebook");
        size_t used = 0;
        const int stage = vq_staging(el, in.K, in.d, kHacVqLds, &used);
        need = std::max(need, used);
        tab.s[s] = HacStream{in.frames, in.codebook, in.ld, in.ldc, (int32_t)in.d, (int32_t)in.K, (int32_t)block0, stage};
        block0 += tiles;
    }
    if (block0 >= kMaxInt) w.bad("more workgroups than a launch holds");
    *lds = need;
    *blocks = block0;
    return tab;
}

void hac_upload_windows(const int64_t *windows, int64_t N, int32_t *d_windows) {
    std::vector<int32_t> w32((size_t)N * 2);
    for (size_t i = 0; i < w32.size(); ++i) w32[i] = (int32_t)windows[i];
    HIPCHK(hipMemcpy(d_windows, w32.data(), w32.size() * sizeof(int32_t), hipMemcpyHostToDevice));
}

void hac_count(const Who &w, int device, int dtype, const klnmf_hac_stream *streams, int S, int64_t T, const int32_t *lags, int L,
               const int64_t *windows, int64_t N, void *d_work, uint64_t work_bytes, int64_t *d_indptr, int64_t *nnz) {
    w.dtype(dtype);
    hac_check_sizes(w, S, T, L, N);
    if (!streams || !nnz || !d_indptr || !d_work) w.bad("null streams, nnz, row pointers or workspace");
    int64_t K[KLNMF_HAC_MAX_STREAMS];
    for (int s = 0; s < S; ++s) K[s] = streams[s].K;
    size_t vq_lds = 0;
    int64_t vq_blocks = 0;
    const HacStreams tab = hac_streams(w, dtype, streams, S, T, &vq_lds, &vq_blocks);
    const HacCall call = hac_check(w, K, S, T, lags, L, windows, N);
    const HacLayout at(S, T, L, N);
    w.workspace(work_bytes, at.total, "klnmf_hac_work_bytes");
    HIPCHK(hipSetDevice(device));
    if (N == 0) {
        HIPCHK(hipMemset(d_indptr, 0, sizeof(int64_t)));
        *nnz = 0;
        return;
    }
    unsigned char *work = (unsigned char *)d_work;
    int32_t *codes = (int32_t *)work, *d_windows = (int32_t *)(work + at.windows), *counts = (int32_t *)(work + at.counts);
    int64_t *offsets = (int64_t *)(work + at.offsets);
    hac_upload_windows(windows, N, d_windows);
    if (vq_blocks > 0)
        by_dtype(dtype, [&](auto tag) {
            hipLaunchKernelGGL((k_hac_vq<tag_t<decltype(tag)>>), dim3((unsigned)vq_blocks), dim3(kHacThreads), vq_lds, 0, tab, codes);
        });
    hac_launch_pass<float, false>(call, codes, d_windows, counts, nullptr, 0, nullptr, nullptr);
    hipLaunchKernelGGL(k_hac_scan, dim3(1), dim3(kHacThreads), 0, 0, counts, call.segs, S * L, offsets, d_indptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(nnz, offsets + call.segs, sizeof(int64_t), hipMemcpyDeviceToHost));
}

void hac_fill(const Who &w, int device, int value_dtype, const int64_t *K, int S, int64_t T, const int32_t *lags, int L,
              const int64_t *windows, int64_t N, const void *d_work, uint64_t work_bytes, int64_t nnz, int32_t *d_indices,
              void *d_values) {
    w.dtype(value_dtype, "value_");
    const HacCall call = hac_check(w, K, S, T, lags, L, windows, N);
    if (nnz < 0) w.bad("nnz negative");
    if (!d_work) w.bad("null workspace");
    const HacLayout at(S, T, L, N);
    w.workspace(work_bytes, at.total, "klnmf_hac_work_bytes");
    if (nnz == 0 || N == 0) return;
    if (!d_indices || !d_values) w.bad("null indices or values");
    HIPCHK(hipSetDevice(device));
    const unsigned char *work = (const unsigned char *)d_work;
    const int32_t *codes = (const int32_t *)work, *d_windows = (const int32_t *)(work + at.windows);
    const int64_t *offsets = (const int64_t *)(work + at.offsets);
    by_dtype(value_dtype, [&](auto tag) {
        using V = tag_t<decltype(tag)>;
        hac_launch_pass<V, true>(call, codes, d_windows, nullptr, offsets, nnz, d_indices, (V *)d_values);
    });
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(0));
}

}  // namespace
}  // namespace klnmf_host

extern "C" {

int klnmf_hac_work_bytes(int n_streams, int64_t T, int n_lags, int64_t n_windows, uint64_t *bytes) {
    return guarded([&] {
        const Who w{"klnmf_hac_work_bytes"};
        if (!bytes) w.bad("null bytes");
        hac_check_sizes(w, n_streams, T, n_lags, n_windows);
        *bytes = (uint64_t)HacLayout(n_streams, T, n_lags, n_windows).total;
    });
}

int klnmf_hac_count_device(int device, int dtype, const klnmf_hac_stream *streams, int n_streams, int64_t T, const int32_t *lags,
                           int n_lags, const int64_t *windows, int64_t n_windows, void *d_work, uint64_t work_bytes,
                           int64_t *d_indptr, int64_t *nnz) {
    return guarded([&] {
        hac_count(Who{"klnmf_hac_count_device"}, device, dtype, streams, n_streams, T, lags, n_lags, windows, n_windows, d_work, work_bytes,
                  d_indptr, nnz);
    });
}

int klnmf_hac_fill_device(int device, int value_dtype, const int64_t *K, int n_streams, int64_t T, const int32_t *lags, int n_lags,
                          const int64_t *windows, int64_t n_windows, const void *d_work, uint64_t work_bytes, int64_t nnz,
                          int32_t *d_indices, void *d_values) {
    return guarded([&] {
        const Who w{"klnmf_hac_fill_device"};
        hac_check_sizes(w, n_streams, T, n_lags, n_windows);
        hac_fill(w, device, value_dtype, K, n_streams, T, lags, n_lags, windows, n_windows, d_work, work_bytes,
                 nnz, d_indices, d_values);
    });
}

int klnmf_hac(int device, int dtype, int value_dtype, const klnmf_hac_stream *streams, int n_streams, int64_t T,
              const int32_t *lags, int n_lags, const int64_t *windows, int64_t n_windows, int64_t *indptr, int64_t capacity,
              int32_t *indices, void *values, int64_t *nnz) {
    return guarded([&] {
        const Who w{"klnmf_hac"};
        w.dtype(dtype);
        w.dtype(value_dtype, "value_");
        hac_check_sizes(w, n_streams, T, n_lags, n_windows);
        if (!streams || !indptr || !nnz || capacity < 0) w.bad("null streams, row pointers or nnz, or a negative capacity");
        const int S = n_streams;
        const size_t el = dtype_bytes(dtype), vel = dtype_bytes(value_dtype);
        int64_t K[KLNMF_HAC_MAX_STREAMS];
        size_t lds = 0;
        int64_t blocks = 0;
        (void)hac_streams(w, dtype, streams, S, T, &lds, &blocks);           // (the streams' own refusals, on the host pointers)
        for (int s = 0; s < S; ++s) K[s] = streams[s].K;
        (void)hac_check(w, K, S, T, lags, n_lags, windows, n_windows);
        HIPCHK(hipSetDevice(device));
        const HacLayout at(S, T, n_lags, n_windows);
        DeviceScratch mem;
        klnmf_hac_stream dev[KLNMF_HAC_MAX_STREAMS];
        for (int s = 0; s < S; ++s) {
            const klnmf_hac_stream &in = streams[s];
            unsigned char *dx = (unsigned char *)mem.take(el * (size_t)T * in.d), *dc = (unsigned char *)mem.take(el * (size_t)in.K * in.d);
            if (T > 0) HIPCHK(hipMemcpy2D(dx, el * in.d, in.frames, el * in.ld, el * in.d, (size_t)T, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy2D(dc, el * in.d, in.codebook, el * in.ldc, el * in.d, (size_t)in.K, hipMemcpyHostToDevice));
            dev[s] = klnmf_hac_stream{dx, in.d, dc, in.d, in.d, in.K};
        }
        void *work = mem.take(at.total);
        int64_t *d_indptr = (int64_t *)mem.take(sizeof(int64_t) * (size_t)(n_windows + 1));
        int64_t found = 0;
        hac_count(w, device, dtype, dev, S, T, lags, n_lags, windows, n_windows, work, at.total, d_indptr, &found);
        HIPCHK(hipMemcpy(indptr, d_indptr, sizeof(int64_t) * (size_t)(n_windows + 1), hipMemcpyDeviceToHost));
        *nnz = found;
        if (found > capacity) w.bad("capacity " + std::to_string(capacity) + " below the " + std::to_string(found) + " stored entries");
        if (found == 0) return;
        if (!indices || !values) w.bad("null indices or values");
        int32_t *d_indices = (int32_t *)mem.take(sizeof(int32_t) * (size_t)found);
        void *d_values = mem.take(vel * (size_t)found);
        hac_fill(w, device, value_dtype, K, S, T, lags, n_lags, windows, n_windows, work, at.total, found, d_indices, d_values);
        HIPCHK(hipMemcpy(indices, d_indices, sizeof(int32_t) * (size_t)found, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(values, d_values, vel * (size_t)found, hipMemcpyDeviceToHost));
    });
}

}  // extern "C"
