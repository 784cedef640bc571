// libklnmf.so, the codebook unit: the Lloyd iterations and the cluster Gram matrix of include/klnmf_kmeans.h -- argument checks,
// the workspace layout, the launches of kmeans.hip.h (included by this unit alone, behind the quantiser of vq.hip.h) and the
// host-array wrapper (ctx.hip.h lists the units).
#include "ctx.hip.h"
#include "feature_host.hip.h"
#include "../../include/klnmf_kmeans.h"
#include "vq.hip.h"
#include "kmeans.hip.h"

static_assert(kKmTile == KLNMF_KMEANS_TILE && kKmGroup == KLNMF_KMEANS_GROUP && kKmMaxKd == KLNMF_KMEANS_MAX_KD
              && kKmGramMaxD == KLNMF_KMEANS_GRAM_MAX_D, "the header's limits and order rule");
static_assert((size_t)kKmMaxKd * 8 + (size_t)kKmMaxKd * 4 + kKmTile * 4 <= (size_t)kKmLds, "the accumulators at the bound fit the LDS");

namespace klnmf_host {
namespace {

// The caller's workspace (byte offsets).  Lloyd: the partial sums at 0, the partial counts.  Gram: the partials at 0, the members
// per group, the count.  One buffer serves either call.
struct KmLayout {
    size_t groups, pcnt, lloyd, pn = 0, count = 0, gram, total;
    KmLayout(int64_t T, int64_t d, int64_t K) {
        groups = (size_t)km_groups(T);
        WorkLayout l, g;
        l.take(groups * (size_t)K * (size_t)d * sizeof(double));
        pcnt = l.take(groups * (size_t)K * sizeof(int32_t));
        lloyd = l.end;
        if (d <= kKmGramMaxD) {
            g.take(groups * (size_t)(d * (d + 1) / 2 + d) * sizeof(double));
            pn = g.take(groups * sizeof(int32_t));
            count = g.take(sizeof(int64_t));
        }
        gram = g.end;
        l.overlay({g});
        total = l.end;
    }
};

void km_check_sizes(const Who &w, int64_t T, int64_t d, int64_t K) {
    if (T < 0 || T >= kMaxInt) w.bad("T negative or not below 2^31 - 1");
    if (d < 1) w.bad("d < 1");
    if (K < 1) w.bad("K < 1");
}

void km_check_bound(const Who &w, int64_t d, int64_t K) {
    if (d > kKmMaxKd || K > kKmMaxKd || K * d > kKmMaxKd)
        w.unsupp("K * d = " + std::to_string(K) + " * " + std::to_string(d) + " is above " + std::to_string(kKmMaxKd)
                 + " fp64 accumulators in LDS");
}

// What is staged in LDS beside the accumulators, and the bytes of the launch.
KmCall km_call(int dtype, const void *x, int64_t ld, int64_t T, int64_t d, void *cb, int64_t ldc, int64_t K, size_t *lds) {
    *lds = (size_t)K * d * sizeof(double) + (size_t)K * sizeof(int32_t) + kKmTile * sizeof(int32_t);
    const int stage = vq_staging(dtype_bytes(dtype), K, d, kKmLds, lds);
    return KmCall{x, cb, ld, ldc, (int32_t)T, (int32_t)d, (int32_t)K, stage, 1};
}

template <typename T>
void km_launch(KmCall call, size_t lds, int n_iter, unsigned char *work, const KmLayout &at, int32_t *labels, int64_t *counts) {
    if (lds > 64 * 1024)        // (beyond the default dynamic LDS of a launch)
        (void)hipFuncSetAttribute((const void *)k_km_assign<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    double *psum = (double *)work;
    int32_t *pcnt = (int32_t *)(work + at.pcnt);
    const unsigned groups = (unsigned)at.groups, cells = (unsigned)((call.K * call.d + kKmThreads - 1) / kKmThreads);
    call.sums = n_iter > 0;
    for (int it = 0; it < std::max(1, n_iter); ++it) {
        hipLaunchKernelGGL((k_km_assign<T>), dim3(groups), dim3(kKmThreads), lds, 0, call, labels, psum, pcnt);
        hipLaunchKernelGGL((k_km_update<T>), dim3(cells), dim3(kKmThreads), 0, 0, call, (int)groups, psum, pcnt, counts);
    }
}

void km_run(const Who &w, int device, int dtype, const void *frames, int64_t ld, int64_t T, int64_t d, void *codebook, int64_t ldc,
            int64_t K, int n_iter, void *d_work, uint64_t work_bytes, int32_t *d_labels, int64_t *d_counts) {
    w.dtype(dtype);
    km_check_sizes(w, T, d, K);
    if (n_iter < 0) w.bad("n_iter negative");
    if (ld < d || ldc < d) w.bad("a stride below d");
    if (!codebook || !d_work || !d_counts) w.bad("null codebook, workspace or counts");
    if (T > 0 && (!frames || !d_labels)) w.bad("null frames or labels");
    km_check_bound(w, d, K);
    const KmLayout at(T, d, K);
    w.workspace(work_bytes, at.total, "klnmf_kmeans_work_bytes");
    HIPCHK(hipSetDevice(device));
    if (T == 0) {
        HIPCHK(hipMemsetAsync(d_counts, 0, sizeof(int64_t) * (size_t)K, 0));
        return;
    }
    size_t lds = 0;
    const KmCall call = km_call(dtype, frames, ld, T, d, codebook, ldc, K, &lds);
    by_dtype(dtype, [&](auto tag) {
        km_launch<tag_t<decltype(tag)>>(call, lds, n_iter, (unsigned char *)d_work, at, d_labels, d_counts);
    });
    HIPCHK(hipGetLastError());
}

}  // namespace
}  // namespace klnmf_host

extern "C" {

int klnmf_kmeans_work_bytes(int64_t T, int64_t d, int64_t K, uint64_t *bytes) {
    return guarded([&] {
        const Who w{"klnmf_kmeans_work_bytes"};
        if (!bytes) w.bad("null bytes");
        km_check_sizes(w, T, d, K);
        km_check_bound(w, d, K);
        *bytes = (uint64_t)KmLayout(T, d, K).total;
    });
}

int klnmf_kmeans_device(int device, int dtype, const void *frames, int64_t ld, int64_t T, int64_t d, void *codebook, int64_t ldc,
                        int64_t K, int n_iter, void *d_work, uint64_t work_bytes, int32_t *d_labels, int64_t *d_counts) {
    return guarded([&] {
        km_run(Who{"klnmf_kmeans_device"}, device, dtype, frames, ld, T, d, codebook, ldc, K, n_iter, d_work, work_bytes, d_labels,
               d_counts);
    });
}

int klnmf_kmeans_gram_device(int device, int dtype, const void *frames, int64_t ld, int64_t T, int64_t d, const int32_t *d_labels,
                             int64_t cluster, void *d_work, uint64_t work_bytes, double *d_gram, double *d_colsum, int64_t *count) {
    return guarded([&] {
        const Who w{"klnmf_kmeans_gram_device"};
        w.dtype(dtype);
        km_check_sizes(w, T, d, 1);
        if (cluster < -1 || cluster >= kMaxInt) w.bad("cluster below -1 or not below 2^31 - 1");
        if (ld < d) w.bad("a stride below d");
        if (!d_gram || !d_colsum || !count || !d_work) w.bad("null gram, column sums, count or workspace");
        if (T > 0 && (!frames || (cluster >= 0 && !d_labels))) w.bad("null frames or labels");
        if (d > kKmGramMaxD) w.unsupp("d = " + std::to_string(d) + " is above " + std::to_string(kKmGramMaxD));
        const KmLayout at(T, d, 1);
        w.workspace(work_bytes, at.gram, "klnmf_kmeans_work_bytes");
        HIPCHK(hipSetDevice(device));
        if (T == 0) {
            HIPCHK(hipMemsetAsync(d_gram, 0, sizeof(double) * (size_t)(d * d), 0));
            HIPCHK(hipMemsetAsync(d_colsum, 0, sizeof(double) * (size_t)d, 0));
            HIPCHK(hipStreamSynchronize(0));
            *count = 0;
            return;
        }
        unsigned char *work = (unsigned char *)d_work;
        double *pg = (double *)work;
        int32_t *pn = (int32_t *)(work + at.pn);
        int64_t *d_count = (int64_t *)(work + at.count);
        const KmGramCall call{frames, d_labels, ld, (int32_t)T, (int32_t)d, (int32_t)cluster};
        const unsigned groups = (unsigned)at.groups;
        const unsigned cells = (unsigned)((d * (d + 1) / 2 + d + 1 + kKmThreads - 1) / kKmThreads);
        by_dtype(dtype, [&](auto tag) {
            hipLaunchKernelGGL((k_km_gram<tag_t<decltype(tag)>>), dim3(groups), dim3(kKmThreads), 0, 0, call, pg, pn);
        });
        hipLaunchKernelGGL(k_km_gram_reduce, dim3(cells), dim3(kKmThreads), 0, 0, (int)d, (int)groups, pg, pn, d_gram, d_colsum, d_count);
        HIPCHK(hipGetLastError());
        int64_t found = 0;
        HIPCHK(hipMemcpy(&found, d_count, sizeof(int64_t), hipMemcpyDeviceToHost));
        *count = found;
    });
}

int klnmf_kmeans(int device, int dtype, const void *frames, int64_t ld, int64_t T, int64_t d, void *codebook, int64_t ldc, int64_t K,
                 int n_iter, int32_t *labels, int64_t *counts) {
    return guarded([&] {
        const Who w{"klnmf_kmeans"};
        w.dtype(dtype);
        km_check_sizes(w, T, d, K);
        if (n_iter < 0) w.bad("n_iter negative");
        if (ld < d || ldc < d) w.bad("a stride below d");
        if (!codebook || !counts) w.bad("null codebook or counts");
        if (T > 0 && (!frames || !labels)) w.bad("null frames or labels");
        km_check_bound(w, d, K);
        const size_t el = dtype_bytes(dtype);
        const KmLayout at(T, d, K);
        HIPCHK(hipSetDevice(device));
        DeviceScratch mem;
        void *dx = mem.take(el * (size_t)T * d), *dc = mem.take(el * (size_t)K * d), *work = mem.take(at.total);
        int32_t *d_labels = (int32_t *)mem.take(sizeof(int32_t) * (size_t)T);
        int64_t *d_counts = (int64_t *)mem.take(sizeof(int64_t) * (size_t)K);
        if (T > 0) HIPCHK(hipMemcpy2D(dx, el * d, frames, el * ld, el * d, (size_t)T, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy2D(dc, el * d, codebook, el * ldc, el * d, (size_t)K, hipMemcpyHostToDevice));
        km_run(w, device, dtype, dx, d, T, d, dc, d, K, n_iter, work, at.total, d_labels, d_counts);
        HIPCHK(hipStreamSynchronize(0));
        if (T > 0) HIPCHK(hipMemcpy(labels, d_labels, sizeof(int32_t) * (size_t)T, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(counts, d_counts, sizeof(int64_t) * (size_t)K, hipMemcpyDeviceToHost));
        if (n_iter > 0 && T > 0) HIPCHK(hipMemcpy2D(codebook, el * ldc, dc, el * d, el * d, (size_t)K, hipMemcpyDeviceToHost));
    });
}

}  // extern "C"
