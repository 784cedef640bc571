// libklnmf.so, the codebook unit: the Lloyd iterations and the cluster Gram matrix of include/klnmf_kmeans.h -- argument checks,
// the workspace layout, the launches of kmeans.hip.h (included by this unit alone) and the host-array wrapper (ctx.hip.h lists
// the units).
#include "ctx.hip.h"
#include "../../include/klnmf_kmeans.h"
#include "kmeans.hip.h"

static_assert(kKmTile == KLNMF_KMEANS_TILE && kKmGroup == KLNMF_KMEANS_GROUP && kKmMaxKd == KLNMF_KMEANS_MAX_KD
              && kKmGramMaxD == KLNMF_KMEANS_GRAM_MAX_D, "the header's limits and order rule");
static_assert((size_t)kKmMaxKd * 8 + (size_t)kKmMaxKd * 4 + kKmTile * 4 <= (size_t)kKmLds, "the accumulators at the bound fit the LDS");

namespace klnmf_host {
namespace {

constexpr int64_t kKmMaxInt = 0x7fffffffLL;

inline size_t km_up16(size_t b) { return (b + 15) & ~(size_t)15; }

// The caller's workspace (byte offsets).  Lloyd: the partial sums at 0, the partial counts.  Gram: the partials at 0, the members
// per group, the count.  One buffer serves either call.
struct KmLayout {
    size_t groups, pcnt, lloyd, pn, count, gram, total;
    KmLayout(int64_t T, int64_t d, int64_t K) {
        groups = (size_t)km_groups(T);
        pcnt = km_up16(groups * (size_t)K * (size_t)d * sizeof(double));
        lloyd = pcnt + km_up16(groups * (size_t)K * sizeof(int32_t));
        gram = 0;
        pn = count = 0;
        if (d <= kKmGramMaxD) {
            pn = km_up16(groups * (size_t)(d * (d + 1) / 2 + d) * sizeof(double));
            count = pn + km_up16(groups * sizeof(int32_t));
            gram = count + 16;
        }
        total = std::max(lloyd, gram);
    }
};

void km_check_sizes(const char *who, int64_t T, int64_t d, int64_t K) {
    auto bad = [&](const char *what) { fail(KLNMF_ERR_ARG, std::string(who) + ": " + what); };
    if (T < 0 || T >= kKmMaxInt) bad("T negative or not below 2^31 - 1");
    if (d < 1) bad("d < 1");
    if (K < 1) bad("K < 1");
}

void km_check_bound(const char *who, int64_t d, int64_t K) {
    if (d > kKmMaxKd || K > kKmMaxKd || K * d > kKmMaxKd)
        fail(KLNMF_ERR_UNSUPP, std::string(who) + ": K * d = " + std::to_string(K) + " * " + std::to_string(d) + " is above "
             + std::to_string(kKmMaxKd) + " fp64 accumulators in LDS");
}

// What is staged in LDS beside the accumulators, and the bytes of the launch.
KmCall km_call(int dtype, const void *x, int64_t ld, int64_t T, int64_t d, void *cb, int64_t ldc, int64_t K, size_t *lds) {
    const size_t el = dtype == KLNMF_DT_F64 ? 8 : 4;
    size_t used = (size_t)K * d * sizeof(double) + (size_t)K * sizeof(int32_t) + kKmTile * sizeof(int32_t);
    const size_t cb_bytes = (size_t)K * d * el, x_bytes = (size_t)kKmFrameStride * d * el;
    int stage = 0;
    if (used + cb_bytes <= (size_t)kKmLds) { stage |= KM_STAGE_CODEBOOK; used += cb_bytes; }
    if (used + x_bytes <= (size_t)kKmLds) { stage |= KM_STAGE_FRAMES; used += x_bytes; }
    *lds = used;
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

void km_run(const char *who, int device, int dtype, const void *frames, int64_t ld, int64_t T, int64_t d, void *codebook, int64_t ldc,
            int64_t K, int n_iter, void *d_work, uint64_t work_bytes, int32_t *d_labels, int64_t *d_counts) {
    auto bad = [&](const char *what) { fail(KLNMF_ERR_ARG, std::string(who) + ": " + what); };
    if (dtype != KLNMF_DT_F32 && dtype != KLNMF_DT_F64) bad("dtype must be KLNMF_DT_F32 or KLNMF_DT_F64");
    km_check_sizes(who, T, d, K);
    if (n_iter < 0) bad("n_iter negative");
    if (ld < d || ldc < d) bad("a stride below d");
    if (!codebook || !d_work || !d_counts) bad("null codebook, workspace or counts");
    if (T > 0 && (!frames || !d_labels)) bad("null frames or labels");
    km_check_bound(who, d, K);
    const KmLayout at(T, d, K);
    if (work_bytes < (uint64_t)at.total) bad("workspace below klnmf_kmeans_work_bytes");
    HIPCHK(hipSetDevice(device));
    if (T == 0) {
        HIPCHK(hipMemsetAsync(d_counts, 0, sizeof(int64_t) * (size_t)K, 0));
        return;
    }
    size_t lds = 0;
    const KmCall call = km_call(dtype, frames, ld, T, d, codebook, ldc, K, &lds);
    if (dtype == KLNMF_DT_F64) km_launch<double>(call, lds, n_iter, (unsigned char *)d_work, at, d_labels, d_counts);
    else km_launch<float>(call, lds, n_iter, (unsigned char *)d_work, at, d_labels, d_counts);
    HIPCHK(hipGetLastError());
}

}  // namespace
}  // namespace klnmf_host

extern "C" {

int klnmf_kmeans_work_bytes(int64_t T, int64_t d, int64_t K, uint64_t *bytes) {
    return guarded([&] {
        if (!bytes) fail(KLNMF_ERR_ARG, "klnmf_kmeans_work_bytes: null bytes");
        km_check_sizes("klnmf_kmeans_work_bytes", T, d, K);
        km_check_bound("klnmf_kmeans_work_bytes", d, K);
        *bytes = (uint64_t)KmLayout(T, d, K).total;
    });
}

int klnmf_kmeans_device(int device, int dtype, const void *frames, int64_t ld, int64_t T, int64_t d, void *codebook, int64_t ldc,
                        int64_t K, int n_iter, void *d_work, uint64_t work_bytes, int32_t *d_labels, int64_t *d_counts) {
    return guarded([&] {
        km_run("klnmf_kmeans_device", device, dtype, frames, ld, T, d, codebook, ldc, K, n_iter, d_work, work_bytes, d_labels, d_counts);
    });
}

int klnmf_kmeans_gram_device(int device, int dtype, const void *frames, int64_t ld, int64_t T, int64_t d, const int32_t *d_labels,
                             int64_t cluster, void *d_work, uint64_t work_bytes, double *d_gram, double *d_colsum, int64_t *count) {
    return guarded([&] {
        const char *who = "klnmf_kmeans_gram_device";
        auto bad = [&](const char *what) { fail(KLNMF_ERR_ARG, std::string(who) + ": " + what); };
        if (dtype != KLNMF_DT_F32 && dtype != KLNMF_DT_F64) bad("dtype must be KLNMF_DT_F32 or KLNMF_DT_F64");
        km_check_sizes(who, T, d, 1);
        if (cluster < -1 || cluster >= kKmMaxInt) bad("cluster below -1 or not below 2^31 - 1");
        if (ld < d) bad("a stride below d");
        if (!d_gram || !d_colsum || !count || !d_work) bad("null gram, column sums, count or workspace");
        if (T > 0 && (!frames || (cluster >= 0 && !d_labels))) bad("null frames or labels");
        if (d > kKmGramMaxD)
            fail(KLNMF_ERR_UNSUPP, std::string(who) + ": d = " + std::to_string(d) + " is above " + std::to_string(kKmGramMaxD));
        const KmLayout at(T, d, 1);
        if (work_bytes < (uint64_t)at.gram) bad("workspace below klnmf_kmeans_work_bytes");
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
        if (dtype == KLNMF_DT_F64) hipLaunchKernelGGL((k_km_gram<double>), dim3(groups), dim3(kKmThreads), 0, 0, call, pg, pn);
        else hipLaunchKernelGGL((k_km_gram<float>), dim3(groups), dim3(kKmThreads), 0, 0, call, pg, pn);
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
        const char *who = "klnmf_kmeans";
        auto bad = [&](const char *what) { fail(KLNMF_ERR_ARG, std::string(who) + ": " + what); };
        if (dtype != KLNMF_DT_F32 && dtype != KLNMF_DT_F64) bad("dtype must be KLNMF_DT_F32 or KLNMF_DT_F64");
        km_check_sizes(who, T, d, K);
        if (n_iter < 0) bad("n_iter negative");
        if (ld < d || ldc < d) bad("a stride below d");
        if (!codebook || !counts) bad("null codebook or counts");
        if (T > 0 && (!frames || !labels)) bad("null frames or labels");
        km_check_bound(who, d, K);
        const size_t el = dtype == KLNMF_DT_F64 ? 8 : 4;
        const KmLayout at(T, d, K);
        HIPCHK(hipSetDevice(device));
        std::vector<void *> held;
        auto take = [&](size_t bytes) {
            void *p = nullptr;
            HIPCHK(hipMalloc(&p, std::max<size_t>(bytes, 16)));
            held.push_back(p);
            return p;
        };
        auto release = [&] { for (void *p : held) (void)hipFree(p); };
        try {
            void *dx = take(el * (size_t)T * d), *dc = take(el * (size_t)K * d), *work = take(at.total);
            int32_t *d_labels = (int32_t *)take(sizeof(int32_t) * (size_t)T);
            int64_t *d_counts = (int64_t *)take(sizeof(int64_t) * (size_t)K);
            if (T > 0) HIPCHK(hipMemcpy2D(dx, el * d, frames, el * ld, el * d, (size_t)T, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy2D(dc, el * d, codebook, el * ldc, el * d, (size_t)K, hipMemcpyHostToDevice));
            km_run(who, device, dtype, dx, d, T, d, dc, d, K, n_iter, work, at.total, d_labels, d_counts);
            HIPCHK(hipStreamSynchronize(0));
            if (T > 0) HIPCHK(hipMemcpy(labels, d_labels, sizeof(int32_t) * (size_t)T, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(counts, d_counts, sizeof(int64_t) * (size_t)K, hipMemcpyDeviceToHost));
            if (n_iter > 0 && T > 0)
                HIPCHK(hipMemcpy2D(codebook, el * ldc, dc, el * d, el * d, (size_t)K, hipMemcpyDeviceToHost));
        } catch (...) {
            release();
            throw;
        }
        release();
    });
}

}  // extern "C"
