// libklnmf.so, the analysis unit: the atom x label information matrix of include/klnmf_information.h -- argument checks, the
// workspace layout, the launches of information.hip.h (included by this unit alone) and the host-array wrapper (ctx.hip.h lists
// the units).
#include "ctx.hip.h"
#include "feature_host.hip.h"
#include "../../include/klnmf_information.h"
#include "information.hip.h"

static_assert(sizeof(klnmf_information_job) == 40, "klnmf_information_job: a pointer, a stride, a pointer, two sizes");
static_assert(kInfoLdsBytes == KLNMF_INFORMATION_LDS_BYTES && kInfoMaxBins == KLNMF_INFORMATION_MAX_BINS, "the header's route rule");

namespace klnmf_host {
namespace {

constexpr int64_t kInfoMaxRows = (int64_t)1 << 30, kInfoMaxAtoms = (int64_t)1 << 20;

// The caller's workspace: the job table and the flags (uploaded as one piece), the ranges, the slabs, the counts.
struct InfoLayout {
    size_t flags, ranges, slab_lo, slab_hi, counts, total;      // byte offsets; the job table lies at 0
    InfoLayout(int64_t count, int64_t atoms, int L, int B) {
        WorkLayout w;
        w.take((size_t)count * sizeof(InfoJob));
        flags = w.take((size_t)count * sizeof(int32_t));
        ranges = w.take((size_t)atoms * 2 * sizeof(double));
        slab_lo = w.take((size_t)atoms * kInfoSlabs * sizeof(double));
        slab_hi = w.take((size_t)atoms * kInfoSlabs * sizeof(double));
        counts = w.take((size_t)atoms * L * B * sizeof(int32_t));
        total = w.end;
    }
};

void info_check_sizes(const Who &w, int64_t count, int64_t atoms, int L, int B) {
    if (count < 0 || count > KLNMF_INFORMATION_MAX_JOBS) w.bad("job count negative or above KLNMF_INFORMATION_MAX_JOBS");
    if (L < 1 || L > KLNMF_INFORMATION_MAX_LABELS) w.bad("n_labels outside [1, 65536]");
    if (B < 1 || B > KLNMF_INFORMATION_MAX_BINS) w.bad("bins outside [1, 256]");
    if (atoms < 0 || atoms > KLNMF_INFORMATION_MAX_CELLS || atoms * L * B > KLNMF_INFORMATION_MAX_CELLS)
        w.bad("(sum of k) * n_labels * bins negative or above 2^28");
}

// Checks a call's arguments (fail() on the first bad one: nothing has been touched then) and returns the device job table.
std::vector<InfoJob> info_check(const Who &w, int dtype, int L, int B, const klnmf_information_job *jobs, int64_t count,
                                int64_t *atoms_out, int64_t *range_blocks, int64_t *hist_blocks) {
    w.dtype(dtype);
    info_check_sizes(w, count, 0, L, B);
    if (count > 0 && !jobs) w.bad("null job table");
    const int ta = info_atom_tile(L, B), hist_tile = ta > 0 ? ta : kInfoTile;
    std::vector<InfoJob> table((size_t)count);
    int64_t atoms = 0, rb = 0, hb = 0;
    for (int64_t q = 0; q < count; ++q) {
        const klnmf_information_job &j = jobs[q];
        if (j.n < 1 || j.k < 1) w.bad("n < 1 or k < 1");
        if (j.n > kInfoMaxRows || j.k > kInfoMaxAtoms) w.bad("n above 2^30 or k above 2^20");
        if (j.lda < j.k) w.bad("a stride below k");
        if (!j.A || !j.labels) w.bad("null matrix or labels");
        const int64_t chunk_rows = std::max<int64_t>(kInfoRows, (j.n + kInfoSlabs - 1) / kInfoSlabs);
        const int64_t chunks = (j.n + chunk_rows - 1) / chunk_rows;
        table[(size_t)q] = InfoJob{j.A, j.labels, j.lda, atoms, (int32_t)j.n, (int32_t)j.k, (int32_t)chunk_rows, (int32_t)chunks,
                                   (int32_t)rb, (int32_t)hb};
        atoms += j.k;
        rb += chunks * ((j.k + kInfoTile - 1) / kInfoTile);
        hb += chunks * ((j.k + hist_tile - 1) / hist_tile);
        info_check_sizes(w, count, atoms, L, B);
        if (rb > kMaxInt || hb > kMaxInt) w.bad("more workgroups than a launch holds");
    }
    *atoms_out = atoms;
    *range_blocks = rb;
    *hist_blocks = hb;
    return table;
}

void info_run(const Who &w, int dtype, int L, int B, const std::vector<InfoJob> &table, int64_t atoms, int64_t range_blocks,
              int64_t hist_blocks, double *d_info, int32_t *d_counts, void *d_work) {
    const int64_t count = (int64_t)table.size();
    const InfoLayout at(count, atoms, L, B);
    unsigned char *work = (unsigned char *)d_work;
    std::vector<unsigned char> head(at.ranges, 0);                 // the job table and the flags, cleared
    std::memcpy(head.data(), table.data(), table.size() * sizeof(InfoJob));
    HIPCHK(hipMemcpy(work, head.data(), head.size(), hipMemcpyHostToDevice));
    const InfoJob *jobs = (const InfoJob *)work;
    int32_t *flags = (int32_t *)(work + at.flags);
    double *ranges = (double *)(work + at.ranges), *slab_lo = (double *)(work + at.slab_lo), *slab_hi = (double *)(work + at.slab_hi);
    int32_t *counts = d_counts ? d_counts : (int32_t *)(work + at.counts);
    HIPCHK(hipMemsetAsync(counts, 0, (size_t)atoms * L * B * sizeof(int32_t), 0));
    const int ta = info_atom_tile(L, B);
    const size_t lds = (size_t)4 * L * B * ta;
    const dim3 threads(kInfoThreads);
    by_dtype(dtype, [&](auto tag) {
        using T = tag_t<decltype(tag)>;
        hipLaunchKernelGGL((k_info_range<T>), dim3((unsigned)range_blocks), threads, 0, 0, jobs, (int)count, atoms, slab_lo, slab_hi);
        hipLaunchKernelGGL(k_info_edges, dim3((unsigned)((atoms + kInfoThreads - 1) / kInfoThreads)), threads, 0, 0, jobs, (int)count,
                           atoms, slab_lo, slab_hi, ranges, flags);
        hipLaunchKernelGGL((k_info_hist<T>), dim3((unsigned)hist_blocks), threads, lds, 0, jobs, (int)count, L, B, ta, ranges, flags,
                           counts);
    });
    hipLaunchKernelGGL(k_info_mi, dim3((unsigned)atoms), threads, 0, 0, jobs, (int)count, L, B, counts, d_info);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(0));
    std::vector<int32_t> seen((size_t)count);
    HIPCHK(hipMemcpy(seen.data(), flags, seen.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int64_t q = 0; q < count; ++q)
        if (seen[(size_t)q])
            w.bad("job " + std::to_string(q) + ": "
                  + (seen[(size_t)q] & kInfoNotFinite ? "a coefficient that is not finite (the range of an atom is not finite)"
                                                      : "a label outside [0, n_labels)"));
}

}  // namespace
}  // namespace klnmf_host

extern "C" {

int klnmf_information_work_bytes(int64_t count, int64_t total_atoms, int n_labels, int bins, uint64_t *bytes) {
    return guarded([&] {
        const Who w{"klnmf_information_work_bytes"};
        if (!bytes) w.bad("null bytes");
        info_check_sizes(w, count, total_atoms, n_labels, bins);
        *bytes = (uint64_t)InfoLayout(count, total_atoms, n_labels, bins).total;
    });
}

int klnmf_information_many_device(int device, int dtype, int n_labels, int bins, const klnmf_information_job *jobs, int64_t count,
                                  double *d_info, int32_t *d_counts, void *d_work, uint64_t work_bytes) {
    return guarded([&] {
        const Who w{"klnmf_information_many_device"};
        int64_t atoms = 0, rb = 0, hb = 0;
        const std::vector<InfoJob> table = info_check(w, dtype, n_labels, bins, jobs, count, &atoms, &rb, &hb);
        if (count == 0) return;
        if (!d_info || !d_work) w.bad("null output or workspace");
        w.workspace(work_bytes, InfoLayout(count, atoms, n_labels, bins).total, "klnmf_information_work_bytes");
        HIPCHK(hipSetDevice(device));
        info_run(w, dtype, n_labels, bins, table, atoms, rb, hb, d_info, d_counts, d_work);
    });
}

int klnmf_information(int device, int dtype, int n_labels, int bins, int64_t n, int64_t k, const void *A, const int32_t *labels,
                      double *info, int32_t *counts) {
    return guarded([&] {
        const Who w{"klnmf_information"};
        klnmf_information_job job{A, k, labels, n, k};
        int64_t atoms = 0, rb = 0, hb = 0;
        std::vector<InfoJob> table = info_check(w, dtype, n_labels, bins, &job, 1, &atoms, &rb, &hb);
        if (!info) w.bad("null info");
        HIPCHK(hipSetDevice(device));
        const size_t el = dtype_bytes(dtype), cells = (size_t)k * n_labels;
        DeviceScratch mem;
        void *dA = mem.take(el * (size_t)(n * k));
        int32_t *dL = (int32_t *)mem.take(sizeof(int32_t) * (size_t)n);
        double *dI = (double *)mem.take(sizeof(double) * cells);
        int32_t *dC = counts ? (int32_t *)mem.take(sizeof(int32_t) * cells * bins) : nullptr;
        void *dW = mem.take(InfoLayout(1, atoms, n_labels, bins).total);
        HIPCHK(hipMemcpy(dA, A, el * (size_t)(n * k), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dL, labels, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
        table[0].A = dA;
        table[0].labels = dL;
        info_run(w, dtype, n_labels, bins, table, atoms, rb, hb, dI, dC, dW);
        HIPCHK(hipMemcpy(info, dI, sizeof(double) * cells, hipMemcpyDeviceToHost));
        if (counts) HIPCHK(hipMemcpy(counts, dC, sizeof(int32_t) * cells * bins, hipMemcpyDeviceToHost));
    });
}

}  // extern "C"
