// libklnmf.so, the motion unit: the angle, whitening, batched k-means and histogram calls of include/klnmf_motion.h -- argument
// checks, the workspace layout, the launches of motion.hip.h (included by this unit alone) and the stop-flag polls of the
// k-means loop.
#include "ctx.hip.h"
#include "feature_host.hip.h"
#include "../../include/klnmf_motion.h"
#include "motion.hip.h"

#include <cmath>

static_assert(kMoTile == KLNMF_MOTION_TILE && kMoGroup == KLNMF_MOTION_GROUP && kMoMaxK == KLNMF_MOTION_MAX_K
              && kMoMaxD == KLNMF_MOTION_MAX_D && kMoMaxKd == KLNMF_MOTION_MAX_KD && kMoMaxPairs == KLNMF_MOTION_MAX_PAIRS
              && kMoMaxGridY == KLNMF_MOTION_MAX_P, "the header's limits and order rule");
static_assert(kMoMaxK <= kMoThreads, "k_mo_hist gives a thread to every bin");
static_assert((size_t)kMoMaxKd * 16 + (size_t)kMoMaxD * kMoXStride * 8 + kMoTile * 12 + kMoMaxK * 8 <= 64 * 1024,
              "the static and, at d = 16, the dynamic LDS of k_mo_assign");

namespace klnmf_host {
namespace {

constexpr size_t kMoPairBytes = 256;                // kMoMaxPairs * 2 int32

// The caller's workspace (byte offsets).  The main part serves one call at a time: whitening (the partials at 0), k-means (the
// partial sums at 0, then distances, counts, and the problems' previous distortion, stop flag and set), histograms (the raw
// sums at 0).  Behind it the offsets and the pairs of the call.
struct MoLayout {
    size_t groups, pdist, pcnt, prev, done, set_of, km, main, offsets, pairs, total;
    MoLayout(int64_t T, int64_t C, int64_t d, int64_t K, int64_t P, int64_t D, int64_t E) {
        groups = (size_t)mo_groups(T);
        WorkLayout w, whiten, kmeans, hist;
        whiten.take(groups * (size_t)C * sizeof(double));
        kmeans.take(groups * (size_t)P * (size_t)K * (size_t)d * sizeof(double));
        pdist = kmeans.take(groups * (size_t)P * sizeof(double));
        pcnt = kmeans.take(groups * (size_t)P * (size_t)K * sizeof(int32_t));
        prev = kmeans.take((size_t)P * sizeof(double));
        done = kmeans.take((size_t)P * sizeof(int32_t));
        set_of = kmeans.take((size_t)P * sizeof(int32_t));
        km = kmeans.end;
        hist.take((size_t)E * (size_t)D * (size_t)K * sizeof(double));
        w.overlay({whiten, kmeans, hist});
        main = w.end;
        offsets = w.take((size_t)(E + 1) * sizeof(int64_t));
        pairs = w.take(kMoPairBytes);
        total = w.end;
    }
};

struct MoWho : Who {                                // the refusals several of this unit's entry points share
    void frames(int64_t T, int64_t least) const {
        if (T < least || T >= kMaxInt) bad("T below " + std::to_string(least) + " or not below 2^31 - 1");
    }
    void limits(int64_t d, int64_t K, int64_t P, int64_t D) const {
        if (K > kMoMaxK || d > kMoMaxD || K * d > kMoMaxKd)
            unsupp("K = " + std::to_string(K) + ", d = " + std::to_string(d) + " beyond K <= " + std::to_string(kMoMaxK) + ", d <= "
                   + std::to_string(kMoMaxD) + ", K * d <= " + std::to_string(kMoMaxKd));
        if (P > kMoMaxGridY || D > kMoMaxGridY) unsupp("more than " + std::to_string(kMoMaxGridY) + " problems or point sets");
    }
    void offsets(const int64_t *off, int64_t E, int64_t T) const {
        if (!off) bad("null offsets");
        if (E < 1 || E >= kMaxInt) bad("E < 1");
        if (off[0] != 0 || off[E] != T) bad("offsets that do not start at 0 or do not end at T");
        for (int64_t e = 0; e < E; ++e)
            if (off[e + 1] < off[e]) bad("offsets that decrease at example " + std::to_string(e));
    }
};

inline size_t mo_tile_bytes(int d) { return (size_t)d * kMoXStride * sizeof(double); }   // the dynamic LDS of k_mo_assign / k_mo_hist

inline unsigned mo_cells(int64_t n) { return (unsigned)((n + kMoThreads - 1) / kMoThreads); }

void mo_upload_offsets(unsigned char *work, const MoLayout &at, const int64_t *offsets, int64_t E) {
    HIPCHK(hipMemcpy(work + at.offsets, offsets, sizeof(int64_t) * (size_t)(E + 1), hipMemcpyHostToDevice));
}

template <typename T>
void mo_angles(const void *records, int64_t frames, int64_t markers, int64_t n_pairs, int64_t E, int64_t delay, int padding,
               const double *bounds, const double *vel_bounds, unsigned char *work, const MoLayout &at, void *angles, int64_t lda,
               void *vels, int64_t ldv) {
    const int32_t *d_pairs = (const int32_t *)(work + at.pairs);
    const int64_t *d_off = (const int64_t *)(work + at.offsets);
    const int cols = (int)(3 * n_pairs);
    hipLaunchKernelGGL((k_mo_angles<T>), dim3(mo_cells(frames * n_pairs)), dim3(kMoThreads), 0, 0, (const T *)records, (int32_t)frames,
                       (int32_t)markers, d_pairs, (int32_t)n_pairs, (T *)angles, lda);
    hipLaunchKernelGGL((k_mo_velocities<T>), dim3(mo_cells(frames * cols)), dim3(kMoThreads), 0, 0, (const T *)angles, lda,
                       (int32_t)frames, cols, d_off, (int32_t)E, delay, padding == KLNMF_MOTION_PAD_CIRCULAR ? 1 : 0,
                       vel_bounds ? 1 : 0, vel_bounds ? vel_bounds[0] : 0.0, vel_bounds ? vel_bounds[1] : 0.0, (T *)vels, ldv);
    if (bounds)
        hipLaunchKernelGGL((k_mo_clip<T>), dim3(mo_cells(frames * cols)), dim3(kMoThreads), 0, 0, (T *)angles, lda, (int32_t)frames,
                           cols, bounds[0], bounds[1]);
}

template <typename T>
void mo_whiten(const void *x, int64_t ld, int64_t frames, int64_t C, unsigned char *work, const MoLayout &at, void *out, int64_t ldo,
               double *mean, double *std) {
    double *part = (double *)work;
    const dim3 grid((unsigned)at.groups, (unsigned)((C + kMoMomCols - 1) / kMoMomCols));
    for (int mode = 0; mode < 2; ++mode) {
        hipLaunchKernelGGL((k_mo_moments<T>), grid, dim3(kMoThreads), 0, 0, (const T *)x, ld, (int32_t)frames, (int32_t)C, mode,
                           (const double *)mean, part);
        hipLaunchKernelGGL(k_mo_moments_reduce, dim3(mo_cells(C)), dim3(kMoThreads), 0, 0, (const double *)part, (int)at.groups,
                           (int32_t)frames, (int32_t)C, mode, mean, std);
    }
    hipLaunchKernelGGL((k_mo_scale<T>), dim3(mo_cells(frames * C)), dim3(kMoThreads), 0, 0, (const T *)x, ld, (int32_t)frames,
                       (int32_t)C, (const double *)std, (T *)out, ldo);
}

// The loop of klnmf_motion_kmeans_device; returns the lowest problem that has not stopped, or -1.
template <typename T>
int mo_kmeans(MoKm call, double thresh, int max_iter, unsigned char *work, const MoLayout &at, double *distortion, int32_t *iters,
              int32_t *labels) {
    double *psum = (double *)work, *pdist = (double *)(work + at.pdist);
    int32_t *pcnt = (int32_t *)(work + at.pcnt);
    const int P = call.P;
    const dim3 grid((unsigned)at.groups, (unsigned)P);
    hipLaunchKernelGGL(k_mo_km_init, dim3(mo_cells((int64_t)P * call.K)), dim3(kMoThreads), 0, 0, call, iters, distortion);
    std::vector<int32_t> done((size_t)P);
    for (int it = 1;; ++it) {
        hipLaunchKernelGGL((k_mo_assign<T>), grid, dim3(kMoThreads), mo_tile_bytes(call.d), 0, call, labels, psum, pcnt, pdist);
        hipLaunchKernelGGL((k_mo_update<T>), dim3((unsigned)P), dim3(kMoThreads), 0, 0, call, (int)at.groups, thresh,
                           (const double *)psum, (const int32_t *)pcnt, (const double *)pdist, iters, distortion);
        if (it % KLNMF_MOTION_POLL != 0 && it < max_iter) continue;
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpy(done.data(), call.done, sizeof(int32_t) * (size_t)P, hipMemcpyDeviceToHost));
        int open = -1;
        for (int p = 0; p < P && open < 0; ++p)
            if (!done[(size_t)p]) open = p;
        if (open < 0 || it >= max_iter) return open;
    }
}

template <typename T>
void mo_hist(MoHist call, int64_t E, unsigned char *work, void *out, int64_t ldo) {
    double *raw = (double *)work;
    hipLaunchKernelGGL((k_mo_hist<T>), dim3((unsigned)E, (unsigned)call.D), dim3(kMoThreads), mo_tile_bytes(call.d), 0, call, raw);
    hipLaunchKernelGGL((k_mo_hist_norm<T>), dim3((unsigned)E), dim3(kMoThreads), 0, 0, (const double *)raw, (int32_t)(call.D * call.K),
                       (T *)out, ldo);
}

}  // namespace
}  // namespace klnmf_host

extern "C" {

int klnmf_motion_work_bytes(int64_t T, int64_t C, int64_t d, int64_t K, int64_t P, int64_t D, int64_t E, uint64_t *bytes) {
    return guarded([&] {
        const MoWho w{{"klnmf_motion_work_bytes"}};
        if (!bytes) w.bad("null bytes");
        w.frames(T, 0);
        if (C < 0 || P < 0 || E < 0 || C >= kMaxInt || E >= kMaxInt) w.bad("C, P or E negative or not below 2^31 - 1");
        if (d < 1 || K < 1 || D < 1) w.bad("d, K or D < 1");
        w.limits(d, K, P, D);
        *bytes = (uint64_t)MoLayout(T, C, d, K, P, D, E).total;
    });
}

int klnmf_motion_angles_device(int device, int dtype, const void *records, int64_t T, int64_t n_markers, const int32_t *pairs,
                               int64_t n_pairs, const int64_t *offsets, int64_t E, int64_t delay, int padding,
                               const double *bounds, const double *vel_bounds, void *d_work, uint64_t work_bytes, void *angles,
                               int64_t lda, void *vels, int64_t ldv) {
    return guarded([&] {
        const MoWho w{{"klnmf_motion_angles_device"}};
        w.dtype(dtype);
        w.frames(T, 1);
        if (!records || !pairs || !angles || !vels || !d_work) w.bad("null records, pairs, angles, velocities or workspace");
        if (n_markers < 1 || n_markers >= kMaxInt / 8) w.bad("n_markers < 1 or too large");
        if (n_pairs < 1) w.bad("n_pairs < 1");
        if (n_pairs > kMoMaxPairs) w.unsupp("n_pairs = " + std::to_string(n_pairs) + " is above " + std::to_string(kMoMaxPairs));
        for (int64_t i = 0; i < 2 * n_pairs; ++i)
            if (pairs[i] < 0 || pairs[i] >= n_markers) w.bad("a pair index outside [0, n_markers)");
        if (lda < 3 * n_pairs || ldv < 3 * n_pairs) w.bad("a stride below 3 n_pairs");
        w.offsets(offsets, E, T);
        if (delay < 1) w.bad("delay < 1");
        if (padding != KLNMF_MOTION_PAD_ZEROS && padding != KLNMF_MOTION_PAD_CIRCULAR) w.bad("unknown padding");
        for (const double *b : {bounds, vel_bounds})
            if (b && !(b[0] <= b[1])) w.bad("bounds with min > max or a NaN");
        const MoLayout at(T, 0, 1, 1, 0, 1, E);
        w.workspace(work_bytes, at.total, "klnmf_motion_work_bytes");
        HIPCHK(hipSetDevice(device));
        unsigned char *work = (unsigned char *)d_work;
        mo_upload_offsets(work, at, offsets, E);
        HIPCHK(hipMemcpy(work + at.pairs, pairs, sizeof(int32_t) * 2 * (size_t)n_pairs, hipMemcpyHostToDevice));
        by_dtype(dtype, [&](auto tag) {
            mo_angles<tag_t<decltype(tag)>>(records, T, n_markers, n_pairs, E, delay, padding, bounds, vel_bounds, work, at, angles, lda,
                                            vels, ldv);
        });
        HIPCHK(hipGetLastError());
    });
}

int klnmf_motion_whiten_device(int device, int dtype, const void *x, int64_t ld, int64_t T, int64_t C, void *d_work,
                               uint64_t work_bytes, void *out, int64_t ldo, double *d_mean, double *d_std) {
    return guarded([&] {
        const MoWho w{{"klnmf_motion_whiten_device"}};
        w.dtype(dtype);
        w.frames(T, 1);
        if (!x || !out || !d_mean || !d_std || !d_work) w.bad("null x, out, mean, std or workspace");
        if (C < 1 || C >= kMaxInt) w.bad("C < 1");
        if (ld < C || ldo < C) w.bad("a stride below C");
        if ((C + kMoMomCols - 1) / kMoMomCols > kMoMaxGridY) w.unsupp("more than 32 * 65535 columns");
        const MoLayout at(T, C, 1, 1, 0, 1, 0);
        w.workspace(work_bytes, at.total, "klnmf_motion_work_bytes");
        HIPCHK(hipSetDevice(device));
        by_dtype(dtype, [&](auto tag) {
            mo_whiten<tag_t<decltype(tag)>>(x, ld, T, C, (unsigned char *)d_work, at, out, ldo, d_mean, d_std);
        });
        HIPCHK(hipGetLastError());
    });
}

int klnmf_motion_kmeans_device(int device, int dtype, const void *points, int64_t set_stride, int64_t ld, int64_t T, int64_t d,
                               int64_t D, const int32_t *set_of, int64_t P, void *codebooks, int64_t K, double thresh,
                               int max_iter, void *d_work, uint64_t work_bytes, int32_t *d_alive, double *d_distortion,
                               int32_t *d_iters, int32_t *d_labels, int *unfinished) {
    return guarded([&] {
        const MoWho w{{"klnmf_motion_kmeans_device"}};
        w.dtype(dtype);
        w.frames(T, 1);
        if (!points || !set_of || !codebooks || !d_alive || !d_distortion || !d_iters || !d_work || !unfinished)
            w.bad("null points, set_of, codebooks, alive, distortion, iters, workspace or unfinished");
        if (d < 1 || K < 1 || D < 1 || P < 1) w.bad("d, K, D or P < 1");
        if (ld < d || set_stride < 0) w.bad("a row stride below d or a negative set stride");
        if (!(thresh >= 0.0)) w.bad("a thresh that is negative or NaN");
        if (max_iter < 1) w.bad("max_iter < 1");
        w.limits(d, K, P, D);
        for (int64_t p = 0; p < P; ++p)
            if (set_of[p] < 0 || set_of[p] >= D) w.bad("a set_of entry outside [0, D)");
        const MoLayout at(T, 0, d, K, P, D, 0);
        w.workspace(work_bytes, at.total, "klnmf_motion_work_bytes");
        HIPCHK(hipSetDevice(device));
        unsigned char *work = (unsigned char *)d_work;
        HIPCHK(hipMemcpy(work + at.set_of, set_of, sizeof(int32_t) * (size_t)P, hipMemcpyHostToDevice));
        const MoKm call{points, codebooks, set_stride, ld, (int32_t)T, (int32_t)d, (int32_t)K, (int32_t)P,
                        (const int32_t *)(work + at.set_of), d_alive, (int32_t *)(work + at.done), (double *)(work + at.prev)};
        by_dtype(dtype, [&](auto tag) {
            *unfinished = mo_kmeans<tag_t<decltype(tag)>>(call, thresh, max_iter, work, at, d_distortion, d_iters, d_labels);
        });
    });
}

int klnmf_motion_hist_device(int device, int dtype, const void *points, int64_t set_stride, int64_t ld, int64_t T, int64_t d,
                             int64_t D, const void *codebooks, int64_t K, const int64_t *offsets, int64_t E, int soft,
                             double alpha, void *d_work, uint64_t work_bytes, void *out, int64_t ldo) {
    return guarded([&] {
        const MoWho w{{"klnmf_motion_hist_device"}};
        w.dtype(dtype);
        w.frames(T, 1);
        if (!points || !codebooks || !out || !d_work) w.bad("null points, codebooks, out or workspace");
        if (d < 1 || K < 1 || D < 1) w.bad("d, K or D < 1");
        if (ld < d || set_stride < 0) w.bad("a row stride below d or a negative set stride");
        w.offsets(offsets, E, T);
        if (soft != 0 && soft != 1) w.bad("soft outside {0, 1}");
        if (!std::isfinite(alpha)) w.bad("an alpha that is not finite");
        w.limits(d, K, 0, D);
        if (ldo < D * K) w.bad("an output stride below D * K");
        const MoLayout at(T, 0, d, K, 0, D, E);
        w.workspace(work_bytes, at.total, "klnmf_motion_work_bytes");
        HIPCHK(hipSetDevice(device));
        unsigned char *work = (unsigned char *)d_work;
        mo_upload_offsets(work, at, offsets, E);
        const MoHist call{points, codebooks, set_stride, ld, (int32_t)d, (int32_t)K, (int32_t)D, soft, alpha,
                          (const int64_t *)(work + at.offsets)};
        by_dtype(dtype, [&](auto tag) { mo_hist<tag_t<decltype(tag)>>(call, E, work, out, ldo); });
        HIPCHK(hipGetLastError());
    });
}

}  // extern "C"
