// The atom x label information matrix (include/klnmf_information.h has the semantics): for a table of jobs -- a
// coefficient matrix A [n, k] with one label per row -- the mutual information between each atom's binned value and the presence
// of each label: what samples/plot_info_matrix.py:66-90, 126-136 computes with k * L calls of np.histogram and of
// metrics.mutual_information (lib/metrics.py:37-43) per run.  Four launches for all jobs of a call:
//   k_info_range<T>   a workgroup takes a chunk of rows x a tile of 64 atoms; lane = atom (loads coalesced along k), the waves walk
//                     the chunk's rows; the waves' minima / maxima meet in LDS in wave order and go to the chunk's slab.  A NaN
//                     makes the slab's minimum a NaN (the finite check rides here).
//   k_info_edges      one thread per atom: the chunks' slabs in chunk order -> (lo, hi), np.histogram's rule for lo == hi; a range
//                     that is not finite flags the job.
//   k_info_hist<T>    the same decomposition; the counters of the workgroup's atoms are privatised in LDS as [label][bin][atom],
//                     the atom fastest, so that the lanes of a wave that work on one row hit distinct counters; integer LDS adds,
//                     flushed with integer atomics on the global counts (zeros skipped).  The atom tile shrinks with L * B
//                     (info_atom_tile); where not one atom fits, the adds go straight to the global counts.  A tile narrower than
//                     the wave puts several rows into one wave (lane -> (row, atom)).  The label check rides here.
//   k_info_mi         a workgroup per atom: the column totals of its table in LDS, then one thread per label.
// Every count is an exact integer and every floating-point order is fixed: the outputs do not depend on scheduling.
// The bin edges and k_info_mi's sums round every product and sum on its own: plain operators, contraction off (vq.hip.h: why).
#pragma once
#pragma clang fp contract(off)
#include "common.hip.h"

namespace klnmf {

constexpr int kInfoThreads = 256;
constexpr int kInfoWaves = kInfoThreads / 64;
constexpr int kInfoRows = 1024;            // rows of a workgroup's chunk (more where a job has more than kInfoSlabs * kInfoRows rows)
constexpr int kInfoSlabs = 256;            // the most row chunks of a job: the slabs' size does not depend on n
constexpr int kInfoTile = 64;              // atoms of a full tile
constexpr int kInfoLdsBytes = 32768;       // the LDS budget of the privatised counters (KLNMF_INFORMATION_LDS_BYTES)
constexpr int kInfoMaxBins = 256;
constexpr int kInfoBadLabel = 1, kInfoNotFinite = 2;       // a job's flags

// Atoms whose counters a workgroup keeps in LDS: 64, fewer, or 0 (the global route).  A function of (L, B) alone.
__host__ __device__ inline int info_atom_tile(int L, int B) {
    const int64_t fit = (int64_t)kInfoLdsBytes / (4 * (int64_t)L * B);
    return (int)(fit < kInfoTile ? fit : kInfoTile);
}

struct InfoJob {                           // device pointers; the row stride in elements
    const void *A;
    const int32_t *labels;
    int64_t lda;
    int64_t atom0;                         // offset of the job's atoms in the outputs: the sum of k of the jobs before it
    int32_t n, k;
    int32_t chunk_rows, chunks;            // rows of a chunk; chunks = ceil(n / chunk_rows) <= kInfoSlabs, none of them empty
    int32_t range_block0, hist_block0;     // the job's first workgroup in the grids of k_info_range and k_info_hist
};

// The job of workgroup `block` of a grid in which the jobs' workgroups lie behind one another: the last q with first[q] <= block.
__device__ __forceinline__ int info_job_of_block(const InfoJob *jobs, int count, int block, int32_t InfoJob::*first) {
    int lo = 0, hi = count;                // the first q with first[q] > block
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (jobs[mid].*first <= block) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

__device__ __forceinline__ int info_job_of_atom(const InfoJob *jobs, int count, int64_t atom) {
    int lo = 0, hi = count;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (jobs[mid].atom0 <= atom) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// np.linspace(lo, hi, B + 1)[b] with its roundings written out (numpy/_core/function_base.py: y = arange * step + start, the
// last element set to stop; step == 0: y = arange / div * delta + start)
__device__ __forceinline__ double info_edge(int b, int B, double lo, double hi, double step, double delta) {
    if (b >= B) return hi;
    const double y = step != 0.0 ? (double)b * step : (double)b / (double)B * delta;
    return y + lo;
}

// The bin of v: the b with e_b <= v < e_(b+1), v == hi in B - 1.  `inv` = B / (hi - lo) only seeds the guess; the edges decide.
__device__ __forceinline__ int info_bin(double v, int B, double lo, double hi, double step, double delta, double inv) {
    int b = (int)((v - lo) * inv);
    b = min(max(b, 0), B - 1);
    while (b > 0 && v < info_edge(b, B, lo, hi, step, delta)) --b;
    while (b < B - 1 && v >= info_edge(b + 1, B, lo, hi, step, delta)) ++b;
    return b;
}

template <typename T>
__global__ __launch_bounds__(kInfoThreads) void k_info_range(const InfoJob *jobs, int count, int64_t total_atoms, double *slab_lo,
                                                             double *slab_hi) {
    __shared__ double smin[kInfoWaves][64], smax[kInfoWaves][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const InfoJob job = jobs[info_job_of_block(jobs, count, (int)blockIdx.x, &InfoJob::range_block0)];
    const int local = (int)blockIdx.x - job.range_block0;
    const int tile = local / job.chunks, chunk = local - tile * job.chunks;
    const int a = tile * kInfoTile + lane;
    const int64_t r0 = (int64_t)chunk * job.chunk_rows, r1 = min(r0 + job.chunk_rows, (int64_t)job.n);
    double mn = __builtin_huge_val(), mx = -__builtin_huge_val();
    bool nan = false;
    if (a < job.k) {
        const T *col = (const T *)job.A + a;
#pragma unroll 4
        for (int64_t r = r0 + wave; r < r1; r += kInfoWaves) {
            const double v = (double)col[r * job.lda];
            nan |= v != v;
            mn = fmin(mn, v);
            mx = fmax(mx, v);
        }
    }
    smin[wave][lane] = nan ? __builtin_nan("") : mn;
    smax[wave][lane] = mx;
    __syncthreads();
    if (wave == 0 && a < job.k) {
        for (int w = 0; w < kInfoWaves; ++w) {                    // wave order; a NaN stays
            const double x = smin[w][lane];
            nan |= x != x;
            mn = w ? fmin(mn, x) : x;
            mx = w ? fmax(mx, smax[w][lane]) : smax[w][lane];
        }
        const int64_t at = (int64_t)chunk * total_atoms + job.atom0 + a;
        slab_lo[at] = nan ? __builtin_nan("") : mn;
        slab_hi[at] = mx;
    }
}

KL_GLOBAL __launch_bounds__(kInfoThreads) void k_info_edges(const InfoJob *jobs, int count, int64_t total_atoms, const double *slab_lo,
                                                            const double *slab_hi, double *ranges, int32_t *flags) {
    const int64_t g = (int64_t)blockIdx.x * kInfoThreads + threadIdx.x;
    if (g >= total_atoms) return;
    const int q = info_job_of_atom(jobs, count, g);
    const int chunks = jobs[q].chunks;
    double lo = slab_lo[g], hi = slab_hi[g];
    bool nan = lo != lo;
#pragma unroll 8
    for (int c = 1; c < chunks; ++c) {                             // (unrolled: the slab loads of eight chunks are in flight together)
        const double x = slab_lo[(int64_t)c * total_atoms + g];
        nan |= x != x;
        lo = fmin(lo, x);
        hi = fmax(hi, slab_hi[(int64_t)c * total_atoms + g]);
    }
    if (nan || !isfinite(lo) || !isfinite(hi)) atomicOr(&flags[q], kInfoNotFinite);
    if (lo == hi) {                                                // np.histogram's _get_outer_edges
        lo -= 0.5;
        hi += 0.5;
    }
    ranges[2 * g] = lo;
    ranges[2 * g + 1] = hi;
}

// ta: info_atom_tile(L, B); the dynamic LDS holds 4 * L * B * ta bytes.  ta == 0: tiles of 64 atoms, global adds.
template <typename T>
__global__ __launch_bounds__(kInfoThreads) void k_info_hist(const InfoJob *jobs, int count, int L, int B, int ta, const double *ranges,
                                                            int32_t *flags, int32_t *counts) {
    extern __shared__ int info_cnt[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = info_job_of_block(jobs, count, (int)blockIdx.x, &InfoJob::hist_block0);
    const InfoJob job = jobs[q];
    const bool lds = ta > 0;
    const int tile_atoms = lds ? ta : kInfoTile;
    const int local = (int)blockIdx.x - job.hist_block0;
    const int tile = local / job.chunks, chunk = local - tile * job.chunks;
    const int a0 = tile * tile_atoms, tw = min(tile_atoms, job.k - a0);          // 1 <= tw <= 64
    const int cells = L * B * tw;                                                // <= kInfoLdsBytes / 4 on the LDS routes
    if (lds) {
        for (int i = threadIdx.x; i < cells; i += kInfoThreads) info_cnt[i] = 0;
        __syncthreads();
    }
    const int rpw = 64 / tw, sub = lane / tw, la = lane - sub * tw;              // rows of a wave instruction; this lane's row and atom
    const int64_t r0 = (int64_t)chunk * job.chunk_rows, r1 = min(r0 + job.chunk_rows, (int64_t)job.n);
    bool bad = false;
    if (sub < rpw) {
        const int64_t g = job.atom0 + a0 + la;
        const double lo = ranges[2 * g], hi = ranges[2 * g + 1];
        const double delta = hi - lo, step = delta / (double)B, inv = (double)B / delta;
        const T *col = (const T *)job.A + a0 + la;
        const int32_t *labels = job.labels;
        int32_t *mine = counts + g * L * B;
        auto count_one = [&](double v, int lab) {
            if ((unsigned)lab >= (unsigned)L) {
                bad = true;
                return;
            }
            const int b = info_bin(v, B, lo, hi, step, delta, inv);
            if (lds) atomicAdd(&info_cnt[(lab * B + b) * tw + la], 1);
            else atomicAdd(&mine[(int64_t)lab * B + b], 1);
        };
        const int64_t stride = (int64_t)kInfoWaves * rpw;
        int64_t r = r0 + wave * rpw + sub;
        for (; r + 3 * stride < r1; r += 4 * stride) {                          // four rows in flight
            const double v0 = (double)col[r * job.lda], v1 = (double)col[(r + stride) * job.lda];
            const double v2 = (double)col[(r + 2 * stride) * job.lda], v3 = (double)col[(r + 3 * stride) * job.lda];
            const int l0 = labels[r], l1 = labels[r + stride], l2 = labels[r + 2 * stride], l3 = labels[r + 3 * stride];
            count_one(v0, l0);
            count_one(v1, l1);
            count_one(v2, l2);
            count_one(v3, l3);
        }
        for (; r < r1; r += stride) count_one((double)col[r * job.lda], labels[r]);
    }
    if (bad) atomicOr(&flags[q], kInfoBadLabel);
    if (lds) {
        __syncthreads();
        int32_t *base = counts + (job.atom0 + a0) * L * B;
        for (int i = threadIdx.x; i < cells; i += kInfoThreads) {
            const int c = info_cnt[i];
            if (c) {
                const int cell = i / tw, a = i - cell * tw;                      // cell = label * B + bin
                atomicAdd(&base[(int64_t)a * L * B + cell], c);
            }
        }
    }
}

// One workgroup per atom g; thread l, l + 256, ...: the label.  info[o * L + l * k + a], o the job's atom offset.
KL_GLOBAL __launch_bounds__(kInfoThreads) void k_info_mi(const InfoJob *jobs, int count, int L, int B, const int32_t *counts,
                                                         double *info) {
    __shared__ int tot[kInfoMaxBins];
    const int64_t g = blockIdx.x;
    const int q = info_job_of_atom(jobs, count, g);
    const int64_t atom0 = jobs[q].atom0;
    const int k = jobs[q].k, a = (int)(g - atom0);
    const double N = (double)jobs[q].n;
    const int32_t *table = counts + g * L * B;
    if ((int)threadIdx.x < B) {
        int s = 0;
        for (int l = 0; l < L; ++l) s += table[(int64_t)l * B + threadIdx.x];
        tot[threadIdx.x] = s;
    }
    __syncthreads();
    for (int l = threadIdx.x; l < L; l += kInfoThreads) {
        const int32_t *t0 = table + (int64_t)l * B;
        int64_t s0 = 0, s1 = 0;
        for (int b = 0; b < B; ++b) {
            s0 += t0[b];
            s1 += tot[b] - t0[b];
        }
        const double pr0 = (double)s0 / N, pr1 = (double)s1 / N;
        double I = 0.0;
        for (int b = 0; b < B; ++b) {
            const int t = t0[b];
            if (t > 0) {
                const double p = (double)t / N, pc = (double)tot[b] / N;
                I = I + p * log(p / (pr0 * pc));
            }
        }
        for (int b = 0; b < B; ++b) {
            const int t = tot[b] - t0[b];
            if (t > 0) {
                const double p = (double)t / N, pc = (double)tot[b] / N;
                I = I + p * log(p / (pr1 * pc));
            }
        }
        info[atom0 * L + (int64_t)l * k + a] = I;
    }
}

}  // namespace klnmf
