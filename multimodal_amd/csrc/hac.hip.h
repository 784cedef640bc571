// Windowed histograms of acoustic co-occurrences as CSR rows: what the reference's sliding evaluation does per
// window with `compute_coocurrences` (features/hac.py:152-175: scipy's vq, the lagged pair codes, np.bincount) and sp.vstack
// (samples/image_sound_eval_sliding.py:97-113), for all windows in a fixed number of launches.
//
//   k_hac_vq<T>      every frame of every stream quantised ONCE: q[t] = the code of vq.hip.h (its rule, its staging: a thread per
//                    frame; the stream's codebook and the block's frames are staged in LDS where the host found room for them,
//                    HacStream::stage, and read from global memory / L2 otherwise).  The unit that includes this header includes
//                    vq.hip.h before it.
//   k_hac_pass<T, 0> one workgroup per segment = (window, stream, lag): the number of DISTINCT pair codes q[t + lag] * K + q[t].
//   k_hac_scan       exclusive scan of the segment counts: the segment offsets, every (S * L)-th of them a row pointer, nnz.
//   k_hac_pass<T, 1> the same text again: the distinct codes in ascending order and their counts, at the segment's offset.
//
// Two routes per segment, by hac_route (host and device evaluate the same function):
//   sort   n_codes <= 4096: the codes in LDS, padded with a sentinel to a power of two, a bitonic network, then the run heads
//          (an ordered compaction of the positions where the sorted sequence changes; a run's length is the count);
//   dense  n_codes > 4096 and K^2 <= 36864: int32 counters over the K^2 bins in LDS (integer adds: exact, order-free), then an
//          ordered compaction of the non-zero bins.
// The segments of a row cover ascending, disjoint column ranges, so sorted segments are a sorted row.  Every count is an exact
// integer held in 32 bits (a window has fewer than 2^31 frames); every write is a plain vector store by exactly one thread.
#pragma once

namespace klnmf {

constexpr int kHacMaxStreams = 8, kHacMaxLags = 8;
constexpr int kHacThreads = 256;
constexpr int kHacSortMax = 4096;              // pair codes of a segment the sort route takes
constexpr int kHacDenseBins = 36864;           // K^2 of the dense route: 144 KiB of int32 counters (K <= 192)
constexpr int kHacVqLds = 64 * 1024;           // bytes of LDS k_hac_vq may stage a codebook and a frame tile in
constexpr int kHacScanItems = 8;
constexpr int32_t kHacSentinel = 0x7fffffff;

enum { HAC_ROUTE_NONE = 0, HAC_ROUTE_SORT = 1, HAC_ROUTE_DENSE = 2, HAC_ROUTE_UNFIT = -1 };
static_assert(kHacThreads == kVqTile, "k_hac_vq: vq.hip.h's tile, a thread per frame");

// The route of a segment of n_codes pair codes over a codebook of K units.
__host__ __device__ inline int hac_route(int64_t n_codes, int64_t K) {
    if (n_codes <= 0) return HAC_ROUTE_NONE;
    if (n_codes <= kHacSortMax) return HAC_ROUTE_SORT;
    return K * K <= kHacDenseBins ? HAC_ROUTE_DENSE : HAC_ROUTE_UNFIT;
}

struct HacStream {                              // one stream: frames [T, d], codebook [K, d]; device pointers, strides in elements
    const void *x, *cb;
    int64_t ldx, ldc;
    int32_t d, K;
    int32_t block0;                             // the first workgroup of the stream in k_hac_vq's grid
    int32_t stage;                              // VQ_STAGE_*: what the host found room for in LDS
};
struct HacStreams {                             // k_hac_vq's table, passed by value
    HacStream s[kHacMaxStreams];
    int32_t count, T;
};
struct HacPlan {                                // the passes' table, passed by value
    int32_t K[kHacMaxStreams];
    int32_t lag[kHacMaxLags];
    int32_t colbase[kHacMaxStreams * kHacMaxLags];   // first column of block (stream, lag): streams outer, lags in the caller's order
    int32_t S, L, T, pad;
};

template <typename T>
__global__ __launch_bounds__(kHacThreads) void k_hac_vq(HacStreams tab, int32_t *codes) {
    extern __shared__ double hac_vq_lds[];
    int s = 0;
    while (s + 1 < tab.count && (int)blockIdx.x >= tab.s[s + 1].block0) ++s;
    const HacStream st = tab.s[s];
    const int d = st.d, K = st.K;
    const T *x = (const T *)st.x, *cb = (const T *)st.cb;
    const int64_t frame0 = (int64_t)((int)blockIdx.x - st.block0) * kHacThreads;
    const int64_t t = frame0 + threadIdx.x;
    T *cbs = (T *)hac_vq_lds;
    T *xs = cbs + ((st.stage & VQ_STAGE_CODEBOOK) ? (int64_t)K * d : 0);
    if (st.stage & VQ_STAGE_CODEBOOK) vq_stage_codebook<T>(cbs, cb, st.ldc, K * d, d);
    if (st.stage & VQ_STAGE_FRAMES)
        vq_stage_frames<T>(xs, x, st.ldx, frame0, (int)min((int64_t)kHacThreads, (int64_t)tab.T - frame0), d);
    __syncthreads();
    if (t >= tab.T) return;
    codes[(int64_t)s * tab.T + t] = vq_code<T>(st.stage, x, st.ldx, t, xs, cb, st.ldc, cbs, K, d);
}

// Ordered compaction over the positions [0, M): emit(rank, i) for every i with flag(i), rank = the flagged positions before i.
// Returns their number (block-uniform).  `wtot`: kHacThreads / 64 ints of LDS.  kFill false: only the number.
template <bool kFill, typename Flag, typename Emit>
__device__ __forceinline__ int hac_compact(int M, Flag flag, Emit emit, int *wtot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;
    for (int c0 = 0; c0 < M; c0 += kHacThreads) {
        const int i = c0 + (int)threadIdx.x;
        const bool f = i < M && flag(i);
        const unsigned long long b = __ballot(f);
        const int before = __popcll(b & ((1ull << lane) - 1ull));
        __syncthreads();                        // (the previous round's readers of wtot are done)
        if (lane == 0) wtot[wave] = __popcll(b);
        __syncthreads();
        int wbase = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kHacThreads / 64; ++w) {
            const int c = wtot[w];
            wbase += w < wave ? c : 0;
            total += c;
        }
        if (kFill && f) emit(base + wbase + before, i);
        base += total;
    }
    return base;
}

// kFill false: seg_count[segment] = its distinct codes.  kFill true: their columns and counts at seg_off[segment] (< nnz).
template <typename T, bool kFill>
__global__ __launch_bounds__(kHacThreads) void k_hac_pass(HacPlan plan, const int32_t *codes, const int32_t *windows,
                                                          int32_t *seg_count, const int64_t *seg_off, int64_t nnz, int32_t *indices,
                                                          T *values) {
    extern __shared__ int32_t hac_lds[];
    __shared__ int wtot[kHacThreads / 64];
    const int64_t seg = blockIdx.x;
    const int SL = plan.S * plan.L;
    const int64_t w = seg / SL;
    const int r = (int)(seg % SL), s = r / plan.L, l = r % plan.L;
    const int K = plan.K[s], lag = plan.lag[l];
    const int64_t t0 = windows[2 * w], t1 = windows[2 * w + 1];
    const int64_t n64 = t1 - t0 - (int64_t)lag;
    const int route = hac_route(n64, K);
    const int n = (int)n64;
    const int32_t *q = codes + (int64_t)s * plan.T + t0;
    const int64_t off = kFill ? seg_off[seg] : 0;
    const int32_t colbase = plan.colbase[r];
    int distinct = 0;
    if (route == HAC_ROUTE_SORT) {
        int P = 64;
        while (P < n) P <<= 1;
        int32_t *a = hac_lds, *pos = hac_lds + P;          // pos: P + 1 entries (the launch reserves 2 P + 1)
        for (int i = threadIdx.x; i < P; i += kHacThreads) a[i] = i < n ? q[i + lag] * K + q[i] : kHacSentinel;
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = threadIdx.x; i < P; i += kHacThreads) {
                    const int p = i ^ j;
                    if (p > i) {
                        const int32_t x = a[i], y = a[p];
                        const bool up = (i & k) == 0;
                        if (up ? x > y : x < y) { a[i] = y; a[p] = x; }
                    }
                }
                __syncthreads();
            }
        distinct = hac_compact<kFill>(n, [&](int i) { return i == 0 || a[i] != a[i - 1]; },
                                      [&](int rank, int i) { pos[rank] = i; }, wtot);
        if (kFill) {
            if (threadIdx.x == 0) pos[distinct] = n;
            __syncthreads();
            for (int e = threadIdx.x; e < distinct; e += kHacThreads)
                if (off + e < nnz) {
                    indices[off + e] = colbase + a[pos[e]];
                    values[off + e] = (T)(pos[e + 1] - pos[e]);
                }
        }
    } else if (route == HAC_ROUTE_DENSE) {
        const int bins = K * K;
        int32_t *cnt = hac_lds;
        for (int i = threadIdx.x; i < bins; i += kHacThreads) cnt[i] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += kHacThreads) atomicAdd(&cnt[q[i + lag] * K + q[i]], 1);
        __syncthreads();
        distinct = hac_compact<kFill>(bins, [&](int i) { return cnt[i] != 0; },
                                      [&](int rank, int i) {
                                          if (off + rank < nnz) {
                                              indices[off + rank] = colbase + i;
                                              values[off + rank] = (T)cnt[i];
                                          }
                                      }, wtot);
    }
    if (!kFill && threadIdx.x == 0) seg_count[seg] = distinct;
}

// off[i] = cnt[0] + ... + cnt[i - 1] for i <= m (off[m] = nnz); indptr[i / SL] = off[i] where SL divides i.  One workgroup.
KL_GLOBAL __launch_bounds__(kHacThreads) void k_hac_scan(const int32_t *cnt, int64_t m, int SL, int64_t *off, int64_t *indptr) {
    __shared__ int64_t wtot[kHacThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t carry = 0;
    for (int64_t c0 = 0; c0 < m; c0 += (int64_t)kHacThreads * kHacScanItems) {
        const int64_t i0 = c0 + (int64_t)threadIdx.x * kHacScanItems;
        int64_t x[kHacScanItems];
        int64_t sum = 0;
#pragma unroll
        for (int u = 0; u < kHacScanItems; ++u) {
            x[u] = i0 + u < m ? (int64_t)cnt[i0 + u] : 0;
            sum += x[u];
        }
        int64_t inc = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t up = __shfl_up(inc, o, 64);
            inc += lane >= o ? up : 0;
        }
        __syncthreads();
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        int64_t wbase = 0, total = 0;
#pragma unroll
        for (int v = 0; v < kHacThreads / 64; ++v) {
            const int64_t c = wtot[v];
            wbase += v < wave ? c : 0;
            total += c;
        }
        int64_t run = carry + wbase + inc - sum;
#pragma unroll
        for (int u = 0; u < kHacScanItems; ++u) {
            const int64_t i = i0 + u;
            if (i < m) {
                off[i] = run;
                if (i % SL == 0) indptr[i / SL] = run;
            }
            run += x[u];
        }
        carry += total;
    }
    if (threadIdx.x == 0) {
        off[m] = carry;
        indptr[m / SL] = carry;
    }
}

}  // namespace klnmf
