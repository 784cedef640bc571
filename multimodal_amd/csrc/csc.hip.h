// The CSC order of a CSR problem, built on the device (klnmf_upload_csr_rows, api_context.hip): the stable order of the stored
// entries by column -- rows ascending within each column, exactly np.argsort(indices, kind='stable') -- as
//   csc_perm[e]    the CSR position of the e-th entry in CSC order
//   csc_rows[e]    its row
//   csc_indptr[j]  the first CSC position of column j (csc_indptr[f] = nnz)
//
// Method: an LSD radix sort of the CSR positions keyed by their column index, kCscBits bits per pass, as many passes as the bit
// width of f - 1 needs (at least one).  Only the positions move: a pass reads its key as indices[position], so the two int64
// arrays csc_perm / csc_rows serve as the passes' ping-pong buffers and no key array is kept.  Per pass:
//   k_csc_hist        per workgroup tile of kCscTile entries, the count of each digit (LDS integer counters) -> counts[digit][tile]
//   k_csc_scan_*      exclusive scan of counts in that digit-major order: the first output slot of (digit, tile)
//   k_csc_scatter     each wave ranks its 64-entry chunks in order (a multi-split by ballots: lanes of equal digit, lower lanes
//                     first) behind per-wave LDS counters; the waves' counts are prefixed in wave order, so an entry's slot is
//                     (digit, tile) base + earlier waves of the tile + earlier entries of its wave -- the pass is stable
// Every count is an exact integer and every order is fixed: the result does not depend on scheduling.  Then k_csc_rows (row of
// each entry by binary search in the CSR row pointers) and k_csc_indptr (first position of each column by binary search in the
// sorted keys).  k_csc_check validates the input first (row pointers non-decreasing, 0 <= index < f, indices non-decreasing
// within a row): the caller refuses bad input before any pass runs.
#pragma once
#include "common.hip.h"

namespace klnmf {

constexpr int kCscThreads = 256;
constexpr int kCscBits = 8;
constexpr int kCscBins = 1 << kCscBits;                      // (== kCscThreads: one bin per thread where bins are walked)
constexpr int kCscWaves = kCscThreads / 64;
constexpr int kCscItems = 16;                                 // 64-entry chunks per wave
constexpr int kCscTile = kCscThreads * kCscItems;             // entries per workgroup of a pass
constexpr int kCscScanItems = 8;
constexpr int kCscScanTile = kCscThreads * kCscScanItems;     // elements per workgroup of the scan
static_assert(kCscBins == kCscThreads, "one digit per thread");

// Row of CSR position p (0 <= p < nnz): the last r with indptr[r] <= p (empty rows share their pointer with the next row)
__device__ __forceinline__ int64_t csc_row_of(const int64_t *indptr, int64_t n, int64_t p) {
    int64_t lo = 0, hi = n + 1;                 // first u with indptr[u] > p
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (indptr[mid] <= p) lo = mid + 1; else hi = mid;
    }
    return min(max(lo - 1, (int64_t)0), n - 1);
}

// bad[0] := 1 if the row pointers decrease somewhere, an index lies outside [0, f), or the indices of a row decrease
KL_GLOBAL __launch_bounds__(256) void k_csc_check(const int64_t *indptr, const int64_t *indices, int64_t n, int64_t f, int64_t nnz,
                                                  int64_t *bad) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < max(n, nnz); t += stride) {
        bool wrong = t < n && indptr[t] > indptr[t + 1];
        if (t < nnz) {
            const int64_t j = indices[t];
            if (j < 0 || j >= f) wrong = true;
            else if (t > 0 && indices[t - 1] > j && t != indptr[csc_row_of(indptr, n, t)]) wrong = true;
        }
        if (wrong) bad[0] = 1;
    }
}

// counts[d * ntiles + tile] = entries of the tile whose digit (key >> shift) & (kCscBins - 1) is d.  src == nullptr: position e itself.
KL_GLOBAL __launch_bounds__(kCscThreads) void k_csc_hist(const int64_t *src, const int64_t *indices, int64_t nnz, int shift,
                                                         int64_t ntiles, int64_t *counts) {
    __shared__ int cnt[kCscBins];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = blockIdx.x * (int64_t)kCscTile;
    for (int i = 0; i < kCscItems; ++i) {
        const int64_t e = base + (int64_t)i * kCscThreads + threadIdx.x;
        if (e < nnz) {
            const int64_t v = src ? src[e] : e;
            atomicAdd(&cnt[(int)((indices[v] >> shift) & (kCscBins - 1))], 1);
        }
    }
    __syncthreads();
    counts[(int64_t)threadIdx.x * ntiles + blockIdx.x] = cnt[threadIdx.x];
}

// Exclusive prefix of one value per thread over the workgroup (Hillis-Steele in LDS); *total: the workgroup's sum
__device__ __forceinline__ int64_t csc_block_excl(int64_t s, int64_t *sh, int64_t *total) {
    const int t = threadIdx.x;
    sh[t] = s;
    __syncthreads();
    for (int off = 1; off < kCscThreads; off <<= 1) {
        const int64_t v = t >= off ? sh[t - off] : 0;
        __syncthreads();
        sh[t] += v;
        __syncthreads();
    }
    const int64_t incl = sh[t];
    *total = sh[kCscThreads - 1];
    __syncthreads();
    return incl - s;
}

// Exclusive scan of a[0 .. m) in place, tile by tile (kCscScanTile elements); part[tile] := the tile's sum
KL_GLOBAL __launch_bounds__(kCscThreads) void k_csc_scan_tiles(int64_t *a, int64_t m, int64_t *part) {
    __shared__ int64_t sh[kCscThreads];
    const int64_t base = blockIdx.x * (int64_t)kCscScanTile + (int64_t)threadIdx.x * kCscScanItems;
    int64_t x[kCscScanItems];
    int64_t s = 0;
#pragma unroll
    for (int i = 0; i < kCscScanItems; ++i) {
        x[i] = base + i < m ? a[base + i] : 0;
        s += x[i];
    }
    int64_t total;
    int64_t run = csc_block_excl(s, sh, &total);
#pragma unroll
    for (int i = 0; i < kCscScanItems; ++i) {
        if (base + i < m) a[base + i] = run;
        run += x[i];
    }
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// Exclusive scan of the tiles' sums part[0 .. np) in place: one workgroup, kCscThreads at a time with a carry
KL_GLOBAL __launch_bounds__(kCscThreads) void k_csc_scan_part(int64_t *part, int64_t np) {
    __shared__ int64_t sh[kCscThreads];
    int64_t carry = 0;
    for (int64_t c0 = 0; c0 < np; c0 += kCscThreads) {
        const int64_t i = c0 + threadIdx.x;
        const int64_t s = i < np ? part[i] : 0;
        int64_t total;
        const int64_t excl = csc_block_excl(s, sh, &total);
        if (i < np) part[i] = carry + excl;
        carry += total;
    }
}

// a[e] += part[tile of e]
KL_GLOBAL __launch_bounds__(256) void k_csc_scan_add(int64_t *a, int64_t m, const int64_t *part) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < m; e += stride) a[e] += part[e / kCscScanTile];
}

// One stable pass: dst[slot] = position, slot = offs[d * ntiles + tile] + entries of digit d in earlier waves of the tile + in
// earlier chunks and lower lanes of this wave.  Wave w of a tile takes its entries [w, w + 1) x kCscTile / kCscWaves in order.
KL_GLOBAL __launch_bounds__(kCscThreads) void k_csc_scatter(const int64_t *src, const int64_t *indices, int64_t nnz, int shift,
                                                            int64_t ntiles, const int64_t *offs, int64_t *dst) {
    __shared__ int wcnt[kCscWaves][kCscBins];
    __shared__ int64_t wbase[kCscWaves][kCscBins];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int q = 0; q < kCscWaves; ++q) wcnt[q][threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = blockIdx.x * (int64_t)kCscTile + (int64_t)w * (kCscTile / kCscWaves);
    const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    int64_t val[kCscItems];
    int dig[kCscItems], loc[kCscItems];
#pragma unroll
    for (int i = 0; i < kCscItems; ++i) {
        const int64_t e = base + (int64_t)i * 64 + lane;
        const bool ok = e < nnz;
        const int64_t v = ok ? (src ? src[e] : e) : 0;
        const int d = ok ? (int)((indices[v] >> shift) & (kCscBins - 1)) : 0;
        uint64_t peers = __ballot(ok);
#pragma unroll
        for (int b = 0; b < kCscBits; ++b) {
            const bool bit = (d >> b) & 1;
            const uint64_t m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const int rank = __popcll(peers & below);
        const int before = wcnt[w][d];          // (every lane's read completes before the leader's write below: it feeds it)
        if (ok && rank == 0) wcnt[w][d] = before + __popcll(peers);
        val[i] = v;
        dig[i] = d;
        loc[i] = before + rank;
    }
    __syncthreads();
    {
        int64_t run = offs[(int64_t)threadIdx.x * ntiles + blockIdx.x];
        for (int q = 0; q < kCscWaves; ++q) {
            wbase[q][threadIdx.x] = run;
            run += wcnt[q][threadIdx.x];
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kCscItems; ++i) {
        const int64_t e = base + (int64_t)i * 64 + lane;
        if (e < nnz) dst[wbase[w][dig[i]] + loc[i]] = val[i];
    }
}

// csc_rows[e] = row of CSR position perm[e]
KL_GLOBAL __launch_bounds__(256) void k_csc_rows(const int64_t *perm, const int64_t *indptr, int64_t n, int64_t nnz, int64_t *rows) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nnz; e += stride) rows[e] = csc_row_of(indptr, n, perm[e]);
}

// csc_indptr[j] = first e with indices[perm[e]] >= j, j = 0 .. f (the keys are sorted)
KL_GLOBAL __launch_bounds__(256) void k_csc_indptr(const int64_t *perm, const int64_t *indices, int64_t nnz, int64_t f,
                                                   int64_t *csc_indptr) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j <= f; j += stride) {
        int64_t lo = 0, hi = nnz;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (indices[perm[mid]] < j) lo = mid + 1; else hi = mid;
        }
        csc_indptr[j] = lo;
    }
}

// Workspace of the build (int64 elements): counts [kCscBins][tiles], the scan's tile sums, the check's flag
struct CscWork {
    int64_t tiles, m, nparts, elems;
    explicit CscWork(int64_t nnz) {
        tiles = nnz > 0 ? (nnz + kCscTile - 1) / kCscTile : 1;
        m = (int64_t)kCscBins * tiles;
        nparts = (m + kCscScanTile - 1) / kCscScanTile;
        elems = m + nparts + 1;
    }
    int64_t flag_at() const { return m + nparts; }
};

}  // namespace klnmf
