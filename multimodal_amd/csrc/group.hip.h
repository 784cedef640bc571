// The exchange of a group of contexts driven from one host thread (api_group.hip, klnmf_group_*): an all-reduce (sum) of the H
// rule's numerator (nmf.py:349) and of the two loss doubles (nmf.py:214) over N per-context buffers, in two launches per context.
// `bufs` / `loss` are device-resident tables of the N peers' buffers (rank order); the buffers may live on other devices (peer
// access, fine-grained memory: DESIGN.md section 8).
//
//   phase A (k_group_reduce, context r)   slice r of the numerator := b0 + b1 + ... + b(N-1), summed in rank order and written in
//                                         place into r's own buffer; the N loss pairs, summed in rank order, into r's private slot
//   phase B (k_group_gather, context r)   slice s of r's buffer := slice s of owner s's buffer, for every s != r; r's loss pair :=
//                                         its private slot
//
// Write rule: in each phase a context writes only locations that no peer reads in that phase.  Phase A reads slice q of every
// buffer in context q and writes slice r of buffer r in context r only; it reads every loss pair and writes the private slot,
// which nobody else reads.  Phase B reads slice s of buffer s (never written in phase B) and the private slot, and writes the
// slices s != r of buffer r and r's loss pair, which no peer reads in phase B.  Between the phases the host orders the streams
// with events (api_group.hip): no kernel here waits on a flag, spins or reads anything another launch may still be writing.
//
// Determinism: every element is summed in rank order ((b0 + b1) + b2) + ..., whichever slice it falls in, and every context
// receives the owner's bits -- the replicas of H stay bit-identical and the result does not depend on where the slices end.
// Slices are whole 16-byte vectors (4 floats / 2 doubles); the last slice also takes the scalar tail of count % vector.
#pragma once
#include "common.hip.h"

namespace klnmf {

template <typename T> struct GroupVec;
template <> struct GroupVec<float> {
    using V = float4;
    static constexpr int n = 4;
    __device__ static V add(V a, V b) { return V{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; }
};
template <> struct GroupVec<double> {
    using V = double2;
    static constexpr int n = 2;
    __device__ static V add(V a, V b) { return V{a.x + b.x, a.y + b.y}; }
};

// First element of slice r (r = nranks: the end): slice bounds fall on whole vectors, the last slice ends at `count`
__host__ __device__ inline int64_t group_slice_begin(int64_t count, int nranks, int r, int vec) {
    if (r >= nranks) return count;
    return (count / vec) * r / nranks * vec;
}

constexpr int kGroupThreads = 256;

// Phase A, context `rank`.  st: the context's loop state (the whole exchange is a no-op once the stop rule has fired -- it fires
// in the same iteration on every context, on identical losses); nullptr: always run (selftest).
template <typename T>
__global__ void __launch_bounds__(kGroupThreads)
k_group_reduce(T *const *bufs, double *const *loss, int nranks, int rank, int64_t count, double *slot, const DevState *st) {
    if (st != nullptr && st->stop) return;
    using G = GroupVec<T>;
    using V = typename G::V;
    T *mine = bufs[rank];
    const int64_t e0 = group_slice_begin(count, nranks, rank, G::n), e1 = group_slice_begin(count, nranks, rank + 1, G::n);
    const int64_t v1 = e1 / G::n;          // whole vectors [e0 / n, v1); scalar tail [v1 * n, e1) (last slice only)
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = e0 / G::n + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < v1; v += stride) {
        V acc = reinterpret_cast<const V *>(bufs[0])[v];
        for (int q = 1; q < nranks; ++q) acc = G::add(acc, reinterpret_cast<const V *>(bufs[q])[v]);
        reinterpret_cast<V *>(mine)[v] = acc;
    }
    if (blockIdx.x != 0) return;
    for (int64_t i = v1 * G::n + threadIdx.x; i < e1; i += blockDim.x) {
        T acc = bufs[0][i];
        for (int q = 1; q < nranks; ++q) acc += bufs[q][i];
        mine[i] = acc;
    }
    if (threadIdx.x < 2) {
        double acc = loss[0][threadIdx.x];
        for (int q = 1; q < nranks; ++q) acc += loss[q][threadIdx.x];
        slot[threadIdx.x] = acc;
    }
}

// Phase B, context `rank`: blockIdx.y = the slice's owner s.  Block (0, rank) copies the loss sum into the context's own pair.
template <typename T>
__global__ void __launch_bounds__(kGroupThreads)
k_group_gather(T *const *bufs, double *loss_mine, int nranks, int rank, int64_t count, const double *slot, const DevState *st) {
    if (st != nullptr && st->stop) return;
    using G = GroupVec<T>;
    using V = typename G::V;
    const int s = (int)blockIdx.y;
    if (s == rank) {
        if (blockIdx.x == 0 && threadIdx.x < 2) loss_mine[threadIdx.x] = slot[threadIdx.x];
        return;
    }
    const T *src = bufs[s];
    T *dst = bufs[rank];
    const int64_t e0 = group_slice_begin(count, nranks, s, G::n), e1 = group_slice_begin(count, nranks, s + 1, G::n);
    const int64_t v1 = e1 / G::n;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = e0 / G::n + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < v1; v += stride)
        reinterpret_cast<V *>(dst)[v] = reinterpret_cast<const V *>(src)[v];
    if (blockIdx.x != 0) return;
    for (int64_t i = v1 * G::n + threadIdx.x; i < e1; i += blockDim.x) dst[i] = src[i];
}

}  // namespace klnmf
