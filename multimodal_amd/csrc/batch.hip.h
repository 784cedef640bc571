// Batched forms of the dense exact loop's kernels (exact.hip.h): B unweighted -- or B masked (presence.hip.h) -- problems of one
// shape (n, f, k) advance through the loop of nmf.py:212-222 together, every stage ONE launch with the problem index on the grid.
//
//   k_gemm_batch<.., EpiQ / EpiW / EpiWpart / EpiN>   the four contractions: k_gemm's tile loop (gemm_body.hip.h), the same epilogues;
//                                                     problem p = blockIdx.y / (row tiles of one problem)
//   k_sum_doubles_batch                               loss reduction + stop rule, one block per problem     nmf.py:214-220
//   k_wrule_batch                                     the W rule from the feature chunks' slabs             nmf.py:338-343
//   k_sum_partials_batch                              the H numerator from the row chunks' slabs            nmf.py:349
//   k_update_H_batch / _part_batch / _norm_batch      the H rule: from slabs, from sums, in segments        nmf.py:349-350
// (the dense loop transposes nothing: a transposed operand of the tile loop is a stride swap)
// A masked batch -- every problem its own presence matrix P, one set of column bounds for all -- runs the same kernels under
// presence.hip.h's policies (EpiQ<T, PresenceWeight>, FacPresW, FacPresH: at_problem / fac_at_problem move their pointers) and
//   k_presence_S_batch                                S of every problem from its H, grid (k, M, B)
//   k_presence_D_part_batch / k_presence_D_sum_batch  D = W_new^T.P of every problem, grid (ceil(k / 64), presence_d_chunks(n), B)
// which are the single problem's kernels' own text (presence_body.hip.h) on problem p's buffers:
// P [B][n][M], S [B][M][k], D [B][k][M], D's slabs [B][chunks][k][M] in double; bounds and the modality bytes once per batch.
//
// Layout: every buffer of the single problem, B times, problem p at p x (the single problem's element count) -- V, Q, W[2], H,
// the slabs [B][chunks][..], loss partials [B][tiles], DevState [B], loss records [B][cap].
// Summation order: what is summed is summed by the code the single-context kernels run -- the tile loop, the epilogues, NumSlabs::get,
// h_product, block_sum, decide_here -- over the same chunk counts, so a problem in a batch has the bits of the same problem alone.
// Stop state: one DevState per problem; the blocks of a stopped problem return at their first instruction, as every block of a
// stopped context does, and nothing waits on anything.
// A beta batch (klnmf_batch_beta.h) -- every problem under one beta != 1, with its own weights Om where uploaded -- runs beta.hip.h's
// loop on the same layout, with B [B][n][f] beside Q (= A), a denominator set beside every numerator set and the rows' sums in
// hpart [B][k][segments]:
//   k_gemm_batch<.., EpiBeta<..>>                     the ratio pass: A, B, (LOSS) the loss partials
//   k_gemm_dual_batch<.., EpiW<T, FacBeta<T>> / EpiWpart<T, 2>, A>, <.., EpiN<T, 2>, B>   k_gemm_dual's own text (gemm_dual_body.hip.h)
//   k_wrule_batch / k_update_H_part_batch under FacBeta, k_sum_partials_sets_batch<T, 2>, k_update_H_sums_batch, k_scale_W_cols_batch
// CSR problems on a batch -- the batched forms of the sparse loop's kernels and their layout: batch_sparse.hip.h, included below.
#pragma once
#include "presence.hip.h"
#include "beta.hip.h"
#include "batch_sparse.hip.h"

namespace klnmf {

// the epilogue of problem p: its pointers moved to the problem's part of each buffer (M x N: the contraction's output shape;
// the slab epilogues hold gridDim.z slabs per problem)
template <typename T>
__device__ __forceinline__ EpiQ<T> at_problem(EpiQ<T> e, int p, int M, int N) {
    const int64_t o = (int64_t)p * M * N;
    e.V += o; e.Q += o;      // (loss_part: indexed by blockIdx.y, which carries p)
    return e;
}
template <typename T, typename Fac>
__device__ __forceinline__ EpiW<T, Fac> at_problem(EpiW<T, Fac> e, int p, int M, int N) {
    const int64_t o = (int64_t)p * M * N;
    e.Wold += o; e.Wnew += o;
    return e;
}
// the masked policies: P [n][nmod] and S [nmod][k] / D [k][nmod] of problem p
template <typename T>
__device__ __forceinline__ EpiQ<T, PresenceWeight<T>> at_problem(EpiQ<T, PresenceWeight<T>> e, int p, int M, int N) {
    const int64_t o = (int64_t)p * M * N;
    e.V += o; e.Q += o;
    e.wt.P += (int64_t)p * M * e.wt.nmod;
    return e;
}
// (a policy without pointers of its own -- FacNum, FacW0 -- is the same for every problem: itself, by reference)
template <typename Fac> __device__ __forceinline__ const Fac &fac_at_problem(const Fac &fac, int, int64_t, int64_t) { return fac; }
template <typename T>
__device__ __forceinline__ FacPresW<T> fac_at_problem(FacPresW<T> fac, int p, int64_t n, int64_t k) {
    fac.P += (int64_t)p * n * fac.nmod; fac.Sm += (int64_t)p * fac.nmod * k;
    return fac;
}
template <typename T>
__device__ __forceinline__ FacPresH<T> fac_at_problem(FacPresH<T> fac, int p, int64_t, int64_t k) {
    fac.D += (int64_t)p * k * fac.nmod;
    return fac;
}
template <typename T>
__device__ __forceinline__ EpiW<T, FacPresW<T>> at_problem(EpiW<T, FacPresW<T>> e, int p, int M, int N) {
    const int64_t o = (int64_t)p * M * N;
    e.Wold += o; e.Wnew += o;
    e.fac = fac_at_problem(e.fac, p, (int64_t)M, (int64_t)N);
    return e;
}
template <typename T>
__device__ __forceinline__ EpiWpart<T, 1> at_problem(EpiWpart<T, 1> e, int p, int, int) {
    e.P[0] += (int64_t)p * gridDim.z * e.slab;
    return e;
}
template <typename T>
__device__ __forceinline__ EpiN<T, 1> at_problem(EpiN<T, 1> e, int p, int, int) {
    e.Npart[0] += (int64_t)p * gridDim.z * e.slab;
    return e;
}

// the beta policies: V, A (the Q buffer) and B of problem p; with weights also Om
template <typename T, bool LOSS, int KIND>
__device__ __forceinline__ EpiBeta<T, NoWeight, LOSS, KIND> at_problem(EpiBeta<T, NoWeight, LOSS, KIND> e, int p, int M, int N) {
    const int64_t o = (int64_t)p * M * N;
    e.V += o; e.A += o; e.Bm += o;      // (loss_part: indexed by blockIdx.y, which carries p)
    return e;
}
template <typename T, bool LOSS, int KIND>
__device__ __forceinline__ EpiBeta<T, ElemWeight<T>, LOSS, KIND> at_problem(EpiBeta<T, ElemWeight<T>, LOSS, KIND> e, int p, int M, int N) {
    const int64_t o = (int64_t)p * M * N;
    e.V += o; e.A += o; e.Bm += o;
    e.wt.Om += o;
    return e;
}
// numerator and denominator slabs side by side (EpiW<T, FacBeta<T>>: the generic EpiW above -- FacBeta holds no pointer)
template <typename T>
__device__ __forceinline__ EpiWpart<T, 2> at_problem(EpiWpart<T, 2> e, int p, int, int) {
    const int64_t o = (int64_t)p * gridDim.z * e.slab;
    e.P[0] += o; e.P[1] += o;
    return e;
}
template <typename T>
__device__ __forceinline__ EpiN<T, 2> at_problem(EpiN<T, 2> e, int p, int, int) {
    const int64_t o = (int64_t)p * gridDim.z * e.slab;
    e.Npart[0] += o; e.Npart[1] += o;
    return e;
}

// k_gemm for B problems: grid (column tiles, B x ytiles, chunks); A and B `aps` / `bps` elements apart from problem to problem.
// The tile loop is k_gemm's own text (gemm_body.hip.h) on problem p's operands, in the instantiation the exact modes run
// (64 x 64 tiles on the fp64 / fp32 MFMA).
template <typename T, typename Epi>
__global__ __launch_bounds__(256, 3) void k_gemm_batch(int M, int N, int K, const T *A0, int64_t ars, int64_t acs, int64_t aps,
                                                       const T *B0, int64_t brs, int64_t bcs, int64_t bps, int kchunk,
                                                       const DevState *st, int ytiles, Epi epi0) {
    const int p = blockIdx.y / ytiles;
    if (st[p].stop) return;
    constexpr int TT = 4;
    constexpr bool MF = true;
    const T *A = A0 + p * aps, *B = B0 + p * bps;
    Epi epi = at_problem(epi0, p, M, N);
    const int row_tile = (int)blockIdx.y - p * ytiles;
#define KL_GEMM_ROW_TILE row_tile
#include "gemm_body.hip.h"
#undef KL_GEMM_ROW_TILE
}

// k_gemm_dual (weighted.hip.h) for B problems: the grid and the problem index of k_gemm_batch; A, B and X2 `aps` / `bps` / `xps`
// elements apart from problem to problem.  The tile loop is k_gemm_dual's own text (gemm_dual_body.hip.h) on problem p's operands.
template <typename T, typename Epi, bool SHARE_B>
__global__ __launch_bounds__(256, 2) void k_gemm_dual_batch(int M, int N, int K, const T *A0, int64_t ars, int64_t acs, int64_t aps,
                                                            const T *B0, int64_t brs, int64_t bcs, int64_t bps, const T *X20, int64_t xps,
                                                            int kchunk, const DevState *st, int ytiles, Epi epi0) {
    const int p = blockIdx.y / ytiles;
    if (st[p].stop) return;
    const T *A = A0 + p * aps, *B = B0 + p * bps, *X2 = X20 + p * xps;
    Epi epi = at_problem(epi0, p, M, N);
    const int row_tile = (int)blockIdx.y - p * ytiles;
#define KL_GEMM_DUAL_ROW_TILE row_tile
#include "gemm_dual_body.hip.h"
#undef KL_GEMM_DUAL_ROW_TILE
}

// k_sum_doubles with the stop rule, block p for problem p: `count` partials each, the loss into out[2 p]
KL_GLOBAL __launch_bounds__(1024) void k_sum_doubles_batch(const double *part, int64_t count, double *out, DevState *st, int decide,
                                                            double tol_abs, double *errors, int64_t cap) {
    const int p = blockIdx.x;
    if (st[p].stop) return;
    __shared__ double red[16];
    part += p * count;
    double s = 0;
    for (int64_t e = threadIdx.x; e < count; e += blockDim.x) s += part[e];
    const double t = block_sum(s, red);
    if (threadIdx.x == 0) {
        out[2 * p] = t; out[2 * p + 1] = 0;
        decide_here(DecideArgs{decide, st + p, tol_abs, errors + p * cap, cap}, t);
    }
}

// k_wrule_exact, grid (.., B): part / epi hold problem 0's pointers; part.slab = n k, part.nslab slabs per problem
template <typename T, typename Fac>
__global__ void k_wrule_batch(NumSlabs<T, Fac::S> part, const DevState *st, EpiW<T, Fac> epi) {
    const int p = blockIdx.y;
    if (st[p].stop) return;
    const NumSlabs<T, Fac::S> mine = part.at((int64_t)p * part.nslab * part.slab);
    epi.Wold += p * part.slab; epi.Wnew += p * part.slab;
    epi.fac = fac_at_problem(epi.fac, p, part.slab / epi.k, epi.k);      // (FacW0: itself)
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < part.slab; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = e / epi.k;
        epi.rule(e, r, e - r * epi.k, mine.get(e));
    }
}

// k_sum_partials, grid (.., B)
template <typename T>
__global__ void k_sum_partials_batch(NumArray<T, 1> part, T *out, int64_t count, int nslab, const DevState *st) {
    const int p = blockIdx.y;
    if (st[p].stop) return;
    const NumSlabs<T, 1> slabs{part.at((int64_t)p * nslab * count), nslab, count};
    out += p * count;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < count; e += (int64_t)gridDim.x * blockDim.x)
        out[e] = slabs.get(e)[0];
}

// k_sum_partials<T, S>, grid (.., B): S slab sets into S sums (a beta batch: numerator and denominator)
template <typename T, int S>
__global__ void k_sum_partials_sets_batch(NumArray<T, S> part, OutSets<T, S> out, int64_t count, int nslab, const DevState *st) {
    const int p = blockIdx.y;
    if (st[p].stop) return;
    const NumSlabs<T, S> slabs{part.at((int64_t)p * nslab * count), nslab, count};
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < count; e += (int64_t)gridDim.x * blockDim.x) {
        const Sums<T, S> v = slabs.get(e);
#pragma unroll
        for (int s = 0; s < S; ++s) out.p[s][p * count + e] = v[s];
    }
}

// elements from one problem's numerator source to the next's
template <typename T, int S> __device__ __forceinline__ int64_t problem_stride(const NumArray<T, S> &, int64_t kf) { return kf; }
template <typename T, int S> __device__ __forceinline__ int64_t problem_stride(const NumSlabs<T, S> &s, int64_t) { return s.nslab * s.slab; }

// k_update_H, grid (k, B); Fac: FacNum, or FacPresH with D [B][k][M]
template <typename T, typename Num, typename Fac = FacNum>
__global__ __launch_bounds__(256) void k_update_H_batch(T *H, RuleIn<Num, Fac> in, int64_t f, const DevState *st) {
    const int p = blockIdx.y;
    if (st[p].stop) return;
    __shared__ double red[16];
    __shared__ double total;
    const int64_t kf = (int64_t)gridDim.x * f;
    T *row = H + p * kf + blockIdx.x * f;
    const double s = h_product(row, in.num.at(p * problem_stride(in.num, kf) + blockIdx.x * f),
                               fac_at_problem(in.fac, p, 0, (int64_t)gridDim.x), (int64_t)blockIdx.x, 0, f);
    const double t = block_sum(s, red);
    if (threadIdx.x == 0) total = t;
    __syncthreads();
    const T d = (T)(kEpsNorm + total);
    for (int64_t j = threadIdx.x; j < f; j += blockDim.x) row[j] = row[j] / d;
}

// k_update_H_sums (beta.hip.h), grid (k, B): k_update_H_batch that also leaves each row's sum in sums[p k + a]
template <typename T, typename Num, typename Fac>
__global__ __launch_bounds__(256) void k_update_H_sums_batch(T *H, RuleIn<Num, Fac> in, int64_t f, double *sums, const DevState *st) {
    const int p = blockIdx.y;
    if (st[p].stop) return;
    __shared__ double red[16];
    __shared__ double total;
    const int64_t kf = (int64_t)gridDim.x * f;
    T *row = H + p * kf + blockIdx.x * f;
    const double s = h_product(row, in.num.at(p * problem_stride(in.num, kf) + blockIdx.x * f),
                               fac_at_problem(in.fac, p, 0, (int64_t)gridDim.x), (int64_t)blockIdx.x, 0, f);
    const double t = block_sum(s, red);
    if (threadIdx.x == 0) { total = t; sums[(int64_t)p * gridDim.x + blockIdx.x] = t; }
    __syncthreads();
    const T d = (T)(kEpsNorm + total);
    for (int64_t j = threadIdx.x; j < f; j += blockDim.x) row[j] = row[j] / d;
}

// k_scale_W_cols (beta.hip.h), grid (.., B): W_p[:, a] *= the sum of row a of H_p before its normalisation, part [B][k][nseg] re-added
// z ascending (k_update_H_norm's order; nseg = 1: k_update_H_sums_batch's sums)
template <typename T>
__global__ __launch_bounds__(256) void k_scale_W_cols_batch(T *W0, int64_t count, int64_t k, const double *part0, int nseg, const DevState *st) {
    const int p = blockIdx.y;
    if (st[p].stop) return;
    T *W = W0 + p * count;
    const double *part = part0 + (int64_t)p * k * nseg;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < count; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t a = e % k;
        double total = 0;
        for (int z = 0; z < nseg; ++z) total += part[a * nseg + z];
        W[e] = W[e] * (T)total;
    }
}

// k_update_H_part / k_update_H_norm, grid (segments, k, B); part [B][k][segments]
template <typename T, typename Fac = FacNum>
__global__ __launch_bounds__(256) void k_update_H_part_batch(T *H, RuleIn<NumArray<T, Fac::S>, Fac> in, int64_t f, int64_t seg,
                                                             double *part, const DevState *st) {
    const int p = blockIdx.z;
    if (st[p].stop) return;
    __shared__ double red[16];
    const int64_t a = blockIdx.y, j0 = blockIdx.x * seg, j1 = min(f, j0 + seg), pa = (int64_t)p * gridDim.y + a;
    const double s = h_product(H + pa * f, in.num.at(pa * f), fac_at_problem(in.fac, p, 0, (int64_t)gridDim.y), a, j0, j1);
    const double t = block_sum(s, red);
    if (threadIdx.x == 0) part[pa * gridDim.x + blockIdx.x] = t;
}
template <typename T>
__global__ __launch_bounds__(256) void k_update_H_norm_batch(T *H, int64_t f, int64_t seg, const double *part, const DevState *st) {
    const int p = blockIdx.z;
    if (st[p].stop) return;
    const int64_t j0 = blockIdx.x * seg, j1 = min(f, j0 + seg), pa = (int64_t)p * gridDim.y + blockIdx.y;
    double total = 0;
    for (unsigned z = 0; z < gridDim.x; ++z) total += part[pa * gridDim.x + z];      // (every thread: the same order, the same bits)
    const T d = (T)(kEpsNorm + total);
    T *row = H + pa * f;
    for (int64_t j = j0 + threadIdx.x; j < j1; j += blockDim.x) row[j] = row[j] / d;
}

// ---- what only a masked batch runs: presence.hip.h's kernels (their text: presence_body.hip.h) on problem p's buffers ------------
// k_presence_S, grid (k, M, B)
template <typename T>
__global__ __launch_bounds__(256) void k_presence_S_batch(const T *H0, const int64_t *bounds, T *S0, int64_t f, int64_t k, const DevState *st) {
    const int p = blockIdx.z;
    if (st[p].stop) return;
    const T *H = H0 + p * k * f;
    T *S = S0 + (int64_t)p * gridDim.y * k;
#define KL_PRESENCE_BODY_S
#include "presence_body.hip.h"
#undef KL_PRESENCE_BODY_S
}

// k_presence_D_part, grid (ceil(k / 64), chunks, B); slabs [B][chunks][k][nmod]
template <typename T>
__global__ __launch_bounds__(256) void k_presence_D_part_batch(const T *W0, const T *P0, double *slab0, int64_t n, int64_t k, int nmod,
                                                               int64_t chunk, const DevState *st) {
    const int p = blockIdx.z;
    if (st[p].stop) return;
    const T *W = W0 + p * n * k, *P = P0 + p * n * nmod;
    double *slab = slab0 + (int64_t)p * gridDim.y * k * nmod;
#define KL_PRESENCE_BODY_D_PART
#include "presence_body.hip.h"
#undef KL_PRESENCE_BODY_D_PART
}

// k_presence_D_sum, grid (.., B); count = k nmod
template <typename T>
__global__ void k_presence_D_sum_batch(const double *slab0, int nslab, int64_t count, T *D0, const DevState *st) {
    const int p = blockIdx.y;
    if (st[p].stop) return;
    const double *slab = slab0 + (int64_t)p * nslab * count;
    T *D = D0 + p * count;
#define KL_PRESENCE_BODY_D_SUM
#include "presence_body.hip.h"
#undef KL_PRESENCE_BODY_D_SUM
}

}  // namespace klnmf
