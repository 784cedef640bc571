// Split-operand bf16 contractions (KLNMF_PREC_BF16X3): the exact fp32 mode's GEMMs on the bf16 matrix cores.
//
// Every fp32 operand element x is split ONCE, when its tile is staged into LDS, into two bf16 parts:
//     hi = bf16_rne(x),   lo = bf16_rne(x - hi)          (the subtraction is exact in fp32)
// and a contraction is hi.hi + hi.lo + lo.hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  The dropped lo.lo term
// and the rounding of lo leave each product within about 2^-16 of a.b (relative); bf16 has fp32's exponent range, so
// no scaling is needed (operands must stay below bf16's largest finite value, 3.39e38).  The conversion is a plain cast
// (v_cvt_pk_bf16_f32: NaN stays NaN).  numpy emulation of the split and of whole fits: experiments/split3_emulation.py.
//
// k_gemm_x3 has the launch contract of k_gemm<float, Epi, 4, true> (exact.hip.h): C[M,N] = A[M,K] . B[K,N], element (r,c)
// of A at A[r*ars + c*acs] (a transposed operand is a stride swap), blockIdx.z the contraction chunk
// [z*kchunk, (z+1)*kchunk), the DevState stop flag, Epi::apply(r, c, float) per output and Epi::finish(red) per block --
// so EpiQ / EpiW / EpiWpart / EpiN / EpiStore, their loss partials (one per 64 x 64 tile) and slab layouts are shared.
// Any M, N, K: edge tiles and the K tail are staged as zeros (a zero hi/lo pair contributes exactly zero); no bound on K.
//
// 256 threads, 64 x 64 output tile, 2 x 2 waves of 32 x 32; contraction steps of 32 (two MFMA k-steps).  LDS images
// [row][k] with k contiguous (rows of 40 bf16 = 80 B: the ds_read_b128 operand reads of 16 consecutive rows hit distinct
// banks), for A and for B^T, hi and lo each: 20 KiB.  Operand maps (cdna_hip_programming.md section 3, 32x32x16 bf16): lane l
// holds A[row l & 31][k = 8 (l >> 5) + j] and B[k = 8 (l >> 5) + j][col l & 31], j = 0..7; result register g of lane l is
// D[(g & 3) + 8 (g >> 2) + 4 (l >> 5)][l & 31].  hi.hi and the two cross products go to two accumulators, the cross
// products with the hi.hi MFMA between them (no back-to-back dependency); a third accumulator would take the kernel past
// 168 VGPRs, i.e. from three waves per SIMD to two (measured at C3's shape: the W.H kernel 5.48 ms with three, 4.00 with two).  The next step's
// fp32 operands are loaded into registers under the current step's MFMAs, as in k_gemm.
#pragma once
#include "common.hip.h"

namespace klnmf {

constexpr int X3_TL = 64;            // output tile edge (= GT of exact.hip.h: EpiQ writes one loss partial per 64 x 64 tile)
constexpr int X3_BK = 32;            // contraction step
constexpr int X3_LD = X3_BK + 8;     // LDS row, bf16 elements

typedef __attribute__((ext_vector_type(8))) __bf16 x3_bf16x8;
typedef __attribute__((ext_vector_type(16))) float x3_f32x16;

template <typename Epi>
__global__ __launch_bounds__(256, 3) void k_gemm_x3(int M, int N, int K, const float *A, int64_t ars, int64_t acs,
                                                    const float *B, int64_t brs, int64_t bcs, int kchunk,
                                                    const DevState *st, Epi epi) {
    if (st && st->stop) return;
    __shared__ __attribute__((aligned(16))) __bf16 Ah[X3_TL][X3_LD];
    __shared__ __attribute__((aligned(16))) __bf16 Al[X3_TL][X3_LD];
    __shared__ __attribute__((aligned(16))) __bf16 Bh[X3_TL][X3_LD];      // B^T: [column][k]
    __shared__ __attribute__((aligned(16))) __bf16 Bl[X3_TL][X3_LD];
    __shared__ double red[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wm = wv >> 1, wn = wv & 1;            // this wave's 32 x 32 quadrant
    const int m0 = blockIdx.y * X3_TL, n0 = blockIdx.x * X3_TL;
    const int kbeg = blockIdx.z * kchunk;
    const int kend = min(K, kbeg + kchunk);

    x3_f32x16 acc_hh, acc_x;          // hi.hi; hi.lo + lo.hi
#pragma unroll
    for (int g = 0; g < 16; ++g) { acc_hh[g] = 0.f; acc_x[g] = 0.f; }

    const bool a_k_contig = (acs == 1);   // consecutive threads walk the contiguous axis
    const bool b_n_contig = (bcs == 1);
    const bool m_inside = m0 + X3_TL <= M, n_inside = n0 + X3_TL <= N;
    constexpr int PER = X3_TL * X3_BK / 256;      // elements of A (and of B) per thread and step
    float ra[PER], rb[PER];
    // element e of a step's A tile: (row m, k kk); of its B tile: (column n, k kk)
    auto a_pos = [&](int e, int &m, int &kk) {
        if (a_k_contig) { kk = e % X3_BK; m = e / X3_BK; } else { m = e % X3_TL; kk = e / X3_TL; }
    };
    auto b_pos = [&](int e, int &n, int &kk) {
        if (b_n_contig) { n = e % X3_TL; kk = e / X3_TL; } else { kk = e % X3_BK; n = e / X3_BK; }
    };
    auto fetch = [&](int k0) {
        const bool k_inside = k0 + X3_BK <= kend;
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            int m, kk;
            a_pos(tid + 256 * u, m, kk);
            const int gm = m0 + m, gk = k0 + kk;
            if (m_inside && k_inside) ra[u] = A[(int64_t)gm * ars + (int64_t)gk * acs];
            else ra[u] = (gm < M && gk < kend) ? A[(int64_t)gm * ars + (int64_t)gk * acs] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            int n, kk;
            b_pos(tid + 256 * u, n, kk);
            const int gn = n0 + n, gk = k0 + kk;
            if (n_inside && k_inside) rb[u] = B[(int64_t)gk * brs + (int64_t)gn * bcs];
            else rb[u] = (gn < N && gk < kend) ? B[(int64_t)gk * brs + (int64_t)gn * bcs] : 0.f;
        }
    };
    // the split, once per staged element
    auto commit = [&]() {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            int m, kk;
            a_pos(tid + 256 * u, m, kk);
            const __bf16 hi = (__bf16)ra[u];
            Ah[m][kk] = hi;
            Al[m][kk] = (__bf16)(ra[u] - (float)hi);
        }
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            int n, kk;
            b_pos(tid + 256 * u, n, kk);
            const __bf16 hi = (__bf16)rb[u];
            Bh[n][kk] = hi;
            Bl[n][kk] = (__bf16)(rb[u] - (float)hi);
        }
    };

    if (kbeg < kend) { fetch(kbeg); commit(); }
    __syncthreads();
    const int orow = 32 * wm + (lane & 31), ocol = 32 * wn + (lane & 31), kh = 8 * (lane >> 5);
    for (int k0 = kbeg; k0 < kend; k0 += X3_BK) {
        const bool more = k0 + X3_BK < kend;
        if (more) fetch(k0 + X3_BK);
#pragma unroll
        for (int s = 0; s < X3_BK / 16; ++s) {
            const x3_bf16x8 a_hi = *(const x3_bf16x8 *)&Ah[orow][16 * s + kh];
            const x3_bf16x8 a_lo = *(const x3_bf16x8 *)&Al[orow][16 * s + kh];
            const x3_bf16x8 b_hi = *(const x3_bf16x8 *)&Bh[ocol][16 * s + kh];
            const x3_bf16x8 b_lo = *(const x3_bf16x8 *)&Bl[ocol][16 * s + kh];
            acc_x = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b_lo, acc_x, 0, 0, 0);
            acc_hh = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b_hi, acc_hh, 0, 0, 0);
            acc_x = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo, b_hi, acc_x, 0, 0, 0);
        }
        __syncthreads();
        if (more) {
            commit();
            __syncthreads();
        }
    }
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        const int r = m0 + 32 * wm + (g & 3) + 8 * (g >> 2) + 4 * (lane >> 5), c = n0 + ocol;
        if (r < M && c < N) epi.apply(r, c, acc_hh[g] + acc_x[g]);
    }
    epi.finish(red);
}

}  // namespace klnmf
