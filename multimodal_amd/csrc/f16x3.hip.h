// Split-operand fp16 contractions in a fused loop (KLNMF_PREC_F16X3, k <= 256): the fp32 mode's storage (V, Q, W, H in fp32) with
// W.H, Q.H^T and W^T.Q on v_mfma_f32_32x32x16_f16.
//
// Every operand x is split into two fp16 parts under a power-of-two scale s: hi = f16(x s), lo = f16(x s - hi) (the
// subtraction is exact in fp32); a contraction is hi.hi + hi.lo + lo.hi with fp32 accumulation, and the result is multiplied
// by the inverse scales (exact).  Each scale puts the largest operand it covers below 2^15 (fp16's largest finite value is
// 65504), so nothing saturates; a lo below 2^-14 (x far below the scaled maximum) keeps fewer bits and one below 2^-25 flushes
// to zero -- an absolute error of at most 2^-40 of the scaled maximum.  The scales (numpy emulation of whole fits:
// experiments/f16x3_emulation.py):
//   W.H     hs[j] per component row of H over all columns (k_x3_hscale, once per iteration); the W operand is W[r, j] / hs[j],
//           scaled per row r of the block (the two power-of-two factors are exact)
//   Q.H^T   Q per row per 64-column tile (the tile's ratios are in LDS: the scale is taken there), H as above
//   W^T.Q   Q per row over all columns: qr[r] = 2^e above the row's largest ratio (the row pass's running maximum); the W
//           operand is W_new[r, j] qr[r], scaled per component j over all rows (xmax[j]: an atomic maximum of the row pass)
//
// k_rowpass_x3<NB>: one workgroup per 64 rows, KP = 64 NB >= k components (zero-padded).  The rows' W image (hi and lo) is
// staged into LDS once; the workgroup then walks the columns in tiles of 64: the tile of H (hi and lo, [column][component]) into
// LDS, MFMA-1 (W.H, a 32 x 32 quadrant per wave), the fp32 epilogue (ratio (x + eps) / (y + eps) with any eps, the loss term
// in fp64 partials -- exact_Q's EpiQ arithmetic -- and the ratio stored in fp32 for the column pass), the ratio tile split into
// LDS, MFMA-2 (Q.H^T into 64 x KP fp32 accumulators held in registers across the tiles).  Behind the last tile: the W rule
// W_new = W (Q.H^T) (EpiW), qr, xmax.  LDS: 151 KiB at KP = 256 (one workgroup per CU; static_assert below).
// k_colpass_x3: W^T.Q of one row chunk into a fixed-order fp32 slab per chunk ([z][k][f], EpiN's layout) -- k_sum_partials /
// k_update_H on the slabs, the H rule and the exchange of the numerator are the fp32 mode's.
#pragma once
#include "common.hip.h"

namespace klnmf {

constexpr int F3_TOP = 15;          // scaled operands below 2^15
constexpr int F3_TR = 64;           // row-pass rows per workgroup
constexpr int F3_TC = 64;           // row-pass columns per tile
constexpr int F3_KMAX = 256;        // components of the fused loop
constexpr int F3_CK = 32;           // column-pass contraction step (rows)

typedef __attribute__((ext_vector_type(8))) _Float16 f3_h8;
typedef __attribute__((ext_vector_type(16))) float f3_f16;

// 2^(F3_TOP - e) for 2^(e-1) <= amax < 2^e (1 for amax = 0), clamped to the normal fp32 range so that it and its inverse are exact
__device__ __forceinline__ float f3_scale(float amax) {
    if (!(amax > 0.f)) return 1.f;
    int e;
    (void)frexpf(amax, &e);
    int s = F3_TOP - e;
    s = s > 126 ? 126 : (s < -126 ? -126 : s);
    return ldexpf(1.f, s);
}

__device__ __forceinline__ void f3_split(float x, _Float16 &hi, _Float16 &lo) {
    hi = (_Float16)x;
    lo = (_Float16)(x - (float)hi);
}

// hs[j] = f3_scale(max_c H[j, c]) for j < k, 1 for k <= j < KP; xmax[j] = 0 (the row pass's maxima of this iteration).
// One workgroup per component row.
KL_GLOBAL __launch_bounds__(256) void k_x3_hscale(const float *H, int64_t f, int k, float *hs, unsigned *xmax,
                                                  const DevState *st) {
    if (st && st->stop) return;
    __shared__ float red[4];
    const int j = blockIdx.x;
    float m = 0.f;
    if (j < k)
        for (int64_t c = threadIdx.x; c < f; c += 256) m = fmaxf(m, H[(int64_t)j * f + c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        hs[j] = j < k ? f3_scale(m) : 1.f;
        xmax[j] = 0u;
    }
}

// The fused row pass.  Q, qr, xmax: nullptr in a transform (no column pass follows).
template <int NB>
__global__ __launch_bounds__(256, 1) void k_rowpass_x3(int64_t n, int64_t f, int k, const float *V, const float *W, float *Wn,
                                                       const float *H, const float *hs, float *Q, float *qr, unsigned *xmax,
                                                       double *loss_part, float eps, const DevState *st) {
    if (st && st->stop) return;
    constexpr int KP = 64 * NB;
    constexpr int LK = KP + 8;                 // LDS row of a [.][component] image (16-byte aligned rows)
    constexpr int LQ = F3_TC + 8;
    __shared__ __attribute__((aligned(16))) _Float16 Wh[F3_TR][LK];
    __shared__ __attribute__((aligned(16))) _Float16 Wl[F3_TR][LK];
    __shared__ __attribute__((aligned(16))) _Float16 Hh[F3_TC][LK];      // [column][component]
    __shared__ __attribute__((aligned(16))) _Float16 Hl[F3_TC][LK];
    __shared__ __attribute__((aligned(16))) _Float16 Qs[2][F3_TR][LQ];   // the ratio tile: fp32 first (aliased), then hi / lo
    __shared__ float hsl[KP], hinv[KP];
    __shared__ float winv[F3_TR], qinv[F3_TR], qrl[F3_TR];
    __shared__ double red[16];
    static_assert(sizeof(Wh) * 4 + sizeof(Qs) + sizeof(float) * (2 * KP + 3 * F3_TR) + sizeof(red) <= 160 * 1024,
                  "k_rowpass_x3: static LDS beyond gfx950's 160 KiB");
    static_assert(sizeof(float) * F3_TR * (F3_TC + 2) <= sizeof(Qs), "fp32 ratio tile must fit the hi / lo images");
    float (*Qf)[F3_TC + 2] = reinterpret_cast<float (*)[F3_TC + 2]>(&Qs[0][0][0]);

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wm = wv >> 1, wn = wv & 1;
    const int64_t r0 = (int64_t)blockIdx.x * F3_TR;
    const int kh = 8 * (lane >> 5), l31 = lane & 31;

    for (int j = tid; j < KP; j += 256) {
        const float s = hs[j];
        hsl[j] = s;
        hinv[j] = 1.f / s;              // (powers of two: exact)
    }
    __syncthreads();
    // the rows' W image: W[r, j] / hs[j], scaled per row; 16 rows per wave, components across the lanes
    for (int rr = wv; rr < F3_TR; rr += 4) {
        const int64_t r = r0 + rr;
        float v[NB];
        float m = 0.f;
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            const int j = lane + 64 * t;
            v[t] = (r < n && j < k) ? W[r * k + j] * hinv[j] : 0.f;
            m = fmaxf(m, v[t]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        const float s = f3_scale(m);
#pragma unroll
        for (int t = 0; t < NB; ++t) f3_split(v[t] * s, Wh[rr][lane + 64 * t], Wl[rr][lane + 64 * t]);
        if (lane == 0) winv[rr] = 1.f / s;
    }

    f3_f16 acc2[NB];                     // Q.H^T: rows 32 wm.., components 32 (wn NB + b)..
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int g = 0; g < 16; ++g) acc2[b][g] = 0.f;
    double local = 0.0;
    float rowmax = 0.f;                   // this thread's share of row tid >> 2's largest ratio
    const int qrow = tid >> 2, qpart = tid & 3;

    for (int64_t c0 = 0; c0 < f; c0 += F3_TC) {
        // H tile, [column][component], scaled per component row
        for (int e = tid; e < F3_TC * KP; e += 256) {
            const int cc = e & (F3_TC - 1), j = e >> 6;
            const int64_t c = c0 + cc;
            const float x = (c < f && j < k) ? H[(int64_t)j * f + c] * hsl[j] : 0.f;
            f3_split(x, Hh[cc][j], Hl[cc][j]);
        }
        __syncthreads();
        // MFMA-1: W.H, quadrant (wm, wn)
        f3_f16 hh, xx;
#pragma unroll
        for (int g = 0; g < 16; ++g) { hh[g] = 0.f; xx[g] = 0.f; }
        {
            const int ar = 32 * wm + l31, bc = 32 * wn + l31;
#pragma unroll 4
            for (int s = 0; s < KP / 16; ++s) {
                const f3_h8 a_hi = *(const f3_h8 *)&Wh[ar][16 * s + kh];
                const f3_h8 a_lo = *(const f3_h8 *)&Wl[ar][16 * s + kh];
                const f3_h8 b_hi = *(const f3_h8 *)&Hh[bc][16 * s + kh];
                const f3_h8 b_lo = *(const f3_h8 *)&Hl[bc][16 * s + kh];
                xx = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_lo, xx, 0, 0, 0);
                hh = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_hi, hh, 0, 0, 0);
                xx = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo, b_hi, xx, 0, 0, 0);
            }
        }
        // epilogue: ratio, loss term, Q store; the fp32 ratio tile into LDS (zeros outside the matrix)
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int rr = 32 * wm + (g & 3) + 8 * (g >> 2) + 4 * (lane >> 5), cc = 32 * wn + l31;
            const int64_t r = r0 + rr, c = c0 + cc;
            float q = 0.f;
            if (r < n && c < f) {
                const float y = (hh[g] + xx[g]) * winv[rr];
                const float x = V[r * f + c];
                q = (x + eps) / (y + eps);
                if (Q) Q[r * f + c] = q;
                local += (double)(x * log(q) - x + y);
            }
            Qf[rr][cc] = q;
        }
        __syncthreads();
        // the tile's ratios per row: largest (4 threads per row), scale, split
        float qv[16];
        float m = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            qv[i] = Qf[qrow][16 * qpart + i];
            m = fmaxf(m, qv[i]);
        }
        m = fmaxf(m, __shfl_xor(m, 1, 64));
        m = fmaxf(m, __shfl_xor(m, 2, 64));
        rowmax = fmaxf(rowmax, m);
        const float qs = f3_scale(m);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; ++i) f3_split(qv[i] * qs, Qs[0][qrow][16 * qpart + i], Qs[1][qrow][16 * qpart + i]);
        if (qpart == 0) qinv[qrow] = 1.f / qs;
        __syncthreads();
        // MFMA-2: Q.H^T over the tile's 64 columns, rows 32 wm.., the wave's NB component blocks
        float qi[16];
#pragma unroll
        for (int g = 0; g < 16; ++g) qi[g] = qinv[32 * wm + (g & 3) + 8 * (g >> 2) + 4 * (lane >> 5)];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int jc = 32 * (wn * NB + b) + l31;
            f3_f16 th, tx;
#pragma unroll
            for (int g = 0; g < 16; ++g) { th[g] = 0.f; tx[g] = 0.f; }
#pragma unroll
            for (int s = 0; s < F3_TC / 16; ++s) {
                const f3_h8 a_hi = *(const f3_h8 *)&Qs[0][32 * wm + l31][16 * s + kh];
                const f3_h8 a_lo = *(const f3_h8 *)&Qs[1][32 * wm + l31][16 * s + kh];
                f3_h8 b_hi, b_lo;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    b_hi[i] = Hh[16 * s + kh + i][jc];
                    b_lo[i] = Hl[16 * s + kh + i][jc];
                }
                tx = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_lo, tx, 0, 0, 0);
                th = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_hi, th, 0, 0, 0);
                tx = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo, b_hi, tx, 0, 0, 0);
            }
#pragma unroll
            for (int g = 0; g < 16; ++g) acc2[b][g] += (th[g] + tx[g]) * qi[g];
        }
        __syncthreads();
    }

    // qr: 2^e above the row's largest ratio (the column pass divides the ratios by it)
    rowmax = fmaxf(rowmax, __shfl_xor(rowmax, 1, 64));
    rowmax = fmaxf(rowmax, __shfl_xor(rowmax, 2, 64));
    if (qpart == 0) {
        float q2 = 1.f;
        if (rowmax > 0.f) {
            int e;
            (void)frexpf(rowmax, &e);
            q2 = ldexpf(1.f, e > 126 ? 126 : (e < -126 ? -126 : e));
        }
        qrl[qrow] = q2;
        if (qr && r0 + qrow < n) qr[r0 + qrow] = q2;
    }
    __syncthreads();
    // the W rule, and the column pass's per-component maxima of W_new qr
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int j = 32 * (wn * NB + b) + l31;
        float m = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int rr = 32 * wm + (g & 3) + 8 * (g >> 2) + 4 * (lane >> 5);
            const int64_t r = r0 + rr;
            if (r < n && j < k) {
                const float w = W[r * k + j] * (acc2[b][g] * hinv[j]);
                Wn[r * k + j] = w;
                m = fmaxf(m, w * qrl[rr]);
            }
        }
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        if (xmax && lane < 32 && j < k) atomicMax(&xmax[j], __float_as_uint(m));     // (non-negative floats order as their bits)
    }
    const double t = block_sum(local, red);
    if (tid == 0) loss_part[blockIdx.x] = t;
}

// numerator slabs: Npart[z][j][c] = sum over the rows of chunk z of W[r, j] Q[r, c].  Grid (f tiles of 64, component tiles of 64,
// chunks); 2 x 2 waves of 32 x 32; contraction steps of F3_CK rows, the next step's fp32 operands loaded under the MFMAs.
KL_GLOBAL __launch_bounds__(256, 2) void k_colpass_x3(int64_t n, int64_t f, int k, const float *W, const float *Q, const float *qr,
                                                     const unsigned *xmax, float *Npart, int kchunk, const DevState *st) {
    if (st && st->stop) return;
    constexpr int LD = F3_CK + 8;
    __shared__ __attribute__((aligned(16))) _Float16 Ah[64][LD];      // [component][row]
    __shared__ __attribute__((aligned(16))) _Float16 Al[64][LD];
    __shared__ __attribute__((aligned(16))) _Float16 Bh[64][LD];      // [column][row]
    __shared__ __attribute__((aligned(16))) _Float16 Bl[64][LD];
    __shared__ float wsc[64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wm = wv >> 1, wn = wv & 1;
    const int64_t c0 = (int64_t)blockIdx.x * 64;
    const int j0 = blockIdx.y * 64;
    const int64_t rbeg = (int64_t)blockIdx.z * kchunk;
    const int64_t rend = min(n, rbeg + kchunk);
    const float qsc = ldexpf(1.f, F3_TOP - 1);
    if (tid < 64) wsc[tid] = (j0 + tid < k) ? f3_scale(__uint_as_float(xmax[j0 + tid])) : 1.f;
    __syncthreads();

    constexpr int PER = 64 * F3_CK / 256;
    float ra[PER], rb[PER];
    // element e of a step: row e >> 6, component / column e & 63 (consecutive threads walk the contiguous axis)
    auto fetch = [&](int64_t rs) {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int e = tid + 256 * u, jj = e & 63, rr = e >> 6;
            const int64_t r = rs + rr;
            const bool in = r < rend;
            const float q2 = in ? qr[r] : 1.f;
            ra[u] = (in && j0 + jj < k) ? W[r * k + j0 + jj] * q2 * wsc[jj] : 0.f;
            // (Q / qr first, below 1; qsc / qr is beyond fp32's range at the smallest qr, 2^-126)
            rb[u] = (in && c0 + jj < f) ? Q[r * f + c0 + jj] / q2 * qsc : 0.f;
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int e = tid + 256 * u, jj = e & 63, rr = e >> 6;
            f3_split(ra[u], Ah[jj][rr], Al[jj][rr]);
            f3_split(rb[u], Bh[jj][rr], Bl[jj][rr]);
        }
    };

    f3_f16 hh, xx;
#pragma unroll
    for (int g = 0; g < 16; ++g) { hh[g] = 0.f; xx[g] = 0.f; }
    if (rbeg < rend) { fetch(rbeg); commit(); }
    __syncthreads();
    const int ar = 32 * wm + (lane & 31), bc = 32 * wn + (lane & 31), kh = 8 * (lane >> 5);
    for (int64_t rs = rbeg; rs < rend; rs += F3_CK) {
        const bool more = rs + F3_CK < rend;
        if (more) fetch(rs + F3_CK);
#pragma unroll
        for (int s = 0; s < F3_CK / 16; ++s) {
            const f3_h8 a_hi = *(const f3_h8 *)&Ah[ar][16 * s + kh];
            const f3_h8 a_lo = *(const f3_h8 *)&Al[ar][16 * s + kh];
            const f3_h8 b_hi = *(const f3_h8 *)&Bh[bc][16 * s + kh];
            const f3_h8 b_lo = *(const f3_h8 *)&Bl[bc][16 * s + kh];
            xx = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_lo, xx, 0, 0, 0);
            hh = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_hi, hh, 0, 0, 0);
            xx = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo, b_hi, xx, 0, 0, 0);
        }
        __syncthreads();
        if (more) {
            commit();
            __syncthreads();
        }
    }
    const int64_t slab = (int64_t)k * f;
    const float qinv = ldexpf(1.f, 1 - F3_TOP);
    // the two inverse scales one after the other: their product wsc qsc is beyond fp32's range for a component whose largest
    // W_new qr is below 2^-98 (the slab would be 0), and the sum over wsc alone for one above 2^98
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        const int jj = 32 * wm + (g & 3) + 8 * (g >> 2) + 4 * (lane >> 5);
        const int64_t c = c0 + bc;
        if (j0 + jj < k && c < f)
            Npart[blockIdx.z * slab + (int64_t)(j0 + jj) * f + c] = (hh[g] + xx[g]) * qinv / wsc[jj];
    }
}

}  // namespace klnmf
