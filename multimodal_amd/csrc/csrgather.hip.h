// Rows of device-resident CSR modalities gathered into a CSR problem (klnmf_upload_csr_device_rows, api_context.hip): the CSR of
//   hstack([c_m * X_m[rows] for m in modalities])                      (experiment.py:163-164 + learner.py:53-56 on sparse data)
// built in the context's own sp_indptr / sp_indices / sp_data from M <= kMaxMod sources that stay on the device across runs.
// Rows come in list order (any order, repeats allowed); within a row the entries go modality by modality with their columns
// offset by the modality's first column -- modalities are contiguous ascending column ranges and every source row is sorted, so
// the result is sorted.
//   k_csrg_len       len[r] = sum_m (indptr_m[idx[r] + 1] - indptr_m[idx[r]]), len[rows] = 0; a row index outside [0, src_rows) or
//                    a source row pointer that decreases sets bad[0] and counts as an empty row (nothing is read through it)
//   (csc.hip.h)      k_csc_scan_tiles / _part / _add: the exclusive scan of len[0 .. rows] in place -> the problem's row pointers
//   k_csrg_copy      one wave per output row, a (row, modality) cell in trips of kCsrgTrip = 64 entries, lane t of a trip its
//                    entry t: a long row is spread over the wave, a cell without entries takes no trip.  Writes the int64 column
//                    (source index + the modality's first column) and the value x * c, the product FORMED IN THE SOURCE'S
//                    ELEMENT TYPE with c rounded to it (what scipy's `csr * float(c)` gives: nmf._csr_of), then cast to the
//                    context's type (as set_matrix casts a host upload) -- the uploaded problem is bit for bit the host path's
//   k_csrg_dense     rows of ONE source into a zero-filled dense [rows, d] float64 matrix (klnmf_csr_rows_to_dense_device: the
//                    raw rows an evaluation compares reconstructions with, experiment.py:266)
// Sources: row pointers int64, column indices int32 (a modality has fewer than 2^31 columns; half the resident bytes of int64),
// values float32 or float64 per source.  Every store is a plain vector store; nothing is summed, so nothing depends on order.
#pragma once
#include "common.hip.h"
#include "presence.hip.h"      // kMaxMod

namespace klnmf {

constexpr int kCsrgThreads = 256;
constexpr int kCsrgTrip = 64;          // entries of a (row, modality) cell per trip: one per lane of the row's wave

// the sources of one call, passed by value (read through the kernel-argument segment: uniform loads, no table in device memory)
struct CsrSources {
    const int64_t *indptr[kMaxMod];
    const int *indices[kMaxMod];
    const void *data[kMaxMod];
    int64_t col0[kMaxMod];
    double scale[kMaxMod];
    int64_t src_rows;
    int n_mod;
    unsigned f64_mask;                 // bit m: the values of source m are float64 (else float32)
};

KL_GLOBAL __launch_bounds__(kCsrgThreads) void k_csrg_len(CsrSources S, const int64_t *idx, int64_t rows, int64_t *len, int64_t *bad) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r <= rows; r += stride) {
        int64_t total = 0;
        if (r < rows) {
            const int64_t i = idx[r];
            bool wrong = i < 0 || i >= S.src_rows;
            if (!wrong) {
                for (int m = 0; m < S.n_mod; ++m) {
                    const int64_t cell = S.indptr[m][i + 1] - S.indptr[m][i];
                    if (cell < 0) wrong = true;
                    total += cell;
                }
            }
            if (wrong) {
                bad[0] = 1;
                total = 0;
            }
        }
        len[r] = total;
    }
}

template <typename T, typename S>
__device__ __forceinline__ void csrg_copy_cell(const int *ci, const S *x, int64_t cell, int64_t col0, S c, int lane, int64_t *out_indices,
                                               T *out_data) {
    for (int64_t t = lane; t < cell; t += kCsrgTrip) {
        out_indices[t] = col0 + (int64_t)ci[t];
        const S prod = x[t] * c;       // in the source's type: see above
        out_data[t] = (T)prod;
    }
}

// Launched only after the host has read bad[0] == 0 and out_indptr[rows] == the problem's nnz: every idx[r] is a source row and
// every store lands in [0, nnz)
template <typename T>
__global__ __launch_bounds__(kCsrgThreads) void k_csrg_copy(CsrSources S, const int64_t *idx, int64_t rows, const int64_t *out_indptr,
                                                            int64_t *out_indices, T *out_data) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6; r < rows; r += nwaves) {
        const int64_t i = idx[r];
        int64_t o = out_indptr[r];
        for (int m = 0; m < S.n_mod; ++m) {
            const int64_t p0 = S.indptr[m][i], cell = S.indptr[m][i + 1] - p0;
            if (cell <= 0) continue;
            if ((S.f64_mask >> m) & 1u)
                csrg_copy_cell<T, double>(S.indices[m] + p0, (const double *)S.data[m] + p0, cell, S.col0[m], S.scale[m], lane,
                                          out_indices + o, out_data + o);
            else
                csrg_copy_cell<T, float>(S.indices[m] + p0, (const float *)S.data[m] + p0, cell, S.col0[m], (float)S.scale[m], lane,
                                         out_indices + o, out_data + o);
            o += cell;
        }
    }
}

// out[r, j] = x for every stored (idx[r], j, x) of the source; `out` ([rows, d], rows ld apart) is zero on entry.  One wave per
// output row; a row index outside [0, src_rows) or a column outside [0, d) writes nothing.
template <typename S>
__global__ __launch_bounds__(kCsrgThreads) void k_csrg_dense(const int64_t *indptr, const int *indices, const S *data, int64_t src_rows,
                                                             const int64_t *idx, int64_t rows, int64_t d, double *out, int64_t ld) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6; r < rows; r += nwaves) {
        const int64_t i = idx[r];
        if (i < 0 || i >= src_rows) continue;
        const int64_t p0 = indptr[i], p1 = indptr[i + 1];
        for (int64_t p = p0 + lane; p < p1; p += kCsrgTrip) {
            const int64_t j = indices[p];
            if (j >= 0 && j < d) out[r * ld + j] = (double)data[p];
        }
    }
}

}  // namespace klnmf
