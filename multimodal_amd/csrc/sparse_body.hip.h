// The bodies of k_sp_transpose_H, k_sp_colsum_part, k_sp_hsum_part, k_sp_dots and k_sp_loss behind their stop test, included as
// text by those kernels (sparse.hip.h) and by their batched forms (batch_sparse.hip.h), which first move the pointers to problem
// p's part of each buffer: one text, one summation order, and each kernel's instruction stream its own (gemm_body.hip.h's
// scheme).  No include guard: one section per inclusion, chosen by the macro the includer defines.  In scope at the inclusion:
//   KL_SP_BODY_TRANSPOSE   T, H, HT, k, f                               elements over (blockIdx.x, gridDim.x)
//   KL_SP_BODY_COLSUM      T, W, part, n, k                             row block = blockIdx.x
//   KL_SP_BODY_HSUM        T, H, f, seg, hpart                          (segment, component) = (blockIdx.x, blockIdx.y) of gridDim.x segments
//   KL_SP_BODY_DOTS        T, wpart, nblk, H, k, f, prod, hpart, S      component = blockIdx.x
//   KL_SP_BODY_LOSS        row_loss, n, prod, k, out, dec               one block
#if defined(KL_SP_BODY_TRANSPOSE)
    const int64_t total = k * f;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = e / k, a = e % k;
        HT[e] = H[a * f + j];
    }
#elif defined(KL_SP_BODY_COLSUM)
    const int64_t r0 = blockIdx.x * (int64_t)kSpColsumRows, r1 = min(n, r0 + kSpColsumRows);
    for (int64_t a = threadIdx.x; a < k; a += blockDim.x) {
        double s = 0;
        for (int64_t i = r0; i < r1; ++i) s += (double)W[i * k + a];
        part[blockIdx.x * k + a] = s;
    }
#elif defined(KL_SP_BODY_HSUM)
    __shared__ double red[16];
    const int64_t a = blockIdx.y, j0 = blockIdx.x * seg, j1 = min(f, j0 + seg);
    double hs = 0;
    for (int64_t j = j0 + threadIdx.x; j < j1; j += blockDim.x) hs += (double)H[a * f + j];
    const double t = block_sum(hs, red);
    if (threadIdx.x == 0) hpart[a * gridDim.x + blockIdx.x] = t;
#elif defined(KL_SP_BODY_DOTS)
    __shared__ double red[16];
    const int64_t a = blockIdx.x;
    double hs = 0, ws = 0;
    if (hpart != nullptr) {
        if (threadIdx.x == 0) for (int z = 0; z < S; ++z) hs += hpart[a * S + z];
    } else
    for (int64_t j = threadIdx.x; j < f; j += blockDim.x) hs += (double)H[a * f + j];
    for (int64_t b = threadIdx.x; b < nblk; b += blockDim.x) ws += wpart[b * k + a];
    const double hsum = block_sum(hs, red);
    const double wsum = block_sum(ws, red);
    if (threadIdx.x == 0) prod[a] = hsum * wsum;
#elif defined(KL_SP_BODY_LOSS)
    __shared__ double red[16];
    double s = 0;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) s += row_loss[i];
    for (int64_t a = threadIdx.x; a < k; a += blockDim.x) s += prod[a];
    const double t = block_sum(s, red);
    if (threadIdx.x == 0) { out[0] = t; out[1] = 0; decide_here(dec, t); }
#else
#error "sparse_body.hip.h: define one of KL_SP_BODY_TRANSPOSE / _COLSUM / _HSUM / _DOTS / _LOSS"
#endif
