// The bodies of k_presence_S, k_presence_D_part and k_presence_D_sum behind their stop test, included as text by those kernels
// (presence.hip.h) and by their batched forms (batch.hip.h), which first move the pointers to problem p's part of each buffer:
// what is summed is summed by one text, in one order, and each kernel's instruction stream is its own (gemm_body.hip.h's
// scheme).  No include guard: one section per inclusion, chosen by the macro the includer defines.  In scope at the inclusion:
//   KL_PRESENCE_BODY_S        T, H, bounds, S, f, k                     block (a, m) = (blockIdx.x, blockIdx.y)
//   KL_PRESENCE_BODY_D_PART   T, W, P, slab, n, k, nmod, chunk          block (x, z) = (blockIdx.x, blockIdx.y)
//   KL_PRESENCE_BODY_D_SUM    T, slab, nslab, count, D                  elements over (blockIdx.x, gridDim.x)
#if defined(KL_PRESENCE_BODY_S)
    __shared__ double red[16];
    const int64_t a = blockIdx.x, m = blockIdx.y;
    const int64_t j0 = bounds[m], j1 = bounds[m + 1];
    const T *row = H + a * f;
    double s = 0;
    for (int64_t j = j0 + threadIdx.x; j < j1; j += blockDim.x) s += (double)row[j];
    const double t = block_sum(s, red);
    if (threadIdx.x == 0) S[m * k + a] = (T)t;
#elif defined(KL_PRESENCE_BODY_D_PART)
    __shared__ double red[3][kMaxMod][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t a = (int64_t)blockIdx.x * 64 + lane;
    const int64_t i0 = (int64_t)blockIdx.y * chunk, i1 = min(n, i0 + chunk);
    double acc[kMaxMod];
#pragma unroll
    for (int m = 0; m < kMaxMod; ++m) acc[m] = 0.0;
    if (a < k) {
        for (int64_t i = i0 + wv; i < i1; i += 4) {
            const double w = (double)W[i * k + a];
            const T *prow = P + i * nmod;
#pragma unroll
            for (int m = 0; m < kMaxMod; ++m)
                if (m < nmod) acc[m] += w * (double)prow[m];
        }
    }
    if (wv > 0) {
#pragma unroll
        for (int m = 0; m < kMaxMod; ++m) red[wv - 1][m][lane] = acc[m];
    }
    __syncthreads();
    if (wv == 0 && a < k) {
        double *out = slab + ((int64_t)blockIdx.y * k + a) * nmod;
#pragma unroll
        for (int m = 0; m < kMaxMod; ++m)
            if (m < nmod) out[m] = ((acc[m] + red[0][m][lane]) + red[1][m][lane]) + red[2][m][lane];
    }
#elif defined(KL_PRESENCE_BODY_D_SUM)
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < count; e += (int64_t)gridDim.x * blockDim.x) {
        double s = 0;
        for (int z = 0; z < nslab; ++z) s += slab[z * count + e];
        D[e] = (T)s;
    }
#else
#error "presence_body.hip.h: define one of KL_PRESENCE_BODY_S / _D_PART / _D_SUM"
#endif
