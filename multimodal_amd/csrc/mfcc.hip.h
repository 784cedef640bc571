// The MFCC front end of the sound modality (include/features/klnmf_mfcc.h states the rules): audio samples to mel
// energies, cepstra and the two delta streams.  Included by api_mfcc.hip alone.
//
// Every operation is fp64 and rounded on its own (contraction off, as in vq.hip.h), there are no floating-point atomics, and every
// sum is formed in a stated order that depends on the call's sizes alone -- never on where an utterance lies in a batch: an
// utterance alone and the same utterance inside a batch give the same bits.
//
// k_mfcc_rows   one thread per mel filter: the span [lo, hi) of its non-zero weights.  A weight of +0 adds +0 to a non-negative
//               sum, so leaving the bins outside the span out changes no bit of a finite result; a triangle spans a few bins of
//               the n_fft / 2 + 1.
// k_mfcc_mel    one workgroup per frame: the frame gathered from the UNPADDED samples by the reflected index, times the window,
//               transformed in LDS, squared, contracted with the filter bank (bins ascending), S[t, :] stored; the workgroup's
//               largest energy goes to wgmax[t].
//     fft       n_fft = 2^p in [64, 4096]: radix-2 decimation in time, in place, on re[n], im[n] (two arrays: a lane reads and
//               writes 8-byte words, neighbouring lanes neighbouring words from the stage of half-length 32 on), the frame
//               stored bit-reversed as it is gathered.  Stage s pairs j and j + 2^s with the twiddle tab[k * n / 2^(s+1)].
//     direct    any even n_fft in [16, 1024]: bin b = sum_j u_j * tab[(j * b) mod n_fft], j ascending, the table in LDS.
// k_mfcc_smax   one workgroup per utterance: the largest of its frames' wgmax (a maximum has no order).
// k_mfcc_cepstra  a tile of frames per workgroup: 10 log10(max(S, 1e-10)), the utterance's floor, then D . Ldb CENTRED on the
//               utterance's top level: sum_m D[i, m] (Ldb[m] - top), m ascending, plus top * rowsum[i] with the basis' exact row sums
//               from the host.  The summands are the levels below the top (0 to -80 dB), not the absolute levels, so the sum's
//               rounding does not grow with the signal's scale, and a flat spectrum gives top * rowsum[i] exactly.
// k_mfcc_delta  one thread per (frame, coefficient): both delta streams from the fp64 cepstra, the utterance edge-padded on its own.
#pragma once
#pragma clang fp contract(off)

namespace klnmf {

constexpr int kMfccThreads = 256;
constexpr int kMfccFftMin = 64, kMfccFftMax = 4096;          // the fft route: powers of two
constexpr int kMfccDirectMin = 16, kMfccDirectMax = 1024;    // the direct route: even sizes
constexpr int kMfccCepFrames = 16;                           // frames of a k_mfcc_cepstra tile (fewer where n_mels is large)
constexpr int kMfccMaxMels = 4096;
constexpr double kMfccAmin = 1e-10, kMfccTopDb = 80.0;

enum { MFCC_ROUTE_AUTO = 0, MFCC_ROUTE_FFT = 1, MFCC_ROUTE_DIRECT = 2 };
enum { MFCC_I16 = 0, MFCC_F32 = 1, MFCC_F64 = 2 };

// The route a call takes (MFCC_ROUTE_FFT / MFCC_ROUTE_DIRECT), or 0 where the size fits neither or not the one asked for.
inline int mfcc_route(int64_t n_fft, int asked) {
    const bool fft = n_fft >= kMfccFftMin && n_fft <= kMfccFftMax && (n_fft & (n_fft - 1)) == 0;
    const bool direct = n_fft >= kMfccDirectMin && n_fft <= kMfccDirectMax && n_fft % 2 == 0;
    if (asked == MFCC_ROUTE_FFT) return fft ? MFCC_ROUTE_FFT : 0;
    if (asked == MFCC_ROUTE_DIRECT) return direct ? MFCC_ROUTE_DIRECT : 0;
    return fft ? MFCC_ROUTE_FFT : direct ? MFCC_ROUTE_DIRECT : 0;
}

// The doubles of dynamic LDS of a k_mfcc_mel launch.
inline size_t mfcc_mel_lds_doubles(int route, int64_t n_fft) {
    return (size_t)(route == MFCC_ROUTE_FFT ? 2 * n_fft : 3 * n_fft + n_fft / 2 + 1) + kMfccThreads;
}

struct MfccMel {
    const void *samples;
    const int64_t *sample_off;      // [U + 1]
    const int32_t *frame_off;       // [U + 1]
    const double *window;           // [n_fft]
    const double *mel;              // [n_mels, n_bins]
    const double *tab;              // [n_fft][2]: cos, sin of 2 pi j / n_fft
    const int32_t *span;            // [n_mels][2]
    double *S;                      // [T_total, n_mels]
    double *wgmax;                  // [T_total]
    int32_t U, n_fft, log2n, hop, n_bins, n_mels;
};

// The utterance of the global frame g: the last u with off[u] <= g (every utterance has a frame).
__device__ __forceinline__ int mfcc_utterance(const int32_t *off, int U, int g) {
    int lo = 0, hi = U;
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (off[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// Sample j of frame t of an utterance of L samples at y, times nothing: np.pad(y, n_fft / 2, 'reflect')[t * hop + j].
template <typename Sample>
__device__ __forceinline__ double mfcc_sample(const Sample *y, int64_t L, int64_t t, int hop, int half, int j) {
    int64_t q = t * hop + j - half;
    q = q < 0 ? -q : q;
    q = q >= L ? 2 * (L - 1) - q : q;
    return (double)y[q];
}

__global__ void __launch_bounds__(kMfccThreads) k_mfcc_rows(const double *mel, int n_mels, int n_bins, int32_t *span) {
    const int m = blockIdx.x * kMfccThreads + threadIdx.x;
    if (m >= n_mels) return;
    const double *row = mel + (int64_t)m * n_bins;
    int lo = n_bins, hi = 0;
    for (int b = 0; b < n_bins; ++b)
        if (row[b] != 0.0) {               // (a NaN weight counts: it stays in the sum)
            lo = b < lo ? b : lo;
            hi = b + 1;
        }
    span[2 * m] = lo < hi ? lo : 0;
    span[2 * m + 1] = hi;
}

// The energies of the workgroup's frame from its power spectrum P (LDS), and the frame's largest; red: kMfccThreads doubles.
__device__ __forceinline__ void mfcc_mel_rows(const MfccMel &a, int g, const double *P, double *red) {
    double top = 0.0;                      // (energies are sums of non-negative terms)
    for (int m = threadIdx.x; m < a.n_mels; m += kMfccThreads) {
        const double *row = a.mel + (int64_t)m * a.n_bins;
        const int lo = a.span[2 * m], hi = a.span[2 * m + 1];
        double acc = 0.0;
        for (int b = lo; b < hi; ++b) acc = acc + row[b] * P[b];
        a.S[(int64_t)g * a.n_mels + m] = acc;
        top = acc > top ? acc : top;
    }
    red[threadIdx.x] = top;
    __syncthreads();
    for (int w = kMfccThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            const double o = red[threadIdx.x + w];
            red[threadIdx.x] = o > red[threadIdx.x] ? o : red[threadIdx.x];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) a.wgmax[g] = red[0];
}

template <typename Sample, int kRoute>
__global__ void __launch_bounds__(kMfccThreads) k_mfcc_mel(const MfccMel a) {
    extern __shared__ double mfcc_lds[];
    const int g = blockIdx.x, n = a.n_fft, half = n / 2;
    const int u = mfcc_utterance(a.frame_off, a.U, g);
    const int64_t s0 = a.sample_off[u], L = a.sample_off[u + 1] - s0, t = g - a.frame_off[u];
    const Sample *y = (const Sample *)a.samples + s0;
    if (kRoute == MFCC_ROUTE_FFT) {
        double *re = mfcc_lds, *im = re + n, *red = im + n;
        const int p = a.log2n;
        for (int j = threadIdx.x; j < n; j += kMfccThreads) {
            const int r = (int)(__brev((unsigned)j) >> (32 - p));
            re[r] = mfcc_sample(y, L, t, a.hop, half, j) * a.window[j];
            im[j] = 0.0;                   // (all zeros: stored in lane order, the bit-reversed store puts a lane group on one bank)
        }
        __syncthreads();
        for (int s = 0; s < p; ++s) {
            const int h = 1 << s;
            for (int i = threadIdx.x; i < half; i += kMfccThreads) {
                const int k = i & (h - 1), j0 = ((i >> s) << (s + 1)) + k, j1 = j0 + h;
                const int e = k << (p - 1 - s);
                const double c = a.tab[2 * e], sn = a.tab[2 * e + 1];          // w = c - i sn
                const double xr = re[j1], xi = im[j1];
                const double tr = xr * c + xi * sn, ti = xi * c - xr * sn;
                const double ar = re[j0], ai = im[j0];
                re[j0] = ar + tr;
                im[j0] = ai + ti;
                re[j1] = ar - tr;
                im[j1] = ai - ti;
            }
            __syncthreads();
        }
        for (int b = threadIdx.x; b < a.n_bins; b += kMfccThreads) re[b] = re[b] * re[b] + im[b] * im[b];     // (bin b: this thread's alone)
        __syncthreads();
        mfcc_mel_rows(a, g, re, red);
    } else {
        double *x = mfcc_lds, *tc = x + n, *ts = tc + n, *P = ts + n, *red = P + a.n_bins;
        for (int j = threadIdx.x; j < n; j += kMfccThreads) {
            x[j] = mfcc_sample(y, L, t, a.hop, half, j) * a.window[j];
            tc[j] = a.tab[2 * j];
            ts[j] = a.tab[2 * j + 1];
        }
        __syncthreads();
        for (int b = threadIdx.x; b < a.n_bins; b += kMfccThreads) {
            double sr = 0.0, si = 0.0;
            int e = 0;
            for (int j = 0; j < n; ++j) {
                sr = sr + x[j] * tc[e];
                si = si + x[j] * ts[e];
                e += b;
                e = e >= n ? e - n : e;
            }
            P[b] = sr * sr + si * si;
        }
        __syncthreads();
        mfcc_mel_rows(a, g, P, red);
    }
}

__global__ void __launch_bounds__(kMfccThreads) k_mfcc_smax(const double *wgmax, const int32_t *frame_off, double *Smax) {
    __shared__ double red[kMfccThreads];
    const int u = blockIdx.x, f0 = frame_off[u], f1 = frame_off[u + 1];
    double top = 0.0;
    for (int f = f0 + threadIdx.x; f < f1; f += kMfccThreads) top = wgmax[f] > top ? wgmax[f] : top;
    red[threadIdx.x] = top;
    __syncthreads();
    for (int w = kMfccThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            const double o = red[threadIdx.x + w];
            red[threadIdx.x] = o > red[threadIdx.x] ? o : red[threadIdx.x];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) Smax[u] = red[0];
}

struct MfccCep {
    const double *S, *Smax, *dct;   // [T_total, n_mels], [U], [n_mfcc, n_mels]
    const double *dct_sums;         // [n_mfcc]: the exact sums of the basis' rows
    const int32_t *frame_off;       // [U + 1]
    double *cep;                    // [T_total, n_mfcc]: what k_mfcc_delta reads
    int32_t U, T, n_mels, n_mfcc, frames;          // frames: of a tile
    int64_t ld;                     // of the three output streams
};

// The tile's frames g0 .. g0 + frames: Ldb - top into LDS (rows n_mels + 1 doubles apart), then a thread per (frame, coefficient).
template <typename T>
__global__ void __launch_bounds__(kMfccThreads) k_mfcc_cepstra(const MfccCep a, T *out) {
    extern __shared__ double mfcc_lds[];
    const int g0 = blockIdx.x * a.frames, nf = min(a.frames, a.T - g0), ldl = a.n_mels + 1;
    double *top_db = mfcc_lds, *ldb = mfcc_lds + kMfccCepFrames;
    if ((int)threadIdx.x < nf) {
        const double top = a.Smax[mfcc_utterance(a.frame_off, a.U, g0 + threadIdx.x)];
        top_db[threadIdx.x] = 10.0 * log10(top > kMfccAmin ? top : kMfccAmin);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nf * a.n_mels; e += kMfccThreads) {
        const int f = e / a.n_mels, m = e - f * a.n_mels;
        const double s = a.S[(int64_t)g0 * a.n_mels + e];
        const double db = 10.0 * log10(s > kMfccAmin ? s : kMfccAmin);
        const double floor_db = top_db[f] - kMfccTopDb;
        ldb[f * ldl + m] = (db > floor_db ? db : floor_db) - top_db[f];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nf * a.n_mfcc; e += kMfccThreads) {
        const int f = e / a.n_mfcc, i = e - f * a.n_mfcc;
        const double *row = a.dct + (int64_t)i * a.n_mels, *l = ldb + f * ldl;
        double acc = 0.0;
        for (int m = 0; m < a.n_mels; ++m) acc = acc + row[m] * l[m];
        acc = acc + top_db[f] * a.dct_sums[i];
        a.cep[(int64_t)(g0 + f) * a.n_mfcc + i] = acc;
        out[(int64_t)(g0 + f) * a.ld + i] = (T)acc;
    }
}

// y1[k] of the utterance's padded axis k in [0, n + 10): lfilter([4, 3, .., -4], 1, .) from a zero state on
// xp[k] = x[clamp(k - 5, 0, n - 1)] -- b0 xp[k] + (b1 xp[k-1] + (... + (b7 xp[k-7] + b8 xp[k-8]))), the sum built from the oldest
// sample on, as the transposed direct form carries it; a sample before the axis is a zero.
__device__ __forceinline__ double mfcc_lfilter1(const double *x, int64_t stride, int n, int k) {
    double acc = 0.0;
    for (int r = 8; r >= 0; --r) {
        const int kk = k - r;
        if (kk < 0) continue;
        int src = kk - 5;
        src = src < 0 ? 0 : src > n - 1 ? n - 1 : src;
        acc = (double)(4 - r) * x[(int64_t)src * stride] + acc;
    }
    return acc;
}

template <typename T>
__global__ void __launch_bounds__(kMfccThreads) k_mfcc_delta(const MfccCep a, T *d1, T *d2) {
    const int64_t e = (int64_t)blockIdx.x * kMfccThreads + threadIdx.x;
    if (e >= (int64_t)a.T * a.n_mfcc) return;
    const int g = (int)(e / a.n_mfcc), i = (int)(e - (int64_t)g * a.n_mfcc);
    const int u = mfcc_utterance(a.frame_off, a.U, g), f0 = a.frame_off[u], n = a.frame_off[u + 1] - f0, t = g - f0;
    const double *x = a.cep + (int64_t)f0 * a.n_mfcc + i;
    d1[(int64_t)g * a.ld + i] = (T)mfcc_lfilter1(x, a.n_mfcc, n, t + 5);
    double acc = 0.0;                      // the filter once more on y1, unpadded: y2[t + 5]
    for (int r = 8; r >= 0; --r) {
        const int kk = t + 5 - r;
        if (kk < 0) continue;
        acc = (double)(4 - r) * mfcc_lfilter1(x, a.n_mfcc, n, kk) + acc;
    }
    d2[(int64_t)g * a.ld + i] = (T)acc;
}

}  // namespace klnmf
