// libklnmf.so, the feature unit: the MFCC front end of include/features/klnmf_mfcc.h -- argument checks, the workspace layout, the
// table of twiddles, the launches of mfcc.hip.h (included by this unit alone) and the host-array wrapper (ctx.hip.h lists the
// units).
#include "ctx.hip.h"
#include "feature_host.hip.h"
#include "../../include/features/klnmf_mfcc.h"
#include "mfcc.hip.h"

#include <cmath>

static_assert(MFCC_I16 == KLNMF_MFCC_I16 && MFCC_F32 == KLNMF_MFCC_F32 && MFCC_F64 == KLNMF_MFCC_F64, "the header's sample kinds");
static_assert(MFCC_ROUTE_AUTO == KLNMF_MFCC_ROUTE_AUTO && MFCC_ROUTE_FFT == KLNMF_MFCC_ROUTE_FFT
              && MFCC_ROUTE_DIRECT == KLNMF_MFCC_ROUTE_DIRECT && kMfccMaxMels == KLNMF_MFCC_MAX_MELS, "the header's route rule");

namespace klnmf_host {
namespace {

// The caller's workspace, as byte offsets.  The mel call: the sample offsets (at 0), the frame offsets, the twiddles, the filters'
// spans, the frames' maxima.  The cepstra call, laid over it: the frame offsets (at 0), the fp64 cepstra.
struct MfccLayout {
    size_t frame_off, tab, span, wgmax, cep, total;
    MfccLayout(int64_t U, int64_t T, int64_t n_fft, int64_t n_mels, int64_t n_mfcc) {
        WorkLayout mel, cepstra;
        mel.take((size_t)(U + 1) * sizeof(int64_t));
        frame_off = mel.take((size_t)(U + 1) * sizeof(int32_t));
        tab = mel.take((size_t)n_fft * 2 * sizeof(double));
        span = mel.take((size_t)n_mels * 2 * sizeof(int32_t));
        wgmax = mel.take((size_t)T * sizeof(double));
        cepstra.take((size_t)(U + 1) * sizeof(int32_t));
        cep = cepstra.take((size_t)T * (size_t)n_mfcc * sizeof(double));
        WorkLayout both;
        both.overlay({mel, cepstra});
        total = both.end;
    }
};

void mfcc_check_sizes(const Who &w, int64_t U, int64_t samples, int64_t T, int64_t n_fft, int64_t n_mels, int64_t n_mfcc) {
    if (U < 0 || samples < 0 || T < 0 || n_mels < 0 || n_mfcc < 0) w.bad("a negative count");
    if (n_fft < 1) w.bad("n_fft below 1");
    if (U >= kMaxInt || samples >= kMaxInt || T >= kMaxInt || n_fft >= kMaxInt || n_mels >= kMaxInt || n_mfcc >= kMaxInt)
        w.bad("a count not below 2^31 - 1");
    if (T * std::max<int64_t>(n_mels, 1) >= kMaxInt || T * std::max<int64_t>(n_mfcc, 1) >= kMaxInt)
        w.bad("total_frames * n_mels or total_frames * n_mfcc not below 2^31 - 1");
}

// The route of a mel call and its frame offsets, from host arithmetic alone; fail() on the first bad argument.
int mfcc_mel_check(const Who &w, int kind, const int64_t *off, int64_t U, int64_t n_fft, int64_t hop, int route, int64_t n_mels,
                   int64_t total_frames, std::vector<int32_t> *frame_off) {
    if (kind != KLNMF_MFCC_I16 && kind != KLNMF_MFCC_F32 && kind != KLNMF_MFCC_F64)
        w.bad("sample_kind must be KLNMF_MFCC_I16, KLNMF_MFCC_F32 or KLNMF_MFCC_F64");
    if (route != KLNMF_MFCC_ROUTE_AUTO && route != KLNMF_MFCC_ROUTE_FFT && route != KLNMF_MFCC_ROUTE_DIRECT)
        w.bad("route must be KLNMF_MFCC_ROUTE_AUTO, _FFT or _DIRECT");
    if (U < 0 || U >= kMaxInt) w.bad("n_utterances negative or not below 2^31 - 1");
    if (hop < 1 || hop >= kMaxInt) w.bad("hop below 1 (or not below 2^31 - 1)");
    if (n_mels < 1) w.bad("n_mels below 1");
    if (n_fft < 2 || n_fft >= kMaxInt) w.bad("n_fft below 2 (or not below 2^31 - 1)");
    if (!off) w.bad("null sample offsets");
    if (off[0] != 0) w.bad("sample offsets that do not start at 0");
    frame_off->assign((size_t)U + 1, 0);
    int64_t frames = 0;
    for (int64_t u = 0; u < U; ++u) {
        const int64_t L = off[u + 1] - off[u];
        if (L < 0) w.bad("sample offsets that do not ascend (utterance " + std::to_string(u) + ")");
        if (L < n_fft / 2 + 1)
            w.bad("utterance " + std::to_string(u) + " has " + std::to_string(L) + " samples: below the n_fft / 2 + 1 = "
                  + std::to_string(n_fft / 2 + 1) + " its reflection needs");
        if (off[u + 1] >= kMaxInt) w.bad("total samples not below 2^31 - 1");
        frames += 1 + L / hop;
        if (frames >= kMaxInt) w.bad("total frames not below 2^31 - 1");
        (*frame_off)[(size_t)u + 1] = (int32_t)frames;
    }
    if (frames != total_frames)
        w.bad("total_frames " + std::to_string(total_frames) + " is not the " + std::to_string(frames) + " of 1 + L / hop per utterance");
    if (frames * n_mels >= kMaxInt) w.bad("total_frames * n_mels not below 2^31 - 1");
    const int taken = mfcc_route(n_fft, route);
    if (!taken)
        w.unsupp("n_fft " + std::to_string(n_fft) + " fits " + (route == KLNMF_MFCC_ROUTE_AUTO ? "neither route" : "not the route asked for")
                 + ": fft takes the powers of two in [64, 4096], direct the even sizes in [16, 1024]");
    if (n_mels > KLNMF_MFCC_MAX_MELS) w.unsupp("n_mels above " + std::to_string(KLNMF_MFCC_MAX_MELS));
    return taken;
}

template <typename Sample>
void mfcc_launch_mel(int route, const MfccMel &a, int64_t frames) {
    const size_t lds = mfcc_mel_lds_doubles(route, a.n_fft) * sizeof(double);
    if (route == MFCC_ROUTE_FFT) {
        if (lds > 64 * 1024)            // (4096 points: beyond the default dynamic LDS of a launch)
            HIPCHK(hipFuncSetAttribute((const void *)k_mfcc_mel<Sample, MFCC_ROUTE_FFT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_mfcc_mel<Sample, MFCC_ROUTE_FFT>), dim3((unsigned)frames), dim3(kMfccThreads), lds, 0, a);
    } else {
        hipLaunchKernelGGL((k_mfcc_mel<Sample, MFCC_ROUTE_DIRECT>), dim3((unsigned)frames), dim3(kMfccThreads), lds, 0, a);
    }
}

void mfcc_mel(const Who &w, int device, int kind, const void *d_samples, const int64_t *off, int64_t U, int64_t n_fft, int64_t hop,
              int route, const double *d_window, const double *d_mel, int64_t n_mels, int64_t total_frames, void *d_work,
              uint64_t work_bytes, double *d_S, double *d_Smax) {
    std::vector<int32_t> frame_off;
    const int taken = mfcc_mel_check(w, kind, off, U, n_fft, hop, route, n_mels, total_frames, &frame_off);
    if (U == 0) return;
    if (!d_samples || !d_window || !d_mel || !d_work || !d_S || !d_Smax) w.bad("null samples, window, filter bank, workspace, S or Smax");
    const MfccLayout at(U, total_frames, n_fft, n_mels, 0);
    w.workspace(work_bytes, at.total, "klnmf_mfcc_work_bytes");
    // cos, sin(2 pi j / n_fft), each the nearest double of the extended-precision value
    std::vector<double> tab((size_t)n_fft * 2);
    const long double step = 2.0L * 3.14159265358979323846264338327950288L / (long double)n_fft;
    for (int64_t j = 0; j < n_fft; ++j) {
        tab[(size_t)2 * j] = (double)cosl(step * (long double)j);
        tab[(size_t)2 * j + 1] = (double)sinl(step * (long double)j);
    }
    HIPCHK(hipSetDevice(device));
    unsigned char *work = (unsigned char *)d_work;
    MfccMel a{};
    a.samples = d_samples;
    a.sample_off = (const int64_t *)work;
    a.frame_off = (const int32_t *)(work + at.frame_off);
    a.window = d_window;
    a.mel = d_mel;
    a.tab = (const double *)(work + at.tab);
    a.span = (const int32_t *)(work + at.span);
    a.S = d_S;
    a.wgmax = (double *)(work + at.wgmax);
    a.U = (int32_t)U;
    a.n_fft = (int32_t)n_fft;
    a.hop = (int32_t)hop;
    a.n_bins = (int32_t)(n_fft / 2 + 1);
    a.n_mels = (int32_t)n_mels;
    for (a.log2n = 0; ((int64_t)1 << a.log2n) < n_fft; ++a.log2n) {}
    HIPCHK(hipMemcpy(work, off, (size_t)(U + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(work + at.frame_off, frame_off.data(), frame_off.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(work + at.tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_mfcc_rows, dim3((unsigned)((n_mels + kMfccThreads - 1) / kMfccThreads)), dim3(kMfccThreads), 0, 0, d_mel,
                       a.n_mels, a.n_bins, (int32_t *)(work + at.span));
    if (kind == KLNMF_MFCC_I16) mfcc_launch_mel<int16_t>(taken, a, total_frames);
    else if (kind == KLNMF_MFCC_F32) mfcc_launch_mel<float>(taken, a, total_frames);
    else mfcc_launch_mel<double>(taken, a, total_frames);
    hipLaunchKernelGGL(k_mfcc_smax, dim3((unsigned)U), dim3(kMfccThreads), 0, 0, a.wgmax, a.frame_off, d_Smax);
    HIPCHK(hipGetLastError());
}

void mfcc_cepstra_check(const Who &w, int dtype, int64_t n_mels, int64_t n_mfcc, const int64_t *frame_off, int64_t U, int64_t ld) {
    w.dtype(dtype);
    if (U < 0 || U >= kMaxInt) w.bad("n_utterances negative or not below 2^31 - 1");
    if (n_mels < 1 || n_mfcc < 1) w.bad("n_mels or n_mfcc below 1");
    if (n_mfcc > n_mels) w.bad("n_mfcc above n_mels");
    if (ld < n_mfcc) w.bad("a stride below n_mfcc");
    if (!frame_off) w.bad("null frame offsets");
    if (frame_off[0] != 0) w.bad("frame offsets that do not start at 0");
    for (int64_t u = 0; u < U; ++u) {
        if (frame_off[u + 1] <= frame_off[u]) w.bad("frame offsets that do not ascend strictly (utterance " + std::to_string(u) + ")");
        if (frame_off[u + 1] >= kMaxInt) w.bad("total frames not below 2^31 - 1");
    }
    if (frame_off[U] * n_mels >= kMaxInt) w.bad("total_frames * n_mels not below 2^31 - 1");
    if (n_mels > KLNMF_MFCC_MAX_MELS) w.unsupp("n_mels above " + std::to_string(KLNMF_MFCC_MAX_MELS));
}

void mfcc_cepstra(const Who &w, int device, int dtype, const double *d_S, const double *d_Smax, const double *d_dct,
                  const double *d_dct_sums, int64_t n_mels,
                  int64_t n_mfcc, const int64_t *frame_off, int64_t U, void *d_work, uint64_t work_bytes, void *d_mfcc,
                  void *d_delta1, void *d_delta2, int64_t ld) {
    mfcc_cepstra_check(w, dtype, n_mels, n_mfcc, frame_off, U, ld);
    if (U == 0) return;
    if (!d_S || !d_Smax || !d_dct || !d_dct_sums || !d_work || !d_mfcc || !d_delta1 || !d_delta2)
        w.bad("null S, Smax, DCT basis, row sums, workspace or stream");
    const int64_t T = frame_off[U];
    const MfccLayout at(U, T, 1, n_mels, n_mfcc);
    w.workspace(work_bytes, MfccLayout(U, T, 1, 0, n_mfcc).total, "klnmf_mfcc_work_bytes");
    std::vector<int32_t> off32((size_t)U + 1);
    for (size_t u = 0; u < off32.size(); ++u) off32[u] = (int32_t)frame_off[u];
    HIPCHK(hipSetDevice(device));
    unsigned char *work = (unsigned char *)d_work;
    HIPCHK(hipMemcpy(work, off32.data(), off32.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    MfccCep a{};
    a.S = d_S;
    a.Smax = d_Smax;
    a.dct = d_dct;
    a.dct_sums = d_dct_sums;
    a.frame_off = (const int32_t *)work;
    a.cep = (double *)(work + at.cep);
    a.U = (int32_t)U;
    a.T = (int32_t)T;
    a.n_mels = (int32_t)n_mels;
    a.n_mfcc = (int32_t)n_mfcc;
    a.frames = (int32_t)std::max<int64_t>(1, std::min<int64_t>(kMfccCepFrames, (48 * 1024 / 8) / (n_mels + 1)));
    a.ld = ld;
    const size_t lds = sizeof(double) * (size_t)(kMfccCepFrames + a.frames * (n_mels + 1));
    const int64_t tiles = (T + a.frames - 1) / a.frames, cells = (T * n_mfcc + kMfccThreads - 1) / kMfccThreads;
    by_dtype(dtype, [&](auto tag) {
        using V = tag_t<decltype(tag)>;
        hipLaunchKernelGGL((k_mfcc_cepstra<V>), dim3((unsigned)tiles), dim3(kMfccThreads), lds, 0, a, (V *)d_mfcc);
        hipLaunchKernelGGL((k_mfcc_delta<V>), dim3((unsigned)cells), dim3(kMfccThreads), 0, 0, a, (V *)d_delta1, (V *)d_delta2);
    });
    HIPCHK(hipGetLastError());
}

}  // namespace
}  // namespace klnmf_host

extern "C" {

int klnmf_mfcc_work_bytes(int64_t n_utterances, int64_t total_samples, int64_t total_frames, int64_t n_fft, int64_t n_mels,
                          int64_t n_mfcc, uint64_t *bytes) {
    return guarded([&] {
        const Who w{"klnmf_mfcc_work_bytes"};
        if (!bytes) w.bad("null bytes");
        mfcc_check_sizes(w, n_utterances, total_samples, total_frames, n_fft, n_mels, n_mfcc);
        *bytes = (uint64_t)MfccLayout(n_utterances, total_frames, n_fft, n_mels, n_mfcc).total;
    });
}

int klnmf_mfcc_mel_device(int device, int sample_kind, const void *d_samples, const int64_t *sample_offsets, int64_t n_utterances,
                          int64_t n_fft, int64_t hop, int route, const double *d_window, const double *d_mel, int64_t n_mels,
                          int64_t total_frames, void *d_work, uint64_t work_bytes, double *d_S, double *d_Smax) {
    return guarded([&] {
        mfcc_mel(Who{"klnmf_mfcc_mel_device"}, device, sample_kind, d_samples, sample_offsets, n_utterances, n_fft, hop, route, d_window,
                 d_mel, n_mels, total_frames, d_work, work_bytes, d_S, d_Smax);
    });
}

int klnmf_mfcc_cepstra_device(int device, int dtype, const double *d_S, const double *d_Smax, const double *d_dct,
                              const double *d_dct_sums, int64_t n_mels, int64_t n_mfcc, const int64_t *frame_offsets, int64_t n_utterances, void *d_work,
                              uint64_t work_bytes, void *d_mfcc, void *d_delta1, void *d_delta2, int64_t ld) {
    return guarded([&] {
        mfcc_cepstra(Who{"klnmf_mfcc_cepstra_device"}, device, dtype, d_S, d_Smax, d_dct, d_dct_sums, n_mels, n_mfcc, frame_offsets, n_utterances,
                     d_work, work_bytes, d_mfcc, d_delta1, d_delta2, ld);
    });
}

int klnmf_mfcc(int device, int sample_kind, int dtype, const void *samples, const int64_t *sample_offsets, int64_t n_utterances,
               int64_t n_fft, int64_t hop, int route, const double *window, const double *mel, int64_t n_mels, const double *dct,
               const double *dct_sums, int64_t n_mfcc, int64_t total_frames, void *mfcc, void *delta1, void *delta2, int64_t ld) {
    return guarded([&] {
        const Who w{"klnmf_mfcc"};
        const int64_t U = n_utterances;
        std::vector<int32_t> frame_off;
        (void)mfcc_mel_check(w, sample_kind, sample_offsets, U, n_fft, hop, route, n_mels, total_frames, &frame_off);
        std::vector<int64_t> frames64(frame_off.begin(), frame_off.end());
        mfcc_cepstra_check(w, dtype, n_mels, n_mfcc, frames64.data(), U, ld);
        if (U == 0) return;
        if (!samples || !window || !mel || !dct || !dct_sums || !mfcc || !delta1 || !delta2) w.bad("null samples, tables or streams");
        const int64_t n_samples = sample_offsets[U], T = total_frames, n_bins = n_fft / 2 + 1;
        const size_t sample_bytes = sample_kind == KLNMF_MFCC_I16 ? 2 : sample_kind == KLNMF_MFCC_F32 ? 4 : 8, el = dtype_bytes(dtype);
        HIPCHK(hipSetDevice(device));
        const MfccLayout at(U, T, n_fft, n_mels, n_mfcc);
        DeviceScratch mem;
        void *d_samples = mem.take(sample_bytes * (size_t)n_samples);
        double *d_window = (double *)mem.take(sizeof(double) * (size_t)n_fft);
        double *d_mel = (double *)mem.take(sizeof(double) * (size_t)n_mels * n_bins);
        double *d_dct = (double *)mem.take(sizeof(double) * (size_t)n_mfcc * n_mels);
        double *d_dct_sums = (double *)mem.take(sizeof(double) * (size_t)n_mfcc);
        double *d_S = (double *)mem.take(sizeof(double) * (size_t)T * n_mels), *d_Smax = (double *)mem.take(sizeof(double) * (size_t)U);
        void *work = mem.take(at.total);
        unsigned char *d_out = (unsigned char *)mem.take(3 * el * (size_t)T * n_mfcc);
        HIPCHK(hipMemcpy(d_samples, samples, sample_bytes * (size_t)n_samples, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_window, window, sizeof(double) * (size_t)n_fft, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_mel, mel, sizeof(double) * (size_t)n_mels * n_bins, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_dct, dct, sizeof(double) * (size_t)n_mfcc * n_mels, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_dct_sums, dct_sums, sizeof(double) * (size_t)n_mfcc, hipMemcpyHostToDevice));
        mfcc_mel(w, device, sample_kind, d_samples, sample_offsets, U, n_fft, hop, route, d_window, d_mel, n_mels, T, work, at.total, d_S,
                 d_Smax);
        const size_t stream_bytes = el * (size_t)T * n_mfcc;
        mfcc_cepstra(w, device, dtype, d_S, d_Smax, d_dct, d_dct_sums, n_mels, n_mfcc, frames64.data(), U, work, at.total, d_out,
                     d_out + stream_bytes, d_out + 2 * stream_bytes, n_mfcc);
        void *outs[3] = {mfcc, delta1, delta2};
        for (int s = 0; s < 3; ++s)
            HIPCHK(hipMemcpy2D(outs[s], el * (size_t)ld, d_out + s * stream_bytes, el * (size_t)n_mfcc, el * (size_t)n_mfcc, (size_t)T,
                               hipMemcpyDeviceToHost));
    });
}

}  // extern "C"
