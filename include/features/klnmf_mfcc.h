/* klnmf_mfcc.h -- C-ABI of the MFCC front end of the sound modality: the samples of many utterances to mel energies, cepstra
 * and the two delta streams, on the device in a fixed number of launches -- the three frame streams that klnmf_hac.h quantises.
 *
 * An interface of its own beside klnmf.h (whose conventions, error codes and dtype numbers it uses): int status returns,
 * klnmf_last_error(), every entry point naming the reference lines it stands in for.  The same library, libklnmf.so, exports the
 * symbols of every header.  (It lies in include/features/: the headers directly under include/ are a closed registry.)
 *
 * THE RULES, per utterance y of L samples (n_fft, hop, n_mels, n_mfcc).  They restate the conventions of the 0.4 series of the
 * audio library the reference imports (`logamplitude`, `melspectrogram`, `delta`, `filters.dct`); they are UNPINNED against that
 * library, which was not at hand.  The window, the filter bank and the DCT basis are the caller's tables: a rule that turns out
 * to differ changes a host table, not a kernel.
 *   1. Frames.  yp = np.pad(y, n_fft / 2, 'reflect'); T = 1 + L / hop frames; frame t = yp[t hop : t hop + n_fft] * window.
 *      L >= n_fft / 2 + 1.  Samples are int16, f32 or f64, promoted exactly to fp64, not scaled.
 *   2. Power.  P[b] = |rfft(frame)[b]|^2, b = 0 .. n_fft / 2.
 *   3. Mel.  S = M . P, M [n_mels, n_fft / 2 + 1] any non-negative matrix, bins ascending.
 *   4. Log.  Ldb = 10 log10(max(S, 1e-10)), then max(Ldb, Ldb.max() - 80), the maximum over the utterance's n_mels x T array
 *      (= 10 log10(max(Smax, 1e-10)), log10 being monotone).
 *   5. DCT.  mfcc = D . Ldb, D [n_mfcc, n_mels], evaluated centred on the utterance's top level Lmax = Ldb.max():
 *      sum_m D[i, m] (Ldb[m] - Lmax), m ascending, plus Lmax * r[i], r the EXACT row sums of the basis (sqrt(n_mels), 0, 0, ..
 *      for the DCT), a host table like D.  The summands are the levels below the top (0 to -80 dB), so the sum's rounding does
 *      not grow with the signal's scale, and a flat spectrum -- silence: every Ldb = -100 -- gives Lmax * r[i] exactly.
 *   6. Deltas.  The time axis edge-padded by 5 frames, scipy.signal.lfilter([4, 3, .., -4], 1, .) from a zero state applied once
 *      (delta 1) or twice without padding again (delta 2), then [5 : -5]; each output is
 *      b0 x[k] + (b1 x[k-1] + (... + b8 x[k-8])), the sum built from the oldest sample on.
 * All arithmetic is fp64, every product and sum rounded on its own (the audio library's spectra are complex64: fp32 grade);
 * no floating-point atomics; every sum in an order fixed by the sizes alone.  An utterance alone and the same utterance inside a
 * batch give the same bits.
 *
 * Routes of the transform.  fft: n_fft a power of two in [64, 4096], radix 2 in LDS.  direct: any even n_fft in [16, 1024],
 * bin b = sum_j frame[j] * tab[(j b) mod n_fft], j ascending.  Both read one table of cos, sin(2 pi j / n_fft) that the host
 * half computes and keeps in the workspace.  KLNMF_MFCC_ROUTE_AUTO: fft where it applies, else direct.  A size that fits
 * neither (or not the route asked for; an odd n_fft, whose last frame rule 1 would read past the padding) is refused with
 * KLNMF_ERR_UNSUPP before anything is launched, as is n_mels > KLNMF_MFCC_MAX_MELS.
 * Limits: utterances, total samples, total frames, total_frames * n_mels < 2^31 - 1. */
#ifndef KLNMF_MFCC_H
#define KLNMF_MFCC_H

#include "../klnmf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KLNMF_MFCC_I16 0
#define KLNMF_MFCC_F32 1
#define KLNMF_MFCC_F64 2
#define KLNMF_MFCC_ROUTE_AUTO 0
#define KLNMF_MFCC_ROUTE_FFT 1
#define KLNMF_MFCC_ROUTE_DIRECT 2
#define KLNMF_MFCC_MAX_MELS 4096

/* The bytes of device workspace the two device calls below need on these sizes (the larger of the two): the sample and frame
 * offsets, the table of n_fft twiddles, the filters' spans, a maximum per frame; the frame offsets and the fp64 cepstra
 * [total_frames, n_mfcc].  Host arithmetic only.
 * KLNMF_ERR_ARG: a null `bytes`, a negative count, a count not below 2^31 - 1, n_fft < 1.
 * Stands in for nothing of the reference: features/hac.py:44-65 allocates an array per stage. */
int klnmf_mfcc_work_bytes(int64_t n_utterances, int64_t total_samples, int64_t total_frames, int64_t n_fft, int64_t n_mels,
                          int64_t n_mfcc, uint64_t *bytes);

/* Rules 1 to 3 and the utterances' maxima, on `device`'s null stream.  d_samples: DEVICE, the utterances' samples one after the
 * other, of `sample_kind`; sample_offsets: HOST int64 [n_utterances + 1], utterance u is [offsets[u], offsets[u + 1]);
 * d_window: DEVICE fp64 [n_fft]; d_mel: DEVICE fp64 [n_mels, n_fft / 2 + 1], contiguous; total_frames: the sum over the
 * utterances of 1 + L / hop, which the call checks.  d_S: DEVICE fp64 [total_frames, n_mels], the utterances' frames one after
 * the other; d_Smax: DEVICE fp64 [n_utterances].  Three launches behind three small uploads (the offsets, the table), whatever
 * n_utterances is; no allocation, no synchronisation.  n_utterances = 0: KLNMF_OK, nothing done.
 * KLNMF_ERR_ARG, nothing launched and nothing written: a null pointer where data is needed, a bad sample_kind or route,
 * offsets that do not start at 0 or do not ascend, an utterance shorter than n_fft / 2 + 1, hop < 1, n_mels < 1, n_fft < 2,
 * a total_frames other than rule 1's, totals not below 2^31 - 1, a workspace below klnmf_mfcc_work_bytes.
 * KLNMF_ERR_UNSUPP, nothing launched and nothing written: the route rule above.
 * Replaces `melspectrogram(y=data, sr=sr, **kwargs)` inside `mfcc` (features/hac.py:64) for all the files of
 * `build_codebooks_from_list_of_wav` (features/hac.py:127-131) at once. */
int klnmf_mfcc_mel_device(int device, int sample_kind, const void *d_samples, const int64_t *sample_offsets, int64_t n_utterances,
                          int64_t n_fft, int64_t hop, int route, const double *d_window, const double *d_mel, int64_t n_mels,
                          int64_t total_frames, void *d_work, uint64_t work_bytes, double *d_S, double *d_Smax);

/* Rules 4 to 6.  d_S, d_Smax: what klnmf_mfcc_mel_device wrote; d_dct: DEVICE fp64 [n_mfcc, n_mels], contiguous; d_dct_sums:
 * DEVICE fp64 [n_mfcc], the exact row sums of the basis;
 * frame_offsets: HOST int64 [n_utterances + 1], every utterance with a frame at least.  d_mfcc, d_delta1, d_delta2: DEVICE
 * `dtype` [total_frames, n_mfcc], rows ld elements apart (an f32 value is the fp64 one rounded once; the deltas are taken from
 * the fp64 cepstra).  Two launches behind one upload; no allocation, no synchronisation.  n_utterances = 0: KLNMF_OK.
 * KLNMF_ERR_ARG, nothing launched and nothing written: a null pointer, a bad dtype, n_mels < 1, n_mfcc < 1, n_mfcc > n_mels,
 * ld < n_mfcc, frame offsets that do not start at 0 or do not ascend strictly, totals not below 2^31 - 1, a workspace below
 * klnmf_mfcc_work_bytes.  KLNMF_ERR_UNSUPP: n_mels > KLNMF_MFCC_MAX_MELS.
 * Replaces `logamplitude(.)` and `np.dot(dct(n_mfcc, S.shape[0]), S)` of `mfcc` (features/hac.py:64-65) and the two `delta`
 * calls of `hac` and of `build_codebooks_from_list_of_wav` (features/hac.py:191-192, 140-145). */
int klnmf_mfcc_cepstra_device(int device, int dtype, const double *d_S, const double *d_Smax, const double *d_dct,
                              const double *d_dct_sums, int64_t n_mels, int64_t n_mfcc, const int64_t *frame_offsets, int64_t n_utterances, void *d_work,
                              uint64_t work_bytes, void *d_mfcc, void *d_delta1, void *d_delta2, int64_t ld);

/* Both calls from HOST arrays: samples, window [n_fft], mel [n_mels, n_fft / 2 + 1], dct [n_mfcc, n_mels], dct_sums [n_mfcc] and the three
 * streams `dtype` [total_frames, n_mfcc] with rows ld apart are host memory.  Allocates, uploads, runs, downloads.
 * Refusals as above, nothing written.
 * Replaces `mfcc` and the deltas (features/hac.py:44-65, 190-193) for callers without device tensors. */
int klnmf_mfcc(int device, int sample_kind, int dtype, const void *samples, const int64_t *sample_offsets, int64_t n_utterances,
               int64_t n_fft, int64_t hop, int route, const double *window, const double *mel, int64_t n_mels, const double *dct,
               const double *dct_sums, int64_t n_mfcc, int64_t total_frames, void *mfcc, void *delta1, void *delta2, int64_t ld);

#ifdef __cplusplus
}
#endif
#endif /* KLNMF_MFCC_H */
