# encoding: utf-8
"""The MFCC front end of the sound modality: audio samples to cepstra and their two delta streams (reference
multimodal/features/hac.py:44-65 and the `delta` calls of :140-145, :191-192).

The reference takes `logamplitude`, `melspectrogram`, `delta` and `filters.dct` from an audio library.  Here the front end is
DEFINED by the rules below -- that library's 0.4-series conventions restated; they are unpinned against the library itself, which
was not at hand when this was written.  Per utterance y of L samples:

1. frames: yp = np.pad(y, n_fft // 2, mode='reflect'), T = 1 + L // hop_length frames, frame t = yp[t hop : t hop + n_fft] times
   scipy's periodic Hann window; L >= n_fft // 2 + 1; samples (int16, float32, float64) enter unscaled;
2. power: |rfft(frame)|^2;
3. mel: S = M . P with the Slaney filter bank M (`mel_filters`);
4. log: 10 log10(max(S, 1e-10)), floored at the utterance's maximum minus 80 dB;
5. DCT: the first n_mfcc rows of the orthonormal DCT-II (`dct_basis`); the device evaluates D . Ldb centred on the utterance's
   top level, sum_m D[i, m] (Ldb[m] - Lmax) + Lmax r[i] with the basis' exact row sums r (`dct_row_sums`): the same value, with
   a rounding that does not grow with the signal's scale, and exact on a flat spectrum (silence);
6. deltas: edge-pad 5 frames, lfilter([4 .. -4], 1, .) once or twice, keep [5:-5] (`host_delta`).

* the host twin in numpy / scipy calls only -- `host_mel_energies`, `host_mfcc`, `host_delta`, `host_mfcc_streams`;
* `mfcc_streams`, the device path: every utterance of a corpus in five launches (klnmf_mfcc_mel_device /
  klnmf_mfcc_cepstra_device, csrc/mfcc.hip.h), the three streams left in device memory with the utterances' frame spans -- the
  `streams` and `windows` of `features.hac.windowed_hac`, the `streams` of `features.codebook.build_codebooks`.

All arithmetic is float64 in both (the audio library's spectra are complex64, float32 grade).  The window, the filter bank and
the DCT basis are host tables the device only consumes: a rule that turns out to differ from the library's changes a few lines
here.
"""
import numpy as np
import scipy.signal

from .. import _native
from .hac import _is_tensor, _torch_device

AMIN, TOP_DB = 1e-10, 80.0
DELTA_TAPS = np.arange(4, -5, -1)
DEFAULTS = dict(n_mfcc=13, n_fft=2048, hop_length=512, n_mels=128, fmin=0.0, fmax=None)      # the reference's, completed


# ---- the tables ---------------------------------------------------------------------------------------------------------------------
def hz_to_mel(f):
    """Slaney's mel scale: 200 / 3 Hz per mel below 1000 Hz, log(6.4) / 27 per mel in log-frequency above."""
    f = np.asarray(f, dtype=np.float64)
    lin = f / (200.0 / 3)
    with np.errstate(divide='ignore', invalid='ignore'):
        log = 1000.0 / (200.0 / 3) + np.log(np.maximum(f, 1000.0) / 1000.0) / (np.log(6.4) / 27.0)
    return np.where(f >= 1000.0, log, lin)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    min_log_mel = 1000.0 / (200.0 / 3)
    return np.where(m >= min_log_mel, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - min_log_mel)), (200.0 / 3) * m)


def mel_band_edges(n_mels, fmin, fmax):
    """The n_mels + 2 band edges in Hz, equally spaced in mel between fmin and fmax."""
    return mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), int(n_mels) + 2))


def mel_triangles(freqs, edges):
    """[n_mels, len(freqs)]: filter i is the triangle max(0, min(lower, upper)) over the edges i, i + 1, i + 2, scaled by
    2 / (edges[i + 2] - edges[i]) -- area 1 over frequency."""
    freqs, edges = np.asarray(freqs, dtype=np.float64), np.asarray(edges, dtype=np.float64)
    n_mels = len(edges) - 2
    W = np.zeros((n_mels, len(freqs)), dtype=np.float64)
    for i in range(n_mels):
        lower = (freqs - edges[i]) / (edges[i + 1] - edges[i])
        upper = (edges[i + 2] - freqs) / (edges[i + 2] - edges[i + 1])
        W[i] = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (edges[i + 2] - edges[i]))
    return W


def mel_filters(sr, n_fft, n_mels=128, fmin=0.0, fmax=None):
    """The Slaney filter bank M [n_mels, n_fft // 2 + 1] over np.linspace(0, sr / 2, n_fft // 2 + 1)."""
    fmax = float(sr) / 2 if fmax is None else float(fmax)
    return mel_triangles(np.linspace(0.0, float(sr) / 2, int(n_fft) // 2 + 1), mel_band_edges(n_mels, float(fmin), fmax))


def dct_basis(n_mfcc, n_mels):
    """D [n_mfcc, n_mels]: row 0 is 1 / sqrt(n_mels), row i is cos(i (2 m + 1) pi / (2 n_mels)) sqrt(2 / n_mels) -- the first rows
    of scipy.fft.dct(type=2, norm='ortho')."""
    n_mfcc, n_mels = int(n_mfcc), int(n_mels)
    m = np.arange(n_mels, dtype=np.float64)
    D = np.cos(np.arange(n_mfcc, dtype=np.float64)[:, None] * (2 * m + 1) * np.pi / (2.0 * n_mels)) * np.sqrt(2.0 / n_mels)
    if n_mfcc:
        D[0] = 1.0 / np.sqrt(n_mels)
    return D


def dct_row_sums(n_mfcc, n_mels):
    """r [n_mfcc]: the exact sums of the rows of the orthonormal DCT-II -- sqrt(n_mels) for row 0 (n_mels times 1 / sqrt(n_mels)),
    0 for every other row (the cosines of a row i >= 1 cancel).  The rounded table's own sums are a few ulps off these."""
    r = np.zeros(int(n_mfcc), dtype=np.float64)
    if n_mfcc:
        r[0] = np.sqrt(float(n_mels))
    return r


def hann(n_fft):
    return scipy.signal.get_window('hann', int(n_fft), fftbins=True).astype(np.float64)


def frame_counts(lengths, hop):
    """int64 [U]: T = 1 + L // hop per utterance."""
    return 1 + np.asarray(lengths, dtype=np.int64) // int(hop)


def reflect_index(p, L, n_fft):
    """The index into y of np.pad(y, n_fft // 2, mode='reflect')[p], for len(y) = L >= n_fft // 2 + 1: what the device gathers by."""
    q = np.asarray(p, dtype=np.int64) - int(n_fft) // 2
    q = np.abs(q)
    return np.where(q >= L, 2 * (L - 1) - q, q)


def frame_spans(counts):
    """[(t0, t1) ...]: the utterances' spans on the concatenated frame axis -- the `windows` of `windowed_hac`."""
    ends = np.cumsum(np.asarray(counts, dtype=np.int64))
    return [(int(e - c), int(e)) for c, e in zip(counts, ends)]


# ---- the host twin ------------------------------------------------------------------------------------------------------------------
def host_frames(y, n_fft, hop, window=None):
    """[T, n_fft] float64: rule 1 by its numpy calls."""
    y = np.asarray(y)
    n_fft, hop = int(n_fft), int(hop)
    if y.ndim != 1 or len(y) < n_fft // 2 + 1:
        raise ValueError("an utterance of at least n_fft // 2 + 1 = %d samples expected, got shape %s" % (n_fft // 2 + 1, y.shape))
    yp = np.pad(y.astype(np.float64), n_fft // 2, mode='reflect')
    T = 1 + len(y) // hop
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]
    return yp[idx] * (hann(n_fft) if window is None else np.asarray(window, dtype=np.float64))


def host_mel_energies(y, n_fft, hop, M, window=None):
    """S [T, n_mels]: rules 1 to 3, np.fft.rfft in float64."""
    P = np.abs(np.fft.rfft(host_frames(y, n_fft, hop, window), axis=1)) ** 2
    return P @ np.asarray(M, dtype=np.float64).T


def host_mfcc(S, D):
    """[T, n_mfcc]: rules 4 and 5 on one utterance's energies S [T, n_mels]; float64, or np.longdouble where S is (the tests'
    extended-precision reference)."""
    S = np.asarray(S)
    dt = np.longdouble if S.dtype == np.longdouble else np.float64
    S = S.astype(dt, copy=False)
    Ldb = 10 * np.log10(np.maximum(S, dt(AMIN)))
    Ldb = np.maximum(Ldb, Ldb.max() - dt(TOP_DB))
    return Ldb @ np.asarray(D, dtype=np.float64).astype(dt).T


def host_delta(x, order=1):
    """Rule 6 on x [n_mfcc, T] (time last, the library's orientation)."""
    x = np.asarray(x, dtype=np.float64)
    d = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(5, 5)], mode='edge')
    for _ in range(int(order)):
        d = scipy.signal.lfilter(DELTA_TAPS, 1, d, axis=-1)
    return d[..., 5:-5]


def host_streams_of_energies(S_list, D):
    """The three streams and the spans from the utterances' energies."""
    cep = [host_mfcc(S, D) for S in S_list]
    streams = [np.vstack(cep), np.vstack([host_delta(c.T, 1).T for c in cep]), np.vstack([host_delta(c.T, 2).T for c in cep])]
    return streams, frame_spans([len(c) for c in cep])


def host_mfcc_streams(audio, sr, n_mfcc=13, n_fft=2048, hop_length=512, n_mels=128, fmin=0.0, fmax=None):
    """([mfcc, delta, delta-delta] each [T_total, n_mfcc], [(t0, t1) per utterance]) of a list of utterances: the twin of
    `mfcc_streams`."""
    M, D = mel_filters(sr, n_fft, n_mels, fmin, fmax), dct_basis(n_mfcc, n_mels)
    return host_streams_of_energies([host_mel_energies(y, n_fft, hop_length, M) for y in _utterances(audio)], D)


# ---- the device path ----------------------------------------------------------------------------------------------------------------
def _utterances(audio):
    if isinstance(audio, np.ndarray) and audio.ndim == 1:
        return [audio]
    return [np.asarray(y) for y in audio]


def check_mfcc_inputs(audio, sr, n_mfcc=13, n_fft=2048, hop_length=512, n_mels=128, fmin=0.0, fmax=None, dtype=np.float64,
                      route='auto'):
    """The arguments of `mfcc_streams` as it uses them -- (samples, offsets int64 [U + 1], frame counts int64 [U], fmax) -- or
    ValueError before anything is uploaded, for everything include/features/klnmf_mfcc.h refuses: samples that are not int16 /
    float32 / float64 vectors (a list of mixed kinds runs as float64; other host types are refused), host values that are not
    finite, an utterance shorter than n_fft // 2 + 1, offsets that do not start at 0 or do not ascend, hop_length < 1,
    n_mels < 1, n_mfcc < 1 or above n_mels, an n_fft no route takes (or not the route asked for), n_mels above MFCC_MAX_MELS,
    streams that are not float32 / float64, totals not below 2^31 - 1, a band 0 <= fmin < fmax <= sr / 2 that is none."""
    if np.dtype(dtype) not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("dtype: float32 or float64 streams, got %s" % np.dtype(dtype))
    for name, v in (('n_mfcc', n_mfcc), ('n_fft', n_fft), ('hop_length', hop_length), ('n_mels', n_mels)):
        if int(v) != v:
            raise ValueError("%s: an integer expected, got %r" % (name, v))
    n_mfcc, n_fft, hop, n_mels = int(n_mfcc), int(n_fft), int(hop_length), int(n_mels)
    if hop < 1:
        raise ValueError("hop_length >= 1 expected, got %d" % hop)
    if n_mels < 1 or n_mels > _native.MFCC_MAX_MELS:
        raise ValueError("1 <= n_mels <= %d expected, got %d" % (_native.MFCC_MAX_MELS, n_mels))
    if n_mfcc < 1 or n_mfcc > n_mels:
        raise ValueError("1 <= n_mfcc <= n_mels expected, got n_mfcc = %d, n_mels = %d" % (n_mfcc, n_mels))
    if route not in _native.MFCC_ROUTES:
        raise ValueError("route: 'auto', 'fft' or 'direct', got %r" % (route,))
    if n_fft < 2 or _native.mfcc_route(n_fft, route) == 'refused':
        raise ValueError("n_fft = %d: the fft route takes the powers of two in [64, 4096], the direct route the even sizes in "
                         "[16, 1024] (route %r)" % (n_fft, route))
    fmax = float(sr) / 2 if fmax is None else float(fmax)
    if not (sr > 0 and 0 <= float(fmin) < fmax <= float(sr) / 2):
        raise ValueError("0 <= fmin < fmax <= sr / 2 expected, got fmin = %r, fmax = %r, sr = %r" % (fmin, fmax, sr))
    if isinstance(audio, tuple) and len(audio) == 2 and _is_tensor(audio[0]):
        samples, offsets = audio
        if samples.dim() != 1 or str(samples.dtype) not in ('torch.int16', 'torch.float32', 'torch.float64') \
                or (samples.numel() > 1 and samples.stride(0) != 1):
            raise ValueError("samples: a contiguous 1-D int16 / float32 / float64 tensor expected")
        offsets = np.asarray(offsets)
        if offsets.ndim != 1 or len(offsets) < 1 or offsets.dtype.kind not in 'iu':
            raise ValueError("offsets: integers [U + 1] expected")
        offsets = offsets.astype(np.int64)
        if offsets[0] != 0 or offsets[-1] != samples.numel():
            raise ValueError("offsets start at 0 and end at the number of samples")
    else:
        parts = _utterances(audio)
        for u, y in enumerate(parts):
            if y.ndim != 1 or y.dtype not in _native.MFCC_SAMPLE_KINDS:
                raise ValueError("utterance %d: an int16 / float32 / float64 vector expected, got %s of shape %s" % (u, y.dtype, y.shape))
            if y.dtype.kind == 'f' and not np.all(np.isfinite(y)):
                raise ValueError("utterance %d: samples that are not finite" % u)
        kinds = set(y.dtype for y in parts)
        kind = kinds.pop() if len(kinds) == 1 else np.dtype(np.float64)
        samples = np.concatenate([y.astype(kind, copy=False) for y in parts]) if parts else np.zeros(0, dtype=kind)
        offsets = np.concatenate([[0], np.cumsum([len(y) for y in parts])]).astype(np.int64)
    lengths = np.diff(offsets)
    if (lengths < 0).any():
        raise ValueError("offsets that do not ascend")
    if len(lengths) and lengths.min() < n_fft // 2 + 1:
        raise ValueError("utterance %d has %d samples: below the n_fft // 2 + 1 = %d its reflection needs"
                         % (int(np.argmin(lengths)), int(lengths.min()), n_fft // 2 + 1))
    counts = frame_counts(lengths, hop)
    limit = 2 ** 31 - 1
    if len(lengths) >= limit or int(offsets[-1]) >= limit or int(counts.sum()) * n_mels >= limit:
        raise ValueError("utterances, samples and frames x n_mels below 2^31 - 1 expected")
    return samples, offsets, counts, fmax


def mfcc_streams(audio, sr, n_mfcc=13, n_fft=2048, hop_length=512, n_mels=128, fmin=0.0, fmax=None, dtype=np.float64, device=None,
                 output='device', route='auto'):
    """([mfcc, delta, delta-delta], spans): the three frame streams [T_total, n_mfcc] of `dtype` of every utterance of `audio`,
    one after the other, and the utterances' frame spans [(t0, t1) ...] -- the reference's `mfcc` and `delta` calls
    (features/hac.py:190-193) for a whole corpus in five launches (csrc/mfcc.hip.h), within the derived bars of `host_mfcc_streams`.

    audio: one vector, a list of vectors (int16, float32 or float64 -- `wavfile.read`'s integers as they are), or a pair
    (samples, offsets) of a 1-D tensor already on `device` and host offsets [U + 1].  output: 'device' -- tensors, what
    `windowed_hac` and `build_codebooks` take; 'numpy' -- host arrays.  ValueError (`check_mfcc_inputs`) before anything is
    uploaded."""
    if output not in ('device', 'numpy'):
        raise ValueError("output: 'device' or 'numpy', got %r" % (output,))
    samples, offsets, counts, fmax = check_mfcc_inputs(audio, sr, n_mfcc, n_fft, hop_length, n_mels, fmin, fmax, dtype, route)
    n_mfcc, n_fft, hop, n_mels = int(n_mfcc), int(n_fft), int(hop_length), int(n_mels)
    import torch
    dev = _torch_device(device)
    ordinal = dev.index if dev.type == 'cuda' and dev.index is not None else 0
    f64 = np.dtype(dtype) == np.float64
    U, T = len(counts), int(counts.sum())
    spans = frame_spans(counts)
    out = [torch.zeros((T, n_mfcc), dtype=torch.float64 if f64 else torch.float32, device=dev) for _ in range(3)]
    if U:
        d_samples = samples.to(dev) if _is_tensor(samples) else torch.from_numpy(samples).to(dev)
        kind = {'int16': _native.MFCC_I16, 'float32': _native.MFCC_F32, 'float64': _native.MFCC_F64}[str(d_samples.dtype).split('.')[-1]]
        table = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
        d_window, d_mel, d_dct = table(hann(n_fft)), table(mel_filters(sr, n_fft, n_mels, fmin, fmax)), table(dct_basis(n_mfcc, n_mels))
        d_dct_sums = table(dct_row_sums(n_mfcc, n_mels))
        work_bytes = _native.mfcc_work_bytes(U, int(offsets[-1]), T, n_fft, n_mels, n_mfcc)
        d_work = torch.empty(max(16, work_bytes), dtype=torch.uint8, device=dev)
        d_S = torch.empty((T, n_mels), dtype=torch.float64, device=dev)
        d_Smax = torch.empty(U, dtype=torch.float64, device=dev)
        _native.mfcc_mel_device(d_samples.data_ptr(), kind, offsets, n_fft, hop, d_window.data_ptr(), d_mel.data_ptr(), n_mels, T,
                                d_work.data_ptr(), work_bytes, d_S.data_ptr(), d_Smax.data_ptr(), route=route, device=ordinal)
        frame_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        _native.mfcc_cepstra_device(d_S.data_ptr(), d_Smax.data_ptr(), d_dct.data_ptr(), d_dct_sums.data_ptr(), n_mels, n_mfcc, frame_offsets,
                                    d_work.data_ptr(), work_bytes, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), n_mfcc,
                                    f64=f64, device=ordinal)
    if output == 'numpy':
        out = [t.cpu().numpy() for t in out]
    return out, spans
