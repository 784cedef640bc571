# encoding: utf-8
"""Histograms of acoustic co-occurrences (HAC) behind the MFCC front end (reference multimodal/features/hac.py:152-196).

The reference's `hac(data, sr, codebooks)` computes MFCCs and their deltas with librosa, quantises each of the three frame
streams on its codebook (`scipy.cluster.vq.vq`) and counts, per lag, the pairs (code at t, code at t + lag).  Everything behind
the MFCCs is integer work with an exact answer, and that part lives here:

* the host twin in numpy -- `quantize`, `coocurrences`, `compute_coocurrences` (the reference's names and outputs) and
  `hac_from_streams` (the reference's `hac` from the streams on);
* `windowed_hac`, the device path: the streams are quantised ONCE and every window [t0, t1) of a list becomes one row of a CSR
  matrix built on the GPU (klnmf_hac_count_device / klnmf_hac_fill_device, csrc/hac.hip.h) -- what the reference's sliding
  evaluation does with a `multiprocessing.Pool` over `process_win` and `sp.vstack` (samples/image_sound_eval_sliding.py:97-113);
* `frame_windows`, the frame ranges of the reference's `slider` (lib/window.py:345-357) on an integer frame axis.

The MFCC front end is `features.mfcc`'s (csrc/mfcc.hip.h), under rules stated there; the reference's names on audio -- `mfcc`,
`hac(data, sr, ...)`, `wav2hac`, `build_codebooks_from_list_of_wav` -- stand at the end of this module on top of it, with
`hac_many` and `build_codebooks_from_audio` for a whole corpus at once.  The codebook builders (`build_codebook`,
`iterative_kmeans`) are `features.codebook`'s, whose device codebooks `windowed_hac` takes as they are.
"""
import numpy as np
import scipy.sparse as sp

from .. import _native

DEFAULT_LAGS = (5, 2)        # the reference's `lags=[5, 2]`


# ---- the host twin ------------------------------------------------------------------------------------------------------------------
def quantize(data, centroids):
    """int32 [T]: for every frame of `data` [T, d] the index of the nearest row of `centroids` [K, d] -- `vq(data, centroids)[0]`
    of the reference (features/hac.py:173) under a stated rule, the one `k_hac_vq` implements: the squared distance
    sum_j (x_j - c_j)^2 in float64, j ascending, every difference, product and sum rounded on its own; the lowest index among
    equal minima; a NaN distance never wins (all NaN: 0)."""
    X = np.asarray(data, dtype=np.float64)
    C = np.asarray(centroids, dtype=np.float64)
    if X.ndim != 2 or C.ndim != 2 or X.shape[1] != C.shape[1] or C.shape[0] < 1:
        raise ValueError("frames [T, d] and a codebook [K >= 1, d] expected, got shapes %s and %s" % (X.shape, C.shape))
    out = np.zeros(X.shape[0], dtype=np.int32)
    step = max(1, (1 << 22) // max(1, C.shape[0]))
    with np.errstate(all='ignore'):
        for r0 in range(0, X.shape[0], step):
            x = X[r0:r0 + step]
            acc = np.zeros((x.shape[0], C.shape[0]), dtype=np.float64)
            for j in range(X.shape[1]):
                diff = x[:, j:j + 1] - C[np.newaxis, :, j]
                acc = acc + diff * diff
            acc[np.isnan(acc)] = np.inf
            out[r0:r0 + step] = np.argmin(acc, axis=1)
    return out


def coocurrences(quantized_data, n_quantized, lag):
    """The vector of n_quantized^2 counts of the pairs (value at t, value at t + lag), the later one the high digit (reference
    features/hac.py:152-169).  A series no longer than the lag gives zeros."""
    q = np.asarray(quantized_data, dtype=np.int64)
    pair_idx = q[lag:] * n_quantized + q[:max(0, len(q) - lag)]
    return np.bincount(pair_idx, minlength=n_quantized ** 2)


def compute_coocurrences(data, centroids, lags):
    """hstack over the lags of the co-occurrence counts of the quantised frames (reference features/hac.py:172-175)."""
    centroids = np.asarray(centroids)
    quantized = quantize(data, centroids)
    return np.hstack([coocurrences(quantized, centroids.shape[0], l) for l in lags])


def hac_from_streams(streams, codebooks, lags=DEFAULT_LAGS):
    """The reference's `hac` (features/hac.py:178-196) from its frame streams on: hstack over (stream, codebook) of
    `compute_coocurrences` -- a dense vector of counts."""
    return np.hstack([compute_coocurrences(stream, codebook, lags) for stream, codebook in zip(streams, codebooks)])


def frame_windows(n_frames, width, shift, partial=False):
    """[(t0, t1) ...]: the windows of `slider(0, n_frames, width, shift, partial)` (reference lib/window.py:345-357) for integer
    arguments -- starts 0, shift, ...; without `partial` the full windows alone (the last start is the last with
    t0 + width <= n_frames), with it every start below n_frames, the windows cut at n_frames."""
    n, width, shift = int(n_frames), int(width), int(shift)
    if n < 0 or width < 1 or shift < 1:
        raise ValueError("n_frames >= 0, width >= 1 and shift >= 1 expected, got %r, %r, %r" % (n_frames, width, shift))
    end = n if partial else n - width
    if end < 0:
        return []
    steps = end // shift
    starts = [i * shift for i in range(steps)]
    if not partial or steps * shift != end:
        starts.append(steps * shift)
    return [(t, min(t + width, n)) for t in starts]


def host_windowed_hac(streams, codebooks, windows, lags=DEFAULT_LAGS, dtype=np.float64):
    """`windowed_hac(..., output='scipy')` from the host twin: one `compute_coocurrences`-style row per window, the streams
    quantised once (a window's labels are the slice of the stream's labels).  What the device path is tested against."""
    codes = [quantize(x, c) for x, c in zip(streams, codebooks)]
    Ks = [np.asarray(c).shape[0] for c in codebooks]
    F = sum(len(lags) * K * K for K in Ks)
    indptr, indices, data = [0], [], []
    for t0, t1 in windows:
        row = np.hstack([coocurrences(q[t0:t1], K, l) for q, K in zip(codes, Ks) for l in lags]) if codes else np.zeros(0, dtype=np.int64)
        nz = np.flatnonzero(row)
        indices.append(nz.astype(np.int32))
        data.append(row[nz].astype(dtype))
        indptr.append(indptr[-1] + len(nz))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)
    return sp.csr_matrix((cat(data, dtype), cat(indices, np.int32), np.asarray(indptr, dtype=np.int64)), shape=(len(indptr) - 1, F))


# ---- the device path ----------------------------------------------------------------------------------------------------------------
class DeviceCsrRows(object):
    """A CSR matrix in device memory as `windowed_hac(..., output='device')` leaves it: `d_indptr` (int64 [n + 1]), `d_indices`
    (int32), `d_data` (float32 / float64) device tensors, `indptr` the host copy of the row pointers; sorted rows, no explicit
    zeros, no duplicates -- `device_data._DeviceCsr`'s form, what klnmf_upload_csr_device_rows reads."""

    def __init__(self, shape, d_indptr, d_indices, d_data, indptr, nnz, f64):
        self.shape = (int(shape[0]), int(shape[1]))
        self.d_indptr, self.d_indices, self.d_data = d_indptr, d_indices, d_data
        self.indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        self.nnz = int(nnz)
        self.f64 = bool(f64)
        self.dtype = np.dtype(np.float64 if f64 else np.float32)
        self._least = None

    @property
    def least(self):
        """The smallest stored value as a numpy scalar of the values' type (None without stored entries): `csr_rows_plan`'s."""
        if self.nnz and self._least is None:
            self._least = self.dtype.type(self.d_data[:self.nnz].min().item())
        return self._least

    def pointers(self):
        return self.d_indptr.data_ptr(), self.d_indices.data_ptr(), self.d_data.data_ptr(), self.f64

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.d_indptr, self.d_indices, self.d_data))

    def to_scipy(self):
        """The matrix as a scipy CSR matrix on the host (a download)."""
        indices = self.d_indices[:self.nnz].cpu().numpy().astype(np.int32, copy=True)
        data = self.d_data[:self.nnz].cpu().numpy().astype(self.dtype, copy=True)
        return sp.csr_matrix((data, indices, self.indptr.copy()), shape=self.shape)


def _is_tensor(a):
    return hasattr(a, 'data_ptr') and hasattr(a, 'stride')


def _torch_device(device):
    import torch
    if device is None:
        return torch.device('cuda', torch.cuda.current_device())
    if isinstance(device, int):
        return torch.device('cuda', device)
    return torch.device(device)


def check_hac_inputs(streams, codebooks, windows, lags, dtype=np.float64):
    """The arguments of `windowed_hac` as it uses them -- (streams, codebooks, windows int64 [N, 2], lags, T, Ks, F, f64) -- or
    ValueError before anything is uploaded: not 1 to 8 streams with a codebook each, not 1 to 8 integer lags >= 1, matrices that
    are not 2-D of float32 / float64 (host arrays of other types are taken as float64) or whose dimensions do not agree (one T
    for all streams, d_s shared by stream s and its codebook, K_s >= 1), host values that are not finite, a window outside
    [0, T] or with t1 < t0, F = sum_s len(lags) * K_s^2 >= 2^31, values that are not float32 / float64."""
    streams, codebooks = list(streams), list(codebooks)
    if not 1 <= len(streams) <= _native.HAC_MAX_STREAMS or len(codebooks) != len(streams):
        raise ValueError("1 to %d streams with one codebook each expected, got %d streams and %d codebooks"
                         % (_native.HAC_MAX_STREAMS, len(streams), len(codebooks)))
    if np.dtype(dtype) not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("dtype: float32 or float64 values, got %s" % np.dtype(dtype))
    lag_list = [l for l in lags]
    if not 1 <= len(lag_list) <= _native.HAC_MAX_LAGS:
        raise ValueError("1 to %d lags expected, got %d" % (_native.HAC_MAX_LAGS, len(lag_list)))
    for l in lag_list:
        if int(l) != l or int(l) < 1 or int(l) >= 2 ** 31:
            raise ValueError("lags are integers >= 1, got %r" % (l,))
    lag_list = [int(l) for l in lag_list]

    def matrix(a, what):
        if _is_tensor(a):
            if a.dim() != 2 or str(a.dtype) not in ('torch.float32', 'torch.float64') or (a.shape[1] > 1 and a.stride(1) != 1):
                raise ValueError("%s: a 2-D float32 / float64 tensor with contiguous rows expected" % what)
            return a
        a = np.asarray(a)
        if a.ndim != 2:
            raise ValueError("%s: a matrix expected, got shape %s" % (what, a.shape))
        a = np.ascontiguousarray(a, dtype=a.dtype if a.dtype in (np.float32, np.float64) else np.float64)
        if not np.all(np.isfinite(a)):
            raise ValueError("%s: values that are not finite" % what)
        return a

    streams = [matrix(x, "stream %d" % s) for s, x in enumerate(streams)]
    codebooks = [matrix(c, "codebook %d" % s) for s, c in enumerate(codebooks)]
    T = int(streams[0].shape[0])
    Ks = []
    for s, (x, c) in enumerate(zip(streams, codebooks)):
        if int(x.shape[0]) != T:
            raise ValueError("stream %d has %d frames, stream 0 has %d" % (s, x.shape[0], T))
        if int(x.shape[1]) != int(c.shape[1]) or int(c.shape[1]) < 1 or int(c.shape[0]) < 1:
            raise ValueError("stream %d: frames of shape %s against a codebook of shape %s" % (s, tuple(x.shape), tuple(c.shape)))
        Ks.append(int(c.shape[0]))
    if T >= 2 ** 31 - 1:
        raise ValueError("fewer than 2^31 - 1 frames expected, got %d" % T)
    F = sum(len(lag_list) * K * K for K in Ks)
    if F >= 2 ** 31 - 1 or max(Ks) > 46340:
        raise ValueError("F = sum of len(lags) * K^2 = %d columns: not below 2^31" % F)
    w = np.asarray(windows)
    if w.size == 0:
        w = np.zeros((0, 2), dtype=np.int64)
    if w.ndim != 2 or w.shape[1] != 2 or (w.dtype.kind not in 'iu' and not np.all(w == np.floor(w))):
        raise ValueError("windows: a list of integer (t0, t1) pairs expected, got shape %s" % (w.shape,))
    w = np.ascontiguousarray(w, dtype=np.int64)
    if len(w) and (w[:, 0].min() < 0 or (w[:, 1] < w[:, 0]).any() or w[:, 1].max() > T):
        raise ValueError("windows: every (t0, t1) must satisfy 0 <= t0 <= t1 <= %d frames" % T)
    if len(w) * len(streams) * len(lag_list) >= 2 ** 31 - 1:
        raise ValueError("windows x streams x lags = %d segments: not below 2^31" % (len(w) * len(streams) * len(lag_list)))
    f32 = all(str(a.dtype).endswith('float32') for a in streams + codebooks)
    return streams, codebooks, w, lag_list, T, Ks, F, not f32


def windowed_hac(streams, codebooks, windows, lags=DEFAULT_LAGS, dtype=np.float64, device=None, output='scipy'):
    """The [len(windows), F] CSR matrix whose row w is `hac_from_streams` of the frames [t0, t1) of window w, built on the GPU:
    every frame quantised once, then a fixed number of launches for all windows (csrc/hac.hip.h).

    streams: S <= 8 matrices [T, d_s]; codebooks: [K_s, d_s] each -- host arrays (uploaded here; float32 if all are float32,
    float64 otherwise) or tensors already on `device`, all of one floating type.  windows: host (t0, t1) pairs with
    0 <= t0 <= t1 <= T.  lags: up to 8 integers >= 1, in the order of the column blocks.  dtype: the type of the counts.
    output: 'scipy' -- a scipy.sparse.csr_matrix on the host; 'device' -- a `DeviceCsrRows` that
    `MultimodalLearner.reconstruct_internal` takes as it is.  ValueError (`check_hac_inputs`) before anything is uploaded;
    `_native.NativeError` (KLNMF_ERR_UNSUPP) before anything is launched for a window of more than HAC_SORT_MAX + lag frames over a
    codebook of more than HAC_DENSE_MAX_K units."""
    if output not in ('scipy', 'device'):
        raise ValueError("output: 'scipy' or 'device', got %r" % (output,))
    streams, codebooks, w, lag_list, T, Ks, F, f64 = check_hac_inputs(streams, codebooks, windows, lags, dtype)
    import torch
    dev = _torch_device(device)
    ordinal = dev.index if dev.type == 'cuda' and dev.index is not None else 0
    tdt = torch.float64 if f64 else torch.float32
    place = lambda a: (a if _is_tensor(a) else torch.from_numpy(a if a.flags.writeable else a.copy())).to(device=dev, dtype=tdt)
    d_streams, d_codebooks = [place(x) for x in streams], [place(c) for c in codebooks]
    table = [(x.data_ptr() if T else 0, x.stride(0) if T > 1 else x.shape[1], c.data_ptr(), c.stride(0) if c.shape[0] > 1 else c.shape[1],
              x.shape[1], K) for x, c, K in zip(d_streams, d_codebooks, Ks)]
    N = len(w)
    work_bytes = _native.hac_work_bytes(len(Ks), T, len(lag_list), N)
    d_work = torch.empty(max(16, work_bytes), dtype=torch.uint8, device=dev)
    d_indptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    nnz = _native.hac_count_device(table, T, lag_list, w, d_work.data_ptr(), work_bytes, d_indptr.data_ptr(), f64=f64, device=ordinal)
    vf64 = np.dtype(dtype) == np.float64
    d_indices = torch.zeros(max(1, nnz), dtype=torch.int32, device=dev)     # (at least one element: a valid pointer)
    d_data = torch.zeros(max(1, nnz), dtype=torch.float64 if vf64 else torch.float32, device=dev)
    _native.hac_fill_device(Ks, T, lag_list, w, d_work.data_ptr(), work_bytes, nnz, d_indices.data_ptr(), d_data.data_ptr(),
                            f64=vf64, device=ordinal)
    rows = DeviceCsrRows((N, F), d_indptr, d_indices, d_data, d_indptr.cpu().numpy(), nnz, vf64)
    return rows if output == 'device' else rows.to_scipy()


# ---- from audio: the reference's entry points behind the device front end ------------------------------------------------------------
def _mfcc_params(values):
    """The reference's `complete_mfcc_params` (features/hac.py:30-41): n_mfcc = 13 unless given."""
    params = {'n_mfcc': 13}
    params.update(values)
    return params


def mfcc(data, sr=22050, n_mfcc=20, device=None, **kwargs):
    """The reference's `mfcc(data, sr, n_mfcc, **kwargs)` (features/hac.py:44-65): a host array [n_mfcc, T], computed on the GPU
    under `features.mfcc`'s rules."""
    from . import mfcc as front
    streams, _ = front.mfcc_streams(np.asarray(data), sr, n_mfcc=n_mfcc, device=device, output='numpy', **kwargs)
    return np.ascontiguousarray(streams[0].T)


def hac_many(audio_list, sr, codebooks, lags=DEFAULT_LAGS, dtype=np.float64, device=None, output='scipy', **mfcc_params):
    """The [len(audio_list), F] CSR matrix whose row u is the reference's `hac(audio_list[u], sr, codebooks, lags, **mfcc_params)`
    (features/hac.py:178-196): ONE `features.mfcc.mfcc_streams` call for the corpus and ONE `windowed_hac` call over the
    utterances' frame spans; the streams never leave the device.  output: 'scipy' or 'device' (a `DeviceCsrRows`, what
    `MultimodalLearner.reconstruct_internal` takes)."""
    from . import mfcc as front
    streams, spans = front.mfcc_streams(audio_list, sr, device=device, output='device', **_mfcc_params(mfcc_params))
    return windowed_hac(streams, codebooks, spans, lags=lags, dtype=dtype, device=device, output=output)


def hac(data, sr, codebooks, lags=DEFAULT_LAGS, device=None, **mfcc_params):
    """The reference's `hac(data, sr, codebooks, lags, **mfcc_params)` (features/hac.py:178-196): the dense vector of counts of
    one utterance."""
    row = hac_many([np.asarray(data)], sr, codebooks, lags=lags, device=device, output='scipy', **mfcc_params)
    return np.asarray(row.toarray()).ravel().astype(np.int64)


def wav2hac(wav_path, codebooks, lags=DEFAULT_LAGS, device=None, **mfcc_params):
    """The reference's `wav2hac` (features/hac.py:199-201)."""
    from scipy.io import wavfile
    sr, data = wavfile.read(wav_path)
    return hac(data, sr, codebooks, lags=lags, device=device, **mfcc_params)


def build_codebooks_from_audio(audio_list, sr, ks, mode='raw', rng=None, device=None, output='numpy', **mfcc_params):
    """The three codebooks of the reference's `build_codebooks_from_list_of_wav` (features/hac.py:110-149) from the utterances'
    samples: `mfcc_streams(output='device')` into `features.codebook.build_codebooks`."""
    from . import codebook, mfcc as front
    streams, _ = front.mfcc_streams(audio_list, sr, device=device, output='device', **_mfcc_params(mfcc_params))
    return codebook.build_codebooks(streams, ks, mode=mode, rng=rng, device=device, output=output)


def build_codebooks_from_list_of_wav(wavs, ks, mode='raw', rng=None, device=None, output='numpy', **mfcc_params):
    """The reference's `build_codebooks_from_list_of_wav(wavs, ks, mode, **mfcc_params)` (features/hac.py:110-149); the files
    share one sample rate (a call has one filter bank)."""
    from scipy.io import wavfile
    read = [wavfile.read(w) for w in wavs]
    rates = set(int(sr) for sr, _ in read)
    if len(rates) != 1:
        raise ValueError("files of one sample rate expected, got %s" % sorted(rates))
    return build_codebooks_from_audio([data for _, data in read], rates.pop(), ks, mode=mode, rng=rng, device=device, output=output,
                                      **mfcc_params)
