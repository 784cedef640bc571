#!/usr/bin/env python3
"""G21: outputs of the REFERENCE's `multimodal.features.hac` (scipy's `vq` labels and `compute_coocurrences`) on window slices of
seeded frame streams, and of its `lib.window.slider` at integer arguments.

    python tests/golden/make_golden_hac.py <directory of the reference checkout>

Writes tests/golden/g21_hac.npz.  The inputs (streams, codebooks, lags, windows) travel with the reference's outputs; nothing of
the reference's source does.  The reference module imports an audio library for its MFCC front end at the top; the functions used
here never call it, so an empty stand-in module takes its place for the import only.

Two sets:
  a  three streams (d = 13, 13, 5; K = 7, 12, 3), T = 401, lags [4, 1], 41 windows of assorted lengths (empty ones, ones no
     longer than a lag, the whole range);
  b  one stream, K = 150, d = 13, T = 1003, lags [5, 2], 50-frame windows every 10 frames.
Frames are a codebook row plus 0.35 sigma noise, rounded to multiples of 2^-10 (exact in float32 and float64; the file compresses).

A condition, not a tolerance: for every frame the gap between the nearest and the second-nearest squared distance must exceed 1e-6
of the second-nearest -- then scipy's BLAS-formula distances and the direct formula cannot disagree on a label, and the fixture
pins the reference's choice itself.  The script asserts it, and that the direct formula's labels are scipy's.

Per window the row is hstack over the streams of `compute_coocurrences(stream[t0:t1], codebook, lags)` -- the reference's `hac`
(features/hac.py:193-196) behind its MFCCs; an empty window (which scipy's `vq` refuses) is an empty row.  Rows are stored as CSR
arrays."""
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SLIDER_ARGS = [(100, 50, 10, False), (100, 50, 10, True), (103, 50, 10, False), (103, 50, 10, True), (50, 50, 10, False),
               (49, 50, 10, False), (49, 50, 10, True), (0, 5, 2, True), (0, 5, 2, False), (7, 1, 1, False), (7, 3, 5, True),
               (1003, 50, 10, False), (60, 7, 7, False), (60, 7, 7, True), (10, 4, 3, True)]


def stand_in_audio_library():
    names = {'librosa': ('logamplitude',), 'librosa.feature': ('delta', 'melspectrogram'), 'librosa.filters': ('dct',)}
    for name, attrs in names.items():
        mod = types.ModuleType(name)
        for a in attrs:
            setattr(mod, a, None)
        sys.modules[name] = mod


def draw(rng, T, K, d):
    codebook = np.round(rng.normal(size=(K, d)) * 1024) / 1024
    rows = rng.integers(0, K, T)
    # runs of a few frames on one unit, as quantised speech has them: repeated pair codes, counts above 1
    rows = np.repeat(rows, 3)[:T]
    frames = np.round((codebook[rows] + 0.35 * rng.normal(size=(T, d))) * 1024) / 1024
    return frames, codebook


def direct_labels(frames, codebook):
    acc = np.zeros((frames.shape[0], codebook.shape[0]))
    for j in range(frames.shape[1]):
        diff = frames[:, j:j + 1] - codebook[np.newaxis, :, j]
        acc = acc + diff * diff
    two = np.sort(acc, axis=1)[:, :2] if codebook.shape[0] > 1 else None
    gap = np.inf if two is None else float(np.min((two[:, 1] - two[:, 0]) / two[:, 1]))
    return np.argmin(acc, axis=1), gap


def rows_of(rhac, vq, streams, codebooks, lags, windows):
    F = sum(len(lags) * c.shape[0] ** 2 for c in codebooks)
    indptr, indices, data = [0], [], []
    for t0, t1 in windows:
        if t1 > t0:
            row = np.hstack([rhac.compute_coocurrences(x[t0:t1], c, lags) for x, c in zip(streams, codebooks)])
        else:
            row = np.zeros(F, dtype=np.int64)
        assert row.shape == (F,)
        nz = np.flatnonzero(row)
        indices.append(nz)
        data.append(row[nz])
        indptr.append(indptr[-1] + len(nz))
    return (np.asarray(indptr, dtype=np.int64), np.concatenate(indices).astype(np.int32), np.concatenate(data).astype(np.int32))


def main(reference):
    stand_in_audio_library()
    sys.path.insert(0, reference)
    from multimodal.features import hac as rhac
    from multimodal.lib.window import slider
    from scipy.cluster.vq import vq
    rng = np.random.default_rng(21)
    out = {}
    sets = {'a': ([(13, 7), (13, 12), (5, 3)], 401, [4, 1]), 'b': ([(13, 150)], 1003, [5, 2])}
    for tag, (shapes, T, lags) in sets.items():
        streams, codebooks = zip(*[draw(rng, T, K, d) for d, K in shapes])
        if tag == 'a':
            windows = [(0, T), (0, 0), (T, T), (17, 17), (5, 6), (5, 7), (9, 13), (9, 14), (30, 35), (0, 1), (T - 1, T), (T - 5, T)]
            while len(windows) < 41:
                t0 = int(rng.integers(0, T))
                windows.append((t0, min(T, t0 + int(rng.integers(0, 120)))))
        else:
            windows = [(int(a), int(b)) for a, b in slider(0, T, 50, 10)]
        worst = np.inf
        for s, (x, c) in enumerate(zip(streams, codebooks)):
            labels, _ = vq(x, c)
            mine, gap = direct_labels(x, c)
            assert gap > 1e-6, (tag, s, gap)
            assert np.array_equal(labels, mine), (tag, s)
            worst = min(worst, gap)
            out['%s_stream%d' % (tag, s)] = x
            out['%s_codebook%d' % (tag, s)] = c
            out['%s_labels%d' % (tag, s)] = labels.astype(np.int16)
        indptr, indices, data = rows_of(rhac, vq, streams, codebooks, lags, windows)
        out['%s_lags' % tag] = np.asarray(lags, dtype=np.int64)
        out['%s_windows' % tag] = np.asarray(windows, dtype=np.int64)
        out['%s_indptr' % tag], out['%s_indices' % tag], out['%s_data' % tag] = indptr, indices, data
        out['%s_n_streams' % tag] = np.asarray(len(streams))
        print('set %s: T = %d, %d windows, nnz = %d, largest count %d, smallest relative gap %.3g'
              % (tag, T, len(windows), indptr[-1], data.max(), worst))
    out['slider_args'] = np.asarray([(n, w, s, int(p)) for n, w, s, p in SLIDER_ARGS], dtype=np.int64)
    spans = [np.asarray(slider(0, n, w, s, partial=p), dtype=np.float64).reshape(-1, 2) for n, w, s, p in SLIDER_ARGS]
    out['slider_indptr'] = np.cumsum([0] + [len(sp) for sp in spans]).astype(np.int64)
    out['slider_windows'] = np.concatenate(spans)
    path = os.path.join(HERE, 'g21_hac.npz')
    np.savez_compressed(path, **out)
    print('%s: %d bytes' % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 200 * 1024


if __name__ == '__main__':
    main(sys.argv[1])
