"""Cases and references of the codebook builders (tests/test_kmeans_cpu.py, tests/test_kmeans_gpu.py).  numpy only.

The reference throughout is the host twin of multimodal_amd/features/codebook.py (`host_lloyd`, `host_gram`,
`host_iterative_kmeans`, `host_build_codebook`), which test_kmeans_cpu.py pins to the REFERENCE's recorded outputs in
tests/golden/g22_kmeans.npz (its `iterative_kmeans`, scipy's `kmeans2`) by equality.  Every comparison of the device with the twin
is bit for bit: `same_bits` asks for equal shapes, types and bit patterns."""
import functools
import os

import numpy as np

from multimodal_amd.features import codebook as cbk

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g22_kmeans.npz')
TILE, GROUP = 256, 4096


@functools.lru_cache(maxsize=None)
def golden():
    """{'a' | 'b': dict(data, K, iterative, init, matrix, matrix_labels, raw, raw_labels, raw_seed)} of G22, read-only."""
    g = np.load(GOLDEN)
    out = {}
    for tag in ('a', 'b'):
        s = {name: g['%s_%s' % (tag, name)] for name in ('data', 'iterative', 'init', 'matrix', 'matrix_labels', 'raw', 'raw_labels')}
        for a in s.values():
            a.setflags(write=False)
        s['matrix_labels'], s['raw_labels'] = s['matrix_labels'].astype(np.int32), s['raw_labels'].astype(np.int32)
        s['raw_seed'] = int(g['%s_raw_seed' % tag])
        s['K'] = s['init'].shape[0]
        out[tag] = s
    return out


def sorted_rows(c):
    c = np.asarray(c)
    return c[np.lexsort(c.T[::-1])]


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    assert got.tobytes() == want.tobytes(), 'bits differ at %d of %d places' % ((got != want).sum(), got.size)
    return True


@functools.lru_cache(maxsize=None)
def normals(seed, T, d, K, f32=False):
    """(frames, init): plain normals around K centres -- sums whose value depends on the order of the additions."""
    rng = np.random.default_rng(seed)
    dt = np.float32 if f32 else np.float64
    centres = rng.normal(size=(K, d))
    x = (centres[rng.integers(0, K, T)] + 0.5 * rng.normal(size=(T, d))).astype(dt)
    init = (centres + 0.1 * rng.normal(size=(K, d))).astype(dt)
    x.setflags(write=False)
    init.setflags(write=False)
    return x, init


@functools.lru_cache(maxsize=None)
def twin_lloyd(seed, T, d, K, f32, n_iter):
    x, init = normals(seed, T, d, K, f32)
    out = cbk.host_lloyd(x, init, n_iter)
    for a in out:
        a.setflags(write=False)
    return out
