"""Cases and references of the windowed co-occurrence histograms (tests/test_hac_cpu.py, tests/test_hac_gpu.py).  numpy only.

The reference throughout is the host twin of multimodal_amd/features/hac.py (`quantize`, `coocurrences`, `host_windowed_hac`),
which test_hac_cpu.py pins to the REFERENCE's outputs in tests/golden/g21_hac.npz (scipy's vq labels and compute_coocurrences on
window slices) as exact integers.  Every comparison with it is exact: `same_csr` asks for equal shapes, row pointers, column
indices and values, and for the types of the CSR contract.

`coded(codes, K)` is a stream whose quantisation is `codes` by construction (d = 1, codebook row k = k, frame = its code), so
that a count test chooses its pair codes directly."""
import functools
import os

import numpy as np
import scipy.sparse as sp

from multimodal_amd.features import hac

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g21_hac.npz')


@functools.lru_cache(maxsize=None)
def golden():
    """{'a' | 'b': dict(streams, codebooks, labels, lags, windows, csr)} and 'slider': [(args, windows)] of G21, read-only."""
    g = np.load(GOLDEN)
    out = {}
    for tag in ('a', 'b'):
        S = int(g['%s_n_streams' % tag])
        streams = [g['%s_stream%d' % (tag, s)] for s in range(S)]
        codebooks = [g['%s_codebook%d' % (tag, s)] for s in range(S)]
        for a in streams + codebooks:
            a.setflags(write=False)
        lags = [int(l) for l in g['%s_lags' % tag]]
        windows = [(int(a), int(b)) for a, b in g['%s_windows' % tag]]
        F = sum(len(lags) * c.shape[0] ** 2 for c in codebooks)
        csr = sp.csr_matrix((g['%s_data' % tag].astype(np.int64), g['%s_indices' % tag], g['%s_indptr' % tag]), shape=(len(windows), F))
        out[tag] = dict(streams=streams, codebooks=codebooks, labels=[g['%s_labels%d' % (tag, s)].astype(np.int32) for s in range(S)],
                        lags=lags, windows=windows, csr=csr)
    ip = g['slider_indptr']
    out['slider'] = [(tuple(int(v) for v in args), g['slider_windows'][ip[i]:ip[i + 1]]) for i, args in enumerate(g['slider_args'])]
    return out


def coded(codes, K):
    """(stream [T, 1], codebook [K, 1]) whose labels are `codes`."""
    codes = np.asarray(codes)
    assert codes.size == 0 or (codes.min() >= 0 and codes.max() < K)
    return codes.astype(np.float64).reshape(-1, 1), np.arange(K, dtype=np.float64).reshape(-1, 1)


def twin(streams, codebooks, windows, lags, dtype=np.float64):
    return hac.host_windowed_hac(streams, codebooks, windows, lags=lags, dtype=dtype)


def same_csr(got, want, dtype=None):
    """`got` IS `want`: shape, int row pointers, sorted int32 indices without duplicates, values without zeros -- all equal."""
    assert sp.isspmatrix_csr(got) and got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got.indptr, want.indptr), 'row pointers'
    assert got.indices.dtype == np.int32 and np.array_equal(got.indices, want.indices), 'column indices'
    assert np.array_equal(got.data, want.data), 'values'
    if dtype is not None:
        assert got.data.dtype == np.dtype(dtype)
    assert not (got.data == 0).any()
    for r in range(got.shape[0]):
        row = got.indices[got.indptr[r]:got.indptr[r + 1]]
        assert (np.diff(row) > 0).all(), 'row %d is not strictly ascending' % r
    return True


def random_codes(seed, T, K):
    return np.random.default_rng(seed).integers(0, K, T)
