"""CSR modalities kept on the device (DeviceDataset(keep_sparse=True)): what runs without a GPU.

  * `csr_rows_plan` -- the per-call planning from the host copies of the row pointers -- against scipy's own stack;
  * the two exports (klnmf_upload_csr_device_rows, klnmf_csr_rows_to_dense_device): declared, bound, counted in the documents;
  * with `_native.Context` replaced by a recording double, a keep-sparse `train` hands the binding pointers and per-modality
    scalars only: no host array of nnz length, and never the host upload `set_problem_sparse`.
"""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from multimodal_amd import _native
from multimodal_amd import device_data
from multimodal_amd.device_data import csr_rows_plan
from multimodal_amd.learner import MultimodalLearner
from multimodal_amd.lib import nmf
from tests import sparse_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUTS = [0, 87, 175, 263]
TINY32 = float(np.finfo(np.float32).smallest_subnormal)


def modalities(seed=5, dtype=np.float64, empty_first=False):
    X = sc.designed_csr(301, 263, 1, 1, seed, dtype=dtype)
    mods = [sp.csr_matrix(X[:, a:b]) for a, b in zip(CUTS[:-1], CUTS[1:])]
    if empty_first:
        mods[0] = sp.csr_matrix(mods[0].shape, dtype=dtype)
    return mods


def plan_of(mods, rows, coefs):
    least = [m.data.min() if m.nnz else None for m in mods]
    return csr_rows_plan([m.indptr for m in mods], rows, coefs, least)


ROW_LISTS = {
    'identity': np.arange(301),
    'reversed': np.arange(301)[::-1],
    'repeats': np.random.RandomState(3).randint(0, 301, 500),
    'single': np.array([17]),
    'none': np.array([], dtype=np.int64),
}


@pytest.mark.parametrize('rows', list(ROW_LISTS), ids=list(ROW_LISTS))
@pytest.mark.parametrize('empty_first', [False, True], ids=['full', 'empty-first'])
def test_the_plan_counts_what_scipy_stacks(rows, empty_first):
    mods = modalities(empty_first=empty_first)
    idx = ROW_LISTS[rows]
    coefs = (1.0, 0.5, 0.3)
    nnz, use_device = plan_of(mods, idx, coefs)
    assert nnz == sp.hstack([c * m[idx] for m, c in zip(mods, coefs)]).nnz
    assert use_device
    if rows == 'repeats':
        assert len(set(idx.tolist())) < idx.size                     # (the list does repeat rows)


def test_a_zero_coefficient_takes_the_host_path():
    mods = modalities()
    idx = ROW_LISTS['repeats']
    nnz, use_device = plan_of(mods, idx, (1.0, 0.0, 0.3))
    assert nnz == sp.hstack([c * m[idx] for m, c in zip(mods, (1.0, 0.0, 0.3))]).nnz      # (scipy keeps the zeros it stores)
    assert not use_device
    assert not plan_of(mods, idx, (1.0, -1.0, 0.3))[1]


def test_a_coefficient_that_underflows_the_smallest_value_takes_the_host_path():
    """The product is formed in the modality's own type: a coefficient that leaves float64 values alone rounds the smallest
    float32 value to zero."""
    m64, m32 = modalities(dtype=np.float64), modalities(dtype=np.float32)
    least = float(min(m.data.min() for m in m32))
    c = 0.4 * TINY32 / least                                         # least * c rounds to 0 in float32, not in float64
    assert np.float32(least) * np.float32(c) == 0 and least * c > 0
    idx = ROW_LISTS['identity']
    for mods, device in ((m64, True), (m32, False)):
        which = int(np.argmin([m.data.min() for m in mods]))
        coefs = [1.0, 1.0, 1.0]
        coefs[which] = c
        nnz, use_device = plan_of(mods, idx, coefs)
        assert nnz == sp.hstack([m[idx] for m in mods]).nnz
        assert use_device == device
        dropped = nmf._csr_of([m[idx] for m in mods], coefs)
        dropped.eliminate_zeros()
        assert (dropped.nnz < nnz) == (not device)                   # (the host path does drop entries exactly then)
    # a modality without stored entries constrains nothing
    assert plan_of(modalities(empty_first=True), idx, (1e-300, 1.0, 1.0))[1]


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------------
def test_the_new_exports_are_declared_bound_and_counted():
    header = open(os.path.join(ROOT, 'include', 'klnmf.h')).read()
    lib = _native.load()
    for name, nargs in (('klnmf_upload_csr_device_rows', 11), ('klnmf_csr_rows_to_dense_device', 11)):
        assert re.search(r'^int %s\s*\(' % name, header, flags=re.M), name
        assert name in _native.SIGNATURES and hasattr(lib, name), name
        assert len(_native.SIGNATURES[name][1]) == nargs, name
    assert callable(_native.Context.upload_csr_device_rows) and callable(_native.Context.set_problem_sparse_shape)
    assert callable(_native.csr_rows_to_dense_device)
    import inspect
    assert inspect.signature(device_data.DeviceDataset.__init__).parameters['keep_sparse'].default is False      # opt-in
    # each cites the reference lines it replaces, as the header's convention asks
    for name in ('klnmf_upload_csr_device_rows', 'klnmf_csr_rows_to_dense_device'):
        comment = header[:header.index('int %s(' % name)].rsplit('/*', 1)[1]
        assert 'experiment.py:163-164' in comment and 'learner.py:53-56' in comment, name
    declared = set(re.findall(r'^(?:int|const char \*)\s*(klnmf_\w+)\s*\(', header, flags=re.M))
    assert declared == set(_native.SIGNATURES)
    for doc in ('README.md', 'INTEGRATION.md', 'DESIGN.md'):
        assert '%d exports' % len(declared) in open(os.path.join(ROOT, doc)).read(), doc


def test_the_gather_kernels_live_in_their_own_header():
    csrc = os.path.join(ROOT, 'multimodal_amd', 'csrc')
    text = open(os.path.join(csrc, 'csrgather.hip.h')).read()
    for kernel in ('k_csrg_len', 'k_csrg_copy', 'k_csrg_dense'):
        assert kernel in text, kernel
    assert '#include "csrgather.hip.h"' in open(os.path.join(csrc, 'api_context.hip')).read()


# ---- nothing of nnz length reaches the binding -----------------------------------------------------------------------------------
class _Tensor(object):
    """What the CSR path asks of a device tensor, on a host array."""

    def __init__(self, a):
        self.a = np.ascontiguousarray(a)

    def data_ptr(self):
        return self.a.ctypes.data

    def numel(self):
        return self.a.size

    def element_size(self):
        return self.a.itemsize


class _HostDataset(device_data.DeviceDataset):
    def _to_device(self, array):
        return _Tensor(array)


class _Recorder(object):
    """Stands in for `_native.Context`: records every call `_fit_uploaded` makes on it."""
    calls = []

    def __init__(self, precision='f64', device=0, stream=None, pooled=False):
        self.precision = _native.PRECISIONS[precision]
        self.precision_name = precision

    def __enter__(self):
        return self

    def __exit__(self, *a):
        pass

    def __getattr__(self, name):
        def method(*args, **kwargs):
            _Recorder.calls.append((name, args, kwargs))
            if name == 'set_problem_sparse_shape':
                self.n, self.f, self.k = args[0], args[1], args[2]
            if name == 'set_problem_sparse':
                (self.n, self.f), self.k = args[0].shape, args[1]
            if name == 'run':
                return [], 0, False
            if name == 'fp8_report':
                return {}
            if name == 'get_W':
                return np.zeros((self.n, self.k))
            if name == 'get_H':
                return np.zeros((self.k, self.f))
        return method


def _sizes(value):
    """Element counts of every array-like in a (nested) argument."""
    if isinstance(value, (np.ndarray, sp.spmatrix)) or sp.issparse(value):
        return [value.nnz if sp.issparse(value) else value.size]
    if isinstance(value, (list, tuple)):
        return [len(value)] + [s for v in value for s in _sizes(v)]
    if isinstance(value, dict):
        return [s for v in value.values() for s in _sizes(v)]
    return []


def test_a_keep_sparse_train_hands_the_binding_no_array_of_nnz_length(monkeypatch):
    mods = modalities()
    rows = ROW_LISTS['repeats']
    coefs = [1.0, 0.5, 0.3]
    k = 3
    nnz = sp.hstack([m[rows] for m in mods]).nnz
    f = CUTS[-1]
    assert nnz > k * f and nnz > rows.size * k and nnz > rows.size      # (so that a count of nnz can only be the data's)
    _Recorder.calls = []
    monkeypatch.setattr(_native, 'Context', _Recorder)
    ds = _HostDataset(mods, device=0, keep_sparse=True)
    assert ds.keep_sparse and ds.sparse == [True] * 3 and ds.blocks == [None] * 3 and ds.dims == [87, 88, 88]
    learner = MultimodalLearner(['a', 'b', 'c'], ds.dims, coefs, k)
    ds.train(learner, rows, 4, init_dictionary=np.full((k, f), 1.0 / f))
    names = [c[0] for c in _Recorder.calls]
    assert 'set_problem_sparse' not in names and 'upload_V' not in names and 'upload_blocks' not in names
    assert names[:2] == ['set_problem_sparse_shape', 'upload_csr_device_rows'], names
    shape = _Recorder.calls[0][1]
    assert tuple(shape) == (rows.size, f, k, 4, nnz)
    sources, bounds, scales, src_rows, idx_ptr, n_rows = _Recorder.calls[1][1]
    assert len(sources) == 3 and all(len(s) == 4 and all(isinstance(v, (int, bool, np.bool_)) for v in s) for s in sources)
    assert list(bounds) == CUTS and list(scales) == coefs and src_rows == 301 and n_rows == rows.size and isinstance(idx_ptr, int)
    for name, args, kwargs in _Recorder.calls:
        assert all(s < nnz for s in _sizes(list(args)) + _sizes(kwargs)), name
    # ... and a coefficient of 0 does take the host upload, said once
    _Recorder.calls = []
    learner = MultimodalLearner(['a', 'b', 'c'], ds.dims, [1.0, 0.0, 0.3], k)
    ds.train(learner, rows, 4, init_dictionary=np.full((k, f), 1.0 / f))
    assert [c[0] for c in _Recorder.calls][0] == 'set_problem_sparse'
