"""CSR batches without a GPU: the exports of include/klnmf_batch_csr.h, and -- with test_batch_cpu's recording fakes standing in
for `_native.Batch` and `_native.Context` -- the route `fit_transform_batch`, `DeviceDataset.train_many`,
`reconstruct_internal_multi_many` and `DeviceEvaluation.internal_many` take for scipy-sparse input: one CSR batch where the
problems allow it, the sequential calls otherwise."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from multimodal_amd import _native
from multimodal_amd import device_data
from multimodal_amd.learner import MultimodalLearner
from multimodal_amd.lib import nmf
from tests import sparse_cases as sc
from tests.test_batch_cpu import _Fake, _FakeBatch, batches_opened, dictionaries_set, make_models, recorded, N, F, K      # noqa: F401
from tests.test_csr_device_rows_cpu import _HostDataset, modalities, CUTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_in(header):
    text = open(os.path.join(ROOT, 'include', header)).read()
    return set(re.findall(r'^(?:int|const char \*)\s*(klnmf_\w+)\s*\(', text, flags=re.M))


HEADER_SIZES = [79, 15, 3, 3, 4, 3, 3, 3, 4, 4, 5]        # the exports of each header of _native.HEADER_TABLES, in its order


def other_headers(header):
    """The headers of _native.HEADER_TABLES but `header`."""
    names = [h for h, _ in _native.HEADER_TABLES]
    assert header in names
    return [h for h in names if h != header]


def check_header_tables():
    """The registry lists every header under include/, each table is its header's declarations, no symbol stands in two tables,
    and no header changed its number of exports."""
    assert sorted(h for h, _ in _native.HEADER_TABLES) == sorted(f for f in os.listdir(os.path.join(ROOT, 'include')) if f.endswith('.h'))
    assert [len(t) for _, t in _native.HEADER_TABLES] == HEADER_SIZES
    owner = {}
    for header, table in _native.HEADER_TABLES:
        assert declared_in(header) == set(table), header
        for name in table:
            assert name not in owner, (name, header, owner[name])
            owner[name] = header


def test_every_declared_csr_batch_symbol_is_bound_and_exported():
    declared = declared_in('klnmf_batch_csr.h')
    assert declared == {'klnmf_batch_set_problem_sparse', 'klnmf_batch_upload_csr_rows', 'klnmf_batch_upload_csr_device_rows'}
    assert declared == set(_native.BATCH_CSR_SIGNATURES)
    lib = _native.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert len(_native.BATCH_CSR_SIGNATURES['klnmf_batch_upload_csr_device_rows'][1]) == 12      # klnmf_upload_csr_device_rows' 11 + p
    check_header_tables()
    for doc in ('README.md', 'INTEGRATION.md', 'DESIGN.md'):
        text = open(os.path.join(ROOT, doc)).read()
        assert 'klnmf_batch_csr.h' in text and '3 exports' in text, doc


# ---- fit_transform_batch ----------------------------------------------------------------------------------------------------------
class _FakeCsrBatch(_FakeBatch):
    """test_batch_cpu's fake batch, which reads `set_problem_sparse` as a context's (X, k, cap): a batch's takes the shape."""

    def set_problem_sparse(self, n, f, k, cap, nnzs):
        _Fake.calls.append(('set_problem_sparse', (n, f, k, cap, list(nnzs)), {}))
        _Fake.batch_calls.append('set_problem_sparse')
        self.n, self.f, self.k = n, f, k


class _FakeCsrContext(_Fake):
    """... and its fake context, which does not know the shape-only form the device gather uses."""

    def set_problem_sparse_shape(self, n, f, k, cap, nnz):
        _Fake.calls.append(('set_problem_sparse_shape', (n, f, k, cap, nnz), {}))
        self.n, self.f, self.k = n, f, k


@pytest.fixture
def recorded_csr(recorded, monkeypatch):
    monkeypatch.setattr(_native, 'Batch', _FakeCsrBatch)
    monkeypatch.setattr(_native, 'Context', _FakeCsrContext)
    return recorded


def problems_in_contexts():
    """The problems set on contexts (a batched call opens one context at most: the probe behind `last_fp8_report`)."""
    return [c for c in _Fake.calls if c[0] == 'set_problem_sparse_shape' or (c[0] == 'set_problem_sparse' and len(c[1]) == 3)]


def sparse_data(count, n=N, densities=(0.3, 0.5, 0.2, 0.4)):
    return [sc.random_csr(n, F, densities[i % len(densities)], seed=40 + i) for i in range(count)]


def test_all_csr_same_shape_opens_one_csr_batch(recorded_csr):
    models, Xs = make_models(3), sparse_data(3)
    assert len(set(X.nnz for X in Xs)) == 3
    np.random.seed(11)
    outs = nmf.fit_transform_batch(models, Xs)
    after = np.random.random()
    assert batches_opened() == [('batch', 'f64', 3, 0)] and len(outs) == 3
    assert not problems_in_contexts()
    assert [m.last_batch_size for m in models] == [3, 3, 3]
    names = _Fake.batch_calls
    assert names[0] == 'set_problem_sparse' and 'set_problem' not in names and 'upload_V' not in names
    shape = [c for c in _Fake.calls if c[0] == 'set_problem_sparse'][0][1]
    assert tuple(shape[:4]) == (N, F, K, 5) and shape[4] == [X.nnz for X in Xs]
    uploads = [c[1] for c in _Fake.calls if c[0] == 'upload_csr_rows']
    assert [u[0] for u in uploads] == [0, 1, 2]
    for (p, X), ref in zip(uploads, Xs):
        assert sp.issparse(X) and (X != ref).nnz == 0 and X.has_sorted_indices
    assert names.count('init_W') == 1 and names.count('run') == 1 and names.count('set_H') == 3
    assert names.index('init_W') > max(i for i, c in enumerate(names) if c in ('upload_csr_rows', 'set_H'))
    assert names.index('run') > names.index('init_W')
    # the initial dictionaries: drawn in list order, the stream left where the sequential calls leave it
    batched = dictionaries_set()
    _Fake.opened, _Fake.calls = [], []
    np.random.seed(11)
    for m, X in zip(make_models(3), Xs):
        m.fit_transform(X)
    assert np.random.random() == after
    sequential = dictionaries_set()
    assert not batches_opened() and len(batched) == len(sequential) == 3
    assert all(np.array_equal(a, b) for a, b in zip(batched, sequential)) and not np.array_equal(batched[0], batched[1])


@pytest.mark.parametrize('prec,resolved', [('f64', 'f64'), ('auto', 'f64'), ('f32', 'f32'), ('bf16', 'f32'), ('bf16x3', 'f32')])
def test_the_arithmetic_is_sparse_precisions(recorded_csr, prec, resolved, capsys):
    nmf.fit_transform_batch(make_models(2, precision=prec), sparse_data(2))
    assert batches_opened() == [('batch', resolved, 2, 0)]


def test_explicit_zeros_are_dropped_before_the_count(recorded_csr):
    Xs = sparse_data(2)
    Xs[1] = Xs[1].copy()
    Xs[1].data[:3] = 0.0
    nmf.fit_transform_batch(make_models(2), Xs)
    shape = [c for c in _Fake.calls if c[0] == 'set_problem_sparse'][0][1]
    assert shape[4] == [Xs[0].nnz, Xs[1].nnz - 3]


def _array_weights():
    return (make_models(2), sparse_data(2)), dict(weights=[np.ones((N, 1)), None])


SEQUENTIAL = {
    'mixed dense and sparse': lambda: ((make_models(2), [sparse_data(1)[0].toarray(), sparse_data(1)[0]]), {}),
    'unequal shapes': lambda: ((make_models(2), [sparse_data(1)[0], sparse_data(1, n=N - 1)[0]]), {}),
    'k = 513': lambda: ((make_models(2, n_components=513), sparse_data(2)), {}),
    'an X without stored entries': lambda: ((make_models(2), [sparse_data(1)[0], sp.csr_matrix((N, F))]), {}),
    'array weights': _array_weights,
    'n_components differ': lambda: ((make_models(1) + make_models(1, n_components=K + 1), sparse_data(2)), {}),
    'a device list': lambda: ((make_models(2, device=[0, 1]), sparse_data(2)), {}),
}


def control_opens_a_batch():
    """The case's neighbour without its deviation -- two CSR problems of one shape -- does open a CSR batch: what follows is
    sequential because of the deviation, not because there are no CSR batches."""
    nmf.fit_transform_batch(make_models(2), sparse_data(2))
    assert batches_opened() == [('batch', 'f64', 2, 0)]
    _Fake.opened, _Fake.calls, _Fake.batch_calls = [], [], []


@pytest.mark.parametrize('name', sorted(SEQUENTIAL))
def test_the_sequential_route(recorded_csr, name, capsys):
    control_opens_a_batch()
    (models, Xs), kw = SEQUENTIAL[name]()
    if name == 'array weights':
        with pytest.raises(ValueError):      # (weights on CSR input: `check_weights` refuses, as fit_transform does)
            nmf.fit_transform_batch(models, Xs, **kw)
        assert not batches_opened()
        return
    outs = nmf.fit_transform_batch(models, Xs, **kw)
    assert not batches_opened() and len(outs) == 2
    assert [m.last_batch_size for m in models] == [1, 1]


def test_validation_is_fit_transforms(recorded_csr):
    control_opens_a_batch()
    bad = sparse_data(1)[0].copy()
    bad.data[0] = -1.0
    with pytest.raises(ValueError) as batched:
        nmf.fit_transform_batch(make_models(2), [sparse_data(1)[0], bad])
    with pytest.raises(ValueError) as alone:
        make_models(1)[0].fit_transform(bad)
    assert str(batched.value) == str(alone.value) and not batches_opened()


# ---- DeviceDataset -----------------------------------------------------------------------------------------------------------------
NAMES = ['a', 'b', 'c']
ROWS = [np.arange(0, 120), np.arange(100, 220), np.random.RandomState(2).randint(0, 301, 120)]
KD = 3


@pytest.fixture
def dataset(recorded_csr, monkeypatch):
    monkeypatch.setattr(device_data.DeviceDataset, '_synchronize', lambda self: None)
    ds = _HostDataset(modalities(), device=0, keep_sparse=True)
    assert ds.sparse == [True] * 3
    return ds


def learners_of(ds, coefs=(1.0, 0.5, 0.3), count=3, trained=False):
    out = []
    for i in range(count):
        lr = MultimodalLearner(NAMES, ds.dims, list(coefs), KD)
        if trained:
            lr.dico = np.full((KD, CUTS[-1]), (1.0 + i) / CUTS[-1])
        out.append(lr)
    return out


def expected_nnz(which, rows_list):
    mods = modalities()
    return [int(sp.hstack([mods[w][rows] for w in which]).nnz) for rows in rows_list]


def check_gathers(which, f):
    shape = [c for c in _Fake.calls if c[0] == 'set_problem_sparse'][0][1]
    assert tuple(shape[:3]) == (120, f, KD) and shape[4] == expected_nnz(which, ROWS)
    gathers = [c[1] for c in _Fake.calls if c[0] == 'upload_csr_device_rows']
    assert [g[0] for g in gathers] == [0, 1, 2]
    for g in gathers:
        p, sources, bounds, scales, src_rows, idx_ptr, n_rows = g
        assert len(sources) == len(which) and bounds[0] == 0 and bounds[-1] == f and src_rows == 301 and n_rows == 120
        assert isinstance(idx_ptr, int)
    names = _Fake.batch_calls
    assert 'upload_csr_rows' not in names and 'upload_V_device_rows_dt' not in names and 'set_problem' not in names
    assert names.count('init_W') == 1 and names.count('run') == 1
    assert names.index('init_W') > max(i for i, c in enumerate(names) if c == 'upload_csr_device_rows')


def test_train_many_gathers_a_csr_batch_on_the_device(dataset):
    f = CUTS[-1]
    learners = learners_of(dataset)
    dataset.train_many(learners, ROWS, 4, init_dictionaries=[np.full((KD, f), 1.0 / f)] * 3)
    assert batches_opened() == [('batch', 'f64', 3, 0)] and not problems_in_contexts()
    check_gathers([0, 1, 2], f)
    assert all(lr.nmf_train.last_batch_size == 3 for lr in learners) and dataset.last_weights_route is None


def control_train_many_opens_a_batch(dataset):
    f = CUTS[-1]
    dataset.train_many(learners_of(dataset), ROWS, 4, init_dictionaries=[np.full((KD, f), 1.0 / f)] * 3)
    assert batches_opened() == [('batch', 'f64', 3, 0)]
    _Fake.opened, _Fake.calls, _Fake.batch_calls = [], [], []


def test_a_zero_coefficient_sends_train_many_sequential(dataset, capsys):
    control_train_many_opens_a_batch(dataset)
    f = CUTS[-1]
    learners = learners_of(dataset)
    learners[1].coef = [1.0, 0.0, 0.3]
    dataset.train_many(learners, ROWS, 4, init_dictionaries=[np.full((KD, f), 1.0 / f)] * 3)
    assert not batches_opened() and len(problems_in_contexts()) == 3


def test_unequal_row_counts_send_train_many_sequential(dataset):
    control_train_many_opens_a_batch(dataset)
    f = CUTS[-1]
    dataset.train_many(learners_of(dataset), [ROWS[0], ROWS[1], ROWS[2][:100]], 4, init_dictionaries=[np.full((KD, f), 1.0 / f)] * 3)
    assert not batches_opened()


def test_reconstruct_internal_multi_many_gathers_a_csr_batch(dataset):
    learners = learners_of(dataset, trained=True)
    outs = dataset.reconstruct_internal_multi_many(learners, ['a', 'c'], ROWS, 4)
    assert len(outs) == 3 and batches_opened() == [('batch', 'f64', 3, 0)]
    check_gathers([0, 2], dataset.dims[0] + dataset.dims[2])
    # the transforms run on the learners' dictionaries, which are the initial ones: one set_H per problem, all before init_W
    names = _Fake.batch_calls
    assert names.count('set_H') == 3 and names.index('init_W') > max(i for i, c in enumerate(names) if c == 'set_H')
    _Fake.opened, _Fake.calls, _Fake.batch_calls = [], [], []
    learners[2].coef = [0.0, 0.5, 0.3]
    dataset.reconstruct_internal_multi_many(learners, ['a', 'c'], ROWS, 4)
    assert not batches_opened()


def test_internal_many_gathers_a_csr_batch(dataset, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **kw: None)
    learners = learners_of(dataset, trained=True)
    evs = []
    for lr in learners:
        ev = device_data.DeviceEvaluation.__new__(device_data.DeviceEvaluation)      # (its constructor moves the dictionary to the GPU)
        ev.torch, ev.ds, ev.learner, ev.iter_test, ev.dev = torch, dataset, lr, 4, torch.device('cpu')
        ev.dico = torch.from_numpy(np.ascontiguousarray(lr.get_dico(), dtype=np.float64))
        ev.k, ev.F = ev.dico.shape
        ev.offsets = [sum(lr.dim[:i]) for i in range(len(lr.dim))]
        ev.last_weights_route = 'unset'
        evs.append(ev)
    outs = device_data.DeviceEvaluation.internal_many(evs, ['b', 'c'], ROWS)
    assert len(outs) == 3 and all(tuple(o.shape) == (120, KD) for o in outs)
    assert batches_opened() == [('batch', 'f64', 3, 0)] and not problems_in_contexts()
    check_gathers([1, 2], dataset.dims[1] + dataset.dims[2])
    names = _Fake.batch_calls
    assert names.count('set_H_device') == 6 and names.count('get_W_device') == 3
    assert all(ev.last_weights_route is None for ev in evs)


def test_a_masked_csr_selection_keeps_raising(recorded_csr, monkeypatch):
    monkeypatch.setattr(device_data.DeviceDataset, '_synchronize', lambda self: None)
    presence = [np.ones(301), None, None]
    presence[0][::7] = 0.0
    control_train_many_opens_a_batch(_HostDataset(modalities(), device=0, keep_sparse=True))
    ds = _HostDataset(modalities(), device=0, keep_sparse=True, presence=presence)
    with pytest.raises(ValueError, match='kept as CSR'):
        ds.train_many(learners_of(ds), ROWS, 4)
    assert not batches_opened()
