"""Masked batches without a GPU: the exports of include/klnmf_batch_mask.h, `fit_transform_batch`'s route choice with `weights`
and its use of the global random stream (the recording fake of tests/test_batch_cpu.py stands in for `_native.Batch` and
`_native.Context`), `batch_precision(weighted=True)`, and `DeviceDataset._batch_route` on a masked selection."""
import os
import re

import numpy as np
import pytest

from multimodal_amd import _native
from multimodal_amd.lib import nmf
from tests.test_batch_cpu import F, K, N, _Fake, batches_opened, dictionaries_set, make_data, make_models, recorded  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_in(header):
    text = open(os.path.join(ROOT, 'include', header)).read()
    return {name: args for name, args in re.findall(r'\bint\s+(klnmf_\w+)\s*\(([^;]*?)\)\s*;', text, flags=re.S)}


def test_every_declared_mask_symbol_is_bound_and_exported():
    declared = declared_in('klnmf_batch_mask.h')
    assert set(declared) == {'klnmf_batch_upload_presence', 'klnmf_batch_upload_presence_device_rows', 'klnmf_batch_clear_presence'}
    assert set(declared) == set(_native.BATCH_MASK_SIGNATURES)
    lib = _native.load()
    for name, args in declared.items():
        restype, argtypes = _native.BATCH_MASK_SIGNATURES[name]
        assert len(argtypes) == len(args.split(',')), name
        fn = getattr(lib, name)          # (AttributeError: not exported)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_the_three_headers_declare_disjoint_symbols():
    mask, batch, core = (set(declared_in(h)) for h in ('klnmf_batch_mask.h', 'klnmf_batch.h', 'klnmf.h'))
    assert mask and not (mask & batch) and not (mask & core) and not (batch & core)
    assert not set(_native.BATCH_MASK_SIGNATURES) & (set(_native.BATCH_SIGNATURES) | set(_native.SIGNATURES))
    # the item the batch query learnt is klnmf.h's own
    assert re.search(r'#define\s+KLNMF_Q_PRESENCE\s+%d\b' % _native.Q_PRESENCE, open(os.path.join(ROOT, 'include', 'klnmf.h')).read())


def presence_columns(count, n=N):
    rng = np.random.default_rng(8)
    return [(rng.random((n, 1)) < 0.7).astype(np.float64) for _ in range(count)]


def calls_named(name):
    return [c for c in _Fake.calls if c[0] == name]


def test_presence_routed_weights_open_one_batch_and_upload_a_mask_per_problem(recorded):
    models, ws = make_models(3), presence_columns(3)
    np.random.seed(11)
    outs = nmf.fit_transform_batch(models, make_data(3), weights=ws)
    after = np.random.random()
    assert batches_opened() == [('batch', 'f64', 3, 0)] and len(outs) == 3
    assert [m.last_batch_size for m in models] == [3, 3, 3] and [m.last_weights_route for m in models] == ['presence'] * 3
    ups = calls_named('upload_presence')
    assert [c[1][0] for c in ups] == [0, 1, 2]
    for (_, args, _), w in zip(ups, ws):
        assert np.array_equal(args[1], w) and list(args[2]) == [0, F]
    names = _Fake.batch_calls
    assert names.count('init_W') == 1 and names.count('run') == 1 and names.count('upload_V') == 3
    assert names.index('init_W') > max(i for i, c in enumerate(names) if c in ('upload_V', 'upload_presence', 'set_H'))
    batched = dictionaries_set()
    # the sequential calls from the same seed: the same dictionaries in the same order, the stream left where they leave it
    _Fake.opened, _Fake.calls = [], []
    np.random.seed(11)
    for m, X, w in zip(make_models(3), make_data(3), ws):
        m.fit_transform(X, weights=w)
        assert m.last_weights_route == 'presence'
    assert np.random.random() == after
    sequential = dictionaries_set()
    assert not batches_opened() and len(batched) == len(sequential) == 3
    assert all(np.array_equal(a, b) for a, b in zip(batched, sequential))


def test_a_model_without_an_array_rides_the_masked_batch_on_ones(recorded):
    models, ws = make_models(3), presence_columns(3)
    nmf.fit_transform_batch(models, make_data(3), weights=[ws[0], None, 1.])
    assert batches_opened() == [('batch', 'f64', 3, 0)]
    ups = calls_named('upload_presence')
    assert len(ups) == 3 and np.array_equal(ups[0][1][1], ws[0])
    assert all(np.array_equal(c[1][1], np.ones((N, 1))) for c in ups[1:])


def test_scalar_weights_are_the_unweighted_batch(recorded):
    models = make_models(2)
    nmf.fit_transform_batch(models, make_data(2), weights=[1., None])
    assert batches_opened() == [('batch', 'f64', 2, 0)] and not calls_named('upload_presence')
    assert [m.last_weights_route for m in models] == [None, None]


@pytest.mark.parametrize('other', ['full', 'row'], ids=['an n x f array', 'a (1, f) row'])
def test_one_array_routed_entry_runs_sequentially(recorded, other):
    models, ws = make_models(3), presence_columns(3)
    ws[1] = np.ones((N, F)) if other == 'full' else np.ones((1, F))
    np.random.seed(4)
    outs = nmf.fit_transform_batch(models, make_data(3), weights=ws)
    after = np.random.random()
    assert not batches_opened() and len(outs) == 3
    assert [m.last_batch_size for m in models] == [1, 1, 1]
    assert [m.last_weights_route for m in models] == ['presence', 'array', 'presence']
    assert len(calls_named('upload_weights')) == 3          # (the context binding routes col_bounds= to klnmf_upload_presence itself)
    np.random.seed(4)
    for m, X, w in zip(make_models(3), make_data(3), ws):
        m.fit_transform(X, weights=w)
    assert np.random.random() == after


def test_weights_are_validated_as_fit_transform_validates_them(recorded):
    ws = presence_columns(2)
    ws[1] = -ws[1] - 1.0
    with pytest.raises(ValueError) as batched:
        nmf.fit_transform_batch(make_models(2), make_data(2), weights=ws)
    with pytest.raises(ValueError) as alone:
        make_models(1)[0].fit_transform(make_data(1)[0], weights=ws[1])
    assert str(batched.value) == str(alone.value) and not batches_opened()
    with pytest.raises(ValueError):
        nmf.fit_transform_batch(make_models(2), make_data(2), weights=ws[:1])


@pytest.mark.parametrize('prec,resolved', [('auto', 'f64'), ('f64', 'f64'), ('f32', 'f32'), ('f16', 'f32'), ('bf16x3', 'f32')])
def test_batch_precision_of_a_masked_batch_is_the_weighted_precision(recorded, prec, resolved, capsys):
    models = make_models(2, precision=prec)
    assert nmf.batch_precision(models, N, F, weighted=True) == resolved == nmf.weighted_precision(prec)
    # the same models, unmasked: what `resolve_precision` names, or no batch at all
    plain = nmf.batch_precision(models, N, F)
    assert plain == ({'auto': 'f64', 'f64': 'f64', 'f32': 'f32'}.get(prec))
    # and the conditions on the models hold for a masked batch too
    assert nmf.batch_precision(make_models(1) + make_models(1, tol=1e-3), N, F, weighted=True) is None
    assert nmf.batch_precision(make_models(2, device=[0, 1]), N, F, weighted=True) is None
    nmf.fit_transform_batch(models, make_data(2), weights=presence_columns(2))
    assert batches_opened() == [('batch', resolved, 2, 0)]


# ---- DeviceDataset: the route of a masked selection --------------------------------------------------------------------------------
class _Tensor(object):
    """What `DeviceDataset` asks of a device tensor, on a numpy array."""

    def __init__(self, a):
        self.a = a
        self.shape = a.shape

    def numel(self):
        return self.a.size

    def element_size(self):
        return self.a.itemsize

    def max(self):
        return self

    def item(self):
        return self.a.max()

    def data_ptr(self):
        return self.a.ctypes.data

    def stride(self, i):
        return self.a.strides[i] // self.a.itemsize


def host_dataset(monkeypatch, mats, presence, keep_sparse=False):
    from multimodal_amd import device_data
    monkeypatch.setattr(device_data.DeviceDataset, '_to_device', lambda self, a: _Tensor(np.ascontiguousarray(a)))
    monkeypatch.setattr(device_data.DeviceDataset, '_synchronize', lambda self: None)
    return device_data.DeviceDataset(mats, device=0, keep_sparse=keep_sparse, presence=presence)


def test_a_masked_selection_takes_the_batched_route_and_gathers_its_rows_of_the_mask(recorded, monkeypatch):
    import scipy.sparse as sp
    from multimodal_amd.learner import MultimodalLearner
    rng = np.random.default_rng(2)
    n = 40
    mats = [rng.random((n, 6)), rng.random((n, 9))]
    absent = (rng.random(n) < 0.7).astype(np.float64)
    ds = host_dataset(monkeypatch, mats, [None, absent])
    rows_list = [list(range(0, 20)), list(range(10, 30)), list(range(20, 40))]
    models = make_models(3, n_components=3)
    assert ds._batch_route([0, 1], rows_list, models, 15) == 'f64'
    assert ds._batch_route([0], rows_list, models, 6) == 'f64'                       # (an unmasked selection: as before)
    assert ds._batch_route([0, 1], [rows_list[0], rows_list[1][:5]], models, 15) is None
    learners = [MultimodalLearner(['a', 'b'], [6, 9], [1.0, 0.5], 3) for _ in range(3)]
    ds.train_many(learners, rows_list, 5, init_dictionaries=[np.full((3, 15), 1.0 / 15)] * 3)
    assert batches_opened() == [('batch', 'f64', 3, 0)]
    assert ds.last_weights_route == 'presence' and all(l.nmf_train.last_weights_route == 'presence' for l in learners)
    assert all(l.nmf_train.last_batch_size == 3 for l in learners)
    gathers = calls_named('upload_presence_device_rows')
    assert [c[1][0] for c in gathers] == [0, 1, 2]
    for (_, args, _) in gathers:
        # (p, mask pointer, f64, source rows, ld, index pointer, rows, source columns, bounds)
        assert args[2] is True and args[3] == n and args[6] == 20 and list(args[7]) == [-1, 1] and list(args[8]) == [0, 6, 15]
    names = _Fake.batch_calls
    assert names.index('init_W') > max(i for i, c in enumerate(names) if c == 'upload_presence_device_rows')
    # the transforms on the masked modality alone, and on the unmasked one
    _Fake.opened, _Fake.calls, _Fake.batch_calls = [], [], []
    for l in learners:
        l.dico = np.full((3, 15), 1.0 / 15)
    ds.reconstruct_internal_multi_many(learners, ['b'], rows_list, 5)
    assert batches_opened() == [('batch', 'f64', 3, 0)] and ds.last_weights_route == 'presence'
    assert all(list(c[1][7]) == [1] and list(c[1][8]) == [0, 9] for c in calls_named('upload_presence_device_rows'))
    _Fake.opened, _Fake.calls, _Fake.batch_calls = [], [], []
    ds.reconstruct_internal_multi_many(learners, ['a'], rows_list, 5)
    assert batches_opened() == [('batch', 'f64', 3, 0)] and ds.last_weights_route is None
    assert not calls_named('upload_presence_device_rows')
    # a masked selection that includes a CSR modality: the ValueError of the single calls
    ds = host_dataset(monkeypatch, [sp.csr_matrix(mats[0]), mats[1]], [None, absent], keep_sparse=True)
    with pytest.raises(ValueError, match='kept as CSR'):
        ds._batch_route([0, 1], rows_list, models, 15)
    with pytest.raises(ValueError, match='kept as CSR'):
        ds.train_many(learners, rows_list, 5)
