"""Batches without a GPU: the exports, the plan rule, `fit_transform_batch`'s route choice and its use of the global random
stream (a recording fake stands in for `_native.Batch` and `_native.Context`), and `sweep_batches`."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from multimodal_amd import _native
from multimodal_amd.device_experiment import sweep_assignment, sweep_batches
from multimodal_amd.lib import nmf
from tests import exact_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_declared_batch_symbol_is_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'klnmf_batch.h')).read()
    declared = set(re.findall(r'\bint\s+(klnmf_batch_\w+)\s*\(', header))
    assert declared == {'klnmf_batch_' + n for n in (
        'create', 'destroy', 'set_problem', 'upload_V', 'upload_V_device_rows_dt', 'set_H', 'set_H_device', 'set_W', 'init_W', 'run',
        'result', 'get_W', 'get_H', 'get_W_device', 'query')}
    assert declared == set(_native.BATCH_SIGNATURES)
    lib = _native.load()
    for name in declared:
        assert name in _native.BATCH_SIGNATURES and hasattr(lib, name), name
    assert re.search(r'#define\s+KLNMF_BATCH_MAX\s+%d\b' % _native.BATCH_MAX, header)
    assert re.search(r'#define\s+KLNMF_Q_BATCH_COUNT\s+%d\b' % _native.Q_BATCH_COUNT, header)


@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('B', [1, 2, 5, 256, 300])
def test_the_batch_plan_is_the_single_plan_for_the_batchs_share_of_the_chip(monkeypatch, prec, B):
    """The counts a batch of B takes at 256 CUs: klnmf_plan_query for max(1, 256 // B) CUs, which is exact_cases' rule."""
    monkeypatch.delenv('KLNMF_DEV', raising=False)
    cu_eff = max(1, ec.MI355X_CUS // B)
    assert cu_eff == {1: 256, 2: 128, 5: 51, 256: 1, 300: 1}[B]
    items = (_native.Q_EX_ROW_CHUNKS, _native.Q_EX_W_CHUNKS, _native.Q_EX_H_SEGMENTS, _native.Q_EX_H_FROM_SLABS)
    for n, f, k in [(15, 17, 1), (65, 65, 65), (300, 700, 17), ec.MID, (4096, 128, 16), (4096, 129, 16), (100, 16385, 33), (900, 2450, 50)]:
        got = tuple(_native.plan_query(prec, n, f, k, what, cu_count=cu_eff) for what in items)
        assert got == ec.query_regime(n, f, k, cu_eff, esize=8 if prec == 'f64' else 4), (n, f, k, B)
    if B == 1:      # B = 1 plans exactly as a context does
        assert cu_eff == ec.MI355X_CUS


# ---- fit_transform_batch: a recording fake for the batch and for the context ---------------------------------------------------------
class _Fake(object):
    """Stands in for `_native.Batch` and `_native.Context`: records what was opened and every call made on it."""
    opened = []
    calls = []
    batch_calls = []      # the names of the calls made on batches alone

    def __init__(self, precision='f64', count=None, device=0, stream=None, pooled=False):
        self.precision_name = precision
        self.precision = _native.PRECISIONS[precision]
        self.count = count
        _Fake.opened.append(('context' if count is None else 'batch', precision, count, device))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        pass

    def __getattr__(self, name):
        def method(*args, **kwargs):
            _Fake.calls.append((name, args, kwargs))
            if self.count is not None:
                _Fake.batch_calls.append(name)
            if name == 'set_problem':
                self.n, self.f, self.k = args[0], args[1], args[2]
            if name == 'set_problem_sparse':
                (self.n, self.f), self.k = args[0].shape, args[1]
            if name == 'run':
                return [([], 0, False)] * self.count if self.count is not None else ([], 0, False)
            if name == 'fp8_report':
                return {}
            if name == 'get_W':
                return np.zeros((self.n, self.k))
            if name == 'get_H':
                return np.zeros((self.k, self.f))
        return method


class _FakeBatch(_Fake):
    def __init__(self, precision, count, device=0):
        _Fake.__init__(self, precision, count, device)


@pytest.fixture
def recorded(monkeypatch):
    _Fake.opened, _Fake.calls, _Fake.batch_calls = [], [], []
    monkeypatch.setattr(_native, 'Context', _Fake)
    monkeypatch.setattr(_native, 'Batch', _FakeBatch)
    monkeypatch.setattr(nmf, '_EXACT_LOOP_REPORT', {})
    monkeypatch.delenv('KLNMF_PRECISION', raising=False)
    monkeypatch.delenv('KLNMF_DEVICES', raising=False)
    return _Fake


def batches_opened():
    return [o for o in _Fake.opened if o[0] == 'batch']


def dictionaries_set():
    """The H arguments of every set_H call, in call order (a batch's carry the problem index in front)."""
    return [c[1][-1] for c in _Fake.calls if c[0] == 'set_H' and c[1][-1].shape != (1, 1)]


N, F, K = 30, 20, 4


def make_models(count, **kw):
    args = dict(n_components=K, max_iter=5, tol=0, precision='f64', device=0)
    args.update(kw)
    return [nmf.KLdivNMF(**args) for _ in range(count)]


def make_data(count, n=N):
    rng = np.random.default_rng(3)
    return [rng.random((n, F)) for _ in range(count)]


def test_the_batched_route_and_its_random_stream(recorded):
    models = make_models(3)
    np.random.seed(11)
    outs = nmf.fit_transform_batch(models, make_data(3))
    after = np.random.random()
    assert batches_opened() == [('batch', 'f64', 3, 0)] and len(outs) == 3
    assert [m.last_batch_size for m in models] == [3, 3, 3]
    batched = dictionaries_set()
    # the sequential calls from the same seed: the same dictionaries in the same order, the stream left where they leave it
    _Fake.opened, _Fake.calls = [], []
    np.random.seed(11)
    for m, X in zip(make_models(3), make_data(3)):
        m.fit_transform(X)
    assert np.random.random() == after
    sequential = dictionaries_set()
    assert not batches_opened() and len(batched) == len(sequential) == 3
    assert all(np.array_equal(a, b) for a, b in zip(batched, sequential))
    assert not np.array_equal(batched[0], batched[1])
    # every problem got its V and its H before one init_W and one run
    names = [c[0] for c in _Fake.calls]
    assert names.count('run') == 3


def test_init_dictionaries_are_taken_and_nothing_is_drawn(recorded):
    models = make_models(2)
    H = [np.full((K, F), 1.0 / F), np.full((K, F), 2.0 / F)]
    for m, h in zip(models, H):
        m._init_dictionary = h
    np.random.seed(5)
    expected = np.random.random()
    np.random.seed(5)
    nmf.fit_transform_batch(models, make_data(2))
    assert np.random.random() == expected
    assert batches_opened() and all(a is b for a, b in zip(dictionaries_set(), H))
    names = _Fake.batch_calls
    assert names.count('init_W') == 1 and names.count('run') == 1 and names.count('upload_V') == 2 and names.count('set_H') == 2
    assert names.index('init_W') > max(i for i, c in enumerate(names) if c in ('upload_V', 'set_H')) and names.index('run') > names.index('init_W')


ROUTES = {
    'unequal shapes': lambda: (make_models(2), [make_data(1)[0], make_data(1, n=N - 1)[0]]),
    'a sparse X': lambda: (make_models(2), [make_data(1)[0], sp.csr_matrix(make_data(1)[0])]),
    'n_components differ': lambda: (make_models(1) + make_models(1, n_components=K + 1), make_data(2)),
    'tol differs': lambda: (make_models(1) + make_models(1, tol=1e-3), make_data(2)),
    'max_iter differs': lambda: (make_models(1) + make_models(1, max_iter=6), make_data(2)),
    'precision differs': lambda: (make_models(1) + make_models(1, precision='f32'), make_data(2)),
    'a 16-bit precision': lambda: (make_models(2, precision='f16'), make_data(2)),
    'a split-operand precision': lambda: (make_models(2, precision='bf16x3'), make_data(2)),
    'devices differ': lambda: (make_models(1) + make_models(1, device=1), make_data(2)),
    'a device list': lambda: (make_models(2, device=[0, 1]), make_data(2)),
}


@pytest.mark.parametrize('name', sorted(ROUTES))
def test_the_sequential_route(recorded, name, capsys):
    models, Xs = ROUTES[name]()
    outs = nmf.fit_transform_batch(models, Xs)
    assert not batches_opened() and len(outs) == 2
    assert [m.last_batch_size for m in models] == [1, 1]


@pytest.mark.parametrize('prec,resolved', [('f64', 'f64'), ('f32', 'f32'), ('auto', 'f64')])
def test_the_batched_route_by_precision(recorded, prec, resolved):
    models = make_models(2, precision=prec)
    nmf.fit_transform_batch(models, make_data(2))
    assert batches_opened() == [('batch', resolved, 2, 0)]


def test_validation_is_fit_transforms(recorded):
    with pytest.raises(ValueError) as batched:
        nmf.fit_transform_batch(make_models(2), [make_data(1)[0], -make_data(1)[0]])
    with pytest.raises(ValueError) as alone:
        make_models(1)[0].fit_transform(-make_data(1)[0])
    assert str(batched.value) == str(alone.value)
    with pytest.raises(ValueError):
        nmf.fit_transform_batch(make_models(2), make_data(3))


# ---- sweep_batches ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('world', [1, 2, 3])
@pytest.mark.parametrize('batch', [1, 2, 3, 8])
def test_sweep_batches(world, batch):
    ks, n_runs = [5, 10, 50], 7
    seen = []
    for rank in range(world):
        pairs = sweep_assignment(ks, n_runs, rank, world)
        groups = sweep_batches(pairs, batch)
        assert sorted(p for g in groups for p in g) == sorted(pairs)              # every pair in exactly one batch
        assert all(len(set(k for k, _ in g)) == 1 and 1 <= len(g) <= batch for g in groups)
        if batch == 1:
            assert [g[0] for g in groups] == pairs                                # today's order
        seen.extend(p for g in groups for p in g)
    assert sorted(seen) == [(k, r) for k in sorted(ks) for r in range(n_runs)]
