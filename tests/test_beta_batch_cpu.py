"""Beta batches without a GPU: the exports of include/klnmf_batch_beta.h, and `beta_nmf.fit_transform_batch`'s route choice, its
call order on the batch and its use of the global random stream (tests/test_batch_cpu.py's recording fakes stand in for
`_native.Batch` and `_native.Context`)."""
import numpy as np
import pytest
import scipy.sparse as sp

from multimodal_amd import _native
from multimodal_amd.lib import beta_nmf, nmf
from tests import beta_cases as bc
from tests.test_batch_cpu import _Fake, batches_opened, dictionaries_set, recorded      # noqa: F401  (the fixture)
from tests.test_batch_csr_cpu import check_header_tables, declared_in, other_headers
from tests.test_beta_cpu import N, F, K, beta_model, comparable, data, names

NEW = {'klnmf_batch_set_divergence', 'klnmf_batch_get_divergence', 'klnmf_batch_upload_weights'}
OTHERS = other_headers('klnmf_batch_beta.h')


# ---- the bindings ---------------------------------------------------------------------------------------------------------------------
def test_every_declared_beta_batch_symbol_is_bound_and_exported():
    declared = declared_in('klnmf_batch_beta.h')
    assert declared == NEW == set(_native.BATCH_BETA_SIGNATURES)
    lib = _native.load()
    for name in declared:
        assert hasattr(lib, name), name
    for header in OTHERS:
        assert not (declared & declared_in(header)), header
    for method in ('set_divergence', 'get_divergence', 'upload_weights'):
        assert callable(getattr(_native.Batch, method))


def test_the_other_headers_declare_what_they_declared():
    check_header_tables()                # (and NEW is this header's own table: the test above)


# ---- the routing ----------------------------------------------------------------------------------------------------------------------
def datas(count):
    return [data() + 0.25 * p for p in range(count)]


def call_index(name, last=False):
    at = [i for i, c in enumerate(_Fake.batch_calls) if c == name]
    return at[-1] if last else at[0]


@pytest.mark.parametrize('prec,resolved', [('f64', 'f64'), ('auto', 'f64'), ('f32', 'f32'), ('f16', 'f32')])
def test_same_beta_models_open_one_batch_and_name_the_cost_once(recorded, prec, resolved):
    models = [beta_model(0.5, precision=prec) for _ in range(3)]
    outs = beta_nmf.fit_transform_batch(models, datas(3))
    assert batches_opened() == [('batch', resolved, 3, 0)] and len(outs) == 3
    assert [m.last_batch_size for m in models] == [3, 3, 3] and [m.last_weights_route for m in models] == [None] * 3
    assert [c[1] for c in _Fake.calls if c[0] == 'set_divergence'] == [(0.5,)]
    order = _Fake.batch_calls
    assert order.count('set_problem') == 1 and order.count('upload_V') == 3 and order.count('set_H') == 3
    assert order.count('init_W') == 1 and order.count('run') == 1 and 'upload_weights' not in order
    div = call_index('set_divergence')
    assert call_index('set_problem') < call_index('upload_V', last=True) < div
    assert div < call_index('set_H') <= call_index('set_H', last=True) < call_index('init_W') < call_index('run')


def test_array_weights_become_upload_weights_calls(recorded):
    models = [beta_model(2.0) for _ in range(3)]
    Om = bc.weights_of(N, F, seed=1)
    col = (np.arange(N) % 3 != 0).astype(float)[:, None]
    beta_nmf.fit_transform_batch(models, datas(3), weights=[Om, 1.0, col])
    assert batches_opened() == [('batch', 'f64', 3, 0)]
    ups = [c for c in _Fake.calls if c[0] == 'upload_weights']
    assert [c[1][0] for c in ups] == [0, 2]                                     # the problem index in front; the scalar: no upload
    assert np.array_equal(ups[0][1][1], Om) and np.array_equal(ups[1][1][1], np.broadcast_to(col, (N, F)))
    assert 'upload_presence' not in _Fake.batch_calls
    assert call_index('set_divergence') < call_index('upload_weights') <= call_index('upload_weights', last=True) < call_index('set_H')
    assert [m.last_weights_route for m in models] == ['array'] * 3
    # weights the single call refuses are refused by the batched call, with its words, before a batch opens
    _Fake.opened, _Fake.calls, _Fake.batch_calls = [], [], []
    with pytest.raises(ValueError) as batched:
        beta_nmf.fit_transform_batch([beta_model(2.0), beta_model(2.0)], datas(2), weights=[-Om, None])
    with pytest.raises(ValueError) as alone:
        beta_model(2.0).fit_transform(data(), weights=-Om)
    assert str(batched.value) == str(alone.value) and not batches_opened()


def sequential_calls(make_models, Xs, weights=None):
    _Fake.opened, _Fake.calls, _Fake.batch_calls = [], [], []
    np.random.seed(7)
    models = make_models()
    for i, (m, X) in enumerate(zip(models, Xs)):
        if weights is None:
            m.fit_transform(X)
        else:
            m.fit_transform(X, weights=weights[i])
    return list(_Fake.opened), comparable(_Fake.calls), [m.last_weights_route for m in models]


ROUTES = {
    'mixed betas': lambda: [beta_model(2.0), beta_model(0.5)],
    'a KL model among them': lambda: [nmf.KLdivNMF(n_components=K, max_iter=5, tol=0, precision='f64', device=0), beta_model(0.5)],
    'n_components differ': lambda: [beta_model(2.0), beta_model(2.0, n_components=K + 1)],
    'tol differs': lambda: [beta_model(2.0), beta_model(2.0, tol=1e-3)],
    'max_iter differs': lambda: [beta_model(2.0), beta_model(2.0, max_iter=6)],
    'precision differs': lambda: [beta_model(2.0), beta_model(2.0, precision='f32')],
    'devices differ': lambda: [beta_model(2.0), beta_model(2.0, device=1)],
    'a device list': lambda: [beta_model(2.0, device=[0, 1]), beta_model(2.0, device=[0, 1])],
}


@pytest.mark.parametrize('name', sorted(ROUTES))
def test_the_sequential_route_makes_todays_calls(recorded, name):
    Xs = datas(2)
    col = (np.arange(N) % 3 != 0).astype(float)[:, None]
    nmf._NOTED.clear()
    expected = sequential_calls(ROUTES[name], Xs, weights=[col, None])
    nmf._NOTED.clear()
    _Fake.opened, _Fake.calls, _Fake.batch_calls = [], [], []
    np.random.seed(7)
    models = ROUTES[name]()
    outs = beta_nmf.fit_transform_batch(models, Xs, weights=[col, None])
    assert not batches_opened() and len(outs) == 2 and [m.last_batch_size for m in models] == [1, 1]
    assert (list(_Fake.opened), comparable(_Fake.calls), [m.last_weights_route for m in models]) == expected


def test_unequal_shapes_run_one_after_another(recorded):
    Xs = [data(), data()[:N - 1]]
    expected = sequential_calls(lambda: [beta_model(2.0), beta_model(2.0)], Xs)
    _Fake.opened, _Fake.calls, _Fake.batch_calls = [], [], []
    np.random.seed(7)
    models = [beta_model(2.0), beta_model(2.0)]
    beta_nmf.fit_transform_batch(models, Xs)
    assert not batches_opened() and [m.last_batch_size for m in models] == [1, 1]
    assert (list(_Fake.opened), comparable(_Fake.calls)) == expected[:2]


def test_sparse_xs_raise_as_fit_transform_does(recorded):
    sparse = [sp.csr_matrix(X) for X in datas(2)]
    with pytest.raises(ValueError, match='scipy-sparse input'):
        beta_nmf.fit_transform_batch([beta_model(2.0), beta_model(2.0)], sparse)
    assert not _Fake.opened and not _Fake.calls
    # one sparse X among dense ones: the first model runs as today, the second raises as today
    with pytest.raises(ValueError, match='scipy-sparse input'):
        beta_nmf.fit_transform_batch([beta_model(2.0), beta_model(2.0)], [data(), sparse[1]])
    assert _Fake.opened == [('context', 'f64', None, 0)] and not batches_opened()


def test_beta_1_delegates(recorded, monkeypatch):
    seen = []
    real = nmf.fit_transform_batch

    def recording(models, Xs, weights=None, _fit=True, return_errors=False):
        seen.append((len(models), weights, _fit, return_errors))
        return real(models, Xs, weights=weights, _fit=_fit, return_errors=return_errors)
    monkeypatch.setattr(nmf, 'fit_transform_batch', recording)
    models = [beta_model(1.0), beta_model(1.0)]
    outs = beta_nmf.fit_transform_batch(models, datas(2), return_errors=True)
    assert seen == [(2, None, True, True)] and len(outs) == 2
    assert batches_opened() == [('batch', 'f64', 2, 0)] and 'set_divergence' not in names()
    assert [m.last_batch_size for m in models] == [2, 2]


def test_the_numpy_stream_is_consumed_as_by_the_sequential_calls(recorded):
    np.random.seed(11)
    beta_nmf.fit_transform_batch([beta_model(0.5) for _ in range(3)], datas(3))
    after = np.random.random()
    batched = dictionaries_set()
    assert batches_opened() == [('batch', 'f64', 3, 0)]
    _Fake.opened, _Fake.calls, _Fake.batch_calls = [], [], []
    np.random.seed(11)
    for m, X in zip([beta_model(0.5) for _ in range(3)], datas(3)):
        m.fit_transform(X)
    assert np.random.random() == after
    sequential = dictionaries_set()
    assert not batches_opened() and len(batched) == len(sequential) == 3
    assert all(np.array_equal(a, b) for a, b in zip(batched, sequential))
    assert not np.array_equal(batched[0], batched[1])


def test_a_transform_sets_the_models_dictionaries_behind_init_W(recorded):
    models = [beta_model(2.0) for _ in range(2)]
    comps = [np.full((K, F), (p + 1.0) / F) for p in range(2)]
    for m, h in zip(models, comps):
        m.components_ = h
    beta_nmf.fit_transform_batch(models, datas(2), _fit=False)
    set_H = [c for c in _Fake.calls if c[0] == 'set_H' and len(c[1]) == 2]      # (the batch's: the problem index in front)
    assert len(set_H) == 4 and all(a[1][1] is h for a, h in zip(set_H[2:], comps))
    assert [c for c in _Fake.calls if c[0] == 'run'][0][1][1] is False
    assert all(m.components_ is h for m, h in zip(models, comps))


def test_nmf_fit_transform_batch_still_opens_no_batch_for_beta_models(recorded):
    models = [beta_model(2.0), beta_model(2.0)]
    outs = nmf.fit_transform_batch(models, datas(2))
    assert not batches_opened() and len(outs) == 2 and [m.last_batch_size for m in models] == [1, 1]
    assert _Fake.opened == [('context', 'f64', None, 0)] * 2
    assert nmf.batch_precision(models, N, F) is None


def test_the_hook_is_optional_and_off_by_default(recorded):
    """`nmf.fit_uploaded_batch` without the hook: every dictionary right behind its problem's upload, as before."""
    models = [nmf.KLdivNMF(n_components=K, max_iter=5, tol=0, precision='f64', device=0) for _ in range(2)]
    nmf.fit_transform_batch(models, datas(2))
    assert _Fake.batch_calls[:6] == ['set_problem', 'upload_V', 'set_H', 'upload_V', 'set_H', 'init_W']
