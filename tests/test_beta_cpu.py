"""The beta-divergence cost without a GPU: the fp64 restatement's own properties (tests/beta_cases.py), the exports of
include/klnmf_beta.h, and -- with test_batch_cpu's recording fake standing in for `_native.Context` -- the route `BetaNMF`,
`MultimodalLearner(beta=...)` and `fit_coefficients(beta=...)` take."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from multimodal_amd import _native
from multimodal_amd import device_data
from multimodal_amd.learner import MultimodalLearner, fit_coefficients
from multimodal_amd.lib import nmf
from tests import beta_cases as bc
from tests import exact_cases as ec
from tests.test_batch_cpu import _Fake, recorded      # noqa: F401  (the fixture)
from tests.test_batch_csr_cpu import declared_in

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def problem(n, f, k):
    V = ec.data(n, f, seed=n + 7 * f + 13 * k, zero_row=n // 2, zero_col=f // 3)
    _, H = ec.factors(n, f, k, seed=k + 1)
    return V, H


@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'weighted'])
@pytest.mark.parametrize('shape', bc.PROPERTY_SHAPES, ids=ec.case_id)
def test_the_loss_record_of_the_restatement_never_rises(shape, weighted):
    """12 iterations on gamma(1, 1) + 0.05 data with an all-zero row and column, summed over the kernels' chunks at 256 CUs: no
    loss exceeds its predecessor by more than 1e-12 relative, and the factors stay finite -- for every beta, with and without
    weights of which 30 % are zero."""
    n, f, k = shape
    V, H0 = problem(n, f, k)
    Om = bc.weights_of(n, f, seed=5) if weighted else None
    _, kchunk, _, wchunk, _, _ = ec.exact_regime(n, f, k, ec.MI355X_CUS)
    for beta in bc.PROPERTY_BETAS:
        W, H, losses = bc.ref_fit(V, H0, 12, beta, Om=Om, kchunk=kchunk, wchunk=wchunk)
        assert np.all(np.isfinite(W)) and np.all(np.isfinite(H)) and np.all(np.isfinite(losses)), beta
        assert bc.worst_rise(losses) <= bc.DESCENT_RISE, (beta, bc.worst_rise(losses))
        assert losses[-1] < losses[0], beta
        assert np.abs(H.sum(axis=1) - 1.0).max() <= 1e-15 * f, beta


def test_the_normalisation_leaves_the_product_alone():
    n, f, k = 65, 65, 65
    V, H0 = problem(n, f, k)
    W0 = ec.ref_init_W(V, H0)
    for beta in bc.PROPERTY_BETAS:
        Ws, Hn, Hu = bc.ref_H_step(V, W0, H0, beta)
        assert np.allclose(Ws.dot(Hn), W0.dot(Hu), rtol=1e-12, atol=0.0), beta


@pytest.mark.parametrize('special', [2.0, 0.0])
def test_the_general_formula_brackets_the_special_cases(special):
    """d_beta at beta = special -+ 1e-6 by the general formula lies on either side of the special case's own formula, up to the
    general formula's rounding and a curvature allowance (h^2 = 1e-12 times the terms and their squared logarithms: where d_beta
    is stationary in beta both neighbours lie on one side), and within 1e-5 of it -- the assertion that binds."""
    rng = np.random.default_rng(1)
    x = rng.gamma(1.0, 1.0, 2000) + 0.05
    y = rng.gamma(1.0, 1.0, 2000) + 0.05
    d = bc.beta_div(x, y, special)
    lo, hi = bc.general_div(x, y, special - 1e-6), bc.general_div(x, y, special + 1e-6)
    scale = np.maximum(d, 1e-3)
    # the general formula's own rounding: its three terms (x^beta, |beta - 1| y^beta, |beta| x y^(beta-1)) cancel, each carrying a few
    # ulps of 2^-52, over a denominator of |beta (beta - 1)| -- 1e-6 beside beta = 0; 8 ulps per term
    # -- and, where d_beta is stationary in beta, the curvature over the step: h^2 = 1e-12 times the terms and their squared logarithms
    def rounding(b):
        terms = x ** b + abs(b - 1.0) * y ** b + abs(b) * x * y ** (b - 1.0)
        return 8 * 2.0 ** -52 * terms / abs(b * (b - 1.0)) + 1e-12 * terms * (1.0 + np.log(x) ** 2 + np.log(y) ** 2)
    slack = np.maximum(rounding(special - 1e-6), rounding(special + 1e-6))
    assert np.all(np.minimum(lo, hi) - slack <= d) and np.all(d <= np.maximum(lo, hi) + slack)
    assert np.all(np.abs(lo - d) <= 1e-5 * scale) and np.all(np.abs(hi - d) <= 1e-5 * scale)


def test_the_cost_is_nonnegative_and_zero_at_an_exact_fit():
    rng = np.random.default_rng(2)
    W, H = ec.factors(40, 30, 5, seed=3)
    V = rng.gamma(1.0, 1.0, (40, 30)) + 0.05
    Om = bc.weights_of(40, 30, seed=4)
    for beta in bc.PROPERTY_BETAS:
        x, y = V + bc.EPS, W.dot(H) + bc.EPS
        assert np.all(bc.beta_div(x, y, beta) >= 0.0), beta
        assert bc.cost(V, W, H, beta) > 0.0 and bc.cost(V, W, H, beta, Om) > 0.0
        exact = bc.cost(W.dot(H), W, H, beta)
        assert abs(exact) <= 1e-13 * float(((W.dot(H) + bc.EPS) ** beta).sum()), (beta, exact)
        if beta in (0.0, 2.0):
            assert exact == 0.0
    assert [bc.gamma_of(b) for b in (-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0)] == [1 / 3.0, 0.5, 1 / 1.5, 1.0, 1.0, 1.0, 0.5]


def test_a_zero_weight_hides_the_entry():
    V, H0 = problem(15, 17, 1)
    Om = bc.weights_of(15, 17, seed=6, zero_row=3)
    V2 = V.copy()
    V2[Om == 0] += 7.0
    W0 = ec.ref_init_W(V, H0)      # (the start W0 = V.H0^T is unweighted: both runs get the same one)
    for beta in bc.BETAS:
        ia, ib = bc.ref_iteration(V, W0, H0, beta, Om), bc.ref_iteration(V2, W0, H0, beta, Om)
        assert ia[0] == ib[0] and np.array_equal(ia[1], ib[1]) and np.array_equal(ia[2], ib[2]), beta
        assert np.array_equal(bc.ref_W_step(V, W0, H0, beta, Om)[1][3], W0[3])      # a row of zero weights keeps its W


# ---- the bindings ---------------------------------------------------------------------------------------------------------------------
def test_every_declared_beta_symbol_is_bound_and_exported():
    declared = declared_in('klnmf_beta.h')
    assert declared == {'klnmf_set_divergence', 'klnmf_get_divergence', 'klnmf_beta_loss', 'klnmf_beta_step'}
    assert declared == set(_native.BETA_SIGNATURES)
    lib = _native.load()
    for name in declared:
        assert hasattr(lib, name), name
    others = [declared_in(h) for h in ('klnmf.h', 'klnmf_batch.h', 'klnmf_batch_mask.h', 'klnmf_batch_csr.h')]
    assert [len(s) for s in others] == [79, len(_native.BATCH_SIGNATURES), len(_native.BATCH_MASK_SIGNATURES),
                                        len(_native.BATCH_CSR_SIGNATURES)]
    assert len(_native.SIGNATURES) == 79 and not (declared & set(_native.SIGNATURES))
    for other in others:
        assert not (declared & other)
    header = open(os.path.join(ROOT, 'include', 'klnmf_beta.h')).read()
    assert header.count('nmf.py:293') >= 4 and header.count('the reference has no counterpart') >= 4
    for doc in ('README.md', 'INTEGRATION.md', 'DESIGN.md'):
        text = open(os.path.join(ROOT, doc)).read()
        assert 'klnmf_beta.h' in text and '4 exports' in text, doc


# ---- the routing ----------------------------------------------------------------------------------------------------------------------
N, F, K = 30, 20, 4


def data():
    return np.random.default_rng(3).random((N, F)) + 0.01


def beta_model(beta, **kw):
    from multimodal_amd.lib import BetaNMF
    args = dict(n_components=K, max_iter=5, tol=0, precision='f64', device=0)
    args.update(kw)
    return BetaNMF(beta=beta, **args)


def names():
    return [c[0] for c in _Fake.calls]


def comparable(calls):
    out = []
    for name, args, kwargs in calls:
        out.append((name, [a.tolist() if isinstance(a, np.ndarray) else a for a in args], sorted(kwargs)))
    return out


@pytest.mark.parametrize('kind', ['dense', 'weighted', 'presence', 'csr'])
def test_beta_1_makes_exactly_kldivnmfs_calls(recorded, kind):
    X = data()
    kw = {}
    if kind == 'weighted':
        kw['weights'] = bc.weights_of(N, F, seed=1)
    if kind == 'presence':
        kw['weights'] = (np.arange(N) % 3 != 0).astype(float)[:, None]
    if kind == 'csr':
        X = sp.csr_matrix(X * (X > 0.5))
    got = []
    for model in (nmf.KLdivNMF(n_components=K, max_iter=5, tol=0, precision='f64', device=0), beta_model(1.0)):
        _Fake.opened, _Fake.calls = [], []
        np.random.seed(4)
        model.fit_transform(X, **kw)
        model.transform(X, **kw)
        model.error(X, np.ones((N, K)), **kw)
        got.append((list(_Fake.opened), comparable(_Fake.calls), model.last_weights_route))
    assert got[0][0] == got[1][0] and got[0][2] == got[1][2]
    assert [c[0] for c in got[0][1]] == [c[0] for c in got[1][1]]
    assert 'set_divergence' not in [c[0] for c in got[1][1]]
    if kind != 'csr':
        assert got[0][1] == got[1][1]
    assert got[1][2] == {'dense': None, 'weighted': 'array', 'presence': 'presence', 'csr': None}[kind]


@pytest.mark.parametrize('prec,resolved', [('f64', 'f64'), ('auto', 'f64'), ('f32', 'f32'), ('bf16', 'f32'), ('f16', 'f32'),
                                           ('bf16x3', 'f32'), ('f16x3', 'f32')])
def test_beta_opens_an_exact_context_and_names_the_cost_behind_the_uploads(recorded, prec, resolved, capsys):
    nmf._NOTED.clear()
    for _ in range(2):
        _Fake.opened, _Fake.calls = [], []
        model = beta_model(0.5, precision=prec)
        model.fit_transform(data(), weights=bc.weights_of(N, F, seed=1))
        assert _Fake.opened == [('context', resolved, None, 0)]
        order = names()
        div = [c for c in _Fake.calls if c[0] == 'set_divergence']
        assert len(div) == 1 and div[0][1] == (0.5,)
        i = order.index('set_divergence')
        assert i > max(j for j, c in enumerate(order) if c in ('upload_blocks', 'upload_weights', 'set_problem'))
        assert i < order.index('set_H') < order.index('init_W') < order.index('run')
        assert model.last_weights_route == 'array'
    err = capsys.readouterr().err
    note = "BetaNMF: beta != 1 with precision=%r runs on the fp32 beta kernels" % prec
    assert err.count(note) == (0 if prec in ('f64', 'auto', 'f32') else 1)
    assert 'KLdivNMF: weights with precision' not in err


def test_a_presence_column_runs_the_array_route(recorded):
    model = beta_model(2.0)
    col = (np.arange(N) % 3 != 0).astype(float)[:, None]
    model.fit_transform(data(), weights=col)
    assert model.last_weights_route == 'array'
    assert 'upload_presence' not in names()
    up = [c for c in _Fake.calls if c[0] == 'upload_weights']
    assert len(up) == 1 and up[0][1][0].shape == (N, F) and 'col_bounds' not in up[0][2]
    model.fit_transform(data())
    assert model.last_weights_route is None
    # transform and error name the cost too
    _Fake.calls = []
    model.transform(data())
    assert names().count('set_divergence') == 1 and 'run' in names()
    _Fake.calls = []
    model.error(data(), np.ones((N, K)), weights=col)
    assert names().index('set_divergence') > names().index('upload_weights') and names()[-1] == 'beta_loss'
    assert 'error' not in names()


def test_a_device_list_runs_on_its_first_device_and_says_so_once(recorded, capsys):
    nmf._NOTED.clear()
    for _ in range(2):
        _Fake.opened = []
        beta_model(2.0, device=[1, 0]).fit_transform(data())
        assert _Fake.opened == [('context', 'f64', None, 1)]
    err = capsys.readouterr().err
    assert err.count('BetaNMF: a beta != 1 fit runs on one device (1)') == 1 and 'KLdivNMF: a weighted fit' not in err


def test_sparse_input_raises_before_any_upload(recorded):
    X = sp.csr_matrix(data())
    model = beta_model(0.0)
    for call in (lambda: model.fit_transform(X), lambda: model.error(X, np.ones((N, K)), H=np.ones((K, F)))):
        with pytest.raises(ValueError, match='scipy-sparse input'):
            call()
    assert not _Fake.opened and not _Fake.calls
    with pytest.raises(ValueError, match='finite'):
        beta_model(float('nan'))


def test_update_refuses_another_eps_before_any_upload(recorded):
    """The beta cost is defined with eps = 1e-8: `_update` with another one raises instead of ignoring it."""
    model = beta_model(0.5)
    model.components_ = np.ones((K, F))
    with pytest.raises(ValueError, match='fixed eps'):
        model._update(data(), np.ones((N, K)), eps=1e-6)
    assert not _Fake.opened and not _Fake.calls


def test_fit_transform_batch_runs_beta_models_one_after_another(recorded, monkeypatch):
    """The batch kernels run the KL cost alone: models with beta != 1 never open a batch -- each runs its own `fit_transform`,
    naming its cost to its context -- and scipy-sparse Xs raise as `BetaNMF.fit_transform` does.  beta = 1 batches as KLdivNMF."""
    from tests.test_batch_cpu import batches_opened
    Xs = [data(), data() + 0.5]
    models = [beta_model(2.0), beta_model(2.0)]
    outs = nmf.fit_transform_batch(models, Xs)
    assert not batches_opened() and len(outs) == 2 and [m.last_batch_size for m in models] == [1, 1]
    assert _Fake.opened == [('context', 'f64', None, 0)] * 2
    assert [c[1] for c in _Fake.calls if c[0] == 'set_divergence'] == [(2.0,), (2.0,)] and names().count('run') == 2
    # one beta model among KL models sends all of them sequential; presence columns take the array route of each beta model
    _Fake.opened, _Fake.calls = [], []
    models = [nmf.KLdivNMF(n_components=K, max_iter=5, tol=0, precision='f64', device=0), beta_model(0.5)]
    col = (np.arange(N) % 3 != 0).astype(float)[:, None]
    nmf.fit_transform_batch(models, Xs, weights=[col, col])
    assert not batches_opened() and [m.last_weights_route for m in models] == ['presence', 'array']
    assert [c[1] for c in _Fake.calls if c[0] == 'set_divergence'] == [(0.5,)]
    # CSR
    _Fake.opened, _Fake.calls = [], []
    sparse = [sp.csr_matrix(X) for X in Xs]
    with pytest.raises(ValueError, match='scipy-sparse input'):
        nmf.fit_transform_batch([beta_model(2.0), beta_model(2.0)], sparse)
    assert not _Fake.opened and not _Fake.calls
    # the control: beta = 1 models are KLdivNMF to the batch too
    nmf.fit_transform_batch([beta_model(1.0), beta_model(1.0)], Xs)
    assert batches_opened() == [('batch', 'f64', 2, 0)] and 'set_divergence' not in names()
    _Fake.opened, _Fake.calls = [], []
    from tests.test_batch_csr_cpu import _FakeCsrBatch      # (the fake batch that knows a CSR batch's set_problem_sparse)
    monkeypatch.setattr(_native, 'Batch', _FakeCsrBatch)
    nmf.fit_transform_batch([beta_model(1.0), beta_model(1.0)], sparse)
    assert batches_opened() == [('batch', 'f64', 2, 0)]


def test_the_learner_builds_a_betanmf_only_when_asked(recorded):
    from multimodal_amd.lib.beta_nmf import BetaNMF
    mods = [data()[:, :12], data()[:, 12:]]
    lr = MultimodalLearner(['a', 'b'], [12, 8], [1.0, 0.5], K, beta=2.0)
    col = (np.arange(N) % 3 != 0).astype(float)[:, None]
    lr.train(mods, 5, weights=[None, col])
    assert isinstance(lr.nmf_train, BetaNMF) and lr.nmf_train.beta == 2.0 and lr.nmf_train.last_weights_route == 'array'
    assert [c[1] for c in _Fake.calls if c[0] == 'set_divergence'] == [(2.0,)]
    _Fake.calls = []
    lr.dico = np.full((K, F), 1.0 / F)
    lr.reconstruct_internal_multi(['b'], [mods[1]], 5)
    assert [c[1] for c in _Fake.calls if c[0] == 'set_divergence'] == [(2.0,)]
    _Fake.calls = []
    fit_coefficients(data(), lr.dico, iter_nmf=3, beta=0.5)
    assert [c[1] for c in _Fake.calls if c[0] == 'set_divergence'] == [(0.5,)]
    # the default is KLdivNMF itself
    _Fake.calls = []
    plain = MultimodalLearner(['a', 'b'], [12, 8], [1.0, 0.5], K)
    plain.train(mods, 5)
    fit_coefficients(data(), lr.dico, iter_nmf=3)
    assert type(plain.nmf_train) is nmf.KLdivNMF and plain.beta == 1.0 and 'set_divergence' not in names()


def test_device_dataset_refuses_a_beta_learner():
    lr = MultimodalLearner(['a'], [F], [1.0], K, beta=2.0)
    ds = object.__new__(device_data.DeviceDataset)
    for call in (lambda: ds.train(lr, [0, 1], 3), lambda: ds.reconstruct_internal_multi(lr, ['a'], [0, 1], 3),
                 lambda: ds.train_many([lr], [[0, 1]], 3), lambda: ds.reconstruct_internal_multi_many([lr], ['a'], [[0, 1]], 3),
                 lambda: device_data.DeviceEvaluation(ds, lr, 3)):
        with pytest.raises(ValueError, match='beta = 2'):
            call()


_CHILD = r'''
import sys
import numpy as np
from multimodal_amd import _native
from tests.test_batch_cpu import _Fake
_native.Context = _Fake
from multimodal_amd.learner import MultimodalLearner, fit_coefficients
X = np.random.default_rng(0).random((30, 20)) + 0.01
lr = MultimodalLearner(['a', 'b'], [12, 8], [1.0, 0.5], 4)
lr.train([X[:, :12], X[:, 12:]], 3)
lr.dico = np.full((4, 20), 0.05)
lr.reconstruct_internal_multi(['a'], [X[:, :12]], 3)
fit_coefficients(X, lr.dico, iter_nmf=3)
assert 'multimodal_amd.lib.beta_nmf' not in sys.modules, 'the default learner imported the beta path'
MultimodalLearner(['a', 'b'], [12, 8], [1.0, 0.5], 4, beta=2.0).train([X[:, :12], X[:, 12:]], 3)
assert 'multimodal_amd.lib.beta_nmf' in sys.modules
print('ok')
'''


def test_a_learner_without_beta_never_imports_the_new_path():
    """In a fresh interpreter (this one has imported lib.beta_nmf for the tests above): the default learner's train,
    reconstruct_internal_multi and fit_coefficients leave `multimodal_amd.lib.beta_nmf` unimported; beta = 2 imports it."""
    out = subprocess.run([sys.executable, '-c', _CHILD], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0 and out.stdout.decode().strip().endswith('ok'), out.stderr.decode(errors='replace')[-2000:]
