"""The weighted KL-NMF update without a GPU: the fp64 restatement (tests/weighted_cases.py) against the existing references,
the host-side validation of `weights`, and the new exports.

  * with weights of 1 the restatement is exact_cases.ref_fit (a fit and a transform, 30 iterations, three shapes, data with a
    zero row and a zero column): W, H and losses within 1e-12 relative.  Measured: 3.5e-14 worst.
  * with weight 0 on a quarter of the rows, H, the losses and the kept rows of W equal the restated fit of V without those
    rows within 1e-12 (measured 1.4e-14), and the zero-weight rows of W stay W0 = V.H0^T exactly.
  * `check_weights` and the public entry points raise ValueError for weights that do not broadcast, negative or non-finite
    weights and weights with CSR input -- before any context exists; a scalar never reaches the weighted path.
"""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from multimodal_amd import _native
from multimodal_amd.lib import nmf
from multimodal_amd.learner import MultimodalLearner, fit_coefficients
from tests import exact_cases as ec
from tests import weighted_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(37, 53, 7), (130, 200, 17), (300, 700, 65)]
ITERS = 30
BAR = 1e-12


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    zero = b == 0
    assert np.all(a[zero] == 0)
    if zero.all():
        return 0.0
    return float(np.max(np.abs(a - b)[~zero] / np.abs(b)[~zero]))


def problem(n, f, k):
    V = ec.data(n, f, seed=1, zero_row=n // 2, zero_col=f // 3)
    _, H0 = ec.factors(n, f, k, seed=2)
    return V, H0


@pytest.mark.parametrize('shape', SHAPES, ids=ec.case_id)
def test_ones_give_the_unweighted_reference(shape):
    n, f, k = shape
    V, H0 = problem(n, f, k)
    ones = np.ones((n, f))
    for kw in (dict(fit=True), dict(fit=False, components=H0)):
        got = wc.ref_fit_w(V, ones, H0, ITERS, **kw)
        ref = ec.ref_fit(V, H0, ITERS, **kw)
        for what, a, b in zip(('W', 'H', 'losses'), got, ref):
            err = rel(a, b)
            print('%s %s %s: %.2e' % (ec.case_id(shape), 'fit' if kw['fit'] else 'transform', what, err))
            assert err <= BAR, (what, err)


@pytest.mark.parametrize('shape', SHAPES, ids=ec.case_id)
def test_zero_weight_rows_are_deleted_rows(shape):
    n, f, k = shape
    V, H0 = problem(n, f, k)
    Om, keep = wc.row_mask(n, f, seed=5)
    assert (~keep).sum() == n // 4
    W, H, losses = wc.ref_fit_w(V, Om, H0, ITERS)
    Wr, Hr, lr = ec.ref_fit(V[keep], H0, ITERS)
    for what, a, b in (('W kept', W[keep], Wr), ('H', H, Hr), ('losses', losses, lr)):
        err = rel(a, b)
        print('%s %s: %.2e' % (ec.case_id(shape), what, err))
        assert err <= BAR, (what, err)
    assert np.array_equal(W[~keep], ec.ref_init_W(V, H0)[~keep])          # W0 = V.H0^T, untouched by 30 updates


def test_a_step_of_the_restatement_by_hand():
    """2 x 2, k = 1, one hidden entry: the rules written out."""
    V = np.array([[2.0, 4.0], [1.0, 3.0]])
    Om = np.array([[1.0, 0.0], [0.5, 2.0]])
    W = np.array([[3.0], [2.0]])
    H = np.array([[0.25, 0.75]])
    eps = 1e-8
    Y = W.dot(H)
    Q = (V + eps) / (Y + eps)
    loss, R, Wn, Hn = wc.ref_step_w(V, Om, W, H)
    assert np.array_equal(R, Om * Q) and R[0, 1] == 0
    assert loss == pytest.approx(sum(Om[i, j] * (V[i, j] * np.log(Q[i, j]) - V[i, j] + Y[i, j]) for i in range(2) for j in range(2)), rel=1e-15)
    w0 = 3.0 * (R[0, 0] * 0.25) / (1.0 * 0.25)
    w1 = 2.0 * (R[1, 0] * 0.25 + R[1, 1] * 0.75) / (0.5 * 0.25 + 2.0 * 0.75)
    assert np.allclose(Wn[:, 0], [w0, w1], rtol=1e-15)
    h = np.array([0.25 * (w0 * R[0, 0] + w1 * R[1, 0]) / (w0 * 1.0 + w1 * 0.5), 0.75 * (w1 * R[1, 1]) / (w1 * 2.0)])
    assert np.allclose(Hn[0], h / (1e-16 + h.sum()), rtol=1e-15)
    # a sample with nothing observed keeps its coefficients; a feature never observed keeps its share of the row
    Om0 = np.array([[0.0, 0.0], [1.0, 0.0]])
    _, _, Wn0, Hn0 = wc.ref_step_w(V, Om0, W, H)
    assert Wn0[0, 0] == 3.0
    assert Hn0[0, 1] / Hn0[0, 0] == pytest.approx(0.75 / (0.25 * (Wn0[1, 0] * (Om0 * Q)[1, 0]) / Wn0[1, 0]), rel=1e-15)


def test_imputation_on_the_restatement():
    """The issue's case on the CPU: hidden entries of exact rank-4 data are reconstructed by the weighted fit (0.006) and
    not by the unweighted fit of the zero-filled matrix (0.51)."""
    V, M, H0 = wc.imputation_case()
    W, H, _ = wc.ref_fit_w(V * M, M, H0, 100)
    Wu, Hu, _ = ec.ref_fit(V * M, H0, 100)
    weighted, zero_filled = wc.hidden_error(V, M, W, H), wc.hidden_error(V, M, Wu, Hu)
    print('hidden-entry relative L1 error: weighted %.4f, zero-filled %.4f' % (weighted, zero_filled))
    assert weighted < 0.05 and weighted * 10 <= zero_filled


def test_the_gpu_shapes_reach_every_route_at_256_cus():
    """tests/test_weighted_gpu.py's shapes on the MI355X: one and many row chunks, one-piece and split W rule, the H rule from
    the slabs, from their sum and in segments (a last segment of one column)."""
    shapes = [(1, 1, 1), (15, 17, 1), (65, 65, 65), (300, 700, 65), (300, 700, 200), (4111, 63, 200), (4096, 128, 16),
              (4096, 129, 16), (100, 16385, 33)]
    regimes = [ec.exact_regime(n, f, k, ec.MI355X_CUS) for n, f, k in shapes]
    assert {r[0] == 1 for r in regimes} == {True, False}
    assert {r[2] == 1 for r in regimes} == {True, False}
    assert any(r[5] and r[0] > 1 for r in regimes) and any(not r[5] and r[4] == 1 for r in regimes) and any(r[4] > 1 for r in regimes)
    assert ec.exact_regime(4096, 128, 16, 256)[5] and not ec.exact_regime(4096, 129, 16, 256)[5]
    assert ec.exact_regime(100, 16385, 33, 256)[4] == 5


# ---- host validation: ValueError before any context exists (this machine may have no GPU at all) -------------------------------
@pytest.fixture
def no_context(monkeypatch):
    def refuse(*a, **kw):
        raise AssertionError('a native context was created')
    monkeypatch.setattr(_native, 'Context', refuse)


X = np.abs(np.random.RandomState(0).random_sample((6, 5))) + 0.1
BAD = [
    ('shape', np.ones((5, 6))),
    ('shape', np.ones(6)),                 # (n,) does not broadcast to (n, f): an (n, 1) column does
    ('negative', -np.ones((6, 5))),
    ('negative', np.array([1.0, 1.0, -1e-300, 1.0, 1.0])),
    ('finite', np.full((6, 1), np.nan)),
    ('finite', np.full((6, 5), np.inf)),
]


@pytest.mark.parametrize('why,w', BAD, ids=[b[0] + str(i) for i, b in enumerate(BAD)])
def test_bad_weights_raise_valueerror_on_the_host(no_context, why, w):
    m = nmf.KLdivNMF(n_components=2, max_iter=3, precision='f64')
    with pytest.raises(ValueError):
        m.fit_transform(X, weights=w)
    with pytest.raises(ValueError):
        m.fit(X, weights=w)
    m.components_ = np.ones((2, 5)) / 5
    with pytest.raises(ValueError):
        m.transform(X, weights=w)
    with pytest.raises(ValueError):
        m.error(X, np.ones((6, 2)), weights=w)
    with pytest.raises(ValueError):
        nmf.KLdivNMF._updated_W(X, np.ones((6, 2)), np.ones((2, 5)), weights=w)
    with pytest.raises(ValueError):
        nmf.KLdivNMF._updated_H(X, np.ones((6, 2)), np.ones((2, 5)), weights=w)
    with pytest.raises(ValueError):
        nmf.check_weights(w, X.shape)


def test_weights_with_csr_input_raise_valueerror_on_the_host(no_context):
    m = nmf.KLdivNMF(n_components=2, max_iter=3, precision='f64')
    with pytest.raises(ValueError):
        m.fit_transform(sp.csr_matrix(X), weights=np.ones((6, 5)))
    with pytest.raises(ValueError):
        m.error(sp.csr_matrix(X), np.ones((6, 2)), H=np.ones((2, 5)), weights=np.ones((6, 5)))
    learner = MultimodalLearner(['a', 'b'], [3, 2], [1., 1.], 2)
    with pytest.raises(ValueError):
        learner.train([sp.csr_matrix(X[:, :3]), X[:, 3:]], 3, weights=[None, np.ones((6, 1))])
    with pytest.raises(ValueError):
        learner.train([X[:, :3], X[:, 3:]], 3, weights=[np.ones((6, 1))])          # one entry per modality
    with pytest.raises(ValueError):
        learner.train([X[:, :3], X[:, 3:]], 3, weights=[None, np.ones((6, 3))])
    with pytest.raises(ValueError):
        fit_coefficients(X, np.ones((2, 5)) / 5, iter_nmf=3, weights=-np.ones((6, 5)))


def test_what_check_weights_returns():
    assert nmf.check_weights(1., X.shape) is None
    assert nmf.check_weights(None, X.shape) is None
    assert nmf.check_weights(np.float64(3.0), X.shape) is None          # np.ndim 0
    assert nmf.check_weights(np.array(2.0), X.shape, sparse=True) is None
    for w in (np.ones(5), np.ones((6, 1)), np.ones((1, 5)), np.ones((6, 5)), [0, 1, 0, 1, 1], np.ones((6, 1), np.float32)):
        out = nmf.check_weights(w, X.shape)
        assert out.shape == X.shape and out.dtype in (np.float32, np.float64)
        assert np.array_equal(out, np.broadcast_to(np.asarray(w, dtype=np.float64), X.shape))


def test_a_scalar_weight_does_not_reach_the_weighted_path(monkeypatch):
    """weights=1. (the default), any other scalar and a 0-d array take the path they always took: `_fit_uploaded` is entered
    with weighted = False, an upload that never uploads weights, and `_context` is asked for an unweighted context."""
    seen = []

    class Ctx(object):
        def upload_blocks(self, blocks, coefs):
            seen.append('blocks')

        def upload_weights(self, *a, **kw):
            seen.append('weights')

    def fake(self, n, f, upload, out_dtype_of, _fit=True, return_errors=False, sparse_X=None, host_blocks=None, weighted=False):
        seen.append(weighted)
        upload(Ctx())
        self.components_ = None
        return np.zeros((n, 2))
    monkeypatch.setattr(nmf.KLdivNMF, '_fit_uploaded', fake)
    m = nmf.KLdivNMF(n_components=2, max_iter=3, precision='f64')
    for w in (1., 0.5, np.array(2.0), np.float32(1)):
        del seen[:]
        m.fit_transform(X, weights=w)
        assert seen == [False, 'blocks'], (w, seen)
    del seen[:]
    m.fit_transform(X)
    assert seen == [False, 'blocks']
    del seen[:]
    m.fit_transform(X, weights=np.ones((6, 1)))
    assert seen == [True, 'blocks', 'weights']
    # per block: only the blocks that carry weights are uploaded
    del seen[:]
    MultimodalLearner(['a', 'b'], [3, 2], [1., 1.], 2).train([X[:, :3], X[:, 3:]], 3, weights=[None, 1.0])
    assert seen == [False, 'blocks']


def test_the_precision_a_weighted_fit_runs_in(capsys):
    nmf._NOTED.clear()
    assert nmf.weighted_precision('f64') == nmf.weighted_precision('auto') == nmf.weighted_precision('float64') == 'f64'
    assert nmf.weighted_precision('f32') == 'f32'
    assert capsys.readouterr().err == ''
    for prec in ('f16', 'bf16', 'bf16x3', 'f16x3'):
        assert nmf.weighted_precision(prec) == 'f32'
        assert nmf.weighted_precision(prec) == 'f32'
    err = capsys.readouterr().err
    assert err.count('\n') == 4 and "precision='f16x3'" in err and 'weights' in err


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------------
def test_the_new_exports_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'klnmf.h')).read()
    lib = _native.load()
    for name in ('klnmf_upload_weights', 'klnmf_clear_weights'):
        assert re.search(r'\bint %s\s*\(' % name, header), name
        assert name in _native.SIGNATURES and hasattr(lib, name)
        # declared with the reference lines it gives meaning to
        decl = header[:header.index('int %s' % name)]
        comment = decl[decl.rindex('/*'):]
        assert 'nmf.py:159-175' in comment, name
    assert re.search(r'the\s+(\*\s+)?reference ignores the argument', header)
    assert re.search(r'#define\s+KLNMF_Q_WEIGHTED\s+%d\b' % _native.Q_WEIGHTED, header)
    assert len(_native.SIGNATURES['klnmf_upload_weights'][1]) == len(_native.SIGNATURES['klnmf_upload_V'][1]) - 1      # no scale
    assert callable(_native.Context.upload_weights) and callable(_native.Context.clear_weights)


def _code(path):
    """The file without its // comments."""
    return re.sub(r'//[^\n]*', '', open(path).read())


def test_the_weighted_route_is_a_host_branch():
    """One kernel family (exact.hip.h) under policies: its own file names no weight buffer and keeps the unweighted epilogue a
    compile-time branch of its own, every rule kernel exists once, what only a weighted problem runs lives in weighted.hip.h and
    every new buffer is problem state sized by the unweighted plan's counts."""
    csrc = os.path.join(ROOT, 'multimodal_amd', 'csrc')
    assert not re.search(r'\bOm\b', open(os.path.join(csrc, 'exact.hip.h')).read())        # (comments included)
    exact = _code(os.path.join(csrc, 'exact.hip.h'))
    assert 'if constexpr (std::is_same<Weight, NoWeight>::value)' in exact
    weighted = _code(os.path.join(csrc, 'weighted.hip.h'))
    for name in ('ElemWeight', 'FacDen', 'w_factor', 'k_gemm_dual', 'k_fill'):
        assert name in weighted, name
    family = exact + weighted + _code(os.path.join(csrc, 'presence.hip.h'))
    for kernel in ('k_update_H', 'k_update_H_part', 'k_update_H_norm', 'k_wrule_exact', 'k_sum_partials', 'h_product'):
        assert len(re.findall(r'\b%s\(' % kernel, family)) == 1 + (kernel == 'h_product') * 2, kernel      # defined once (h_product: + two calls)
    for epi in ('EpiQ', 'EpiW', 'EpiWpart', 'EpiN'):
        assert len(re.findall(r'struct %s\b' % epi, family)) == 1, epi
    assert 'mfma_f64_16x16x4f64' in exact and 'mfma_f32_16x16x4f32' in exact
    ctx = open(os.path.join(csrc, 'ctx.hip.h')).read()
    state = ctx[ctx.index('struct ProblemState'):ctx.index('struct LoopState')]
    assert re.search(r'\*Om\b', state) and 'Dpart' in state
