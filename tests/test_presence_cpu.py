"""Row x modality presence masks on the host: the factored restatement (tests/presence_cases.py) against the weighted one on the
broadcast mask, the routing decision of KLdivNMF._fit_blocks, the host's ValueErrors and the C-ABI's declarations.  No GPU.

Measured here: the factored step agrees with weighted_cases.ref_step_w to 3.7e-15 and a 10-iteration fit to 1.7e-14 (bars:
1e-12 on a step, 1e-10 on the fit's losses, 1e-9 on its factors -- test_exact_gpu.BARS['f64'], which the device is held to).
"""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from multimodal_amd import _native
from multimodal_amd.lib import nmf
from multimodal_amd.learner import MultimodalLearner
from tests import exact_cases as ec
from tests import presence_cases as pc
from tests import weighted_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1), (15, 17, 1), (65, 65, 65), (300, 700, 65), (300, 700, 200), (4111, 63, 200), (4096, 129, 16), (100, 16385, 33)]
MODALITIES = [1, 2, 3, 16]
ITERS = 10


def rel(got, ref):
    """Worst elementwise relative error; an exact zero of the reference must be reproduced."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    assert np.array_equal(got == 0, ref == 0)
    nz = ref != 0
    return float(np.max(np.abs(got[nz] - ref[nz]) / np.abs(ref[nz]))) if nz.any() else 0.0


CASES = [(shape, M) for shape in SHAPES for M in MODALITIES if M <= shape[1]]      # (a modality holds a column at least)


@pytest.mark.parametrize('shape,M', CASES, ids=['%s-M%d' % (ec.case_id(s), M) for s, M in CASES])
def test_the_factored_form_is_the_weighted_update_on_the_broadcast_mask(shape, M):
    n, f, k = shape
    V = ec.data(n, f, seed=n + 7 * f + 13 * k, zero_row=n // 2 if n >= 4 else None, zero_col=f // 3 if f >= 4 else None)
    W, H = ec.factors(n, f, k, seed=k + 1)
    b = pc.bounds(f, M)
    assert len(b) == M + 1 and b[0] == 0 and b[-1] == f and all(x < y for x, y in zip(b[:-1], b[1:]))
    P = pc.mask(n, M, seed=3 * n + 5 * f + k + M)
    Om = pc.omega(P, b)
    assert Om.shape == (n, f)
    _, kchunk, _, wchunk, _, _ = ec.exact_regime(n, f, k, ec.MI355X_CUS)
    worst = 0.0
    for got, ref in zip(pc.ref_step_p(V, P, b, W, H, kchunk, wchunk), wc.ref_step_w(V, Om, W, H, kchunk, wchunk)):
        worst = max(worst, rel(got, ref))
    assert worst <= 1e-12, worst
    for fit in (True, False):
        got = pc.ref_fit_p(V, P, b, H, ITERS, fit=fit, components=H, kchunk=kchunk, wchunk=wchunk)
        ref = wc.ref_fit_w(V, Om, H, ITERS, fit=fit, components=H, kchunk=kchunk, wchunk=wchunk)
        e_loss, e_fac = rel(got[2], ref[2]), max(rel(got[0], ref[0]), rel(got[1], ref[1]))
        print('%s M=%d fit=%d: step %.1e, fit losses %.1e, factors %.1e' % (ec.case_id(shape), M, fit, worst, e_loss, e_fac))
        assert e_loss <= 1e-10 and e_fac <= 1e-9, (e_loss, e_fac)


def test_the_mask_generator_holds_its_edge_cases():
    for n, M in ((300, 1), (300, 3), (15, 16), (4096, 2)):
        P = pc.mask(n, M, seed=n + M)
        assert P.min() == 0.0 and P.max() == 1.0 and ((P > 0) & (P < 1)).any()
        assert not P[n // 3].any()                                   # a sample with no modality present
        assert (M < 3) or not P[:, M // 2].any()                     # a modality absent from every row
        assert (P.sum(axis=0) > 0).sum() == (M if M < 3 else M - 1)
    assert (pc.mask(1, 1, seed=0) > 0).all()
    assert pc.bounds(65, 3) == [0, 1, 64, 65] and pc.bounds(17, 16) == list(range(16)) + [17]
    assert all(v % 64 for v in pc.bounds(700, 3)[1:-1]) and pc.bounds(4096, 2) == [0, 2049, 4096]


# ---- the routing decision of _fit_blocks -------------------------------------------------------------------------------------------
N, DIMS = 6, [3, 2]
RS = np.random.RandomState(0)
A, B = RS.random_sample((N, DIMS[0])) + 0.1, RS.random_sample((N, DIMS[1])) + 0.1
COL = (RS.random_sample((N, 1)) > 0.4).astype(np.float64)

ROUTES = [
    ('none', [None, None], None),
    ('scalar', [None, 2.0], None),
    ('(n, 1)', [None, COL], 'presence'),
    ('(n, 1) twice', [COL, 1.0 - COL], 'presence'),
    ('(n, 1) and a scalar', [0.5, COL], 'presence'),
    ('(n, 1) float32', [None, COL.astype(np.float32)], 'presence'),
    ('(n, f_b)', [None, np.ones((N, DIMS[1]))], 'array'),
    ('(f_b,)', [np.ones(DIMS[0]), None], 'array'),
    ('(1, f_b)', [np.ones((1, DIMS[0])), None], 'array'),
    ('(n, 1) and (n, f_b)', [COL, np.ones((N, DIMS[1]))], 'array'),
    ('(n, 1) and (f_b,)', [COL, np.ones(DIMS[1])], 'array'),
]


class _Ctx(object):
    """Records the uploads `_fit_blocks` asks of a context."""

    def __init__(self):
        self.calls = []

    def upload_blocks(self, blocks, coefs):
        self.calls.append(('blocks', len(blocks)))

    def upload_weights(self, block, row0=0, col0=0, col_bounds=None):
        self.calls.append(('weights', np.array(block, dtype=np.float64), col0, None if col_bounds is None else list(col_bounds)))


@pytest.fixture
def uploads(monkeypatch):
    """`_fit_uploaded` replaced by one that runs the upload on a recording context: (weighted, calls) per loop."""
    seen = []

    def fake(self, n, f, upload, out_dtype_of, _fit=True, return_errors=False, sparse_X=None, host_blocks=None, weighted=False):
        self.last_weights_route = None                # (as the real one does)
        ctx = _Ctx()
        upload(ctx)
        seen.append((weighted, ctx.calls))
        self.components_ = None
        return np.zeros((n, 2))
    monkeypatch.setattr(nmf.KLdivNMF, '_fit_uploaded', fake)
    return seen


@pytest.mark.parametrize('name,weights,route', ROUTES, ids=[r[0] for r in ROUTES])
def test_the_route_fit_blocks_takes(uploads, name, weights, route):
    assert nmf.weights_route(weights, [A, B]) == route
    m = nmf.KLdivNMF(n_components=2, max_iter=3, precision='f64')
    assert m.last_weights_route is None
    m._fit_blocks([A, B], [1.0, 0.5], weights=weights)
    assert m.last_weights_route == route
    (weighted, calls), = uploads
    assert weighted == (route is not None) and calls[0] == ('blocks', 2)
    if route is None:
        assert len(calls) == 1
    elif route == 'presence':
        (_, P, col0, cb), = calls[1:]                                 # one upload: the n x M matrix and the blocks' widths
        assert cb == [0, 3, 5] and col0 == 0 and P.shape == (N, 2)
        for m_, w in enumerate(weights):
            want = np.ones(N) if (w is None or np.ndim(w) == 0) else np.asarray(w, dtype=np.float64)[:, 0]
            assert np.array_equal(P[:, m_], want)
    else:
        assert all(c[3] is None for c in calls[1:])                   # blocks of the n x f buffer, one per block with weights
        assert len(calls) - 1 == sum(1 for w in weights if not (w is None or np.ndim(w) == 0))
        assert [c[1].shape for c in calls[1:]] == [(N, d) for d, w in zip(DIMS, weights) if not (w is None or np.ndim(w) == 0)]
    # the route is named per loop: a loop without weights behind a weighted one
    m._fit_blocks([A, B], [1.0, 0.5])
    assert m.last_weights_route is None


def test_seventeen_blocks_take_the_array_route(uploads):
    blocks = [A[:, :1]] * 17
    weights = [None] * 16 + [COL]
    assert nmf.weights_route(weights, blocks) == 'array'
    assert nmf.weights_route(weights[1:], blocks[1:]) == 'presence' and _native.MAX_MODALITIES == 16
    m = nmf.KLdivNMF(n_components=2, max_iter=3, precision='f64')
    m._fit_blocks(blocks, [1.0] * 17, weights=weights)
    assert m.last_weights_route == 'array'
    (_, calls), = uploads
    assert len(calls) == 2 and calls[1][2] == 16 and calls[1][3] is None
    del uploads[:]
    m._fit_blocks(blocks[1:], [1.0] * 16, weights=weights[1:])
    assert m.last_weights_route == 'presence'
    assert uploads[0][1][1][3] == list(range(17))


def test_fit_transform_and_the_learner_reach_the_route(uploads):
    X = np.hstack([A, B])
    m = nmf.KLdivNMF(n_components=2, max_iter=3, precision='f64')
    m.fit_transform(X, weights=COL)                                   # M = 1
    assert m.last_weights_route == 'presence' and uploads[-1][1][1][3] == [0, 5]
    m.fit_transform(X, weights=np.ones((N, 5)))
    assert m.last_weights_route == 'array'
    m.fit_transform(X, weights=np.ones(5))
    assert m.last_weights_route == 'array'
    m.fit_transform(X)
    assert m.last_weights_route is None
    m.components_ = np.ones((2, 5)) / 5
    m.transform(X, weights=COL)
    assert m.last_weights_route == 'presence'
    del uploads[:]
    MultimodalLearner(['a', 'b'], DIMS, [1., 0.5], 2).train([A, B], 3, weights=[None, COL])
    (weighted, calls), = uploads
    assert weighted and calls[1][3] == [0, 3, 5] and np.array_equal(calls[1][1], np.hstack([np.ones((N, 1)), COL]))


# ---- the host's ValueErrors: before any context exists ---------------------------------------------------------------------------
@pytest.fixture
def no_context(monkeypatch):
    def refuse(*a, **kw):
        raise AssertionError('a native context was created')
    monkeypatch.setattr(_native, 'Context', refuse)


@pytest.mark.parametrize('w', [np.full((N, 1), np.nan), -COL - 1e-300, np.full((N, 1), np.inf), np.ones((N + 1, 1)), np.ones((N - 1, 1))],
                         ids=['nan', 'negative', 'inf', 'a row too many', 'a row too few'])
def test_a_bad_presence_column_raises_valueerror_on_the_host(no_context, w):
    m = nmf.KLdivNMF(n_components=2, max_iter=3, precision='f64')
    with pytest.raises(ValueError):
        m.fit_transform(np.hstack([A, B]), weights=w)
    with pytest.raises(ValueError):
        m._fit_blocks([A, B], [1.0, 1.0], weights=[None, w])
    with pytest.raises(ValueError):
        MultimodalLearner(['a', 'b'], DIMS, [1., 1.], 2).train([A, B], 3, weights=[None, w])


def test_a_presence_column_with_csr_input_raises_valueerror_on_the_host(no_context):
    m = nmf.KLdivNMF(n_components=2, max_iter=3, precision='f64')
    with pytest.raises(ValueError):
        m._fit_blocks([sp.csr_matrix(A), B], [1.0, 1.0], weights=[None, COL])
    with pytest.raises(ValueError):
        m._fit_blocks([A, B], [1.0, 1.0], weights=[COL])              # one entry per block


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------------
def test_the_new_export_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'klnmf.h')).read()
    lib = _native.load()
    assert re.search(r'\bint klnmf_upload_presence\s*\(', header)
    assert 'klnmf_upload_presence' in _native.SIGNATURES and hasattr(lib, 'klnmf_upload_presence')
    assert len(_native.SIGNATURES['klnmf_upload_presence'][1]) == 8
    assert re.search(r'#define\s+KLNMF_Q_PRESENCE\s+%d\b' % _native.Q_PRESENCE, header) and _native.Q_PRESENCE == 21
    assert re.search(r'#define\s+KLNMF_MAX_MODALITIES\s+%d\b' % _native.MAX_MODALITIES, header)
    assert callable(_native.Context.upload_presence) and callable(_native.Context.presence)
    # every symbol of the header is bound, and the documents count them alike
    declared = set(re.findall(r'^(?:int|const char \*)\s*(klnmf_\w+)\s*\(', header, flags=re.M))
    assert declared == set(_native.SIGNATURES)
    for doc in ('README.md', 'INTEGRATION.md', 'DESIGN.md'):
        assert '%d exports' % len(declared) in open(os.path.join(ROOT, doc)).read(), doc


def test_the_masked_route_is_a_host_branch():
    """No code of exact.hip.h or weighted.hip.h knows of the mask; its policies and its own kernels live in presence.hip.h."""
    csrc = os.path.join(ROOT, 'multimodal_amd', 'csrc')
    for name in ('exact.hip.h', 'weighted.hip.h'):
        whole = open(os.path.join(csrc, name)).read()
        assert not re.search(r'presence|modalit', whole), name                        # (comments included)
        assert 'Pres' not in re.sub(r'//[^\n]*', '', whole), name                     # the mask's policies: named in comments at most
    text = re.sub(r'//[^\n]*', '', open(os.path.join(csrc, 'presence.hip.h')).read())
    for name in ('PresenceWeight', 'k_presence_S', 'presence_den', 'FacPresW', 'k_presence_D_part', 'k_presence_D_sum', 'FacPresH',
                 'presence_d_chunks'):
        assert name in text, name
    assert not re.search(r'k_update_H|k_wrule_exact|struct Epi', text)        # the rules and epilogues are the family's
    loop = open(os.path.join(csrc, 'api_loop.hip')).read()
    assert all(('presence_%s<T>' % p) in loop for p in 'SD')
