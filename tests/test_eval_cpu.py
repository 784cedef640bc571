"""CPU side of the evaluation-kernel tests (tests/test_eval_gpu.py): the extended-precision references of tests/eval_cases.py
against the recorded reference outputs (fixture G10) and the oracle, the bars against plain fp64 evaluation in the kernels' own
order, and the content every case claims.  No GPU needed."""
import numpy as np
import pytest
from numpy.testing import assert_allclose

from oracle import klnmf_oracle as orc
from tests import eval_cases as evc
from tests import golden_inputs as gi

QUARTER = 0.25


def test_longdouble_is_an_extended_format():
    assert np.finfo(evc.ld()).eps < 2.0 ** -60


def test_the_metric_codes_are_the_bindings():
    from multimodal_amd import _native
    assert (evc.KL, evc.REV_KL, evc.SYM_KL, evc.FROBENIUS, evc.COSINE_DIFF) == \
        (_native.DIST_KL, _native.DIST_REV_KL, _native.DIST_SYM_KL, _native.DIST_FROBENIUS, _native.DIST_COSINE_DIFF)
    assert evc.EPS == orc.EPS_RATIO


def test_reference_reproduces_fixture_g10():
    g = gi.load('g10_distances')
    A, B = gi.g10_inputs(g)
    for metric, name in evc.METRICS:
        value, M = evc.all_pairs(A, B, metric)
        assert value.shape == M.shape == g[name].shape
        assert_allclose(value.astype(np.float64), g[name], rtol=1e-13, atol=0)
        assert np.all(M >= np.abs(value))


def test_reference_generalized_kl_matches_the_oracle():
    rng = np.random.default_rng(5)
    x = (rng.random((37, 53)) + 0.05) * (rng.random((37, 53)) >= 0.3)
    y = rng.random((37, 53)) + 0.05
    for axis in (None, 0, 1):
        for eps in (1e-8, 1e-3):
            value, M = evc.generalized_kl(x, y, eps, axis=axis)
            assert_allclose(np.asarray(value, dtype=np.float64), orc.generalized_kl(x, y, eps, axis=axis), rtol=1e-13, atol=0)
            assert np.all(M >= np.abs(value))
    value, M = evc.generalized_kl(np.zeros(0), np.zeros(0), 1e-8)
    assert value == 0 and M == 0


@pytest.mark.parametrize('d', evc.DIMS)
def test_fp64_in_kernel_order_stays_within_a_quarter_of_the_distance_bars(d):
    for na, nb in evc.SHAPES:
        case = evc.pair_case(na, nb, d)
        for f32 in (False, True):
            A, B = evc.case_inputs(case, f32)
            for metric, name in evc.METRICS:
                ref, M = evc.pair_reference(na, nb, d, metric, f32)
                got = evc.kernel_order_distances(A, B, metric)
                ok, worst = evc.within(got, ref, QUARTER * evc.distance_bar(d, M))
                assert ok, '%s %dx%d d=%d: plain fp64 is at %.2f of the bar' % (name, na, nb, d, QUARTER * worst)


def test_fp64_kl_in_kernel_order_over_every_length_to_4097():
    """One pair per length 1 .. 4097, so every count of whole and ragged trips up to 65."""
    rng = np.random.default_rng(11)
    for d in range(1, 4098):
        a = ((rng.random((1, d)) + 0.05) * (rng.random((1, d)) >= 0.3))
        b = rng.random((1, d)) + 0.05
        ref, M = evc.all_pairs(a, b, evc.KL)
        got = evc.kernel_order_distances(a, b, evc.KL)
        assert evc.within(got, ref, QUARTER * evc.distance_bar(d, M))[0], d


@pytest.mark.parametrize('count', evc.GKL_COUNTS)
def test_fp64_in_kernel_order_stays_within_a_quarter_of_the_gkl_bar(count):
    for eps in evc.GKL_EPS:
        for f32 in (False, True):
            x, y = evc.gkl_case(count, eps)
            if f32:
                x, y = evc.as_f32(x), evc.as_f32(y)
            ref, M = evc.gkl_reference(count, eps, f32)
            got = evc.kernel_order_gkl(x, y, eps)
            ok, worst = evc.within(got, ref, QUARTER * evc.gkl_bar(count, M))
            assert ok, 'count %d eps %g: plain fp64 is at %.2f of the bar' % (count, eps, QUARTER * worst)


def test_the_gkl_counts_reach_the_grid_cap_and_the_stride_loop():
    grids = dict((c, evc.gkl_grid(c)) for c in evc.GKL_COUNTS)
    assert grids[0] == 0 and grids[1] == grids[255] == grids[256] == 1 and grids[257] == 2
    assert grids[262144] == 1024 and 262144 == 1024 * 256                 # the cap, every thread one element
    assert grids[262145] == 1024 and grids[600001] == 1024                # one thread, and most threads, take further trips
    assert 600001 > 2 * 1024 * 256 and 600001 % (1024 * 256) % 64 != 0     # a third, ragged trip
    assert evc.gkl_bar(0, 0.0) == 0.0


def test_every_pair_case_has_what_it_claims():
    pairs = sorted(na * nb for na, nb in evc.SHAPES)
    assert pairs == [1, 3, 3, 15, 16, 63, 561]
    assert any(p % 4 for p in pairs) and any(nb == 1 for _, nb in evc.SHAPES) and any(na == 1 for na, _ in evc.SHAPES)
    assert set(evc.DIMS) >= {0, 1, 63, 64, 65, 127, 128, 129} and max(evc.DIMS) > 15 * 64    # none, one, two, three and 16 trips
    for d in evc.DIMS:
        for na, nb in evc.SHAPES:
            c = evc.pair_case(na, nb, d)
            assert c.A.shape == (na, d) and c.B.shape == (nb, d)
            assert np.all(c.A >= 0) and np.all(c.B >= 0)
            for i in c.zero_a:
                assert not c.A[i].any()
            for j in c.zero_b:
                assert not c.B[j].any()
            for i, j in c.same:
                assert np.array_equal(c.A[i], c.B[j])
            if na >= 4 and nb >= 3:                       # enough rows for every role
                assert c.zero_a and c.zero_b and c.same and c.sparse_a and c.sparse_b and c.scaled
            if d >= 63:
                for side, rows in ((c.A, c.sparse_a), (c.B, c.sparse_b)):
                    for r in rows:
                        zeros = np.mean(side[r] == 0)
                        assert 0.1 < zeros < 0.5, (na, nb, d, r, zeros)
                for side, r in c.scaled:
                    row = (c.A if side == 'a' else c.B)[r]
                    assert 0 < row.max() < 2e-6
                # 0 log 0 on either operand: a zero of A against a positive entry of B and the reverse
                if c.sparse_a and c.sparse_b and nb > 1:
                    assert np.any((c.A[c.sparse_a[0]] == 0) & (c.B[1] > 0))
                    assert np.any((c.B[c.sparse_b[0]] == 0) & (c.A[c.sparse_a[0]] > 0))
    for count in evc.GKL_COUNTS:
        for eps in evc.GKL_EPS:
            x, y = evc.gkl_case(count, eps)
            assert x.shape == y.shape == (count,) and np.all(y > 0)
            if eps == 0:
                assert np.all(x > 0)
            elif count >= 255:
                assert 0.2 < np.mean(x == 0) < 0.4


def test_exact_facts_hold_in_the_reference():
    """What tests/test_eval_gpu.py asserts with ==: identical rows, a zero vector, d = 0."""
    c = evc.pair_case(7, 9, 65)
    for metric, name in evc.METRICS:
        v, _ = evc.pair_reference(7, 9, 65, metric, False)
        for i, j in c.same:
            if metric != evc.COSINE_DIFF:
                assert v[i, j] == 0, name
        if metric == evc.COSINE_DIFF:
            assert np.all(v[c.zero_a, :] == 0) and np.all(v[:, c.zero_b] == 0)
        if metric == evc.FROBENIUS:
            L = evc.ld()
            assert_allclose(v[c.zero_a[0]].astype(np.float64), np.sqrt(np.square(c.B.astype(L)).sum(axis=1)).astype(np.float64), rtol=1e-15)
        v0, _ = evc.pair_reference(5, 3, 0, metric, False)
        assert v0.shape == (5, 3) and np.all(v0 == 0)
