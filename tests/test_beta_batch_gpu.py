"""Beta batches (klnmf_batch_set_divergence, include/klnmf_batch_beta.h, multimodal_amd/csrc/batch.hip.h): B dense problems of one
shape under one beta != 1 -- weighted where an Om was uploaded -- advancing through the beta loop together, one launch per stage.

What is held to what:
  * every problem of a beta batch against THE SAME problem alone in a `_native.Context` with `set_divergence(beta)` (and its weights)
    whose KLNMF_EX_ROW_CHUNKS / KLNMF_EX_W_CHUNKS are forced to the counts the batch reports: W0, W, H, the loss record, n_done and
    the stop flag BIT FOR BIT (np.array_equal: no tolerance) -- on the natural routes, on forced routes, with weights, with
    problems that stop apart, in transforms and across re-use;
  * and against the restatement of the beta loop (tests/beta_cases.ref_fit) summed over the batch's chunks, within
    tests/test_beta_gpu.py's bars, which are tests/test_exact_gpu.py's: f64 fit losses 1e-10, fit W and H 1e-9 (W0: 1e-12); f32 (the
    restatement fed the fp32-rounded inputs) 3e-5 and 3e-4 relative to at least the smallest normal fp32 number (W0: 3e-5), the
    f32 losses relative to at least tests/test_beta_gpu.loss_floor.  No bar of this file's own.
The switch helpers, the upload helpers, the problems and `assert_same_bits` are tests/test_batch_gpu.py's, by import.  Fits never
stop early (NO_STOP) except in the test that is about stopping.
Measured on the MI355X (worst over every case of this file, kept in profiles/beta_batch_gpu_tests.txt): every comparison with a
solo run 0 differing bits; against the restatement f64 W0 5.8e-16, fit losses 1.0e-15, W 4.8e-15, H 1.1e-14; f32 W0 1.1e-6, fit
losses 6.3e-7, W 4.9e-6, H 6.5e-6; the public route against the loop over `fit_transform` 0.  No bar was widened.
The measured worst errors are printed after each test (pytest -v) and are in each assertion message.
"""
import functools

import numpy as np
import pytest

from multimodal_amd import _native
from tests import beta_cases as bc
from tests import exact_cases as ec
from tests.loop_piece_cases import stop_rule
from tests.test_batch_gpu import (BARS, FLOOR, ITERS, PRECS, assert_same_bits, cu_count, esize, problem, raises, seen, set_switches,
                                  upload_form)
from tests.test_beta_gpu import loss_floor
from tests.test_sparse_gpu import _MEASURED, _report_measured, check  # noqa: F401  (the autouse fixture prints what was measured)

pytestmark = pytest.mark.gpu

ZERO_WEIGHT_ROW = 5


def weights(n, f, p):
    """Om of problem p: 30 % zeros and a row of zeros (tests/beta_cases.weights_of)."""
    return bc.weights_of(n, f, seed=3 * n + 5 * f + 11 * p, zero_row=ZERO_WEIGHT_ROW)


def beta_batch_run(batch, prec, Vs, H0s, beta, Oms=None, iters=ITERS, fit=True, tol_abs=ec.NO_STOP, components=None, W_start=None):
    """[(W0, W, H, errors, n_done, stopped)] per problem: the uploads, the cost behind them, the weights, W0 = V.H0^T (W_start: and the
    loop's start set over it), the loop."""
    for p, V in enumerate(Vs):
        batch.upload_V(p, upload_form(prec, V))
    batch.set_divergence(beta)
    assert batch.get_divergence() == beta
    for p, Om in enumerate(Oms or []):
        if Om is not None:
            batch.upload_weights(p, upload_form(prec, Om))
    for p, H0 in enumerate(H0s):
        batch.set_H(p, upload_form(prec, H0))
    batch.init_W()
    W0s = [batch.get_W(p) for p in range(batch.count)]
    if components is not None:
        for p, H in enumerate(components):
            batch.set_H(p, upload_form(prec, H))
    for p, W in enumerate(W_start or []):
        batch.set_W(p, upload_form(prec, W))
    results = batch.run(iters, fit, tol_abs)
    return [(W0s[p], batch.get_W(p), batch.get_H(p), np.array(results[p][0]), results[p][1], results[p][2]) for p in range(batch.count)]


def solo_beta(monkeypatch, prec, V, H0, k, regime, beta, Om=None, iters=ITERS, fit=True, tol_abs=ec.NO_STOP, components=None, h_seg=0,
              natural=False, cap=None):
    """The same problem alone in a context under the same cost, its chunk counts forced to `regime`'s (natural: its own plan)."""
    if natural:
        set_switches(monkeypatch)
    else:
        set_switches(monkeypatch, row_chunks=regime[0], w_chunks=regime[1], h_seg=h_seg)
    with _native.Context(prec) as ctx:
        ctx.set_problem(V.shape[0], V.shape[1], k, cap or iters)
        if not natural:
            assert ctx.exact_regime() == tuple(regime), (ctx.exact_regime(), regime)
        ctx.upload_V(upload_form(prec, V))
        if Om is not None:
            ctx.upload_weights(upload_form(prec, Om))
        ctx.set_divergence(beta)
        ctx.set_H(upload_form(prec, H0))
        ctx.init_W()
        W0 = ctx.get_W()
        if components is not None:
            ctx.set_H(upload_form(prec, components))
        errors, n_done, stopped = ctx.run(iters, fit, tol_abs)
        return W0, ctx.get_W(), ctx.get_H(), np.array(errors), n_done, stopped, ctx.exact_regime()


@functools.lru_cache(maxsize=8)
def reference(n, f, k, p, beta, weighted, f32_inputs, kchunk, wchunk, fit, iters=ITERS):
    """(W0, (W, H, losses), the f32 loss floor's inputs) of the restatement on problem p, summed over the batch's chunks."""
    V, H0 = problem(n, f, k, p)
    Om = weights(n, f, p) if weighted else None
    if f32_inputs:
        V, H0, Om = ec.as_f32(V), ec.as_f32(H0), None if Om is None else ec.as_f32(Om)
    W0 = ec.ref_init_W(V, H0, wchunk)
    return W0, bc.ref_fit(V, H0, iters, beta, Om=Om, fit=fit, components=H0, kchunk=kchunk, wchunk=wchunk), (V, Om, H0)


def check_against_reference(case, prec, got, ref, beta):
    W0r, (Wr, Hr, er), (V, Om, H0) = ref
    check(case, 'W0', got[0], W0r, BARS[prec]['step'], FLOOR[prec])
    assert len(got[3]) == len(er)
    check(case, 'losses', got[3], er, BARS[prec]['fit_loss'], loss_floor(prec, V, Om, W0r, H0, beta))
    check(case, 'W', got[1], Wr, BARS[prec]['fit_factor'], FLOOR[prec])
    check(case, 'H', got[2], Hr, BARS[prec]['fit_factor'], FLOOR[prec])


def plan_of(prec, n, f, k, B, **forced):
    return ec.exact_regime(n, f, k, max(1, cu_count() // B), esize(prec), **forced)


# ---- 1. a batch of one is the context -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('beta', [0.0, 2.0])
@pytest.mark.parametrize('shape', [(65, 65, 65), ec.MID], ids=ec.case_id)
def test_a_batch_of_one_is_the_context(monkeypatch, prec, shape, beta):
    n, f, k = shape
    V, H0 = problem(n, f, k, 0)
    solo = solo_beta(monkeypatch, prec, V, H0, k, None, beta, natural=True)
    set_switches(monkeypatch)
    with _native.Batch(prec, 1) as batch:
        batch.set_problem(n, f, k, ITERS)
        assert batch.exact_regime() == solo[6] and batch.get_divergence() == 1.0
        got = beta_batch_run(batch, prec, [V], [H0], beta)[0]
    assert got[4] == ITERS
    assert_same_bits('%s %s beta=%g B=1' % (prec, ec.case_id(shape), beta), got, solo)


# ---- 2. batch against solo runs and the restatement -----------------------------------------------------------------------------------
SHAPES = [(15, 17, 1), (65, 65, 65), (300, 700, 17), (4096, 129, 16)]
BATCHES = [(s, B) for s in SHAPES for B in (2, 3)] + [((100, 16385, 33), 2)]


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('beta', bc.BETAS)
@pytest.mark.parametrize('shape,B', BATCHES, ids=['%s-B%d' % (ec.case_id(s), B) for s, B in BATCHES])
def test_batch_against_solo_runs_and_the_restatement(monkeypatch, prec, shape, B, beta):
    n, f, k = shape
    s, kchunk, w, wchunk, h, slabs = plan_of(prec, n, f, k, B)
    probs = [problem(n, f, k, p) for p in range(B)]
    set_switches(monkeypatch)
    with _native.Batch(prec, B) as batch:
        batch.set_problem(n, f, k, ITERS)
        regime = batch.exact_regime()
        assert regime == (s, w, h, int(slabs))
        got = beta_batch_run(batch, prec, [v for v, _ in probs], [h0 for _, h0 in probs], beta)
    for p, (V, H0) in enumerate(probs):
        case = '%s %s beta=%g B=%d p=%d %r' % (prec, ec.case_id(shape), beta, B, p, regime)
        assert got[p][4] == ITERS and not got[p][5]
        assert_same_bits(case, got[p], solo_beta(monkeypatch, prec, V, H0, k, regime, beta))
        check_against_reference(case, prec, got[p], reference(n, f, k, p, beta, False, prec != 'f64', kchunk, wchunk, True), beta)
    assert not np.array_equal(got[0][1], got[1][1])      # (the problems differ from one another)


# ---- 3. forced routes ---------------------------------------------------------------------------------------------------------------
FORCED = [('row_chunks', 1), ('row_chunks', 3), ('row_chunks', 7), ('w_chunks', 1), ('w_chunks', 3), ('h_seg', 100), ('h_seg', 128)]


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('forced', FORCED, ids=['%s-%d' % fv for fv in FORCED])
def test_forced_routes_on_the_batch(monkeypatch, prec, forced):
    """1000 x 300, k = 40 at beta = 0.5: the split W rule from two slab sets (w_chunks 3), H from slabs and from sums (row_chunks), H
    in segments (h_seg)."""
    n, f, k = ec.MID
    B, beta = 2, 0.5
    kw = {forced[0]: forced[1]}
    s, kchunk, w, wchunk, h, slabs = plan_of(prec, n, f, k, B, **kw)
    probs = [problem(n, f, k, p) for p in range(B)]
    set_switches(monkeypatch, **kw)
    with _native.Batch(prec, B) as batch:
        batch.set_problem(n, f, k, ITERS)
        regime = batch.exact_regime()
        assert regime == (s, w, h, int(slabs))
        got = beta_batch_run(batch, prec, [v for v, _ in probs], [h0 for _, h0 in probs], beta)
    for p, (V, H0) in enumerate(probs):
        case = '%s beta=0.5 %s=%d p=%d %r' % (prec, forced[0], forced[1], p, regime)
        assert_same_bits(case, got[p], solo_beta(monkeypatch, prec, V, H0, k, regime, beta, h_seg=kw.get('h_seg', 0)))
        check_against_reference(case, prec, got[p], reference(n, f, k, p, beta, False, prec != 'f64', kchunk, wchunk, True), beta)


# ---- 4. weights -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('beta', bc.BETAS)
def test_weights(monkeypatch, prec, beta):
    """Om on problems 0 and 1, none on problem 2, which must run as under weights of ones; V changed where Om = 0 leaves every bit;
    the W rule leaves the row whose weights are all zero as it was."""
    n, f, k = 300, 700, 17
    B = 3
    s, kchunk, w, wchunk, h, slabs = plan_of(prec, n, f, k, B)
    probs = [problem(n, f, k, p) for p in range(B)]
    Vs, H0s = [v for v, _ in probs], [h0 for _, h0 in probs]
    Oms = [weights(n, f, 0), weights(n, f, 1), None]
    V2s = [V.copy() for V in Vs]
    for V2, Om in zip(V2s[:2], Oms[:2]):
        V2[Om == 0] += 3.0
    set_switches(monkeypatch)
    with _native.Batch(prec, B) as batch:
        batch.set_problem(n, f, k, ITERS)
        regime = batch.exact_regime()
        got = beta_batch_run(batch, prec, Vs, H0s, beta, Oms=Oms)
        Ws = [ec.factors(n, f, k, seed=40 + p)[0] for p in range(B)]
        shown = beta_batch_run(batch, prec, Vs, H0s, beta, W_start=Ws)       # (the weights stay with the problem)
        hidden = beta_batch_run(batch, prec, V2s, H0s, beta, W_start=Ws)     # (W_start: W0 = V.H0^T is unweighted and sees V2)
        one = beta_batch_run(batch, prec, Vs, H0s, beta, iters=1, fit=False)
    for p in range(B):
        case = '%s weighted beta=%g p=%d' % (prec, beta, p)
        solo = solo_beta(monkeypatch, prec, Vs[p], H0s[p], k, regime, beta, Om=Oms[p] if Oms[p] is not None else np.ones((n, f)))
        assert_same_bits(case, got[p], solo)
        for a, b in zip(hidden[p][1:4], shown[p][1:4]):
            assert np.array_equal(a, b), case + ': V changed under zero weights changed a bit'
        assert hidden[p][4:] == shown[p][4:] and not np.array_equal(shown[p][1], got[p][1])
        check_against_reference(case, prec, got[p], reference(n, f, k, p, beta, p < 2, prec != 'f64', kchunk, wchunk, True), beta)
    for p in range(2):
        assert np.array_equal(one[p][1][ZERO_WEIGHT_ROW], one[p][0][ZERO_WEIGHT_ROW])
        assert not np.array_equal(one[p][1][ZERO_WEIGHT_ROW + 1], one[p][0][ZERO_WEIGHT_ROW + 1])
    assert not np.array_equal(one[2][1][ZERO_WEIGHT_ROW], one[2][0][ZERO_WEIGHT_ROW])


# ---- 5. problems that stop apart ----------------------------------------------------------------------------------------------------
STOP_SHAPE, STOP_CAP, STOP_BETA, STOP_TOL, STOP_SCALES, STOP_MARGIN = (300, 700, 17), 40, 0.5, 1000.0, (1e-4, 1.0, 64.0, 1600.0), 0.5


@functools.lru_cache(maxsize=2)
def stop_case(f32_inputs, kchunk, wchunk):
    """(Vs, H0s, the restatement's n_done per problem).  The restatement's record on 300 x 700, k = 17 at beta = 0.5 falls by about
    2e6, 2e4, 300, 54, 50 and then by 50 to 160 per iteration; the cost of data scaled by s falls s^0.5 times as much, so under
    tol_abs = 1000 the four scales stop the problems at the second, third and fourth evaluation and never.  Every fall next to a
    stop lies STOP_MARGIN or more (relative) off tol_abs, far beyond the fp32 loss's rounding (asserted here)."""
    n, f, k = STOP_SHAPE
    Vs = [s * problem(n, f, k, p)[0] for p, s in enumerate(STOP_SCALES)]
    H0s = [problem(n, f, k, p)[1] for p in range(len(Vs))]
    see = ec.as_f32 if f32_inputs else (lambda a: a)
    records = [bc.ref_fit(see(V), see(H0), STOP_CAP, STOP_BETA, kchunk=kchunk, wchunk=wchunk)[2] for V, H0 in zip(Vs, H0s)]
    done = [stop_rule(r, STOP_TOL) for r in records]
    for r, d in zip(records, done):
        falls = (r[:-1] - r[1:])[:d]      # (every fall the rule saw: the last one below tol_abs where it fired)
        assert np.all(np.abs(falls / STOP_TOL - 1.0) >= STOP_MARGIN), (falls, STOP_TOL)
    return Vs, H0s, done


@pytest.mark.parametrize('prec', PRECS)
def test_problems_that_stop_apart(monkeypatch, prec):
    n, f, k = STOP_SHAPE
    B = len(STOP_SCALES)
    s, kchunk, w, wchunk, h, slabs = plan_of(prec, n, f, k, B)
    Vs, H0s, ref_done = stop_case(prec != 'f64', kchunk, wchunk)
    tol = STOP_TOL
    assert ref_done == [2, 3, 4, STOP_CAP], ref_done
    set_switches(monkeypatch)
    with _native.Batch(prec, B) as batch:
        batch.set_problem(n, f, k, STOP_CAP)
        regime = batch.exact_regime()
        got = beta_batch_run(batch, prec, Vs, H0s, STOP_BETA, iters=STOP_CAP, tol_abs=tol)
    assert [g[4] for g in got] == ref_done
    assert [g[5] for g in got] == [d < STOP_CAP for d in ref_done]
    for p in range(B):
        solo = solo_beta(monkeypatch, prec, Vs[p], H0s[p], k, regime, STOP_BETA, iters=STOP_CAP, tol_abs=tol)
        assert_same_bits('%s stop p=%d' % (prec, p), got[p], solo)
        assert len(got[p][3]) == got[p][4]
        # frozen at its stop: W and H of exactly n_done iterations, whatever the others went on to do
        at_stop = solo_beta(monkeypatch, prec, Vs[p], H0s[p], k, regime, STOP_BETA, iters=got[p][4], cap=STOP_CAP)
        assert np.array_equal(got[p][1], at_stop[1]) and np.array_equal(got[p][2], at_stop[2]), p


# ---- 6. transform -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('beta', [0.5, 2.0])
@pytest.mark.parametrize('shape', [(65, 65, 65), (300, 700, 17)], ids=ec.case_id)
def test_transform_with_a_dictionary_per_problem(monkeypatch, prec, shape, beta):
    n, f, k = shape
    B = 3
    probs = [problem(n, f, k, p) for p in range(B)]
    s, kchunk, w, wchunk, h, slabs = plan_of(prec, n, f, k, B)
    set_switches(monkeypatch)
    with _native.Batch(prec, B) as batch:
        batch.set_problem(n, f, k, ITERS)
        regime = batch.exact_regime()
        got = beta_batch_run(batch, prec, [v for v, _ in probs], [h0 for _, h0 in probs], beta, fit=False)
    for p, (V, H0) in enumerate(probs):
        case = '%s %s beta=%g transform p=%d' % (prec, ec.case_id(shape), beta, p)
        assert np.array_equal(got[p][2], seen(prec, H0)), case + ': the dictionary changed'
        assert_same_bits(case, got[p], solo_beta(monkeypatch, prec, V, H0, k, regime, beta, fit=False))
        check_against_reference(case, prec, got[p], reference(n, f, k, p, beta, False, prec != 'f64', kchunk, wchunk, False), beta)


# ---- 7. back to beta = 1, and re-use ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', PRECS)
def test_beta_1_after_a_beta_run_is_the_kl_batch(monkeypatch, prec):
    from tests.test_batch_gpu import batch_run
    n, f, k = 300, 700, 17
    B = 3
    probs = [problem(n, f, k, p) for p in range(B)]
    Vs, H0s = [v for v, _ in probs], [h0 for _, h0 in probs]
    set_switches(monkeypatch)
    with _native.Batch(prec, B) as batch:
        batch.set_problem(n, f, k, ITERS)
        kl = batch_run(batch, prec, Vs, H0s)                  # a batch that never saw another cost
    with _native.Batch(prec, B) as batch:
        batch.set_problem(n, f, k, ITERS)
        first = beta_batch_run(batch, prec, Vs, H0s, 0.5, Oms=[weights(n, f, 0), None, None])
        again = beta_batch_run(batch, prec, Vs, H0s, 0.5)
        batch.set_divergence(1.0)
        assert batch.get_divergence() == 1.0
        back = batch_run(batch, prec, Vs, H0s)
        batch.set_divergence(3.0)                             # (and the weights went with beta = 1)
        unweighted = beta_batch_run(batch, prec, Vs, H0s, 3.0)
        batch.set_problem(n, f, k, ITERS)
        assert batch.get_divergence() == 1.0                  # set_problem returns the batch to the KL loop
        fresh = batch_run(batch, prec, Vs, H0s)
    for p, (V, H0) in enumerate(probs):
        case = '%s p=%d' % (prec, p)
        assert_same_bits(case + ' two beta runs', again[p], first[p])
        assert_same_bits(case + ' beta = 1 after beta = 0.5', back[p], kl[p])
        assert_same_bits(case + ' set_problem after beta', fresh[p], kl[p])
        assert not np.array_equal(first[p][1], kl[p][1])
        assert_same_bits(case + ' beta = 3 without the weights', unweighted[p], solo_beta(
            monkeypatch, prec, V, H0, k, ec.query_regime(n, f, k, max(1, cu_count() // B), esize=esize(prec)), 3.0))


# ---- 8. refusals leave the batch usable ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', PRECS)
def test_refusals_leave_the_batch_usable(monkeypatch, prec):
    import scipy.sparse as sp
    n, f, k = 65, 65, 65
    B = 2
    probs = [problem(n, f, k, p) for p in range(B)]
    Vs, H0s = [v for v, _ in probs], [h0 for _, h0 in probs]
    Om = upload_form(prec, weights(n, f, 0))
    set_switches(monkeypatch)

    def same(a, b):
        for p in range(B):
            assert_same_bits('%s refusals p=%d' % (prec, p), a[p], b[p])
    with _native.Batch(prec, B) as batch:
        raises(_native.ERR_ARG, batch.set_divergence, 0.5)                         # no problem yet
        batch.set_problem(n, f, k, ITERS)
        first = beta_batch_run(batch, prec, Vs, H0s, 0.5)
        # a beta that is not finite; in f32 a beta that fp32 rounds to 1 or to 0 without being it
        for bad in (float('nan'), float('inf'), -float('inf')):
            raises(_native.ERR_ARG, batch.set_divergence, bad)
        for edge in (1.0 + 1e-12, 1e-50):
            if prec == 'f32':
                raises(_native.ERR_ARG, batch.set_divergence, edge)
            else:
                batch.set_divergence(edge)
                assert batch.get_divergence() == edge
        assert batch.get_divergence() == (0.5 if prec == 'f32' else 1e-50)
        # p out of range
        raises(_native.ERR_ARG, batch.upload_weights, B, Om)
        raises(_native.ERR_ARG, batch.upload_weights, -1, Om)
        # a presence mask on a beta batch
        raises(_native.ERR_UNSUPP, batch.upload_presence, 0, np.ones((n, 1)), [0, f])
        assert batch.presence() == 0
        same(beta_batch_run(batch, prec, Vs, H0s, 0.5), first)
        # the other order: the cost on a masked batch; weights on a beta = 1 batch
        batch.set_divergence(1.0)
        raises(_native.ERR_UNSUPP, batch.upload_weights, 0, Om)
        batch.upload_presence(0, np.ones((n, 1)), [0, f])
        raises(_native.ERR_UNSUPP, batch.set_divergence, 0.5)
        assert batch.presence() == 1 and batch.get_divergence() == 1.0
        batch.clear_presence()
        same(beta_batch_run(batch, prec, Vs, H0s, 0.5), first)
        # a CSR batch
        X = sp.csr_matrix(Vs[0])
        batch.set_problem_sparse(n, f, k, ITERS, [X.nnz] * B)
        raises(_native.ERR_UNSUPP, batch.set_divergence, 0.5)
        raises(_native.ERR_UNSUPP, batch.upload_weights, 0, Om)
        assert batch.get_divergence() == 1.0
        batch.set_problem(n, f, k, ITERS)
        same(beta_batch_run(batch, prec, Vs, H0s, 0.5), first)


# ---- 9. the public route ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'weighted'])
def test_fit_transform_batch_against_a_loop_over_fit_transform(prec, weighted):
    """From the same seed: the dictionaries drawn are the same; the results are equal within the fit bars (the batch plans for its
    share of the chip), and bit for bit where the batch's chunk counts are the context's."""
    from multimodal_amd.lib.beta_nmf import BetaNMF, fit_transform_batch
    n, f, k = 300, 700, 17
    B, beta = 3, 0.5
    Xs = [problem(n, f, k, p)[0] for p in range(B)]
    Oms = [weights(n, f, 0), None, weights(n, f, 2)] if weighted else None

    def models():
        return [BetaNMF(beta=beta, n_components=k, max_iter=ITERS, tol=0, precision=prec, device=0) for _ in range(B)]
    batched = models()
    np.random.seed(21)
    outs = fit_transform_batch(batched, Xs, weights=Oms, return_errors=True)
    after = np.random.random()
    alone = models()
    np.random.seed(21)
    refs = [m.fit_transform(X, return_errors=True, **({} if Oms is None else {'weights': Oms[p]})) for p, (m, X) in enumerate(zip(alone, Xs))]
    assert np.random.random() == after
    same_plan = ec.query_regime(n, f, k, cu_count(), esize=esize(prec)) == ec.query_regime(n, f, k, max(1, cu_count() // B), esize=esize(prec))
    for p, (m, a, (W, errors), (Wa, ea)) in enumerate(zip(batched, alone, outs, refs)):
        case = '%s fit_transform_batch %s p=%d' % (prec, 'weighted' if weighted else 'plain', p)
        assert m.last_batch_size == B and len(errors) == len(ea) == ITERS
        assert m.last_weights_route == ('array' if weighted else None)
        W0 = ec.ref_init_W(seen(prec, Xs[p]), np.full((k, f), 1.0 / f), None)
        check(case, 'losses', errors, ea, BARS[prec]['fit_loss'],
              loss_floor(prec, seen(prec, Xs[p]), None if Oms is None or Oms[p] is None else Oms[p], W0, np.full((k, f), 1.0 / f), beta))
        check(case, 'W', W, Wa, BARS[prec]['fit_factor'], FLOOR[prec])
        check(case, 'H', m.components_, a.components_, BARS[prec]['fit_factor'], FLOOR[prec])
        if same_plan and (not weighted or Oms[p] is not None):
            assert np.array_equal(W, Wa) and list(errors) == list(ea) and np.array_equal(m.components_, a.components_), case
