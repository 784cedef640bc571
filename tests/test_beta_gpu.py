"""The beta-divergence loop (multimodal_amd/csrc/beta.hip.h, include/klnmf_beta.h) against its fp64 restatement
(tests/beta_cases.py) on every route of the exact plan.

Driven through `_native.Context`, so that every test asserts which route ran (`exact_regime()`), as test_exact_gpu does:
  * the smallest cases of exact_cases.CASES that reach each route, beta in {0, 0.5, 2, 3}, in f64 (and in f32 on four of them):
    `beta_loss`, one W step and one H step of `beta_step`, a 10-iteration fit and a 10-iteration transform of `run`;
  * the same with weights (30 % zeros, a row of zeros) on two cases; V changed wherever the weight is 0 leaves every output bit
    as it was; a row of zero weights keeps its W;
  * 1, 3, 7 row chunks, 1, 3 W chunks and H segments of 100 and 128 columns forced on 1000 x 300, k = 40 at beta = 0.5, each
    against the restatement and against the natural route;
  * descent: 30 iterations on 300 x 700, k = 17 for beta in {0, 0.5, 1.5, 2, 3}, with and without weights -- no loss exceeds its
    predecessor by more than 1e-12 relative, and the last is below the first;
  * beta = 1: `BetaNMF(beta=1)` and `KLdivNMF` bit for bit on a dense, a weighted, a presence-column and a CSR input;
    `set_divergence(1.0)` after `set_divergence(0.5)` gives the KL loop's bits; two runs of one fit give the same bits;
  * the normalisation, the refusals (each leaving the context usable) and `MultimodalLearner(beta=2)`;
  * a context takes the beta cost after a group run and after a loop nobody ended, out of the context pool too; in f32 a beta
    that fp32 rounds to 1 or 0 is refused.
Fits never stop early (tol = exact_cases.NO_STOP).

Bars: test_exact_gpu's own, imported (BARS, FLOOR, FORCED_VS_NATURAL), relative, element by element -- f64: steps 1e-12, fit
losses 1e-10, W and H 1e-9, floor 0; f32 (the restatement fed the fp32-rounded inputs): 3e-5 / 3e-5 / 3e-4 relative to at least
the smallest normal fp32 number.  The f32 losses have a floor of this module's own, `loss_floor`, in the role of
`test_exact_gpu.loss_floor` (2^-23 sum(V) there: the fp32 kernels form the loss terms in fp32), not of FLOOR: 2^-23 of the summed
magnitudes of the beta cost's terms; it lies orders of magnitude below every loss compared here and widens no bar.  gamma <= 1, so the
rules' power amplifies nothing, and exp(c log y) adds about |c log y| ulps: under 40 at y = 1e-8, |c| <= 2.
Measured on the MI355X (worst over every case and beta): f64 steps 4.1e-15, fit losses 1.9e-15, fit W 4.6e-15, fit H 9.7e-15,
forced against natural 1.1e-14; f32 steps 1.9e-6, fit losses 6.3e-7, fit W 4.9e-6, fit H 3.3e-6; descent: the worst step of every
record is a fall (the smallest, 2.5e-4 relative at beta = 3); beta = 1 against KLdivNMF, two runs and V changed under zero
weights 0.  No bar was widened.
The measured worst errors are printed after each test (pytest -v), are in each assertion message and are kept in
profiles/beta_gpu_tests.txt.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from multimodal_amd import _native
from multimodal_amd.learner import MultimodalLearner
from multimodal_amd.lib import nmf
from tests import beta_cases as bc
from tests import exact_cases as ec
from tests.test_exact_gpu import BARS, FLOOR, FORCED_VS_NATURAL, cu_count, esize, open_problem
from tests.test_exact_gpu import problem as exact_problem
from tests.test_sparse_gpu import _MEASURED, _report_measured, check  # noqa: F401  (the autouse fixture prints what was measured)

pytestmark = pytest.mark.gpu

ITERS = 10
CASES = [(15, 17, 1), (65, 65, 65), (300, 700, 17), (300, 700, 129), (16384, 300, 64), (4096, 128, 16), (4096, 129, 16),
         (100, 16385, 33), (70001, 64, 8)]
F32_CASES = [(15, 17, 1), (65, 65, 65), (300, 700, 17), (300, 700, 129)]
WEIGHTED_CASES = [(300, 700, 17), (4096, 129, 16)]
FORCED = [('row_chunks', 1), ('row_chunks', 3), ('row_chunks', 7), ('w_chunks', 1), ('w_chunks', 3), ('h_seg', 100), ('h_seg', 128)]
ZERO_WEIGHT_ROW = 5


def test_the_cases_are_exact_cases():
    assert set(CASES) <= set(c[:3] for c in ec.CASES) and set(F32_CASES) <= set(CASES) and set(WEIGHTED_CASES) <= set(CASES)


@functools.lru_cache(maxsize=4)
def problem(n, f, k, weighted):
    """(V, Om or None, W, H) in fp64: test_exact_gpu's problem (a zero row and a zero column of V)."""
    V, W, H = exact_problem(n, f, k)
    Om = bc.weights_of(n, f, seed=3 * n + 5 * f + k, zero_row=ZERO_WEIGHT_ROW) if weighted else None
    return V, Om, W, H


def inputs(prec, *arrays):
    """The restatement's inputs (what the kernels of `prec` see, in fp64) and the arrays to upload."""
    if prec == 'f64':
        return arrays, arrays
    return (tuple(None if a is None else ec.as_f32(a) for a in arrays),
            tuple(None if a is None else np.asarray(a, np.float32) for a in arrays))


@functools.lru_cache(maxsize=4)
def reference(n, f, k, weighted, beta, f32_inputs, kchunk, wchunk, iters=ITERS):
    """(loss, W step, H step, fit, transform) of the restatement on the case's inputs, summed over the kernels' chunks."""
    V, Om, W, H = problem(n, f, k, weighted)
    if f32_inputs:
        V, Om, W, H = (None if a is None else ec.as_f32(a) for a in (V, Om, W, H))
    loss, Wn = bc.ref_W_step(V, W, H, beta, Om, wchunk)
    Ws, Hn, _ = bc.ref_H_step(V, W, H, beta, Om, kchunk)
    fit = bc.ref_fit(V, H, iters, beta, Om=Om, kchunk=kchunk, wchunk=wchunk)
    transform = bc.ref_fit(V, H, iters, beta, Om=Om, fit=False, components=H, kchunk=kchunk, wchunk=wchunk)
    return loss, Wn, (Ws, Hn), fit, transform


def open_beta(monkeypatch, prec, Vu, Omu, k, cap, beta, **forced):
    ctx = open_problem(monkeypatch, prec, Vu, k, cap, **forced)
    if Omu is not None:
        ctx.upload_weights(Omu)
    assert ctx.get_divergence() == 1.0
    ctx.set_divergence(beta)
    assert ctx.get_divergence() == beta and ctx.weighted() == (Omu is not None)
    return ctx


def gpu_steps(ctx, W, H):
    """(loss, W of the W step, (W, H) of the H step), each at (W, H)."""
    ctx.set_H(H)
    ctx.set_W(W)
    loss = ctx.beta_loss()
    ctx.beta_step(0)
    Wn = ctx.get_W()
    ctx.set_H(H)
    ctx.set_W(W)
    ctx.beta_step(1)
    return loss, Wn, (ctx.get_W(), ctx.get_H())


def gpu_fit(ctx, H0, iters=ITERS, fit=True, W0=None):
    """`iters` iterations of klnmf_run from W0 = V.H0^T (or from the W given); fit=False holds H0."""
    ctx.set_H(H0)
    if W0 is None:
        ctx.init_W()
    else:
        ctx.set_W(W0)
    errors, n_done, _ = ctx.run(iters, fit, ec.NO_STOP)
    assert n_done == len(errors) == iters
    return ctx.get_W(), ctx.get_H(), np.array(errors)


def loss_floor(prec, V, Om, W, H, beta):
    """The fp32 kernels form the cost's terms in fp32: its losses relative to at least 2^-23 of the largest summed term."""
    if prec == 'f64':
        return 0.0
    x, y = V + bc.EPS, W.dot(H) + bc.EPS
    w = 1.0 if Om is None else Om
    if beta == 2.0:
        terms = 0.5 * (x * x + y * y)
    elif beta == 0.0:
        terms = x / y + np.abs(np.log(x / y)) + 1.0
    else:
        terms = (x ** beta + abs(beta - 1.0) * y ** beta + abs(beta) * x * y ** (beta - 1.0)) / abs(beta * (beta - 1.0))
    return 2.0 ** -23 * float((w * terms).sum())


def check_steps(case, prec, got, ref, floor_loss):
    bar = BARS[prec]['step']
    check(case, 'loss', got[0], ref[0], bar, floor_loss)
    check(case, 'W rule', got[1], ref[1], bar, FLOOR[prec])
    check(case, 'H: W', got[2][0], ref[2][0], bar, FLOOR[prec])
    check(case, 'H rule', got[2][1], ref[2][1], bar, FLOOR[prec])


def check_fit(case, prec, got, ref, floor_loss, bars=None):
    bars = bars or BARS[prec]
    assert len(got[2]) == len(ref[2])
    check(case, 'losses', got[2], ref[2], bars['fit_loss'], floor_loss)
    check(case, 'W', got[0], ref[0], bars['fit_factor'], FLOOR[prec])
    check(case, 'H', got[1], ref[1], bars['fit_factor'], FLOOR[prec])


def run_case(monkeypatch, prec, shape, beta, weighted=False, **forced):
    """`beta_loss`, one W step, one H step, a fit and a transform on the (forced) route against the restatement; returns what
    the device gave."""
    n, f, k = shape
    V, Om, W, H = problem(n, f, k, weighted)
    (Vr, Omr, Wr, Hr), (Vu, Omu, Wu, Hu) = inputs(prec, V, Om, W, H)
    s, kchunk, w, wchunk, h, slabs = ec.exact_regime(n, f, k, cu_count(), esize(prec), **forced)
    ref = reference(n, f, k, weighted, beta, prec != 'f64', kchunk, wchunk)
    floor_loss = loss_floor(prec, Vr, Omr, Wr, Hr, beta)
    case = '%s %s beta=%g %s%s(%d, %d, %d, %d)' % (prec, ec.case_id(shape), beta, 'weighted ' if weighted else '',
                                                  ''.join('%s=%d ' % kv for kv in forced.items()), s, w, h, slabs)
    with open_beta(monkeypatch, prec, Vu, Omu, k, ITERS, beta, **forced) as ctx:
        assert ctx.exact_regime() == (s, w, h, int(slabs))
        got_steps = gpu_steps(ctx, Wu, Hu)
        check_steps(case + ' step', prec, got_steps, ref, floor_loss)
        got_fit = gpu_fit(ctx, Hu)
        check_fit(case + ' fit', prec, got_fit, ref[3], floor_loss)
        check_fit(case + ' transform', prec, gpu_fit(ctx, Hu, fit=False), ref[4], floor_loss)
    return got_steps, got_fit


@pytest.mark.parametrize('beta', bc.BETAS)
@pytest.mark.parametrize('shape', CASES, ids=ec.case_id)
def test_every_route_in_f64(monkeypatch, shape, beta):
    run_case(monkeypatch, 'f64', shape, beta)


@pytest.mark.parametrize('beta', bc.BETAS)
@pytest.mark.parametrize('shape', F32_CASES, ids=ec.case_id)
def test_the_small_cases_in_f32(monkeypatch, shape, beta):
    run_case(monkeypatch, 'f32', shape, beta)


@pytest.mark.parametrize('beta', bc.BETAS)
@pytest.mark.parametrize('shape', WEIGHTED_CASES, ids=ec.case_id)
def test_weighted(monkeypatch, shape, beta):
    run_case(monkeypatch, 'f64', shape, beta, weighted=True)


@pytest.mark.parametrize('beta', bc.BETAS)
def test_weighted_in_f32(monkeypatch, beta):
    run_case(monkeypatch, 'f32', WEIGHTED_CASES[0], beta, weighted=True)


@pytest.mark.parametrize('beta', bc.BETAS)
@pytest.mark.parametrize('shape', WEIGHTED_CASES, ids=ec.case_id)
def test_a_zero_weight_hides_the_entry_and_a_row_of_zeros_keeps_its_w(monkeypatch, shape, beta):
    """V changed wherever Om = 0: the loss, both steps and a fit from the same (W, H) keep every bit.  The W rule leaves the row
    whose weights are all zero as it was."""
    n, f, k = shape
    V, Om, W, H = problem(n, f, k, True)
    V2 = V.copy()
    V2[Om == 0] += 3.0
    got = []
    for data in (V, V2):
        with open_beta(monkeypatch, 'f64', data, Om, k, ITERS, beta) as ctx:
            steps = gpu_steps(ctx, W, H)
            got.append((steps[0], steps[1]) + steps[2] + gpu_fit(ctx, H, W0=W))
    assert got[0][0] == got[1][0]
    for a, b in zip(got[0][1:], got[1][1:]):
        assert np.array_equal(a, b)
    assert np.array_equal(got[0][1][ZERO_WEIGHT_ROW], W[ZERO_WEIGHT_ROW])
    assert not np.array_equal(got[0][1][ZERO_WEIGHT_ROW + 1], W[ZERO_WEIGHT_ROW + 1])


@pytest.mark.parametrize('forced', FORCED, ids=lambda v: '%s=%d' % v)
def test_forced_routes(monkeypatch, forced):
    """1000 x 300, k = 40 at beta = 0.5 on a forced route against the restatement summed over the forced chunks, and against the
    same problem on its natural route."""
    shape, beta = ec.MID, 0.5
    n, f, k = shape
    got_steps, got_fit = run_case(monkeypatch, 'f64', shape, beta, **dict([forced]))
    V, _, W, H = problem(n, f, k, False)
    with open_beta(monkeypatch, 'f64', V, None, k, ITERS, beta) as nat:
        assert nat.exact_regime() == ec.query_regime(n, f, k, cu_count())
        nat_steps = gpu_steps(nat, W, H)
        nat_fit = gpu_fit(nat, H)
    case = 'f64 %s beta=0.5 %s=%d' % ((ec.case_id(shape),) + forced)
    flat = lambda s: (s[0], s[1], s[2][0], s[2][1])
    for what, a, b in zip(('loss', 'W rule', 'H: W', 'H rule'), flat(got_steps), flat(nat_steps)):
        check(case + ' vs natural', what, a, b, FORCED_VS_NATURAL['step'])
    for what, a, b in zip(('W', 'H', 'losses'), got_fit, nat_fit):
        check(case + ' fit vs natural', what, a, b, FORCED_VS_NATURAL['fit'])


@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'weighted'])
@pytest.mark.parametrize('beta', bc.DESCENT_BETAS)
def test_descent(monkeypatch, beta, weighted):
    """30 iterations on 300 x 700, k = 17: no loss exceeds its predecessor by more than 1e-12 relative (the restatement's own worst
    step on this input is a rise of exactly 0: test_beta_cpu), and the last loss is below the first."""
    n, f, k = 300, 700, 17
    V, Om, _, H = problem(n, f, k, weighted)
    with open_beta(monkeypatch, 'f64', V, Om, k, 30, beta) as ctx:
        _, _, losses = gpu_fit(ctx, H, iters=30)
    rise = bc.worst_rise(losses)
    _MEASURED.append('    descent beta=%g %s: worst relative rise %.2e, loss %.6g -> %.6g' % (beta, 'weighted' if weighted else 'plain', rise,
                                                                                             losses[0], losses[-1]))
    assert rise <= bc.DESCENT_RISE, (rise, losses)
    assert losses[-1] < losses[0]


# ---- beta = 1 is KLdivNMF ----------------------------------------------------------------------------------------------------------------
def kl_inputs(kind):
    n, f, k = 300, 700, 17
    V, Om, _, H0 = problem(n, f, k, True)
    kw = {}
    if kind == 'weighted':
        kw['weights'] = Om
    if kind == 'presence':
        kw['weights'] = (Om[:, :1] > 0).astype(np.float64)
    if kind == 'csr':
        V = sp.csr_matrix(V * (Om > 0))
    return V, H0, k, kw


@pytest.mark.parametrize('kind', ['dense', 'weighted', 'presence', 'csr'])
def test_beta_1_is_kldivnmf_bit_for_bit(kind):
    from multimodal_amd.lib import BetaNMF
    V, H0, k, kw = kl_inputs(kind)
    got = []
    for cls, extra in ((nmf.KLdivNMF, {}), (BetaNMF, {'beta': 1.0})):
        m = cls(n_components=k, max_iter=ITERS, tol=ec.NO_STOP, precision='f64', **extra)
        m._init_dictionary = H0
        W, errors = m.fit_transform(V, return_errors=True, **kw)
        got.append((W, m.components_, np.array(errors), m.transform(V, **kw), np.float64(m.error(V, W, **kw)), m.last_weights_route))
    assert got[0][-1] == got[1][-1] == {'dense': None, 'weighted': 'array', 'presence': 'presence', 'csr': None}[kind]
    for a, b in zip(got[0][:-1], got[1][:-1]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'weighted'])
def test_back_to_beta_1_gives_the_kl_loops_bits_and_two_runs_agree(monkeypatch, weighted):
    n, f, k = ec.MID
    V, Om, _, H = problem(n, f, k, weighted)
    with open_problem(monkeypatch, 'f64', V, k, ITERS) as ctx:
        if weighted:
            ctx.upload_weights(Om)
        want = gpu_fit(ctx, H)
    with open_beta(monkeypatch, 'f64', V, Om, k, ITERS, 0.5) as ctx:
        first = gpu_fit(ctx, H)
        second = gpu_fit(ctx, H)
        ctx.set_divergence(1.0)
        assert ctx.get_divergence() == 1.0 and ctx.weighted() == weighted
        back = gpu_fit(ctx, H)
        ctx.set_divergence(0.5)
        third = gpu_fit(ctx, H)
    for a, b, c, d, e in zip(want, back, first, second, third):
        assert np.array_equal(a, b) and np.array_equal(c, d) and np.array_equal(c, e) and not np.array_equal(a, c)


def test_the_loop_in_pieces_and_the_single_update_run_the_beta_rules(monkeypatch):
    """klnmf_loop_begin + the pieces, and klnmf_update, on a beta context: the same iteration (the H rule from the summed slabs)."""
    n, f, k = ec.MID
    beta = 0.5
    V, _, W, H = problem(n, f, k, False)
    _, kchunk, _, wchunk, _, _ = ec.exact_regime(n, f, k, cu_count())
    with open_beta(monkeypatch, 'f64', V, None, k, ITERS, beta) as ctx:
        ctx.set_H(H)
        ctx.init_W()
        ctx.loop_begin()
        for it in range(ITERS):
            ctx.iter_rowpass(True)
            if it == 3:      # the cost may not change between the pieces of an open loop
                for other in (2.0, 1.0):
                    assert 'klnmf_loop_end' in refused(lambda: ctx.set_divergence(other))
                assert ctx.get_divergence() == beta
            ctx.iter_decide(ec.NO_STOP)
            ctx.iter_colpass()
            ctx.iter_update_H()
            ctx.iter_advance()
        errors, n_done, _ = ctx.loop_end(ITERS)
        pieces = (ctx.get_W(), ctx.get_H(), np.array(errors))
        check_fit('f64 pieces beta=0.5', 'f64', pieces, bc.ref_fit(V, H, ITERS, beta, kchunk=kchunk, wchunk=wchunk), 0.0)
        ctx.set_H(H)
        ctx.set_W(W)
        ctx.update(True)
        _, Wr, Hr = bc.ref_iteration(V, W, H, beta, None, kchunk, wchunk)
        check('f64 update beta=0.5', 'W', ctx.get_W(), Wr, BARS['f64']['step'])
        check('f64 update beta=0.5', 'H', ctx.get_H(), Hr, BARS['f64']['step'])
        for step in (ctx.step_Q, ctx.step_W, ctx.step_H, ctx.error):      # (the KL steps and the KL loss: not this context's)
            refused(step)
        own = ctx.exchange_buffers()[:2]
        assert 'denominator' in refused(lambda: ctx.bind_exchange(*own))      # a caller's exchange: not on a beta context
        check('f64 beta_loss after the refusals', 'loss', ctx.beta_loss(), bc.cost(V, ctx.get_W(), ctx.get_H(), beta), BARS['f64']['step'])
        ctx.set_divergence(1.0)
        ctx.bind_exchange(*own)                                              # ... and a bound exchange refuses the beta cost
        assert 'klnmf_bind_exchange' in refused(lambda: ctx.set_divergence(beta))
        assert ctx.get_divergence() == 1.0 and np.isfinite(ctx.error())


def test_normalisation():
    """After a fit `components_` rows sum to 1 within 1e-15 f; one H step leaves W.H equal to the product with the un-normalised
    H within the step bar."""
    from multimodal_amd.lib import BetaNMF
    n, f, k = 300, 700, 17
    V, _, W, H = problem(n, f, k, False)
    for beta in bc.BETAS:
        m = BetaNMF(beta=beta, n_components=k, max_iter=ITERS, tol=ec.NO_STOP, precision='f64')
        m._init_dictionary = H
        m.fit_transform(V)
        assert np.abs(m.components_.sum(axis=1) - 1.0).max() <= 1e-15 * f
        with _native.Context('f64') as ctx:
            ctx.set_problem(n, f, k, 1)
            ctx.upload_V(V)
            ctx.set_divergence(beta)
            _, _, (Ws, Hn) = gpu_steps(ctx, W, H)
        _, _, Hu = bc.ref_H_step(V, W, H, beta, kchunk=ec.exact_regime(n, f, k, cu_count())[1])
        check('f64 normalisation beta=%g' % beta, 'W.H', Ws.dot(Hn), W.dot(Hu), BARS['f64']['step'])


def test_the_public_api_against_the_restatement(capsys):
    """BetaNMF.fit_transform / transform / error with a (f,) weight vector in f64, and in 'f16' (run in f32, said once)."""
    from multimodal_amd.lib import BetaNMF
    n, f, k = 300, 700, 17
    beta = 0.5
    V, Om, W, H0 = problem(n, f, k, True)
    w = Om[7]
    full = np.broadcast_to(w, (n, f))
    _, kchunk, _, wchunk, _, _ = ec.exact_regime(n, f, k, cu_count())
    m = BetaNMF(beta=beta, n_components=k, max_iter=ITERS, tol=ec.NO_STOP, precision='f64')
    m._init_dictionary = H0
    Wg, errors = m.fit_transform(V, weights=w, return_errors=True)
    assert m.last_weights_route == 'array'
    check_fit('f64 BetaNMF.fit_transform', 'f64', (Wg, m.components_, np.array(errors)),
              bc.ref_fit(V, H0, ITERS, beta, Om=full, kchunk=kchunk, wchunk=wchunk), 0.0)
    check('f64 BetaNMF.error', 'loss', m.error(V, W, H=H0, weights=w), bc.cost(V, W, H0, beta, full), BARS['f64']['step'])
    nmf._NOTED.clear()
    capsys.readouterr()
    Vr, Omr, Hr = (ec.as_f32(a) for a in (V, full, H0))
    _, kchunk, _, wchunk, _, _ = ec.exact_regime(n, f, k, cu_count(), 4)
    ref = bc.ref_fit(Vr, Hr, ITERS, beta, Om=Omr, kchunk=kchunk, wchunk=wchunk)
    for _ in range(2):
        m = BetaNMF(beta=beta, n_components=k, max_iter=ITERS, tol=ec.NO_STOP, precision='f16')
        m._init_dictionary = H0.astype(np.float32)
        Wg, errors = m.fit_transform(V.astype(np.float32), weights=w.astype(np.float32), return_errors=True)
        check_fit('f16 -> f32 BetaNMF.fit_transform', 'f32', (Wg, m.components_, np.array(errors)), ref,
                  loss_floor('f32', Vr, Omr, ec.ref_init_W(Vr, Hr), Hr, beta))
    err = capsys.readouterr().err
    assert err.count("BetaNMF: beta != 1 with precision='f16' runs on the fp32 beta kernels") == 1 and err.count('\n') == 1, err
    with pytest.raises(ValueError):
        m.fit_transform(sp.csr_matrix(V))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def refused(call, code=_native.ERR_UNSUPP):
    with pytest.raises(_native.NativeError) as e:
        call()
    assert e.value.code == code, e.value
    return str(e.value)


def test_refusals_leave_the_context_usable(monkeypatch):
    n, f, k = 64, 256, 16
    V, Om, W, H = problem(n, f, k, True)
    # a CSR problem
    with _native.Context('f64') as ctx:
        ctx.set_problem_sparse(sp.csr_matrix(V * (Om > 0)), k, 2)
        ctx.set_H(H)
        ctx.set_W(W)
        before = ctx.error()
        assert 'CSR' in refused(lambda: ctx.set_divergence(0.5))
        assert ctx.get_divergence() == 1.0 and ctx.error() == before and ctx.beta_loss() == before
    # a 16-bit context
    with _native.Context('f16') as ctx:
        ctx.set_problem(n, f, k, 2)
        ctx.upload_blocks([V])
        assert 'KLNMF_PREC_F64' in refused(lambda: ctx.set_divergence(2.0))
        ctx.set_H(H)
        ctx.init_W()
        errors, n_done, _ = ctx.run(2, True, ec.NO_STOP)
        assert n_done == 2 and np.all(np.isfinite(errors))
    with open_problem(monkeypatch, 'f64', V, k, 2) as ctx:
        want_kl = gpu_fit(ctx, H, 2)
        # a non-finite beta
        for bad in (float('nan'), float('inf')):
            refused(lambda: ctx.set_divergence(bad), _native.ERR_ARG)
        refused(lambda: ctx.beta_step(0))                      # (beta = 1: klnmf_step_* are its steps)
        # a presence mask, either way round
        ctx.upload_presence((Om[:, :2] > 0).astype(np.float64), [0, 100, f])
        masked = gpu_fit(ctx, H, 2)
        assert 'presence' in refused(lambda: ctx.set_divergence(0.5))
        assert ctx.get_divergence() == 1.0
        for a, b in zip(gpu_fit(ctx, H, 2), masked):
            assert np.array_equal(a, b)
        ctx.clear_weights()
        ctx.set_divergence(0.5)
        want = gpu_fit(ctx, H, 2)
        refused(lambda: ctx.upload_presence((Om[:, :2] > 0).astype(np.float64), [0, 100, f]))
        refused(lambda: ctx.beta_step(2), _native.ERR_ARG)
        # a group: at its creation on a beta context, and klnmf_set_divergence on a member
        refused(lambda: _native.Group([ctx]))
        # the loop sequenced by the caller over row shards
        refused(lambda: ctx.loop_begin(1.0, 1.0))
        for a, b in zip(gpu_fit(ctx, H, 2), want):
            assert np.array_equal(a, b)
        ctx.set_divergence(1.0)
        gpu_fit(ctx, H, 2)
        with _native.Group([ctx]):
            assert 'group' in refused(lambda: ctx.set_divergence(0.5))
            assert ctx.get_divergence() == 1.0
        ctx.loop_begin(float(V.sum()), float(n * f))
        assert 'row shards' in refused(lambda: ctx.set_divergence(0.5))
        ctx.loop_end(2)
        for a, b in zip(gpu_fit(ctx, H, 2), want_kl):
            assert np.array_equal(a, b)


def test_a_group_run_or_an_abandoned_loop_leaves_no_loop_open_behind_it():
    """A context that was a member of klnmf_group_run, or whose klnmf_loop_begin never met its klnmf_loop_end, takes the beta
    cost on its next problem -- also when it comes back out of the pool of `Context(pooled=True)`, as KLdivNMF's device-list
    fits leave it there for the next BetaNMF."""
    n, f, k = 64, 256, 16
    beta = 0.5
    V, _, W, H = problem(n, f, k, False)

    def fresh_problem(ctx):
        ctx.set_problem(n, f, k, 2)
        ctx.upload_blocks([V])

    with _native.Context('f64') as ctx:
        fresh_problem(ctx)
        ctx.set_divergence(beta)
        want = gpu_fit(ctx, H, 2)

    def beta_fit_is_as_ever(ctx):
        fresh_problem(ctx)
        ctx.set_divergence(beta)
        for a, b in zip(gpu_fit(ctx, H, 2), want):
            assert np.array_equal(a, b)

    with _native.Context('f64') as ctx:
        fresh_problem(ctx)
        ctx.set_H(H)
        ctx.init_W()
        with _native.Group([ctx]) as group:
            _, n_done, _ = group.run(n, 2, True, 0.0)
            assert n_done == 2
        ctx.set_divergence(beta)              # on the group's own problem, the group gone
        assert ctx.get_divergence() == beta
        beta_fit_is_as_ever(ctx)              # ... and on the next one
        ctx.set_divergence(1.0)
        ctx.loop_begin()                      # a loop that nobody ends
        ctx.iter_rowpass(True)
        assert 'klnmf_loop_end' in refused(lambda: ctx.set_divergence(beta))
        beta_fit_is_as_ever(ctx)              # its problem's end is its end
    handles = []
    for _ in range(2):                        # through the pool: the second Context is the first one's handle
        with _native.Context('f64', pooled=True) as ctx:
            handles.append(ctx._h.value)
            if len(handles) == 2:
                beta_fit_is_as_ever(ctx)
                continue
            fresh_problem(ctx)
            ctx.set_H(H)
            ctx.init_W()
            with _native.Group([ctx]) as group:
                group.run(n, 2, True, 0.0)
    assert handles[0] == handles[1]


def test_a_beta_that_fp32_rounds_to_1_or_0_is_refused_in_f32(monkeypatch):
    """The fp32 kernels see (float)beta: a beta within 2^-25 of 1, or a denormal-small one, would run the general cost with
    beta (beta - 1) = 0.  KLNMF_ERR_ARG, the context as it was; f64 takes the same values, and 1 and 0 themselves pass."""
    n, f, k = 15, 17, 1
    V, _, W, H = problem(n, f, k, False)
    with open_problem(monkeypatch, 'f32', V.astype(np.float32), k, 2) as ctx:
        for bad in (1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30, 1e-60, -1e-60):
            assert 'fp32' in refused(lambda: ctx.set_divergence(bad), _native.ERR_ARG)
            assert ctx.get_divergence() == 1.0
        for good in (0.0, 1.0 + 2.0 ** -20, 1.0):
            ctx.set_divergence(good)
            assert ctx.get_divergence() == good
            ctx.set_H(H.astype(np.float32))
            ctx.set_W(W.astype(np.float32))
            assert np.isfinite(ctx.beta_loss())
    with open_problem(monkeypatch, 'f64', V, k, 2) as ctx:
        ctx.set_divergence(1.0 + 2.0 ** -30)
        ctx.set_H(H)
        ctx.set_W(W)
        assert np.isfinite(ctx.beta_loss())


def test_update_scales_w_as_kldivnmf_does_and_refuses_another_eps():
    from multimodal_amd.lib import BetaNMF
    from multimodal_amd.lib.array_utils import normalize_sum
    n, f, k = 65, 65, 65
    V, _, W, H = problem(n, f, k, False)
    m = BetaNMF(beta=2.0, n_components=k, precision='f64')
    m.components_ = H
    with pytest.raises(ValueError):
        m._update(V, W, eps=1e-6)
    scaled = normalize_sum(W, axis=1) * V.sum(axis=1)[:, None]
    got = m._update(V, W, _fit=False, scale_W=True)
    assert np.array_equal(got, m._update(V, scaled, _fit=False)) and not np.array_equal(got, m._update(V, W, _fit=False))


# ---- the learner ----------------------------------------------------------------------------------------------------------------------
def test_learner_with_beta_2_and_a_presence_column():
    """train / reconstruct_internal_multi of MultimodalLearner(beta=2) with an (n, 1) presence column on the second of two
    modalities: BetaNMF called by hand on the stacked matrix with the stacked weights."""
    from multimodal_amd.lib import BetaNMF
    n, dims, k, coefs = 200, [40, 30], 5, [1.0, 0.5]
    rng = np.random.default_rng(21)
    A, B = rng.gamma(1.0, 1.0, (n, dims[0])) + 0.05, rng.gamma(1.0, 1.0, (n, dims[1])) + 0.05
    present = (rng.random((n, 1)) > 0.3).astype(np.float64)
    B = B * present
    stacked = np.hstack([coefs[0] * A, coefs[1] * B])
    weights = np.hstack([np.ones((n, dims[0])), np.broadcast_to(present, (n, dims[1]))])
    learner = MultimodalLearner(['a', 'b'], dims, coefs, k, beta=2.0)
    np.random.seed(3)
    learner.train([A, B], ITERS, weights=[None, present])
    assert isinstance(learner.nmf_train, BetaNMF) and learner.nmf_train.last_weights_route == 'array'
    np.random.seed(3)
    m = BetaNMF(beta=2.0, n_components=k, max_iter=ITERS, tol=0)
    W = m.fit_transform(stacked, weights=weights)
    bars = BARS['f64']
    check('learner train beta=2', 'dico', learner.dico, m.components_, bars['fit_factor'])
    np.random.seed(3)
    kl = MultimodalLearner(['a', 'b'], dims, coefs, k)
    kl.train([A, B], ITERS, weights=[None, present])
    assert np.max(np.abs(kl.dico - learner.dico)) > 1e-3 * np.max(kl.dico)          # another cost, another dictionary
    got = learner.reconstruct_internal_multi(['a', 'b'], [A, B], ITERS, weights=[None, present])
    m2 = BetaNMF(beta=2.0, n_components=k, max_iter=ITERS, tol=0)
    m2.components_ = learner.dico
    check('learner reconstruct beta=2', 'internal', got, m2.transform(stacked, weights=weights), bars['fit_factor'])
    assert W.shape == got.shape == (n, k)
