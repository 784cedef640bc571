"""The weighted KL-NMF kernels (multimodal_amd/csrc/weighted.hip.h) against the fp64 restatement (tests/weighted_cases.py) on
every route of the dense exact dispatch, in f64 and f32, and `weights=` through the public API.

  * general weights (uniform with 30 % exact zeros, an all-zero row, an all-zero column) at every shape of SHAPES: one step
    (the loss pass alone, step_Q -- which leaves R = Om o Q --, step_W, step_H), a 10-iteration fit and a 10-iteration
    transform of `run`; each test asserts `exact_regime()` against the host rule, so the route it names is the route that ran
    (tests/test_weighted_cpu.py: at 256 CUs the shapes reach every route);
  * 1, 3, 7 row chunks, 1, 3 W chunks and H segments of 100 and 128 columns forced on 1000 x 300, k = 40, against the
    restatement and, in f64, against the natural route;
  * weights of all ones against the unweighted kernels; weight 0 on a quarter of the rows against the unweighted device fit
    of the matrix without them; `run` against the loop in pieces and two runs of one fit, bit for bit; a weighted fit, then
    an unweighted one in the same pooled context against a fresh context, bit for bit;
  * the refusals (a CSR problem, an f16 context, a group, weights uploaded into an open loop over row shards), each leaving
    the context usable;
  * KLdivNMF.fit_transform / transform / error / _updated_W / _updated_H with array weights, MultimodalLearner.train and
    reconstruct_internal_multi with a presence column, and the imputation case of the issue.

Bars: test_exact_gpu.BARS with its floors (f64: steps 1e-12, fit losses 1e-10, fit W and H 1e-9, floor 0; f32, the
restatement fed the fp32-rounded V, W, H and weights: steps 3e-5, fit losses 3e-5, fit W and H 3e-4, relative to
max(|reference|, the smallest normal fp32 number); fp32 losses relative to at least 2^-23 sum(Om o V)).  The step's reference
loss is asserted to be at least 1e-2 sum(Om o V), so that its cancellation does not set the bar.
Measured on the MI355X (worst over every case): MEASURED below, read off the run recorded in profiles/weighted_gpu_tests.txt;
no bar was widened.  The measured worst errors are printed after each test (pytest -v) and are in each assertion message.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from multimodal_amd import _native
from multimodal_amd.lib import nmf
from multimodal_amd.learner import MultimodalLearner
from oracle import klnmf_oracle as orc
from tests import exact_cases as ec
from tests import weighted_cases as wc
from tests.test_exact_gpu import BARS, FLOOR, FORCED_VS_NATURAL, ITERS, cu_count, esize, gpu_init_W, open_problem
from tests.test_exact_gpu import problem as exact_problem
from tests.test_sparse_gpu import _MEASURED, _report_measured, check  # noqa: F401  (the autouse fixture prints what was measured)

pytestmark = pytest.mark.gpu

MEASURED = """f64: steps 4.8e-15, fit losses 6.7e-16, fit W 9.0e-15, fit H 1.7e-14, forced against natural 1.5e-14; f32: steps
2.1e-6, fit losses 8.7e-8, fit W 9.4e-6, fit H 7.6e-6; ones against the unweighted kernels 5.7e-15 (f64) and 1.9e-6 (f32); deleted
rows 2.8e-15 (f64) and 1.9e-6 (f32); run against pieces, two runs and pooled reuse 0; public API in f64 4.2e-15, in 'f16'
(run in f32) 1.5e-6; learner against the stacked fit 0; imputation 0.0058 weighted against 0.5143 zero-filled."""

EXACT = ['f64', 'f32']
SHAPES = [(1, 1, 1), (15, 17, 1), (65, 65, 65), (300, 700, 65), (300, 700, 200), (4111, 63, 200), (4096, 128, 16),
          (4096, 129, 16), (100, 16385, 33)]
FORCED = [('row_chunks', 1), ('row_chunks', 3), ('row_chunks', 7), ('w_chunks', 1), ('w_chunks', 3), ('h_seg', 100), ('h_seg', 128)]


@functools.lru_cache(maxsize=4)
def problem(n, f, k):
    """(V, Om, W, H) in fp64: test_exact_gpu's problem (a zero row and a zero column of V) with general weights."""
    V, W, H = exact_problem(n, f, k)
    return V, wc.general(n, f, seed=3 * n + 5 * f + k), W, H


def inputs(prec, *arrays):
    """The restatement's inputs (what the kernels of `prec` see, in fp64) and the arrays to upload."""
    if prec == 'f64':
        return arrays, arrays
    return tuple(ec.as_f32(a) for a in arrays), tuple(np.asarray(a, np.float32) for a in arrays)


@functools.lru_cache(maxsize=8)
def reference(n, f, k, f32_inputs, kchunk, wchunk):
    """(step, fit, transform) of the restatement on the case's inputs, summed over the kernels' chunks."""
    V, Om, W, H = problem(n, f, k)
    if f32_inputs:
        V, Om, W, H = (ec.as_f32(a) for a in (V, Om, W, H))
    step = wc.ref_step_w(V, Om, W, H, kchunk, wchunk)
    assert step[0] >= 1e-2 * (Om * V).sum()          # the loss's own cancellation does not dominate the step bars
    fit = wc.ref_fit_w(V, Om, H, ITERS, kchunk=kchunk, wchunk=wchunk)
    transform = wc.ref_fit_w(V, Om, H, ITERS, fit=False, components=H, kchunk=kchunk, wchunk=wchunk)
    return step, fit, transform


def open_weighted(monkeypatch, prec, Vu, Omu, k, cap, **forced):
    ctx = open_problem(monkeypatch, prec, Vu, k, cap, **forced)
    assert not ctx.weighted()
    ctx.upload_weights(Omu)
    assert ctx.weighted()
    return ctx


def gpu_step(ctx, W, H):
    """(loss, R, W_new, H_new) of one update on the device: klnmf_error (the loss pass alone), then klnmf_step_Q / _W / _H."""
    ctx.set_H(H)
    ctx.set_W(W)
    loss = ctx.error()
    ctx.step_Q()
    R = ctx.get_Q()
    ctx.step_W()
    Wn = ctx.get_W()
    ctx.step_H()
    return loss, R, Wn, ctx.get_H()


def gpu_fit(ctx, H0, iters=ITERS, fit=True):
    gpu_init_W(ctx, H0)
    errors, n_done, _ = ctx.run(iters, fit, ec.NO_STOP)
    assert n_done == len(errors) == iters
    return ctx.get_W(), ctx.get_H(), np.array(errors)


def gpu_pieces(ctx, H0, iters=ITERS):
    gpu_init_W(ctx, H0)
    ctx.loop_begin()
    for _ in range(iters):
        ctx.iter_rowpass(True)
        ctx.iter_decide(ec.NO_STOP)
        ctx.iter_colpass()
        ctx.iter_update_H()
        ctx.iter_advance()
    errors, n_done, _ = ctx.loop_end(iters)
    assert n_done == len(errors) == iters
    return ctx.get_W(), ctx.get_H(), np.array(errors)


def loss_floor(prec, V, Om):
    return 0.0 if prec == 'f64' else 2.0 ** -23 * float((Om * V).sum())


def check_step(case, prec, got, ref, V, Om):
    bar = BARS[prec]['step']
    check(case, 'loss', got[0], ref[0], bar, loss_floor(prec, V, Om))
    for what, a, b in zip(('R', 'W rule', 'H rule'), got[1:], ref[1:]):
        check(case, what, a, b, bar, FLOOR[prec])


def check_fit(case, prec, got, ref, V, Om, bars=None):
    bars = bars or BARS[prec]
    assert len(got[2]) == len(ref[2])
    check(case, 'losses', got[2], ref[2], bars['fit_loss'], loss_floor(prec, V, Om))
    check(case, 'W', got[0], ref[0], bars['fit_factor'], FLOOR[prec])
    check(case, 'H', got[1], ref[1], bars['fit_factor'], FLOOR[prec])


def run_case(monkeypatch, prec, n, f, k, **forced):
    """One step, a fit and a transform on the (forced) route against the restatement; returns what the device gave."""
    V, Om, W, H = problem(n, f, k)
    (Vr, Omr, Wr, Hr), (Vu, Omu, Wu, Hu) = inputs(prec, V, Om, W, H)
    s, kchunk, w, wchunk, h, slabs = ec.exact_regime(n, f, k, cu_count(), esize(prec), **forced)
    step, fit, transform = reference(n, f, k, prec != 'f64', kchunk, wchunk)
    case = '%s %s %s(%d, %d, %d, %d)' % (prec, ec.case_id((n, f, k)), ''.join('%s=%d ' % kv for kv in forced.items()), s, w, h, slabs)
    with open_weighted(monkeypatch, prec, Vu, Omu, k, ITERS, **forced) as ctx:
        assert ctx.exact_regime() == (s, w, h, int(slabs))
        got_step = gpu_step(ctx, Wu, Hu)
        check_step(case + ' step', prec, got_step, step, Vr, Omr)
        got_fit = gpu_fit(ctx, Hu)
        check_fit(case + ' fit', prec, got_fit, fit, Vr, Omr)
        check_fit(case + ' transform', prec, gpu_fit(ctx, Hu, fit=False), transform, Vr, Omr)
    return got_step, got_fit


@pytest.mark.parametrize('prec', EXACT)
@pytest.mark.parametrize('shape', SHAPES, ids=ec.case_id)
def test_every_route(monkeypatch, prec, shape):
    run_case(monkeypatch, prec, *shape)


@pytest.mark.parametrize('prec', EXACT)
@pytest.mark.parametrize('forced', FORCED, ids=lambda v: '%s=%d' % v)
def test_forced_routes(monkeypatch, prec, forced):
    n, f, k = ec.MID
    got_step, got_fit = run_case(monkeypatch, prec, n, f, k, **dict([forced]))
    if prec != 'f64':
        return
    V, Om, W, H = problem(n, f, k)
    with open_weighted(monkeypatch, prec, V, Om, k, ITERS) as nat:
        assert nat.exact_regime() == ec.query_regime(n, f, k, cu_count())
        nat_step = gpu_step(nat, W, H)
        nat_fit = gpu_fit(nat, H)
    case = 'f64 %s %s=%d vs natural' % ((ec.case_id(ec.MID),) + forced)
    for what, a, b in zip(('loss', 'R', 'W rule', 'H rule'), got_step, nat_step):
        check(case, what, a, b, FORCED_VS_NATURAL['step'])
    for what, a, b in zip(('W', 'H', 'losses'), got_fit, nat_fit):
        check(case + ' fit', what, a, b, FORCED_VS_NATURAL['fit'])


@pytest.mark.parametrize('prec', EXACT)
@pytest.mark.parametrize('shape', [ec.MID, (300, 700, 65)], ids=ec.case_id)
def test_weights_of_one_give_the_unweighted_kernels_results(monkeypatch, prec, shape):
    n, f, k = shape
    V, _, W, H = problem(n, f, k)
    (Vr, _, _, _), (Vu, _, Wu, Hu) = inputs(prec, V, V, W, H)
    ones = np.ones((n, f), dtype=Vu.dtype)
    with open_problem(monkeypatch, prec, Vu, k, ITERS) as ctx:
        plain = [gpu_fit(ctx, Hu), gpu_fit(ctx, Hu, fit=False)]
    with open_weighted(monkeypatch, prec, Vu, ones, k, ITERS) as ctx:
        weighted = [gpu_fit(ctx, Hu), gpu_fit(ctx, Hu, fit=False)]
    for what, got, ref in zip(('fit', 'transform'), weighted, plain):
        check_fit('%s %s ones %s' % (prec, ec.case_id(shape), what), prec, got, ref, Vr, ones)


@pytest.mark.parametrize('prec', EXACT)
def test_zero_weight_rows_are_deleted_rows(monkeypatch, prec):
    n, f, k = ec.MID
    V, _, W, H = problem(n, f, k)
    Om, keep = wc.row_mask(n, f, seed=5)
    (Vr, Omr, _, _), (Vu, Omu, _, Hu) = inputs(prec, V, Om, W, H)
    with open_problem(monkeypatch, prec, np.ascontiguousarray(Vu[keep]), k, ITERS) as ctx:
        Wd, Hd, ed = gpu_fit(ctx, Hu)
    with open_weighted(monkeypatch, prec, Vu, Omu, k, ITERS) as ctx:
        W0 = gpu_init_W(ctx, Hu)
        Ww, Hw, ew = gpu_fit(ctx, Hu)
    check_fit('%s %s deleted rows' % (prec, ec.case_id(ec.MID)), prec, (Ww[keep], Hw, ew), (Wd, Hd, ed), Vr, Omr)
    assert np.array_equal(Ww[~keep], W0[~keep])          # a sample with no observed entry keeps its coefficients


@pytest.mark.parametrize('prec', EXACT)
@pytest.mark.parametrize('shape', [(4096, 128, 16), ec.MID, (100, 16385, 33)], ids=ec.case_id)
def test_run_and_the_loop_in_pieces_give_the_same_bits(monkeypatch, prec, shape):
    """(4096 x 128 and 1000 x 300: `run` applies the H rule from the two slab sets, the pieces from their sums.)"""
    n, f, k = shape
    V, Om, W, H = problem(n, f, k)
    _, (Vu, Omu, _, Hu) = inputs(prec, V, Om, W, H)
    with open_weighted(monkeypatch, prec, Vu, Omu, k, ITERS) as ctx:
        run = gpu_fit(ctx, Hu)
        pieces = gpu_pieces(ctx, Hu)
        ctx.set_H(Hu)
        gpu_init_W(ctx, Hu)
        for _ in range(ITERS):
            ctx.update(True)
        updates = ctx.get_W(), ctx.get_H()
    for a, b in zip(run, pieces):
        assert np.array_equal(a, b)
    for a, b in zip(run, updates):
        assert np.array_equal(a, b)


@pytest.mark.parametrize('prec', EXACT)
def test_two_runs_of_one_weighted_fit_give_the_same_bits(monkeypatch, prec):
    n, f, k = ec.MID
    V, Om, W, H = problem(n, f, k)
    _, (Vu, Omu, _, Hu) = inputs(prec, V, Om, W, H)
    got = []
    for _ in range(2):
        with open_weighted(monkeypatch, prec, Vu, Omu, k, ITERS) as ctx:
            got.append(gpu_fit(ctx, Hu))
    for a, b in zip(*got):
        assert np.array_equal(a, b)


@pytest.mark.parametrize('prec', EXACT)
def test_a_pooled_context_forgets_the_weights(monkeypatch, prec):
    """A weighted fit, then an unweighted fit of the same shape in the same pooled context: exactly a fresh context's result.
    klnmf_set_problem and klnmf_release_problem drop the weights; klnmf_clear_weights does on a live problem."""
    monkeypatch.delenv('KLNMF_NO_POOL', raising=False)
    n, f, k = ec.MID
    V, Om, W, H = problem(n, f, k)
    _, (Vu, Omu, _, Hu) = inputs(prec, V, Om, W, H)
    with open_problem(monkeypatch, prec, Vu, k, ITERS) as fresh:
        want = gpu_fit(fresh, Hu)
    ctx = _native.Context(prec, pooled=True)
    handle = ctx._h.value
    ctx.set_problem(n, f, k, ITERS)
    ctx.upload_V(Vu)
    ctx.upload_weights(Omu)
    weighted = gpu_fit(ctx, Hu)
    assert not np.array_equal(weighted[1], want[1])
    ctx.set_problem(n, f, k, ITERS)                       # the same context, a new problem
    assert not ctx.weighted()
    ctx.upload_V(Vu)
    again = gpu_fit(ctx, Hu)
    ctx.upload_weights(Omu)
    assert ctx.weighted()
    ctx.clear_weights()
    assert not ctx.weighted()
    cleared = gpu_fit(ctx, Hu)
    ctx.upload_weights(Omu[:, :7], col0=5)                # left weighted when it goes back to the pool
    ctx.close()
    with _native.Context(prec, pooled=True) as ctx2:      # the pool hands the same native context out
        assert ctx2._h.value == handle
        ctx2.set_problem(n, f, k, ITERS)
        assert not ctx2.weighted()
        ctx2.upload_V(Vu)
        pooled = gpu_fit(ctx2, Hu)
    for got in (again, cleared, pooled):
        for a, b in zip(got, want):
            assert np.array_equal(a, b)


def test_blocks_of_weights_land_where_they_are_put(monkeypatch):
    """The first upload fills the buffer with 1; blocks (float32 or float64, strided) replace their part of it."""
    n, f, k = 70, 90, 3
    V, Om, W, H = problem(n, f, k)
    want = np.ones((n, f))
    want[10:40, 64:90] = Om[10:40, 64:90]
    want[:, 3:4] = Om[:, 3:4]
    with open_problem(monkeypatch, 'f64', V, k, 1) as ctx:
        ctx.upload_weights(Om[10:40, 64:90], row0=10, col0=64)          # a strided view
        ctx.upload_weights(Om[:, 3:4].astype(np.float32), col0=3)
        want[:, 3:4] = ec.as_f32(Om[:, 3:4])
        got = gpu_step(ctx, W, H)
        with pytest.raises(_native.NativeError) as e:
            ctx.upload_weights(Om[:, :5], col0=f - 4)
        assert e.value.code == _native.ERR_ARG
    ref = wc.ref_step_w(V, want, W, H, *ec.exact_regime(n, f, k, cu_count())[1:4:2])
    check_step('f64 70x90k3 blocks', 'f64', got, ref, V, want)


def test_refusals_leave_the_context_usable(monkeypatch):
    n, f, k = 64, 256, 16
    V, Om, W, H = problem(n, f, k)
    # a CSR problem
    X = sp.csr_matrix(V * (Om > 0.5))
    with _native.Context('f64') as ctx:
        ctx.set_problem_sparse(X, k, 2)
        ctx.set_H(H)
        ctx.set_W(W)
        before = ctx.error()
        with pytest.raises(_native.NativeError) as e:
            ctx.upload_weights(Om)
        assert e.value.code == _native.ERR_UNSUPP and 'CSR' in str(e.value)
        assert not ctx.weighted() and ctx.error() == before
    # every precision but f64 and f32
    for prec in ('f16', 'bf16x3', 'f16x3'):
        with _native.Context(prec) as ctx:
            ctx.set_problem(n, f, k, 2)
            ctx.upload_blocks([V])
            with pytest.raises(_native.NativeError) as e:
                ctx.upload_weights(Om)
            assert e.value.code == _native.ERR_UNSUPP and 'KLNMF_PREC_F64' in str(e.value)
            assert not ctx.weighted()
            ctx.set_H(H)
            ctx.init_W()
            errors, n_done, _ = ctx.run(2, True, ec.NO_STOP)
            assert n_done == 2 and np.all(np.isfinite(errors))
    # a group: at its creation, and at its run if the weights came later
    with open_weighted(monkeypatch, 'f64', V, Om, k, 2) as ctx:
        want = gpu_fit(ctx, H, 2)
        with pytest.raises(_native.NativeError) as e:
            _native.Group([ctx])
        assert e.value.code == _native.ERR_UNSUPP and 'denominator' in str(e.value)
        ctx.clear_weights()
        gpu_init_W(ctx, H)
        with _native.Group([ctx]) as group:
            ctx.upload_weights(Om)
            with pytest.raises(_native.NativeError) as e:
                group.run(n, 2, True, 0.0)
            assert e.value.code == _native.ERR_UNSUPP
        with pytest.raises(_native.NativeError) as e:
            ctx.loop_begin(1.0, 1.0)                       # the loop sequenced by the caller over row shards
        assert e.value.code == _native.ERR_UNSUPP
        # ... and weights that arrive while such a loop is open: its pieces would run the weighted kernels under an exchange
        # of the numerator alone
        ctx.clear_weights()
        gpu_init_W(ctx, H)
        ctx.loop_begin(float(V.sum()), float(n * f))
        with pytest.raises(_native.NativeError) as e:
            ctx.upload_weights(Om)
        assert e.value.code == _native.ERR_UNSUPP and 'row shards' in str(e.value)
        assert not ctx.weighted()
        ctx.iter_rowpass(True)
        ctx.iter_decide(ec.NO_STOP)
        ctx.iter_colpass()
        ctx.iter_update_H()
        ctx.iter_advance()
        assert ctx.loop_end(2)[1] == 1
        ctx.upload_weights(Om)                             # the loop has ended
        for a, b in zip(gpu_fit(ctx, H, 2), want):
            assert np.array_equal(a, b)


# ---- through the public API -------------------------------------------------------------------------------------------------------
def model(k, H0, iters=ITERS, **kw):
    m = nmf.KLdivNMF(n_components=k, max_iter=iters, tol=ec.NO_STOP, **kw)
    m._init_dictionary = H0
    return m


@pytest.mark.parametrize('wshape', ['(f,)', '(n, 1)', '(n, f)'])
def test_fit_transform_with_weights(wshape):
    n, f, k = 300, 700, 17
    V, Om, _, H0 = problem(n, f, k)
    w = {'(f,)': Om[7], '(n, 1)': Om[:, 11:12], '(n, f)': Om}[wshape]
    full = np.broadcast_to(w, (n, f))
    _, kchunk, _, wchunk, _, _ = ec.exact_regime(n, f, k, cu_count())
    m = model(k, H0, precision='f64')
    W, errors = m.fit_transform(V, weights=w, return_errors=True)
    assert m.last_fp8_report is not None and m.last_fp8_report['allowed'] is False
    ref = wc.ref_fit_w(V, full, H0, ITERS, kchunk=kchunk, wchunk=wchunk)
    check_fit('f64 fit_transform weights %s' % wshape, 'f64', (W, m.components_, np.array(errors)), ref, V, full)
    Wt, errors = m.transform(V, weights=w, return_errors=True)
    ref = wc.ref_fit_w(V, full, m.components_, ITERS, fit=False, components=m.components_, kchunk=kchunk, wchunk=wchunk)
    check_fit('f64 transform weights %s' % wshape, 'f64', (Wt, m.components_, np.array(errors)), ref, V, full)
    # and they were not ignored
    W1 = model(k, H0, precision='f64').fit_transform(V)
    assert np.max(np.abs(W1 - W)) > 1e-3 * np.max(W1)


def test_the_16_bit_mode_runs_weights_in_f32_and_says_so_once(capsys):
    n, f, k = 300, 700, 17
    V, Om, _, H0 = problem(n, f, k)
    Vr, Omr, Hr = (ec.as_f32(a) for a in (V, Om, H0))
    nmf._NOTED.clear()
    capsys.readouterr()
    _, kchunk, _, wchunk, _, _ = ec.exact_regime(n, f, k, cu_count(), 4)
    ref = wc.ref_fit_w(Vr, Omr, Hr, ITERS, kchunk=kchunk, wchunk=wchunk)
    for _ in range(2):
        m = model(k, H0.astype(np.float32), precision='f16')
        W, errors = m.fit_transform(V.astype(np.float32), weights=Om.astype(np.float32), return_errors=True)
        check_fit('f16 -> f32 fit_transform', 'f32', (W, m.components_, np.array(errors)), ref, Vr, Omr)
    err = capsys.readouterr().err
    assert err.count("weights with precision='f16' run on the fp32 weighted kernels") == 1 and err.count('\n') == 1, err


def test_error_and_single_steps_with_weights():
    n, f, k = 65, 65, 65
    V, Om, W, H = problem(n, f, k)
    loss, R, Wn, _ = wc.ref_step_w(V, Om, W, H)
    m = nmf.KLdivNMF(n_components=k, precision='f64')
    check('f64 error(weights)', 'loss', m.error(V, W, H=H, weights=Om), loss, BARS['f64']['step'])
    check('f64 error(weights (f,))', 'loss', m.error(V, W, H=H, weights=Om[3]), wc.ref_step_w(V, np.broadcast_to(Om[3], V.shape), W, H)[0],
          BARS['f64']['step'])
    assert m.error(V, W, H=H, weights=2.0) == m.error(V, W, H=H)          # a scalar is ignored as before
    check('f64 _updated_W(weights)', 'W', nmf.KLdivNMF._updated_W(V, W, H, weights=Om), Wn, BARS['f64']['step'])
    Hn = orc.normalize_sum(H * wc.factor(W.T.dot(R), W.T.dot(Om)), axis=1)
    check('f64 _updated_H(weights)', 'H', nmf.KLdivNMF._updated_H(V, W, H, weights=Om), Hn, BARS['f64']['step'])
    Q = (V + orc.EPS_RATIO) / (W.dot(H) + orc.EPS_RATIO)
    check('f64 _updated_W(weights, Q)', 'W', nmf.KLdivNMF._updated_W(V, W, H, weights=Om, Q=Q), Wn, BARS['f64']['step'])


def test_learner_with_a_presence_column():
    """train / reconstruct_internal_multi with an (n, 1) presence column on the second of two modalities: fit_transform /
    transform of the stacked matrix with the stacked weights."""
    n, dims, k, coefs = 60, [40, 30], 5, [1.0, 0.5]
    rng = np.random.default_rng(21)
    A, B = rng.gamma(1.0, 1.0, (n, dims[0])) + 0.05, rng.gamma(1.0, 1.0, (n, dims[1])) + 0.05
    present = (rng.random((n, 1)) > 0.3).astype(np.float64)
    B = B * present                                       # a missing modality is stored as zeros
    stacked = np.hstack([coefs[0] * A, coefs[1] * B])
    weights = np.hstack([np.ones((n, dims[0])), np.broadcast_to(present, (n, dims[1]))])
    learner = MultimodalLearner(['a', 'b'], dims, coefs, k)
    np.random.seed(3)
    learner.train([A, B], ITERS, weights=[None, present])
    np.random.seed(3)
    m = nmf.KLdivNMF(n_components=k, max_iter=ITERS, tol=0)
    W = m.fit_transform(stacked, weights=weights)
    bars = BARS['f64']
    check('learner train', 'dico', learner.dico, m.components_, bars['fit_factor'])
    np.random.seed(3)
    plain = MultimodalLearner(['a', 'b'], dims, coefs, k)
    plain.train([A, B], ITERS)
    assert np.max(np.abs(plain.dico - learner.dico)) > 1e-3 * np.max(plain.dico)          # the weights were honoured
    got = learner.reconstruct_internal_multi(['a', 'b'], [A, B], ITERS, weights=[None, present])
    m2 = nmf.KLdivNMF(n_components=k, max_iter=ITERS, tol=0)
    m2.components_ = learner.dico
    check('learner reconstruct', 'internal', got, m2.transform(stacked, weights=weights), bars['fit_factor'])
    assert W.shape == got.shape == (n, k)


def test_imputation():
    """Exactly rank-4 data, 120 x 90, 40 % of the entries hidden, 100 iterations in f64: the weighted fit reconstructs the hidden
    entries (relative L1 error below 0.05; the restatement gives 0.006), the unweighted fit of the zero-filled matrix does
    not (0.51): at least 10 x apart."""
    V, M, H0 = wc.imputation_case()
    m = model(4, H0, iters=100, precision='f64')
    W = m.fit_transform(V * M, weights=M)
    weighted = wc.hidden_error(V, M, W, m.components_)
    m = model(4, H0, iters=100, precision='f64')
    W = m.fit_transform(V * M)
    zero_filled = wc.hidden_error(V, M, W, m.components_)
    _MEASURED.append('    hidden-entry relative L1 error: weighted %.4f, zero-filled %.4f' % (weighted, zero_filled))
    assert weighted < 0.05, weighted
    assert 10 * weighted <= zero_filled, (weighted, zero_filled)
