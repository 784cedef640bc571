"""The masked KL-NMF kernels (multimodal_amd/csrc/presence.hip.h: weights Om[i, j] = P[i, m(j)] without the n x f buffer) against
the fp64 weighted restatement on the broadcast mask (tests/weighted_cases.ref_step_w / ref_fit_w on presence_cases.omega), on
every route of the dense exact dispatch, in f64 and f32, and (n, 1) `weights=` through the public API.

Shapes -- the smallest at which each route and edge exists:
  (1, 1, 1)                        the degenerate problem
  (15, 17, 1)                      M = 16, modalities of width 1
  (65, 65, 65)                     one ragged tile each way; bounds [0, 1, 64, 65]: three modalities in one 64-column tile and one
                                   modality in a tile of its own
  (300, 700, 65), (300, 700, 200)  bounds off tile edges
  (4111, 63, 200)                  row chunks
  (4096, 129, 16)                  a modality that ends one column into a tile
  (100, 16385, 33)                 the segmented H rule (a modality that ends one column into a segment, a last one of one column)
Masks (presence_cases.mask): values in [0, 1] with exact zeros and ones, an all-zero row, for M >= 3 a modality absent from every
row.

  * every shape x {f64, f32} x M in {1, 3} (or the M the shape names): one step (the loss pass alone, step_Q -- which leaves
    R = Om o Q --, step_W, step_H), a 10-iteration fit and a 10-iteration transform of `run`; `exact_regime()` asserted against the
    host rule;
  * the forced routes of test_weighted_gpu.FORCED on 300 x 700, k = 65, against the reference and, in f64, the natural route;
  * the same mask through upload_presence and through upload_weights (broadcast), on the device;
  * P of all ones against the unweighted kernels; P = 0 on a quarter of the rows against the unweighted device fit of the matrix
    without them; `run` against the loop in pieces and against klnmf_update, two runs of one fit, an unweighted fit in a pooled
    context behind a masked one against a fresh context: bit for bit;
  * P uploaded in row pieces and as a strided view; other bounds on a second upload; every refusal, each leaving the context
    usable;
  * MultimodalLearner.train / reconstruct_internal_multi with a presence column, KLdivNMF.last_weights_route, precision='f16'.

Bars: test_exact_gpu.BARS with its floors, unchanged (f64: steps 1e-12, fit losses 1e-10, fit W and H 1e-9, floor 0; f32, the
reference fed the fp32-rounded V, W, H and P: steps 3e-5, fit losses 3e-5, fit W and H 3e-4, relative to max(|reference|, the
smallest normal fp32 number); fp32 losses relative to at least 2^-23 sum(Om o V)): the factored form agrees with the reference
to 3.7e-15 on a step and 1.7e-14 on a fit in fp64 (tests/test_presence_cpu.py), elementwise, exact zeros reproduced.
Measured on the MI355X (worst over every case): MEASURED below, read off the run recorded in profiles/presence_gpu_tests.txt.
The measured worst errors are printed after each test (pytest -v) and are in each assertion message.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from multimodal_amd import _native
from multimodal_amd.lib import nmf
from multimodal_amd.learner import MultimodalLearner
from tests import exact_cases as ec
from tests import presence_cases as pc
from tests import weighted_cases as wc
from tests.test_exact_gpu import BARS, FLOOR, FORCED_VS_NATURAL, ITERS, cu_count, esize, gpu_init_W, open_problem
from tests.test_exact_gpu import problem as exact_problem
from tests.test_sparse_gpu import _MEASURED, _report_measured, check  # noqa: F401  (the autouse fixture prints what was measured)
from tests.test_weighted_gpu import FORCED, check_fit, check_step, gpu_fit, gpu_pieces, gpu_step, inputs

pytestmark = pytest.mark.gpu

MEASURED = """f64: steps 2.7e-15, fit losses 1.9e-15, fit W 1.8e-14, fit H 6.3e-15, forced against natural 1.0e-14; f32: steps
1.5e-6, fit losses 7.5e-7, fit W 4.8e-6, fit H 4.4e-6; the mask against the broadcast weights on the device 6.6e-15 (f64) and
3.2e-6 (f32); ones against the unweighted kernels 4.1e-15 (f64) and 1.5e-6 (f32); deleted rows 2.6e-15 (f64) and 1.9e-6 (f32); run
against pieces and single updates, two runs, row pieces against one upload and pooled reuse 0; learner against the stacked
weight-buffer fit 3.3e-15; fit_transform with (n, 1) weights in f64 2.2e-15, in 'f16' (run in f32) 1.2e-6."""

EXACT = ['f64', 'f32']
SHAPES = [(1, 1, 1), (15, 17, 1), (65, 65, 65), (300, 700, 65), (300, 700, 200), (4111, 63, 200), (4096, 129, 16), (100, 16385, 33)]
NAMED_M = {(1, 1, 1): (1,), (15, 17, 1): (16,)}
CASES = [(shape, M) for shape in SHAPES for M in NAMED_M.get(shape, (1, 3))]
FORCED_SHAPE = (300, 700, 65)


def case_id(case):
    return '%s-M%d' % (ec.case_id(case[0]), case[1])


@functools.lru_cache(maxsize=4)
def problem(n, f, k, M):
    """(V, P, bounds, W, H) in fp64: test_exact_gpu's problem (a zero row and a zero column of V) with a mask of M modalities."""
    V, W, H = exact_problem(n, f, k)
    return V, pc.mask(n, M, seed=3 * n + 5 * f + k + M), tuple(pc.bounds(f, M)), W, H


@functools.lru_cache(maxsize=8)
def reference(n, f, k, M, f32_inputs, kchunk, wchunk):
    """(step, fit, transform) of the weighted restatement on the broadcast mask, summed over the kernels' chunks."""
    V, P, b, W, H = problem(n, f, k, M)
    if f32_inputs:
        V, P, W, H = (ec.as_f32(a) for a in (V, P, W, H))
    Om = pc.omega(P, b)
    step = wc.ref_step_w(V, Om, W, H, kchunk, wchunk)
    assert step[0] >= 1e-2 * (Om * V).sum()          # the loss's own cancellation does not dominate the step bars
    fit = wc.ref_fit_w(V, Om, H, ITERS, kchunk=kchunk, wchunk=wchunk)
    transform = wc.ref_fit_w(V, Om, H, ITERS, fit=False, components=H, kchunk=kchunk, wchunk=wchunk)
    return step, fit, transform


def open_masked(monkeypatch, prec, Vu, Pu, bounds, k, cap, **forced):
    ctx = open_problem(monkeypatch, prec, Vu, k, cap, **forced)
    assert ctx.presence() == 0 and not ctx.weighted()
    ctx.upload_presence(Pu, bounds)
    assert ctx.presence() == len(bounds) - 1 and not ctx.weighted()
    return ctx


def run_case(monkeypatch, prec, shape, M, **forced):
    """One step, a fit and a transform on the (forced) route against the reference; returns what the device gave."""
    n, f, k = shape
    V, P, b, W, H = problem(n, f, k, M)
    (Vr, Pr, _, _), (Vu, Pu, Wu, Hu) = inputs(prec, V, P, W, H)
    Omr = pc.omega(Pr, b)
    s, kchunk, w, wchunk, h, slabs = ec.exact_regime(n, f, k, cu_count(), esize(prec), **forced)
    step, fit, transform = reference(n, f, k, M, prec != 'f64', kchunk, wchunk)
    case = '%s %s %s(%d, %d, %d, %d)' % (prec, case_id((shape, M)), ''.join('%s=%d ' % kv for kv in forced.items()), s, w, h, slabs)
    with open_masked(monkeypatch, prec, Vu, Pu, b, k, ITERS, **forced) as ctx:
        assert ctx.exact_regime() == (s, w, h, int(slabs))
        got_step = gpu_step(ctx, Wu, Hu)
        check_step(case + ' step', prec, got_step, step, Vr, Omr)
        got_fit = gpu_fit(ctx, Hu)
        check_fit(case + ' fit', prec, got_fit, fit, Vr, Omr)
        check_fit(case + ' transform', prec, gpu_fit(ctx, Hu, fit=False), transform, Vr, Omr)
    return got_step, got_fit


@pytest.mark.parametrize('prec', EXACT)
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_every_route(monkeypatch, prec, case):
    run_case(monkeypatch, prec, *case)


@pytest.mark.parametrize('prec', EXACT)
@pytest.mark.parametrize('forced', FORCED, ids=lambda v: '%s=%d' % v)
def test_forced_routes(monkeypatch, prec, forced):
    n, f, k = FORCED_SHAPE
    got_step, got_fit = run_case(monkeypatch, prec, FORCED_SHAPE, 3, **dict([forced]))
    if prec != 'f64':
        return
    V, P, b, W, H = problem(n, f, k, 3)
    with open_masked(monkeypatch, prec, V, P, b, k, ITERS) as nat:
        assert nat.exact_regime() == ec.query_regime(n, f, k, cu_count())
        nat_step = gpu_step(nat, W, H)
        nat_fit = gpu_fit(nat, H)
    case = 'f64 %s %s=%d vs natural' % ((ec.case_id(FORCED_SHAPE),) + forced)
    for what, a, c in zip(('loss', 'R', 'W rule', 'H rule'), got_step, nat_step):
        check(case, what, a, c, FORCED_VS_NATURAL['step'])
    for what, a, c in zip(('W', 'H', 'losses'), got_fit, nat_fit):
        check(case + ' fit', what, a, c, FORCED_VS_NATURAL['fit'])


@pytest.mark.parametrize('prec', EXACT)
@pytest.mark.parametrize('M', [1, 3])
def test_the_mask_and_the_broadcast_weights_agree_on_the_device(monkeypatch, prec, M):
    n, f, k = FORCED_SHAPE
    V, P, b, W, H = problem(n, f, k, M)
    (Vr, Pr, _, _), (Vu, Pu, Wu, Hu) = inputs(prec, V, P, W, H)
    Omr, Omu = pc.omega(Pr, b), pc.omega(Pu, b)
    with open_masked(monkeypatch, prec, Vu, Pu, b, k, ITERS) as ctx:
        masked = gpu_step(ctx, Wu, Hu), gpu_fit(ctx, Hu), gpu_fit(ctx, Hu, fit=False)
    with open_problem(monkeypatch, prec, Vu, k, ITERS) as ctx:
        ctx.upload_weights(Omu)
        assert ctx.weighted() and ctx.presence() == 0
        weighted = gpu_step(ctx, Wu, Hu), gpu_fit(ctx, Hu), gpu_fit(ctx, Hu, fit=False)
    case = '%s %s mask vs weights' % (prec, case_id((FORCED_SHAPE, M)))
    check_step(case + ' step', prec, masked[0], weighted[0], Vr, Omr)
    check_fit(case + ' fit', prec, masked[1], weighted[1], Vr, Omr)
    check_fit(case + ' transform', prec, masked[2], weighted[2], Vr, Omr)


@pytest.mark.parametrize('prec', EXACT)
@pytest.mark.parametrize('shape', [ec.MID, (300, 700, 65)], ids=ec.case_id)
def test_a_mask_of_ones_gives_the_unweighted_kernels_results(monkeypatch, prec, shape):
    n, f, k = shape
    V, _, b, W, H = problem(n, f, k, 3)
    assert np.allclose(H.sum(axis=1), 1.0, rtol=1e-12)          # (the W rule's denominator P.S is the row sums: 1)
    (Vr, _, _), (Vu, _, Hu) = inputs(prec, V, W, H)
    ones = np.ones((n, 3), dtype=Vu.dtype)
    with open_problem(monkeypatch, prec, Vu, k, ITERS) as ctx:
        plain = [gpu_fit(ctx, Hu), gpu_fit(ctx, Hu, fit=False)]
    with open_masked(monkeypatch, prec, Vu, ones, b, k, ITERS) as ctx:
        masked = [gpu_fit(ctx, Hu), gpu_fit(ctx, Hu, fit=False)]
    for what, got, ref in zip(('fit', 'transform'), masked, plain):
        check_fit('%s %s ones %s' % (prec, ec.case_id(shape), what), prec, got, ref, Vr, np.ones((n, f)))


@pytest.mark.parametrize('prec', EXACT)
def test_absent_rows_are_deleted_rows(monkeypatch, prec):
    n, f, k = ec.MID
    V, _, b, W, H = problem(n, f, k, 2)
    Om, keep = wc.row_mask(n, f, seed=5)
    P = np.repeat(keep[:, None].astype(np.float64), 2, axis=1)
    (Vr, _, _), (Vu, _, Hu) = inputs(prec, V, W, H)
    with open_problem(monkeypatch, prec, np.ascontiguousarray(Vu[keep]), k, ITERS) as ctx:
        Wd, Hd, ed = gpu_fit(ctx, Hu)
    with open_masked(monkeypatch, prec, Vu, P.astype(Vu.dtype), b, k, ITERS) as ctx:
        W0 = gpu_init_W(ctx, Hu)
        Wm, Hm, em = gpu_fit(ctx, Hu)
    check_fit('%s %s deleted rows' % (prec, ec.case_id(ec.MID)), prec, (Wm[keep], Hm, em), (Wd, Hd, ed), Vr, Om)
    assert np.array_equal(Wm[~keep], W0[~keep])          # a sample with no modality present keeps its coefficients


@pytest.mark.parametrize('prec', EXACT)
@pytest.mark.parametrize('shape', [(4096, 128, 16), ec.MID, (100, 16385, 33)], ids=ec.case_id)
def test_run_the_loop_in_pieces_and_single_updates_give_the_same_bits(monkeypatch, prec, shape):
    """(4096 x 128 and 1000 x 300: `run` applies the H rule from the slabs, the pieces from their sum.)"""
    n, f, k = shape
    V, P, b, W, H = problem(n, f, k, 3)
    _, (Vu, Pu, _, Hu) = inputs(prec, V, P, W, H)
    with open_masked(monkeypatch, prec, Vu, Pu, b, k, ITERS) as ctx:
        run = gpu_fit(ctx, Hu)
        pieces = gpu_pieces(ctx, Hu)
        gpu_init_W(ctx, Hu)
        for _ in range(ITERS):
            ctx.update(True)
        updates = ctx.get_W(), ctx.get_H()
    for a, c in zip(run, pieces):
        assert np.array_equal(a, c)
    for a, c in zip(run, updates):
        assert np.array_equal(a, c)


@pytest.mark.parametrize('prec', EXACT)
def test_two_runs_of_one_masked_fit_give_the_same_bits(monkeypatch, prec):
    n, f, k = ec.MID
    V, P, b, W, H = problem(n, f, k, 3)
    _, (Vu, Pu, _, Hu) = inputs(prec, V, P, W, H)
    got = []
    for _ in range(2):
        with open_masked(monkeypatch, prec, Vu, Pu, b, k, ITERS) as ctx:
            got.append(gpu_fit(ctx, Hu))
    for a, c in zip(*got):
        assert np.array_equal(a, c)


@pytest.mark.parametrize('prec', EXACT)
def test_a_pooled_context_forgets_the_mask(monkeypatch, prec):
    """A masked fit, then an unweighted fit of the same shape in the same pooled context: exactly a fresh context's result.
    klnmf_set_problem and klnmf_release_problem drop the mask; klnmf_clear_weights does on a live problem."""
    monkeypatch.delenv('KLNMF_NO_POOL', raising=False)
    n, f, k = ec.MID
    V, P, b, W, H = problem(n, f, k, 3)
    _, (Vu, Pu, _, Hu) = inputs(prec, V, P, W, H)
    with open_problem(monkeypatch, prec, Vu, k, ITERS) as fresh:
        want = gpu_fit(fresh, Hu)
    ctx = _native.Context(prec, pooled=True)
    handle = ctx._h.value
    ctx.set_problem(n, f, k, ITERS)
    ctx.upload_V(Vu)
    ctx.upload_presence(Pu, b)
    masked = gpu_fit(ctx, Hu)
    assert not np.array_equal(masked[1], want[1])
    ctx.set_problem(n, f, k, ITERS)                       # the same context, a new problem
    assert ctx.presence() == 0
    ctx.upload_V(Vu)
    again = gpu_fit(ctx, Hu)
    ctx.upload_presence(Pu, b)
    assert ctx.presence() == 3
    ctx.clear_weights()
    assert ctx.presence() == 0 and not ctx.weighted()
    cleared = gpu_fit(ctx, Hu)
    ctx.upload_presence(Pu[:7], b, row0=5)                # left masked when it goes back to the pool
    ctx.close()
    with _native.Context(prec, pooled=True) as ctx2:      # the pool hands the same native context out
        assert ctx2._h.value == handle
        ctx2.set_problem(n, f, k, ITERS)
        assert ctx2.presence() == 0
        ctx2.upload_V(Vu)
        pooled = gpu_fit(ctx2, Hu)
    for got in (again, cleared, pooled):
        for a, c in zip(got, want):
            assert np.array_equal(a, c)


def test_rows_of_the_mask_land_where_they_are_put(monkeypatch):
    """The first upload fills P with 1; row pieces (float32 or float64, strided views) replace their rows; the bounds are fixed."""
    n, f, k = 70, 90, 3
    V, P, b, W, H = problem(n, f, k, 3)
    wide = np.zeros((n, 7))
    wide[:, 2:5] = P
    with open_masked(monkeypatch, 'f64', V, P, b, k, 1) as ctx:
        whole = gpu_step(ctx, W, H)
    with open_problem(monkeypatch, 'f64', V, k, 1) as ctx:
        ctx.upload_presence(P[10:40], b, row0=10)
        assert ctx.presence() == 3 and not ctx.weighted()
        part = np.ones((n, 3))
        part[10:40] = P[10:40]
        got = gpu_step(ctx, W, H)
        check_step('f64 70x90k3 rows 10..39', 'f64', got, wc.ref_step_w(V, pc.omega(part, b), W, H,
                                                                         *ec.exact_regime(n, f, k, cu_count())[1:4:2]), V, pc.omega(part, b))
        ctx.upload_presence(wide[:10, 2:5], b)                          # a strided view
        ctx.upload_presence(wide[40:, 2:5], b, row0=40)
        pieces = gpu_step(ctx, W, H)
        with pytest.raises(_native.NativeError) as e:
            ctx.upload_presence(P, [0, 31, 60, 90])                     # other bounds
        assert e.value.code == _native.ERR_ARG and 'bounds' in str(e.value)
        with pytest.raises(_native.NativeError) as e:
            ctx.upload_presence(P[:, :2], [0, 30, 90])                  # another count
        assert e.value.code == _native.ERR_ARG
        assert ctx.presence() == 3 and not ctx.weighted()
        after = gpu_step(ctx, W, H)
        ctx.upload_presence(P.astype(np.float32), b)
        single = gpu_step(ctx, W, H)
    for a, c, d in zip(whole, pieces, after):
        assert np.array_equal(a, c) and np.array_equal(a, d)
    with open_masked(monkeypatch, 'f64', V, ec.as_f32(P), b, k, 1) as ctx:
        for a, c in zip(gpu_step(ctx, W, H), single):
            assert np.array_equal(a, c)


def test_refusals_leave_the_context_usable(monkeypatch):
    n, f, k = 64, 256, 16
    V, P, b, W, H = problem(n, f, k, 3)
    Om = pc.omega(P, b)
    # a CSR problem
    X = sp.csr_matrix(V * (Om > 0.5))
    with _native.Context('f64') as ctx:
        ctx.set_problem_sparse(X, k, 2)
        ctx.set_H(H)
        ctx.set_W(W)
        before = ctx.error()
        with pytest.raises(_native.NativeError) as e:
            ctx.upload_presence(P, b)
        assert e.value.code == _native.ERR_UNSUPP and 'CSR' in str(e.value)
        assert ctx.presence() == 0 and ctx.error() == before
    # every precision but f64 and f32
    for prec in ('f16', 'bf16x3', 'f16x3'):
        with _native.Context(prec) as ctx:
            ctx.set_problem(n, f, k, 2)
            ctx.upload_blocks([V])
            ctx.set_H(H)
            ctx.init_W()
            want = ctx.run(2, True, ec.NO_STOP)[0]
            with pytest.raises(_native.NativeError) as e:
                ctx.upload_presence(P, b)
            assert e.value.code == _native.ERR_UNSUPP and 'KLNMF_PREC_F64' in str(e.value)
            assert ctx.presence() == 0
            ctx.set_H(H)
            ctx.init_W()
            errors, n_done, _ = ctx.run(2, True, ec.NO_STOP)
            assert n_done == 2 and (prec == 'f16' or list(errors) == list(want)) and np.all(np.isfinite(errors))
    with open_problem(monkeypatch, 'f64', V, k, 2) as ctx:
        plain = gpu_fit(ctx, H, 2)
        # bad bounds, too many modalities, rows out of range: the problem stays unweighted
        bad = [(P, [1, 100, 200, f]), (P, [0, 100, 200, f - 1]), (P, [0, 100, 200, f + 1]), (P, [0, 100, 100, f]), (P, [0, 200, 100, f]),
               (np.ones((n, 17)), list(range(17)) + [f]), (np.ones((n + 1, 3)), b), (np.ones((0, 0)), [0])]
        for Pb, bb in bad:
            with pytest.raises(_native.NativeError) as e:
                ctx.upload_presence(Pb, bb)
            assert e.value.code == _native.ERR_ARG, bb
        for row0 in (-1, 1, n):
            with pytest.raises(_native.NativeError) as e:
                ctx.upload_presence(P, b, row0=row0)
            assert e.value.code == _native.ERR_ARG
        assert ctx.presence() == 0 and not ctx.weighted()
        for a, c in zip(gpu_fit(ctx, H, 2), plain):
            assert np.array_equal(a, c)
        # a mask on a problem that holds weights, weights on a problem that holds a mask
        ctx.upload_weights(Om)
        weighted = gpu_fit(ctx, H, 2)
        with pytest.raises(_native.NativeError) as e:
            ctx.upload_presence(P, b)
        assert e.value.code == _native.ERR_ARG and 'klnmf_upload_weights' in str(e.value)
        assert ctx.weighted() and ctx.presence() == 0
        for a, c in zip(gpu_fit(ctx, H, 2), weighted):
            assert np.array_equal(a, c)
        ctx.clear_weights()
        ctx.upload_presence(P, b)
        want = gpu_fit(ctx, H, 2)
        with pytest.raises(_native.NativeError) as e:
            ctx.upload_weights(Om)
        assert e.value.code == _native.ERR_ARG and 'presence' in str(e.value)
        with pytest.raises(_native.NativeError) as e:
            ctx.upload_weights(Om[:, :5], col0=f - 4)             # (a refusal upload_weights had: unchanged, and first)
        assert e.value.code == _native.ERR_ARG and 'out of range' in str(e.value)
        assert ctx.presence() == 3 and not ctx.weighted()
        for a, c in zip(gpu_fit(ctx, H, 2), want):
            assert np.array_equal(a, c)
        # a group: at its creation, and at its run if the mask came later
        with pytest.raises(_native.NativeError) as e:
            _native.Group([ctx])
        assert e.value.code == _native.ERR_UNSUPP and 'presence' in str(e.value)
        ctx.clear_weights()
        gpu_init_W(ctx, H)
        with _native.Group([ctx]) as group:
            ctx.upload_presence(P, b)
            with pytest.raises(_native.NativeError) as e:
                group.run(n, 2, True, 0.0)
            assert e.value.code == _native.ERR_UNSUPP
        with pytest.raises(_native.NativeError) as e:
            ctx.loop_begin(1.0, 1.0)                       # the loop sequenced by the caller over row shards
        assert e.value.code == _native.ERR_UNSUPP
        for a, c in zip(gpu_fit(ctx, H, 2), want):
            assert np.array_equal(a, c)
        # ... and a mask that arrives while such a loop is open
        ctx.clear_weights()
        gpu_init_W(ctx, H)
        ctx.loop_begin(float(V.sum()), float(n * f))
        with pytest.raises(_native.NativeError) as e:
            ctx.upload_presence(P, b)
        assert e.value.code == _native.ERR_UNSUPP and 'row shards' in str(e.value)
        assert ctx.presence() == 0
        ctx.iter_rowpass(True)
        ctx.iter_decide(ec.NO_STOP)
        ctx.iter_colpass()
        ctx.iter_update_H()
        ctx.iter_advance()
        assert ctx.loop_end(2)[1] == 1
        ctx.upload_presence(P, b)                          # the loop has ended
        for a, c in zip(gpu_fit(ctx, H, 2), want):
            assert np.array_equal(a, c)


# ---- through the public API -------------------------------------------------------------------------------------------------------
def model(k, H0, iters=ITERS, **kw):
    m = nmf.KLdivNMF(n_components=k, max_iter=iters, tol=ec.NO_STOP, **kw)
    m._init_dictionary = H0
    return m


def test_learner_with_a_presence_column(monkeypatch):
    """test_weighted_gpu's learner case: train / reconstruct_internal_multi with an (n, 1) presence column on the second of two
    modalities take the mask; the stacked matrix with the stacked (n, f) weights takes the weight buffer."""
    n, dims, k, coefs = 60, [40, 30], 5, [1.0, 0.5]
    rng = np.random.default_rng(21)
    A, B = rng.gamma(1.0, 1.0, (n, dims[0])) + 0.05, rng.gamma(1.0, 1.0, (n, dims[1])) + 0.05
    present = (rng.random((n, 1)) > 0.3).astype(np.float64)
    B = B * present                                       # a missing modality is stored as zeros
    stacked = np.hstack([coefs[0] * A, coefs[1] * B])
    weights = np.hstack([np.ones((n, dims[0])), np.broadcast_to(present, (n, dims[1]))])
    masks = []
    real = _native.Context.upload_presence
    monkeypatch.setattr(_native.Context, 'upload_presence', lambda self, P, cb, row0=0: (masks.append(list(cb)), real(self, P, cb, row0))[1])
    learner = MultimodalLearner(['a', 'b'], dims, coefs, k)
    np.random.seed(3)
    learner.train([A, B], ITERS, weights=[None, present])
    assert learner.nmf_train.last_weights_route == 'presence' and masks == [[0, 40, 70]]
    np.random.seed(3)
    m = nmf.KLdivNMF(n_components=k, max_iter=ITERS, tol=0)
    W = m.fit_transform(stacked, weights=weights)
    assert m.last_weights_route == 'array'
    bars = BARS['f64']
    check('learner train', 'dico', learner.dico, m.components_, bars['fit_factor'])
    got = learner.reconstruct_internal_multi(['a', 'b'], [A, B], ITERS, weights=[None, present])
    assert masks == [[0, 40, 70]] * 2                     # (the transform behind it took the mask too)
    m2 = nmf.KLdivNMF(n_components=k, max_iter=ITERS, tol=0)
    m2.components_ = learner.dico
    check('learner reconstruct', 'internal', got, m2.transform(stacked, weights=weights), bars['fit_factor'])
    assert m2.last_weights_route == 'array' and masks == [[0, 40, 70]] * 2 and W.shape == got.shape == (n, k)


def test_the_route_fit_transform_takes():
    n, f, k = 300, 700, 17
    V, P, b, _, H0 = problem(n, f, k, 1)
    col = P[:, :1]
    full = np.broadcast_to(col, (n, f))
    _, kchunk, _, wchunk, _, _ = ec.exact_regime(n, f, k, cu_count())
    m = model(k, H0, precision='f64')
    assert m.last_weights_route is None
    W, errors = m.fit_transform(V, weights=col, return_errors=True)
    assert m.last_weights_route == 'presence'
    ref = wc.ref_fit_w(V, full, H0, ITERS, kchunk=kchunk, wchunk=wchunk)
    check_fit('f64 fit_transform weights (n, 1)', 'f64', (W, m.components_, np.array(errors)), ref, V, full)
    Wt = m.transform(V, weights=col)
    assert m.last_weights_route == 'presence' and Wt.shape == (n, k)
    m = model(k, H0, iters=2, precision='f64')
    for w, route in ((np.ascontiguousarray(full), 'array'), (full[0], 'array'), (col, 'presence'), (1.0, None)):
        m.fit_transform(V, weights=w)
        assert m.last_weights_route == route
    m.fit_transform(V)
    assert m.last_weights_route is None


def test_the_16_bit_mode_runs_a_presence_column_in_f32_and_says_so_once(capsys):
    n, f, k = 300, 700, 17
    V, P, b, _, H0 = problem(n, f, k, 1)
    col = P[:, :1]
    Vr, colr, Hr = (ec.as_f32(a) for a in (V, col, H0))
    full = np.broadcast_to(colr, (n, f))
    nmf._NOTED.clear()
    capsys.readouterr()
    _, kchunk, _, wchunk, _, _ = ec.exact_regime(n, f, k, cu_count(), 4)
    ref = wc.ref_fit_w(Vr, full, Hr, ITERS, kchunk=kchunk, wchunk=wchunk)
    for _ in range(2):
        m = model(k, H0.astype(np.float32), precision='f16')
        W, errors = m.fit_transform(V.astype(np.float32), weights=col.astype(np.float32), return_errors=True)
        assert m.last_weights_route == 'presence'
        check_fit('f16 -> f32 fit_transform (n, 1)', 'f32', (W, m.components_, np.array(errors)), ref, Vr, full)
    err = capsys.readouterr().err
    assert err.count("weights with precision='f16' run on the fp32 weighted kernels") == 1 and err.count('\n') == 1, err
