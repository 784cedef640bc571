"""Batches (klnmf_batch_*, multimodal_amd/csrc/batch.hip.h): B dense, unweighted problems of one shape advancing through the
loop together, one launch per stage.

What is held to what:
  * every problem of a batch against THE SAME problem alone in a `_native.Context` whose KLNMF_EX_ROW_CHUNKS /
    KLNMF_EX_W_CHUNKS are forced to the counts the batch reports: W0, W, H, the loss record, n_done and the stop flag BIT FOR
    BIT (np.array_equal: no tolerance) -- on the natural routes, on forced routes, with problems that stop apart, in
    transforms and across re-use;
  * and against the chunked fp64 reference (tests/exact_cases.ref_fit), within tests/test_exact_gpu.py's bars, restated:
        f64   fit losses 1e-10, fit W and H 1e-9
        f32   fit losses 3e-5 (relative to at least 2^-23 sum(V)), fit W and H 3e-4 relative to max(|reference|, the
              smallest normal fp32 number) -- the reference fed the fp32-rounded inputs
    (one step / W0: 1e-12 and 3e-5);
  * the batch's reported counts against tests/exact_cases.exact_regime for max(1, cu_count // B) compute units.
Every problem of a batch has its own data (a seed per problem) and its own H0.  Fits never stop early (NO_STOP) except in
the test that is about stopping.
"""
import functools

import numpy as np
import pytest

from multimodal_amd import _native
from oracle import klnmf_oracle as orc
from tests import exact_cases as ec
from tests.loop_piece_cases import stop_rule
from tests.test_sparse_gpu import _MEASURED, _report_measured, check  # noqa: F401  (the autouse fixture prints what was measured)

pytestmark = pytest.mark.gpu

ITERS = 10
TINY32 = float(np.finfo(np.float32).tiny)
BARS = {'f64': {'step': 1e-12, 'fit_loss': 1e-10, 'fit_factor': 1e-9},
        'f32': {'step': 3e-5, 'fit_loss': 3e-5, 'fit_factor': 3e-4}}
FLOOR = {'f64': 0.0, 'f32': TINY32}
PRECS = ['f64', 'f32']
SWITCHES = ('KLNMF_EX_ROW_CHUNKS', 'KLNMF_EX_W_CHUNKS', 'KLNMF_EX_H_SEG')


@functools.lru_cache(maxsize=None)
def cu_count():
    return _native.device_info()['cu_count']


def esize(prec):
    return 8 if prec == 'f64' else 4


def loss_floor(prec, V):
    return 0.0 if prec == 'f64' else 2.0 ** -23 * float(V.sum())


@functools.lru_cache(maxsize=8)
def problem(n, f, k, p):
    """(V, H0) of problem p of a batch, fp64: its own data and its own initial dictionary."""
    V = ec.data(n, f, seed=1000 * p + n + 7 * f + 13 * k, zero_row=n // 2 if n >= 4 else None, zero_col=f // 3 if f >= 4 else None)
    _, H0 = ec.factors(n, f, k, seed=100 * p + k + 1)
    return V, H0


def rank_one(n, f, seed):
    """V = w.h exactly of rank 1 with h summing to 1, of the order of `exact_cases.data`."""
    rng = np.random.default_rng(seed)
    w = (rng.random((n, 1)) + 0.05) * f
    h = orc.normalize_sum(rng.random((1, f)) + 0.05, axis=1)
    return w.dot(h)


def upload_form(prec, a):
    return np.asarray(a, np.float64 if prec == 'f64' else np.float32)


def seen(prec, a):
    """What the kernels of `prec` see of an fp64 input, in fp64."""
    return a if prec == 'f64' else ec.as_f32(a)


@functools.lru_cache(maxsize=16)
def reference(n, f, k, p, f32_inputs, kchunk, wchunk, fit):
    V, H0 = problem(n, f, k, p)
    if f32_inputs:
        V, H0 = ec.as_f32(V), ec.as_f32(H0)
    return ec.ref_init_W(V, H0, wchunk), ec.ref_fit(V, H0, ITERS, fit=fit, components=H0, kchunk=kchunk, wchunk=wchunk)


def set_switches(monkeypatch, row_chunks=0, w_chunks=0, h_seg=0):
    monkeypatch.setenv('KLNMF_DEV', '1')
    for name, v in zip(SWITCHES, (row_chunks, w_chunks, h_seg)):
        if v:
            monkeypatch.setenv(name, str(v))
        else:
            monkeypatch.delenv(name, raising=False)


def batch_run(batch, prec, Vs, H0s, iters=ITERS, fit=True, tol_abs=ec.NO_STOP, components=None):
    """[(W0, W, H, errors, n_done, stopped)] per problem: upload, W0 = V.H0^T, the loop."""
    for p, (V, H0) in enumerate(zip(Vs, H0s)):
        batch.upload_V(p, upload_form(prec, V))
        batch.set_H(p, upload_form(prec, H0))
    batch.init_W()
    W0s = [batch.get_W(p) for p in range(batch.count)]
    if components is not None:
        for p, H in enumerate(components):
            batch.set_H(p, upload_form(prec, H))
    results = batch.run(iters, fit, tol_abs)
    return [(W0s[p], batch.get_W(p), batch.get_H(p), np.array(results[p][0]), results[p][1], results[p][2]) for p in range(batch.count)]


def solo_run(monkeypatch, prec, V, H0, k, regime, iters=ITERS, fit=True, tol_abs=ec.NO_STOP, components=None, h_seg=0, natural=False):
    """The same problem alone in a context, its chunk counts forced to `regime`'s (natural: the context's own plan)."""
    if natural:
        set_switches(monkeypatch)
    else:
        set_switches(monkeypatch, row_chunks=regime[0], w_chunks=regime[1], h_seg=h_seg)
    with _native.Context(prec) as ctx:
        ctx.set_problem(V.shape[0], V.shape[1], k, iters)
        if not natural:
            assert ctx.exact_regime() == tuple(regime), (ctx.exact_regime(), regime)
        ctx.upload_V(upload_form(prec, V))
        ctx.set_H(upload_form(prec, H0))
        ctx.init_W()
        W0 = ctx.get_W()
        if components is not None:
            ctx.set_H(upload_form(prec, components))
        errors, n_done, stopped = ctx.run(iters, fit, tol_abs)
        return W0, ctx.get_W(), ctx.get_H(), np.array(errors), n_done, stopped, ctx.exact_regime()


def assert_same_bits(case, got, solo):
    for name, a, b in zip(('W0', 'W', 'H', 'losses'), got[:4], solo[:4]):
        assert a.shape == b.shape and np.array_equal(a, b), '%s: %s differs from the solo run in %d of %d elements (max %.3e)' % (
            case, name, int((a != b).sum()), a.size, float(np.max(np.abs(a - b))))
    assert got[4] == solo[4] and got[5] == solo[5], '%s: (n_done, stopped) %r, solo %r' % (case, got[4:6], solo[4:6])


def check_against_reference(case, prec, got, ref, V):
    W0r, (Wr, Hr, er) = ref
    check(case, 'W0', got[0], W0r, BARS[prec]['step'], FLOOR[prec])
    assert len(got[3]) == len(er)
    check(case, 'losses', got[3], er, BARS[prec]['fit_loss'], loss_floor(prec, V))
    check(case, 'W', got[1], Wr, BARS[prec]['fit_factor'], FLOOR[prec])
    check(case, 'H', got[2], Hr, BARS[prec]['fit_factor'], FLOOR[prec])


# ---- 1. B = 1 is the context --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('shape', [(65, 65, 65), ec.MID], ids=ec.case_id)
def test_a_batch_of_one_is_the_context(monkeypatch, prec, shape):
    n, f, k = shape
    V, H0 = problem(n, f, k, 0)
    solo = solo_run(monkeypatch, prec, V, H0, k, None, natural=True)
    set_switches(monkeypatch)
    with _native.Batch(prec, 1) as batch:
        batch.set_problem(n, f, k, ITERS)
        assert batch.exact_regime() == solo[6]
        assert batch.query(_native.Q_BATCH_COUNT) == 1
        got = batch_run(batch, prec, [V], [H0])[0]
    assert got[4] == ITERS
    assert_same_bits('%s %s B=1' % (prec, ec.case_id(shape)), got, solo)


# ---- 2. batch against solo runs and the fp64 reference ---------------------------------------------------------------------------
SHAPES = [(15, 17, 1), (65, 65, 65), (300, 700, 17), ec.MID, (4096, 128, 16), (4096, 129, 16)]
BATCHES = [(s, B) for s in SHAPES for B in (2, 3, 5)] + [((100, 16385, 33), 2)]


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('shape,B', BATCHES, ids=['%s-B%d' % (ec.case_id(s), B) for s, B in BATCHES])
def test_batch_against_solo_runs_and_the_reference(monkeypatch, prec, shape, B):
    n, f, k = shape
    cu_eff = max(1, cu_count() // B)
    s, kchunk, w, wchunk, h, slabs = ec.exact_regime(n, f, k, cu_eff, esize(prec))
    probs = [problem(n, f, k, p) for p in range(B)]
    set_switches(monkeypatch)
    with _native.Batch(prec, B) as batch:
        batch.set_problem(n, f, k, ITERS)
        regime = batch.exact_regime()
        assert regime == ec.query_regime(n, f, k, cu_eff, esize=esize(prec)) == (s, w, h, int(slabs))
        got = batch_run(batch, prec, [v for v, _ in probs], [h0 for _, h0 in probs])
    for p, (V, H0) in enumerate(probs):
        case = '%s %s B=%d p=%d %r' % (prec, ec.case_id(shape), B, p, regime)
        assert got[p][4] == ITERS and not got[p][5]
        assert_same_bits(case, got[p], solo_run(monkeypatch, prec, V, H0, k, regime))
        check_against_reference(case, prec, got[p], reference(n, f, k, p, prec != 'f64', kchunk, wchunk, True), seen(prec, V))


# ---- 3. forced routes on the batch ---------------------------------------------------------------------------------------------
FORCED = ([('row_chunks', r) for r in ec.FORCED_ROW_CHUNKS] + [('w_chunks', c) for c in ec.FORCED_W_CHUNKS]
          + [('h_seg', L) for L in ec.FORCED_H_SEG])


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('forced', FORCED, ids=['%s-%d' % fv for fv in FORCED])
def test_forced_routes_on_the_batch(monkeypatch, prec, forced):
    n, f, k = ec.MID
    B = 2
    kw = {forced[0]: forced[1]}
    cu_eff = max(1, cu_count() // B)
    s, kchunk, w, wchunk, h, slabs = ec.exact_regime(n, f, k, cu_eff, esize(prec), **kw)
    probs = [problem(n, f, k, p) for p in range(B)]
    set_switches(monkeypatch, **kw)
    with _native.Batch(prec, B) as batch:
        batch.set_problem(n, f, k, ITERS)
        regime = batch.exact_regime()
        assert regime == (s, w, h, int(slabs))
        got = batch_run(batch, prec, [v for v, _ in probs], [h0 for _, h0 in probs])
    for p, (V, H0) in enumerate(probs):
        case = '%s %s=%d p=%d %r' % (prec, forced[0], forced[1], p, regime)
        solo = solo_run(monkeypatch, prec, V, H0, k, regime, h_seg=kw.get('h_seg', 0))
        assert_same_bits(case, got[p], solo)
        check_against_reference(case, prec, got[p], reference(n, f, k, p, prec != 'f64', kchunk, wchunk, True), seen(prec, V))


# ---- 4. problems that stop apart ---------------------------------------------------------------------------------------------------
STOP_SHAPE, STOP_CAP, STOP_TOL = (300, 700, 17), 40, 1.0


@pytest.mark.parametrize('prec', PRECS)
def test_problems_that_stop_apart(monkeypatch, prec):
    """Problem 0 is exactly of rank 1: its loss is at rounding level after one update and the rule (tol_abs = 1) fires at the
    third evaluation; the generic problems lose 70 and more per iteration and run to the cap."""
    n, f, k = STOP_SHAPE
    B = 3
    Vs = [rank_one(n, f, 5)] + [problem(n, f, k, p)[0] for p in (1, 2)]
    H0s = [problem(n, f, k, p)[1] for p in range(B)]
    cu_eff = max(1, cu_count() // B)
    s, kchunk, w, wchunk, h, slabs = ec.exact_regime(n, f, k, cu_eff, esize(prec))
    # the fp64 reference stops problem 0 early and runs the others to the cap
    ref_done = [stop_rule(ec.ref_fit(V, H0, STOP_CAP, kchunk=kchunk, wchunk=wchunk)[2], STOP_TOL) for V, H0 in zip(Vs, H0s)]
    assert 0 < ref_done[0] < 16 and ref_done[1] == ref_done[2] == STOP_CAP, ref_done
    set_switches(monkeypatch)
    with _native.Batch(prec, B) as batch:
        batch.set_problem(n, f, k, STOP_CAP)
        regime = batch.exact_regime()
        got = batch_run(batch, prec, Vs, H0s, iters=STOP_CAP, tol_abs=STOP_TOL)
    for p in range(B):
        solo = solo_run(monkeypatch, prec, Vs[p], H0s[p], k, regime, iters=STOP_CAP, tol_abs=STOP_TOL)
        assert_same_bits('%s stop p=%d' % (prec, p), got[p], solo)
        assert len(got[p][3]) == got[p][4]
    assert got[0][5] and not got[1][5] and not got[2][5]
    assert got[0][4] < got[1][4] == got[2][4] == STOP_CAP
    if prec == 'f64':
        assert [g[4] for g in got] == ref_done


# ---- 5. transform ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('shape', [(65, 65, 65), (300, 700, 17)], ids=ec.case_id)
def test_transform_with_a_dictionary_per_problem(monkeypatch, prec, shape):
    n, f, k = shape
    B = 3
    probs = [problem(n, f, k, p) for p in range(B)]
    cu_eff = max(1, cu_count() // B)
    s, kchunk, w, wchunk, h, slabs = ec.exact_regime(n, f, k, cu_eff, esize(prec))
    set_switches(monkeypatch)
    with _native.Batch(prec, B) as batch:
        batch.set_problem(n, f, k, ITERS)
        regime = batch.exact_regime()
        got = batch_run(batch, prec, [v for v, _ in probs], [h0 for _, h0 in probs], fit=False)
    for p, (V, H0) in enumerate(probs):
        case = '%s %s transform p=%d' % (prec, ec.case_id(shape), p)
        assert np.array_equal(got[p][2], seen(prec, H0)), case + ': the dictionary changed'
        assert_same_bits(case, got[p], solo_run(monkeypatch, prec, V, H0, k, regime, fit=False))
        check_against_reference(case, prec, got[p], reference(n, f, k, p, prec != 'f64', kchunk, wchunk, False), seen(prec, V))


# ---- 6. reuse and refusals ---------------------------------------------------------------------------------------------------------
def raises(code, fn, *args, **kw):
    with pytest.raises(_native.NativeError) as e:
        fn(*args, **kw)
    assert e.value.code == code, e.value
    return e.value


@pytest.mark.parametrize('prec', PRECS)
def test_reuse_and_refusals(monkeypatch, prec):
    n, f, k = 300, 700, 17
    B = 3
    probs = [problem(n, f, k, p) for p in range(B)]
    Vs, H0s = [v for v, _ in probs], [h0 for _, h0 in probs]
    set_switches(monkeypatch)
    for name in ('f16', 'bf16x3', 'f16x3'):
        raises(_native.ERR_UNSUPP, _native.Batch, name, B)
    for count in (0, _native.BATCH_MAX + 1):
        raises(_native.ERR_ARG, _native.Batch, prec, count)

    def same(a, b):
        for p in range(B):
            assert_same_bits('%s reuse p=%d' % (prec, p), a[p], b[p])
    with _native.Batch(prec, B) as batch:
        batch.set_problem(n, f, k, ITERS)
        first = batch_run(batch, prec, Vs, H0s)
        same(batch_run(batch, prec, Vs, H0s), first)          # two runs of one batch after re-upload
        # refusals: each leaves the batch usable
        raises(_native.ERR_ARG, batch.upload_V, B, upload_form(prec, Vs[0]))
        raises(_native.ERR_ARG, batch.upload_V, -1, upload_form(prec, Vs[0]))
        raises(_native.ERR_ARG, batch.set_H, B, upload_form(prec, H0s[0]))
        raises(_native.ERR_ARG, batch.get_W, B)
        raises(_native.ERR_ARG, batch.result, B)
        raises(_native.ERR_ARG, batch.set_problem, 0, f, k, ITERS)
        same(batch_run(batch, prec, Vs, H0s), first)
        # another shape, a run with a problem lacking V refused, and back
        batch.set_problem(65, 65, 65, ITERS)
        other = [problem(65, 65, 65, p) for p in range(B)]
        for p in range(B - 1):
            batch.upload_V(p, upload_form(prec, other[p][0]))
        for p in range(B):
            batch.set_H(p, upload_form(prec, other[p][1]))
        raises(_native.ERR_ARG, batch.run, ITERS, True, ec.NO_STOP)
        batch.upload_V(B - 1, upload_form(prec, other[B - 1][0]))
        small = batch_run(batch, prec, [v for v, _ in other], [h for _, h in other])
        assert all(g[4] == ITERS for g in small)
        batch.set_problem(n, f, k, ITERS)
        raises(_native.ERR_ARG, batch.run, ITERS, True, ec.NO_STOP)          # nothing uploaded yet
        same(batch_run(batch, prec, Vs, H0s), first)


# ---- 7. the Python layers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', PRECS)
def test_fit_transform_batch(prec):
    from multimodal_amd.lib.nmf import KLdivNMF, fit_transform_batch
    n, f, k = 300, 700, 17
    probs = [problem(n, f, k, p) for p in range(3)]

    def models():
        out = []
        for _, H0 in probs:
            m = KLdivNMF(n_components=k, max_iter=ITERS, tol=0, precision=prec, device=0)
            m._init_dictionary = H0
            out.append(m)
        return out
    batched = models()
    outs = fit_transform_batch(batched, [v for v, _ in probs], return_errors=True)
    for p, (m, (W, errors)) in enumerate(zip(batched, outs)):
        assert m.last_batch_size == 3
        alone = models()[p]
        Wa, ea = alone.fit_transform(probs[p][0], return_errors=True)
        case = '%s fit_transform_batch p=%d' % (prec, p)
        assert m.last_fp8_report == alone.last_fp8_report
        check(case, 'losses', errors, ea, BARS[prec]['fit_loss'], loss_floor(prec, probs[p][0]))
        check(case, 'W', W, Wa, BARS[prec]['fit_factor'], FLOOR[prec])
        check(case, 'H', m.components_, alone.components_, BARS[prec]['fit_factor'], FLOOR[prec])
    # Xs of unequal shapes: the sequential path, its bits
    Xs = [probs[0][0], probs[1][0][:200], probs[2][0]]
    seq = models()
    outs = fit_transform_batch(seq, Xs, return_errors=True)
    for p, (m, (W, errors)) in enumerate(zip(seq, outs)):
        assert m.last_batch_size == 1
        alone = models()[p]
        Wa, ea = alone.fit_transform(Xs[p], return_errors=True)
        assert np.array_equal(W, Wa) and errors == ea and np.array_equal(m.components_, alone.components_)


def class_blocks(seed=0, n_labels=6, per_label=20, dims=(40, 60), noise=0.05):
    """Two paired modalities of n_labels x per_label samples: every label has its own positive pattern in each modality, every
    sample its label's patterns times (1 + small noise) -- nearest-example searches have one clear answer."""
    rng = np.random.default_rng(seed)
    labels = [l for l in range(n_labels) for _ in range(per_label)]
    mods = []
    for d in dims:
        patterns = rng.random((n_labels, d)) ** 3 + 0.02
        mods.append(patterns[labels] * (1.0 + noise * rng.random((len(labels), d))))
    return mods, labels


@pytest.mark.parametrize('prec', PRECS)
def test_train_many_against_a_loop_over_train(monkeypatch, prec):
    from multimodal_amd.device_data import DeviceDataset
    from multimodal_amd.learner import MultimodalLearner
    monkeypatch.setenv('KLNMF_PRECISION', prec)
    monkeypatch.delenv('KLNMF_DEVICES', raising=False)
    data, _ = class_blocks()
    ds = DeviceDataset(data, device=0)
    k, n = 6, len(data[0])
    rng = np.random.default_rng(4)
    rows_list = [sorted(rng.permutation(n)[:90].tolist()) for _ in range(3)]
    inits = [ec.factors(90, sum(ds.dims), k, seed=p)[1] for p in range(3)]

    def learners():
        return [MultimodalLearner(['a', 'b'], list(ds.dims), [1.0, 0.5], k) for _ in range(3)]
    many = ds.train_many(learners(), rows_list, ITERS, init_dictionaries=inits)
    for p, (learner, alone) in enumerate(zip(many, learners())):
        ds.train(alone, rows_list[p], ITERS, init_dictionary=inits[p])
        assert learner.nmf_train.last_batch_size == 3
        check('%s train_many p=%d' % (prec, p), 'H', learner.dico, alone.dico, BARS[prec]['fit_factor'], FLOOR[prec])
    # transforms of the trained learners: the same route
    Ws = ds.reconstruct_internal_multi_many(many, ['a'], [r[:30] for r in rows_list], ITERS)
    for p, learner in enumerate(many):
        Wa = ds.reconstruct_internal_multi(learner, ['a'], rows_list[p][:30], ITERS)
        check('%s internal_many p=%d' % (prec, p), 'W', Ws[p], Wa, BARS[prec]['fit_factor'], FLOOR[prec])
    # row lists of unequal length: the loop over train, its bits
    uneven = [rows_list[0], rows_list[1][:80], rows_list[2]]
    inits_u = [ec.factors(len(r), sum(ds.dims), k, seed=p)[1] for p, r in enumerate(uneven)]
    seq = ds.train_many(learners(), uneven, ITERS, init_dictionaries=inits_u)
    for p, (learner, alone) in enumerate(zip(seq, learners())):
        ds.train(alone, uneven[p], ITERS, init_dictionary=inits_u[p])
        assert np.array_equal(learner.dico, alone.dico)
        assert getattr(learner.nmf_train, 'last_batch_size', 1) == 1


def test_run_sweep_in_batches_gives_the_unbatched_labels_and_scores(monkeypatch):
    """f64; the batched runs differ from the unbatched ones in summation order alone (other chunk counts): 1e-10 of the
    coefficients.  Every nearest-example search of the unbatched sweep is decided by more than 1e-6 relative (asserted), so the
    found labels, and with them the score tables, must be equal."""
    from multimodal_amd import device_data
    from multimodal_amd.device_experiment import run_sweep
    data, labels = class_blocks()
    original = device_data.DeviceEvaluation.found_labels
    found, margins = [], []

    def recording(self, test, examples, labels_ex, metric):
        out = self.torch.empty((test.shape[0], examples.shape[0]), dtype=self.torch.float64, device=self.dev)
        _native.all_distances_device(test.data_ptr(), test.stride(0), examples.data_ptr(), examples.stride(0), out.data_ptr(),
                                     test.shape[0], examples.shape[0], test.shape[1], metric, f64=True, device=self.dev.index or 0)
        d = np.sort(out.cpu().numpy(), axis=1)
        margins.extend(((d[:, 1] - d[:, 0]) / np.maximum(np.maximum(np.abs(d[:, 0]), np.abs(d[:, 1])), 1e-300)).tolist())
        got = original(self, test, examples, labels_ex, metric)
        found.append(list(got))
        return got
    monkeypatch.setattr(device_data.DeviceEvaluation, 'found_labels', recording)
    args = dict(ks=[6, 8], n_runs=2, iter_train=20, iter_test=20, devices=[0], precision='f64', seed=3)
    table1, raw1 = run_sweep(data, labels, ['a', 'b'], **args)
    found1, margins1 = list(found), list(margins)
    assert margins1 and np.all(np.isfinite(margins1)) and min(margins1) > 1e-6, min(margins1)
    del found[:], margins[:]
    opened = []
    real_batch = _native.Batch

    class CountingBatch(real_batch):
        def __init__(self, precision, count, device=0):
            opened.append(count)
            real_batch.__init__(self, precision, count, device)
    monkeypatch.setattr(_native, 'Batch', CountingBatch)
    table3, raw3 = run_sweep(data, labels, ['a', 'b'], batch=3, **args)
    assert opened and set(opened) == {2}                      # two runs per k: batches of two, trainings and transforms
    assert found == found1
    assert raw3 == raw1 and table3 == table1
