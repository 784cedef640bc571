"""The fused nearest-example search (include/klnmf_nearest.h, csrc/nearest.hip.h) against the distance matrices of the kernel it
replaces.

The reference throughout is `_native.all_distances_device` on the same operands -- k_all_distances, never the new kernel -- and
every comparison is exact: the index is np.argmin of that matrix (lowest index among equal minima, a NaN ahead of every number)
and the returned distance has the bits of the matrix element.  Nothing here has a tolerance.

  * every shape: d in eval_cases.DIMS x (na, nb) in eval_cases.SHAPES + (5, 2), (3, 5), (2, 260) (fewer examples than the
    W = 4 waves that share a row, more than one trip of the waves, 65 trips), f64 and f32, each single measure, the
    evaluation's four and all five, on eval_cases.pair_case's rows (zero rows, copies, scaled and sparse rows);
  * ties by construction, NaN rows, strided sub-views with guarded outputs, many jobs in one call (1, 2, 48, 385), refusals,
    the host form, and the public route (`perform_one_run` / `run_sweep` with search='fused').
"""
import ctypes

import numpy as np
import pytest

from multimodal_amd import _native
from tests import eval_cases as evc

pytestmark = pytest.mark.gpu

NP = {False: np.float64, True: np.float32}
BITS = {False: np.uint64, True: np.uint32}
W = 4                                   # kNearestWaves: the waves that share one row of A
ALL = _native.DIST_MASK_ALL
FOUR = _native.metric_mask([evc.KL, evc.REV_KL, evc.FROBENIUS, evc.COSINE_DIFF])        # device_experiment.DEVICE_MEASURES
MASKS = [1 << m for m in range(5)] + [FOUR, ALL]
SHAPES = evc.SHAPES + ((5, 2), (3, 5), (2, 260))
IDX_GUARD, DIST_GUARD = -77, -12345.0


def torch_mod():
    import torch
    return torch


def on_device(M, f32):
    torch = torch_mod()
    return torch.from_numpy(np.array(M, dtype=NP[f32], order='C')).to('cuda')       # (a copy: the cases are read-only)


_MATRICES = {}


def matrix(A, B, metric, f32, key=None):
    """[na, nb] of k_all_distances on device copies of A and B (cached under `key` where the caller names the case)."""
    if key is not None and (key, metric, f32) in _MATRICES:
        return _MATRICES[(key, metric, f32)]
    torch = torch_mod()
    na, d = A.shape
    nb = B.shape[0]
    dA, dB = on_device(A, f32), on_device(B, f32)
    out = torch.empty((na, nb), dtype=torch.float32 if f32 else torch.float64, device='cuda')
    _native.all_distances_device(dA.data_ptr(), d, dB.data_ptr(), d, out.data_ptr(), na, nb, d, metric, f64=not f32)
    D = out.cpu().numpy()
    D.setflags(write=False)
    if key is not None:
        _MATRICES[(key, metric, f32)] = D
    return D


def expected(A, B, mask, f32, key=None):
    """(indices [na, M], distances [na, M]) from the parent's matrices: np.argmin and the element it points at."""
    order = _native.mask_metrics(mask)
    idx = np.zeros((A.shape[0], len(order)), dtype=np.int32)
    val = np.zeros((A.shape[0], len(order)), dtype=NP[f32])
    for s, metric in enumerate(order):
        D = matrix(A, B, metric, f32, key)
        with np.errstate(invalid='ignore'):
            j = np.argmin(D, axis=1)
        idx[:, s] = j
        val[:, s] = D[np.arange(A.shape[0]), j]
    return idx, val


def search(jobs, mask, f32, with_dist=True):
    """klnmf_nearest_many_device on `jobs` = [(device A, lda, device B, ldb, na, nb, d)] into guarded outputs."""
    torch = torch_mod()
    M = len(_native.mask_metrics(mask))
    rows = sum(j[4] for j in jobs)
    idx = torch.full((rows * M + 8,), IDX_GUARD, dtype=torch.int32, device='cuda')
    dist = torch.full((rows * M + 8,), DIST_GUARD, dtype=torch.float32 if f32 else torch.float64, device='cuda')
    nbytes = _native.nearest_work_bytes(len(jobs), rows)
    work = torch.zeros((nbytes + 16,), dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    _native.nearest_many_device([(a.data_ptr(), lda, b.data_ptr(), ldb, na, nb, d) for a, lda, b, ldb, na, nb, d in jobs], mask,
                                idx.data_ptr(), dist.data_ptr() if with_dist else None, work.data_ptr(), nbytes, f64=not f32)
    hi, hd = idx.cpu().numpy(), dist.cpu().numpy()
    assert np.all(hi[rows * M:] == IDX_GUARD) and np.all(hd[rows * M:] == DIST_GUARD), 'written behind the outputs'
    if not with_dist:
        assert np.all(hd == DIST_GUARD)
    return hi[:rows * M].reshape(rows, M), hd[:rows * M].reshape(rows, M)


def one_search(A, B, mask, f32, with_dist=True):
    dA, dB = on_device(A, f32), on_device(B, f32)
    return search([(dA, A.shape[1], dB, A.shape[1], A.shape[0], B.shape[0], A.shape[1])], mask, f32, with_dist)


def assert_same(what, got, want, f32, nan=False):
    """Equal indices and distances of equal bits (nan: a NaN against a NaN, whatever its payload)."""
    (gi, gd), (wi, wd) = got, want
    assert np.array_equal(gi, wi), '%s: indices\n%s\n%s' % (what, gi, wi)
    gb, wb = np.ascontiguousarray(gd).view(BITS[f32]), np.ascontiguousarray(wd).view(BITS[f32])
    if nan:
        assert np.array_equal(np.isnan(gd), np.isnan(wd)), what + ': distances'
        gb, wb = gb[~np.isnan(gd)], wb[~np.isnan(wd)]
    assert np.array_equal(gb, wb), what + ': distances'


# ---- every shape against the matrix -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
@pytest.mark.parametrize('d', evc.DIMS)
def test_every_shape_and_mask_against_argmin_of_the_matrix(d, f32):
    ties = 0
    for na, nb in SHAPES:
        case = evc.pair_case(na, nb, d)
        A, B = case.A.astype(NP[f32]), case.B.astype(NP[f32])
        for mask in MASKS:
            want = expected(A, B, mask, f32, key=(na, nb, d))
            assert_same('%dx%d d=%d mask=%d' % (na, nb, d, mask), one_search(A, B, mask, f32), want, f32)
        for metric in range(5):
            D = matrix(A, B, metric, f32, key=(na, nb, d))
            ties += int(np.sum(np.sum(D == D.min(axis=1, keepdims=True), axis=1) > 1))
    assert ties > 0, 'the cases hold no exact tie'      # (zero rows against the cosine, d = 0, copies)


# ---- ties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
def test_the_lowest_index_among_equal_minima(f32):
    rng = np.random.default_rng(5)
    nb, d = 14, 65
    B = rng.random((nb, d)) + 0.05
    B[3] = B[2]                          # (j, j + 1): neighbours, met across two waves
    B[5 + W] = B[5]                      # (j, j + W): consecutive trips of ONE wave
    B[nb - 1] = B[7]                     # (j, nb - 1): the last example, in another wave
    A = np.concatenate([B[[2, 5, 7]], rng.random((1, d)) + 0.05])
    for mask in MASKS:
        got = one_search(A, B, mask, f32)
        assert_same('duplicates, mask %d' % mask, got, expected(A, B, mask, f32), f32)
        assert np.all(got[0][:3] == np.array([[2], [5], [7]])), (mask, got[0])
    same = np.tile(B[:1], (11, 1))
    for mask in MASKS:
        got = one_search(A, same, mask, f32)
        assert np.all(got[0] == 0), mask
        assert_same('equal rows, mask %d' % mask, got, expected(A, same, mask, f32), f32)


# ---- NaN ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
def test_nan_counts_as_the_smallest_value(f32):
    rng = np.random.default_rng(6)
    nb, d = 9, 65
    A = rng.random((5, d)) + 0.05
    for at in (0, nb // 2, nb - 1):
        B = rng.random((nb, d)) + 0.05
        B[at, 17] = np.nan
        got = one_search(A, B, ALL, f32)
        assert_same('NaN in example %d' % at, got, expected(A, B, ALL, f32), f32, nan=True)
        assert np.all(got[0] == at) and np.isnan(got[1]).all()
    B = rng.random((nb, d)) + 0.05
    B[[2, 6], 3] = np.nan                # two NaN rows, in two waves: the lower index
    got = one_search(A, B, ALL, f32)
    assert_same('two NaN examples', got, expected(A, B, ALL, f32), f32, nan=True)
    assert np.all(got[0] == 2)
    B = rng.random((nb, d)) + 0.05
    An = A.copy()
    An[1, 64] = np.nan
    got = one_search(An, B, ALL, f32)
    assert_same('NaN in a test row', got, expected(An, B, ALL, f32), f32, nan=True)
    assert np.all(got[0][1] == 0) and np.isnan(got[1][1]).all() and not np.isnan(got[1][[0, 2, 3, 4]]).any()


# ---- strided views ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
@pytest.mark.parametrize('d', [0, 65, 1000])
def test_strided_sub_views_and_guarded_outputs(d, f32):
    torch = torch_mod()
    na, nb = 7, 9
    case = evc.pair_case(na, nb, d)
    lda, ldb = d + 3, d + 5

    def padded(M, ld, off):
        host = np.full(off + M.shape[0] * ld + 4, np.nan, dtype=NP[f32])
        view = host[off:off + M.shape[0] * ld].reshape(M.shape[0], ld)
        view[:, :d] = M
        big = torch.from_numpy(host).to('cuda')
        return big, big[off:]
    bigA, subA = padded(case.A, lda, 7)
    bigB, subB = padded(case.B, ldb, 3)
    assert subA.data_ptr() == bigA.data_ptr() + 7 * bigA.element_size()
    A, B = case.A.astype(NP[f32]), case.B.astype(NP[f32])
    for mask in (FOUR, ALL):
        got = search([(subA, lda, subB, ldb, na, nb, d)], mask, f32)
        assert not np.isnan(got[1]).any(), 'the padding was read'
        assert_same('views d=%d mask=%d' % (d, mask), got, expected(A, B, mask, f32, key=(na, nb, d)), f32)


# ---- many jobs in one call ----------------------------------------------------------------------------------------------------------
POOL = ((5, 3, 65), (0, 4, 10), (3, 1, 7), (2, 6, 0), (7, 9, 129), (1, 3, 1), (33, 17, 64), (0, 0, 5), (2, 260, 63), (4, 4, 128))
LONG = (3, 5, 1000)


@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
def test_many_jobs_of_mixed_shapes_equal_each_job_alone(f32):
    alone, tensors = {}, {}
    for shape in POOL + (LONG,):
        na, nb, d = shape
        case = evc.pair_case(na, nb, d)
        tensors[shape] = (on_device(case.A, f32), d, on_device(case.B, f32), d, na, nb, d)
        alone[shape] = search([tensors[shape]], FOUR, f32) if na else (np.zeros((0, 4), np.int32), np.zeros((0, 4), NP[f32]))
        if na:
            assert_same('alone %s' % (shape,), alone[shape], expected(case.A.astype(NP[f32]), case.B.astype(NP[f32]), FOUR, f32), f32)
    for count in (1, 2, 48, 385):
        shapes = [POOL[q % len(POOL)] for q in range(count)]
        if count > 1:
            shapes[count // 2] = LONG                     # one job with d = 1000, in the middle
        want = (np.concatenate([alone[s][0] for s in shapes]), np.concatenate([alone[s][1] for s in shapes]))
        jobs = [tensors[s] for s in shapes]
        assert_same('%d jobs' % count, search(jobs, FOUR, f32), want, f32)
        assert np.array_equal(search(jobs, FOUR, f32, with_dist=False)[0], want[0]), '%d jobs without distances' % count


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_leave_the_process_usable():
    torch = torch_mod()
    lib = _native.load()
    na, nb, d, M = 5, 3, 65, 4
    case = evc.pair_case(na, nb, d)
    A, B = np.array(case.A), np.array(case.B)
    dA, dB = on_device(A, False), on_device(B, False)
    want = expected(A, B, FOUR, False)
    idx = torch.full((na * M + 8,), IDX_GUARD, dtype=torch.int32, device='cuda')
    dist = torch.full((na * M + 8,), DIST_GUARD, dtype=torch.float64, device='cuda')
    nbytes = _native.nearest_work_bytes(1, na)
    assert nbytes >= 4 * na + 8 and nbytes == _native.nearest_work_bytes(1, na)
    work = torch.zeros((nbytes,), dtype=torch.uint8, device='cuda')
    hidx, hdist = np.full((na, M), IDX_GUARD, dtype=np.int32), np.full((na, M), DIST_GUARD)
    torch.cuda.synchronize()
    v = ctypes.c_void_p
    p = lambda a: a.ctypes.data_as(v)

    def dev(dtype=_native.DT_F64, mask=FOUR, a=dA.data_ptr(), lda=d, b=dB.data_ptr(), ldb=d, na=na, nb=nb, d=d, count=1, jobs=True,
            i=idx.data_ptr(), w=work.data_ptr(), wb=nbytes):
        table = (_native.NearestJob * 1)(_native.NearestJob(a, lda, b, ldb, na, nb, d))
        return lib.klnmf_nearest_many_device(0, dtype, mask, ctypes.cast(table, v) if jobs else None, count, v(i), v(dist.data_ptr()),
                                             v(w), wb)

    def host(dtype=_native.DT_F64, mask=FOUR, na=na, nb=nb, d=d, a=p(A), b=p(B), i=p(hidx)):
        return lib.klnmf_nearest(0, dtype, mask, na, nb, d, a, b, i, p(hdist))

    def untouched():
        return (np.all(idx.cpu().numpy() == IDX_GUARD) and np.all(dist.cpu().numpy() == DIST_GUARD) and np.all(hidx == IDX_GUARD)
                and np.all(hdist == DIST_GUARD))

    def still_right():
        assert dev() == 0
        gi, gd = idx.cpu().numpy(), dist.cpu().numpy()
        assert_same('after a refusal', (gi[:na * M].reshape(na, M), gd[:na * M].reshape(na, M)), want, False)
        assert np.all(gi[na * M:] == IDX_GUARD) and np.all(gd[na * M:] == DIST_GUARD)
        assert host() == 0
        assert_same('after a refusal, host form', (hidx, hdist), want, False)
        idx.fill_(IDX_GUARD)
        dist.fill_(DIST_GUARD)
        hidx.fill(IDX_GUARD)
        hdist.fill(DIST_GUARD)
        torch.cuda.synchronize()

    refused = [lambda: dev(jobs=False), lambda: dev(i=None), lambda: dev(w=None), lambda: dev(a=None), lambda: dev(b=None),
               lambda: dev(lda=d - 1), lambda: dev(ldb=d - 1), lambda: dev(mask=0), lambda: dev(mask=32), lambda: dev(mask=-1),
               lambda: dev(dtype=7), lambda: dev(nb=0), lambda: dev(count=-1), lambda: dev(na=-1), lambda: dev(nb=-1), lambda: dev(d=-1),
               lambda: dev(wb=nbytes - 1), lambda: dev(wb=0), lambda: dev(count=_native.NEAREST_MAX_JOBS + 1),
               lambda: host(a=None), lambda: host(b=None), lambda: host(i=None), lambda: host(mask=0), lambda: host(mask=32),
               lambda: host(dtype=7), lambda: host(nb=0), lambda: host(na=-1), lambda: host(d=-1)]
    for n, call in enumerate(refused):
        status = call()
        assert status == _native.ERR_ARG, (n, status)
        with pytest.raises(_native.NativeError):
            _native._check(status)
        assert untouched(), n
        still_right()
    out = ctypes.c_uint64(0)
    for args in ((-1, 0), (0, -1), (_native.NEAREST_MAX_JOBS + 1, 0), (1, (1 << 24) + 1)):
        assert lib.klnmf_nearest_work_bytes(args[0], args[1], ctypes.byref(out)) == _native.ERR_ARG, args
    assert lib.klnmf_nearest_work_bytes(1, 1, None) == _native.ERR_ARG
    # nothing to do: success, nothing touched (no pointer is needed then)
    assert dev(count=0) == 0 and dev(count=0, jobs=False, i=None, w=None, wb=0) == 0 and dev(na=0) == 0 and dev(na=0, nb=0) == 0
    assert host(na=0) == 0 and host(na=0, nb=0) == 0
    assert untouched()
    with pytest.raises(ValueError):
        _native.nearest(A, B[:, :64], FOUR)
    with pytest.raises(_native.NativeError):
        _native.nearest(A, B, 0)
    still_right()


# ---- the host form ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
def test_the_host_form_equals_the_device_form(f32):
    from multimodal_amd import evaluation
    from multimodal_amd.lib import metrics
    for na, nb, d in ((7, 9, 129), (2, 260, 63), (3, 1, 0)):
        case = evc.pair_case(na, nb, d)
        A, B = case.A.astype(NP[f32]), case.B.astype(NP[f32])
        for mask in (1 << evc.SYM_KL, FOUR, ALL):
            idx, dist = _native.nearest(A, B, mask, return_distances=True)
            assert idx.dtype == np.int32 and dist.dtype == NP[f32]
            assert_same('host form %dx%d d=%d mask=%d' % (na, nb, d, mask), (idx, dist), one_search(A, B, mask, f32), f32)
            assert np.array_equal(_native.nearest(A, B, mask), idx)
    case = evc.pair_case(33, 17, 64)
    want = expected(np.array(case.A), np.array(case.B), ALL, False)[0]
    measures = [metrics.cosine_diff, metrics.kl_div, 'frobenius', metrics.rev_kl_div, 'sym_kl_div']
    code = {metrics.cosine_diff: 4, metrics.kl_div: 0, 'frobenius': 3, metrics.rev_kl_div: 1, 'sym_kl_div': 2}
    got = evaluation.nearest_examples(case.A, case.B, measures)
    assert list(got) == measures
    labels = [100 + j for j in range(17)]
    found = evaluation.classify_NN_measures(case.A, case.B, labels, measures)
    for m in measures:
        assert np.array_equal(got[m], want[:, code[m]]), m
        assert found[m] == [labels[j] for j in want[:, code[m]]]
    assert found[metrics.kl_div] == evaluation.classify_NN(case.A, case.B, labels, metrics.kl_div)
    with pytest.raises(ValueError):
        evaluation.nearest_examples(case.A, case.B, ['manhattan'])


# ---- the public route ---------------------------------------------------------------------------------------------------------------
class Calls(object):
    """Counting wrappers on the three device searches."""

    def __init__(self, monkeypatch):
        from multimodal_amd import device_data
        self.fused, self.matrix, self.found = [], [], []
        real_many, real_all, real_found = _native.nearest_many_device, _native.all_distances_device, device_data.DeviceEvaluation.found_labels

        def many(jobs, *a, **kw):
            jobs = list(jobs)
            self.fused.append(len(jobs))
            return real_many(jobs, *a, **kw)

        def all_distances_device(*a, **kw):
            self.matrix.append(1)
            return real_all(*a, **kw)

        def found_labels(ev, *a, **kw):
            self.found.append(1)
            return real_found(ev, *a, **kw)
        monkeypatch.setattr(_native, 'nearest_many_device', many)
        monkeypatch.setattr(_native, 'all_distances_device', all_distances_device)
        monkeypatch.setattr(device_data.DeviceEvaluation, 'found_labels', found_labels)

    def reset(self):
        del self.fused[:], self.matrix[:], self.found[:]


def same_results(a, b):
    assert list(a) == list(b)
    for key in a:
        if key == 'dictionary':
            assert np.array_equal(a[key], b[key])
        else:
            assert a[key] == b[key], key
            assert type(a[key]) is type(b[key]), key


def dataset_of(variant, kind):
    import scipy.sparse as sp
    from tests.test_batch_gpu import class_blocks
    data, labels = class_blocks(dims=(40, 60) if kind == 'two' else (40, 60, 30))
    kw = {}
    if variant == 'keep_sparse':
        data = [sp.csr_matrix(np.where(m > 0.15, m, 0.0)) for m in data]
        kw['keep_sparse'] = True
    elif variant == 'presence':
        absent = np.zeros(len(labels), dtype=bool)
        absent[np.random.default_rng(12).permutation(len(labels))[:len(labels) // 3]] = True
        kw['presence'] = [None, np.where(absent, 0.0, 1.0)] + [None] * (len(data) - 2)
    return data, labels, kw


@pytest.mark.parametrize('variant', ['dense', 'keep_sparse', 'presence'])
@pytest.mark.parametrize('kind', ['two', 'internal'])
def test_perform_one_run_fused_gives_the_default_route_s_results(monkeypatch, kind, variant):
    from multimodal_amd.device_data import DeviceDataset
    from multimodal_amd.device_experiment import perform_one_run
    monkeypatch.setenv('KLNMF_PRECISION', 'f64')
    monkeypatch.delenv('KLNMF_DEVICES', raising=False)
    data, labels, kw = dataset_of(variant, kind)
    mods = ['a', 'b', 'c'][:len(data)]
    ds = DeviceDataset(data, device=0, **kw)
    n, k = len(labels), 6
    examples = [labels.index(l) for l in sorted(set(labels))]
    rest = [i for i in range(n) if i not in examples]
    order = np.random.default_rng(2).permutation(len(rest))
    test, train = [rest[i] for i in order[:25]], [rest[i] for i in order[25:]]
    rng = np.random.default_rng(9)
    H0 = rng.random((k, sum(ds.dims))) + .01
    H0 /= H0.sum(axis=1, keepdims=True)
    args = (ds, mods, [1.0] * len(mods), k, 15, 15, train, test, examples, [labels[t] for t in test], [labels[e] for e in examples])
    calls = Calls(monkeypatch)
    _, default = perform_one_run(*args, init_dictionary=H0, kind=kind)
    assert calls.fused == [] and len(calls.found) == 48 and len(calls.matrix) == 48
    calls.reset()
    _, fused = perform_one_run(*args, init_dictionary=H0, kind=kind, search='fused')
    assert calls.fused == [12] and calls.found == [] and calls.matrix == []
    same_results(fused, default)
    assert sum(1 for key in fused if key.startswith('found_')) == 48
    with pytest.raises(ValueError):
        perform_one_run(*args, init_dictionary=H0, kind=kind, search='device')


def test_run_sweep_fused_gives_the_tables_of_the_default_route(monkeypatch):
    from multimodal_amd.device_experiment import run_sweep
    from tests.test_batch_gpu import class_blocks
    data, labels = class_blocks()
    args = dict(ks=[6, 8], n_runs=3, iter_train=20, iter_test=20, devices=[0], precision='f64', seed=3)
    calls = Calls(monkeypatch)
    table1, raw1 = run_sweep(data, labels, ['a', 'b'], **args)
    assert calls.fused == [] and len(calls.found) == 6 * 48
    calls.reset()
    table3, raw3 = run_sweep(data, labels, ['a', 'b'], batch=3, **args)
    assert calls.fused == [] and len(calls.found) == 6 * 48
    calls.reset()
    table3f, raw3f = run_sweep(data, labels, ['a', 'b'], batch=3, search='fused', **args)
    assert calls.fused == [36, 36] and calls.found == [] and calls.matrix == []      # one call per batch of three runs
    assert raw3f == raw3 == raw1 and table3f == table3 == table1
    calls.reset()
    table1f, raw1f = run_sweep(data, labels, ['a', 'b'], search='fused', **args)
    assert calls.fused == [12] * 6 and calls.found == [] and calls.matrix == []      # one call per run
    assert raw1f == raw1 and table1f == table1
    with pytest.raises(ValueError):
        run_sweep(data, labels, ['a', 'b'], search='both', **args)
