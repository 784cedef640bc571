"""The evaluation kernels against exact references (tests/eval_cases.py): k_all_distances through `_native.all_distances`,
`_native.all_distances_device` and the `metrics.*` wrappers, k_gkl through `Context.generalized_kl` and
`metrics.generalized_KL`, k_csrg_dense through `_native.csr_rows_to_dense_device`.

  * distances: the five measures in f64 and f32 on d in {0, 1, 63, 64, 65, 127, 128, 129, 1000} x (na, nb) in {(1,1), (1,3), (3,1),
    (5,3), (4,4), (7,9), (33,17)} (no, one, two, three and 16 trips of the 64-lane stride loop; 1 .. 561 pairs: partial last
    blocks, nb = 1), every pair within its bar of the extended-precision reference; what is exact asserted with ==
    (identical rows, a zero vector, d = 0); the reverse measure against the transposed forward one and the symmetric one
    against their mean.  The device form on sub-views at a nonzero offset of a larger tensor, row strides d + 3 and d + 5
    with NaN in the padding, a guarded output: bit-identical to the host-operand form.  The wrappers' row-paired form at 3
    and 1025 rows (the diagonals of two blocks) and the vector form.  Refusals, each followed by a valid call.
  * generalized_KL: counts {0, 1, 255, 256, 257, 262144, 262145, 600001} (one block, two, the grid cap of 1024 blocks, the
    grid-stride loop's second and third trip) x eps {1e-8, 1e-3, 0} in f64 and f32; the wrapper's axis None / 0 / 1, a
    broadcast pair, integers and a mixed pair.
  * CSR rows to dense: 50 x 70 with empty rows, a full row (two trips), single entries in column 0 and d - 1, f32 and f64 values;
    row lists (a permutation, repeats, one row, 65 rows, none), ld = d and d + 7 with NaN beyond column d and guard elements
    behind the last row: bit-identical to X[idx].toarray().  Both guards of k_csrg_dense stand before the loads they protect
    (`i` is tested before indptr[i] is read, `j` before data[p] is read and before the store), so a narrower d and a row index
    outside the source are cases here.

Bars are the derived ones of tests/eval_cases.py, nothing measured: distances (ceil(d / 64) + 16) 2^-53 M (+ 2^-24 |ref| for
the fp32 cast), generalized_KL (grid + ceil(count / (256 grid)) + 24) 2^-53 M.  The two relations between device results
(reverse against swapped forward, symmetric against the mean) hold within ONE such bar in f64; in f32 each value compared
was cast on its own, so 2^-24 of each of them stands in place of the single 2^-24 |ref|.
Measured on the MI355X, worst |error| / bar over every case (printed after each test, pytest -v): distances f64 0.20 (d = 128;
the wrappers 0.22), f32 0.99 (the final cast alone is up to 2^-24 |ref|, which is most of that bar); generalized_KL f64 0.013
(one element) and 0.005 at 600 001, f32 0.014; metrics.generalized_KL 0.028.  Nothing was widened.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from multimodal_amd import _native
from tests import eval_cases as evc
from tests.test_sparse_gpu import _MEASURED, _report_measured, check, worst_rel  # noqa: F401  (the autouse fixture prints what was measured)

pytestmark = pytest.mark.gpu

NP = {False: np.float64, True: np.float32}
SENTINEL = -12345.0


def torch_mod():
    import torch
    return torch


def report(group, worst):
    _MEASURED.append('    %-40s worst |error| / bar %.3f' % (group, worst))


def assert_within(what, got, ref, bar):
    ok, worst = evc.within(got, ref, bar)
    assert ok, '%s: %.3f of its bar' % (what, worst)
    return worst


# ---- distances ------------------------------------------------------------------------------------------------------------------
def device_distances(A, B, metric, f32):
    """klnmf_all_distances_device on sub-views of larger tensors: operands at element offsets 7 and 3, row strides d + 3 and
    d + 5, NaN wherever the kernel must not read, 8 guard elements behind the output."""
    torch = torch_mod()
    dt = torch.float32 if f32 else torch.float64
    na, d = A.shape
    nb = B.shape[0]
    lda, ldb = d + 3, d + 5

    def padded(M, ld, off):
        host = np.full(off + M.shape[0] * ld + 4, np.nan, dtype=NP[f32])
        view = host[off:off + M.shape[0] * ld].reshape(M.shape[0], ld)
        view[:, :d] = M
        big = torch.from_numpy(host).to('cuda')
        return big, big[off:]
    bigA, subA = padded(A, lda, 7)
    bigB, subB = padded(B, ldb, 3)
    out = torch.full((na * nb + 8,), SENTINEL, dtype=dt, device='cuda')
    torch.cuda.synchronize()
    assert subA.data_ptr() == bigA.data_ptr() + 7 * bigA.element_size()
    _native.all_distances_device(subA.data_ptr(), lda, subB.data_ptr(), ldb, out.data_ptr(), na, nb, d, metric, f64=not f32)
    got = out.cpu().numpy()
    assert np.all(got[na * nb:] == SENTINEL), 'the guard behind the output was written'
    return got[:na * nb].reshape(na, nb)


@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
@pytest.mark.parametrize('d', evc.DIMS)
def test_all_distances_within_the_derived_bars(d, f32):
    worst = 0.0
    for na, nb in evc.SHAPES:
        case = evc.pair_case(na, nb, d)
        A, B = case.A.astype(NP[f32]), case.B.astype(NP[f32])
        got = {}
        for metric, name in evc.METRICS:
            what = '%s %dx%d d=%d' % (name, na, nb, d)
            ref, M = evc.pair_reference(na, nb, d, metric, f32)
            D = _native.all_distances(A, B, metric)
            assert D.shape == (na, nb) and D.dtype == NP[f32]
            worst = max(worst, assert_within(what, D, ref, evc.distance_bar(d, M, ref, f32)))
            Dd = device_distances(A, B, metric, f32)
            assert not np.isnan(Dd).any(), what + ': the device form read its padding'
            assert np.array_equal(Dd.view(np.uint32 if f32 else np.uint64), D.view(np.uint32 if f32 else np.uint64)), \
                what + ': device operands and host operands differ'
            got[metric] = D
            # what is exact
            if d == 0:
                assert np.all(D == 0), what
                if metric == evc.COSINE_DIFF:
                    assert np.all(np.signbit(D)), what + ': -(0 / 1)'
            if metric != evc.COSINE_DIFF:
                for i, j in case.same:
                    assert D[i, j] == 0, what + ': identical rows'
            else:
                assert np.all(D[case.zero_a, :] == 0) and np.all(D[:, case.zero_b] == 0), what + ': a zero vector'
            if metric == evc.FROBENIUS:
                L = evc.ld()
                for i in case.zero_a:
                    norm = np.sqrt(np.square(np.asarray(B, dtype=L)).sum(axis=1))
                    assert_within(what + ': against a zero vector', D[i], norm, evc.distance_bar(d, norm, norm, f32))
        # the reverse measure is the forward one of the swapped operands, the symmetric one their mean: within ONE bar in f64;
        # in f32 every value compared carries a final cast of its own, 2^-24 of it each (module docstring)
        cast = (lambda *vals: 2.0 ** -24 * sum(np.abs(v.astype(np.float64)) for v in vals)) if f32 else (lambda *vals: 0.0)
        _, M = evc.pair_reference(na, nb, d, evc.REV_KL, f32)
        swapped = _native.all_distances(B, A, evc.KL).T
        assert_within('rev_kl_div(A, B) against kl_div(B, A) %dx%d d=%d' % (na, nb, d), got[evc.REV_KL],
                      swapped.astype(np.float64), evc.distance_bar(d, M) + cast(got[evc.REV_KL], swapped))
        _, M = evc.pair_reference(na, nb, d, evc.SYM_KL, f32)
        mean = 0.5 * (got[evc.KL].astype(np.float64) + got[evc.REV_KL].astype(np.float64))
        assert_within('sym_kl_div against the mean %dx%d d=%d' % (na, nb, d), got[evc.SYM_KL], mean,
                      evc.distance_bar(d, M) + cast(got[evc.SYM_KL]) + 0.5 * cast(got[evc.KL], got[evc.REV_KL]))
    report('distances %s d=%d' % ('f32' if f32 else 'f64', d), worst)


@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
def test_metrics_wrappers_row_paired_and_vector_forms(f32):
    from multimodal_amd.lib import metrics as Mx
    worst = 0.0
    d = 8
    for n in (3, 1025):                 # 1025: the diagonal of a 1024-row block and of a block of one row
        a, b = evc.paired_rows(n, d, seed=n)
        au, bu = a.astype(NP[f32]), b.astype(NP[f32])
        ar, br = (evc.as_f32(a), evc.as_f32(b)) if f32 else (a, b)
        for metric, name in evc.METRICS:
            ref, M = evc.measure(ar, br, metric)
            got = getattr(Mx, name)(au, bu)
            assert got.shape == (n,) and got.dtype == NP[f32]
            worst = max(worst, assert_within('%s, %d paired rows' % (name, n), got, ref, evc.distance_bar(d, M, ref, f32)))
            if metric != evc.COSINE_DIFF:
                assert got[2] == 0
            else:
                assert got[1] == 0
    a, b = evc.paired_rows(1, 129, seed=9)
    for metric, name in evc.METRICS:
        ar, br = (evc.as_f32(a[0]), evc.as_f32(b[0])) if f32 else (a[0], b[0])
        ref, M = evc.measure(ar, br, metric)
        got = getattr(Mx, name)(a[0].astype(NP[f32]), b[0].astype(NP[f32]))
        assert np.ndim(got) == 0
        worst = max(worst, assert_within('%s, vectors' % name, got, ref, evc.distance_bar(129, M, ref, f32)))
    report('metrics wrappers %s' % ('f32' if f32 else 'f64'), worst)


def test_all_distances_refusals_leave_the_process_usable():
    torch = torch_mod()
    lib = _native.load()
    case = evc.pair_case(5, 3, 65)
    A, B = case.A, case.B
    want = _native.all_distances(A, B, evc.KL)
    dA, dB = torch.from_numpy(A.copy()).to('cuda'), torch.from_numpy(B.copy()).to('cuda')
    out = torch.full((15 + 8,), SENTINEL, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    hout = np.full(15, SENTINEL)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    v = ctypes.c_void_p

    def host(dtype=_native.DT_F64, metric=evc.KL, na=5, nb=3, d=65, a=p(A), b=p(B), o=p(hout)):
        return lib.klnmf_all_distances(0, dtype, metric, na, nb, d, a, b, o)

    def dev(dtype=_native.DT_F64, metric=evc.KL, na=5, nb=3, d=65, a=dA.data_ptr(), lda=65, b=dB.data_ptr(), ldb=65, o=out.data_ptr()):
        return lib.klnmf_all_distances_device(0, dtype, metric, na, nb, d, v(a), lda, v(b), ldb, v(o))

    def still_right():
        assert np.array_equal(_native.all_distances(A, B, evc.KL), want)
        out.fill_(SENTINEL)
        torch.cuda.synchronize()
        _native.all_distances_device(dA.data_ptr(), 65, dB.data_ptr(), 65, out.data_ptr(), 5, 3, 65, evc.KL)
        got = out.cpu().numpy()
        assert np.array_equal(got[:15].reshape(5, 3), want) and np.all(got[15:] == SENTINEL)
        out.fill_(SENTINEL)
        torch.cuda.synchronize()

    refused = [lambda: host(metric=-1), lambda: host(metric=5), lambda: host(dtype=7), lambda: host(a=None), lambda: host(b=None),
               lambda: host(o=None), lambda: host(na=-1),
               lambda: dev(metric=-1), lambda: dev(metric=5), lambda: dev(dtype=7), lambda: dev(lda=64), lambda: dev(ldb=64),
               lambda: dev(a=None), lambda: dev(b=None), lambda: dev(o=None), lambda: dev(d=-1)]
    for n, call in enumerate(refused):
        status = call()
        assert status == _native.ERR_ARG, (n, status)
        with pytest.raises(_native.NativeError):
            _native._check(status)
        assert np.all(hout == SENTINEL) and np.all(out.cpu().numpy() == SENTINEL), n
        still_right()
    # no rows on either side: success, and nothing is touched
    for kw in ({'na': 0}, {'nb': 0}):
        assert host(**kw) == 0 and dev(**kw) == 0
        assert np.all(hout == SENTINEL) and np.all(out.cpu().numpy() == SENTINEL)
    with pytest.raises(_native.NativeError):
        _native.all_distances(A, B, 5)
    with pytest.raises(ValueError):
        _native.all_distances(A, B[:, :64], evc.KL)
    still_right()


# ---- generalized_KL -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
@pytest.mark.parametrize('count', evc.GKL_COUNTS)
def test_generalized_kl_within_the_derived_bar(count, f32):
    worst = 0.0
    with _native.Context('f64') as ctx:
        for eps in evc.GKL_EPS:
            x, y = evc.gkl_case(count, eps)
            ref, M = evc.gkl_reference(count, eps, f32)
            got = ctx.generalized_kl(x.astype(NP[f32]), y.astype(NP[f32]), eps)
            assert isinstance(got, float)
            if count == 0:
                assert got == 0.0 and not np.signbit(got)
            worst = max(worst, assert_within('generalized_KL of %d elements, eps %g' % (count, eps), got, ref, evc.gkl_bar(count, M)))
    report('generalized_KL %s count=%d' % ('f32' if f32 else 'f64', count), worst)


def test_metrics_generalized_kl_axes_broadcast_and_types():
    from multimodal_amd.lib import metrics as Mx
    rng = np.random.default_rng(3)
    x = (rng.random((37, 53)) + 0.05) * (rng.random((37, 53)) >= 0.3)
    y = rng.random((37, 53)) + 0.05
    worst = 0.0

    def one(what, xs, ys, xr, yr, axis, eps=1e-8):
        ref, M = evc.generalized_kl(xr, yr, eps, axis=axis)
        got = Mx.generalized_KL(xs, ys, eps=eps, axis=axis)
        assert np.shape(got) == np.shape(ref), what
        count = np.broadcast(xr, yr).size if axis is None else np.broadcast(xr, yr).shape[axis]
        return assert_within(what, got, ref, evc.gkl_bar(count, M))
    for axis in (None, 0, 1):
        worst = max(worst, one('axis %s' % axis, x, y, x, y, axis))
        worst = max(worst, one('axis %s, eps 1e-3' % axis, x, y, x, y, axis, eps=1e-3))
    col, row = x[:, :1], y[:1, :]
    for axis in (None, 0, 1):
        worst = max(worst, one('[n,1] x [1,m], axis %s' % axis, col, row, *np.broadcast_arrays(col, row), axis=axis))
    xi = rng.integers(0, 5, (37, 53))
    yi = rng.integers(1, 6, (37, 53))
    worst = max(worst, one('integers', xi, yi, xi.astype(np.float64), yi.astype(np.float64), None))
    worst = max(worst, one('integers against floats', xi, y, xi.astype(np.float64), y, 1))
    x32 = x.astype(np.float32)
    worst = max(worst, one('float32 x against float64 y', x32, y, x32.astype(np.float64), y, None))
    worst = max(worst, one('float64 x against float32 y', x, y.astype(np.float32), x, evc.as_f32(y), 0))
    worst = max(worst, one('float32 pair', x32, y.astype(np.float32), evc.as_f32(x), evc.as_f32(y), 1))
    report('metrics.generalized_KL', worst)


# ---- CSR rows to dense ----------------------------------------------------------------------------------------------------------
CSR_ROWS, CSR_D = 50, 70


def csr_source(dtype):
    rng = np.random.default_rng(21)
    X = (rng.random((CSR_ROWS, CSR_D)) + 0.05) * (rng.random((CSR_ROWS, CSR_D)) < 0.25)
    X[[0, 7, 49], :] = 0.0                                   # empty rows, the first and the last among them
    X[3, :] = rng.random(CSR_D) + 0.05                       # a full row: 70 entries, two trips of 64
    X[5, :] = 0.0
    X[5, 0] = 1.25                                           # only column 0
    X[6, :] = 0.0
    X[6, CSR_D - 1] = 2.5                                    # only column d - 1
    X = sp.csr_matrix(X.astype(dtype))
    X.sort_indices()
    lengths = np.diff(X.indptr)
    assert (lengths == 0).sum() == 3 and lengths[3] == CSR_D > 64 and lengths[5] == lengths[6] == 1
    assert X.indices[X.indptr[5]] == 0 and X.indices[X.indptr[6]] == CSR_D - 1
    return X


ROW_LISTS = {
    'a permutation': np.random.default_rng(4).permutation(CSR_ROWS),
    'repeats': np.array([3, 3, 0, 5, 3, 6, 49, 5, 6, 6, 12]),
    'one row': np.array([3]),
    '65 rows': np.concatenate([np.arange(CSR_ROWS), np.arange(15)[::-1]]),
    'no rows': np.zeros(0, dtype=np.int64),
}


def to_dense(X, idx, d, ld, src_rows=None, with_entries=True, guard=8):
    """klnmf_csr_rows_to_dense_device into a NaN-filled [rows, ld] device matrix with `guard` elements behind it -> (the
    [rows, ld] matrix, the guard), on the host."""
    torch = torch_mod()
    idx = np.asarray(idx, dtype=np.int64)
    rows = idx.size
    indptr = torch.from_numpy(X.indptr.astype(np.int64)).to('cuda')
    indices = torch.from_numpy(X.indices.astype(np.int32)).to('cuda')
    data = torch.from_numpy(np.ascontiguousarray(X.data)).to('cuda')
    didx = torch.from_numpy(np.concatenate([idx, [0]])).to('cuda')        # (never an empty allocation)
    out = torch.full((rows * ld + guard,), float('nan'), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    _native.csr_rows_to_dense_device(indptr.data_ptr(), indices.data_ptr() if with_entries else 0, data.data_ptr() if with_entries else 0,
                                     X.dtype == np.float64, X.shape[0] if src_rows is None else src_rows, didx.data_ptr(), rows, d,
                                     out.data_ptr(), ld)
    got = out.cpu().numpy()
    return got[:rows * ld].reshape(rows, ld), got[rows * ld:]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('rows', sorted(ROW_LISTS))
def test_csr_rows_to_dense_is_the_dense_rows_bit_for_bit(rows, dtype):
    X = csr_source(dtype)
    idx = ROW_LISTS[rows]
    want = X[idx].toarray().astype(np.float64) if idx.size else np.zeros((0, CSR_D))
    for ld in (CSR_D, CSR_D + 7):
        got, guard = to_dense(X, idx, CSR_D, ld)
        assert same_bits(got[:, :CSR_D], want), '%s, ld %d' % (rows, ld)
        assert np.isnan(got[:, CSR_D:]).all() and np.isnan(guard).all(), '%s, ld %d: written beyond column d' % (rows, ld)


def test_csr_rows_to_dense_documented_edges_and_refusals():
    X = csr_source(np.float32)
    idx = ROW_LISTS['repeats']
    # a matrix without stored entries may come without index and value arrays: zeros
    E = sp.csr_matrix((CSR_ROWS, CSR_D), dtype=np.float32)
    got, guard = to_dense(E, idx, CSR_D, CSR_D + 7, with_entries=False)
    assert np.all(got[:, :CSR_D] == 0) and not np.signbit(got[:, :CSR_D]).any() and np.isnan(got[:, CSR_D:]).all() and np.isnan(guard).all()
    # a d narrower than the source drops the columns beyond it (the column is tested before the value is read and stored)
    for d in (1, 33, 69):
        got, guard = to_dense(X, idx, d, d + 7)
        assert same_bits(got[:, :d], X[idx].toarray()[:, :d]) and np.isnan(got[:, d:]).all() and np.isnan(guard).all(), d
    # a row index outside [0, src_rows) is a zero row (tested before the row pointers are read): here rows 40 .. 49 of the
    # source are declared away, and -1 is outside every source
    odd = np.array([3, 40, -1, 49, 39, 1 << 40])
    got, guard = to_dense(X, odd, CSR_D, CSR_D + 7, src_rows=40)
    want = np.zeros((odd.size, CSR_D))
    want[0], want[4] = X[3].toarray()[0], X[39].toarray()[0]
    assert same_bits(got[:, :CSR_D], want) and np.isnan(got[:, CSR_D:]).all() and np.isnan(guard).all()
    # refusals on the host, before any launch
    torch = torch_mod()
    lib = _native.load()
    indptr = torch.from_numpy(X.indptr.astype(np.int64)).to('cuda')
    indices = torch.from_numpy(X.indices.astype(np.int32)).to('cuda')
    data = torch.from_numpy(X.data).to('cuda')
    didx = torch.from_numpy(idx.astype(np.int64)).to('cuda')
    out = torch.full((idx.size * CSR_D + 8,), float('nan'), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    v = ctypes.c_void_p

    def call(dtype=_native.DT_F32, ip=indptr.data_ptr(), ix=didx.data_ptr(), o=out.data_ptr(), rows=idx.size, d=CSR_D, ld=CSR_D):
        return lib.klnmf_csr_rows_to_dense_device(0, dtype, v(ip), v(indices.data_ptr()), v(data.data_ptr()), CSR_ROWS, v(ix), rows, d, v(o), ld)
    for kw in ({'ld': CSR_D - 1}, {'ip': None}, {'ix': None}, {'o': None}, {'dtype': 7}, {'rows': -1}, {'d': -1}):
        assert call(**kw) == _native.ERR_ARG, kw
        assert np.isnan(out.cpu().numpy()).all(), kw
    assert call(rows=0) == 0 and call(d=0) == 0 and np.isnan(out.cpu().numpy()).all()       # nothing to do: nothing touched
    assert call() == 0
    got = out.cpu().numpy()
    assert same_bits(got[:-8].reshape(idx.size, CSR_D), X[idx].toarray()) and np.isnan(got[-8:]).all()
