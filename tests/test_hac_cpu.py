"""The windowed co-occurrence histograms without a GPU: the exports of include/klnmf_hac.h; the host twin
(multimodal_amd/features/hac.py) against the REFERENCE's recorded outputs (tests/golden/g21_hac.npz: scipy's vq labels, every
window's `compute_coocurrences` row, `slider`) as exact integers; the route rule at its edges; and the routing of `windowed_hac`,
of `MultimodalLearner.reconstruct_internal` on a `DeviceCsrRows` and of `evaluation.sliding_distances`, with recording stand-ins
for the native calls that answer from the host twin on CPU tensors.  Every host refusal raises before any native call."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from multimodal_amd import _native, evaluation
from multimodal_amd.features import hac
from multimodal_amd.learner import MultimodalLearner
from tests import hac_cases as hc
from tests.test_batch_csr_cpu import check_header_tables, declared_in, other_headers

NEW = {'klnmf_hac_work_bytes', 'klnmf_hac_count_device', 'klnmf_hac_fill_device', 'klnmf_hac'}
OTHERS = other_headers('klnmf_hac.h')


# ---- the bindings -------------------------------------------------------------------------------------------------------------------
def test_every_declared_hac_symbol_is_bound_and_exported():
    declared = declared_in('klnmf_hac.h')
    assert declared == NEW == set(_native.HAC_SIGNATURES)
    lib = _native.load()
    for name in declared:
        assert hasattr(lib, name), name
    for header in OTHERS:
        assert not (declared & declared_in(header)), header
    for name in ('hac_work_bytes', 'hac_count_device', 'hac_fill_device', 'hac', 'hac_route'):
        assert callable(getattr(_native, name))
    assert ctypes.sizeof(_native.HacStream) == 48                  # klnmf_hac_stream: two pointers and four int64


def test_the_other_headers_declare_what_they_declared():
    check_header_tables()                # (and NEW is this header's own table: the test above)


def test_every_entry_point_names_the_reference_lines_it_replaces():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'klnmf_hac.h')).read()
    for name in NEW:
        comment = header[:header.index('int %s(' % name)].rsplit('/*', 1)[1]
        assert 'features/hac.py' in comment or 'image_sound_eval_sliding.py' in comment, name


def test_the_workspace_size_is_host_arithmetic():
    base = _native.hac_work_bytes(3, 400, 2, 40)
    assert _native.hac_work_bytes(3, 400 + 4, 2, 40) == base + 3 * 4 * 4            # the codes: int32 per stream and frame
    assert _native.hac_work_bytes(3, 400, 2, 40 + 2) == base + 2 * 2 * 4 + 12 * 4 + 12 * 8   # windows, counts, offsets
    assert _native.hac_work_bytes(1, 0, 1, 0) > 0
    for bad in ((0, 10, 1, 1), (9, 10, 1, 1), (1, 10, 0, 1), (1, 10, 9, 1), (1, -1, 1, 1), (1, 10, 1, -1), (1, 1 << 31, 1, 1),
                (8, 10, 8, 1 << 26)):
        with pytest.raises(_native.NativeError):
            _native.hac_work_bytes(*bad)


def test_the_route_rule_at_its_edges():
    r = _native.hac_route
    assert r(0, 150) == r(-3, 150) == 'none'
    assert r(1, 150) == r(4096, 150) == r(4096, 10 ** 4) == 'sort'
    assert r(4097, 1) == r(4097, 192) == r(10 ** 9, 192) == 'dense'
    assert r(4097, 193) == r(10 ** 9, 193) == 'refused'
    assert 192 * 192 * 4 == 144 * 1024                                             # the dense route's counters: 144 KiB of LDS
    assert (_native.HAC_SORT_MAX, _native.HAC_DENSE_MAX_K, _native.HAC_MAX_STREAMS, _native.HAC_MAX_LAGS) == (4096, 192, 8, 8)


# ---- the host twin against the reference's recorded outputs ---------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['a', 'b'])
def test_the_host_twin_gives_the_reference_s_labels_and_rows(tag):
    g = hc.golden()[tag]
    for x, c, labels in zip(g['streams'], g['codebooks'], g['labels']):
        got = hac.quantize(x, c)
        assert got.dtype == np.int32 and np.array_equal(got, labels)
        assert np.array_equal(hac.quantize(x.astype(np.float32), c.astype(np.float32)), labels)       # (the frames are exact in f32)
    want = g['csr']
    got = hc.twin(g['streams'], g['codebooks'], g['windows'], g['lags'])
    assert hc.same_csr(got, sp.csr_matrix(want, dtype=np.float64), np.float64)
    assert want.data.max() > 1 and (tag == 'b' or (np.diff(want.indptr) == 0).any())      # counts above 1; set a: empty rows
    for w in (0, 5, 20, len(g['windows']) - 1):                                    # the reference's names, dense vectors
        t0, t1 = g['windows'][w]
        if t1 > t0:
            row = hac.hac_from_streams([x[t0:t1] for x in g['streams']], g['codebooks'], g['lags'])
            assert row.dtype.kind == 'i' and np.array_equal(row, want[w].toarray().ravel())
    x, c = g['streams'][0], g['codebooks'][0]
    one = hac.compute_coocurrences(x, c, g['lags'])
    assert np.array_equal(one, np.hstack([hac.coocurrences(g['labels'][0], c.shape[0], l) for l in g['lags']]))
    assert np.array_equal(hac.coocurrences(np.array([1, 0, 1]), 2, 1), [0, 1, 1, 0])      # (0 then 1) -> 1 * 2 + 0; (1 then 0) -> 1
    assert np.array_equal(hac.coocurrences(np.array([1, 0]), 2, 2), [0, 0, 0, 0]) and hac.coocurrences(np.array([], dtype=int), 3, 1).sum() == 0


def test_quantize_breaks_ties_low_and_never_picks_a_nan():
    assert list(hac.quantize([[0.5], [0.0], [1.0]], [[0.0], [1.0]])) == [0, 0, 1]
    assert list(hac.quantize([[0.0, 0.0]], [[np.nan, 0.0], [3.0, 4.0], [3.0, 4.0]])) == [1]
    assert list(hac.quantize([[np.nan]], [[0.0], [1.0]])) == [0]
    # a distance that ties in float32 and does not in float64: 1 + 2^-26 against 1
    x = np.zeros((1, 2), dtype=np.float32)
    c = np.array([[1.0, 2.0 ** -13], [1.0, 0.0]], dtype=np.float32)
    assert np.float32(1.0) + np.float32(2.0 ** -26) == np.float32(1.0) and list(hac.quantize(x, c)) == [1]


def test_frame_windows_are_the_reference_s_slider_at_integer_arguments():
    records = hc.golden()['slider']
    assert len(records) >= 12
    for (n, width, shift, partial), want in records:
        got = hac.frame_windows(n, width, shift, partial=bool(partial))
        assert all(isinstance(v, int) for pair in got for v in pair)
        assert np.array_equal(np.asarray(got, dtype=np.float64).reshape(-1, 2), want), (n, width, shift, partial)
    assert hac.frame_windows(1003, 50, 10) == hc.golden()['b']['windows']
    for bad in ((-1, 5, 1), (10, 0, 1), (10, 5, 0)):
        with pytest.raises(ValueError):
            hac.frame_windows(*bad)


# ---- the routing, with recording stand-ins --------------------------------------------------------------------------------------------
def host_matrix(ptr, rows, ld, d, dt):
    if rows == 0 or d == 0 or not ptr:
        return np.zeros((rows, d), dtype=dt)
    item = np.dtype(dt).itemsize
    ctype = ctypes.c_double if item == 8 else ctypes.c_float
    flat = np.ctypeslib.as_array((ctype * ((rows - 1) * ld + d)).from_address(ptr))
    return np.lib.stride_tricks.as_strided(flat, shape=(rows, d), strides=(item * ld, item)).copy()


class HacRecorder(object):
    """Stand-ins for the two device calls: they answer from the host twin and record what they were asked."""

    def __init__(self, monkeypatch):
        self.counts, self.fills, self.pending = [], [], None
        monkeypatch.setattr(_native, 'hac_count_device', self.count)
        monkeypatch.setattr(_native, 'hac_fill_device', self.fill)
        monkeypatch.setattr(_native, 'hac', self.never)

    def never(self, *a, **k):
        raise AssertionError('the host-array entry is not the device path')

    def count(self, streams, T, lags, windows, d_work, work_bytes, d_indptr, f64=True, device=0):
        dt = np.float64 if f64 else np.float32
        streams = list(streams)
        mats = [(host_matrix(dx, T, ld, d, dt), host_matrix(dc, K, ldc, d, dt)) for dx, ld, dc, ldc, d, K in streams]
        windows = [tuple(int(v) for v in w) for w in np.asarray(windows).reshape(-1, 2)]
        assert work_bytes == _native.hac_work_bytes(len(streams), T, len(lags), len(windows)) and d_work
        X = hc.twin([m[0] for m in mats], [m[1] for m in mats], windows, list(lags))
        np.ctypeslib.as_array((ctypes.c_int64 * (len(windows) + 1)).from_address(d_indptr))[:] = X.indptr
        self.pending = (X, d_work)
        self.counts.append(dict(T=T, lags=list(lags), windows=windows, f64=f64, Ks=[s[5] for s in streams], ds=[s[4] for s in streams]))
        return int(X.nnz)

    def fill(self, Ks, T, lags, windows, d_work, work_bytes, nnz, d_indices, d_values, f64=True, device=0):
        X, work = self.pending
        last = self.counts[-1]
        assert work == d_work and nnz == X.nnz and list(Ks) == last['Ks'] and T == last['T'] and list(lags) == last['lags']
        assert [tuple(int(v) for v in w) for w in np.asarray(windows).reshape(-1, 2)] == last['windows']
        if nnz:
            np.ctypeslib.as_array((ctypes.c_int32 * nnz).from_address(d_indices))[:] = X.indices
            ctype = ctypes.c_double if f64 else ctypes.c_float
            np.ctypeslib.as_array((ctype * nnz).from_address(d_values))[:] = X.data
        self.fills.append(dict(nnz=nnz, f64=f64))


class ContextRecorder(object):
    """Stands in for `_native.Context`: records every call `_fit_uploaded` makes on it."""
    calls = []

    def __init__(self, precision='f64', device=0, stream=None, pooled=False):
        self.precision = _native.PRECISIONS[precision]
        self.precision_name = precision

    def __enter__(self):
        return self

    def __exit__(self, *a):
        pass

    def __getattr__(self, name):
        def method(*args, **kwargs):
            ContextRecorder.calls.append((name, args, kwargs))
            if name == 'set_problem_sparse_shape':
                self.n, self.f, self.k = args[0], args[1], args[2]
            if name == 'set_problem_sparse':
                (self.n, self.f), self.k = args[0].shape, args[1]
            if name == 'run':
                return [], 0, False
            if name == 'fp8_report':
                return {}
            if name == 'get_W':
                return np.full((self.n, self.k), 0.25)
        return method


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
def test_windowed_hac_makes_one_count_and_one_fill_call(monkeypatch, dtype):
    rec = HacRecorder(monkeypatch)
    g = hc.golden()['a']
    want = sp.csr_matrix(g['csr'], dtype=dtype)
    got = hac.windowed_hac(g['streams'], g['codebooks'], g['windows'], lags=g['lags'], dtype=dtype, device='cpu')
    assert hc.same_csr(got, want, dtype)
    assert len(rec.counts) == 1 and len(rec.fills) == 1
    assert rec.counts[0]['f64'] and rec.counts[0]['Ks'] == [7, 12, 3] and rec.counts[0]['ds'] == [13, 13, 5] and rec.counts[0]['T'] == 401
    assert rec.fills[0] == dict(nnz=want.nnz, f64=dtype == np.float64)
    rows = hac.windowed_hac([x.astype(np.float32) for x in g['streams']], [c.astype(np.float32) for c in g['codebooks']], g['windows'],
                            lags=g['lags'], dtype=dtype, device='cpu', output='device')
    assert not rec.counts[1]['f64']                                                # float32 streams stay float32
    assert isinstance(rows, hac.DeviceCsrRows) and rows.shape == want.shape and rows.nnz == want.nnz
    assert rows.f64 == (dtype == np.float64) and rows.least == 1 and type(rows.least) is np.dtype(dtype).type
    assert np.array_equal(rows.indptr, want.indptr) and rows.indptr.dtype == np.int64
    ptrs = rows.pointers()
    assert ptrs == (rows.d_indptr.data_ptr(), rows.d_indices.data_ptr(), rows.d_data.data_ptr(), dtype == np.float64)
    assert hc.same_csr(rows.to_scipy(), want, dtype)
    import torch
    as_tensors = hac.windowed_hac([torch.from_numpy(x) for x in g['streams']], [torch.from_numpy(c) for c in g['codebooks']],
                                  g['windows'], lags=g['lags'], dtype=dtype, device='cpu')
    assert hc.same_csr(as_tensors, want, dtype) and len(rec.counts) == 3
    # no window: a matrix of no row and every column
    empty = hac.windowed_hac(g['streams'], g['codebooks'], [], lags=g['lags'], dtype=dtype, device='cpu')
    assert empty.shape == (0, want.shape[1]) and empty.nnz == 0


def learner_of(f, k=4, coef=0.5):
    learner = MultimodalLearner(['sound', 'objects'], [f, 6], [coef, 1.0], k)
    learner.dico = np.full((k, f + 6), 1.0 / (f + 6))
    return learner


def test_reconstruct_internal_gathers_a_device_csr_on_the_device(monkeypatch):
    rec = HacRecorder(monkeypatch)
    g = hc.golden()['a']
    rows = hac.windowed_hac(g['streams'], g['codebooks'], g['windows'], lags=g['lags'], device='cpu', output='device')
    n, f = rows.shape
    ContextRecorder.calls = []
    monkeypatch.setattr(_native, 'Context', ContextRecorder)
    learner = learner_of(f)
    W = learner.reconstruct_internal('sound', rows, 7)
    assert W.shape == (n, 4)
    names = [c[0] for c in ContextRecorder.calls]
    assert names[:2] == ['set_problem_sparse_shape', 'upload_csr_device_rows'] and 'set_problem_sparse' not in names
    assert tuple(ContextRecorder.calls[0][1]) == (n, f, 4, 7, rows.nnz)
    sources, bounds, scales, src_rows, idx_ptr, n_rows = ContextRecorder.calls[1][1]
    assert list(sources) == [rows.pointers()] and list(bounds) == [0, f] and list(scales) == [0.5] and src_rows == n_rows == n
    assert isinstance(idx_ptr, int) and idx_ptr
    set_H = [c for c in ContextRecorder.calls if c[0] == 'set_H']
    assert set_H and set_H[0][1][0].shape == (4, f)                                # the modality's slice of the dictionary
    run = [c for c in ContextRecorder.calls if c[0] == 'run'][0]
    assert run[1][0] == 7 and run[1][1] is False and run[1][2] == 0                # a transform of 7 updates, tol 0
    # a coefficient of 0: `csr_rows_plan` sends the call to the host path, on the downloaded matrix
    ContextRecorder.calls = []
    learner_of(f, coef=0.0).reconstruct_internal('sound', rows, 7)
    first = ContextRecorder.calls[0]
    assert first[0] == 'set_problem_sparse' and first[1][0].shape == (n, f)
    # every other input type takes the path it took: a scipy matrix is the host upload
    ContextRecorder.calls = []
    learner.reconstruct_internal('sound', rows.to_scipy(), 7)
    assert ContextRecorder.calls[0][0] == 'set_problem_sparse'


def test_sliding_distances_is_windows_then_transform_then_distances(monkeypatch):
    rec = HacRecorder(monkeypatch)
    g = hc.golden()['a']
    f = g['csr'].shape[1]
    ContextRecorder.calls = []
    monkeypatch.setattr(_native, 'Context', ContextRecorder)
    seen = []

    def all_distances(A, B, metric, device=0):
        seen.append((A.shape, B.shape, metric, len(rec.fills), len(ContextRecorder.calls)))
        return np.zeros((A.shape[0], B.shape[0]))
    monkeypatch.setattr(_native, 'all_distances', all_distances)
    examples = np.random.default_rng(3).random((5, 4))
    D = evaluation.sliding_distances(learner_of(f), 'sound', g['streams'], g['codebooks'], g['windows'], examples, 9, lags=g['lags'],
                                     device='cpu')
    n = len(g['windows'])
    assert D.shape == (n, 5)
    assert len(rec.counts) == 1 and len(rec.fills) == 1 and rec.fills[0]['f64']
    assert [c[0] for c in ContextRecorder.calls][:2] == ['set_problem_sparse_shape', 'upload_csr_device_rows']
    assert len(seen) == 1 and seen[0][:3] == ((n, 4), (5, 4), _native.DIST_COSINE_DIFF)
    assert seen[0][3] == 1 and seen[0][4] == len(ContextRecorder.calls)            # the distances come last
    with pytest.raises(ValueError):
        evaluation.sliding_distances(learner_of(f), 'sound', g['streams'], g['codebooks'], g['windows'], examples, 9, metric='manhattan')
    with pytest.raises(ValueError):
        evaluation.sliding_distances(learner_of(f), 'sound', g['streams'], g['codebooks'], g['windows'], examples[:, :3], 9)
    assert len(rec.counts) == 1


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_every_host_refusal_raises_before_any_native_call(monkeypatch):
    rec = HacRecorder(monkeypatch)
    calls = []
    monkeypatch.setattr(_native, 'hac_work_bytes', lambda *a: calls.append(a) or 1 << 20)
    x, c = np.random.default_rng(0).random((30, 4)), np.random.default_rng(1).random((5, 4))
    ok = dict(streams=[x], codebooks=[c], windows=[(0, 30)], lags=[5, 2])

    def refused(**change):
        args = dict(ok, **change)
        with pytest.raises(ValueError):
            hac.windowed_hac(args['streams'], args['codebooks'], args['windows'], lags=args['lags'], device='cpu',
                             **{k: v for k, v in args.items() if k in ('dtype', 'output')})

    for bad in (np.nan, np.inf, -np.inf):
        xb = x.copy()
        xb[7, 2] = bad
        refused(streams=[xb])
        cb = c.copy()
        cb[0, 0] = bad
        refused(codebooks=[cb])
    refused(codebooks=[c[:, :3]])                                                  # d of the codebook
    refused(streams=[x, x[:29]], codebooks=[c, c])                                 # T of the second stream
    refused(streams=[x, x], codebooks=[c])                                         # a codebook per stream
    refused(streams=[x.ravel()])
    refused(codebooks=[c[:0]])                                                     # K = 0
    for w in ([(0, 31)], [(-1, 4)], [(5, 4)], [(0, 30, 1)], [(0.5, 4)]):
        refused(windows=w)
    for lags in ([0], [5, 0], [-1], [], [1] * 9, [1.5]):
        refused(lags=lags)
    refused(streams=[x] * 9, codebooks=[c] * 9)
    big = np.arange(32768, dtype=np.float64).reshape(-1, 1)                        # 2 lags x 32768^2 = 2^31 columns
    refused(streams=[x[:, :1]], codebooks=[big])
    refused(dtype=np.int32)
    refused(output='dense')
    assert rec.counts == [] and rec.fills == [] and calls == []
