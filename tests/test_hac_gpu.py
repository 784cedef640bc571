"""The windowed co-occurrence histograms on the device (include/klnmf_hac.h, csrc/hac.hip.h) against the host twin.

Every comparison is exact equality of the row pointers, the column indices and the values with
`features.hac.host_windowed_hac` (tests/hac_cases.py; pinned to the reference's recorded outputs by tests/test_hac_cpu.py): the
work is integer work, nothing here has a tolerance -- but for `sliding_distances`, whose last step is k_all_distances and keeps
that kernel's bar (tests/eval_cases.py, distance_bar).  The shapes are the smallest at which each mechanism can go wrong: the
staging choices of the quantisation (d = 1 ... 65, codebooks of 1 unit), the sort route at 63 ... 4096 codes (its padding, one
and many waves), the dense route at 4097 and 9000 codes, window lengths around a lag, counts beyond 2^16."""
import numpy as np
import pytest
import scipy.sparse as sp

from multimodal_amd import _native, evaluation
from multimodal_amd.features import hac
from multimodal_amd.learner import MultimodalLearner
from multimodal_amd.lib.nmf import KLdivNMF
from tests import eval_cases as evc
from tests import hac_cases as hc

pytestmark = pytest.mark.gpu


def check(streams, codebooks, windows, lags, dtype=np.float64):
    """windowed_hac IS the host twin on these arguments; returns the matrix."""
    got = hac.windowed_hac(streams, codebooks, windows, lags=lags, dtype=dtype)
    want = hc.twin(streams, codebooks, windows, lags, dtype=dtype)
    assert hc.same_csr(got, want, dtype)
    return got


def on_device(a):
    import torch
    return torch.from_numpy(np.array(a, order='C')).to('cuda')


# ---- the recorded cases -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['a', 'b'])
@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
@pytest.mark.parametrize('tensors', [False, True], ids=['host', 'device'])
def test_the_recorded_cases_are_the_reference_s_rows(tag, f32, tensors):
    g = hc.golden()[tag]
    dt = np.float32 if f32 else np.float64
    streams, codebooks = [x.astype(dt) for x in g['streams']], [c.astype(dt) for c in g['codebooks']]     # (exact in float32)
    if tensors:
        streams, codebooks = [on_device(x) for x in streams], [on_device(c) for c in codebooks]
    got = hac.windowed_hac(streams, codebooks, g['windows'], lags=g['lags'], dtype=dt)
    assert hc.same_csr(got, sp.csr_matrix(g['csr'], dtype=dt), dt)
    if tag == 'a' and not tensors:                                                 # the host-array entry of the C-ABI
        indptr, indices, values = _native.hac(streams, codebooks, g['lags'], g['windows'], dtype=dt)
        assert hc.same_csr(sp.csr_matrix((values, indices, indptr), shape=got.shape), got, dt)


# ---- quantisation -----------------------------------------------------------------------------------------------------------------
def labels_on_device(x, c, dt=None):
    """The device's label of every frame, read back through windows of two frames at lag 1 (one entry: q[t + 1] * K + q[t])."""
    x, c = np.asarray(x), np.asarray(c)
    if dt is not None:
        x, c = x.astype(dt), c.astype(dt)
    T, K = x.shape[0], c.shape[0]
    x2 = np.vstack([x, x[-1:]])
    got = hac.windowed_hac([x2], [c], [(t, t + 2) for t in range(T)], lags=[1])
    assert np.array_equal(np.diff(got.indptr), np.ones(T)) and np.array_equal(got.data, np.ones(T))
    q = got.indices % K
    assert np.array_equal(got.indices // K, np.append(q[1:], q[-1]))
    return q


@pytest.mark.parametrize('d', [1, 13, 33, 65])
@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
def test_labels_at_every_staging_choice(d, f32):
    rng = np.random.default_rng(d)
    dt = np.float32 if f32 else np.float64
    for K, T in ((1, 5), (2, 300), (9, 257), (150 if d <= 13 else 700, 70)):      # (700 x 33 and 700 x 65: codebooks beyond the LDS budget)
        c = rng.normal(size=(K, d)).astype(dt)
        x = (c[rng.integers(0, K, T)] + 0.3 * rng.normal(size=(T, d))).astype(dt)
        x[T // 2] = c[K - 1]                                                       # a frame equal to a codebook row
        want = hac.quantize(x, c)
        assert want[T // 2] == K - 1 or np.array_equal(c[want[T // 2]], c[K - 1])
        assert np.array_equal(labels_on_device(x, c), want), (K, T)


def test_ties_go_to_the_lowest_index_and_f32_inputs_are_compared_in_f64():
    mid = np.array([[0.5], [0.0], [1.0], [0.5]])
    assert list(labels_on_device(mid, [[0.0], [1.0]])) == [0, 0, 1, 0]            # exactly midway: index 0
    assert list(labels_on_device(mid, [[1.0], [0.0]])) == [0, 1, 0, 0]
    assert list(labels_on_device(mid, [[0.25], [0.25], [0.25]])) == [0, 0, 0, 0]
    # 1 + 2^-26 against 1: a tie in float32 arithmetic (index 0), not in float64 (index 1)
    x = np.zeros((3, 2), dtype=np.float32)
    c = np.array([[1.0, 2.0 ** -13], [1.0, 0.0]], dtype=np.float32)
    assert list(hac.quantize(x, c)) == [1, 1, 1] and list(labels_on_device(x, c)) == [1, 1, 1]


def fused_distance(row):
    """The squared distance of the origin to `row` as a loop of fused multiply-adds forms it: acc = fl(v * v + acc), exact
    arithmetic rounded once per step."""
    from fractions import Fraction
    acc = 0.0
    for v in row:
        acc = float(Fraction(float(v)) * Fraction(float(v)) + Fraction(acc))
    return acc


def test_labels_where_fused_and_unfused_distances_disagree():
    """Frames at the origin against the codebook [[a, b], [b, a]], fp64.  Rounded on their own, the two distances are the same two
    products added in either order: an exact tie, label 0.  A fused loop forms fl(fl(a^2) + b^2) against fl(fl(b^2) + a^2), which
    differ for many (a, b); the pairs kept here are those for which it would pick label 1 (asserted, so that the inputs cannot
    stop being adversarial).  The histogram builder, the codebook builder and the host twin must all say 0.  float32 inputs cannot
    show the difference with frames at the origin -- products of 24-bit values are exact in fp64 -- so the f32 instantiation
    rests on its device code holding no fused fp64 multiply-add (profiles/feature_units_refactor_ab.txt)."""
    rng = np.random.default_rng(0)
    pairs = []
    for _ in range(2000):
        a, b = rng.uniform(1, 2, 2)
        if fused_distance((b, a)) < fused_distance((a, b)):
            pairs.append((a, b))
        if len(pairs) == 8:
            break
    assert len(pairs) == 8
    x = np.zeros((3, 2))
    for a, b in pairs:
        c = np.array([[a, b], [b, a]])
        assert a * a + b * b == b * b + a * a and fused_distance(c[1]) < fused_distance(c[0])
        assert list(hac.quantize(x, c)) == [0, 0, 0]
        assert list(labels_on_device(x, c)) == [0, 0, 0], (a, b)
        assert list(_native.kmeans(x, c, n_iter=0)[1]) == [0, 0, 0], (a, b)


def test_a_single_frame_and_no_frame():
    x, c = hc.coded([2], 4)
    got = check([x], [c], [(0, 1), (0, 0), (1, 1)], [1])
    assert got.nnz == 0 and got.shape == (3, 16)
    none = check([x[:0]], [c], [(0, 0), (0, 0)], [5, 2])
    assert none.shape == (2, 32) and none.nnz == 0


# ---- windows against a lag, segments on both routes -----------------------------------------------------------------------------------
def test_window_lengths_around_the_lag():
    x, c = hc.coded(hc.random_codes(1, 40, 5), 5)
    windows = [(t0, t0 + n) for n in (0, 1, 5, 6, 7) for t0 in (0, 11, 40 - n)]
    got = check([x], [c], windows, [5])
    assert list(np.diff(got.indptr)[:9]) == [0] * 9 and (np.diff(got.indptr)[9:] > 0).all()
    assert got[9].sum() == 1 and got[12].sum() == 2


@pytest.mark.parametrize('K', [3, 37, 150])
def test_the_sort_route_at_its_paddings(K):
    codes = hc.random_codes(K, 4200, K)
    x, c = hc.coded(codes, K)
    lag = 3
    sizes = (63, 64, 65, 255, 256, 257, 4095, 4096)
    assert all(_native.hac_route(n, K) == 'sort' for n in sizes)
    windows = [(t0, t0 + n + lag) for n in sizes for t0 in (0, 4200 - n - lag)]
    got = check([x], [c], windows, [lag])
    assert np.array_equal(np.asarray(got.sum(axis=1)).ravel(), np.repeat(sizes, 2))


@pytest.mark.parametrize('K', [1, 4, 192])
@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
def test_the_dense_route(K, f32):
    codes = hc.random_codes(K + 7, 9005, K)
    x, c = hc.coded(codes, K)
    assert _native.hac_route(4097, K) == _native.hac_route(9000, K) == 'dense'
    windows = [(0, 4097 + 5), (3, 3 + 4097 + 5), (0, 9005), (9005 - 4096 - 5, 9005), (100, 120)]        # the last two: sort route
    got = check([x], [c], windows, [5, 2], dtype=np.float32 if f32 else np.float64)
    assert got[2, :K * K].sum() == 9000 and got[0, :K * K].sum() == 4097


def test_a_segment_that_fits_neither_route_is_refused_with_the_outputs_untouched():
    import torch
    K, lag = 193, 1
    x, c = hc.coded(hc.random_codes(2, 4300, K), K)
    assert _native.hac_route(4097, K) == 'refused'
    windows = [(0, 50), (7, 7 + 4097 + lag), (0, 10)]
    with pytest.raises(_native.NativeError) as err:
        hac.windowed_hac([x], [c], windows, lags=[lag])
    assert err.value.code == _native.ERR_UNSUPP and 'window 1' in str(err.value) and 'stream 0' in str(err.value)
    dx, dc = on_device(x), on_device(c)
    nbytes = _native.hac_work_bytes(1, 4300, 1, 3)
    work = torch.full((nbytes,), 0x5a, dtype=torch.uint8, device='cuda')
    indptr = torch.full((4,), -77, dtype=torch.int64, device='cuda')
    with pytest.raises(_native.NativeError) as err:
        _native.hac_count_device([(dx.data_ptr(), 1, dc.data_ptr(), 1, 1, K)], 4300, [lag], windows, work.data_ptr(), nbytes, indptr.data_ptr())
    assert err.value.code == _native.ERR_UNSUPP
    assert (indptr.cpu().numpy() == -77).all() and (work.cpu().numpy() == 0x5a).all()
    # one code fewer fits the sort route
    check([x], [c], [(0, 50), (7, 7 + 4096 + lag), (0, 10)], [lag])


# ---- shapes of the counts -----------------------------------------------------------------------------------------------------------
def test_one_entry_holds_a_count_beyond_sixteen_bits():
    x, c = hc.coded(np.full(70005, 3), 4)
    for dt in (np.float64, np.float32):
        got = check([x], [c], [(0, 70005), (0, 4000)], [5], dtype=dt)
        assert got.nnz == 2 and list(got.indices) == [15, 15] and list(got.data) == [70000, 3995]
    one = check([x[:, :1]], [c[3:]], [(0, 70005)], [5])                            # K = 1: one column
    assert one.shape == (1, 1) and one[0, 0] == 70000


def test_all_pair_codes_distinct_and_the_first_and_last_columns():
    n, K = 300, 300
    x, c = hc.coded(np.arange(n) % K, K)
    got = check([x], [c], [(0, n)], [1])
    assert got.nnz == n - 1 and (got.data == 1).all()
    # first column: stream 0 all in unit 0; last column F - 1: the last stream all in its last unit, at the last lag
    x0, c0 = hc.coded(np.zeros(50, dtype=int), 6)
    x1, c1 = hc.coded(hc.random_codes(5, 50, 3), 3)
    x2, c2 = hc.coded(np.full(50, 4), 5)
    got = check([x0, x1, x2], [c0, c1, c2], [(0, 50), (10, 30)], [2, 7])
    F = 2 * (36 + 9 + 25)
    assert got.shape == (2, F) and got[0, 0] == 48 and got[0, F - 1] == 43 and got[1, F - 1] == 13 and got.indices.max() == F - 1


def test_lags_equal_single_and_longer_than_every_window():
    x, c = hc.coded(hc.random_codes(8, 120, 6), 6)
    windows = [(0, 120), (5, 17), (60, 61)]
    twice = check([x], [c], windows, [2, 2])
    assert np.array_equal(twice[:, :36].toarray(), twice[:, 36:].toarray())
    check([x], [c], windows, [1])
    none = check([x], [c], windows, [120, 500])
    assert none.nnz == 0 and not none.indptr.any()
    check([x], [c], windows, [3, 119, 1, 7, 2, 2, 50, 11])                          # eight lags, in the caller's order


def test_one_and_three_streams_of_unequal_shape():
    rng = np.random.default_rng(4)
    shapes = [(7, 3), (12, 13), (2, 40)]                                           # (K, d)
    codebooks = [rng.normal(size=s) for s in shapes]
    streams = [c[rng.integers(0, len(c), 90)] + 0.2 * rng.normal(size=(90, c.shape[1])) for c in codebooks]
    windows = [(0, 90), (3, 50), (40, 41), (88, 90)]
    check(streams, codebooks, windows, [5, 2])
    check(streams[1:2], codebooks[1:2], windows, [5, 2])
    check([s.astype(np.float32) for s in streams], [c.astype(np.float32) for c in codebooks], windows, [5, 2], dtype=np.float32)


def test_window_sets():
    x, c = hc.coded(hc.random_codes(9, 500, 7), 7)
    y, e = hc.coded(hc.random_codes(10, 500, 4), 4)
    args = ([x, y], [c, e])
    same = check(*args, windows=[(20, 90)] * 5, lags=[5, 2])
    assert all(np.array_equal(same[0].toarray(), same[r].toarray()) for r in range(5))
    check(*args, windows=[(0, 500), (10, 400), (100, 300), (150, 160), (155, 155)], lags=[5, 2])     # nested
    check(*args, windows=[(t, t + 50) for t in range(450, -1, -30)], lags=[5, 2])                    # descending
    check(*args, windows=[(3, 77)], lags=[5, 2])
    none = check(*args, windows=[], lags=[5, 2])
    assert none.shape == (0, 2 * (49 + 16))
    many = check(*args, windows=[(t % 493, t % 493 + 8) for t in range(3000)], lags=[5, 2])
    assert many.shape[0] == 3000 and many.sum() == 3000 * 2 * (3 + 6)


# ---- into the transform -----------------------------------------------------------------------------------------------------------
def trained_learner(f, k, dtype):
    rng = np.random.default_rng(12)
    learner = MultimodalLearner(['sound', 'objects'], [f, 5], [0.5, 1.0], k)
    dico = rng.random((k, f + 5)) + 0.01
    learner.dico = (dico / dico.sum(axis=1, keepdims=True)).astype(dtype)
    return learner


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
def test_reconstruct_internal_on_the_device_rows_is_the_host_upload_bit_for_bit(dtype):
    g = hc.golden()['a']
    rows = hac.windowed_hac(g['streams'], g['codebooks'], g['windows'], lags=g['lags'], dtype=dtype, output='device')
    assert isinstance(rows, hac.DeviceCsrRows) and rows.nnz == g['csr'].nnz
    learner = trained_learner(rows.shape[1], 6, dtype)
    on_rows = learner.reconstruct_internal('sound', rows, 8)
    downloaded = learner.reconstruct_internal('sound', rows.to_scipy(), 8)
    from_twin = learner.reconstruct_internal('sound', hc.twin(g['streams'], g['codebooks'], g['windows'], g['lags'], dtype=dtype), 8)
    assert on_rows.dtype == downloaded.dtype == np.dtype(dtype) and on_rows.shape == (len(g['windows']), 6)
    assert np.array_equal(on_rows, downloaded) and np.array_equal(on_rows, from_twin)
    assert np.isfinite(on_rows).all() and on_rows.max() > 0


def test_sliding_distances_is_the_composition_of_its_host_pieces():
    g = hc.golden()['b']
    k, it = 6, 8
    f = g['csr'].shape[1]
    learner = trained_learner(f, k, np.float64)
    examples = np.random.default_rng(2).random((7, k)) + 0.01
    got = evaluation.sliding_distances(learner, 'sound', g['streams'], g['codebooks'], g['windows'], examples, it, lags=g['lags'])
    assert got.shape == (len(g['windows']), 7) and got.dtype == np.float64
    X = hc.twin(g['streams'], g['codebooks'], g['windows'], g['lags'])
    internal = learner.reconstruct_internal('sound', X, it)                        # the CSR transform on the host matrix: the same bits
    assert np.array_equal(got, _native.all_distances(internal, examples, _native.DIST_COSINE_DIFF))
    ref, M = evc.all_pairs(internal, examples, evc.COSINE_DIFF)
    ok, worst = evc.within(got, ref, evc.distance_bar(k, M))
    assert ok, worst


def test_two_calls_on_one_workspace_give_equal_bits_and_leave_a_csr_fit_alone():
    import torch
    g = hc.golden()['a']
    Xs = sp.csr_matrix(g['csr'][:, :200], dtype=np.float64)

    def fit():
        m = KLdivNMF(n_components=4, max_iter=6, tol=0, precision='f64')
        m._init_dictionary = np.full((4, 200), 1.0 / 200)
        return m.fit_transform(Xs), m.components_
    W1, H1 = fit()
    dx = [on_device(x) for x in g['streams']]
    dc = [on_device(c) for c in g['codebooks']]
    table = [(x.data_ptr(), x.stride(0), c.data_ptr(), c.stride(0), x.shape[1], c.shape[0]) for x, c in zip(dx, dc)]
    T, N, Ks = 401, len(g['windows']), [c.shape[0] for c in dc]
    nbytes = _native.hac_work_bytes(3, T, 2, N)
    work = torch.zeros((nbytes,), dtype=torch.uint8, device='cuda')
    outs = []
    for _ in range(2):
        indptr = torch.full((N + 1,), -1, dtype=torch.int64, device='cuda')
        nnz = _native.hac_count_device(table, T, g['lags'], g['windows'], work.data_ptr(), nbytes, indptr.data_ptr())
        indices = torch.full((nnz,), -1, dtype=torch.int32, device='cuda')
        values = torch.full((nnz,), -1.0, dtype=torch.float64, device='cuda')
        _native.hac_fill_device(Ks, T, g['lags'], g['windows'], work.data_ptr(), nbytes, nnz, indices.data_ptr(), values.data_ptr())
        outs.append((indptr.cpu().numpy(), indices.cpu().numpy(), values.cpu().numpy()))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    assert hc.same_csr(sp.csr_matrix((outs[0][2], outs[0][1], outs[0][0]), shape=g['csr'].shape), sp.csr_matrix(g['csr'], dtype=np.float64))
    W2, H2 = fit()
    assert np.array_equal(W1, W2) and np.array_equal(H1, H2)


def test_native_refusals_leave_the_outputs_alone():
    import torch
    x, c = on_device(np.zeros((10, 2))), on_device(np.ones((3, 2)))
    nbytes = _native.hac_work_bytes(1, 10, 1, 1)
    work = torch.zeros((nbytes,), dtype=torch.uint8, device='cuda')
    indptr = torch.full((2,), -77, dtype=torch.int64, device='cuda')
    ok = dict(stream=(x.data_ptr(), 2, c.data_ptr(), 2, 2, 3), T=10, lags=[1], windows=[(0, 10)], nbytes=nbytes)

    def refused(**change):
        a = dict(ok, **change)
        with pytest.raises(_native.NativeError) as err:
            _native.hac_count_device([a['stream']] * a.get('copies', 1), a['T'], a['lags'], a['windows'], work.data_ptr(), a['nbytes'],
                                     indptr.data_ptr())
        assert err.value.code == _native.ERR_ARG
    refused(stream=(x.data_ptr(), 1, c.data_ptr(), 2, 2, 3))                       # a stride below d
    refused(stream=(0, 2, c.data_ptr(), 2, 2, 3))
    refused(stream=(x.data_ptr(), 2, 0, 2, 2, 3))
    refused(windows=[(0, 11)])
    refused(windows=[(5, 4)])
    refused(windows=[(-1, 4)])
    refused(lags=[0])
    refused(lags=[1] * 9)
    refused(copies=9)
    refused(nbytes=nbytes - 1)
    refused(stream=(x.data_ptr(), 2, c.data_ptr(), 2, 2, 46341))                   # F >= 2^31
    assert (indptr.cpu().numpy() == -77).all()
    assert _native.hac_count_device([ok['stream']], 10, [1], [], work.data_ptr(), nbytes, indptr.data_ptr()) == 0      # N = 0
    assert list(indptr.cpu().numpy()) == [0, -77]
