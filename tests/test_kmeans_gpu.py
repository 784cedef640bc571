"""The codebook builders on the device (include/klnmf_kmeans.h, csrc/kmeans.hip.h) against the host twin.

Every comparison with the twin (multimodal_amd/features/codebook.py; pinned to the reference's recorded outputs by
tests/test_kmeans_cpu.py) is bit for bit, in float64 and float32: the labels are `features.hac.quantize`'s, the sums follow the
stated order, the mean is one division -- nothing here has a tolerance.  The shapes are the smallest at which each mechanism can
go wrong: T around a tile (256 frames) and a group (4096 frames, the unit of the summation order), K and d at every staging
choice and every ownership map of the accumulators (d below and above 256 threads), K * d at the LDS bound."""
import numpy as np
import pytest

from multimodal_amd import _native
from multimodal_amd.features import codebook as cbk
from multimodal_amd.features import hac
from tests import kmeans_cases as kc

pytestmark = pytest.mark.gpu

TILE, GROUP = kc.TILE, kc.GROUP
F32 = pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])


def on_device(a):
    import torch
    return torch.from_numpy(np.array(a, order='C')).to('cuda')


def device_lloyd(x, init, n_iter, pad=0):
    """(codebook, labels, counts) of klnmf_kmeans_device on uploads of x and init; `pad`: extra columns of the row strides."""
    import torch
    x, init = np.asarray(x), np.asarray(init)
    f64 = x.dtype == np.float64
    (T, d), K = x.shape, init.shape[0]
    dx = torch.full((max(T, 1), d + pad), 99.0, dtype=torch.float64 if f64 else torch.float32, device='cuda')
    dc = torch.full((K, d + pad), 77.0, dtype=dx.dtype, device='cuda')
    dx[:T, :d] = on_device(x)
    dc[:, :d] = on_device(init)
    wb = _native.kmeans_work_bytes(T, d, K)
    work = torch.empty(max(16, wb), dtype=torch.uint8, device='cuda')
    labels = torch.full((max(T, 1),), -7, dtype=torch.int32, device='cuda')
    counts = torch.full((K,), -7, dtype=torch.int64, device='cuda')
    _native.kmeans_device(dx.data_ptr(), d + pad, T, d, dc.data_ptr(), d + pad, K, n_iter, work.data_ptr(), wb, labels.data_ptr(),
                          counts.data_ptr(), f64=f64)
    torch.cuda.synchronize()
    if pad:
        assert (dc[:, d:] == 77.0).all()
    return dc[:, :d].cpu().numpy().copy(), labels[:T].cpu().numpy(), counts.cpu().numpy()


def device_gram(x, labels, cluster, pad=0):
    import torch
    x = np.asarray(x)
    f64 = x.dtype == np.float64
    T, d = x.shape
    dx = torch.full((max(T, 1), d + pad), 99.0, dtype=torch.float64 if f64 else torch.float32, device='cuda')
    dx[:T, :d] = on_device(x)
    d_labels = on_device(np.asarray(labels, dtype=np.int32)) if labels is not None else None
    wb = _native.kmeans_work_bytes(T, d, 1)
    work = torch.empty(max(16, wb), dtype=torch.uint8, device='cuda')
    out = torch.full((d * d + d,), -7.0, dtype=torch.float64, device='cuda')
    n = _native.kmeans_gram_device(dx.data_ptr(), d + pad, T, d, d_labels.data_ptr() if d_labels is not None else 0, cluster,
                                   work.data_ptr(), wb, out.data_ptr(), out.data_ptr() + 8 * d * d, f64=f64)
    out = out.cpu().numpy()
    return out[:d * d].reshape(d, d), out[d * d:], n


def check_lloyd(x, init, n_iter, pad=0):
    got, want = device_lloyd(x, init, n_iter, pad), cbk.host_lloyd(x, init, n_iter)
    for a, b in zip(got, want):
        assert kc.same_bits(a, b)
    assert got[2].sum() == len(x)
    return got


def check_gram(x, labels, cluster, pad=0):
    got, want = device_gram(x, labels, cluster, pad), cbk.host_gram(x, labels, cluster)
    assert kc.same_bits(got[0], want[0]) and kc.same_bits(got[1], want[1]) and got[2] == want[2]
    assert kc.same_bits(got[0], got[0].T.copy())
    return got


# ---- the recorded cases -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['a', 'b'])
@F32
@pytest.mark.parametrize('tensors', [False, True], ids=['host', 'device'])
def test_the_recorded_cases(tag, f32, tensors):
    g = kc.golden()[tag]
    dt = np.float32 if f32 else np.float64
    X, init, K = g['data'].astype(dt), g['init'].astype(dt), g['K']                # (the frames are exact in float32)
    want = cbk.host_kmeans(X, init)
    data, first = (on_device(X), on_device(init)) if tensors else (X, init)
    cb, labels = cbk.kmeans(data, first)
    assert kc.same_bits(cb, want[0]) and kc.same_bits(labels, want[1])
    it = cbk.iterative_kmeans(data, K)
    assert kc.same_bits(it, cbk.host_iterative_kmeans(X, K))
    raw = cbk.build_codebook(data, K, rng=g['raw_seed'])
    assert kc.same_bits(raw, cbk.host_build_codebook(X, K, rng=g['raw_seed']))
    if not f32:                                                                    # the reference's own numbers
        assert kc.same_bits(cb, g['matrix']) and kc.same_bits(labels, g['matrix_labels']) and kc.same_bits(raw, g['raw'])
        assert kc.same_bits(kc.sorted_rows(it), kc.sorted_rows(g['iterative']))
    if not tensors:                                                                # the host-array entry of the C-ABI
        cb, labels, counts = _native.kmeans(X, init, 10)
        assert kc.same_bits(cb, want[0]) and kc.same_bits(labels, want[1])
        assert kc.same_bits(counts, np.bincount(labels, minlength=K).astype(np.int64))


# ---- the order of the additions ---------------------------------------------------------------------------------------------------
@F32
def test_sums_of_plain_normals_follow_the_stated_order_and_repeat(f32):
    T, d, K = 2 * GROUP + 300, 13, 7
    x, init = kc.normals(11, T, d, K, f32)
    want = kc.twin_lloyd(11, T, d, K, f32, 3)
    first, second = device_lloyd(x, init, 3), device_lloyd(x, init, 3)
    for a, b, c in zip(first, second, want):
        assert kc.same_bits(a, c) and kc.same_bits(b, c)
    labels = want[1]
    naive = np.vstack([x[labels == k].astype(np.float64).mean(axis=0) for k in range(K)])
    assert f32 or not np.array_equal(naive, first[0])                              # (another order gives other bits: the data shows it)
    check_gram(x, labels, 3)
    check_gram(x[:GROUP + 9], None, -1)


@pytest.mark.parametrize('T', [1, TILE - 1, TILE, TILE + 1, GROUP - TILE, GROUP - 1, GROUP, GROUP + 1, GROUP + TILE, 3 * GROUP + 77])
def test_frame_counts_at_the_edges_of_tiles_and_groups(T):
    x, init = kc.normals(T, T, 3, 4)
    check_lloyd(x, init, 2)
    _, labels, _ = cbk.host_lloyd(x, init, 0)
    check_gram(x, labels, 1)
    check_gram(x.astype(np.float32), None, -1)


@pytest.mark.parametrize('d', [1, 13, 33, 65])
@pytest.mark.parametrize('K', [1, 2, 150])
@F32
def test_lloyd_at_every_k_and_d(K, d, f32):
    x, init = kc.normals(100 * K + d, 600, d, K, f32)
    check_lloyd(x, init, 2)


@pytest.mark.parametrize('K,d', [(1000, 13), (3, 300), (2, 256), (150, 39)])
def test_lloyd_at_the_other_staging_and_ownership_choices(K, d):
    # 1000 x 13: the frames staged, the codebook not; d >= 256: a thread owns columns of every cluster
    x, init = kc.normals(K + d, 700, d, K)
    check_lloyd(x, init, 2)


@pytest.mark.parametrize('d', [1, 13, 64])
@F32
def test_the_gram_matrix(d, f32):
    T = GROUP + 70
    x, _ = kc.normals(d, T, d, 3, f32)
    labels = np.random.default_rng(d).integers(0, 3, T).astype(np.int32)
    labels[labels == 2] = 0
    labels[GROUP + 5] = 2                                                          # one member, in the second group
    G, s, n = check_gram(x, None, -1)
    assert n == T
    check_gram(x, labels, 1)
    G, s, n = check_gram(x, labels, 2)
    x1 = x[GROUP + 5].astype(np.float64)
    assert n == 1 and kc.same_bits(G, np.outer(x1, x1)) and kc.same_bits(s, x1)
    G, s, n = check_gram(x, labels, 4)                                             # no member
    assert n == 0 and not G.any() and not s.any()
    check_gram(x, labels, 1, pad=3)


def test_rows_with_a_stride_above_d():
    x, init = kc.normals(21, GROUP + 40, 13, 9)
    check_lloyd(x, init, 2, pad=5)
    check_lloyd(x.astype(np.float32), init.astype(np.float32), 2, pad=1)


@pytest.mark.parametrize('K,d', [(13312, 1), (1, 13312), (1024, 13)])
def test_the_lds_bound_passes_and_one_past_it_is_refused(K, d):
    import torch
    assert K * d == cbk.MAX_KD
    x, init = kc.normals(K, 300, d, K)
    check_lloyd(x, init, 1)
    K1, d1 = (K + 1, d) if d == 1 else (K, d + 1)
    dx, dc = torch.zeros((300, d1), dtype=torch.float64, device='cuda'), torch.full((K1, d1), 5.0, dtype=torch.float64, device='cuda')
    work = torch.empty(1 << 24, dtype=torch.uint8, device='cuda')
    labels, counts = torch.full((300,), -7, dtype=torch.int32, device='cuda'), torch.full((K1,), -7, dtype=torch.int64, device='cuda')
    with pytest.raises(_native.NativeError) as e:
        _native.kmeans_device(dx.data_ptr(), d1, 300, d1, dc.data_ptr(), d1, K1, 1, work.data_ptr(), 1 << 24, labels.data_ptr(),
                              counts.data_ptr())
    torch.cuda.synchronize()
    assert e.value.code == _native.ERR_UNSUPP
    assert (dc == 5.0).all() and (labels == -7).all() and (counts == -7).all()


def test_refused_arguments_write_nothing():
    import torch
    dx, dc = torch.zeros((40, 4), dtype=torch.float64, device='cuda'), torch.full((3, 4), 5.0, dtype=torch.float64, device='cuda')
    work = torch.empty(1 << 16, dtype=torch.uint8, device='cuda')
    labels, counts = torch.full((40,), -7, dtype=torch.int32, device='cuda'), torch.full((3,), -7, dtype=torch.int64, device='cuda')
    out = torch.full((20,), -7.0, dtype=torch.float64, device='cuda')
    ok = dict(d_frames=dx.data_ptr(), ld=4, T=40, d=4, d_codebook=dc.data_ptr(), ldc=4, K=3, n_iter=1, d_work=work.data_ptr(),
              work_bytes=1 << 16, d_labels=labels.data_ptr(), d_counts=counts.data_ptr())
    for change in (dict(d_frames=0), dict(d_codebook=0), dict(d_work=0), dict(d_labels=0), dict(d_counts=0), dict(ld=3), dict(ldc=3),
                   dict(d=0), dict(K=0), dict(T=-1), dict(T=1 << 31), dict(n_iter=-1), dict(work_bytes=8)):
        with pytest.raises(_native.NativeError) as e:
            _native.kmeans_device(**dict(ok, **change))
        assert e.value.code == _native.ERR_ARG, change
    lib = _native.load()
    assert lib.klnmf_kmeans_device(0, 7, dx.data_ptr(), 4, 40, 4, dc.data_ptr(), 4, 3, 1, work.data_ptr(), 1 << 16, labels.data_ptr(),
                                   counts.data_ptr()) == _native.ERR_ARG                              # a bad dtype
    gram = dict(d_frames=dx.data_ptr(), ld=4, T=40, d=4, d_labels=labels.data_ptr(), cluster=0, d_work=work.data_ptr(),
                work_bytes=1 << 16, d_gram=out.data_ptr(), d_colsum=out.data_ptr() + 128)
    for change in (dict(cluster=-2), dict(d_frames=0), dict(d_labels=0), dict(d_gram=0), dict(d_colsum=0), dict(d_work=0), dict(ld=3),
                   dict(d=0), dict(T=-1), dict(work_bytes=8)):
        with pytest.raises(_native.NativeError) as e:
            _native.kmeans_gram_device(**dict(gram, **change))
        assert e.value.code == _native.ERR_ARG, change
    with pytest.raises(_native.NativeError) as e:
        _native.kmeans_gram_device(**dict(gram, d=65, ld=65))
    assert e.value.code == _native.ERR_UNSUPP
    torch.cuda.synchronize()
    assert (dc == 5.0).all() and (labels == -7).all() and (counts == -7).all() and (out == -7.0).all()
    # T = 0: KLNMF_OK, the codebook untouched, the counts 0
    _native.kmeans_device(**dict(ok, T=0, d_frames=0, d_labels=0))
    torch.cuda.synchronize()
    assert (dc == 5.0).all() and (counts == 0).all()
    assert _native.kmeans_gram_device(**dict(gram, T=0, d_frames=0, cluster=-1, d_labels=0)) == 0 and (out[:20] == 0).all()


# ---- empty clusters, labels, counts -------------------------------------------------------------------------------------------------
@F32
def test_clusters_without_members_keep_their_rows(f32):
    dt = np.float32 if f32 else np.float64
    x, _ = kc.normals(31, 500, 3, 2, f32)
    far = np.array([1e6 + 1.0 / 3.0, -1e6, np.pi]).astype(dt)
    cb, labels, counts = check_lloyd(x, np.vstack([x[0], far, x[1]]), 3)
    assert counts[1] == 0 and kc.same_bits(cb[1], far)
    cb, labels, counts = check_lloyd(x, np.vstack([x[0], x[0], x[1]]), 1)          # duplicate rows: the tie goes low
    assert counts[1] == 0 and counts[0] > 0 and kc.same_bits(cb[1], x[0])
    cb, labels, counts = check_lloyd(x[:2], (x[:5] + dt(0.01)).astype(dt), 2)      # K > T
    assert list(counts) == [1, 1, 0, 0, 0] and kc.same_bits(cb[2:], (x[2:5] + dt(0.01)).astype(dt))


def test_no_iteration_is_labels_and_counts_alone():
    x, init = kc.normals(41, GROUP + 3, 5, 6)
    cb, labels, counts = check_lloyd(x, init, 0)
    assert kc.same_bits(cb, init) and kc.same_bits(labels, hac.quantize(x, init))
    assert kc.same_bits(counts, np.bincount(labels, minlength=6).astype(np.int64))


def test_the_labels_are_those_of_the_last_assignment():
    x = np.array([[0.0], [1.0], [1.2], [10.0]])
    cb, labels, counts = check_lloyd(x, np.array([[0.0], [1.15]]), 1)
    assert list(labels) == [0, 1, 1, 1] and list(counts) == [1, 3] and list(hac.quantize(x, cb)) == [0, 0, 0, 1]
    mid = np.array([[0.5], [0.0], [1.0], [0.5]])
    assert list(check_lloyd(mid, np.array([[0.0], [1.0]]), 1)[1]) == [0, 0, 1, 0]  # exactly midway: index 0


# ---- the builders end to end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T,d,K', [(600, 13, 12), (GROUP + 300, 5, 6)])
def test_iterative_kmeans_end_to_end_and_into_windowed_hac(T, d, K):
    X = kc.golden()['a']['data'] if T == 600 else kc.normals(51, T, d, K)[0]
    want = cbk.host_iterative_kmeans(X, K)
    dX = on_device(X)
    book = cbk.iterative_kmeans(dX, K, output='device')
    assert book.is_cuda and kc.same_bits(book.cpu().numpy(), want)
    assert kc.same_bits(cbk.iterative_kmeans(X, K), want)
    windows = hac.frame_windows(T, 50, 25)
    on = hac.windowed_hac([dX], [book], windows)
    off = hac.windowed_hac([X], [book.cpu().numpy()], windows)
    assert np.array_equal(on.indptr, off.indptr) and np.array_equal(on.indices, off.indices) and np.array_equal(on.data, off.data)
    assert on.nnz > 0
    books = cbk.build_codebooks([dX, dX[: T // 2]], (3, 2), mode='raw', rng=5, output='device')
    rng = np.random.default_rng(5)
    for got, x, k in zip(books, (X, X[: T // 2]), (3, 2)):
        assert kc.same_bits(got.cpu().numpy(), cbk.host_build_codebook(x, k, rng=rng))
