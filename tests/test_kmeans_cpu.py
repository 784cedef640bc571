"""The codebook builders without a GPU: the exports of include/klnmf_kmeans.h; the host twin (multimodal_amd/features/codebook.py)
against the REFERENCE's recorded outputs (tests/golden/g22_kmeans.npz: its `iterative_kmeans`, scipy's `kmeans2` from a matrix and
from its 'random' initialisation) by equality; the twin's edge rules; and the routing of `kmeans`, `iterative_kmeans`,
`build_codebook` and `build_codebooks`, with recording stand-ins for the native calls that answer from the host twin on CPU
tensors.  Every host refusal raises before any native call."""
import ctypes
import os
import re

import numpy as np
import pytest

from multimodal_amd import _native
from multimodal_amd.features import codebook as cbk
from multimodal_amd.features import hac
from tests import kmeans_cases as kc
from tests.test_batch_csr_cpu import check_header_tables, declared_in, other_headers
from tests.test_hac_cpu import host_matrix

NEW = {'klnmf_kmeans_work_bytes', 'klnmf_kmeans_device', 'klnmf_kmeans_gram_device', 'klnmf_kmeans'}
OTHERS = other_headers('klnmf_kmeans.h')
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'klnmf_kmeans.h')


# ---- the bindings -------------------------------------------------------------------------------------------------------------------
def test_every_declared_kmeans_symbol_is_bound_and_exported():
    declared = declared_in('klnmf_kmeans.h')
    assert declared == NEW == set(_native.KMEANS_SIGNATURES)
    lib = _native.load()
    for name in declared:
        assert hasattr(lib, name), name
    for header in OTHERS:
        assert not (declared & declared_in(header)), header
    for name in ('kmeans_work_bytes', 'kmeans_device', 'kmeans_gram_device', 'kmeans'):
        assert callable(getattr(_native, name))
    defines = dict(re.findall(r'^#define (KLNMF_KMEANS_\w+) (\d+)$', open(HEADER).read(), flags=re.M))
    assert {k: int(v) for k, v in defines.items()} == {
        'KLNMF_KMEANS_TILE': _native.KMEANS_TILE, 'KLNMF_KMEANS_GROUP': _native.KMEANS_GROUP,
        'KLNMF_KMEANS_MAX_KD': _native.KMEANS_MAX_KD, 'KLNMF_KMEANS_GRAM_MAX_D': _native.KMEANS_GRAM_MAX_D}
    assert (kc.TILE, kc.GROUP, cbk.GROUP, cbk.MAX_KD, cbk.GRAM_MAX_D) == (256, 4096, 4096, 13312, 64)
    assert 150 * 39 <= cbk.MAX_KD and 1000 * 13 <= cbk.MAX_KD
    assert cbk.MAX_KD * 8 + cbk.MAX_KD * 4 + 256 * 4 <= 160 * 1024               # accumulators, counts (d = 1) and labels in LDS


def test_the_other_headers_declare_what_they_declared():
    check_header_tables()                # (and NEW is this header's own table: the test above)


def test_every_entry_point_names_the_reference_lines_it_replaces():
    header = open(HEADER).read()
    for name in NEW:
        comment = header[:header.index('int %s(' % name)].rsplit('/*', 1)[1]
        assert 'features/hac.py' in comment, name


def test_the_workspace_size_is_host_arithmetic():
    up16 = lambda b: (b + 15) // 16 * 16
    pairs = lambda d: d * (d + 1) // 2 + d

    def want(T, d, K):
        G = max(1, -(-T // 4096))
        lloyd = up16(G * K * d * 8) + up16(G * K * 4)
        gram = up16(G * pairs(d) * 8) + up16(G * 4) + 16 if d <= 64 else 0
        return max(lloyd, gram)
    for T, d, K in ((0, 1, 1), (1, 13, 1), (4096, 13, 150), (4097, 13, 150), (800000, 39, 100), (5000, 65, 3), (9000, 64, 2),
                    (100, 1, 13312), (100, 13312, 1), (100, 13, 1024)):
        assert _native.kmeans_work_bytes(T, d, K) == want(T, d, K), (T, d, K)
    for bad in ((-1, 3, 3), (1 << 31, 3, 3), (10, 0, 3), (10, 3, 0)):
        with pytest.raises(_native.NativeError) as e:
            _native.kmeans_work_bytes(*bad)
        assert e.value.code == _native.ERR_ARG
    for beyond in ((10, 13, 1025), (10, 1, 13313), (10, 13313, 1), (10, 1 << 40, 1 << 40)):
        with pytest.raises(_native.NativeError) as e:
            _native.kmeans_work_bytes(*beyond)
        assert e.value.code == _native.ERR_UNSUPP


# ---- the host twin against the reference's recorded outputs ---------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['a', 'b'])
def test_the_host_twin_gives_the_recorded_codebooks(tag):
    g = kc.golden()[tag]
    X, K = g['data'], g['K']
    assert np.array_equal(X * 1024, np.round(X * 1024))                            # multiples of 2^-10: every sum is exact
    cb, labels = cbk.host_kmeans(X, g['init'])
    assert kc.same_bits(cb, g['matrix']) and kc.same_bits(labels, g['matrix_labels'])
    assert len(np.unique(labels)) == K
    it = cbk.host_iterative_kmeans(X, K)
    assert it.shape == (K, X.shape[1]) and kc.same_bits(kc.sorted_rows(it), kc.sorted_rows(g['iterative']))
    assert kc.same_bits(cbk.host_build_codebook(X, K, mode='iterative'), it)
    raw = cbk.host_build_codebook(X, K, mode='raw', rng=g['raw_seed'])
    assert kc.same_bits(raw, g['raw'])
    assert kc.same_bits(cbk.host_build_codebook(X, K, mode='raw', rng=np.random.default_rng(g['raw_seed'])), g['raw'])
    assert kc.same_bits(cbk.host_lloyd(X, g['raw'], 0)[1], hac.quantize(X, g['raw']))
    G, s, T = cbk.host_gram(X, None, -1)
    assert kc.same_bits(cbk.host_kmeans(X, cbk.random_init(G, s, T, K, g['raw_seed']))[1], g['raw_labels'])
    # float32: the frames are exact, one update is the float64 one rounded once
    one32 = cbk.host_lloyd(X.astype(np.float32), g['init'].astype(np.float32), 1)
    one64 = cbk.host_lloyd(X, g['init'], 1)
    assert one32[0].dtype == np.float32 and kc.same_bits(one32[0], one64[0].astype(np.float32)) and kc.same_bits(one32[1], one64[1])
    with pytest.raises(ValueError):
        cbk.host_build_codebook(X, K, mode='kmeans++')


# ---- the twin's edge rules ----------------------------------------------------------------------------------------------------------
def test_labels_tie_low_and_are_those_before_the_last_update():
    x = np.array([[0.5], [0.0], [1.0], [0.5]])
    cb, labels, counts = cbk.host_lloyd(x, [[0.0], [1.0]], 1)
    assert list(labels) == [0, 0, 1, 0] and list(counts) == [3, 1] and counts.dtype == np.int64 and labels.dtype == np.int32
    assert kc.same_bits(cb, np.array([[1.0 / 3.0], [1.0]]))
    assert list(hac.quantize(x, cb)) == [0, 0, 1, 0]
    # labels of the last assignment, not of the final codebook
    x = np.array([[0.0], [1.0], [1.2], [10.0]])
    cb, labels = cbk.host_kmeans(x, [[0.0], [5.5]], iter=1)
    assert list(labels) == [0, 0, 0, 1] and list(hac.quantize(x, cb)) == [0, 0, 0, 1]
    cb, labels = cbk.host_kmeans(x, [[0.0], [1.15]], iter=1)                       # 0 | 1, 1.2, 10 -> rows 0 and 12.2 / 3
    assert list(labels) == [0, 1, 1, 1] and list(hac.quantize(x, cb)) == [0, 0, 0, 1]
    same, zero, counts = cbk.host_lloyd(x, [[0.0], [1.15]], 0)
    assert kc.same_bits(same, np.array([[0.0], [1.15]])) and list(zero) == [0, 1, 1, 1] and list(counts) == [1, 3]


def test_a_cluster_without_members_keeps_its_row():
    rng = np.random.default_rng(4)
    x = rng.normal(size=(50, 3))
    far = np.array([1e6 + 1.0 / 3.0, -1e6, np.pi])
    init = np.vstack([x[0], far, x[1]])
    cb, labels, counts = cbk.host_lloyd(x, init, 3)
    assert counts[1] == 0 and 1 not in labels and kc.same_bits(cb[1], far) and counts.sum() == 50
    # duplicate rows: the tie goes low, the duplicate stays empty
    cb, labels, counts = cbk.host_lloyd(x, np.vstack([x[0], x[0], x[1]]), 1)
    assert counts[1] == 0 and kc.same_bits(cb[1], x[0])
    # K > T
    cb, labels, counts = cbk.host_lloyd(x[:2], x[:5] + 0.01, 2)
    assert list(labels) == [0, 1] and list(counts) == [1, 1, 0, 0, 0] and kc.same_bits(cb[2:], x[2:5] + 0.01) and kc.same_bits(cb[:2], x[:2])
    # all frames in one cluster
    cb, labels, counts = cbk.host_lloyd(x, np.vstack([x.mean(axis=0), far]), 2)
    assert list(counts) == [50, 0] and not labels.any()


def test_the_summation_order_is_the_stated_one():
    x, init = kc.normals(5, 2 * kc.GROUP + 77, 3, 4)
    cb, labels, counts = cbk.host_lloyd(x, init, 1)
    for k in range(4):
        total = np.zeros(3)
        for g0 in range(0, len(x), kc.GROUP):
            part = np.zeros(3)
            for t in range(g0, min(len(x), g0 + kc.GROUP)):
                if labels[t] == k:
                    part = part + x[t]
            total = total + part
        assert kc.same_bits(cb[k], total / float(counts[k]))
    assert not np.array_equal(cb, np.vstack([x[labels == k].mean(axis=0) for k in range(4)]))      # (numpy's order is another)
    G, s, n = cbk.host_gram(x, labels, 2)
    want = np.zeros((3, 3))
    for g0 in range(0, len(x), kc.GROUP):
        part = np.zeros((3, 3))
        for t in range(g0, min(len(x), g0 + kc.GROUP)):
            if labels[t] == 2:
                part = part + np.outer(x[t], x[t])
        want = want + part
    assert kc.same_bits(G, want) and kc.same_bits(G, G.T.copy()) and n == counts[2]


def test_the_split_rules():
    assert kc.same_bits(cbk.split_direction(np.zeros((3, 3))), np.zeros(3))        # lambda = 0: p = 0
    rows = cbk.split_rows(np.array([1.0, 2.0, 3.0]), np.zeros(3), 0.01, np.float64)
    assert kc.same_bits(rows, np.array([[1.0, 2.0, 3.0]] * 2))
    p = cbk.split_direction(np.diag([1.0, 16.0, 4.0]))
    assert np.allclose(p, [0.0, 2.0, 0.0]) and p[1] > 0                            # v * lambda^(1/4), the sign positive
    v = np.array([1.0, -3.0, 2.0])
    p = cbk.split_direction(np.outer(v, v))
    assert p[1] > 0 and np.allclose(p, -v / np.sqrt(14.0) * 14.0 ** 0.25)          # the largest component made positive
    v = np.array([2.0, -2.0])
    assert cbk.split_direction(np.outer(v, v))[0] > 0                              # equal magnitudes: the lowest index
    # the reference's form on the members themselves: v[0] * sqrt(s[0])
    x = np.random.default_rng(8).normal(size=(40, 5)) + 3.0
    u, s, vt = np.linalg.svd(x)
    ref = vt[0] * np.sqrt(s[0])
    got = cbk.split_direction(x.T @ x)
    assert np.allclose(got, ref if ref[np.argmax(np.abs(ref))] > 0 else -ref, rtol=1e-12, atol=1e-14)


def test_the_largest_cluster_is_the_lowest_index_among_equal_counts():
    x = np.array([[0.0], [0.0], [4.0], [4.0]])
    a = 0.01 * 32.0 ** 0.25
    cb = cbk.host_iterative_kmeans(x, 2)
    assert kc.same_bits(cb, np.array([[4.0], [0.0]]))                              # 2 + a p takes the frames at 4
    cb = cbk.host_iterative_kmeans(x, 3)
    # counts [2, 2]: cluster 0 (the frames at 4) is split, so that row 0 is the old row 1; of the two new rows, about as far from
    # 4 on either side, one takes both frames and the other stays where the split put it
    assert cb[0, 0] == 0.0 and sorted(np.round(np.abs(cb[1:, 0] - 4.0) / a, 9)) == [0.0, 1.0]


# ---- the routing, with recording stand-ins --------------------------------------------------------------------------------------------
def write_matrix(ptr, a, ld):
    ctype = ctypes.c_double if a.dtype == np.float64 else ctypes.c_float
    for r, row in enumerate(a):
        np.ctypeslib.as_array((ctype * a.shape[1]).from_address(ptr + r * ld * a.itemsize))[:] = row


class KmRecorder(object):
    """Stand-ins for the device calls: they answer from the host twin and record what they were asked."""

    def __init__(self, monkeypatch):
        self.calls, self.labels = [], None
        monkeypatch.setattr(_native, 'kmeans_device', self.lloyd)
        monkeypatch.setattr(_native, 'kmeans_gram_device', self.gram)
        monkeypatch.setattr(_native, 'kmeans', self.never)

    def never(self, *a, **k):
        raise AssertionError('the host-array entry is not the device path')

    def lloyd(self, d_frames, ld, T, d, d_codebook, ldc, K, n_iter, d_work, work_bytes, d_labels, d_counts, f64=True, device=0):
        dt = np.float64 if f64 else np.float32
        assert work_bytes >= _native.kmeans_work_bytes(T, d, K) and d_work and ld >= d and ldc >= d
        x, c = host_matrix(d_frames, T, ld, d, dt), host_matrix(d_codebook, K, ldc, d, dt)
        cb, labels, counts = cbk.host_lloyd(x, c, n_iter)
        if n_iter:
            write_matrix(d_codebook, cb, ldc)
        np.ctypeslib.as_array((ctypes.c_int32 * T).from_address(d_labels))[:] = labels
        np.ctypeslib.as_array((ctypes.c_int64 * K).from_address(d_counts))[:] = counts
        self.labels = (d_labels, labels)
        self.calls.append(dict(call='lloyd', frames=d_frames, ld=ld, T=T, d=d, K=K, n_iter=n_iter, f64=f64, codebook=d_codebook,
                               counts=counts))

    def gram(self, d_frames, ld, T, d, d_labels, cluster, d_work, work_bytes, d_gram, d_colsum, f64=True, device=0):
        dt = np.float64 if f64 else np.float32
        assert work_bytes >= _native.kmeans_work_bytes(T, d, 1) and d_work
        if cluster >= 0:
            assert self.labels[0] == d_labels
        G, s, n = cbk.host_gram(host_matrix(d_frames, T, ld, d, dt), None if cluster < 0 else self.labels[1], cluster)
        np.ctypeslib.as_array((ctypes.c_double * (d * d)).from_address(d_gram))[:] = G.ravel()
        np.ctypeslib.as_array((ctypes.c_double * d).from_address(d_colsum))[:] = s
        self.calls.append(dict(call='gram', frames=d_frames, ld=ld, T=T, d=d, cluster=cluster, f64=f64))
        return n


@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
def test_kmeans_is_one_lloyd_call(monkeypatch, f32):
    import torch
    rec = KmRecorder(monkeypatch)
    x, init = kc.normals(1, 700, 5, 6, f32)
    want = cbk.host_kmeans(x, init, iter=4)
    cb, labels = cbk.kmeans(x, init, iter=4, device='cpu')
    assert kc.same_bits(cb, want[0]) and kc.same_bits(labels, want[1])
    assert len(rec.calls) == 1
    call = rec.calls[0]
    assert (call['call'], call['T'], call['d'], call['K'], call['n_iter'], call['f64'], call['ld']) == ('lloyd', 700, 5, 6, 4, not f32, 5)
    # tensors are used in place, a row stride above d included; the initial codebook is not written
    wide = torch.zeros((700, 8), dtype=torch.float32 if f32 else torch.float64)
    wide[:, :5] = torch.from_numpy(x.copy())
    t_init = torch.from_numpy(init.copy())
    d_cb, d_labels = cbk.kmeans(wide[:, :5], t_init, iter=4, device='cpu', output='device')
    call = rec.calls[1]
    assert call['frames'] == wide.data_ptr() and call['ld'] == 8 and call['codebook'] == d_cb.data_ptr() != t_init.data_ptr()
    assert torch.is_tensor(d_cb) and d_cb.is_contiguous() and d_labels.dtype == torch.int32
    assert kc.same_bits(d_cb.numpy(), want[0]) and kc.same_bits(d_labels.numpy(), want[1]) and kc.same_bits(t_init.numpy(), init)
    # mixed types are float64
    cbk.kmeans(x, init.astype(np.float64), iter=1, device='cpu')
    assert rec.calls[2]['f64']


def test_iterative_kmeans_makes_three_calls_per_round_in_order(monkeypatch):
    rec = KmRecorder(monkeypatch)
    g = kc.golden()['b']
    X, K = g['data'], g['K']
    cb = cbk.iterative_kmeans(X, K, device='cpu')
    want = cbk.host_iterative_kmeans(X, K)
    assert kc.same_bits(cb, want) and kc.same_bits(kc.sorted_rows(cb), kc.sorted_rows(g['iterative']))
    names = [(c['call'], c.get('n_iter'), c.get('K')) for c in rec.calls]
    expect = [('lloyd', 1, 1)]
    for k in range(1, K):
        expect += [('lloyd', 0, k), ('gram', None, None), ('lloyd', 10, k + 1)]
    assert names == expect
    for i in range(1, len(rec.calls), 3):
        assert rec.calls[i + 1]['cluster'] == int(np.argmax(rec.calls[i]['counts']))
    assert len({c['frames'] for c in rec.calls}) == 1                              # one upload of the frames
    # float32 frames stay float32; iter and alpha reach the calls
    n = len(rec.calls)
    cb32 = cbk.iterative_kmeans(X.astype(np.float32), 3, alpha=0.05, iter=2, device='cpu')
    assert cb32.dtype == np.float32 and kc.same_bits(cb32, cbk.host_iterative_kmeans(X.astype(np.float32), 3, alpha=0.05, iter=2))
    assert [c.get('n_iter') for c in rec.calls[n:]] == [1, 0, None, 2, 0, None, 2] and not rec.calls[n]['f64']
    # k = 1: the mean alone
    assert kc.same_bits(cbk.iterative_kmeans(X, 1, device='cpu'), want_mean(X))


def want_mean(X):
    return cbk.host_lloyd(X, np.zeros((1, X.shape[1])), 1)[0]


def test_build_codebook_routes_by_mode(monkeypatch):
    rec = KmRecorder(monkeypatch)
    g = kc.golden()['b']
    X, K = g['data'], g['K']
    raw = cbk.build_codebook(X, K, rng=g['raw_seed'], device='cpu')
    assert kc.same_bits(raw, g['raw'])
    assert [(c['call'], c.get('cluster'), c.get('n_iter')) for c in rec.calls] == [('gram', -1, None), ('lloyd', None, 10)]
    rec.calls[:] = []
    it = cbk.build_codebook(X, K, mode='iterative', device='cpu')
    assert kc.same_bits(it, cbk.host_iterative_kmeans(X, K)) and len(rec.calls) == 1 + 3 * (K - 1)
    streams = [X, X[:200] * 0.5, X[50:] + 1.0]
    rng = np.random.default_rng(3)
    want = tuple(cbk.host_build_codebook(x, k, mode='raw', rng=rng) for x, k in zip(streams, (5, 3, 4)))
    got = cbk.build_codebooks(streams, (5, 3, 4), rng=3, device='cpu')
    assert isinstance(got, tuple) and len(got) == 3 and all(kc.same_bits(a, b) for a, b in zip(got, want))
    got = cbk.build_codebooks(streams, (5, 3, 4), mode='iterative', device='cpu')
    assert all(kc.same_bits(a, cbk.host_iterative_kmeans(x, k)) for a, x, k in zip(got, streams, (5, 3, 4)))


def test_device_codebooks_pass_into_windowed_hac_unchanged(monkeypatch):
    import torch
    KmRecorder(monkeypatch)
    g = kc.golden()['b']
    X = torch.from_numpy(g['data'].copy())
    books = cbk.build_codebooks([X, X], (4, 3), mode='iterative', device='cpu', output='device')
    seen = []
    monkeypatch.setattr(_native, 'hac_count_device', lambda streams, *a, **k: seen.append(list(streams)) or 0)
    monkeypatch.setattr(_native, 'hac_fill_device', lambda *a, **k: None)
    rows = hac.windowed_hac([X, X], books, [(0, 100), (50, 300)], device='cpu', output='device')
    assert rows.shape == (2, 2 * (16 + 9)) and len(seen) == 1
    for (dx, ld, dc, ldc, d, K), book in zip(seen[0], books):
        assert dx == X.data_ptr() and dc == book.data_ptr() and (ldc, d, K) == (3, 3, book.shape[0])


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_every_host_refusal_raises_before_any_native_call(monkeypatch):
    rec = KmRecorder(monkeypatch)
    calls = []
    monkeypatch.setattr(_native, 'kmeans_work_bytes', lambda *a: calls.append(a) or 1 << 20)
    x, c = np.random.default_rng(0).random((30, 4)), np.random.default_rng(1).random((5, 4))

    def refused(fn, *args, **kwargs):
        with pytest.raises(ValueError):
            fn(*args, device='cpu', **kwargs)

    for bad in (np.nan, np.inf, -np.inf):
        xb = x.copy()
        xb[7, 2] = bad
        cb = c.copy()
        cb[0, 0] = bad
        refused(cbk.kmeans, xb, c)
        refused(cbk.kmeans, x, cb)
        refused(cbk.iterative_kmeans, xb, 3)
        refused(cbk.build_codebook, xb, 3)
    refused(cbk.kmeans, x, c[:, :3])                                               # shapes that do not agree
    refused(cbk.kmeans, x.ravel(), c)
    refused(cbk.kmeans, x, c.ravel())
    refused(cbk.kmeans, x[:0], c)
    refused(cbk.kmeans, x, c[:0])                                                  # K < 1
    refused(cbk.iterative_kmeans, x, 0)
    refused(cbk.iterative_kmeans, x, 2.5)
    refused(cbk.build_codebook, x, 0)
    for it in (0, -1, 1.5):
        refused(cbk.kmeans, x, c, iter=it)
        refused(cbk.iterative_kmeans, x, 3, iter=it)
        refused(cbk.build_codebook, x, 3, iter=it)
    wide = np.random.default_rng(2).random((80, 65))
    refused(cbk.iterative_kmeans, wide, 3)                                         # d > 64 needs the Gram call
    refused(cbk.build_codebook, wide, 3)
    refused(cbk.build_codebook, wide, 3, mode='iterative')
    refused(cbk.kmeans, x, np.zeros((13312 // 4 + 1, 4)))                          # K * d beyond the bound
    refused(cbk.iterative_kmeans, x, 13312 // 4 + 1)
    refused(cbk.build_codebook, x[:4], 2)                                          # T <= d: scipy's rank-deficient branch
    refused(cbk.build_codebook, x, 3, mode='kmeans++')
    refused(cbk.build_codebooks, [x, x], (3, 3), mode='other')
    refused(cbk.build_codebooks, [x, x], (3,))
    refused(cbk.kmeans, x, c, output='scipy')
    refused(cbk.iterative_kmeans, x, 3, output='dense')
    refused(cbk.build_codebook, x, 3, output='dense')
    import torch
    refused(cbk.kmeans, torch.from_numpy(x).T, c)                                  # rows that are not contiguous
    refused(cbk.kmeans, torch.from_numpy(x).to(torch.float16), c)
    assert rec.calls == [] and calls == []
