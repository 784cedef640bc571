"""CSR problems over row shards, and the CSC order built on the device (klnmf_upload_csr_rows: csrc/csc.hip.h).

  * the device-built order against the host's np.argsort(kind='stable') order uploaded through klnmf_upload_csr: one fit step
    from each must give the same bits, for f = 1, f > 2^16 (three radix passes), empty rows and columns, no stored entry, one
    column stored in every row of 120 000 rows, in the blocked and the unblocked regime;
  * bad structure refused with KLNMF_ERR_ARG before anything is reordered, and a good upload taken afterwards;
  * groups of CSR contexts on repeated device 0 against one context (f64: the loss to 1e-12, H to 1e-11) and the oracle, fit,
    transform, a shard without stored entries, a stop by tol; the same in f32 within tests/test_sparse_gpu.py's bars;
  * KLdivNMF(device=[0, 0]) on fixture G9, ShardedKLNMF on CSR row blocks over gloo ranks and on a one-rank communicator.
"""
import contextlib
import io
import os
import socket

import numpy as np
import pytest
import scipy.sparse as sp
from numpy.testing import assert_allclose, assert_array_equal

from oracle import klnmf_oracle as orc
from tests import golden_inputs as gi
from tests import sparse_cases as sc

pytestmark = pytest.mark.gpu

F32_BARS = {'fit_loss': 3e-5, 'fit_factor': 3e-4}       # tests/test_sparse_gpu.py: BARS['f32']
F32_FLOOR = float(np.finfo(np.float32).tiny)


def _env_blocks(monkeypatch, blocks):
    monkeypatch.setenv('KLNMF_DEV', '1')
    for name, v in (('KLNMF_SP_CB', blocks and blocks[0]), ('KLNMF_SP_RB', blocks and blocks[1])):
        if v:
            monkeypatch.setenv(name, str(v))
        else:
            monkeypatch.delenv(name, raising=False)


def _host_order_upload(ctx, X, k, cap):
    """The problem through klnmf_upload_csr with the CSC order sorted on the host (the parent's path)."""
    from multimodal_amd import _native
    X = sp.csr_matrix(X, copy=True)
    X.eliminate_zeros()
    X.sort_indices()
    n, f = X.shape
    lib = ctx._lib
    assert lib.klnmf_set_problem_sparse(ctx._h, n, f, k, cap, X.nnz) == 0
    indptr = np.ascontiguousarray(X.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(X.indices, dtype=np.int64)
    data = np.ascontiguousarray(X.data, dtype=np.float64)
    perm = np.argsort(indices, kind='stable').astype(np.int64)
    rows = np.ascontiguousarray(np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))[perm])
    cptr = np.zeros(f + 1, dtype=np.int64)
    np.cumsum(np.bincount(indices, minlength=f), out=cptr[1:])
    p = lambda a: a.ctypes.data_as(_native._c.c_void_p)
    assert lib.klnmf_upload_csr(ctx._h, _native.DT_F64, p(indptr), p(indices), p(data), p(cptr), p(rows), p(perm)) == 0
    ctx.n, ctx.f, ctx.k, ctx.cap, ctx.nnz = n, f, k, cap, X.nnz


def _one_step(ctx, H0, fit=True):
    ctx.set_H(H0)
    ctx.init_W()
    errors, n_done, _ = ctx.run(1, fit, 0.0)
    return ctx.get_W(), ctx.get_H(), errors


def _csc_cases():
    rng = np.random.default_rng(7)
    out = []
    out.append(('f = 1', sc.random_csr(300, 1, 0.6, 1), 3))
    out.append(('f > 2^16', sc.random_csr(400, 70001, 0.001, 2), 6))
    X = sc.random_csr(500, 300, 0.05, 3).tolil()
    X[10:40, :] = 0
    X[:, 100:160] = 0
    out.append(('empty rows and columns', sp.csr_matrix(X), 8))
    out.append(('nnz = 0', sp.csr_matrix((64, 40)), 4))
    n = 120000
    rows = np.arange(n)
    cols = np.full(n, 3)
    extra = rng.integers(0, 40, size=n // 2)
    X = sp.csr_matrix((np.concatenate([rng.random(n) + 0.1, rng.random(n // 2) + 0.1]),
                       (np.concatenate([rows, rng.integers(0, n, size=n // 2)]), np.concatenate([cols, extra]))), shape=(n, 40))
    X.sum_duplicates()
    out.append(('one column in all of 120 000 rows', X, 4))
    return out


@pytest.mark.parametrize('blocks', [None, (2, 3), 'unblocked'])
def test_device_csc_order_is_bit_identical_to_the_host_order(monkeypatch, blocks):
    from multimodal_amd import _native
    _env_blocks(monkeypatch, None if blocks == 'unblocked' else blocks)
    for name, X, k in _csc_cases():
        if blocks == 'unblocked':
            k = 513                                # k > 512: the unblocked kernels read csc_indptr / csc_rows / csc_perm
        H0 = orc.normalize_sum(np.random.default_rng(11).random((k, X.shape[1])) + 0.05, axis=1)
        with _native.Context('f64', device=0) as a, _native.Context('f64', device=0) as b:
            a.set_problem_sparse(X, k, 1)
            _host_order_upload(b, X, k, 1)
            assert a.sparse_blocks() == b.sparse_blocks(), name
            if blocks == 'unblocked' or X.nnz == 0:
                assert a.sparse_blocks() == (0, 0), name
            elif blocks is not None:
                assert a.sparse_blocks() == (min(blocks[0], (X.shape[1] + 63) // 64), min(blocks[1], (X.shape[0] + 63) // 64)), name
            Wa, Ha, ea = _one_step(a, H0)
            Wb, Hb, eb = _one_step(b, H0)
        assert_array_equal(ea, eb, err_msg=name)
        assert_array_equal(Wa, Wb, err_msg=name)
        assert_array_equal(Ha, Hb, err_msg=name)
        assert np.isfinite(Ha).all(), name


def test_bad_structure_is_refused_and_a_good_upload_follows(monkeypatch):
    from multimodal_amd import _native
    _env_blocks(monkeypatch, (2, 2))
    X = sc.random_csr(301, 263, 0.08, 5)
    k = 12
    H0 = orc.normalize_sum(np.random.default_rng(3).random((k, 263)) + 0.05, axis=1)
    indptr = np.ascontiguousarray(X.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(X.indices, dtype=np.int64)
    data = np.ascontiguousarray(X.data, dtype=np.float64)
    row = int(np.flatnonzero(np.diff(indptr) >= 2)[0])
    p0 = int(indptr[row])
    unsorted = indices.copy()
    unsorted[p0], unsorted[p0 + 1] = unsorted[p0 + 1], unsorted[p0]
    too_big = indices.copy()
    too_big[-1] = 263
    negative = indices.copy()
    negative[0] = -1
    huge = indices.copy()
    huge[len(huge) // 2] = 1 << 40
    bad_ptr = indptr.copy()
    bad_ptr[5] = bad_ptr[6] + 1
    with _native.Context('f64', device=0) as ctx, _native.Context('f64', device=0) as ref:
        assert ctx._lib.klnmf_set_problem_sparse(ctx._h, 301, 263, k, 1, X.nnz) == 0
        ptr = lambda a: a.ctypes.data_as(_native._c.c_void_p)
        upload = lambda ip, idx: ctx._lib.klnmf_upload_csr_rows(ctx._h, _native.DT_F64, ptr(ip), ptr(idx), ptr(data))
        for ip, idx in ((indptr, unsorted), (indptr, too_big), (indptr, negative), (indptr, huge), (bad_ptr, indices)):
            assert upload(ip, idx) == _native.ERR_ARG
            assert b'klnmf_upload_csr_rows' in ctx._lib.klnmf_last_error()
        assert upload(indptr, indices) == 0
        ctx.n, ctx.f, ctx.k, ctx.cap, ctx.nnz = 301, 263, k, 1, X.nnz
        ref.set_problem_sparse(X, k, 1)
        got, want = _one_step(ctx, H0), _one_step(ref, H0)
    for g, w in zip(got, want):
        assert_array_equal(g, w)


# ---- groups of CSR contexts on device 0 ---------------------------------------------------------------------------------------
def _csr_group_fit(X, H0, k, iters, tol, precision, bounds, fit=True, H_loop=None):
    from multimodal_amd import _native
    n, f = X.shape
    ctxs = []
    try:
        for r0, r1 in bounds:
            c = _native.Context(precision, device=0)
            ctxs.append(c)
            c.set_problem_sparse(X[r0:r1], k, iters)
            c.set_H(H0)
            c.init_W()
            if H_loop is not None:
                c.set_H(H_loop)
        with _native.Group(ctxs) as g:
            errors, n_done, stopped = g.run(n, iters, fit, tol)
        dt = np.float64 if precision == 'f64' else np.float32
        W = np.vstack([c.get_W(dtype=dt) for c in ctxs])
        Hs = [c.get_H(dtype=dt) for c in ctxs]
        return W, Hs, np.array(errors)
    finally:
        for c in ctxs:
            c.close()


def _csr_single_fit(X, H0, k, iters, tol, precision, fit=True, H_loop=None):
    from multimodal_amd import _native
    n, f = X.shape
    with _native.Context(precision, device=0) as c:
        c.set_problem_sparse(X, k, iters)
        c.set_H(H0)
        c.init_W()
        if H_loop is not None:
            c.set_H(H_loop)
        errors, _, _ = c.run(iters, fit, tol * n * f)
        dt = np.float64 if precision == 'f64' else np.float32
        return c.get_W(dtype=dt), c.get_H(dtype=dt), np.array(errors)


def _group_data(precision):
    X = sc.random_csr(1500, 700, 0.02, 31)
    X = sp.vstack([X, sc.random_csr(300, 700, 0.2, 32), sp.csr_matrix((40, 700))], format='csr')     # a dense tail, empty rows
    k = 16
    H0 = orc.normalize_sum(np.random.default_rng(33).random((k, 700)) + 0.05, axis=1)
    if precision == 'f32':
        return X.astype(np.float32), H0.astype(np.float32), sc.as_f32(X), sc.as_f32(H0), k
    return X, H0, X, H0, k


def _plans(X, N):
    """('balanced', csr_row_partition) and ('ragged', N - 1 uneven shards of the stored rows + one of the 40 empty rows)."""
    from multimodal_amd.distributed import csr_row_partition
    yield 'balanced', csr_row_partition(X.indptr, N)
    n = X.shape[0]
    cuts = [0] + [(n - 40) * i * i // ((N - 1) * (N - 1)) for i in range(1, N - 1)] + [n - 40, n]
    bounds = [(cuts[i], cuts[i + 1]) for i in range(N)]
    assert X[bounds[-1][0]:].nnz == 0
    yield 'ragged', bounds


def _check_rel(name, what, got, ref, bar, floor=0.0):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    scale = np.maximum(np.abs(ref), floor)
    nz = scale > 0
    assert np.all(got[~nz] == 0), '%s: %s has non-zeros where the reference is 0' % (name, what)
    err = float(np.max(np.abs(got[nz] - ref[nz]) / scale[nz])) if nz.any() else 0.0
    assert err <= bar, '%s: %s differs by %.3e relative (bar %.0e)' % (name, what, err, bar)


@pytest.mark.parametrize('N', [2, 3, 4])
def test_csr_group_f64_equals_one_context_and_the_oracle(N):
    X, H0, Xr, Hr, k = _group_data('f64')
    n = X.shape[0]
    iters = 12
    W1, H1, e1 = _csr_single_fit(X, H0, k, iters, 0.0, 'f64')
    Wo, Ho, eo = orc.sparse_fit_transform(X, k, H0, max_iter=iters, tol=0)
    for plan_name, bounds in _plans(X, N):
        name = '%s N=%d' % (plan_name, N)
        W, Hs, e = _csr_group_fit(X, H0, k, iters, 0.0, 'f64', bounds)
        for H in Hs[1:]:
            assert_array_equal(H, Hs[0])                      # replicas bit-identical
        assert len(e) == iters
        _check_rel(name, 'losses', e, e1, 1e-12)
        _check_rel(name, 'H', Hs[0], H1, 1e-11)
        _check_rel(name, 'W', W, W1, 1e-11)
        assert_allclose(e, eo, rtol=1e-9)
        assert_allclose(Hs[0], Ho, rtol=1e-9, atol=1e-300)
        assert_allclose(W, Wo, rtol=1e-9, atol=1e-300)
        # transform on the learnt dictionary: the loss alone is exchanged, H stays
        Wt1, Ht1, et1 = _csr_single_fit(X, H0, k, 6, 0.0, 'f64', fit=False, H_loop=H1)
        Wt, Hts, et = _csr_group_fit(X, H0, k, 6, 0.0, 'f64', bounds, fit=False, H_loop=H1)
        assert all(np.array_equal(H, H1) for H in Hts)
        _check_rel(name + ' transform', 'losses', et, et1, 1e-12)
        _check_rel(name + ' transform', 'W', Wt, Wt1, 1e-11)
        Wto, _, eto = orc.sparse_fit_transform(X, k, H0, max_iter=6, tol=0, fit=False, components=H1)
        assert_allclose(et, eto, rtol=1e-9)
        assert_allclose(Wt, Wto, rtol=1e-9, atol=1e-300)


def test_csr_group_stops_by_tol_where_one_context_does():
    X, H0, _, _, k = _group_data('f64')
    from multimodal_amd.distributed import csr_row_partition
    tol = 2e-4
    _, H1, e1 = _csr_single_fit(X, H0, k, 300, tol, 'f64')
    assert 2 < len(e1) < 300
    _, _, eo = orc.sparse_fit_transform(X, k, H0, max_iter=300, tol=tol)
    assert len(eo) == len(e1)
    for N in (2, 4):
        _, Hs, e = _csr_group_fit(X, H0, k, 300, tol, 'f64', csr_row_partition(X.indptr, N))
        assert len(e) == len(e1), (N, len(e), len(e1))
        _check_rel('tol N=%d' % N, 'losses', e, e1, 1e-12)
        _check_rel('tol N=%d' % N, 'H', Hs[0], H1, 1e-11)


@pytest.mark.parametrize('N', [2, 4])
def test_csr_group_f32_within_the_sparse_bars(N):
    X, H0, Xr, Hr, k = _group_data('f32')
    iters = 10
    Wr, Hr_, er = sc.ref_fit(Xr, Hr, iters)
    for plan_name, bounds in _plans(X, N):
        name = 'f32 %s N=%d' % (plan_name, N)
        W, Hs, e = _csr_group_fit(X, H0, k, iters, 0.0, 'f32', bounds)
        assert W.dtype == np.float32
        for H in Hs[1:]:
            assert_array_equal(H, Hs[0])
        assert len(e) == iters
        _check_rel(name, 'losses', e, er, F32_BARS['fit_loss'])
        _check_rel(name, 'W', W, Wr, F32_BARS['fit_factor'], F32_FLOOR)
        _check_rel(name, 'H', Hs[0], Hr_, F32_BARS['fit_factor'], F32_FLOOR)
        Wt, _, et = _csr_group_fit(X, H0, k, 5, 0.0, 'f32', bounds, fit=False, H_loop=Hs[0])
        Wtr, _, etr = sc.ref_fit(Xr, Hr, 5, fit=False, components=Hs[0].astype(np.float64))
        _check_rel(name + ' transform', 'losses', et, etr, F32_BARS['fit_loss'])
        _check_rel(name + ' transform', 'W', Wt, Wtr, F32_BARS['fit_factor'], F32_FLOOR)


def test_mixed_csr_and_dense_group_is_refused_and_contexts_stay_usable():
    from multimodal_amd import _native
    X, H0, _, _, k = _group_data('f64')
    A = X[:800]
    D = np.asarray(X[800:].toarray())
    with _native.Context('f64', device=0) as a, _native.Context('f64', device=0) as d:
        a.set_problem_sparse(A, k, 3)
        d.set_problem(D.shape[0], D.shape[1], k, 3)
        d.upload_V(D)
        for pair in ((a, d), (d, a)):
            with pytest.raises(_native.NativeError) as ei:
                _native.Group(list(pair))
            assert ei.value.code == _native.ERR_ARG and 'all dense or all CSR' in str(ei.value)
        for c, (W_o, H_o, e_o) in ((a, orc.sparse_fit_transform(A, k, H0, max_iter=3, tol=0)),
                                   (d, orc.fit_transform(D, k=k, H0=H0, max_iter=3, tol=0))):
            c.set_H(H0)
            c.init_W()
            errors, n_done, _ = c.run(3, True, 0.0)
            assert_allclose(errors, e_o, rtol=1e-10)
            assert_allclose(c.get_H(), H_o, rtol=1e-9, atol=1e-300)


def test_g9_through_kldivnmf_on_a_device_list(monkeypatch):
    """Fixture G9 (the reference's CSR branch: an empty row and an empty column) through KLdivNMF(device=[0, 0]) with the
    threshold lowered so that it shards, held to the bounds of the single-device G9 test (tests/test_gpu_parity.py)."""
    from multimodal_amd.lib import nmf
    g = gi.load('g9_sparse_fit')
    dense, H0 = gi.g9_inputs(g)
    X = sp.csr_matrix(dense)
    k = int(g['k'])
    monkeypatch.setattr(nmf, 'CSR_SHARD_MIN_NNZ', max(1, X.nnz // 3))
    assert len(nmf.csr_shard_plan(X.indptr, (0, 0))) == 2

    def fit(max_iter, tol, precision='f64', device=(0, 0)):
        m = nmf.KLdivNMF(n_components=k, max_iter=max_iter, tol=tol, precision=precision, device=list(device))
        m._init_dictionary = H0
        buf = io.StringIO()
        with contextlib.redirect_stderr(buf):
            W, errors = m.fit_transform(X, return_errors=True)
        return m, W, np.array(errors), buf.getvalue()

    m, W, errors, note = fit(12, 0)
    assert 'runs on one device' not in note
    assert m.last_fp8_report['shards'] == 2
    assert_allclose(errors, g['errors'], rtol=1e-11)
    assert_allclose(W, g['W'], rtol=1e-9, atol=1e-300)
    assert_allclose(m.components_, g['H'], rtol=1e-9, atol=1e-300)
    Wt = m.transform(X[:20])                      # 20 rows: below the threshold, one device
    assert_allclose(Wt, g['Wt'], rtol=1e-9, atol=1e-300)
    m2, W2, e2, _ = fit(300, 1e-4)
    assert len(e2) == len(g['errors_tol'])
    assert_allclose(e2, g['errors_tol'], rtol=1e-10)
    assert_allclose(m2.components_, g['H_tol'], rtol=1e-8, atol=1e-300)
    m3, W3, e3, _ = fit(12, 0, precision='f32')
    assert W3.dtype == np.float64                 # (X and H0 are float64: the output follows the CSR rule)
    assert_allclose(e3, g['errors'], rtol=2e-4)
    # the sharded transform of the whole matrix equals the single device's
    Wt_all = m.transform(X)
    m1 = nmf.KLdivNMF(n_components=k, max_iter=12, tol=0, precision='f64', device=0)
    m1.components_ = m.components_
    assert_allclose(Wt_all, m1.transform(X), rtol=1e-11, atol=1e-300)


# ---- ShardedKLNMF on CSR row blocks ---------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _sharded_data():
    X = sp.vstack([sc.random_csr(700, 300, 0.03, 41), sc.random_csr(120, 300, 0.3, 42)], format='csr')
    k = 10
    H0 = orc.normalize_sum(np.random.default_rng(43).random((k, 300)) + 0.05, axis=1)
    return X, H0, k


def _csr_worker(rank, world, port, iters, out_dir):
    import torch
    import torch.distributed as dist
    from multimodal_amd.distributed import ShardedKLNMF, csr_row_partition
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        X, H0, k = _sharded_data()
        r0, r1 = csr_row_partition(X.indptr, world)[rank]
        m = ShardedKLNMF(X.shape[0], r1 - r0, X.shape[1], k, max_iter=iters, precision='f64', csr=X[r0:r1])
        for call in (lambda: m.set_v_max(1.0), lambda: m.upload_V(np.zeros((r1 - r0, X.shape[1])))):
            try:
                call()
                raise AssertionError('a CSR shard took a dense upload')
            except ValueError:
                pass
        m.set_H(H0)
        m.init_W()
        errors, n_done, stopped = m.run(iters, fit=True, tol=0.0)
        W = m.gather_W()
        np.savez(os.path.join(out_dir, 'r%d.npz' % rank), W=W, H=m.get_H(), errors=np.array(errors))
        m.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('world', [2, 4])
def test_sharded_csr_over_gloo_ranks_equals_the_oracle(tmp_path, world):
    import torch.multiprocessing as mp
    iters = 8
    mp.spawn(_csr_worker, args=(world, _free_port(), iters, str(tmp_path)), nprocs=world, join=True)
    X, H0, k = _sharded_data()
    Wo, Ho, eo = orc.sparse_fit_transform(X, k, H0, max_iter=iters, tol=0)
    res = [np.load(os.path.join(str(tmp_path), 'r%d.npz' % r)) for r in range(world)]
    for r in res[1:]:
        assert_array_equal(res[0]['H'], r['H'])
        assert_array_equal(res[0]['errors'], r['errors'])
    for r in res:
        assert_allclose(r['errors'], eo, rtol=1e-9)
        assert_allclose(r['H'], Ho, rtol=1e-9, atol=1e-300)
        assert_allclose(r['W'], Wo, rtol=1e-9, atol=1e-300)


def test_sharded_csr_native_collective_on_a_one_rank_communicator(monkeypatch):
    """collective='native' with KLNMF_COMM_SINGLE=1: the collective branch of klnmf_run_sharded (and of klnmf_loop_begin /
    klnmf_run_more) on a CSR shard; a one-rank all-reduce is the identity, so the result is the single context's bit for bit."""
    from multimodal_amd.distributed import ShardedKLNMF
    monkeypatch.setenv('KLNMF_COMM_SINGLE', '1')
    X, H0, k = _sharded_data()
    iters = 6
    W1, H1, e1 = _csr_single_fit(X, H0, k, iters, 0.0, 'f64')
    m = ShardedKLNMF(X.shape[0], X.shape[0], X.shape[1], k, max_iter=iters, precision='f64', collective='native', csr=X)
    try:
        assert m.rccl_ranks() == 1
        m.set_H(H0)
        m.init_W()
        errors, n_done, stopped = m.run(iters, fit=True, tol=0.0)
        assert n_done == iters and not stopped
        assert_array_equal(np.array(errors), e1)
        assert_array_equal(m.get_H(), H1)
        assert_array_equal(m.gather_W(), W1)
        # the same loop in parts (klnmf_loop_begin / klnmf_run_more on the communicator)
        m.set_H(H0)
        m.init_W()
        m.begin()
        m.iterate_many(iters, fit=True)
        errors2, _, _ = m.end()
        assert_array_equal(np.array(errors2), e1)
        assert_array_equal(m.get_H(), H1)
    finally:
        m.close()
