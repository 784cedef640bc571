"""The CSR kernels (multimodal_amd/csrc/sparse.hip.h, sparseb.hip.h) against the fp64 reference in every dispatch regime.

Driven through `_native.Context` directly, so that every test can assert which kernels ran (`sparse_blocks()`:
KLNMF_Q_SP_COL_BLOCKS / KLNMF_Q_SP_ROW_BLOCKS):
  * every component chunk of the blocked kernels (KC = 1, 2, 4 with a dead fourth chunk, 4, 8; the KEEP form and the
    second-gather form with full and ragged trips) in one column block and one row block;
  * the unblocked kernels k_sp_q_anyk / k_sp_w / k_sp_n (k > 512, and a matrix with no stored entries);
  * 2, 3 and 7 column and row blocks forced through KLNMF_SP_CB / KLNMF_SP_RB (development switches, read at
    set_problem_sparse; conftest sets KLNMF_DEV=1), on block widths that are not multiples of 64, each compared with the
    reference and with the same problem in one block of each kind;
  * blocks chosen by the size rule (>= 2 of each kind), the segmented H rule and loss row sums (f >= 16 384), the
    transform (fit = False), the loss evaluation alone and a caller's eps.
Matrices come from tests/sparse_cases.py, whose cells hit the edges of the kernels' trips; each test checks that they do.

Bars (relative, element by element; an exact zero of the reference must be an exact zero):
  f64  single steps 1e-12; fits: losses 1e-10, W and H 1e-9; blocked against one block of each kind 1e-12.
  f32  (the reference fed the fp32-rounded inputs, so input rounding is not counted) steps and fit losses 3e-5, fit W and H
       3e-4 (1e-3 for k >= 400, below), relative to max(|reference|, the smallest normal fp32 number).  The floor is there because ten multiplicative
       updates drive some coefficients to 1e-70 .. 1e-110 in fp64, which fp32 holds as 0: without it those entries measured
       a relative error of exactly 1 in every fp32 fit, the rest stayed within the bar.
       Measured on the MI355X: fp32 single steps <= 1.3e-6 and fp32 fit losses <= 5e-7 in every case; fp32 fit factors
       within 3e-4 up to k = 200, but 3.3e-4 (k = 400, 2 x 3 blocks), 4.1e-4 (k = 513) and 4.7e-4 (k = 600) beyond.  The
       same cases hold 1e-12 per step and 1e-9 per fit in fp64, and their fp32 steps are 20x inside their bar, so no term
       is wrong: ten fp32 iterations amplify the per-step rounding, more so with more components.  The fp32 fit-factor bar
       at k >= 400 is therefore 1e-3 (F32_FIT_FACTOR_LARGE_K); every other bar is the stated one.
The measured worst errors are printed after each test (pytest -v) and are in each assertion message.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from multimodal_amd import _native
from tests import sparse_cases as sc

pytestmark = pytest.mark.gpu

BARS = {'f64': {'step': 1e-12, 'fit_loss': 1e-10, 'fit_factor': 1e-9},
        'f32': {'step': 3e-5, 'fit_loss': 3e-5, 'fit_factor': 3e-4}}
SAME_PROBLEM_ONE_BLOCK = 1e-12
F32_FIT_FACTOR_LARGE_K = 1e-3        # fp32 fits, W and H, k >= 400 (module docstring)

FLOOR = {'f64': 0.0, 'f32': float(np.finfo(np.float32).tiny)}
_MEASURED = []


@pytest.fixture(autouse=True)
def _report_measured(capsys):
    """Prints what the test measured below its line of the verbose output."""
    del _MEASURED[:]
    yield
    with capsys.disabled():
        for line in _MEASURED:
            print('\n' + line, end='')
        if _MEASURED:
            print()


def worst_rel(got, ref, floor=0.0):
    """max |got - ref| / max(|ref|, floor); with floor = 0 an exact zero of the reference must be one in `got` (inf
    otherwise).  inf if `got` is not finite."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.all(np.isfinite(got)):
        return float('inf')
    scale = np.maximum(np.abs(ref), floor)
    zero = scale == 0
    if np.any(got[zero] != 0):
        return float('inf')
    if zero.all():
        return 0.0
    return float(np.max(np.abs(got[~zero] - ref[~zero]) / scale[~zero]))


def check(case, what, got, ref, bar, floor=0.0):
    err = worst_rel(got, ref, floor)
    _MEASURED.append('    %-40s %-7s %.2e  (bar %.0e)' % (case, what, err, bar))
    assert err <= bar, '%s: %s differs from the reference by %.3e relative (bar %.0e)' % (case, what, err, bar)
    return err


@functools.lru_cache(maxsize=None)
def designed(n, f, cb, rb, seed):
    X = sc.designed_csr(n, f, cb, rb, seed)
    rows, cols = sc.cell_counts(X, cb, rb)
    assert set(sc.ROW_CELLS) <= rows and set(sc.COL_CELLS) <= cols, (sorted(rows), sorted(cols))
    lengths = sc.row_lengths(X)
    assert (lengths == 0).any() and (lengths == 1).any()
    return X


def open_problem(monkeypatch, prec, X, k, cap, blocks):
    """A context with CSR X uploaded; blocks = (cb, rb) forced through the development switches, or None: the size rule."""
    monkeypatch.setenv('KLNMF_DEV', '1')
    for name, v in (('KLNMF_SP_CB', blocks and blocks[0]), ('KLNMF_SP_RB', blocks and blocks[1])):
        if v:
            monkeypatch.setenv(name, str(v))
        else:
            monkeypatch.delenv(name, raising=False)
    ctx = _native.Context(prec)
    ctx.set_problem_sparse(X.astype(np.float32) if prec == 'f32' else X, k, cap)
    return ctx


def inputs(prec, X, *arrays):
    """X and the factors as the kernels of `prec` see them, in fp64 (the reference's inputs), and the factors to upload."""
    if prec == 'f64':
        return (X,) + arrays, arrays
    return (sc.as_f32(X),) + tuple(sc.as_f32(a) for a in arrays), tuple(a.astype(np.float32) for a in arrays)


def gpu_step(ctx, W, H, eps=None, fit=True):
    """(loss, q in CSR order, W_new, H_new) of one update on the device: klnmf_error (the loss pass alone), then
    klnmf_step_Q / _W / _H."""
    ctx.set_H(H)
    ctx.set_W(W)
    if eps is not None:
        ctx.set_ratio_eps(eps)
    loss = ctx.error()
    ctx.step_Q()
    q = ctx.get_Q_values()
    ctx.step_W()
    Wn = ctx.get_W()
    Hn = None
    if fit:
        ctx.step_H()
        Hn = ctx.get_H()
    return loss, q, Wn, Hn


def gpu_fit(ctx, H0, iters, fit=True, components=None):
    ctx.set_H(H0)
    ctx.init_W()                                   # W0 = X . H0^T (nmf.py:156)
    if not fit:
        ctx.set_H(components)
    errors, n_done, _ = ctx.run(iters, fit, 0.0)
    assert n_done == len(errors)
    return ctx.get_W(), ctx.get_H(), np.array(errors)


def check_step(case, prec, got, ref, fit=True):
    bar = BARS[prec]['step']
    check(case, 'loss', got[0], ref[0], bar)
    check(case, 'Q', got[1], ref[1], bar, FLOOR[prec])
    check(case, 'W rule', got[2], ref[2], bar, FLOOR[prec])
    if fit:
        check(case, 'H rule', got[3], ref[3], bar, FLOOR[prec])


def check_fit(case, prec, got, ref):
    W, H, errors = got
    Wr, Hr, er = ref
    assert len(errors) == len(er), '%s: %d iterations recorded, the reference %d' % (case, len(errors), len(er))
    check(case, 'losses', errors, er, BARS[prec]['fit_loss'])
    bar = F32_FIT_FACTOR_LARGE_K if prec == 'f32' and Hr.shape[0] >= 400 else BARS[prec]['fit_factor']
    check(case, 'W', W, Wr, bar, FLOOR[prec])
    check(case, 'H', H, Hr, bar, FLOOR[prec])


PRECS = ['f64', 'f32']
SMALL = (301, 263)           # n, f: 150 odd rows, 132 even columns for cells of up to 65 entries; n not a multiple of 32


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('k', [1, 64, 65, 128, 129, 192, 193, 256, 257, 512])
def test_every_component_chunk_in_one_block(monkeypatch, prec, k):
    """KC = 1 (k <= 64), 2 (65-128, the KEEP form with 16 entries per trip), 4 (129-256; 129-192 with a dead fourth chunk)
    and 8 (257-512): the fused ratio / W-rule pass, the loss pass and the H numerator, one step in each precision."""
    n, f = SMALL
    X = designed(n, f, 1, 1, seed=11)
    W, H = sc.factors(n, f, k, seed=k)
    (Xr, Wr, Hr), (Wu, Hu) = inputs(prec, X, W, H)
    with open_problem(monkeypatch, prec, X, k, 1, (1, 1)) as ctx:
        assert ctx.sparse_blocks() == (1, 1)
        got = gpu_step(ctx, Wu, Hu)
    check_step('chunks %s k=%d (1, 1)' % (prec, k), prec, got, sc.ref_step(Xr, Wr, Hr))


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('k', [513, 600])
def test_unblocked_kernels_beyond_k_512(monkeypatch, prec, k):
    """k_sp_q_anyk, k_sp_w and k_sp_n (more components than threads of a block: their component loop): one step and a
    10-iteration fit."""
    n, f = SMALL
    X = designed(n, f, 1, 1, seed=12)
    W, H = sc.factors(n, f, k, seed=k)
    (Xr, Wr, Hr), (Wu, Hu) = inputs(prec, X, W, H)
    case = 'unblocked %s k=%d (0, 0)' % (prec, k)
    with open_problem(monkeypatch, prec, X, k, 10, None) as ctx:
        assert ctx.sparse_blocks() == (0, 0)
        check_step(case, prec, gpu_step(ctx, Wu, Hu), sc.ref_step(Xr, Wr, Hr))
        check_fit(case, prec, gpu_fit(ctx, Hu, 10), sc.ref_fit(Xr, Hr, 10))


FORCED = [(2, 3), (3, 7), (7, 2)]
BLOCKED = (1001, 1000)       # block widths 500 / 334 / 143 columns and 501 / 334 / 143 rows: none a multiple of 64


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('k', [40, 100, 200, 400])
@pytest.mark.parametrize('blocks', FORCED, ids=lambda b: 'cb%d-rb%d' % b)
def test_forced_blocks(monkeypatch, prec, k, blocks):
    """Several column blocks (slabs G[b] summed by k_spb_wrule) and row blocks (slabs NT[rb] summed and transposed by
    k_spb_numer), block pointers at edges that are not multiples of 64, empty cells: one step and a 10-iteration fit
    against the reference; in f64 the step also against the same problem in one block of each kind (summation order)."""
    n, f = BLOCKED
    X = designed(n, f, blocks[0], blocks[1], seed=13)
    W, H = sc.factors(n, f, k, seed=k)
    (Xr, Wr, Hr), (Wu, Hu) = inputs(prec, X, W, H)
    case = 'forced %s k=%d %s' % (prec, k, blocks)
    with open_problem(monkeypatch, prec, X, k, 10, blocks) as ctx:
        assert ctx.sparse_blocks() == blocks
        step = gpu_step(ctx, Wu, Hu)
        check_step(case, prec, step, sc.ref_step(Xr, Wr, Hr))
        check_fit(case, prec, gpu_fit(ctx, Hu, 10), sc.ref_fit(Xr, Hr, 10))
    if prec == 'f64':
        with open_problem(monkeypatch, prec, X, k, 1, (1, 1)) as one:
            assert one.sparse_blocks() == (1, 1)
            ref1 = gpu_step(one, Wu, Hu)
        for what, a, b in zip(('loss', 'Q', 'W rule', 'H rule'), step, ref1):
            check(case + ' vs (1, 1)', what, a, b, SAME_PROBLEM_ONE_BLOCK)


def test_blocks_chosen_by_the_size_rule(monkeypatch):
    """No switches: at 7000 x 7000, 4 % stored, k = 64 in f64 the rule takes 2 column and 2 row blocks (3 MiB of H^T / W
    per block, >= 128 entries per CSR cell, >= 32 per CSC cell).  3 iterations against the chunked reference."""
    n = f = 7000
    k = 64
    X = sc.random_csr(n, f, 0.04, seed=14)
    _, H0 = sc.factors(n, f, k, seed=15)
    with open_problem(monkeypatch, 'f64', X, k, 3, None) as ctx:
        cb, rb = ctx.sparse_blocks()
        assert cb >= 2 and rb >= 2, (cb, rb)
        check_fit('size rule f64 k=64 (%d, %d)' % (cb, rb), 'f64', gpu_fit(ctx, H0, 3), sc.ref_fit(X, H0, 3))


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('k', [40, 300])
def test_long_dictionary_rows(monkeypatch, prec, k):
    """f = 20 001: the H rule and the loss term's row sums of H in 5 segments of 4096 (k_sp_hsum_part, k_update_H_part;
    the last segment ragged), 5-iteration fit."""
    n, f = 150, 20001
    X = sc.random_csr(n, f, 0.005, seed=16)
    _, H0 = sc.factors(n, f, k, seed=k)
    (Xr, Hr), (Hu,) = inputs(prec, X, H0)
    with open_problem(monkeypatch, prec, X, k, 5, None) as ctx:
        assert ctx.sparse_blocks() == (1, 1)
        check_fit('long rows %s k=%d (1, 1)' % (prec, k), prec, gpu_fit(ctx, Hu, 5), sc.ref_fit(Xr, Hr, 5))


@pytest.mark.parametrize('prec', PRECS)
def test_no_stored_entries(monkeypatch, prec):
    """An all-zero 70 x 50 CSR matrix runs the unblocked kernels: W = H = 0 and every loss 0, as in the reference."""
    X = sp.csr_matrix((70, 50), dtype=np.float64)
    _, H0 = sc.factors(70, 50, 6, seed=17)
    (Xr, Hr), (Hu,) = inputs(prec, X, H0)
    with open_problem(monkeypatch, prec, X, 6, 10, None) as ctx:
        assert ctx.sparse_blocks() == (0, 0)
        W, H, errors = gpu_fit(ctx, Hu, 10)
    Wr, Hr_, er = sc.ref_fit(Xr, Hr, 10)
    assert len(errors) == len(er) == 10
    assert np.all(errors == 0) and np.all(W == 0) and np.all(H == 0)
    assert np.all(np.asarray(er) == 0) and np.all(Wr == 0) and np.all(Hr_ == 0)


@pytest.mark.parametrize('prec', PRECS)
def test_transform_loss_alone_and_eps_on_blocks(monkeypatch, prec):
    """On a forced-block problem (3 column, 2 row blocks, k = 100): a transform (fit = False, the dictionary held), the
    loss evaluation alone (SPB_LOSS) and one step with eps = 1e-5, the reference given the same eps."""
    n, f = BLOCKED
    k, blocks = 100, (3, 2)
    X = designed(n, f, blocks[0], blocks[1], seed=18)
    W, H = sc.factors(n, f, k, seed=19)
    (Xr, Wr, Hr), (Wu, Hu) = inputs(prec, X, W, H)
    bar = BARS[prec]['step']
    case = 'transform/eps %s k=%d %s' % (prec, k, blocks)
    with open_problem(monkeypatch, prec, X, k, 10, blocks) as ctx:
        assert ctx.sparse_blocks() == blocks
        ctx.set_H(Hu)
        ctx.set_W(Wu)
        check(case, 'loss', ctx.error(), sc.ref_step(Xr, Wr, Hr)[0], bar)
        got = gpu_step(ctx, Wu, Hu, eps=1e-5)
        check_step(case + ' eps=1e-5', prec, got, sc.ref_step(Xr, Wr, Hr, eps=1e-5))
        ctx.set_ratio_eps(1e-8)
        Wt, Ht, et = gpu_fit(ctx, Hu, 10, fit=False, components=Hu)
        assert np.array_equal(Ht, Hr)
        check_fit(case + ' fit=False', prec, (Wt, Ht, et), sc.ref_fit(Xr, Hr, 10, fit=False, components=Hr))


def test_unsorted_rows_are_refused_in_the_blocked_regime(monkeypatch):
    """k_spb_blkptr binary-searches the sorted indices of a row: an upload with one row out of order is refused with
    KLNMF_ERR_ARG (the search stays inside the row: nothing is read out of bounds), and the context then takes a good
    upload and computes the right step."""
    n, f = SMALL
    k, blocks = 20, (2, 2)
    X = designed(n, f, blocks[0], blocks[1], seed=20)
    W, H = sc.factors(n, f, k, seed=21)
    with open_problem(monkeypatch, 'f64', X, k, 1, blocks) as ctx:
        assert ctx.sparse_blocks() == blocks
        indptr = np.ascontiguousarray(X.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(X.indices, dtype=np.int64)
        data = np.ascontiguousarray(X.data, dtype=np.float64)
        perm = np.argsort(indices, kind='stable').astype(np.int64)
        csc_rows = np.ascontiguousarray(np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))[perm])
        csc_indptr = np.zeros(f + 1, dtype=np.int64)
        np.cumsum(np.bincount(indices, minlength=f), out=csc_indptr[1:])
        row = int(np.flatnonzero(np.diff(indptr) >= 2)[0])
        bad = indices.copy()
        p = int(indptr[row])
        bad[p], bad[p + 1] = bad[p + 1], bad[p]
        lib = ctx._lib
        ptr = lambda a: a.ctypes.data_as(_native._c.c_void_p)
        upload = lambda idx: lib.klnmf_upload_csr(ctx._h, _native.DT_F64, ptr(indptr), ptr(idx), ptr(data), ptr(csc_indptr),
                                                  ptr(csc_rows), ptr(perm))
        assert upload(bad) == _native.ERR_ARG
        assert b'must be sorted' in lib.klnmf_last_error()
        assert upload(indices) == 0
        got = gpu_step(ctx, W, H)
    check_step('refusal then good upload f64 k=20 (2, 2)', 'f64', got, sc.ref_step(X, W, H))
