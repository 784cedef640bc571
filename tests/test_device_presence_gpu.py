"""Presence masks on the device-resident experiment path: klnmf_upload_presence_device_rows (csrc/presence.hip.h: k_presence_rows_check,
k_presence_gather) through the C-ABI, and `DeviceDataset(data, presence=[...])` through the public classes.

  1. the gather against the host upload (`Context.upload_presence` of P[idx][:, cols], 1 where the column is -1): f64 and f32
     contexts x float32 and float64 sources x a permutation, reversed rows, repeated rows, a single row, an empty list and a null
     index pointer; 67 x 130, k = 5, bounds [0, 1, 65, 130], a resident mask of 200 rows with ld = 5 and source columns [4, -1, 0].
     The ratio values, W and H after the single steps, the loss record and W and H of a 5-iteration run: np.array_equal.  Two calls
     on row pieces (row0) against one call.
  2. the stride loops: 131 073 rows (one more than kPresGatherMaxBlocks x 256 threads), 16 one-column modalities, f32 -- the
     gather's second trip against the host upload, the index check's by a refusal whose one bad index sits in the last row.
  3. every refusal, each leaving the mask and a 2-iteration fit as they were.
  4. the public path in f64 against `MultimodalLearner` on host slices with `weights=`: bit for bit; a subset without a mask
     against a dataset built without one; in f32 against presence_cases.ref_fit_p within DESIGN.md 7d's bars (losses 3e-5, W and
     H 3e-4, test_presence_gpu's floors).
  5. `perform_one_run(..., presence=)` against the host pipeline: dictionary np.array_equal, every found_* list equal.
  6. the imputation case (tests/device_presence_cases.py): the device's masked fit within the f64 bars (losses 1e-10, W and H 1e-9)
     of the fp64 restatement, and so its error on the absent block.
"""
import functools
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from multimodal_amd import _native
from multimodal_amd import device_experiment as de
from multimodal_amd.device_data import DeviceDataset, DeviceEvaluation
from multimodal_amd.learner import MultimodalLearner
from multimodal_amd.lib import nmf
from tests import device_presence_cases as dc
from tests import exact_cases as ec
from tests import presence_cases as pc
from tests.test_exact_gpu import cu_count, open_problem
from tests.test_sparse_gpu import _MEASURED, _report_measured  # noqa: F401  (the autouse fixture prints what was measured)
from tests.test_weighted_gpu import check_fit, gpu_fit, gpu_step

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, F, K = 67, 130, 5
BOUNDS = [0, 1, 65, 130]
SRC_ROWS, LD, SRC_COLS = 200, 5, [4, -1, 0]
RUN = 5


def _rows():
    rng = np.random.default_rng(9)
    return {
        'permutation': rng.permutation(SRC_ROWS)[:N],
        'reversed': np.arange(100, 100 + N)[::-1].copy(),
        'repeats': rng.integers(0, 12, N),
        'single': np.array([17]),
        'empty': np.array([], dtype=np.int64),
        'null': None,
    }


ROWS = _rows()


@functools.lru_cache(maxsize=None)
def problem():
    """(V, W, H, R): the data and factors, and the resident mask (200 x 5: distinct values, exact 0s and 1s)."""
    V = ec.data(N, F, seed=N + 7 * F + 13 * K, zero_row=N // 2, zero_col=F // 3)
    W, H = ec.factors(N, F, K, seed=K + 1)
    R = pc.mask(SRC_ROWS, LD, seed=31)
    assert len(np.unique(R[:, [0, 4]])) > SRC_ROWS // 2 and (R[:, [0, 4]] == 0).any() and (R[:, [0, 4]] == 1).any()
    return V, W, H, R


def selected(R, idx, cols):
    """P[idx][:, cols], 1 where the column is -1 -- what the host path uploads."""
    rows = R[:N] if idx is None else R[np.asarray(idx, dtype=np.int64)]
    out = np.ones((rows.shape[0], len(cols)), dtype=R.dtype)
    for m, c in enumerate(cols):
        if c >= 0:
            out[:, m] = rows[:, c]
    return out


def on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def everything(ctx, W, H, iters=RUN):
    """(loss, R, W rule, H rule) of the single steps, then (W, H, losses) of a run."""
    return tuple(gpu_step(ctx, W, H)) + tuple(gpu_fit(ctx, H, iters))


def assert_same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def upload_from_device(ctx, dR, idx, cols=SRC_COLS, bounds=BOUNDS, row0=0, src_rows=SRC_ROWS):
    """One klnmf_upload_presence_device_rows; returns the tensors that must outlive nothing (the call synchronises)."""
    import torch
    if idx is None:
        ctx.upload_presence_device_rows(dR.data_ptr(), dR.dtype == torch.float64, src_rows, dR.stride(0), 0, N, cols, bounds, row0=row0)
        return
    d_idx = on_device(np.asarray(idx, dtype=np.int64)) if len(idx) else torch.zeros(1, dtype=torch.int64, device='cuda')
    ctx.upload_presence_device_rows(dR.data_ptr(), dR.dtype == torch.float64, src_rows, dR.stride(0), d_idx.data_ptr(), len(idx), cols,
                                    bounds, row0=row0)


# ---- 1. the gather against the host upload -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', list(ROWS), ids=list(ROWS))
@pytest.mark.parametrize('src', ['f32', 'f64'], ids=['src-f32', 'src-f64'])
@pytest.mark.parametrize('prec', ['f64', 'f32'])
def test_the_gather_is_the_host_upload_bit_for_bit(monkeypatch, prec, src, rows):
    V, W, H, R = problem()
    idx = ROWS[rows]
    Rs = R.astype(np.float32) if src == 'f32' else R
    dt = np.float64 if prec == 'f64' else np.float32
    Vu, Wu, Hu = (np.asarray(a, dtype=dt) for a in (V, W, H))
    with open_problem(monkeypatch, prec, Vu, K, RUN) as ctx:
        # (no rows: the first upload takes P filled with 1, which the host binding is handed as N rows of ones)
        ctx.upload_presence(selected(Rs, idx, SRC_COLS) if rows != 'empty' else np.ones((N, 3), dtype=Rs.dtype), BOUNDS)
        assert ctx.presence() == 3
        want = everything(ctx, Wu, Hu)
    with open_problem(monkeypatch, prec, Vu, K, RUN) as ctx:
        assert ctx.presence() == 0
        upload_from_device(ctx, on_device(Rs), idx)
        assert ctx.presence() == 3 and not ctx.weighted()
        got = everything(ctx, Wu, Hu)
    assert_same(got, want)
    if rows in ('permutation', 'null'):             # (the mask does act: not the unmasked problem's bits)
        with open_problem(monkeypatch, prec, Vu, K, RUN) as ctx:
            assert not np.array_equal(gpu_step(ctx, Wu, Hu)[2], got[2])


@pytest.mark.parametrize('prec', ['f64', 'f32'])
def test_two_calls_on_row_pieces_are_one_call(monkeypatch, prec):
    V, W, H, R = problem()
    idx = ROWS['permutation']
    dt = np.float64 if prec == 'f64' else np.float32
    Vu, Wu, Hu = (np.asarray(a, dtype=dt) for a in (V, W, H))
    dR = on_device(R)
    with open_problem(monkeypatch, prec, Vu, K, RUN) as ctx:
        upload_from_device(ctx, dR, idx)
        want = everything(ctx, Wu, Hu)
    d_idx = on_device(idx.astype(np.int64))
    with open_problem(monkeypatch, prec, Vu, K, RUN) as ctx:
        # the second piece first: the first call takes P filled with 1, the other fills in the rest
        ctx.upload_presence_device_rows(dR.data_ptr(), True, SRC_ROWS, LD, d_idx.data_ptr() + 8 * 30, N - 30, SRC_COLS, BOUNDS, row0=30)
        piece = gpu_step(ctx, Wu, Hu)
        ctx.upload_presence_device_rows(dR.data_ptr(), True, SRC_ROWS, LD, d_idx.data_ptr(), 30, SRC_COLS, BOUNDS, row0=0)
        got = everything(ctx, Wu, Hu)
    assert_same(got, want)
    assert not np.array_equal(piece[2], want[2])


# ---- 2. the stride loop ----------------------------------------------------------------------------------------------------------------
def test_more_rows_than_the_gathers_grid_holds(monkeypatch):
    header = open(os.path.join(ROOT, 'multimodal_amd', 'csrc', 'presence.hip.h')).read()
    cap = int(re.search(r'kPresGatherMaxBlocks = (\d+);', header).group(1))
    n, M, k = 131073, 16, 2
    assert cap * 256 < n <= (cap + 1) * 256         # past the grid by less than one block: the last row is a second trip's
    rng = np.random.default_rng(4)
    V = ec.data(n, M, seed=3).astype(np.float32)
    W, H = (a.astype(np.float32) for a in ec.factors(n, M, k, seed=6))
    R = pc.mask(n + 7, M, seed=8).astype(np.float32)
    idx = rng.permutation(n + 7)[:n]
    cols = [int(c) for c in rng.permutation(M)]
    cols[5] = -1
    bounds = list(range(M + 1))
    with open_problem(monkeypatch, 'f32', V, k, 1) as ctx:
        ctx.upload_presence(selected(R, idx, cols), bounds)
        want = gpu_step(ctx, W, H)
    with open_problem(monkeypatch, 'f32', V, k, 1) as ctx:
        d_idx = on_device(idx.astype(np.int64))
        dR = on_device(R)
        # the check's own second trip: the one bad index sits in the last row, which only the stride loop reaches (the source is
        # declared one row shorter than it is allocated, so even a kernel that read through the index would read allocated memory)
        bad = np.arange(n, dtype=np.int64)
        bad[n - 1] = n + 6
        d_bad = on_device(bad)
        with pytest.raises(_native.NativeError) as e:
            ctx.upload_presence_device_rows(dR.data_ptr(), False, n + 6, M, d_bad.data_ptr(), n, cols, bounds)
        assert e.value.code == _native.ERR_ARG and 'row index' in str(e.value) and ctx.presence() == 0
        ctx.upload_presence_device_rows(dR.data_ptr(), False, n + 7, M, d_idx.data_ptr(), n, cols, bounds)
        got = gpu_step(ctx, W, H)
    assert_same(got, want)


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(monkeypatch):
    import torch
    V, W, H, R = problem()
    # a row before and a row behind the source are allocated: even a kernel that read through a refused index (-1, src_rows)
    # would read allocated memory
    pad = np.full((1, LD), 0.25)
    dR = on_device(np.vstack([pad, R, pad]))[1:]
    good = ROWS['permutation']

    def refused(ctx, code, word=None, idx=good, cols=SRC_COLS, bounds=BOUNDS):
        with pytest.raises(_native.NativeError) as e:
            upload_from_device(ctx, dR, idx, cols=cols, bounds=bounds)
        assert e.value.code == code and (word is None or word in str(e.value)), str(e.value)

    def bad_calls(ctx):
        over, under = good.copy(), good.copy()
        over[40], under[N - 1] = SRC_ROWS, -1
        refused(ctx, _native.ERR_ARG, 'row index', idx=over)
        refused(ctx, _native.ERR_ARG, 'row index', idx=under)
        refused(ctx, _native.ERR_ARG, 'source column', cols=[4, -1, LD])
        refused(ctx, _native.ERR_ARG, 'source column', cols=[-2, -1, 0])

    with open_problem(monkeypatch, 'f64', V, K, 2) as ctx:
        plain = gpu_fit(ctx, H, 2)
        bad_calls(ctx)                                   # each would have been the first upload: no mask is taken
        with pytest.raises(_native.NativeError) as e:    # a null index pointer reads rows 0 .. rows - 1 of the source
            ctx.upload_presence_device_rows(dR.data_ptr(), True, N - 1, LD, 0, N, SRC_COLS, BOUNDS)
        assert e.value.code == _native.ERR_ARG
        refused(ctx, _native.ERR_ARG, 'bounds', bounds=[0, 1, 65, F - 1])
        assert ctx.presence() == 0 and not ctx.weighted()
        assert_same(gpu_fit(ctx, H, 2), plain)
        upload_from_device(ctx, dR, good)
        assert ctx.presence() == 3
        want = gpu_fit(ctx, H, 2)
        assert not np.array_equal(want[0], plain[0])
        bad_calls(ctx)                                   # no row of P changes
        refused(ctx, _native.ERR_ARG, 'bounds', bounds=[0, 2, 65, F])          # other bounds than the first upload's
        refused(ctx, _native.ERR_ARG, None, cols=[4, 0], bounds=[0, 65, F])    # another count
        assert ctx.presence() == 3
        assert_same(gpu_fit(ctx, H, 2), want)
        # a problem that holds weights
        ctx.clear_weights()
        Om = pc.omega(selected(R, good, SRC_COLS), BOUNDS)
        ctx.upload_weights(Om)
        weighted = gpu_fit(ctx, H, 2)
        refused(ctx, _native.ERR_ARG, 'klnmf_upload_weights')
        assert ctx.weighted() and ctx.presence() == 0
        assert_same(gpu_fit(ctx, H, 2), weighted)
    # a CSR problem
    with _native.Context('f64') as ctx:
        ctx.set_problem_sparse(sp.csr_matrix(V * (V > np.median(V))), K, 2)
        ctx.set_H(H)
        ctx.set_W(W)
        before = ctx.error()
        refused(ctx, _native.ERR_UNSUPP, 'CSR')
        assert ctx.presence() == 0 and ctx.error() == before
    # a 16-bit context
    with _native.Context('f16') as ctx:
        ctx.set_problem(N, F, K, 2)
        ctx.upload_blocks([V])
        refused(ctx, _native.ERR_UNSUPP, 'KLNMF_PREC_F64')
        assert ctx.presence() == 0
        ctx.set_H(H)
        ctx.init_W()
        errors, n_done, _ = ctx.run(2, True, ec.NO_STOP)
        assert n_done == 2 and np.all(np.isfinite(errors))
    torch.cuda.synchronize()


def test_a_context_that_ran_in_a_group_takes_a_mask_again(monkeypatch):
    """The group's loop has ended when klnmf_group_run returns: a mask (from the host or from the device) is accepted afterwards,
    on the same problem and on the next one of a pooled context."""
    V, W, H, R = problem()
    with open_problem(monkeypatch, 'f64', V, K, 2) as ctx:
        ctx.set_H(H)
        ctx.init_W()
        with _native.Group([ctx]) as group:
            group.run(N, 2, True, 0.0)
        upload_from_device(ctx, on_device(R), ROWS['permutation'])
        assert ctx.presence() == 3
        got = gpu_fit(ctx, H, 2)
    with open_problem(monkeypatch, 'f64', V, K, 2) as ctx:
        ctx.upload_presence(selected(R, ROWS['permutation'], SRC_COLS), BOUNDS)
        assert_same(got, gpu_fit(ctx, H, 2))


# ---- 4. the public path ----------------------------------------------------------------------------------------------------------------
N_ALL, DIMS, COEFS, KP, ITERS = 90, [40, 30, 20], [1.0, 0.5, 2.0], 5, 10
MODS = ['a', 'b', 'c']


@functools.lru_cache(maxsize=None)
def public_case():
    rng = np.random.default_rng(21)
    data = [rng.gamma(1.0, 1.0, (N_ALL, d)) + 0.05 for d in DIMS]
    P = pc.mask(N_ALL, 3, seed=17)
    masks = [P[:, 0], None, P[:, 2:3]]                                   # (n,) and (n, 1); the second modality has no mask entry
    rows = np.concatenate([np.arange(80)[::-1], [3, 3, 7, 80]])          # in reverse, with repeats
    H0 = rng.random((KP, sum(DIMS))) + .01
    H0 /= H0.sum(axis=1, keepdims=True)
    return data, P, masks, rows, H0


def host_weights(P, which, rows):
    return [None if w == 1 else P[rows][:, w:w + 1] for w in which]


def host_learner(data, P, rows, H0, iters=ITERS):
    learner = MultimodalLearner(list(MODS), list(DIMS), list(COEFS), KP)
    np.random.seed(3)
    learner.train([x[rows] for x in data], iters, weights=host_weights(P, [0, 1, 2], rows))
    return learner


def test_the_resident_path_is_the_host_path_bit_for_bit(monkeypatch):
    monkeypatch.setenv('KLNMF_PRECISION', 'f64')
    data, P, masks, rows, H0 = public_case()
    host = host_learner(data, P, rows, H0)
    assert host.nmf_train.last_weights_route == 'presence'
    ds = DeviceDataset(data, presence=masks)
    assert ds.resident_bytes() == DeviceDataset(data).resident_bytes() + 8 * N_ALL * 3
    learner = MultimodalLearner(list(MODS), list(DIMS), list(COEFS), KP)
    np.random.seed(3)
    ds.train(learner, rows, ITERS)
    assert learner.nmf_train.last_weights_route == 'presence' and ds.last_weights_route == 'presence'
    assert np.array_equal(learner.dico, host.dico)
    plain = DeviceDataset(data)
    np.random.seed(3)
    unmasked = MultimodalLearner(list(MODS), list(DIMS), list(COEFS), KP)
    plain.train(unmasked, rows, ITERS)
    assert unmasked.nmf_train.last_weights_route is None and not np.array_equal(unmasked.dico, host.dico)
    # the transforms: every masked subset, through both classes
    test_rows = np.array([89, 85, 2, 2, 30, 81])
    ev = DeviceEvaluation(ds, learner, ITERS)
    for mods in (['a'], ['c'], ['a', 'c'], ['c', 'b'], ['a', 'b', 'c']):
        which = [MODS.index(m) for m in mods]
        want = host.reconstruct_internal_multi(mods, [data[w][test_rows] for w in which], ITERS, weights=host_weights(P, which, test_rows))
        got = ds.reconstruct_internal_multi(learner, mods, test_rows, ITERS)
        assert ds.last_weights_route == 'presence' and got.dtype == np.float64
        assert np.array_equal(got, np.asarray(want, dtype=np.float64)), mods
        dev = ev.internal(mods, test_rows).cpu().numpy()
        assert ev.last_weights_route == 'presence' and np.array_equal(dev, got), mods
    # the modality without a mask alone: the unmasked call of a dataset built without a mask
    want = plain.reconstruct_internal(learner, 'b', test_rows, ITERS)
    got = ds.reconstruct_internal(learner, 'b', test_rows, ITERS)
    assert ds.last_weights_route is None and plain.last_weights_route is None and np.array_equal(got, want)
    dev = ev.internal(['b'], test_rows).cpu().numpy()
    assert ev.last_weights_route is None
    assert np.array_equal(dev, DeviceEvaluation(plain, learner, ITERS).internal(['b'], test_rows).cpu().numpy())
    assert np.array_equal(got, host.reconstruct_internal('b', data[1][test_rows], ITERS))


def test_the_resident_path_in_f32_against_the_reference(monkeypatch):
    """The f32 resident blocks are not the host path's bits (fp32 copies of the data): held to the restatement, fed what the
    kernels see -- the fp32-rounded data (the coefficients are powers of two: exact), mask and dictionary."""
    monkeypatch.setenv('KLNMF_PRECISION', 'f32')
    data, P, masks, rows, H0 = public_case()
    n, f = rows.size, sum(DIMS)
    bounds = [0, 40, 70, 90]
    Vr = np.hstack([c * ec.as_f32(x[rows]) for x, c in zip(data, COEFS)])
    Pr = ec.as_f32(np.hstack([P[rows][:, :1], np.ones((n, 1)), P[rows][:, 2:]]))
    _, kchunk, _, wchunk, _, _ = ec.exact_regime(n, f, KP, cu_count(), 4)
    ref = pc.ref_fit_p(Vr, Pr, bounds, ec.as_f32(H0), ITERS, kchunk=kchunk, wchunk=wchunk)
    ds = DeviceDataset(data, presence=masks)
    m = nmf.KLdivNMF(n_components=KP, max_iter=ITERS, tol=0)
    m._init_dictionary = H0
    W, errors = ds._fit_dense(m, [0, 1, 2], rows, COEFS, f, True, return_errors=True)
    assert m.last_weights_route == 'presence' and len(errors) == ITERS
    check_fit('f32 resident masked fit', 'f32', (W, m.components_, np.array(errors)), ref, Vr, pc.omega(Pr, bounds))
    learner = MultimodalLearner(list(MODS), list(DIMS), list(COEFS), KP)
    ds.train(learner, rows, ITERS, init_dictionary=H0)                  # the public call: the same loop
    assert learner.nmf_train.last_weights_route == 'presence' and np.array_equal(learner.dico, m.components_)


# ---- 5. one whole run --------------------------------------------------------------------------------------------------------------------
class _HostData(object):
    """What device_experiment.evaluate / evaluate_internal ask of a dataset, on host slices through the learner's own methods."""

    def __init__(self, data, P, masked):
        self.data, self.P, self.masked = data, P, masked

    def rows_of(self, which, rows):
        return self.data[which][np.asarray(rows, dtype=np.int64), :]

    def reconstruct_internal_multi(self, learner, mods, rows, iterations):
        rows = np.asarray(rows, dtype=np.int64)
        which = [learner.get_index(m) for m in mods]
        weights = [self.P[rows][:, w:w + 1] if self.masked[w] else None for w in which]
        return learner.reconstruct_internal_multi(mods, [self.data[w][rows] for w in which], iterations,
                                                  weights=weights if any(self.masked[w] for w in which) else None)

    def reconstruct_internal(self, learner, mod, rows, iterations):
        return self.reconstruct_internal_multi(learner, [mod], rows, iterations)


@functools.lru_cache(maxsize=None)
def run_case(n_mod):
    """Three classes of 30 samples, paired across the modalities; the last modality absent from a third of the samples."""
    rng = np.random.default_rng(40 + n_mod)
    dims = [24, 18, 14][:n_mod]
    labels = np.repeat(np.arange(3), 30)
    centres = [rng.gamma(1.0, 1.0, (3, d)) + 0.05 for d in dims]
    data = [c[labels] * rng.uniform(0.7, 1.3, (90, d)) for c, d in zip(centres, dims)]
    examples = [0, 30, 60]
    P = np.ones((90, n_mod))
    absent = rng.random(90) < 0.33
    absent[examples] = False
    # weights in (0.5, 1] where the modality is there (some exactly 1), 0 where it is absent and stored as zeros
    P[:, -1] = np.where(absent, 0.0, np.where(rng.random(90) < 0.3, 1.0, rng.uniform(0.5, 1.0, 90)))
    data[-1] = data[-1] * (P[:, -1:] > 0)
    masks = [None] * (n_mod - 1) + [P[:, -1]]
    order = [int(i) for i in rng.permutation(90) if i not in examples]
    # scoring and the choice of test rows are the caller's: rows that have every modality are tested, the absent ones train
    test = [i for i in order if not absent[i]][:20]
    train = [i for i in order if i not in test]
    assert absent[train].sum() >= 15
    return data, dims, labels, P, masks, train, test, examples


@pytest.mark.parametrize('on_device', [True, False], ids=['on-device', 'host-arrays'])
@pytest.mark.parametrize('n_mod', [2, 3], ids=['two', 'three'])
def test_one_whole_run_equals_the_host_pipeline(monkeypatch, n_mod, on_device):
    monkeypatch.setenv('KLNMF_PRECISION', 'f64')
    data, dims, labels, P, masks, train, test, examples = run_case(n_mod)
    mods, coefs, k, it = list('abc'[:n_mod]), [1.0, 0.5, 2.0][:n_mod], 4, 8
    masked = [m is not None for m in masks]
    # the host pipeline: train with weights, then the host-array evaluation with the same masks passed to the transforms
    host = MultimodalLearner(list(mods), list(dims), list(coefs), k)
    rows = np.asarray(train)
    np.random.seed(7)                                # (both sides draw the initial dictionary from the global stream, nmf.py:149-151)
    host.train([x[rows] for x in data], it, weights=[P[rows][:, w:w + 1] if masked[w] else None for w in range(n_mod)])
    assert host.nmf_train.last_weights_route == 'presence'
    ev = de.evaluate if n_mod == 2 else de.evaluate_internal
    lt, le = [int(labels[t]) for t in test], [int(labels[e]) for e in examples]
    want = ev(_HostData(data, P, masked), host, test, examples, lt, le, it)
    np.random.seed(7)
    learner, got = de.perform_one_run(data, mods, coefs, k, it, it, train, test, examples, lt, le,
                                      on_device=on_device, presence=masks)
    assert learner.nmf_train.last_weights_route == 'presence'
    assert np.array_equal(got['dictionary'], host.dico)
    found = sorted(key for key in want if key.startswith('found_'))
    assert found and sorted(key for key in got if key.startswith('found_')) == found
    for key in found:
        assert list(got[key]) == list(want[key]), key
        assert got['score_' + key[6:]] == want['score_' + key[6:]]
    # a dataset built with another mask is refused, the one built with this mask is taken
    ds = DeviceDataset(data, presence=masks)
    with pytest.raises(ValueError):
        de.perform_one_run(ds, mods, coefs, k, it, it, train, test, examples, lt, le, presence=[None] * (n_mod - 1) + [1.0 - P[:, -1]])
    np.random.seed(7)
    _, again = de.perform_one_run(ds, mods, coefs, k, it, it, train, test, examples, lt, le, on_device=on_device,
                                  presence=masks)
    assert np.array_equal(again['dictionary'], host.dico)


# ---- 6. what it is for ---------------------------------------------------------------------------------------------------------------------
def test_the_masked_resident_fit_recovers_the_absent_modality(monkeypatch):
    monkeypatch.setenv('KLNMF_PRECISION', 'f64')
    X, Xz, absent, P, H0 = dc.imputation_case()
    n, f, k, iters = dc.IMPUTE_N, sum(dc.IMPUTE_DIMS), dc.IMPUTE_K, dc.IMPUTE_ITERS
    _, kchunk, _, wchunk, _, _ = ec.exact_regime(n, f, k, cu_count())
    ref = pc.ref_fit_p(Xz, P, dc.IMPUTE_BOUNDS, H0, iters, kchunk=kchunk, wchunk=wchunk)
    d0 = dc.IMPUTE_DIMS[0]
    ds = DeviceDataset([Xz[:, :d0], Xz[:, d0:]], presence=[None, P[:, 1]])
    m = nmf.KLdivNMF(n_components=k, max_iter=iters, tol=0)
    m._init_dictionary = H0
    W, errors = ds._fit_dense(m, [0, 1], np.arange(n), [1.0, 1.0], f, True, return_errors=True)
    assert m.last_weights_route == 'presence'
    check_fit('f64 imputation', 'f64', (W, m.components_, np.array(errors)), ref, Xz, pc.omega(P, dc.IMPUTE_BOUNDS))
    masked_err, ref_err = dc.absent_block_error(X, absent, W, m.components_), dc.absent_block_error(X, absent, ref[0], ref[1])
    plain = DeviceDataset([Xz[:, :d0], Xz[:, d0:]])
    mu = nmf.KLdivNMF(n_components=k, max_iter=iters, tol=0)
    mu._init_dictionary = H0
    Wu = plain._fit_dense(mu, [0, 1], np.arange(n), [1.0, 1.0], f, True)
    unmasked_err = dc.absent_block_error(X, absent, Wu, mu.components_)
    _MEASURED.append('    imputation: masked %.5f (reference %.5f), unmasked %.5f' % (masked_err, ref_err, unmasked_err))
    assert abs(masked_err - ref_err) <= 1e-6 * ref_err
    assert unmasked_err >= 0.99 and masked_err * dc.IMPUTE_GAIN <= unmasked_err and masked_err <= dc.IMPUTE_CEILING
