"""CSR modalities kept on the device: the problem klnmf_upload_csr_device_rows gathers there against the one the host path
uploads from host slices (`nmf._csr_of` + `set_problem_sparse`), and the public classes on top of it.

The bar is BIT IDENTITY (np.array_equal): both paths hand the same arrays to the same kernels, so there is nothing to tolerate.
Per case, in 'f64' and 'f32': nnz, the block counts, W0 of init_W, the ratio values of step_Q, W and H after step_W / step_H,
and the loss record, W and H of a 5-iteration run.

Data: tests/sparse_cases.designed_csr(301, 263, 1, 1, seed) -- rows of 0, 1, 15 ... 65 entries -- cut into three modalities at
columns [0, 87, 175, 263], plus rows whose first-modality cell holds 63, 64, 65 and 87 entries: the copy kernel takes a (row,
modality) cell in trips of 64 entries (csrc/csrgather.hip.h, kCsrgTrip), and the designed cells alone stay below one trip.
`base` asserts that coverage.  Row lists: identity, reversed, a permutation with repeats, a single row, and 2047 / 2048 / 2049
rows drawn with repeats -- with the row pointers' n + 1 entries on both sides of the scan's 2048-element tile; the scan's second
level (more than 256 tiles: 524 289 rows) is compared through init_W and one step_Q only.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from multimodal_amd import _native
from multimodal_amd import device_data
from multimodal_amd.device_data import DeviceDataset, DeviceEvaluation, csr_rows_plan
from multimodal_amd.device_experiment import evaluate, perform_one_run
from multimodal_amd.evaluation import classify_NN
from multimodal_amd.learner import MultimodalLearner
from multimodal_amd.lib import nmf
from multimodal_amd.lib.metrics import kl_div
from tests import sparse_cases as sc

pytestmark = pytest.mark.gpu

N, F, K = 301, 263, 5
CUTS = [0, 87, 175, 263]
COEFS = (1.0, 0.5, 0.3)
TRIP = 64                               # kCsrgTrip
TRIP_ROWS = {3: 63, 5: 64, 7: 65, 9: 87}      # row -> entries of its first-modality cell
PRECS = ['f64', 'f32']
_BASE = {}


def base(dtype=np.float64):
    """The designed matrix with the trip-edge rows, built once per value type and never changed."""
    key = np.dtype(dtype).name
    if key not in _BASE:
        X = sc.designed_csr(N, F, 1, 1, 21).toarray()
        rng = np.random.default_rng(22)
        for r, c in TRIP_ROWS.items():
            X[r, :CUTS[1]] = 0.0
            X[r, :c] = rng.gamma(1.0, 1.0, c) + 0.05
        X = sp.csr_matrix(X.astype(dtype))
        X.sort_indices()
        lengths = sc.row_lengths(X)
        assert (lengths == 0).any() and (lengths == 1).any() and lengths.max() > TRIP
        cells = set(np.diff(sp.csr_matrix(X[:, :CUTS[1]]).indptr).tolist())
        assert {0, 1, TRIP - 1, TRIP, TRIP + 1, CUTS[1]} <= cells, sorted(cells)      # no trip, both sides of one, two trips
        _BASE[key] = X
    return _BASE[key]


def cut(X, cuts):
    return [sp.csr_matrix(X[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])]


def variant(name):
    """The modalities of a case: scipy CSR, or a dense array in the mixed stack."""
    if name == 'f32':
        return cut(base(np.float32), CUTS)
    if name == 'one-column':
        return cut(base(), [0, 87, 88, 263])
    mods = cut(base(), CUTS)
    if name == 'empty-first':
        mods[0] = sp.csr_matrix(mods[0].shape, dtype=np.float64)
    elif name == 'mixed':
        mods[1] = mods[1].toarray()
    else:
        assert name == 'three'
    return mods


VARIANTS = ['three', 'empty-first', 'one-column', 'mixed', 'f32']
_RS = np.random.RandomState(5)
ROW_LISTS = {
    'identity': np.arange(N),
    'reversed': np.arange(N)[::-1].copy(),
    'repeats': np.concatenate([_RS.permutation(N), _RS.randint(0, N, 150)]),
    'single': np.array([7]),
    'r2047': _RS.randint(0, N, 2047),
    'r2048': _RS.randint(0, N, 2048),
    'r2049': _RS.randint(0, N, 2049),
}


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_problem(prec, mods, rows, coefs, k, cap, nnz=None):
    """A context whose CSR problem was gathered on the device; (ctx, what must stay alive)."""
    srcs = [device_data._DeviceCsr(m, to_device) for m in mods]
    plan_nnz, use_device = csr_rows_plan([s.indptr for s in srcs], rows, coefs, [s.least for s in srcs])
    assert use_device
    bounds = np.concatenate([[0], np.cumsum([m.shape[1] for m in mods])])
    idx = to_device(np.asarray(rows, dtype=np.int64))
    ctx = _native.Context(prec)
    ctx.set_problem_sparse_shape(len(rows), int(bounds[-1]), k, cap, plan_nnz if nnz is None else nnz)
    ctx.upload_csr_device_rows([s.pointers() for s in srcs], bounds, coefs, mods[0].shape[0], idx.data_ptr(), len(rows))
    return ctx


def host_problem(prec, mods, rows, coefs, k, cap):
    ctx = _native.Context(prec)
    ctx.set_problem_sparse(nmf._csr_of([m[rows] for m in mods], coefs), k, cap)
    return ctx


def walk(ctx, H0, deep=True):
    """Everything a case compares, in order."""
    out = [('nnz', np.int64(ctx.nnz)), ('blocks', np.array(ctx.sparse_blocks()))]
    ctx.set_H(H0)
    ctx.init_W()
    out.append(('W0', ctx.get_W()))
    ctx.step_Q()
    out.append(('Q', ctx.get_Q_values()))
    if not deep:
        return out
    ctx.step_W()
    out.append(('W after step_W', ctx.get_W()))
    ctx.step_H()
    out.append(('H after step_H', ctx.get_H()))
    ctx.set_H(H0)
    ctx.init_W()
    errors, n_done, stopped = ctx.run(5, True, 0.0)
    out += [('losses', np.array(errors)), ('n_done', np.int64(n_done)), ('W of the run', ctx.get_W()), ('H of the run', ctx.get_H())]
    return out


def same(case, got, ref):
    assert [g[0] for g in got] == [r[0] for r in ref]
    for (what, a), (_, b) in zip(got, ref):
        assert np.array_equal(a, b), '%s: %s differs' % (case, what)
        assert np.isfinite(np.asarray(a, dtype=np.float64)).all(), (case, what)


def compare(case, prec, mods, rows, coefs=COEFS, k=K, deep=True, blocks=None):
    f = sum(m.shape[1] for m in mods)
    H0 = sc.factors(len(rows), f, k, seed=3)[1]
    with device_problem(prec, mods, rows, coefs, k, 5) as dev, host_problem(prec, mods, rows, coefs, k, 5) as host:
        if blocks is not None:
            assert dev.sparse_blocks() == blocks and host.sparse_blocks() == blocks
        got, ref = walk(dev, H0, deep), walk(host, H0, deep)
    same(case, got, ref)
    return got


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('rows', list(ROW_LISTS))
@pytest.mark.parametrize('name', VARIANTS)
def test_the_gathered_problem_is_the_host_paths(name, rows, prec):
    got = compare('%s %s %s' % (name, rows, prec), prec, variant(name), ROW_LISTS[rows])
    assert dict(got)['nnz'] > 0


@pytest.mark.parametrize('prec', PRECS)
def test_forced_blocks(monkeypatch, prec):
    """Two column and three row blocks (KLNMF_SP_CB / KLNMF_SP_RB): the blocked set-up behind the gather."""
    monkeypatch.setenv('KLNMF_DEV', '1')
    monkeypatch.setenv('KLNMF_SP_CB', '2')
    monkeypatch.setenv('KLNMF_SP_RB', '3')
    compare('forced (2, 3) %s' % prec, prec, variant('three'), ROW_LISTS['repeats'], blocks=(2, 3))


@pytest.mark.parametrize('prec', PRECS)
def test_the_scans_second_level(prec):
    """524 289 rows: 257 tiles of row pointers, so k_csc_scan_part carries over its first 256.  Mostly empty and single-entry
    rows (the problem stays small), every 500th pick any row; compared through init_W and one step_Q."""
    mods = variant('three')
    lengths = sc.row_lengths(base())
    short = np.flatnonzero(lengths <= 1)
    rs = np.random.RandomState(9)
    rows = short[rs.randint(0, short.size, 524289)]
    rows[::500] = rs.randint(0, N, rows[::500].size)
    assert (rows.size + 1 + 2047) // 2048 == 257
    got = compare('second level %s' % prec, prec, mods, rows, deep=False)
    assert 100000 < dict(got)['nnz'] < 2000000


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def usable(ctx, prec):
    """A host upload and a step on the refused context succeed, and give what a fresh context gives."""
    X = nmf._csr_of([m[ROW_LISTS['reversed']] for m in variant('three')], COEFS)
    H0 = sc.factors(N, F, K, seed=3)[1]
    ctx.set_problem_sparse(X, K, 5)
    got = walk(ctx, H0, deep=False)
    with _native.Context(prec) as fresh:
        fresh.set_problem_sparse(X, K, 5)
        same('after a refusal', got, walk(fresh, H0, deep=False))


@pytest.mark.parametrize('prec', PRECS)
def test_refusals_leave_the_context_usable(prec):
    mods, rows = variant('three'), ROW_LISTS['repeats']
    srcs = [device_data._DeviceCsr(m, to_device) for m in mods]
    nnz = csr_rows_plan([s.indptr for s in srcs], rows, COEFS, [s.least for s in srcs])[0]
    args = lambda idx: ([s.pointers() for s in srcs], CUTS, COEFS, N, idx.data_ptr(), idx.numel())
    idx = to_device(rows.astype(np.int64))
    beyond = rows.astype(np.int64).copy()
    beyond[11] = N                                       # one row index past the sources
    idx_beyond = to_device(beyond)
    with _native.Context(prec) as ctx:
        ctx.set_problem_sparse_shape(rows.size, F, K, 5, nnz + 1)          # wrong nnz
        with pytest.raises(_native.NativeError) as e:
            ctx.upload_csr_device_rows(*args(idx))
        assert e.value.code == _native.ERR_ARG and 'stored entries' in str(e.value)
        usable(ctx, prec)
        ctx.set_problem_sparse_shape(rows.size, F, K, 5, nnz)              # a row index >= n
        with pytest.raises(_native.NativeError) as e:
            ctx.upload_csr_device_rows(*args(idx_beyond))
        assert e.value.code == _native.ERR_ARG and 'row index' in str(e.value)
        usable(ctx, prec)
        ctx.set_problem(rows.size, F, K, 5)                                # a dense problem
        with pytest.raises(_native.NativeError) as e:
            ctx.upload_csr_device_rows(*args(idx))
        assert e.value.code == _native.ERR_ARG
        usable(ctx, prec)
        ctx.set_problem_sparse_shape(rows.size, F, K, 5, nnz)              # bounds that do not end at f, a wrong row count
        with pytest.raises(_native.NativeError):
            ctx.upload_csr_device_rows([s.pointers() for s in srcs], [0, 87, 175, 262], COEFS, N, idx.data_ptr(), idx.numel())
        with pytest.raises(_native.NativeError):
            ctx.upload_csr_device_rows([s.pointers() for s in srcs], CUTS, COEFS, N, idx.data_ptr(), idx.numel() - 1)
        usable(ctx, prec)


# ---- the public classes ------------------------------------------------------------------------------------------------------------
MODS = ['a', 'b', 'c']
TRAIN = np.concatenate([np.arange(0, 200), [5, 5, 199]])
TEST = np.arange(200, 260)
EXAMPLES = np.arange(260, 301)


def host_slices(mods, rows, which=(0, 1, 2)):
    return [mods[w][rows] for w in which]


def trained_pair(monkeypatch, prec, mods, coefs=COEFS, iters=6):
    """(dataset, learner trained through it, learner trained on host slices), both from the same draw of the global stream."""
    monkeypatch.setenv('KLNMF_PRECISION', prec)
    ds = DeviceDataset(mods, keep_sparse=True)
    dims = [m.shape[1] for m in mods]
    dev, host = MultimodalLearner(MODS, dims, list(coefs), K), MultimodalLearner(MODS, dims, list(coefs), K)
    np.random.seed(17)
    ds.train(dev, TRAIN, iters)
    np.random.seed(17)
    host.train(host_slices(mods, TRAIN), iters)
    return ds, dev, host


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('name', ['three', 'mixed', 'f32'])
def test_train_and_transforms_equal_the_host_calls(monkeypatch, name, prec):
    mods = variant(name)
    ds, dev, host = trained_pair(monkeypatch, prec, mods)
    assert ds.keep_sparse and ds.sparse == [sp.issparse(m) for m in mods]
    assert np.array_equal(dev.dico, host.dico) and np.isfinite(host.dico).all() and host.dico.std() > 0
    for which in ((0, 2), (1,), (0, 1, 2)):
        names = [MODS[w] for w in which]
        got = ds.reconstruct_internal_multi(dev, names, TEST, 4)
        ref = host.reconstruct_internal_multi(names, host_slices(mods, TEST, which), 4)
        assert np.array_equal(got, ref), which
        ev = DeviceEvaluation(ds, dev, 4)
        assert np.array_equal(ev.internal(names, TEST).cpu().numpy(), ref), which
    for w, m in enumerate(mods):
        raw = m[EXAMPLES].toarray() if sp.issparse(m) else m[EXAMPLES]
        assert np.array_equal(ev.raw(w, EXAMPLES).cpu().numpy(), np.asarray(raw, dtype=np.float64)), w
        assert np.array_equal(ds.rows_of(w, EXAMPLES), raw), w
    labels_ex = [int(i) % 7 for i in EXAMPLES]
    t_test, t_ex = ev.internal(['a'], TEST), ev.internal(['c'], EXAMPLES)
    found = ev.found_labels(t_test, t_ex, labels_ex, _native.DIST_KL)
    assert found == classify_NN(t_test.cpu().numpy(), t_ex.cpu().numpy(), labels_ex, kl_div)


@pytest.mark.parametrize('prec', PRECS)
def test_a_subset_of_dense_modalities_still_runs_the_dense_path(monkeypatch, prec):
    mods = variant('mixed')
    ds, dev, _ = trained_pair(monkeypatch, prec, mods)
    dense = DeviceDataset([m.toarray() if sp.issparse(m) else m for m in mods])
    assert not ds.sparse_route([1]) and ds.sparse_route([0, 1]) and not dense.keep_sparse
    assert np.array_equal(ds.reconstruct_internal(dev, 'b', TEST, 4), dense.reconstruct_internal(dev, 'b', TEST, 4))
    a, b = DeviceEvaluation(ds, dev, 4), DeviceEvaluation(dense, dev, 4)
    assert np.array_equal(a.internal(['b'], TEST).cpu().numpy(), b.internal(['b'], TEST).cpu().numpy())
    assert np.array_equal(a.raw(1, TEST).cpu().numpy(), b.raw(1, TEST).cpu().numpy())


@pytest.mark.parametrize('prec', PRECS)
def test_the_default_is_the_dense_branch_as_before(monkeypatch, prec):
    """keep_sparse=False on sparse input: densified at creation, the dense branch, bit for bit what dense input gives."""
    monkeypatch.setenv('KLNMF_PRECISION', prec)
    mods = variant('three')
    dims = [m.shape[1] for m in mods]
    results = []
    for data in (mods, [m.toarray() for m in mods]):
        ds = DeviceDataset(data)
        assert not ds.keep_sparse and not any(ds.sparse) and all(b is not None for b in ds.blocks)
        learner = MultimodalLearner(MODS, dims, list(COEFS), K)
        np.random.seed(17)
        ds.train(learner, TRAIN, 6)
        results.append((learner.dico, ds.reconstruct_internal(learner, 'a', TEST, 4)))
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])
    # ... and it is not the sparse branch's result
    kept = DeviceDataset(mods, keep_sparse=True)
    learner = MultimodalLearner(MODS, dims, list(COEFS), K)
    np.random.seed(17)
    kept.train(learner, TRAIN, 6)
    assert not np.array_equal(learner.dico, results[0][0])


@pytest.mark.parametrize('case', ['zero', 'underflow'])
def test_dropped_products_take_the_host_path_and_equal_it(monkeypatch, capsys, case):
    if case == 'zero':
        mods, coefs = variant('three'), (1.0, 0.0, 0.3)
    else:
        mods = variant('f32')
        least = [float(m.data.min()) for m in mods]
        w = int(np.argmin(least))
        coefs = [1.0, 0.5, 0.3]
        coefs[w] = 0.4 * float(np.finfo(np.float32).smallest_subnormal) / least[w]
        assert np.float32(least[w]) * np.float32(coefs[w]) == 0
    nmf._NOTED.discard(('csr-device-rows-host',))                # (said once per process: let this case hear it)
    ds, dev, host = trained_pair(monkeypatch, 'f64', mods, coefs=coefs)
    assert 'on the host' in capsys.readouterr().err
    assert np.array_equal(dev.dico, host.dico) and np.isfinite(host.dico).all()
    got = DeviceEvaluation(ds, dev, 4).internal(MODS, TEST).cpu().numpy()
    assert np.array_equal(got, host.reconstruct_internal_multi(MODS, host_slices(mods, TEST), 4))


class _HostData(object):
    """What `device_experiment.evaluate` asks of a dataset, answered by the host calls on host slices."""

    def __init__(self, mods):
        self.mods = mods

    def reconstruct_internal(self, learner, mod, rows, iterations):
        w = learner.get_index(mod)
        return learner.reconstruct_internal(mod, self.mods[w][np.asarray(rows)], iterations)

    def rows_of(self, which, rows):
        return np.asarray(self.mods[which][np.asarray(rows)].toarray())


def toy_set(seed=1, n_labels=5, per_label=14, dims=(40, 30)):
    """Two sparse modalities: every label a few active columns per modality, Poisson counts on them."""
    rng = np.random.default_rng(seed)
    labels = np.repeat(np.arange(n_labels), per_label)
    mods = []
    for d in dims:
        proto = np.zeros((n_labels, d))
        for l in range(n_labels):
            proto[l, rng.choice(d, size=6, replace=False)] = rng.uniform(2.0, 6.0, 6)
        mods.append(sp.csr_matrix(rng.poisson(proto[labels]).astype(np.float64)))
    return mods, [int(l) for l in labels]


@pytest.mark.parametrize('on_device', [True, False])
def test_one_run_on_sparse_modalities_equals_the_host_pipeline(monkeypatch, on_device):
    monkeypatch.setenv('KLNMF_PRECISION', 'f64')
    mods, labels = toy_set()
    n = len(labels)
    examples = [labels.index(l) for l in sorted(set(labels))]
    others = [i for i in range(n) if i not in examples]
    perm = np.random.RandomState(4).permutation(len(others))
    test, train = [others[i] for i in perm[:12]], [others[i] for i in perm[12:]]
    names, coefs, k = ['u', 'v'], [1.0, 0.7], 6
    np.random.seed(23)
    learner, res = perform_one_run(mods, names, coefs, k, 15, 8, train, test, examples, [labels[t] for t in test],
                                   [labels[e] for e in examples], on_device=on_device, keep_sparse=True)
    host = MultimodalLearner(names, [m.shape[1] for m in mods], coefs, k)
    np.random.seed(23)
    host.train([m[train] for m in mods], 15)
    assert np.array_equal(res['dictionary'], host.get_dico())
    ref = evaluate(_HostData(mods), host, test, examples, [labels[t] for t in test], [labels[e] for e in examples], 8)
    keys = sorted(key for key in ref if key.startswith('found_'))
    assert len(keys) == 48
    for key in keys:
        assert list(res[key]) == list(ref[key]), key
        assert res[key.replace('found_', 'score_', 1)] == ref[key.replace('found_', 'score_', 1)], key
    assert np.mean([ref[key.replace('found_', 'score_', 1)] for key in keys]) > 0.5      # (it does classify: chance = 0.2)


def test_run_sweep_keeps_sparse_modalities_on_the_sparse_branch(monkeypatch):
    """`run_sweep(..., keep_sparse=True)` hands the flag to its worker's DeviceDataset: every fit and transform of the sweep
    gathers a CSR problem on the device and none uploads dense rows; the default densifies and does the opposite."""
    from multimodal_amd.device_experiment import run_sweep
    mods, labels = toy_set()
    calls = {'csr': 0, 'dense': 0}
    gather, dense = _native.Context.upload_csr_device_rows, _native.Context.upload_V_device_rows_dt

    def count(key, fn):
        def wrapped(self, *a, **kw):
            calls[key] += 1
            return fn(self, *a, **kw)
        return wrapped
    monkeypatch.setattr(_native.Context, 'upload_csr_device_rows', count('csr', gather))
    monkeypatch.setattr(_native.Context, 'upload_V_device_rows_dt', count('dense', dense))
    kw = dict(iter_train=15, iter_test=8, coefs=[1.0, 0.7], seed=2, devices=[0], precision='f64')
    table, raw = run_sweep(mods, labels, ['u', 'v'], [6], 2, keep_sparse=True, **kw)
    assert calls['csr'] > 0 and calls['dense'] == 0, calls
    assert len(raw) == 2 and len(table[6]) == 48
    assert np.mean([table[6][key][0] for key in table[6]]) > 0.5         # (it does classify: chance = 0.2)
    calls.update(csr=0, dense=0)
    run_sweep(mods, labels, ['u', 'v'], [6], 1, **kw)
    assert calls['csr'] == 0 and calls['dense'] > 0, calls
