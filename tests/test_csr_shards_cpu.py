"""Host side of CSR input over a device list (tests/test_csr_shards_gpu.py runs it): `distributed.csr_row_partition`, the routing
of `KLdivNMF` (a group of CSR contexts above `nmf.CSR_SHARD_MIN_NNZ` stored entries per shard, one device below), and the C-ABI's
declaration of klnmf_upload_csr_rows.  No GPU needed: the native context and group are replaced by recording doubles."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
from numpy.testing import assert_array_equal

from multimodal_amd import _native
from multimodal_amd.distributed import csr_row_partition
from multimodal_amd.lib import nmf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _indptr(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def _check_partition(indptr, parts):
    """csr_row_partition's contract: contiguous, covering, one row at least per part, no part above nnz / parts + one row."""
    ranges = csr_row_partition(indptr, parts)
    n = len(indptr) - 1
    assert len(ranges) == parts
    assert ranges[0][0] == 0 and ranges[-1][1] == n
    assert all(a < b for a, b in ranges)
    assert all(ranges[i][1] == ranges[i + 1][0] for i in range(parts - 1))
    lengths = np.diff(indptr)
    held = [int(indptr[b] - indptr[a]) for a, b in ranges]
    assert sum(held) == int(indptr[-1])
    assert max(held) <= indptr[-1] / parts + lengths.max(), (held, indptr[-1] / parts, lengths.max())
    return ranges, held


def test_partition_balances_stored_entries_on_skewed_rows():
    rs = np.random.RandomState(0)
    lengths = (rs.pareto(1.2, 5000) * 20).astype(np.int64)          # heavy tail: a few rows hold most entries
    lengths[::7] = 0
    indptr = _indptr(lengths)
    for parts in (2, 3, 4, 7, 8, 64):
        ranges, held = _check_partition(indptr, parts)
        if parts == 4:
            # rows are far from balanced (the point of balancing entries)
            sizes = [b - a for a, b in ranges]
            assert max(sizes) > 1.5 * min(sizes)
    # one very long row in the middle
    lengths = np.ones(1000, dtype=np.int64)
    lengths[500] = 100000
    _check_partition(_indptr(lengths), 4)


def test_partition_with_empty_rows_and_more_parts_than_nonempty_rows():
    indptr = _indptr([0, 0, 0, 100])
    assert csr_row_partition(indptr, 2) == [(0, 3), (3, 4)]
    assert csr_row_partition(indptr, 4) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    indptr = _indptr([5, 0, 0, 0, 0, 0, 7, 0])
    for parts in (2, 3, 5, 8):
        ranges, held = _check_partition(indptr, parts)
        assert sum(h == 0 for h in held) >= parts - 2           # parts beyond the non-empty rows hold no entry
    # no stored entry at all: every part still gets rows
    _check_partition(_indptr([0] * 10), 3)
    assert csr_row_partition(_indptr([3]), 1) == [(0, 1)]


def test_partition_is_deterministic():
    lengths = np.random.RandomState(3).randint(0, 50, size=777)
    indptr = _indptr(lengths)
    first = csr_row_partition(indptr, 5)
    for _ in range(3):
        assert csr_row_partition(indptr.copy(), 5) == first
    assert csr_row_partition(list(indptr), 5) == first


def test_partition_refuses_too_few_rows():
    with pytest.raises(ValueError):
        csr_row_partition(_indptr([4, 4]), 3)
    with pytest.raises(ValueError):
        csr_row_partition(_indptr([4, 4]), 0)
    with pytest.raises(ValueError):
        csr_row_partition(_indptr([]), 1)


def test_csr_shard_plan(monkeypatch):
    indptr = _indptr([10] * 100)               # 1000 entries
    monkeypatch.setattr(nmf, 'CSR_SHARD_MIN_NNZ', 300)
    assert nmf.csr_shard_plan(indptr, (5, 6, 7)) == [(5, (0, 34)), (6, (34, 67)), (7, (67, 100))]
    # too few entries for four shards of 300: three
    assert [d for d, _ in nmf.csr_shard_plan(indptr, (1, 2, 3, 4))] == [1, 2, 3]
    monkeypatch.setattr(nmf, 'CSR_SHARD_MIN_NNZ', 600)
    assert nmf.csr_shard_plan(indptr, (5, 6)) == [(5, (0, 100))]
    assert nmf.csr_shard_plan(indptr, (5,)) == [(5, (0, 100))]


class _FakeContext(object):
    """Records what the host layer asks of one shard's context; its W is the first k columns of its (densified) X."""
    made = []

    def __init__(self, precision='f64', device=0, stream=None, pooled=False):
        self.precision = _native.PRECISIONS[precision] if isinstance(precision, str) else precision
        self.device = device
        self.calls = []
        _FakeContext.made.append(self)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def close(self):
        self.calls.append('close')

    def set_problem(self, n, f, k, cap):
        self.n, self.f, self.k, self.cap = n, f, k, max(1, cap)
        self.calls.append('dense')

    def set_problem_sparse(self, X, k, cap):
        self.n, self.f, self.k, self.cap = X.shape[0], X.shape[1], k, max(1, cap)
        self.X = sp.csr_matrix(X)
        self.calls.append('sparse')
        return X

    def set_H(self, H):
        self.H = np.array(H, dtype=np.float64)

    def init_W(self):
        self.calls.append('init_W')

    def run(self, max_iter, fit, tol_abs):
        return [1.0] * max_iter, max_iter, False

    def fp8_report(self):
        return {'allowed': False, 'kl_over_sum_v': -1.0}

    def get_W(self, dtype=np.float64):
        return np.asarray(self.X[:, :self.k].toarray(), dtype=dtype)

    def get_H(self, dtype=np.float64):
        return self.H.astype(dtype)


class _FakeGroup(object):
    made = []

    def __init__(self, contexts):
        self.contexts = contexts
        self.closed = False
        _FakeGroup.made.append(self)

    def run(self, n_total, max_iter, fit, tol):
        self.args = (n_total, max_iter, fit, tol)
        return [2.0] * max_iter, max_iter, False

    def close(self):
        self.closed = True


@pytest.fixture
def fakes(monkeypatch):
    monkeypatch.delenv('KLNMF_DEVICES', raising=False)
    monkeypatch.delenv('KLNMF_DEVICE', raising=False)
    _FakeContext.made[:] = []
    _FakeGroup.made[:] = []
    monkeypatch.setattr(_native, 'Context', _FakeContext)
    monkeypatch.setattr(_native, 'Group', _FakeGroup)
    monkeypatch.setattr(nmf, '_NOTED', set())
    return monkeypatch


def _skewed_csr(n, f, seed):
    rs = np.random.RandomState(seed)
    X = sp.random(n, f, density=0.05, format='csr', random_state=rs)
    X = sp.vstack([X, sp.random(n // 4, f, density=0.6, format='csr', random_state=rs)], format='csr')
    X.data += 0.5
    return X


def test_csr_above_the_threshold_runs_one_group_over_row_shards(fakes):
    X = _skewed_csr(400, 60, seed=4)
    fakes.setattr(nmf, 'CSR_SHARD_MIN_NNZ', X.nnz // 4)
    m = nmf.KLdivNMF(n_components=5, max_iter=6, tol=1e-4, precision='f64', device=[2, 0, 1])
    W, errors = m.fit_transform(X, return_errors=True)
    made = _FakeContext.made
    assert [c.device for c in made] == [2, 0, 1]
    assert all(c.calls[0] == 'sparse' and 'dense' not in c.calls for c in made)
    assert all(c.precision == _native.PREC_F64 for c in made)
    # the row blocks stack back to the input; they balance stored entries, not rows
    assert (sp.vstack([c.X for c in made], format='csr') != X).nnz == 0
    assert [c.n for c in made] != [X.shape[0] // 3] * 3
    assert min(c.X.nnz for c in made) >= nmf.CSR_SHARD_MIN_NNZ
    # W in row order, one group run on the global shape
    assert_array_equal(W, X[:, :5].toarray())
    g, = _FakeGroup.made
    assert g.args == (X.shape[0], 6, True, 1e-4) and g.closed
    assert errors == [2.0] * 6
    assert m.last_fp8_report['shards'] == 3
    assert all(c.calls[-1] == 'close' for c in made)
    # transform: the same route, on the learnt dictionary
    _FakeContext.made[:] = []
    _FakeGroup.made[:] = []
    m.components_ = np.full((5, 60), 0.25)
    m.transform(X)
    assert len(_FakeContext.made) == 3 and len(_FakeGroup.made) == 1
    assert _FakeGroup.made[0].args[2] is False
    assert all(np.array_equal(c.H, m.components_) for c in _FakeContext.made)


def test_csr_group_output_dtype_and_precision_follow_the_single_context_rule(fakes, capsys):
    X = _skewed_csr(200, 30, seed=5).astype(np.float32)
    fakes.setattr(nmf, 'CSR_SHARD_MIN_NNZ', 1)
    H0 = np.full((3, 30), 1.0 / 30, dtype=np.float32)
    m = nmf.KLdivNMF(n_components=3, max_iter=2, tol=0, precision='bf16', device=[0, 0])
    m._init_dictionary = H0
    W = m.fit_transform(X)
    assert W.dtype == np.float32 and m.components_.dtype == np.float32
    assert [c.precision for c in _FakeContext.made] == [_native.PREC_F32] * 2
    assert capsys.readouterr().err.count("CSR input with precision='bf16'") == 1


def test_csr_below_the_threshold_runs_on_the_first_device_with_the_note(fakes, capsys):
    X = sp.random(200, 30, density=0.2, format='csr', random_state=np.random.RandomState(2))
    assert X.nnz < nmf.CSR_SHARD_MIN_NNZ
    for _ in range(2):
        nmf.KLdivNMF(n_components=3, max_iter=2, tol=0, device=[4, 5]).fit_transform(X)
    assert [c.device for c in _FakeContext.made] == [4, 4]
    assert all('sparse' in c.calls for c in _FakeContext.made)
    assert not _FakeGroup.made
    err = capsys.readouterr().err
    assert err.count('CSR input runs on one device (4)') == 1
    # explicit zeros do not count as stored entries
    fakes.setattr(nmf, '_NOTED', set())
    _FakeContext.made[:] = []
    Y = sp.csr_matrix(X, copy=True)
    Y.data[:] = 0.0
    Y.data[:10] = 1.0
    fakes.setattr(nmf, 'CSR_SHARD_MIN_NNZ', 6)
    nmf.KLdivNMF(n_components=3, max_iter=2, tol=0, device=[4, 5]).fit_transform(Y)
    assert len(_FakeContext.made) == 1 and not _FakeGroup.made


def test_upload_csr_rows_is_declared_and_bound():
    with open(os.path.join(ROOT, 'include', 'klnmf.h')) as fh:
        code = re.sub(r'/\*.*?\*/', '', fh.read(), flags=re.S)
    m = re.search(r'\bint\s+klnmf_upload_csr_rows\s*\(([^)]*)\)', code)
    assert m, 'klnmf_upload_csr_rows is not declared'
    assert len(m.group(1).split(',')) == 5
    res, args = _native.SIGNATURES['klnmf_upload_csr_rows']
    assert res is _native._c.c_int and len(args) == 5
    # the host path no longer sorts: the CSC order is built by the library
    import inspect
    src = inspect.getsource(_native.Context.set_problem_sparse)
    assert 'klnmf_upload_csr_rows' in src and 'argsort' not in src
