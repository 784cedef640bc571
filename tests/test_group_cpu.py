"""Host side of the group of contexts (klnmf_group_*; tests/test_group_gpu.py runs it): which devices KLdivNMF runs on, the
shard plan, the paths that stay on the first device, and the C-ABI's declarations.  No GPU needed: the native context and
group are replaced by recording doubles."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
from numpy.testing import assert_array_equal

from multimodal_amd import _native
from multimodal_amd.lib import nmf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def clean_env(monkeypatch):
    monkeypatch.delenv('KLNMF_DEVICES', raising=False)
    monkeypatch.delenv('KLNMF_DEVICE', raising=False)
    return monkeypatch


def test_device_precedence_argument_then_klnmf_devices_then_klnmf_device(clean_env):
    assert nmf.KLdivNMF().devices == (0,) and nmf.KLdivNMF().device == 0
    clean_env.setenv('KLNMF_DEVICE', '3')
    assert nmf.KLdivNMF().devices == (3,) and nmf._default_device() == 3
    clean_env.setenv('KLNMF_DEVICES', '1, 2,1')
    m = nmf.KLdivNMF()
    assert m.devices == (1, 2, 1) and m.device == 1
    assert nmf._default_device() == 1              # (the paths that do not shard: the list's first device)
    assert nmf.KLdivNMF(device=5).devices == (5,)
    assert nmf.KLdivNMF(device=[0, 0]).devices == (0, 0)
    assert nmf.KLdivNMF(device=(4,)).device == 4
    assert nmf.KLdivNMF(device=np.int64(2)).devices == (2,)
    for bad in ([], [-1], ['0'], [0.5], 'x'):
        with pytest.raises(ValueError):
            nmf.KLdivNMF(device=bad)
    clean_env.setenv('KLNMF_DEVICES', '0,a')
    with pytest.raises(ValueError, match='KLNMF_DEVICES'):
        nmf.KLdivNMF()


def test_without_klnmf_devices_nothing_changes(clean_env):
    clean_env.setenv('KLNMF_DEVICE', '2')
    assert nmf._default_device() == 2
    assert nmf.KLdivNMF().device == 2 and nmf.KLdivNMF(device=7).device == 7


def test_shard_plan():
    from multimodal_amd.distributed import row_partition
    # fewer 32-row tiles than devices: fewer shards
    assert nmf.shard_plan(100, (0, 1, 2, 3, 4, 5)) == [(0, (0, 32)), (1, (32, 64)), (2, (64, 96)), (3, (96, 100))]
    assert nmf.shard_plan(40, (0, 0, 0)) == [(0, (0, 32)), (0, (32, 40))]
    # one tile, or a one-entry list: one shard (the plain path)
    assert nmf.shard_plan(32, (0, 1)) == [(0, (0, 32))]
    assert nmf.shard_plan(10 ** 6, (6,)) == [(6, (0, 10 ** 6))]
    # enough tiles: every device, distributed.row_partition's ranges
    plan = nmf.shard_plan(132032, (0, 0))
    assert [b for _, b in plan] == row_partition(132032, 2) == [(0, 66016), (66016, 132032)]
    assert [d for d, _ in nmf.shard_plan(1000, (3, 1, 2))] == [3, 1, 2]


class _FakeContext(object):
    """Records what the host layer asks of one shard's context; its W is the first k columns of its V, its H the last one set."""
    made = []

    def __init__(self, precision='f64', device=0, stream=None, pooled=False):
        self.precision = _native.PRECISIONS[precision] if isinstance(precision, str) else precision
        self.device = device
        self.calls = []
        self.cap = 0
        _FakeContext.made.append(self)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def close(self):
        self.calls.append('close')

    def set_problem(self, n, f, k, cap):
        self.n, self.f, self.k, self.cap = n, f, k, max(1, cap)
        self.V = np.zeros((n, f))

    def set_problem_sparse(self, X, k, cap):
        self.set_problem(X.shape[0], X.shape[1], k, cap)
        self.calls.append('sparse')
        return X

    def set_v_max(self, v):
        self.vmax = v

    def upload_V(self, block, row0=0, col0=0, scale=1.0):
        self.V[row0:row0 + block.shape[0], col0:col0 + block.shape[1]] = scale * np.asarray(block)

    def upload_blocks(self, blocks, scales=None):
        col = 0
        for b, s in zip(blocks, scales):
            self.upload_V(b, 0, col, s)
            col += b.shape[1]

    def set_H(self, H):
        self.H = np.array(H, dtype=np.float64)

    def init_W(self):
        self.calls.append('init_W')

    def run(self, max_iter, fit, tol_abs):
        return [1.0] * max_iter, max_iter, False

    def fp8_report(self):
        return {'allowed': False, 'kl_over_sum_v': -1.0}

    def get_W(self, dtype=np.float64):
        return (self.V[:, :self.k] + 0.0).astype(dtype)

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
def fakes(monkeypatch, clean_env):
    _FakeContext.made[:] = []
    _FakeGroup.made[:] = []
    monkeypatch.setattr(_native, 'Context', _FakeContext)
    monkeypatch.setattr(_native, 'Group', _FakeGroup)
    return monkeypatch


def test_dense_fit_on_a_device_list_runs_one_group_over_row_shards(fakes):
    rs = np.random.RandomState(0)
    a, b = rs.random_sample((100, 6)), rs.random_sample((100, 4)) * 3.0
    m = nmf.KLdivNMF(n_components=4, max_iter=5, tol=1e-4, precision='f64', device=[2, 0, 1])
    W, errors = m._fit_blocks([a, b], [1.0, 0.5], return_errors=True)
    assert [c.device for c in _FakeContext.made] == [2, 0, 1]
    assert [c.n for c in _FakeContext.made] == [64, 32, 4]
    # one storage factor from the global maximum of the (scaled) blocks
    vmax = max(a.max(), 0.5 * b.max())
    assert all(c.vmax == vmax for c in _FakeContext.made)
    # each shard holds its rows of hstack([1.0 a, 0.5 b]); W comes back in row order
    X = np.hstack([a, 0.5 * b])
    assert_array_equal(np.vstack([c.V for c in _FakeContext.made]), X)
    assert_array_equal(W, X[:, :4])
    g, = _FakeGroup.made
    assert g.args == (100, 5, True, 1e-4) and g.closed
    assert errors == [2.0] * 5
    assert m.last_fp8_report['shards'] == 3
    assert all(c.calls[-1] == 'close' for c in _FakeContext.made)


def test_one_entry_list_and_few_rows_take_the_plain_path(fakes):
    X = np.random.RandomState(1).random_sample((40, 8))
    for dev, rows in (([3], 40), ([0, 1], 32)):
        _FakeContext.made[:] = []
        nmf.KLdivNMF(n_components=2, max_iter=3, tol=0, device=dev).fit_transform(X[:rows])
        assert len(_FakeContext.made) == 1 and _FakeContext.made[0].device == dev[0]
    assert not _FakeGroup.made


def test_csr_input_with_a_device_list_runs_on_the_first_device_and_says_so(fakes, capsys):
    fakes.setattr(nmf, '_NOTED', set())
    X = sp.random(200, 30, density=0.2, format='csr', random_state=np.random.RandomState(2))
    for _ in range(2):
        nmf.KLdivNMF(n_components=3, max_iter=2, tol=0, device=[4, 5]).fit_transform(X)
    assert [c.device for c in _FakeContext.made] == [4, 4]
    assert all('sparse' in c.calls for c in _FakeContext.made)
    assert not _FakeGroup.made
    err = capsys.readouterr().err
    assert err.count('CSR input runs on one device (4)') == 1


def test_group_exports_are_declared_and_bound():
    with open(os.path.join(ROOT, 'include', 'klnmf.h')) as fh:
        header = fh.read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name in ('klnmf_group_create', 'klnmf_group_run', 'klnmf_group_destroy', 'klnmf_group_enqueue_time', 'klnmf_group_selftest'):
        assert re.search(r'\bint\s+%s\s*\(' % name, code), name
        assert name in _native.SIGNATURES
    m = re.search(r'#define KLNMF_ERR_REPLICA\s+(-?\d+)', header)
    assert m and int(m.group(1)) == _native.ERR_REPLICA
    codes = [int(v) for v in re.findall(r'#define KLNMF_ERR_\w+\s+(-?\d+)', header)]
    assert len(codes) == len(set(codes))
    assert 'typedef struct klnmf_group klnmf_group;' in code
