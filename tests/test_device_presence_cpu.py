"""Presence masks on DeviceDataset (`DeviceDataset(data, presence=[...])`): what runs without a GPU.

  * `presence=` is validated on the host, before anything is uploaded (`device_data.check_presence`);
  * with `_native.Context` replaced by a recording double and `_to_device` by host arrays (the way test_csr_device_rows_cpu.py fakes
    them), the route every call takes: an unmasked subset makes no presence call, a masked one exactly one -- with the source columns
    and bounds of its modalities --, a masked subset that holds a CSR modality raises ValueError;
  * `perform_one_run` / `run_sweep` forward the mask; a `DeviceDataset` built with another one is refused;
  * the new export (klnmf_upload_presence_device_rows): declared, bound, exported, counted in the documents;
  * the imputation case (tests/device_presence_cases.py) on the fp64 restatement alone: 0.01087 under the mask against 1.00000
    without it after 100 iterations, 0.00177 after 300.
"""
import inspect
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from multimodal_amd import _native
from multimodal_amd import device_data
from multimodal_amd import device_experiment
from multimodal_amd.learner import MultimodalLearner
from tests import device_presence_cases as dc
from tests import presence_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, DIMS, K = 30, [7, 5, 4], 3
RS = np.random.RandomState(2)
DATA = [RS.random_sample((N, d)) + 0.1 for d in DIMS]
P = pc.mask(N, 3, seed=11)
MASKS = [P[:, 0], None, P[:, 2:3]]                # (n,) and (n, 1); the second modality has no mask


# ---- validation --------------------------------------------------------------------------------------------------------------------
class _NoUpload(device_data.DeviceDataset):
    def _to_device(self, array):
        raise AssertionError('something was uploaded')


BAD = {
    'an entry too few': [P[:, 0], None],
    'an entry too many': [None] * 4,
    'a row too many': [np.ones(N + 1), None, None],
    'a row too few': [None, np.ones((N - 1, 1)), None],
    'two columns': [None, None, np.ones((N, 2))],
    'a row vector': [np.ones((1, N)), None, None],
    'negative': [None, -P[:, 0] - 1e-300, None],
    'nan': [np.full(N, np.nan), None, None],
    'inf': [None, None, np.full((N, 1), np.inf)],
}


@pytest.mark.parametrize('name', list(BAD), ids=list(BAD))
def test_a_bad_mask_raises_valueerror_before_anything_is_uploaded(name):
    with pytest.raises(ValueError):
        _NoUpload(DATA, device=0, presence=BAD[name])
    with pytest.raises(ValueError):
        device_data.check_presence(BAD[name], N, 3)


def test_more_modalities_than_a_mask_holds_raise_valueerror():
    many = [DATA[0][:, :1]] * (_native.MAX_MODALITIES + 1)
    with pytest.raises(ValueError):
        _NoUpload(many, device=0, presence=[P[:, 0]] + [None] * _native.MAX_MODALITIES)
    # ... without an array among the entries there is no mask, and nothing to refuse
    assert device_data.check_presence([None] * 17, N, 17) == (None, [False] * 17)
    assert device_data.check_presence([1.0] + [None] * 16, N, 17) == (None, [False] * 17)


def test_the_mask_as_it_is_kept():
    Pk, masked = device_data.check_presence(MASKS, N, 3)
    assert masked == [True, False, True] and Pk.dtype == np.float64 and Pk.shape == (N, 3)
    assert np.array_equal(Pk[:, 0], P[:, 0]) and np.array_equal(Pk[:, 2], P[:, 2]) and (Pk[:, 1] == 1).all()
    assert device_data.check_presence(None, N, 3) == (None, [False] * 3)
    assert device_data.check_presence([None, 2.0, None], N, 3) == (None, [False] * 3)      # a scalar is no mask
    assert device_data.check_presence([P[:, 0].astype(np.float32), None, None], N, 3)[0].dtype == np.float64
    assert inspect.signature(device_data.DeviceDataset.__init__).parameters['presence'].default is None      # opt-in


# ---- routing: a recording context, host arrays for tensors -------------------------------------------------------------------------
class _HostDataset(device_data.DeviceDataset):
    def _to_device(self, array):
        return dc.HostTensor(array)

    def _synchronize(self):
        pass


class _Recorder(object):
    """Stands in for `_native.Context`: records every call `_fit_uploaded` makes on it."""
    calls = []
    opened = []

    def __init__(self, precision='f64', device=0, stream=None, pooled=False):
        self.precision = _native.PRECISIONS[precision]
        self.precision_name = precision
        _Recorder.opened.append(precision)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        pass

    def __getattr__(self, name):
        def method(*args, **kwargs):
            _Recorder.calls.append((name, args, kwargs))
            if name in ('set_problem', 'set_problem_sparse_shape'):
                self.n, self.f, self.k = args[0], args[1], args[2]
            if name == 'set_problem_sparse':
                (self.n, self.f), self.k = args[0].shape, args[1]
            if name == 'run':
                return [], 0, False
            if name == 'fp8_report':
                return {}
            if name == 'get_W':
                return np.zeros((self.n, self.k))
            if name == 'get_H':
                return np.zeros((self.k, self.f))
        return method


@pytest.fixture
def recorded(monkeypatch):
    _Recorder.calls, _Recorder.opened = [], []
    monkeypatch.setattr(_native, 'Context', _Recorder)
    monkeypatch.delenv('KLNMF_PRECISION', raising=False)
    return _Recorder


def presence_calls():
    return [c for c in _Recorder.calls if c[0] == 'upload_presence_device_rows']


def names():
    return [c[0] for c in _Recorder.calls]


def trained(ds, rows, mods='abc'):
    learner = MultimodalLearner(list(mods), list(ds.dims), [1.0, 0.5, 2.0][:len(ds.dims)], K)
    f = sum(ds.dims)
    ds.train(learner, rows, 4, init_dictionary=np.full((K, f), 1.0 / f))
    return learner


def test_a_masked_train_makes_one_presence_call_behind_the_data(recorded):
    ds = _HostDataset(DATA, device=0, presence=MASKS)
    assert ds.masked == [True, False, True] and ds.presence.a.shape == (N, 3) and ds.presence.a.dtype == np.float64
    plain = _HostDataset(DATA, device=0)
    assert ds.resident_bytes() == plain.resident_bytes() + 8 * N * 3 and plain.presence is None
    rows = np.array([5, 4, 4, 29, 0])
    learner = trained(ds, rows)
    assert learner.nmf_train.last_weights_route == 'presence' and ds.last_weights_route == 'presence'
    assert recorded.opened == ['f64']                                         # `weighted_precision` of the default
    order = names()
    assert order[0] == 'set_problem' and order.count('upload_V_device_rows_dt') == 3
    (_, args, kwargs), = presence_calls()
    assert order.index('upload_presence_device_rows') == max(i for i, c in enumerate(order) if c == 'upload_V_device_rows_dt') + 1
    ptr, f64, src_rows, ld, idx_ptr, n, src_cols, bounds = args
    assert ptr == ds.presence.data_ptr() and f64 is True and src_rows == N and ld == 3 and n == rows.size and not kwargs
    assert list(src_cols) == [0, -1, 2] and list(bounds) == [0, 7, 12, 16]
    # the row indices are the call's own, the ones the data rows were gathered by
    v = [c for c in _Recorder.calls if c[0] == 'upload_V_device_rows_dt']
    assert all(c[1][2] == idx_ptr and c[1][3] == rows.size for c in v) and isinstance(idx_ptr, int)
    # nothing of the host path
    assert 'upload_presence' not in order and 'upload_weights' not in order and 'upload_blocks' not in order


@pytest.mark.parametrize('mods,src_cols,bounds', [(['a'], [0], [0, 7]), (['c', 'a'], [2, 0], [0, 4, 11]), (['b', 'c'], [-1, 2], [0, 5, 9]),
                                                  (['a', 'b', 'c'], [0, -1, 2], [0, 7, 12, 16])], ids=['a', 'c+a', 'b+c', 'all'])
def test_a_masked_subset_names_its_own_columns_and_bounds(recorded, mods, src_cols, bounds):
    ds = _HostDataset(DATA, device=0, presence=MASKS)
    learner = trained(ds, np.arange(N))
    _Recorder.calls = []
    ds.reconstruct_internal_multi(learner, mods, [3, 1, 1], 2)
    assert ds.last_weights_route == 'presence'
    (_, args, _), = presence_calls()
    assert list(args[6]) == src_cols and list(args[7]) == bounds and args[5] == 3 and args[2] == N


def test_an_unmasked_subset_is_the_unmasked_call(recorded):
    ds = _HostDataset(DATA, device=0, presence=MASKS)
    plain = _HostDataset(DATA, device=0)
    learner = trained(ds, np.arange(N))
    seen = []
    for d in (ds, plain):
        _Recorder.calls, _Recorder.opened = [], []
        d.reconstruct_internal(learner, 'b', [3, 1, 1], 2)
        assert d.last_weights_route is None and not presence_calls()
        seen.append(([(n, a[1:2] + a[3:], k) for n, a, k in _Recorder.calls if n != 'set_H'], list(_Recorder.opened)))
    assert seen[0] == seen[1]                       # the same calls with the same arguments (but for the tensors' addresses)
    # a dataset whose entries hold no array has no mask at all
    none = _HostDataset(DATA, device=0, presence=[None, 1.0, None])
    assert none.presence is None and none.masked == [False] * 3
    _Recorder.calls = []
    trained(none, np.arange(N))
    assert none.last_weights_route is None and not presence_calls()


def test_a_mask_on_a_csr_modality_raises_valueerror_on_the_host(recorded):
    mods = [sp.csr_matrix(DATA[0] * (DATA[0] > 0.6)), DATA[1], DATA[2]]
    ds = _HostDataset(mods, device=0, keep_sparse=True, presence=[None, None, P[:, 2]])
    assert ds.sparse == [True, False, False] and ds.masked == [False, False, True]
    learner = MultimodalLearner(['a', 'b', 'c'], list(ds.dims), [1.0, 0.5, 2.0], K)
    with pytest.raises(ValueError) as e:
        ds.train(learner, np.arange(N), 2, init_dictionary=np.full((K, 16), 1.0 / 16))
    assert 'CSR' in str(e.value)
    assert not _Recorder.calls                      # before a context exists
    learner.dico = np.full((K, 16), 1.0 / 16)
    with pytest.raises(ValueError) as e:
        ds.reconstruct_internal_multi(learner, ['a', 'c'], [0, 1], 2)
    assert 'CSR' in str(e.value) and not _Recorder.calls
    with pytest.raises(ValueError):
        ds.presence_route([2, 0])
    # a masked subset of dense modalities of such a dataset runs; the CSR modality without the masked one runs the sparse branch
    ds.reconstruct_internal_multi(learner, ['b', 'c'], [0, 1], 2)
    assert ds.last_weights_route == 'presence' and len(presence_calls()) == 1 and 'upload_csr_device_rows' not in names()
    _Recorder.calls = []
    ds.reconstruct_internal_multi(learner, ['a', 'b'], [0, 1], 2)
    assert ds.last_weights_route is None and not presence_calls() and 'upload_csr_device_rows' in names()
    # the mask on the CSR modality itself
    with pytest.raises(ValueError):
        _HostDataset(mods, device=0, keep_sparse=True, presence=[P[:, 0], None, None]).reconstruct_internal(learner, 'a', [0], 2)


def test_a_16_bit_mode_runs_the_masked_call_in_f32(recorded, monkeypatch, capsys):
    monkeypatch.setenv('KLNMF_PRECISION', 'f16')
    ds = _HostDataset(DATA, device=0, presence=MASKS)
    trained(ds, np.arange(N))
    assert recorded.opened == ['f32']
    v = [c for c in _Recorder.calls if c[0] == 'upload_V_device_rows_dt']
    assert [c[1][0] for c in v] == [b.data_ptr() for b in ds.blocks] and not any(c[1][1] for c in v)       # the float32 blocks
    (_, args, _), = presence_calls()
    assert args[1] is True                          # the mask stays float64; the kernel casts it


# ---- the experiment driver ---------------------------------------------------------------------------------------------------------
def test_perform_one_run_forwards_the_mask_or_refuses_another(monkeypatch):
    made = []

    class Stop(Exception):
        pass

    class Fake(object):
        def __init__(self, data, device=None, keep_sparse=False, presence=None):
            made.append((keep_sparse, presence))
            raise Stop()
    monkeypatch.setattr(device_data, 'DeviceDataset', Fake)
    with pytest.raises(Stop):
        device_experiment.perform_one_run(DATA, 'abc', [1., 1., 1.], K, 2, 2, [0], [1], [2], [0], [0], presence=MASKS)
    assert made == [(False, MASKS)]
    monkeypatch.undo()
    ds = _HostDataset(DATA, device=0, presence=MASKS)
    assert ds.same_presence(MASKS) and ds.same_presence([P[:, :1], 1.0, P[:, 2]]) and not ds.same_presence(None)
    assert not ds.same_presence([P[:, 0], None, None]) and not ds.same_presence([P[:, 0], np.ones(N), P[:, 2]])
    other = [P[:, 0], None, 1.0 - P[:, 2]]
    with pytest.raises(ValueError) as e:
        device_experiment.perform_one_run(ds, 'abc', [1., 1., 1.], K, 2, 2, [0], [1], [2], [0], [0], presence=other)
    assert 'presence' in str(e.value)
    assert 'presence' in inspect.signature(device_experiment.run_sweep).parameters
    with pytest.raises(ValueError):                 # checked before any worker starts
        device_experiment.run_sweep(DATA, [0] * N, 'abc', [2], 1, presence=[np.ones(N - 1), None, None])


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_new_export_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'klnmf.h')).read()
    lib = _native.load()
    name = 'klnmf_upload_presence_device_rows'
    assert re.search(r'^int %s\s*\(' % name, header, flags=re.M)
    assert name in _native.SIGNATURES and hasattr(lib, name)
    assert len(_native.SIGNATURES[name][1]) == 11
    assert callable(_native.Context.upload_presence_device_rows)
    comment = header[:header.index('int %s(' % name)].rsplit('/*', 1)[1]
    assert 'the reference has no counterpart' in comment
    declared = set(re.findall(r'^(?:int|const char \*)\s*(klnmf_\w+)\s*\(', header, flags=re.M))
    assert declared == set(_native.SIGNATURES) and len(declared) == 79
    for doc in ('README.md', 'INTEGRATION.md', 'DESIGN.md'):
        text = open(os.path.join(ROOT, doc)).read()
        assert '79 exports' in text and name in text, doc
    csrc = os.path.join(ROOT, 'multimodal_amd', 'csrc')
    kernels = re.sub(r'//[^\n]*', '', open(os.path.join(csrc, 'presence.hip.h')).read())
    assert 'k_presence_gather' in kernels and 'k_presence_rows_check' in kernels


# ---- what it is for ----------------------------------------------------------------------------------------------------------------
def test_the_mask_recovers_an_absent_modality_on_the_reference():
    X, Xz, absent, Pm, H0 = dc.imputation_case()
    assert X.shape == (dc.IMPUTE_N, sum(dc.IMPUTE_DIMS)) and np.linalg.matrix_rank(X) == dc.IMPUTE_K
    assert 30 <= absent.sum() <= 60 and not Xz[absent, dc.IMPUTE_DIMS[0]:].any() and np.array_equal(Xz[~absent], X[~absent])
    ones = np.ones_like(Pm)
    errs = {}
    for iters in (dc.IMPUTE_ITERS, 300):
        Wm, Hm, _ = pc.ref_fit_p(Xz, Pm, dc.IMPUTE_BOUNDS, H0, iters)
        Wu, Hu, _ = pc.ref_fit_p(Xz, ones, dc.IMPUTE_BOUNDS, H0, iters)
        errs[iters] = dc.absent_block_error(X, absent, Wm, Hm), dc.absent_block_error(X, absent, Wu, Hu)
        print('%d iterations: masked %.5f, unmasked %.5f' % ((iters,) + errs[iters]))
        assert errs[iters][1] >= 0.99                                          # the unmasked fit learns the zeros
        assert errs[iters][0] * dc.IMPUTE_GAIN <= errs[iters][1]
    assert errs[dc.IMPUTE_ITERS][0] <= dc.IMPUTE_CEILING
    assert errs[300][0] < errs[dc.IMPUTE_ITERS][0]                             # and keeps converging on the block it never saw
