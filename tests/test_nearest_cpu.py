"""The fused nearest-example search without a GPU: the exports of include/klnmf_nearest.h, and the 'fused' route of the device
evaluations -- which searches it lists, in which order, how many calls it makes and how indices become labels -- with recording
stand-ins for `_native.nearest_many_device` and `_native.all_distances_device` that answer from numpy
(tests.eval_cases.kernel_order_distances; np.argmin) on an evaluation whose device matrices are CPU tensors."""
import ctypes
import zlib

import numpy as np
import pytest

from multimodal_amd import _native, device_data, device_experiment as dx
from multimodal_amd.learner import MultimodalLearner
from tests import eval_cases as evc
from tests.test_batch_csr_cpu import check_header_tables, declared_in, other_headers

NEW = {'klnmf_nearest_work_bytes', 'klnmf_nearest_many_device', 'klnmf_nearest'}
OTHERS = other_headers('klnmf_nearest.h')
FOUR = [metric for metric, _suffix in dx.DEVICE_MEASURES]


# ---- the bindings -------------------------------------------------------------------------------------------------------------------
def test_every_declared_nearest_symbol_is_bound_and_exported():
    declared = declared_in('klnmf_nearest.h')
    assert declared == NEW == set(_native.NEAREST_SIGNATURES)
    lib = _native.load()
    for name in declared:
        assert hasattr(lib, name), name
    for header in OTHERS:
        assert not (declared & declared_in(header)), header
    for name in ('nearest_work_bytes', 'nearest_many_device', 'nearest'):
        assert callable(getattr(_native, name))
    assert ctypes.sizeof(_native.NearestJob) == 56                 # klnmf_nearest_job: two pointers and five int64


def test_the_other_headers_declare_what_they_declared():
    check_header_tables()                # (and NEW is this header's own table: the test above)


def test_the_workspace_size_and_the_masks_are_host_arithmetic():
    small, more_rows, more_jobs = _native.nearest_work_bytes(1, 5), _native.nearest_work_bytes(1, 6), _native.nearest_work_bytes(2, 5)
    assert more_rows == small + 4 and more_jobs > small and _native.nearest_work_bytes(0, 0) == 0
    with pytest.raises(_native.NativeError):
        _native.nearest_work_bytes(-1, 0)
    with pytest.raises(_native.NativeError):
        _native.nearest_work_bytes(1, (1 << 24) + 1)
    assert _native.metric_mask(FOUR) == 0b11011 and _native.mask_metrics(0b11011) == [0, 1, 3, 4]
    assert _native.mask_metrics(_native.DIST_MASK_ALL) == [0, 1, 2, 3, 4]


# ---- the routing --------------------------------------------------------------------------------------------------------------------
def host_matrix(ptr, rows, ld, d):
    if rows == 0 or d == 0:
        return np.zeros((rows, d))
    flat = np.ctypeslib.as_array((ctypes.c_double * ((rows - 1) * ld + d)).from_address(ptr))
    return np.lib.stride_tricks.as_strided(flat, shape=(rows, d), strides=(8 * ld, 8)).copy()


def fingerprint(A, B):
    return (A.shape, B.shape, zlib.crc32(A.tobytes()), zlib.crc32(B.tobytes()))


class Recorder(object):
    """Stand-ins for the two device searches: they answer from numpy in the kernels' order and record what they were asked."""

    def __init__(self, monkeypatch):
        self.fused, self.matrix = [], []          # per call: the list of job fingerprints / (fingerprint, metric)
        monkeypatch.setattr(_native, 'nearest_many_device', self.nearest_many_device)
        monkeypatch.setattr(_native, 'all_distances_device', self.all_distances_device)

    def nearest_many_device(self, jobs, mask, d_idx, d_dist, d_work, work_bytes, f64=True, device=0):
        jobs = list(jobs)
        order = _native.mask_metrics(mask)
        rows = sum(j[4] for j in jobs)
        assert f64 and d_dist is None and work_bytes == _native.nearest_work_bytes(len(jobs), rows)
        seen, row0 = [], 0
        if rows:
            out = np.ctypeslib.as_array((ctypes.c_int32 * (rows * len(order))).from_address(d_idx)).reshape(rows, len(order))
        for dA, lda, dB, ldb, na, nb, d in jobs:
            A, B = host_matrix(dA, na, lda, d), host_matrix(dB, nb, ldb, d)
            seen.append(fingerprint(A, B))
            for s, metric in enumerate(order if na else []):
                out[row0:row0 + na, s] = np.argmin(evc.kernel_order_distances(A, B, metric), axis=1)
            row0 += na
        self.fused.append(seen)

    def all_distances_device(self, dA, lda, dB, ldb, dout, na, nb, d, metric, f64=True, device=0):
        A, B = host_matrix(dA, na, lda, d), host_matrix(dB, nb, ldb, d)
        self.matrix.append((fingerprint(A, B), metric))
        np.ctypeslib.as_array((ctypes.c_double * (na * nb)).from_address(dout))[:] = evc.kernel_order_distances(A, B, metric).ravel()


def cpu_tensor(seed, shape):
    import torch
    return torch.from_numpy(np.random.default_rng(seed).random(shape) + 0.05)


class CpuEvaluation(device_data.DeviceEvaluation):
    """A DeviceEvaluation whose matrices are CPU tensors drawn from seeds of (learner, modalities, rows): no device, no fit; the
    searches (`found_labels`, `found_labels_many`) are the class's own."""

    def __init__(self, dataset, learner, iter_test):
        import torch
        self.torch, self.ds, self.learner, self.dev = torch, dataset, learner, torch.device('cpu')
        self.k = learner.k
        self.tag = getattr(learner, 'tag', 0)

    def _seed(self, *what):
        return zlib.crc32(repr((self.tag,) + what).encode())

    def internal(self, mods, rows):
        return cpu_tensor(self._seed('internal', tuple(mods), tuple(rows)), (len(rows), self.k))

    @staticmethod
    def internal_many(evaluations, mods, rows_list):
        return [ev.internal(mods, rows) for ev, rows in zip(evaluations, rows_list)]

    def raw(self, which, rows):
        return cpu_tensor(self._seed('raw', which, tuple(rows)), (len(rows), self.learner.dim[which]))

    def reconstruct(self, internal, dest_mod):
        d = self.learner.dim[self.learner.get_index(dest_mod)]
        return internal @ cpu_tensor(self._seed('dico', dest_mod), (self.k, d))


class NoDataset(object):
    """What `_sweep_batch` asks of a dataset besides the evaluation: sizes and a training that is not under test."""

    def __init__(self, dims, n_samples):
        self.dims, self.n_samples = list(dims), n_samples

    def train_many(self, learners, rows_list, iterations, init_dictionaries=None):
        for tag, learner in enumerate(learners):
            learner.tag = tag
        return learners


def learner_of(dims, k=5):
    return MultimodalLearner(['m%d' % i for i in range(len(dims))], list(dims), [1.0] * len(dims), k)


ROWS_TEST, ROWS_EX = [3, 9, 4, 11, 17, 8, 2], [0, 5, 10, 15]
LABELS_TEST, LABELS_EX = [0, 1, 0, 2, 3, 1, 0], [10, 11, 12, 13]


@pytest.mark.parametrize('dims,evaluate_', [((6, 9), dx.evaluate_on_device), ((6, 9, 4), dx.evaluate_internal_on_device)],
                         ids=['two', 'three'])
def test_a_fused_evaluation_lists_the_default_route_s_twelve_searches_in_its_order(monkeypatch, dims, evaluate_):
    rec = Recorder(monkeypatch)
    learner = learner_of(dims)
    args = (None, learner, ROWS_TEST, ROWS_EX, LABELS_TEST, LABELS_EX, 7)
    default = evaluate_(*args, ev=CpuEvaluation(None, learner, 7))
    assert rec.fused == [] and len(rec.matrix) == 48                       # default arguments: the fused entry is never called
    assert [m for _f, m in rec.matrix] == FOUR * 12
    in_order = [f for f, _m in rec.matrix[::4]]
    assert all(rec.matrix[4 * q + s][0] == in_order[q] for q in range(12) for s in range(4))
    del rec.matrix[:]
    fused = evaluate_(*args, ev=CpuEvaluation(None, learner, 7), search='fused')
    assert rec.matrix == [] and len(rec.fused) == 1 and rec.fused[0] == in_order
    assert list(fused) == list(default) and len(fused) == 96
    for key in default:
        assert fused[key] == default[key], key
    assert set(l for key in fused if key.startswith('found_') for l in fused[key]) <= set(LABELS_EX)
    with pytest.raises(ValueError):
        evaluate_(*args, ev=CpuEvaluation(None, learner, 7), search='device')
    assert rec.matrix == [] and len(rec.fused) == 1


@pytest.mark.parametrize('dims', [(6, 9), (6, 9, 4)], ids=['two', 'three'])
def test_a_batch_of_three_runs_makes_one_call_with_thirty_six_jobs(monkeypatch, dims):
    rec = Recorder(monkeypatch)
    monkeypatch.setattr(device_data, 'DeviceEvaluation', CpuEvaluation)
    labels = [i % 4 for i in range(40)]
    args = (NoDataset(dims, 40), ['m%d' % i for i in range(len(dims))], [1.0] * len(dims), labels, [0, 1, 2, 3], 5, [0, 1, 2], 3, 3, .2, 11,
            None)
    default = dx._sweep_batch(*args)
    assert rec.fused == [] and len(rec.matrix) == 3 * 48
    per_run = [[f for f, _m in rec.matrix[48 * r:48 * (r + 1):4]] for r in range(3)]
    del rec.matrix[:]
    fused = dx._sweep_batch(*args, search='fused')
    assert rec.matrix == [] and len(rec.fused) == 1 and len(rec.fused[0]) == 36
    assert rec.fused[0] == per_run[0] + per_run[1] + per_run[2]
    assert fused == default and [run for _k, run, _s in fused] == [0, 1, 2]
    with pytest.raises(ValueError):
        dx._sweep_batch(*args, search='many')


def test_indices_become_labels_with_each_search_s_own_examples(monkeypatch):
    rec = Recorder(monkeypatch)
    ev = CpuEvaluation(None, learner_of((6, 9)), 7)
    shapes = ((5, 3, 8), (0, 2, 8), (4, 6, 3), (2, 1, 70))
    searches = [(cpu_tensor(50 + q, (na, d)), cpu_tensor(60 + q, (nb, d)), ['s%d_%d' % (q, j) for j in range(nb)])
                for q, (na, nb, d) in enumerate(shapes)]
    got = ev.found_labels_many(searches, FOUR)
    assert len(rec.fused) == 1 and len(rec.fused[0]) == 4 and len(got) == 4
    for (test, examples, labels_ex), found in zip(searches, got):
        assert list(found) == FOUR
        for metric in FOUR:
            D = evc.kernel_order_distances(test.numpy(), examples.numpy(), metric)
            assert found[metric] == [labels_ex[j] for j in np.argmin(D, axis=1)]
            assert test.shape[0] == 0 or found[metric] == ev.found_labels(test, examples, labels_ex, metric)
    assert got[1] == {metric: [] for metric in FOUR}
    import torch
    with pytest.raises(ValueError):
        ev.found_labels_many([(searches[0][0].to(torch.float32), searches[0][1], searches[0][2])], FOUR)
    with pytest.raises(ValueError):
        ev.found_labels_many([(searches[0][0], searches[2][1], searches[2][2])], FOUR)


def test_an_unknown_search_is_refused_before_anything_runs(monkeypatch):
    rec = Recorder(monkeypatch)
    for call in (lambda: dx.run_sweep([np.ones((4, 3)), np.ones((4, 2))], [0, 1, 0, 1], ['a', 'b'], [2], 1, search='both'),
                 lambda: dx.perform_one_run(object(), ['a', 'b'], [1, 1], 2, 1, 1, [0], [1], [2], [0], [0], search=None)):
        with pytest.raises(ValueError, match='search'):
            call()
    assert rec.fused == [] and rec.matrix == []
    assert dx.SEARCHES == ('matrix', 'fused')
