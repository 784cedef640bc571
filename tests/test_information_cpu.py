"""The atom x label information matrix without a GPU: the exports of include/klnmf_information.h, the restatement and the new
`lib.metrics` functions against the reference's own outputs (G20), the bin rule against np.histogram as exact integers, the
routing of `DeviceEvaluation.information_matrix_many` / `perform_one_run(information=...)` with a recording stand-in for
`_native.information_many_device` that answers from numpy, and the host-side refusals."""
import ctypes
import os

import numpy as np
import pytest

from multimodal_amd import _native, device_data, device_experiment as dx, evaluation
from multimodal_amd.lib import metrics
from tests import information_cases as ic
from tests.test_batch_csr_cpu import check_header_tables, declared_in, other_headers
from tests.test_nearest_cpu import CpuEvaluation, host_matrix, learner_of

NEW = {'klnmf_information_work_bytes', 'klnmf_information_many_device', 'klnmf_information'}
OTHERS = other_headers('klnmf_information.h')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g20_information.npz')


# ---- the bindings -------------------------------------------------------------------------------------------------------------------
def test_every_declared_information_symbol_is_bound_and_exported():
    declared = declared_in('klnmf_information.h')
    assert declared == NEW == set(_native.INFORMATION_SIGNATURES)
    lib = _native.load()
    for name in declared:
        assert hasattr(lib, name), name
    for header in OTHERS:
        assert not (declared & declared_in(header)), header
    for name in ('information_work_bytes', 'information_many_device', 'information', 'information_route'):
        assert callable(getattr(_native, name))
    assert ctypes.sizeof(_native.InformationJob) == 40             # klnmf_information_job: two pointers and three int64


def test_the_other_headers_declare_what_they_declared():
    check_header_tables()                # (and NEW is this header's own table: the test above)


def test_the_workspace_size_and_the_route_are_host_arithmetic():
    base = _native.information_work_bytes(1, 5, 10, 10)
    assert _native.information_work_bytes(1, 6, 10, 10) > base and _native.information_work_bytes(2, 5, 10, 10) > base
    assert _native.information_work_bytes(1, 5, 10, 12) == base + 5 * 10 * 2 * 4              # the counts alone grow with the bins
    for bad in ((-1, 5, 10, 10), (1, -1, 10, 10), (1, 5, 0, 10), (1, 5, 10, 0), (1, 5, 10, 257), (1, 5, 65537, 10),
                ((1 << 16) + 1, 5, 10, 10), (1, 1 << 20, 64, 8)):
        with pytest.raises(_native.NativeError):
            _native.information_work_bytes(*bad)
    assert _native.information_route(10, 10) == ('lds', 64) and _native.information_route(1, 1) == ('lds', 64)
    assert _native.information_route(8, 16) == ('lds', 64) and _native.information_route(17, 16) == ('lds-shrunk', 30)
    assert _native.information_route(50, 10) == ('lds-shrunk', 16) and _native.information_route(40, 100) == ('lds-shrunk', 2)
    assert _native.information_route(32, 256) == ('lds-shrunk', 1) and _native.information_route(65, 128) == ('global', 0)
    header = open(os.path.join(os.path.dirname(GOLDEN), '..', '..', 'include', 'klnmf_information.h')).read()
    assert '#define KLNMF_INFORMATION_LDS_BYTES %d' % _native.INFORMATION_LDS_BYTES in header
    kernels = open(os.path.join(os.path.dirname(GOLDEN), '..', '..', 'multimodal_amd', 'csrc', 'information.hip.h')).read()
    assert 'kInfoRows = %d;' % _native.INFORMATION_ROWS in kernels and 'kInfoLdsBytes = %d;' % _native.INFORMATION_LDS_BYTES in kernels
    assert ic.R == _native.INFORMATION_ROWS


# ---- the arithmetic -----------------------------------------------------------------------------------------------------------------
def golden_tables():
    g = np.load(GOLDEN)
    for i, (rows, cols) in enumerate(g['shapes']):
        c = g['counts'][i, :rows, :cols]
        yield i, 1. * c / c.sum(), g


def test_the_restatement_and_lib_metrics_match_the_reference_on_g20():
    seen = 0
    for i, p, g in golden_tables():
        for got in (ic.table_information(p), metrics.mutual_information(p)):
            assert abs(got - g['mutual_information'][i]) <= 1e-15, (i, got)
        for got in (ic.table_entropy(p), metrics.entropy(p)):
            assert abs(got - g['entropy'][i]) <= 1e-15, (i, got)
        for axis in (0, 1):
            for got in (ic.table_conditional_entropy(p, axis), metrics.conditional_entropy(p, axis=axis)):
                assert abs(got - g['conditional_entropy_%d' % axis][i]) <= 1e-15, (i, axis, got)
        seen += 1
    assert seen >= 200
    g = np.load(GOLDEN)
    kinds = [g['counts'][i, :r, :c] for i, (r, c) in enumerate(g['shapes'])]
    assert any((c == 0).any() and (c != 0).sum() > 1 for c in kinds)          # zero cells
    assert any((c[0] == 0).all() and c.sum() > 0 for c in kinds)              # a zero row
    assert any((c != 0).sum() == 1 for c in kinds)                            # a single non-zero cell


def test_lib_metrics_has_the_reference_s_statistics():
    with pytest.raises(AssertionError):
        metrics.mutual_information(np.ones((2, 3)))                           # does not sum to 1
    with pytest.raises(AssertionError):
        metrics.mutual_information(np.ones(4) / 4)                            # not a table
    with pytest.raises(AssertionError):
        metrics.conditional_entropy(np.ones((2, 2)))
    assert metrics.mutual_information(np.array([[.5, 0], [0, .5]])) == pytest.approx(np.log(2), abs=1e-15)
    assert metrics.mutual_information(np.full((2, 2), .25)) == 0.0
    assert metrics.entropy(np.array([.5, .5, 0])) == pytest.approx(np.log(2), abs=1e-15)
    X = np.array([[1., 0, 0, 0], [1, 1, 1, 1]])
    assert metrics.real_sparsity(X) == 1 - 5 / 8
    import scipy.sparse as sp
    assert metrics.real_sparsity(sp.csr_matrix(X)) == 1 - 5 / 8
    # one row with a single entry (sparseness 1) and one flat row (sparseness 0): the mean ratio of the norms is (1 + 2) / 2
    assert metrics.hoyer_sparseness(X) == pytest.approx((2 - 1.5) / (2 - 1), abs=1e-7)
    assert metrics.hoyer_sparseness(X, axis=0, eps=0) == pytest.approx((np.sqrt(2) - np.mean([np.sqrt(2)] + [1] * 3)) / (np.sqrt(2) - 1))


def test_the_bin_rule_equals_np_histogram_on_adversarial_vectors():
    wrong = 0
    seen = 0
    for v in ic.adversarial_vectors():
        v64 = v.astype(np.float64)
        want = np.histogram(v64, bins=10, range=(float(v.min()), float(v.max())))[0]
        lo, hi, e = ic.rule_edges(float(v64.min()), float(v64.max()), 10)
        assert np.array_equal(e, np.linspace(lo, hi, 11))
        wrong += not np.array_equal(ic.rule_counts(v), want)
        seen += 1
    assert seen == 3000 and wrong == 0
    for bins in (1, 2, 16):
        for v in ic.adversarial_vectors(count=120, seed=bins, bins=bins):
            want = np.histogram(v.astype(np.float64), bins=bins, range=(float(v.min()), float(v.max())))[0]
            assert np.array_equal(ic.rule_counts(v, bins), want), bins


def test_the_restatement_counts_every_row_once_and_handles_the_special_atoms():
    A = ic.coefficients(3, 50, 7)
    lab = ic.labels_of(3, 50, 4)
    counts, info = ic.reference_information(A, lab, 4, 10)
    assert counts.shape == (7, 4, 10) and info.shape == (4, 7)
    assert (counts.sum(axis=(1, 2)) == 50).all()
    assert (counts[:, 2] == 0).all() and (np.abs(info[2]) <= 1e-15).all()     # the label no row carries (the row sums round)
    assert counts[6, :, 5].sum() == 50 and counts[5, :, 5].sum() == 50        # constant and all-zero atoms: one bin, the middle one
    assert (np.abs(info[:, 5:]) <= 1e-15).all()
    one = ic.reference_information(A, ic.labels_of(3, 50, 3, 'one'), 3, 10)[1]
    assert (np.abs(one) <= 1e-15).all()                                       # one label on every row: nothing to know
    assert ic.information_bar(10) == 1e-12 and ic.information_bar(16) == 1e-12 and ic.information_bar(256) == 1.6e-11


# ---- the routing --------------------------------------------------------------------------------------------------------------------
class Recorder(object):
    """A stand-in for the device analysis: answers from the restatement and records what it was asked."""

    def __init__(self, monkeypatch):
        self.calls = []
        monkeypatch.setattr(_native, 'information_many_device', self.information_many_device)

    def information_many_device(self, jobs, n_labels, bins, d_info, d_counts, d_work, work_bytes, f64=True, device=0):
        jobs = list(jobs)
        atoms = sum(j[4] for j in jobs)
        assert f64 and d_counts is None and work_bytes == _native.information_work_bytes(len(jobs), atoms, n_labels, bins)
        out = np.ctypeslib.as_array((ctypes.c_double * (atoms * n_labels)).from_address(d_info))
        seen, at = [], 0
        for dA, lda, d_labels, n, k in jobs:
            A = host_matrix(dA, n, lda, k)
            lab = np.ctypeslib.as_array((ctypes.c_int32 * n).from_address(d_labels)).copy()
            out[at:at + n_labels * k] = ic.reference_information(A, lab, n_labels, bins)[1].ravel()
            at += n_labels * k
            seen.append((A, lab))
        self.calls.append((seen, n_labels, bins))


def test_information_matrix_many_makes_one_native_call_for_all_runs(monkeypatch):
    rec = Recorder(monkeypatch)
    evs = []
    for tag in range(3):
        ev = CpuEvaluation(None, learner_of((6, 9), k=4 + tag), 7)
        ev.tag = tag
        evs.append(ev)
    rows_list = [[3, 9, 4, 11, 17], [1, 2, 3, 4, 5, 6, 7], [8, 0, 2]]
    labels_list = [[0, 1, 0, 2, 1], [2, 2, 0, 1, 0, 0, 1], [1, 1, 0]]
    got = device_data.DeviceEvaluation.information_matrix_many(evs, ['m0', 'm1'], rows_list, labels_list, 3, bins=4)
    assert len(rec.calls) == 1 and len(rec.calls[0][0]) == 3 and rec.calls[0][1:] == (3, 4)
    for ev, rows, labels, mine, (A, lab) in zip(evs, rows_list, labels_list, got, rec.calls[0][0]):
        internal = ev.internal(['m0', 'm1'], rows).numpy()
        assert np.array_equal(A, internal) and list(lab) == labels
        assert mine.shape == (3, ev.k) and mine.dtype == np.float64
        assert np.array_equal(mine, ic.reference_information(internal, labels, 3, 4)[1])
    single = evs[1].information_matrix(['m0', 'm1'], rows_list[1], labels_list[1], 3, bins=4)
    assert len(rec.calls) == 2 and len(rec.calls[1][0]) == 1 and np.array_equal(single, got[1])
    assert device_data.DeviceEvaluation.information_matrix_many([], ['m0'], [], [], 3) == [] and len(rec.calls) == 2
    for bad in (dict(labels_list=[[0, 1, 0, 2, 3]] + labels_list[1:]), dict(labels_list=[[0, 1, 0, 2]] + labels_list[1:]),
                dict(labels_list=[[0, 1, 0, 2, 1.5]] + labels_list[1:]), dict(labels_list=labels_list[:2]), dict(bins=0), dict(bins=257)):
        args = dict(rows_list=rows_list, labels_list=labels_list, n_labels=3, bins=4)
        args.update(bad)
        with pytest.raises(ValueError):
            device_data.DeviceEvaluation.information_matrix_many(evs, ['m0', 'm1'], **args)
    assert len(rec.calls) == 2


class FakeDataset(object):
    dims = [6, 9]
    n_samples = 40
    keep_sparse_asked = False

    def train(self, learner, rows, iterations, init_dictionary=None):
        learner.tag = 5


def test_perform_one_run_adds_the_matrix_only_when_asked(monkeypatch):
    rec = Recorder(monkeypatch)
    monkeypatch.setattr(device_data, 'DeviceDataset', FakeDataset)
    monkeypatch.setattr(device_data, 'DeviceEvaluation', CpuEvaluation)
    monkeypatch.setattr(dx, 'evaluate_on_device', lambda *a, **kw: {'score_stub': 1.0})
    rows_test, labels_test, labels_ex = [3, 9, 4, 11, 17, 8], ['b', 'a', 'b', 'd', 'a', 'b'], ['a', 'b', 'c']
    args = (FakeDataset(), ['m0', 'm1'], [1.0, 1.0], 5, 3, 7, [20, 21, 22], rows_test, [0, 5, 10], labels_test, labels_ex)
    _learner, default = dx.perform_one_run(*args)
    assert rec.calls == [] and sorted(default) == ['dictionary', 'score_stub', 'test', 'train']
    _learner, explicit = dx.perform_one_run(*args, information=False)
    assert rec.calls == [] and sorted(explicit) == sorted(default)
    learner, asked = dx.perform_one_run(*args, information=True)
    assert len(rec.calls) == 1 and sorted(asked) == sorted(list(default) + ['information', 'information_labels'])
    assert asked['information_labels'] == ['a', 'b', 'c', 'd'] and asked['information'].shape == (4, 5)
    (A, lab), = rec.calls[0][0]
    assert rec.calls[0][1:] == (4, 10) and list(lab) == [1, 0, 1, 3, 0, 1]
    assert np.array_equal(A, CpuEvaluation(None, learner, 7).internal(['m0', 'm1'], rows_test).numpy())
    assert np.array_equal(asked['information'], ic.reference_information(A, lab, 4, 10)[1])
    assert (np.abs(asked['information'][2]) <= 1e-15).all()        # 'c' is an example's label only (the reference's row sums round)


# ---- the host-side refusals ---------------------------------------------------------------------------------------------------------
def test_information_matrix_refuses_on_the_host(monkeypatch):
    called = []
    monkeypatch.setattr(_native, 'information', lambda *a, **kw: called.append(a))
    A = ic.coefficients(1, 12, 3)
    lab = ic.labels_of(1, 12, 3)
    bad_A = A.copy()
    bad_A[4, 1] = np.nan
    inf_A = A.copy()
    inf_A[0, 0] = np.inf
    for args, kw in (((A, lab.astype(np.float64) + 0.5), {}), ((A, lab - 1), {}), ((A, lab), dict(n_labels=2)), ((A, lab[:-1]), {}),
                     ((A, lab), dict(n_labels=0)), ((A[:0], lab[:0]), {}), ((A[:, :0], lab), {}), ((A[0], lab[:3]), {}),
                     ((bad_A, lab), {}), ((inf_A, lab), {}), ((A, lab), dict(bins=0)), ((A, lab), dict(bins=257)),
                     ((A, ['x'] * 12), {})):
        with pytest.raises(ValueError):
            evaluation.information_matrix(*args, **kw)
    assert called == []
    evaluation.information_matrix(A, lab)                          # n_labels defaults to max(labels) + 1
    evaluation.information_matrix(A, lab.astype(np.float64), bins=3, return_counts=True)
    assert len(called) == 2 and called[0][2] == int(lab.max()) + 1 and called[1][1].dtype == np.int32
