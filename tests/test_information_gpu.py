"""The atom x label information matrix (include/klnmf_information.h, csrc/information.hip.h) against its fp64 restatement
(tests/information_cases.py: np.histogram per (atom, label) on the values widened to float64, then the reference's table formula).

  * counts: equal to np.histogram's as integers, on every shape, dtype, stride and counter route;
  * info: within information_cases.information_bar(B) = 1e-12 absolute for B <= 16 of the restatement (the derivation is there);
    the worst difference of a run is printed by `test_zz_report_the_worst_difference`;
  * identical bits from call to call, from a many-call and its jobs alone, with the counts requested or not;
  * refusals write nothing; a bad label and a NaN coefficient name their job;
  * the device route of `DeviceEvaluation` equals the host route on the downloaded coefficients bit for bit.

Shapes: n in {1, 2, R - 1, R, R + 1, 3R + 5} (R = 1024 rows per workgroup chunk) x k in {1, 63, 64, 65, 200}, each pair once, with
L in {1, 2, 10, 17}, B in {1, 2, 10, 16}, the dtype, the row stride (k or k + 3) and the label layout cycling so that every value
of each occurs with small and large shapes; and one (L, B) per counter route on k = 3, n = 2R + 1."""
import itertools

import numpy as np
import pytest

from multimodal_amd import _native
from tests import information_cases as ic

pytestmark = pytest.mark.gpu

R = ic.R
NP = {False: np.float64, True: np.float32}
INFO_GUARD, COUNT_GUARD = -12345.0, -77
WORST = {}


def torch_mod():
    import torch
    return torch


class Job(object):
    """A host matrix and its labels on the device, rows `k + pad` elements apart."""

    def __init__(self, A, labels, pad=0):
        torch = torch_mod()
        self.A, self.labels = A, np.asarray(labels, dtype=np.int32)
        self.n, self.k = A.shape
        self.buf = torch.full((self.n, self.k + pad), -5.0, dtype=torch.float32 if A.dtype == np.float32 else torch.float64, device='cuda')
        self.buf[:, :self.k] = torch.from_numpy(np.ascontiguousarray(A)).to('cuda')
        self.d_labels = torch.from_numpy(self.labels).to('cuda')

    def entry(self):
        return (self.buf.data_ptr(), self.buf.stride(0), self.d_labels.data_ptr(), self.n, self.k)


def analyse(jobs, L, B, f32, with_counts=True, entries=None, work_bytes=None):
    """klnmf_information_many_device on `jobs` into guarded outputs: ([info (L, k) per job], [counts (k, L, B) per job] or None)."""
    torch = torch_mod()
    atoms = sum(j.k for j in jobs)
    info = torch.full((atoms * L + 8,), INFO_GUARD, dtype=torch.float64, device='cuda')
    counts = torch.full((atoms * L * B + 8,), COUNT_GUARD, dtype=torch.int32, device='cuda') if with_counts else None
    nbytes = _native.information_work_bytes(len(jobs), atoms, L, B)
    work = torch.zeros((nbytes + 64,), dtype=torch.uint8, device='cuda')
    _native.information_many_device(entries if entries is not None else [j.entry() for j in jobs], L, B, info.data_ptr(),
                                    counts.data_ptr() if with_counts else None, work.data_ptr(),
                                    nbytes if work_bytes is None else work_bytes, f64=not f32)
    info = info.cpu().numpy()
    assert (info[atoms * L:] == INFO_GUARD).all()
    if with_counts:
        counts = counts.cpu().numpy()
        assert (counts[atoms * L * B:] == COUNT_GUARD).all()
    out_i, out_c, at = [], [], 0
    for j in jobs:
        out_i.append(info[at * L:(at + j.k) * L].reshape(L, j.k).copy())
        if with_counts:
            out_c.append(counts[at * L * B:(at + j.k) * L * B].reshape(j.k, L, B).copy())
        at += j.k
    return out_i, (out_c if with_counts else None)


def check_against_the_restatement(A, labels, L, B, f32, pad=0, tag=None):
    job = Job(A, labels, pad)
    (info,), (counts,) = analyse([job], L, B, f32)
    want_counts, want_info = ic.reference_information(A, labels, L, B)
    assert np.array_equal(counts, want_counts), tag
    worst = float(np.max(np.abs(info - want_info)))
    print('information %s: worst |info - restatement| = %.3e (bar %.1e)' % (tag, worst, ic.information_bar(B)))
    WORST[tag] = (worst, B)
    assert worst <= ic.information_bar(B), (tag, worst)
    return info, counts


NS, KS, LS, BS = (1, 2, R - 1, R, R + 1, 3 * R + 5), (1, 63, 64, 65, 200), (1, 2, 10, 17), (1, 2, 10, 16)
CASES = []
for i, (n, k) in enumerate(itertools.product(NS, KS)):
    # (n, k) pairs in row-major order: L follows i, B follows i + i // 4 (so that the 16 (L, B) pairs all occur), the dtype
    # alternates, the stride alternates in pairs, every seventh case puts one label on all rows
    CASES.append((n, k, LS[i % 4], BS[(i + i // 4) % 4], bool(i % 2), 3 * ((i // 2) % 2), 'one' if i % 7 == 3 else 'spread'))
# the largest shape with many labels and bins, which the cycle above does not reach
CASES += [(3 * R + 5, 200, 17, 16, False, 3, 'spread'), (3 * R + 5, 200, 10, 10, True, 0, 'spread')]


def test_the_cases_cover_what_they_promise():
    assert len(CASES) == 32 and len(set(CASES)) == 32
    assert {(L, B) for _n, _k, L, B, _f, _p, _kind in CASES} == set(itertools.product(LS, BS))
    for f32, pad in itertools.product((False, True), (0, 3)):
        mine = [c for c in CASES if c[4] == f32 and c[5] == pad]
        assert {c[0] for c in mine} >= {1, 3 * R + 5} and any(c[1] == 200 for c in mine) and any(c[1] == 1 for c in mine), (f32, pad)
    assert {c[6] for c in CASES} == {'one', 'spread'} and {c[1] for c in CASES if c[6] == 'one'} == {1, 64, 65, 200}


@pytest.mark.parametrize('n,k,L,B,f32,pad,kind', CASES, ids=['n%d-k%d-L%d-B%d-%s-pad%d-%s' % (c[0], c[1], c[2], c[3], 'f32' if c[4] else 'f64',
                                                                                         c[5], c[6]) for c in CASES])
def test_every_shape_against_the_restatement(n, k, L, B, f32, pad, kind):
    A = ic.coefficients(n * 1000 + k, n, k, bins=B, dtype=NP[f32])
    labels = ic.labels_of(n + k, n, L, kind)
    info, counts = check_against_the_restatement(A, labels, L, B, f32, pad, tag='n%d-k%d-L%d-B%d-f32=%d' % (n, k, L, B, f32))
    assert (counts.sum(axis=(1, 2)) == n).all()
    if L == 1 or kind == 'one':
        assert (info == 0).all()                                    # one label on every row: p / (pr pc) is exactly 1
    if L >= 3 and kind == 'spread':
        assert (counts[:, L - 2] == 0).all() and (info[L - 2] == 0).all()           # the label no row carries


ROUTES = [('lds', 10, 10), ('lds-shrunk', 40, 100), ('global', 65, 128)]


@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
@pytest.mark.parametrize('route,L,B', ROUTES, ids=[r[0] for r in ROUTES])
def test_every_counter_route_counts_the_same_integers(route, L, B, f32):
    assert _native.information_route(L, B)[0] == route
    n, k = 2 * R + 1, 3
    A = ic.coefficients(77, n, k, bins=B, dtype=NP[f32])
    A[:, 0] = ic.coefficients(78, n, 5, bins=B, dtype=NP[f32])[:, 1]           # an atom one ulp either side of the edges
    labels = ic.labels_of(5, n, L)
    check_against_the_restatement(A, labels, L, B, f32, tag='route-%s-f32=%d' % (route, f32))


@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
def test_edges_and_their_neighbours_at_several_widths(f32):
    """The atoms on and next to linspace edges at B = 10 and 16, wide enough (k = 70) to put them into the second tile."""
    for B in (10, 16):
        n, k, L = R + 37, 70, 5
        A = ic.coefficients(B, n, k, bins=B, dtype=NP[f32])
        check_against_the_restatement(A, ic.labels_of(B, n, L), L, B, f32, pad=3, tag='edges-B%d-f32=%d' % (B, f32))


def mixed_jobs(f32):
    torch = torch_mod()
    dt = NP[f32]
    shapes = ((R + 3, 5), (7, 65), (2 * R, 64), (300, 9))
    jobs = [Job(ic.coefficients(40 + q, n, k, dtype=dt), ic.labels_of(40 + q, n, 6), pad=3 if q == 1 else 0) for q, (n, k) in enumerate(shapes)]
    # the last job a strided view into a wider matrix: columns 4 .. 13 of 20
    wide = ic.coefficients(50, 300, 20, dtype=dt)
    view = Job(np.ascontiguousarray(wide[:, 4:13]), jobs[3].labels)
    view.buf = torch.from_numpy(wide).to('cuda')
    view.entry = lambda: (view.buf.data_ptr() + 4 * wide.itemsize, view.buf.stride(0), view.d_labels.data_ptr(), 300, 9)
    jobs[3] = view
    return jobs


@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
def test_a_many_call_equals_its_jobs_alone_and_two_calls_agree(f32):
    jobs = mixed_jobs(f32)
    L, B = 6, 10
    info, counts = analyse(jobs, L, B, f32)
    again, counts_again = analyse(jobs, L, B, f32)
    without, none = analyse(jobs, L, B, f32, with_counts=False)
    assert none is None
    for q, job in enumerate(jobs):
        (alone,), (alone_counts,) = analyse([job], L, B, f32)
        for other in (again[q], without[q], alone):
            assert np.array_equal(info[q].view(np.uint64), other.view(np.uint64)), q
        assert np.array_equal(counts[q], counts_again[q]) and np.array_equal(counts[q], alone_counts), q
        want_counts, want_info = ic.reference_information(job.A, job.labels, L, B)
        assert np.array_equal(counts[q], want_counts), q
        assert np.max(np.abs(info[q] - want_info)) <= ic.information_bar(B), q


def test_refusals_write_nothing_and_name_the_job():
    torch = torch_mod()
    good = Job(ic.coefficients(1, 40, 6), ic.labels_of(1, 40, 4))
    L, B = 4, 10
    e = good.entry()

    def refused(entries, L=L, B=B, f32=False, null=None, work_bytes=None, match=None):
        atoms = 6 * max(1, len(entries))
        info = torch.full((atoms * 4 + 8,), INFO_GUARD, dtype=torch.float64, device='cuda')
        counts = torch.full((atoms * 4 * 10 + 8,), COUNT_GUARD, dtype=torch.int32, device='cuda')
        nbytes = _native.information_work_bytes(3, 18, 4, 10)
        work = torch.zeros((nbytes,), dtype=torch.uint8, device='cuda')
        with pytest.raises(_native.NativeError, match=match) as err:
            if f32 == 'other':
                table = (_native.InformationJob * 1)(_native.InformationJob(*entries[0]))
                import ctypes
                _native._check(_native.load().klnmf_information_many_device(0, 2, L, B, ctypes.cast(table, ctypes.c_void_p), 1,
                                                                            ctypes.c_void_p(info.data_ptr()), None,
                                                                            ctypes.c_void_p(work.data_ptr()), nbytes))
            else:
                _native.information_many_device(entries, L, B, None if null == 'info' else info.data_ptr(), counts.data_ptr(),
                                                None if null == 'work' else work.data_ptr(),
                                                nbytes if work_bytes is None else work_bytes, f64=not f32)
        assert err.value.code == _native.ERR_ARG
        assert (info.cpu().numpy() == INFO_GUARD).all() and (counts.cpu().numpy() == COUNT_GUARD).all()
        assert not work.cpu().numpy().any()

    refused([e], null='info')
    refused([e], null='work')
    refused([(0, e[1], e[2], e[3], e[4])])                         # null A
    refused([(e[0], e[1], 0, e[3], e[4])])                         # null labels
    refused([(e[0], 5, e[2], e[3], e[4])])                         # lda < k
    refused([e], f32='other')                                      # a dtype other than f32 / f64
    refused([(e[0], e[1], e[2], 0, e[4])])                         # n < 1
    refused([(e[0], e[1], e[2], e[3], 0)])                         # k < 1
    refused([e], L=0)
    refused([e], B=0)
    refused([e], B=257)
    refused([e], L=65537)
    refused([(e[0], e[1], e[2], (1 << 30) + 1, e[4])])             # n beyond the limit
    refused([(e[0], 1 << 21, e[2], e[3], (1 << 20) + 1)])          # k beyond the limit
    refused([(e[0], 1 << 20, e[2], e[3], 1 << 20)], L=64, B=8)     # k * L * B beyond 2^28
    refused([e] * ((1 << 16) + 1))                                 # more jobs than the limit
    refused([e, e, e], work_bytes=_native.information_work_bytes(3, 18, 4, 10) - 1)
    # found on the device: the call names the first such job; the process stays usable
    for wrong in (-1, 4):
        labels = good.labels.copy()
        labels[17] = wrong
        bad = Job(good.A, labels)
        with pytest.raises(_native.NativeError, match=r'job 2: a label outside') as err:
            analyse([good, good, bad, bad], L, B, False)
        assert err.value.code == _native.ERR_ARG
    for value in (np.nan, np.inf, -np.inf):
        A = good.A.copy()
        A[33, 2] = value
        with pytest.raises(_native.NativeError, match=r'job 1: a coefficient that is not finite'):
            analyse([good, Job(A, good.labels), good], L, B, False)
        with pytest.raises(_native.NativeError, match=r'job 0: a coefficient that is not finite'):
            analyse([Job(A.astype(np.float32), good.labels)], L, B, True)
    (info,), (counts,) = analyse([good], L, B, False)
    want_counts, want_info = ic.reference_information(good.A, good.labels, L, B)
    assert np.array_equal(counts, want_counts) and np.max(np.abs(info - want_info)) <= ic.information_bar(B)


@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
def test_the_host_form_equals_the_device_form(f32):
    from multimodal_amd import evaluation
    n, k, L, B = R + 9, 66, 7, 10
    A = ic.coefficients(21, n, k, dtype=NP[f32])
    labels = ic.labels_of(21, n, L)
    (info,), (counts,) = analyse([Job(A, labels)], L, B, f32)
    host_info, host_counts = _native.information(A, labels, L, bins=B, return_counts=True)
    assert host_info.shape == (L, k) and host_counts.shape == (k, L, B)
    assert np.array_equal(host_info.view(np.uint64), info.view(np.uint64)) and np.array_equal(host_counts, counts)
    public = evaluation.information_matrix(A, labels.astype(np.int64), bins=B)
    assert np.array_equal(public.view(np.uint64), info.view(np.uint64))                   # n_labels = max + 1 = L here
    assert labels.max() == L - 1
    public, public_counts = evaluation.information_matrix(A.tolist(), list(labels), n_labels=L + 2, bins=B, return_counts=True)
    assert public.shape == (L + 2, k) and (public[L:] == 0).all() and (public_counts[:, L:] == 0).all()
    if not f32:                                                    # (a list of floats runs as float64)
        assert np.array_equal(public[:L].view(np.uint64), info.view(np.uint64))
    for bad in (-1, L):
        wrong = labels.copy()
        wrong[5] = bad
        with pytest.raises(_native.NativeError, match='job 0: a label outside'):
            _native.information(A, wrong, L, bins=B)


def small_dataset():
    from multimodal_amd.device_data import DeviceDataset
    from tests.test_batch_gpu import class_blocks
    data, labels = class_blocks(n_labels=6, per_label=10, dims=(40, 60))                  # 60 samples, two modalities
    return DeviceDataset(data, device=0), labels


def trained(ds, rows, k, seed):
    from multimodal_amd.learner import MultimodalLearner
    learner = MultimodalLearner(['a', 'b'], list(ds.dims), [1.0, 1.0], k)
    H0 = np.random.default_rng(seed).random((k, sum(ds.dims))) + .01
    H0 /= H0.sum(axis=1, keepdims=True)
    ds.train(learner, rows, 10, init_dictionary=H0)
    return learner


def test_device_evaluation_equals_the_host_route_on_the_downloaded_internals(monkeypatch):
    from multimodal_amd import evaluation
    from multimodal_amd.device_data import DeviceEvaluation
    monkeypatch.setenv('KLNMF_PRECISION', 'f64')
    monkeypatch.delenv('KLNMF_DEVICES', raising=False)
    ds, labels = small_dataset()
    order = np.random.default_rng(4).permutation(60)
    runs = []
    for r in range(3):
        train, test = [int(i) for i in order[20:]], [int(i) for i in np.roll(order, 7 * r)[:20]]
        runs.append((DeviceEvaluation(ds, trained(ds, train, 5, r), 10), test, [labels[t] for t in test]))
    singles = []
    for ev, test, lab in runs:
        got = ev.information_matrix(['a', 'b'], test, lab, 6)
        internal = ev.internal(['a', 'b'], test).cpu().numpy()
        want = evaluation.information_matrix(internal, lab, n_labels=6)
        assert got.shape == (6, 5) and got.dtype == np.float64
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
        assert np.max(np.abs(got - ic.reference_information(internal, lab, 6, 10)[1])) <= ic.information_bar(10)
        assert got.max() > 0.01                                    # the atoms do tell the labels apart
        singles.append(got)
    many = DeviceEvaluation.information_matrix_many([ev for ev, _t, _l in runs], ['a', 'b'], [t for _e, t, _l in runs],
                                                    [l for _e, _t, l in runs], 6)
    assert len(many) == 3
    for got, alone in zip(many, singles):
        assert np.array_equal(got.view(np.uint64), alone.view(np.uint64))


def test_perform_one_run_returns_the_matrix_of_the_test_rows(monkeypatch):
    from multimodal_amd.device_data import DeviceEvaluation
    from multimodal_amd.device_experiment import perform_one_run
    monkeypatch.setenv('KLNMF_PRECISION', 'f64')
    monkeypatch.delenv('KLNMF_DEVICES', raising=False)
    ds, labels = small_dataset()
    examples = [labels.index(l) for l in sorted(set(labels))]
    rest = [i for i in range(60) if i not in examples]
    test, train = rest[::3], [i for i in rest if i not in rest[::3]]
    H0 = np.random.default_rng(9).random((5, sum(ds.dims))) + .01
    H0 /= H0.sum(axis=1, keepdims=True)
    args = (ds, ['a', 'b'], [1.0, 1.0], 5, 10, 10, train, test, examples, [labels[t] for t in test], [labels[e] for e in examples])
    _l, default = perform_one_run(*args, init_dictionary=H0)
    learner, asked = perform_one_run(*args, init_dictionary=H0, information=True)
    assert sorted(asked) == sorted(list(default) + ['information', 'information_labels'])
    assert asked['information_labels'] == sorted(set(labels)) and asked['information'].shape == (6, 5)
    for key in default:
        assert np.array_equal(asked[key], default[key]) if key == 'dictionary' else asked[key] == default[key], key
    want = DeviceEvaluation(ds, learner, 10).information_matrix(['a', 'b'], test, [labels[t] for t in test], 6)
    assert np.array_equal(asked['information'].view(np.uint64), want.view(np.uint64))


def test_zz_report_the_worst_difference():
    """Runs last in the file: the largest |info - restatement| the tests above measured, per bin count."""
    assert WORST, 'the comparisons above did not run'
    for B in sorted({b for _w, b in WORST.values()}):
        worst = max(w for w, b in WORST.values() if b == B)
        print('information: worst |info - restatement| at B = %d: %.3e (bar %.1e)' % (B, worst, ic.information_bar(B)))
        assert worst <= ic.information_bar(B)
