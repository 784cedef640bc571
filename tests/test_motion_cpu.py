"""The motion modality without a GPU: the exports of include/klnmf_motion.h; the host twin
(multimodal_amd/features/angle_histograms.py) against the REFERENCE's recorded outputs (tests/golden/g23_motion.npz: its
`record_to_angle_array`, `delayed_velocities` and `get_histos`, scipy's `whiten` and `kmeans`) by equality where the arithmetic
is exact and under the derived bars of tests/motion_cases.py elsewhere; the twin's edge rules; and the routing of the public
functions, with recording stand-ins for the native calls that answer from the host twin on CPU tensors.  Every host refusal
raises before any native call."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

from multimodal_amd import _native
from multimodal_amd.features import angle_histograms as ah
from tests import motion_cases as mc
from tests.test_batch_csr_cpu import check_header_tables, declared_in, other_headers
from tests.test_hac_cpu import host_matrix
from tests.test_kmeans_cpu import write_matrix

NEW = {'klnmf_motion_work_bytes', 'klnmf_motion_angles_device', 'klnmf_motion_whiten_device', 'klnmf_motion_kmeans_device',
       'klnmf_motion_hist_device'}
OTHERS = other_headers('klnmf_motion.h')
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'klnmf_motion.h')


# ---- the bindings -------------------------------------------------------------------------------------------------------------------
def test_every_declared_motion_symbol_is_bound_and_exported():
    declared = declared_in('klnmf_motion.h')
    assert declared == NEW == set(_native.MOTION_SIGNATURES)
    lib = _native.load()
    for name in declared:
        assert hasattr(lib, name), name
    for header in OTHERS:
        assert not (declared & declared_in(header)), header
    for name in NEW:
        assert callable(getattr(_native, name[len('klnmf_'):]))
    defines = dict(re.findall(r'^#define (KLNMF_MOTION_\w+) (\d+)$', open(HEADER).read(), flags=re.M))
    assert {k: int(v) for k, v in defines.items()} == {
        'KLNMF_MOTION_TILE': _native.MOTION_TILE, 'KLNMF_MOTION_GROUP': _native.MOTION_GROUP, 'KLNMF_MOTION_MAX_K': _native.MOTION_MAX_K,
        'KLNMF_MOTION_MAX_D': _native.MOTION_MAX_D, 'KLNMF_MOTION_MAX_KD': _native.MOTION_MAX_KD,
        'KLNMF_MOTION_MAX_PAIRS': _native.MOTION_MAX_PAIRS, 'KLNMF_MOTION_MAX_P': _native.MOTION_MAX_P,
        'KLNMF_MOTION_POLL': _native.MOTION_POLL, 'KLNMF_MOTION_PAD_ZEROS': _native.MOTION_PADDINGS['zeros'],
        'KLNMF_MOTION_PAD_CIRCULAR': _native.MOTION_PADDINGS['circular']}
    assert (mc.TILE, mc.GROUP, ah.GROUP) == (256, 4096, _native.KMEANS_GROUP)
    assert 64 * 2 <= ah.MAX_KD and 64 <= ah.MAX_K and 2 <= ah.MAX_D                   # d = 2, K = 16 ... 64 is comfortable
    # the static LDS of k_mo_assign: accumulators and codebook, a tile of points, distances, labels, counts and mask
    assert ah.MAX_KD * 16 + ah.MAX_D * 257 * 8 + 256 * 12 + ah.MAX_K * 8 <= 64 * 1024


def test_the_other_headers_keep_their_sets():
    check_header_tables()                # (and NEW is this header's own table: the test above)


def test_every_entry_point_names_the_reference_lines_it_replaces():
    header = open(HEADER).read()
    for name in NEW:
        comment = header[:header.index('int %s(' % name)].rsplit('/*', 1)[1]
        assert re.search(r'features/angle_histograms\.py:\d+', comment), name


def test_the_workspace_size_is_host_arithmetic():
    up16 = lambda b: (b + 15) // 16 * 16

    def want(T, C, d, K, P, D, E):
        G = max(1, -(-T // 4096))
        km = up16(G * P * K * d * 8) + up16(G * P * 8) + up16(G * P * K * 4) + up16(P * 8) + 2 * up16(P * 4)
        return max(up16(G * C * 8), km, up16(E * D * K * 8)) + up16((E + 1) * 8) + 256
    for sizes in ((0, 0, 1, 1, 0, 1, 0), (1, 60, 1, 1, 0, 1, 0), (4096, 0, 2, 16, 600, 30, 0), (4097, 0, 2, 16, 600, 30, 0),
                  (150000, 0, 2, 16, 0, 30, 1000), (100, 0, 16, 64, 3, 2, 0), (100, 0, 4, 256, 1, 1, 7), (9000, 7, 1, 1, 65535, 65535, 3)):
        assert _native.motion_work_bytes(*sizes) == want(*sizes), sizes
    for bad in ((-1, 0, 1, 1, 0, 1, 0), (2 ** 31 - 1, 0, 1, 1, 0, 1, 0), (5, -1, 1, 1, 0, 1, 0), (5, 0, 0, 1, 0, 1, 0), (5, 0, 1, 0, 0, 1, 0),
                (5, 0, 1, 1, -1, 1, 0), (5, 0, 1, 1, 0, 0, 0), (5, 0, 1, 1, 0, 1, -1)):
        with pytest.raises(_native.NativeError) as e:
            _native.motion_work_bytes(*bad)
        assert e.value.code == _native.ERR_ARG, bad
    for beyond in ((5, 0, 17, 1, 0, 1, 0), (5, 0, 1, 257, 0, 1, 0), (5, 0, 8, 129, 0, 1, 0), (5, 0, 1, 1, 65536, 1, 0), (5, 0, 1, 1, 0, 65536, 0)):
        with pytest.raises(_native.NativeError) as e:
            _native.motion_work_bytes(*beyond)
        assert e.value.code == _native.ERR_UNSUPP, beyond
    assert _native.load().klnmf_motion_work_bytes(5, 0, 1, 1, 0, 1, 0, None) == _native.ERR_ARG


# ---- the host twin against the reference's recorded outputs ---------------------------------------------------------------------------
def w_points(g):
    return np.stack([g['w_angles'], g['w_vels_1_zeros']], axis=2).reshape(g['w_angles'].shape[0], -1)


def test_the_twin_gives_the_recorded_angles_and_velocities():
    g = mc.golden()
    names = list(g['names'])
    assert names == mc.NAMES and ah.angles_indices(names) == [(names.index(s), names.index(d)) for s, d in ah.ANGLES]
    angles, vels, offsets = ah.host_angle_arrays((g['w_records'], g['w_offsets']), names)
    assert mc.same_bits(offsets, g['w_offsets']) and angles.shape == g['w_angles'].shape == (offsets[-1], 30)
    err = np.abs(angles - g['w_angles'])
    bar = mc.angle_bar_reference(g['w_angles'])
    print('angles, twin against the reference: worst %.3g, worst share of its bar %.3g' % (err.max(), (err / bar).max()))
    assert (err <= bar).all()
    # the same from a list of examples
    parts = [g['w_records'][a:b] for a, b in zip(offsets[:-1], offsets[1:])]
    again = ah.host_angle_arrays(parts, names)
    assert mc.same_bits(again[0], angles) and mc.same_bits(again[1], vels) and mc.same_bits(again[2], offsets)
    # the subtraction is exact given equal angles: from the RECORDED angles every recorded velocity, bit for bit
    for delay in (1, 10):
        for padding in ('zeros', 'circular'):
            v = np.vstack([ah.host_delayed_velocities(delay, g['w_angles'][a:b], padding) for a, b in zip(offsets[:-1], offsets[1:])])
            want = g['w_vels_%d_%s' % (delay, padding)]
            assert mc.same_bits(v if want.shape[1] == 30 else np.ascontiguousarray(v[:, ::6]), want)
    # the clip is filter_values'
    lo, hi = -0.5, 0.25
    a2, v2, _ = ah.host_angle_arrays(parts, names, bounds=(lo, hi), vel_bounds=(-0.01, 0.02))
    assert mc.same_bits(a2, np.maximum(np.minimum(angles, hi), lo)) and mc.same_bits(v2, np.maximum(np.minimum(vels, 0.02), -0.01))


def test_the_twin_gives_the_recorded_whitened_points():
    g = mc.golden()
    white, mean, std = ah.host_whiten(w_points(g))
    sets = white.reshape(white.shape[0], -1, 2).transpose(1, 0, 2)
    rel = np.abs(sets - g['w_white']) / np.abs(g['w_white'])
    bar = (4096 + 1 + 4) * 2.0 ** -53
    print('whitened points, twin against scipy: worst relative %.3g (bar %.3g)' % (np.nanmax(rel), bar))
    assert np.nanmax(rel) <= bar and np.array_equal(sets == 0, g['w_white'] == 0)
    x = w_points(g)
    assert np.abs(mean - x.mean(axis=0)).max() <= bar * np.abs(x).sum(axis=0).max() / x.shape[0]
    assert (np.abs(std - x.std(axis=0)) <= bar * x.std(axis=0)).all()


@pytest.mark.parametrize('tag', ['w', 'g'])
def test_the_twin_gives_the_recorded_codebooks(tag):
    g = mc.golden()
    sets = g['w_white'] if tag == 'w' else g['g_points']
    T = sets.shape[1]
    thresh = float(g['thresh'])
    exact = tag == 'g'
    if exact:
        assert np.array_equal(sets * 1024, np.round(sets * 1024))                     # multiples of 2^-10: every cluster sum is exact
    # a mean of up to T members summed in another order; the distortion is a mean of T distances
    bar = 0.0 if exact else (T + 4) * 2.0 ** -53
    dist_bar = (T + 4) * 2.0 ** -53
    worst = 0.0
    for s in range(sets.shape[0]):
        cb, alive, dist, iters, labels = ah.host_kmeans_converged_from(sets[s], g[tag + '_init'][s], thresh)
        assert alive.all() and iters == g[tag + '_init_iters'][s] and labels.dtype == np.int32
        want = g[tag + '_init_cb'][s]
        if exact:
            assert mc.same_bits(cb, want)
        worst = max(worst, (np.abs(cb - want) / np.abs(want)).max())
        assert abs(dist - g[tag + '_init_dist'][s]) <= dist_bar * dist
        # scipy's kmeans(points, k, iter=3) under np.random.seed(s): the twin under RandomState(s)
        got, d3 = ah.host_kmeans_converged(sets[s], want.shape[0], iter=int(g['restarts']), thresh=thresh,
                                           rng=np.random.RandomState(int(g[tag + '_seed'][s])))
        want3 = g[tag + '_seed_cb'][s]
        if exact:
            assert mc.same_bits(got, want3)
        worst = max(worst, (np.abs(got - want3) / np.abs(want3)).max())
        assert abs(d3 - g[tag + '_seed_dist'][s]) <= dist_bar * d3
    print('codebooks of set %s, twin against scipy: worst relative %.3g (bar %.3g)' % (tag, worst, bar))
    assert worst <= bar
    # the init made to lose a cluster: scipy's code_book[has_members] is the live rows in order
    s = 0 if tag == 'w' else 1
    cb, alive, dist, _, _ = ah.host_kmeans_converged_from(sets[s], g[tag + '_far_init'], thresh)
    want = g[tag + '_far_cb']
    assert alive.sum() == want.shape[0] == cb.shape[0] - 1 and not alive[1 if tag == 'w' else 5]
    assert mc.same_bits(cb[~alive], g[tag + '_far_init'][~alive])                     # a dropped row keeps its values
    assert (np.abs(cb[alive] - want) <= bar * np.abs(want)).all() and abs(dist - g[tag + '_far_dist']) <= dist_bar * dist
    got, d1 = ah.host_kmeans_converged(sets[s], g[tag + '_far_init'], thresh=thresh)
    assert mc.same_bits(got, cb[alive]) and d1 == dist


def test_the_twin_gives_the_recorded_matrices():
    g = mc.golden()
    frames = np.diff(g['w_offsets'])
    hard = ah.host_histograms(g['w_white'], g['w_seed_cb'], g['w_offsets'])
    assert mc.same_bits(hard, g['w_hard'])                                            # integer counts, exact sums, one division
    soft = ah.host_histograms(g['w_white'], g['w_seed_cb'], g['w_offsets'], .5)
    rel = np.abs(soft - g['w_soft']) / g['w_soft']
    bar = mc.soft_bar(frames, 4)[:, np.newaxis]
    print('soft matrix, twin against the reference: worst relative %.3g, worst share of its bar %.3g' % (rel.max(), (rel / bar).max()))
    assert (rel <= bar).all() and soft.shape == (6, 120)
    assert np.abs(soft.sum(axis=1) - 1).max() < 1e-14 and np.abs(hard.sum(axis=1) - 1).max() < 1e-14
    # the grid set: offsets with a one-frame example and examples across a tile boundary
    frames = np.diff(g['g_offsets'])
    assert mc.same_bits(ah.host_histograms(g['g_points'], g['g_seed_cb'], g['g_offsets']), g['g_hard'])
    soft = ah.host_histograms(g['g_points'], g['g_seed_cb'], g['g_offsets'], .5)
    assert (np.abs(soft - g['g_soft']) <= mc.soft_bar(frames, 8)[:, np.newaxis] * g['g_soft']).all()
    # the whole chain from the records on: the layout is [example][dof][bin]
    X, cbs = ah.host_vq_hist_matrix((g['w_records'], g['w_offsets']), list(g['names']), nb_bins=4, iter=3, rng=5, return_codebooks=True)
    assert X.shape == (6, 120) and cbs.shape == (30, 4, 2)
    angles, vels, offsets = ah.host_angle_arrays((g['w_records'], g['w_offsets']), list(g['names']))
    white = ah.host_whiten(np.stack([angles[:, 7], vels[:, 7]], axis=1))[0]
    one = ah.host_histograms(white[np.newaxis], cbs[7:8], offsets)
    n = np.diff(offsets).astype(np.float64)[:, np.newaxis]
    counts = np.round(one * n)
    assert np.array_equal(counts.sum(axis=1, keepdims=True), n) and mc.same_bits(X[:, 28:32], counts / (30.0 * n))


# ---- the twin's edge rules ----------------------------------------------------------------------------------------------------------
def test_velocities_stay_inside_an_example():
    a = np.arange(1.0, 13.0).reshape(6, 2) ** 2
    for delay in (6, 7, 100):                                                         # delay >= the example's length
        assert mc.same_bits(ah.host_delayed_velocities(delay, a, 'zeros'), a)
        assert mc.same_bits(ah.host_delayed_velocities(delay, a, 'circular'), np.zeros_like(a))
    assert mc.same_bits(ah.host_delayed_velocities(2, a, 'zeros'), np.vstack([a[:2], a[2:] - a[:-2]]))
    assert mc.same_bits(ah.host_delayed_velocities(2, a, 'circular'), a - np.vstack([a[-2:], a[:-2]]))
    one = a[:1]                                                                       # a one-frame example
    assert mc.same_bits(ah.host_delayed_velocities(1, one, 'zeros'), one)
    assert mc.same_bits(ah.host_delayed_velocities(3, one, 'circular'), np.zeros_like(one))
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError):
            ah.host_delayed_velocities(bad, a)
    with pytest.raises(ValueError):
        ah.host_delayed_velocities(1, a, 'mirror')
    # E = 1 and one-frame examples through host_angle_arrays: nothing reaches across an offset
    rec = np.array(mc.records(3, 9))
    pairs = [(1, 2), (3, 0)]
    whole = ah.host_angle_arrays([rec], pairs, vel_delay=2)
    cut = ah.host_angle_arrays([rec[:1], rec[1:5], rec[5:]], pairs, vel_delay=2)
    assert list(whole[2]) == [0, 9] and list(cut[2]) == [0, 1, 5, 9] and mc.same_bits(whole[0], cut[0])
    assert mc.same_bits(cut[1][[0, 1, 2, 5, 6]], cut[0][[0, 1, 2, 5, 6]]) and mc.same_bits(cut[1][3], cut[0][3] - cut[0][1])
    assert mc.same_bits(whole[1][5], whole[0][5] - whole[0][3])


def test_both_euler_branches_and_the_identity_branch():
    def angles_of(q_src, q_dst):
        rec = np.zeros((1, 2, 7))
        rec[0, 0, 3:], rec[0, 1, 3:] = q_src, q_dst
        return ah.host_angle_array(rec, [(0, 1)])[0]
    unit = [0.0, 0.0, 0.0, 1.0]
    # (values are compared, not the signs of zeros)
    assert np.array_equal(angles_of(unit, unit), np.zeros(3))
    # a quarter turn about x, exactly representable: quaternion_matrix scales q = (1, 0, 0, 1) itself; the regular branch
    assert np.array_equal(angles_of(unit, [1.0, 0.0, 0.0, 1.0]), [np.pi / 2, 0.0, 0.0])
    assert np.array_equal(angles_of([0.0, 0.0, 2.0, 2.0], [0.0, 0.0, 0.0, 4.0]), [0.0, 0.0, -np.pi / 2])
    # the gimbal case: a quarter turn about y gives m00 = m10 = 0, cy = 0 <= _EPS: az = 0, ax = atan2(-m12, m11) = atan2(0, 1)
    assert np.array_equal(angles_of(unit, [0.0, 1.0, 0.0, 1.0]), [0.0, np.pi / 2, 0.0])
    # and with a turn about x before it (q = qy * qx = (1, 1, -1, 1) / 2): m12 = -1, m11 = 0, so ax = atan2(1, 0); the scale
    # sqrt(2 / 4) is not exact here, cy is a few 1e-16 -- still below _EPS -- and az = 0 exactly shows the branch
    got = angles_of(unit, [1.0, 1.0, -1.0, 1.0])
    assert got[2] == 0.0 and np.abs(got[:2] - np.pi / 2).max() < 1e-15
    # nq < _EPS: the identity matrix, all angles 0 -- the dest quaternion is tiny, not zero
    assert np.array_equal(angles_of(unit, [2.0 ** -30, 0.0, 0.0, 2.0 ** -30]), np.zeros(3))
    assert angles_of(unit, [2.0 ** -20, 0.0, 0.0, 2.0 ** -20])[0] == np.pi / 2        # just above: a rotation again
    # float32 records give float32 angles, formed in float64
    rec = mc.records(4, 5, True)
    a32 = ah.host_angle_array(rec, [(1, 2)])
    assert a32.dtype == np.float32 and mc.same_bits(a32, ah.host_angle_array(rec.astype(np.float64), [(1, 2)]).astype(np.float32))


def test_whitening_follows_the_order_rule_and_scipys_zero_rule():
    rng = np.random.default_rng(2)
    x = rng.normal(size=(2 * mc.GROUP + 9, 3)) * [1.0, 1e3, 1e-3] + [0.0, 5.0, -2.0]
    white, mean, std = ah.host_whiten(x)
    T = x.shape[0]
    for c in range(3):
        total = 0.0
        for g0 in range(0, T, mc.GROUP):
            part = 0.0
            for v in x[g0:g0 + mc.GROUP, c]:
                part = part + v
            total = total + part
        assert mean[c] == total / T
        total = 0.0
        for g0 in range(0, T, mc.GROUP):
            part = 0.0
            for v in x[g0:g0 + mc.GROUP, c]:
                part = part + (v - mean[c]) * (v - mean[c])
            total = total + part
        assert std[c] == np.sqrt(total / T)
    assert mc.same_bits(white, x / std)
    flat = np.hstack([x[:50, :1], np.full((50, 1), 0.75)])
    with pytest.warns(RuntimeWarning):
        white, mean, std = ah.host_whiten(flat)
    assert std[1] == 1.0 and mc.same_bits(white[:, 1], flat[:, 1]) and mean[1] == 0.75
    w32 = ah.host_whiten(x[:100].astype(np.float32))
    assert w32[0].dtype == np.float32 and w32[1].dtype == np.float64
    assert mc.same_bits(w32[0], (x[:100].astype(np.float32).astype(np.float64) / w32[2]).astype(np.float32))


def test_kmeans_edges_one_cluster_ties_and_restart_ties():
    pts, _ = mc.clouds(1, 1, 300, 2, 4)
    x = pts[0]
    # K = 1: the mean after one update, measured at the second iteration, the stop at the third with diff = 0
    cb, alive, dist, iters, labels = ah.host_kmeans_converged_from(x, x[:1], 1e-5)
    assert iters == 3 and alive.all() and not labels.any() and mc.same_bits(cb[0], ah._order_sum(x) / 300.0)
    # equal distances: the lowest live index
    cb, alive, _, _, labels = ah.host_kmeans_converged_from(np.array([[0.5], [0.0], [1.0], [0.5]]), [[0.0], [1.0]], 10.0)
    assert list(labels) == [0, 0, 1, 0] and mc.same_bits(cb, np.array([[1.0 / 3.0], [1.0]]))
    # duplicate rows: the duplicate never has members and is dropped at once
    cb, alive, _, _, _ = ah.host_kmeans_converged_from(x, np.vstack([x[0], x[0], x[1]]), 1e-5)
    assert list(alive) == [True, False, True] and mc.same_bits(cb[1], x[0])
    # a restart tie: with k = T every restart is a permutation of the points, every distortion 0; the FIRST is kept
    small = x[:6]
    got, dist = ah.host_kmeans_converged(small, 6, iter=4, rng=np.random.RandomState(3))
    first = np.random.RandomState(3).choice(6, size=6, replace=False)
    assert dist == 0.0 and mc.same_bits(got, small[first])
    # a Generator and a seed for one draw the same rows
    a = ah.host_kmeans_converged(x, 3, iter=2, rng=7)
    b = ah.host_kmeans_converged(x, 3, iter=2, rng=np.random.default_rng(7))
    assert mc.same_bits(a[0], b[0]) and a[1] == b[1]
    rows = ah.draw_rows(np.random.RandomState(5), 300, 3, 2, 2)
    replay = np.random.RandomState(5)
    assert rows.shape == (2, 2, 3) and all((rows[s, r] == replay.choice(300, size=3, replace=False)).all() for s in range(2) for r in range(2))
    with pytest.raises(RuntimeError, match='max_iter'):
        ah.host_kmeans_converged_from(x, x[:4], 0.0, max_iter=2)


def test_a_lost_cluster_in_the_best_codebook_is_a_value_error():
    pts, init = mc.clouds(2, 1, 200, 2, 3)
    best = [(ah.host_kmeans_converged(pts[0], mc.far_init(init[0]))[0], 0.0)]
    assert best[0][0].shape == (2, 2)
    with pytest.raises(ValueError, match='lost 1 of its 3'):
        ah._full_codebooks(best, 3)


# ---- the routing of the public functions ------------------------------------------------------------------------------------------
def ints_at(ptr, n, ctype=ctypes.c_int32):
    return np.ctypeslib.as_array((ctype * n).from_address(ptr))


class MotionRecorder(object):
    """Stand-ins for the device calls: they answer from the host twin on CPU tensors and record what they were asked."""

    def __init__(self, monkeypatch):
        self.calls = []
        for name in ('angles', 'whiten', 'kmeans', 'hist'):
            monkeypatch.setattr(_native, 'motion_%s_device' % name, getattr(self, name))

    def points(self, ptr, set_stride, ld, T, d, D, dt):
        item = np.dtype(dt).itemsize
        return np.stack([host_matrix(ptr + s * set_stride * item, T, ld, d, dt) for s in range(D)])

    def angles(self, d_records, T, n_markers, pairs, offsets, delay, padding, bounds, vel_bounds, d_work, work_bytes, d_angles, lda,
               d_vels, ldv, f64=True, device=0):
        dt = np.float64 if f64 else np.float32
        assert d_work and work_bytes >= _native.motion_work_bytes(T, E=len(offsets) - 1)
        rec = host_matrix(d_records, T, n_markers * 7, n_markers * 7, dt).reshape(T, n_markers, 7)
        name = {v: k for k, v in _native.MOTION_PADDINGS.items()}[padding]
        a, v, _ = ah.host_angle_arrays((rec, np.asarray(offsets)), pairs, delay, name, bounds, vel_bounds)
        write_matrix(d_angles, a, lda)
        write_matrix(d_vels, v, ldv)
        self.calls.append(dict(call='angles', T=T, markers=n_markers, pairs=list(pairs), offsets=list(offsets), delay=delay,
                               padding=name, bounds=bounds, vel_bounds=vel_bounds, f64=f64, records=d_records, out=(d_angles, d_vels)))

    def whiten(self, d_x, ld, T, C, d_work, work_bytes, d_out, ldo, d_mean, d_std, f64=True, device=0):
        assert d_work and work_bytes >= _native.motion_work_bytes(T, C=C)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            out, mean, std = ah.host_whiten(host_matrix(d_x, T, ld, C, np.float64 if f64 else np.float32))
        write_matrix(d_out, out, ldo)
        ints_at(d_mean, C, ctypes.c_double)[:] = mean
        ints_at(d_std, C, ctypes.c_double)[:] = std
        self.calls.append(dict(call='whiten', T=T, C=C, x=d_x, out=d_out, f64=f64))

    def kmeans(self, d_points, set_stride, ld, T, d, D, set_of, d_codebooks, K, thresh, max_iter, d_work, work_bytes, d_alive,
               d_distortion, d_iters, d_labels=0, f64=True, device=0):
        dt = np.float64 if f64 else np.float32
        P = len(set_of)
        assert d_work and work_bytes >= _native.motion_work_bytes(T, d=d, K=K, P=P, D=D)
        sets = self.points(d_points, set_stride, ld, T, d, D, dt)
        cbs = host_matrix(d_codebooks, P * K, d, d, dt).reshape(P, K, d)
        iters = []
        for p in range(P):
            try:
                cb, alive, dist, it, labels = ah.host_kmeans_converged_from(sets[set_of[p]], cbs[p], thresh, max_iter)
            except RuntimeError:
                return p
            write_matrix(d_codebooks + p * K * d * cb.itemsize, cb, d)
            ints_at(d_alive + 4 * p * K, K)[:] = alive
            ints_at(d_distortion + 8 * p, 1, ctypes.c_double)[:] = dist
            ints_at(d_iters + 4 * p, 1)[:] = it
            if d_labels:
                ints_at(d_labels + 4 * p * T, T)[:] = labels
            iters.append(it)
        self.calls.append(dict(call='kmeans', T=T, d=d, D=D, K=K, P=P, set_of=list(set_of), set_stride=set_stride, ld=ld, thresh=thresh,
                               max_iter=max_iter, f64=f64, points=d_points, init=cbs, iters=iters))
        return -1

    def hist(self, d_points, set_stride, ld, T, d, D, d_codebooks, K, offsets, soft, alpha, d_work, work_bytes, d_out, ldo, f64=True,
             device=0):
        dt = np.float64 if f64 else np.float32
        assert d_work and work_bytes >= _native.motion_work_bytes(T, d=d, K=K, D=D, E=len(offsets) - 1)
        sets = self.points(d_points, set_stride, ld, T, d, D, dt)
        cbs = host_matrix(d_codebooks, D * K, d, d, dt).reshape(D, K, d)
        write_matrix(d_out, ah.host_histograms(sets, cbs, offsets, alpha if soft else None), ldo)
        self.calls.append(dict(call='hist', T=T, d=d, D=D, K=K, offsets=list(offsets), soft=soft, alpha=alpha, set_stride=set_stride,
                               ld=ld, f64=f64, points=d_points))


@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
def test_vq_hist_matrix_is_one_call_per_stage(monkeypatch, f32):
    import torch
    rec = MotionRecorder(monkeypatch)
    parts = [np.array(mc.records(s, n, f32)) for s, n in ((1, 40), (2, 1), (3, 25))]
    kw = dict(vel_delay=3, vel_padding='circular', nb_bins=4, iter=3, rng=9, bounds=(-2.0, 2.0), vel_bounds=(-0.5, 0.5))
    want, want_cbs = ah.host_vq_hist_matrix(parts, mc.NAMES, return_codebooks=True, **kw)
    X, cbs = ah.vq_hist_matrix(parts, mc.NAMES, device='cpu', return_codebooks=True, **kw)
    assert mc.same_bits(X, want) and mc.same_bits(cbs, want_cbs) and X.dtype == (np.float32 if f32 else np.float64)
    assert [c['call'] for c in rec.calls] == ['angles', 'whiten', 'kmeans', 'hist']
    a, w, k, h = rec.calls
    assert (a['T'], a['markers'], a['offsets'], a['delay'], a['padding'], a['f64']) == (66, 14, [0, 40, 41, 66], 3, 'circular', not f32)
    assert a['pairs'] == [tuple(p) for p in ah.angles_indices(mc.NAMES)] or [list(p) for p in a['pairs']] == [list(p) for p in ah.angles_indices(mc.NAMES)]
    assert a['bounds'] == (-2.0, 2.0) and a['vel_bounds'] == (-0.5, 0.5)
    assert (w['T'], w['C']) == (66, 60) and w['x'] == w['out']                         # whitened in place
    assert (k['T'], k['d'], k['D'], k['K'], k['P'], k['set_stride'], k['ld']) == (66, 2, 30, 4, 90, 2, 60)
    assert k['set_of'] == [s for s in range(30) for _ in range(3)] and k['points'] == w['out'] == h['points']
    assert (k['thresh'], k['max_iter']) == (1e-5, 1000)
    assert (h['D'], h['K'], h['offsets'], h['soft'], h['set_stride'], h['ld']) == (30, 4, [0, 40, 41, 66], 0, 2, 60)
    # the drawn rows: scipy's draws, set after set, restart after restart
    rows = ah.draw_rows(np.random.default_rng(9), 66, 4, 3, 30)
    angles, vels, _ = ah.host_angle_arrays(parts, mc.NAMES, 3, 'circular', (-2.0, 2.0), (-0.5, 0.5))
    pts = ah.host_whiten(ah._interleave(angles, vels))[0].reshape(66, 30, 2)
    assert mc.same_bits(k['init'], np.stack([pts[rows[s, r], s] for s in range(30) for r in range(3)]))
    # soft, device tensors in, a device tensor out
    rec.calls[:] = []
    t_parts = [torch.from_numpy(p) for p in parts]
    Xs = ah.vq_hist_matrix(t_parts, mc.NAMES, soft_vq=.5, device='cpu', output='device', **kw)
    assert torch.is_tensor(Xs) and mc.same_bits(Xs.numpy(), ah.host_vq_hist_matrix(parts, mc.NAMES, soft_vq=.5, **kw))
    assert (rec.calls[3]['soft'], rec.calls[3]['alpha']) == (1, .5)
    # a stacked tensor with offsets is used in place
    stacked = torch.from_numpy(np.concatenate(parts))
    rec.calls[:] = []
    ah.vq_hist_matrix((stacked, np.array([0, 40, 41, 66])), mc.NAMES, device='cpu', **kw)
    assert rec.calls[0]['records'] == stacked.data_ptr()
    # from angles on: three calls
    rec.calls[:] = []
    angles, vels, offsets = ah.host_angle_arrays(parts, mc.NAMES)
    got = ah.vq_hist_matrix_from_angles(angles, vels, offsets, nb_bins=4, iter=3, rng=9, device='cpu')
    assert [c['call'] for c in rec.calls] == ['whiten', 'kmeans', 'hist']
    assert mc.same_bits(got, ah.host_vq_hist_matrix_from_angles(angles, vels, offsets, nb_bins=4, iter=3, rng=9))


def test_the_stage_functions_route_to_their_calls(monkeypatch):
    rec = MotionRecorder(monkeypatch)
    parts = [np.array(mc.records(5, 12)), np.array(mc.records(6, 7))]
    pairs = [(0, 1), (2, 3), (1, 1)]
    got = ah.angle_arrays(parts, pairs, vel_delay=10, device='cpu')
    want = ah.host_angle_arrays(parts, pairs, vel_delay=10)
    assert all(mc.same_bits(a, b) for a, b in zip(got, want)) and rec.calls[0]['delay'] == 10 and rec.calls[0]['bounds'] is None
    x = np.hstack([got[0][:, :2], np.full((19, 1), 2.5)])
    with pytest.warns(RuntimeWarning):
        w = ah.whiten(x, device='cpu')
    with pytest.warns(RuntimeWarning):
        hw = ah.host_whiten(x)
    assert all(mc.same_bits(a, b) for a, b in zip(w, hw))
    pts, init = mc.clouds(3, 2, 120, 3, 5)
    rec.calls[:] = []
    got = ah.kmeans_converged_many(pts, 5, iter=2, rng=4, device='cpu')
    want = ah.host_kmeans_converged_many(pts, 5, iter=2, rng=4)
    assert all(mc.same_bits(a[0], b[0]) and a[1] == b[1] for a, b in zip(got, want))
    k = rec.calls[0]
    assert (k['P'], k['D'], k['d'], k['K'], k['set_stride'], k['ld'], k['set_of']) == (4, 2, 3, 5, 360, 3, [0, 0, 1, 1])
    cb, dist = ah.kmeans_converged(pts[0], init[0], device='cpu')
    want = ah.host_kmeans_converged(pts[0], init[0])
    assert mc.same_bits(cb, want[0]) and dist == want[1] and rec.calls[1]['P'] == 1
    cb, dist = ah.kmeans_converged(pts[1], 5, iter=3, rng=np.random.RandomState(2), device='cpu')
    want = ah.host_kmeans_converged(pts[1], 5, iter=3, rng=np.random.RandomState(2))
    assert mc.same_bits(cb, want[0]) and dist == want[1] and rec.calls[2]['P'] == 3
    # a dropped cluster: the compacted codebook
    cb, _ = ah.kmeans_converged(pts[0], mc.far_init(init[0]), device='cpu')
    assert cb.shape == (4, 3) and mc.same_bits(cb, ah.host_kmeans_converged(pts[0], mc.far_init(init[0]))[0])
    off = [0, 1, 50, 120]
    cbs = np.stack([w[0] for w in ah.host_kmeans_converged_many(pts, 5, iter=1, rng=1)])
    for soft in (None, .5):
        assert mc.same_bits(ah.histograms(pts, cbs, off, soft, device='cpu'), ah.host_histograms(pts, cbs, off, soft))
    # the guard scipy does not have names the problem
    with pytest.raises(RuntimeError, match=r'problem 0 \(point set 0\).*max_iter = 1'):
        ah.kmeans_converged_many(pts, 5, iter=2, rng=4, max_iter=1, device='cpu')


def test_a_lost_cluster_is_refused_before_the_histogram_launch(monkeypatch):
    rec = MotionRecorder(monkeypatch)
    # two well separated blobs and three bins drawn from one of them ... a far row is simpler: patch the draw
    pts, init = mc.clouds(2, 1, 200, 2, 3)
    angles, vels = pts[0][:, :1].copy(), pts[0][:, 1:].copy()
    far = {'on': True}
    real = ah.draw_rows
    monkeypatch.setattr(ah, 'draw_rows', lambda rng, T, k, restarts, sets=1: np.zeros((sets, restarts, k), dtype=np.int64) if far['on']
                        else real(rng, T, k, restarts, sets))
    with pytest.raises(ValueError, match='lost 2 of its 3'):                           # three equal rows: two never have members
        ah.vq_hist_matrix_from_angles(angles, vels, [0, 200], nb_bins=3, iter=2, device='cpu')
    assert [c['call'] for c in rec.calls] == ['whiten', 'kmeans']


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_every_host_refusal_raises_before_any_native_call(monkeypatch):
    import torch
    rec = MotionRecorder(monkeypatch)
    calls = []
    monkeypatch.setattr(_native, 'motion_work_bytes', lambda *a, **k: calls.append((a, k)) or 1 << 20)
    parts = [np.array(mc.records(1, 30)), np.array(mc.records(2, 12))]
    pts, init = mc.clouds(3, 2, 60, 2, 4)

    def refused(fn, *args, **kwargs):
        with pytest.raises(ValueError):
            fn(*args, device='cpu', **kwargs)

    for fn in (ah.angle_arrays, ah.vq_hist_matrix):
        for delay in (0, -1, 1.5):
            refused(fn, parts, mc.NAMES, vel_delay=delay)                             # the reference's slice breaks below 1
        refused(fn, parts, mc.NAMES, vel_padding='mirror')
        refused(fn, parts, mc.NAMES, bounds=(1.0, -1.0))
        refused(fn, parts, mc.NAMES, vel_bounds=(np.nan, 1.0))
        refused(fn, [], mc.NAMES)
        refused(fn, parts, [])
        refused(fn, parts, mc.NAMES[:-1])                                             # a name ANGLES needs is missing
        refused(fn, parts, [(0, 14)])                                                 # a marker index out of range
        refused(fn, parts, [(0, 1)] * 33)                                             # more pairs than a call takes
        refused(fn, [parts[0], parts[1][:, :5]], mc.NAMES)
        refused(fn, [parts[0][:, :, :6]], mc.NAMES)
        refused(fn, (np.concatenate(parts), np.array([0, 30, 41])), mc.NAMES)         # offsets that do not end at T
        refused(fn, (np.concatenate(parts), np.array([0, 31, 30, 42])), mc.NAMES)     # offsets that decrease
        refused(fn, (np.concatenate(parts), np.array([1, 30, 42])), mc.NAMES)
        bad = parts[0].copy()
        bad[3, 2, 4] = np.nan
        refused(fn, [bad], mc.NAMES)
        refused(fn, [torch.from_numpy(parts[0]).to(torch.float16)], mc.NAMES)
        refused(fn, parts, mc.NAMES, output='scipy')
    refused(ah.vq_hist_matrix, parts, mc.NAMES, nb_bins=0)
    refused(ah.vq_hist_matrix, parts, mc.NAMES, nb_bins=257)
    refused(ah.vq_hist_matrix, parts, mc.NAMES, nb_bins=43)                           # more rows than frames to draw from
    refused(ah.vq_hist_matrix, parts, mc.NAMES, iter=0)
    refused(ah.vq_hist_matrix, parts, mc.NAMES, iter=65535 // 30 + 1)                 # more problems than a call takes
    refused(ah.vq_hist_matrix, parts, mc.NAMES, thresh=-1.0)
    refused(ah.vq_hist_matrix, parts, mc.NAMES, thresh=np.nan)
    refused(ah.vq_hist_matrix, parts, mc.NAMES, max_iter=0)
    refused(ah.vq_hist_matrix, parts, mc.NAMES, soft_vq=np.inf)
    a, v = pts[0], pts[1]
    refused(ah.vq_hist_matrix_from_angles, a, v[:-1], [0, 60])
    refused(ah.vq_hist_matrix_from_angles, a, v, [0, 61])
    refused(ah.vq_hist_matrix_from_angles, a.ravel(), v.ravel(), [0, 120])
    refused(ah.vq_hist_matrix_from_angles, torch.from_numpy(a.copy()), v, [0, 60])    # one tensor, one array
    refused(ah.vq_hist_matrix_from_angles, a, v, [0.0, 60.0])
    refused(ah.kmeans_converged_many, pts, 0)
    refused(ah.kmeans_converged_many, pts, 2.5)
    refused(ah.kmeans_converged_many, pts, 61)
    refused(ah.kmeans_converged_many, pts[0], 3)
    refused(ah.kmeans_converged_many, pts, 3, iter=0)
    refused(ah.kmeans_converged_many, np.zeros((1, 300, 17)), 3)                      # d beyond the limit
    refused(ah.kmeans_converged_many, np.zeros((1, 300, 8)), 129)                     # K * d beyond the limit
    refused(ah.kmeans_converged, pts[0], init[0][:, :1])
    refused(ah.kmeans_converged, pts[0], np.full((2, 2), np.inf))
    refused(ah.kmeans_converged, pts[0], 3, output='dense')
    refused(ah.histograms, pts, init[:1], [0, 60])
    refused(ah.histograms, pts, init, [0, 59])
    refused(ah.histograms, pts, init, [0, 60], soft_vq=np.nan)
    refused(ah.whiten, np.zeros(5))
    assert rec.calls == [] and calls == []
