"""The motion modality on the device (include/klnmf_motion.h, csrc/motion.hip.h) against the host twin
(multimodal_amd/features/angle_histograms.py, pinned to the reference's recorded outputs by tests/test_motion_cpu.py).

Where stages chain, the twin runs on the device's own earlier outputs.  Bit for bit, in float64 and float32: velocities and
clips, moments and whitened points, labels, live-row masks, iteration counts, codebooks, distortions (the fp64 sqrt and division
of the device are correctly rounded, which the whitening test shows on its own: one sqrt, one division) and the hard matrix.
Under the derived bars of tests/motion_cases.py: the angles (atan2) and the soft matrix (exp); the worst values are printed.
The shapes are the smallest at which each mechanism can go wrong: T around a tile (256) and a group (4096, the unit of the
summation order), examples across both boundaries, of one frame and longer than a group, padded strides with sentinels, K and d
at the header's limits."""
import numpy as np
import pytest

from multimodal_amd import _native
from multimodal_amd.features import angle_histograms as ah
from tests import motion_cases as mc

pytestmark = pytest.mark.gpu

F32 = pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
SIZES = pytest.mark.parametrize('T', [255, 256, 257, 4095, 4096, 4097])
PAIRS = [(1, 2), (3, 0), (4, 4), (0, 13)]


def tdt(f32):
    import torch
    return torch.float32 if f32 else torch.float64


def on_device(a):
    import torch
    return torch.from_numpy(np.array(a, order='C')).to('cuda')


def padded(a, pad, fill=99.0):
    """A device matrix with `pad` sentinel columns behind a's."""
    import torch
    a = np.asarray(a)
    out = torch.full((a.shape[0], a.shape[1] + pad), fill, dtype=tdt(a.dtype == np.float32), device='cuda')
    out[:, :a.shape[1]] = on_device(a)
    return out


def workspace(**sizes):
    import torch
    need = _native.motion_work_bytes(**sizes)
    return torch.empty(max(16, need), dtype=torch.uint8, device='cuda'), need


def device_angles(rec, offsets, pairs, delay=1, padding='zeros', bounds=None, vel_bounds=None, pad=3):
    import torch
    rec = np.asarray(rec)
    f32 = rec.dtype == np.float32
    T, M, cols = rec.shape[0], rec.shape[1], 3 * len(pairs)
    d_rec = on_device(rec)
    angles, vels = padded(np.zeros((T, cols), rec.dtype), pad, 55.0), padded(np.zeros((T, cols), rec.dtype), pad, 66.0)
    work, need = workspace(T=T, E=len(offsets) - 1)
    _native.motion_angles_device(d_rec.data_ptr(), T, M, pairs, offsets, delay, _native.MOTION_PADDINGS[padding], bounds, vel_bounds,
                                 work.data_ptr(), need, angles.data_ptr(), cols + pad, vels.data_ptr(), cols + pad, f64=not f32)
    torch.cuda.synchronize()
    assert (angles[:, cols:] == 55.0).all() and (vels[:, cols:] == 66.0).all()
    return angles[:, :cols].cpu().numpy().copy(), vels[:, :cols].cpu().numpy().copy()


def twin_velocities(angles, offsets, delay, padding, vel_bounds=None):
    v = np.vstack([ah.host_delayed_velocities(delay, angles[a:b], padding) for a, b in zip(offsets[:-1], offsets[1:]) if b > a])
    return ah._clip64(v, vel_bounds)


# ---- angles and velocities ----------------------------------------------------------------------------------------------------------
@F32
@SIZES
def test_angles_within_the_atan2_bar_and_velocities_bit_for_bit(T, f32):
    rec = mc.records(T, T, f32)
    offsets = mc.offsets_for(T)
    want = ah.host_angle_array(rec, PAIRS)
    for delay, padding in ((1, 'zeros'), (10, 'circular'), (5000, 'zeros'), (300, 'circular')):
        angles, vels = device_angles(rec, offsets, PAIRS, delay, padding)
        if f32:
            assert (np.abs(angles - want) <= np.spacing(np.abs(want))).all()
        else:
            err = np.abs(angles - want).max()
            assert err <= mc.ANGLE_BAR, err
        assert mc.same_bits(vels, twin_velocities(angles, offsets, delay, padding))
    if not f32:
        print('T = %d: worst |device - twin| angle %.3g (bar %.3g)' % (T, np.abs(angles - want).max(), mc.ANGLE_BAR))
    # the clips: the velocities come from the unclipped angles
    clipped, cvels = device_angles(rec, offsets, PAIRS, 2, 'zeros', bounds=(-0.5, 1.0), vel_bounds=(-0.01, 0.02))
    assert mc.same_bits(clipped, ah._clip64(angles, (-0.5, 1.0)))
    assert mc.same_bits(cvels, twin_velocities(angles, offsets, 2, 'zeros', (-0.01, 0.02)))
    assert (clipped == 1.0).any() and (clipped == -0.5).any() and (cvels == 0.02).any()


def test_the_branch_cases_on_exact_quaternions():
    rec = np.zeros((6, 2, 7))
    rec[:, 0, 6] = 1.0
    rec[:, 1, 3:] = [[0, 0, 0, 1], [1, 0, 0, 1], [0, 1, 0, 1], [1, 1, -1, 1], [2.0 ** -30, 0, 0, 2.0 ** -30], [2.0 ** -20, 0, 0, 2.0 ** -20]]
    angles, vels = device_angles(rec, [0, 6], [(0, 1)])
    want = ah.host_angle_array(rec, [(0, 1)])
    assert np.abs(angles - want).max() <= mc.ANGLE_BAR
    assert np.array_equal(angles[[0, 4]], np.zeros((2, 3)))                            # the identity, and nq < _EPS
    assert np.array_equal(angles[2], [0.0, want[2, 1], 0.0]) and angles[3, 2] == 0.0   # the gimbal case: az = 0
    assert abs(angles[1, 0] - np.pi / 2) <= mc.ANGLE_BAR and abs(angles[5, 0] - np.pi / 2) <= mc.ANGLE_BAR
    a1, v1 = device_angles(rec[:1], [0, 1], [(0, 1)], 3, 'circular')                   # E = 1, one frame
    assert np.array_equal(a1, np.zeros((1, 3))) and np.array_equal(v1, np.zeros((1, 3)))


# ---- whitening ----------------------------------------------------------------------------------------------------------------------
def device_whiten(x, pad=2):
    import torch
    x = np.asarray(x)
    T, C = x.shape
    src, out = padded(x, pad), padded(np.zeros_like(x), pad, 44.0)
    moments = torch.full((2, C + 1), -7.0, dtype=torch.float64, device='cuda')
    work, need = workspace(T=T, C=C)
    _native.motion_whiten_device(src.data_ptr(), C + pad, T, C, work.data_ptr(), need, out.data_ptr(), C + pad, moments[0].data_ptr(),
                                 moments[1].data_ptr(), f64=x.dtype == np.float64)
    torch.cuda.synchronize()
    assert (out[:, C:] == 44.0).all() and (moments[:, C] == -7.0).all() and (src[:, C:] == 99.0).all()
    return out[:, :C].cpu().numpy().copy(), moments[0, :C].cpu().numpy().copy(), moments[1, :C].cpu().numpy().copy()


@F32
@SIZES
def test_moments_and_whitened_points_bit_for_bit(T, f32):
    rng = np.random.default_rng(T)
    x = (rng.normal(size=(T, 33)) * rng.uniform(0.01, 100.0, 33) + rng.normal(size=33)).astype(np.float32 if f32 else np.float64)
    x[:, 7] = 0.75                                                                     # a zero deviation becomes 1
    with pytest.warns(RuntimeWarning):
        want = ah.host_whiten(x)
    got = device_whiten(x)
    for a, b in zip(got, want):
        assert mc.same_bits(a, b)
    assert got[2][7] == 1.0 and mc.same_bits(got[0][:, 7], x[:, 7])


def test_whiten_takes_more_than_two_groups_and_sixty_columns():
    x = np.random.default_rng(3).normal(size=(2 * mc.GROUP + 77, 60)) + 3.0
    for a, b in zip(device_whiten(x, 0), ah.host_whiten(x)):
        assert mc.same_bits(a, b)
    with pytest.warns(RuntimeWarning):
        got = ah.whiten(np.hstack([x[:300, :2], np.ones((300, 1))]))
    with pytest.warns(RuntimeWarning):
        want = ah.host_whiten(np.hstack([x[:300, :2], np.ones((300, 1))]))
    assert all(mc.same_bits(a, b) for a, b in zip(got, want))


# ---- batched k-means ----------------------------------------------------------------------------------------------------------------
def device_kmeans(sets, inits, set_of, thresh=1e-5, max_iter=1000):
    """klnmf_motion_kmeans_device on point sets [D, T, d] laid out side by side with a sentinel column behind each set's d
    (set_stride = d + 1, ld = D (d + 1)): (codebooks [P, K, d], alive bool [P, K], distortion [P], iters [P], labels [P, T], open)."""
    import torch
    sets, inits = np.asarray(sets), np.asarray(inits)
    f32 = sets.dtype == np.float32
    (D, T, d), (P, K, _) = sets.shape, inits.shape
    buf = torch.full((T, D * (d + 1)), 99.0, dtype=tdt(f32), device='cuda')
    for s in range(D):
        buf[:, s * (d + 1):s * (d + 1) + d] = on_device(sets[s])
    cbs = on_device(inits.astype(sets.dtype))
    alive = torch.full((P, K), -7, dtype=torch.int32, device='cuda')
    dist = torch.full((P,), -7.0, dtype=torch.float64, device='cuda')
    iters = torch.full((P,), -7, dtype=torch.int32, device='cuda')
    labels = torch.full((P, T), -7, dtype=torch.int32, device='cuda')
    work, need = workspace(T=T, d=d, K=K, P=P, D=D)
    open_ = _native.motion_kmeans_device(buf.data_ptr(), d + 1, D * (d + 1), T, d, D, set_of, cbs.data_ptr(), K, thresh, max_iter,
                                         work.data_ptr(), need, alive.data_ptr(), dist.data_ptr(), iters.data_ptr(), labels.data_ptr(),
                                         f64=not f32)
    torch.cuda.synchronize()
    assert (buf.view(T, D, d + 1)[:, :, d] == 99.0).all()
    return cbs.cpu().numpy(), alive.cpu().numpy() != 0, dist.cpu().numpy(), iters.cpu().numpy(), labels.cpu().numpy(), open_


def check_kmeans(sets, inits, set_of, thresh=1e-5):
    got = device_kmeans(sets, inits, set_of, thresh)
    assert got[5] == -1
    for p, s in enumerate(set_of):
        cb, alive, dist, iters, labels = ah.host_kmeans_converged_from(sets[s], np.asarray(inits[p], dtype=sets.dtype), thresh)
        assert iters == got[3][p], (p, iters, got[3][p])
        assert mc.same_bits(got[4][p], labels) and mc.same_bits(got[1][p], alive)
        assert mc.same_bits(got[0][p], cb), p
        assert got[2][p] == dist, (p, got[2][p], dist)
    return got


@F32
@SIZES
def test_one_problem_bit_for_bit_around_the_tile_and_the_group(T, f32):
    pts, init = mc.clouds(T, 1, T, 2, 4, f32)
    check_kmeans(pts, init, [0])


@F32
def test_a_batch_whose_problems_stop_at_different_iterations(f32):
    D, R, T, K = 3, 3, 2 * mc.GROUP + 301, 16
    pts, _ = mc.clouds(11, D, T, 2, K, f32)
    rows = ah.draw_rows(np.random.default_rng(5), T, K, R, D)
    inits = np.stack([pts[s][rows[s, r]] for s in range(D) for r in range(R)])
    inits[4] = mc.far_init(inits[4])                                                   # one problem of the batch drops a cluster
    set_of = [s for s in range(D) for _ in range(R)]
    got = check_kmeans(pts, inits, set_of)
    assert len(set(got[3])) > 1, got[3]                                                # the iteration counts differ
    assert not got[1][4][1] and got[1][4].sum() == K - 1 and got[1].sum() == D * R * K - 1
    assert mc.same_bits(got[0][4][1], inits[4][1])                                     # a dropped row keeps its values
    print('iterations per problem:', list(got[3]))


@pytest.mark.parametrize('d,K', [(2, 1), (1, 5), (4, 256), (16, 64), (16, 1), (3, 100)])
def test_kmeans_at_the_limits_of_k_and_d(d, K):
    pts, init = mc.clouds(K + d, 2, 700, d, K)
    got = check_kmeans(pts, np.concatenate([init, init[:1]]), [0, 1, 1])               # problem 2: set 1 from set 0's rows
    assert got[1].shape == (3, K)


def test_the_public_kmeans_functions_equal_their_twins():
    import torch
    pts, init = mc.clouds(21, 3, 900, 2, 8)
    got, runs = ah.kmeans_converged_many(pts, 8, iter=3, rng=2, return_all=True)
    want, twin_runs = ah.host_kmeans_converged_many(pts, 8, iter=3, rng=2, return_all=True)
    assert all(mc.same_bits(a[0], b[0]) and a[1] == b[1] for a, b in zip(got, want))
    iters = runs.iters.cpu().numpy().reshape(3, 3)
    assert [[r[3] for r in per] for per in twin_runs] == iters.tolist()
    cb, dist = ah.kmeans_converged(on_device(pts[1]), 8, iter=3, rng=np.random.RandomState(4), output='device')
    want = ah.host_kmeans_converged(pts[1], 8, iter=3, rng=np.random.RandomState(4))
    assert torch.is_tensor(cb) and mc.same_bits(cb.cpu().numpy(), want[0]) and dist == want[1]
    cb, dist = ah.kmeans_converged(pts[0], mc.far_init(init[0]))
    want = ah.host_kmeans_converged(pts[0], mc.far_init(init[0]))
    assert cb.shape == (7, 2) and mc.same_bits(cb, want[0]) and dist == want[1]
    with pytest.raises(RuntimeError, match='max_iter = 2'):
        ah.kmeans_converged_many(pts, 8, iter=2, rng=2, thresh=0.0, max_iter=2)


# ---- histograms ---------------------------------------------------------------------------------------------------------------------
def device_hist(sets, cbs, offsets, soft_vq, pad=3):
    import torch
    sets, cbs = np.asarray(sets), np.asarray(cbs)
    f32 = sets.dtype == np.float32
    (D, T, d), K, E = sets.shape, cbs.shape[1], len(offsets) - 1
    out = torch.full((E, D * K + pad), 33.0, dtype=tdt(f32), device='cuda')
    work, need = workspace(T=T, d=d, K=K, D=D, E=E)
    d_sets, d_cbs = on_device(sets), on_device(cbs.astype(sets.dtype))
    _native.motion_hist_device(d_sets.data_ptr(), T * d, d, T, d, D, d_cbs.data_ptr(), K, offsets, 0 if soft_vq is None else 1,
                               soft_vq or 0.0, work.data_ptr(), need, out.data_ptr(), D * K + pad, f64=not f32)
    torch.cuda.synchronize()
    assert (out[:, D * K:] == 33.0).all()
    return out[:, :D * K].cpu().numpy().copy()


def check_hist(sets, cbs, offsets, label):
    K = cbs.shape[1]
    assert mc.same_bits(device_hist(sets, cbs, offsets, None), ah.host_histograms(sets, cbs, offsets))
    got, want = device_hist(sets, cbs, offsets, .5), ah.host_histograms(sets, cbs, offsets, .5)
    if sets.dtype == np.float32:
        assert (np.abs(got - want) <= np.spacing(want)).all()
        return
    with np.errstate(invalid='ignore', divide='ignore'):
        share = np.abs(got - want) / want / mc.soft_bar(np.diff(offsets), K)[:, np.newaxis]
    share[want == 0] = np.where(got[want == 0] == 0, 0.0, np.inf)
    with np.errstate(invalid='ignore', divide='ignore'):
        worst = np.nanmax(np.abs(got - want) / want)
    print('%s: soft matrix worst relative %.3g, worst share of its bar %.3g' % (label, worst, share.max()))
    assert (share <= 1.0).all()


@F32
@SIZES
def test_histograms_hard_bit_for_bit_soft_within_the_exp_bar(T, f32):
    pts, init = mc.clouds(T + 1, 2, T, 2, 5, f32)
    check_hist(pts, init, mc.offsets_for(T), 'T = %d' % T)


@pytest.mark.parametrize('d,K', [(2, 1), (1, 5), (4, 256), (16, 64)])
def test_histograms_at_the_limits_and_over_more_than_two_groups(d, K):
    T = 2 * mc.GROUP + 301 if K == 5 else 700
    pts, init = mc.clouds(K + d + 1, 2, T, d, K)
    check_hist(pts, init, mc.offsets_for(T), 'd = %d, K = %d' % (d, K))


# ---- refusals: every one of the header at its boundary, nothing written ----------------------------------------------------------
def test_every_refusal_of_the_header_leaves_everything_unwritten():
    import torch
    T, M, d, K, D, P, E = 40, 3, 2, 4, 2, 3, 2
    rec = on_device(mc.records(1, T, False, M))
    pts, init = mc.clouds(5, D, T, d, K)
    d_pts, d_cbs = on_device(pts), on_device(np.concatenate([init, init[:1]]))
    outs = [torch.full((T, 8), -3.0, dtype=torch.float64, device='cuda') for _ in range(3)]
    small = [torch.full((64,), -3.0, dtype=torch.float64, device='cuda') for _ in range(2)]
    ints = [torch.full((P * T,), -3, dtype=torch.int32, device='cuda') for _ in range(3)]
    work = torch.full((1 << 16,), 7, dtype=torch.uint8, device='cuda')
    before = [t.clone() for t in outs + small + ints + [work, d_cbs, d_pts]]
    off, pairs = [0, 15, T], [(0, 1), (2, 0)]
    wb, NULL = 1 << 16, 0

    def refused(code, fn, *args, **kw):
        with pytest.raises(_native.NativeError) as e:
            fn(*args, **kw)
        assert e.value.code == code, (fn.__name__, args, e.value)

    ARG, UNSUPP = _native.ERR_ARG, _native.ERR_UNSUPP
    lib = _native.load()

    def angles(records=rec.data_ptr(), T=T, M=M, pairs=pairs, off=off, delay=1, padding=0, bounds=None, vb=None, work=work.data_ptr(),
               wb=wb, a=outs[0].data_ptr(), lda=8, v=outs[1].data_ptr(), ldv=8, f64=True):
        _native.motion_angles_device(records, T, M, pairs, off, delay, padding, bounds, vb, work, wb, a, lda, v, ldv, f64=f64)
    for kw in (dict(records=NULL), dict(work=NULL), dict(a=NULL), dict(v=NULL), dict(lda=5), dict(ldv=5), dict(T=0), dict(M=0),
               dict(pairs=[(0, 3)]), dict(pairs=[(-1, 0)]), dict(off=[1, 15, T]), dict(off=[0, 16, 15, T]), dict(off=[0, 15, T - 1]),
               dict(delay=0), dict(padding=2), dict(bounds=(1.0, 0.5)), dict(vb=(np.nan, 1.0)),
               dict(wb=_native.motion_work_bytes(T, E=E) - 1)):
        refused(ARG, angles, **kw)
    refused(UNSUPP, angles, pairs=[(0, 1)] * 33, lda=99, ldv=99)
    need = _native.motion_work_bytes(T, E=E)
    for dtype, p_pairs, p_off, n_pairs in ((2, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)):       # bad dtype, null pairs / offsets
        host = np.zeros(4, dtype=np.int64)
        host[2] = T
        h = host.ctypes.data
        assert lib.klnmf_motion_angles_device(0, dtype, rec.data_ptr(), T, M, h if p_pairs else None, n_pairs, h + 8 if p_off else None,
                                              1, 1, 0, None, None, work.data_ptr(), need, outs[0].data_ptr(), 8, outs[1].data_ptr(),
                                              8) == ARG

    def whiten(x=outs[2].data_ptr(), ld=8, T=T, C=6, work=work.data_ptr(), wb=wb, out=outs[0].data_ptr(), ldo=8, mean=small[0].data_ptr(),
               std=small[1].data_ptr()):
        _native.motion_whiten_device(x, ld, T, C, work, wb, out, ldo, mean, std)
    for kw in (dict(x=NULL), dict(work=NULL), dict(out=NULL), dict(mean=NULL), dict(std=NULL), dict(ld=5), dict(ldo=5), dict(T=0),
               dict(C=0), dict(wb=_native.motion_work_bytes(T, C=6) - 1)):
        refused(ARG, whiten, **kw)
    assert lib.klnmf_motion_whiten_device(0, 7, outs[2].data_ptr(), 8, T, 6, work.data_ptr(), wb, outs[0].data_ptr(), 8,
                                          small[0].data_ptr(), small[1].data_ptr()) == ARG

    def kmeans(pts=d_pts.data_ptr(), ss=T * d, ld=d, T=T, d=d, D=D, set_of=(0, 1, 1), cbs=d_cbs.data_ptr(), K=K, thresh=1e-5, mi=10,
               work=work.data_ptr(), wb=wb, alive=ints[0].data_ptr(), dist=small[0].data_ptr(), iters=ints[1].data_ptr(),
               labels=ints[2].data_ptr(), f64=True):
        _native.motion_kmeans_device(pts, ss, ld, T, d, D, set_of, cbs, K, thresh, mi, work, wb, alive, dist, iters, labels, f64=f64)
    for kw in (dict(pts=NULL), dict(cbs=NULL), dict(work=NULL), dict(alive=NULL), dict(dist=NULL), dict(iters=NULL), dict(ld=1), dict(ss=-1),
               dict(T=0), dict(d=0), dict(K=0), dict(D=0), dict(set_of=(0, 2, 1)), dict(set_of=(0, -1, 1)), dict(thresh=-1e-9),
               dict(thresh=np.nan), dict(mi=0), dict(wb=_native.motion_work_bytes(T, d=d, K=K, P=P, D=D) - 1)):
        refused(ARG, kmeans, **kw)
    for kw in (dict(K=257), dict(d=17, ld=17), dict(K=129, d=8, ld=8), dict(D=65536)):
        refused(UNSUPP, kmeans, **kw)
    sets3 = np.array([0, 1, 1], dtype=np.int32)
    un = np.zeros(1, dtype=np.int32)
    common = (d_cbs.data_ptr(), K, 1e-5, 10, work.data_ptr(), wb, ints[0].data_ptr(), small[0].data_ptr(), ints[1].data_ptr(), None)
    assert lib.klnmf_motion_kmeans_device(0, 1, d_pts.data_ptr(), T * d, d, T, d, D, None, 3, *common, un.ctypes.data_as(_native._c.POINTER(_native._c.c_int))) == ARG
    assert lib.klnmf_motion_kmeans_device(0, 1, d_pts.data_ptr(), T * d, d, T, d, D, sets3.ctypes.data, 3, *common, None) == ARG
    assert lib.klnmf_motion_kmeans_device(0, 1, d_pts.data_ptr(), T * d, d, T, d, D, sets3.ctypes.data, 0, *common, un.ctypes.data_as(_native._c.POINTER(_native._c.c_int))) == ARG
    assert lib.klnmf_motion_kmeans_device(0, 3, d_pts.data_ptr(), T * d, d, T, d, D, sets3.ctypes.data, 3, *common, un.ctypes.data_as(_native._c.POINTER(_native._c.c_int))) == ARG

    def hist(pts=d_pts.data_ptr(), ss=T * d, ld=d, T=T, d=d, D=D, cbs=d_cbs.data_ptr(), K=K, off=off, soft=0, alpha=0.5, work=work.data_ptr(),
             wb=wb, out=outs[0].data_ptr(), ldo=8, f64=True):
        _native.motion_hist_device(pts, ss, ld, T, d, D, cbs, K, off, soft, alpha, work, wb, out, ldo, f64=f64)
    for kw in (dict(pts=NULL), dict(cbs=NULL), dict(work=NULL), dict(out=NULL), dict(ld=1), dict(ss=-1), dict(ldo=7), dict(T=0), dict(d=0),
               dict(K=0), dict(D=0), dict(off=[1, 15, T]), dict(off=[0, 16, 15, T]), dict(off=[0, 15, T + 1]), dict(soft=2), dict(soft=-1),
               dict(soft=1, alpha=np.inf), dict(alpha=np.nan), dict(wb=_native.motion_work_bytes(T, d=d, K=K, D=D, E=E) - 1)):
        refused(ARG, hist, **kw)
    for kw in (dict(K=257, ldo=9999), dict(d=17, ld=17), dict(K=129, d=8, ld=8, ldo=9999), dict(D=65536, ldo=1 << 30)):
        refused(UNSUPP, hist, **kw)
    host = np.array([0, 15, T], dtype=np.int64)
    assert lib.klnmf_motion_hist_device(0, 5, d_pts.data_ptr(), T * d, d, T, d, D, d_cbs.data_ptr(), K, host.ctypes.data, E, 0, 0.5,
                                        work.data_ptr(), wb, outs[0].data_ptr(), 8) == ARG
    assert lib.klnmf_motion_hist_device(0, 1, d_pts.data_ptr(), T * d, d, T, d, D, d_cbs.data_ptr(), K, None, E, 0, 0.5,
                                        work.data_ptr(), wb, outs[0].data_ptr(), 8) == ARG
    assert lib.klnmf_motion_hist_device(0, 1, d_pts.data_ptr(), T * d, d, T, d, D, d_cbs.data_ptr(), K, host.ctypes.data, 0, 0, 0.5,
                                        work.data_ptr(), wb, outs[0].data_ptr(), 8) == ARG
    torch.cuda.synchronize()
    for now, then in zip(outs + small + ints + [work, d_cbs, d_pts], before):
        assert torch.equal(now, then)
    # and the accepted boundary values right beside: the limits themselves run
    check_kmeans(*(lambda c: (c[0], c[1], [0]))(mc.clouds(9, 1, 300, 4, 256)))


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('source', ['host', 'device'])
def test_g23_through_vq_hist_matrix(source):
    import torch
    g = mc.golden()
    names, offsets = list(g['names']), g['w_offsets']
    rec = g['w_records'] if source == 'host' else on_device(g['w_records'])
    kw = dict(nb_bins=4, iter=3, rng=17)
    angles, vels, off = ah.angle_arrays((rec, offsets), names)
    assert (np.abs(angles - g['w_angles']) <= mc.angle_bar_reference(g['w_angles']) + mc.ANGLE_BAR).all() and mc.same_bits(off, offsets)
    for soft in (None, .5):
        X, cbs = ah.vq_hist_matrix((rec, offsets), names, soft_vq=soft, return_codebooks=True,
                                   output='numpy' if source == 'host' else 'device', **kw)
        if source == 'device':
            assert torch.is_tensor(X) and X.is_cuda and X.shape == (6, 120)
            X, cbs = X.cpu().numpy(), cbs.cpu().numpy()
        want, want_cbs = ah.host_vq_hist_matrix_from_angles(angles, vels, offsets, soft_vq=soft, return_codebooks=True, **kw)
        assert mc.same_bits(cbs, want_cbs)
        if soft is None:
            assert mc.same_bits(X, want)
        else:
            assert (np.abs(X - want) <= mc.soft_bar(np.diff(offsets), 4)[:, np.newaxis] * want).all()
    # the grid set: two degrees of freedom whose (angle, velocity) points are the recorded grid points
    pts = g['g_points']
    a, v = np.ascontiguousarray(pts[:, :, 0].T), np.ascontiguousarray(pts[:, :, 1].T)
    if source == 'device':
        a, v = on_device(a), on_device(v)
    for soft in (None, .5):
        X = ah.vq_hist_matrix_from_angles(a, v, g['g_offsets'], nb_bins=8, iter=3, rng=3, soft_vq=soft)
        want = ah.host_vq_hist_matrix_from_angles(pts[:, :, 0].T, pts[:, :, 1].T, g['g_offsets'], nb_bins=8, iter=3, rng=3, soft_vq=soft)
        if soft is None:
            assert mc.same_bits(X, want)
        else:
            assert (np.abs(X - want) <= mc.soft_bar(np.diff(g['g_offsets']), 8)[:, np.newaxis] * want).all()
