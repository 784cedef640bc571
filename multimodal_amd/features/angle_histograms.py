# encoding: utf-8
"""The motion modality: Kinect records to the matrix of vector-quantisation histograms of (angle, velocity) points, the
reference's `db_to_VQ_hist_matrix` (multimodal/features/angle_histograms.py:171-223), with every stage on the device.

The stages, each with a host twin in vectorised numpy (`host_*`) that restates the rules of csrc/motion.hip.h, the order of every
sum included, and a device path on include/klnmf_motion.h:

1. `angle_arrays`: per frame and (source, dest) pair of `ANGLES` the Euler angles ('sxyz') of q_src^-1 * q_dst -- the reference
   makes one Python call per frame and joint (:45-67) -- and per example the delayed velocities (lib/utils.py:103-123), with the
   optional clip to bounds (`filter_values`).
2. `whiten`: per column x / std, std = sqrt(sum((x - mean)^2) / T), a zero deviation taken as 1 (scipy's `whiten`).
3. `kmeans_converged`, `kmeans_converged_many`: scipy's `kmeans` -- Lloyd iterations until the mean distance of the points to
   their codes changes by no more than `thresh`, a cluster without members dropped for good, `iter` restarts from drawn rows, the
   lowest distortion kept (the first among equals).  All restarts of all point sets advance together, two launches per iteration.
4. `histograms`: per example the sum of the frames' hard (one-hot) or soft (lib/vector_quantization.py:36-48) associations, laid
   out [example][dof][bin], each row divided by its sum.
5. `vq_hist_matrix`, `vq_hist_matrix_from_angles`: the whole chain; between the stages only the stop flags, the restarts'
   distortions and live-row masks (P numbers each) and the drawn row indices cross the bus.

THE SUMMATION ORDER (features.codebook's): every sum over frames -- a column's sum and sum of squared deviations, a cluster's
column sums, the sum of distances -- is formed per group of GROUP = 4096 consecutive frames, the group's contributing frames
added in ascending order starting from +0, and the groups' partial sums are then added in ascending group order starting from
+0.  A histogram bin adds its example's frames in ascending order from +0; a row's sum adds the columns in ascending order.
Every operation is fp64, each rounded on its own; float32 storage rounds a stored result once more.

Against the reference: the angles use numpy's arctan2 and sqrt where it uses math's; scipy's `update_cluster_means` adds a
cluster's members in one ascending chain and numpy's `mean` / `sum` add pairwise, so on data whose sums are not exact the twin's
last bits differ from scipy's (tests/golden/make_golden_motion.py records by how much); on grid data they are equal.

`vel_delay`: the reference's `db_to_VQ_hist_matrix` accepts `vel_delay` and `vel_padding` and then passes a hard-coded 1 and
'zeros' (:192).  Here the arguments are honoured; the defaults, 1 and 'zeros', reproduce the reference.

Not here: `db_to_binned_hist_matrix` and the KDE smoother (lib/kde2d.py), the dataset loaders.
"""
import warnings

import numpy as np

from .. import _native
from . import hac

GROUP = _native.MOTION_GROUP
MAX_K, MAX_D, MAX_KD = _native.MOTION_MAX_K, _native.MOTION_MAX_D, _native.MOTION_MAX_KD
MAX_PAIRS, MAX_P, POLL = _native.MOTION_MAX_PAIRS, _native.MOTION_MAX_P, _native.MOTION_POLL
EPS = 4.0 * np.finfo(np.float64).eps           # lib/transformations.py's _EPS
SOFT_EPSILON = 1.e-9                           # lib/vector_quantization.py's EPSILON

ANGLES = [
    ('left_shoulder', 'left_elbow'),
    ('left_elbow', 'left_hand'),
    ('torso', 'left_hip'),
    ('left_hip', 'left_knee'),
    ('left_knee', 'left_foot'),
    ('right_shoulder', 'right_elbow'),
    ('right_elbow', 'right_hand'),
    ('torso', 'right_hip'),
    ('right_hip', 'right_knee'),
    ('right_knee', 'right_foot'),
]


def angles_indices(marker_names):
    """[(source index, dest index)] of `ANGLES` in `marker_names` (features/angle_histograms.py:40-42)."""
    marker_names = list(marker_names)
    return [(marker_names.index(source), marker_names.index(dest)) for source, dest in ANGLES]


# ---- the host twins -----------------------------------------------------------------------------------------------------------------
def _float_type(*arrays):
    return np.float32 if all(str(a.dtype).endswith('float32') for a in arrays) else np.float64


def _chain(v):
    """The sum of v over axis 0 in ascending order starting from +0."""
    return np.cumsum(np.concatenate([np.zeros((1,) + v.shape[1:]), v]), axis=0)[-1]


def _order_sum(v):
    """The sum of float64 v over axis 0 under the summation order."""
    total = np.zeros(v.shape[1:])
    for g0 in range(0, max(1, v.shape[0]), GROUP):
        total = total + _chain(v[g0:g0 + GROUP])
    return total


def host_angle_array(records, angles_idx):
    """[T, 3 len(angles_idx)]: `record_to_angle_array` (features/angle_histograms.py:45-67) for every frame of records
    [T, n_markers, 7] at once, the operations of lib/transformations.py in their order.  float32 if `records` is."""
    records = np.asarray(records)
    dt = _float_type(records)
    r = records.astype(np.float64)
    out = np.empty((r.shape[0], 3 * len(angles_idx)))
    for p, (src, dst) in enumerate(angles_idx):
        sx, sy, sz, sw = (r[:, src, 3 + i] for i in range(4))
        x0, y0, z0, w0 = (r[:, dst, 3 + i] for i in range(4))
        with np.errstate(all='ignore'):
            ns = ((sx * sx + sy * sy) + sz * sz) + sw * sw
            x1, y1, z1, w1 = -sx / ns, -sy / ns, -sz / ns, sw / ns
            q0 = ((x1 * w0 + y1 * z0) - z1 * y0) + w1 * x0
            q1 = ((-x1 * z0 + y1 * w0) + z1 * x0) + w1 * y0
            q2 = ((x1 * y0 - y1 * x0) + z1 * w0) + w1 * z0
            q3 = ((-x1 * x0 - y1 * y0) - z1 * z0) + w1 * w0
            nq = ((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3
            s = np.sqrt(2.0 / nq)
            q0, q1, q2, q3 = q0 * s, q1 * s, q2 * s, q3 * s
            unit = nq < EPS                                                 # quaternion_matrix's identity branch
            pick = lambda value, identity: np.where(unit, identity, value)
            m00 = pick((1.0 - q1 * q1) - q2 * q2, 1.0)
            m10 = pick(q0 * q1 + q2 * q3, 0.0)
            m20 = pick(q0 * q2 - q1 * q3, 0.0)
            m11 = pick((1.0 - q0 * q0) - q2 * q2, 1.0)
            m12 = pick(q1 * q2 - q0 * q3, 0.0)
            m21 = pick(q1 * q2 + q0 * q3, 0.0)
            m22 = pick((1.0 - q0 * q0) - q1 * q1, 1.0)
            cy = np.sqrt(m00 * m00 + m10 * m10)
            regular = cy > EPS
            out[:, 3 * p] = np.where(regular, np.arctan2(m21, m22), np.arctan2(-m12, m11))
            out[:, 3 * p + 1] = np.arctan2(-m20, cy)
            out[:, 3 * p + 2] = np.where(regular, np.arctan2(m10, m00), 0.0)
    return out.astype(dt)


def _check_delay(delay, padding):
    if int(delay) != delay or int(delay) < 1:
        raise ValueError("vel_delay: an integer >= 1 expected, got %r (the reference's slice breaks below 1)" % (delay,))
    if padding not in _native.MOTION_PADDINGS:
        raise ValueError("Wrong padding (either 'circular' or 'zeros')")


def host_delayed_velocities(delay, positions, padding='zeros'):
    """`delayed_velocities(delay, positions, padding)` (lib/utils.py:103-123) of one example; the difference formed in float64."""
    _check_delay(delay, padding)
    positions = np.asarray(positions)
    p = positions.astype(np.float64)
    n = p.shape[0]
    delay = min(int(delay), n)
    head = p[n - delay:] if padding == 'circular' else np.zeros((delay, p.shape[1]))
    return (p - np.vstack([head, p[:n - delay]])).astype(_float_type(positions))


def _clip64(x, bounds):
    """The cut in float64, stored in x's type (the device's)."""
    return x if bounds is None else np.maximum(np.minimum(x.astype(np.float64), bounds[1]), bounds[0]).astype(x.dtype)


def host_angle_arrays(records, markers, vel_delay=1, vel_padding='zeros', bounds=None, vel_bounds=None):
    """(angles, vels, offsets): `angle_arrays`' numpy twin."""
    stacked, offsets, pairs = check_records(records, markers, vel_delay, vel_padding, bounds, vel_bounds)
    angles = host_angle_array(stacked, pairs)
    vels = np.vstack([host_delayed_velocities(vel_delay, angles[a:b], vel_padding) for a, b in zip(offsets[:-1], offsets[1:])])
    return _clip64(angles, bounds), _clip64(vels, vel_bounds), offsets


def host_whiten(x):
    """(x / std, mean, std) per column under the summation order -- klnmf_motion_whiten_device's numpy twin.  The warning of
    scipy's `whiten` on a zero deviation is kept."""
    x = np.asarray(x)
    dt = _float_type(x)
    x64 = x.astype(np.float64)
    T = x64.shape[0]
    mean = _order_sum(x64) / float(T)
    dev = x64 - mean
    std = np.sqrt(_order_sum(dev * dev) / float(T))
    if np.any(std == 0):
        std[std == 0] = 1.0
        warnings.warn("Some columns have standard deviation zero. The values of these columns will not change.", RuntimeWarning,
                      stacklevel=2)
    return (x64 / std).astype(dt), mean, std


def square_distances(x64, c64):
    """float64 [T, K]: `square_distances` (lib/vector_quantization.py:15-25) in its direct form, j ascending."""
    acc = np.zeros((x64.shape[0], c64.shape[0]))
    for j in range(x64.shape[1]):
        df = x64[:, j][:, np.newaxis] - c64[:, j][np.newaxis, :]
        acc = acc + df * df
    return acc


def host_kmeans_converged_from(points, init, thresh=1e-5, max_iter=1000):
    """One problem of klnmf_motion_kmeans_device in numpy: (codebook [K, d] with the dropped rows in place, alive bool [K],
    distortion, iterations, labels int32 [T] of the last assignment).  scipy's `_kmeans(obs, guess, thresh)` returns
    (codebook[alive], distortion)."""
    points, init = np.asarray(points), np.asarray(init)
    dt = _float_type(points, init)
    x64 = np.ascontiguousarray(points, dtype=dt).astype(np.float64)
    cb = np.array(init, dtype=dt, order='C')
    K, T = cb.shape[0], x64.shape[0]
    alive = np.ones(K, dtype=bool)
    prev = np.inf
    for it in range(1, int(max_iter) + 1):
        live = np.flatnonzero(alive)
        d2 = square_distances(x64, cb[live].astype(np.float64))
        pos = np.argmin(d2, axis=1)                                        # the first among equal minima
        labels = live[pos].astype(np.int32)
        now = float(_order_sum(np.sqrt(d2[np.arange(T), pos])[:, np.newaxis])[0] / float(T))
        sums, counts = np.zeros((K, x64.shape[1])), np.bincount(labels, minlength=K)
        for g0 in range(0, T, GROUP):
            part = np.zeros_like(sums)
            np.add.at(part, labels[g0:g0 + GROUP], x64[g0:g0 + GROUP])     # unbuffered: row by row, ascending
            sums = sums + part
        full = counts > 0
        cb[full] = (sums[full] / counts[full].astype(np.float64)[:, np.newaxis]).astype(dt)
        alive = alive & full
        diff = abs(prev - now)
        prev = now
        if diff <= thresh:
            return cb, alive, now, it, labels
    raise RuntimeError("k-means problem 0 has not stopped after max_iter = %d iterations" % max_iter)


def _rng(rng):
    if isinstance(rng, (np.random.Generator, np.random.RandomState)):
        return rng
    return np.random.default_rng(rng)


def draw_rows(rng, T, k, restarts, sets=1):
    """int64 [sets, restarts, k]: scipy's `_kpoints` draws, `rng.choice(T, size=k, replace=False)`, set after set, restart after
    restart -- the order in which `kmeans(d, k, iter)` per set consumes the generator."""
    return np.array([[rng.choice(T, size=int(k), replace=False) for _ in range(restarts)] for _ in range(sets)],
                    dtype=np.int64).reshape(sets, restarts, int(k))


def host_kmeans_converged(data, k_or_guess, iter=20, thresh=1e-5, rng=None, max_iter=1000):
    """(codebook, distortion): scipy's `kmeans(data, k_or_guess, iter, thresh)` under the stated rules."""
    data = np.asarray(data)
    if np.ndim(k_or_guess) == 2:
        cb, alive, dist, _, _ = host_kmeans_converged_from(data, k_or_guess, thresh, max_iter)
        return cb[alive], dist
    return host_kmeans_converged_many(data[np.newaxis], k_or_guess, iter, thresh, rng, max_iter)[0]


def host_kmeans_converged_many(point_sets, k, iter=20, thresh=1e-5, rng=None, max_iter=1000, return_all=False):
    """[(codebook, distortion)] per point set of [D, T, d]; `return_all`: also the restarts' (codebook, alive, distortion,
    iterations, labels) as [D][iter]."""
    point_sets, k, iter = _check_many(point_sets, k, iter, thresh, max_iter)
    D, T, _ = point_sets.shape
    rows = draw_rows(_rng(rng), T, k, iter, D)
    runs = [[host_kmeans_converged_from(point_sets[s], point_sets[s][rows[s, r]], thresh, max_iter) for r in range(iter)]
            for s in range(D)]
    best = [int(np.argmin([run[2] for run in per_set])) for per_set in runs]
    out = [(runs[s][b][0][runs[s][b][1]], runs[s][b][2]) for s, b in enumerate(best)]
    return (out, runs) if return_all else out


def host_histograms(point_sets, codebooks, offsets, soft_vq=None):
    """[E, D K]: klnmf_motion_hist_device's numpy twin on point sets [D, T, d] and codebooks [D, K, d]."""
    point_sets, codebooks = np.asarray(point_sets), np.asarray(codebooks)
    dt = _float_type(point_sets, codebooks)
    D, K = codebooks.shape[0], codebooks.shape[1]
    offsets = np.asarray(offsets, dtype=np.int64)
    E = offsets.size - 1
    raw = np.zeros((E, D, K))
    for s in range(D):
        d2 = square_distances(point_sets[s].astype(dt).astype(np.float64), codebooks[s].astype(dt).astype(np.float64))
        least = np.min(d2, axis=1)
        if soft_vq is None:
            h = np.zeros_like(d2)
            h[np.arange(d2.shape[0]), np.argmin(d2, axis=1)] = 1.0
        else:
            w = np.exp(-float(soft_vq) * d2 / (SOFT_EPSILON + least[:, np.newaxis]))
            h = w / _chain(w.T)[:, np.newaxis]
        for e in range(E):
            raw[e, s] = _chain(h[offsets[e]:offsets[e + 1]])
    raw = raw.reshape(E, D * K)
    with np.errstate(invalid='ignore'):
        return (raw / _chain(raw.T)[:, np.newaxis]).astype(dt)


def _interleave(angles, vels):
    """[T, 2 D]: column 2 s the angle, 2 s + 1 the velocity of degree of freedom s."""
    return np.stack([angles, vels], axis=2).reshape(angles.shape[0], -1)


def _full_codebooks(best, nb_bins):
    for s, (cb, _) in enumerate(best):
        if cb.shape[0] != nb_bins:
            raise ValueError("degree of freedom %d: the best codebook lost %d of its %d clusters; the histogram matrix needs "
                             "nb_bins rows of every codebook" % (s, nb_bins - cb.shape[0], nb_bins))
    return np.stack([cb for cb, _ in best])


def host_vq_hist_matrix_from_angles(angles, vels, offsets, nb_bins=16, soft_vq=None, iter=20, thresh=1e-5, rng=None, max_iter=1000,
                                    return_codebooks=False):
    """`vq_hist_matrix_from_angles`' numpy twin."""
    angles, vels, offsets = check_angles(angles, vels, offsets)
    white, _, _ = host_whiten(_interleave(np.asarray(angles), np.asarray(vels)))
    sets = np.ascontiguousarray(white.reshape(white.shape[0], -1, 2).transpose(1, 0, 2))
    best = host_kmeans_converged_many(sets, nb_bins, iter, thresh, rng, max_iter)
    cbs = _full_codebooks(best, nb_bins)
    X = host_histograms(sets, cbs, offsets, soft_vq)
    return (X, cbs) if return_codebooks else X


def host_vq_hist_matrix(records, markers, vel_delay=1, vel_padding='zeros', nb_bins=16, bounds=None, vel_bounds=None, soft_vq=None,
                        iter=20, thresh=1e-5, rng=None, max_iter=1000, return_codebooks=False):
    """`vq_hist_matrix`' numpy twin: `db_to_VQ_hist_matrix` (features/angle_histograms.py:171-223) under the stated rules."""
    angles, vels, offsets = host_angle_arrays(records, markers, vel_delay, vel_padding, bounds, vel_bounds)
    return host_vq_hist_matrix_from_angles(angles, vels, offsets, nb_bins, soft_vq, iter, thresh, rng, max_iter, return_codebooks)


# ---- the checks: ValueError before any native call --------------------------------------------------------------------------------
def _is_float_tensor(a):
    return hac._is_tensor(a) and str(a.dtype) in ('torch.float32', 'torch.float64')


def _host_float(a, what, ndim):
    a = np.asarray(a)
    if a.ndim != ndim:
        raise ValueError("%s: %d dimensions expected, got shape %s" % (what, ndim, a.shape))
    a = np.ascontiguousarray(a, dtype=a.dtype if a.dtype in (np.float32, np.float64) else np.float64)
    if not np.all(np.isfinite(a)):
        raise ValueError("%s: values that are not finite" % what)
    return a


def _check_bounds(b, what):
    if b is not None and not (len(b) == 2 and float(b[0]) <= float(b[1])):
        raise ValueError("%s: (min, max) with min <= max expected, got %r" % (what, b))


def _check_offsets(offsets, T):
    offsets = np.asarray(offsets)
    if offsets.ndim != 1 or offsets.size < 2 or not np.issubdtype(offsets.dtype, np.integer):
        raise ValueError("offsets: integers [E + 1], E >= 1, expected")
    offsets = offsets.astype(np.int64)
    if offsets[0] != 0 or offsets[-1] != T or np.any(np.diff(offsets) < 0):
        raise ValueError("offsets: 0 = offsets[0] <= ... <= offsets[E] = T = %d expected" % T)
    return offsets


def check_records(records, markers, vel_delay=1, vel_padding='zeros', bounds=None, vel_bounds=None):
    """(stacked [T, n_markers, 7], offsets int64 [E + 1], pairs [(source, dest)]) or ValueError.  records: a sequence of examples
    [n_e, n_markers, 7] (host arrays, or float tensors of one type on one device), or a pair (stacked [T, n_markers, 7], offsets).
    markers: the marker names (the pairs are `ANGLES`') or the (source, dest) index pairs themselves."""
    _check_delay(vel_delay, vel_padding)
    _check_bounds(bounds, 'bounds')
    _check_bounds(vel_bounds, 'vel_bounds')
    markers = list(markers)
    if not markers:
        raise ValueError("markers: names or (source, dest) pairs expected")
    pairs = angles_indices(markers) if isinstance(markers[0], str) else [(int(s), int(d)) for s, d in markers]
    if len(pairs) > MAX_PAIRS:
        raise ValueError("%d marker pairs are above the %d of one call" % (len(pairs), MAX_PAIRS))
    paired = isinstance(records, tuple) and len(records) == 2 and np.ndim(records[1]) == 1 and not hac._is_tensor(records[1]) \
        and np.ndim(records[0]) == 3
    examples = [records[0]] if paired else list(records)
    if not examples:
        raise ValueError("records: at least one example expected")
    if all(hac._is_tensor(r) for r in examples):
        if any(not _is_float_tensor(r) or r.dim() != 3 or r.dtype != examples[0].dtype for r in examples):
            raise ValueError("records: float32 / float64 tensors [n, n_markers, 7] of one type expected")
        import torch
        stacked = examples[0].contiguous() if len(examples) == 1 else torch.cat(examples)
    else:
        examples = [_host_float(r, "records", 3) for r in examples]
        stacked = np.concatenate(examples).astype(_float_type(*examples))
    T, M = int(stacked.shape[0]), int(stacked.shape[1])
    if any(r.shape[1:] != stacked.shape[1:] for r in examples) or stacked.shape[2] != 7 or T < 1 or T >= 2 ** 31 - 1:
        raise ValueError("records: examples [n, n_markers, 7] with 1 <= T < 2^31 - 1 frames in all expected")
    if any(not 0 <= i < M for pair in pairs for i in pair):
        raise ValueError("a marker index outside [0, %d)" % M)
    offsets = _check_offsets(records[1] if paired else np.concatenate([[0], np.cumsum([int(r.shape[0]) for r in examples])]), T)
    return stacked, offsets, pairs


def check_angles(angles, vels, offsets):
    """(angles, vels, offsets) as the device path uses them, or ValueError: two matrices [T, D] of one kind (host arrays, or
    float tensors of one type), finite where they are host arrays; offsets as `check_records`."""
    if hac._is_tensor(angles) or hac._is_tensor(vels):
        if not (_is_float_tensor(angles) and _is_float_tensor(vels)) or angles.dim() != 2 or angles.dtype != vels.dtype:
            raise ValueError("angles, vels: two float32 / float64 tensors [T, D] of one type expected")
    else:
        angles, vels = _host_float(angles, "angles", 2), _host_float(vels, "vels", 2)
        dt = _float_type(angles, vels)
        angles, vels = angles.astype(dt), vels.astype(dt)
    if tuple(angles.shape) != tuple(vels.shape) or angles.shape[0] < 1 or angles.shape[1] < 1 or angles.shape[1] > MAX_P:
        raise ValueError("angles %s against vels %s: two matrices [T >= 1, 1 <= D <= %d] expected"
                         % (tuple(angles.shape), tuple(vels.shape), MAX_P))
    return angles, vels, _check_offsets(offsets, int(angles.shape[0]))


def _check_many(point_sets, k, iter, thresh, max_iter):
    if not hac._is_tensor(point_sets):
        point_sets = _host_float(point_sets, "point_sets", 3)
    elif not _is_float_tensor(point_sets) or point_sets.dim() != 3:
        raise ValueError("point_sets: a float32 / float64 tensor [D, T, d] expected")
    D, T, d = (int(n) for n in point_sets.shape)
    if np.ndim(k) != 0 or int(k) != k or int(k) < 1:
        raise ValueError("k: an integer >= 1 expected, got %r" % (k,))
    if int(iter) != iter or int(iter) < 1:
        raise ValueError("iter must be at least 1, got %r" % (iter,))
    _check_sizes(D, T, d, int(k), D * int(iter), thresh, max_iter)
    if int(k) > T:
        raise ValueError("k = %d rows cannot be drawn from T = %d points without replacement" % (k, T))
    return point_sets, int(k), int(iter)


def _check_sizes(D, T, d, K, P, thresh, max_iter):
    if D < 1 or d < 1 or T < 1 or T >= 2 ** 31 - 1:
        raise ValueError("point sets [D >= 1, 1 <= T < 2^31 - 1, d >= 1] expected, got %s" % ((D, T, d),))
    if K > MAX_K or d > MAX_D or K * d > MAX_KD:
        raise ValueError("K = %d, d = %d: beyond K <= %d, d <= %d, K * d <= %d" % (K, d, MAX_K, MAX_D, MAX_KD))
    if P > MAX_P or D > MAX_P:
        raise ValueError("%d problems on %d point sets: at most %d of each in one call" % (P, D, MAX_P))
    if not float(thresh) >= 0:
        raise ValueError("thresh: a number >= 0 expected, got %r" % (thresh,))
    if int(max_iter) != max_iter or int(max_iter) < 1:
        raise ValueError("max_iter: an integer >= 1 expected, got %r" % (max_iter,))


def _check_output(output):
    if output not in ('numpy', 'device'):
        raise ValueError("output: 'numpy' or 'device', got %r" % (output,))


# ---- the device path ----------------------------------------------------------------------------------------------------------------
class _Device(object):
    """The device, its tensors' types and one workspace that grows to the largest call."""

    def __init__(self, device, f64):
        import torch
        self.torch = torch
        self.dev = hac._torch_device(device)
        self.ordinal = self.dev.index if self.dev.type == 'cuda' and self.dev.index is not None else 0
        self.f64 = f64
        self.tdt = torch.float64 if f64 else torch.float32
        self.work = None

    def place(self, a):
        if not hac._is_tensor(a):
            a = self.torch.from_numpy(a if a.flags.writeable else a.copy())
        return a.to(device=self.dev, dtype=self.tdt)

    def empty(self, shape, dtype=None):
        return self.torch.empty(shape, dtype=dtype or self.tdt, device=self.dev)

    def workspace(self, **sizes):
        need = _native.motion_work_bytes(**sizes)
        if self.work is None or self.work.numel() < need:
            self.work = self.torch.empty(max(16, need), dtype=self.torch.uint8, device=self.dev)
        return self.work.data_ptr(), need


def _is_f64(a):
    return str(a.dtype).endswith('float64')


def _angles_on(dv, stacked, offsets, pairs, vel_delay, vel_padding, bounds, vel_bounds):
    rec = dv.place(stacked).contiguous()
    T, M, cols = int(rec.shape[0]), int(rec.shape[1]), 3 * len(pairs)
    angles, vels = dv.empty((T, cols)), dv.empty((T, cols))
    work, need = dv.workspace(T=T, E=offsets.size - 1)
    _native.motion_angles_device(rec.data_ptr(), T, M, pairs, offsets, int(vel_delay), _native.MOTION_PADDINGS[vel_padding], bounds,
                                 vel_bounds, work, need, angles.data_ptr(), cols, vels.data_ptr(), cols, f64=dv.f64,
                                 device=dv.ordinal)
    return angles, vels


def angle_arrays(records, markers, vel_delay=1, vel_padding='zeros', bounds=None, vel_bounds=None, device=None, output='numpy'):
    """(angles [T, 30], vels [T, 30], offsets int64 [E + 1]) of the examples' frames stacked: `db_to_angles_and_vels` and
    `filter_values` (features/angle_histograms.py:45-94, 192-198) on the GPU, two launches (three with `bounds`).

    records, markers: see `check_records`.  The velocities never reach across an example; `vel_delay` above an example's length is
    that length (the reference's rule), below 1 a ValueError.  The reference's `db_to_VQ_hist_matrix` ignores its `vel_delay` and
    `vel_padding` and uses 1 and 'zeros' (:192); here they are honoured and those are the defaults.  Velocities and clips equal
    the twin's bit for bit given equal angles; the angles differ from it by the device's atan2 and sqrt.
    output: 'numpy' or 'device' (tensors; the offsets stay a host array)."""
    _check_output(output)
    stacked, offsets, pairs = check_records(records, markers, vel_delay, vel_padding, bounds, vel_bounds)
    dv = _Device(device, _is_f64(stacked))
    angles, vels = _angles_on(dv, stacked, offsets, pairs, vel_delay, vel_padding, bounds, vel_bounds)
    if output == 'device':
        return angles, vels, offsets
    return angles.cpu().numpy(), vels.cpu().numpy(), offsets


def _whiten_on(dv, x):
    """x [T, C] (contiguous device tensor) whitened in place; (mean, std) fp64 device tensors."""
    T, C = int(x.shape[0]), int(x.shape[1])
    moments = dv.empty((2, C), dv.torch.float64)
    work, need = dv.workspace(T=T, C=C)
    _native.motion_whiten_device(x.data_ptr(), C, T, C, work, need, x.data_ptr(), C, moments[0].data_ptr(), moments[1].data_ptr(),
                                 f64=dv.f64, device=dv.ordinal)
    return moments[0], moments[1]


def whiten(x, device=None, output='numpy'):
    """(x / std, mean, std) per column: scipy's `whiten` (features/angle_histograms.py:209) on the GPU, bit for bit `host_whiten`.
    scipy's warning on a zero deviation is raised here too (it needs the C deviations on the host)."""
    _check_output(output)
    x = x if _is_float_tensor(x) and x.dim() == 2 else _host_float(x, "x", 2)
    if x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("x: a matrix [T >= 1, C >= 1] expected")
    dv = _Device(device, _is_f64(x))
    out = dv.place(x).clone().contiguous()
    mean, std = _whiten_on(dv, out)
    h_std = std.cpu().numpy()
    # a deviation of exactly 1 that came from 0: the column is constant
    if np.any(h_std == 1.0) and bool(((out == out[:1]).all(dim=0).cpu().numpy() & (h_std == 1.0)).any()):
        warnings.warn("Some columns have standard deviation zero. The values of these columns will not change.", RuntimeWarning,
                      stacklevel=2)
    if output == 'device':
        return out, mean, std
    return out.cpu().numpy(), mean.cpu().numpy(), h_std


class _Runs(object):
    """The state of P problems after klnmf_motion_kmeans_device: device tensors."""

    def __init__(self, dv, pts, set_stride, ld, T, d, D, set_of, init, thresh, max_iter, labels=False):
        torch = dv.torch
        P, K = int(init.shape[0]), int(init.shape[1])
        self.codebooks = init.contiguous()
        self.alive = dv.empty((P, K), torch.int32)
        self.distortion = dv.empty((P,), torch.float64)
        self.iters = dv.empty((P,), torch.int32)
        self.labels = dv.empty((P, T), torch.int32) if labels else None
        work, need = dv.workspace(T=T, d=d, K=K, P=P, D=D)
        open_ = _native.motion_kmeans_device(pts.data_ptr(), set_stride, ld, T, d, D, set_of, self.codebooks.data_ptr(), K, thresh,
                                             max_iter, work, need, self.alive.data_ptr(), self.distortion.data_ptr(),
                                             self.iters.data_ptr(), self.labels.data_ptr() if labels else 0, f64=dv.f64,
                                             device=dv.ordinal)
        if open_ >= 0:
            raise RuntimeError("k-means problem %d (point set %d) has not stopped after max_iter = %d iterations"
                               % (open_, int(set_of[open_]), max_iter))


def _restarts_on(dv, pts, view, set_stride, ld, T, d, D, k, iter, thresh, rng, max_iter, labels=False):
    """All D * iter problems from drawn rows.  view: pts as [T, D, d] or [D, T, d] strided tensor indexable as view[s] -> [T, d]."""
    rows = draw_rows(_rng(rng), T, k, iter, D)
    idx = dv.torch.from_numpy(rows).to(dv.dev)
    init = dv.torch.stack([view(s)[idx[s]] for s in range(D)]).reshape(D * iter, k, d)
    set_of = np.repeat(np.arange(D, dtype=np.int32), iter)
    return _Runs(dv, pts, set_stride, ld, T, d, D, set_of, init, float(thresh), int(max_iter), labels)


def _best(runs, D, iter):
    """(best restart per set int64 [D], distortions [D, iter], alive [D, iter, K]) on the host: 2 P small numbers."""
    dist = runs.distortion.cpu().numpy().reshape(D, iter)
    alive = runs.alive.cpu().numpy().reshape(D, iter, -1) != 0
    return np.argmin(dist, axis=1), dist, alive


def kmeans_converged_many(point_sets, k, iter=20, thresh=1e-5, rng=None, max_iter=1000, device=None, output='numpy',
                          return_all=False):
    """[(codebook, distortion)] per point set of [D, T, d]: scipy's `kmeans(points, k, iter, thresh)` for every set
    (features/angle_histograms.py:212), all D * iter restarts as one batch -- two launches per Lloyd iteration for all of them,
    the stop flags polled every 4 iterations -- bit for bit `host_kmeans_converged_many`.

    rng: a numpy Generator or RandomState (its `choice(T, size=k, replace=False)` is scipy's draw, set after set, restart after
    restart), or a seed for `numpy.random.default_rng`.  The lowest distortion of a set wins, the first among equals.  A cluster
    without members is dropped: a codebook may have fewer than k rows.  RuntimeError names the first problem that has not
    stopped after `max_iter` iterations, a guard scipy does not have.  `return_all`: also the `_Runs` of the batch."""
    _check_output(output)
    point_sets, k, iter = _check_many(point_sets, k, iter, thresh, max_iter)
    D, T, d = (int(n) for n in point_sets.shape)
    dv = _Device(device, _is_f64(point_sets))
    pts = dv.place(point_sets).contiguous()
    runs = _restarts_on(dv, pts, lambda s: pts[s], T * d, d, T, d, D, k, iter, thresh, rng, max_iter, labels=return_all)
    best, dist, alive = _best(runs, D, iter)
    out = []
    for s, b in enumerate(best):
        cb = runs.codebooks[s * iter + b][dv.torch.from_numpy(alive[s, b]).to(dv.dev)]
        out.append((cb if output == 'device' else cb.cpu().numpy(), float(dist[s, b])))
    return (out, runs) if return_all else out


def kmeans_converged(data, k_or_guess, iter=20, thresh=1e-5, rng=None, max_iter=1000, device=None, output='numpy'):
    """(codebook, distortion): scipy's `kmeans(data, k_or_guess, iter, thresh)` on the GPU, bit for bit `host_kmeans_converged`.
    An int k: `iter` restarts from drawn rows (`kmeans_converged_many`); a matrix: one run from it."""
    _check_output(output)
    if np.ndim(k_or_guess) != 2:
        sets = data.unsqueeze(0) if hac._is_tensor(data) and data.dim() == 2 else np.asarray(data)[np.newaxis]
        return kmeans_converged_many(sets, k_or_guess, iter, thresh, rng, max_iter, device, output)[0]
    data = data if _is_float_tensor(data) and data.dim() == 2 else _host_float(data, "data", 2)
    guess = k_or_guess if _is_float_tensor(k_or_guess) else _host_float(k_or_guess, "k_or_guess", 2)
    T, d, K = int(data.shape[0]), int(data.shape[1]), int(guess.shape[0])
    if int(guess.shape[1]) != d or K < 1:
        raise ValueError("data of shape %s against a guess of shape %s" % ((T, d), tuple(guess.shape)))
    _check_sizes(1, T, d, K, 1, thresh, max_iter)
    dv = _Device(device, _is_f64(data) or _is_f64(guess))
    pts = dv.place(data).contiguous()
    runs = _Runs(dv, pts, 0, d, T, d, 1, np.zeros(1, dtype=np.int32), dv.place(guess).clone().reshape(1, K, d), float(thresh),
                 int(max_iter))
    cb = runs.codebooks[0][runs.alive[0] != 0]
    return (cb if output == 'device' else cb.cpu().numpy()), float(runs.distortion.cpu().numpy()[0])


def _hist_on(dv, pts, set_stride, ld, T, d, D, cbs, offsets, soft_vq):
    K, E = int(cbs.shape[1]), offsets.size - 1
    out = dv.empty((E, D * K))
    work, need = dv.workspace(T=T, d=d, K=K, D=D, E=E)
    _native.motion_hist_device(pts.data_ptr(), set_stride, ld, T, d, D, cbs.data_ptr(), K, offsets, 0 if soft_vq is None else 1,
                               0.0 if soft_vq is None else float(soft_vq), work, need, out.data_ptr(), D * K, f64=dv.f64,
                               device=dv.ordinal)
    return out


def histograms(point_sets, codebooks, offsets, soft_vq=None, device=None, output='numpy'):
    """[E, D K]: the examples' row-normalised histograms of point sets [D, T, d] against codebooks [D, K, d] -- `get_histos` and
    the sums per example (features/angle_histograms.py:214-222) on the GPU.  soft_vq None: hard, bit for bit `host_histograms`;
    a number: lib/vector_quantization.py's `soft_associate` with that alpha."""
    _check_output(output)
    point_sets = point_sets if _is_float_tensor(point_sets) else _host_float(point_sets, "point_sets", 3)
    codebooks = codebooks if _is_float_tensor(codebooks) else _host_float(codebooks, "codebooks", 3)
    if len(point_sets.shape) != 3 or len(codebooks.shape) != 3 or point_sets.shape[0] != codebooks.shape[0] \
            or point_sets.shape[2] != codebooks.shape[2]:
        raise ValueError("point sets [D, T, d] against codebooks [D, K, d] expected, got %s and %s"
                         % (tuple(point_sets.shape), tuple(codebooks.shape)))
    D, T, d = (int(n) for n in point_sets.shape)
    _check_sizes(D, T, d, int(codebooks.shape[1]), 0, 0.0, 1)
    if soft_vq is not None and not np.isfinite(float(soft_vq)):
        raise ValueError("soft_vq: None or a finite number expected")
    offsets = _check_offsets(offsets, T)
    dv = _Device(device, _is_f64(point_sets) or _is_f64(codebooks))
    out = _hist_on(dv, dv.place(point_sets).contiguous(), T * d, d, T, d, D, dv.place(codebooks).contiguous(), offsets, soft_vq)
    return out if output == 'device' else out.cpu().numpy()


def _from_angles_on(dv, angles, vels, offsets, nb_bins, soft_vq, iter, thresh, rng, max_iter, output, return_codebooks):
    torch = dv.torch
    T, D = int(angles.shape[0]), int(angles.shape[1])
    pts = torch.stack([dv.place(angles), dv.place(vels)], dim=2).reshape(T, 2 * D).contiguous()
    _whiten_on(dv, pts)
    by_set = pts.view(T, D, 2)
    runs = _restarts_on(dv, pts, lambda s: by_set[:, s], 2, 2 * D, T, 2, D, nb_bins, iter, thresh, rng, max_iter)
    best, _, alive = _best(runs, D, iter)
    for s, b in enumerate(best):
        lost = int((~alive[s, b]).sum())
        if lost:
            raise ValueError("degree of freedom %d: the best codebook lost %d of its %d clusters; the histogram matrix needs "
                             "nb_bins rows of every codebook" % (s, lost, nb_bins))
    pick = torch.from_numpy(np.arange(D) * iter + best).to(dv.dev)
    cbs = runs.codebooks[pick].contiguous()
    X = _hist_on(dv, pts, 2, 2 * D, T, 2, D, cbs, offsets, soft_vq)
    if output != 'device':
        X, cbs = X.cpu().numpy(), cbs.cpu().numpy()
    return (X, cbs) if return_codebooks else X


def _check_matrix_args(nb_bins, soft_vq, iter, thresh, max_iter, T, D, output):
    _check_output(output)
    if int(nb_bins) != nb_bins or int(iter) != iter or int(iter) < 1 or int(nb_bins) < 1:
        raise ValueError("nb_bins and iter: integers >= 1 expected, got %r and %r" % (nb_bins, iter))
    _check_sizes(D, T, 2, int(nb_bins), D * int(iter), thresh, max_iter)
    if int(nb_bins) > T:
        raise ValueError("nb_bins = %d rows cannot be drawn from T = %d frames without replacement" % (nb_bins, T))
    if soft_vq is not None and not np.isfinite(float(soft_vq)):
        raise ValueError("soft_vq: None or a finite number expected")


def vq_hist_matrix_from_angles(angles, vels, offsets, nb_bins=16, soft_vq=None, iter=20, thresh=1e-5, rng=None, max_iter=1000,
                               device=None, output='numpy', return_codebooks=False):
    """`vq_hist_matrix` for callers who hold the angles and velocities [T, D] (host arrays or device tensors) and the offsets."""
    angles, vels, offsets = check_angles(angles, vels, offsets)
    T, D = int(angles.shape[0]), int(angles.shape[1])
    _check_matrix_args(nb_bins, soft_vq, iter, thresh, max_iter, T, D, output)
    dv = _Device(device, _is_f64(angles))
    return _from_angles_on(dv, angles, vels, offsets, int(nb_bins), soft_vq, int(iter), thresh, rng, int(max_iter), output,
                           return_codebooks)


def vq_hist_matrix(records, markers, vel_delay=1, vel_padding='zeros', nb_bins=16, bounds=None, vel_bounds=None, soft_vq=None,
                   iter=20, thresh=1e-5, rng=None, max_iter=1000, device=None, output='numpy', return_codebooks=False):
    """The [examples, 30 nb_bins] matrix of `db_to_VQ_hist_matrix` (features/angle_histograms.py:171-223) on the GPU: angles and
    velocities, whitening per degree of freedom, `kmeans(points, nb_bins, iter)` per degree of freedom with all restarts of all
    degrees in one batch, hard (`soft_vq=None`) or soft histograms per example, rows normalised.  Between the stages only the
    drawn row indices (up), and the stop flags, the restarts' distortions and live-row masks (down) cross the bus.

    records, markers: see `check_records`; `vel_delay`, `vel_padding`: honoured (the reference ignores them, see `angle_arrays`);
    rng, max_iter: see `kmeans_converged_many`.  ValueError before the histogram launch where the best codebook of a degree of
    freedom lost a cluster (the reference's reshape fails there too).  output: 'numpy', or 'device': a tensor usable wherever
    the package takes device operands.  `return_codebooks`: also the codebooks [30, nb_bins, 2]."""
    stacked, offsets, pairs = check_records(records, markers, vel_delay, vel_padding, bounds, vel_bounds)
    T, D = int(stacked.shape[0]), 3 * len(pairs)
    _check_matrix_args(nb_bins, soft_vq, iter, thresh, max_iter, T, D, output)
    dv = _Device(device, _is_f64(stacked))
    angles, vels = _angles_on(dv, stacked, offsets, pairs, vel_delay, vel_padding, bounds, vel_bounds)
    return _from_angles_on(dv, angles, vels, offsets, int(nb_bins), soft_vq, int(iter), thresh, rng, int(max_iter), output,
                           return_codebooks)
