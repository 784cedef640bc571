"""Cases and references of the motion modality (tests/test_motion_cpu.py, tests/test_motion_gpu.py).  numpy only.

The reference throughout is the host twin of multimodal_amd/features/angle_histograms.py, which test_motion_cpu.py pins to the
REFERENCE's recorded outputs in tests/golden/g23_motion.npz (tests/golden/make_golden_motion.py).  `same_bits` asks for equal
shapes, types and bit patterns.

The derived bars (none comes from what the code under test gives):

* ANGLE_BAR, device against twin.  Both form the rotation matrix with the same IEEE operations (contraction off, sqrt and
  division correctly rounded), so the arguments of atan2 are equal bit for bit and only atan2 itself differs: at most 2 ulp of
  the result for the device's (HIP's published accuracy of the fp64 function) and 1 ulp for the host's libm, the result at most
  pi in magnitude: 3 ulp(pi), taken as 4 ulp(pi) = 1.78e-15 absolute ("a few ulp of pi").  float32 storage: equal after the
  rounding, or one float32 ulp apart where the fp64 values straddle a rounding boundary.
* `angle_bar_reference`, twin against the reference.  The reference forms dot(q, q) with numpy.dot, whose order of additions is
  the BLAS's: the scale sqrt(2 / nq) and with it every matrix entry (sums of at most three terms of magnitude at most 2) carry up
  to 12 roundings that differ, 24 * 2^-53 absolute on either argument; atan2(y, x) moves by at most (|dy| + |dx|) / hypot(y, x),
  and hypot is cy = cos(ay) for ax and az and 1 for ay.  So 24 * 2^-53 / cos(ay) + 2 ulp(pi).
* `sum_bar`: a sum of n terms of one sign formed in two different orders differs by at most (n + 4) * 2^-53 relative; the
  issue's form for the moments is (4096 + groups + 4) * 2^-53 and for a soft histogram entry (frames + K + 8) * 2^-52.
"""
import functools
import os

import numpy as np

from multimodal_amd.features import angle_histograms as ah

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g23_motion.npz')
TILE, GROUP = 256, 4096
ULP_PI = float(np.spacing(np.pi))
ANGLE_BAR = 4 * ULP_PI
NAMES = ['spare', 'torso', 'left_shoulder', 'left_elbow', 'left_hand', 'left_hip', 'left_knee', 'left_foot', 'right_shoulder',
         'right_elbow', 'right_hand', 'right_hip', 'right_knee', 'right_foot']


@functools.lru_cache(maxsize=None)
def golden():
    g = dict(np.load(GOLDEN))
    for a in g.values():
        a.setflags(write=False)
    return g


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    assert got.tobytes() == want.tobytes(), 'bits differ at %d of %d places' % ((got != want).sum(), got.size)
    return True


def angle_bar_reference(angles):
    """[T, 3 n] absolute bars of the twin's angles against the reference's (the module's text)."""
    cy = np.cos(angles[:, 1::3])
    bar = np.empty_like(angles)
    bar[:, 0::3] = bar[:, 2::3] = 24 * 2.0 ** -53 / cy + 2 * ULP_PI
    bar[:, 1::3] = 24 * 2.0 ** -53 + 2 * ULP_PI
    return bar


def moments_bar(T):
    return (GROUP + -(-T // GROUP) + 4) * 2.0 ** -53


def soft_bar(frames, K):
    """Relative bar per entry of the soft matrix for an example of `frames` frames."""
    return (np.asarray(frames, dtype=np.float64) + K + 8) * 2.0 ** -52


def offsets_for(T):
    """Offsets over T frames: one-frame examples, examples across the tile (256) and group (4096) boundaries, an example longer than
    a group where T allows."""
    cuts = {0, 1, 2, min(T, 200), min(T, 300), min(T, 301), T}
    if T > GROUP:
        cuts |= {GROUP - 3}
    if T > 2 * GROUP:
        cuts |= {2 * GROUP + 5, T - 1}
    else:
        cuts |= {max(0, T - 1)}
    return np.array(sorted(cuts), dtype=np.int64)


@functools.lru_cache(maxsize=None)
def records(seed, T, f32=False, markers=len(NAMES)):
    """[T, markers, 7]: smooth quaternion paths away from the branch thresholds (|q| around 1, no gimbal lock in reach)."""
    rng = np.random.default_rng(seed)
    r = rng.normal(size=(1, markers, 7)) + np.cumsum(0.05 * rng.normal(size=(T, markers, 7)), axis=0)
    r = r.astype(np.float32 if f32 else np.float64)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def clouds(seed, D, T, d, K, f32=False):
    """(point sets [D, T, d], init [D, K, d]): normals around K centres per set, the spread growing with the set so that the
    problems need different numbers of iterations."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(D, K, d)) * 3.0
    pts = np.stack([centres[s][rng.integers(0, K, T)] + (0.3 + 0.5 * s) * rng.normal(size=(T, d)) for s in range(D)])
    pts = pts.astype(np.float32 if f32 else np.float64)
    init = np.stack([pts[s][rng.choice(T, size=K, replace=False)] for s in range(D)])
    pts.setflags(write=False)
    init.setflags(write=False)
    return pts, init


@functools.lru_cache(maxsize=None)
def twin_run(seed, D, T, d, K, f32, s, far=False):
    """`host_kmeans_converged_from` on set s of `clouds` from its init (`far`: row 1 moved where no point is nearest)."""
    pts, init = clouds(seed, D, T, d, K, f32)
    out = ah.host_kmeans_converged_from(pts[s], far_init(init[s]) if far else init[s], 1e-5)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def far_init(init):
    init = np.array(init)
    init[min(1, init.shape[0] - 1)] = 1e3
    return init
