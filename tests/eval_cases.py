"""The evaluation kernels' references, bars and cases (tests/test_eval_cpu.py, tests/test_eval_gpu.py).  numpy only.

References.  `measure` restates the five measures of multimodal_amd/lib/metrics.py (reference metrics.py:58-86) and
`generalized_kl` the loss of metrics.py:18-20 in extended precision (np.longdouble; `ld()` asserts that its epsilon is below
2^-60 and fails -- does not skip -- where it is not).  Each returns the value AND the magnitude M its bar is relative to:
  KL, reverse KL, generalized_KL   M = sum(|x l| + x + y), l = log((x + eps) / (y + eps)) (x and y swapped for the reverse)
  symmetric KL                     the mean of the two
  Frobenius, cosine                |value| (sums of nonnegative terms; the cosine's three sums too)

Bars (u = 2^-53), derived from the kernels' order of operations, not measured:
  k_all_distances, fp64   (ceil(d / 64) + 16) u M.  A lane adds its ceil(d / 64) terms in sequence, each add rounding by at
      most u of the partial sum (<= the lane's share of M); wave_sum adds 6 levels, each u of M at most; 10 u cover one
      term: the two adds and the division forming the ratio (1.5 u absolute on l, times x <= M), a log accurate to about
      1 ulp, the product and the two adds of x l - x + y -- and for the other measures the product, the square root, the
      division and the final halving, all below that.
  k_all_distances, fp32   the kernel widens its fp32 operands, computes as above and rounds ONCE: the same bar against the
      reference on the fp32-rounded inputs, plus 2^-24 |reference| for the cast.
  k_gkl (klnmf_generalized_kl)   (grid + ceil(count / (256 grid)) + 24) u M with grid = min(1024, ceil(count / 256)): a thread adds
      ceil(count / (256 grid)) terms in sequence, block_sum is 6 tree levels and 4 wave sums, the host adds the `grid` partials
      in sequence, 10 u for a term as above.  fp32 operands are widened and nothing is cast: the same bar on rounded inputs.
`kernel_order_*` evaluate in plain fp64 numpy in the kernels' own order (64 strided lanes then the tree; grid x 256 strided
threads, the block sum, the host's sequential sum): tests/test_eval_cpu.py holds them within a quarter of every bar.

Cases.  `pair_case(na, nb, d)`: nonnegative rows with fixed roles (below), so that a shape of enough rows holds a zero row on
each side, rows with about 30 % zeros on each side (0 log 0 on either operand), a row of A equal to a row of B and a row
scaled by 1e-6; `PairCase` records where they are.  `gkl_case(count, eps)`: x with about 30 % zeros for eps > 0, strictly
positive operands for eps = 0.
"""
import functools
import math

import numpy as np

U = 2.0 ** -53
EPS = 1e-8                       # kEpsRatio: the eps of the five measures (metrics.py ignores the caller's)
KL, REV_KL, SYM_KL, FROBENIUS, COSINE_DIFF = 0, 1, 2, 3, 4       # _native.DIST_*
METRICS = ((KL, 'kl_div'), (REV_KL, 'rev_kl_div'), (SYM_KL, 'sym_kl_div'), (FROBENIUS, 'frobenius'), (COSINE_DIFF, 'cosine_diff'))

DIMS = (0, 1, 63, 64, 65, 127, 128, 129, 1000)
SHAPES = ((1, 1), (1, 3), (3, 1), (5, 3), (4, 4), (7, 9), (33, 17))
GKL_COUNTS = (0, 1, 255, 256, 257, 262144, 262145, 600001)
GKL_EPS = (1e-8, 1e-3, 0.0)
GKL_GRID_CAP, GKL_THREADS = 1024, 256


def ld():
    """np.longdouble, where it is an extended format."""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, 'np.longdouble is no extended-precision format here'
    return np.longdouble


def as_f32(a):
    """What a kernel on fp32 operands sees of an fp64 input, widened back."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _ceil(a, b):
    return -(-int(a) // int(b))


# ---- references ---------------------------------------------------------------------------------------------------------------
def _gkl_terms(x, y, eps):
    """(terms of generalized_KL(x, y), terms of its magnitude) in extended precision."""
    L = ld()
    x, y, eps = np.asarray(x, dtype=L), np.asarray(y, dtype=L), L(eps)
    with np.errstate(divide='ignore', invalid='ignore'):
        l = np.log((x + eps) / (y + eps))
        xl = x * l
    return xl - x + y, np.abs(xl) + x + y


def measure(a, b, metric):
    """(value, M) of measure `metric` of a against b over the last axis (operands broadcast), extended precision."""
    L = ld()
    a, b = np.asarray(a, dtype=L), np.asarray(b, dtype=L)
    if metric in (KL, REV_KL, SYM_KL):
        t0, m0 = _gkl_terms(a, b, EPS)
        t1, m1 = _gkl_terms(b, a, EPS)
        v0, v1, m0, m1 = t0.sum(axis=-1), t1.sum(axis=-1), m0.sum(axis=-1), m1.sum(axis=-1)
        if metric == KL:
            return v0, m0
        if metric == REV_KL:
            return v1, m1
        return L(0.5) * (v0 + v1), L(0.5) * (m0 + m1)
    if metric == FROBENIUS:
        v = np.sqrt(np.square(a - b).sum(axis=-1))
        return v, v
    if metric == COSINE_DIFF:
        ab = (a * b).sum(axis=-1)
        v = -(ab / (np.sqrt(np.square(a).sum(axis=-1) * np.square(b).sum(axis=-1)) + (ab == 0)))
        return v, np.abs(v)
    raise ValueError(metric)


def all_pairs(A, B, metric):
    """(value, M), each [len(A), len(B)]: the pattern of evaluation.py:103-106."""
    A, B = np.asarray(A), np.asarray(B)
    return measure(A[:, None, :], B[None, :, :], metric)


def generalized_kl(x, y, eps, axis=None):
    """(value, M) of sum(x log((x + eps) / (y + eps)) - x + y) over `axis`, extended precision."""
    t, m = _gkl_terms(x, y, eps)
    return t.sum(axis=axis), m.sum(axis=axis)


# ---- bars -----------------------------------------------------------------------------------------------------------------------
def distance_bar(d, M, ref=None, f32=False):
    """The bar of k_all_distances on vectors of length d (module docstring); f32: with the final cast of `ref`."""
    bar = (_ceil(d, 64) + 16) * U * np.asarray(M, dtype=np.float64)
    if f32:
        bar = bar + 2.0 ** -24 * np.abs(np.asarray(ref, dtype=np.float64))
    return bar


def gkl_grid(count):
    return min(GKL_GRID_CAP, _ceil(count, GKL_THREADS))


def gkl_bar(count, M):
    grid = gkl_grid(count)
    per_thread = _ceil(count, GKL_THREADS * grid) if grid else 0
    return (grid + per_thread + 24) * U * np.asarray(M, dtype=np.float64)


# ---- the kernels' order in plain fp64 -------------------------------------------------------------------------------------------
def _tree64(v):
    """wave_sum over the last axis of 64: lane 0's value."""
    v = np.array(v, dtype=np.float64)
    for o in (32, 16, 8, 4, 2, 1):
        v[..., :o] = v[..., :o] + v[..., o:2 * o]
    return v[..., 0]


def _strided_lanes(terms, lanes):
    """Lane j adds terms j, j + lanes, ... in sequence (zero-padded: x + 0.0 is x)."""
    d = terms.shape[-1]
    trips = max(1, _ceil(d, lanes))
    pad = np.zeros(terms.shape[:-1] + (trips * lanes,), dtype=np.float64)
    pad[..., :d] = terms
    pad = pad.reshape(terms.shape[:-1] + (trips, lanes))
    s = np.zeros(terms.shape[:-1] + (lanes,), dtype=np.float64)
    for t in range(trips):
        s = s + pad[..., t, :]
    return s


def kernel_order_distances(A, B, metric):
    """k_all_distances in fp64 numpy: the same terms, 64 strided lanes, the tree, the same closing expression."""
    a = np.asarray(A, dtype=np.float64)[:, None, :]
    b = np.asarray(B, dtype=np.float64)[None, :, :]
    a, b = np.broadcast_arrays(a, b)
    wave = lambda t: _tree64(_strided_lanes(t, 64))
    with np.errstate(divide='ignore', invalid='ignore'):
        if metric <= SYM_KL:
            l = np.log((a + EPS) / (b + EPS))
            s0, s1 = wave(a * l - a + b), wave(-b * l - b + a)
            return s0 if metric == KL else s1 if metric == REV_KL else 0.5 * (s0 + s1)
        if metric == FROBENIUS:
            return np.sqrt(wave((a - b) * (a - b)))
        s0, s1, s2 = wave(a * b), wave(a * a), wave(b * b)
        return -(s0 / (np.sqrt(s1 * s2) + (s0 == 0.0)))


def kernel_order_gkl(x, y, eps):
    """klnmf_generalized_kl in fp64 numpy: grid x 256 strided threads, block_sum (tree per wave, the waves in sequence), the host's
    sequential sum of the partials."""
    x, y = np.asarray(x, dtype=np.float64).ravel(), np.asarray(y, dtype=np.float64).ravel()
    grid = max(1, gkl_grid(x.size))
    with np.errstate(divide='ignore', invalid='ignore'):
        terms = x * np.log((x + eps) / (y + eps)) - x + y
    threads = _strided_lanes(terms, grid * GKL_THREADS).reshape(grid, GKL_THREADS // 64, 64)
    waves = _tree64(threads)
    total = 0.0
    for g in range(grid):
        t = 0.0
        for w in range(GKL_THREADS // 64):
            t += waves[g, w]
        total += t
    return total


# ---- cases ----------------------------------------------------------------------------------------------------------------------
# the role of row i of A and of row j of B, by i % 5 and j % 5
A_ROLES = ('sparse', 'zero', 'copy', 'scaled', 'dense')
B_ROLES = ('sparse', 'dense', 'zero', 'scaled', 'sparse')


class PairCase(object):
    """A [na, d] and B [nb, d] in fp64 and where their special rows are."""

    def __init__(self, A, B, zero_a, zero_b, same, sparse_a, sparse_b, scaled):
        self.A, self.B = A, B
        self.zero_a, self.zero_b = zero_a, zero_b        # indices of all-zero rows
        self.same = same                                 # (i, j): A[i] is B[j]
        self.sparse_a, self.sparse_b = sparse_a, sparse_b  # rows drawn with about 30 % zeros
        self.scaled = scaled                             # ('a' | 'b', index): rows scaled by 1e-6
        self.na, self.nb, self.d = A.shape[0], B.shape[0], A.shape[1]


def _row(rng, d, role):
    v = rng.random(d) + 0.05
    if role == 'sparse':
        v = v * (rng.random(d) >= 0.3)
    elif role == 'zero':
        v = np.zeros(d)
    elif role == 'scaled':
        v = v * 1e-6
    return v


@functools.lru_cache(maxsize=None)
def pair_case(na, nb, d):
    rng = np.random.default_rng(1000003 * d + 1009 * na + nb)
    B = np.array([_row(rng, d, B_ROLES[j % 5]) for j in range(nb)]).reshape(nb, d)
    A = np.array([_row(rng, d, A_ROLES[i % 5]) for i in range(na)]).reshape(na, d)
    same = []
    for i in range(na):
        if A_ROLES[i % 5] == 'copy':
            j = (i // 5) % nb
            A[i] = B[j]
            same.append((i, j))
    A.setflags(write=False)
    B.setflags(write=False)
    return PairCase(A, B,
                    zero_a=[i for i in range(na) if A_ROLES[i % 5] == 'zero'], zero_b=[j for j in range(nb) if B_ROLES[j % 5] == 'zero'],
                    same=same, sparse_a=[i for i in range(na) if A_ROLES[i % 5] == 'sparse'],
                    sparse_b=[j for j in range(nb) if B_ROLES[j % 5] == 'sparse'],
                    scaled=[('a', i) for i in range(na) if A_ROLES[i % 5] == 'scaled'] + [('b', j) for j in range(nb) if B_ROLES[j % 5] == 'scaled'])


def case_inputs(case, f32):
    """(A, B) as the kernels of the type see them, in fp64."""
    return (as_f32(case.A), as_f32(case.B)) if f32 else (case.A, case.B)


@functools.lru_cache(maxsize=None)
def pair_reference(na, nb, d, metric, f32):
    """(value, M) of the case in extended precision, read-only and shared."""
    v, m = all_pairs(*case_inputs(pair_case(na, nb, d), f32), metric=metric)
    v.setflags(write=False)
    m.setflags(write=False)
    return v, m


def paired_rows(n, d, seed):
    """(a, b), [n, d] each, for the row-paired form of the metrics wrappers: row 1 of a is zero, row 2 of b is row 2 of a."""
    rng = np.random.default_rng(seed)
    a = (rng.random((n, d)) + 0.05) * (rng.random((n, d)) >= 0.3)
    b = rng.random((n, d)) + 0.05
    if n > 2:
        a[1] = 0.0
        b[2] = a[2]
    return a, b


@functools.lru_cache(maxsize=None)
def gkl_case(count, eps):
    """(x, y) of `count` elements: x with about 30 % zeros where eps > 0, both strictly positive where eps = 0."""
    rng = np.random.default_rng(77 + count)
    x = rng.gamma(1.0, 1.0, count) + 0.05
    y = rng.gamma(1.0, 1.0, count) + 0.05
    if eps > 0:
        x = x * (rng.random(count) >= 0.3)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def gkl_reference(count, eps, f32):
    x, y = gkl_case(count, eps)
    if f32:
        x, y = as_f32(x), as_f32(y)
    return generalized_kl(x, y, eps)


def within(got, ref, bar):
    """(every |got - ref| <= bar, the worst |got - ref| / bar with 0 / 0 = 0) in extended precision; a non-finite `got` fails."""
    L = ld()
    got = np.asarray(got)
    err = np.abs(np.asarray(got, dtype=L) - np.asarray(ref, dtype=L))
    bar = np.asarray(bar, dtype=L) + np.zeros_like(err)
    if not np.all(np.isfinite(got)):
        return False, float('inf')
    ok = bool(np.all(err <= bar))
    pos = bar > 0
    worst = float(np.max(err[pos] / bar[pos])) if np.any(pos) else 0.0
    if np.any(err[~pos] > 0):
        worst = float('inf')
    return ok, worst


def units(got, ref, M):
    """The worst |got - ref| in units of 2^-53 M (0 where M = 0 and the two agree)."""
    return within(got, ref, U * np.asarray(M, dtype=np.float64))[1]
