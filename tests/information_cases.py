"""What the information-matrix tests share: an fp64 restatement of the analysis in numpy -- np.histogram per (atom, label), then the
reference's table formula (samples/plot_info_matrix.py:66-90 on lib/metrics.py:37-43) -- the bin rule of the kernels restated on
the host, and the input builders.

Nothing here calls the code under test.  `reference_counts` / `reference_information` are the yardstick of the GPU tests: the
counts are np.histogram's own integers on the values widened to float64 over each atom's own (min, max), and the information is the
reference's expression on the 2 x B table of probabilities."""
import numpy as np

R = 1024            # rows of a workgroup's chunk (csrc/information.hip.h kInfoRows; _native.INFORMATION_ROWS)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def table_information(histo):
    """The mutual information of a joint table of probabilities, an empty cell contributing 0: metrics.mutual_information's
    expression (lib/metrics.py:37-43) restated -- pinned to the reference's outputs by the golden tables G20."""
    histo = np.asarray(histo, dtype=np.float64)
    hole = (histo == 0) * 1
    outer = histo.sum(axis=0)[None, :] * histo.sum(axis=1)[:, None]
    return float((histo * np.log((histo + hole) / (outer + hole))).sum())


def table_entropy(vect):
    vect = np.asarray(vect, dtype=np.float64)
    return float(-np.sum(vect * np.log(vect + (vect == 0))))


def table_conditional_entropy(histo, axis=0):
    histo = np.asarray(histo, dtype=np.float64)
    return table_entropy(histo) - table_entropy(np.moveaxis(histo, axis, -1).reshape(-1, histo.shape[axis]).sum(axis=0))


def reference_counts(A, labels, n_labels, bins):
    """int64 [k, n_labels, bins]: np.histogram of every atom's float64 values per label over the atom's own (min, max)."""
    A = np.asarray(A).astype(np.float64)
    labels = np.asarray(labels)
    by_label = [np.flatnonzero(labels == l) for l in range(n_labels)]
    out = np.zeros((A.shape[1], n_labels, bins), dtype=np.int64)
    for a in range(A.shape[1]):
        v = A[:, a]
        span = (float(v.min()), float(v.max()))
        for l, idx in enumerate(by_label):
            out[a, l] = np.histogram(v[idx], bins=bins, range=span)[0]
    return out


def information_of_counts(counts):
    """(n_labels, k) float64 from counts [k, n_labels, bins]: for (a, l) the table [counts[a, l], the other labels' sum], divided
    by its total (plot_info_matrix.py:88-90), through `table_information`."""
    counts = np.asarray(counts)
    k, n_labels, _bins = counts.shape
    out = np.zeros((n_labels, k))
    for a in range(k):
        total = counts[a].sum(axis=0)
        for l in range(n_labels):
            joint = np.vstack([counts[a, l], total - counts[a, l]])
            out[l, a] = table_information(1. * joint / joint.sum())
    return out


def reference_information(A, labels, n_labels, bins):
    counts = reference_counts(A, labels, n_labels, bins)
    return counts, information_of_counts(counts)


def information_bar(bins):
    """The absolute bar on an information value against the restatement.  The terms p log(p / (pr pc)) of a table have magnitudes
    that sum to at most 2 ln N <= 42 (N <= 2^30); each carries a few ulps of relative error and a 2B-term fp64 sum adds at most
    2B * 2^-53 * 42 (1.5e-13 at B = 16); the restatement's own expression has the same class of error.  1e-12 is about three times
    the sum of both bounds at B = 16; the bound is linear in B, so larger B scale it."""
    return 1e-12 * max(1.0, bins / 16.0)


# ---- the bin rule on the host (what csrc/information.hip.h's info_edge / info_bin compute) ----------------------------------------------
def rule_edges(lo, hi, bins):
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    step = (hi - lo) / bins
    e = np.arange(bins + 1, dtype=np.float64) * step + lo if step != 0 else np.arange(bins + 1, dtype=np.float64) / bins * (hi - lo) + lo
    e[-1] = hi
    return lo, hi, e


def rule_counts(v, bins=10):
    """The counts of the rule 'the b with e_b <= v < e_(b+1), v == hi in the last bin': guess, clamp, correct against the edges."""
    v = np.asarray(v).astype(np.float64)
    lo, hi, e = rule_edges(float(v.min()), float(v.max()), bins)
    with np.errstate(all='ignore'):
        b = np.clip(np.nan_to_num((v - lo) * (bins / (hi - lo))).astype(np.int64), 0, bins - 1)
    for _ in range(bins):
        b -= (b > 0) & (v < e[b])
    for _ in range(bins):
        b += (b < bins - 1) & (v >= e[np.minimum(b + 1, bins)])
    return np.bincount(b, minlength=bins)


def adversarial_vectors(count=3000, seed=0, bins=10):
    """Vectors on which a bin rule goes wrong if it can: uniform and gamma values, mostly-zero vectors with one repeated value,
    values exactly on linspace edges, one ulp either side of every edge, float32 values; n from 1 to 400."""
    rng = np.random.default_rng(seed)
    for t in range(count):
        n = int(rng.integers(1, 400))
        kind = t % 6
        if kind == 0:
            v = rng.random(n)
        elif kind == 1:
            v = rng.gamma(0.3, 2.0, n)
        elif kind == 2:
            v = np.zeros(n)
            v[rng.random(n) < 0.3] = rng.random()
        elif kind == 3:
            lo, hi = sorted(rng.random(2) * 10)
            v = np.concatenate([np.linspace(lo, hi, bins + 1)[rng.integers(0, bins + 1, n)], [lo, hi]])
        elif kind == 4:
            lo, hi = sorted(rng.random(2))
            c = np.linspace(lo, hi, bins + 1)[rng.integers(0, bins + 1, n)]
            v = np.concatenate([np.clip(np.nextafter(c, rng.choice([-np.inf, np.inf], n)), lo, hi), [lo, hi]])
        else:
            v = (rng.random(n) * 7).astype(np.float32)
        yield v


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def coefficients(seed, n, k, bins=10, dtype=np.float64):
    """[n, k] as NMF coefficients look -- gamma-distributed with 60 % exact zeros -- with, where k allows, special atoms from the
    right: a constant atom, an all-zero atom, an atom of exact linspace edges, an atom one ulp either side of those edges (in
    `dtype`, so that float32 inputs sit on float32 neighbours of the edges)."""
    rng = np.random.default_rng(seed)
    A = rng.gamma(0.5, 2.0, (n, k))
    A[rng.random((n, k)) < 0.6] = 0.0
    A = A.astype(dtype)
    if k >= 2:
        A[:, k - 1] = dtype(0.75)
    if k >= 3:
        A[:, k - 2] = 0
    if k >= 5 and n >= 2:
        lo, hi = dtype(0.125), dtype(3.5)
        edges = np.linspace(float(lo), float(hi), bins + 1).astype(dtype)
        pick = rng.integers(0, bins + 1, n)
        on = edges[pick]
        on[0], on[-1] = lo, hi
        A[:, k - 3] = on
        side = rng.choice(np.array([-np.inf, np.inf], dtype=dtype), n)
        near = np.clip(np.nextafter(edges[pick], side), lo, hi)
        near[0], near[-1] = lo, hi
        A[:, k - 4] = near
    return A


def labels_of(seed, n, n_labels, kind='spread'):
    """int32 [n].  'spread': uniformly drawn, label n_labels - 2 carried by no row (where n_labels >= 3); 'one': every row the
    same label."""
    rng = np.random.default_rng(seed + 1000)
    if kind == 'one':
        return np.full(n, n_labels - 1, dtype=np.int32)
    lab = rng.integers(0, n_labels, n).astype(np.int32)
    if n_labels >= 3:
        lab[lab == n_labels - 2] = 0
    return lab
