#!/usr/bin/env python3
"""G22: outputs of the REFERENCE's `multimodal.features.hac.iterative_kmeans` and of scipy's `kmeans2` (what its `build_codebook`
calls) on seeded frame sets.

    python tests/golden/make_golden_kmeans.py <directory of the reference checkout>

Writes tests/golden/g22_kmeans.npz.  The inputs (frames, initial codebooks, seeds) travel with the recorded outputs; nothing of
the reference's source does.  The reference module imports an audio library for its MFCC front end at the top; the functions used
here never call it, so an empty stand-in module takes its place for the import only.

Two sets:  a  600 x 13 frames, K = 12;   b  300 x 3 frames, K = 5.
Frames are drawn as G21's: a codebook row plus 0.35 sigma noise, rounded to multiples of 2^-10.  Per set are recorded
  iterative   `iterative_kmeans(data, K)` of the reference;
  matrix      `kmeans2(data, init, minit='matrix')`, codebook and labels, `init` = K distinct frames;
  raw         `kmeans2(data, K, minit='random', rng=default_rng(seed))`, codebook and labels -- `build_codebook(mode='raw')`
              with its generator pinned.

Conditions, not tolerances; the script asserts each:
  * at every assignment of every iteration of every run the relative gap between the nearest and the second-nearest squared
    distance exceeds 1e-6 -- then scipy's BLAS-form distances and the direct form cannot disagree on a label;
  * the largest count is unique at every split of the iterative builder;
  * no cluster is empty at any assignment of the matrix and raw runs;
  * the numpy twin (multimodal_amd/features/codebook.py) reproduces the recorded outputs: equality, and for the iterative builder
    equality of the codebooks as sets of rows (rows sorted lexicographically: LAPACK's singular-vector sign is not a rule one can
    restate).
On such data every cluster sum is a sum of multiples of 2^-10 and exact in fp64 in any order, and the mean is one division: hence
equality."""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden_hac import direct_labels, draw, stand_in_audio_library     # noqa: E402

SETS = {'a': dict(T=600, d=13, K=12, seed=2201, raw_seed=5), 'b': dict(T=300, d=3, K=5, seed=2202, raw_seed=7)}
GAP = 1e-6


def sorted_rows(c):
    return c[np.lexsort(c.T[::-1])]


def stepped_lloyd(cbk, X, init, n_iter, allow_empty):
    """The twin's Lloyd call one iteration at a time: (codebook, labels, the smallest gap met)."""
    cb, worst, labels = np.array(init), np.inf, None
    for _ in range(n_iter):
        mine, gap = direct_labels(X, cb)
        worst = min(worst, gap)
        assert allow_empty or len(np.unique(mine)) == cb.shape[0], 'an empty cluster'
        cb, labels, _ = cbk.host_lloyd(X, cb, 1)
        assert np.array_equal(labels, mine)
    return cb, labels, worst


def stepped_iterative(cbk, X, K, alpha=0.01):
    """The twin's iterative builder with every assignment's gap and every split's counts looked at."""
    worst = np.inf
    cb = X.mean(axis=0)[np.newaxis, :]
    assert np.array_equal(cb, cbk.host_lloyd(X, np.zeros((1, X.shape[1])), 1)[0])
    while cb.shape[0] < K:
        labels, gap = direct_labels(X, cb)
        worst = min(worst, gap)
        counts = np.bincount(labels, minlength=cb.shape[0])
        assert (counts == counts.max()).sum() == 1, 'a tie for the largest cluster'
        h = int(np.argmax(counts))
        G, _, _ = cbk.host_gram(X, labels, h)
        cb = np.vstack([cb[:h], cb[h + 1:], cbk.split_rows(cb[h], cbk.split_direction(G), alpha, np.float64)])
        cb, _, gap = stepped_lloyd(cbk, X, cb, 10, allow_empty=True)
        worst = min(worst, gap)
    return cb, worst


def main(reference):
    stand_in_audio_library()
    sys.path.insert(0, reference)
    from multimodal.features import hac as rhac
    from scipy.cluster.vq import kmeans2
    from multimodal_amd.features import codebook as cbk
    out = {}
    for tag, s in SETS.items():
        rng = np.random.default_rng(s['seed'])
        X, _ = draw(rng, s['T'], s['K'], s['d'])
        init = X[np.sort(rng.choice(s['T'], s['K'], replace=False))].copy()
        out['%s_data' % tag] = X
        # the reference's iterative builder
        want = rhac.iterative_kmeans(X, s['K'])
        mine, gap_i = stepped_iterative(cbk, X, s['K'])
        assert gap_i > GAP, (tag, 'iterative', gap_i)
        assert np.array_equal(mine, cbk.host_iterative_kmeans(X, s['K']))
        assert np.array_equal(sorted_rows(mine), sorted_rows(want)), (tag, 'iterative')
        out['%s_iterative' % tag] = want
        # kmeans2 from a given matrix
        cb, labels = kmeans2(X, init, minit='matrix')
        mine, mine_labels, gap_m = stepped_lloyd(cbk, X, init, 10, allow_empty=False)
        assert gap_m > GAP, (tag, 'matrix', gap_m)
        assert np.array_equal(mine, cb) and np.array_equal(mine_labels, labels), (tag, 'matrix')
        twin = cbk.host_kmeans(X, init)
        assert np.array_equal(twin[0], cb) and np.array_equal(twin[1], labels)
        out['%s_init' % tag], out['%s_matrix' % tag], out['%s_matrix_labels' % tag] = init, cb, labels.astype(np.int16)
        # kmeans2 from its 'random' initialisation: build_codebook(mode='raw') with the generator pinned
        cb, labels = kmeans2(X, s['K'], minit='random', rng=np.random.default_rng(s['raw_seed']))
        G, colsum, T = cbk.host_gram(X, None, -1)
        first = cbk.random_init(G, colsum, T, s['K'], np.random.default_rng(s['raw_seed']))
        mine, mine_labels, gap_r = stepped_lloyd(cbk, X, first, 10, allow_empty=False)
        assert gap_r > GAP, (tag, 'raw', gap_r)
        assert np.array_equal(mine, cb) and np.array_equal(mine_labels, labels), (tag, 'raw')
        assert np.array_equal(cbk.host_build_codebook(X, s['K'], mode='raw', rng=s['raw_seed']), cb)
        out['%s_raw' % tag], out['%s_raw_labels' % tag], out['%s_raw_seed' % tag] = cb, labels.astype(np.int16), np.asarray(s['raw_seed'])
        print('set %s: %d x %d, K = %d: smallest relative gap iterative %.3g, matrix %.3g, raw %.3g'
              % (tag, s['T'], s['d'], s['K'], gap_i, gap_m, gap_r))
    path = os.path.join(HERE, 'g22_kmeans.npz')
    np.savez_compressed(path, **out)
    print('%s: %d bytes' % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 200 * 1024


if __name__ == '__main__':
    main(sys.argv[1])
