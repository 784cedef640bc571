#!/usr/bin/env python3
"""G20: outputs of the REFERENCE's `metrics.mutual_information`, `entropy` and `conditional_entropy` on small joint tables.

    python tests/golden/make_golden_information.py <directory of the reference checkout>

Writes tests/golden/g20_information.npz.  The tables are regenerated from the seed by `tables()` below (so the fixture holds them
only for the record); the reference's outputs are the data that travels.  Nothing of the reference's source does.

The tables: 2 x B and a few R x C tables of counts divided by their total -- as plot_info_matrix.py:88-90 forms them -- with
B from 1 to 16; among them tables with zero cells, a zero row, a single non-zero cell, and skewed tables whose mass sits in the
first bin (what histograms of NMF coefficients look like)."""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
WIDTH = 16          # tables are stored padded to [4, WIDTH]; `shapes` holds their own sizes


def tables(seed=20):
    rng = np.random.default_rng(seed)
    out = []
    for t in range(200):
        kind = t % 8
        rows = 2 if kind != 7 else int(rng.integers(2, 5))
        cols = int(rng.integers(1, WIDTH + 1))
        if kind == 0:        # dense counts
            c = rng.integers(1, 400, (rows, cols))
        elif kind == 1:      # many zero cells
            c = rng.integers(0, 50, (rows, cols)) * (rng.random((rows, cols)) < 0.4)
        elif kind == 2:      # a zero row
            c = rng.integers(0, 90, (rows, cols))
            c[0] = 0
        elif kind == 3:      # one non-zero cell
            c = np.zeros((rows, cols), dtype=np.int64)
            c[rng.integers(0, rows), rng.integers(0, cols)] = rng.integers(1, 1000)
        elif kind == 4:      # the mass in the first bin
            c = rng.integers(0, 6, (rows, cols))
            c[:, 0] += rng.integers(200, 5000, rows)
        elif kind == 5:      # a rare label against a common rest
            c = np.vstack([rng.integers(0, 3, cols), rng.integers(100, 100000, cols)])
        elif kind == 6:      # large counts
            c = rng.integers(0, 1 << 28, (rows, cols))
        else:                # more than two rows
            c = rng.integers(0, 30, (rows, cols))
        c = np.asarray(c, dtype=np.int64)
        if c.sum() == 0:
            c[0, 0] = 1
        out.append(c)
    return out


def main(reference):
    sys.path.insert(0, reference)
    from multimodal.lib import metrics as rmetrics
    counts = tables()
    padded = np.zeros((len(counts), 4, WIDTH), dtype=np.int64)
    shapes = np.zeros((len(counts), 2), dtype=np.int64)
    mi, ent, cond0, cond1 = (np.zeros(len(counts)) for _ in range(4))
    for i, c in enumerate(counts):
        padded[i, :c.shape[0], :c.shape[1]] = c
        shapes[i] = c.shape
        p = 1. * c / c.sum()
        mi[i] = rmetrics.mutual_information(p)
        ent[i] = rmetrics.entropy(p)
        cond0[i] = rmetrics.conditional_entropy(p, axis=0)
        cond1[i] = rmetrics.conditional_entropy(p, axis=1)
    path = os.path.join(HERE, 'g20_information.npz')
    np.savez_compressed(path, counts=padded, shapes=shapes, mutual_information=mi, entropy=ent, conditional_entropy_0=cond0,
                        conditional_entropy_1=cond1)
    print('%s: %d tables, %d bytes' % (path, len(counts), os.path.getsize(path)))


if __name__ == '__main__':
    main(sys.argv[1])
