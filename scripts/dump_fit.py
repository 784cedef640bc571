#!/usr/bin/env python3
"""Dump W, H and the loss record of a few seeded fits to an .npz (to compare two builds of the library bit by bit:
KLNMF_LIB=ab/libklnmf_A.so scripts/dump_fit.py a.npz; KLNMF_LIB=... scripts/dump_fit.py b.npz; scripts/dump_fit.py --cmp a.npz b.npz)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

# (n, f, k, iterations, precision, devices): few rows (column-split row pass), many rows, k = 200 and 500 on 16-bit tiles; a fit that
# enters the fp8 regime; an f64 fit; a two-member group on one device
CASES = [(3000, 520, 200, 4, 'f16', None), (70000, 256, 200, 5, 'f16', None), (2100, 4096, 500, 3, 'f16', None),
         (520, 1030, 200, 5, 'f16', None), (50000, 4096, 50, 30, 'f16', None), (3000, 520, 20, 6, 'f64', None),
         (3000, 520, 200, 4, 'f16', (0, 0))]


def main():
    if sys.argv[1] == '--cmp':
        a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
        bad = 0
        for key in a.files:
            same = np.array_equal(a[key], b[key])
            d = np.abs(a[key].astype(np.float64) - b[key].astype(np.float64)).max() / max(1e-300, np.abs(a[key]).max())
            print('%-28s %s  (max rel diff %.2e)' % (key, 'identical' if same else 'DIFFERENT', d))
            bad += 0 if same else 1
        sys.exit(1 if bad else 0)
    from multimodal_amd.lib.nmf import KLdivNMF
    from oracle import klnmf_oracle as orc
    out = {}
    for (n, f, k, iters, prec, devices) in CASES:
        X = orc.synthetic_V(5, n, f, min(k, 32))
        H0 = orc.synthetic_H0(5, f, k)
        try:
            m = KLdivNMF(n_components=k, max_iter=iters, tol=0, precision=prec, device=devices)
            m._init_dictionary = H0
            W, e = m.fit_transform(X, return_errors=True)
        except RuntimeError as err:
            print('skipped %s: %s' % ((n, f, k), str(err)[:70]))
            continue
        tag = '%dx%dk%d' % (n, f, k) + ('' if prec == 'f16' else '_' + prec) + ('_group%d' % len(devices) if devices else '')
        out[tag + '_W'] = W
        out[tag + '_H'] = m.components_
        out[tag + '_e'] = np.array(e)
        print(tag, 'loss', e[-1], 'fp8', m.last_fp8_report, flush=True)
    np.savez(sys.argv[1], **out)


if __name__ == '__main__':
    main()
