#!/usr/bin/env python3
"""Dump W, H and the loss record of a few seeded fits to an .npz (to compare two builds of the library bit by bit:
KLNMF_LIB=ab/libklnmf_A.so scripts/dump_fit.py a.npz; KLNMF_LIB=... scripts/dump_fit.py b.npz; scripts/dump_fit.py --cmp a.npz b.npz).

Every fit runs on the pooled context of its precision (multimodal_amd/_native.py: one native context per (precision, device),
its problem released between fits), so the case list is also a reuse sequence.  POOLED_SEQUENCES are explicit ones -- dense, CSR,
dense with other shapes; large, small, large -- whose last fit is run again on a fresh context (KLNMF_NO_POOL=1): the pair must
be bit-identical within ONE library (a field that survived from an earlier problem would show here), which --cmp checks too."""
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

# (n, f, k, iterations, precision, devices, CSR density or None).  16-bit mode: few rows (column-split row pass), many rows,
# k = 200 and 500 on 16-bit tiles, a fit that enters the fp8 regime (fp8 tiles, the fp8 x fp8 column pass), a hybrid tail (90 000
# rows); exact modes: an f64 fit, f64 / f32 with several W chunks and H segments (100 x 16385), f16x3 on its fused kernels
# (k <= 256) and on bf16x3's (k > 256); CSR in the blocked regime (two column blocks) and unblocked (k = 513); a two-member
# group on one device
CASES = [(3000, 520, 200, 4, 'f16', None, None), (70000, 256, 200, 5, 'f16', None, None), (2100, 4096, 500, 3, 'f16', None, None),
         (520, 1030, 200, 5, 'f16', None, None), (50000, 4096, 50, 30, 'f16', None, None), (3000, 520, 20, 6, 'f64', None, None),
         (3000, 520, 200, 4, 'f16', (0, 0), None),
         (100, 16385, 33, 4, 'f64', None, None), (100, 16385, 33, 4, 'f32', None, None),
         (700, 900, 200, 4, 'f16x3', None, None), (600, 800, 300, 3, 'f16x3', None, None),
         (90000, 6144, 200, 2, 'f16', None, None),
         (4000, 30000, 32, 4, 'f32', None, 0.02), (300, 700, 513, 3, 'f64', None, 0.1)]
# weighted and masked fits of the exact modes (n, f, k, iterations, precision, 'weights' | 'presence', route), built the way
# tests/test_weighted_gpu.py and tests/test_presence_gpu.py build theirs (weighted_cases.general; presence_cases.mask / bounds with
# three modalities).  route: what (W chunks, H segments, H rule from the slabs) of the context's plan must be (cost_fit asserts
# it; None: any) -- the whole W rule with the H rule from the slabs, the issue's 3000 x 520 (W chunks, H rule from the summed
# slabs on a 256-CU device), and several W chunks with H segments
COST_SHAPES = ((4111, 63, 200, 4, (1, 1, 1)), (3000, 520, 20, 4, None), (100, 16385, 33, 3, ('>1', '>1', 0)))
COST_CASES = [(n, f, k, it, prec, cost, route) for (n, f, k, it, route) in COST_SHAPES for prec in ('f64', 'f32')
              for cost in ('weights', 'presence')]
POOLED_SEQUENCES = {
    'pool_f32': [(500, 300, 20, 5, 'f32', None, None), (2000, 3000, 16, 4, 'f32', None, 0.02), (1200, 700, 40, 5, 'f32', None, None)],
    'pool_f16': [(70000, 256, 200, 5, 'f16', None, None), (520, 1030, 200, 5, 'f16', None, None), (40000, 512, 50, 6, 'f16', None, None)],
}


def tag_of(case):
    n, f, k, _, prec, devices, density = case
    return ('%dx%dk%d' % (n, f, k) + ('' if prec == 'f16' else '_' + prec) + ('_group%d' % len(devices) if devices else '')
            + ('_csr' if density else ''))


def fit(case):
    """(W, H, losses, fp8 report) of one seeded fit."""
    from multimodal_amd.lib.nmf import KLdivNMF
    from oracle import klnmf_oracle as orc
    n, f, k, iters, prec, devices, density = case
    if density:
        X = sp.random(n, f, density=density, format='csr', random_state=5, data_rvs=np.random.default_rng(5).random)
        X.data += 0.05
    else:
        X = orc.synthetic_V(5, n, f, min(k, 32))
    m = KLdivNMF(n_components=k, max_iter=iters, tol=0, precision=prec, device=devices)
    m._init_dictionary = orc.synthetic_H0(5, f, k)
    W, e = m.fit_transform(X, return_errors=True)
    return W, m.components_, np.array(e), m.last_fp8_report


def cost_fit(case):
    """(W, H, losses, route) of one seeded weighted or masked fit on a context of its own."""
    from multimodal_amd import _native
    from oracle import klnmf_oracle as orc
    from tests import presence_cases as pc
    from tests import weighted_cases as wc
    n, f, k, iters, prec, cost, want = case
    dt = np.float64 if prec == 'f64' else np.float32
    V, H0 = orc.synthetic_V(5, n, f, min(k, 32)), orc.synthetic_H0(5, f, k)
    with _native.Context(prec) as ctx:
        ctx.set_problem(n, f, k, iters)
        ctx.upload_V(V.astype(dt))
        if cost == 'weights':
            ctx.upload_weights(wc.general(n, f, seed=3 * n + 5 * f + k).astype(dt))
        else:
            ctx.upload_presence(pc.mask(n, 3, seed=3 * n + 5 * f + k).astype(dt), pc.bounds(f, 3))
        route = list(ctx.exact_regime())
        for got, w in zip(route[1:], want or ()):
            assert (got > 1) if w == '>1' else (got == w), (case, route)
        ctx.set_H(H0.astype(dt))
        ctx.init_W()
        errors, n_done, _ = ctx.run(iters, True, -1e300)
        assert n_done == iters
        return ctx.get_W(), ctx.get_H(), np.array(errors), route


def main():
    if sys.argv[1] == '--cmp':
        a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
        bad = 0 if sorted(a.files) == sorted(b.files) else 1
        for key in a.files:
            same = key in b.files and np.array_equal(a[key], b[key])
            d = np.abs(a[key].astype(np.float64) - b[key].astype(np.float64)).max() / max(1e-300, np.abs(a[key]).max()) if key in b.files else np.nan
            print('%-36s %s  (max rel diff %.2e)' % (key, 'identical' if same else 'DIFFERENT', d))
            bad += 0 if same else 1
        for name, z in ((sys.argv[2], a), (sys.argv[3], b)):
            for key in z.files:
                if '_third_' in key:
                    same = np.array_equal(z[key], z[key.replace('_third_', '_fresh_')])
                    print('%-36s %s its fresh-context twin in %s' % (key, 'identical to' if same else 'DIFFERENT from', name))
                    bad += 0 if same else 1
        sys.exit(1 if bad else 0)
    out = {}

    def record(tag, case):
        try:
            W, H, e, fp8 = fit(case)
        except RuntimeError as err:
            print('skipped %s: %s' % (tag, str(err)[:70]))
            return
        out[tag + '_W'], out[tag + '_H'], out[tag + '_e'] = W, H, e
        print(tag, 'loss', e[-1], 'fp8', fp8, flush=True)

    for case in CASES:
        record(tag_of(case), case)
    for case in COST_CASES:
        tag = '%dx%dk%d_%s_%s' % (case[0], case[1], case[2], case[4], case[5])
        W, H, e, route = cost_fit(case)
        out[tag + '_W'], out[tag + '_H'], out[tag + '_e'] = W, H, e
        print(tag, 'loss', e[-1], 'route', route, flush=True)
    for name, seq in POOLED_SEQUENCES.items():
        for i, case in enumerate(seq):
            record('%s_%s_%s' % (name, ('first', 'second', 'third')[i], tag_of(case)), case)
        os.environ['KLNMF_NO_POOL'] = '1'          # (read at every context's creation)
        try:
            record('%s_fresh_%s' % (name, tag_of(seq[-1])), seq[-1])
        finally:
            del os.environ['KLNMF_NO_POOL']
    np.savez(sys.argv[1], **out)


if __name__ == '__main__':
    main()
