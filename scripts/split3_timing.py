#!/usr/bin/env python3
"""Per-iteration time of klnmf_run in precision='bf16x3' next to 'f32' and 'f16', in one process on one GPU, at four shapes:
2000 x 4096 k = 200, G19's 40 000 x 512 k = 16, C3's 90 000 x 6144 k = 200, and 1 000 000 x 128 k = 20 (a shape 'auto'
sends to f32).  Targets of the mode (estimates from peak rates): no shape slower than f32, at
least 2.5x faster than f32 at the two k = 200 shapes.

    python scripts/split3_timing.py [--shapes 0,1,2,3] [--modes bf16x3,f32,f16]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from multimodal_amd import _native  # noqa: E402

# (n, f, k, timed iterations)
SHAPES = [(2000, 4096, 200, 200), (40000, 512, 16, 100), (90000, 6144, 200, 20), (1000000, 128, 20, 20)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='0,1,2,3')
    ap.add_argument('--modes', default='bf16x3,f32,f16')
    a = ap.parse_args()
    modes = a.modes.split(',')
    table = {}
    for si in [int(s) for s in a.shapes.split(',')]:
        n, f, k, iters = SHAPES[si]
        rng = np.random.default_rng(3)
        X = rng.random((n, f), dtype=np.float32) + np.float32(0.01)
        H0 = rng.random((k, f)) + .01
        H0 /= H0.sum(axis=1, keepdims=True)
        for mode in modes:
            with _native.Context(mode, device=0) as ctx:
                ctx.set_problem(n, f, k, iters + 3)
                if not ctx.exact:
                    ctx.set_v_max(float(X.max()))
                ctx.upload_blocks([X])
                ctx.set_H(H0)
                ctx.init_W()
                ctx.run(3, True, -1e300)                      # warm-up
                t0 = time.perf_counter()
                errs, n_done, stopped = ctx.run(iters, True, -1e300)
                dt = time.perf_counter() - t0
            us = 1e6 * dt / max(1, n_done)
            table[(si, mode)] = us
            print('%7d x %5d k=%3d %6s: %9.1f us / iteration  (%d iterations, last loss %.9e)'
                  % (n, f, k, mode, us, n_done, errs[-1]), flush=True)
        del X
    print('\nshape                      ' + ''.join('%12s' % m for m in modes) + '   f32 / bf16x3')
    for si in sorted({s for s, _ in table}):
        n, f, k, _ = SHAPES[si]
        row = ''.join('%12.1f' % table[(si, m)] if (si, m) in table else '%12s' % '-' for m in modes)
        ratio = table[(si, 'f32')] / table[(si, 'bf16x3')] if (si, 'f32') in table and (si, 'bf16x3') in table else float('nan')
        print('%7d x %5d k=%3d      %s   %.2fx' % (n, f, k, row, ratio))


if __name__ == '__main__':
    main()
