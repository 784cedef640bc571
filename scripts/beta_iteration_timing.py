#!/usr/bin/env python3
"""Milliseconds per fit iteration of the beta loop beside the weighted KL iteration, one problem per process:

    python scripts/beta_iteration_timing.py --precision f64 --beta 0.5 [--weights] [--n 2000 --f 4096 --k 200]

--beta 1 times the KL loop (with --weights: the weighted one, whose launch list the beta iteration extends by one ratio pass).
KLNMF_LIB selects the library (an A/B against another build runs this script once per build, alternating).  Prints one JSON
line: the median and the fastest of --repeats timed segments of --iters iterations behind --warmup iterations."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_amd import _native      # noqa: E402

NO_STOP = -1e300


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--precision', default='f64', choices=['f64', 'f32'])
    p.add_argument('--beta', type=float, default=2.0)
    p.add_argument('--weights', action='store_true')
    p.add_argument('--n', type=int, default=2000)
    p.add_argument('--f', type=int, default=4096)
    p.add_argument('--k', type=int, default=200)
    p.add_argument('--iters', type=int, default=30)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--repeats', type=int, default=5)
    a = p.parse_args()
    rng = np.random.default_rng(1)
    dt = np.float64 if a.precision == 'f64' else np.float32
    V = (rng.gamma(1.0, 1.0, (a.n, a.f)) + 0.05).astype(dt)
    H = rng.random((a.k, a.f)) + 0.05
    H = (H / H.sum(axis=1, keepdims=True)).astype(dt)
    with _native.Context(a.precision) as ctx:
        ctx.set_problem(a.n, a.f, a.k, max(a.iters, a.warmup))
        ctx.upload_V(V)
        if a.weights:
            ctx.upload_weights((rng.random((a.n, a.f)) + 0.5).astype(dt))
        if a.beta != 1.0:
            ctx.set_divergence(a.beta)
        ctx.set_H(H)
        ctx.init_W()
        ctx.run(a.warmup, True, NO_STOP)
        ms = []
        for _ in range(a.repeats):
            ctx.synchronize()
            t0 = time.perf_counter()
            ctx.run(a.iters, True, NO_STOP)
            ms.append((time.perf_counter() - t0) * 1e3 / a.iters)
    print(json.dumps({'lib': os.environ.get('KLNMF_LIB', 'tree'),
                      'precision': a.precision, 'beta': a.beta, 'weights': a.weights, 'shape': [a.n, a.f, a.k],
                      'ms_per_iteration_median': round(float(np.median(ms)), 4), 'ms_per_iteration_min': round(min(ms), 4)}))


if __name__ == '__main__':
    main()
