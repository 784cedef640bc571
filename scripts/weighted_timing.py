#!/usr/bin/env python3
"""A weighted against an unweighted fit iteration of the exact modes at the README's exact-mode shape (2000 x 4096, k = 200), in
f64 and f32, in one process.

    python scripts/weighted_timing.py [--n 2000 --f 4096 --k 200] [--iters 50 --segments 7] [--out FILE.json]
    rocprofv3 --kernel-trace --stats -d OUT -o weighted -- python scripts/weighted_timing.py --segments 1 --precisions f64

Per precision one context holds the problem; segments alternate between the unweighted loop (klnmf_clear_weights) and the
weighted one (klnmf_upload_weights: uniform weights with 30 % zeros), each a fresh fit from W0 = V.H0^T: klnmf_loop_begin, a
warm-up of `--warmup` iterations, a synchronise, then `--iters` iterations of klnmf_run_more (tol = 0: the stop rule never
fires on a falling loss) under a host clock that ends in a synchronise.  Reported: the median over the segments of
ms per iteration, their spread (min .. max), and weighted / unweighted.  The weighted iteration does five contractions of
n f k where the unweighted does three and reads the weights in three of its passes.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=2000)
    ap.add_argument('--f', type=int, default=4096)
    ap.add_argument('--k', type=int, default=200)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--segments', type=int, default=7)
    ap.add_argument('--precisions', default='f64,f32')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from multimodal_amd import _native

    rng = np.random.default_rng(0)
    V = rng.gamma(1.0, 1.0, (a.n, a.f)) + 0.05
    Om = rng.random((a.n, a.f)) * (rng.random((a.n, a.f)) > 0.3)
    H0 = rng.random((a.k, a.f)) + 0.05
    H0 /= H0.sum(axis=1, keepdims=True)
    result = {'shape': [a.n, a.f, a.k], 'iters': a.iters, 'segments': a.segments, 'device': _native.device_info(0)}
    for prec in a.precisions.split(','):
        dt = np.float64 if prec == 'f64' else np.float32
        Vu, Omu, Hu = V.astype(dt), Om.astype(dt), H0.astype(dt)
        times = {'unweighted': [], 'weighted': []}
        with _native.Context(prec, device=0) as c:
            c.set_problem(a.n, a.f, a.k, a.iters + a.warmup)
            c.upload_V(Vu)
            result.setdefault('regime', {})[prec] = list(c.exact_regime())
            for _ in range(a.segments):
                for which in ('unweighted', 'weighted'):
                    if which == 'weighted':
                        c.upload_weights(Omu)
                    else:
                        c.clear_weights()
                    assert c.weighted() == (which == 'weighted')
                    c.set_H(Hu)
                    c.init_W()
                    c.loop_begin()
                    c.run_more(a.warmup, True, 0.0)
                    c.synchronize()
                    t0 = time.perf_counter()
                    c.run_more(a.iters, True, 0.0)
                    c.synchronize()
                    dt_s = time.perf_counter() - t0
                    _, n_done, stopped = c.loop_end(a.iters + a.warmup)
                    assert n_done == a.iters + a.warmup and not stopped, (which, n_done, stopped)
                    times[which].append(1e3 * dt_s / a.iters)
        row = {}
        for which, t in times.items():
            row[which] = {'median_ms': float(np.median(t)), 'min_ms': float(min(t)), 'max_ms': float(max(t))}
        row['ratio'] = row['weighted']['median_ms'] / row['unweighted']['median_ms']
        result[prec] = row
        print('%s  unweighted %.4f ms (%.4f .. %.4f)   weighted %.4f ms (%.4f .. %.4f)   ratio %.3f'
              % (prec, row['unweighted']['median_ms'], row['unweighted']['min_ms'], row['unweighted']['max_ms'],
                 row['weighted']['median_ms'], row['weighted']['min_ms'], row['weighted']['max_ms'], row['ratio']), flush=True)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
