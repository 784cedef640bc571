#!/usr/bin/env python3
"""A fit iteration of the exact modes with a row x modality presence mask against the same mask as an n x f weight buffer and
against the unweighted iteration, at the README's exact-mode shape (2000 x 4096, k = 200), in f64 and f32, in one process.

    python scripts/presence_timing.py [--n 2000 --f 4096 --k 200] [--iters 50 --segments 7] [--out FILE.json]
    rocprofv3 --kernel-trace --stats -d OUT -o presence -- python scripts/presence_timing.py --segments 1 --precisions f64

Two modalities of f / 2 columns, the second absent from 30 % of the rows.  Per precision one context holds the problem; segments
alternate between three loops -- unweighted (klnmf_clear_weights), the mask broadcast through klnmf_upload_weights (the path of
csrc/weighted.hip.h: five contractions of n f k, 7 n f streamed) and the mask through klnmf_upload_presence (csrc/presence.hip.h:
three contractions plus O(n k M), 4 n f streamed) -- each a fresh fit from W0 = V.H0^T: klnmf_loop_begin, a warm-up of `--warmup`
iterations, a synchronise, then `--iters` iterations of klnmf_run_more (tol = 0: the stop rule never fires on a falling loss)
under a host clock that ends in a synchronise.  Reported: the median over the segments of ms per iteration, their spread
(min .. max), each loop over the unweighted one, and whether the presence median lies below the midpoint of the other two.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

LOOPS = ('unweighted', 'weights', 'presence')


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
    bounds = [0, a.f // 2, a.f]
    P = np.ones((a.n, 2))
    P[:, 1] = rng.random(a.n) > 0.3
    V[:, bounds[1]:] *= P[:, 1:2]                       # a missing modality is stored as zeros
    Om = np.repeat(P, np.diff(bounds), axis=1)
    H0 = rng.random((a.k, a.f)) + 0.05
    H0 /= H0.sum(axis=1, keepdims=True)
    result = {'shape': [a.n, a.f, a.k], 'bounds': bounds, 'absent': float(1.0 - P[:, 1].mean()), 'iters': a.iters,
              'segments': a.segments, 'device': _native.device_info(0)}
    for prec in a.precisions.split(','):
        dt = np.float64 if prec == 'f64' else np.float32
        Vu, Omu, Pu, Hu = V.astype(dt), Om.astype(dt), P.astype(dt), H0.astype(dt)
        times = dict((which, []) for which in LOOPS)
        with _native.Context(prec, device=0) as c:
            c.set_problem(a.n, a.f, a.k, a.iters + a.warmup)
            c.upload_V(Vu)
            result.setdefault('regime', {})[prec] = list(c.exact_regime())
            for _ in range(a.segments):
                for which in LOOPS:
                    c.clear_weights()
                    if which == 'weights':
                        c.upload_weights(Omu)
                    elif which == 'presence':
                        c.upload_presence(Pu, bounds)
                    assert c.weighted() == (which == 'weights') and c.presence() == (2 if which == 'presence' else 0)
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
        med = dict((which, row[which]['median_ms']) for which in LOOPS)
        row['weights_ratio'] = med['weights'] / med['unweighted']
        row['presence_ratio'] = med['presence'] / med['unweighted']
        row['midpoint_ms'] = 0.5 * (med['unweighted'] + med['weights'])
        row['presence_below_midpoint'] = bool(med['presence'] < row['midpoint_ms'])
        result[prec] = row
        print('%s  ' % prec + '   '.join('%s %.4f ms (%.4f .. %.4f)' % (which, row[which]['median_ms'], row[which]['min_ms'],
                                                                        row[which]['max_ms']) for which in LOOPS), flush=True)
        print('%s  weights / unweighted %.3f   presence / unweighted %.3f   midpoint %.4f ms: presence %s'
              % (prec, row['weights_ratio'], row['presence_ratio'], row['midpoint_ms'],
                 'below' if row['presence_below_midpoint'] else 'ABOVE'), flush=True)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
