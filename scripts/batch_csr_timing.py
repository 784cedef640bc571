#!/usr/bin/env python3
"""B same-shape CSR problems as ONE CSR batch (klnmf_batch_set_problem_sparse, csrc/batch_sparse.hip.h) against the same B problems
one after another in CSR contexts (klnmf_set_problem_sparse + klnmf_run: what `keep_sparse=True, batch=B` ran before CSR batches
existed -- the BASELINE), at the reference experiment's own scale, in f64 and f32, in one process.  scripts/batch_timing.py's
protocol on CSR input.

    python scripts/batch_csr_timing.py [--sizes 2,8,32] [--iters 50 --segments 7] [--out FILE.json]

The data: a synthetic CSR histogram set of 1000 samples x 2450 columns (two modalities of 450 + 2000 columns, 5 % stored, counts
1 + Poisson(2)) resident on the device; problem p is the 900 rows a run draws (a seeded permutation's first 900, sorted) with the
coefficients 1 / mean row sum, k = 50, its own H0; tol = 0.
The loop.  Per precision and B the problems are gathered once, into one batch and into B contexts.  A segment re-sets every
dictionary, forms W0 = X.H0^T, synchronises, and then times the fit loop alone under a host clock that ends in a synchronise:
klnmf_batch_run of `--iters` iterations, or klnmf_run of `--iters` iterations on each of the B contexts in turn.  The two loops
alternate, `--segments` times.  Reported: the median over the segments with min .. max, per loop and per iteration and problem,
sequential over batched, and whether the batched median lies below the MINIMUM segment of the sequential loop.
The set-up.  Also per segment, alternating: the wall time of klnmf_batch_set_problem_sparse + B gathers with their CSC builds
(klnmf_batch_upload_csr_device_rows) against B times klnmf_set_problem_sparse + klnmf_upload_csr_device_rows."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402

N_SAMPLES, DIMS, N_ROWS, K = 1000, (450, 2000), 900, 50


def dataset(dt):
    rng = np.random.default_rng(7)
    mods = []
    for d in DIMS:
        m = sp.random(N_SAMPLES, d, density=0.05, format='csr', random_state=rng, data_rvs=lambda s: 1.0 + rng.poisson(2.0, s))
        m = sp.csr_matrix(m, dtype=dt)
        m.sort_indices()
        mods.append(m)
    return mods


def stats(t):
    return {'median_ms': float(np.median(t)), 'min_ms': float(min(t)), 'max_ms': float(max(t))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='2,8,32')
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--segments', type=int, default=7)
    ap.add_argument('--precisions', default='f64,f32')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from multimodal_amd import _native
    from multimodal_amd import device_data

    sizes = [int(s) for s in a.sizes.split(',')]
    to_device = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).cuda()
    result = {'iters': a.iters, 'segments': a.segments, 'baseline': 'B CSR contexts one after another (the parent commit\'s route for '
              'keep_sparse=True, batch=B)', 'rows': [], 'device': _native.device_info(0)}
    f = sum(DIMS)
    bounds = [0, DIMS[0], f]
    for prec in a.precisions.split(','):
        dt = np.float64 if prec == 'f64' else np.float32
        mods = dataset(dt)
        coefs = [1.0 / float(m.sum(axis=1).mean()) for m in mods]
        srcs = [device_data._DeviceCsr(m, to_device) for m in mods]
        sources = [s.pointers() for s in srcs]
        for B in sizes:
            rows = [np.sort(np.random.default_rng(100 + p).permutation(N_SAMPLES)[:N_ROWS]).astype(np.int64) for p in range(B)]
            idxs = [to_device(r) for r in rows]
            nnzs = [device_data.csr_rows_plan([s.indptr for s in srcs], r, coefs, [s.least for s in srcs])[0] for r in rows]
            H0s = []
            for p in range(B):
                H0 = np.random.default_rng(1000 + p).random((K, f)) + 0.05
                H0s.append((H0 / H0.sum(axis=1, keepdims=True)).astype(dt))
            times = {'batched': [], 'sequential': [], 'setup_batched': [], 'setup_sequential': []}
            ctxs = [_native.Context(prec, device=0) for _ in range(B)]
            batch = _native.Batch(prec, B, device=0)

            def setup_batch():
                batch.set_problem_sparse(N_ROWS, f, K, a.iters, nnzs)
                for p in range(B):
                    batch.upload_csr_device_rows(p, sources, bounds, coefs, N_SAMPLES, idxs[p].data_ptr(), N_ROWS)

            def setup_contexts():
                for p, c in enumerate(ctxs):
                    c.set_problem_sparse_shape(N_ROWS, f, K, a.iters, nnzs[p])
                    c.upload_csr_device_rows(sources, bounds, coefs, N_SAMPLES, idxs[p].data_ptr(), N_ROWS)
            try:
                for _ in range(a.segments):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    setup_batch()                                   # (every upload synchronous on return)
                    times['setup_batched'].append(1e3 * (time.perf_counter() - t0))
                    t0 = time.perf_counter()
                    setup_contexts()
                    times['setup_sequential'].append(1e3 * (time.perf_counter() - t0))
                    for p in range(B):
                        batch.set_H(p, H0s[p])
                    batch.init_W()
                    t0 = time.perf_counter()
                    done = batch.run(a.iters, True, 0.0)          # (synchronous on return)
                    times['batched'].append(1e3 * (time.perf_counter() - t0))
                    assert all(r[1] == a.iters and not r[2] for r in done)
                    for p, c in enumerate(ctxs):
                        c.set_H(H0s[p])
                        c.init_W()
                        c.synchronize()
                    t0 = time.perf_counter()
                    done = [c.run(a.iters, True, 0.0) for c in ctxs]      # (each synchronous on return)
                    times['sequential'].append(1e3 * (time.perf_counter() - t0))
                    assert all(r[1] == a.iters and not r[2] for r in done)
                blocks = {'batch': list(batch.sparse_blocks()), 'context': list(ctxs[0].sparse_blocks())}
                same = all(np.array_equal(batch.get_W(p), ctxs[p].get_W()) for p in range(min(B, 2)))
            finally:
                batch.close()
                for c in ctxs:
                    c.close()
            row = {'precision': prec, 'n': N_ROWS, 'f': f, 'k': K, 'B': B, 'nnz_mean': float(np.mean(nnzs)), 'blocks': blocks,
                   'bits_equal': bool(same)}
            for which, t in times.items():
                row[which] = stats(t)
            b, s = row['batched'], row['sequential']
            per = 1e3 / (a.iters * B)
            row['us_per_iteration_and_problem'] = {'batched': b['median_ms'] * per, 'sequential': s['median_ms'] * per}
            row['sequential_over_batched'] = s['median_ms'] / b['median_ms']
            row['batched_median_below_sequential_minimum'] = bool(b['median_ms'] < s['min_ms'])
            row['setup_sequential_over_batched'] = row['setup_sequential']['median_ms'] / row['setup_batched']['median_ms']
            result['rows'].append(row)
            print('%s CSR fit %d x %d k=%d nnz~%d  B=%-2d  batched %8.3f ms (%.3f .. %.3f)   sequential %8.3f ms (%.3f .. %.3f)   x%.2f  %s'
                  '   | per iteration and problem %.1f vs %.1f us | set-up %.2f ms (%.2f .. %.2f) vs %.2f ms (%.2f .. %.2f) | blocks %s bits %s'
                  % (prec, N_ROWS, f, K, int(np.mean(nnzs)), B, b['median_ms'], b['min_ms'], b['max_ms'], s['median_ms'], s['min_ms'],
                     s['max_ms'], row['sequential_over_batched'],
                     'faster' if row['batched_median_below_sequential_minimum'] else 'NOT FASTER',
                     row['us_per_iteration_and_problem']['batched'], row['us_per_iteration_and_problem']['sequential'],
                     row['setup_batched']['median_ms'], row['setup_batched']['min_ms'], row['setup_batched']['max_ms'],
                     row['setup_sequential']['median_ms'], row['setup_sequential']['min_ms'], row['setup_sequential']['max_ms'],
                     blocks, same), flush=True)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
