#!/usr/bin/env python3
"""B same-shape MASKED problems of the exact modes as ONE batch (klnmf_batch_upload_presence, csrc/batch.hip.h) against the same B
masked problems one after another in contexts (klnmf_upload_presence + klnmf_run: what these calls ran before masked batches
existed), at the reference's own scale, in f64 and f32, in one process.  scripts/batch_timing.py's protocol under a mask.

    python scripts/batch_mask_timing.py [--sizes 1,2,4,8,16,32] [--iters 100 --segments 7] [--sweep] [--out FILE.json]

Two shapes: a fit of 900 x 2450, k = 50, under M = 2 modalities of 450 + 2000 columns, the second one absent from a third of the
rows; and a transform of 100 x 450, k = 50, under one modality absent from a third of the rows (those rows keep their W0).  Every
problem has its own data, its own H0 and its own mask (another third of the rows); tol = 0.
Per precision, shape and B the problems are uploaded once, into one batch and into B contexts.  A segment re-sets every
dictionary, forms W0 = V.H0^T, synchronises, and then times the loop alone under a host clock that ends in a synchronise:
klnmf_batch_run of `--iters` iterations, or klnmf_run of `--iters` iterations on each of the B contexts in turn (each returns
synchronised, as it does for KLdivNMF).  The two loops alternate, `--segments` times.  Reported: the median over the segments of
ms per loop with min .. max, sequential over batched, and whether the batched median lies below the MINIMUM segment of the
sequential loop.

--sweep: also one masked `run_sweep` wall time with batch = 1 and batch = 8 on the synthetic two-modality set of
scripts/time_experiment_run.py (1000 samples, 450 + 2000 columns, the second modality absent from a third of the samples), k = 50,
8 runs, 50 + 50 iterations, f64; the second of two rounds is reported."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

# (name, n, f, k, fit, column bounds of the modalities; the last modality is the one absent from a third of the rows)
SHAPES = (('fit', 900, 2450, 50, True, (0, 450, 2450)), ('transform', 100, 450, 50, False, (0, 450)))


def absent_third(n, seed):
    """A presence column: 0 in a seeded third of the rows, 1 elsewhere."""
    col = np.ones(n)
    col[np.random.default_rng(seed).permutation(n)[:n // 3]] = 0.0
    return col


def problems(n, f, k, count, dt, n_mod):
    out = []
    for p in range(count):
        rng = np.random.default_rng(1000 + p)
        V = rng.gamma(1.0, 1.0, (n, f)) + 0.05
        H0 = rng.random((k, f)) + 0.05
        H0 /= H0.sum(axis=1, keepdims=True)
        P = np.ones((n, n_mod))
        P[:, -1] = absent_third(n, 2000 + p)
        out.append((V.astype(dt), H0.astype(dt), P.astype(dt)))
    return out


def time_sweep():
    from multimodal_amd.device_experiment import run_sweep
    from tests import golden_inputs as gi
    mods = gi.experiment_modalities(21, n_per_label=100, n_labels=10, dims=(450, 2000))
    data, labels = [m[0] for m in mods], list(mods[0][1])
    presence = [None, absent_third(len(labels), 5)]
    out = {}
    for batch in (1, 8, 1, 8):          # (the first pair warms the library up; the second is reported)
        t0 = time.perf_counter()
        run_sweep(data, labels, ['motion', 'sound'], [50], 8, iter_train=50, iter_test=50, devices=[0], precision='f64', presence=presence, batch=batch)
        out['batch_%d_s' % batch] = time.perf_counter() - t0
    print('masked run_sweep, k = 50, 8 runs, 50 + 50 iterations, f64: batch=1 %.3f s   batch=8 %.3f s' % (out['batch_1_s'], out['batch_8_s']),
          flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='1,2,4,8,16,32')
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--segments', type=int, default=7)
    ap.add_argument('--precisions', default='f64,f32')
    ap.add_argument('--sweep', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from multimodal_amd import _native

    sizes = [int(s) for s in a.sizes.split(',')]
    result = {'iters': a.iters, 'segments': a.segments, 'rows': []}
    if a.sweep:          # (first: the sweep's DeviceDataset brings torch's runtime up before the library opens its contexts)
        result['run_sweep'] = time_sweep()
    result['device'] = _native.device_info(0)
    for prec in a.precisions.split(','):
        dt = np.float64 if prec == 'f64' else np.float32
        for name, n, f, k, fit, bounds in SHAPES:
            probs = problems(n, f, k, max(sizes), dt, len(bounds) - 1)
            for B in sizes:
                times = {'batched': [], 'sequential': []}
                ctxs = [_native.Context(prec, device=0) for _ in range(B)]
                batch = _native.Batch(prec, B, device=0)
                try:
                    batch.set_problem(n, f, k, a.iters)
                    for p, c in enumerate(ctxs):
                        c.set_problem(n, f, k, a.iters)
                        c.upload_V(probs[p][0])
                        c.upload_presence(probs[p][2], bounds)
                        batch.upload_V(p, probs[p][0])
                        batch.upload_presence(p, probs[p][2], bounds)
                    assert batch.presence() == len(bounds) - 1 and all(c.presence() == len(bounds) - 1 for c in ctxs)
                    for _ in range(a.segments):
                        for p in range(B):
                            batch.set_H(p, probs[p][1])
                        batch.init_W()
                        t0 = time.perf_counter()
                        done = batch.run(a.iters, fit, 0.0)          # (synchronous on return)
                        times['batched'].append(1e3 * (time.perf_counter() - t0))
                        assert all(r[1] == a.iters and not r[2] for r in done)
                        for p, c in enumerate(ctxs):
                            c.set_H(probs[p][1])
                            c.init_W()
                            c.synchronize()
                        t0 = time.perf_counter()
                        done = [c.run(a.iters, fit, 0.0) for c in ctxs]      # (each synchronous on return)
                        times['sequential'].append(1e3 * (time.perf_counter() - t0))
                        assert all(r[1] == a.iters and not r[2] for r in done)
                    regime = {'batch': list(batch.exact_regime()), 'context': list(ctxs[0].exact_regime())}
                finally:
                    batch.close()
                    for c in ctxs:
                        c.close()
                row = {'precision': prec, 'shape': name, 'n': n, 'f': f, 'k': k, 'B': B, 'modalities': len(bounds) - 1, 'regime': regime}
                for which, t in times.items():
                    row[which] = {'median_ms': float(np.median(t)), 'min_ms': float(min(t)), 'max_ms': float(max(t))}
                b, s = row['batched'], row['sequential']
                row['sequential_over_batched'] = s['median_ms'] / b['median_ms']
                row['batched_median_below_sequential_minimum'] = bool(b['median_ms'] < s['min_ms'])
                result['rows'].append(row)
                print('%s masked %-9s %4d x %4d k=%d  B=%-2d  batched %8.3f ms (%.3f .. %.3f)   sequential %8.3f ms (%.3f .. %.3f)   x%.2f  %s'
                      % (prec, name, n, f, k, B, b['median_ms'], b['min_ms'], b['max_ms'], s['median_ms'], s['min_ms'], s['max_ms'],
                         row['sequential_over_batched'], 'faster' if row['batched_median_below_sequential_minimum'] else 'NOT FASTER'),
                      flush=True)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
