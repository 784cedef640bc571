#!/usr/bin/env python3
"""A beta batch beside the same problems run one after another, for information (no bar is set on it):

    python scripts/beta_batch_timing.py [--count 8 --n 500 --f 2450 --k 50 --beta 0.5 --iters 30] > profiles/beta_batch_timing.txt

`--count` problems of one shape, in f64 and in f32: `--iters` fit iterations of all of them as ONE `_native.Batch` under
`set_divergence(beta)`, against the same problems in `--count` contexts of the same library, each running its `--iters` iterations
behind the other.  Both arms are set up once; a timed segment is the loop call(s) alone (the batch's one `run`, the contexts'
`run`s one after another), behind `--warmup` iterations.  Two rounds alternate the arms (batch, contexts, batch, contexts) in one
process, `--repeats` segments each; the table holds the median and the fastest over both rounds in milliseconds per segment, and
the ratio of the medians."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_amd import _native      # noqa: E402

NO_STOP = -1e300


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--count', type=int, default=8)
    p.add_argument('--n', type=int, default=500)
    p.add_argument('--f', type=int, default=2450)
    p.add_argument('--k', type=int, default=50)
    p.add_argument('--beta', type=float, default=0.5)
    p.add_argument('--iters', type=int, default=30)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--repeats', type=int, default=5)
    a = p.parse_args()
    print('%d problems of %d x %d, k = %d, beta = %g: %d fit iterations per segment, milliseconds per segment (all problems)'
          % (a.count, a.n, a.f, a.k, a.beta, a.iters))
    print('%-5s %-22s %12s %12s' % ('prec', 'arm', 'median', 'fastest'))
    for prec in ('f64', 'f32'):
        rng = np.random.default_rng(1)
        dt = np.float64 if prec == 'f64' else np.float32
        Vs = [(rng.gamma(1.0, 1.0, (a.n, a.f)) + 0.05).astype(dt) for _ in range(a.count)]
        Hs = []
        for _ in range(a.count):
            H = rng.random((a.k, a.f)) + 0.05
            Hs.append((H / H.sum(axis=1, keepdims=True)).astype(dt))
        cap = max(a.iters, a.warmup)
        contexts = []
        with _native.Batch(prec, a.count) as batch:
            try:
                batch.set_problem(a.n, a.f, a.k, cap)
                for q, V in enumerate(Vs):
                    batch.upload_V(q, V)
                batch.set_divergence(a.beta)
                for q, H in enumerate(Hs):
                    batch.set_H(q, H)
                batch.init_W()
                batch.run(a.warmup, True, NO_STOP)
                for V, H in zip(Vs, Hs):
                    ctx = _native.Context(prec)
                    contexts.append(ctx)
                    ctx.set_problem(a.n, a.f, a.k, cap)
                    ctx.upload_V(V)
                    ctx.set_divergence(a.beta)
                    ctx.set_H(H)
                    ctx.init_W()
                    ctx.run(a.warmup, True, NO_STOP)

                def one_batch():
                    batch.run(a.iters, True, NO_STOP)

                def one_after_another():
                    for ctx in contexts:
                        ctx.run(a.iters, True, NO_STOP)
                ms = {'one batch': [], 'one after another': []}
                for _ in range(2):
                    for name, arm in (('one batch', one_batch), ('one after another', one_after_another)):
                        for _ in range(a.repeats):
                            t0 = time.perf_counter()
                            arm()      # (both loops return behind a synchronisation of their stream)
                            ms[name].append((time.perf_counter() - t0) * 1e3)
                regime = batch.exact_regime()
                solo_regime = contexts[0].exact_regime()
            finally:
                for ctx in contexts:
                    ctx.close()
        for name in ('one batch', 'one after another'):
            print('%-5s %-22s %12.3f %12.3f' % (prec, name, float(np.median(ms[name])), min(ms[name])))
        print('%-5s one after another / one batch = %.2f   (chunk counts: batch %r, context %r)'
              % (prec, float(np.median(ms['one after another'])) / float(np.median(ms['one batch'])), regime, solo_regime))


if __name__ == '__main__':
    main()
