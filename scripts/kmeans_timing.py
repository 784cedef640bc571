#!/usr/bin/env python3
"""What the codebook builders cost on the device, against scipy on the host of the same machine.

Frames: T = 800 000 rows drawn around 150 centres (0.35 sigma noise), d = 13 (one MFCC stream) or 39 columns.

  (a) `features.codebook.iterative_kmeans` to K = 150 on d = 13 and to K = 100 on d = 39, float64 and float32, from tensors
      already on the device: one warm-up to K = 3, then the whole build timed once with a host clock that ends in a synchronise.
      The host side is the reference's algorithm as it runs it (features/hac.py:68-97: scipy's vq, np.linalg.svd of the members,
      kmeans2 of 10 iterations), float64.  A whole host build takes minutes, so by default its rounds are SAMPLED: one round
      timed at each of five codebook sizes spread over 1 ... K - 1, the build estimated as (K - 1) x their mean (a round's cost
      grows linearly with the codebook) and labelled an estimate; `--host-full` runs every round.
  (b) one 10-iteration Lloyd call against the labels-and-counts call (n_iter = 0) on the same (T, K, d): medians of `--runs` runs
      after a warm-up.  (10-iteration time / 10) - (n_iter = 0 time) is what the accumulation and the reduction add per
      iteration.
  (c) the assignment pass (the n_iter = 0 call: k_km_assign without sums, k_km_update for the counts) against the bounds: its
      separately rounded fp64 instructions -- 3 T K d: a difference, a product and a sum per element -- against the vector
      pipe's 39.3 T instructions/s (the 78.6 TFLOP/s fp64 vector peak counts a fused multiply-add as two), and its bytes
      (frames read once, labels written) against the 6.29 TB/s a streaming copy reaches.

Each case runs in a child process of its own under its own time limit; a case that fails or overruns ends the script.  No bar:
the file records what was seen.

    python scripts/kmeans_timing.py [--runs 7] [--host-full]          # writes profiles/kmeans_timing.txt
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
T = 800000
CASES = (('build_13', 500), ('build_39', 500), ('lloyd', 300))        # (name, the child's time limit in seconds)
FP64_INSTR_PEAK, STREAM_PEAK = 39.3e12, 6.29e12


def frames(d, seed=7):
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(150, d))
    return centres[rng.integers(0, 150, T)] + 0.35 * rng.normal(size=(T, d))


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def host_round(X, centroids):
    """One round of the reference's loop (features/hac.py:80-96) with scipy, restated: its time and the new codebook."""
    from scipy.cluster.vq import kmeans2, vq
    t0 = time.perf_counter()
    quantized, _ = vq(X, centroids)
    counts = np.bincount(quantized, minlength=centroids.shape[0])
    h = counts.argmax()
    u, s, v = np.linalg.svd(X[(quantized == h).nonzero()[0], :], full_matrices=False)
    p = v[0, :] * np.sqrt(s[0])
    centroids = np.vstack([centroids[:h, :], centroids[h + 1:, :], centroids[h] + 0.01 * p, centroids[h] - 0.01 * p])
    centroids, _ = kmeans2(X, centroids, minit='matrix')
    return time.perf_counter() - t0, centroids


def run_build(d, K, host_full):
    import torch
    from multimodal_amd import _native
    from multimodal_amd.features import codebook as cbk
    X = frames(d)
    print('build case: iterative_kmeans to K = %d on %d x %d frames (device tensors resident)' % (K, T, d), flush=True)
    books = {}
    for name, dt in (('f64', np.float64), ('f32', np.float32)):
        dX = torch.from_numpy(X.astype(dt)).to('cuda')
        wall(lambda: cbk.iterative_kmeans(dX, 3, output='device'))             # the warm-up
        t, book = wall(lambda: cbk.iterative_kmeans(dX, K, output='device'))
        books[name] = (t, book.cpu().numpy())
        print('%-72s %9.3f s  (once; %d rounds, %.2f ms per round)' % ('device, %s' % name, t, K - 1, 1e3 * t / (K - 1)), flush=True)
        del dX
    if host_full:
        cb, t_host = X.mean(axis=0)[np.newaxis, :], 0.0
        while cb.shape[0] < K:
            t, cb = host_round(X, cb)
            t_host += t
        what = 'host, f64: scipy vq / svd / kmeans2, every round'
    else:
        sizes = sorted(set(int(round(v)) for v in np.linspace(1, K - 1, 5)))
        book, seen = books['f64'][1], []
        for k in sizes:                        # a codebook of k rows as the build had it: the first k rows of the final one
            t, _ = host_round(X, book[:k].copy())
            seen.append(t)
            print('    host round at a codebook of %3d rows: %.3f s' % (k, t), flush=True)
        t_host = (K - 1) * float(np.mean(seen))
        what = 'host, f64: scipy vq / svd / kmeans2, ESTIMATE (K - 1) x mean of %d sampled rounds' % len(sizes)
    print('%-72s %9.3f s' % (what, t_host), flush=True)
    for name in ('f64', 'f32'):
        print('    host / device (%s): %.0f x' % (name, t_host / books[name][0]), flush=True)
    print('    device: %s' % _native.device_info(0)['arch'], flush=True)
    return 0


def run_lloyd(runs):
    import torch
    from multimodal_amd import _native
    line = lambda what, ts: '%-72s %9.3f ms  (%.3f ... %.3f)' % (what, 1e3 * float(np.median(ts)), 1e3 * min(ts), 1e3 * max(ts))
    for d, K in ((13, 150), (39, 100), (13, 1000)):
        X = frames(d)
        rng = np.random.default_rng(1)
        init = X[rng.choice(T, K, replace=False)]
        for name, dt, el in (('f64', np.float64, 8), ('f32', np.float32, 4)):
            dX = torch.from_numpy(X.astype(dt)).to('cuda')
            first = torch.from_numpy(init.astype(dt)).to('cuda')
            wb = _native.kmeans_work_bytes(T, d, K)
            work = torch.empty(wb, dtype=torch.uint8, device='cuda')
            labels, counts = torch.zeros(T, dtype=torch.int32, device='cuda'), torch.zeros(K, dtype=torch.int64, device='cuda')

            def call(n_iter):
                cb = first.clone()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _native.kmeans_device(dX.data_ptr(), d, T, d, cb.data_ptr(), d, K, n_iter, work.data_ptr(), wb, labels.data_ptr(),
                                      counts.data_ptr(), f64=dt == np.float64)
                torch.cuda.synchronize()
                return time.perf_counter() - t0
            call(0), call(10)
            t0 = [call(0) for _ in range(runs)]
            t10 = [call(10) for _ in range(runs)]
            m0, m10 = float(np.median(t0)), float(np.median(t10))
            print('Lloyd case: T = %d, d = %d, K = %d, %s; workspace %.1f MB against %.1f MB of frames'
                  % (T, d, K, name, wb / 1e6, T * d * el / 1e6), flush=True)
            print(line('    labels and counts alone (n_iter = 0: 2 launches)', t0), flush=True)
            print(line('    10 Lloyd iterations (20 launches)', t10), flush=True)
            print('    per iteration %.3f ms: the sums and their reduction add %.3f ms (%.0f %% of the assignment)'
                  % (1e2 * m10, 1e3 * (m10 / 10 - m0), 100 * (m10 / 10 - m0) / m0), flush=True)
            instr, nbytes = 3.0 * T * K * d, T * d * el + 4.0 * T
            print('    assignment: %.2f T fp64 instructions/s = %.0f %% of the vector pipe; %.3f TB/s = %.1f %% of the stream rate: %s binds'
                  % (instr / m0 / 1e12, 100 * instr / m0 / FP64_INSTR_PEAK, nbytes / m0 / 1e12, 100 * nbytes / m0 / STREAM_PEAK,
                     'arithmetic' if instr / FP64_INSTR_PEAK > nbytes / STREAM_PEAK else 'memory'), flush=True)
            del dX
    print('    device: %s' % _native.device_info(0)['arch'], flush=True)
    return 0


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--runs', type=int, default=7)
    p.add_argument('--host-full', action='store_true')
    p.add_argument('--case', choices=[c for c, _ in CASES])
    args = p.parse_args()
    if args.case:
        sys.exit(run_lloyd(args.runs) if args.case == 'lloyd' else
                 run_build(13, 150, args.host_full) if args.case == 'build_13' else run_build(39, 100, args.host_full))
    out = os.path.join(ROOT, 'profiles', 'kmeans_timing.txt')
    text = ['# scripts/kmeans_timing.py --runs %d%s: wall time on the host, each run ending in a synchronise; (b), (c): medians of '
            '%d runs after one warm-up, min ... max' % (args.runs, ' --host-full' if args.host_full else '', args.runs)]
    status = 0
    for case, limit in CASES:
        cmd = ['timeout', '-k', '10', str(limit * (6 if args.host_full else 1)), sys.executable, os.path.abspath(__file__), '--case',
               case, '--runs', str(args.runs)] + (['--host-full'] if args.host_full else [])
        child = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, cwd=ROOT)
        for said in child.stdout:                      # (passed on as it comes: a long case is not a silent one)
            print(said.rstrip(), flush=True)
            text.append(said.rstrip())
        status = child.wait()
        if status != 0:
            text.append('# the %s case ended with status %d; nothing more was started' % (case, status))
            print(text[-1], flush=True)
            break
    with open(out, 'w') as fh:
        fh.write('\n'.join(text) + '\n')
    sys.exit(status)


if __name__ == '__main__':
    main()
