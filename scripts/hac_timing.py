#!/usr/bin/env python3
"""What the windowed co-occurrence histograms cost on the device, against the host twin on the same machine.

  * the sliding case: three streams of d = 13, codebooks of 150 / 150 / 100 units, lags [5, 2], T = 60 000 frames, 50-frame
    windows every 10 frames (5 996 windows; F = 110 000 columns) -- samples/image_sound_eval_sliding.py's shape;
  * the whole-utterance case: 2 000 consecutive windows of 200 to 600 frames over the same codebooks.

Per case: `features.hac.windowed_hac(..., output='device')` timed with a host clock that ends in a synchronise, the median of
`--runs` runs after one warm-up (min ... max), once from host arrays (the upload of the streams counted) and once from tensors
already on the device (not counted); and the host twin as the reference runs it -- `hac_from_streams` on every window's slice
(vq, bincount) in one process, each row made sparse and the rows stacked -- timed once.  The two matrices are compared for
equality.  No bar: the file records what was seen.

Each case runs in a child process of its own under its own time limit; a case that fails or overruns ends the script.

    python scripts/hac_timing.py [--runs 7]          # writes profiles/hac_timing.txt
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = (('sliding', 300), ('utterance', 600))        # (name, the child's time limit in seconds)
KS, D, LAGS = (150, 150, 100), 13, [5, 2]


def inputs(case):
    rng = np.random.default_rng(7)
    if case == 'sliding':
        T = 60000
        from multimodal_amd.features.hac import frame_windows
        windows = frame_windows(T, 50, 10)
    else:
        lengths = rng.integers(200, 601, 2000)
        ends = np.cumsum(lengths)
        T = int(ends[-1])
        windows = [(int(e - n), int(e)) for e, n in zip(ends, lengths)]
    codebooks = [rng.normal(size=(K, D)) for K in KS]
    streams = [c[np.repeat(rng.integers(0, len(c), (T + 2) // 3), 3)[:T]] + 0.35 * rng.normal(size=(T, D)) for c in codebooks]
    return streams, codebooks, windows, T


def line(what, times):
    return '%-72s %9.5f s  (%.5f ... %.5f)' % (what, float(np.median(times)), min(times), max(times))


def run_case(case, runs):
    import scipy.sparse as sp
    import torch
    from multimodal_amd import _native
    from multimodal_amd.features import hac
    streams, codebooks, windows, T = inputs(case)
    lengths = [b - a for a, b in windows]
    routes = sorted(set(_native.hac_route(n - l, K) for n in lengths for l in LAGS for K in KS))
    print('%s case: T = %d frames, %d windows of %d ... %d frames, K = %s, d = %d, lags %s, f64; routes %s'
          % (case, T, len(windows), min(lengths), max(lengths), list(KS), D, LAGS, routes), flush=True)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    from_host = lambda: hac.windowed_hac(streams, codebooks, windows, lags=LAGS, output='device')
    dev_streams = [torch.from_numpy(x).to('cuda') for x in streams]
    dev_codebooks = [torch.from_numpy(c).to('cuda') for c in codebooks]
    from_device = lambda: hac.windowed_hac(dev_streams, dev_codebooks, windows, lags=LAGS, output='device')
    _, rows = wall(from_host)                          # the warm-up
    print('    the matrix: %d x %d, nnz = %d (%.1f per row), %.1f MB on the device'
          % (rows.shape + (rows.nnz, rows.nnz / max(1, rows.shape[0]), rows.nbytes() / 1e6)), flush=True)
    print(line('windowed_hac from host arrays (upload of the streams counted)', [wall(from_host)[0] for _ in range(runs)]), flush=True)
    wall(from_device)
    print(line('windowed_hac from device tensors (no upload of the streams)', [wall(from_device)[0] for _ in range(runs)]), flush=True)

    def twin():
        vectors = [sp.csr_matrix(hac.hac_from_streams([x[a:b] for x in streams], codebooks, LAGS)) for a, b in windows]
        return sp.vstack(vectors, format='csr')
    t0 = time.perf_counter()
    X = twin()
    t_twin = time.perf_counter() - t0
    print('%-72s %9.5f s  (once)' % ('host twin: hac_from_streams per window, sparse rows, sp.vstack (one process)', t_twin), flush=True)
    got = rows.to_scipy()
    same = (got.shape == X.shape and np.array_equal(got.indptr, X.indptr) and np.array_equal(got.indices, X.indices)
            and np.array_equal(got.data, X.data))
    print('    device matrix == host twin: %s' % same, flush=True)
    print('    device: %s' % _native.device_info(0)['arch'], flush=True)
    return 0 if same else 1


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--runs', type=int, default=7)
    p.add_argument('--case', choices=[c for c, _ in CASES])
    args = p.parse_args()
    if args.case:
        sys.exit(run_case(args.case, args.runs))
    out = os.path.join(ROOT, 'profiles', 'hac_timing.txt')
    text = ['# scripts/hac_timing.py --runs %d: medians of %d runs after one warm-up, min ... max; wall time on the host, each run '
            'ending in a synchronise' % (args.runs, args.runs)]
    status = 0
    for case, limit in CASES:
        cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--case', case, '--runs', str(args.runs)]
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
