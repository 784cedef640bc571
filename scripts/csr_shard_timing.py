#!/usr/bin/env python3
"""CSR input at scripts/bench_sparse.py's shape (20 000 x 110 000, 0.5 % stored, k = 50): the upload with the CSC order built on
the device against the host sort it replaces, and a group of CSR contexts on ONE GPU (devices = [0] * N).

    python scripts/csr_shard_timing.py --mode upload [--repeats 5]       # set_problem_sparse, host clock, f64 and f32
    python scripts/csr_shard_timing.py --mode group [--shards 1,2,4]     # klnmf_group_run over csr_row_partition shards
    rocprofv3 --kernel-trace --stats -d OUT -o csc -- python scripts/csr_shard_timing.py --mode trace

upload  the median of --repeats (problem set + structure and values uploaded + synchronised) per path:
          'device'  Context.set_problem_sparse (klnmf_upload_csr_rows: the CSC order built by csrc/csc.hip.h)
          'host'    the previous path: np.argsort(indices, kind='stable') and the CSC arrays on the host, klnmf_upload_csr
        The host sort is also timed alone.
trace   one device-path upload per precision, nothing timed (the kernels' times come from rocprofv3).
group   per N: ms per iteration of klnmf_group_run as the slope between a --short and a --long loop (fresh fits from H0; the
        loop's entry, result fetch and replica check cancel), median of --repeats; the same slope for one context holding each
        shard alone, summed over the shards (what N shards on one chip are to be compared with); the numerator bytes the
        exchange moves per shard and iteration (k x f x 8 in f64).  One GPU shows the group's overhead, not a speedup.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402


def bench_matrix(n, f, density):
    """scripts/bench_sparse.py's matrix: `per_row` uniformly random columns per row (RandomState(0)), Gamma(1, 1) values."""
    rs = np.random.RandomState(0)
    per_row = max(1, int(round(density * f)))
    cols = np.sort(rs.randint(0, f, size=(n, per_row)), axis=1)
    X = sp.csr_matrix((rs.gamma(1.0, 1.0, n * per_row), cols.ravel(), np.arange(0, n * per_row + 1, per_row)), shape=(n, f))
    X.sum_duplicates()
    X.sort_indices()
    return X


def host_order_upload(ctx, X, k, cap):
    """The previous upload path: the CSC order sorted on the host, klnmf_upload_csr."""
    from multimodal_amd import _native
    X = sp.csr_matrix(X, copy=True)
    X.eliminate_zeros()
    X.sort_indices()
    n, f = X.shape
    dt = np.float32 if X.dtype == np.float32 else np.float64
    _native._check(ctx._lib.klnmf_set_problem_sparse(ctx._h, n, f, k, cap, int(X.nnz)))
    indptr = np.ascontiguousarray(X.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(X.indices, dtype=np.int64)
    data = np.ascontiguousarray(X.data, dtype=dt)
    perm = np.argsort(indices, kind='stable').astype(np.int64)
    rows_of = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    csc_rows = np.ascontiguousarray(rows_of[perm])
    csc_indptr = np.zeros(f + 1, dtype=np.int64)
    np.cumsum(np.bincount(indices, minlength=f), out=csc_indptr[1:])
    p = lambda a: a.ctypes.data_as(_native._c.c_void_p)
    _native._check(ctx._lib.klnmf_upload_csr(ctx._h, _native.DT_F32 if dt == np.float32 else _native.DT_F64, p(indptr), p(indices),
                                             p(data), p(csc_indptr), p(csc_rows), p(perm)))


def mode_upload(X, k, repeats):
    from multimodal_amd import _native
    out = []
    for prec in ('f64', 'f32'):
        Xp = X.astype(np.float32) if prec == 'f32' else X
        with _native.Context(prec, device=0) as c:
            for path in ('device', 'host'):
                ts = []
                for _ in range(repeats + 1):
                    c.synchronize()
                    t0 = time.perf_counter()
                    if path == 'device':
                        c.set_problem_sparse(Xp, k, 10)
                    else:
                        host_order_upload(c, Xp, k, 10)
                    c.synchronize()
                    ts.append(time.perf_counter() - t0)
                ts = ts[1:]                         # (the first call also warms the allocator's cache)
                out.append({'precision': prec, 'path': path, 'median_s': float(np.median(ts)), 'all_s': ts})
    idx = np.ascontiguousarray(X.indices, dtype=np.int64)
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        np.argsort(idx, kind='stable')
        ts.append(time.perf_counter() - t0)
    out.append({'what': "np.argsort(indices, kind='stable') alone", 'median_s': float(np.median(ts)), 'all_s': ts})
    return out


def loop_ms(run, short, long_, repeats):
    """Slope between a short and a long fresh loop, median of `repeats` pairs (after one warm-up pair)."""
    run(short)
    run(long_)
    s = []
    for _ in range(repeats):
        a = run(short)
        b = run(long_)
        s.append((b - a) / (long_ - short) * 1e3)
    return float(np.median(s))


def mode_group(X, k, shards, short, long_, repeats):
    from multimodal_amd import _native
    from multimodal_amd.distributed import csr_row_partition
    from oracle import klnmf_oracle as orc
    n, f = X.shape
    H0 = orc.synthetic_H0(3, f, k)
    cap = long_
    single = {}

    def single_ms(r0, r1):
        if (r0, r1) not in single:
            with _native.Context('f64', device=0) as c:
                c.set_problem_sparse(X[r0:r1], k, cap)

                def run(it):
                    c.set_H(H0)
                    c.init_W()
                    c.synchronize()
                    t0 = time.perf_counter()
                    c.run(it, True, 0.0)
                    return time.perf_counter() - t0
                single[(r0, r1)] = loop_ms(run, short, long_, repeats)
        return single[(r0, r1)]

    out = []
    for N in shards:
        bounds = csr_row_partition(X.indptr, N)
        ctxs = []
        try:
            for r0, r1 in bounds:
                c = _native.Context('f64', device=0)
                ctxs.append(c)
                c.set_problem_sparse(X[r0:r1], k, cap)
            g = _native.Group(ctxs)

            def run(it):
                for c in ctxs:
                    c.set_H(H0)
                    c.init_W()
                    c.synchronize()
                t0 = time.perf_counter()
                errs, nd, _ = g.run(n, it, True, 0.0)
                assert nd == it
                return time.perf_counter() - t0
            ms = loop_ms(run, short, long_, repeats)
            enq = g.enqueue_time()
            g.close()
        finally:
            for c in ctxs:
                c.close()
        parts = [single_ms(r0, r1) for r0, r1 in bounds]
        r = {'shards': N, 'bounds': bounds, 'nnz': [int(X.indptr[b] - X.indptr[a]) for a, b in bounds],
             'group_ms_per_iteration': ms, 'sum_of_shards_ms': float(sum(parts)), 'shard_ms': parts,
             'ratio': ms / sum(parts), 'enqueue_median_ms': enq[1],
             'numerator_bytes_per_shard_per_iteration': k * f * 8, 'loss_bytes_per_shard_per_iteration': 16}
        out.append(r)
        print(json.dumps(r), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=['upload', 'trace', 'group'], default='upload')
    ap.add_argument('--n', type=int, default=20000)
    ap.add_argument('--f', type=int, default=110000)
    ap.add_argument('--k', type=int, default=50)
    ap.add_argument('--density', type=float, default=0.005)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--shards', default='1,2,4')
    ap.add_argument('--short', type=int, default=10)
    ap.add_argument('--long', type=int, default=50)
    ap.add_argument('--json', default=None, help='write the results here too')
    args = ap.parse_args()
    from multimodal_amd import _native
    X = bench_matrix(args.n, args.f, args.density)
    res = {'shape': [args.n, args.f], 'nnz': int(X.nnz), 'k': args.k, 'device': _native.device_info(0)}
    if args.mode == 'trace':
        for prec in ('f64', 'f32'):
            with _native.Context(prec, device=0) as c:
                c.set_problem_sparse(X.astype(np.float32) if prec == 'f32' else X, args.k, 10)
                c.synchronize()
        return
    if args.mode == 'upload':
        res['upload'] = mode_upload(X, args.k, args.repeats)
    else:
        res['group'] = mode_group(X, args.k, [int(s) for s in args.shards.split(',')], args.short, args.long, args.repeats)
    print(json.dumps(res), flush=True)
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
