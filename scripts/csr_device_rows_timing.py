"""What one experiment call pays to set its CSR problem up: rows gathered on the device from CSR modalities that stay there
(DeviceDataset(keep_sparse=True): klnmf_upload_csr_device_rows, csrc/csrgather.hip.h) against the host path it replaces (slice the
modalities on the host, stack them -- nmf._csr_of --, upload: Context.set_problem_sparse).  Shape of scripts/bench_sparse.py
(20 000 x 110 000, 0.5 % stored) cut into two modalities, an 80 % random row subset (a run's training rows, experiment.py:163-164).

    python3 scripts/csr_device_rows_timing.py [--precision f64|f32] [--out profiles/csr_device_rows_timing]

Timed, host clock, each ending in a device synchronise: the whole set-up of one call (plan / slice, set problem, upload).  The two
paths alternate in one process, 2 warm-up rounds, then 7 timed ones: median with min .. max.  Both problems are then compared
through init_W and one step_Q (bit identity), and the dataset's resident bytes are set against the densified copies
DeviceDataset keeps without keep_sparse.  Writes <out>.json and <out>.txt."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import scipy.sparse as sp


def stats(v):
    v = sorted(v)
    return {'median_ms': 1e3 * v[len(v) // 2], 'min_ms': 1e3 * v[0], 'max_ms': 1e3 * v[-1], 'samples': len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=20000)
    ap.add_argument('--f', type=int, default=110000)
    ap.add_argument('--k', type=int, default=50)
    ap.add_argument('--density', type=float, default=0.005)
    ap.add_argument('--subset', type=float, default=0.8)
    ap.add_argument('--precision', default='f64', choices=['f64', 'f32'])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'csr_device_rows_timing'))
    args = ap.parse_args()
    import torch
    from multimodal_amd import _native
    from multimodal_amd.device_data import DeviceDataset
    from multimodal_amd.lib import nmf
    from oracle import klnmf_oracle as orc

    n, f, k = args.n, args.f, args.k
    rs = np.random.RandomState(0)
    per_row = max(1, int(round(args.density * f)))          # (bench_sparse.py's generator)
    cols = np.sort(rs.randint(0, f, size=(n, per_row)), axis=1)
    X = sp.csr_matrix((rs.gamma(1.0, 1.0, n * per_row), cols.ravel(), np.arange(0, n * per_row + 1, per_row)), shape=(n, f))
    X.sum_duplicates()
    X.sort_indices()
    del cols
    half = f // 2
    mods = [sp.csr_matrix(X[:, :half]), sp.csr_matrix(X[:, half:])]
    coefs = [1.0, 0.5]
    rows = rs.permutation(n)[:int(round(args.subset * n))]
    ds = DeviceDataset(mods, keep_sparse=True)
    which = [0, 1]
    H0 = orc.synthetic_H0(3, f, k)

    def device_setup(ctx):
        t0 = time.perf_counter()
        upload, r, nnz, use_device = ds._sparse_uploader(which, rows, coefs)
        assert use_device
        ctx.set_problem_sparse_shape(r, f, k, 1, nnz)
        upload(ctx)
        ctx.synchronize()
        return time.perf_counter() - t0, 0.0

    def host_setup(ctx):
        t0 = time.perf_counter()
        Xr = nmf._csr_of([m[rows] for m in mods], coefs)
        t1 = time.perf_counter()
        ctx.set_problem_sparse(Xr, k, 1)
        ctx.synchronize()
        return time.perf_counter() - t0, t1 - t0

    dev_t, host_t, slice_t = [], [], []
    with _native.Context(args.precision) as cd, _native.Context(args.precision) as ch:
        for r in range(args.warmup + args.rounds):
            a, _ = device_setup(cd)
            b, s = host_setup(ch)
            if r >= args.warmup:
                dev_t.append(a)
                host_t.append(b)
                slice_t.append(s)
        same = cd.nnz == ch.nnz
        q = []
        for c in (cd, ch):
            c.set_H(H0)
            c.init_W()
            c.step_Q()
            q.append((c.get_W(), c.get_Q_values()))
        same = bool(same and np.array_equal(q[0][0], q[1][0]) and np.array_equal(q[0][1], q[1][1]))
        nnz = int(cd.nnz)
    torch.cuda.synchronize()
    resident = ds.resident_bytes()
    out = {
        'what': 'problem set-up of one call on CSR modalities: device gather vs host slice + upload (host clock, each ending in a device synchronise)',
        'shape': {'n': n, 'f': f, 'k': k, 'stored_entries': int(X.nnz), 'modalities': [m.shape[1] for m in mods],
                  'rows_selected': int(rows.size), 'stored_entries_selected': nnz, 'precision': args.precision},
        'method': '%d warm-up rounds, then %d rounds of (device, host) alternating in one process: median, min .. max' % (args.warmup, args.rounds),
        'device_gather': stats(dev_t),
        'host_path': dict(stats(host_t), of_which_host_slice_and_stack=stats(slice_t)),
        'speedup_median': sorted(host_t)[len(host_t) // 2] / sorted(dev_t)[len(dev_t) // 2],
        'same_problem_bit_for_bit': same,
        'resident_bytes': {'csr_dataset': int(resident), 'dense_fp32_copy': int(n) * int(f) * 4, 'dense_fp64_copy_of_f64_mode': int(n) * int(f) * 8,
                           'bytes_per_call_over_the_bus': int(rows.size) * 8},
        'device': _native.device_info(0),
    }
    d, h, s = out['device_gather'], out['host_path'], out['host_path']['of_which_host_slice_and_stack']
    text = ('CSR problem set-up of one call, %d of %d rows x %d columns in two modalities, %d stored entries selected, %s\n'
            '  device gather (klnmf_upload_csr_device_rows)   median %8.2f ms   (min %.2f .. max %.2f, %d rounds)\n'
            '  host path (slice + stack + upload)             median %8.2f ms   (min %.2f .. max %.2f)\n'
            '    of which slice + stack on the host           median %8.2f ms   (min %.2f .. max %.2f)\n'
            '  host / device                                  %.1f x\n'
            '  same problem bit for bit (nnz, W0, ratio)      %s\n'
            '  resident: CSR dataset %.3f GB; densified fp32 copy %.1f GB (+ %.1f GB fp64 copy in the f64 mode); per call over the bus: %d bytes of row indices\n'
            % (rows.size, n, f, nnz, args.precision, d['median_ms'], d['min_ms'], d['max_ms'], d['samples'], h['median_ms'], h['min_ms'],
               h['max_ms'], s['median_ms'], s['min_ms'], s['max_ms'], out['speedup_median'], same, resident / 1e9, n * f * 4 / 1e9,
               n * f * 8 / 1e9, rows.size * 8))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out + '.json', 'w'), indent=1)
    open(args.out + '.txt', 'w').write(text)
    sys.stdout.write(text)
    if not same:
        sys.exit(1)


if __name__ == '__main__':
    main()
