"""What one experiment call pays to set a masked problem up: the rows of the modalities and of the presence mask gathered on the
device from a DeviceDataset(presence=[...]) (klnmf_upload_V_device_rows_dt + klnmf_upload_presence_device_rows) against the host path
it replaces (slice the modalities and the mask on the host, Context.upload_blocks + Context.upload_presence: what
MultimodalLearner.train(host slices, weights=[...]) does per call).  2000 x 4096 in two modalities, k = 200, an 80 % random row subset.

    python3 scripts/device_presence_timing.py [--precision f64|f32] [--out profiles/device_presence_timing]

Timed, host clock, each ending in a device synchronise: set problem + V rows + mask.  The two paths alternate in one process, 2
warm-up rounds, then 7 timed ones: median with min .. max.  Both problems are then compared through init_W and one step_Q (bit
identity; in f32 the resident fp32 blocks are not the host path's bits and the comparison is reported, not required).  Writes
<out>.json and <out>.txt."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def stats(v):
    v = sorted(v)
    return {'median_ms': 1e3 * v[len(v) // 2], 'min_ms': 1e3 * v[0], 'max_ms': 1e3 * v[-1], 'samples': len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=2000)
    ap.add_argument('--f', type=int, default=4096)
    ap.add_argument('--k', type=int, default=200)
    ap.add_argument('--subset', type=float, default=0.8)
    ap.add_argument('--precision', default='f64', choices=['f64', 'f32'])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'device_presence_timing'))
    args = ap.parse_args()
    import torch
    from multimodal_amd import _native
    from multimodal_amd.device_data import DeviceDataset
    from oracle import klnmf_oracle as orc

    n, f, k = args.n, args.f, args.k
    rs = np.random.RandomState(0)
    half = f // 2
    dims = [half, f - half]
    bounds = [0, half, f]
    mods = [rs.gamma(1.0, 1.0, (n, d)) for d in dims]
    P = np.ones((n, 2))
    P[:, 1] = (rs.random_sample(n) > 0.4).astype(np.float64)
    mods[1] = mods[1] * P[:, 1:]
    coefs = [1.0, 0.5]
    rows = rs.permutation(n)[:int(round(args.subset * n))]
    ds = DeviceDataset(mods, presence=[None, P[:, 1]])
    which = [0, 1]
    for w in which:
        ds.source(w, args.precision)           # (the float64 copies of the f64 mode are made on first use: not a call's cost)
    H0 = orc.synthetic_H0(3, f, k)

    def device_setup(ctx):
        t0 = time.perf_counter()
        upload, r = ds._uploader(which, rows, coefs, masked=True)
        ctx.set_problem(r, f, k, 1)
        upload(ctx)
        ctx.synchronize()
        return time.perf_counter() - t0, 0.0

    def host_setup(ctx):
        t0 = time.perf_counter()
        blocks = [m[rows] for m in mods]
        Pr = P[rows]
        t1 = time.perf_counter()
        ctx.set_problem(rows.size, f, k, 1)
        ctx.upload_blocks(blocks, coefs)
        ctx.upload_presence(Pr, bounds)
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
        q = []
        for c in (cd, ch):
            assert c.presence() == 2
            c.set_H(H0)
            c.init_W()
            c.step_Q()
            q.append((c.get_W(), c.get_Q()))
        same = bool(np.array_equal(q[0][0], q[1][0]) and np.array_equal(q[0][1], q[1][1]))
    torch.cuda.synchronize()
    out = {
        'what': 'problem set-up of one masked call: device gather of V rows and mask rows vs host slices + upload_blocks + upload_presence '
                '(host clock, each ending in a device synchronise)',
        'shape': {'n': n, 'f': f, 'k': k, 'modalities': dims, 'rows_selected': int(rows.size), 'precision': args.precision},
        'method': '%d warm-up rounds, then %d rounds of (device, host) alternating in one process: median, min .. max' % (args.warmup, args.rounds),
        'device_gather': stats(dev_t),
        'host_path': dict(stats(host_t), of_which_host_slices=stats(slice_t)),
        'speedup_median': sorted(host_t)[len(host_t) // 2] / sorted(dev_t)[len(dev_t) // 2],
        'same_problem_bit_for_bit': same,
        'bytes_per_call_over_the_bus': {'device_gather': int(rows.size) * 8, 'host_path': int(rows.size) * (f + 2) * 8},
        'resident_mask_bytes': 8 * n * 2,
        'device': _native.device_info(0),
    }
    d, h, s = out['device_gather'], out['host_path'], out['host_path']['of_which_host_slices']
    text = ('masked problem set-up of one call, %d of %d rows x %d columns in two modalities, k = %d, %s\n'
            '  device gather (V rows + klnmf_upload_presence_device_rows)   median %8.3f ms   (min %.3f .. max %.3f, %d rounds)\n'
            '  host path (slices + upload_blocks + upload_presence)         median %8.3f ms   (min %.3f .. max %.3f)\n'
            '    of which slicing on the host                               median %8.3f ms   (min %.3f .. max %.3f)\n'
            '  host / device                                                %.1f x\n'
            '  same problem bit for bit (W0, masked ratio)                  %s\n'
            '  per call over the bus: %d bytes of row indices against %d bytes of float64 rows and mask\n'
            % (rows.size, n, f, k, args.precision, d['median_ms'], d['min_ms'], d['max_ms'], d['samples'], h['median_ms'], h['min_ms'],
               h['max_ms'], s['median_ms'], s['min_ms'], s['max_ms'], out['speedup_median'], same, rows.size * 8, rows.size * (f + 2) * 8))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out + '.json', 'w'), indent=1)
    open(args.out + '.txt', 'w').write(text)
    sys.stdout.write(text)
    if args.precision == 'f64' and not same:
        sys.exit(1)


if __name__ == '__main__':
    main()
