#!/usr/bin/env python3
"""A group of N contexts on ONE GPU (devices = [0] * N: klnmf_group_run) at configuration 4's shape -- 1 000 000 x 4096, k = 200,
precision 'f16' -- for N = 1, 2, 4, 8: what an N-GPU node's loop would enqueue, every shard sharing one chip.

Per N it reports
  * ms per iteration: the slope between a short and a long loop, each a fresh fit from H0 (the loop's entry, its first two
    16-bit iterations, result fetch and replica check cancel), the median of --repeats pairs after a long warm-up loop;
  * the host's enqueue time per iteration while the GPU is busy (klnmf_group_enqueue_time: the median over the long loop's
    iterations -- the host runs ahead of a 4.6 ms iteration, so every iteration's enqueue happens with the GPU busy);
  * the sum over the shards of one context's time at the shard's size (profiles/r06_shards_of_c4.txt), which is what the
    group on ONE chip is to be compared with: N shards of n / N rows cost more than one context of n rows before any exchange.
The exchange kernels' own time comes from a separate run under rocprofv3 (--mode trace: a few iterations, nothing timed here):

    python scripts/group_timing.py [--shards 1,2,4,8] [--short 10] [--long 50] [--data host|device]
    rocprofv3 --kernel-trace --stats -d OUT -o group -- python scripts/group_timing.py --mode trace --shards 8
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

# one context at a shard's size, native collective branch (profiles/r06_shards_of_c4.txt): rows -> ms per iteration
R06_SHARD_MS = {1000000: 4.5987, 500000: 2.3377, 250000: 1.2024, 125000: 0.6444}


def build_group_host(n, f, k, cap, shards, seed=1234):
    """The same with bench.py's default data (`--data host`: the seeded RandomState row blocks of multimodal_amd/synthetic.py,
    the data of bench.py's headline, whose fit stays in the fp8 regime): every shard uploads its global rows."""
    from multimodal_amd import _native, synthetic
    from multimodal_amd.distributed import row_partition
    vmax = synthetic.for_each_block(seed, 0, n, n, f, k, None)
    H0 = synthetic.H0_of(seed, f, k)
    ctxs = []
    for r0, r1 in row_partition(n, shards):
        c = _native.Context('f16', device=0)
        c.set_problem(r1 - r0, f, k, cap)
        c.set_v_max(vmax)
        synthetic.for_each_block(seed, r0, r1, n, f, k, lambda lo, arr, c=c: c.upload_V(arr, row0=lo, col0=0))
        c.set_H(H0)
        c.init_W()
        ctxs.append(c)
    return ctxs


def build_group(torch, n, f, k, cap, shards, seed=1234, block=8192):
    """N contexts on device 0 holding the row shards of one seeded synthetic V -- rank 0's matrix of `bench.py --data device`
    (SURVEY 8d's family V = Wt.Ht / k + 0.05 U, generated block by block on the GPU with one generator stream), so that a shard
    of R rows holds what profiles/r06_shards_of_c4.txt timed at R rows; one storage factor from the global maximum, the same H0
    on every shard, W0 = V.H0^T."""
    from multimodal_amd import _native, synthetic
    from multimodal_amd.distributed import row_partition
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    Ht = torch.randn((k, f), device=dev, generator=g).square_().mul_(0.5)
    g.manual_seed(seed + 1000)

    def block_of(rows):
        Wt = torch.rand((rows, k), device=dev, generator=g).neg_().add_(1.0).log_().neg_()
        Vb = torch.rand((rows, f), device=dev, generator=g).mul_(0.05)
        return Vb.addmm_(Wt, Ht, alpha=1.0 / k)
    state = g.get_state()
    vmax = 0.0
    for b0 in range(0, n, block):
        vmax = max(vmax, float(block_of(min(block, n - b0)).max().item()))
    g.set_state(state)
    H0 = synthetic.H0_of(seed, f, k)
    ctxs = []
    for r0, r1 in row_partition(n, shards):
        c = _native.Context('f16', device=0)
        c.set_problem(r1 - r0, f, k, cap)
        c.set_v_max(vmax)
        ctxs.append((c, r0, r1))
    for b0 in range(0, n, block):
        Vb = block_of(min(block, n - b0))
        for c, r0, r1 in ctxs:
            lo, hi = max(b0, r0), min(b0 + Vb.shape[0], r1)
            if lo < hi:
                part = Vb[lo - b0:hi - b0].contiguous()
                c.upload_V_device(part.data_ptr(), hi - lo, f, f, row0=lo - r0, col0=0)
        torch.cuda.synchronize()
    for c, _, _ in ctxs:
        c.set_H(H0)
        c.init_W()
    return [c for c, _, _ in ctxs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shards', default='1,2,4,8')
    ap.add_argument('--n', type=int, default=1000000)
    ap.add_argument('--f', type=int, default=4096)
    ap.add_argument('--k', type=int, default=200)
    ap.add_argument('--short', type=int, default=10)
    ap.add_argument('--long', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--mode', choices=['time', 'trace'], default='time')
    ap.add_argument('--data', choices=['host', 'device'], default='host')
    ap.add_argument('--json', default=None, help='write the results here too')
    a = ap.parse_args()
    import torch
    from multimodal_amd import _native
    out = []
    for N in [int(s) for s in a.shards.split(',')]:
        if a.data == 'host':
            ctxs = build_group_host(a.n, a.f, a.k, max(a.short, a.long), N)
        else:
            ctxs = build_group(torch, a.n, a.f, a.k, max(a.short, a.long), N)
        from multimodal_amd import synthetic
        H0 = synthetic.H0_of(1234, a.f, a.k)
        try:
            with _native.Group(ctxs) as g:
                if a.mode == 'trace':
                    g.run(a.n, a.short, True, 0.0)
                    continue
                def fresh():
                    # every timed loop is a fresh fit (as bench.py's segments: H0, W0 = V.H0^T), so that it runs the fp8 regime
                    # of a fit's early iterations and not whatever a long-running fit has reached
                    for c in ctxs:
                        c.set_H(H0)
                        c.init_W()
                    for c in ctxs:
                        c.synchronize()
                # warm-up: a whole long loop (code objects, pinned poll buffers, the monitor's first checks)
                fresh()
                g.run(a.n, a.long, True, 0.0)
                slopes = []
                for _ in range(a.repeats):
                    fresh()
                    t0 = time.perf_counter()
                    g.run(a.n, a.short, True, 0.0)
                    t1 = time.perf_counter()
                    fresh()
                    t1b = time.perf_counter()
                    e_long, _, _ = g.run(a.n, a.long, True, 0.0)
                    t2 = time.perf_counter()
                    slopes.append(((t2 - t1b) - (t1 - t0)) / (a.long - a.short) * 1e3)
                timed, enq_med, enq_max = g.enqueue_time()         # (of the last long loop)
                rep = ctxs[0].fp8_report()
        finally:
            for c in ctxs:
                c.close()
        ms = float(np.median(slopes))
        rows = a.n // N
        ref = R06_SHARD_MS.get(rows) if a.n == 1000000 and a.f == 4096 and a.k == 200 else None
        r = {'shards': N, 'rows_per_shard': rows, 'ms_per_iter': round(ms, 4),
             'ms_per_iter_repeats': [round(v, 4) for v in slopes],
             'enqueue_ms_median': round(enq_med, 4), 'enqueue_ms_max': round(enq_max, 4), 'enqueue_iters': timed,
             'sum_of_shard_ms_r06': round(N * ref, 4) if ref else None,
             'vs_sum_of_shards': round(ms / (N * ref), 4) if ref else None,
             'fp8': {key: rep[key] for key in ('allowed', 'tile_iterations', 'column_pass_iterations', 'gave_up', 'monitor_trips',
                                               'ratio_unfixed')},
             'final_loss': e_long[-1], 'finite': bool(np.all(np.isfinite(e_long)))}
        print(json.dumps(r), flush=True)
        out.append(r)
    if a.json and out:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
