#!/usr/bin/env python3
"""What the atom x label information matrix costs, and what it replaces.

  * shape 1, the experiment's scale: 8 runs of 1000 x 50 coefficients, L = 10 labels, B = 10 bins, f64 -- one
    klnmf_information_many_device call for all runs against the path that existed before it: download the eight matrices and run
    the numpy restatement (np.histogram per atom and label, then the table formula; tests/information_cases.py);
  * shape 2, the benchmark's scale: one job of 1M x 200 in f64 and in f32, L = 50, B = 10 -- the wall time of the call and the
    fraction of the HBM stream rate (6.3 TB/s, a plain read) on the 2 * n * k * element-size bytes its two passes must read.

After one warm-up every arm is timed once per segment; the lines give the median of the segments with min ... max.  No bar.

    python scripts/information_timing.py [--segments 7] > profiles/information_timing.txt
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import information_cases as ic  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument('--segments', type=int, default=7)
p.add_argument('--rows', type=int, default=1000000)
p.add_argument('--skip-small', action='store_true', help='shape 2 alone (for a kernel trace of the large shape)')
args = p.parse_args()

import torch  # noqa: E402
from multimodal_amd import _native  # noqa: E402

STREAM = 6.3e12          # bytes / s: the measured rate of a plain read of HBM on this device class
dev = torch.device('cuda', 0)


def line(what, times):
    return '%-66s %9.5f s  (%.5f ... %.5f)' % (what, float(np.median(times)), min(times), max(times))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def many(mats, labs, L, B, f64):
    jobs = [(m.data_ptr(), m.stride(0), l.data_ptr(), m.shape[0], m.shape[1]) for m, l in zip(mats, labs)]
    atoms = sum(m.shape[1] for m in mats)
    nbytes = _native.information_work_bytes(len(jobs), atoms, L, B)
    info = torch.empty((atoms * L,), dtype=torch.float64, device=dev)
    work = torch.empty((nbytes,), dtype=torch.uint8, device=dev)

    def call():
        _native.information_many_device(jobs, L, B, info.data_ptr(), None, work.data_ptr(), nbytes, f64=f64)
        return info.cpu().numpy()
    return call


# ---- shape 1 ---------------------------------------------------------------------------------------------------------------------------
def shape_1():
    RUNS, N, K, L, B = 8, 1000, 50, 10, 10
    host = [ic.coefficients(100 + r, N, K) for r in range(RUNS)]
    host_labels = [ic.labels_of(100 + r, N, L) for r in range(RUNS)]
    mats = [torch.from_numpy(m).to(dev) for m in host]
    labs = [torch.from_numpy(l).to(dev) for l in host_labels]
    call = many(mats, labs, L, B, True)

    def numpy_path():
        return [ic.reference_information(m.cpu().numpy(), l, L, B)[1] for m, l in zip(mats, host_labels)]

    flat, want = call(), numpy_path()                                 # the warm-up, and the same matrices
    worst = max(float(np.max(np.abs(flat[r * K * L:(r + 1) * K * L].reshape(L, K) - want[r]))) for r in range(RUNS))
    print('shape 1: %d runs of %d x %d, L = %d, B = %d, f64; %d segments after one warm-up; worst |device - numpy| = %.2e'
          % (RUNS, N, K, L, B, args.segments, worst), flush=True)
    times = {'device': [], 'numpy': []}
    for _segment in range(args.segments):
        times['device'].append(wall(call))
        times['numpy'].append(wall(numpy_path))
    print(line('1 x klnmf_information_many_device (8 jobs) + the copy of the matrices', times['device']), flush=True)
    print(line('download + numpy restatement (8 x 50 x 10 np.histogram)', times['numpy']), flush=True)


if not args.skip_small:
    shape_1()

# ---- shape 2 ---------------------------------------------------------------------------------------------------------------------------
N, K, L, B = args.rows, 200, 50, 10
gen = torch.Generator(device=dev)
gen.manual_seed(5)
big = -torch.log(torch.rand((N, K), dtype=torch.float64, device=dev, generator=gen).clamp_(min=1e-300)) * 2.0
big *= (torch.rand((N, K), dtype=torch.float64, device=dev, generator=gen) >= 0.6)          # 60 % exact zeros
big_labels = torch.randint(0, L, (N,), dtype=torch.int32, device=dev, generator=gen)
print('shape 2: 1 job of %d x %d, L = %d, B = %d (counter route %s, atom tile %d); %d segments after one warm-up'
      % ((N, K, L, B) + _native.information_route(L, B) + (args.segments,)), flush=True)
for f64 in (True, False):
    m = big if f64 else big.to(torch.float32)
    call = many([m], [big_labels], L, B, f64)
    info = call()
    assert np.isfinite(info).all() and info.min() >= -1e-12
    t = [wall(call) for _segment in range(args.segments)]
    must_read = 2.0 * N * K * (8 if f64 else 4)
    med = float(np.median(t))
    print(line('klnmf_information_many_device, %s' % ('f64' if f64 else 'f32'), t), flush=True)
    print('    %.3f GB to read in two passes -> %.2f TB/s = %.0f %% of the %.1f TB/s stream rate'
          % (must_read / 1e9, must_read / med / 1e12, 100.0 * must_read / med / STREAM, STREAM / 1e12), flush=True)
    del m
print('device: %s' % _native.device_info(0)['arch'])
