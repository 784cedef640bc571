#!/usr/bin/env python3
"""What the fused nearest-example search (search='fused') does to a sweep's wall time.

  * the `run_sweep` of DESIGN.md 7g's closing paragraph -- the synthetic two-modality set of scripts/time_experiment_run.py
    (1000 samples, 450 + 2000 columns), k = 50, 8 runs, 50 + 50 iterations, f64 -- with batch=8 and batch=1, search='matrix'
    (the baseline: the existing path, call for call) against search='fused';
  * the search alone: the 48 searches of one run's shapes (100 test rows x 10 examples; 4 comparisons each in d = 50, 450 and
    2000, 4 measures) as 48 x `found_labels` against one `found_labels_many`.

All arms alternate in one process; after one warm-up round every arm is timed once per segment; the lines give the median of the
segments with min ... max.  Acceptance (batch=8): the fused arm's median lies below the matrix arm's fastest segment.

    python scripts/nearest_timing.py [--segments 7] > profiles/nearest_timing.txt
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import golden_inputs as gi  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument('--segments', type=int, default=7)
p.add_argument('--k', type=int, default=50)
p.add_argument('--runs', type=int, default=8)
p.add_argument('--iters', type=int, default=50)
args = p.parse_args()
assert args.segments >= 5

import torch  # noqa: E402
from multimodal_amd import _native  # noqa: E402
from multimodal_amd.device_data import DeviceEvaluation  # noqa: E402
from multimodal_amd.device_experiment import DEVICE_MEASURES, run_sweep  # noqa: E402

DIMS = (450, 2000)
mods = gi.experiment_modalities(21, n_per_label=100, n_labels=10, dims=DIMS)
data, labels = [m[0] for m in mods], mods[0][1]


def line(what, times):
    return '%-58s %8.4f s  (%.4f ... %.4f)' % (what, float(np.median(times)), min(times), max(times))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def sweep(batch, search):
    return run_sweep(data, labels, ['motion', 'sound'], [args.k], args.runs, iter_train=args.iters, iter_test=args.iters, devices=[0],
                     precision='f64', seed=1, batch=batch, search=search)


print('run_sweep: %d samples, modalities %s, k = %d, %d runs, %d + %d iterations, f64; %d segments after one warm-up round'
      % (data[0].shape[0], DIMS, args.k, args.runs, args.iters, args.iters, args.segments), flush=True)
arms = [(8, 'matrix'), (8, 'fused'), (1, 'matrix'), (1, 'fused')]
tables = {arm: sweep(*arm)[0] for arm in arms}                                  # the warm-up round
print('score tables equal: batch=8 %s, batch=1 %s' % (tables[(8, 'matrix')] == tables[(8, 'fused')],
                                                      tables[(1, 'matrix')] == tables[(1, 'fused')]), flush=True)
times = {arm: [] for arm in arms}
for _segment in range(args.segments):
    for arm in arms:
        times[arm].append(wall(lambda: sweep(*arm)))
for arm in arms:
    print(line("run_sweep(batch=%d, search='%s')" % arm, times[arm]), flush=True)
fused, fastest = float(np.median(times[(8, 'fused')])), min(times[(8, 'matrix')])
print("acceptance at batch=8: fused median %.4f s %s the matrix arm's fastest segment %.4f s -> %s"
      % (fused, '<' if fused < fastest else '>=', fastest, 'holds' if fused < fastest else 'DOES NOT HOLD'), flush=True)

# ---- the search alone ----------------------------------------------------------------------------------------------------------------
dev = torch.device('cuda', 0)
ev = object.__new__(DeviceEvaluation)              # the two searches need the module and the device of an evaluation, nothing else
ev.torch, ev.dev = torch, dev
rng = np.random.default_rng(3)
labels_ex = list(range(10))
searches = [(torch.from_numpy(rng.random((100, d)) + 0.05).to(dev), torch.from_numpy(rng.random((10, d)) + 0.05).to(dev), labels_ex)
            for d in (50, 450, 2000) for _ in range(4)]
metrics = [m for m, _suffix in DEVICE_MEASURES]


def per_search():
    return [{m: ev.found_labels(t, e, l, m) for m in metrics} for t, e, l in searches]


def fused_search():
    return ev.found_labels_many(searches, metrics)


assert per_search() == fused_search()                                           # the warm-up, and the same labels
alone = {'48 x found_labels': [], '1 x found_labels_many (12 jobs x 4 measures)': []}
for _segment in range(max(args.segments, 20)):
    alone['48 x found_labels'].append(wall(per_search))
    alone['1 x found_labels_many (12 jobs x 4 measures)'].append(wall(fused_search))
print('the search alone: 12 comparisons of 100 x 10 rows, d = 50 / 450 / 2000 (4 each), 4 measures; %d segments' % max(args.segments, 20))
for what, t in alone.items():
    print(line(what, t), flush=True)
print('device: %s' % _native.device_info(0)['arch'])
