"""bench.py end to end on one GPU: what a plain run measures and what `--full` adds to it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, capture_output=True, text=True, timeout=300,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])


@pytest.mark.gpu
def test_bench_plain_run_is_the_headline_and_full_adds_the_rest(tmp_path):
    """A plain run times the same segments and dumps the same outputs as a --full run with the same arguments, bit for bit, and
    leaves out what --full measures besides them: the CPU baseline and its parity leg, the all-16-bit segment, the power and
    clock samples.  70 000 rows: more than 65 536, so the loop runs fp8 ratio tiles and --full has a 16-bit segment to run."""
    common = ['--steps', '4', '--warmup', '3', '--repeats', '2', '--rows', '70000', '--features', '256', '--components', '40']
    plain = _bench(common + ['--dump-outputs', str(tmp_path / 'plain')])
    full = _bench(common + ['--full', '--dump-outputs', str(tmp_path / 'full')])
    for d in (plain, full):
        assert d['valid'] and d['loss_finite_and_decreasing'] and d['value'] > 0
        assert d['config']['fp8']['timed_iterations_with_fp8_ratio_tiles'] == 4
    for key in ('metric', 'unit', 'higher_is_better', 'dtype', 'steps', 'warmup', 'n_gpus', 'loss_first', 'loss_last'):
        assert plain[key] == full[key], key
    assert plain['value_16bit'] is None and plain['power_clock'] is None
    assert 'cpu_baseline' not in plain and 'parity' not in plain
    assert full['value_16bit']['valid'] and full['value_16bit']['fp8_tile_iterations'] == 0
    assert full['cpu_baseline']['value'] > 0
    parity = full['parity']
    assert 'error' not in parity, parity
    assert parity['len_errors'][0] == parity['len_errors'][1] and parity['final_kl_rel_err'] <= parity['tolerance'], parity
    assert plain['dump_outputs']['arrays'] == full['dump_outputs']['arrays']
    for name in plain['dump_outputs']['arrays']:
        np.testing.assert_array_equal(np.load(str(tmp_path / 'plain' / (name + '.npy'))),
                                      np.load(str(tmp_path / 'full' / (name + '.npy'))), err_msg=name)
