"""The row-sharded driver with the REAL HIP contexts: two ranks, both on GPU 0, collectives over gloo
(NCCL refuses two ranks on one device; gloo all-reduces CUDA tensors through the host).  What is checked is
everything the CPU test cannot see: the kernels' exchange buffers bound to torch tensors, the ordering of
the collectives against the context's stream, the common fp16 storage factor, and that the sharded fit
equals the single-process fit of the same kernels."""
import os
import socket

import numpy as np
import pytest

from oracle import klnmf_oracle as orc


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, n, f, k, iters, precision, out_dir):
    import torch
    import torch.distributed as dist
    from multimodal_amd.distributed import ShardedKLNMF, row_partition
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        X = orc.synthetic_V(77, n, f, k)
        H0 = orc.synthetic_H0(77, f, k)
        r0, r1 = row_partition(n, world)[rank]
        m = ShardedKLNMF(n, r1 - r0, f, k, max_iter=iters, precision=precision)
        m.set_v_max(X[r0:r1].max())
        Xd = torch.from_numpy(X[r0:r1].astype(np.float32)).cuda()
        m.upload_V_device(Xd)
        Xd.fill_(7.0e8)                      # the upload must be ordered before this (same stream)
        m.set_H(H0)
        m.init_W()
        errors, n_done, stopped = m.run(iters, fit=True, tol=0.0)
        W = m.gather_W()
        np.savez(os.path.join(out_dir, 'r%d.npz' % rank), W=W, H=m.get_H(), errors=np.array(errors))
        m.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize('precision,rtol,world', [('f16', 2e-4, 2), ('f64', 1e-9, 2), ('f16', 2e-4, 4)])
def test_two_ranks_on_one_gpu_equal_single_process(tmp_path, precision, rtol, world):
    import torch.multiprocessing as mp
    from multimodal_amd.lib import nmf
    n, f, k, iters = 4096 + 96, 512, 40, 4                   # ragged last shard (world 4: 4 ranks + this process on the card)
    mp.spawn(_worker, args=(world, _free_port(), n, f, k, iters, precision, str(tmp_path)), nprocs=world, join=True)
    X = orc.synthetic_V(77, n, f, k)
    H0 = orc.synthetic_H0(77, f, k)
    m = nmf.KLdivNMF(n_components=k, max_iter=iters, tol=0, precision=precision)
    m._init_dictionary = H0
    W1, e1 = m.fit_transform(X.astype(np.float32).astype(np.float64), return_errors=True)
    res = [np.load(os.path.join(str(tmp_path), 'r%d.npz' % r)) for r in range(world)]
    for r in res[1:]:
        np.testing.assert_array_equal(res[0]['H'], r['H'])               # replicas bit-identical
        np.testing.assert_array_equal(res[0]['errors'], r['errors'])
    for r in res:
        np.testing.assert_allclose(r['errors'], e1, rtol=rtol)
        np.testing.assert_allclose(r['H'], m.components_, rtol=50 * rtol, atol=1e-7)
        np.testing.assert_allclose(r['W'], W1, rtol=50 * rtol, atol=1e-6 * np.abs(W1).max())


def _worker_wide(rank, world, port, n, f, k, iters, out_dir):
    import torch
    import torch.distributed as dist
    from multimodal_amd.distributed import ShardedKLNMF, row_partition
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        X = orc.synthetic_V(7 + n + f + k, n, f, k)
        H0 = orc.synthetic_H0(7 + n + f + k, f, k)
        r0, r1 = row_partition(n, world)[rank]
        m = ShardedKLNMF(n, r1 - r0, f, k, max_iter=iters, precision='f16')
        m.set_v_max(X.max())
        m.upload_V(X[r0:r1])
        m.set_H(H0)
        m.init_W()
        errors, n_done, stopped = m.run(iters, fit=True, tol=0.0)
        np.savez(os.path.join(out_dir, 'r%d.npz' % rank), W=m.gather_W(), H=m.get_H(), errors=np.array(errors))
        m.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_row_shards_take_the_same_ratio_scale_in_the_first_update(tmp_path):
    """f / k = 1377: the first update's ratios pass the fp16 range and the dictionary image carries the ratio scale
    (k_ratio_scale).  The scale is derived from the dictionary alone, so every rank takes the same one whatever its rows
    hold: the replicas of H stay bit-identical, the all-reduced numerator is scaled as a whole, and losses and factors
    equal the oracle's as in the single-context test (test_first_update_after_init_keeps_its_ratios_inside_the_half_range)."""
    import torch.multiprocessing as mp
    n, f, k, iters, world = 400, 2755, 2, 3, 2
    mp.spawn(_worker_wide, args=(world, _free_port(), n, f, k, iters, str(tmp_path)), nprocs=world, join=True)
    X = orc.synthetic_V(7 + n + f + k, n, f, k)
    H0 = orc.synthetic_H0(7 + n + f + k, f, k)
    Wo, Ho, eo = orc.fit_transform(X, k=k, H0=H0, max_iter=iters, tol=0)
    res = [np.load(os.path.join(str(tmp_path), 'r%d.npz' % r)) for r in range(world)]
    np.testing.assert_array_equal(res[0]['H'], res[1]['H'])
    np.testing.assert_array_equal(res[0]['errors'], res[1]['errors'])
    np.testing.assert_allclose(res[0]['errors'], eo, rtol=1e-4)
    assert np.abs(res[0]['H'] - Ho).max() < 5e-3 * np.abs(Ho).max()
    assert np.abs(res[0]['W'] - Wo).max() < 5e-3 * np.abs(Wo).max()


@pytest.mark.gpu
@pytest.mark.parametrize('precision', ['f16', 'f64'])
def test_native_collective_path_single_rank_communicator(precision):
    """klnmf_run_sharded with a real RCCL communicator (one rank: NCCL refuses two ranks on one device): librccl is
    opened, the communicator built, the max exchange and the loop run through the native path, and the result is the
    single-context klnmf_run's, bit for bit (a one-rank all-reduce is the identity)."""
    from multimodal_amd import _native
    n, f, k, iters = 700, 384, 24, 5
    X = orc.synthetic_V(5, n, f, k)
    H0 = orc.synthetic_H0(5, f, k)
    out = []
    for native in (False, True):
        with _native.Context(precision, device=0) as ctx:
            ctx.set_problem(n, f, k, iters)
            if native:
                ctx.comm_init(_native.Context.comm_unique_id(), 0, 1)
                assert ctx.comm_max(3.25) == 3.25
                assert ctx.query(_native.Q_COMM_RANKS) == 1          # what RCCL itself reports (ncclCommCount): bench.py prints it
            ctx.upload_blocks([X])
            ctx.set_H(H0)
            ctx.init_W()
            errs, n_done, stopped = (ctx.run_sharded(n, iters, True, 0.0) if native else ctx.run(iters, True, 0.0))
            out.append((np.array(errs), n_done, stopped, ctx.get_W(), ctx.get_H()))
            if native:
                ctx.comm_destroy()
    assert out[0][1] == out[1][1] == iters and not out[1][2]
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][3], out[1][3])
    np.testing.assert_array_equal(out[0][4], out[1][4])


@pytest.mark.gpu
@pytest.mark.parametrize('precision,n,f,k,iters', [('f16', 700, 384, 24, 5), ('f64', 700, 384, 24, 5), ('f32', 900, 200, 10, 4),
                                                   ('f16', 66048, 256, 128, 6)])
def test_collective_branch_of_run_sharded_on_a_one_rank_communicator(monkeypatch, precision, n, f, k, iters):
    """The lines of klnmf_run_sharded that only N > 1 ranks execute -- the agreement block (refusal flags max, sums of V and
    cells sum), ONE grouped RCCL launch per iteration on the loop's own buffers (numerator: k x f_pad floats or k x f doubles,
    loss: 2 doubles), the separate decision kernel -- forced onto a one-rank communicator by KLNMF_COMM_SINGLE=1 (RCCL refuses
    two ranks on one device).  A one-rank all-reduce is the identity, so W and H must equal klnmf_run's bit for bit (the losses to fp64 summation order);
    the last case runs them with fp8 ratio tiles and the fp8 x fp8 column pass (the decision taken from the all-reduced sums)."""
    from multimodal_amd import _native
    X = orc.synthetic_V(5, n, f, k)
    H0 = orc.synthetic_H0(5, f, k)
    out = []
    for native in (False, True):
        if native:
            monkeypatch.setenv('KLNMF_COMM_SINGLE', '1')
        with _native.Context(precision, device=0) as ctx:
            ctx.set_problem(n, f, k, iters)
            if native:
                ctx.comm_init(_native.Context.comm_unique_id(), 0, 1)
                assert ctx.comm_max(3.25) == 3.25                    # a real ncclAllReduce(max) this time
            if precision == 'f16':
                ctx.set_v_max(float(X.max()))
            ctx.upload_blocks([X])
            ctx.set_H(H0)
            ctx.init_W()
            errs, n_done, stopped = (ctx.run_sharded(n, iters, True, 0.0) if native else ctx.run(iters, True, 0.0))
            rep = ctx.fp8_report() if precision == 'f16' else None
            out.append((np.array(errs), n_done, stopped, ctx.get_W(), ctx.get_H(), rep))
            if native:
                ctx.comm_destroy()
    assert out[0][1] == out[1][1] == iters and not out[1][2]
    # the loss: the same partial sums, added in fp64 by the slab-sum kernel's last block (klnmf_run defers it there) or by the
    # loss kernel in front of the exchange -- another order of a few hundred fp64 additions (6e-14 measured at 66 048 rows)
    np.testing.assert_allclose(out[1][0], out[0][0], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(out[0][3], out[1][3])
    np.testing.assert_array_equal(out[0][4], out[1][4])
    if n > 65536:
        assert out[1][5]['allowed'] and out[1][5]['column_pass_iterations'] == iters - 2 == out[0][5]['column_pass_iterations']


@pytest.mark.gpu
@pytest.mark.parametrize('precision', ['f16', 'f64'])
def test_loop_in_parts_on_a_communicator_is_run_sharded(monkeypatch, precision):
    """klnmf_loop_begin + klnmf_run_more + klnmf_loop_end on a context with a communicator = klnmf_run_sharded in parts (what
    bench.py's native path times: warm-up | fence | timed iterations of ONE loop): bit-identical losses, W and H."""
    from multimodal_amd import _native
    monkeypatch.setenv('KLNMF_COMM_SINGLE', '1')
    n, f, k, iters = 40000, 256, 64, 7               # (fp8 ratio tiles from the loop's third iteration on in f16)
    X = orc.synthetic_V(11, n, f, k)
    H0 = orc.synthetic_H0(11, f, k)
    out = []
    for parts in (False, True):
        with _native.Context(precision, device=0) as ctx:
            ctx.set_problem(n, f, k, iters)
            ctx.comm_init(_native.Context.comm_unique_id(), 0, 1)
            ctx.upload_blocks([X])
            ctx.set_H(H0)
            ctx.init_W()
            if parts:
                ctx.loop_begin()
                ctx.run_more(3, True, 0.0)
                ctx.synchronize()
                ctx.run_more(iters - 3, True, 0.0)
                errs, n_done, stopped = ctx.loop_end(iters)
            else:
                errs, n_done, stopped = ctx.run_sharded(n, iters, True, 0.0)
            rep = ctx.fp8_report() if precision == 'f16' else None
            out.append((np.array(errs), n_done, stopped, ctx.get_W(), ctx.get_H(), rep))
            ctx.comm_destroy()
    assert out[0][1] == out[1][1] == iters
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][3], out[1][3])
    np.testing.assert_array_equal(out[0][4], out[1][4])
    if precision == 'f16':
        assert out[0][5]['tile_iterations'] == out[1][5]['tile_iterations'] == iters - 2


@pytest.mark.gpu
def test_bench_native_path_on_a_one_rank_communicator():
    """bench.py's NATIVE collective path end to end on one GPU (KLNMF_COMM_SINGLE=1: a one-rank RCCL communicator, the
    library's collective branch with its all-reduces): the line says which path ran and how many ranks RCCL saw, and the timed
    iterations are the tail of ONE loop (every one of them on fp8 tiles after a warm-up of 2 or more)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, KLNMF_COMM_SINGLE='1')
    cmd = [sys.executable, os.path.join(root, 'bench.py'), '--steps', '5', '--warmup', '3', '--repeats', '2', '--rows', '40000',
           '--features', '512', '--components', '40', '--no-cpu-baseline', '--no-16bit-segment', '--collective', 'native']
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    cfg = d['config']
    assert cfg['collective_path'] == 'native' and cfg['rccl_ranks'] == 1
    assert d['valid'] and d['n_gpus'] == 1 and d['loss_finite_and_decreasing']
    assert cfg['fp8']['timed_iterations_with_fp8_ratio_tiles'] == 5


@pytest.mark.gpu
def test_collective_branch_refuses_together(monkeypatch):
    """The agreement block's refusal: a shard whose V exceeds the announced maximum fails klnmf_run_sharded with the rank's
    own message after the flags went through the all-reduce (KLNMF_COMM_SINGLE: the collective branch on one rank)."""
    from multimodal_amd import _native
    monkeypatch.setenv('KLNMF_COMM_SINGLE', '1')
    n, f, k = 512, 256, 16
    X = orc.synthetic_V(9, n, f, k)
    with _native.Context('f16', device=0) as ctx:
        ctx.set_problem(n, f, k, 3)
        ctx.comm_init(_native.Context.comm_unique_id(), 0, 1)
        ctx.set_v_max(float(X.max()) / 64.0)                         # the announced maximum is too small: storage factor too large
        Xb = X.copy(); Xb[3, 5] = X.max() * 4000.0
        ctx.upload_V(Xb)
        ctx.set_H(orc.synthetic_H0(9, f, k))
        ctx.init_W()
        with pytest.raises(_native.NativeError, match='exceeds the maximum given to klnmf_set_v_max'):
            ctx.run_sharded(n, 3, True, 0.0)
        ctx.comm_destroy()


@pytest.mark.gpu
def test_bench_two_rank_rehearsal(tmp_path):
    """bench.py's N > 1 code path end to end on one GPU (KLNMF_BENCH_REHEARSAL: both ranks on device 0, gloo): shard
    generation from the seeded blocks, the common storage factor, the sharded loop, max-over-ranks timing, one JSON line.
    --dump-outputs: the ranks' sampled rows of W, H and the loss record equal a one-process run's on the same arguments (the
    same seeded sample of the global rows; the numerator summed in another order)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, KLNMF_BENCH_REHEARSAL='1')
    common = ['--steps', '4', '--warmup', '2', '--repeats', '2', '--rows', '20000', '--features', '512', '--components', '40',
              '--full', '--no-cpu-baseline']
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), os.path.join(root, 'bench.py'), '--gpus', '2'] + common \
        + ['--dump-outputs', str(tmp_path / 'two')]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1]
    d = json.loads(line)
    assert d['n_gpus'] == 2 and d['valid'] and d['scaling'] == 'strong' and d['steps'] == 4
    assert d['config']['rows_per_gpu'] == 10016 and len(d['segments_ms_per_step']) == 2
    assert d['loss_finite_and_decreasing'] and d['value'] > 0
    # what a driver needs to trust an N > 1 line: which collective path ran, how many ranks RCCL saw (None on the gloo
    # rehearsal: no RCCL communicator), and what the loop ran on e4m3 operands as the LIBRARY reports it
    cfg = d['config']
    assert cfg['collective_path'] == 'torch' and 'rccl_ranks' in cfg and cfg['rccl_ranks'] is None
    assert cfg['fp8']['source'] == 'klnmf_query' and cfg['fp8']['timed_iterations_with_fp8_ratio_tiles'] == 0      # 10 016 rows per rank
    assert d['dtype'] == 'f16' and d['value_16bit'] is None
    assert d['dump_outputs']['arrays'] == {'W': [20000, 40], 'W_rows': [20000], 'errors': [6], 'H': [40, 512]}
    r1 = subprocess.run([sys.executable, os.path.join(root, 'bench.py')] + common + ['--dump-outputs', str(tmp_path / 'one')],
                        capture_output=True, text=True, timeout=300, cwd=root)
    assert r1.returncode == 0, r1.stderr[-2000:]
    two, one = ({name: np.load(str(tmp_path / run / (name + '.npy'))) for name in ('W', 'W_rows', 'errors', 'H')}
                for run in ('two', 'one'))
    assert one['W'].dtype == np.float32 and np.array_equal(one['W_rows'], two['W_rows'])
    assert d['loss_last'] == two['errors'][-1]
    np.testing.assert_allclose(two['errors'], one['errors'], rtol=2e-4)
    for name in ('W', 'H'):
        assert np.abs(two[name] - one[name]).max() <= 1e-2 * np.abs(one[name]).max(), name


@pytest.mark.gpu
@pytest.mark.parametrize('n,f,k,iters', [(3000, 1024, 40, 5), (66048, 1024, 128, 6), (40000, 768, 300, 5)])
def test_numerator_in_column_parts_with_overlapped_all_reduce(monkeypatch, n, f, k, iters):
    """Round 4: on a communicator the H numerator can be produced and exchanged in column parts (KLNMF_COMM_PARTS = 2 / 3), the
    all-reduce of part p on the communicator's own stream behind an event while the column pass of part p + 1 computes, the
    last part's all-reduce grouped with the loss on the context's stream AFTER the earlier ones have completed.  Run on a
    one-rank communicator (KLNMF_COMM_SINGLE=1: RCCL refuses two ranks on one device; a one-rank all-reduce is the identity):
      * overlap on == overlap off (KLNMF_COMM_OVERLAP=0: every all-reduce on the context's stream), bit for bit -- the second
        stream and the events change nothing but the timing;
      * parts == no parts to the order of the fp32 slab sums (each part has its own row chunks);
    at a small shape (column-split update pass), with fp8 tiles + fp8 x fp8 column pass, and on the component-split kernels."""
    from multimodal_amd import _native
    monkeypatch.setenv('KLNMF_COMM_SINGLE', '1')
    X = orc.synthetic_V(5, n, f, 12)
    H0 = orc.synthetic_H0(5, f, k)
    out = {}
    for parts, overlap in ((1, 1), (2, 1), (2, 0), (3, 1)):
        monkeypatch.setenv('KLNMF_COMM_PARTS', str(parts))
        monkeypatch.setenv('KLNMF_COMM_OVERLAP', str(overlap))
        with _native.Context('f16', device=0) as ctx:
            ctx.set_problem(n, f, k, iters)
            ctx.comm_init(_native.Context.comm_unique_id(), 0, 1)
            ctx.set_v_max(float(X.max()))
            ctx.upload_blocks([X])
            ctx.set_H(H0)
            ctx.init_W()
            layout = ctx.exchange_parts()
            assert len(layout) == min(parts, (f + 255) // 256)
            assert sum(nc for _, _, _, nc in layout) == f and layout[0][2] == 0
            errs, n_done, stopped = ctx.run_sharded(n, iters, True, 0.0)
            out[(parts, overlap)] = (np.array(errs), n_done, ctx.get_W(), ctx.get_H(), ctx.fp8_report())
            ctx.comm_destroy()
    base = out[(1, 1)]
    assert base[1] == iters
    for key in ((2, 1), (2, 0), (3, 1)):
        o = out[key]
        assert o[1] == iters and o[4]['tile_iterations'] == base[4]['tile_iterations']
        assert o[0][0] == base[0][0]                                  # the first loss: before any H rule, the same bits
        np.testing.assert_allclose(o[0], base[0], rtol=1e-6)          # (later ones see H to another fp32 summation order)
        np.testing.assert_allclose(o[2], base[2], rtol=1e-3, atol=1e-5 * np.abs(base[2]).max())
        np.testing.assert_allclose(o[3], base[3], rtol=1e-3, atol=1e-5 * np.abs(base[3]).max())
    for i in (0, 2, 3):
        np.testing.assert_array_equal(out[(2, 1)][i], out[(2, 0)][i])      # overlapped == serial, bit for bit
    Wo, Ho, eo = orc.fit_transform(X, k=k, H0=H0, max_iter=iters, tol=0)
    np.testing.assert_allclose(out[(2, 1)][0], eo, rtol=1e-3)


@pytest.mark.gpu
def test_torch_path_exchanges_the_numerator_in_parts(monkeypatch, tmp_path):
    """The torch-sequenced loop on the split layout (klnmf_exchange_parts / klnmf_iter_colpass_part): one process, no
    collective -- the sequencing of the pieces and the layout, against the same loop unsplit."""
    import torch
    from multimodal_amd.distributed import ShardedKLNMF
    n, f, k, iters = 40000, 768, 64, 6
    X = orc.synthetic_V(8, n, f, 12)
    H0 = orc.synthetic_H0(8, f, k)
    res = {}
    for parts in (1, 2):
        monkeypatch.setenv('KLNMF_COMM_PARTS', str(parts))
        m = ShardedKLNMF(n, n, f, k, max_iter=iters, precision='f16', collective='torch')
        assert (m.parts is None) == (parts == 1)
        m.set_v_max(float(X.max()))
        m.upload_V(X)
        m.set_H(H0)
        m.init_W()
        m.begin()
        for _ in range(iters):
            m.iterate(fit=True, tol=0.0)
        errors, n_done, stopped = m.end()
        res[parts] = (np.array(errors), n_done, m.get_W_local(), m.get_H())
        m.close()
    assert res[1][1] == res[2][1] == iters
    np.testing.assert_allclose(res[2][0], res[1][0], rtol=1e-6)
    # (the two runs see H to different fp32 summation orders; a ratio on an e4m3 rounding boundary may then fall to the other
    # side: single entries of W differ by the fp8 tiles' own step, the bulk by 1e-6)
    np.testing.assert_allclose(res[2][2], res[1][2], rtol=1e-3, atol=1e-5 * np.abs(res[1][2]).max())
    np.testing.assert_allclose(res[2][3], res[1][3], rtol=1e-3, atol=1e-5 * np.abs(res[1][3]).max())


@pytest.mark.gpu
@pytest.mark.parametrize('parts', [1, 2])
def test_exact_fix_ups_on_the_collective_path(monkeypatch, parts):
    """Ratios beyond the fp8 tiles' range (spikes the model cannot follow) on the path row shards take: the fix-ups run in
    k_post's SUMMING launch -- per column part, before the numerator is exchanged -- with the dictionary's old master, not in
    the launch that applies the H rule.  One-rank communicator (KLNMF_COMM_SINGLE=1), whole matrix and two column parts
    (512 columns: the spikes sit in both parts); the result must be what the single-context loop gives and keep the oracle's
    1e-4, with every saturated entry counted and none left unfixed."""
    from multimodal_amd import _native
    monkeypatch.setenv('KLNMF_COMM_SINGLE', '1')
    monkeypatch.setenv('KLNMF_COMM_PARTS', str(parts))
    n, f, k, iters = 70000, 512, 200, 8
    rs = np.random.RandomState(5)
    X = orc.synthetic_V(13, n, f, 12)
    X[:, f // 2:] = 1e-4 * rs.random_sample((n, f - f // 2))
    X[:, 100:140] = 1e-4 * rs.random_sample((n, 40))
    spikes = [(100, 103), (7000, 139), (30001, f // 2 + 64), (65999, f - 40)]
    for (i, j) in spikes:
        X[i, j] = 100.0 * X.mean()
    H0 = orc.synthetic_H0(13, f, k)
    Wo, Ho, eo = orc.fit_transform(X, k=k, H0=H0, max_iter=iters, tol=0)
    fo = orc.kl_error(X, Wo, Ho)
    out = []
    for native in (False, True):
        with _native.Context('f16', device=0) as ctx:
            ctx.set_problem(n, f, k, iters)
            if native:
                ctx.comm_init(_native.Context.comm_unique_id(), 0, 1)
            ctx.set_v_max(float(X.max()))
            ctx.upload_blocks([X])
            ctx.set_H(H0)
            ctx.init_W()
            errs, n_done, stopped = (ctx.run_sharded(n, iters, True, 0.0) if native else ctx.run(iters, True, 0.0))
            out.append((np.array(errs), ctx.get_W(), ctx.get_H(), ctx.fp8_report()))
            if native:
                ctx.comm_destroy()
    for e, W, H, rep in out:
        assert rep['tile_iterations'] == iters - 2 and rep['ratio_saturated'] >= len(spikes) and rep['ratio_unfixed'] == 0, rep
        np.testing.assert_allclose(e, eo, rtol=1e-4)
        assert abs(orc.kl_error(X, W.astype(np.float64), H.astype(np.float64)) - fo) <= 1e-4 * fo
    cols = sorted({j for _, j in spikes})
    scale = Ho.max()
    assert np.abs(out[1][2][:, cols] - out[0][2][:, cols]).max() <= 2e-3 * scale        # the spikes' dictionary columns: same correction
    np.testing.assert_allclose(out[1][0], out[0][0], rtol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize('parts', [1, 2])
def test_stop_rule_on_the_collective_path_breaks_where_the_oracle_does(monkeypatch, parts):
    """The stop rule of row shards rides in k_post's RULE launch behind the all-reduce (every block evaluates it from the
    exchanged loss, block 0 records): a tolerance that fires mid-way must break at the oracle's iteration (nmf.py:214-220,
    tol x n_total x f), `len(errors)` equal, and the dictionary handed back must be the one of the last executed update
    (the H ping-pong is settled from n_done) -- for an even and an odd number of launches enqueued behind the break."""
    from multimodal_amd import _native
    monkeypatch.setenv('KLNMF_COMM_SINGLE', '1')
    monkeypatch.setenv('KLNMF_COMM_PARTS', str(parts))
    n, f, k = 3000, 512, 24
    X = orc.synthetic_V(17, n, f, 12)
    H0 = orc.synthetic_H0(17, f, k)
    _, _, e_all = orc.fit_transform(X, k=k, H0=H0, max_iter=100, tol=0, warn=False)
    desc = -np.diff(np.array(e_all)) / (n * f)
    i = next(j for j in range(40, 95) if desc[j] > 1.02 * desc[j + 1] and np.all(desc[:j + 1] > np.sqrt(desc[j] * desc[j + 1])))
    tol = float(np.sqrt(desc[i] * desc[i + 1]))             # between two consecutive descents, below every earlier one
    Wo, Ho, eo = orc.fit_transform(X, k=k, H0=H0, max_iter=100, tol=tol, warn=False)
    assert len(eo) == i + 2
    for extra in (0, 1):
        with _native.Context('f16', device=0) as ctx:
            ctx.set_problem(n, f, k, 100 + extra)
            ctx.comm_init(_native.Context.comm_unique_id(), 0, 1)
            ctx.set_v_max(float(X.max()))
            ctx.upload_blocks([X])
            ctx.set_H(H0)
            ctx.init_W()
            errs, n_done, stopped = ctx.run_sharded(n, 100 + extra, True, tol)
            W, H = ctx.get_W(), ctx.get_H()
            ctx.comm_destroy()
        assert stopped and n_done == len(eo) == len(errs), (n_done, len(eo))
        np.testing.assert_allclose(errs, eo, rtol=1e-4)
        assert np.abs(H - Ho).max() <= 5e-3 * Ho.max() and np.abs(W - Wo).max() <= 5e-3 * Wo.max()


# ---- the fp8 regime on MORE THAN ONE rank (round-5 verdict, missing 3 / weak 3): torch-sequenced loop, ranks on one GPU over gloo -------

def _shard_data(kind, seed, n, f, k, world):
    """The whole matrix, the same on every rank (seeded): 'dense' = factorisable + noise of rank k (SURVEY 8d's kind);
    'last_shard_sparse' = the same with 95 % of the LAST rank's rows zeroed (histogram data stored densely)."""
    from multimodal_amd.distributed import row_partition
    X = orc.synthetic_V(seed, n, f, min(k, 24) if kind != 'dense' else k)
    if kind == 'last_shard_sparse':
        r0, r1 = row_partition(n, world)[world - 1]
        X = X.copy()
        X[r0:r1] *= (np.random.RandomState(seed + 1).random_sample((r1 - r0, f)) < 0.05)
    return X


def _worker_fp8(rank, world, port, kind, seed, n, f, k, iters, env_by_rank, out_dir):
    import torch
    import torch.distributed as dist
    for name, value in (env_by_rank.get(rank) or {}).items():
        os.environ[name] = value
    from multimodal_amd.distributed import ShardedKLNMF, row_partition
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        X = _shard_data(kind, seed, n, f, k, world)
        H0 = orc.synthetic_H0(seed, f, k)
        r0, r1 = row_partition(n, world)[rank]
        m = ShardedKLNMF(n, r1 - r0, f, k, max_iter=iters, precision='f16', collective='torch')
        m.set_v_max(X[r0:r1].max())
        m.upload_V(X[r0:r1])
        m.set_H(H0)
        m.init_W()
        errors, n_done, stopped = m.run(iters, fit=True, tol=0.0)
        rep = m.ctx.fp8_report()
        np.savez(os.path.join(out_dir, 'r%d.npz' % rank), W=m.get_W_local(), H=m.get_H(), errors=np.array(errors),
                 rows=np.array([r0, r1]), tile_iterations=rep['tile_iterations'], col8=rep['column_pass_iterations'],
                 allowed=rep['allowed'], gave_up=rep['gave_up'], trips=rep['monitor_trips'], checks=rep['monitor_checks'])
        m.close()
    finally:
        dist.destroy_process_group()


def _run_fp8_ranks(tmp_path, world, kind, seed, n, f, k, iters, env_by_rank=None):
    import torch.multiprocessing as mp
    mp.spawn(_worker_fp8, args=(world, _free_port(), kind, seed, n, f, k, iters, env_by_rank or {}, str(tmp_path)),
             nprocs=world, join=True)
    res = [np.load(os.path.join(str(tmp_path), 'r%d.npz' % r)) for r in range(world)]
    for r in res[1:]:
        np.testing.assert_array_equal(res[0]['H'], r['H'])               # replicas bit-identical
        np.testing.assert_array_equal(res[0]['errors'], r['errors'])
    W = np.vstack([r['W'] for r in res])
    assert W.shape[0] == n
    return res, W


@pytest.mark.gpu
@pytest.mark.parametrize('world,rows_per_rank', [(2, 66016), (4, 33024)])
def test_fp8_regime_on_row_shards_for_30_iterations(tmp_path, world, rows_per_rank):
    """What the 8-GPU run of configuration 4 executes on every rank, on 2 and 4 ranks for 30 iterations against the oracle
    (nmf.py:212-222, 345-351): fp8 ratio tiles from the loop's third iteration (world 2: 66 016 rows per rank = also the
    fp8 x fp8 column pass, k = 200; world 4: 33 024 rows per rank = fp8 tiles under f16 W operands), the monitor's checks with
    their polls (the trip count exchanged behind the column pass), the agreed shape rule at the loop's entry.  Every rank stays
    on the tiles for all 28 remaining iterations, the replicas of H are bit-identical, every loss and the TRUE final KL of the
    gathered factors are within 1e-4 of the oracle's."""
    n, f, k, iters = world * rows_per_rank, 256, 200, 30
    res, W = _run_fp8_ranks(tmp_path, world, 'dense', 21, n, f, k, iters)
    for r in res:
        assert bool(r['allowed']) and int(r['tile_iterations']) == iters - 2 and not bool(r['gave_up']), dict(r)
        assert int(r['checks']) >= 5 and int(r['trips']) == 0
        assert int(r['col8']) == (iters - 2 if rows_per_rank >= 65536 else 0)
    X = _shard_data('dense', 21, n, f, k, world)
    H0 = orc.synthetic_H0(21, f, k)
    Wo, Ho, eo = orc.fit_transform(X, k=k, H0=H0, max_iter=iters, tol=0)
    assert len(res[0]['errors']) == iters
    np.testing.assert_allclose(res[0]['errors'], eo, rtol=1e-4)
    fo = orc.kl_error(X, Wo, Ho)
    fg = orc.kl_error(X, W.astype(np.float64), res[0]['H'].astype(np.float64))
    assert abs(fg - fo) <= 1e-4 * fo, (fg, fo)


@pytest.mark.gpu
def test_one_sparse_shard_takes_every_rank_off_the_fp8_tiles_together(tmp_path):
    """One rank's shard is 95 % zeros (its columns hold too few entries for the tiles' noise to average out: the monitor's
    dry run on the loop's first iteration measures 1e-3 against its threshold of 8e-4), the other rank's shard is dense and
    would keep the tiles.  Ranks must not mix tile formats (the numerators differ by sqrt(2)): the trip count travels with
    the loss exchange -- behind the column pass that publishes it -- and EVERY rank continues on 16-bit
    tiles from the same iteration on: only the sparse rank counted trips, both gave the regime up, neither took a tile, the
    replicas are bit-identical and the fit keeps the oracle's 1e-4."""
    world, f, k, iters = 2, 96, 40, 12
    n = world * 40000
    res, W = _run_fp8_ranks(tmp_path, world, 'last_shard_sparse', 5, n, f, k, iters)
    assert int(res[0]['trips']) == 0 and int(res[1]['trips']) > 0
    for r in res:          # ('allowed' reads as False once a loop has given the regime up)
        assert bool(r['gave_up']) and int(r['tile_iterations']) == 0 and int(r['checks']) == 1, {a: r[a] for a in ('gave_up', 'tile_iterations', 'checks', 'trips')}
    X = _shard_data('last_shard_sparse', 5, n, f, k, world)
    H0 = orc.synthetic_H0(5, f, k)
    Wo, Ho, eo = orc.fit_transform(X, k=k, H0=H0, max_iter=iters, tol=0)
    np.testing.assert_allclose(res[0]['errors'], eo, rtol=1e-4)
    fo = orc.kl_error(X, Wo, Ho)
    assert abs(orc.kl_error(X, W.astype(np.float64), res[0]['H'].astype(np.float64)) - fo) <= 1e-4 * fo


@pytest.mark.gpu
def test_only_one_ranks_monitor_trips_and_every_rank_follows(tmp_path):
    """The same agreement with the trip forced on ONE rank by its own threshold (KLNMF_MON_THRESHOLD, a development switch, set
    in rank 1's environment only; dense data that passes everywhere else): rank 1's dry run trips, rank 0's does not; both
    must read the all-reduced count at the poll and neither may take an fp8 tile."""
    world, f, k, iters = 2, 256, 40, 8
    n = world * 40000
    res, _ = _run_fp8_ranks(tmp_path, world, 'dense', 9, n, f, k, iters, env_by_rank={1: {'KLNMF_DEV': '1', 'KLNMF_MON_THRESHOLD': '1e-9'}})
    assert int(res[0]['trips']) == 0 and int(res[1]['trips']) > 0
    for r in res:
        assert bool(r['gave_up']) and int(r['tile_iterations']) == 0, dict(r)
    # ... and without the forced trip the same ranks keep the tiles
    sub = tmp_path / 'plain'
    sub.mkdir()
    res2, _ = _run_fp8_ranks(sub, world, 'dense', 9, n, f, k, iters)
    for r in res2:
        assert not bool(r['gave_up']) and int(r['tile_iterations']) == iters - 2


@pytest.mark.gpu
def test_shards_straddling_the_fp8_row_threshold_stay_on_16_bit_tiles(tmp_path):
    """65 568 rows over two ranks = 32 800 + 32 768: the first shard's shape allows fp8 ratio tiles (more than 32 768 rows), the
    second's does not.  The shape rule is agreed at the loop's entry (klnmf_loop_begin_agreed): every
    rank runs 16-bit tiles, the result equals the single-process fit of the same kernels' 16-bit regime and the oracle."""
    from multimodal_amd.distributed import row_partition
    world, n, f, k, iters = 2, 65568, 256, 40, 6
    assert [b - a for a, b in row_partition(n, world)] == [32800, 32768]
    res, W = _run_fp8_ranks(tmp_path, world, 'dense', 13, n, f, k, iters)
    for r in res:
        assert not bool(r['allowed']) and int(r['tile_iterations']) == 0 and int(r['checks']) == 0, dict(r)
    X = _shard_data('dense', 13, n, f, k, world)
    H0 = orc.synthetic_H0(13, f, k)
    Wo, Ho, eo = orc.fit_transform(X, k=k, H0=H0, max_iter=iters, tol=0)
    np.testing.assert_allclose(res[0]['errors'], eo, rtol=1e-4)
    fo = orc.kl_error(X, Wo, Ho)
    assert abs(orc.kl_error(X, W.astype(np.float64), res[0]['H'].astype(np.float64)) - fo) <= 1e-4 * fo


@pytest.mark.gpu
def test_bench_native_path_at_one_ranks_shard_of_configuration_4_with_monitor_polls():
    """One rank's shard of the 8-GPU run of configuration 4 (125 000 x 4096, k = 200) through bench.py's NATIVE collective path
    (KLNMF_COMM_SINGLE=1: one-rank RCCL communicator, grouped all-reduce of numerator + loss per iteration): every timed
    iteration on fp8 tiles + the fp8 x fp8 column pass, and the monitor's checks 2, 4, 8, 16 -- each followed by a poll that reads
    the all-reduced count -- INSIDE the timed region (warm-up 3 = the dry run and check 1)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, KLNMF_COMM_SINGLE='1', KLNMF_DEV='1')
    cmd = [sys.executable, os.path.join(root, 'bench.py'), '--steps', '20', '--warmup', '3', '--repeats', '2', '--rows', '125000',
           '--data', 'device', '--no-cpu-baseline', '--no-16bit-segment', '--collective', 'native']
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    cfg = d['config']
    assert cfg['collective_path'] == 'native' and cfg['rccl_ranks'] == 1 and d['valid'] and d['loss_finite_and_decreasing']
    fp8 = cfg['fp8']
    assert fp8['timed_iterations_with_fp8_ratio_tiles'] == 20 and fp8['timed_iterations_with_fp8_x_fp8_column_pass'] == 20
    assert fp8['monitor_checks'] == 6 and fp8['monitor_trips'] == 0 and not fp8['gave_up'], fp8


@pytest.mark.gpu
def test_bench_two_rank_rehearsal_in_the_fp8_regime():
    """bench.py's N > 1 path on the torch-sequenced loop with BOTH ranks' shards large enough for fp8 ratio tiles (2 x 40 000
    rows): the timed iterations run on the tiles on every rank, the monitor's polls (loss[1] exchanged behind the column pass:
    distributed.py) happen inside the timed region, and the line is valid."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, KLNMF_BENCH_REHEARSAL='1')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), os.path.join(root, 'bench.py'), '--gpus', '2', '--steps', '12', '--warmup', '3',
           '--repeats', '2', '--rows', '80000', '--features', '256', '--components', '40', '--no-cpu-baseline', '--no-16bit-segment']
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=400, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    cfg = d['config']
    assert d['n_gpus'] == 2 and d['valid'] and d['loss_finite_and_decreasing'] and cfg['rows_per_gpu'] == 40000
    assert cfg['collective_path'] == 'torch'
    fp8 = cfg['fp8']
    assert fp8['loop_allowed'] and fp8['timed_iterations_with_fp8_ratio_tiles'] == 12 and not fp8['gave_up'] and fp8['monitor_checks'] >= 4, fp8
