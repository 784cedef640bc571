"""CPU-side tests: the C-ABI library loads and exports exactly what
include/klnmf.h declares, the host logic (input contract, error conventions,
learner bookkeeping) behaves like the reference, and the product path refuses
to run without a GPU instead of falling back to anything."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
from numpy.testing import assert_array_almost_equal

from multimodal_amd import _native
from multimodal_amd.lib import nmf
from multimodal_amd.lib.array_utils import normalize_sum, safe_hstack
from multimodal_amd.lib.sklearn_utils import atleast2d_or_csr
from multimodal_amd.learner import MultimodalLearner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'klnmf.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(klnmf_[a-z_A-Z0-9]+)\s*\(', text)))


def test_library_exports_every_declared_symbol():
    lib = _native.load()
    declared = _declared_symbols()
    assert len(declared) >= 30
    for name in declared:
        assert hasattr(lib, name), "libklnmf.so does not export %s" % name
    # and the ctypes table binds exactly the header
    assert sorted(_native.SIGNATURES) == declared
    assert lib.klnmf_version() == 100


def _csrc(name):
    with open(os.path.join(ROOT, 'multimodal_amd', 'csrc', name)) as fh:
        return fh.read()


def test_problem_counts_are_assigned_by_the_plan_alone():
    """Every shape-derived count of a problem is a field of ProblemPlan (csrc/plan.hip.h) and reaches the context as one
    assignment of the whole plan: api_context.hip assigns none of them, and the hand-written reset lists are gone."""
    plan = _csrc('plan.hip.h')
    counts = ('nsplit kchunk wsplit wchunk hseg hseg_n loss_part_count sp_nblk sp_blocked sp_cb sp_rb sp_cb_cols sp_rb_rows KT KP ks '
              'big n_pad f_pad w_rows nrt nct nct_used ncb nchunks stages_per_chunk q8_ok ne_ok kc_shape row_chunks row_ct_chunk '
              'tail_wg tail_chunks tail_ct_chunk nparts_cfg whole sparse nnz n f k').split()
    for name in counts:
        assert re.search(r'\b%s\b' % name, plan[plan.index('struct ProblemPlan'):plan.index('inline bool h_from_slabs')]), name
    pattern = re.compile(r'c->(%s)\s*=[^=]' % '|'.join(counts))
    for unit in ('api_context.hip', 'api_loop.hip', 'api_eval.hip', 'api_comm.hip', 'api_group.hip'):
        assert not pattern.search(_csrc(unit)), (unit, pattern.search(_csrc(unit)).group(0))
    ctx = _csrc('api_context.hip')
    assert ctx.count('static_cast<ProblemPlan &>(*c) = plan;') == 1
    # the dead parameters stay out
    for unit in ('ctx.hip.h', 'plan.hip.h', 'api_context.hip', 'api_loop.hip'):
        assert not re.search(r'\b(q_tt|w_tt|n_tt|nst)\b', _csrc(unit)), unit
    # resets are assignments of a default-constructed group: one for the problem (free_all), one for the loop (begin_fp8_loop)
    assert _csrc('ctx.hip.h').count('static_cast<ProblemState &>(*this) = ProblemState();') == 1
    assert _csrc('api_loop.hip').count('static_cast<LoopState &>(*c) = LoopState();') == 1


def test_the_development_switches_are_read_at_the_call_sites_that_remain_by_design():
    sites = {}
    for name in sorted(os.listdir(os.path.join(ROOT, 'multimodal_amd', 'csrc'))):
        if name.endswith('.hip') or name.endswith('.hip.h'):
            n = len(re.findall(r'DevSwitches::read\(\)', _csrc(name)))
            if n:
                sites[name] = n
    assert sites == {
        'api_context.hip': 1,       # set_problem: both klnmf_set_problem entry points, before the plan
        'api_loop.hip': 1,          # begin_fp8_loop: every loop entry
        'api_comm.hip': 1,          # comm_multi: KLNMF_COMM_SINGLE, asked outside problems and loops
        'api_eval.hip': 1,          # klnmf_plan_query: as klnmf_set_problem reads them, without a context
    }


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except Exception:
        return True


@pytest.mark.skipif(not _no_gpu(), reason="only meaningful on a box without a GPU")
def test_no_silent_cpu_fallback():
    X = np.abs(np.random.RandomState(0).random_sample((6, 5)))
    with pytest.raises((RuntimeError, MemoryError)):
        nmf.KLdivNMF(n_components=2, max_iter=3).fit(X)
    with pytest.raises((RuntimeError, MemoryError)):
        nmf.KLdivNMF._Q(X, np.ones((6, 2)), np.ones((2, 5)))


def test_product_does_not_import_oracle():
    """The oracle is test infrastructure: nothing under multimodal_amd/ may
    import, link or execute it."""
    pkg = os.path.join(ROOT, 'multimodal_amd')
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if not fn.endswith(('.py', '.h', '.hip')):
                continue
            for line in open(os.path.join(dirpath, fn)).read().splitlines():
                if 'import' in line or '#include' in line or 'exec' in line:
                    assert 'oracle' not in line, "%s uses the oracle: %s" % (fn, line)


# ---- error conventions (raised on the host before any upload) ----------------

def test_negative_and_nonfinite_input_raise_valueerror():
    with pytest.raises(ValueError) as e:
        nmf.KLdivNMF(n_components=1).fit(np.array([[1., -1.], [0., 1.]]))
    assert str(e.value) == "Negative values in data passed to NMF.fit"
    with pytest.raises(ValueError) as e:
        nmf.KLdivNMF(n_components=1).fit(np.array([[1., np.nan], [0., 1.]]))
    assert str(e.value) == "array contains NaN or infinity"
    with pytest.raises(ValueError):
        nmf.KLdivNMF(n_components=1).fit(np.array([[1., np.inf], [0., 1.]]))
    with pytest.raises(ValueError):
        nmf.KLdivNMF(n_components=1).fit(sp.csr_matrix(np.array([[1., -2.], [0., 1.]])))


def test_scale_helper_matches_reference_tests():
    # reference tests/test_nmf_kl.py:25-68
    assert nmf._scale(np.zeros((3, 4)), np.zeros((3,)), axis=1).shape == (3, 4)
    with pytest.raises(ValueError):
        nmf._scale(np.zeros((3, 4)), np.zeros((4,)), axis=3)
    with pytest.raises(ValueError):
        nmf._scale(np.zeros((3, 4, 6)), np.zeros((3,)), axis=1)
    with pytest.raises(ValueError):
        nmf._scale(np.zeros((3,)), np.zeros((3,)), axis=1)
    with pytest.raises(ValueError):
        nmf._scale(np.zeros((3, 4)), np.zeros((2,)), axis=1)
    m = np.array([[1, 2, 3], [4, 5, 6]])
    assert_array_almost_equal(nmf._scale(m, np.array([2, 3]), axis=1),
                              np.array([[2, 4, 6], [12, 15, 18]]))
    assert_array_almost_equal(nmf._scale(m, np.array([3, 2, 1]), axis=0),
                              np.array([[3, 4, 3], [12, 10, 6]]))


def test_normalize_sum_matches_reference_tests():
    # reference tests/test_array_utils.py:9-58
    a = np.array([[0., 1., 3.], [2., 3., 3.]])
    assert np.all(normalize_sum(a, axis=0) == np.array([[0., .25, .5], [1., .75, .5]]))
    assert np.all(normalize_sum(a, axis=1) == np.array([[0., .25, .75], [.25, .375, .375]]))
    with pytest.raises(ValueError):
        normalize_sum(np.ones((2, 3, 4)), axis=3)
    z = np.abs(np.random.RandomState(1).random_sample((2, 4)))
    z[1, :] = 0
    assert not np.any(np.isnan(normalize_sum(z, axis=1)))
    for shape in [(3,), (2, 4), (1, 2, 3)]:
        b = np.abs(np.random.RandomState(2).random_sample(shape))
        for ax in range(len(shape)):
            n = normalize_sum(b, axis=ax)
            assert n.shape == b.shape
            assert_array_almost_equal(n.sum(axis=ax), 1.)


def test_special_sparse_dot_matches_reference_tests():
    # reference tests/test_nmf_kl.py:175-192
    rs = np.random.RandomState(5)
    ref = sp.rand(5, 6, .3, random_state=rs).tocsr()
    a, b = rs.random_sample((5, 7)), rs.random_sample((7, 6))
    ab = nmf._special_sparse_dot(a, b, ref)
    assert (ab.indptr == ref.indptr).all() and (ab.indices == ref.indices).all()
    ok = np.multiply(np.dot(a, b), (ref.toarray() != 0))
    assert_array_almost_equal(ab.toarray(), ok)


def test_input_contract():
    assert atleast2d_or_csr([1., 2., 3.]).shape == (1, 3)
    assert isinstance(atleast2d_or_csr(np.matrix([[1., 2.]])), np.ndarray)
    assert sp.isspmatrix_csr(atleast2d_or_csr(sp.coo_matrix(np.eye(3))))
    m = nmf.KLdivNMF()
    assert (m.tol, m.max_iter, m.eps, m.subit) == (1e-6, 200, 1e-8, 10)
    assert m.n_components is None and m._init_dictionary is None and m.random_state is None
    m2 = nmf.KLdivNMF(n_components=3)
    m2._init_dictionary = np.ones((2, 5))
    with pytest.raises(AssertionError):     # shape mismatch, nmf.py:153-154
        m2.fit(np.ones((4, 5)))


def test_learner_bookkeeping():
    lr = MultimodalLearner(['a', 'b', 'c'], [3, 5, 2], [2., .5, 1.], 4)
    assert lr.get_axis_range('a') == (0, 3)
    assert lr.get_axis_range('b') == (3, 8)
    assert lr.get_axis_range('c') == (8, 10)
    rs = np.random.RandomState(0)
    blocks = [rs.random_sample((4, d)) for d in (3, 5, 2)]
    V = lr.stack_data(['a', 'b', 'c'], blocks)
    assert V.shape == (4, 10)
    assert np.allclose(V[:, 3:8], .5 * blocks[1])
    V2 = lr.stack_data(['c', 'a'], [blocks[2], blocks[0]])
    assert np.allclose(V2, np.hstack([blocks[2], 2. * blocks[0]]))
    assert sp.issparse(safe_hstack([sp.csr_matrix(blocks[0]), blocks[1]]))
    lr.dico = rs.random_sample((4, 10))          # assigned from outside, as the scripts do
    assert lr.get_dico() is lr.dico
    view = lr.get_dico('b')
    assert view.base is lr.dico and view.shape == (4, 5)
    assert lr.get_stacked_dicos(['c', 'a']).shape == (4, 5)
    internal = rs.random_sample((6, 4))
    import torch
    if not torch.cuda.is_available():            # the reconstruction product runs on the device: no CPU fallback
        with pytest.raises((RuntimeError, MemoryError)):
            lr.reconstruct_modality('b', internal)
    with pytest.raises(AssertionError):
        lr.train([blocks[0], blocks[1][:3], blocks[2]], 2)
    with pytest.raises(AssertionError):
        lr.reconstruct_internal('a', blocks[1], 2)
    lr2 = MultimodalLearner(['a'], [3], [1.], 2, sparseness='data')
    with pytest.raises(TypeError):               # `raise NotImplemented`, learner.py:37-38
        lr2.train([blocks[0]], 1)


def test_synthetic_generators_agree():
    """bench.py's block generator (multimodal_amd/synthetic.py), the fixtures' (tests/golden_inputs.py) and the
    oracle's are the same seeded streams: any row range, any thread count, bit for bit."""
    from multimodal_amd import synthetic as syn
    from oracle import klnmf_oracle as orc
    from tests import golden_inputs as gi
    n, f, k = 20000, 96, 6
    X, H0 = gi.synthetic_problem(11, n, f, k)
    assert np.array_equal(X, orc.synthetic_V(11, n, f, k)) and np.array_equal(H0, orc.synthetic_H0(11, f, k))
    assert np.array_equal(H0, syn.H0_of(11, f, k))
    assert np.array_equal(X[5000:17001], syn.rows_of(11, 5000, 17001, n, f, k))
    got = np.zeros((12001, f), dtype=np.float32)
    pieces = []

    def consume(lo, arr):
        pieces.append(lo)
        got[lo:lo + arr.shape[0]] = arr
    vmax = syn.for_each_block(11, 5000, 17001, n, f, k, consume, workers=3)
    assert pieces == sorted(pieces) and np.array_equal(got, X[5000:17001].astype(np.float32))
    assert vmax == X[5000:17001].max()


def test_lean_cpu_iteration_is_the_same_iteration():
    """bench.py's "optimised CPU" baseline (one W.H, float32) against the faithful restatement."""
    from oracle import klnmf_oracle as orc
    X = orc.synthetic_V(5, 300, 200, 8)
    H0 = orc.synthetic_H0(5, 200, 8)
    W, H = orc.init_factors(X, 8, H0=H0)
    W32, H32, X32 = W.astype(np.float32), H.astype(np.float32), X.astype(np.float32)
    for it in range(4):
        loss = orc.kl_error(X, W, H)
        W, H = orc.update_step(X, W, H)
        l32, W32, H32 = orc.fit_iteration_lean32(X32, W32, H32)
        assert abs(l32 - loss) <= 2e-6 * loss
        assert np.abs(W32 - W).max() <= 2e-5 * np.abs(W).max() and np.abs(H32 - H).max() <= 2e-5 * np.abs(H).max()


def test_bench_defaults_follow_the_measurement_contract():
    import bench
    a = bench.parse_args([])
    assert (a.gpus, a.n, a.f, a.k, a.precision) == (1, 1000000, 4096, 200, 'f16')       # BASELINE.json configs[3]
    assert a.tol == 0.0 and a.repeats == 5 and a.data == 'blocks'
    # the CPU sample is SURVEY 8d's n = 100 000 (more than 65 536: the parity leg on it runs fp8 tiles and the fp8 x fp8 column
    # pass), 1 + 5 iterations: about 25 s of fp64 work on the GPU box's host, 4 of the 6 GPU iterations on fp8
    assert a.cpu_rows == 100000 and a.cpu_iters == 5 and a.segment_timeout > 0
    assert a.dump_outputs is None
    # a plain run measures the headline alone: the CPU baseline, value_16bit and power_clock are --full's
    assert not a.full and bench.parse_args(['--full']).full
    with pytest.raises(SystemExit):
        bench.parse_args(['--steps', '0'])


def test_bench_dump_outputs_are_a_fixed_sample_within_64_mb(tmp_path, monkeypatch):
    """bench.py --dump-outputs: W's rows (and H's columns, where H alone would exceed its share) are a seeded sample that
    depends on the arguments only; at the default shape every mode stays within 64 MB; a shard contributes exactly the
    sampled rows it holds, and the files load back as written."""
    import bench

    class Shard(object):             # what collect_outputs reads of a ShardedKLNMF
        def __init__(self, n_total, r0, r1, f, k):
            self.n_total, self.k, self.r0, self.r1, self.f = n_total, k, r0, r1, f

        def get_W_local(self, dtype=np.float64):
            return np.repeat(np.arange(self.r0, self.r1, dtype=dtype)[:, None], self.k, axis=1)      # each row holds its index

        def get_H(self, dtype=np.float64):
            return np.arange(self.k * self.f, dtype=dtype).reshape(self.k, self.f)

    for precision, item in (('f16', 4), ('f32', 4), ('f64', 8)):
        for n, f, k in ((1000000, 4096, 200), (4000000, 2000000, 1)):          # (the default shape; one where indices weigh most)
            a = bench.parse_args(['--precision', precision, '--rows', str(n), '--features', str(f), '--components', str(k)])
            rows = bench.dump_sample(n, k * item + 8, bench.DUMP_W_BYTES, a.seed + 17)
            cols = bench.dump_sample(f, k * item + 8, bench.DUMP_H_BYTES, a.seed + 18)
            total = rows.size * (k * item + 8) + k * cols.size * item + (cols.size * 8 if cols.size < f else 0) \
                + (a.warmup + a.steps) * 8
            assert total <= 64 << 20 and 0 < rows.size < n and (cols.size == f) == (k > 1)
            assert np.array_equal(rows, bench.dump_sample(n, k * item + 8, bench.DUMP_W_BYTES, a.seed + 17))
            assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < n

    a = bench.parse_args(['--rows', '5000', '--features', '300', '--components', '7', '--dump-outputs', str(tmp_path)])
    full = bench.collect_outputs(a, Shard(5000, 0, 5000, 300, 7), None, 1, 0, 0, 5000, [3.0, 2.0], with_H=True)
    assert full['W'].dtype == np.float32 and full['W'].shape == (5000, 7) and 'H_cols' not in full
    assert np.array_equal(full['W_rows'], np.arange(5000.0)) and full['H'].shape == (7, 300)
    # a sampled W (the budget shrunk to sample at a small shape): every rank contributes the sampled rows of its own range, in order
    monkeypatch.setattr(bench, 'DUMP_W_BYTES', 1 << 16)
    a = bench.parse_args(['--rows', '3000', '--features', '64', '--components', '5'])
    one = bench.collect_outputs(a, Shard(3000, 0, 3000, 64, 5), None, 1, 0, 0, 3000, [1.0], with_H=False)
    assert 'H' not in one and one['W'].shape[0] == one['W_rows'].size < 3000
    assert np.array_equal(one['W'][:, 0], one['W_rows']) and np.array_equal(one['W'][:, -1], one['W_rows'])
    halves = [bench.collect_outputs(a, Shard(3000, r0, r1, 64, 5), None, 1, 0, r0, r1, [1.0], with_H=False)['W']
              for r0, r1 in ((0, 1504), (1504, 3000))]
    assert np.array_equal(np.concatenate(halves), one['W'])
    monkeypatch.setattr(bench, 'DUMP_H_BYTES', 1 << 10)
    sampled = bench.collect_outputs(a, Shard(3000, 0, 3000, 64, 5), None, 1, 0, 0, 3000, [1.0], with_H=True)
    cols = sampled['H_cols'].astype(np.int64)
    assert 0 < cols.size < 64 and np.array_equal(sampled['H'], Shard(3000, 0, 3000, 64, 5).get_H(np.float32)[:, cols])
    written = bench.write_outputs(str(tmp_path), full)
    assert written['arrays']['W'] == [5000, 7]
    for name, arr in full.items():
        back = np.load(os.path.join(str(tmp_path), name + '.npy'))
        assert back.dtype in (np.float32, np.float64) and np.array_equal(back, arr)


def test_scale_inverse_scales_W_columns_and_H_rows():
    """KLdivNMF.scale (nmf.py:314-321): W columns times (factors + eps), H rows divided by it: W.H unchanged."""
    rs = np.random.RandomState(4)
    W, H = rs.random_sample((6, 3)), rs.random_sample((3, 5))
    factors = np.array([2., .5, 4.])
    m = nmf.KLdivNMF(n_components=3)
    sW, sH = m.scale(W, H, factors)
    assert_array_almost_equal(sW, W * (factors + 1e-8)[None, :])
    assert_array_almost_equal(sH, H / (factors + 1e-8)[:, None])
    assert_array_almost_equal(sW.dot(sH), W.dot(H))
    assert_array_almost_equal(nmf.KLdivNMF(eps=.5).scale(W, H, factors)[0], W * (factors + .5)[None, :])    # the one place self.eps is read


def test_build_staleness_sees_every_kernel_header():
    """__graft_entry__.build() recompiles when ANY source of the library is newer than the built .so -- the list is a
    glob of csrc/, so a header added later (round 2: colq8x.hip.h was missing from a hand-kept list) cannot be forgotten."""
    import __graft_entry__ as ge
    names = {os.path.basename(p) for p in ge._sources()}
    for must in ('ctx.hip.h', 'api_context.hip', 'api_loop.hip', 'api_comm.hip', 'api_eval.hip', 'mfma4.hip.h', 'colq.hip.h', 'colq8x.hip.h',
                 'post.hip.h', 'monitor.hip.h', 'exact.hip.h', 'sparse.hip.h', 'sparseb.hip.h', 'klnmf.h',
                 'rowpass4_list.hip.h', 'stage_chunks.h', 'api_batch.hip', 'rowpass4_inst_1.hip', 'rowpass4_inst_2.hip', 'rowpass4_inst_3.hip'):
        assert must in names
    if not os.path.exists(ge.LIB):
        assert ge._stale()
        return
    hdr = os.path.join(ge.CSRC, 'colq8x.hip.h')
    st = os.stat(hdr)
    lib_t = os.path.getmtime(ge.LIB)
    try:
        os.utime(hdr, (lib_t + 10, lib_t + 10))
        assert ge._stale()
    finally:
        os.utime(hdr, (st.st_atime, st.st_mtime))


def test_bench_watchdog_exits_nonzero_with_a_diagnostic():
    """A rank stuck in a collective no peer will join must not hang the job: bench.py runs every segment under a timer
    that prints what the rank was doing and leaves with status 3 (os._exit: never a re-exec, no clean-up that could block)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, time; sys.path.insert(0, %r); import bench\n"
            "with bench.Watchdog(0.3, 'segment 0 (test)', 5):\n    time.sleep(20)\n" % root)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=60)
    assert r.returncode == 3
    assert 'watchdog' in r.stderr and 'rank 5' in r.stderr and 'segment 0 (test)' in r.stderr
    ok = subprocess.run([sys.executable, '-c', "import sys; sys.path.insert(0, %r); import bench\nwith bench.Watchdog(30, 'x', 0):\n    pass\n" % root],
                        capture_output=True, text=True, timeout=60)
    assert ok.returncode == 0


def test_auto_precision_picks_the_exact_mode_for_small_problems_and_f16_for_large_ones():
    """precision='auto' (KLNMF_PRECISION=auto): f64 = the reference's results where a fit is cheap, the MFMA path from 2e9
    multiply-adds per W.H on; the default stays 'f64' (defaults must reproduce the reference's results)."""
    assert nmf.resolve_precision('auto', 500, 1000, 10) == 'f64'            # BASELINE config 1
    assert nmf.resolve_precision('auto', 1000, 2450, 50) == 'f64'           # the reference's own experiment scale
    assert nmf.resolve_precision('auto', 50000, 4096, 50) == 'f16'          # config 2
    assert nmf.resolve_precision('auto', 1000000, 4096, 200) == 'f16'       # config 4
    assert nmf.resolve_precision('f32', 1000000, 4096, 200) == 'f32'
    # outside the 16-bit mode's envelope (few columns / few components: weak averaging of its rounding noise): fp32
    assert nmf.resolve_precision('auto', 4000000, 64, 50) == 'f32' and nmf.resolve_precision('auto', 1000000, 4096, 8) == 'f32'
    assert nmf.resolve_precision('auto', 1000000, 256, 16) == 'f16'
    # ... unless the rows exceed what one context of the exact modes holds (65 535 x 64: klnmf_set_problem refuses beyond):
    # the 16-bit path then runs it, as 'auto' did before the envelope rule, and says so (the note's text:
    # test_f16_outside_its_envelope_is_never_silent)
    assert nmf.MAX_ROWS_EXACT == 65535 * 64
    assert nmf.resolve_precision('auto', nmf.MAX_ROWS_EXACT, 64, 50) == 'f32'
    assert nmf.resolve_precision('auto', 10000000, 64, 50) == 'f16'
    # k > 512: the 16-bit modes hand the problem to the fp32 kernels instead of refusing it; the exact modes are untouched
    assert nmf.resolve_precision('f16', 5000, 1200, 600) == 'f32' and nmf.resolve_precision('auto', 500000, 4096, 600) == 'f32'
    assert nmf.resolve_precision('f16', 5000, 1200, 512) == 'f16' and nmf.resolve_precision('f64', 5000, 1200, 600) == 'f64'
    assert nmf._default_precision() in ('f64', os.environ.get('KLNMF_PRECISION'))
    m = nmf.KLdivNMF(n_components=3, precision='auto')
    assert m._sparse_route(sp.csr_matrix(np.eye(3)))                        # sparse input: the exact sparse branch


def test_bench_power_clock_sampler_is_harmless_without_a_card():
    """bench.py's rocm-smi sampler is informative only: where rocm-smi is missing or reports nothing (this container) it yields
    None and never raises."""
    import time
    import bench
    with bench.PowerClockSampler(0) as sampler:
        time.sleep(0.3)
    assert sampler.summary() is None or 'sclk_mhz_median' in sampler.summary()


def test_every_launched_rowpass4_instantiation_is_in_the_list():
    """The k_rowpass4 instantiations are named in ONE place, the X-macro lists of rowpass4_list.hip.h: rowpass4_inst_*.hip define
    them, ctx.hip.h declares them `extern`, and the launch looks its kernel up in a table built from the same lists (a
    static_assert there proves that the lists and the table's index cover each other).  An instantiation named anywhere else
    would be compiled a second time, silently, in the unit that names it.
    (a) on the text: under csrc/ the template-id `k_rowpass4<` is only ever followed by the lists' macro parameters;
    (b) on the built library: its gfx950 code objects define 264 distinct k_rowpass4 kernels, each exactly once -- nothing
    compiled twice, nothing compiled outside the lists."""
    import collections
    import glob
    import re
    import subprocess
    import sys
    import tempfile
    import __graft_entry__ as ge
    params = 'KT, ODD, MODE, EP, NW, SPLIT, Q8>'
    for path in sorted(glob.glob(os.path.join(ge.CSRC, '*.hip')) + glob.glob(os.path.join(ge.CSRC, '*.hip.h'))):
        text = open(path).read()
        for m in re.finditer(r'k_rowpass4<', text):
            assert text.startswith(params, m.end()), (os.path.basename(path), text[m.start():m.end() + 40])
    lst = open(os.path.join(ge.CSRC, 'rowpass4_list.hip.h')).read()
    assert 'static_assert(rowpass4_lists_match_index()' in lst
    if not os.path.exists(ge.LIB):
        pytest.skip('libklnmf.so has not been built')
    sys.path.insert(0, os.path.join(ge.ROOT, 'scripts'))
    try:
        import kernel_fingerprint as kf
    finally:
        sys.path.pop(0)
    defined = collections.Counter()
    with tempfile.TemporaryDirectory() as tmp:
        for co in kf.device_code(ge.LIB, tmp):
            table = subprocess.run([kf.OBJDUMP, '-t', co], capture_output=True, text=True, check=True).stdout
            for line in table.splitlines():
                cols = line.split()
                if 'k_rowpass4' in line and ' F ' in line and not cols[-1].endswith('.kd'):
                    defined[cols[-1]] += 1
    assert len(defined) == 7 * 32 + 5 * 8, len(defined)
    assert set(defined.values()) == {1}, [name for name, count in defined.items() if count != 1]


def test_csr_input_and_large_k_never_change_arithmetic_silently(capsys):
    """Round-3 verdict: CSR input in a 16-bit mode was densified (another algorithm: off X's structure the dense ratio is
    eps / (W.H + eps), not 0) and k > 512 went to the fp32 kernels without a word.  Both now name the arithmetic that runs,
    once per process, on stderr; CSR input always takes the sparse kernels."""
    from multimodal_amd.lib import nmf as nm
    nm._NOTED.clear()
    assert nm.sparse_precision('auto') == 'f64' and nm.sparse_precision('f64') == 'f64' and nm.sparse_precision('f32') == 'f32'
    assert capsys.readouterr().err == ''
    assert nm.sparse_precision('f16') == 'f32' and nm.sparse_precision('f16') == 'f32'
    err = capsys.readouterr().err
    assert err.count("CSR input with precision='f16' runs the reference's sparse branch") == 1
    assert nm.resolve_precision('f16', 1000, 300, 512) == 'f16'
    assert capsys.readouterr().err == ''
    assert nm.resolve_precision('f16', 1000, 100, 600) == 'f32' and nm.resolve_precision('f16', 10, 10, 700) == 'f32'
    err = capsys.readouterr().err
    assert err.count("k = 600 runs on the fp32 kernels") == 1 and 'k = 700' not in err
    import scipy.sparse as sp
    m = nm.KLdivNMF(n_components=3, precision='f16')
    assert m._sparse_route(sp.csr_matrix(np.eye(3))) and not m._sparse_route(np.eye(3))


def test_f16_outside_its_envelope_is_never_silent(capsys):
    """Round-5 verdict: an explicit precision='f16' on a shape outside the mode's accuracy envelope (f < 256 or k < 16: final KL
    up to 5e-4 off the reference's) ran without a word.  It is still honoured -- the caller asked for it --
    but says so once per process and cause on stderr; inside the envelope nothing is written; 'auto' beyond the exact modes'
    row limit says that it took the 16-bit path.  (The run-time half -- KL / sum(V) below 2e-3 -- needs a fit: GPU test.)"""
    from multimodal_amd.lib import nmf as nm
    nm._NOTED.clear()
    assert nm.resolve_precision('f16', 70000, 256, 16) == 'f16' and nm.resolve_precision('bf16', 70000, 4096, 200) == 'bf16'
    assert capsys.readouterr().err == ''
    assert nm.resolve_precision('f16', 70000, 64, 8) == 'f16' and nm.resolve_precision('f16', 500, 64, 8) == 'f16'
    err = capsys.readouterr().err
    assert err.count("outside the 16-bit mode's accuracy envelope") == 1 and "f = 64, k = 8" in err and "'f32' keeps 1e-6" in err
    assert nm.resolve_precision('f16', 70000, 4096, 8) == 'f16'          # another cause (k alone): its own line
    assert capsys.readouterr().err.count("outside the 16-bit mode's accuracy envelope") == 1
    assert nm.resolve_precision('f64', 70000, 64, 8) == 'f64' and nm.resolve_precision('f32', 70000, 64, 8) == 'f32'
    assert capsys.readouterr().err == ''
    assert nm.resolve_precision('auto', 10000000, 64, 50) == 'f16'
    err = capsys.readouterr().err
    assert "exceed one fp32 context" in err and "precision='f16'" in err
