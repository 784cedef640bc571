"""A group of contexts (klnmf_group_*: include/klnmf.h) on repeated device 0: the N-shard loop with its exchange kernels
(csrc/group.hip.h), the agreed loop entry and the fp8 regime run for real on one GPU.  Every group is checked against one
context (f64: the same arithmetic up to the loss's summation order) or the fp64 oracle, and its replicas of H bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

from oracle import klnmf_oracle as orc
from tests import golden_inputs as gi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bounds(n, parts):
    """Row ranges of `parts` shards of n rows, as even as possible (the C-ABI takes any shard sizes)."""
    cuts = [n * i // parts for i in range(parts + 1)]
    return [(cuts[i], cuts[i + 1]) for i in range(parts)]


def _group_fit(X, H0, k, iters, tol, precision, bounds, fit=True, H_loop=None):
    """The loop through _native.Group on contexts of device 0 (one per row range); returns W, the H of every shard, errors and
    every shard's fp8 report."""
    from multimodal_amd import _native
    n, f = X.shape
    ctxs = []
    try:
        for r0, r1 in bounds:
            c = _native.Context(precision, device=0)
            ctxs.append(c)
            c.set_problem(r1 - r0, f, k, iters)
            c.set_v_max(float(X.max()))
            c.upload_V(X[r0:r1])
            c.set_H(H0)
            c.init_W()
            if H_loop is not None:
                c.set_H(H_loop)
        with _native.Group(ctxs) as g:
            errors, n_done, stopped = g.run(n, iters, fit, tol)
        W = np.vstack([c.get_W() for c in ctxs])
        Hs = [c.get_H(dtype=np.float64 if precision == 'f64' else np.float32) for c in ctxs]
        reps = [c.fp8_report() for c in ctxs]
        return W, Hs, errors, reps
    finally:
        for c in ctxs:
            c.close()


def _single_fit(X, H0, k, iters, tol, precision, fit=True, H_loop=None):
    from multimodal_amd import _native
    n, f = X.shape
    with _native.Context(precision, device=0) as c:
        c.set_problem(n, f, k, iters)
        c.set_v_max(float(X.max()))
        c.upload_V(X)
        c.set_H(H0)
        c.init_W()
        if H_loop is not None:
            c.set_H(H_loop)
        errors, _, _ = c.run(iters, fit, tol * n * f)
        return c.get_W(), c.get_H(), errors


@pytest.mark.parametrize('n_dev', [2, 3, 8])
@pytest.mark.parametrize('f64', [False, True])
def test_exchange_selftest_is_bit_exact_on_ragged_counts(n_dev, f64):
    """Both phases of the exchange on values whose sum depends on the order of summation (1e8, 1, -1e8, subnormals): every
    element of every buffer equals the host's sum in shard order, bit for bit, for counts that divide by neither the number of
    buffers nor the vector width, counts smaller than one vector per buffer, and none."""
    from multimodal_amd import _native
    for count in (0, 1, 3, 4 * n_dev - 1, 4 * n_dev + 1, 1000, 65537, 819203):
        assert _native.group_selftest([0] * n_dev, count, f64=f64) == 0, count


def _f64_cases():
    g = gi.load('g1_500x1000_k10')
    X1, H1 = gi.gen_inputs(int(g['seed']), int(g['n']), int(g['f']), int(g['k']))
    g4 = gi.load('g4_tol')
    X4, H4 = gi.gen_inputs(int(g4['seed']), int(g4['n']), int(g4['f']), int(g4['k']))
    X3, H3 = orc.synthetic_V(31, 3000, 512, 24), orc.synthetic_H0(31, 512, 24)
    return [('g1', X1, H1, int(g['k']), 50, 0.0), ('g4', X4, H4, int(g4['k']), 200, 1e-6), ('g4b', X4, H4, int(g4['k']), 200, 1e-3),
            ('3000x512', X3, H3, 24, 40, 1e-5)]


@pytest.mark.parametrize('parts', [2, 3])
def test_f64_group_matches_one_context(parts):
    """f64 over 2 and 3 shards equals one context up to the loss's summation order: losses within 1e-12, W and H within 1e-10,
    the stop rule fires in the same iteration (tol > 0), every replica of H bit-identical."""
    for name, X, H0, k, iters, tol in _f64_cases():
        W, Hs, e, _ = _group_fit(X, H0, k, iters, tol, 'f64', _bounds(X.shape[0], parts))
        Ws, Hss, es = _single_fit(X, H0, k, iters, tol, 'f64')
        assert len(e) == len(es), name
        assert_allclose(e, es, rtol=1e-12, err_msg=name)
        assert_allclose(W, Ws, rtol=1e-10, atol=1e-14, err_msg=name)
        for H in Hs:
            assert_array_equal(H, Hs[0])
        assert_allclose(Hs[0], Hss, rtol=1e-10, atol=1e-15, err_msg=name)


def test_kldivnmf_device_list_matches_device_0_on_g1():
    """The public path: KLdivNMF(device=[0, 0]) and [0, 0, 0] against device=0 on G1 (f64)."""
    from multimodal_amd.lib.nmf import KLdivNMF
    g = gi.load('g1_500x1000_k10')
    X, H0 = gi.gen_inputs(int(g['seed']), int(g['n']), int(g['f']), int(g['k']))
    outs = []
    for dev in (0, [0, 0], [0, 0, 0]):
        m = KLdivNMF(n_components=int(g['k']), max_iter=50, tol=0, precision='f64', device=dev)
        m._init_dictionary = H0
        W, e = m.fit_transform(X, return_errors=True)
        outs.append((W, m.components_, e))
    for W, H, e in outs[1:]:
        assert_allclose(e, outs[0][2], rtol=1e-12)
        assert_allclose(W, outs[0][0], rtol=1e-10, atol=1e-14)
        assert_allclose(H, outs[0][1], rtol=1e-10, atol=1e-15)
    assert_allclose(outs[1][2], g['errors_50'], rtol=1e-10)


@pytest.mark.parametrize('precision', ['f32', 'bf16x3', 'f16x3'])
def test_fp32_grade_modes_on_a_group_match_the_oracle(precision):
    from multimodal_amd.lib.nmf import KLdivNMF
    n, f, k, iters = 3000, 512, 24, 20
    X, H0 = orc.synthetic_V(33, n, f, k), orc.synthetic_H0(33, f, k)
    m = KLdivNMF(n_components=k, max_iter=iters, tol=0, precision=precision, device=[0, 0, 0])
    m._init_dictionary = H0
    W, e = m.fit_transform(X, return_errors=True)
    Wo, Ho, eo = orc.fit_transform(X, k=k, H0=H0, max_iter=iters, tol=0)
    assert len(e) == iters
    assert_allclose(e, eo, rtol=1e-5)
    fo = orc.kl_error(X, Wo, Ho)
    assert abs(orc.kl_error(X, W, m.components_) - fo) <= 1e-5 * fo


@pytest.mark.parametrize('parts,rows', [(2, 66016), (4, 33024)])
def test_f16_fp8_regime_on_a_group(parts, rows):
    """What test_distributed_gpu's torch-sequenced ranks run (2 x 66 016 rows: also the fp8 x fp8 column pass; 4 x 33 024: fp8
    tiles under f16 W operands), as one group: every shard takes the tiles in the same 28 iterations, the replicas stay
    bit-identical, every loss and the final KL of the gathered factors are within 1e-4 of the oracle's."""
    n, f, k, iters = parts * rows, 256, 200, 30
    X, H0 = orc.synthetic_V(21, n, f, k), orc.synthetic_H0(21, f, k)
    from multimodal_amd.lib.nmf import shard_plan
    bounds = [b for _, b in shard_plan(n, [0] * parts)]
    assert [b - a for a, b in bounds] == [rows] * parts
    W, Hs, e, reps = _group_fit(X, H0, k, iters, 0.0, 'f16', bounds)
    for H in Hs:
        assert_array_equal(H, Hs[0])
    for rep in reps:
        assert rep['allowed'] and rep['tile_iterations'] == iters - 2 and not rep['gave_up'], rep
        assert rep['column_pass_iterations'] == reps[0]['column_pass_iterations']
    Wo, Ho, eo = orc.fit_transform(X, k=k, H0=H0, max_iter=iters, tol=0)
    assert len(e) == iters
    assert_allclose(e, eo, rtol=1e-4)
    fo = orc.kl_error(X, Wo, Ho)
    assert abs(orc.kl_error(X, W, Hs[0].astype(np.float64)) - fo) <= 1e-4 * fo


def test_f16_shards_straddling_the_fp8_row_threshold_stay_on_16_bit_tiles():
    """32 800 + 32 768 rows: the first shard's shape allows fp8 tiles, the second's does not -- agreed at the loop's entry,
    every shard runs 16-bit tiles."""
    n, f, k, iters = 65568, 256, 40, 6
    X, H0 = orc.synthetic_V(13, n, f, k), orc.synthetic_H0(13, f, k)
    W, Hs, e, reps = _group_fit(X, H0, k, iters, 0.0, 'f16', [(0, 32800), (32800, n)])
    for rep in reps:
        assert not rep['allowed'] and rep['tile_iterations'] == 0, rep
    _, _, eo = orc.fit_transform(X, k=k, H0=H0, max_iter=iters, tol=0)
    assert_allclose(e, eo, rtol=1e-4)


def test_group_runs_are_deterministic():
    n, f, k, iters = 3000, 512, 24, 12
    X, H0 = orc.synthetic_V(35, n, f, k), orc.synthetic_H0(35, f, k)
    for precision in ('f16', 'f32'):
        a = _group_fit(X, H0, k, iters, 0.0, precision, _bounds(n, 3))
        b = _group_fit(X, H0, k, iters, 0.0, precision, _bounds(n, 3))
        assert_array_equal(a[0], b[0])
        assert_array_equal(a[1][0], b[1][0])
        assert a[2] == b[2]


def test_transform_on_a_group_matches_one_context():
    from multimodal_amd.lib.nmf import KLdivNMF
    g = gi.load('g2_transform')
    X, H0, Xt = gi.g2_inputs(g)
    k = int(g['k'])
    Xt2 = np.abs(np.random.RandomState(5).random_sample((100, X.shape[1])))      # (4 row tiles: 2 shards)
    outs = []
    for dev in (0, [0, 0]):
        t = KLdivNMF(n_components=k, max_iter=25, tol=0, precision='f64', device=dev)
        t._init_dictionary = H0
        t.fit(X)
        outs.append([t.transform(x, return_errors=True) for x in (Xt, Xt2)])
    for (Wg, eg), (Ws, es) in zip(outs[1], outs[0]):
        assert_allclose(eg, es, rtol=1e-12)
        assert_allclose(Wg, Ws, rtol=1e-10, atol=1e-14)
    # ... and a transform of more rows than one shard on the low-level group: the loss alone is exchanged
    n, f = 640, 96
    Xb, Hb = orc.synthetic_V(37, n, f, 8), orc.synthetic_H0(37, f, 8)
    W, Hs, e, _ = _group_fit(Xb, Hb, 8, 15, 0.0, 'f64', _bounds(n, 4), fit=False)
    Ws, Hss, es = _single_fit(Xb, Hb, 8, 15, 0.0, 'f64', fit=False)
    assert_allclose(e, es, rtol=1e-12)
    assert_allclose(W, Ws, rtol=1e-10, atol=1e-14)
    assert_array_equal(Hs[0], Hss)


_CHILD = r'''
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from multimodal_amd.learner import MultimodalLearner, fit_coefficients
rs = np.random.RandomState(3)
a = rs.random_sample((400, 40)); b = rs.random_sample((400, 30))
np.random.seed(11)
lrn = MultimodalLearner(['a', 'b'], [40, 30], [1., 2.], 8)
lrn.train([a, b], 30)
coef = fit_coefficients(rs.random_sample((200, 40)), lrn.get_dico('a'), iter_nmf=20)
rec = lrn.reconstruct_internal('a', a[:100], 20)
np.savez(sys.argv[2], dico=lrn.dico, coef=coef, rec=rec)
'''


def test_learner_and_fit_coefficients_with_klnmf_devices():
    """MultimodalLearner.train, fit_coefficients and reconstruct_internal unchanged, in a child process with KLNMF_DEVICES=0,0
    against the same calls with KLNMF_DEVICE=0."""
    import tempfile
    outs = []
    with tempfile.TemporaryDirectory() as tmp:
        for key, value in (('KLNMF_DEVICE', '0'), ('KLNMF_DEVICES', '0,0')):
            env = {k: v for k, v in os.environ.items() if k not in ('KLNMF_DEVICE', 'KLNMF_DEVICES')}
            env[key] = value
            env['KLNMF_PRECISION'] = 'f64'
            out = os.path.join(tmp, key + '.npz')
            subprocess.run([sys.executable, '-c', _CHILD, ROOT, out], env=env, check=True, timeout=300)
            outs.append(np.load(out))
    for name in ('dico', 'coef', 'rec'):
        assert_allclose(outs[1][name], outs[0][name], rtol=1e-10, atol=1e-14, err_msg=name)


def test_eight_contexts_on_one_device():
    """[0] * 8: eight streams of one device share its hardware queues; the host's enqueue order keeps every event record ahead
    of every wait on it, so the group runs (and matches one context)."""
    from multimodal_amd.lib.nmf import KLdivNMF
    n, f, k, iters = 3000, 512, 24, 20
    X, H0 = orc.synthetic_V(39, n, f, k), orc.synthetic_H0(39, f, k)
    outs = []
    for dev in (0, [0] * 8):
        m = KLdivNMF(n_components=k, max_iter=iters, tol=1e-6, precision='f64', device=dev)
        m._init_dictionary = H0
        W, e = m.fit_transform(X, return_errors=True)
        outs.append((W, m.components_, e))
    assert len(outs[1][2]) == len(outs[0][2])
    assert_allclose(outs[1][2], outs[0][2], rtol=1e-12)
    assert_allclose(outs[1][0], outs[0][0], rtol=1e-10, atol=1e-14)
    assert_allclose(outs[1][1], outs[0][1], rtol=1e-10, atol=1e-15)
    # ... and in the 16-bit mode, with the replicas compared inside klnmf_group_run
    W, Hs, e, _ = _group_fit(X, H0, k, iters, 0.0, 'f16', _bounds(n, 8))
    assert len(e) == iters and all(np.isfinite(e))


def test_a_refused_shard_refuses_the_whole_group_and_the_contexts_stay_usable():
    """Shard 1's factors beyond the fp16 operand range (test_gpu_parity's refused case: rows spanning 2^18 in mass, an initial
    dictionary 5000 times too heavy -- shard 0 holds the same rows with a sane one): klnmf_group_run fails on every shard before
    anything is enqueued, naming the shard; with a sane dictionary the same contexts then run the group."""
    from multimodal_amd import _native
    n, f, k, iters = 520, 300, 40, 5
    X = orc.synthetic_V(8, n, f, k)
    X[:40] *= 2.0 ** 9
    X[40:80] *= 2.0 ** -9
    H0 = orc.synthetic_H0(8, f, k)
    Xs = np.vstack([X, X])
    bounds = [(0, n), (n, 2 * n)]
    ctxs = [_native.Context('f16', device=0) for _ in bounds]
    try:
        for i, (c, (r0, r1)) in enumerate(zip(ctxs, bounds)):
            c.set_problem(r1 - r0, f, k, iters)
            c.set_v_max(float(Xs.max()))
            c.upload_V(Xs[r0:r1])
            c.set_H(H0 * 5e3 if i == 1 else H0)
            c.init_W()
        with _native.Group(ctxs) as g:
            with pytest.raises(_native.NativeError) as ei:
                g.run(2 * n, iters, True, 0.0)
            assert 'shard 1' in str(ei.value) and 'operand range' in str(ei.value), str(ei.value)
            assert ei.value.code == _native.ERR_UNSUPP
            ctxs[1].set_H(H0)
            ctxs[1].init_W()
            errors, n_done, _ = g.run(2 * n, iters, True, 0.0)
        assert n_done == iters
        W = np.vstack([c.get_W() for c in ctxs])
    finally:
        for c in ctxs:
            c.close()
    W2, Hs, e2, _ = _group_fit(Xs, H0, k, iters, 0.0, 'f16', bounds)
    assert errors == e2
    assert_array_equal(W, W2)
