"""precision='f16x3' on the GPU: the fp32 mode's storage with the loop's row pass (loss + ratio + W rule) and column pass fused
on split fp16 operands (csrc/f16x3.hip.h).  Fits are held to 2e-5 of the reference on every recorded loss and on the true final
KL (fp64 evaluation of the returned factors), len(errors) equal, unless a test says otherwise."""
import contextlib
import io
import os

import numpy as np
import pytest
from numpy.testing import assert_allclose

from oracle import klnmf_oracle as orc
from tests import golden_inputs as gi
from tests.test_gpu_parity import fit_gpu
from multimodal_amd import _native
from multimodal_amd.lib import nmf

pytestmark = pytest.mark.gpu

TOL = 2e-5
STEP_RTOL = 2.0 ** -18


def _true_dev(X, W, H, ref):
    return abs(orc.kl_error(X, np.asarray(W, np.float64), np.asarray(H, np.float64)) - ref) / ref


def _devs(X, H0, k, iters, ref_errors, ref_final, precision='f16x3'):
    nmf._NOTED.clear()
    m, W, errors, err_text = fit_gpu(X, H0, k, iters, 0, precision=precision)
    assert len(errors) == len(ref_errors) == iters
    loss_dev = float(np.max(np.abs(errors - ref_errors) / ref_errors))
    final_dev = _true_dev(X, W, m.components_, float(ref_final))
    print('%s: max loss deviation %.2e, final KL deviation %.2e' % (precision, loss_dev, final_dev))
    return loss_dev, final_dev, m, W, err_text


def test_g19_within_2e5_where_f16_misses_1e4():
    """Fixture G19 (40 000 x 512, k = 16, 150 iterations): the emulation predicts 8.6e-7."""
    g = gi.load('g19_plateau_escape_150it')
    k, iters = int(g['k']), int(g['iters'])
    X, H0 = gi.steep_problem(int(g['n']), int(g['f']), k)
    loss_dev, final_dev, _, _, err_text = _devs(X, H0, k, iters, g['errors'], g['final'])
    assert loss_dev <= TOL and final_dev <= TOL
    assert err_text == ''
    f16_loss, f16_final, _, _, _ = _devs(X, H0, k, iters, g['errors'], g['final'], precision='f16')
    assert max(f16_loss, f16_final) > 1e-4          # what the mode adds


def test_g18_within_2e5():
    g = gi.load('g18_rank12_k200_150it')
    n, f, k, iters = int(g['n']), int(g['f']), int(g['k']), int(g['iters'])
    X, H0 = gi.low_rank_problem(int(g['seed']), n, f, 12, k)
    loss_dev, final_dev, m, _, err_text = _devs(X, H0, k, iters, g['errors'], g['final'])
    assert loss_dev <= TOL and final_dev <= TOL
    assert err_text == ''


@pytest.mark.parametrize('name', ['g11_c4shape_50it', 'g12_c2shape_200it', 'g17_c2kind_40000rows_200it'])
def test_configuration_fixtures_within_2e5(name):
    g = gi.load(name)
    n, f, k, iters = int(g['n']), int(g['f']), int(g['k']), int(g['iters'])
    X, H0 = gi.synthetic_problem(int(g['seed']), n, f, k)
    loss_dev, final_dev, _, _, _ = _devs(X, H0, k, iters, g['errors'], g['final'])
    assert loss_dev <= TOL and final_dev <= TOL


@pytest.mark.parametrize('name', ['g1_20x30_k3', 'g1_37x53_k7', 'g1_500x1000_k10'])
def test_g1_within_1e5(name):
    g = gi.load(name)
    k = int(g['k'])
    X, H0 = gi.gen_inputs(int(g['seed']), int(g['n']), int(g['f']), k)
    for it in g['iters']:
        nmf._NOTED.clear()
        m, W, errors, _ = fit_gpu(X, H0, k, int(it), 0, precision='f16x3')
        assert len(errors) == len(g['errors_%d' % it])
        assert_allclose(errors, g['errors_%d' % it], rtol=1e-5)
        assert _true_dev(X, W, m.components_, float(g['final_%d' % it])) <= 1e-5


def test_g3_single_steps_within_2_18_of_sum_abs():
    g = gi.load('g3_steps')
    X, W, H = gi.g3_inputs(g)
    k = int(g['k'])
    ctx = _native.Context('f16x3', device=0)
    with ctx:
        ctx.set_problem(X.shape[0], X.shape[1], k, 1)
        ctx.upload_blocks([X])
        ctx.set_H(H)
        ctx.set_W(W)
        ctx.step_Q()
        Q = ctx.get_Q()
        X32, W32, H32 = (np.asarray(a, np.float32).astype(np.float64) for a in (X, W, H))
        WH = W32 @ H32
        D = (X32 + 1e-8) / Q - 1e-8
        assert np.all(np.abs(D - WH) <= STEP_RTOL * WH + 1e-6 * WH.max())
        assert_allclose(Q, g['Q'], rtol=1e-5)
        ctx.step_W()
        assert_allclose(ctx.get_W(), g['Wn'], rtol=1e-5)
        ctx.step_H()
        assert_allclose(ctx.get_H(), g['Hn'], rtol=1e-5)


def test_g2_transform():
    g = gi.load('g2_transform')
    X, H0, Xt = gi.g2_inputs(g)
    t = nmf.KLdivNMF(n_components=int(g['k']), max_iter=25, tol=0, precision='f16x3')
    t.components_ = g['H']
    Wt, et = t.transform(Xt, return_errors=True, scale_W=True)
    assert_allclose(et, g['errors_t'], rtol=TOL)
    assert_allclose(Wt, g['Wt'], rtol=1e-3, atol=1e-6 * np.abs(g['Wt']).max())
    assert (t.components_ == g['H']).all()


def test_g5_through_the_learner(monkeypatch):
    """Fixture G5: MultimodalLearner.train (20 iterations) with KLNMF_PRECISION=f16x3 -- the dictionary and one
    reconstruction against the reference's."""
    from multimodal_amd.learner import MultimodalLearner
    import multimodal_amd.learner as L
    g = gi.load('g5_learner2')
    blocks, dims, H0, test = gi.g5_inputs(g)
    coefs = [float(c) for c in g['coefs']]
    mods = ['m%d' % i for i in range(len(dims))]
    k = int(g['k'])
    monkeypatch.setenv('KLNMF_PRECISION', 'f16x3')
    orig = L.NMF
    seen = []

    def factory(**kw):
        m = orig(**kw)
        m._init_dictionary = H0.copy()
        seen.append(m.precision)
        return m
    monkeypatch.setattr(L, 'NMF', factory)
    lr = MultimodalLearner(mods, dims, coefs, k)
    lr.train(blocks, 20)
    assert seen and set(seen) == {'f16x3'}
    assert_allclose(lr.dico, g['dico'], rtol=1e-3, atol=1e-4 * np.abs(g['dico']).max())
    got = lr.reconstruct_internal(mods[0], test[0], 15)
    assert_allclose(got, g['internal_0'], rtol=1e-3, atol=1e-4 * np.abs(g['internal_0']).max())


def _oracle_devs(X, k, iters, H0=None, seed=0, **kw):
    X = np.asarray(X, np.float32).astype(np.float64)
    if H0 is None:
        H0 = orc.normalize_sum(np.random.RandomState(seed).random_sample((k, X.shape[1])) + .01, axis=1)
    Wo, Ho, eo = orc.fit_transform(X, k=k, H0=H0, max_iter=iters, tol=-np.inf, warn=False)
    nmf._NOTED.clear()
    m, W, e, err_text = fit_gpu(X, H0, k, iters, -np.inf, precision='f16x3')
    assert len(e) == len(eo) == iters
    # A recorded loss is the fp32 mode's: each element's term x log q - x + y is rounded in fp32 before the fp64 sum, so it
    # cannot come closer than about 2^-24 sum(V) to the reference's.  A fit that becomes exact (n = 1, f = 1, k >= n or f:
    # a loss of 1e-15) is held to that floor, 2^-23 sum(V); every other fit to TOL of its loss.
    floor = 2.0 ** -23 * X.sum() / TOL
    eo = np.asarray(eo)
    loss_dev = float(np.max(np.abs(e - eo) / np.maximum(np.abs(eo), floor)))
    ref = orc.kl_error(X, Wo, Ho)
    final_dev = abs(orc.kl_error(X, np.asarray(W, np.float64), np.asarray(m.components_, np.float64)) - ref) / max(abs(ref), floor)
    return loss_dev, final_dev, m, W, err_text


RAGGED = [(1, 255, 16), (31, 7, 1), (31, 4097, 15), (65537, 7, 33), (65537, 1, 1), (31, 255, 256), (200, 1, 200),
          (1, 4097, 256), (65537, 255, 16), (31, 7, 200), (200, 4097, 33), (65537, 7, 256)]


@pytest.mark.parametrize('n,f,k', RAGGED)
def test_ragged_shapes_against_the_oracle(n, f, k):
    rs = np.random.RandomState(n + 3 * f + 7 * k)
    X = rs.gamma(1.0, 1.0, (n, f)) + 0.01
    loss_dev, final_dev, _, _, _ = _oracle_devs(X, k, 6, seed=k)
    assert loss_dev <= TOL and final_dev <= TOL


def test_a_zero_row_gives_an_exactly_zero_w_row():
    rs = np.random.RandomState(8)
    X = rs.gamma(1.0, 1.0, (300, 130)) + 0.01
    X[17] = 0.0
    X[299] = 0.0
    loss_dev, final_dev, m, W, _ = _oracle_devs(X, 20, 8, seed=2)
    assert np.all(W[17] == 0) and np.all(W[299] == 0)
    assert loss_dev <= TOL and final_dev <= TOL


@pytest.mark.parametrize('scale', [1e-9, 1e9])
def test_scaled_data(scale):
    rs = np.random.RandomState(11)
    X = (rs.gamma(1.0, 1.0, (500, 300)).dot(rs.gamma(0.5, 1.0, (300, 300))) / 300 + 0.05) * scale
    loss_dev, final_dev, _, _, _ = _oracle_devs(X, 24, 10, seed=3)
    assert loss_dev <= TOL and final_dev <= TOL


def test_worst_first_ratio():
    """One entry 1e4 x the rest (scripts/data_fuzz.py's worst first-ratio case): a ratio far above fp16's range on the first
    update; the per-row tile scales keep it."""
    rs = np.random.RandomState(12)
    X = rs.random_sample((400, 333)) + 0.01
    X[123, 45] = 1e4 * X.max()
    loss_dev, final_dev, _, _, _ = _oracle_devs(X, 16, 8, seed=4)
    assert loss_dev <= TOL and final_dev <= TOL


def test_non_default_eps_is_honoured():
    g = gi.load('g3_steps')
    X, W, H = gi.g3_inputs(g)
    res = {}
    for prec in ('f32', 'f16x3'):
        m = nmf.KLdivNMF(n_components=int(g['k']), precision=prec)
        m.components_ = H.copy()
        res[prec] = (m._update(X, W, _fit=True, eps=1e-3), m.components_)
    assert_allclose(res['f16x3'][0], res['f32'][0], rtol=1e-5)
    assert_allclose(res['f16x3'][1], res['f32'][1], rtol=1e-5)
    Wr, Hr = orc.update_step(X, W, H)
    assert not np.allclose(res['f16x3'][0], Wr, rtol=1e-4)


def test_k300_runs_on_bf16x3_with_one_note():
    n, f, k, iters = 800, 400, 300, 5
    X = orc.synthetic_V(31, n, f, 20)
    H0 = orc.synthetic_H0(31, f, k)
    Wo, Ho, eo = orc.fit_transform(X, k=k, H0=H0, max_iter=iters, tol=0)
    nmf._NOTED.clear()
    m, W, e, err_text = fit_gpu(X, H0, k, iters, 0, precision='f16x3')
    assert err_text.count('\n') == 1 and "precision='bf16x3'" in err_text
    assert len(e) == len(eo) == iters
    assert_allclose(e, eo, rtol=1e-4)


def test_two_ranks_on_one_gpu_against_the_oracle(tmp_path):
    """ShardedKLNMF in f16x3: two ranks on GPU 0 over gloo (the launcher of test_distributed_gpu.py) against the fp64 oracle."""
    import torch.multiprocessing as mp
    from tests.test_distributed_gpu import _worker, _free_port
    n, f, k, iters, world = 4096 + 96, 512, 40, 4, 2
    mp.spawn(_worker, args=(world, _free_port(), n, f, k, iters, 'f16x3', str(tmp_path)), nprocs=world, join=True)
    X = orc.synthetic_V(77, n, f, k)
    H0 = orc.synthetic_H0(77, f, k)
    Wo, Ho, eo = orc.fit_transform(X.astype(np.float32).astype(np.float64), k=k, H0=H0, max_iter=iters, tol=0)
    res = [np.load(os.path.join(str(tmp_path), 'r%d.npz' % r)) for r in range(world)]
    np.testing.assert_array_equal(res[0]['H'], res[1]['H'])
    for r in res:
        assert len(r['errors']) == iters
        assert_allclose(r['errors'], eo, rtol=TOL)
        assert_allclose(r['H'], Ho, rtol=1e-3, atol=1e-7)
        assert_allclose(r['W'], Wo, rtol=1e-3, atol=1e-6 * np.abs(Wo).max())
