"""precision='bf16x3' on the GPU: the exact fp32 mode's loop with its dense contractions on the split-operand bf16 kernel
(csrc/split3.hip.h).  Fits are held to 1e-4 of the reference on every recorded loss and on the true final KL (fp64
evaluation of the returned factors), len(errors) equal, unless a test says otherwise; single contractions to
2^-14 sum |a.b| per element (nonnegative operands here: a relative bound)."""
import contextlib
import io
import os

import numpy as np
import pytest
import scipy.sparse as sp
from numpy.testing import assert_allclose

from oracle import klnmf_oracle as orc
from tests import golden_inputs as gi
from tests.test_gpu_parity import fit_gpu
from multimodal_amd import _native
from multimodal_amd.lib import nmf

pytestmark = pytest.mark.gpu

CONTRACTION_RTOL = 2.0 ** -14


def _true_dev(X, W, H, ref):
    return abs(orc.kl_error(X, np.asarray(W, np.float64), np.asarray(H, np.float64)) - ref) / ref


def _fit_against_fixture(g, X, H0, tol=1e-4):
    k, iters = int(g['k']), int(g['iters'])
    nmf._NOTED.clear()
    m, W, errors, err_text = fit_gpu(X, H0, k, iters, 0, precision='bf16x3')
    assert len(errors) == len(g['errors']) == iters
    loss_dev = float(np.max(np.abs(errors - g['errors']) / g['errors']))
    final_dev = _true_dev(X, W, m.components_, float(g['final']))
    print('bf16x3: max loss deviation %.2e, final KL deviation %.2e' % (loss_dev, final_dev))
    assert loss_dev <= tol and final_dev <= tol
    return m, err_text


def test_g19_plateau_escape_within_1e4():
    """Fixture G19 (40 000 x 512, k = 16): the f16 mode ends 3.9e-4 / 1.3e-4 off here (test_gpu_parity.py); the numpy
    emulation of the split predicts 6e-7."""
    g = gi.load('g19_plateau_escape_150it')
    X, H0 = gi.steep_problem(int(g['n']), int(g['f']), int(g['k']))
    m, err_text = _fit_against_fixture(g, X, H0)
    assert 'so little residual' not in err_text and 'envelope' not in err_text


def test_g18_rank12_under_200_components_without_fp8_tiles():
    """Fixture G18 (70 000 x 256, k = 200): no fp8 tiles, no monitor, no envelope note."""
    g = gi.load('g18_rank12_k200_150it')
    n, f, k = int(g['n']), int(g['f']), int(g['k'])
    X, H0 = gi.low_rank_problem(int(g['seed']), n, f, 12, k)
    m, err_text = _fit_against_fixture(g, X, H0)
    rep = m.last_fp8_report
    assert not rep or rep.get('tile_iterations', 0) == 0, rep
    assert not rep or not rep.get('outside_f16_envelope'), rep
    assert 'so little residual' not in err_text and 'envelope' not in err_text


@pytest.mark.parametrize('name', ['g1_20x30_k3', 'g1_37x53_k7'])
def test_g1_small_fits_within_1e5(name):
    """f < 256 and k < 16: outside the f16 mode's envelope, no envelope here."""
    g = gi.load(name)
    k = int(g['k'])
    X, H0 = gi.gen_inputs(int(g['seed']), int(g['n']), int(g['f']), k)
    for it in g['iters']:
        nmf._NOTED.clear()
        m, W, errors, err_text = fit_gpu(X, H0, k, int(it), 0, precision='bf16x3')
        assert len(errors) == len(g['errors_%d' % it])
        assert_allclose(errors, g['errors_%d' % it], rtol=1e-5)
        assert _true_dev(X, W, m.components_, float(g['final_%d' % it])) <= 1e-5
        assert 'envelope' not in err_text


def _ctx(X, k, H, W=None):
    ctx = _native.Context('bf16x3', device=0)
    ctx.set_problem(X.shape[0], X.shape[1], k, 1)
    ctx.upload_blocks([X])
    ctx.set_H(H)
    if W is None:
        ctx.init_W()
    else:
        ctx.set_W(W)
    return ctx


def test_g3_single_steps_through_the_step_api():
    """klnmf_step_Q / W / H against the fp64 fixture.  W and H within 1e-5; Q is one contraction of k = 3 terms with no
    averaging, held to the contraction bound 2^-14 (the emulation of this fixture: 1.1e-5)."""
    g = gi.load('g3_steps')
    X, W, H = gi.g3_inputs(g)
    with _ctx(X, int(g['k']), H, W) as ctx:
        ctx.step_Q()
        assert_allclose(ctx.get_Q(), g['Q'], rtol=CONTRACTION_RTOL)
        ctx.step_W()
        assert_allclose(ctx.get_W(), g['Wn'], rtol=1e-5)
        ctx.step_H()
        assert_allclose(ctx.get_H(), g['Hn'], rtol=1e-5)


def test_g14_k500_against_the_reference():
    """Fixture G14 (65 536 x 3072, k = 500, 50 iterations): the f16 mode's largest k."""
    from multimodal_amd.learner import MultimodalLearner
    g = gi.load('g14_c5shape_k500_50it')
    n, k, iters = int(g['n']), int(g['k']), int(g['iters'])
    dims = [int(d) for d in g['dims']]
    blocks, coefs, H0 = gi.synthetic_modalities(int(g['seed']), n, dims, k)
    mods = ['m%d' % i for i in range(len(dims))]
    X = MultimodalLearner(mods, dims, coefs, k).stack_data(mods, blocks)
    del blocks
    _fit_against_fixture(g, X, H0)


def test_k600_against_the_oracle():
    """k = 600 > 512: beyond the f16 kernels' bound, no hand-off and no note."""
    n, f, k, iters = 3000, 700, 600, 8
    X = orc.synthetic_V(21, n, f, 40)
    H0 = orc.synthetic_H0(21, f, k)
    Wo, Ho, eo = orc.fit_transform(X, k=k, H0=H0, max_iter=iters, tol=0)
    nmf._NOTED.clear()
    m = nmf.KLdivNMF(n_components=k, max_iter=iters, tol=0, precision='bf16x3')
    m._init_dictionary = H0
    buf = io.StringIO()
    with contextlib.redirect_stderr(buf):
        W, e = m.fit_transform(X, return_errors=True)
    assert buf.getvalue() == ''
    assert len(e) == len(eo) == iters
    assert_allclose(e, eo, rtol=1e-4)
    assert _true_dev(X, W, m.components_, orc.kl_error(X, Wo, Ho)) <= 1e-4


def _contraction_check(got, A, B, rtol=CONTRACTION_RTOL):
    """got ~ A.B (fp64 of the fp32 operands) within rtol sum |a.b| per element."""
    A = np.asarray(A, np.float32).astype(np.float64)
    B = np.asarray(B, np.float32).astype(np.float64)
    bound = rtol * (np.abs(A) @ np.abs(B)) + 1e-37
    err = np.abs(np.asarray(got, np.float64) - A @ B)
    assert np.all(err <= bound), float(np.max(err / bound))


@pytest.mark.parametrize('n,f,k', [(77, 133, 19), (130, 301, 37), (16384, 300, 64), (1, 1, 1), (65, 17, 33)])
def test_step_contractions_on_ragged_shapes(n, f, k):
    """M, N, K off the 64 x 64 tile and the 32-step (and the 16 of the MFMA); W0 = V.H0^T (multiply = 0); the W rule on
    few rows (n k / 4096 output tiles below the CU count: the feature axis split into slabs, wsplit > 1) and on enough rows
    for one pass (16 384 x 64: wsplit = 1); the numerator W^T.Q over row chunks (nsplit > 1 from 128 rows)."""
    rs = np.random.RandomState(n + f + k)
    X = (rs.random_sample((n, f)) + 0.01).astype(np.float32)
    H = (rs.random_sample((k, f)) + 0.01).astype(np.float32)
    H /= H.sum(axis=1, keepdims=True)
    with _ctx(X, k, H) as ctx:
        W0 = ctx.get_W(dtype=np.float32)
        _contraction_check(W0, X, H.T)                                        # multiply = 0
        ctx.step_Q()
        Q = ctx.get_Q(dtype=np.float32)
        D = (X.astype(np.float64) + 1e-8) / Q.astype(np.float64) - 1e-8      # W.H as the ratio saw it
        WH = W0.astype(np.float64) @ H.astype(np.float64)
        assert np.all(np.abs(D - WH) <= (2 * CONTRACTION_RTOL) * WH + 1e-6 * np.abs(WH).max())
        ctx.step_W()
        W1 = ctx.get_W(dtype=np.float32)
        G = Q.astype(np.float64) @ H.T.astype(np.float64)
        assert np.all(np.abs(W1 - W0 * G) <= (CONTRACTION_RTOL + 2.0 ** -22) * np.abs(W0 * G))
        ctx.step_H()
        H1 = ctx.get_H(dtype=np.float64)
        N = W1.T.astype(np.float64) @ Q.astype(np.float64)
        Hr = H * N
        Hr /= Hr.sum(axis=1, keepdims=True)
        assert_allclose(H1, Hr, rtol=2 * CONTRACTION_RTOL + 2.0 ** -20)


def test_wide_magnitudes_within_a_row_and_a_column():
    """Entries from 1e-20 to 1e20 along every row of V and 1e-10 to 1e10 along the dictionary: products from 1e-30 to
    1e30, inside fp32's normal range (and so are the lo parts' products).  W0 = V.H^T (the plain contraction, multiply = 0)."""
    rs = np.random.RandomState(4)
    n, f, k = 150, 257, 45
    X = (rs.random_sample((n, f)) + 0.5) * 10.0 ** rs.uniform(-20, 20, (n, f))
    H = (rs.random_sample((k, f)) + 0.5) * 10.0 ** rs.uniform(-10, 10, (k, f))
    X = X.astype(np.float32)
    H = H.astype(np.float32)
    with _ctx(X, k, H) as ctx:
        _contraction_check(ctx.get_W(dtype=np.float32), X, H.T)


def test_csr_input_equals_f32_bit_for_bit_with_one_note():
    rs = np.random.RandomState(91)
    n, f, k = 60, 90, 5
    dense = np.abs(rs.random_sample((n, f))) * (rs.random_sample((n, f)) < .3)
    X = sp.csr_matrix(dense)
    H0 = orc.normalize_sum(np.abs(rs.random_sample((k, f))) + .01, axis=1)
    out = {}
    for prec in ('f32', 'bf16x3'):
        nmf._NOTED.clear()
        out[prec] = fit_gpu(X, H0, k, 12, 0, precision=prec)
    m32, W32, e32, _ = out['f32']
    mx3, Wx3, ex3, err_text = out['bf16x3']
    np.testing.assert_array_equal(Wx3, W32)
    np.testing.assert_array_equal(mx3.components_, m32.components_)
    np.testing.assert_array_equal(ex3, e32)
    assert err_text.count("CSR input with precision='bf16x3'") == 1


def test_non_default_eps_is_honoured():
    g = gi.load('g3_steps')
    X, W, H = gi.g3_inputs(g)
    res = {}
    for prec in ('f32', 'bf16x3'):
        m = nmf.KLdivNMF(n_components=int(g['k']), precision=prec)
        m.components_ = H.copy()
        res[prec] = (m._update(X, W, _fit=True, eps=1e-3), m.components_)
    assert_allclose(res['bf16x3'][0], res['f32'][0], rtol=1e-5)
    assert_allclose(res['bf16x3'][1], res['f32'][1], rtol=1e-5)
    Wr, Hr = orc.update_step(X, W, H)
    assert not np.allclose(res['bf16x3'][0], Wr, rtol=1e-4)        # eps = 1e-3 changed the result: it was used


def test_two_ranks_on_one_gpu_against_the_oracle(tmp_path):
    """ShardedKLNMF in bf16x3: two ranks on GPU 0 over gloo (the launcher of test_distributed_gpu.py) against the fp64 oracle."""
    import torch.multiprocessing as mp
    from tests.test_distributed_gpu import _worker, _free_port
    n, f, k, iters, world = 4096 + 96, 512, 40, 4, 2
    mp.spawn(_worker, args=(world, _free_port(), n, f, k, iters, 'bf16x3', str(tmp_path)), nprocs=world, join=True)
    X = orc.synthetic_V(77, n, f, k)
    H0 = orc.synthetic_H0(77, f, k)
    Wo, Ho, eo = orc.fit_transform(X.astype(np.float32).astype(np.float64), k=k, H0=H0, max_iter=iters, tol=0)
    res = [np.load(os.path.join(str(tmp_path), 'r%d.npz' % r)) for r in range(world)]
    np.testing.assert_array_equal(res[0]['H'], res[1]['H'])
    for r in res:
        assert len(r['errors']) == iters
        assert_allclose(r['errors'], eo, rtol=1e-5)
        assert_allclose(r['H'], Ho, rtol=1e-3, atol=1e-7)
        assert_allclose(r['W'], Wo, rtol=1e-3, atol=1e-6 * np.abs(Wo).max())
