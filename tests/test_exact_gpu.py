"""The dense exact-mode kernels (multimodal_amd/csrc/exact.hip.h, split3.hip.h, f16x3.hip.h) against the fp64 reference on
every route of their dispatch (tests/exact_cases.py).

Driven through `_native.Context` directly, so that every test can assert which route ran (`exact_regime()`:
KLNMF_Q_EX_ROW_CHUNKS / _W_CHUNKS / _H_SEGMENTS / _H_FROM_SLABS) against the host rule restated for the device's own CU
count:
  * every case of exact_cases.CASES in f64 and f32: one step (the loss pass alone, step_Q, step_W, step_H), W0 = V.H0^T,
    a 10-iteration fit and a 10-iteration transform (fit = False) of `run`; the same in bf16x3 and f16x3 but the largest n;
  * 1, 2, 3, 7 row chunks, 1, 2, 3 W chunks and H segments of 100 and 128 columns forced through KLNMF_EX_ROW_CHUNKS /
    KLNMF_EX_W_CHUNKS / KLNMF_EX_H_SEG (development switches; conftest sets KLNMF_DEV=1) on 1000 x 300, k = 40, each
    against the reference and, in f64, against the same problem on its natural route;
  * the H rule straight from the slabs (k_update_H_slabs, a single-context `run`) bit-identical to the H rule from their
    sum (k_sum_partials + k_update_H, the loop in pieces), in all four modes; two runs of one fit bit-identical;
  * the row limit of the exact modes, the reconstruction GEMM (klnmf_matmul / klnmf_matmul_device: k_gemm's VALU
    instantiation), and the switches honoured only under KLNMF_DEV=1.
Fits never stop early (tol = exact_cases.NO_STOP): a plateau's last-bit rises would otherwise end the two loops at
different iterations.

Bars (relative, element by element; with the f64 floor 0 an exact zero of the reference must be an exact zero):
  f64     single steps and W0 1e-12; fits: losses 1e-10, W and H 1e-9; a forced route against the natural one 1e-12 per step,
          1e-10 per fit.
  f32     (the reference fed the fp32-rounded inputs) steps and W0 3e-5, fit losses 3e-5, fit W and H 3e-4, relative to
          max(|reference|, the smallest normal fp32 number): ten updates drive the dictionary's zero column to 1e-80, which
          fp32 holds as 0.  Losses of the fp32-storage modes relative to at least 2^-23 sum(V) (loss_floor).
  bf16x3  (and f16x3 at k > 256, which contracts on the same kernel) r = 2^-14 of sum |a.b| per contraction element
          (test_split3_gpu.CONTRACTION_RTOL; nonnegative operands: a relative bound).  A step against the fp64 reference: W0
          r + 2^-22, Q 2 r (its own contraction, the fp32 division), the W rule 4 r (Q's error, its contraction, the product),
          the H rule 8 r (W_new's and Q's errors, the contraction, the row sum); the loss of one step within the fit bar.
  f16x3   at k <= 256 the step API and W0 run the fp32 kernels (only the loop fuses its passes on split fp16 operands):
          the f32 step bar.
  Fits of both: every loss and the fp64 KL of the returned factors within the modules' fit bars (1e-4 bf16x3,
  test_split3_gpu; 2e-5 f16x3, test_f16x3_gpu.TOL).
Measured on the MI355X (worst over every case): f64 steps and W0 3.8e-15, fits 1.1e-14, forced against natural 1.0e-14;
f32 steps 2.1e-6, fit losses 1.6e-7, fit W 1.7e-5, fit H 5.1e-6; bf16x3 steps 1.4e-5 (Q), fit losses 1.3e-6; f16x3 steps
2.6e-6, fit losses 9.1e-8; run against pieces 0 in all four modes; matmul 3.6e-15 (f64) and 1.8e-6 (f32).  No bar was widened.
The measured worst errors are printed after each test (pytest -v) and are in each assertion message.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from multimodal_amd import _native
from oracle import klnmf_oracle as orc
from tests import exact_cases as ec
from tests.test_sparse_gpu import _MEASURED, _report_measured, check, worst_rel  # noqa: F401  (the autouse fixture prints what was measured)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS = 10
TINY32 = float(np.finfo(np.float32).tiny)
CONTRACTION_RTOL = 2.0 ** -14        # test_split3_gpu.py
F3_KMAX = 256                        # f16x3's fused loop (csrc/f16x3.hip.h); beyond, its contractions are bf16x3's
BARS = {'f64': {'step': 1e-12, 'fit_loss': 1e-10, 'fit_factor': 1e-9},
        'f32': {'step': 3e-5, 'fit_loss': 3e-5, 'fit_factor': 3e-4}}
SPLIT_FIT_LOSS = {'bf16x3': 1e-4, 'f16x3': 2e-5}
FORCED_VS_NATURAL = {'step': 1e-12, 'fit': 1e-10}
FLOOR = {'f64': 0.0, 'f32': TINY32, 'bf16x3': TINY32, 'f16x3': TINY32}

EXACT = ['f64', 'f32']
SPLIT = ['bf16x3', 'f16x3']
SWITCHES = ('KLNMF_EX_ROW_CHUNKS', 'KLNMF_EX_W_CHUNKS', 'KLNMF_EX_H_SEG')


@functools.lru_cache(maxsize=None)
def cu_count():
    return _native.device_info()['cu_count']


def esize(prec):
    return 8 if prec == 'f64' else 4


def step_bars(prec, k):
    """Bars of one step and of W0 (module docstring)."""
    if prec in BARS or (prec == 'f16x3' and k <= F3_KMAX):
        return dict.fromkeys(('loss', 'Q', 'W rule', 'H rule', 'W0'), BARS['f64' if prec == 'f64' else 'f32']['step'])
    r = CONTRACTION_RTOL
    return {'loss': SPLIT_FIT_LOSS[prec], 'Q': 2 * r, 'W rule': 4 * r, 'H rule': 8 * r, 'W0': r + 2.0 ** -22}


@functools.lru_cache(maxsize=4)
def problem(n, f, k):
    """(V, W, H) in fp64: V with a zero row and a zero column where it has four of each."""
    V = ec.data(n, f, seed=n + 7 * f + 13 * k, zero_row=n // 2 if n >= 4 else None, zero_col=f // 3 if f >= 4 else None)
    W, H = ec.factors(n, f, k, seed=k + 1)
    return V, W, H


def inputs(prec, V, W, H):
    """The reference's inputs (what the kernels of `prec` see, in fp64) and the arrays to upload."""
    if prec == 'f64':
        return (V, W, H), (V, W, H)
    return tuple(ec.as_f32(a) for a in (V, W, H)), tuple(np.asarray(a, np.float32) for a in (V, W, H))


@functools.lru_cache(maxsize=8)
def reference(n, f, k, f32_inputs, kchunk, wchunk):
    """(step, W0, fit, transform) of the reference on the case's inputs, summed over the kernels' chunks."""
    V, W, H = problem(n, f, k)
    if f32_inputs:
        V, W, H = (ec.as_f32(a) for a in (V, W, H))
    step = ec.ref_step(V, W, H, kchunk, wchunk)
    assert step[0] >= 1e-2 * V.sum()          # the loss's own cancellation does not dominate the step bars
    W0 = ec.ref_init_W(V, H, wchunk)
    fit = ec.ref_fit(V, H, ITERS, kchunk=kchunk, wchunk=wchunk)
    transform = ec.ref_fit(V, H, ITERS, fit=False, components=H, kchunk=kchunk, wchunk=wchunk)
    return step, W0, fit, transform


def open_problem(monkeypatch, prec, Vu, k, cap, row_chunks=0, w_chunks=0, h_seg=0):
    """A context with dense V uploaded; the three switches set where given (KLNMF_DEV=1), cleared otherwise."""
    monkeypatch.setenv('KLNMF_DEV', '1')
    for name, v in zip(SWITCHES, (row_chunks, w_chunks, h_seg)):
        if v:
            monkeypatch.setenv(name, str(v))
        else:
            monkeypatch.delenv(name, raising=False)
    ctx = _native.Context(prec)
    ctx.set_problem(Vu.shape[0], Vu.shape[1], k, cap)
    ctx.upload_V(Vu)
    return ctx


def gpu_step(ctx, W, H):
    """(loss, Q, W_new, H_new) of one update on the device: klnmf_error (the loss pass alone), then klnmf_step_Q / _W / _H."""
    ctx.set_H(H)
    ctx.set_W(W)
    loss = ctx.error()
    ctx.step_Q()
    Q = ctx.get_Q()
    ctx.step_W()
    Wn = ctx.get_W()
    ctx.step_H()
    return loss, Q, Wn, ctx.get_H()


def gpu_init_W(ctx, H0):
    ctx.set_H(H0)
    ctx.init_W()                                   # W0 = V . H0^T (nmf.py:156)
    return ctx.get_W()


def gpu_fit(ctx, H0, iters=ITERS, fit=True):
    """`iters` iterations of klnmf_run from W0 = V.H0^T; fit=False holds H0 (the transform of a dictionary H0)."""
    gpu_init_W(ctx, H0)
    errors, n_done, _ = ctx.run(iters, fit, ec.NO_STOP)
    assert n_done == len(errors) == iters
    return ctx.get_W(), ctx.get_H(), np.array(errors)


def gpu_pieces(ctx, H0, iters=ITERS):
    """The same fit through the loop in pieces (klnmf_iter_*): the H rule always from the summed slabs."""
    gpu_init_W(ctx, H0)
    ctx.loop_begin()
    for _ in range(iters):
        ctx.iter_rowpass(True)
        ctx.iter_decide(ec.NO_STOP)
        ctx.iter_colpass()
        ctx.iter_update_H()
        ctx.iter_advance()
    errors, n_done, _ = ctx.loop_end(iters)
    assert n_done == len(errors) == iters
    return ctx.get_W(), ctx.get_H(), np.array(errors)


def loss_floor(prec, V):
    """The fp32 modes' losses relative to at least 2^-23 sum(V): their terms are formed in fp32.  (1 x 1, k = 1 is fitted
    exactly from the first update on: the fp64 reference's losses are then 5.6e-17 of rounding, the fp32 kernels' 0.)"""
    return 0.0 if prec == 'f64' else 2.0 ** -23 * float(V.sum())


def check_step(case, prec, got, ref, k, V):
    loss, Q, Wn, Hn = ref
    floor = FLOOR[prec]
    bars = step_bars(prec, k)
    check(case, 'loss', got[0], loss, bars['loss'], loss_floor(prec, V))
    check(case, 'Q', got[1], Q, bars['Q'], floor)
    check(case, 'W rule', got[2], Wn, bars['W rule'], floor)
    check(case, 'H rule', got[3], Hn, bars['H rule'], floor)


def check_init(case, prec, got, ref, k):
    check(case, 'W0', got, ref, step_bars(prec, k)['W0'], FLOOR[prec])


def check_fit(case, prec, got, ref, V):
    W, H, errors = got
    Wr, Hr, er = ref
    assert len(errors) == len(er), '%s: %d iterations recorded, the reference %d' % (case, len(errors), len(er))
    if prec in BARS:
        check(case, 'losses', errors, er, BARS[prec]['fit_loss'], loss_floor(prec, V))
        check(case, 'W', W, Wr, BARS[prec]['fit_factor'], FLOOR[prec])
        check(case, 'H', H, Hr, BARS[prec]['fit_factor'], FLOOR[prec])
    else:
        # the 16-bit-operand modes' fit contract: every loss and the true KL of the returned factors
        check(case, 'losses', errors, er, SPLIT_FIT_LOSS[prec], loss_floor(prec, V))
        check(case, 'final KL', orc.kl_error(V, W, H), orc.kl_error(V, Wr, Hr), SPLIT_FIT_LOSS[prec], loss_floor(prec, V))


def run_case(monkeypatch, prec, n, f, k):
    V, W, H = problem(n, f, k)
    (Vr, Wr, Hr), (Vu, Wu, Hu) = inputs(prec, V, W, H)
    s, kchunk, w, wchunk, h, slabs = ec.exact_regime(n, f, k, cu_count(), esize(prec))
    step, W0, fit, transform = reference(n, f, k, prec != 'f64', kchunk, wchunk)
    case = '%s %s (%d, %d, %d, %d)' % (prec, ec.case_id((n, f, k)), s, w, h, slabs)
    with open_problem(monkeypatch, prec, Vu, k, ITERS) as ctx:
        assert ctx.exact_regime() == (s, w, h, int(slabs))
        check_step(case + ' step', prec, gpu_step(ctx, Wu, Hu), step, k, Vr)
        check_init(case, prec, gpu_init_W(ctx, Hu), W0, k)
        check_fit(case + ' fit', prec, gpu_fit(ctx, Hu), fit, Vr)
        check_fit(case + ' transform', prec, gpu_fit(ctx, Hu, fit=False), transform, Vr)


@pytest.mark.parametrize('prec', EXACT)
@pytest.mark.parametrize('case', ec.CASES, ids=ec.case_id)
def test_every_route_in_f64_and_f32(monkeypatch, prec, case):
    """One step, W0, a fit and a transform of every case against the chunked fp64 reference."""
    run_case(monkeypatch, prec, *case[:3])


@pytest.mark.parametrize('prec', SPLIT)
@pytest.mark.parametrize('case', [c for c in ec.CASES if c[:3] != ec.LARGEST_N], ids=ec.case_id)
def test_every_route_in_the_split_operand_modes(monkeypatch, prec, case):
    """The same cases on the split-operand contractions (bf16x3; f16x3's fused row and column passes for k <= 256, whose
    column pass walks the same row chunks)."""
    run_case(monkeypatch, prec, *case[:3])


def _forced_ids(v):
    return '%s=%d' % v


FORCED = ([('row_chunks', r) for r in ec.FORCED_ROW_CHUNKS] + [('w_chunks', w) for w in ec.FORCED_W_CHUNKS]
          + [('h_seg', L) for L in ec.FORCED_H_SEG])


@pytest.mark.parametrize('prec', EXACT + SPLIT)
@pytest.mark.parametrize('forced', FORCED, ids=_forced_ids)
def test_forced_routes(monkeypatch, prec, forced):
    """1000 x 300, k = 40 (a zero row and column) on a forced route: one step, W0, a fit and a transform against the
    reference summed over the forced chunks; in f64 also against the same problem on its natural route (16 row chunks,
    5 W chunks, the H rule from the slabs)."""
    n, f, k = ec.MID
    assert ec.exact_regime(n, f, k, cu_count())[:5:2] == (16, 5, 1) or cu_count() != ec.MI355X_CUS
    V, W, H = problem(n, f, k)
    (Vr, Wr, Hr), (Vu, Wu, Hu) = inputs(prec, V, W, H)
    kw = dict([forced])
    s, kchunk, w, wchunk, h, slabs = ec.exact_regime(n, f, k, cu_count(), esize(prec), **kw)
    step, W0, fit, transform = reference(n, f, k, prec != 'f64', kchunk, wchunk)
    case = '%s %s %s=%d (%d, %d, %d, %d)' % (prec, ec.case_id(ec.MID), forced[0], forced[1], s, w, h, slabs)
    with open_problem(monkeypatch, prec, Vu, k, ITERS, **kw) as ctx:
        assert ctx.exact_regime() == (s, w, h, int(slabs))
        got_step = gpu_step(ctx, Wu, Hu)
        check_step(case + ' step', prec, got_step, step, k, Vr)
        check_init(case, prec, gpu_init_W(ctx, Hu), W0, k)
        got_fit = gpu_fit(ctx, Hu)
        check_fit(case + ' fit', prec, got_fit, fit, Vr)
        check_fit(case + ' transform', prec, gpu_fit(ctx, Hu, fit=False), transform, Vr)
    if prec != 'f64':
        return
    with open_problem(monkeypatch, prec, Vu, k, ITERS) as nat:
        assert nat.exact_regime() == ec.query_regime(n, f, k, cu_count())
        nat_step = gpu_step(nat, Wu, Hu)
        nat_fit = gpu_fit(nat, Hu)
    for what, a, b in zip(('loss', 'Q', 'W rule', 'H rule'), got_step, nat_step):
        check(case + ' vs natural', what, a, b, FORCED_VS_NATURAL['step'])
    for what, a, b in zip(('W', 'H', 'losses'), got_fit, nat_fit):
        check(case + ' fit vs natural', what, a, b, FORCED_VS_NATURAL['fit'])


@pytest.mark.parametrize('prec', EXACT + SPLIT)
@pytest.mark.parametrize('shape', [(4096, 128, 16), (500, 1000, 10)], ids=ec.case_id)
def test_h_rule_from_the_slabs_gives_the_bits_of_the_summed_slabs(monkeypatch, prec, shape):
    """exact.hip.h: k_update_H_slabs sums the slabs in k_sum_partials' order and then does exactly k_update_H.  A single-
    context `run` (the slabs route) and the loop in pieces (the summed route) give the same W, H and losses, bit for bit."""
    n, f, k = shape
    V, W, H = problem(n, f, k)
    _, (Vu, _, Hu) = inputs(prec, V, W, H)
    with open_problem(monkeypatch, prec, Vu, k, ITERS) as ctx:
        s, _, _, slabs = ctx.exact_regime()
        assert slabs == 1 and s > 1, ctx.exact_regime()
        run = gpu_fit(ctx, Hu)
        pieces = gpu_pieces(ctx, Hu)
    for what, a, b in zip(('W', 'H', 'losses'), run, pieces):
        check('%s %s run vs pieces' % (prec, ec.case_id(shape)), what, a, b, 0.0)
        assert np.array_equal(a, b)


@pytest.mark.parametrize('prec', EXACT + SPLIT)
@pytest.mark.parametrize('shape', [ec.MID, (70001, 64, 8)], ids=ec.case_id)
def test_two_runs_of_one_fit_give_the_same_bits(monkeypatch, prec, shape):
    n, f, k = shape
    V, W, H = problem(n, f, k)
    _, (Vu, _, Hu) = inputs(prec, V, W, H)
    got = []
    for _ in range(2):
        with open_problem(monkeypatch, prec, Vu, k, ITERS) as ctx:
            got.append(gpu_fit(ctx, Hu))
    for a, b in zip(*got):
        assert np.array_equal(a, b)


@pytest.mark.parametrize('prec', EXACT + SPLIT)
def test_the_row_limit(monkeypatch, prec):
    """More than 65535 x 64 rows is refused with KLNMF_ERR_UNSUPP before anything is freed or allocated: the context keeps
    its problem and computes with it.  (The largest accepted n runs in test_every_route_in_f64_and_f32.)"""
    V, W, H = problem(65, 65, 65)
    _, (Vu, Wu, Hu) = inputs(prec, V, W, H)
    with open_problem(monkeypatch, prec, Vu, 65, 1) as ctx:
        before = ctx.exact_regime()
        ctx.set_H(Hu)
        ctx.set_W(Wu)
        loss = ctx.error()
        with pytest.raises(_native.NativeError) as e:
            ctx.set_problem(ec.ROWS_MAX + 1, 3, 2, 1)
        assert e.value.code == _native.ERR_UNSUPP
        assert ctx.exact_regime() == before
        assert ctx.error() == loss


MM_MN = (1, 63, 64, 65, 129)
MM_K = (1, 15, 16, 17, 200, 1000)
MM_BAR = {'f64': 1e-12, 'f32': 2e-5}


@pytest.mark.parametrize('prec', EXACT)
def test_reconstruction_gemm(prec):
    """klnmf_matmul (host operands) on every m, n at and around the 64-tile and kk around the 16-step, nonnegative
    operands, against the fp64 product of the same operands."""
    dt = np.float64 if prec == 'f64' else np.float32
    rng = np.random.default_rng(3)
    worst = 0.0
    for m in MM_MN:
        for n in MM_MN:
            for kk in MM_K:
                A = rng.random((m, kk)).astype(dt)
                B = rng.random((kk, n)).astype(dt)
                C = _native.matmul(A, B)
                assert C.dtype == dt
                err = worst_rel(C, A.astype(np.float64).dot(B.astype(np.float64)))
                assert err <= MM_BAR[prec], 'matmul %s %d x %d x %d: %.3e relative (bar %.0e)' % (prec, m, n, kk, err, MM_BAR[prec])
                worst = max(worst, err)
    _MEASURED.append('    matmul %s, %d shapes: worst %.2e  (bar %.0e)' % (prec, len(MM_MN) ** 2 * len(MM_K), worst, MM_BAR[prec]))


@pytest.mark.parametrize('prec', EXACT)
def test_reconstruction_gemm_on_device_operands(prec):
    """klnmf_matmul_device with row strides lda > kk, ldb > n, ldc > n: the product lands in C's first n columns, the
    sentinel in its padding columns survives."""
    import torch
    tdt = torch.float64 if prec == 'f64' else torch.float32
    rng = np.random.default_rng(4)
    sentinel = -7.25
    worst = 0.0
    for m in MM_MN:
        for n in MM_MN:
            for kk in MM_K:
                lda, ldb, ldc = kk + 3, n + 5, n + 2
                A = rng.random((m, lda))
                B = rng.random((kk, ldb))
                dA = torch.tensor(A, dtype=tdt, device='cuda')
                dB = torch.tensor(B, dtype=tdt, device='cuda')
                dC = torch.full((m, ldc), sentinel, dtype=tdt, device='cuda')
                torch.cuda.synchronize()
                _native.matmul_device(dA.data_ptr(), lda, dB.data_ptr(), ldb, dC.data_ptr(), ldc, m, n, kk, f64=prec == 'f64')
                C = dC.cpu().numpy().astype(np.float64)
                Ar = dA.cpu().numpy().astype(np.float64)[:, :kk]
                Br = dB.cpu().numpy().astype(np.float64)[:, :n]
                assert np.all(C[:, n:] == sentinel), (m, n, kk)
                err = worst_rel(C[:, :n], Ar.dot(Br))
                assert err <= MM_BAR[prec], 'matmul_device %s %d x %d x %d: %.3e relative (bar %.0e)' % (prec, m, n, kk, err,
                                                                                                          MM_BAR[prec])
                worst = max(worst, err)
    _MEASURED.append('    matmul_device %s, %d shapes: worst %.2e  (bar %.0e)' % (prec, len(MM_MN) ** 2 * len(MM_K), worst,
                                                                                MM_BAR[prec]))


_CHILD = r'''
import json
import numpy as np
from multimodal_amd import _native
ctx = _native.Context('f64')
ctx.set_problem(1000, 300, 40, 1)
print(json.dumps(list(ctx.exact_regime())))
ctx.close()
'''


def test_switches_need_klnmf_dev():
    """A child process with the three switches set reports the natural regime without KLNMF_DEV, the forced one with
    KLNMF_DEV=1 (one child at a time)."""
    n, f, k = ec.MID
    forced = dict(row_chunks=3, w_chunks=2, h_seg=128)
    env = dict(os.environ)
    env.update(dict(zip(SWITCHES, ('3', '2', '128'))))
    got = {}
    for dev in (None, '1'):
        env.pop('KLNMF_DEV', None)
        if dev:
            env['KLNMF_DEV'] = dev
        out = subprocess.run([sys.executable, '-c', _CHILD], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, timeout=180)
        assert out.returncode == 0, out.stderr.decode(errors='replace')[-2000:]
        got[dev] = tuple(json.loads(out.stdout.decode().strip().splitlines()[-1]))
    assert got[None] == ec.query_regime(n, f, k, cu_count())
    assert got['1'] == ec.query_regime(n, f, k, cu_count(), **forced) == (3, 2, 3, 0)
