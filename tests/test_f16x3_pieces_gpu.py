"""precision='f16x3' at k <= 256, element by element: the three kernels no other mode runs (csrc/f16x3.hip.h: k_x3_hscale,
k_rowpass_x3<1..4>, k_colpass_x3) and the hand-off between them (x3_ready, csrc/api_loop.hip), driven through the loop in pieces
(klnmf_iter_*) with torch-owned exchange buffers (tests/loop_piece_cases.py).

Every piece of an iteration -- Q, W_new, the H numerator, H_new, the loss -- is compared with fp64 arithmetic on the values the
kernel that made it read, under the per-element bound that follows from the mode's specification (tests/f16x3_cases.py: split
operands under power-of-two scales, lo.lo dropped, r = 2^-18 for the fp32 accumulation).  tests/test_f16x3_pieces_cpu.py shows on
the numpy emulation that a correct implementation stays within these bounds (worst |error| / bound: Q 0.23, W_new 0.17, numerator
0.83; an earlier run of the emulation at (300, 700, 256) and (1000, 300, 40) as well: plain 0.32, wide 0.78, spike 0.68, all on
the numerator) and that a dropped lo.hi
product, a wrong last row / column / component, a tile's or component's scale taken from a neighbour and a chunk's partial last
contraction step all exceed them.

Cases: f16x3_cases.CASES (every NB of the row pass, one tile exactly and one past it on every axis, eleven column tiles, ragged
row chunks, more row blocks than CUs, kchunk = 336 and 144 forced) on five kinds of data (plain, wide, spike, x 2^100, x 2^-100).
Beyond one iteration: three in sequence from the device's own factors (xmax reset, qr rewritten), a transform's row pass (null Q, qr,
xmax) against the fit's, step_Q and set_Q between the row and the column pass (the column pass must not take a qr that no longer
bounds Q), a context reused for a smaller problem, two runs bit for bit, and k = 257 on the bf16x3 kernels.

What the tests measured on the MI355X is in profiles/f16x3_pieces_gpu_tests.txt (worst |error| / bound per piece, kind and case),
printed after each test (pytest -v) and in every assertion message: over everything Q 0.28, W_new 0.12, numerator 0.83 (wide),
H_new 0.41, loss 3.4e-7 against its 2e-5.  No bound was widened; r = 2^-18 stands.  The x 2^100 and x 2^-100 kinds and set_Q failed
on the kernels as they were (a NaN and a zero numerator from scale products beyond fp32's range, a stale qr): DESIGN.md 7b.
"""
import functools

import numpy as np
import pytest

from multimodal_amd import _native
from tests import exact_cases as ec
from tests import f16x3_cases as fc
from tests import loop_piece_cases as lp
from tests import test_exact_gpu as te
from tests import test_f16x3_gpu as tf
from tests.test_sparse_gpu import _MEASURED, _report_measured  # noqa: F401  (the autouse fixture prints what was measured)

pytestmark = pytest.mark.gpu

PREC = 'f16x3'


def test_the_bound_s_constants_are_the_project_s():
    assert fc.R == tf.STEP_RTOL and fc.TOL == tf.TOL and fc.KMAX == te.F3_KMAX
    assert fc.TINY32 == te.TINY32 and fc.EPS == float(np.float32(1e-8))


@functools.lru_cache(maxsize=4)
def problem(kind, n, f, k):
    return fc.problem(kind, n, f, k)


class Device(object):
    """A context of one case with its exchange buffers; `iteration()` runs one fit iteration in pieces and reads every piece."""

    def __init__(self, monkeypatch, V, k, cap, chunks=0):
        import torch
        n, f = V.shape
        if chunks:
            # (the switch is read when the problem is planned; the context has its own stream: synchronised before every read)
            self.ctx = te.open_problem(monkeypatch, PREC, V, k, cap, row_chunks=chunks)
            self.xch = None
        else:
            for name in te.SWITCHES:
                monkeypatch.delenv(name, raising=False)
            self.ctx, self.xch = lp.open_context(PREC, V, np.full((k, f), 1.0 / f, np.float32), k, cap)
        self.V, self.k, self.chunks = V, k, chunks
        try:
            if self.xch is None:
                self.xch = lp.Exchange(self.ctx)
            torch.cuda.synchronize()
            self.expect_regime(n, f, k, chunks)
        except Exception:
            self.ctx.close()
            raise

    def expect_regime(self, n, f, k, chunks=0):
        assert self.ctx.exact_regime() == ec.query_regime(n, f, k, te.cu_count(), esize=4, row_chunks=chunks)
        self.nsplit = ec.exact_regime(n, f, k, te.cu_count(), esize=4, row_chunks=chunks)[0]

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ctx.close()

    def start(self, W, H):
        self.ctx.set_H(H)
        self.ctx.set_W(W)

    def iteration(self, fit=True, between=None):
        """dict(loss, Q, N, W, H) of one iteration of the open loop; `between(self)` runs between the row and the column pass
        and may return the Q the column pass then reads."""
        ctx, xch = self.ctx, self.xch
        got = {}
        ctx.iter_rowpass(fit)
        ctx.synchronize()
        got['loss'] = float(xch.read_loss()[0])
        if fit:
            got['Q'] = ctx.get_Q(np.float32)
            if between is not None:
                Q = between(self)
                if Q is not None:
                    got['Q'] = Q
            ctx.iter_colpass()
            ctx.synchronize()
            got['N'] = xch.read_numerator().astype(np.float32)
        ctx.iter_decide(lp.NO_STOP)
        if fit:
            ctx.iter_update_H()
        ctx.iter_advance()
        got['W'] = ctx.get_W(np.float32)
        got['H'] = ctx.get_H(np.float32)
        return got

    def one(self, W, H, **kw):
        self.start(W, H)
        self.ctx.loop_begin()
        got = self.iteration(**kw)
        errors, n_done, stopped = self.ctx.loop_end(1)
        assert (n_done, stopped) == (1, False)
        got['recorded'] = errors[0]
        return got


def judge(case, V, W, H, got, nsplit):
    rec = fc.Record()
    try:
        fc.check_iteration(rec, case, V, W, H, got, nsplit)
    finally:
        _MEASURED.extend(rec.lines)
    return rec


def same_bits(a, b, what):
    for key in sorted(set(a) & set(b)):
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), '%s: %s differs' % (what, key)


# ---- one iteration in pieces -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', fc.KINDS)
@pytest.mark.parametrize('case', fc.CASES, ids=fc.case_id)
def test_one_iteration_piece_by_piece(monkeypatch, case, kind):
    n, f, k, chunks = case[:4]
    V, W, H = problem(kind, n, f, k)
    with Device(monkeypatch, V, k, 1, chunks) as dev:
        got = dev.one(W, H)
    judge('%s %s' % (fc.case_id(case), kind), V, W, H, got, dev.nsplit)
    assert got['recorded'] == got['loss']
    if kind == 'plain' and fc.zero_row(n) is not None:
        assert np.all(V[fc.zero_row(n)] == 0) and np.all(got['W'][fc.zero_row(n)] == 0)          # a zero row of V (W0's row is 0): exactly 0
    if kind == 'wide' and fc.zero_component(k) is not None:
        j = fc.zero_component(k)
        assert np.all(got['W'][:, j] == 0) and np.all(got['N'][j] == 0)                           # xmax = 0


# ---- three iterations in sequence ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['plain', 'spike'])
@pytest.mark.parametrize('case', fc.SEQUENCE_CASES, ids=fc.case_id)
def test_three_iterations_each_from_the_device_s_own_factors(monkeypatch, case, kind):
    """xmax is reset and qr rewritten by every row pass: the spike kind's first ratios are 1e4 times the later ones."""
    n, f, k, chunks = case
    V, W, H = problem(kind, n, f, k)
    with Device(monkeypatch, V, k, 3, chunks) as dev:
        dev.start(W, H)
        dev.ctx.loop_begin()
        steps = [dev.iteration() for _ in range(3)]
        errors, n_done, _ = dev.ctx.loop_end(3)
    assert n_done == 3 and list(errors) == [s['loss'] for s in steps]
    for it, got in enumerate(steps):
        judge('%s %s iteration %d' % (fc.case_id(case), kind, it + 1), V, W, H, got, dev.nsplit)
        W, H = got['W'], got['H']


# ---- a transform's row pass -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [(65, 65, 65, 0), (200, 193, 193, 0), (300, 700, 17, 0)], ids=fc.case_id)
def test_a_transform_row_pass_gives_the_fit_s_bits(monkeypatch, case):
    """iter_rowpass(False) passes null Q, qr and xmax: the same W_new and loss, H untouched."""
    n, f, k, chunks = case
    V, W, H = problem('plain', n, f, k)
    with Device(monkeypatch, V, k, 1, chunks) as dev:
        fit = dev.one(W, H)
        judge('%s fit' % fc.case_id(case), V, W, H, fit, dev.nsplit)
        tr = dev.one(W, H, fit=False)
    assert np.array_equal(tr['W'], fit['W']) and tr['loss'] == fit['loss']
    assert np.array_equal(tr['H'], H)


# ---- the hand-off ----------------------------------------------------------------------------------------------------------------------------
def _step_q(dev):
    dev.ctx.step_Q()                      # rewrites Q on the fp32 kernel: the fused row pass's Q, qr and xmax are no longer one set
    return dev.ctx.get_Q(np.float32)


def _set_q(dev):
    Q = (8 * dev.ctx.get_Q(np.float32)).astype(np.float32)          # 8 Q / qr >= 4: 2^14 times that is beyond fp16's range
    dev.ctx.set_Q(Q)
    return Q


@pytest.mark.parametrize('between', [_step_q, _set_q], ids=['step_Q', 'set_Q'])
@pytest.mark.parametrize('case', [(130, 130, 129, 0), (1000, 300, 40, 7)], ids=fc.case_id)
def test_q_rewritten_between_the_row_and_the_column_pass(monkeypatch, case, between):
    """The numerator that follows is W_new^T.Q of the Q that is there, within the bound (the column pass takes the fp32 kernel: qr
    and xmax belong to the Q the row pass wrote)."""
    n, f, k, chunks = case
    V, W, H = problem('plain', n, f, k)
    with Device(monkeypatch, V, k, 1, chunks) as dev:
        got = dev.one(W, H, between=between)
    rec = fc.Record()
    try:
        rec.check('%s %s' % (fc.case_id(case), between.__name__), 'numerator', got['N'], *fc.ref_N(got['W'], got['Q'], dev.nsplit))
        rec.check('%s %s' % (fc.case_id(case), between.__name__), 'H_new', got['H'], *fc.ref_H(H, got['N']))
    finally:
        _MEASURED.extend(rec.lines)


# ---- stale state ---------------------------------------------------------------------------------------------------------------------------------
def test_a_context_reused_for_a_smaller_problem_gives_a_fresh_context_s_bits(monkeypatch):
    big, small = (200, 193, 193), (65, 65, 65)
    Vb, Wb, Hb = problem('spike', *big)
    Vs, Ws, Hs = problem('plain', *small)
    with Device(monkeypatch, Vs, small[2], 1) as dev:
        fresh = dev.one(Ws, Hs)
    judge('%s fresh' % fc.case_id(small + (0,)), Vs, Ws, Hs, fresh, dev.nsplit)
    with Device(monkeypatch, Vb, big[2], 1) as dev:
        dev.one(Wb, Hb)
        dev.ctx.set_problem(small[0], small[1], small[2], 1)
        dev.xch = lp.Exchange(dev.ctx)
        dev.ctx.upload_V(Vs)
        dev.expect_regime(*small)
        reused = dev.one(Ws, Hs)
    same_bits(fresh, reused, 'reused context')


# ---- two runs -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [(4111, 63, 200, 0), (16449, 65, 8, 0)], ids=fc.case_id)
def test_two_runs_of_one_case_give_the_same_bits(monkeypatch, case):
    """The atomic maximum on float bits does not depend on the order the workgroups arrive in."""
    n, f, k, chunks = case
    V, W, H = problem('wide', n, f, k)
    runs = []
    for _ in range(2):
        with Device(monkeypatch, V, k, 1, chunks) as dev:
            runs.append(dev.one(W, H))
    same_bits(runs[0], runs[1], 'second run')


# ---- k = 257 ------------------------------------------------------------------------------------------------------------------------------------------
def test_k_257_takes_the_bf16x3_kernels(monkeypatch):
    """A routing assertion: one iteration in pieces at k = 257 within test_exact_gpu's bf16x3 step bars against the fp64 reference
    (the fused kernels hold 256 components: at 257 they would drop one)."""
    n, f, k = 130, 130, 257
    V, W, H = problem('plain', n, f, k)
    s, kchunk, w, wchunk, h, slabs = ec.exact_regime(n, f, k, te.cu_count(), esize=4)
    bars = te.step_bars(PREC, k)
    assert bars['Q'] == 2 * te.CONTRACTION_RTOL
    with Device(monkeypatch, V, k, 1) as dev:
        got = dev.one(W, H)
    ref = ec.ref_step(fc.f64(V), fc.f64(W), fc.f64(H), kchunk, wchunk)
    te.check_step('%s k=257' % PREC, PREC, (got['loss'], got['Q'], got['W'], got['H']), ref, k, fc.f64(V))
    worst, _ = fc.Record().ratio(got['Q'], *fc.ref_Q(V, W, H))
    _MEASURED.append('    k = 257: Q is %.2f of the fused kernels\' bound (bf16x3 operands: measured, not asserted)' % worst)
