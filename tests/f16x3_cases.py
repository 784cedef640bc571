"""Helpers of the element-by-element tests of precision='f16x3' at k <= 256 (tests/test_f16x3_pieces_cpu.py,
tests/test_f16x3_pieces_gpu.py): the cases, the per-element error bounds that follow from the mode's specification (the header of
multimodal_amd/csrc/f16x3.hip.h), and one fit iteration restated in fp64 piece by piece.  Importing needs no GPU.

The bound.  An operand x is held as (hi + lo) / s, hi = f16(x s), lo = f16(x s - hi), s the power of two that puts the largest
operand M it covers into [2^14, 2^15).  hi carries 11 bits, a normal lo 11 more, and a lo below fp16's normal range (2^-14) is
rounded to a multiple of 2^-24, at most 2^-25 / s <= 2^-39 M off:

    |dx| <= max(2^-22 |x|, 2^-39 M)                                                                        (`_delta`)

A contraction is hi.hi + hi.lo + lo.hi in fp32; the dropped lo.lo is at most 2^-22 |a b|.  Per element of a contraction

    bound = sum |da| |b| + sum |a| |db| + r sum |a| |b|,   r = 2^-18                                        (`R`)

r is the project's own figure (test_f16x3_gpu.STEP_RTOL; "within 2^-18 of sum |a.b|", csrc/api_loop.hip): it covers lo.lo and
the fp32 accumulation.  The maxima M are the ones each scale covers (`bound_wh`, `bound_qht`, `bound_wtq`).  The numerator
W_new^T.Q therefore has NO relative bound: Q / qr is held under the row's scale, so a ratio 2^-25 of its row's largest (V's zero
column beside ordinary ratios; every other entry of a row with one spike) loses bits or flushes to 0 -- an error of up to 1
relative to that element, of 2^-39 of the row's weight absolutely, which is what the bound allows and what the loss cannot see.

Every piece is judged against fp64 arithmetic on the values the kernel that made it actually read (the device's own Q for the W
rule, its own W_new and Q for the numerator, its own numerator for the H rule), so no piece's error enters another's bar
(`check_iteration`).  Terms relative to a reference value take max(|ref|, the smallest normal fp32 number), as
tests/test_exact_gpu.py's fp32 bars do: an fp32 result below that has no 24 bits to be held to.
"""
import contextlib
import importlib.util
import os
import sys

import numpy as np

from tests import exact_cases as ec
from tests import loop_piece_cases as lp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

R = 2.0 ** -18                 # test_f16x3_gpu.STEP_RTOL (tests/test_f16x3_pieces_gpu.py holds the two to each other)
U24 = 2.0 ** -24               # half an ulp of fp32
TOL = 2e-5                     # test_f16x3_gpu.TOL: the mode's bar on a loss
TINY32 = float(np.finfo(np.float32).tiny)
EPS = float(np.float32(1e-8))  # kEpsRatio as the kernel holds it: (float)eps
TILE = 64                      # F3_TC / F3_TR: columns per row-pass tile, rows per workgroup
CK = 32                        # F3_CK: the column pass's contraction step
KMAX = 256                     # F3_KMAX

# (n, f, k, row chunks forced through KLNMF_EX_ROW_CHUNKS or 0, what the case is for)
CASES = [
    (1, 1, 1, 0, 'smallest problem'),
    (15, 17, 1, 0, 'one partial tile'),
    (64, 64, 64, 0, 'exactly one tile'),
    (65, 65, 65, 0, 'NB = 2 with one real component in the second block; one past a tile on every axis'),
    (130, 130, 129, 0, 'NB = 3'),
    (200, 193, 193, 0, 'NB = 4, ragged'),
    (96, 70, 256, 0, 'NB = 4, full: the 151 KiB LDS layout'),
    (300, 700, 17, 0, 'eleven column tiles, the last of 60 columns'),
    (4111, 63, 200, 0, 'ragged row chunks'),
    (16449, 65, 8, 0, 'more row blocks than CUs'),
    (1000, 300, 40, 3, 'kchunk = 336'),
    (1000, 300, 40, 7, 'kchunk = 144: not a multiple of the 32-row contraction step'),
]
KINDS = ['plain', 'wide', 'spike', 'scaled-up', 'scaled-down']
SEQUENCE_CASES = [(130, 130, 129, 0), (1000, 300, 40, 0)]          # three iterations in sequence


def case_id(case):
    return '%dx%dk%d' % case[:3] + ('-chunks%d' % case[3] if case[3] else '')


_EMU = []


def emulation():
    """experiments/f16x3_emulation.py as a module (loaded once, the way tests/test_f16x3_cpu.py loads it)."""
    if not _EMU:
        sys.path.insert(0, os.path.join(ROOT, 'experiments'))
        try:
            spec = importlib.util.spec_from_file_location('f16x3_emulation', os.path.join(ROOT, 'experiments', 'f16x3_emulation.py'))
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
        finally:
            sys.path.remove(os.path.join(ROOT, 'experiments'))
        _EMU.append(mod)
    return _EMU[0]


# ---- data ----------------------------------------------------------------------------------------------------------------------------
def zero_row(n):
    return n // 2 if n >= 4 else None


def zero_col(f):
    return f // 3 if f >= 4 else None


def spike_at(n, f):
    """(row, column) of the spike: neither V's zero row nor its zero column."""
    return n // 3, f // 2


def zero_component(k):
    """The component whose column of W is 0 in the wide kind (never k - 1, which the planted faults move); None at k = 1, where it
    would leave no model at all."""
    return (k - 1) // 2 if k >= 2 else None


def problem(kind, n, f, k):
    """(V, W, H) as float32: exact_cases.data (a zero row and a zero column where it has four of each) and exact_cases.factors.

    plain        W's row of V's zero row is 0 as well, as W0 = V.H0^T leaves it: the row pass's scale of an all-zero row
    wide         W entries x 2^U[-20, 20], H rows x 2^U[-12, 12], V entries x 2^U[-10, 10], one column of W 0 (its xmax is 0)
    spike        one entry of V at 1e4 x the largest
    scaled-up    V and W x 2^100   (W with V: the model stays of the data's order, and W_new^T.Q within fp32's range -- from V
    scaled-down  V and W x 2^-100   alone x 2^100 the numerator's true value is 2^200)"""
    assert kind in KINDS, kind
    V = ec.data(n, f, seed=n + 7 * f + 13 * k, zero_row=zero_row(n), zero_col=zero_col(f))
    W, H = ec.factors(n, f, k, seed=k + 1)
    rng = np.random.default_rng(1000 + n + 3 * f + 5 * k)
    if kind == 'plain':
        if zero_row(n) is not None:
            W[zero_row(n)] = 0.0
    elif kind == 'wide':
        W = W * np.exp2(rng.uniform(-20, 20, W.shape))
        H = H * np.exp2(rng.uniform(-12, 12, (k, 1)))
        V = V * np.exp2(rng.uniform(-10, 10, V.shape))
        if zero_component(k) is not None:
            W[:, zero_component(k)] = 0.0
    elif kind == 'spike':
        V[spike_at(n, f)] = 1e4 * V.max()
    else:
        s = 2.0 ** (100 if kind == 'scaled-up' else -100)
        V, W = V * s, W * s
    return tuple(np.ascontiguousarray(a, dtype=np.float32) for a in (V, W, H))


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- the scales, restated in fp64 (powers of two: exact) -------------------------------------------------------------------------------
def hscale(H):
    """hs[j] of k_x3_hscale."""
    return f64(emulation().pow2_scale(f64(H).max(axis=1)))


def qr_of(Q):
    """qr[r] of k_rowpass_x3: 2^e above the row's largest ratio (1 for an all-zero row)."""
    m = f64(Q).max(axis=1)
    pos = m > 0
    e = np.floor(np.log2(np.where(pos, m, 1.0))) + 1
    return np.where(pos, np.exp2(e), 1.0)


# ---- the bounds ----------------------------------------------------------------------------------------------------------------------
def _delta(x, M):
    return np.maximum(2.0 ** -22 * np.abs(x), 2.0 ** -39 * M)


def _contraction(a, da, b, db, r):
    return da.dot(b) + a.dot(db) + r * a.dot(b)


def bound_wh(W, H, r=R):
    """[n, f] bound of W.H: a = W[r, j] / hs[j] under the maximum of row r, b = H[j, c] hs[j] under the maximum of row j."""
    W, H = f64(W), f64(H)
    hs = hscale(H)
    a, b = W / hs[None, :], H * hs[:, None]
    return _contraction(a, _delta(a, a.max(axis=1, keepdims=True)), b, _delta(b, b.max(axis=1, keepdims=True)), r)


def bound_qht(Q, H, r=R):
    """[n, k] bound of Q.H^T: per TILE-column tile a = Q[r, c] under the row's maximum within the tile, b as in W.H; the tiles'
    bounds summed, then divided by hs[j]."""
    Q, H = f64(Q), f64(H)
    hs = hscale(H)
    b = H * hs[:, None]
    db = _delta(b, b.max(axis=1, keepdims=True))
    out = np.zeros((Q.shape[0], H.shape[0]))
    for c0 in range(0, Q.shape[1], TILE):
        a = Q[:, c0:c0 + TILE]
        out += _contraction(a, _delta(a, a.max(axis=1, keepdims=True)), b[:, c0:c0 + TILE].T, db[:, c0:c0 + TILE].T, r)
    return out / hs[None, :]


def bound_wtq(Wn, Q, r=R):
    """[k, f] bound of W_new^T.Q: a = W_new[r, j] qr[r] under the maximum of column j over all rows, b = Q[r, c] / qr[r] under 1."""
    Wn, Q = f64(Wn), f64(Q)
    qr = qr_of(Q)
    a, b = Wn * qr[:, None], Q / qr[:, None]
    return _contraction(a.T, _delta(a, a.max(axis=0, keepdims=True)).T, b, _delta(b, 1.0), r)


# ---- the pieces of one iteration in fp64 -----------------------------------------------------------------------------------------------
def _rel(ref):
    return np.maximum(np.abs(ref), TINY32)


def ref_Q(V, W, H):
    """(Q, bound): (V + eps) / (W.H + eps); the contraction's bound carried through the division, and 4 x 2^-24 for the fp32
    epilogue (x + eps, y + eps, the division, the sum of the two accumulators' scaled values)."""
    V, W, H = f64(V), f64(W), f64(H)
    D = W.dot(H)
    Q = (V + EPS) / (D + EPS)
    return Q, Q * (bound_wh(W, H) / (D + EPS)) + 4 * U24 * _rel(Q)


def ref_loss(V, W, H):
    V, W, H = f64(V), f64(W), f64(H)
    D = W.dot(H)
    return float((V * np.log((V + EPS) / (D + EPS)) - V + D).sum())


def ref_W(W, H, Q_dev):
    """(W_new, bound) from the device's own Q."""
    W, H, Q_dev = f64(W), f64(H), f64(Q_dev)
    ref = W * Q_dev.dot(H.T)
    return ref, W * bound_qht(Q_dev, H) + 4 * U24 * _rel(ref)


def ref_N(Wn_dev, Q_dev, nsplit):
    """(numerator, bound) from the device's own W_new and Q; the row chunks' slabs are summed in fp32 (k_sum_partials)."""
    ref = f64(Wn_dev).T.dot(f64(Q_dev))
    return ref, bound_wtq(Wn_dev, Q_dev) + (nsplit + 2) * U24 * _rel(ref)


def ref_H(H, N_dev):
    """(H_new, bound) from the device's own numerator: loop_piece_cases.ref_h_rule at BAR_F32 (the fp32 mode's kernels)."""
    ref = lp.ref_h_rule(H, N_dev, np.shape(H)[1])
    return ref, lp.BAR_F32 * _rel(ref)


class Record(object):
    """Worst |got - ref| / bound of every check, kept as lines (`lines`) and put into each assertion message."""

    def __init__(self):
        self.lines = []
        self.worst = {}

    def ratio(self, got, ref, bound):
        """(worst ratio, its index).  Where the bound is 0 the result must equal the reference; a result that is not finite: inf."""
        got, ref, bound = f64(got), f64(ref), f64(bound)
        assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
        err = np.abs(got - ref)
        with np.errstate(divide='ignore', invalid='ignore'):
            q = np.where(err == 0, 0.0, err / bound)
        q = np.where(np.isfinite(got), q, np.inf)
        q = np.where(np.isnan(q), np.inf, q)
        at = np.unravel_index(int(np.argmax(q)), q.shape) if q.size else ()
        return (float(q[at]) if q.size else 0.0), at

    def check(self, case, piece, got, ref, bound):
        worst, at = self.ratio(got, ref, bound)
        self.lines.append('    %-44s %-10s %.3f of the bound' % (case, piece, worst))
        self.worst[piece] = max(self.worst.get(piece, 0.0), worst)
        assert worst <= 1.0, '%s: %s is %.3f times its bound at %r (got %r, reference %r, bound %.3e)' % (
            case, piece, worst, at, float(f64(got)[at]), float(f64(ref)[at]), float(f64(bound)[at]))
        return worst

    def check_loss(self, case, got, ref, V):
        floor = 2.0 ** -23 * float(f64(V).sum())          # test_exact_gpu.loss_floor
        dev = abs(float(got) - ref) / max(abs(ref), floor) if np.isfinite(got) else np.inf
        self.lines.append('    %-44s %-10s %.2e  (bar %.0e)' % (case, 'loss', dev, TOL))
        assert dev <= TOL, '%s: the loss %r differs from %r by %.3e relative (bar %.0e)' % (case, got, ref, dev, TOL)
        return dev


def check_iteration(rec, case, V, W, H, got, nsplit):
    """One fit iteration from (W, H): got = dict(Q, W, N, H, loss) as the kernels left them (any subset but Q before W, W before N)."""
    if 'loss' in got:
        rec.check_loss(case, got['loss'], ref_loss(V, W, H), V)
    if 'Q' in got:
        rec.check(case, 'Q', got['Q'], *ref_Q(V, W, H))
    if 'W' in got:
        rec.check(case, 'W_new', got['W'], *ref_W(W, H, got['Q']))
    if 'N' in got:
        rec.check(case, 'numerator', got['N'], *ref_N(got['W'], got['Q'], nsplit))
    if 'H' in got:
        rec.check(case, 'H_new', got['H'], *ref_H(H, got['N']))


# ---- the emulation as the device (tests/test_f16x3_pieces_cpu.py) ------------------------------------------------------------------------
def chunk_rows(n, kchunk):
    return [(a, min(n, a + kchunk)) for a in range(0, n, kchunk)]


def emulate(V, W, H, kchunk, rows=None):
    """dict(Q, W, N, H, loss) of one iteration by the emulation's three contractions, the numerator in slabs of `kchunk` rows
    summed in fp32 in order; `rows(a, b)`: the rows of chunk [a, b) the column pass takes (a planted fault; default all)."""
    emu = emulation()
    V, W, H = (np.ascontiguousarray(x, dtype=np.float32) for x in (V, W, H))
    eps = np.float32(EPS)
    hs = emu.pow2_scale(H.max(axis=1))
    D = emu.wh(W, H, hs)
    Q = ((V + eps) / (D + eps)).astype(np.float32)
    with np.errstate(divide='ignore', invalid='ignore'):
        loss = float((V * np.log(Q) - V + D).astype(np.float32).sum(dtype=np.float64))
    Wn = (W * emu.qht(Q, H, hs)).astype(np.float32)
    N = numerator(Wn, Q, kchunk, rows)
    Hn = lp.ref_h_rule(H, N, H.shape[1]).astype(np.float32)
    return {'Q': Q, 'W': Wn, 'N': N, 'H': Hn, 'loss': loss}


def numerator(Wn, Q, kchunk, rows=None, wj=None):
    """W_new^T.Q as the column pass forms it: qr and the per-component scales over ALL rows, one slab per row chunk.  `wj`: a
    function of the per-component scales (a planted fault)."""
    emu = emulation()
    qr = qr_of(Q).astype(np.float32)
    Wp = (Wn * qr[:, None]).astype(np.float32)
    s = emu.pow2_scale(np.abs(Wp).max(axis=0))
    if wj is not None:
        s = wj(s)
    qsc = np.float32(2.0 ** (emu.TOP - 1))
    N = np.zeros((Wn.shape[1], Q.shape[1]), np.float32)
    for a, b in chunk_rows(Q.shape[0], kchunk):
        if rows is not None:
            a, b = rows(a, b)
        with np.errstate(over='ignore', invalid='ignore'):
            part = emu.prod3(np.ascontiguousarray((Wp[a:b] * s[None, :]).T), Q[a:b] / qr[a:b, None] * qsc) / qsc / s[:, None]
        N = (N + part.astype(np.float32)).astype(np.float32)
    return N


@contextlib.contextmanager
def without_lo_hi():
    """The emulation with the lo.hi product dropped from every contraction (a planted fault)."""
    emu = emulation()
    keep = emu.prod3

    def prod2(A, B):
        ah, _ = emu.split16(A)
        bh, bl = emu.split16(B)
        return (np.dot(ah, bh) + np.dot(ah, bl)).astype(np.float32)
    emu.prod3 = prod2
    try:
        yield
    finally:
        emu.prod3 = keep


def qht_with_neighbour_scale(Q, H, tile, neighbour):
    """The emulation's Q.H^T with tile `tile`'s row scales taken from tile `neighbour` (a planted fault)."""
    emu = emulation()
    Q, H = (np.ascontiguousarray(x, dtype=np.float32) for x in (Q, H))
    hs = emu.pow2_scale(H.max(axis=1))
    acc = np.zeros((Q.shape[0], H.shape[0]), np.float32)
    HsT = np.ascontiguousarray((H * hs[:, None]).T)
    for t, c0 in enumerate(range(0, Q.shape[1], TILE)):
        q = Q[:, c0:c0 + TILE]
        src = Q[:, neighbour * TILE:(neighbour + 1) * TILE] if t == tile else q
        qs = emu.pow2_scale(np.abs(src).max(axis=1))
        with np.errstate(over='ignore', invalid='ignore'):
            acc = (acc + emu.prod3(q * qs[:, None], HsT[c0:c0 + TILE]) / qs[:, None]).astype(np.float32)
    return (acc / hs[None, :]).astype(np.float32)
