"""The checks of tests/test_f16x3_pieces_gpu.py, tried without a GPU on the numpy emulation of the mode
(experiments/f16x3_emulation.py through tests/f16x3_cases.py):

  * the emulation stays within every per-element bound on every case and data kind -- the bounds are not too tight for a correct
    implementation whose only freedom is the order of its fp32 sums;
  * every planted fault -- lo.hi dropped; the last row, the last column or component k - 1 zeroed or taken from its neighbour; one
    tile's Q scale taken from the neighbouring tile; one component's xmax taken from another; the last kchunk % 32 rows of every
    chunk left out -- exceeds a bound on at least one element: the GPU test would see such a kernel.  Two of them are faults of a
    SCALE, and a power-of-two scale that is merely a few binades off costs split fp16 operands nothing (the exponent absorbs it);
    such a fault shows where the wrong scale lets an operand overflow, so those two are planted on the kinds that make the scales
    differ (spike: a ratio 1e4 times its neighbours'; wide: component maxima 2^+-12 apart), at the place where they overflow.

Worst |error| / bound of the emulation over all cases (this file, numpy's sum order): Q 0.23, W_new 0.17, numerator 0.83 (wide).
The x 2^-100 kind is what showed that the column pass's product of its two scales leaves fp32's range (the numerator was 0).
"""
import numpy as np
import pytest

from tests import exact_cases as ec
from tests import f16x3_cases as fc

PLANT = (300, 700, 17, 0)            # eleven column tiles: every planted fault has its edge here
PLANT_CHUNKED = (1000, 300, 40, 7)   # kchunk = 144


def regime(case, cu_count=ec.MI355X_CUS):
    n, f, k, chunks = case[:4]
    return ec.exact_regime(n, f, k, cu_count, esize=4, row_chunks=chunks)


def test_cases_reach_every_row_pass_instantiation_and_the_named_chunks():
    assert {(c[2] + 63) // 64 for c in fc.CASES} == {1, 2, 3, 4}
    assert all(c[2] <= fc.KMAX and c[0] * c[1] <= 1100000 for c in fc.CASES)
    kchunks = {c[3]: regime(c)[1] for c in fc.CASES if c[3]}
    assert kchunks == {3: 336, 7: 144}
    assert kchunks[7] % fc.CK != 0 and kchunks[7] % ec.GK == 0
    n, f, k = 4111, 63, 200
    s, kchunk = regime((n, f, k, 0))[:2]
    assert s > 1 and 0 < n % kchunk < ec.GK          # the last chunk is shorter than one contraction step, and than one MFMA's 16
    assert (16449 + 63) // 64 > ec.MI355X_CUS
    assert 700 % fc.TILE == 60 and -(-700 // fc.TILE) == 11


@pytest.mark.parametrize('kind', fc.KINDS)
def test_kinds_are_what_they_say(kind):
    n, f, k = 300, 700, 17
    V, W, H = fc.problem(kind, n, f, k)
    assert V.dtype == W.dtype == H.dtype == np.float32
    assert np.all(V[fc.zero_row(n)] == 0) and np.all(V[:, fc.zero_col(f)] == 0)
    assert np.all(np.isfinite(V)) and np.all(np.isfinite(W)) and np.all(np.isfinite(H))
    if kind == 'plain':
        assert np.all(W[fc.zero_row(n)] == 0)
    if kind == 'wide':
        assert np.all(W[:, fc.zero_component(k)] == 0) and fc.zero_component(k) != k - 1
        assert W[W > 0].max() / W[W > 0].min() > 2.0 ** 30
    if kind == 'spike':
        rest = np.delete(V.ravel(), np.ravel_multi_index(fc.spike_at(n, f), V.shape))
        assert V[fc.spike_at(n, f)] >= 0.99e4 * rest.max()
    if kind.startswith('scaled'):
        assert (np.log2(V.max()) > 90) == (kind == 'scaled-up') and (np.log2(V.max()) < -90) == (kind == 'scaled-down')


@pytest.mark.parametrize('kind', fc.KINDS)
@pytest.mark.parametrize('case', fc.CASES, ids=fc.case_id)
def test_the_emulation_is_within_every_bound(case, kind):
    n, f, k, _ = case[:4]
    V, W, H = fc.problem(kind, n, f, k)
    s, kchunk = regime(case)[:2]
    rec = fc.Record()
    got = fc.emulate(V, W, H, kchunk)
    fc.check_iteration(rec, '%s %s' % (fc.case_id(case), kind), V, W, H, got, s)
    if kind == 'plain' and fc.zero_row(n) is not None:
        assert np.all(got['W'][fc.zero_row(n)] == 0)
    print('\n'.join(rec.lines))


def test_three_emulated_iterations_in_sequence_are_within_every_bound():
    n, f, k, _ = fc.SEQUENCE_CASES[0]
    V, W, H = fc.problem('plain', n, f, k)
    s, kchunk = regime((n, f, k, 0))[:2]
    rec = fc.Record()
    for it in range(3):
        got = fc.emulate(V, W, H, kchunk)
        fc.check_iteration(rec, 'iteration %d' % (it + 1), V, W, H, got, s)
        W, H = got['W'], got['H']


# ---- planted faults ------------------------------------------------------------------------------------------------------------------
def exceeds(piece, got, ref, bound):
    worst, at = fc.Record().ratio(got, ref, bound)
    assert worst > 1.0, '%s: the planted fault stays within the bound (worst %.3f at %r)' % (piece, worst, at)
    return worst


@pytest.mark.parametrize('kind', ['plain', 'wide', 'spike'])
def test_dropping_lo_hi_exceeds_every_contraction_s_bound(kind):
    n, f, k, _ = PLANT
    V, W, H = fc.problem(kind, n, f, k)
    s, kchunk = regime(PLANT)[:2]
    with fc.without_lo_hi():
        got = fc.emulate(V, W, H, kchunk)
    assert fc.emulation().prod3.__name__ == 'prod3'
    ratios = (exceeds('Q', got['Q'], *fc.ref_Q(V, W, H)), exceeds('W_new', got['W'], *fc.ref_W(W, H, got['Q'])),
              exceeds('numerator', got['N'], *fc.ref_N(got['W'], got['Q'], s)))
    assert min(ratios) > 5, ratios
    # ... which the numerator's sum-based view cannot see: the same fault moves it by a few 1e-4 of its value
    ref = fc.ref_N(got['W'], got['Q'], s)[0]
    live = ref > 1e-3 * ref.max()
    assert np.max(np.abs(got['N'][live] - ref[live]) / ref[live]) < 1e-3


EDGES = [(piece, axis, how) for piece in ('Q', 'W', 'N') for axis in (0, 1) for how in ('zeroed', 'neighbour')]


@pytest.mark.parametrize('case', [(15, 17, 2, 0), (65, 65, 65, 0), PLANT], ids=fc.case_id)
@pytest.mark.parametrize('piece,axis,how', EDGES)
def test_a_wrong_last_row_column_or_component_exceeds_the_bound(case, piece, axis, how):
    """Q's last row and column, W_new's last row and component k - 1, the numerator's component k - 1 and last column."""
    n, f, k, _ = case
    V, W, H = fc.problem('plain', n, f, k)
    s, kchunk = regime(case)[:2]
    got = fc.emulate(V, W, H, kchunk)
    bad = got[piece].copy()
    edge = [slice(None), slice(None)]
    edge[axis] = -1
    other = list(edge)
    other[axis] = -2
    bad[tuple(edge)] = 0.0 if how == 'zeroed' else bad[tuple(other)]
    ref = {'Q': lambda: fc.ref_Q(V, W, H), 'W': lambda: fc.ref_W(W, H, got['Q']), 'N': lambda: fc.ref_N(got['W'], got['Q'], s)}[piece]()
    exceeds('%s, axis %d %s' % (piece, axis, how), bad, *ref)


def test_a_tile_s_q_scale_from_the_neighbouring_tile_exceeds_the_bound():
    """The spike's tile under its neighbour's scale: the spike's ratio is 1e4 times the neighbour's largest, its scaled operand beyond
    fp16's range."""
    n, f, k, _ = PLANT
    V, W, H = fc.problem('spike', n, f, k)
    s, kchunk = regime(PLANT)[:2]
    got = fc.emulate(V, W, H, kchunk)
    tile = fc.spike_at(n, f)[1] // fc.TILE
    assert 0 < tile < -(-f // fc.TILE) - 1
    right = (W * fc.qht_with_neighbour_scale(got['Q'], H, tile, tile)).astype(np.float32)
    assert np.array_equal(right, got['W'])                               # the restated loop is the emulation's
    for neighbour in (tile - 1, tile + 1):
        bad = (W * fc.qht_with_neighbour_scale(got['Q'], H, tile, neighbour)).astype(np.float32)
        exceeds('W_new', bad, *fc.ref_W(W, H, got['Q']))


def test_a_component_s_xmax_from_another_component_exceeds_the_bound():
    """The component with the largest W_new qr under the scale of the one with the smallest non-zero maximum (wide: 2^+-12 apart)."""
    n, f, k, _ = PLANT
    V, W, H = fc.problem('wide', n, f, k)
    s, kchunk = regime(PLANT)[:2]
    got = fc.emulate(V, W, H, kchunk)
    top = (got['W'] * fc.qr_of(got['Q'])[:, None]).max(axis=0)
    big = int(np.argmax(top))
    small = int(np.argmin(np.where(top > 0, top, np.inf)))
    assert top[big] >= 8 * top[small] > 0

    def stale(sc):
        sc = sc.copy()
        sc[big] = sc[small]
        return sc
    assert np.array_equal(fc.numerator(got['W'], got['Q'], kchunk), got['N'])
    exceeds('numerator', fc.numerator(got['W'], got['Q'], kchunk, wj=stale), *fc.ref_N(got['W'], got['Q'], s))
    assert top[fc.zero_component(k)] == 0 and np.all(got['N'][fc.zero_component(k)] == 0)          # xmax = 0: scale 1, zeros


def test_leaving_out_a_chunk_s_last_partial_contraction_step_exceeds_the_bound():
    n, f, k, _ = PLANT_CHUNKED
    V, W, H = fc.problem('plain', n, f, k)
    s, kchunk = regime(PLANT_CHUNKED)[:2]
    assert kchunk % fc.CK == 16
    got = fc.emulate(V, W, H, kchunk)
    bad = fc.numerator(got['W'], got['Q'], kchunk, rows=lambda a, b: (a, a + (b - a) // fc.CK * fc.CK))
    exceeds('numerator', bad, *fc.ref_N(got['W'], got['Q'], s))
