"""Masked batches (include/klnmf_batch_mask.h, multimodal_amd/csrc/batch.hip.h): B dense problems of one shape, each under its own
row x modality presence mask, advancing through the masked loop together, one launch per stage.

What is held to what:
  * every problem of a masked batch against THE SAME masked problem alone in a `_native.Context` (upload_presence) whose
    KLNMF_EX_ROW_CHUNKS / KLNMF_EX_W_CHUNKS are forced to the counts the batch reports: W0, W, H, the loss record, n_done and the
    stop flag BIT FOR BIT (np.array_equal: no tolerance) -- on the natural routes, on forced routes, with problems that stop
    apart, in transforms, through the device gather and across the mask's state changes;
  * and against the chunked fp64 restatement of the masked update (tests/presence_cases.ref_fit_p), within the exact modes' bars
    (tests/test_batch_gpu.BARS with its floors, unchanged):
        f64   fit losses 1e-10, fit W and H 1e-9
        f32   fit losses 3e-5 (relative to at least 2^-23 sum(V)), fit W and H 3e-4 relative to max(|reference|, the smallest
              normal fp32 number) -- the reference fed the fp32-rounded inputs, the mask included
    (W0: 1e-12 and 3e-5);
  * the batch's reported counts against tests/exact_cases.exact_regime for max(1, cu_count // B) compute units.
Every problem of a batch has its own data, its own H0 and its own mask (presence_cases.mask, a seed per problem: exact zeros and
ones, an all-zero row, for M >= 3 a modality absent from every row).  Fits never stop early (NO_STOP) except in the test that is
about stopping.
"""
import functools

import numpy as np
import pytest

from multimodal_amd import _native
from tests import exact_cases as ec
from tests import presence_cases as pc
from tests.loop_piece_cases import stop_rule
from tests.test_batch_gpu import (BARS, FLOOR, FORCED, ITERS, PRECS, STOP_CAP, STOP_SHAPE, STOP_TOL, assert_same_bits, class_blocks,
                                  cu_count, esize, loss_floor, problem, raises, rank_one, seen, set_switches, upload_form)
from tests.test_sparse_gpu import _MEASURED, _report_measured, check  # noqa: F401  (the autouse fixture prints what was measured)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def mask_of(n, f, k, M, p):
    """Problem p's mask (fp64) and the batch's bounds."""
    return pc.mask(n, M, seed=7 * n + 3 * f + k + M + 101 * p), tuple(pc.bounds(f, M))


@functools.lru_cache(maxsize=16)
def reference(n, f, k, M, p, f32_inputs, kchunk, wchunk, fit):
    """(W0, (W, H, losses)) of problem p's masked fit in fp64 over the kernels' chunks; M = 0: the unweighted reference."""
    V, H0 = problem(n, f, k, p)
    P, b = mask_of(n, f, k, M, p) if M else (None, None)
    if f32_inputs:
        V, H0 = ec.as_f32(V), ec.as_f32(H0)
        P = ec.as_f32(P) if M else None
    if not M:
        return ec.ref_init_W(V, H0, wchunk), ec.ref_fit(V, H0, ITERS, fit=fit, components=H0, kchunk=kchunk, wchunk=wchunk)
    return ec.ref_init_W(V, H0, wchunk), pc.ref_fit_p(V, P, b, H0, ITERS, fit=fit, components=H0, kchunk=kchunk, wchunk=wchunk)


def place(batch, prec, Vs, Ps, bounds, H0s):
    """V, the mask (None: no upload for that problem) and H0 of every problem."""
    for p, (V, P, H0) in enumerate(zip(Vs, Ps, H0s)):
        batch.upload_V(p, upload_form(prec, V))
        if P is not None:
            batch.upload_presence(p, upload_form(prec, P), bounds)
        batch.set_H(p, upload_form(prec, H0))


def loop(batch, prec, iters=ITERS, fit=True, tol_abs=ec.NO_STOP, components=None):
    """[(W0, W, H, errors, n_done, stopped)] per problem: W0 = V.H0^T, the loop."""
    batch.init_W()
    W0s = [batch.get_W(p) for p in range(batch.count)]
    if components is not None:
        for p, H in enumerate(components):
            batch.set_H(p, upload_form(prec, H))
    results = batch.run(iters, fit, tol_abs)
    return [(W0s[p], batch.get_W(p), batch.get_H(p), np.array(results[p][0]), results[p][1], results[p][2]) for p in range(batch.count)]


def batch_run(batch, prec, Vs, Ps, bounds, H0s, **kw):
    place(batch, prec, Vs, Ps, bounds, H0s)
    return loop(batch, prec, **kw)


def solo_run(monkeypatch, prec, V, P, bounds, H0, k, regime, iters=ITERS, fit=True, tol_abs=ec.NO_STOP, h_seg=0):
    """The same masked problem alone in a context, its chunk counts forced to `regime`'s (P None: the unmasked problem)."""
    set_switches(monkeypatch, row_chunks=regime[0], w_chunks=regime[1], h_seg=h_seg)
    with _native.Context(prec) as ctx:
        ctx.set_problem(V.shape[0], V.shape[1], k, iters)
        assert ctx.exact_regime() == tuple(regime), (ctx.exact_regime(), regime)
        ctx.upload_V(upload_form(prec, V))
        if P is not None:
            ctx.upload_presence(upload_form(prec, P), bounds)
            assert ctx.presence() == len(bounds) - 1
        ctx.set_H(upload_form(prec, H0))
        ctx.init_W()
        W0 = ctx.get_W()
        errors, n_done, stopped = ctx.run(iters, fit, tol_abs)
        return W0, ctx.get_W(), ctx.get_H(), np.array(errors), n_done, stopped


def check_against_reference(case, prec, got, ref, V, P, bounds):
    W0r, (Wr, Hr, er) = ref
    weight = V if P is None else pc.omega(seen(prec, P), bounds) * V
    check(case, 'W0', got[0], W0r, BARS[prec]['step'], FLOOR[prec])
    assert len(got[3]) == len(er)
    check(case, 'losses', got[3], er, BARS[prec]['fit_loss'], loss_floor(prec, weight))
    check(case, 'W', got[1], Wr, BARS[prec]['fit_factor'], FLOOR[prec])
    check(case, 'H', got[2], Hr, BARS[prec]['fit_factor'], FLOOR[prec])


def inputs(n, f, k, M, B):
    probs = [problem(n, f, k, p) for p in range(B)]
    masks = [mask_of(n, f, k, M, p) for p in range(B)]
    return [v for v, _ in probs], [P for P, _ in masks], list(masks[0][1]), [h for _, h in probs]


# ---- 1. batch against solo runs and the fp64 reference ---------------------------------------------------------------------------
# (shape, M): the smallest that reach each branch (DESIGN 7h lists them)
SHAPES = [((15, 17, 1), 1),             # the degenerate shape, one modality
          ((65, 65, 65), 3),            # bounds [0, 1, 64, 65]: a tile of several modalities; D_part's second, one-component block
          ((300, 700, 17), 2),          # three D chunks, the last one 44 rows
          (ec.MID, 16),                 # the most modalities
          ((4096, 128, 16), 3),         # the H rule from the slabs ...
          ((4096, 129, 16), 3),         # ... and from their sum: the two sides of the slab rule
          ((8200, 33, 5), 2)]           # ceil(n / 128) = 65 > 64: D's chunk cap
BATCHES = [(s, M, B) for s, M in SHAPES for B in (2, 3, 5)] + [((100, 16385, 33), 3, 2)]      # (the segmented H rule under FacPresH)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('shape,M,B', BATCHES, ids=['%s-M%d-B%d' % (ec.case_id(s), M, B) for s, M, B in BATCHES])
def test_masked_batch_against_solo_runs_and_the_reference(monkeypatch, prec, shape, M, B):
    n, f, k = shape
    cu_eff = max(1, cu_count() // B)
    s, kchunk, w, wchunk, h, slabs = ec.exact_regime(n, f, k, cu_eff, esize(prec))
    Vs, Ps, bounds, H0s = inputs(n, f, k, M, B)
    assert len(set(P.tobytes() for P in Ps)) == B          # every problem its own mask
    set_switches(monkeypatch)
    with _native.Batch(prec, B) as batch:
        batch.set_problem(n, f, k, ITERS)
        regime = batch.exact_regime()
        assert regime == ec.query_regime(n, f, k, cu_eff, esize=esize(prec)) == (s, w, h, int(slabs))
        assert batch.presence() == 0
        got = batch_run(batch, prec, Vs, Ps, bounds, H0s)
        assert batch.presence() == M and batch.exact_regime() == regime
    for p in range(B):
        case = '%s %s M=%d B=%d p=%d %r' % (prec, ec.case_id(shape), M, B, p, regime)
        assert got[p][4] == ITERS and not got[p][5]
        assert_same_bits(case, got[p], solo_run(monkeypatch, prec, Vs[p], Ps[p], bounds, H0s[p], k, regime))
        check_against_reference(case, prec, got[p], reference(n, f, k, M, p, prec != 'f64', kchunk, wchunk, True), seen(prec, Vs[p]),
                                Ps[p], bounds)


# ---- 2. degenerate masks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', PRECS)
def test_a_row_with_every_modality_absent_keeps_its_W0_and_adds_nothing_to_the_loss(monkeypatch, prec):
    """Problems 0 and 1 differ in the data of ONE row, absent from every modality in both: the row keeps its W0, and -- its loss
    terms and its ratios being exactly 0 -- the loss records and the dictionaries of the two problems have the same bits."""
    n, f, k = 300, 700, 17
    M, B, r = 2, 2, 130          # (row 130: inside a row tile, not the mask's own all-zero row 100)
    V0, H0 = problem(n, f, k, 0)
    V1 = V0.copy()
    V1[r] = problem(n, f, k, 1)[0][r] + 1.0
    P, bounds = mask_of(n, f, k, M, 0)
    P = P.copy()
    P[r] = 0.0
    set_switches(monkeypatch)
    with _native.Batch(prec, B) as batch:
        batch.set_problem(n, f, k, ITERS)
        regime = batch.exact_regime()
        got = batch_run(batch, prec, [V0, V1], [P, P], list(bounds), [H0, H0])
    for p, V in enumerate((V0, V1)):
        assert_same_bits('%s absent row p=%d' % (prec, p), got[p], solo_run(monkeypatch, prec, V, P, list(bounds), H0, k, regime))
        assert np.array_equal(got[p][1][r], got[p][0][r]) and np.array_equal(got[p][1][100], got[p][0][100])
        live = int(np.flatnonzero((P > 0).any(axis=1))[0])
        assert not np.array_equal(got[p][1][live], got[p][0][live])          # (a row with a modality present does move)
    assert not np.array_equal(got[0][0][r], got[1][0][r])                            # the rows do differ
    assert np.array_equal(got[0][3], got[1][3]) and np.array_equal(got[0][2], got[1][2])
    keep = np.arange(n) != r
    assert np.array_equal(got[0][1][keep], got[1][1][keep])


@pytest.mark.parametrize('prec', PRECS)
def test_a_modality_absent_from_every_row_of_one_problem(monkeypatch, prec):
    """Problem 1 has modality 1 nowhere: D[:, 1] = 0, so its H keeps factor 1 in that modality's columns before the rows are
    normalised -- after one iteration H1[a, j] = fl(H0[a, j] / d_a) there, one divisor per row: H0 / H1 is constant along those
    columns to two roundings (4 units of the precision's epsilon allowed).  Problem 0 beside it has every modality."""
    n, f, k = 300, 700, 17
    M, B = 3, 2
    Vs, Ps, bounds, H0s = inputs(n, f, k, M, B)
    Ps = [Ps[0].copy(), Ps[1].copy()]
    Ps[0][:, 1] = np.where(np.arange(n) % 3 == 0, 0.0, 1.0)          # (presence_cases.mask empties modality M // 2 itself: fill it here)
    Ps[1][:, 1] = 0.0
    cols = slice(bounds[1], bounds[2])
    eps = {'f64': 2.0 ** -52, 'f32': 2.0 ** -23}[prec]
    set_switches(monkeypatch)
    with _native.Batch(prec, B) as batch:
        batch.set_problem(n, f, k, ITERS)
        regime = batch.exact_regime()
        one = batch_run(batch, prec, Vs, Ps, bounds, H0s, iters=1)
        got = batch_run(batch, prec, Vs, Ps, bounds, H0s)
    H0u = seen(prec, H0s[1])
    ratio = H0u[:, cols] / one[1][2][:, cols]
    assert np.all(np.abs(ratio / ratio[:, :1] - 1.0) <= 4 * eps), float(np.max(np.abs(ratio / ratio[:, :1] - 1.0)))
    ratio0 = seen(prec, H0s[0])[:, cols] / one[0][2][:, cols]
    assert np.max(np.abs(ratio0 / ratio0[:, :1] - 1.0)) > 1e-3          # (where the modality is present the factor is not 1)
    for p in range(B):
        case = '%s absent modality p=%d' % (prec, p)
        assert_same_bits(case, got[p], solo_run(monkeypatch, prec, Vs[p], Ps[p], bounds, H0s[p], k, regime))
        assert_same_bits(case + ' one iteration', one[p], solo_run(monkeypatch, prec, Vs[p], Ps[p], bounds, H0s[p], k, regime, iters=1))


@pytest.mark.parametrize('prec', PRECS)
def test_a_problem_without_an_upload_runs_on_a_mask_of_ones(monkeypatch, prec):
    n, f, k = ec.MID
    M, B = 3, 3
    Vs, Ps, bounds, H0s = inputs(n, f, k, M, B)
    cu_eff = max(1, cu_count() // B)
    s, kchunk, w, wchunk, h, slabs = ec.exact_regime(n, f, k, cu_eff, esize(prec))
    set_switches(monkeypatch)
    with _native.Batch(prec, B) as batch:
        batch.set_problem(n, f, k, ITERS)
        regime = batch.exact_regime()
        got = batch_run(batch, prec, Vs, [Ps[0], None, Ps[2]], bounds, H0s)          # (problem 1: no upload)
        assert batch.presence() == M
    ones = np.ones((n, M))
    for p, P in enumerate((Ps[0], ones, Ps[2])):
        assert_same_bits('%s no upload p=%d' % (prec, p), got[p], solo_run(monkeypatch, prec, Vs[p], P, bounds, H0s[p], k, regime))
    check_against_reference('%s no upload against the unweighted reference' % prec, prec, got[1],
                            reference(n, f, k, 0, 1, prec != 'f64', kchunk, wchunk, True), seen(prec, Vs[1]), None, None)


# ---- 3. forced routes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('forced', FORCED, ids=['%s-%d' % fv for fv in FORCED])
def test_forced_routes_on_the_masked_batch(monkeypatch, prec, forced):
    n, f, k = ec.MID
    M, B = 3, 3
    kw = {forced[0]: forced[1]}
    cu_eff = max(1, cu_count() // B)
    s, kchunk, w, wchunk, h, slabs = ec.exact_regime(n, f, k, cu_eff, esize(prec), **kw)
    Vs, Ps, bounds, H0s = inputs(n, f, k, M, B)
    set_switches(monkeypatch, **kw)
    with _native.Batch(prec, B) as batch:
        batch.set_problem(n, f, k, ITERS)
        regime = batch.exact_regime()
        assert regime == (s, w, h, int(slabs))
        got = batch_run(batch, prec, Vs, Ps, bounds, H0s)
    for p in range(B):
        case = '%s %s=%d p=%d %r' % (prec, forced[0], forced[1], p, regime)
        assert_same_bits(case, got[p], solo_run(monkeypatch, prec, Vs[p], Ps[p], bounds, H0s[p], k, regime, h_seg=kw.get('h_seg', 0)))
        check_against_reference(case, prec, got[p], reference(n, f, k, M, p, prec != 'f64', kchunk, wchunk, True), seen(prec, Vs[p]),
                                Ps[p], bounds)


# ---- 4. problems that stop apart ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', PRECS)
def test_masked_problems_that_stop_apart(monkeypatch, prec):
    """tests/test_batch_gpu.test_problems_that_stop_apart's construction under ONE mask for the three problems, with no all-absent
    row: problem 0 is exactly of rank 1 and the rule (tol_abs = 1) fires within a few evaluations (the fp64 restatement: after 4
    recorded losses); the generic problems lose 90 and more per iteration and run to the cap."""
    n, f, k = STOP_SHAPE
    M, B = 2, 3
    Vs = [rank_one(n, f, 5)] + [problem(n, f, k, p)[0] for p in (1, 2)]
    H0s = [problem(n, f, k, p)[1] for p in range(B)]
    P, bounds = mask_of(n, f, k, M, 0)
    P = P.copy()
    P[~(P > 0).any(axis=1)] = 1.0
    assert (P > 0).any(axis=1).all() and (P == 0).any()
    cu_eff = max(1, cu_count() // B)
    s, kchunk, w, wchunk, h, slabs = ec.exact_regime(n, f, k, cu_eff, esize(prec))
    ref_done = [stop_rule(pc.ref_fit_p(V, P, list(bounds), H0, STOP_CAP, kchunk=kchunk, wchunk=wchunk)[2], STOP_TOL) for V, H0 in zip(Vs, H0s)]
    assert 0 < ref_done[0] < 16 and ref_done[1] == ref_done[2] == STOP_CAP, ref_done
    set_switches(monkeypatch)
    with _native.Batch(prec, B) as batch:
        batch.set_problem(n, f, k, STOP_CAP)
        regime = batch.exact_regime()
        got = batch_run(batch, prec, Vs, [P] * B, list(bounds), H0s, iters=STOP_CAP, tol_abs=STOP_TOL)
    solos = [solo_run(monkeypatch, prec, Vs[p], P, list(bounds), H0s[p], k, regime, iters=STOP_CAP, tol_abs=STOP_TOL) for p in range(B)]
    assert solos[0][4] < solos[1][4] and solos[0][4] < solos[2][4], [s_[4] for s_ in solos]          # (else the input is wrong)
    for p in range(B):
        assert_same_bits('%s masked stop p=%d' % (prec, p), got[p], solos[p])
        assert len(got[p][3]) == got[p][4]
    assert got[0][5] and not got[1][5] and not got[2][5]
    assert got[0][4] < got[1][4] == got[2][4] == STOP_CAP
    if prec == 'f64':
        assert [g[4] for g in got] == ref_done


# ---- 5. transforms ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('shape,M', [((65, 65, 65), 3), ((300, 700, 17), 2)], ids=lambda v: ec.case_id(v) if isinstance(v, tuple) else 'M%d' % v)
def test_masked_transform_with_a_dictionary_per_problem(monkeypatch, prec, shape, M):
    n, f, k = shape
    B = 3
    Vs, Ps, bounds, H0s = inputs(n, f, k, M, B)
    cu_eff = max(1, cu_count() // B)
    s, kchunk, w, wchunk, h, slabs = ec.exact_regime(n, f, k, cu_eff, esize(prec))
    set_switches(monkeypatch)
    with _native.Batch(prec, B) as batch:
        batch.set_problem(n, f, k, ITERS)
        regime = batch.exact_regime()
        got = batch_run(batch, prec, Vs, Ps, bounds, H0s, fit=False)
    for p in range(B):
        case = '%s %s M=%d transform p=%d' % (prec, ec.case_id(shape), M, p)
        assert np.array_equal(got[p][2], seen(prec, H0s[p])), case + ': the dictionary changed'
        assert_same_bits(case, got[p], solo_run(monkeypatch, prec, Vs[p], Ps[p], bounds, H0s[p], k, regime, fit=False))
        check_against_reference(case, prec, got[p], reference(n, f, k, M, p, prec != 'f64', kchunk, wchunk, False), seen(prec, Vs[p]),
                                Ps[p], bounds)


# ---- 6. the device gather ------------------------------------------------------------------------------------------------------------
GN, GF, GK = 67, 130, 5
G_BOUNDS = [0, 1, 65, 130]
G_SRC_ROWS, G_LD, G_SRC_COLS = 200, 5, [4, -1, 0]          # (a -1 column: that modality's weights are 1)


def gather_rows():
    rng = np.random.default_rng(9)
    return [rng.integers(0, 12, GN),                        # repeats
            rng.permutation(G_SRC_ROWS)[:GN],               # arbitrary order
            np.arange(100, 100 + GN)[::-1].copy()]          # descending


def selected(R, idx):
    out = np.ones((len(idx), len(G_SRC_COLS)), dtype=R.dtype)
    for m, c in enumerate(G_SRC_COLS):
        if c >= 0:
            out[:, m] = R[idx, c]
    return out


@pytest.mark.parametrize('src', ['f32', 'f64'], ids=['src-f32', 'src-f64'])
@pytest.mark.parametrize('prec', PRECS)
def test_the_device_gather_is_the_host_upload_bit_for_bit(monkeypatch, prec, src):
    import torch
    B = 3
    probs = [problem(GN, GF, GK, p) for p in range(B)]
    Vs, H0s = [v for v, _ in probs], [h for _, h in probs]
    R = pc.mask(G_SRC_ROWS, G_LD, seed=31)
    Rs = R.astype(np.float32) if src == 'f32' else R
    idxs = gather_rows()
    set_switches(monkeypatch)
    with _native.Batch(prec, B) as batch:
        batch.set_problem(GN, GF, GK, ITERS)
        want = batch_run(batch, prec, Vs, [selected(Rs, i) for i in idxs], G_BOUNDS, H0s)
        assert len(set(w[1].tobytes() for w in want)) == B
    dR = torch.from_numpy(np.ascontiguousarray(Rs)).cuda()
    with _native.Batch(prec, B) as batch:
        batch.set_problem(GN, GF, GK, ITERS)
        place(batch, prec, Vs, [None] * B, G_BOUNDS, H0s)
        assert batch.presence() == 0
        for p in (2, 0, 1):                                                          # (any order of the problems)
            d_idx = torch.from_numpy(np.asarray(idxs[p], dtype=np.int64)).cuda()
            batch.upload_presence_device_rows(p, dR.data_ptr(), src == 'f64', G_SRC_ROWS, dR.stride(0), d_idx.data_ptr(), GN, G_SRC_COLS,
                                              G_BOUNDS)
            del d_idx                                                                # (synchronous: free to go)
        assert batch.presence() == 3
        got = loop(batch, prec)
    for p in range(B):
        assert_same_bits('%s %s gather p=%d' % (prec, src, p), got[p], want[p])
    # null indices: rows 0 .. n - 1 of the source
    with _native.Batch(prec, 1) as batch:
        batch.set_problem(GN, GF, GK, ITERS)
        place(batch, prec, Vs[:1], [None], G_BOUNDS, H0s[:1])
        batch.upload_presence_device_rows(0, dR.data_ptr(), src == 'f64', G_SRC_ROWS, dR.stride(0), 0, GN, G_SRC_COLS, G_BOUNDS)
        head = loop(batch, prec)[0]
        place(batch, prec, Vs[:1], [selected(Rs, np.arange(GN))], G_BOUNDS, H0s[:1])
        assert_same_bits('%s %s gather of the first rows' % (prec, src), head, loop(batch, prec)[0])


# ---- 7. state and refusals -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', PRECS)
def test_state_and_refusals(monkeypatch, prec):
    import torch
    n, f, k = 300, 700, 17
    M, B = 2, 3
    Vs, Ps, bounds, H0s = inputs(n, f, k, M, B)
    Pu = [upload_form(prec, P) for P in Ps]
    set_switches(monkeypatch)

    def same(a, b, what):
        for p in range(B):
            assert_same_bits('%s %s p=%d' % (prec, what, p), a[p], b[p])

    def rerun(batch):
        """The fit again from H0 on what the batch holds: V and the mask are not uploaded again."""
        for p in range(B):
            batch.set_H(p, upload_form(prec, H0s[p]))
        return loop(batch, prec)
    with _native.Batch(prec, B) as batch:
        assert batch.presence() == 0                                                 # no problem yet
        raises(_native.ERR_ARG, batch.upload_presence, 0, Pu[0], bounds)             # a call with no problem set
        raises(_native.ERR_ARG, batch.clear_presence)
        batch.set_problem(n, f, k, ITERS)
        assert batch.presence() == 0
        plain = batch_run(batch, prec, Vs, [None] * B, bounds, H0s)
        dR = torch.from_numpy(np.ascontiguousarray(Ps[0])).cuda()
        good = torch.arange(n, dtype=torch.int64).cuda()
        bad_low, bad_high = good.clone(), good.clone()
        bad_low[n // 2] = -1
        bad_high[n - 1] = n

        def gather(p=0, ptr=dR.data_ptr(), idx=good, rows=n, row0=0, cols=(0, -1), b=bounds, src_rows=n, ld=M):
            batch.upload_presence_device_rows(p, ptr, True, src_rows, ld, idx.data_ptr(), rows, list(cols), b, row0=row0)

        def refusals():
            """Every refusal of the two uploads; none reads or writes through a bad index."""
            for p in (-1, B):
                raises(_native.ERR_ARG, batch.upload_presence, p, Pu[0], bounds)
                raises(_native.ERR_ARG, gather, p=p)
            for b in ([0, 300, 699], [1, 300, 700], [0, 300, 300, 700][:3], [0, 400, 300], [0, 0, 700]):      # bad bounds
                raises(_native.ERR_ARG, batch.upload_presence, 0, Pu[0], b)
                raises(_native.ERR_ARG, gather, b=b)
            raises(_native.ERR_ARG, batch.upload_presence, 0, np.ones((n, 17), dtype=Pu[0].dtype), list(range(17)) + [f])      # n_mod = 17
            raises(_native.ERR_ARG, batch.upload_presence, 0, Pu[0], bounds, row0=1)          # rows out of range
            raises(_native.ERR_ARG, batch.upload_presence, 0, Pu[0], bounds, row0=-1)
            raises(_native.ERR_ARG, gather, rows=n, row0=1)
            raises(_native.ERR_ARG, gather, idx=torch.zeros(1, dtype=torch.int64).cuda(), rows=-1)
            raises(_native.ERR_ARG, gather, cols=(0, M))                                      # a source column outside [-1, ld)
            raises(_native.ERR_ARG, gather, cols=(-2, 0))
            raises(_native.ERR_ARG, gather, idx=bad_low)                                      # a row index outside [0, src_rows)
            raises(_native.ERR_ARG, gather, idx=bad_high)
            raises(_native.ERR_ARG, gather, idx=good, src_rows=n - 1)
            raises(_native.ERR_ARG, gather, ptr=0)                                            # a null source
            lib, h = batch._lib, batch._h
            cb = (_native._i64 * 3)(*bounds)
            assert lib.klnmf_batch_upload_presence(h, 0, None, _native.DT_F64, n, M, 0, cb, M) == _native.ERR_ARG
            assert lib.klnmf_batch_upload_presence(h, 0, Pu[0].ctypes.data, 99, n, M, 0, cb, M) == _native.ERR_ARG      # an unknown dtype
        # every refusal on the unmasked batch: it stays unmasked, with its bits
        refusals()
        assert batch.presence() == 0
        same(rerun(batch), plain, 'unmasked after refusals')
        # the masked batch
        masked = batch_run(batch, prec, Vs, Ps, bounds, H0s)
        assert batch.presence() == M
        assert not np.array_equal(masked[0][1], plain[0][1])
        refusals()
        raises(_native.ERR_ARG, batch.upload_presence, 0, Pu[0], [0, 301, 700])              # other bounds after the first upload
        raises(_native.ERR_ARG, gather, b=[0, 301, 700])
        raises(_native.ERR_ARG, batch.upload_presence, 0, np.ones((n, 1), dtype=Pu[0].dtype), [0, 700])
        assert batch.presence() == M
        same(rerun(batch), masked, 'masked after refusals')
        # clear: the unmasked batch's bits; and a mask again
        batch.clear_presence()
        assert batch.presence() == 0
        batch.clear_presence()                                                       # (nothing to clear: nothing happens)
        same(rerun(batch), plain, 'cleared')
        batch.upload_presence(1, Pu[1], [0, 301, 700])                               # (a cleared batch takes other bounds)
        assert batch.presence() == M
        batch.clear_presence()
        same(batch_run(batch, prec, Vs, Ps, bounds, H0s), masked, 'masked again')
        # another shape and back: set_problem drops the mask
        batch.set_problem(65, 65, 65, ITERS)
        assert batch.presence() == 0
        batch.set_problem(n, f, k, ITERS)
        assert batch.presence() == 0
        same(batch_run(batch, prec, Vs, [None] * B, bounds, H0s), plain, 'after set_problem')
    # a batch that never held a mask
    with _native.Batch(prec, B) as batch:
        batch.set_problem(n, f, k, ITERS)
        same(batch_run(batch, prec, Vs, [None] * B, bounds, H0s), plain, 'a fresh batch')


# ---- 8. the Python layers --------------------------------------------------------------------------------------------------------------
def masked_blocks():
    """tests/test_batch_gpu.class_blocks() and a mask: the second modality absent from a seeded third of the rows (so no row loses
    both)."""
    data, labels = class_blocks()
    n = len(labels)
    absent = np.zeros(n, dtype=bool)
    absent[np.random.default_rng(12).permutation(n)[:n // 3]] = True
    return data, labels, [None, np.where(absent, 0.0, 1.0)]


@pytest.mark.parametrize('prec', PRECS)
def test_masked_train_many_against_a_loop_over_train(monkeypatch, prec):
    from multimodal_amd.device_data import DeviceDataset
    from multimodal_amd.learner import MultimodalLearner
    monkeypatch.setenv('KLNMF_PRECISION', prec)
    monkeypatch.delenv('KLNMF_DEVICES', raising=False)
    data, _, presence = masked_blocks()
    ds = DeviceDataset(data, device=0, presence=presence)
    k, n = 6, len(data[0])
    rng = np.random.default_rng(4)
    rows_list = [sorted(rng.permutation(n)[:90].tolist()) for _ in range(3)]
    assert all(0 < sum(presence[1][r] == 0 for r in rows) < 90 for rows in rows_list)
    inits = [ec.factors(90, sum(ds.dims), k, seed=p)[1] for p in range(3)]

    def learners():
        return [MultimodalLearner(['a', 'b'], list(ds.dims), [1.0, 0.5], k) for _ in range(3)]
    many = ds.train_many(learners(), rows_list, ITERS, init_dictionaries=inits)
    assert ds.last_weights_route == 'presence'
    for p, (learner, alone) in enumerate(zip(many, learners())):
        ds.train(alone, rows_list[p], ITERS, init_dictionary=inits[p])
        assert alone.nmf_train.last_weights_route == 'presence'
        assert learner.nmf_train.last_batch_size == 3
        assert learner.nmf_train.last_weights_route == 'presence'
        check('%s masked train_many p=%d' % (prec, p), 'H', learner.dico, alone.dico, BARS[prec]['fit_factor'], FLOOR[prec])
    # transforms of the trained learners on the masked modality: the same route
    Ws = ds.reconstruct_internal_multi_many(many, ['b'], [r[:30] for r in rows_list], ITERS)
    assert ds.last_weights_route == 'presence'
    for p, learner in enumerate(many):
        Wa = ds.reconstruct_internal_multi(learner, ['b'], rows_list[p][:30], ITERS)
        assert ds.last_weights_route == 'presence'
        check('%s masked internal_many p=%d' % (prec, p), 'W', Ws[p], Wa, BARS[prec]['fit_factor'], FLOOR[prec])
    # ... and on the unmasked one: the unmasked batch
    Ws = ds.reconstruct_internal_multi_many(many, ['a'], [r[:30] for r in rows_list], ITERS)
    assert ds.last_weights_route is None
    for p, learner in enumerate(many):
        Wa = ds.reconstruct_internal_multi(learner, ['a'], rows_list[p][:30], ITERS)
        check('%s unmasked internal_many p=%d' % (prec, p), 'W', Ws[p], Wa, BARS[prec]['fit_factor'], FLOOR[prec])
    # row lists of unequal length: the loop over train, its bits
    uneven = [rows_list[0], rows_list[1][:80], rows_list[2]]
    inits_u = [ec.factors(len(r), sum(ds.dims), k, seed=p)[1] for p, r in enumerate(uneven)]
    seq = ds.train_many(learners(), uneven, ITERS, init_dictionaries=inits_u)
    for p, (learner, alone) in enumerate(zip(seq, learners())):
        ds.train(alone, uneven[p], ITERS, init_dictionary=inits_u[p])
        assert np.array_equal(learner.dico, alone.dico)
        assert getattr(learner.nmf_train, 'last_batch_size', 1) == 1 and learner.nmf_train.last_weights_route == 'presence'


@pytest.mark.parametrize('prec', PRECS)
def test_fit_transform_batch_with_presence_columns(prec):
    from multimodal_amd.lib.nmf import KLdivNMF, fit_transform_batch
    n, f, k = 300, 700, 17
    probs = [problem(n, f, k, p) for p in range(3)]
    ws = [mask_of(n, f, k, 1, p)[0] for p in range(3)]
    assert all(w.shape == (n, 1) and (w == 0).any() for w in ws)

    def models():
        out = []
        for _, H0 in probs:
            m = KLdivNMF(n_components=k, max_iter=ITERS, tol=0, precision=prec, device=0)
            m._init_dictionary = H0
            out.append(m)
        return out
    batched = models()
    outs = fit_transform_batch(batched, [v for v, _ in probs], weights=ws, return_errors=True)
    for p, (m, (W, errors)) in enumerate(zip(batched, outs)):
        assert m.last_batch_size == 3 and m.last_weights_route == 'presence'
        alone = models()[p]
        Wa, ea = alone.fit_transform(probs[p][0], weights=ws[p], return_errors=True)
        assert alone.last_weights_route == 'presence'
        case = '%s fit_transform_batch(weights) p=%d' % (prec, p)
        assert m.last_fp8_report == alone.last_fp8_report
        check(case, 'losses', errors, ea, BARS[prec]['fit_loss'], loss_floor(prec, ws[p] * probs[p][0]))
        check(case, 'W', W, Wa, BARS[prec]['fit_factor'], FLOOR[prec])
        check(case, 'H', m.components_, alone.components_, BARS[prec]['fit_factor'], FLOOR[prec])
    # one entry that routes to 'array': the sequential path, its bits
    mixed = [ws[0], np.broadcast_to(ws[1], (n, f)).copy(), ws[2]]
    seq = models()
    outs = fit_transform_batch(seq, [v for v, _ in probs], weights=mixed, return_errors=True)
    for p, (m, (W, errors)) in enumerate(zip(seq, outs)):
        assert m.last_batch_size == 1 and m.last_weights_route == ('array' if p == 1 else 'presence')
        alone = models()[p]
        Wa, ea = alone.fit_transform(probs[p][0], weights=mixed[p], return_errors=True)
        assert np.array_equal(W, Wa) and errors == ea and np.array_equal(m.components_, alone.components_)


# ---- 9. run_sweep ----------------------------------------------------------------------------------------------------------------------
def test_masked_run_sweep_in_batches_gives_the_unbatched_labels_and_scores(monkeypatch):
    """f64; tests/test_batch_gpu.test_run_sweep_in_batches...'s recording on a masked dataset.  Every nearest-example search of the
    unbatched masked sweep is decided by more than 1e-6 relative (asserted: a condition on the input), so the found labels, and
    with them the score tables, must be equal; the batched sweep opens batches of two -- masked trainings and transforms among
    them."""
    from multimodal_amd import device_data
    from multimodal_amd.device_experiment import run_sweep
    data, labels, presence = masked_blocks()
    original = device_data.DeviceEvaluation.found_labels
    found, margins = [], []

    def recording(self, test, examples, labels_ex, metric):
        out = self.torch.empty((test.shape[0], examples.shape[0]), dtype=self.torch.float64, device=self.dev)
        _native.all_distances_device(test.data_ptr(), test.stride(0), examples.data_ptr(), examples.stride(0), out.data_ptr(),
                                     test.shape[0], examples.shape[0], test.shape[1], metric, f64=True, device=self.dev.index or 0)
        d = np.sort(out.cpu().numpy(), axis=1)
        margins.extend(((d[:, 1] - d[:, 0]) / np.maximum(np.maximum(np.abs(d[:, 0]), np.abs(d[:, 1])), 1e-300)).tolist())
        got = original(self, test, examples, labels_ex, metric)
        found.append(list(got))
        return got
    monkeypatch.setattr(device_data.DeviceEvaluation, 'found_labels', recording)
    args = dict(ks=[6, 8], n_runs=2, iter_train=20, iter_test=20, devices=[0], precision='f64', seed=3, presence=presence)
    table1, raw1 = run_sweep(data, labels, ['a', 'b'], **args)
    found1, margins1 = list(found), list(margins)
    assert margins1 and np.all(np.isfinite(margins1)) and min(margins1) > 1e-6, min(margins1)
    del found[:], margins[:]
    opened, gathers = [], []
    real_batch = _native.Batch

    class CountingBatch(real_batch):
        def __init__(self, precision, count, device=0):
            opened.append(count)
            real_batch.__init__(self, precision, count, device)

        def upload_presence_device_rows(self, p, *a, **kw):
            gathers.append(p)
            return real_batch.upload_presence_device_rows(self, p, *a, **kw)
    monkeypatch.setattr(_native, 'Batch', CountingBatch)
    table3, raw3 = run_sweep(data, labels, ['a', 'b'], batch=3, **args)
    assert opened and set(opened) == {2}                      # two runs per k: batches of two, trainings and transforms
    assert gathers and set(gathers) == {0, 1}                 # and masks gathered into them
    assert found == found1
    assert raw3 == raw1 and table3 == table1
