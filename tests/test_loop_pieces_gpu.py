"""The loop's H rule and stop rule in isolation, on exchange buffers the test writes (tests/loop_piece_cases.py says how).

The benchmark's 16-bit loop is otherwise checked end to end only, to 1e-3 .. 1e-4 of the oracle's loss and 5e-3 of the factors'
maxima: one wrong dictionary column at a part boundary, a wrong tail at f % 4 != 0, a padding element leaking into a valid row
or a stop rule off by one at prev - err == tol_abs all pass that.  Here the two pieces behind the exchange get chosen inputs:

  1  a numerator N = 2^U(-20, 20) (padding 3e30) -> H, elementwise against `ref_h_rule` in fp64:  |got - ref| <= bar x ref,
     bar = 8 x 2^-24 where the masters are fp32, 8 x 2^-53 x (1 + f / 8) in 'f64' (loop_piece_cases.h_bar: derived there);
  2  the same through 2, 3 and 4 column parts: the parts' layout, and H bit for bit the unsplit context's;
  3  one-hot numerators at the seams of the layout; an all-zero numerator row; padding that holds inf / NaN;
  4  the 16-bit images follow the master: the next row pass's loss against the oracle's on (W, injected H), rtol 1e-4, where
     the fp16 image can hold the injected dictionary (MASTER_SHAPES), and on (W, the fp16 image of the injected H) at every
     shape with f > 1;
  5  scripted losses -> the stop rule, exact: n_done, the recorded doubles, the flag, and nothing moves after the stop;
  6  the pieces against the fused loop (`run`), bit for bit;
  7  the stop rule at prev - err == tol_abs exactly on the loop's own losses, fused and in pieces.

Every precision runs every test it has the pieces for ('f16' alone has column parts and 16-bit images).  A context that refuses
the loop or a piece must do so with KLNMF_ERR_UNSUPP and stay usable (`refused`).  Data is tiny: the pieces under test never
look at it.
"""
import functools

import numpy as np
import pytest

from multimodal_amd import _native
from oracle import klnmf_oracle as orc
from tests import loop_piece_cases as lp
from tests.test_sparse_gpu import _MEASURED, _report_measured, check  # noqa: F401  (the autouse fixture prints what was measured)

pytestmark = pytest.mark.gpu

F_SET = [1, 3, 127, 128, 129, 257, 1030, 4097]
K_SET = [1, 15, 16, 17, 33, 200]           # (every mode's limit is beyond: the 16-bit MFMA kernels cover k <= 512)
SHAPES = [(f, k) for f in F_SET for k in K_SET]


def shape_id(s):
    return 'f%d-k%d' % s


def rows_for(f, k):
    """n in {64, 300}: both at every f and at every k of SHAPES (each set holds odd and even values)."""
    return 64 if (f + k) % 2 == 0 else 300


@functools.lru_cache(maxsize=None)
def problem(n, f, k):
    """(V, H0), fp64, read-only: H0's entries are >= 1e-6, so that no product with a numerator >= 2^-20 underflows in fp32."""
    V = orc.synthetic_V(1000 + f + k, n, f, min(k, 12))
    H0 = orc.synthetic_H0(2000 + f + 7 * k, f, k)
    assert H0.min() >= 1e-6 and np.float32(H0.min()) * np.float32(2.0 ** -20) > 1e6 * np.finfo(np.float32).tiny
    V.setflags(write=False)
    H0.setflags(write=False)
    return V, H0


def wide_numerator(f, k, seed=0):
    """N = 2^U(-20, 20) per entry."""
    return 2.0 ** np.random.default_rng(10007 * seed + 31 * f + k).uniform(-20.0, 20.0, (k, f))


def refused(ctx, err):
    """A precision without the pieces: the refusal's code, and the context still works."""
    if isinstance(err, _native.NativeError) and err.code == _native.ERR_HIP:
        pytest.exit('the HIP runtime reported an error (%s): nothing more is started on this device' % err, returncode=3)
    assert isinstance(err, _native.NativeError) and err.code == _native.ERR_UNSUPP, err
    assert np.isfinite(ctx.error())
    _MEASURED.append('    refused: %s' % err)


def inject_once(prec, f, k, numerator, pad=lp.PAD, parts=1, monkeypatch=None, then=None):
    """One iteration in pieces whose numerator is overwritten behind the real column pass (loss[0] stays the row pass's, the stop
    rule cannot fire).  `numerator(xch, H_before)` -> N[k, f].  Returns (H_before as read back, N as the buffer holds it, H after,
    the Exchange, what `then(ctx, xch)` returned) -- or None after a refusal."""
    n = rows_for(f, k)
    V, H0 = problem(n, f, k)
    if monkeypatch is not None:
        monkeypatch.setenv('KLNMF_COMM_PARTS', str(parts))
    ctx, xch = lp.open_context(prec, V, H0, k, 2)
    with ctx:
        H_before = ctx.get_H()
        assert np.array_equal(H_before, H0 if prec == 'f64' else H0.astype(np.float32).astype(np.float64))
        N = xch.rounded(numerator(xch, H_before))
        try:
            result = lp.drive(ctx, 1, after_colpass=lambda it: xch.write_numerator(N, pad=pad), nparts=xch.nparts, end=then is None)
            extra = then(ctx, xch) if then is not None else None
        except _native.NativeError as e:
            refused(ctx, e)
            return None
        if then is None:
            errors, n_done, stopped = result
            assert (n_done, stopped) == (1, False) and len(errors) == 1 and np.isfinite(errors[0])
        return H_before, N, ctx.get_H(), xch, extra


# ---- 1. injected numerator -> H, elementwise ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', lp.PRECISIONS)
@pytest.mark.parametrize('shape', SHAPES, ids=shape_id)
def test_injected_numerator_gives_the_h_rule(prec, shape):
    f, k = shape
    out = inject_once(prec, f, k, lambda xch, H: wide_numerator(f, k))
    if out is None:
        return
    H_before, N, H_after, xch, _ = out
    assert xch.nparts == 1
    assert int(lp.valid_mask(xch.layout).sum()) == k * f
    check('%s %s' % (prec, shape_id(shape)), 'H rule', H_after, lp.ref_h_rule(H_before, N, f), lp.h_bar(prec, f))


# ---- 2. the same in column parts ---------------------------------------------------------------------------------------------------
PART_SHAPES = [(f, k) for f in (256, 257, 511, 513, 769, 1030) for k in (17, 200)]


@functools.lru_cache(maxsize=None)
def _unsplit_h(f, k):
    import os
    old = os.environ.get('KLNMF_COMM_PARTS')
    os.environ['KLNMF_COMM_PARTS'] = '1'
    try:
        out = inject_once('f16', f, k, lambda xch, H: wide_numerator(f, k))
    finally:
        if old is None:
            del os.environ['KLNMF_COMM_PARTS']
        else:
            os.environ['KLNMF_COMM_PARTS'] = old
    assert out is not None and out[3].nparts == 1
    out[2].setflags(write=False)
    return out[2]


def check_parts(f, k, parts, xch):
    """What `exchange_parts()` promises of the split layout."""
    raw = xch.raw_parts
    assert len(raw) == min(parts, -(-f // 256)) == xch.nparts
    assert sum(nc for _, _, _, nc in raw) == f
    assert all(c0 % 128 == 0 for _, _, c0, _ in raw)
    assert [c0 for _, _, c0, _ in raw] == [sum(nc for _, _, _, nc in raw[:p]) for p in range(len(raw))]
    spans = sorted((off, off + cnt) for off, cnt, _, _ in raw)
    assert spans[0][0] >= 0 and spans[-1][1] <= xch.layout.count
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans
    assert all(cnt % k == 0 and cnt // k >= nc for _, cnt, _, nc in raw)


@pytest.mark.parametrize('parts', [2, 3, 4])
@pytest.mark.parametrize('shape', PART_SHAPES, ids=shape_id)
def test_injected_numerator_in_column_parts(monkeypatch, parts, shape):
    f, k = shape
    whole = _unsplit_h(f, k)
    out = inject_once('f16', f, k, lambda xch, H: wide_numerator(f, k), parts=parts, monkeypatch=monkeypatch)
    assert out is not None
    H_before, N, H_after, xch, _ = out
    check_parts(f, k, parts, xch)
    check('f16 %s P=%d' % (shape_id(shape), parts), 'H rule', H_after, lp.ref_h_rule(H_before, N, f), lp.h_bar('f16', f))
    # the rule reads one value per element wherever the layout keeps it: no sum changes its order
    assert np.array_equal(H_after, whole), 'H differs from the unsplit context in %d elements (max %.3e)' % (
        int((H_after != whole).sum()), float(np.max(np.abs(H_after - whole))))


@pytest.mark.parametrize('prec', [p for p in lp.PRECISIONS if p != 'f16'])
def test_exact_precisions_have_one_part(monkeypatch, prec):
    monkeypatch.setenv('KLNMF_COMM_PARTS', '3')
    f, k = 769, 17
    V, H0 = problem(rows_for(f, k), f, k)
    ctx, xch = lp.open_context(prec, V, H0, k, 2)
    with ctx:
        assert xch.raw_parts == [(0, k * f, 0, f)] and xch.layout.count == k * f
        assert lp.valid_mask(xch.layout).all()
        try:
            ctx.loop_begin()
            ctx.iter_rowpass(True)
            with pytest.raises(_native.NativeError) as e:
                ctx.iter_colpass_part(1)
            assert e.value.code == _native.ERR_ARG
            ctx.iter_colpass_part(0)
            ctx.iter_decide(lp.NO_STOP)
            ctx.iter_update_H()
            ctx.iter_advance()
            assert ctx.loop_end(1)[1] == 1
        except _native.NativeError as err:
            refused(ctx, err)


# ---- 3. one-hot numerators at the seams, a zero row, padding that holds anything ---------------------------------------------------
SEAM_CASES = [(prec, f, k, parts) for prec in lp.PRECISIONS for (f, k) in [(3, 1), (257, 17), (1030, 33), (769, 200)]
              for parts in ((1, 2, 3, 4) if prec == 'f16' and f > 256 else (1,))]


@pytest.mark.parametrize('prec,f,k,parts', SEAM_CASES, ids=['%s-f%d-k%d-P%d' % c for c in SEAM_CASES])
def test_one_hot_numerators_at_the_seams(monkeypatch, prec, f, k, parts):
    """N[:, j] = 1, 0 elsewhere: every row of H is 0 except at j, where it is h / (kEpsNorm + h).  A column read from another
    part, offset or row lands somewhere else exactly."""
    n = rows_for(f, k)
    V, H0 = problem(n, f, k)
    monkeypatch.setenv('KLNMF_COMM_PARTS', str(parts))
    ctx, xch = lp.open_context(prec, V, H0, k, 2)
    with ctx:
        if parts > 1:
            check_parts(f, k, parts, xch)
        H_before = ctx.get_H()
        probes = {0, 127, 128, f - 1}
        for p in xch.layout.parts:
            probes |= {p.col0 - 1, p.col0, p.col0 + p.ncols - 1}
        worst = 0.0
        for j in sorted(c for c in probes if 0 <= c < f):
            N = np.zeros((k, f))
            N[:, j] = 1.0
            try:
                errors, n_done, stopped = lp.drive(ctx, 1, after_colpass=lambda it: xch.write_numerator(N), nparts=xch.nparts)
            except _native.NativeError as e:
                refused(ctx, e)
                return
            assert (n_done, stopped) == (1, False)
            H = ctx.get_H()
            ref = lp.ref_h_rule(H_before, N, f)
            assert np.count_nonzero(ref) == k and np.all(ref[:, j] > 0.999)
            others = np.delete(H, j, axis=1)
            assert np.all(others == 0), 'column %d: %d elements of other columns are not 0 (first at %r)' % (
                j, int(np.count_nonzero(others)), tuple(np.argwhere(np.delete(H, j, axis=1) != 0)[0]))
            err = float(np.max(np.abs(H[:, j] - ref[:, j]) / ref[:, j]))
            assert err <= lp.h_bar(prec, f), 'column %d: %.3e (bar %.1e)' % (j, err, lp.h_bar(prec, f))
            worst = max(worst, err)
            # the next probe starts from the same dictionary and coefficients
            ctx.set_H(H0)
            ctx.init_W()
            assert np.array_equal(ctx.get_H(), H_before)
        _MEASURED.append('    %-40s %-7s %.2e  (bar %.0e)' % ('%s f%d k%d P=%d one-hot' % (prec, f, k, parts), 'H rule', worst,
                                                              lp.h_bar(prec, f)))


ZERO_ROW_CASES = [(prec, f, k, parts) for prec in lp.PRECISIONS for (f, k) in [(129, 16), (513, 33)]
                  for parts in ((1, 2) if prec == 'f16' and f > 256 else (1,))]


@pytest.mark.parametrize('pad', [lp.PAD, np.inf, np.nan], ids=['pad3e30', 'padinf', 'padnan'])
@pytest.mark.parametrize('prec,f,k,parts', ZERO_ROW_CASES, ids=['%s-f%d-k%d-P%d' % c for c in ZERO_ROW_CASES])
def test_a_zero_numerator_row_and_padding_that_holds_anything(monkeypatch, prec, f, k, parts, pad):
    """One all-zero numerator row: its divisor is kEpsNorm and its H row exactly 0, finite; the other rows meet the bars.  What a
    collective leaves in the padding is not the library's to choose: 3e30, inf and NaN there must not reach a valid element
    (0 x inf is NaN: a padding element that is multiplied at all shows)."""
    zero = k // 2

    def numerator(xch, H):
        N = wide_numerator(f, k, seed=3)
        N[zero] = 0.0
        return N
    out = inject_once(prec, f, k, numerator, pad=pad, parts=parts, monkeypatch=monkeypatch)
    if out is None:
        return
    H_before, N, H_after, xch, _ = out
    assert np.all(np.isfinite(H_after))
    assert np.all(H_after[zero] == 0)
    check('%s f%d k%d P=%d pad %r' % (prec, f, k, parts, pad), 'H rule', H_after, lp.ref_h_rule(H_before, N, f), lp.h_bar(prec, f))


# ---- 4. the 16-bit images follow the master ------------------------------------------------------------------------------------------
def _loss_behind_the_injected_update(f, k):
    """'f16': the injected update of test 1, then one more real row pass.  (H before, N, H after, the loss that pass left in
    loss[0], W before that pass)."""
    def then(ctx, xch):
        ctx.iter_rowpass(True)
        loss = float(xch.read_loss()[0])
        errors, n_done, stopped = ctx.loop_end(2)
        assert (n_done, stopped) == (1, False)
        return loss, ctx.get_W()
    out = inject_once('f16', f, k, lambda xch, H: wide_numerator(f, k), then=then)
    assert out is not None
    H_before, N, H_after, xch, (loss, W) = out
    check('f16 %s' % shape_id((f, k)), 'H rule', H_after, lp.ref_h_rule(H_before, N, f), lp.h_bar('f16', f))
    return H_before, N, H_after, loss, W


# Where the loss on the MASTER dictionary is a fair reference for a pass that multiplies the dictionary's fp16 image (H x 8192
# rounded to fp16: 11 bits, normal down to H = 2^-27), from the format alone:
#   * f >= 18.  Every image entry carries a rounding of up to 2^-12 relative, 1.4e-4 rms -- above the bar.  The bar was stated
#     where these average out (test_bf16_pieces_match_oracle: f = 333); after this injection a column's product is carried by
#     one or a few entries, so about f independent roundings meet in the loss: 1.4e-4 / sqrt(f), a third of the bar from f = 18.
#     At f = 1 the case shows nothing at all: a row-normalised dictionary of one column is all ones before and after ANY
#     update (the stale image is the right one), the W rule then fits V exactly and the loss is 0 but for eps.
#   * k >= 15.  N = 2^U(-20, 20) leaves rows whose entries span 2^40 and more, the image's normal range ends 2^27 below the
#     row's sum: with ONE component a third to a half of the columns are below it and the format does not hold the dictionary;
#     with 15 and more a column has all its components there with a probability of 0.5^15 at the most.
# The shapes this leaves out of SHAPES (f = 1, 3 and k = 1) are held by the test behind this one, whose reference carries the
# image's rounding and range itself -- at f > 1, where there is something to see.
MASTER_SHAPES = [(f, k) for (f, k) in SHAPES if f >= 18 and k >= 15]


@pytest.mark.parametrize('shape', MASTER_SHAPES, ids=shape_id)
def test_the_next_row_pass_sees_the_injected_dictionary(shape):
    """'f16': behind the injected update of test 1 one more real row pass; the loss it leaves in loss[0] is the oracle's on (W
    before that pass, the injected H as read back) to the suite's bar for this evaluation, rtol 1e-4
    (test_bf16_pieces_match_oracle).  A stale or misplaced fp16 tile image or image row sum of the new dictionary fails this;
    the master alone would not show it.  Shapes: MASTER_SHAPES, and why, above.

    What the reference cannot see at the other shapes of test 1, measured on an MI355X (gpu = the pass's loss):
        shape        gpu              oracle on the master   relative   oracle on fp16(8192 H) / 8192   relative
        f1-k1        7.826826979e-09  4.780800666e-08        8.4e-01    (the same; f1-k15 .. f1-k200: 6.5e-03 .. 2.1e+00)
        f3-k17       1.148413923e+01  1.148094409e+01        2.8e-04    1.148299961e+01                 9.9e-05
        f3-k33       8.044624947e+00  8.043575382e+00        1.3e-04    8.044139744e+00                 6.0e-05
        f127-k1      5.123659414e+04  5.122762048e+04        1.8e-04    5.123678064e+04                 3.6e-06
        f128-k1      2.046836822e+05  2.047048234e+05        1.0e-04    2.046822838e+05                 6.8e-06
        f257-k1      1.044043609e+05  1.043458338e+05        5.6e-04    1.044041378e+05                 2.1e-06
        f1030-k1     1.596055745e+06  1.594554939e+06        9.4e-04    1.596042117e+06                 8.5e-06
        f4097-k1     1.489942621e+06  1.484866372e+06        3.4e-03    1.489930312e+06                 8.3e-06
    (k = 1: 34 .. 52 % of the columns below the image's normal range; the pass's loss IS the oracle's on the image.)"""
    f, k = shape
    H_before, N, H_after, loss, W = _loss_behind_the_injected_update(f, k)
    V = problem(rows_for(f, k), f, k)[0]
    ref = orc.kl_error(V, W, H_after)
    stale = orc.kl_error(V, W, H_before)
    assert abs(stale - ref) > 1e-2 * abs(ref), 'the injected update does not move the loss: the case shows nothing'
    _MEASURED.append('    %-40s %-7s %.2e  (bar %.0e)' % ('f16 %s' % shape_id(shape), 'loss', abs(loss - ref) / abs(ref), 1e-4))
    np.testing.assert_allclose(loss, ref, rtol=1e-4)


@pytest.mark.parametrize('shape', [s for s in SHAPES if s[0] > 1], ids=shape_id)
def test_the_next_row_pass_sees_the_image_of_the_injected_dictionary(shape):
    """The same loss against the oracle's on (W before that pass, fp16(8192 x injected H) / 8192): what k_post packs (post.hip.h:
    the row-normalised master x 1 / kOpScaleW, rounded to the fp16 operand type), to the same rtol 1e-4.  The image's rounding
    and range are then in the reference, and what remains is the pass itself -- on the image of THIS dictionary: the image of
    the dictionary before the update gives another loss altogether (asserted).  f = 1 is left out: its dictionary is all ones
    before and after, and its loss an exact fit's (MASTER_SHAPES, above)."""
    f, k = shape
    H_before, N, H_after, loss, W = _loss_behind_the_injected_update(f, k)
    V = problem(rows_for(f, k), f, k)[0]
    image = (H_after * 8192.0).astype(np.float16).astype(np.float64) / 8192.0
    ref = orc.kl_error(V, W, image)
    stale = orc.kl_error(V, W, H_before)
    assert abs(stale - ref) > 1e-2 * abs(ref), 'the injected update does not move the loss: the case shows nothing'
    _MEASURED.append('    %-40s %-7s %.2e  (bar %.0e)' % ('f16 %s image' % shape_id(shape), 'loss', abs(loss - ref) / abs(ref), 1e-4))
    np.testing.assert_allclose(loss, ref, rtol=1e-4)


# ---- 5. injected losses -> the stop rule --------------------------------------------------------------------------------------------
STOP_CAP, STOP_TOL, SCRIPTS = lp.STOP_CAP, lp.STOP_TOL, lp.SCRIPTS
STOP_SHAPE = (257, 17)
STOP_CASES = [(prec, parts) for prec in lp.PRECISIONS for parts in ((1, 2) if prec == 'f16' else (1,))]


def _scripted_run(prec, parts, script, steps):
    """`steps` iterations whose loss[0] is script[it] and whose numerator is a fresh 2^U(-2, 2) per iteration."""
    f, k = STOP_SHAPE
    V, H0 = problem(rows_for(f, k), f, k)
    ctx, xch = lp.open_context(prec, V, H0, k, STOP_CAP)
    with ctx:
        assert xch.nparts == parts
        rng = np.random.default_rng(77)
        numerators = [2.0 ** rng.uniform(-2.0, 2.0, (k, f)) for _ in range(STOP_CAP)]
        try:
            errors, n_done, stopped = lp.drive(ctx, steps, tol_abs=STOP_TOL, nparts=xch.nparts,
                                               after_rowpass=lambda it: xch.write_loss(script[it]),
                                               after_colpass=lambda it: xch.write_numerator(numerators[it]))
        except _native.NativeError as e:
            refused(ctx, e)
            return None
        return np.array(errors), n_done, stopped, ctx.get_W(), ctx.get_H()


@pytest.mark.parametrize('name', sorted(SCRIPTS))
@pytest.mark.parametrize('prec,parts', STOP_CASES, ids=['%s-P%d' % c for c in STOP_CASES])
def test_injected_losses_drive_the_stop_rule(monkeypatch, prec, parts, name):
    """Exact: n_done is `stop_rule`'s, the recorded errors are the injected doubles, the flag says whether the rule fired; and
    whole iterations enqueued behind the stop, with fresh numerators, change neither W nor H."""
    monkeypatch.setenv('KLNMF_COMM_PARTS', str(parts))
    script = SCRIPTS[name]
    want = lp.stop_rule(script, STOP_TOL)
    full = _scripted_run(prec, parts, script, STOP_CAP)
    if full is None:
        return
    errors, n_done, stopped, W, H = full
    assert n_done == want
    assert stopped == (want < STOP_CAP)
    assert errors.dtype == np.float64 and np.array_equal(errors, np.array(script[:want], dtype=np.float64))
    assert np.all(np.isfinite(W)) and np.all(np.isfinite(H))
    if want < STOP_CAP:
        # a run that ended at the stop: the iteration whose decision fired is its last
        e2, n2, s2, W2, H2 = _scripted_run(prec, parts, script, want + 1)
        assert (n2, s2) == (want, True) and np.array_equal(e2, errors)
        assert np.array_equal(W, W2) and np.array_equal(H, H2)
        # ... and the iterations before the stop did move both
        e3, n3, s3, W3, H3 = _scripted_run(prec, parts, script, want)
        assert (n3, s3) == (want, False)
        assert np.array_equal(W, W3) and np.array_equal(H, H3)
        if want > 1:
            e4, n4, s4, W4, H4 = _scripted_run(prec, parts, script, want - 1)
            assert n4 == want - 1 and not np.array_equal(W, W4) and not np.array_equal(H, H4)


# ---- 6. pieces equal the fused loop ---------------------------------------------------------------------------------------------------
# (precision, buffer) pairs whose fused launch sums in another order than the pieces' and may therefore differ, within rtol 1e-6
# (the bar test_torch_path_exchanges_the_numerator_in_parts states for that reason); everything else is bit for bit.  Measured on
# an MI355X: none -- every precision gives the same bits in losses, W and H at every shape below.
ORDER_DIFFERS = set()
FUSED_SHAPES = [(64, 129, 33), (300, 257, 17), (300, 1030, 200)]


@pytest.mark.parametrize('prec', lp.PRECISIONS)
@pytest.mark.parametrize('shape', FUSED_SHAPES, ids=lambda s: '%dx%dk%d' % s)
def test_pieces_equal_the_fused_loop(prec, shape):
    """3 iterations, nothing injected, via `run(3, True, NO_STOP)` and via `drive`: losses, W and H bit for bit -- except the pairs of
    ORDER_DIFFERS, which are held to rtol 1e-6 and reported.  Tests 1 to 5 certify the forms the pieces launch (k_post's POST_RULE,
    k_decide, the exact modes' H-rule kernels); this ties them to the fused form the benchmark runs."""
    n, f, k = shape
    V, H0 = problem(n, f, k)
    ctx, xch = lp.open_context(prec, V, H0, k, 3)
    with ctx:
        errors, n_done, stopped = ctx.run(3, True, lp.NO_STOP)
        fused = {'losses': np.array(errors), 'W': ctx.get_W(), 'H': ctx.get_H()}
        assert (n_done, stopped) == (3, False)
    ctx, xch = lp.open_context(prec, V, H0, k, 3)
    with ctx:
        try:
            errors, n_done, stopped = lp.drive(ctx, 3, nparts=xch.nparts)
        except _native.NativeError as e:
            refused(ctx, e)
            return
        pieces = {'losses': np.array(errors), 'W': ctx.get_W(), 'H': ctx.get_H()}
        assert (n_done, stopped) == (3, False)
    found = {}
    for name in ('losses', 'W', 'H'):
        a, b = pieces[name], fused[name]
        assert a.shape == b.shape and np.all(np.isfinite(a))
        found[name] = (np.array_equal(a, b), float(np.max(np.abs(a - b) / np.maximum(np.abs(b), np.finfo(np.float64).tiny))))
        _MEASURED.append('    %-40s %-7s %s' % ('%s %dx%dk%d' % ((prec,) + shape), name,
                                                'same bits' if found[name][0] else 'max rel %.2e' % found[name][1]))
    for name in ('losses', 'W', 'H'):
        a, b = pieces[name], fused[name]
        same, rel = found[name]
        if (prec, name) in ORDER_DIFFERS:
            np.testing.assert_allclose(a, b, rtol=1e-6, atol=0)
        else:
            assert same, '%s: %s differs from the fused loop in %d of %d elements (max rel %.3e)' % (prec, name, int((a != b).sum()), a.size, rel)


# ---- 7. the stop rule at prev - err == tol_abs on the loop's own losses, fused and in pieces -----------------------------------------
@pytest.mark.parametrize('route', ['fused', 'pieces'])
@pytest.mark.parametrize('prec', lp.PRECISIONS)
def test_stop_rule_at_the_boundary_on_real_losses(prec, route):
    """Test 5 reaches k_decide alone; the fused loop decides in the launch that reduces the loss (k_post in the 16-bit mode, the
    one-block reductions of the exact modes), on a loss nobody can inject.  But the loop is deterministic: a run without the rule
    gives the record e, and tol_abs = e[1] - e[2] is then met EXACTLY at the third comparison of a second run -- which must not
    stop there, while the next double above must.  Exact: n_done, the recorded doubles and the flag are `stop_rule`'s on e."""
    n, f, k = 300, 257, 17
    steps = 5
    V, H0 = problem(n, f, k)

    def run(tol_abs):
        ctx, xch = lp.open_context(prec, V, H0, k, steps)
        with ctx:
            if route == 'fused':
                errors, n_done, stopped = ctx.run(steps, True, tol_abs)
            else:
                errors, n_done, stopped = lp.drive(ctx, steps, tol_abs=tol_abs, nparts=xch.nparts)
            return np.array(errors), n_done, stopped
    try:
        free, n_done, stopped = run(lp.NO_STOP)
    except _native.NativeError as e:
        assert route == 'pieces' and e.code == _native.ERR_UNSUPP, e
        _MEASURED.append('    refused: %s' % e)
        return
    assert (n_done, stopped) == (steps, False) and np.all(np.isfinite(free))
    again = run(lp.NO_STOP)
    assert np.array_equal(again[0], free), 'two runs of one problem differ: the loop is not deterministic'
    at = free[1] - free[2]
    above = float(np.nextafter(at, np.inf))
    want_at, want_above = lp.stop_rule(free, at), lp.stop_rule(free, above)
    assert want_above == 2 < want_at, (free, at)             # the premise: only the boundary separates the two tolerances
    for tol_abs, want in ((at, want_at), (above, want_above)):
        errors, n_done, stopped = run(tol_abs)
        assert n_done == want, '%s %s: tol_abs = %r stopped after %d, the rule says %d' % (prec, route, tol_abs, n_done, want)
        assert stopped == (want < steps)
        assert np.array_equal(errors, free[:want])
