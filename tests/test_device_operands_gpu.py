"""The kernels that move device-resident operands in and out of a context (k_copy_2d, k_place_V and k_tile_V with row indices:
klnmf_set_H_device, klnmf_get_W_device, klnmf_upload_V_device[_rows[_dt]]) against their host twins, bit for bit.

One problem in 'f64', 'f32', 'bf16x3' (fp32 storage) and 'f16' (the 16-bit mode: tiled V, padded fp32 masters f_pad / KP,
1 / v_scale on the way out): n = 70, f = 300, k = 20, none a multiple of 32.  The dictionary is [20, 360] in device memory: four
modalities of 140, 60, 96 and 64 columns, of which the third, the first and the fourth are stacked -- so source offsets (200,
0, 296) differ from the destination columns (0, 96, 236) and an unselected modality lies between them; blocks are passed as
base + offset with ld = 360, as DeviceEvaluation._set_dictionary does.

  * set_H_device (f64 and f32 sources): get_H equals get_H after a host set_H of the stacked matrix and the source rounded
    once to the storage type; init_W and a 3-iteration transform then give the same losses, W and H, bit for bit -- also on a
    context that held a dictionary of 7.0 before (no padding of the old dictionary survives in the 16-bit images).  In the
    16-bit mode the losses of two CONTEXTS agree within 2^-40 sum(V) only (each context's sum of V comes from its own
    atomicAdds, below); the same context given the dictionary by set_H and then by set_H_device repeats every bit of them.
  * get_W_device after that run into a NaN-filled [n + 2, k + 5] tensor in f64 and f32: [:n, :k] is get_W() (rounded once for
    f32; 1 / v_scale is a power of two), everything else still NaN.
  * uploads from a [90, 307] device matrix (row stride > columns used), f32 and f64 sources, 70 rows placed as 37 + 33 through
    a permutation, a list with repeats and a decreasing list (and contiguous rows for the two forms without an index list),
    three column blocks with a scale each.  The twin: a context given the same matrix, gathered and scaled in numpy, by ONE
    host upload_V.  Exact and split modes: with constant W and H (W.H = 2.5 exactly), step_Q / get_Q exposes every element of
    V at its position -- bit-identical to the twin's and within the step bar of tests/test_exact_gpu.py of the numpy value;
    error() bit-identical.  16-bit mode: after init_W and a 2-iteration fit W and H bit-identical to the twin's; every loss
    within 2^-40 sum(V) (k_tile_V adds at most 8192 block partials by atomicAdd in no fixed order, the two contexts in
    different blocks: 8192 . 2^-53; the storage-rounding corrections in the loss are such sums); KLNMF_QF_NNZ_V equal.
    KLNMF_QF_SUM_V turned out bit-identical and is asserted so, and equal to the numpy sum of the fp16-rounded matrix: on
    this data every partial sum of the stored values is exact in fp64 (the test checks the premise).  reset_V and the same
    uploads again: the same bits (the counters were cleared).
  * refusals (column block beyond f, ld < ncols, ld < k, an upload block beyond n or f, null pointers): each raises and the
    context then takes the valid call and gives the right bits.
Measured on the MI355X: Q against the numpy value 0 (f64; bar 1e-12), 8.3e-8 (f32; bar 3e-5) and 8.3e-8 (bf16x3; bar 2 . 2^-14);
the 16-bit mode's losses differed from the twin's by 0 in every case, so did those of two contexts in the dictionary test.
They stay at 2^-40 sum(V): the corrections they contain are inexact sums in an order that is not fixed.  Printed after each
test (pytest -v).
"""
import math

import numpy as np
import pytest

from multimodal_amd import _native
from tests import exact_cases as ec
from tests import test_exact_gpu as teg
from tests.test_sparse_gpu import _MEASURED, _report_measured, check, worst_rel  # noqa: F401  (the autouse fixture prints what was measured)

pytestmark = pytest.mark.gpu

PRECISIONS = ['f64', 'f32', 'bf16x3', 'f16']
N, F, K = 70, 300, 20
DICT_WIDTHS = (140, 60, 96, 64)                 # the dictionary's modalities in source order: [20, 360]
DICT_F = sum(DICT_WIDTHS)
SELECTED = (2, 0, 3)                            # stacked in this order: 96 + 140 + 64 = f
WIDTHS = tuple(DICT_WIDTHS[m] for m in SELECTED)
SRC_OFF = tuple(sum(DICT_WIDTHS[:m]) for m in SELECTED)
COL0 = (0, 96, 236)
SRC_ROWS, SRC_LD = 90, 307                      # the data source: [90, 307], 300 columns used
V_SRC_COL = (204, 0, 140)                       # where each destination block's columns start in the source
SCALES = (0.37, 1.3, 2.9)
PARTS = ((0, 37), (37, 33))                     # (row0, rows) of the two calls per block
SUM_BAR = 2.0 ** -40
assert sum(WIDTHS) == F and COL0 == (0, WIDTHS[0], WIDTHS[0] + WIDTHS[1]) and SRC_OFF == (200, 0, 296)
assert all(c + w <= 300 for c, w in zip(V_SRC_COL, WIDTHS)) and sorted(V_SRC_COL) != list(V_SRC_COL)


def torch_mod():
    import torch
    return torch


def storage(prec, a):
    """`a` rounded once to what the mode stores W, H and V masters in, widened to fp64."""
    return np.asarray(a, dtype=np.float64) if prec == 'f64' else ec.as_f32(a)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def data_source(seed=31):
    """[90, 307] nonnegative with zeros (about 20 %), fp32-representable so that f32 and f64 sources hold the same values."""
    rng = np.random.default_rng(seed)
    S = (rng.gamma(1.0, 1.0, (SRC_ROWS, SRC_LD)) + 0.05) * (rng.random((SRC_ROWS, SRC_LD)) >= 0.2)
    return ec.as_f32(S)


def assembled(S, idx):
    """The matrix the uploads build, in numpy: V[i, col0_b + j] = scale_b * S[idx[i], src_col_b + j] (one fp64 product each)."""
    V = np.empty((N, F))
    for c0, w, scale, s0 in zip(COL0, WIDTHS, SCALES, V_SRC_COL):
        V[:, c0:c0 + w] = scale * S[idx][:, s0:s0 + w]
    return V


def dictionary(seed=17):
    rng = np.random.default_rng(seed)
    D = rng.random((K, DICT_F)) + 0.05
    D /= stacked(D).sum(axis=1, keepdims=True)   # the stacked dictionary's rows sum to 1, as a fitted one's do
    D[:, 140:200] = 1e3                          # the unselected modality: nothing of it may arrive
    return D


def stacked(D):
    return np.ascontiguousarray(np.hstack([D[:, o:o + w] for o, w in zip(SRC_OFF, WIDTHS)]))


def fixed_V():
    """The matrix of the dictionary tests."""
    return ec.data(N, F, seed=5, zero_row=N // 2, zero_col=F // 3)


def open_ctx(prec, V=None, cap=4):
    ctx = _native.Context(prec)
    ctx.set_problem(N, F, K, cap)
    if V is not None:
        ctx.set_v_max(float(V.max()))
        ctx.upload_V(V)
    return ctx


def set_dictionary_device(ctx, dev_D, f64):
    es = 8 if f64 else 4
    for b, (o, w, c0) in enumerate(zip(SRC_OFF, WIDTHS, COL0)):
        ctx.set_H_device(dev_D.data_ptr() + es * o, f64, DICT_F, c0, w, last=(b == len(WIDTHS) - 1))


def transform(ctx, iters=3):
    ctx.init_W()
    errors, n_done, _ = ctx.run(iters, False, ec.NO_STOP)
    assert n_done == iters
    return np.array(errors), ctx.get_W(), ctx.get_H()


@pytest.mark.parametrize('src_f64', [True, False], ids=['src_f64', 'src_f32'])
@pytest.mark.parametrize('prec', PRECISIONS)
def test_set_H_device_and_get_W_device_equal_the_host_calls(prec, src_f64):
    torch = torch_mod()
    V = fixed_V()
    D = dictionary().astype(np.float64 if src_f64 else np.float32)
    Hs = stacked(D)                                # in the source's type: the host twin rounds from the same values
    dev_D = torch.from_numpy(D).to('cuda')
    torch.cuda.synchronize()
    with open_ctx(prec, V) as host, open_ctx(prec, V) as dev, open_ctx(prec, V) as used:
        host.set_H(Hs)
        want_H = host.get_H()
        assert same_bits(want_H, storage(prec, Hs)), 'host set_H does not round once'
        set_dictionary_device(dev, dev_D, src_f64)
        assert same_bits(dev.get_H(), want_H), 'set_H_device differs from set_H'
        used.set_H(np.full((K, F), 7.0))
        set_dictionary_device(used, dev_D, src_f64)
        assert same_bits(used.get_H(), want_H), 'set_H_device over an earlier dictionary differs from set_H'
        want = transform(host)
        assert np.all(np.isfinite(want[0])) and np.all(want[1] >= 0) and want[1].max() > 0
        for name, ctx in (('a fresh context', dev), ('a context that held another dictionary', used)):
            got = transform(ctx)
            for what, g, w in zip(('losses', 'W', 'H'), got, want):
                if prec == 'f16' and what == 'losses':       # the contexts' sums of V come from atomicAdds of their own
                    assert np.all(np.abs(g - w) <= SUM_BAR * float(V.sum())), '%s: losses %r against %r' % (name, g, w)
                    _MEASURED.append('    %-60s losses %.2e of 2^-40 sum(V)' % (name, float(np.max(np.abs(g - w))) / (SUM_BAR * float(V.sum()))))
                    continue
                assert same_bits(g, w), '%s: %s of the transform differ from the host dictionary\'s' % (name, what)
        # ... and on ONE context (one sum of V), the device dictionary behind the host one: every bit, the losses too
        set_dictionary_device(host, dev_D, src_f64)
        for what, g, w in zip(('losses', 'W', 'H'), transform(host), want):
            assert same_bits(g, w), 'the same context: %s of the transform differ after set_H_device' % what

        # ---- get_W_device after that run
        W = dev.get_W()
        for f64 in (True, False):
            out = torch.full((N + 2, K + 5), float('nan'), dtype=torch.float64 if f64 else torch.float32, device='cuda')
            torch.cuda.synchronize()
            dev.get_W_device(out.data_ptr(), f64, K + 5)
            got = out.cpu().numpy()
            assert same_bits(got[:N, :K], W if f64 else W.astype(np.float32)), 'get_W_device (%s) differs from get_W' % got.dtype
            assert np.isnan(got[:N, K:]).all() and np.isnan(got[N:]).all(), 'get_W_device wrote beyond [n, k]'
        assert same_bits(dev.get_W(np.float32), W.astype(np.float32))


# ---- V uploads ------------------------------------------------------------------------------------------------------------------
def row_lists():
    rng = np.random.default_rng(8)
    rep = rng.integers(0, SRC_ROWS, N)
    rep[[1, 2, 40]] = rep[0]                                   # a row in both parts, twice in the first
    return {'a permutation': rng.permutation(SRC_ROWS)[:N].astype(np.int64),
            'repeats': rep.astype(np.int64),
            'decreasing': np.arange(SRC_ROWS - 1, SRC_ROWS - 1 - N, -1, dtype=np.int64)}


CONTIGUOUS = np.concatenate([np.arange(5, 5 + 37), np.arange(50, 50 + 33)]).astype(np.int64)     # the forms without an index list
APIS = ('device', 'rows', 'rows_dt f32', 'rows_dt f64', 'rows_dt f64 no index')


def do_uploads(ctx, api, src, idx_host, idx_dev):
    """The six calls (3 column blocks x 2 row parts) of one upload of the assembled matrix; the context's stream is drained."""
    f64 = src.dtype == torch_mod().float64
    es = src.element_size()
    for c0, w, scale, s0 in zip(COL0, WIDTHS, SCALES, V_SRC_COL):
        for row0, rows in PARTS:
            if api in ('device', 'rows_dt f64 no index'):       # contiguous source rows from idx_host[row0] on
                ptr = src.data_ptr() + es * (int(idx_host[row0]) * SRC_LD + s0)
                assert int(idx_host[row0]) + rows <= SRC_ROWS
                if api == 'device':
                    ctx.upload_V_device(ptr, rows, w, SRC_LD, row0=row0, col0=c0, scale=scale)
                else:
                    ctx.upload_V_device_rows_dt(ptr, f64, 0, rows, w, SRC_LD, row0=row0, col0=c0, scale=scale)
                continue
            ptr, ip = src.data_ptr() + es * s0, idx_dev.data_ptr() + 8 * row0
            if api == 'rows':
                ctx.upload_V_device_rows(ptr, ip, rows, w, SRC_LD, row0=row0, col0=c0, scale=scale)
            else:
                ctx.upload_V_device_rows_dt(ptr, f64, ip, rows, w, SRC_LD, row0=row0, col0=c0, scale=scale)
    ctx.synchronize()


def expose_V(ctx):
    """(Q, loss) with W.H = 2.5 everywhere: Q = (V + eps) / (2.5 + eps) element by element."""
    ctx.set_W(np.full((N, K), 0.5))
    ctx.set_H(np.full((K, F), 0.25))
    ctx.step_Q()
    return ctx.get_Q(), ctx.error()


def fit16(ctx, H0):
    ctx.set_H(H0)
    ctx.init_W()
    errors, n_done, _ = ctx.run(2, True, ec.NO_STOP)
    assert n_done == 2
    return np.array(errors), ctx.get_W(), ctx.get_H(), ctx.sum_V(), ctx.nnz_V()


@pytest.mark.parametrize('api', APIS)
@pytest.mark.parametrize('prec', PRECISIONS)
def test_device_uploads_equal_one_host_upload_of_the_assembled_matrix(prec, api):
    torch = torch_mod()
    S = data_source()
    f64src = api.startswith('rows_dt f64')
    src = torch.from_numpy(S.astype(np.float64 if f64src else np.float32)).to('cuda')
    assert src.stride(0) == SRC_LD > F
    lists = {'contiguous rows': CONTIGUOUS} if api in ('device', 'rows_dt f64 no index') else row_lists()
    H0 = ec.factors(N, F, K, seed=3)[1]
    for name, idx in sorted(lists.items()):
        case = '%s %s, %s' % (prec, api, name)
        assert idx.shape == (N,) and idx.min() >= 0 and idx.max() < SRC_ROWS
        idx_dev = torch.from_numpy(idx).to('cuda')
        torch.cuda.synchronize()
        V = assembled(S, idx)
        vmax = float(V.max())
        with open_ctx(prec) as ctx, open_ctx(prec) as twin:
            twin.set_v_max(vmax)
            twin.upload_V(V)
            ctx.set_v_max(vmax)
            do_uploads(ctx, api, src, idx, idx_dev)
            if prec != 'f16':
                Q, loss = expose_V(ctx)
                Qt, loss_t = expose_V(twin)
                assert same_bits(Q, Qt), case + ': the uploaded matrix differs from the twin\'s'
                assert loss == loss_t, case
                Vs = storage(prec, V)
                check(case, 'Q', Q, (Vs + ec.orc.EPS_RATIO) / (2.5 + ec.orc.EPS_RATIO), teg.step_bars(prec, K)['Q'], teg.FLOOR[prec])
                ctx.reset_V()
                do_uploads(ctx, api, src, idx, idx_dev)
                Q2, loss2 = expose_V(ctx)
                assert same_bits(Q2, Q) and loss2 == loss, case + ': after reset_V'
                continue
            bar = SUM_BAR * float(V.sum())
            # V as stored: c V in fp16, c = 2^(15 - e) from vmax = m 2^e (klnmf_set_v_max).  Here every stored value is 0 or at
            # least 1, so a multiple of 2^-10, and their sum is below 2^43: every partial sum is exact in fp64, in any order --
            # KLNMF_QF_SUM_V is the numpy sum to the bit, whatever order the atomicAdds took
            c = 2.0 ** (15 - math.frexp(vmax)[1])
            stored = (V * c).astype(np.float16).astype(np.float64)
            assert stored[stored > 0].min() >= 1.0 and stored.sum() < 2.0 ** 43 and np.count_nonzero(stored) == np.count_nonzero(V)
            want = fit16(twin, H0)
            for again in (False, True):
                if again:
                    ctx.reset_V()
                    do_uploads(ctx, api, src, idx, idx_dev)
                got = fit16(ctx, H0)
                tag = case + (': after reset_V' if again else '')
                assert same_bits(got[1], want[1]) and same_bits(got[2], want[2]), tag + ': W or H differ from the twin\'s'
                assert got[4] == want[4], tag + ': entries > 0 as stored'
                assert got[3] == want[3] == float(stored.sum()) / c, tag + ': sum of V %r against %r' % (got[3], want[3])
                assert np.all(np.abs(got[0] - want[0]) <= bar), tag + ': losses %r against %r' % (got[0], want[0])
                _MEASURED.append('    %-60s losses %.2e of 2^-40 sum(V)' % (tag, float(np.max(np.abs(got[0] - want[0]))) / bar))
            assert want[4] == float(np.count_nonzero(stored)), case + ': entries > 0 as stored'


# ---- refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', PRECISIONS)
def test_refused_device_operands_leave_the_context_usable(prec):
    torch = torch_mod()
    S = data_source()
    src = torch.from_numpy(S.astype(np.float32)).to('cuda')
    idx = row_lists()['a permutation']
    idx_dev = torch.from_numpy(idx).to('cuda')
    D = dictionary()
    dev_D = torch.from_numpy(D).to('cuda')
    out = torch.full((N, K), float('nan'), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    V = assembled(S, idx)
    with open_ctx(prec) as ctx, open_ctx(prec, V) as twin:
        ctx.set_v_max(float(V.max()))
        p, ip, dp = src.data_ptr(), idx_dev.data_ptr(), dev_D.data_ptr()
        refused = [
            lambda: ctx.set_H_device(dp, True, DICT_F, F - 63, 64),            # col0 + ncols > f
            lambda: ctx.set_H_device(dp, True, DICT_F, -1, 64),
            lambda: ctx.set_H_device(dp, True, 63, 0, 64),                     # ld < ncols
            lambda: ctx.set_H_device(0, True, DICT_F, 0, 64),
            lambda: _native._check(ctx._lib.klnmf_set_H_device(ctx._h, dp, 7, DICT_F, 0, 64, 1)),     # an unknown dtype code
            lambda: ctx.get_W_device(out.data_ptr(), True, K - 1),             # ld < k
            lambda: ctx.get_W_device(0, True, K),
            lambda: ctx.upload_V_device(p, N + 1, 96, SRC_LD),                 # beyond n
            lambda: ctx.upload_V_device(p, 37, 96, SRC_LD, row0=N - 36),
            lambda: ctx.upload_V_device(p, 37, 96, SRC_LD, col0=F - 95),       # beyond f
            lambda: ctx.upload_V_device(p, 37, 96, 95),                        # ld < cols
            lambda: ctx.upload_V_device(0, 37, 96, SRC_LD),
            lambda: ctx.upload_V_device_rows(p, ip, 37, 96, SRC_LD, row0=N - 36),
            lambda: ctx.upload_V_device_rows(p, 0, 37, 96, SRC_LD),
            lambda: ctx.upload_V_device_rows(0, ip, 37, 96, SRC_LD),
            lambda: ctx.upload_V_device_rows_dt(p, False, ip, 37, 96, SRC_LD, col0=F - 95),
            lambda: ctx.upload_V_device_rows_dt(p, False, ip, -1, 96, SRC_LD),
            lambda: ctx.upload_V_device_rows_dt(0, False, ip, 37, 96, SRC_LD),
        ]
        for n, call in enumerate(refused):
            with pytest.raises(_native.NativeError) as err:
                call()
            assert err.value.code == _native.ERR_ARG, n
        assert np.isnan(out.cpu().numpy()).all()
        # the same context takes the valid calls and gives the twin's bits
        do_uploads(ctx, 'rows_dt f32', src, idx, idx_dev)
        Hs = stacked(D)
        twin.set_H(Hs)
        set_dictionary_device(ctx, dev_D, True)
        assert same_bits(ctx.get_H(), twin.get_H())
        want, got = transform(twin, 2), transform(ctx, 2)
        assert same_bits(got[1], want[1]) and same_bits(got[2], want[2])
        if prec == 'f16':
            assert np.all(np.abs(got[0] - want[0]) <= SUM_BAR * float(V.sum()))
        else:
            assert same_bits(got[0], want[0])
        ctx.get_W_device(out.data_ptr(), True, K)
        assert same_bits(out.cpu().numpy(), want[1])
