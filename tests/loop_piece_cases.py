"""Helpers of the loop-piece tests (tests/test_loop_pieces_cpu.py, tests/test_loop_pieces_gpu.py).  Importing needs no GPU.

The pieces of an iteration (include/klnmf.h: klnmf_iter_*) exchange two buffers with the caller: the H-rule numerator
W_new^T.Q and two loss doubles (klnmf_bind_exchange / klnmf_exchange_buffers / _layout / _parts).  A row-sharded loop sums
them over the ranks between `iter_colpass` and `iter_decide` (multimodal_amd/distributed.py, ShardedKLNMF.iterate); the tests
WRITE them there instead and so choose the inputs of the two pieces whose arithmetic has an exact specification:

  stop rule   stop iff prev - err < tol_abs, else record err                                             (nmf.py:214-220)
  H rule      H_new[c, j] = H_old[c, j] * N[c, j] / (kEpsNorm + sum_j H_old[c, j] * N[c, j]),  j < f     (nmf.py:349-350)

Layouts.  A `Layout` says where the [k, f] numerator lives in the flat exchange buffer: `count` elements in all, and per column
part (offset, row stride, first column, valid columns).  The whole-matrix layout is one part at offset 0 whose row stride is
what `exchange_layout()` reports; the split layout has one part per entry of `exchange_parts()`, whose element count is
k x row stride.  Everything outside the parts' [k, ncols] blocks is padding: the rest of a row stride, columns beyond a part's
ncols, component rows >= k.
"""
import collections

import numpy as np

# kEpsNorm of multimodal_amd/csrc/common.hip.h (line `constexpr double kEpsNorm = 1.0e-16;`), which is the reference's
# normalize_sum default (array_utils.py:19) and oracle.klnmf_oracle.EPS_NORMALIZE; tests/test_loop_pieces_cpu.py reads the
# header and holds the three to each other
K_EPS_NORM = 1.0e-16

NO_STOP = -1e300              # a tolerance the stop rule never meets (tests/exact_cases.py)
PAD = 3e30                    # what the tests leave in every element of the exchange buffer that is not the numerator
PRECISIONS = ['f16', 'bf16x3', 'f16x3', 'f32', 'f64']

# |got - ref| <= bar x |ref| per element of the H rule.  Masters in fp32: the product is one rounding (2^-24), the fp64 row sum of
# the rounded products inherits at most that much, its conversion to the fp32 divisor is one rounding, a non-IEEE fp32
# division at most 2.5 ulp -- 4.5 x 2^-24 and a little; the bar is 8 x 2^-24.  'f64': tests/test_exact_gpu.py's one-step bar.
BAR_F32 = 8 * 2.0 ** -24


def h_bar(prec, f):
    return 8 * 2.0 ** -53 * (1 + f * 2.0 ** -3) if prec == 'f64' else BAR_F32


def ref_h_rule(H_old, N, f):
    """The H rule in fp64 from the values as given (fp32 values: converted, not re-rounded), columns j < f."""
    H_old = np.asarray(H_old, dtype=np.float64)[:, :f]
    N = np.asarray(N, dtype=np.float64)[:, :f]
    P = H_old * N
    return P / (K_EPS_NORM + P.sum(axis=1, keepdims=True))


def stop_rule(losses, tol_abs):
    """n_done of nmf.py:214-220 on a loss record computed without the rule; len(losses) if it never fires."""
    prev = np.inf
    for i, e in enumerate(losses):
        if prev - e < tol_abs:
            return i
        prev = e
    return len(losses)


# ---- loss scripts of the stop-rule test: STOP_CAP injected losses each, tol_abs = STOP_TOL ------------------------------------------
STOP_CAP, STOP_TOL = 12, 1.0
BELOW_ONE = float(np.nextafter(1.0, 0.0))


def _fill(head, step=2.0):
    """`head`, then steadily decreasing by `step` to STOP_CAP entries."""
    out = list(head)
    while len(out) < STOP_CAP:
        out.append(out[-1] - step)
    return out


SCRIPTS = {
    'decreasing': _fill([100.0]),                               # never stops
    'step-equals-tol': _fill([9.0, 7.0, 6.0]),                  # 7 - 6 == tol_abs: must NOT stop
    'step-just-below-tol': _fill([5.0, 3.0, 1.0, 2.0 ** -53]),  # 1 - 2^-53 == nextafter(1, 0) < tol_abs: stops there
    'increase': _fill([50.0, 48.0, 49.0]),                      # stops at the increase
    'inf-first': _fill([np.inf, 40.0, 38.0, 37.5]),             # inf - inf is NaN, inf - 40 is inf: neither stops; 38 - 37.5 does
    'second-comparison': _fill([1e308, 1e308]),                 # the first comparison cannot stop (prev = inf); the second does
}
SCRIPT_DONE = {'decreasing': 12, 'step-equals-tol': 12, 'step-just-below-tol': 3, 'increase': 2, 'inf-first': 3, 'second-comparison': 1}

# ---- layouts ----------------------------------------------------------------------------------------------------------------
Part = collections.namedtuple('Part', 'offset stride col0 ncols')
Layout = collections.namedtuple('Layout', 'count k f parts')


def whole_layout(count, k, f, stride):
    """The layout `exchange_layout()` describes: component rows `stride` apart from element 0, `count` = `exchange_buffers()`'s."""
    return Layout(int(count), int(k), int(f), (Part(0, int(stride), 0, int(f)),))


def parts_layout(count, k, f, parts):
    """The layout `exchange_parts()` describes: (offset, element count = k x row stride, first column, columns) per part."""
    out = []
    for off, cnt, col0, ncols in parts:
        assert cnt % k == 0, (cnt, k)
        out.append(Part(int(off), int(cnt) // int(k), int(col0), int(ncols)))
    return Layout(int(count), int(k), int(f), tuple(out))


def _index(layout):
    """Flat index of every numerator element, [k, f]; every column belongs to exactly one part."""
    idx = np.full((layout.k, layout.f), -1, dtype=np.int64)
    rows = np.arange(layout.k, dtype=np.int64)[:, None]
    for p in layout.parts:
        assert 0 <= p.col0 and p.col0 + p.ncols <= layout.f and p.ncols <= p.stride, p
        assert np.all(idx[:, p.col0:p.col0 + p.ncols] == -1), 'parts overlap in columns'
        idx[:, p.col0:p.col0 + p.ncols] = p.offset + rows * p.stride + np.arange(p.ncols, dtype=np.int64)[None, :]
    assert np.all(idx >= 0), 'columns without a part'
    assert np.all(idx < layout.count), 'a part leaves the buffer'
    assert len(np.unique(idx)) == idx.size, 'parts overlap in the buffer'
    return idx


def valid_mask(layout):
    """bool[count]: the elements of the flat buffer that hold the numerator."""
    mask = np.zeros(layout.count, dtype=bool)
    mask[_index(layout).ravel()] = True
    return mask


def place(layout, N, pad=PAD, dtype=np.float32):
    """The flat exchange buffer that holds N[k, f] under `layout`, `pad` in every other element."""
    N = np.asarray(N)
    assert N.shape == (layout.k, layout.f), (N.shape, layout.k, layout.f)
    flat = np.full(layout.count, pad, dtype=dtype)
    flat[_index(layout).ravel()] = N.astype(dtype).ravel()
    return flat


def unplace(layout, flat):
    """N[k, f] back from the flat buffer."""
    flat = np.asarray(flat)
    assert flat.shape == (layout.count,), (flat.shape, layout.count)
    return flat[_index(layout)]


# ---- a context with torch-owned exchange buffers -----------------------------------------------------------------------------
class Exchange(object):
    """The two exchange buffers of `ctx` as torch tensors (fp64 numerator iff `exchange_buffers()` says so), bound with
    `bind_exchange`, and the numerator's layout.

    Ordering.  The context runs on torch's current stream (`open_context`), as ShardedKLNMF's does: a `copy_` into these tensors
    is enqueued on that stream behind the pieces already enqueued and in front of the next ones, and a read (`.cpu()`)
    synchronises with it.  The tensors must outlive the context's use of them: keep this object until the context is closed."""

    def __init__(self, ctx):
        import torch
        self.torch = torch
        _, _, count, is64 = ctx.exchange_buffers()
        dev = torch.device('cuda', torch.cuda.current_device())
        self.np_dtype = np.float64 if is64 else np.float32
        self.numer_t = torch.zeros(count, dtype=torch.float64 if is64 else torch.float32, device=dev)
        self.loss_t = torch.zeros(2, dtype=torch.float64, device=dev)
        ctx.bind_exchange(self.loss_t.data_ptr(), self.numer_t.data_ptr())
        self.raw_parts = ctx.exchange_parts()
        if len(self.raw_parts) > 1:
            self.layout = parts_layout(count, ctx.k, ctx.f, self.raw_parts)
        else:
            stride, valid = ctx.exchange_layout()
            assert valid == ctx.k * stride and valid <= count, (stride, valid, count)
            self.layout = whole_layout(count, ctx.k, ctx.f, stride)
        self.nparts = len(self.raw_parts)

    def rounded(self, N):
        """N as the buffer's number format holds it, in fp64."""
        return np.asarray(N, dtype=self.np_dtype).astype(np.float64)

    def write_numerator(self, N, pad=PAD):
        self.numer_t.copy_(self.torch.from_numpy(place(self.layout, N, pad=pad, dtype=self.np_dtype)))

    def read_numerator(self):
        return unplace(self.layout, self.numer_t.cpu().numpy())

    def write_loss(self, value, index=0):
        self.loss_t[index:index + 1].copy_(self.torch.tensor([float(value)], dtype=self.torch.float64))

    def read_loss(self):
        return self.loss_t.cpu().numpy().copy()


def open_context(prec, V, H0, k, cap):
    """(ctx, Exchange): a context on torch's current stream with V uploaded, H = H0, W = W0 = V.H0^T and torch-owned exchange buffers."""
    import torch
    from multimodal_amd import _native
    dev = torch.cuda.current_device()
    ctx = _native.Context(prec, device=dev, stream=torch.cuda.current_stream(dev).cuda_stream)
    try:
        ctx.set_problem(V.shape[0], V.shape[1], k, cap)
        xch = Exchange(ctx)
        if ctx.exact:
            ctx.upload_V(V)
        else:
            ctx.upload_blocks([V])
        ctx.set_H(H0)
        ctx.init_W()
    except Exception:
        ctx.close()
        raise
    return ctx, xch


def drive(ctx, steps, tol_abs=NO_STOP, after_rowpass=None, after_colpass=None, nparts=1, end=True):
    """`steps` fit iterations in pieces, sequenced as ShardedKLNMF.iterate (collective='torch') sequences them:

        iter_rowpass | [after_rowpass(it): where the loss all-reduce sits -- loss[0]]
        iter_colpass, or iter_colpass_part(p) for every part | [after_colpass(it): where the numerator's and loss[1]'s sit]
        iter_decide | iter_update_H | iter_advance

    between `loop_begin` and `loop_end`.  Returns loop_end's (errors, n_done, stopped); end=False: the loop is left open (None)."""
    ctx.loop_begin()
    for it in range(steps):
        ctx.iter_rowpass(True)
        if after_rowpass is not None:
            after_rowpass(it)
        if nparts > 1:
            for p in range(nparts):
                ctx.iter_colpass_part(p)
        else:
            ctx.iter_colpass()
        if after_colpass is not None:
            after_colpass(it)
        ctx.iter_decide(tol_abs)
        ctx.iter_update_H()
        ctx.iter_advance()
    return ctx.loop_end(max(1, steps)) if end else None
