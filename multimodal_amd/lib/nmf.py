"""KL-divergence (I-divergence) NMF on MI355X -- host side.

Same public surface as reference multimodal/lib/nmf.py (`KLdivNMF`, `_scale`,
`_special_sparse_dot`, `check_non_negative`), so `multimodal/learner.py`,
`experiment.py` and the sample scripts can use it unchanged.  All arithmetic of
the path -- W0 = X.H0^T, the loss, the ratio Q, the W and H rules, the row
normalisation and the stop rule of the loop -- runs in the HIP kernels of
`csrc/` through the C-ABI of `include/klnmf.h`.  This module only validates
input (the reference's ValueErrors are raised before anything is uploaded),
moves arrays, and keeps the reference's object protocol (`components_`,
`_init_dictionary`, `return_errors`, the stderr warning).

There is no CPU implementation behind these calls: without the HIP extension or
a gfx950 device they raise.

Behaviour kept on purpose: `scale_W` passed to
fit/fit_transform/transform is accepted and ignored (q1, nmf.py:222); the H
rule pairs the ratio of the OLD W with the NEW W (q2, nmf.py:251-256, done that
way inside the kernels); the random initial dictionary comes from the global
`np.random` stream (q3, nmf.py:150); the loop's eps is the hard-coded 1e-8 (q4);
the loss is recorded before each update and the breaking iteration's loss is not
appended (q5, nmf.py:214-220).

Extra (non-reference) constructor arguments: `precision` ('f64' default =
the reference's float64 arithmetic; 'f32'; 'bf16x3' = the f32 mode with its contractions on the bf16 matrix cores, every
fp32 operand split into two bf16 parts (hi.hi + hi.lo + lo.hi, fp32 accumulation: each product within ~2^-16 of a.b; any
shape, any k, any eps); 'f16x3' = the same with fp16 operand parts under power-of-two scales and, for k <= 256, the
loop's passes fused (k > 256: 'bf16x3'); 'f16' (= 'bf16') = MFMA fast path with V stored as power-of-two-scaled fp16; 'auto'), `device` (a GPU index, or a
list of them: the dense loop then runs over row shards, one context per entry -- `_fit_group`; CSR input too, above
`CSR_SHARD_MIN_NNZ` stored entries per shard -- `_fit_group_csr`).  Environment: KLNMF_PRECISION,
KLNMF_DEVICES (a comma-separated list, the default `device`), KLNMF_DEVICE.
"""
import copy
import os
import sys

import numpy as np
import scipy.sparse as sp

from .array_utils import normalize_sum
from .sklearn_utils import atleast2d_or_csr
from .. import _native


def _default_precision():
    return os.environ.get('KLNMF_PRECISION', 'f64')


# precision='auto' (KLNMF_PRECISION=auto): the reference's own arithmetic (f64: results equal to the reference's) where a
# fit is cheap anyway, the fp16-operand MFMA path (final KL within 1e-4) from this many multiply-adds per W.H on -- 2e9 is
# 10 000 x 4096 at k = 50: below it an f64 iteration is well under a millisecond.  The default stays 'f64' (SURVEY section 5:
# defaults must reproduce the reference's results).
AUTO_F16_WORK = 2e9
# ... and only on shapes inside the 16-bit mode's accuracy envelope: its rounding noise averages out over the columns (W rule), the
# rows (H rule) and the components (W.H), and with few of either the averaging is weak -- measured against the oracle (round 5,
# profiles/r05_monitor_calibration.txt): f = 8 ends 2.4e-4 off, f = 64 is up to 4.5e-4 off in mid-descent, k <= 8 on low-noise data
# up to 8e-4 after 150 iterations; from f = 256 and k = 16 on every class stays within 1e-4.  Smaller shapes run in fp32 (1e-6).
AUTO_F16_MIN_F = 256
AUTO_F16_MIN_K = 16


# ... and on the data: a fit whose final KL / sum(V) falls below this has so little residual left that the f16 operands' own
# rounding noise (about 3e-4 / sqrt(terms) per product) can pass 1e-4 of the loss (measured: low-noise rank-8 data, 160 000 rows,
# 150 iterations: 8e-4, at KL / sum(V) = 4e-4; the reference's fixtures G18 / G19 sit at 5.5e-4 and 2.9e-3; the BASELINE
# configurations' data at 4.8e-3 .. 9.5e-3).  The library reports the ratio of every loop (klnmf_query_f64
# KLNMF_QF_KL_OVER_SUM_V); `KLdivNMF.last_fp8_report['outside_f16_envelope']` and one stderr line say when a fit ended below it.
F16_MIN_KL_OVER_SUM_V = 3e-3

MAX_K_F16X3 = 256         # the fused split-fp16 loop of 'f16x3' holds a workgroup's Q.H^T of all components in registers
MAX_K_MFMA = 512          # the 16-bit MFMA kernels hold a wave's accumulators of all components in registers: k <= 512
MAX_ROWS_EXACT = 65535 * 64   # the exact modes' row tiles ride on gridDim.y (csrc/plan.hip.h: KLNMF_ERR_UNSUPP beyond)

# CSR input on a device list runs over row shards (`_fit_group_csr`) when every shard holds at least this many stored entries;
# below, on the list's first device.  At the measured fp64 rate of the sparse loop (about 8.5 G entries/s: README) 2^20 entries
# are about 0.12 ms of a shard's work per iteration; the group's own cost, measured on one GPU at the bench shape, is 0.02 - 0.04 ms
# per shard and iteration (N = 2, 4: profiles/csr_shards_group.json), so a shard at the threshold does 3x
# more work than it costs.  An estimate on one chip: the exchange between distinct devices has not been measured.
CSR_SHARD_MIN_NNZ = 1 << 20

_NOTED = set()


def _note_once(key, text):
    """One stderr line per process and cause when a problem runs in another arithmetic than the one asked for (never silently)."""
    if key not in _NOTED:
        _NOTED.add(key)
        sys.stderr.write(text)


def resolve_precision(precision, n, f, k):
    """The arithmetic one problem runs in.  'auto' by size (above); the 16-bit modes hand k > 512 to the fp32 kernels of the
    same library (LDS-tiled VALU GEMMs: any k, at least the 16-bit mode's accuracy) instead of refusing the problem -- and
    say so once on stderr (the fp32 kernels are an order of magnitude slower than the MFMA path).  An explicit 'f64', 'f32' or
    'bf16x3' runs as asked on every shape (the exact modes' kernels have no k bound and no accuracy envelope).  'f16x3' is
    explicit only ('auto' never picks it); k > 256 runs on bf16x3's kernels, said once on stderr."""
    if precision == 'auto':
        if float(n) * float(f) * float(k) < AUTO_F16_WORK:
            precision = 'f64'
        elif f >= AUTO_F16_MIN_F and k >= AUTO_F16_MIN_K:
            precision = 'f16'
        elif n > MAX_ROWS_EXACT:
            # outside the 16-bit mode's envelope, but beyond what one context of the exact modes holds: the 16-bit path runs
            # it (as 'auto' did before the envelope rule existed) and says what that means
            _note_once(('auto-rows', f < AUTO_F16_MIN_F, k < AUTO_F16_MIN_K),
                       "KLdivNMF: precision='auto': %d rows exceed one fp32 context (%d); the problem runs with precision='f16' although "
                       "f = %d, k = %d lie outside its accuracy envelope (f >= %d, k >= %d: final KL within 1e-4 of the reference's; "
                       "here up to 5e-4) -- shard the rows for fp32\n"
                       % (n, MAX_ROWS_EXACT, f, k, AUTO_F16_MIN_F, AUTO_F16_MIN_K))
            precision = 'f16'
        else:
            precision = 'f32'
    elif (_native.PRECISIONS[precision] == _native.PREC_BF16 and k <= MAX_K_MFMA
          and (f < AUTO_F16_MIN_F or k < AUTO_F16_MIN_K)):
        # an explicit 16-bit mode on a shape outside its envelope is honoured -- and never silent about it
        _note_once(('envelope', precision, f < AUTO_F16_MIN_F, k < AUTO_F16_MIN_K),
                   "KLdivNMF: precision=%r on f = %d, k = %d: outside the 16-bit mode's accuracy envelope (f >= %d and k >= %d keep "
                   "the final KL within 1e-4 of the reference's; measured up to 5e-4 below) -- precision='auto' or 'f32' keeps 1e-6\n"
                   % (precision, f, k, AUTO_F16_MIN_F, AUTO_F16_MIN_K))
    code = _native.PRECISIONS[precision]
    if code == _native.PREC_F16X3 and k > MAX_K_F16X3:
        _note_once(('k', precision), "KLdivNMF: precision=%r fuses k <= %d; k = %d runs on the split bf16 kernels (precision='bf16x3')\n"
                   % (precision, MAX_K_F16X3, k))
        return 'bf16x3'
    if code == _native.PREC_BF16 and k > MAX_K_MFMA:
        _note_once(('k', precision), "KLdivNMF: precision=%r holds k <= %d; k = %d runs on the fp32 kernels (precision='f32')\n"
                   % (precision, MAX_K_MFMA, k))
        return 'f32'
    return precision


def sparse_precision(precision):
    """The arithmetic CSR input runs in: the reference's sparse branch (ratio on the stored entries only, nmf.py:52-70,
    301-308, 331-334) exists as SDDMM + SpMM kernels in the exact modes.  'f64' / 'auto' -> f64, 'f32' -> f32; the 16-bit
    modes run it in fp32 (never the dense rule on a densified matrix, which is a different algorithm: off X's structure the
    dense ratio is eps / (W.H + eps), not 0) and say so once on stderr."""
    if precision in ('auto', 'f64'):
        return 'f64'
    if _native.PRECISIONS[precision] == _native.PREC_F32:
        return 'f32'
    if _native.PRECISIONS[precision] in (_native.PREC_BF16X3, _native.PREC_F16X3):
        _note_once(('csr', precision), "KLdivNMF: CSR input with precision=%r runs the reference's sparse branch on the fp32 "
                   "sparse kernels (precision='f32'); pass a dense array for the split-operand contractions\n" % (precision,))
        return 'f32'
    _note_once(('csr', precision), "KLdivNMF: CSR input with precision=%r runs the reference's sparse branch on the fp32 "
               "sparse kernels (precision='f32'); pass a dense array for the 16-bit MFMA path\n" % (precision,))
    return 'f32'


def weighted_precision(precision):
    """The arithmetic a weighted fit runs in (array `weights`): the weighted kernels exist in the two exact modes with plain
    operands (csrc/weighted.hip.h).  'f64' / 'auto' -> f64, 'f32' -> f32; every other mode runs them in fp32 and says so once
    on stderr (the `sparse_precision` pattern)."""
    if precision in ('auto', 'f64'):
        return 'f64'
    if _native.PRECISIONS[precision] == _native.PREC_F64:
        return 'f64'
    if _native.PRECISIONS[precision] == _native.PREC_F32:
        return 'f32'
    _note_once(('weights', precision), "KLdivNMF: weights with precision=%r run on the fp32 weighted kernels (precision='f32'); "
               "the weighted update exists in 'f64' and 'f32' only\n" % (precision,))
    return 'f32'


def check_weights(weights, shape, sparse=False):
    """`weights` as the loop honours it: None for a scalar (np.ndim 0: the reference's default 1., ignored as the reference
    ignores it), else a read-only float array broadcast to `shape` with np.broadcast_to.  ValueError -- on the host, before
    anything is uploaded -- for weights that do not broadcast to `shape`, negative or non-finite weights, and weights
    together with CSR input (the sparse branch's ratio lives on the stored entries only)."""
    if weights is None or np.ndim(weights) == 0:
        return None
    w = np.asarray(weights)
    if w.dtype not in (np.float32, np.float64):
        w = w.astype(np.float64)
    if sparse:
        raise ValueError("weights are not supported with CSR input: pass a dense array")
    try:
        wb = np.broadcast_to(w, tuple(shape))
    except ValueError:
        raise ValueError("weights of shape %s do not broadcast to the data's shape %s" % (w.shape, tuple(shape)))
    if not np.isfinite(w).all():
        raise ValueError("Non-finite values in weights passed to NMF.fit")
    if (w < 0).any():
        raise ValueError("Negative values in weights passed to NMF.fit")
    return wb


def weights_route(weights, blocks):
    """How `_fit_blocks` carries per-block `weights` (None, or one entry per block) to the device: None (no array among them:
    the unweighted loop), 'presence' or 'array'.  'presence' -- a row x modality mask, klnmf_upload_presence, no n x f weight
    buffer (csrc/presence.hip.h) -- where every entry is None, a scalar or an array of shape exactly (n, 1), at least one is
    an array, and there are at most `_native.MAX_MODALITIES` blocks: M = the number of blocks, the bounds are the block widths, the
    column of a block without weights is 1.  Every other case is 'array' (klnmf_upload_weights, csrc/weighted.hip.h)."""
    if weights is None:
        return None
    arrays = [w for w in weights if not (w is None or np.ndim(w) == 0)]
    if not arrays:
        return None
    n = blocks[0].shape[0]
    if len(blocks) <= _native.MAX_MODALITIES and all(np.shape(w) == (n, 1) for w in arrays):
        return 'presence'
    return 'array'


def _devices_of(device):
    """`device` as a tuple of GPU indices: an int is a one-entry list; a sequence of ints is a list (entries may repeat)."""
    if isinstance(device, (int, np.integer)) and not isinstance(device, bool):
        return (int(device),)
    try:
        devices = tuple(device)
    except TypeError:
        raise ValueError("device must be a GPU index or a sequence of them, not %r" % (device,))
    if not devices or any(isinstance(d, bool) or not isinstance(d, (int, np.integer)) or d < 0 for d in devices):
        raise ValueError("device must be a GPU index or a non-empty sequence of them, not %r" % (device,))
    return tuple(int(d) for d in devices)


def _default_devices():
    """KLNMF_DEVICES (comma-separated GPU indices) if set, else KLNMF_DEVICE (one index, default 0)."""
    env = os.environ.get('KLNMF_DEVICES', '').strip()
    if env:
        try:
            return _devices_of([int(x) for x in env.split(',') if x.strip()])
        except ValueError:
            raise ValueError("KLNMF_DEVICES=%r: expected comma-separated GPU indices, e.g. 0,1,2,3" % env)
    return (int(os.environ.get('KLNMF_DEVICE', '0')),)


def _default_device():
    """The one device of the paths that do not shard (single steps, evaluation, reconstruction): the first default device."""
    return _default_devices()[0]


def shard_plan(n, devices):
    """[(device, (row0, row1)), ...] of a dense loop on `devices`: `distributed.row_partition` over min(len(devices),
    ceil(n / 32)) of them (every shard holds at least one 32-row tile).  One entry: the plain single-context path."""
    from ..distributed import row_partition
    m = min(len(devices), (int(n) + 31) // 32)
    if m <= 1:
        return [(devices[0], (0, int(n)))]
    return list(zip(devices[:m], row_partition(int(n), m)))


def csr_shard_plan(indptr, devices):
    """[(device, (row0, row1)), ...] of a CSR loop on `devices`: `distributed.csr_row_partition` (stored entries balanced) over as
    many of them as keep every shard at `CSR_SHARD_MIN_NNZ` stored entries or more.  One entry: the plain single-context path."""
    from ..distributed import csr_row_partition
    indptr = np.asarray(indptr, dtype=np.int64)
    n, nnz = len(indptr) - 1, int(indptr[-1])
    m = min(len(devices), n, nnz // max(1, int(CSR_SHARD_MIN_NNZ)))
    while m > 1:
        parts = csr_row_partition(indptr, m)
        if all(int(indptr[b] - indptr[a]) >= CSR_SHARD_MIN_NNZ for a, b in parts):
            return list(zip(devices[:m], parts))
        m -= 1
    return [(devices[0], (0, n))]


def check_non_negative(X, whom):
    """ValueError on negative entries (reference nmf.py:23-26)."""
    X = X.data if sp.issparse(X) else X
    if (X < 0).any():
        raise ValueError("Negative values in data passed to %s" % whom)


def _scale(matrix, factors, axis=0):
    """Scale the columns (axis=0) or the lines (axis=1) of a 2-D array by a
    vector (reference nmf.py:29-49; host helper, not on the GPU loop)."""
    if not (len(matrix.shape) == 2):
        raise ValueError("Wrong array shape: %s, should have only 2 dimensions."
                         % str(matrix.shape))
    if axis not in (0, 1):
        raise ValueError('Wrong axis, should be 0 (scaling lines) '
                         'or 1 (scaling columns).')
    factors = np.squeeze(np.asarray(factors))
    if axis == 1:
        factors = factors[:, np.newaxis]
    return np.multiply(matrix, factors)


def _special_sparse_dot(a, b, refmat):
    """a.b sampled on the non-zeros of refmat, returned as CSR with refmat's
    structure (reference nmf.py:52-70, including its `eliminate_zeros` side
    effect on refmat).  Host scipy helper kept for callers of the module function; the
    fit / transform / error of CSR input run the same SDDMM on the device (csrc/sparse.hip.h)."""
    refmat.eliminate_zeros()
    ii, jj = refmat.nonzero()
    vals = np.einsum('ij,ij->i', a[ii, :], b.T[jj, :])
    return sp.coo_matrix((vals, (ii, jj)), shape=refmat.shape).tocsr()


def _dense(X):
    """Dense ndarray of validated input (only reached with CSR input by the single-step helpers that are handed an
    explicit dense Q; fit / transform / error / _update of CSR input take the sparse kernels: `_sparse_route`)."""
    if sp.issparse(X):
        return np.asarray(X.toarray())
    return np.asarray(X)


def _csr_of(blocks, coefs):
    """CSR of hstack([c * b ...]) (safe_hstack keeps the stack sparse if any block is, array_utils.py:5-9)."""
    mats = [sp.csr_matrix(b) * float(c) if sp.issparse(b) else sp.csr_matrix(np.asarray(b) * float(c))
            for b, c in zip(blocks, coefs)]
    X = mats[0] if len(mats) == 1 else sp.hstack(mats, format='csr')
    return sp.csr_matrix(X)


def _out_dtype(*arrays):
    """The reference computes in float32 only if every operand is float32."""
    if all(np.asarray(a).dtype == np.float32 for a in arrays):
        return np.float32
    return np.float64


class KLdivNMF(object):
    """Non negative factorization with Kullback Leibler divergence cost
    (Lee & Seung multiplicative updates), GPU implementation of reference
    nmf.py:73-351.

    Parameters as in the reference: n_components, tol (1e-6), max_iter (200),
    eps (1e-8; only used by `scale`), subit (unused), random_state (stored,
    unused -- the reference never reads it either).
    """

    def __init__(self, n_components=None, tol=1e-6, max_iter=200, eps=1.e-8,
                 subit=10, random_state=None, precision=None, device=None):
        self.n_components = n_components
        self._init_dictionary = None
        self.random_state = random_state
        self.tol = tol
        self.max_iter = max_iter
        self.eps = eps
        self.subit = subit
        self.precision = precision if precision is not None else _default_precision()
        # device: an int, or a list (KLNMF_DEVICES by default): the loop on two or more runs over row shards (`_fit_group`, CSR:
        # `_fit_group_csr`);
        # `device` is the first entry -- where everything that does not shard runs
        self.devices = _devices_of(device) if device is not None else _default_devices()
        self.device = self.devices[0]
        self.last_fp8_report = None         # set by every loop: what it ran on e4m3 operands (klnmf_query)
        self.last_weights_route = None      # set by every loop: how it carried array `weights` -- None, 'array' or 'presence' (`weights_route`)

    # ------------------------------------------------------------ helpers ---
    def _sparse_route(self, *blocks):
        """CSR input ALWAYS runs the reference's sparse branch (ratio on the stored entries only, nmf.py:52-70,
        301-308, 331-334): SDDMM + SpMM kernels of the exact modes, in the arithmetic `sparse_precision` names."""
        return any(sp.issparse(b) for b in blocks)

    def _context(self, exact=False, shape=None, sparse=False, weighted=False):
        prec = self.precision
        if weighted:                              # array weights: f64 ('auto', 'f64') or f32 (everything else)
            prec = weighted_precision(prec)
        elif sparse:                                # CSR input: f64 ('auto', 'f64') or f32 (everything else), never densified
            prec = sparse_precision(prec)
        elif prec == 'auto' and shape is None:    # single steps and loss evaluations: exact
            prec = 'f64'
        elif shape is not None:                   # decided per problem (shape = (n, f, k)): 'auto' by size, k > 512 -> fp32 kernels
            prec = resolve_precision(prec, *shape)
        if exact and _native.PRECISIONS[prec] not in (_native.PREC_F64, _native.PREC_F32, _native.PREC_BF16X3, _native.PREC_F16X3):
            prec = 'f64'
        return _native.Context(precision=prec, device=self.device, pooled=True)

    @classmethod
    def _exact_context(cls):
        return _native.Context(precision=os.environ.get('KLNMF_STEP_PRECISION', 'f64'),
                               device=_default_device(), pooled=True)

    def _init_H(self, n_features):
        """Initial dictionary (reference nmf.py:149-155)."""
        if self._init_dictionary is None:
            return normalize_sum(np.abs(np.random.random(
                (self.n_components, n_features))) + .01, axis=1)
        assert(self._init_dictionary.shape ==
               (self.n_components, n_features))
        return self._init_dictionary

    # --------------------------------------------------------------- loop ---
    def fit_transform(self, X, y=None, weights=1., _fit=True,
                      return_errors=False, scale_W=False):
        """Learn a NMF model for X and return the transformed data
        (reference nmf.py:159-230).  `y` and `scale_W` are accepted and
        ignored exactly as in the reference.

        `weights` (nmf.py:171-174: "weights on the cost function used as coefficients on each element of the data ...
        standard numpy broadcasting is used"; the reference then never reads it): an ARRAY -- anything with np.ndim >= 1,
        broadcast to X.shape -- is honoured: the loop minimises sum(weights * d(X | W.H)), its loss record and stop rule are
        the weighted ones, and an entry of weight 0 is missing data (`check_weights`: ValueError for a shape that does not
        broadcast, negative or non-finite weights, CSR input).  A scalar, the default 1. included, is ignored exactly as
        before: that path is bit-identical to the unweighted one.  The weighted update (csrc/weighted.hip.h) is
        W <- W * (R.H^T) / (weights.H^T), H <- rows normalised of H * (W^T.R) / (W^T.weights) with R = weights * ratio, a
        factor 1 where a denominator is 0; with weights of 1 and dictionary rows summing to 1 this is the reference's
        loop.  With a dictionary whose rows do not sum to 1 (a transform on a column slice of a dictionary) the weighted W
        rule divides by the row sums where the reference's does not.  It runs in 'f64' ('f64', 'auto') or 'f32' (every
        other precision, said once on stderr), on the first device of a device list (said once on stderr)."""
        X = atleast2d_or_csr(X)
        check_non_negative(X, "NMF.fit")
        return self._fit_blocks([X], [1.], _fit=_fit, return_errors=return_errors, weights=[weights])

    def _fit_blocks(self, blocks, coefs, _fit=True, return_errors=False, weights=None):
        """fit_transform of hstack([c * b for b, c in zip(blocks, coefs)])
        without building the stacked matrix on the host: each modality block is
        scaled, cast and placed by the upload kernel (learner.py:53-56 fused).
        `weights`: None, or one entry per block -- None / a scalar (that block's weights are 1) or an array broadcastable
        to the block (`check_weights`), uploaded block by block beside the data; `coefs` scale the data only.  Where every
        array among them is an (n, 1) presence column (`weights_route`), one n x M presence matrix is uploaded instead and the
        loop runs the masked kernels (csrc/presence.hip.h); `last_weights_route` names the path the loop took."""
        sparse = self._sparse_route(*blocks)
        route = None
        if weights is not None:
            if len(weights) != len(blocks):
                raise ValueError("weights: one entry per block expected (%d blocks, %d entries)" % (len(blocks), len(weights)))
            route = weights_route(weights, blocks)      # (from the shapes as given: check_weights broadcasts them)
            weights = [check_weights(w, b.shape, sparse) for w, b in zip(weights, blocks)]
            if all(w is None for w in weights):
                weights = None
        if sparse:
            X = _csr_of(blocks, coefs)
            return self._fit_uploaded(X.shape[0], X.shape[1], None,
                                      lambda H_init: np.float32 if (X.dtype == np.float32 and H_init.dtype == np.float32)
                                      else np.float64, _fit=_fit, return_errors=return_errors, sparse_X=X)
        blocks = [_dense(b) for b in blocks]
        n_samples = blocks[0].shape[0]
        n_features = sum(b.shape[1] for b in blocks)
        if weights is None:
            upload = lambda ctx: ctx.upload_blocks(blocks, coefs)
        elif route == 'presence':
            # one presence column per block (1 for a block without weights), the blocks' widths as the modalities' bounds
            P = np.ones((n_samples, len(blocks)), dtype=np.float64)
            for m, w in enumerate(weights):
                if w is not None:
                    P[:, m] = w[:, 0]
            bounds = np.concatenate([[0], np.cumsum([b.shape[1] for b in blocks])])

            def upload(ctx):
                ctx.upload_blocks(blocks, coefs)
                ctx.upload_weights(P, col_bounds=bounds)      # (the factored form: klnmf_upload_presence)
        else:
            def upload(ctx):
                ctx.upload_blocks(blocks, coefs)
                col = 0
                for b, w in zip(blocks, weights):
                    if w is not None:
                        ctx.upload_weights(w, row0=0, col0=col)
                    col += b.shape[1]
        out = self._fit_uploaded(n_samples, n_features, upload,
                                 lambda H_init: _out_dtype(H_init, *blocks), _fit=_fit,
                                 return_errors=return_errors, host_blocks=(blocks, coefs), weighted=weights is not None)
        self.last_weights_route = route if weights is not None else None
        return out

    def _after_upload(self, ctx):
        """Hook of `_fit_uploaded` behind the uploads, in front of the first dictionary: nothing here (subclasses with another
        cost function name it to the context: `beta_nmf.BetaNMF`)."""

    def _note_weighted_on_one_device(self):
        """(the group's exchange carries the H numerator alone: a weighted fit stays in one context)"""
        if len(self.devices) > 1:
            _note_once(('weights-group',), "KLdivNMF: a weighted fit runs on one device (%d), not over the row shards of devices %s\n"
                       % (self.device, list(self.devices)))

    def _fit_uploaded(self, n_samples, n_features, upload, out_dtype_of, _fit=True, return_errors=False,
                      sparse_X=None, host_blocks=None, weighted=False, sparse_nnz=None):
        """The loop of nmf.py:159-230 on a matrix that `upload(ctx)` places in the context: host blocks
        (`_fit_blocks`, which also passes them as `host_blocks` = (blocks, coefs): with two or more devices the loop runs over
        row shards, `_fit_group`) or rows gathered from device-resident data (`device_data.DeviceDataset`: first device).
        `sparse_nnz`: the matrix is a CSR problem of (n_samples, n_features, sparse_nnz) whose arrays `upload(ctx)` fills (rows
        gathered from device-resident CSR modalities): the reference's sparse branch in the arithmetic `sparse_precision` names,
        as with `sparse_X`, on the first device."""
        self.last_weights_route = None      # (`_fit_blocks` names the route of a weighted loop behind it)
        if not self.n_components:
            self.n_components = n_features
        H_init = self._init_H(n_features)
        k = self.n_components
        max_iter = int(self.max_iter)
        out_dtype = out_dtype_of(H_init)

        if len(self.devices) > 1 and weighted:
            self._note_weighted_on_one_device()
        elif len(self.devices) > 1:
            if sparse_X is not None:
                X = sp.csr_matrix(sparse_X, copy=True)      # (what set_problem_sparse uploads: no explicit zeros, sorted rows)
                X.eliminate_zeros()
                X.sort_indices()
                plan = csr_shard_plan(X.indptr, self.devices)
                if len(plan) > 1:
                    return self._fit_group_csr(plan, X, n_samples, n_features, H_init, out_dtype, _fit, return_errors)
                _note_once(('csr-group',), "KLdivNMF: CSR input runs on one device (%d), not over the row shards of devices %s "
                           "(fewer than CSR_SHARD_MIN_NNZ = %d stored entries per shard)\n"
                           % (self.device, list(self.devices), CSR_SHARD_MIN_NNZ))
            elif host_blocks is not None:
                plan = shard_plan(n_samples, self.devices)
                if len(plan) > 1:
                    return self._fit_group(plan, host_blocks[0], host_blocks[1], n_samples, n_features, H_init, out_dtype, _fit,
                                           return_errors)

        sparse = sparse_X is not None or sparse_nnz is not None
        with self._context(shape=None if sparse else (n_samples, n_features, k), sparse=sparse, weighted=weighted) as ctx:
            if sparse_X is not None:
                ctx.set_problem_sparse(sparse_X, k, max_iter)
            elif sparse_nnz is not None:
                ctx.set_problem_sparse_shape(n_samples, n_features, k, max_iter, sparse_nnz)
                upload(ctx)
            else:
                ctx.set_problem(n_samples, n_features, k, max_iter)
                upload(ctx)
            self._after_upload(ctx)
            ctx.set_H(H_init)
            ctx.init_W()                       # W0 = X . H_init^T (nmf.py:156)
            if _fit:
                self.components_ = H_init      # nmf.py:203-204
            elif self.components_ is not H_init:
                ctx.set_H(self.components_)    # loop runs on components_ (nmf.py:214)
            tol_abs = self.tol * n_samples * n_features      # nmf.py:207
            errors, n_done, stopped = ctx.run(max_iter, _fit, tol_abs)
            # what the loop ran on e4m3 operands (16-bit modes, large problems; all zero otherwise) -- as the library
            # reports it (klnmf_query); no reference counterpart
            self.last_fp8_report = ctx.fp8_report()
            self._check_f16_envelope(ctx, n_samples, n_features, k)
            W = ctx.get_W(dtype=out_dtype)
            if _fit and n_done > 0:
                self.components_ = ctx.get_H(dtype=out_dtype)

        n_iter = n_done + 1 if stopped else max_iter
        if max_iter > 0 and n_iter == max_iter and tol_abs > 0:   # nmf.py:224-225
            sys.stderr.write("Warning: Iteration limit reached during fit\n")
        if return_errors:
            return W, errors
        return W

    def _fit_group(self, plan, blocks, coefs, n_samples, n_features, H_init, out_dtype, _fit, return_errors):
        """`_fit_uploaded` over row shards: one context per entry of `plan` (`shard_plan`), driven as one group
        (klnmf_group_run: the numerator of the H rule and the loss exchanged between the contexts every iteration).  The
        arithmetic is the one the global shape picks; V is stored with one factor from the global maximum; W comes back in
        row order, `components_`, the loss record and `last_fp8_report` from shard 0 (identical on every shard)."""
        k = self.n_components
        prec = resolve_precision(self.precision, n_samples, n_features, k)
        vmax = 0.0
        for b, c in zip(blocks, coefs):
            if b.size:
                vmax = max(vmax, float(c) * float(np.max(b)))

        def load(ctx, r0, r1):
            ctx.set_problem(r1 - r0, n_features, k, int(self.max_iter))
            ctx.set_v_max(vmax)
            col = 0
            for b, c in zip(blocks, coefs):
                ctx.upload_V(b[r0:r1], row0=0, col0=col, scale=c)
                col += b.shape[1]
        return self._run_group(plan, prec, load, n_samples, n_features, H_init, out_dtype, _fit, return_errors)

    def _fit_group_csr(self, plan, X, n_samples, n_features, H_init, out_dtype, _fit, return_errors):
        """`_fit_group` for CSR input (`csr_shard_plan`): each context holds the CSR rows of its shard (klnmf_set_problem_sparse,
        the CSC order built on its device), in the arithmetic `sparse_precision` names -- the same as one context's."""
        k = self.n_components
        prec = sparse_precision(self.precision)

        def load(ctx, r0, r1):
            ctx.set_problem_sparse(X[r0:r1], k, int(self.max_iter))
        return self._run_group(plan, prec, load, n_samples, n_features, H_init, out_dtype, _fit, return_errors)

    def _run_group(self, plan, prec, load, n_samples, n_features, H_init, out_dtype, _fit, return_errors):
        """The group loop of `_fit_group` / `_fit_group_csr`: `load(ctx, row0, row1)` sets a shard's problem and data."""
        k = self.n_components
        max_iter = int(self.max_iter)
        H_loop = H_init if (_fit or self.components_ is H_init) else self.components_
        ctxs, group = [], None
        try:
            for dev, (r0, r1) in plan:
                ctx = _native.Context(precision=prec, device=dev, pooled=True)
                ctxs.append(ctx)
                load(ctx, r0, r1)
                ctx.set_H(H_init)
                ctx.init_W()                       # W0 = X . H_init^T (nmf.py:156), this shard's rows
                if H_loop is not H_init:
                    ctx.set_H(H_loop)              # loop runs on components_ (nmf.py:214)
            if _fit:
                self.components_ = H_init          # nmf.py:203-204
            group = _native.Group(ctxs)
            errors, n_done, stopped = group.run(n_samples, max_iter, _fit, self.tol)
            self.last_fp8_report = ctxs[0].fp8_report()
            self.last_fp8_report['shards'] = len(ctxs)
            self._check_f16_envelope(ctxs[0], n_samples, n_features, k)
            W = np.vstack([ctx.get_W(dtype=out_dtype) for ctx in ctxs])
            if _fit and n_done > 0:
                self.components_ = ctxs[0].get_H(dtype=out_dtype)
        finally:
            if group is not None:
                group.close()
            for ctx in ctxs:
                ctx.close()
        tol_abs = self.tol * n_samples * n_features
        n_iter = n_done + 1 if stopped else max_iter
        if max_iter > 0 and n_iter == max_iter and tol_abs > 0:   # nmf.py:224-225
            sys.stderr.write("Warning: Iteration limit reached during fit\n")
        if return_errors:
            return W, errors
        return W

    def _check_f16_envelope(self, ctx, n, f, k):
        """The run-time half of the 16-bit mode's envelope: the library holds loss and sum(V) on the device; a loop that ended
        with KL / sum(V) below `F16_MIN_KL_OVER_SUM_V` is reported in `last_fp8_report` and said once on stderr (the shape
        half is `resolve_precision`'s).  No reference counterpart (nmf.py has one arithmetic)."""
        rep = self.last_fp8_report
        if rep is None:
            return
        if ctx.precision != _native.PREC_BF16:
            rep['outside_f16_envelope'] = None      # (not a 16-bit loop: the key is there, the question does not arise)
            return
        r = rep.get('kl_over_sum_v', -1.0)
        reasons = []
        if f < AUTO_F16_MIN_F:
            reasons.append('f < %d' % AUTO_F16_MIN_F)
        if k < AUTO_F16_MIN_K:
            reasons.append('k < %d' % AUTO_F16_MIN_K)
        if 0.0 <= r < F16_MIN_KL_OVER_SUM_V:
            reasons.append('KL / sum(V) = %.2e < %.0e' % (r, F16_MIN_KL_OVER_SUM_V))
            _note_once(('residual',),
                       "KLdivNMF: this 16-bit fit ended with KL / sum(V) = %.2e (< %.0e): so little residual that the f16 operands' "
                       "rounding noise can exceed 1e-4 of the final KL (measured up to 8e-4) -- precision='f32' keeps 1e-6\n"
                       % (r, F16_MIN_KL_OVER_SUM_V))
        rep['outside_f16_envelope'] = reasons

    def fit(self, X, y=None, **params):
        """Learn a NMF model for X; returns self (reference nmf.py:259-273)."""
        self.fit_transform(X, **params)
        return self

    def transform(self, X, **params):
        """Coefficients of X for the fitted dictionary (reference
        nmf.py:275-291; leaves `_init_dictionary` set, like the reference)."""
        self._init_dictionary = self.components_
        params['_fit'] = False
        return self.fit_transform(X, **params)

    def _transform_blocks(self, blocks, coefs, return_errors=False, weights=None):
        self._init_dictionary = self.components_
        return self._fit_blocks(blocks, coefs, _fit=False, return_errors=return_errors, weights=weights)

    # -------------------------------------------------------- single steps ---
    def _update(self, X, W, _fit=True, scale_W=False, eps=1.e-8):
        """One update iteration (reference nmf.py:232-257)."""
        sparse = self._sparse_route(X)
        Xd = None if sparse else _dense(X)
        if scale_W:
            # dead from every caller in the reference (nmf.py:246-250), kept
            W = _scale(normalize_sum(W, axis=1), np.asarray(X.sum(axis=1)).ravel(), axis=1)
        if (eps != 1.e-8 and not sparse and self.precision != 'auto'
                and _native.PRECISIONS[self.precision] == _native.PREC_BF16):
            raise ValueError("the bf16 kernels use the reference's fixed eps = 1e-8")
        H = self.components_
        with self._context(sparse=sparse) as ctx:
            if sparse:
                Xc = ctx.set_problem_sparse(X, H.shape[0], 1)
                dt = _out_dtype(Xc.data, W, H)
            else:
                ctx.set_problem(Xd.shape[0], Xd.shape[1], H.shape[0], 1)
                ctx.upload_blocks([Xd])
                dt = _out_dtype(Xd, W, H)
            ctx.set_H(H)
            ctx.set_W(W)
            if eps != 1.e-8:
                ctx.set_ratio_eps(eps)
                ctx.step_Q()
                ctx.step_W()
                if _fit:
                    ctx.step_H()
            else:
                ctx.update(_fit)
            Wn = ctx.get_W(dtype=dt)
            if _fit:
                self.components_ = ctx.get_H(dtype=dt)
        return Wn

    def error(self, X, W, H=None, weights=1., eps=1.e-8):
        """generalized_KL(X, W.H) (reference nmf.py:297-310; `eps` is ignored by the reference's dense branch too, and so
        are `weights` there).  Array `weights` (np.ndim >= 1, broadcast to X.shape: `check_weights`) give the weighted loss
        sum(weights * (X log((X + eps) / (W.H + eps)) - X + W.H)) in 'f64' or 'f32' (`weighted_precision`); a scalar is
        ignored as before."""
        X = atleast2d_or_csr(X)
        if H is None:
            H = self.components_
        Om = check_weights(weights, X.shape, self._sparse_route(X))
        with self._context(sparse=self._sparse_route(X), weighted=Om is not None) as ctx:
            if self._sparse_route(X):
                ctx.set_problem_sparse(X, np.shape(H)[0], 1)      # nmf.py:301-308
            else:
                Xd = _dense(X)
                ctx.set_problem(Xd.shape[0], Xd.shape[1], np.shape(H)[0], 1)
                ctx.upload_blocks([Xd])
                if Om is not None:
                    ctx.upload_weights(Om)
            ctx.set_H(H)
            ctx.set_W(W)
            return ctx.error()

    def scale(self, W, H, factors):
        """Scale W columns and H rows inversely (reference nmf.py:314-321)."""
        safe_factors = factors + self.eps
        s_W = _scale(W, safe_factors, axis=0)
        s_H = _scale(H, 1. / safe_factors, axis=1)
        return s_W, s_H

    @classmethod
    def _Q(cls, X, W, H, eps=1.e-8):
        """(X + eps) / (W.H + eps), element-wise (reference nmf.py:325-336).
        CSR input gives a CSR result on X's structure, as in the reference."""
        if sp.issparse(X):
            with cls._exact_context() as ctx:
                Xc = ctx.set_problem_sparse(X, np.shape(H)[0], 1)
                ctx.set_H(H)
                ctx.set_W(W)
                ctx.set_ratio_eps(eps)
                ctx.step_Q()
                q = ctx.get_Q_values(dtype=_out_dtype(Xc.data, W, H))
            return sp.csr_matrix((q, Xc.indices, Xc.indptr), shape=Xc.shape)
        Xd = _dense(X)
        with cls._exact_context() as ctx:
            ctx.set_problem(Xd.shape[0], Xd.shape[1], np.shape(H)[0], 1)
            ctx.upload_V(Xd)
            ctx.set_H(H)
            ctx.set_W(W)
            ctx.set_ratio_eps(eps)
            ctx.step_Q()
            return ctx.get_Q(dtype=_out_dtype(Xd, W, H))

    @classmethod
    def _step(cls, X, W, H, Q, eps, which, weights=1.):
        Om = check_weights(weights, np.shape(X), sp.issparse(X))
        if sp.issparse(X) and Q is None:          # the sparse branch end to end (nmf.py:331-351)
            with cls._exact_context() as ctx:
                Xc = ctx.set_problem_sparse(X, np.shape(H)[0], 1)
                ctx.set_H(H)
                ctx.set_W(W)
                ctx.set_ratio_eps(eps)
                ctx.step_Q()
                dt = _out_dtype(Xc.data, W, H)
                if which == 'W':
                    ctx.step_W()
                    return ctx.get_W(dtype=dt)
                ctx.step_H()
                return ctx.get_H(dtype=dt)
        Xd = _dense(X)
        with cls._exact_context() as ctx:
            ctx.set_problem(Xd.shape[0], Xd.shape[1], np.shape(H)[0], 1)
            ctx.upload_V(Xd)
            if Om is not None:
                ctx.upload_weights(Om)
            ctx.set_H(H)
            ctx.set_W(W)
            if Q is None:
                ctx.set_ratio_eps(eps)
                ctx.step_Q()
            else:                                  # (a weighted rule contracts R = weights * Q)
                ctx.set_Q(_dense(Q) if Om is None else Om * _dense(Q))
            dt = _out_dtype(Xd, W, H)
            if which == 'W':
                ctx.step_W()
                return ctx.get_W(dtype=dt)
            ctx.step_H()
            return ctx.get_H(dtype=dt)

    @classmethod
    def _updated_W(cls, X, W, H, weights=1., Q=None, eps=1.e-8):
        """W * (Q.H^T) (reference nmf.py:338-343); array `weights`: W * ((weights * Q).H^T) / (weights.H^T), factor 1 where
        the denominator is 0 (a scalar is ignored as in the reference)."""
        return cls._step(X, W, H, Q, eps, 'W', weights)

    @classmethod
    def _updated_H(cls, X, W, H, weights=1., Q=None, eps=1.e-8):
        """normalize_rows(H * (W^T.Q)) (reference nmf.py:345-351); array `weights`:
        normalize_rows(H * (W^T.(weights * Q)) / (W^T.weights)), factor 1 where the denominator is 0."""
        return cls._step(X, W, H, Q, eps, 'H', weights)


# ------------------------------------------------------------------ batches ---
_EXACT_LOOP_REPORT = {}


def _exact_loop_report(precision, device):
    """`Context.fp8_report()` behind a loop of the exact modes -- no e4m3 operand, no monitor: the same record whatever the
    problem -- as the library itself reports it: read once per (precision, device) behind a one-element fit."""
    key = (precision, int(device))
    if key not in _EXACT_LOOP_REPORT:
        with _native.Context(precision=precision, device=int(device)) as ctx:
            ctx.set_problem(1, 1, 1, 1)
            ctx.upload_V(np.ones((1, 1)))
            ctx.set_H(np.ones((1, 1)))
            ctx.init_W()
            ctx.run(1, True, 0.0)
            _EXACT_LOOP_REPORT[key] = ctx.fp8_report()
    return copy.deepcopy(_EXACT_LOOP_REPORT[key])


CSR_BATCH_MAX_K = 512      # klnmf_batch_set_problem_sparse refuses more components (csrc/sparseb.hip.h: the blocked regime's limit)


def batch_precision(models, n, f, weighted=False, sparse=False):
    """'f64' / 'f32' if `models` can run as ONE batch of dense n x f problems (klnmf_batch_*): they agree in n_components, tol,
    max_iter and precision, that precision resolves to f64 or f32 for the shape (`resolve_precision`), and every model is on
    one and the same single device.  None otherwise.  weighted: a batch of masked problems -- the arithmetic is
    `weighted_precision`'s, which is what the single masked call runs in ('auto' -> f64, the 16-bit modes -> f32).  sparse: a
    batch of CSR problems -- `sparse_precision`'s arithmetic, with its stderr note, and k <= CSR_BATCH_MAX_K (the blocked sparse
    kernels; beyond, a context runs the unblocked ones).  A model under another cost function (`beta_nmf.BetaNMF` with
    beta != 1) never batches: the batch kernels run the Kullback-Leibler cost alone, and its own `fit_transform` runs it."""
    first = models[0]
    if any(getattr(m, 'beta', 1.0) != 1.0 for m in models):
        return None
    same = all((m.n_components, m.tol, m.max_iter, m.precision, m.devices) ==
               (first.n_components, first.tol, first.max_iter, first.precision, first.devices) for m in models)
    if not same or len(first.devices) != 1 or not 1 <= len(models) <= _native.BATCH_MAX:
        return None
    if weighted:
        return weighted_precision(first.precision)
    if sparse:
        return sparse_precision(first.precision) if (first.n_components or f) <= CSR_BATCH_MAX_K else None
    prec = resolve_precision(first.precision, n, f, first.n_components or f)
    return prec if _native.PRECISIONS[prec] in (_native.PREC_F64, _native.PREC_F32) else None


def fit_uploaded_batch(models, precision, n_samples, n_features, uploads, out_dtype_ofs, _fit=True, return_errors=False, masked=False,
                       sparse_nnzs=None, after_uploads=None):
    """`KLdivNMF._fit_uploaded` for len(models) dense problems of one shape as one `_native.Batch`: problem p is placed by
    `uploads[p](batch, p)`; model p ends as its own `_fit_uploaded` would leave it, with `last_batch_size` set.  masked: the
    uploads place a presence mask behind every V (`Batch.upload_presence*`, one set of bounds) and the loop is the masked one;
    every model ends with `last_weights_route` 'presence' (None otherwise).  sparse_nnzs: the problems are CSR ones of
    sparse_nnzs[p] stored entries (`Batch.set_problem_sparse`) that the uploads fill with `Batch.upload_csr_rows` /
    `upload_csr_device_rows`.  after_uploads: a hook `after_uploads(batch)` called behind every problem's upload and in front of the
    dictionaries and `init_W` -- where another cost function is named to the batch (`beta_nmf.fit_transform_batch`); None: every
    dictionary is set right behind its problem's upload, as ever.  Returns the list of the calls' results."""
    B = len(models)
    max_iter = int(models[0].max_iter)
    H_inits = []
    for m in models:                          # (list order: the global numpy stream is consumed as the sequential calls would)
        m.last_weights_route = None
        if not m.n_components:
            m.n_components = n_features
        H_inits.append(m._init_H(n_features))
    k = models[0].n_components
    tol_abs = models[0].tol * n_samples * n_features      # nmf.py:207
    with _native.Batch(precision, B, device=models[0].device) as batch:
        if sparse_nnzs is not None:
            batch.set_problem_sparse(n_samples, n_features, k, max_iter, sparse_nnzs)
        else:
            batch.set_problem(n_samples, n_features, k, max_iter)
        for p in range(B):
            uploads[p](batch, p)
            if after_uploads is None:
                batch.set_H(p, H_inits[p])
        if after_uploads is not None:
            after_uploads(batch)
            for p in range(B):
                batch.set_H(p, H_inits[p])
        batch.init_W()                       # W0 = X . H_init^T (nmf.py:156)
        for p, m in enumerate(models):
            if _fit:
                m.components_ = H_inits[p]    # nmf.py:203-204
            elif m.components_ is not H_inits[p]:
                batch.set_H(p, m.components_)      # loop runs on components_ (nmf.py:214)
        results = batch.run(max_iter, _fit, tol_abs)
        outs = []
        for p, (m, (errors, n_done, stopped)) in enumerate(zip(models, results)):
            out_dtype = out_dtype_ofs[p](H_inits[p])
            m.last_fp8_report = _exact_loop_report(precision, m.device)
            m.last_fp8_report['outside_f16_envelope'] = None      # (`_check_f16_envelope`: not a 16-bit loop)
            m.last_batch_size = B
            m.last_weights_route = 'presence' if masked else None
            W = batch.get_W(p, dtype=out_dtype)
            if _fit and n_done > 0:
                m.components_ = batch.get_H(p, dtype=out_dtype)
            n_iter = n_done + 1 if stopped else max_iter
            if max_iter > 0 and n_iter == max_iter and tol_abs > 0:   # nmf.py:224-225
                sys.stderr.write("Warning: Iteration limit reached during fit\n")
            outs.append((W, errors) if return_errors else W)
    return outs


def fit_transform_batch(models, Xs, weights=None, _fit=True, return_errors=False):
    """[models[i].fit_transform(Xs[i], weights=weights[i], _fit=_fit, return_errors=return_errors) for i ...] -- the independent
    fits of a sweep (samples/launcher.py:68-99) -- as ONE batch where that is possible: all Xs dense and of one shape, the models
    as `batch_precision` asks, and `weights` (None, or one entry per model as `fit_transform` takes it) either without an array
    -- every entry None or a scalar: the unweighted batch -- or every entry None / a scalar / an (n, 1) presence column
    (`weights_route` 'presence'): the masked batch, a model without an array on a mask of ones.  Every stage of an iteration is
    then one launch for all problems (csrc/batch.hip.h); each model stops on its own loss record.  Otherwise (an entry that
    routes to 'array' among them) the models run one after another through `fit_transform`, unchanged.  Each model gets
    `last_batch_size`: the batch's size, or 1.  The initial dictionaries are drawn in list order (or taken from
    `_init_dictionary`), so the global numpy stream is consumed exactly as by the sequential calls.

    CSR input: every X scipy-sparse, of one shape, each with stored entries, k <= CSR_BATCH_MAX_K, no array `weights` and models as
    `batch_precision` asks run as ONE CSR batch (csrc/batch_sparse.hip.h) -- the reference's sparse branch in the arithmetic
    `sparse_precision` names, validation and output dtype as `_fit_blocks` on CSR.  A mix of dense and sparse Xs runs one after
    another."""
    models, Xs = list(models), list(Xs)
    if len(models) != len(Xs):
        raise ValueError("fit_transform_batch: one X per model expected (%d models, %d Xs)" % (len(models), len(Xs)))
    if weights is not None:
        weights = list(weights)
        if len(weights) != len(models):
            raise ValueError("fit_transform_batch: one weights entry per model expected (%d models, %d entries)" % (len(models), len(weights)))
    if Xs and all(sp.issparse(X) for X in Xs) and len(set(X.shape for X in Xs)) == 1 and \
            (weights is None or all(w is None or np.ndim(w) == 0 for w in weights)):
        outs = _fit_transform_batch_csr(models, Xs, _fit, return_errors)
        if outs is not None:
            return outs
    dense = bool(Xs) and not any(sp.issparse(X) for X in Xs)
    if dense:
        Xs = [atleast2d_or_csr(X) for X in Xs]
        dense = len(set(X.shape for X in Xs)) == 1
    routes = [None] * len(models) if weights is None or not dense else [weights_route([w], [X]) for w, X in zip(weights, Xs)]
    masked = 'presence' in routes
    precision = batch_precision(models, *Xs[0].shape, weighted=masked) if dense and 'array' not in routes else None
    if precision is None:
        outs = []
        for i, (m, X) in enumerate(zip(models, Xs)):
            if weights is None:
                outs.append(m.fit_transform(X, _fit=_fit, return_errors=return_errors))
            else:
                outs.append(m.fit_transform(X, weights=weights[i], _fit=_fit, return_errors=return_errors))
            m.last_batch_size = 1
        return outs
    blocks = []
    for X in Xs:
        check_non_negative(X, "NMF.fit")
        blocks.append(_dense(X))
    n, f = blocks[0].shape
    if masked:
        # one presence column per problem (1 for a model without an array), one modality of all f columns: `_fit_blocks`'s form
        Ps = [np.ones((n, 1)) if r is None else np.array(check_weights(w, (n, 1)), dtype=np.float64) for w, r in zip(weights, routes)]

        def place(batch, p, b, P):
            batch.upload_V(p, b)
            batch.upload_presence(p, P, [0, f])
        uploads = [lambda batch, p, b=b, P=P: place(batch, p, b, P) for b, P in zip(blocks, Ps)]
    else:
        uploads = [lambda batch, p, b=b: batch.upload_V(p, b) for b in blocks]
    out_dtype_ofs = [lambda H_init, b=b: _out_dtype(H_init, b) for b in blocks]
    return fit_uploaded_batch(models, precision, n, f, uploads, out_dtype_ofs, _fit=_fit, return_errors=return_errors, masked=masked)


def _fit_transform_batch_csr(models, Xs, _fit, return_errors):
    """`fit_transform_batch`'s CSR batch for scipy-sparse Xs of one shape; None where the sequential route has to run (the models
    do not agree, k > CSR_BATCH_MAX_K, an X without stored entries)."""
    n, f = Xs[0].shape
    for X in Xs:                       # (`fit_transform`'s validation, `_fit_blocks`'s stack of one block)
        check_non_negative(atleast2d_or_csr(X), "NMF.fit")
    mats = [_native.csr_canonical(_csr_of([atleast2d_or_csr(X)], [1.])) for X in Xs]
    if any(X.nnz == 0 for X in mats) or not 1 <= len(models) <= _native.BATCH_MAX:
        return None
    precision = batch_precision(models, n, f, sparse=True)
    if precision is None:
        return None
    uploads = [lambda batch, p, X=X: batch.upload_csr_rows(p, X) for X in mats]
    out_dtype_ofs = [lambda H_init, X=X: np.float32 if (X.dtype == np.float32 and H_init.dtype == np.float32) else np.float64
                     for X in mats]
    return fit_uploaded_batch(models, precision, n, f, uploads, out_dtype_ofs, _fit=_fit, return_errors=return_errors,
                              sparse_nnzs=[int(X.nnz) for X in mats])
