# encoding: utf-8
"""NMF under a beta divergence: `KLdivNMF`'s loop on another cost function (csrc/beta.hip.h, include/klnmf_beta.h).

The reference announces "Helpers for beta divergence and related updates" (nmf.py:293) and holds none; its constructor carries
`subit`, "only for gradient updates".  `BetaNMF(beta=...)` is that family on the exact kernels: beta = 2 the Euclidean cost,
beta = 0 Itakura-Saito, beta = 1 Kullback-Leibler -- which is `KLdivNMF`'s own code on every call, bit for bit --, any other
finite beta the general formula.  With x = X + 1e-8 and y = W.H + 1e-8 the cost is sum(weights * d_beta(x | y)) and the rules are
the majorise-minimise ones,
    W <- W * ((A.H^T) / (B.H^T))^gamma,   H <- H * ((W^T.A) / (W^T.B))^gamma,   A = weights * x * y^(beta-2), B = weights * y^(beta-1),
gamma = 1/(2-beta) below 1, 1 up to 2, 1/(beta-1) beyond; H's rows are normalised to sum 1 and W's columns take the sums, so W.H is
what the rules left.  Every half step forms its own A and B: the loss record never rises.
"""
import numpy as np
import scipy.sparse as sp

from .. import _native
from . import nmf
from .array_utils import normalize_sum
from .nmf import KLdivNMF, _dense, _note_once, _out_dtype, _scale, check_non_negative, check_weights
from .sklearn_utils import atleast2d_or_csr


def beta_precision(precision):
    """The arithmetic a beta != 1 problem runs in: the beta kernels exist in the two exact modes with plain operands, as the
    weighted ones do (`nmf.weighted_precision`).  'f64' / 'auto' -> f64, 'f32' -> f32; every other mode runs them in fp32 and
    says so once on stderr."""
    if precision in ('auto', 'f64'):
        return 'f64'
    if _native.PRECISIONS[precision] == _native.PREC_F64:
        return 'f64'
    if _native.PRECISIONS[precision] == _native.PREC_F32:
        return 'f32'
    _note_once(('beta', precision), "BetaNMF: beta != 1 with precision=%r runs on the fp32 beta kernels (precision='f32'); "
               "the beta update exists in 'f64' and 'f32' only\n" % (precision,))
    return 'f32'


def beta_batch_precision(models):
    """'f64' / 'f32' if `models` can run as ONE beta batch (klnmf_batch_set_divergence): every model a `BetaNMF` of one and the same
    beta != 1, the models agreeing as `nmf.batch_precision` asks -- n_components, tol, max_iter, precision, one and the same single
    device -- with the arithmetic `beta_precision` names (what the single beta call runs in).  None otherwise."""
    first = models[0]
    if not all(isinstance(m, BetaNMF) and m.beta == first.beta for m in models) or first.beta == 1.0:
        return None
    same = all((m.n_components, m.tol, m.max_iter, m.precision, m.devices) ==
               (first.n_components, first.tol, first.max_iter, first.precision, first.devices) for m in models)
    if not same or len(first.devices) != 1 or not 1 <= len(models) <= _native.BATCH_MAX:
        return None
    return beta_precision(first.precision)


def fit_transform_batch(models, Xs, weights=None, _fit=True, return_errors=False):
    """[models[i].fit_transform(Xs[i], weights=weights[i], _fit=_fit, return_errors=return_errors) for i ...] as ONE beta batch
    (csrc/batch.hip.h, include/klnmf_batch_beta.h) where that is possible: every model a `BetaNMF` of one and the same beta != 1, all
    Xs dense and of one shape, the models as `beta_batch_precision` asks, and every `weights` entry None, a scalar or an array that
    passes `check_weights` -- arrays are uploaded as the problems' weights (a model without one is weighted by ones) and the models
    end with `last_weights_route` 'array'.  Every stage of a beta iteration is then one launch for all problems; each model stops
    on its own loss record.  Everything else is `nmf.fit_transform_batch`'s, unchanged: beta = 1 throughout runs its batches, and
    mixed betas, sparse Xs (which raise as in `fit_transform`), unequal shapes and device lists run one after another.  Each
    model gets `last_batch_size`; the initial dictionaries are drawn in list order, so the global numpy stream ends where the
    sequential calls leave it."""
    models, Xs = list(models), list(Xs)
    if weights is not None:
        weights = list(weights)

    def elsewhere():
        return nmf.fit_transform_batch(models, Xs, weights=weights, _fit=_fit, return_errors=return_errors)
    if not models or len(models) != len(Xs) or (weights is not None and len(weights) != len(models)):
        return elsewhere()
    precision = beta_batch_precision(models) if not any(sp.issparse(X) for X in Xs) else None
    if precision is None:
        return elsewhere()
    Xs = [atleast2d_or_csr(X) for X in Xs]
    if len(set(X.shape for X in Xs)) != 1:
        return elsewhere()
    try:
        Oms = [None] * len(models) if weights is None else [check_weights(w, X.shape) for w, X in zip(weights, Xs)]
    except ValueError:
        return elsewhere()      # (the sequential calls raise it where they meet it)
    blocks = []
    for X in Xs:
        check_non_negative(X, "NMF.fit")
        blocks.append(_dense(X))
    n, f = blocks[0].shape
    beta = models[0].beta
    weighted = any(w is not None for w in Oms)

    def name_cost(batch):
        batch.set_divergence(beta)
        for p, w in enumerate(Oms):
            if w is not None:
                batch.upload_weights(p, w)
    uploads = [lambda batch, p, b=b: batch.upload_V(p, b) for b in blocks]
    out_dtype_ofs = [lambda H_init, b=b: _out_dtype(H_init, b) for b in blocks]
    outs = nmf.fit_uploaded_batch(models, precision, n, f, uploads, out_dtype_ofs, _fit=_fit, return_errors=return_errors,
                                  after_uploads=name_cost)
    for m in models:
        m.last_weights_route = 'array' if weighted else None
    return outs


class BetaNMF(KLdivNMF):
    """Non negative factorization under the beta divergence `beta` (2.0: Euclidean; 0: Itakura-Saito; 1: `KLdivNMF` itself).
    The other parameters, `fit_transform` / `fit` / `transform` (`weights`, `_fit`, `return_errors`, `scale_W`), the start, the
    stop rule `tol * n * f` and the iteration-limit warning are `KLdivNMF`'s.

    With beta != 1: array `weights` of any broadcastable shape run the weighted route (`last_weights_route` 'array'; an (n, 1)
    presence column too: the masked form exists for beta = 1 only); the loop runs in 'f64' ('f64', 'auto') or 'f32' (every other
    precision, said once on stderr), on the first device of a device list (said once on stderr); scipy-sparse input raises
    ValueError before anything is uploaded."""

    def __init__(self, beta=2.0, n_components=None, tol=1e-6, max_iter=200, eps=1.e-8,
                 subit=10, random_state=None, precision=None, device=None):
        KLdivNMF.__init__(self, n_components=n_components, tol=tol, max_iter=max_iter, eps=eps, subit=subit,
                          random_state=random_state, precision=precision, device=device)
        beta = float(beta)
        if not np.isfinite(beta):
            raise ValueError("beta must be finite, not %r" % (beta,))
        self.beta = beta

    @property
    def _kl(self):
        return self.beta == 1.0

    # ------------------------------------------------------------ helpers ---
    def _context(self, exact=False, shape=None, sparse=False, weighted=False):
        if self._kl:
            return KLdivNMF._context(self, exact=exact, shape=shape, sparse=sparse, weighted=weighted)
        return _native.Context(precision=beta_precision(self.precision), device=self.device, pooled=True)

    def _after_upload(self, ctx):
        if not self._kl:
            ctx.set_divergence(self.beta)

    def _note_weighted_on_one_device(self):
        if self._kl:
            return KLdivNMF._note_weighted_on_one_device(self)
        if len(self.devices) > 1:
            _note_once(('beta-group',), "BetaNMF: a beta != 1 fit runs on one device (%d), not over the row shards of devices %s\n"
                       % (self.device, list(self.devices)))

    def _refuse_sparse(self, *blocks):
        if self._sparse_route(*blocks):
            raise ValueError("BetaNMF(beta=%g): scipy-sparse input is supported with beta = 1 only (the sparse branch's ratio lives "
                             "on the stored entries); pass a dense array" % self.beta)

    # --------------------------------------------------------------- loop ---
    def _fit_blocks(self, blocks, coefs, _fit=True, return_errors=False, weights=None):
        """`KLdivNMF._fit_blocks` under the beta cost: every array among `weights` is uploaded block by block beside the data
        (klnmf_upload_weights), and the context is told the cost behind the uploads (klnmf_set_divergence)."""
        if self._kl:
            return KLdivNMF._fit_blocks(self, blocks, coefs, _fit=_fit, return_errors=return_errors, weights=weights)
        self._refuse_sparse(*blocks)
        if weights is not None:
            if len(weights) != len(blocks):
                raise ValueError("weights: one entry per block expected (%d blocks, %d entries)" % (len(blocks), len(weights)))
            weights = [check_weights(w, b.shape) for w, b in zip(weights, blocks)]
            if all(w is None for w in weights):
                weights = None
        blocks = [_dense(b) for b in blocks]
        n_samples = blocks[0].shape[0]
        n_features = sum(b.shape[1] for b in blocks)

        def upload(ctx):
            ctx.upload_blocks(blocks, coefs)
            col = 0
            for b, w in zip(blocks, weights or [None] * len(blocks)):
                if w is not None:
                    ctx.upload_weights(w, row0=0, col0=col)
                col += b.shape[1]
        # (weighted=True: one context on the first device, in the arithmetic `_context` names)
        out = self._fit_uploaded(n_samples, n_features, upload, lambda H_init: _out_dtype(H_init, *blocks), _fit=_fit,
                                 return_errors=return_errors, weighted=True)
        self.last_weights_route = 'array' if weights is not None else None
        return out

    # -------------------------------------------------------- single steps ---
    def _update(self, X, W, _fit=True, scale_W=False, eps=1.e-8):
        """One iteration of the beta loop at (W, components_): the W rule, and in a fit the H rule from a fresh ratio.
        `scale_W` rescales W's rows to X's row sums first, as `KLdivNMF._update` does; the beta cost is defined with
        eps = 1e-8, so any other `eps` raises ValueError."""
        if self._kl:
            return KLdivNMF._update(self, X, W, _fit=_fit, scale_W=scale_W, eps=eps)
        self._refuse_sparse(X)
        if eps != 1.e-8:
            raise ValueError("BetaNMF(beta=%g): the beta kernels use the fixed eps = 1e-8" % self.beta)
        Xd = _dense(X)
        if scale_W:
            W = _scale(normalize_sum(W, axis=1), np.asarray(Xd.sum(axis=1)).ravel(), axis=1)
        H = self.components_
        dt = _out_dtype(Xd, W, H)
        with self._context() as ctx:
            ctx.set_problem(Xd.shape[0], Xd.shape[1], H.shape[0], 1)
            ctx.upload_blocks([Xd])
            ctx.set_divergence(self.beta)
            ctx.set_H(H)
            ctx.set_W(W)
            ctx.update(_fit)
            Wn = ctx.get_W(dtype=dt)
            if _fit:
                self.components_ = ctx.get_H(dtype=dt)
        return Wn

    def error(self, X, W, H=None, weights=1., eps=1.e-8):
        """sum(weights * d_beta(X + 1e-8 | W.H + 1e-8)) (klnmf_beta_loss); beta = 1: `KLdivNMF.error`.  `eps` is ignored as the
        reference's dense branch ignores it."""
        if self._kl:
            return KLdivNMF.error(self, X, W, H=H, weights=weights, eps=eps)
        X = atleast2d_or_csr(X)
        self._refuse_sparse(X)
        if H is None:
            H = self.components_
        Om = check_weights(weights, X.shape)
        Xd = _dense(X)
        with self._context() as ctx:
            ctx.set_problem(Xd.shape[0], Xd.shape[1], np.shape(H)[0], 1)
            ctx.upload_blocks([Xd])
            if Om is not None:
                ctx.upload_weights(Om)
            ctx.set_divergence(self.beta)
            ctx.set_H(H)
            ctx.set_W(W)
            return ctx.beta_loss()
