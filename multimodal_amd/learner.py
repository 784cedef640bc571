# encoding: utf-8
"""Multimodal dictionary learning on top of the GPU KL-NMF.

Interface-compatible with reference multimodal/learner.py (`MultimodalLearner`
with attributes mod/dim/coef/k/dico/nmf_train and its twelve methods, plus
`fit_coefficients`), so `experiment.py` and the sample scripts can drive it
unchanged.  What differs is where the work happens: the per-modality blocks and
their balancing coefficients go straight to the NMF upload, where scale, cast
and column placement are one kernel per block, instead of first materialising
`safe_hstack([c * m ...])` on the host (reference learner.py:53-56).
The arithmetic is KLdivNMF's: KLNMF_PRECISION = f64 (default) | f32 | bf16x3 | f16x3 | f16 | auto (lib/nmf.py).
"""
from .lib.nmf import KLdivNMF as NMF
from .lib.nmf import check_non_negative
from .lib.array_utils import safe_hstack
from .lib.sklearn_utils import atleast2d_or_csr
from . import _native
from .lib.nmf import _default_device


def _checked(blocks):
    """Apply the input contract of NMF.fit to every modality block."""
    checked = []
    for block in blocks:
        block = atleast2d_or_csr(block)
        check_non_negative(block, "NMF.fit")
        checked.append(block)
    return checked


def _model(beta, **kw):
    """The NMF of a learner: `KLdivNMF` for the default cost (beta = 1.0: today's code path, call for call), `BetaNMF` for every
    other beta -- imported only then."""
    if beta == 1.0:
        return NMF(**kw)
    from .lib.beta_nmf import BetaNMF
    return BetaNMF(beta=beta, **kw)


def _coefficients_on(dictionary, blocks, scales, iter_nmf, weights=None, beta=1.0):
    """tol=0 transform of the (virtually) stacked blocks on a fixed dictionary; `weights`: None or one entry per block
    (`KLdivNMF._fit_blocks`); `beta`: the cost (`_model`)."""
    model = _model(beta, n_components=dictionary.shape[0], max_iter=iter_nmf, tol=0)
    model.components_ = dictionary
    return model._transform_blocks(_checked(blocks), scales, weights=weights)


def fit_coefficients(data_obs, dictionary, iter_nmf=100, verbose=False, weights=None, beta=1.0):
    """Non-negative coefficients of `data_obs` on `dictionary`
    (reference learner.py:11-15: tol=0 transform for iter_nmf iterations).  `weights`: None, or an array broadcastable to
    `data_obs` -- weights on the cost function, 0 = a missing entry (`KLdivNMF.fit_transform`).  `beta`: the beta divergence
    of the cost (1.0: Kullback-Leibler, the reference's; `lib.beta_nmf.BetaNMF` otherwise)."""
    return _coefficients_on(dictionary, [data_obs], [1.], iter_nmf, weights=None if weights is None else [weights], beta=beta)


class MultimodalLearner(object):
    """Holds one dictionary over several column-stacked modalities.

    modalities: names; dimensions: number of columns of each; coefficients:
    per-modality scale applied before stacking; k: number of atoms.
    `dico` ([k, sum(dimensions)] ndarray, None until trained) may also be
    assigned from outside (the sample scripts do).  `beta`: the beta divergence of the cost function, 1.0 (Kullback-Leibler, the
    reference's) by default; with another value `train`, `reconstruct_internal_multi` and what builds on them run
    `lib.beta_nmf.BetaNMF` (2.0: Euclidean, 0: Itakura-Saito).
    """

    def __init__(self, modalities, dimensions, coefficients, k,
                 sparseness=None, sp_coef=.1, beta=1.0):
        self.mod = modalities
        self.dim = dimensions
        self.coef = coefficients
        self.k = k
        self.sparseness = sparseness
        self.sp_coef = sp_coef
        self.beta = float(beta)
        self.dico = None

    # ---- bookkeeping ----
    def get_index(self, modality):
        return self.mod.index(modality)

    def get_axis_range(self, modality):
        """(start, stop) columns of a modality in the stacked matrix
        (reference learner.py:58-62)."""
        idx = self.get_index(modality)
        start = sum(self.dim[:idx])
        return (start, start + self.dim[idx])

    def _scales(self, modalities):
        return [self.coef[self.get_index(m)] for m in modalities]

    def stack_data(self, modalities, data_matrices):
        """Host-side stacked matrix hstack(c_m * X_m) (reference learner.py:53-56).
        Kept for callers; train/reconstruct do not need it."""
        return safe_hstack([c * m for m, c in
                            zip(data_matrices, self._scales(modalities))])

    # ---- dictionary ----
    def train(self, data_matrices, iterations, weights=None):
        """Fit the dictionary on all modalities: `iterations` multiplicative
        updates with tol=0 (reference learner.py:31-41).  `weights`: None, or a list with one entry per modality, each None
        or an array broadcastable to that modality's block -- weights on the cost function, uploaded block by block beside
        the data (`KLdivNMF.fit_transform`).  An (n, 1) column of 0 / 1 marks the samples in which a modality is missing.
        The modality coefficients `coef` keep scaling the data only."""
        n_samples = data_matrices[0].shape[0]
        for m, d in zip(data_matrices, self.dim):
            assert(m.shape == (n_samples, d))
        if self.sparseness is not None:
            raise NotImplemented        # as the reference (learner.py:37-38)
        self.nmf_train = _model(self.beta, n_components=self.k, max_iter=iterations, tol=0)
        self.nmf_train._fit_blocks(_checked(data_matrices), self._scales(self.mod),
                                   _fit=True, weights=weights)
        self.dico = self.nmf_train.components_

    def get_dico(self, modality=None):
        """Whole dictionary, or the column slice (a view) of one modality."""
        if modality is None:
            return self.dico
        start, stop = self.get_axis_range(modality)
        return self.dico[:, start:stop]

    def get_stacked_dicos(self, modalities):
        return safe_hstack([self.get_dico(modality=m) for m in modalities])

    # ---- inference ----
    def reconstruct_internal_multi(self, orig_mods, test_data, iterations, weights=None):
        """Internal coefficients from a subset of modalities
        (reference learner.py:71-78).  `weights`: as in `train`, one entry per modality of `orig_mods`."""
        for mod, data in zip(orig_mods, test_data):
            assert(data.shape[1] == self.dim[self.get_index(mod)])
        return _coefficients_on(self.get_stacked_dicos(orig_mods), test_data,
                                self._scales(orig_mods), iterations, weights=weights, beta=self.beta)

    def reconstruct_internal(self, orig_mod, test_data, iterations):
        """Internal coefficients from one modality (reference learner.py:68-69).  `test_data` may be a
        `features.hac.DeviceCsrRows` (a CSR matrix built on the device): see `_reconstruct_internal_device_rows`."""
        from .features.hac import DeviceCsrRows
        if isinstance(test_data, DeviceCsrRows):
            return self._reconstruct_internal_device_rows(orig_mod, test_data, iterations)
        return self.reconstruct_internal_multi([orig_mod], [test_data],
                                               iterations)

    def _reconstruct_internal_device_rows(self, orig_mod, X, iterations):
        """`reconstruct_internal(orig_mod, X.to_scipy(), iterations)`, bit for bit, without the download: the CSR problem is
        gathered from X's device arrays (klnmf_upload_csr_device_rows: X the single source, the identity as row index, the
        modality's coefficient as scale), as `DeviceDataset._fit_sparse` does.  Where `device_data.csr_rows_plan` says the
        gather cannot reproduce the reference's dropped zeros -- and for another cost than Kullback-Leibler, or a matrix
        without stored entries -- the host path runs on `X.to_scipy()`."""
        import numpy as np
        from .device_data import csr_rows_plan
        idx = self.get_index(orig_mod)
        n, f = X.shape
        assert(f == self.dim[idx])
        coef = self.coef[idx]
        nnz, use_device = csr_rows_plan([X.indptr], np.arange(n, dtype=np.int64), [coef], [X.least])
        if self.beta != 1.0 or not use_device or nnz == 0:
            return self.reconstruct_internal_multi([orig_mod], [X.to_scipy()], iterations)
        import torch
        rows = torch.arange(n, dtype=torch.int64, device=X.d_indptr.device)

        def upload(ctx):         # (synchronous: `rows` is free to go when it returns)
            ctx.upload_csr_device_rows([X.pointers()], [0, f], [float(coef)], n, rows.data_ptr(), n)
        dictionary = self.get_stacked_dicos([orig_mod])
        model = NMF(n_components=dictionary.shape[0], max_iter=iterations, tol=0)
        model.components_ = dictionary
        model._init_dictionary = dictionary       # (`_transform_blocks`)
        out_dtype_of = lambda H: np.float32 if (not X.f64 and H.dtype == np.float32) else np.float64      # (as `_fit_blocks` on CSR)
        return model._fit_uploaded(n, f, upload, out_dtype_of, _fit=False, sparse_nnz=nnz)

    def reconstruct_modalities(self, dest_mods, internal):
        """internal . stacked dictionaries of dest_mods (reference learner.py:83-84),
        on the device (klnmf_matmul), in the operands' arithmetic."""
        return _native.matmul(internal, self.get_stacked_dicos(dest_mods), _default_device())

    def reconstruct_modality(self, dest_mod, internal):
        """internal . dictionary of dest_mod (reference learner.py:80-81)."""
        return _native.matmul(internal, self.get_dico(dest_mod), _default_device())

    def modalities_to_modalities(self, orig_mods, dest_mods, test_data,
                                 iterations):
        internal = self.reconstruct_internal_multi(orig_mods, test_data,
                                                   iterations)
        return self.reconstruct_modalities(dest_mods, internal)

    def modality_to_modality(self, orig_mod, dest_mod, test_data, iterations):
        return self.modalities_to_modalities([orig_mod], [dest_mod],
                                             [test_data], iterations)
