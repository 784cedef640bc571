# encoding: utf-8
"""Experiment data resident on the GPU across runs (next-row N2 of SURVEY.md 8f).

The reference's experiment loop slices every modality on the host for each run
(`data_train = [x[train, :] for x in self.data]`, experiment.py:163-164) and the learner re-uploads
what it is given.  Here the modalities are uploaded once (fp32); a run hands over row indices, and
the rows are gathered by the tiling upload kernel itself (`klnmf_upload_V_device_rows`), together
with the per-modality coefficient and the column placement (learner.py:53-56).

The reference's datasets are sparse (db/objects.py:79-81 builds CSR histograms) and `safe_hstack` keeps their stack sparse, so
an experiment on them runs the reference's sparse branch (nmf.py:52-70, 301-308, 331-334).  `DeviceDataset(keep_sparse=True)`
does the same on the device: sparse modalities stay CSR in device memory, and a run's stacked CSR of the selected rows is
gathered there (`klnmf_upload_csr_device_rows`, csrc/csrgather.hip.h) -- nothing of nnz length is sliced on the host.

`DeviceDataset(presence=[...])` keeps a row x modality presence mask (a modality absent from some samples) resident beside the
modalities: a call whose modalities carry a mask column gathers its rows of the mask on the device
(`klnmf_upload_presence_device_rows`) and runs the masked loop of csrc/presence.hip.h -- the reference has no counterpart.
"""
import numpy as np
import scipy.sparse as sp

from . import _native
from .lib.nmf import (KLdivNMF, check_non_negative, check_weights, _default_precision, resolve_precision, _csr_of, _note_once,
                      batch_precision, fit_uploaded_batch)
from .lib.sklearn_utils import atleast2d_or_csr


def csr_rows_plan(indptrs, rows, coefs, minima):
    """What one call on the rows `rows` of CSR modalities needs to know before anything is launched -- from the host copies of
    the row pointers alone, nothing of nnz length: (nnz, use_device).

    nnz: the stored entries of hstack([c * X[rows] ...]), repeats counted as often as they occur.  use_device: the device gather
    uploads the problem the host path uploads.  The reference drops stored entries that become zero (nmf.py:66) and a device
    gather cannot once nnz is fixed, so a call takes the host path when a coefficient is not positive, or when a modality's
    smallest stored value (`minima`: a numpy scalar of the modality's own type, None without stored entries) times its
    coefficient rounded to that type is zero -- the product as `sp.csr_matrix(b) * float(c)` forms it."""
    rows = np.asarray(rows, dtype=np.int64)
    nnz = 0
    for ip in indptrs:
        ip = np.asarray(ip)
        nnz += int((ip[rows + 1] - ip[rows]).sum())
    use_device = True
    for c, least in zip(coefs, minima):
        if not float(c) > 0.0:
            use_device = False
        elif least is not None:
            with np.errstate(all='ignore'):
                if least * type(least)(float(c)) == 0:
                    use_device = False
    return nnz, use_device


def refuse_beta(*learners):
    """The device-resident runs exist for the default cost alone: a learner with beta != 1 (`MultimodalLearner(beta=...)`) raises
    ValueError here, before anything is gathered -- its host calls run `BetaNMF`."""
    for learner in learners:
        beta = getattr(learner, 'beta', 1.0)
        if beta != 1.0:
            raise ValueError("DeviceDataset runs the Kullback-Leibler cost only: this learner has beta = %g; call its own train / "
                             "reconstruct_internal_multi on host matrices" % beta)


class _ProblemOf(object):
    """Problem p of a `_native.Batch` with a context's upload methods: what `DeviceDataset._sparse_uploader`'s upload calls."""

    def __init__(self, batch, p):
        self.batch, self.p = batch, p

    def upload_csr_device_rows(self, *args):
        self.batch.upload_csr_device_rows(self.p, *args)


def check_presence(presence, n_samples, n_modalities):
    """`presence` of `DeviceDataset` as it is kept: (P, masked) -- P the float64 [n_samples, n_modalities] mask, the column of a
    modality without an array all 1, and masked[m] whether modality m came with an array; (None, [False ...]) where no entry is
    an array (None and scalars: weights of 1, as `nmf.check_weights` reads them).  ValueError, before anything is uploaded: not
    one entry per modality, an array that is not of shape (n_samples,) or (n_samples, 1), negative or non-finite values
    (`nmf.check_weights`), more than `_native.MAX_MODALITIES` modalities under a mask."""
    none = [False] * n_modalities
    if presence is None:
        return None, none
    presence = list(presence)
    if len(presence) != n_modalities:
        raise ValueError("presence: one entry per modality expected (%d modalities, %d entries)" % (n_modalities, len(presence)))
    P, masked = np.ones((n_samples, n_modalities), dtype=np.float64), list(none)
    for m, p in enumerate(presence):
        if p is None or np.ndim(p) == 0:
            continue
        a = np.asarray(p)
        if a.shape not in ((n_samples,), (n_samples, 1)):
            raise ValueError("presence[%d] of shape %s: (%d,) or (%d, 1) expected" % (m, a.shape, n_samples, n_samples))
        P[:, m] = check_weights(a.reshape(n_samples, 1), (n_samples, 1))[:, 0]
        masked[m] = True
    if not any(masked):
        return None, none
    if n_modalities > _native.MAX_MODALITIES:
        raise ValueError("presence: a mask holds at most %d modalities, the dataset has %d" % (_native.MAX_MODALITIES, n_modalities))
    return P, masked


class _DeviceCsr(object):
    """One modality as CSR in device memory: int64 row pointers (also kept on the host), int32 column indices, values in the
    caller's type (float32 stays float32, everything else float64); sorted rows, no explicit zeros, no duplicates."""

    def __init__(self, m, to_device):
        dt = np.float32 if m.dtype == np.float32 else np.float64
        X = sp.csr_matrix(m, dtype=dt, copy=True) if sp.issparse(m) else sp.csr_matrix(np.asarray(m, dtype=dt))
        X.sum_duplicates()
        X.eliminate_zeros()
        X.sort_indices()
        assert X.shape[1] < 2 ** 31
        self.host = X
        self.f64 = dt == np.float64
        self.indptr = np.ascontiguousarray(X.indptr, dtype=np.int64)
        self.least = X.data.min() if X.nnz else None
        self.greatest = float(X.data.max()) if X.nnz else 0.0
        dev = to_device
        self.d_indptr = dev(self.indptr)
        # (at least one element each: a modality without stored entries still hands the library a valid pointer)
        self.d_indices = dev(np.ascontiguousarray(X.indices, dtype=np.int32) if X.nnz else np.zeros(1, dtype=np.int32))
        self.d_data = dev(np.ascontiguousarray(X.data, dtype=dt) if X.nnz else np.zeros(1, dtype=dt))

    def pointers(self):
        return self.d_indptr.data_ptr(), self.d_indices.data_ptr(), self.d_data.data_ptr(), self.f64

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.d_indptr, self.d_indices, self.d_data))


class DeviceDataset(object):
    """modalities: list of [n_samples, d_m] arrays (dense or scipy sparse), kept as fp32 on `device`.

    keep_sparse=True (and at least one scipy-sparse modality): sparse modalities stay CSR in device memory and are never
    densified; every modality then also has a CSR form there (dense ones converted once, here, and kept dense as well for
    subsets of dense modalities).  A fit or transform on modalities of which at least one is sparse runs the reference's sparse
    branch (the rule of `KLdivNMF._sparse_route` for host blocks) on a CSR problem gathered on the device
    (klnmf_upload_csr_device_rows); a subset of dense modalities runs the dense path as ever.  The default keeps every modality
    dense, as before.

    presence: None (no mask: every call is the unmasked one, as before), or a list with one entry per modality -- None, a scalar
    (both: that modality is present everywhere, no mask) or an array of shape (n_samples,) / (n_samples, 1) of weights >= 0: the
    weight of that modality in each sample, 0 where it is absent (`check_presence`: ValueError on the host).  The mask stays on
    the device as one float64 [n_samples, M] matrix.  A call (`train`, `reconstruct_internal_multi`, `DeviceEvaluation.internal`)
    whose modalities include one with an array gathers its rows of the mask on the device (klnmf_upload_presence_device_rows) and
    minimises the masked cost (csrc/presence.hip.h), in the arithmetic `nmf.weighted_precision` names, on the first device;
    `last_weights_route` then reads 'presence', on the dataset and on the model the call used.  A call on modalities without an
    array is the unmasked call, bit for bit (`last_weights_route` None).  A row from which every selected modality is absent keeps
    its W0 (a factor of 1 where the denominator is 0).  Scoring and the choice of rows stay the caller's.  A masked call that
    selects a modality kept as CSR raises ValueError: CSR problems have no masked kernels."""

    def __init__(self, data_matrices, device=None, keep_sparse=False, presence=None):
        import torch
        self.torch = torch
        self.device = torch.device('cuda', torch.cuda.current_device() if device is None else device)
        self.blocks = []
        self.maxima = []
        self.host = []           # the caller's matrices (for comparisons on the raw data, experiment.py:266: no transformation)
        mats = []
        for m in data_matrices:
            m = atleast2d_or_csr(m)
            check_non_negative(m, "NMF.fit")
            mats.append(m)
        self.keep_sparse_asked = bool(keep_sparse)
        self.keep_sparse = self.keep_sparse_asked and any(sp.issparse(m) for m in mats)
        self.sparse = [self.keep_sparse and sp.issparse(m) for m in mats]
        self.dims = [int(m.shape[1]) for m in mats]
        self.n_samples = int(mats[0].shape[0])
        assert all(m.shape[0] == self.n_samples for m in mats)
        self.presence_host, self.masked = check_presence(presence, self.n_samples, len(mats))      # (before anything is uploaded)
        self.last_weights_route = None      # set by every call: 'presence' where it ran the masked loop
        self.csr = [_DeviceCsr(m, self._to_device) for m in mats] if self.keep_sparse else [None] * len(mats)
        for m, kept, c in zip(mats, self.sparse, self.csr):
            if kept:             # CSR only: no dense copy on either side
                self.host.append(c.host)
                self.blocks.append(None)
                self.maxima.append(c.greatest)
                continue
            if hasattr(m, 'toarray'):
                m = m.toarray()
            self.host.append(np.asarray(m))
            t = self._to_device(np.ascontiguousarray(m, dtype=np.float32))
            self.blocks.append(t)
            self.maxima.append(float(t.max().item()) if t.numel() else 0.0)
        self._blocks64 = {}
        self.presence = None if self.presence_host is None else self._to_device(self.presence_host)      # float64 [n_samples, M]

    def _to_device(self, array):
        """A host array as a tensor on `device` (the one place the uploads touch torch: tests replace it)."""
        return self.torch.from_numpy(array).to(self.device)

    def _synchronize(self):
        self.torch.cuda.synchronize(self.device)

    def resident_bytes(self):
        """Device bytes the modalities take as stored now (dense fp32 blocks, fp64 copies made so far, CSR arrays, the mask)."""
        total = sum(b.numel() * b.element_size() for b in self.blocks if b is not None)
        total += sum(b.numel() * b.element_size() for b in self._blocks64.values())
        total += 0 if self.presence is None else self.presence.numel() * self.presence.element_size()
        return total + sum(c.nbytes() for c in self.csr if c is not None)

    def same_presence(self, presence):
        """`presence` (as the constructor takes it) is the mask this dataset was built with."""
        P, masked = check_presence(presence, self.n_samples, len(self.dims))
        if P is None or self.presence_host is None:
            return P is None and self.presence_host is None
        return masked == self.masked and np.array_equal(P, self.presence_host)

    def presence_route(self, which):
        """The modalities `which` run the masked loop: at least one of them came with a presence array.  ValueError where one
        of them is kept as CSR as well (the refusal of klnmf_upload_presence on a CSR problem, said on the host)."""
        if not any(self.masked[w] for w in which):
            return False
        if self.sparse_route(which):
            raise ValueError("a presence mask on modalities of which %s kept as CSR (keep_sparse=True): CSR problems have no masked "
                             "kernels; select dense modalities, or build the dataset without keep_sparse"
                             % ', '.join('%d is' % w for w in which if self.sparse[w]))
        return True

    def upload_presence(self, ctx, which, idx_ptr, n, p=None):
        """The rows of the mask for the modalities `which` into the problem of `ctx` (p: into problem p of a `_native.Batch`):
        gathered on the device by the row indices at `idx_ptr` (`n` int64 in device memory), column `w` of the resident mask for a
        masked modality w, 1 for the others; the bounds are the selected modalities' widths."""
        bounds = [0]
        for w in which:
            bounds.append(bounds[-1] + self.dims[w])
        args = (self.presence.data_ptr(), True, self.n_samples, self.presence.stride(0), idx_ptr, n,
                [w if self.masked[w] else -1 for w in which], bounds)
        if p is None:
            ctx.upload_presence_device_rows(*args)
        else:
            ctx.upload_presence_device_rows(p, *args)

    def sparse_route(self, which):
        """The modalities `which` run the sparse branch: at least one of them is kept as CSR (`KLdivNMF._sparse_route`)."""
        return any(self.sparse[w] for w in which)

    def _sparse_uploader(self, which, rows, coefs):
        """(upload, n, nnz, use_device) for the CSR problem of hstack([c * X_w[rows] ...]): `upload(ctx)` gathers it on the device
        into a problem set for (n, sum of the widths, nnz); use_device False: the call must take the host path (`csr_rows_plan`)."""
        rows = np.asarray(rows, dtype=np.int64)
        assert rows.size == 0 or (int(rows.min()) >= 0 and int(rows.max()) < self.n_samples)
        srcs = [self.csr[w] for w in which]
        nnz, use_device = csr_rows_plan([s.indptr for s in srcs], rows, coefs, [s.least for s in srcs])
        bounds = [0]
        for w in which:
            bounds.append(bounds[-1] + self.dims[w])
        idx = self._to_device(np.ascontiguousarray(rows))

        def upload(ctx):         # (synchronous: idx is free to go when it returns)
            ctx.upload_csr_device_rows([s.pointers() for s in srcs], bounds, [float(c) for c in coefs], self.n_samples,
                                       idx.data_ptr(), idx.numel())
        return upload, int(rows.size), nnz, use_device

    def _host_csr(self, which, rows, coefs):
        """The stacked CSR of the rows as the host path builds it (`nmf._csr_of` on host slices): where the device gather cannot
        reproduce the reference's dropped zeros.  Said once on stderr."""
        _note_once(('csr-device-rows-host',),
                   "DeviceDataset: a coefficient of 0, or one that rounds a stored value to 0: the reference drops such entries "
                   "(nmf.py:66), so this call slices the CSR rows on the host instead of gathering them on the device\n")
        rows = np.asarray(rows, dtype=np.int64)
        return _csr_of([self.host[w][rows] for w in which], coefs)

    def _fit_sparse(self, nmf, which, rows, coefs, _fit):
        upload, n, nnz, use_device = self._sparse_uploader(which, rows, coefs)
        out_dtype_of = self._sparse_out_dtype(which)
        if use_device:
            return nmf._fit_uploaded(n, sum(self.dims[w] for w in which), upload, out_dtype_of, _fit=_fit, sparse_nnz=nnz)
        X = self._host_csr(which, rows, coefs)
        return nmf._fit_uploaded(X.shape[0], X.shape[1], None, out_dtype_of, _fit=_fit, sparse_X=X)

    def source(self, which, precision=None):
        """(device matrix, is_float64) the fits and transforms read modality `which` from: the float64 copy when the NMF runs
        in the reference's own arithmetic (f64: results then agree with the reference to summation order), the float32 one
        otherwise (the 16-bit modes store V in 16 bits anyway).  `precision`: what the context that reads it resolved to
        (`Context.precision_name`); None: the process default."""
        if self.sparse[which]:
            raise ValueError("modality %d is kept as CSR (keep_sparse=True): it has no dense device copy" % which)
        if precision is None:
            precision = _default_precision()
        if precision == 'auto' or _native.PRECISIONS[precision] == _native.PREC_F64:
            return self.block64(which), True           # ('auto' decides per fit: the float64 copy serves either outcome)
        return self.blocks[which], False

    def block64(self, which):
        """float64 device copy of modality `which` (made on first use): the evaluation compares raw rows with
        reconstructions in the caller's own precision (experiment.py:266)."""
        if self.sparse[which]:
            raise ValueError("modality %d is kept as CSR (keep_sparse=True): it has no dense device copy" % which)
        if which not in self._blocks64:
            self._blocks64[which] = self._to_device(np.ascontiguousarray(self.host[which], dtype=np.float64))
        return self._blocks64[which]

    def _uploader(self, which, rows, coefs, masked=False):
        """(upload, n): `upload(ctx)` places the rows of the dense modalities `which` in the problem of `ctx`; masked: and their
        rows of the presence mask behind them (`upload_presence`)."""
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        assert rows.size == 0 or (int(rows.min()) >= 0 and int(rows.max()) < self.n_samples)
        idx = self._to_device(rows)

        def upload(ctx):
            # an upper bound of the stacked maximum fixes the 16-bit storage factor (any bound is valid)
            ctx.set_v_max(max([c * self.maxima[w] for w, c in zip(which, coefs)] + [0.0]))
            col = 0
            for w, c in zip(which, coefs):
                b, f64 = self.source(w, getattr(ctx, 'precision_name', None))
                ctx.upload_V_device_rows_dt(b.data_ptr(), f64, idx.data_ptr(), idx.numel(), b.shape[1], b.stride(0),
                                            row0=0, col0=col, scale=c)
                col += b.shape[1]
            if masked:
                self.upload_presence(ctx, which, idx.data_ptr(), idx.numel())
            self._synchronize()      # the context runs on its own stream; idx must outlive the kernel
        return upload, idx.numel()

    def _fit_dense(self, nmf, which, rows, coefs, n_features, _fit, return_errors=False):
        """The loop on the rows of dense modalities: the masked one where `presence_route` says so."""
        masked = self.presence_route(which)
        upload, n = self._uploader(which, rows, coefs, masked)
        out = nmf._fit_uploaded(n, n_features, upload, lambda H: np.float64, _fit=_fit, return_errors=return_errors, weighted=masked)
        self.last_weights_route = nmf.last_weights_route = 'presence' if masked else None
        return out

    # ---- what experiment.py:_perform_one_run does with the sliced copies ----
    def rows_of(self, which, rows):
        """Host rows of modality `which` as the caller gave them (what experiment.py compares raw data with)."""
        if self.sparse[which]:
            return np.asarray(self.host[which][np.asarray(rows, dtype=np.int64)].toarray())
        return self.host[which][np.asarray(rows, dtype=np.int64), :]

    def train(self, learner, rows, iterations, init_dictionary=None):
        """learner.train([x[rows] for x in data], iterations) (learner.py:31-41) without the host slices.
        `init_dictionary`: the initial dictionary instead of a draw from the global numpy stream (nmf.py:149-155).
        With a presence mask on the dataset: learner.train(..., weights=[P_m[rows] ...]), `learner.nmf_train.last_weights_route`
        'presence'.  A row in which every modality is absent keeps its W0 and gives the dictionary nothing."""
        refuse_beta(learner)
        if learner.sparseness is not None:
            raise NotImplemented
        which = list(range(len(self.blocks)))
        assert self.dims == list(learner.dim)
        nmf = KLdivNMF(n_components=learner.k, max_iter=iterations, tol=0)
        if init_dictionary is not None:
            nmf._init_dictionary = np.asarray(init_dictionary)
        if not self.presence_route(which) and self.sparse_route(which):
            self.last_weights_route = None
            self._fit_sparse(nmf, which, rows, list(learner.coef), True)
        else:
            self._fit_dense(nmf, which, rows, list(learner.coef), sum(learner.dim), True)
        learner.nmf_train = nmf
        learner.dico = nmf.components_
        return learner

    def reconstruct_internal_multi(self, learner, orig_mods, rows, iterations):
        """learner.reconstruct_internal_multi(orig_mods, [x[rows] ...], iterations) (learner.py:71-78).  Where one of `orig_mods`
        has a presence array: ... with weights=[P_m[rows] ...], the masked transform -- over all modalities it uses in every row
        whatever that row has; a row from which every selected modality is absent keeps its W0 = x . dico^T (factor 1 where the
        denominator is 0).  `self.last_weights_route` names the route."""
        refuse_beta(learner)
        which = [learner.get_index(m) for m in orig_mods]
        coefs = [learner.coef[w] for w in which]
        dico = learner.get_stacked_dicos(orig_mods)
        nmf = KLdivNMF(n_components=dico.shape[0], max_iter=iterations, tol=0)
        nmf.components_ = dico
        nmf._init_dictionary = dico
        if not self.presence_route(which) and self.sparse_route(which):
            self.last_weights_route = None
            return self._fit_sparse(nmf, which, rows, coefs, False)
        return self._fit_dense(nmf, which, rows, coefs, dico.shape[1], False)

    def reconstruct_internal(self, learner, orig_mod, rows, iterations):
        return self.reconstruct_internal_multi(learner, [orig_mod], rows, iterations)

    # ---- the same calls for the runs of a sweep that share a shape: one batch (klnmf_batch_*, csrc/batch.hip.h) ----
    def _batch_uploads(self, which, rows_list, coefs_list, masked=False):
        """One `upload(batch, p)` per row list: the rows of the dense modalities `which` into problem p of a `_native.Batch`;
        masked: and problem p's rows of the resident presence mask behind them (`upload_presence`)."""
        uploads = []
        for rows, coefs in zip(rows_list, coefs_list):
            rows = np.ascontiguousarray(rows, dtype=np.int64)
            assert rows.size == 0 or (int(rows.min()) >= 0 and int(rows.max()) < self.n_samples)
            idx = self._to_device(rows)

            def upload(batch, p, idx=idx, coefs=coefs):
                col = 0
                for w, c in zip(which, coefs):
                    b, f64 = self.source(w, batch.precision_name)
                    batch.upload_V_device_rows_dt(p, b.data_ptr(), f64, idx.data_ptr(), idx.numel(), b.shape[1], b.stride(0),
                                                  row0=0, col0=col, scale=c)
                    col += b.shape[1]
                if masked:
                    self.upload_presence(batch, which, idx.data_ptr(), idx.numel(), p=p)
                self._synchronize()      # the batch runs on its own stream; idx must outlive the kernel
            uploads.append(upload)
        return uploads

    def _batch_route(self, which, rows_list, nmfs, n_features):
        """'f64' / 'f32' if the calls on `rows_list` can run as one batch: row lists of one length, dense modalities -- masked ones
        included: the batch is then the masked one, `presence_route(which)`, in `weighted_precision`'s arithmetic as the single masked
        call -- and models that `batch_precision` accepts.  None: the loop over the single calls.  ValueError for a masked
        selection that includes a CSR modality (`presence_route`)."""
        if not nmfs or len(set(len(r) for r in rows_list)) != 1:
            return None
        masked = self.presence_route(which)
        if self.sparse_route(which):
            return None
        return batch_precision(nmfs, len(rows_list[0]), n_features, weighted=masked)

    def _batch_route_sparse(self, which, rows_list, coefs_list, nmfs, n_features):
        """(precision, uploads, nnzs) if the calls on `rows_list` can run as one CSR batch (klnmf_batch_csr.h): the selection runs
        the sparse branch without a mask, the row lists have one length, every problem's `csr_rows_plan` allows the device gather
        and finds stored entries, and the models are as `batch_precision(sparse=True)` asks (k <= 512 among it).  uploads[p](batch, p)
        gathers problem p on the device (`Batch.upload_csr_device_rows`).  None: the loop over the single calls -- ONE problem that
        needs the host path (a coefficient of 0) sends the whole call there.  ValueError for a masked selection that includes a
        CSR modality (`presence_route`)."""
        if not nmfs or len(set(len(r) for r in rows_list)) != 1:
            return None
        if self.presence_route(which) or not self.sparse_route(which):
            return None
        prec = batch_precision(nmfs, len(rows_list[0]), n_features, sparse=True)
        if prec is None:
            return None
        uploads, nnzs = [], []
        for rows, coefs in zip(rows_list, coefs_list):
            upload, _, nnz, use_device = self._sparse_uploader(which, rows, coefs)
            if not use_device or nnz == 0:
                return None
            uploads.append(lambda batch, p, upload=upload: upload(_ProblemOf(batch, p)))
            nnzs.append(nnz)
        return prec, uploads, nnzs

    def _sparse_out_dtype(self, which):
        all32 = all(not self.csr[w].f64 for w in which)
        return lambda H: np.float32 if (all32 and H.dtype == np.float32) else np.float64      # (as `_fit_blocks` on CSR)

    def train_many(self, learners, rows_list, iterations, init_dictionaries=None):
        """[self.train(l, rows, iterations, init) for l, rows, init in ...] -- as ONE batch where all row lists have one length and
        all learners share k: the dense batch, or where a modality is kept as CSR the CSR batch (`_batch_route_sparse`); the loop
        over `train` otherwise.  With a presence mask on the
        dataset the batch is the masked one: `last_weights_route` 'presence' here and on every `learner.nmf_train`."""
        learners, rows_list = list(learners), [list(r) for r in rows_list]
        refuse_beta(*learners)
        inits = list(init_dictionaries) if init_dictionaries is not None else [None] * len(learners)
        which = list(range(len(self.blocks)))
        nmfs = []
        for learner, init in zip(learners, inits):
            nmf = KLdivNMF(n_components=learner.k, max_iter=iterations, tol=0)
            if init is not None:
                nmf._init_dictionary = np.asarray(init)
            nmfs.append(nmf)
        plain = all(l.sparseness is None and self.dims == list(l.dim) for l in learners)
        prec = self._batch_route(which, rows_list, nmfs, sum(self.dims)) if plain else None
        csr = self._batch_route_sparse(which, rows_list, [list(l.coef) for l in learners], nmfs, sum(self.dims)) \
            if plain and prec is None else None
        if csr is not None:
            fit_uploaded_batch(nmfs, csr[0], len(rows_list[0]), sum(self.dims), csr[1], [self._sparse_out_dtype(which)] * len(nmfs),
                               _fit=True, sparse_nnzs=csr[2])
            self.last_weights_route = None
            for learner, nmf in zip(learners, nmfs):
                learner.nmf_train = nmf
                learner.dico = nmf.components_
            return learners
        if prec is None:
            return [self.train(l, rows, iterations, init_dictionary=init) for l, rows, init in zip(learners, rows_list, inits)]
        masked = self.presence_route(which)
        uploads = self._batch_uploads(which, rows_list, [list(l.coef) for l in learners], masked)
        fit_uploaded_batch(nmfs, prec, len(rows_list[0]), sum(self.dims), uploads, [lambda H: np.float64] * len(nmfs), _fit=True,
                           masked=masked)
        self.last_weights_route = 'presence' if masked else None
        for learner, nmf in zip(learners, nmfs):
            learner.nmf_train = nmf
            learner.dico = nmf.components_
        return learners

    def reconstruct_internal_multi_many(self, learners, orig_mods, rows_list, iterations):
        """[self.reconstruct_internal_multi(l, orig_mods, rows, iterations) for l, rows in ...] -- as one batch under
        `train_many`'s conditions (here: on the selected modalities)."""
        learners, rows_list = list(learners), [list(r) for r in rows_list]
        refuse_beta(*learners)
        if not learners:
            return []
        which = [learners[0].get_index(m) for m in orig_mods]
        nmfs = []
        for learner in learners:
            dico = learner.get_stacked_dicos(orig_mods)
            nmf = KLdivNMF(n_components=dico.shape[0], max_iter=iterations, tol=0)
            nmf.components_ = dico
            nmf._init_dictionary = dico
            nmfs.append(nmf)
        same = all([l.get_index(m) for m in orig_mods] == which and list(l.dim) == self.dims for l in learners)
        n_features = sum(self.dims[w] for w in which)
        prec = self._batch_route(which, rows_list, nmfs, n_features) if same else None
        csr = self._batch_route_sparse(which, rows_list, [[l.coef[w] for w in which] for l in learners], nmfs, n_features) \
            if same and prec is None else None
        if csr is not None:
            self.last_weights_route = None
            return fit_uploaded_batch(nmfs, csr[0], len(rows_list[0]), n_features, csr[1], [self._sparse_out_dtype(which)] * len(nmfs),
                                      _fit=False, sparse_nnzs=csr[2])
        if prec is None:
            return [self.reconstruct_internal_multi(l, orig_mods, rows, iterations) for l, rows in zip(learners, rows_list)]
        masked = self.presence_route(which)
        uploads = self._batch_uploads(which, rows_list, [[l.coef[w] for w in which] for l in learners], masked)
        out = fit_uploaded_batch(nmfs, prec, len(rows_list[0]), n_features, uploads, [lambda H: np.float64] * len(nmfs), _fit=False,
                                 masked=masked)
        self.last_weights_route = 'presence' if masked else None
        return out


class DeviceEvaluation(object):
    """What one run's evaluation needs of a trained learner, kept on the GPU (next-row N1; experiment.py:233-277, 332-371):

      * the dictionary is uploaded ONCE and every transform takes its column blocks from there (klnmf_set_H_device;
        get_dico / get_stacked_dicos, learner.py:43-51);
      * the test / example rows are gathered from the device-resident modalities by the upload kernel;
      * the coefficients stay on the device (klnmf_get_W_device), the reconstructions are products of device matrices
        (klnmf_matmul_device; learner.py:80-84), and the nearest-example search reads both sides from device memory
        (klnmf_all_distances_device) -- only the [n_test, n_examples] distance matrix comes back (`found_labels`), or, for
        many searches and all their measures in one launch, only the indices (`found_labels_many`, klnmf_nearest_many_device).

    All intermediates are float64 (as the host path's); the loop itself runs in the learner's NMF precision."""

    def __init__(self, dataset, learner, iter_test):
        import torch
        refuse_beta(learner)
        self.torch, self.ds, self.learner, self.iter_test = torch, dataset, learner, int(iter_test)
        self.dev = dataset.device
        self.dico = torch.from_numpy(np.ascontiguousarray(learner.get_dico(), dtype=np.float64)).to(self.dev)
        self.k, self.F = self.dico.shape
        self.offsets = [sum(learner.dim[:i]) for i in range(len(learner.dim))]
        self.last_weights_route = None      # set by every `internal`

    def _rows(self, rows):
        idx = self.torch.as_tensor(np.asarray(rows, dtype=np.int64), device=self.dev)
        assert idx.numel() == 0 or (int(idx.min()) >= 0 and int(idx.max()) < self.ds.n_samples)
        return idx

    def internal(self, mods, rows):
        """learner.reconstruct_internal_multi(mods, [x[rows] ...], iter_test) -> device tensor [len(rows), k].  Where one of
        `mods` has a presence array on the dataset, the masked transform (`DeviceDataset.reconstruct_internal_multi`):
        `self.last_weights_route` reads 'presence', None otherwise."""
        torch, lr = self.torch, self.learner
        which = [lr.get_index(m) for m in mods]
        idx = self._rows(rows)
        n, f = int(idx.numel()), sum(lr.dim[w] for w in which)
        out = torch.empty((n, self.k), dtype=torch.float64, device=self.dev)
        model = KLdivNMF(n_components=self.k, max_iter=self.iter_test, tol=0)
        masked = self.ds.presence_route(which)
        self.last_weights_route = model.last_weights_route = 'presence' if masked else None
        if self.ds.sparse_route(which):
            return self._internal_sparse(model, mods, which, rows, out)
        if masked:
            model._note_weighted_on_one_device()
        # (the shape decides the arithmetic exactly as the host path's _fit_uploaded does: 'auto' by size, k beyond the MFMA
        # kernels' range on the fp32 kernels)
        # (a masked transform: f64 or f32 as `weighted_precision` names them, first device -- `_fit_uploaded`'s choice)
        with model._context(shape=(n, f, self.k), weighted=masked) as ctx:
            ctx.set_problem(n, f, self.k, self.iter_test)
            ctx.set_v_max(max([lr.coef[w] * self.ds.maxima[w] for w in which] + [0.0]))
            col = 0
            for w in which:
                b, f64 = self.ds.source(w, getattr(ctx, 'precision_name', None))
                ctx.upload_V_device_rows_dt(b.data_ptr(), f64, idx.data_ptr(), n, b.shape[1], b.stride(0), row0=0, col0=col,
                                            scale=lr.coef[w])
                col += b.shape[1]
            if masked:
                self.ds.upload_presence(ctx, which, idx.data_ptr(), n)
            self._set_dictionary(ctx, which)
            ctx.init_W()                                   # W0 = X . H^T with the dictionary itself (nmf.py:156, 283)
            ctx.run(self.iter_test, False, 0.0)
            ctx.get_W_device(out.data_ptr(), True, self.k)
        torch.cuda.synchronize(self.dev)
        return out

    @staticmethod
    def internal_many(evaluations, mods, rows_list):
        """[ev.internal(mods, rows) for ev, rows in ...] for the evaluations of a sweep's runs -- as ONE batch where they share the
        dataset, k, the iteration count and the number of rows and the shape runs in f64 / f32 -- with a selected modality kept as
        CSR: the CSR batch, `DeviceDataset._batch_route_sparse` -- (a masked selection: the masked batch, `last_weights_route` 'presence' on every evaluation): the dictionaries go
        in by klnmf_batch_set_H_device, the coefficients stay on the device (klnmf_batch_get_W_device).  The loop over `internal`
        otherwise."""
        evaluations, rows_list = list(evaluations), list(rows_list)
        if not evaluations:
            return []
        first = evaluations[0]
        torch, ds, lr = first.torch, first.ds, first.learner
        which = [lr.get_index(m) for m in mods]
        models = [KLdivNMF(n_components=ev.k, max_iter=ev.iter_test, tol=0) for ev in evaluations]
        same = all(ev.ds is ds and list(ev.learner.dim) == list(lr.dim) and [ev.learner.get_index(m) for m in mods] == which
                   for ev in evaluations)
        n, f = len(rows_list[0]), sum(lr.dim[w] for w in which)
        prec = ds._batch_route(which, rows_list, models, f) if same else None
        csr = ds._batch_route_sparse(which, rows_list, [[ev.learner.coef[w] for w in which] for ev in evaluations], models, f) \
            if same and prec is None else None
        if csr is not None:      # the CSR batch: gathered on the device, dictionaries and coefficients as below
            outs = [torch.empty((n, ev.k), dtype=torch.float64, device=ev.dev) for ev in evaluations]
            with _native.Batch(csr[0], len(evaluations), device=models[0].device) as batch:
                batch.set_problem_sparse(n, f, first.k, first.iter_test, csr[2])
                for p, ev in enumerate(evaluations):
                    csr[1][p](batch, p)
                    ev._set_dictionary(batch, which, p)
                    ev.last_weights_route = models[p].last_weights_route = None
                batch.init_W()
                batch.run(first.iter_test, False, 0.0)
                for p, out in enumerate(outs):
                    batch.get_W_device(p, out.data_ptr(), True, first.k)
            torch.cuda.synchronize(first.dev)
            return outs
        if prec is None:
            return [ev.internal(mods, rows) for ev, rows in zip(evaluations, rows_list)]
        masked = ds.presence_route(which)
        idxs = [ev._rows(rows) for ev, rows in zip(evaluations, rows_list)]
        outs = [torch.empty((n, ev.k), dtype=torch.float64, device=ev.dev) for ev in evaluations]
        with _native.Batch(prec, len(evaluations), device=models[0].device) as batch:
            batch.set_problem(n, f, first.k, first.iter_test)
            for p, (ev, idx) in enumerate(zip(evaluations, idxs)):
                col = 0
                for w in which:
                    b, f64 = ds.source(w, batch.precision_name)
                    batch.upload_V_device_rows_dt(p, b.data_ptr(), f64, idx.data_ptr(), n, b.shape[1], b.stride(0), row0=0, col0=col,
                                                  scale=ev.learner.coef[w])
                    col += b.shape[1]
                if masked:
                    ds.upload_presence(batch, which, idx.data_ptr(), n, p=p)
                ev._set_dictionary(batch, which, p)
                ev.last_weights_route = models[p].last_weights_route = 'presence' if masked else None
            ds._synchronize()                              # the batch runs on its own stream; the indices must outlive the kernels
            batch.init_W()                                 # W0 = X . H^T with the dictionary itself (nmf.py:156, 283)
            batch.run(first.iter_test, False, 0.0)
            for p, out in enumerate(outs):
                batch.get_W_device(p, out.data_ptr(), True, first.k)
        torch.cuda.synchronize(first.dev)
        return outs

    def _set_dictionary(self, ctx, which, p=None):
        """The stacked dictionary of the modalities `which` into `ctx` (p: into problem p of a `_native.Batch`)."""
        put = ctx.set_H_device if p is None else (lambda *a, **kw: ctx.set_H_device(p, *a, **kw))
        col = 0
        for i, w in enumerate(which):                      # the stacked dictionary of these modalities, block by block
            d = self.learner.dim[w]
            put(self.dico.data_ptr() + 8 * self.offsets[w], True, self.F, col, d, last=(i == len(which) - 1))
            col += d

    def _internal_sparse(self, model, mods, which, rows, out):
        """`internal` where a selected modality is kept as CSR: the reference's sparse branch on a CSR problem gathered on the
        device (the host path, uploaded, where `csr_rows_plan` says the gather cannot reproduce it)."""
        lr = self.learner
        upload, n, nnz, use_device = self.ds._sparse_uploader(which, rows, [lr.coef[w] for w in which])
        if not use_device:
            W = self.ds.reconstruct_internal_multi(lr, mods, rows, self.iter_test)
            return self.torch.from_numpy(np.ascontiguousarray(W, dtype=np.float64)).to(self.dev)
        with model._context(sparse=True) as ctx:
            ctx.set_problem_sparse_shape(n, sum(lr.dim[w] for w in which), self.k, self.iter_test, nnz)
            upload(ctx)
            self._set_dictionary(ctx, which)
            ctx.init_W()
            ctx.run(self.iter_test, False, 0.0)
            ctx.get_W_device(out.data_ptr(), True, self.k)
        self.torch.cuda.synchronize(self.dev)
        return out

    def reconstruct(self, internal, dest_mod):
        """learner.reconstruct_modality(dest_mod, internal) (learner.py:80-81) between device matrices."""
        w = self.learner.get_index(dest_mod)
        d = self.learner.dim[w]
        out = self.torch.empty((internal.shape[0], d), dtype=self.torch.float64, device=self.dev)
        _native.matmul_device(internal.data_ptr(), internal.stride(0), self.dico.data_ptr() + 8 * self.offsets[w], self.F,
                              out.data_ptr(), d, internal.shape[0], d, self.k, f64=True, device=self.dev.index or 0)
        return out

    def raw(self, which, rows):
        """The rows of modality `which` as the experiment compares raw data (float64 device copy of the caller's matrix)."""
        if self.ds.sparse[which]:      # densified on the device, these rows only (klnmf_csr_rows_to_dense_device)
            idx, c, d = self._rows(rows), self.ds.csr[which], self.ds.dims[which]
            out = self.torch.empty((int(idx.numel()), d), dtype=self.torch.float64, device=self.dev)
            _native.csr_rows_to_dense_device(*(c.pointers() + (self.ds.n_samples, idx.data_ptr(), int(idx.numel()), d,
                                                               out.data_ptr(), d)), device=self.dev.index or 0)
            return out
        return self.ds.block64(which).index_select(0, self._rows(rows))

    def found_labels(self, test, examples, labels_ex, metric):
        """classify_NN (evaluation.py:109-116): nearest example's label for every row of `test` -- both on the device."""
        out = self.torch.empty((test.shape[0], examples.shape[0]), dtype=self.torch.float64, device=self.dev)
        _native.all_distances_device(test.data_ptr(), test.stride(0), examples.data_ptr(), examples.stride(0), out.data_ptr(),
                                     test.shape[0], examples.shape[0], test.shape[1], metric, f64=True,
                                     device=self.dev.index or 0)
        nearest = np.argmin(out.cpu().numpy(), axis=1)
        return [labels_ex[j] for j in nearest]

    def found_labels_many(self, searches, metrics):
        """[{metric: found_labels(test, examples, labels_ex, metric)} for (test, examples, labels_ex) in searches] -- float64
        device matrices of any shapes on this evaluation's device, of this run or of several -- by ONE launch
        (klnmf_nearest_many_device) and one copy of the int32 indices: the distance matrices are never formed."""
        torch = self.torch
        searches, metrics = list(searches), [int(m) for m in metrics]
        mask = _native.metric_mask(metrics)
        slot = {m: s for s, m in enumerate(_native.mask_metrics(mask))}
        for test, examples, _labels in searches:
            if test.dtype != torch.float64 or examples.dtype != torch.float64 or test.shape[1] != examples.shape[1]:
                raise ValueError("found_labels_many: float64 matrices of one row length, got %s %s and %s %s"
                                 % (test.dtype, tuple(test.shape), examples.dtype, tuple(examples.shape)))
        jobs = [(t.data_ptr(), t.stride(0), e.data_ptr(), e.stride(0), t.shape[0], e.shape[0], t.shape[1]) for t, e, _l in searches]
        rows = sum(j[4] for j in jobs)
        nbytes = _native.nearest_work_bytes(len(jobs), rows)
        idx = torch.empty((rows, len(slot)), dtype=torch.int32, device=self.dev)
        work = torch.empty((max(1, nbytes),), dtype=torch.uint8, device=self.dev)
        _native.nearest_many_device(jobs, mask, idx.data_ptr(), None, work.data_ptr(), nbytes, f64=True, device=self.dev.index or 0)
        nearest = idx.cpu().numpy()
        out, row0 = [], 0
        for (test, _examples, labels_ex) in searches:
            mine = nearest[row0:row0 + test.shape[0]]
            out.append({m: [labels_ex[j] for j in mine[:, slot[m]]] for m in metrics})
            row0 += test.shape[0]
        return out

    def information_matrix(self, mods, rows, labels, n_labels, bins=10):
        """evaluation.information_matrix(self.internal(mods, rows), labels, n_labels, bins) with the coefficients left on the
        device: the (n_labels, k) float64 matrix alone comes back (klnmf_information_many_device; the reference's
        samples/plot_info_matrix.py:126-136 for one run)."""
        return DeviceEvaluation.information_matrix_many([self], mods, [rows], [labels], n_labels, bins=bins)[0]

    @staticmethod
    def information_matrix_many(evaluations, mods, rows_list, labels_list, n_labels, bins=10):
        """[ev.information_matrix(mods, rows, labels, n_labels, bins) for ...] for the evaluations of several runs on one device
        (the loop over N_RUN of samples/plot_info_matrix.py:106-136): the internals by `internal_many`, then ONE
        klnmf_information_many_device call for all runs and one copy of the matrices."""
        from .evaluation import checked_labels
        evaluations, rows_list = list(evaluations), [list(rows) for rows in rows_list]
        if not evaluations:
            return []
        first = evaluations[0]
        torch, dev = first.torch, first.dev
        if not 1 <= int(bins) <= 256:
            raise ValueError("bins must lie in [1, 256], got %r" % (bins,))
        checked = [checked_labels(labels, len(rows), n_labels)[0] for labels, rows in zip(labels_list, rows_list)]
        if len(checked) != len(evaluations) or len(rows_list) != len(evaluations):
            raise ValueError("one list of rows and one of labels per evaluation")
        internals = type(first).internal_many(evaluations, mods, rows_list)
        d_labels = [torch.from_numpy(np.ascontiguousarray(l)).to(dev) for l in checked]
        jobs = [(t.data_ptr(), t.stride(0), l.data_ptr(), t.shape[0], t.shape[1]) for t, l in zip(internals, d_labels)]
        atoms = sum(j[4] for j in jobs)
        nbytes = _native.information_work_bytes(len(jobs), atoms, n_labels, bins)
        info = torch.empty((atoms * int(n_labels),), dtype=torch.float64, device=dev)
        work = torch.empty((max(1, nbytes),), dtype=torch.uint8, device=dev)
        _native.information_many_device(jobs, n_labels, bins, info.data_ptr(), None, work.data_ptr(), nbytes, f64=True,
                                        device=dev.index or 0)
        flat = info.cpu().numpy()
        out, at = [], 0
        for t in internals:
            out.append(flat[at:at + int(n_labels) * t.shape[1]].reshape(int(n_labels), t.shape[1]).copy())
            at += int(n_labels) * t.shape[1]
        return out
