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
"""
import numpy as np
import scipy.sparse as sp

from . import _native
from .lib.nmf import KLdivNMF, check_non_negative, _default_precision, resolve_precision, _csr_of, _note_once
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
    dense, as before."""

    def __init__(self, data_matrices, device=None, keep_sparse=False):
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
            t = torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)).to(self.device)
            self.blocks.append(t)
            self.maxima.append(float(t.max().item()) if t.numel() else 0.0)
        self.n_samples = int(mats[0].shape[0])
        assert all(m.shape[0] == self.n_samples for m in mats)
        self._blocks64 = {}

    def _to_device(self, array):
        """A host array of the CSR path as a tensor on `device` (the one place that path touches torch: tests replace it)."""
        return self.torch.from_numpy(array).to(self.device)

    def resident_bytes(self):
        """Device bytes the modalities take as stored now (dense fp32 blocks, fp64 copies made so far, CSR arrays)."""
        total = sum(b.numel() * b.element_size() for b in self.blocks if b is not None)
        total += sum(b.numel() * b.element_size() for b in self._blocks64.values())
        return total + sum(c.nbytes() for c in self.csr if c is not None)

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
        all32 = all(not self.csr[w].f64 for w in which)
        out_dtype_of = lambda H: np.float32 if (all32 and H.dtype == np.float32) else np.float64      # (as `_fit_blocks` on CSR)
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
            self._blocks64[which] = self.torch.from_numpy(np.ascontiguousarray(self.host[which], dtype=np.float64)).to(self.device)
        return self._blocks64[which]

    def _uploader(self, which, rows, coefs):
        torch = self.torch
        idx = torch.as_tensor(np.asarray(rows, dtype=np.int64), device=self.device)
        assert idx.numel() == 0 or (int(idx.min()) >= 0 and int(idx.max()) < self.n_samples)

        def upload(ctx):
            # an upper bound of the stacked maximum fixes the 16-bit storage factor (any bound is valid)
            ctx.set_v_max(max([c * self.maxima[w] for w, c in zip(which, coefs)] + [0.0]))
            col = 0
            for w, c in zip(which, coefs):
                b, f64 = self.source(w, getattr(ctx, 'precision_name', None))
                ctx.upload_V_device_rows_dt(b.data_ptr(), f64, idx.data_ptr(), idx.numel(), b.shape[1], b.stride(0),
                                            row0=0, col0=col, scale=c)
                col += b.shape[1]
            torch.cuda.synchronize(self.device)      # the context runs on its own stream; idx must outlive the kernel
        return upload, idx.numel()

    # ---- what experiment.py:_perform_one_run does with the sliced copies ----
    def rows_of(self, which, rows):
        """Host rows of modality `which` as the caller gave them (what experiment.py compares raw data with)."""
        if self.sparse[which]:
            return np.asarray(self.host[which][np.asarray(rows, dtype=np.int64)].toarray())
        return self.host[which][np.asarray(rows, dtype=np.int64), :]

    def train(self, learner, rows, iterations, init_dictionary=None):
        """learner.train([x[rows] for x in data], iterations) (learner.py:31-41) without the host slices.
        `init_dictionary`: the initial dictionary instead of a draw from the global numpy stream (nmf.py:149-155)."""
        if learner.sparseness is not None:
            raise NotImplemented
        which = list(range(len(self.blocks)))
        assert self.dims == list(learner.dim)
        nmf = KLdivNMF(n_components=learner.k, max_iter=iterations, tol=0)
        if init_dictionary is not None:
            nmf._init_dictionary = np.asarray(init_dictionary)
        if self.sparse_route(which):
            self._fit_sparse(nmf, which, rows, list(learner.coef), True)
        else:
            upload, n = self._uploader(which, rows, list(learner.coef))
            nmf._fit_uploaded(n, sum(learner.dim), upload, lambda H: np.float64, _fit=True)
        learner.nmf_train = nmf
        learner.dico = nmf.components_
        return learner

    def reconstruct_internal_multi(self, learner, orig_mods, rows, iterations):
        """learner.reconstruct_internal_multi(orig_mods, [x[rows] ...], iterations) (learner.py:71-78)."""
        which = [learner.get_index(m) for m in orig_mods]
        coefs = [learner.coef[w] for w in which]
        dico = learner.get_stacked_dicos(orig_mods)
        nmf = KLdivNMF(n_components=dico.shape[0], max_iter=iterations, tol=0)
        nmf.components_ = dico
        nmf._init_dictionary = dico
        if self.sparse_route(which):
            return self._fit_sparse(nmf, which, rows, coefs, False)
        upload, n = self._uploader(which, rows, coefs)
        return nmf._fit_uploaded(n, dico.shape[1], upload, lambda H: np.float64, _fit=False)

    def reconstruct_internal(self, learner, orig_mod, rows, iterations):
        return self.reconstruct_internal_multi(learner, [orig_mod], rows, iterations)


class DeviceEvaluation(object):
    """What one run's evaluation needs of a trained learner, kept on the GPU (next-row N1; experiment.py:233-277, 332-371):

      * the dictionary is uploaded ONCE and every transform takes its column blocks from there (klnmf_set_H_device;
        get_dico / get_stacked_dicos, learner.py:43-51);
      * the test / example rows are gathered from the device-resident modalities by the upload kernel;
      * the coefficients stay on the device (klnmf_get_W_device), the reconstructions are products of device matrices
        (klnmf_matmul_device; learner.py:80-84), and the nearest-example search reads both sides from device memory
        (klnmf_all_distances_device) -- only the [n_test, n_examples] distance matrix comes back.

    All intermediates are float64 (as the host path's); the loop itself runs in the learner's NMF precision."""

    def __init__(self, dataset, learner, iter_test):
        import torch
        self.torch, self.ds, self.learner, self.iter_test = torch, dataset, learner, int(iter_test)
        self.dev = dataset.device
        self.dico = torch.from_numpy(np.ascontiguousarray(learner.get_dico(), dtype=np.float64)).to(self.dev)
        self.k, self.F = self.dico.shape
        self.offsets = [sum(learner.dim[:i]) for i in range(len(learner.dim))]

    def _rows(self, rows):
        idx = self.torch.as_tensor(np.asarray(rows, dtype=np.int64), device=self.dev)
        assert idx.numel() == 0 or (int(idx.min()) >= 0 and int(idx.max()) < self.ds.n_samples)
        return idx

    def internal(self, mods, rows):
        """learner.reconstruct_internal_multi(mods, [x[rows] ...], iter_test) -> device tensor [len(rows), k]."""
        torch, lr = self.torch, self.learner
        which = [lr.get_index(m) for m in mods]
        idx = self._rows(rows)
        n, f = int(idx.numel()), sum(lr.dim[w] for w in which)
        out = torch.empty((n, self.k), dtype=torch.float64, device=self.dev)
        model = KLdivNMF(n_components=self.k, max_iter=self.iter_test, tol=0)
        if self.ds.sparse_route(which):
            return self._internal_sparse(model, mods, which, rows, out)
        # (the shape decides the arithmetic exactly as the host path's _fit_uploaded does: 'auto' by size, k beyond the MFMA
        # kernels' range on the fp32 kernels)
        with model._context(shape=(n, f, self.k)) as ctx:
            ctx.set_problem(n, f, self.k, self.iter_test)
            ctx.set_v_max(max([lr.coef[w] * self.ds.maxima[w] for w in which] + [0.0]))
            col = 0
            for w in which:
                b, f64 = self.ds.source(w, getattr(ctx, 'precision_name', None))
                ctx.upload_V_device_rows_dt(b.data_ptr(), f64, idx.data_ptr(), n, b.shape[1], b.stride(0), row0=0, col0=col,
                                            scale=lr.coef[w])
                col += b.shape[1]
            self._set_dictionary(ctx, which)
            ctx.init_W()                                   # W0 = X . H^T with the dictionary itself (nmf.py:156, 283)
            ctx.run(self.iter_test, False, 0.0)
            ctx.get_W_device(out.data_ptr(), True, self.k)
        torch.cuda.synchronize(self.dev)
        return out

    def _set_dictionary(self, ctx, which):
        col = 0
        for i, w in enumerate(which):                      # the stacked dictionary of these modalities, block by block
            d = self.learner.dim[w]
            ctx.set_H_device(self.dico.data_ptr() + 8 * self.offsets[w], True, self.F, col, d, last=(i == len(which) - 1))
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
