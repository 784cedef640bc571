"""CSR test matrices with prescribed cell counts, and a chunked fp64 restatement of the reference's sparse branch.

The blocked CSR kernels (multimodal_amd/csrc/sparseb.hip.h) walk the stored entries per (row, column block) cell in trips
of 32 (k <= 64 and k > 128) or 16 (65 <= k <= 128) entries, and per (column, row block) cell in trips of 64 entries taken
in groups of 16.  `designed_csr` builds matrices whose cells hit the edges of those trips; `cell_counts` measures what a
matrix actually holds, so that a test checks its coverage instead of assuming it.

`ref_step` / `ref_fit` are the oracle's CSR branch (oracle/klnmf_oracle.py, nmf.py:52-70, 301-308, 331-334) in fp64.  For
large problems they form W.H on the stored entries in chunks: `orc.sparse_wh` builds an nnz x k array at once.
tests/test_sparse_cpu.py pins the chunked form to the oracle.
"""
import numpy as np
import scipy.sparse as sp

from oracle import klnmf_oracle as orc

# entries per (row, column block): both trip sizes (NB = 32 and 16), one past and one short of each, and more than two trips
ROW_CELLS = (0, 1, 15, 16, 17, 31, 32, 33, 65)
# entries per (column, row block): k_spb_n's groups of 16 and trips of 64
COL_CELLS = (0, 1, 15, 16, 17, 63, 64, 65)

# at or below this many products of W.H on the stored entries the oracle itself is the reference
ORACLE_MAX_PRODUCTS = 1 << 22


def block_width(extent, blocks):
    """Columns (rows) per block of the CSR kernels: ceil(extent / blocks), as the library cuts them."""
    return -(-int(extent) // int(blocks))


def cell_counts(X, cb, rb):
    """(set of entries per (row, column block), set of entries per (column, row block)) of CSR X cut into cb column blocks
    of ceil(f / cb) columns and rb row blocks of ceil(n / rb) rows."""
    X = sp.csr_matrix(X)
    n, f = X.shape
    wc, wr = block_width(f, cb), block_width(n, rb)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(X.indptr))
    cols = X.indices.astype(np.int64)
    row_cells = np.bincount(rows * cb + cols // wc, minlength=n * cb)
    col_cells = np.bincount(cols * rb + rows // wr, minlength=f * rb)
    return set(row_cells.tolist()), set(col_cells.tolist())


def row_lengths(X):
    return np.diff(sp.csr_matrix(X).indptr)


def designed_csr(n, f, cb, rb, seed, dtype=np.float64):
    """CSR X (n x f, sorted, positive values) whose cells cover ROW_CELLS and COL_CELLS for cb column blocks and rb row blocks.

    Even rows hold entries in even columns only: their (row, column block) cells cycle through ROW_CELLS, every 10th
    even row is empty and every 11th holds a single entry.  Odd columns hold entries in odd rows only: their (column,
    row block) cells cycle through COL_CELLS.  So neither side's counts disturb the other's.  Every block needs at least
    max(cells) rows / columns of its parity: blocks at least 131 wide."""
    rng = np.random.default_rng(seed)
    wc, wr = block_width(f, cb), block_width(n, rb)
    ii, jj = [], []
    L = len(ROW_CELLS)
    for r, i in enumerate(range(0, n, 2)):
        t = r % (L + 2)
        for b in range(cb):
            start = b * wc
            cand = np.arange(start + start % 2, min(f, start + wc), 2)
            if t == L:
                c = 0                                    # an empty row
            elif t == L + 1:
                c = 1 if b == 0 else 0                   # a row with a single entry
            else:
                c = ROW_CELLS[(t + b) % L]
            assert c <= len(cand), "column block %d has %d even columns for a cell of %d" % (b, len(cand), c)
            ii.append(np.full(c, i))
            jj.append(rng.choice(cand, size=c, replace=False))
    M = len(COL_CELLS)
    for s, j in enumerate(range(1, f, 2)):
        for b in range(rb):
            start = b * wr
            cand = np.arange(start + 1 - start % 2, min(n, start + wr), 2)
            c = COL_CELLS[(s + b) % M]
            assert c <= len(cand), "row block %d has %d odd rows for a cell of %d" % (b, len(cand), c)
            ii.append(rng.choice(cand, size=c, replace=False))
            jj.append(np.full(c, j))
    ii, jj = np.concatenate(ii), np.concatenate(jj)
    vals = rng.gamma(1.0, 1.0, ii.size) + 0.05
    X = sp.csr_matrix((vals.astype(dtype), (ii, jj)), shape=(n, f))
    X.sort_indices()
    return X


def random_csr(n, f, density, seed, dtype=np.float64):
    """scipy's uniform random structure with gamma(1, 1) + 0.05 values (sorted CSR)."""
    rng = np.random.default_rng(seed)
    X = sp.random(n, f, density=density, format='csr', random_state=rng, data_rvs=lambda s: rng.gamma(1.0, 1.0, s) + 0.05)
    X = sp.csr_matrix(X, dtype=dtype)
    X.sort_indices()
    return X


def factors(n, f, k, seed):
    """Positive (W, H) with H's rows summing to 1 and W.H of the order of the data."""
    rng = np.random.default_rng(seed)
    H = orc.normalize_sum(rng.random((k, f)) + 0.05, axis=1)
    W = (rng.random((n, k)) + 0.05) * (f / k)
    return W, H


def as_f32(a):
    """What the fp32 kernels see of an fp64 input: rounded to float32, widened back to fp64."""
    if sp.issparse(a):
        b = sp.csr_matrix(a, dtype=np.float32, copy=True)
        return sp.csr_matrix(b, dtype=np.float64)
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _clean(X):
    """The stored entries the reference and the library see: explicit zeros dropped, indices sorted (nmf.py:66)."""
    X = sp.csr_matrix(X, copy=True)
    X.eliminate_zeros()
    X.sort_indices()
    return X


def chunked_terms(X, W, H, eps=orc.EPS_RATIO, chunk=ORACLE_MAX_PRODUCTS):
    """(loss, q) of the reference's CSR branch: q = (x + eps) / (W.H + eps) on the stored entries in CSR order, and
    loss = sum x log q - sum x + sum_a colsum(W)_a rowsum(H)_a (nmf.py:301-308, 331-334); W.H on the stored entries
    in runs of consecutive rows holding at most `chunk` products."""
    X = _clean(X)
    n, k = W.shape
    HT = np.ascontiguousarray(H.T)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(X.indptr))
    wh = np.empty(X.nnz)
    step = max(1, chunk // max(1, k))
    for p0 in range(0, X.nnz, step):
        p1 = min(X.nnz, p0 + step)
        wh[p0:p1] = np.multiply(W[rows[p0:p1]], HT[X.indices[p0:p1]]).sum(axis=1)
    x = X.data.astype(np.float64)
    q = (x + eps) / (wh + eps)
    loss = np.multiply(x, np.log(q)).sum() - x.sum() + np.sum(np.multiply(np.sum(W, axis=0), np.sum(H, axis=1)))
    return loss, q


def _rules(X, W, H, q, fit):
    """The W and H rules from the ratio values (nmf.py:338-351: the old ratio in both, the new W in the H rule)."""
    Q = sp.csr_matrix((q, X.indices, X.indptr), shape=X.shape)
    W_new = np.multiply(W, np.asarray(Q.dot(H.T)))
    H_new = orc.normalize_sum(np.multiply(H, np.asarray(Q.T.dot(W_new)).T), axis=1) if fit else H
    return W_new, H_new


def ref_step(X, W, H, eps=orc.EPS_RATIO, fit=True, chunked=None):
    """(loss, q in CSR order, W_new, H_new) of one update at (W, H), fp64.  chunked=None: the oracle's own functions when
    W.H on the stored entries is small (ORACLE_MAX_PRODUCTS), the chunked form otherwise."""
    X = _clean(X)
    if chunked is None:
        chunked = X.nnz * W.shape[1] > ORACLE_MAX_PRODUCTS
    if chunked:
        loss, q = chunked_terms(X, W, H, eps)
    else:
        loss = orc.sparse_kl_error(X, W, H, eps)
        q = orc.sparse_ratio_q(X, W, H, eps)[3]
    return (loss, q) + _rules(X, W, H, q, fit)


def ref_fit(X, H0, iters, fit=True, components=None, chunked=None):
    """(W, H, losses) of `iters` iterations with tol = 0: orc.sparse_fit_transform, or the same loop on the chunked step."""
    X = _clean(X)
    if chunked is None:
        chunked = X.nnz * H0.shape[0] > ORACLE_MAX_PRODUCTS
    if not chunked:
        return orc.sparse_fit_transform(X, H0.shape[0], H0, max_iter=iters, tol=0, fit=fit, components=components)
    H = np.array(H0, dtype=np.float64)
    W = np.asarray(X.dot(H.T))                                   # nmf.py:156
    if not fit:
        H = np.array(components, dtype=np.float64)
    prev, losses = np.inf, []
    for _ in range(iters):
        loss, q = chunked_terms(X, W, H)
        if prev - loss < 0:                                      # tol_abs = 0 (nmf.py:214-216)
            break
        prev = loss
        losses.append(loss)
        W, H = _rules(X, W, H, q, fit)
    return W, H, losses
