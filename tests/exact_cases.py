"""The dense exact-mode routes (multimodal_amd/csrc/exact.hip.h and its dispatch) restated on the host, the cases that reach
them, and a chunked fp64 restatement of the reference's dense update.

`exact_regime` is klnmf_set_problem's size rule for a dense problem in KLNMF_PREC_F64 / F32 / BF16X3 / F16X3
(csrc/plan.hip.h, plan_dense_exact) and piece_fit_tail's choice of H-rule route (h_from_slabs there):
  * the H numerator W^T.Q in `nsplit` row chunks of `kchunk` rows (a multiple of GK = 16), one slab per chunk (EpiN);
  * the W rule's Q.H^T in one piece (EpiW) or in `wsplit` feature chunks of `wchunk` columns (EpiWpart + k_wrule_exact);
  * the H rule in `hseg_n` segments of 4096 columns (k_update_H_part + k_update_H_norm) from f = 16 384 on;
  * a single-context fit loop applies the H rule straight from the slabs (k_update_H_slabs) while nsplit * f <= 8192 and
    the rule is in one segment, otherwise from their sum (k_sum_partials + k_update_H).
tests/test_exact_cpu.py checks that CASES reach every route and edge at 256 CUs (the MI355X) and that the library's own rule
(klnmf_plan_query: no device needed) gives what this module computes; tests/test_exact_gpu.py checks the same on a context,
for the device's own CU count.

`ref_step` / `ref_fit` are the oracle's dense update (oracle/klnmf_oracle.py, nmf.py:212-222, 232-257, 297-351) in fp64
with the W rule's contraction summed over the same feature chunks and the H numerator over the same row chunks as the
kernels; tests/test_exact_cpu.py pins them to the oracle at 1e-13.
"""
import numpy as np

from oracle import klnmf_oracle as orc

GT, GK = 64, 16              # k_gemm's output tile edge and contraction step
HSEG = 4096                  # segment length of the H rule on long rows ...
HSEG_FROM = 16384            # ... from this many columns on
SLABS_MAX = 8192             # the H rule from the slabs while nsplit * f <= this (single-context loops)
WPART_CAP = 256 << 20        # bytes of the W rule's slabs (Wpart) the rule may allocate
ROWS_MAX = 65535 * GT        # row tiles ride on gridDim.y
MI355X_CUS = 256

NO_STOP = -1e300             # a tolerance the stop rule never meets: every fit runs all its iterations


def _ceil(a, b):
    return -(-int(a) // int(b))


def exact_regime(n, f, k, cu_count, esize=8, row_chunks=0, w_chunks=0, h_seg=0):
    """(nsplit, kchunk, wsplit, wchunk, hseg_n, from_slabs) of a dense n x f problem with k components on `cu_count` CUs;
    esize: bytes per element (8: f64, 4: the fp32 modes); row_chunks / w_chunks / h_seg: KLNMF_EX_ROW_CHUNKS /
    KLNMF_EX_W_CHUNKS / KLNMF_EX_H_SEG (0: the size rule)."""
    def tiles(M, N):
        return _ceil(M, GT) * _ceil(N, GT)
    if row_chunks:
        s = row_chunks
    else:
        s = max(1, min(_ceil(4 * cu_count, tiles(k, f)), _ceil(n, 64)))
    kchunk = _ceil(_ceil(n, s), GK) * GK
    nsplit = _ceil(n, kchunk)
    hseg_n = _ceil(f, HSEG) if f >= HSEG_FROM else 1
    if h_seg:
        hseg_n = _ceil(f, h_seg) if f > h_seg else 1
    wt = tiles(k, n)
    w = _ceil(2 * cu_count, wt) if wt < cu_count else 1
    w = min(w, _ceil(f, 4 * GK))
    if w_chunks:
        w = w_chunks
    while w > 1 and w * n * k * esize > WPART_CAP:
        w -= 1
    wchunk = _ceil(_ceil(f, w), GK) * GK
    wsplit = _ceil(f, wchunk)
    from_slabs = hseg_n == 1 and nsplit * f <= SLABS_MAX
    return nsplit, kchunk, wsplit, wchunk, hseg_n, from_slabs


def query_regime(n, f, k, cu_count, **forced):
    """What Context.exact_regime() reports: (row chunks, W chunks, H segments, from slabs)."""
    s, _, w, _, h, slabs = exact_regime(n, f, k, cu_count, **forced)
    return s, w, h, int(slabs)


# (n, f, k, what the case is for).  The routes each reaches at 256 CUs are checked by tests/test_exact_cpu.py.
CASES = [
    (1, 1, 1, 'one partial tile, contraction shorter than 16'),
    (15, 17, 1, 'one partial tile, contraction shorter than 16'),
    (64, 64, 64, 'exactly one tile'),
    (65, 65, 65, 'one past a tile on every axis'),
] + [
    (300, 700, k, 'component axis edge') for k in (16, 17, 63, 64, 65, 128, 129, 200, 512, 513, 1000)
] + [
    (200, 8192, 512, 'one row chunk with n > 64'),
    (16384, 300, 64, 'one-piece W rule, many rows, H rule from the sum'),
    (4111, 63, 200, 'one-piece W rule, many rows, ragged chunks'),
    (2048, 520, 513, 'one-piece W rule, k > 512'),
    (4096, 128, 16, 'nsplit * f = 8192: H rule from the slabs'),
    (4096, 129, 16, 'nsplit * f = 8256: H rule from the sum'),
    (100, 16384, 17, 'H rule in whole segments'),
    (100, 16385, 33, 'H rule, last segment of one column'),
    (77, 20000, 130, 'H rule, ragged last segment'),
    (70001, 64, 8, 'many row chunks, the last one ragged'),
    (ROWS_MAX, 3, 2, 'the largest accepted n'),
]
LARGEST_N = (ROWS_MAX, 3, 2)

# forced routes against the natural one (1000 x 300, k = 40: 16 row chunks, 5 W chunks, the H rule from the slabs)
MID = (1000, 300, 40)
FORCED_ROW_CHUNKS = (1, 2, 3, 7)
FORCED_W_CHUNKS = (1, 2, 3)          # 3: chunks of 112 columns, the last one 76
FORCED_H_SEG = (100, 128)            # 100: three whole segments; 128: the last one 44 columns


def case_id(case):
    return '%dx%dk%d' % case[:3]


def data(n, f, seed, zero_row=None, zero_col=None):
    """Dense V (n x f) that no k-component model fits exactly: gamma(1, 1) + 0.05 entries, with an all-zero row and column
    where asked (the reference's exact zeros: W's row stays 0, the dictionary's column decays)."""
    rng = np.random.default_rng(seed)
    V = rng.gamma(1.0, 1.0, (n, f)) + 0.05
    if zero_row is not None:
        V[zero_row, :] = 0.0
    if zero_col is not None:
        V[:, zero_col] = 0.0
    return V


def factors(n, f, k, seed):
    """Positive (W, H) with H's rows summing to 1 and W.H of the order of the data: the loss of a step is far above 1e-2 of
    sum(V)."""
    rng = np.random.default_rng(seed)
    H = orc.normalize_sum(rng.random((k, f)) + 0.05, axis=1)
    W = (rng.random((n, k)) + 0.05) * (2.0 / k)
    return W, H


def as_f32(a):
    """What the fp32 kernels see of an fp64 input: rounded to float32, widened back to fp64."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _chunks(extent, chunk):
    chunk = int(chunk) if chunk else int(extent)
    return [(a, min(extent, a + chunk)) for a in range(0, extent, max(1, chunk))]


def w_product(Q, H, wchunk=None):
    """Q.H^T summed over feature chunks of `wchunk` columns (the W rule's slabs, k_wrule_exact's order)."""
    G = None
    for a, b in _chunks(Q.shape[1], wchunk):
        part = Q[:, a:b].dot(H[:, a:b].T)
        G = part if G is None else G + part
    return G


def h_numerator(W, Q, kchunk=None):
    """W^T.Q summed over row chunks of `kchunk` rows (the H numerator's slabs, k_sum_partials' order)."""
    N = None
    for a, b in _chunks(Q.shape[0], kchunk):
        part = W[a:b].T.dot(Q[a:b])
        N = part if N is None else N + part
    return N


def ref_step(V, W, H, kchunk=None, wchunk=None, eps=orc.EPS_RATIO, fit=True):
    """(loss, Q, W_new, H_new) of one update at (W, H) in fp64: the loss before the update (nmf.py:297-310), the ratio of the
    old W (nmf.py:325-336) in both rules, the new W in the H rule (nmf.py:338-351)."""
    WH = W.dot(H)
    Q = (V + eps) / (WH + eps)
    loss = float((V * np.log(Q) - V + WH).sum())
    W_new = W * w_product(Q, H, wchunk)
    H_new = orc.normalize_sum(H * h_numerator(W_new, Q, kchunk), axis=1) if fit else H
    return loss, Q, W_new, H_new


def ref_init_W(V, H0, wchunk=None):
    """W0 = V.H0^T (nmf.py:156): the W rule's contraction with multiply = 0."""
    return w_product(V, H0, wchunk)


def ref_fit(V, H0, iters, fit=True, components=None, kchunk=None, wchunk=None):
    """(W, H, losses) of `iters` iterations that never stop early (NO_STOP): W0 = V.H0^T, then the update; fit=False holds
    the dictionary `components` (nmf.py:275-291)."""
    W = ref_init_W(V, H0, wchunk)
    H = np.array(H0 if fit else components, dtype=np.float64)
    losses = []
    for _ in range(iters):
        loss, _, W, H = ref_step(V, W, H, kchunk, wchunk, fit=fit)
        losses.append(loss)
    return W, H, np.array(losses)
