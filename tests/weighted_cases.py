"""The weighted / masked KL-NMF update (the exact kernel family of multimodal_amd/csrc/exact.hip.h under weighted.hip.h's policies)
restated in fp64, and the weights the tests use.

With Om >= 0 (n x f), eps = 1e-8 and Y = W.H one iteration is
    Q = (V + eps) / (Y + eps),  loss = sum Om o (V log Q - V + Y)  (before the update),  R = Om o Q
    W <- W o (R.H^T) / (Om.H^T)                       factor 1 where the denominator is exactly 0
    H <- rows normalised of H o (W_new^T.R) / (W_new^T.Om)     (fit only; factor 1 where the denominator is 0; the rows divided
                                                      by 1e-16 + their sum as orc.normalize_sum does)
from W0 = V.H0^T: the multiplicative update of sum Om o d(V | W.H) until the rows are rescaled.  With Om = 1 and H's rows
summing to 1 it is exact_cases.ref_step (tests/test_weighted_cpu.py pins that at 1e-12).  The contractions are summed over the
kernels' chunks as exact_cases does (`kchunk` rows of the H rule, `wchunk` columns of the W rule), numerator and denominator
alike.
"""
import numpy as np

from oracle import klnmf_oracle as orc
from tests import exact_cases as ec


def factor(num, den):
    """num / den, 1 where den is exactly 0."""
    pos = den > 0
    return np.where(pos, num / np.where(pos, den, 1.0), 1.0)


def ref_step_w(V, Om, W, H, kchunk=None, wchunk=None, eps=orc.EPS_RATIO, fit=True):
    """(loss, R, W_new, H_new) of one weighted update at (W, H) in fp64."""
    WH = W.dot(H)
    Q = (V + eps) / (WH + eps)
    loss = float((Om * (V * np.log(Q) - V + WH)).sum())
    R = Om * Q
    W_new = W * factor(ec.w_product(R, H, wchunk), ec.w_product(Om, H, wchunk))
    if not fit:
        return loss, R, W_new, H
    H_new = orc.normalize_sum(H * factor(ec.h_numerator(W_new, R, kchunk), ec.h_numerator(W_new, Om, kchunk)), axis=1)
    return loss, R, W_new, H_new


def ref_fit_w(V, Om, H0, iters, fit=True, components=None, kchunk=None, wchunk=None):
    """(W, H, losses) of `iters` weighted iterations that never stop early, from W0 = V.H0^T (unweighted, as the start always
    is); fit=False holds the dictionary `components`."""
    W = ec.ref_init_W(V, H0, wchunk)
    H = np.array(H0 if fit else components, dtype=np.float64)
    losses = []
    for _ in range(iters):
        loss, _, W, H = ref_step_w(V, Om, W, H, kchunk, wchunk, fit=fit)
        losses.append(loss)
    return W, H, np.array(losses)


def general(n, f, seed):
    """Uniform weights in [0, 1) with 30 % exact zeros, one all-zero row (a sample with nothing observed) and one all-zero
    column (a feature never observed) where the matrix has four of each; a matrix of fewer than 16 entries keeps every
    weight positive (at 1 x 1 a zero would leave nothing to fit)."""
    rng = np.random.default_rng(seed)
    Om = rng.random((n, f))
    if n * f < 16:
        return Om + 0.1
    Om = Om * (rng.random((n, f)) > 0.3)
    if n >= 4:
        Om[n // 3, :] = 0.0
    if f >= 4:
        Om[:, f // 2] = 0.0
    return Om


def row_mask(n, f, seed):
    """(Om, keep): weight 0 on a quarter of the rows (chosen at random), 1 elsewhere."""
    rng = np.random.default_rng(seed)
    keep = np.ones(n, dtype=bool)
    keep[rng.choice(n, n // 4, replace=False)] = False
    Om = np.ones((n, f))
    Om[~keep] = 0.0
    return Om, keep


def imputation_case():
    """(V, M, H0): seeded data of exact rank 4, 120 x 90, with 40 % of the entries hidden (M = 0) -- the issue's case."""
    rng = np.random.default_rng(11)
    n, f, k = 120, 90, 4
    Wt = rng.gamma(1.0, 1.0, (n, k))
    Ht = orc.normalize_sum(rng.gamma(0.5, 1.0, (k, f)) + 0.01, axis=1)
    V = Wt.dot(Ht) * f
    M = (rng.random((n, f)) > 0.4).astype(np.float64)
    H0 = orc.normalize_sum(rng.random((k, f)) + 0.01, axis=1)
    return V, M, H0


def hidden_error(V, M, W, H):
    """Relative L1 error of W.H on the hidden entries."""
    hid = M == 0
    return float(np.abs(W.dot(H) - V)[hid].sum() / V[hid].sum())
