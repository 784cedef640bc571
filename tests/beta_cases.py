"""The beta-divergence loop (multimodal_amd/csrc/beta.hip.h, include/klnmf_beta.h) restated in numpy fp64: the reference of
tests/test_beta_cpu.py and tests/test_beta_gpu.py.  The reference project has no counterpart (nmf.py:293 announces "Helpers for
beta divergence and related updates" and holds none), so the semantics are the ones fixed with the feature:

  x = V + 1e-8, y = W.H + 1e-8 in every term; Om: optional weights >= 0
  cost   sum(Om * d_beta(x | y));  d_2 = (x - y)^2 / 2;  d_0 = x/y - log(x/y) - 1;
         d_beta = (x^beta + (beta - 1) y^beta - beta x y^(beta-1)) / (beta (beta - 1)) otherwise
  A = Om * x * y^(beta-2),  B = Om * y^(beta-1)
  W rule  W <- W * ((A.H^T) / (B.H^T))^gamma        H rule  H <- H * ((W^T.A) / (W^T.B))^gamma      (den = 0: the factor 1)
  gamma = 1/(2-beta) below beta = 1, 1 up to beta = 2, 1/(beta-1) above (the majorise-minimise exponent: <= 1)
  one fit iteration: loss, A, B at (W, H) -> W rule -> A, B at (W_new, H) -> H rule with W_new -> H's rows divided by
  1e-16 + row sum, W_new's columns multiplied by the row sums.  A transform: the first two steps.

The contractions are summed over the same feature chunks (W rule) and row chunks (H numerator) as the kernels sum them:
`exact_cases.w_product` / `h_numerator` with the chunks of `exact_cases.exact_regime`, as `exact_cases.ref_step` does.
"""
import numpy as np

from oracle import klnmf_oracle as orc
from tests import exact_cases as ec

EPS = orc.EPS_RATIO
EPS_NORM = orc.EPS_NORMALIZE

BETAS = (0.0, 0.5, 2.0, 3.0)                 # per-case runs on the GPU
DESCENT_BETAS = (0.0, 0.5, 1.5, 2.0, 3.0)
PROPERTY_BETAS = (-1.0, 0.0, 0.5, 1.5, 2.0, 3.0)
PROPERTY_SHAPES = ((15, 17, 1), (65, 65, 65), (300, 700, 17), (100, 300, 129))
DESCENT_RISE = 1e-12                         # no loss exceeds its predecessor by more than this, relative


def gamma_of(beta):
    if beta < 1.0:
        return 1.0 / (2.0 - beta)
    if beta <= 2.0:
        return 1.0
    return 1.0 / (beta - 1.0)


def general_div(x, y, beta):
    """The general formula, element-wise (beta not 0 or 1)."""
    return (x ** beta + (beta - 1.0) * y ** beta - beta * x * y ** (beta - 1.0)) / (beta * (beta - 1.0))


def beta_div(x, y, beta):
    """d_beta(x | y), element-wise, x, y > 0."""
    if beta == 2.0:
        return 0.5 * (x - y) ** 2
    if beta == 0.0:
        q = x / y
        return q - np.log(q) - 1.0
    return general_div(x, y, beta)


def weights_of(n, f, seed, zero_fraction=0.3, zero_row=None):
    """Om >= 0: uniform in (0.5, 1.5) with `zero_fraction` of the entries 0, and a whole row of zeros where asked."""
    rng = np.random.default_rng(seed)
    Om = rng.random((n, f)) + 0.5
    Om[rng.random((n, f)) < zero_fraction] = 0.0
    if zero_row is not None:
        Om[zero_row, :] = 0.0
    return Om


def matrices(V, W, H, beta, Om=None):
    """(loss, A, B) at (W, H)."""
    x = V + EPS
    y = W.dot(H) + EPS
    d = beta_div(x, y, beta)
    A = x * y ** (beta - 2.0)
    B = y ** (beta - 1.0)
    if Om is not None:
        obs = Om != 0
        d = np.where(obs, Om * d, 0.0)
        A = np.where(obs, Om * A, 0.0)
        B = np.where(obs, Om * B, 0.0)
    return float(d.sum()), A, B


def cost(V, W, H, beta, Om=None):
    return matrices(V, W, H, beta, Om)[0]


def factor(num, den, gamma):
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(den > 0, num / np.where(den > 0, den, 1.0), 1.0)
    return np.where(den > 0, q ** gamma, 1.0)


def ref_W_step(V, W, H, beta, Om=None, wchunk=None):
    """(loss, W_new): the W rule from A, B at (W, H)."""
    loss, A, B = matrices(V, W, H, beta, Om)
    return loss, W * factor(ec.w_product(A, H, wchunk), ec.w_product(B, H, wchunk), gamma_of(beta))


def ref_H_step(V, W, H, beta, Om=None, kchunk=None):
    """(W_scaled, H_new, H_unnormalised): the H rule from A, B at (W, H), H's rows divided by 1e-16 + row sum, W's columns
    multiplied by the sums."""
    _, A, B = matrices(V, W, H, beta, Om)
    Hu = H * factor(ec.h_numerator(W, A, kchunk), ec.h_numerator(W, B, kchunk), gamma_of(beta))
    s = Hu.sum(axis=1)
    return W * s[np.newaxis, :], Hu / (EPS_NORM + s)[:, np.newaxis], Hu


def ref_iteration(V, W, H, beta, Om=None, kchunk=None, wchunk=None, fit=True):
    """(loss at (W, H), W_new, H_new) of one iteration."""
    loss, Wn = ref_W_step(V, W, H, beta, Om, wchunk)
    if not fit:
        return loss, Wn, H
    Ws, Hn, _ = ref_H_step(V, Wn, H, beta, Om, kchunk)
    return loss, Ws, Hn


def ref_fit(V, H0, iters, beta, Om=None, fit=True, components=None, kchunk=None, wchunk=None):
    """(W, H, losses) of `iters` iterations that never stop early: W0 = V.H0^T (unweighted, as KLdivNMF's start), then the
    iteration; fit=False holds the dictionary `components`."""
    W = ec.ref_init_W(V, H0, wchunk)
    H = np.array(H0 if fit else components, dtype=np.float64)
    losses = []
    for _ in range(iters):
        loss, W, H = ref_iteration(V, W, H, beta, Om, kchunk, wchunk, fit)
        losses.append(loss)
    return W, H, np.array(losses)


def worst_rise(losses):
    """The largest relative rise of a loss over its predecessor (<= 0: the record never rises)."""
    losses = np.asarray(losses, dtype=np.float64)
    return float(np.max((losses[1:] - losses[:-1]) / np.abs(losses[:-1]))) if len(losses) > 1 else 0.0
