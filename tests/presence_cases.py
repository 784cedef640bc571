"""The masked KL-NMF update in its factored form (the exact kernel family of multimodal_amd/csrc/exact.hip.h under
presence.hip.h's policies) restated in fp64, and the masks and column
bounds the tests use.

The weights are Om[i, j] = P[i, m(j)]: P is n x M, m(j) the modality whose column range [bounds[m], bounds[m + 1]) holds j.
With Y = W.H, Q = (V + eps) / (Y + eps) and R = Om o Q one iteration is weighted_cases.ref_step_w's, with the two denominators
in the form the kernels use:
    Om.H^T = P.S           S[m] = sum of H[:, j] over the columns of modality m (M x k), summed over m = 0 .. M - 1 in order
    (W^T.Om)[:, j] = D[:, m(j)]      D = W_new^T.P (k x M)
The device is held to weighted_cases.ref_step_w / ref_fit_w on the broadcast mask `omega(P, bounds)`; tests/test_presence_cpu.py
pins this restatement to them (1e-12 on a step, 1e-10 / 1e-9 on a fit).
"""
import numpy as np

from oracle import klnmf_oracle as orc
from tests import exact_cases as ec
from tests import weighted_cases as wc

MAX_MODALITIES = 16


def modality_of(bounds):
    """m(j) for every column j."""
    bounds = np.asarray(bounds, dtype=np.int64)
    return np.repeat(np.arange(len(bounds) - 1), np.diff(bounds))


def omega(P, bounds):
    """The n x f weights the mask stands for."""
    return np.ascontiguousarray(np.asarray(P)[:, modality_of(bounds)])


def modality_sums(H, bounds):
    """S (M x k): the dictionary's row sums per modality."""
    return np.stack([H[:, a:b].sum(axis=1) for a, b in zip(bounds[:-1], bounds[1:])])


def ref_step_p(V, P, bounds, W, H, kchunk=None, wchunk=None, eps=orc.EPS_RATIO, fit=True):
    """(loss, R, W_new, H_new) of one masked update at (W, H) in fp64, the denominators factored."""
    mod = modality_of(bounds)
    Om = P[:, mod]
    WH = W.dot(H)
    Q = (V + eps) / (WH + eps)
    loss = float((Om * (V * np.log(Q) - V + WH)).sum())
    R = Om * Q
    S = modality_sums(H, bounds)
    den = np.zeros_like(W)
    for m in range(P.shape[1]):
        den = den + P[:, m:m + 1] * S[m][None, :]
    W_new = W * wc.factor(ec.w_product(R, H, wchunk), den)
    if not fit:
        return loss, R, W_new, H
    D = W_new.T.dot(P)
    H_new = orc.normalize_sum(H * wc.factor(ec.h_numerator(W_new, R, kchunk), D[:, mod]), axis=1)
    return loss, R, W_new, H_new


def ref_fit_p(V, P, bounds, H0, iters, fit=True, components=None, kchunk=None, wchunk=None):
    """(W, H, losses) of `iters` masked iterations that never stop early, from W0 = V.H0^T (unweighted, as the start is)."""
    W = ec.ref_init_W(V, H0, wchunk)
    H = np.array(H0 if fit else components, dtype=np.float64)
    losses = []
    for _ in range(iters):
        loss, _, W, H = ref_step_p(V, P, bounds, W, H, kchunk, wchunk, fit=fit)
        losses.append(loss)
    return W, H, np.array(losses)


def mask(n, M, seed):
    """P (n x M) in [0, 1]: 30 % exact zeros, 30 % exact ones, the rest uniform; one all-zero row (a sample with no modality
    present) where there are four rows, and for M >= 3 one modality absent from every row.  A mask of fewer than four entries
    keeps every value positive (at 1 x 1 a zero would leave nothing to fit)."""
    rng = np.random.default_rng(seed)
    u, t = rng.random((n, M)), rng.random((n, M))
    if n * M < 4:
        return 0.5 + 0.5 * u
    P = np.where(t < 0.3, 0.0, np.where(t < 0.6, 1.0, u))
    if n >= 4:
        P[n // 3, :] = 0.0
    if M >= 3:
        P[:, M // 2] = 0.0
    return P


# bounds a shape names (tests/test_presence_gpu.py's table)
NAMED_BOUNDS = {
    (65, 3): [0, 1, 64, 65],                # three modalities in the first 64-column tile, one modality in a tile of its own
    (129, 3): [0, 65, 100, 129],            # a modality that ends one column into a tile
    (16385, 3): [0, 4097, 16384, 16385],    # one past a segment of the H rule; a last modality of one column
}


def bounds(f, M):
    """M + 1 column bounds 0 = b_0 < ... < b_M = f: NAMED_BOUNDS where the shape names them, modalities of width 1 (the last one
    takes the rest) where f < 2 M, else near-equal widths with every inner bound moved off the 64-column tile edges."""
    if (f, M) in NAMED_BOUNDS:
        return list(NAMED_BOUNDS[(f, M)])
    assert 1 <= M <= f
    if f < 2 * M:
        return list(range(M)) + [f]
    b = [(f * m) // M for m in range(M + 1)]
    return [v + 1 if (0 < i < M and v % 64 == 0) else v for i, v in enumerate(b)]
