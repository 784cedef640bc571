"""Inputs shared by tests/test_device_presence_cpu.py and tests/test_device_presence_gpu.py (presence masks on DeviceDataset).

The imputation case -- what the mask is for: exact rank-4 data, n = 120, two modalities of 50 + 40 columns, the second one absent
(and stored as zeros) in the rows where a uniform draw falls below 0.4; k = 4, 100 iterations.  On the fp64 restatement
(presence_cases.ref_fit_p) the relative L1 error of the reconstructed absent block is 0.01087 under the mask and 1.00000 for the
unmasked fit of the zero-filled matrix (which learns the zeros); at 300 iterations 0.00177 and 1.00000.
"""
import numpy as np

IMPUTE_N, IMPUTE_DIMS, IMPUTE_K, IMPUTE_ITERS = 120, (50, 40), 4, 100
IMPUTE_BOUNDS = [0, 50, 90]
# the unmasked fit reproduces the stored zeros, an error of 1; the mask is worth having if it recovers the block ten times better
IMPUTE_GAIN = 10.0
# ... and in absolute terms: the restatement's own error on the absent block after 100 iterations is 0.01087; a fit that is off by
# twice that has not converged as the restatement does
IMPUTE_CEILING = 0.02


def imputation_case():
    """(X, Xz, absent, P, H0): the full data, the data as stored (zeros where the second modality is absent), the absent rows, the
    n x 2 mask and the initial dictionary (the rule of nmf.py:149-151)."""
    rng = np.random.default_rng(5)
    n, f, k = IMPUTE_N, sum(IMPUTE_DIMS), IMPUTE_K
    X = rng.gamma(1.0, 1.0, (n, k)).dot(rng.gamma(1.0, 1.0, (k, f)))
    absent = rng.random(n) < 0.4
    Xz = X.copy()
    Xz[absent, IMPUTE_DIMS[0]:] = 0.0
    P = np.ones((n, 2))
    P[absent, 1] = 0.0
    H0 = rng.random((k, f)) + .01
    H0 /= H0.sum(axis=1, keepdims=True)
    return X, Xz, absent, P, H0


def absent_block_error(X, absent, W, H):
    """Relative L1 error of W.H on the block that was absent."""
    d0 = IMPUTE_DIMS[0]
    truth = X[absent, d0:]
    return float(np.abs(W.dot(H)[absent, d0:] - truth).sum() / np.abs(truth).sum())


class HostTensor(object):
    """What DeviceDataset asks of a device tensor, on a host array (the CPU tests' `_to_device`)."""

    def __init__(self, a):
        self.a = np.ascontiguousarray(a)
        self.shape = self.a.shape

    def data_ptr(self):
        return self.a.ctypes.data

    def numel(self):
        return self.a.size

    def element_size(self):
        return self.a.itemsize

    def stride(self, axis):
        return self.a.strides[axis] // self.a.itemsize

    def max(self):
        return self.a.max()
