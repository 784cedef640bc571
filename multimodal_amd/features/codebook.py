# encoding: utf-8
"""The codebook builders of the HAC features (reference multimodal/features/hac.py:68-107) with their hot half on the device.

The reference's `build_codebook(mode='raw')` is scipy's `kmeans2(data, k)`; `mode='iterative'` is its `iterative_kmeans`
([Driesen2012] Alg. 1.1): k - 1 rounds of `vq`, an SVD of the largest cluster's members and ten Lloyd iterations.  Here:

* the host twins in numpy -- `host_lloyd`, `host_kmeans`, `host_gram`, `host_iterative_kmeans`, `host_build_codebook` -- which
  restate the rules of csrc/kmeans.hip.h, the summation order included, and which the device path equals bit for bit;
* the device path -- `kmeans`, `iterative_kmeans`, `build_codebook`, `build_codebooks` -- on klnmf_kmeans_device and
  klnmf_kmeans_gram_device (include/klnmf_kmeans.h).  With `output='device'` the codebooks stay device tensors that
  `features.hac.windowed_hac` takes unchanged.

The rules.  A frame's label is `features.hac.quantize`'s.  A cluster's new row is the fp64 sum of its frames divided once by
their count, stored in the call's type; a cluster without a member keeps its row bit for bit; exactly `iter` iterations run and
the labels are those of the last assignment, before the last update (kmeans2's).  THE SUMMATION ORDER: every sum over frames is
formed per group of GROUP = 4096 consecutive frames, the group's contributing frames added in ascending order starting from +0,
and the groups' partial sums are then added in ascending group order starting from +0.  The Gram matrix adds the fp64 products
x_i * x_j, each rounded on its own, under the same rule.

The split of the iterative builder: (lambda, v) the top eigenpair of the Gram matrix of the largest cluster's members
(`numpy.linalg.eigh`), p = v * sqrt(sqrt(lambda)) -- the reference's `v[0] * sqrt(s[0])` of the members' SVD, since
s_0^2 = lambda -- with the sign that makes p's component of largest magnitude positive (the lowest index among ties), p = 0
where lambda <= 0; the largest cluster is the lowest index among equal counts.

Not here: the MFCC front end, scipy's rank-deficient 'random' initialisation (T <= d: ValueError), k-means++.
"""
import numpy as np

from .. import _native
from . import hac

GROUP = _native.KMEANS_GROUP
MAX_KD = _native.KMEANS_MAX_KD
GRAM_MAX_D = _native.KMEANS_GRAM_MAX_D


# ---- the host twins -----------------------------------------------------------------------------------------------------------------
def _float_type(*arrays):
    return np.float32 if all(str(a.dtype).endswith('float32') for a in arrays) else np.float64


def _group_sums(X64, labels, K):
    """float64 [K, d]: the sums of the rows of X64 per label under the summation order."""
    total = np.zeros((K, X64.shape[1]), dtype=np.float64)
    for g0 in range(0, X64.shape[0], GROUP):
        part = np.zeros_like(total)
        np.add.at(part, labels[g0:g0 + GROUP], X64[g0:g0 + GROUP])      # unbuffered: row by row, ascending
        total = total + part
    return total


def host_lloyd(data, init, n_iter):
    """(codebook, labels int32 [T], counts int64 [K]) after `n_iter` >= 0 Lloyd iterations from `init` -- klnmf_kmeans_device's
    numpy twin.  float32 if data and init both are, float64 otherwise."""
    data, init = np.asarray(data), np.asarray(init)
    dt = _float_type(data, init)
    X64 = np.ascontiguousarray(data, dtype=dt).astype(np.float64)
    cb = np.array(init, dtype=dt, order='C')
    K = cb.shape[0]
    labels = hac.quantize(X64, cb)
    counts = np.bincount(labels, minlength=K).astype(np.int64)
    for it in range(int(n_iter)):
        if it:
            labels = hac.quantize(X64, cb)
            counts = np.bincount(labels, minlength=K).astype(np.int64)
        sums = _group_sums(X64, labels, K)
        full = counts > 0
        cb[full] = (sums[full] / counts[full].astype(np.float64)[:, np.newaxis]).astype(dt)
    return cb, labels, counts


def host_kmeans(data, init, iter=10):
    """(codebook, labels): `scipy.cluster.vq.kmeans2(data, init, iter, minit='matrix')` under the stated rules."""
    cb, labels, _ = host_lloyd(data, init, iter)
    return cb, labels


def host_gram(data, labels, cluster):
    """(G float64 [d, d], column sums float64 [d], count) of the frames with label `cluster` (-1: all) --
    klnmf_kmeans_gram_device's numpy twin."""
    X64 = np.asarray(data).astype(np.float64)
    T, d = X64.shape
    member = np.ones(T, dtype=bool) if cluster < 0 else (np.asarray(labels) == cluster)
    G, s = np.zeros((d, d)), np.zeros(d)
    for g0 in range(0, T, GROUP):
        pg, ps = np.zeros((d, d)), np.zeros(d)
        for x in X64[g0:g0 + GROUP][member[g0:g0 + GROUP]]:
            pg = pg + x[:, np.newaxis] * x[np.newaxis, :]
            ps = ps + x
        G, s = G + pg, s + ps
    return G, s, int(member.sum())


def split_direction(G):
    """p of the module's text from the Gram matrix of a cluster's members."""
    lam, V = np.linalg.eigh(np.asarray(G, dtype=np.float64))
    if not lam[-1] > 0:
        return np.zeros(G.shape[0])
    p = V[:, -1] * np.sqrt(np.sqrt(lam[-1]))
    return -p if p[int(np.argmax(np.abs(p)))] < 0 else p


def split_rows(row, p, alpha, dt):
    """The two rows that replace `row`: row + alpha p, row - alpha p, formed in float64 and stored as `dt`."""
    c = np.asarray(row).astype(np.float64)
    return np.stack([c + alpha * p, c - alpha * p]).astype(dt)


def host_iterative_kmeans(data, k, alpha=0.01, iter=10):
    """The reference's `iterative_kmeans(data, k, alpha)` (features/hac.py:68-97) under the stated rules: the codebook [k, d]."""
    data = np.asarray(data)
    dt = _float_type(data)
    X = np.ascontiguousarray(data, dtype=dt)
    cb = host_lloyd(X, np.zeros((1, X.shape[1]), dtype=dt), 1)[0]          # the mean of all frames
    while cb.shape[0] < k:
        _, labels, counts = host_lloyd(X, cb, 0)
        h = int(np.argmax(counts))
        G, _, _ = host_gram(X, labels, h)
        cb = np.vstack([cb[:h], cb[h + 1:], split_rows(cb[h], split_direction(G), alpha, dt)])
        cb = host_lloyd(X, cb, iter)[0]
    return cb


def _generator(rng):
    return rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)


def random_init(G, s, T, k, rng, dt=np.float64):
    """scipy's 'random' initialisation of kmeans2 restated from the Gram matrix G, the column sums s and the number T of frames:
    k x d standard normals of `rng` times the transposed Cholesky factor of the covariance (G - s s^T / T) / (T - 1), plus the
    mean s / T."""
    mu = s / T
    cov = (G - np.outer(s, s) / T) / (T - 1)
    x = _generator(rng).standard_normal(size=(int(k), mu.size))
    x = x @ np.linalg.cholesky(cov).T
    x += mu
    return x.astype(dt)


def host_build_codebook(data, k, mode='raw', rng=None, alpha=0.01, iter=10):
    """The reference's `build_codebook` (features/hac.py:100-107) from the host twins."""
    if mode not in ('raw', 'iterative'):
        raise ValueError('Invalid mode, should be raw or iterative')
    data = np.asarray(data)
    if mode == 'iterative':
        return host_iterative_kmeans(data, k, alpha=alpha, iter=iter)
    G, s, T = host_gram(data, None, -1)
    return host_kmeans(data, random_init(G, s, T, k, rng, _float_type(data)), iter)[0]


# ---- the device path ----------------------------------------------------------------------------------------------------------------
def _matrix(a, what):
    if hac._is_tensor(a):
        if a.dim() != 2 or str(a.dtype) not in ('torch.float32', 'torch.float64') or (a.shape[1] > 1 and a.stride(1) != 1):
            raise ValueError("%s: a 2-D float32 / float64 tensor with contiguous rows expected" % what)
        if a.shape[0] > 1 and a.stride(0) < a.shape[1]:
            raise ValueError("%s: a row stride below the row length" % what)
        return a
    a = np.asarray(a)
    if a.ndim != 2:
        raise ValueError("%s: a matrix expected, got shape %s" % (what, a.shape))
    a = np.ascontiguousarray(a, dtype=a.dtype if a.dtype in (np.float32, np.float64) else np.float64)
    if not np.all(np.isfinite(a)):
        raise ValueError("%s: values that are not finite" % what)
    return a


def check_kmeans_inputs(data, init=None, k=None, iter=10, gram=False):
    """(data, init, T, d, K, f64) as the device path uses them, or ValueError before any native call: matrices that are not 2-D of
    float32 / float64 (host arrays of other types are taken as float64), host values that are not finite, no frame, d < 1, a
    codebook whose d is not the frames', K < 1, iter < 1, K * d above MAX_KD = 13312, d above GRAM_MAX_D = 64 where the Gram
    matrix is needed (`gram`)."""
    data = _matrix(data, "data")
    T, d = int(data.shape[0]), int(data.shape[1])
    if d < 1 or T < 1 or T >= 2 ** 31 - 1:
        raise ValueError("frames [1 <= T < 2^31 - 1, d >= 1] expected, got shape %s" % ((T, d),))
    if init is not None:
        init = _matrix(init, "init")
        if int(init.shape[1]) != d:
            raise ValueError("frames of shape %s against a codebook of shape %s" % ((T, d), tuple(init.shape)))
        K = int(init.shape[0])
    else:
        if k is None or int(k) != k:
            raise ValueError("k: an integer expected, got %r" % (k,))
        K = int(k)
    if K < 1:
        raise ValueError("a codebook of at least one unit expected, got K = %d" % K)
    if int(iter) != iter or int(iter) < 1:
        raise ValueError("iter: an integer >= 1 expected, got %r" % (iter,))
    if K * d > MAX_KD:
        raise ValueError("K * d = %d * %d is above the %d fp64 accumulators of a workgroup" % (K, d, MAX_KD))
    if gram and d > GRAM_MAX_D:
        raise ValueError("d = %d is above the %d columns of the Gram call" % (d, GRAM_MAX_D))
    f32 = str(data.dtype).endswith('float32') and (init is None or str(init.dtype).endswith('float32'))
    return data, init, T, d, K, not f32


class _Frames(object):
    """The frames on the device with the buffers the calls on them share: labels, counts, workspace, Gram matrix."""

    def __init__(self, data, T, d, K, f64, device):
        import torch
        self.torch = torch
        self.dev = hac._torch_device(device)
        self.ordinal = self.dev.index if self.dev.type == 'cuda' and self.dev.index is not None else 0
        self.T, self.d, self.f64 = T, d, f64
        self.tdt = torch.float64 if f64 else torch.float32
        self.ndt = np.float64 if f64 else np.float32
        self.x = self.place(data)
        self.ld = self.x.stride(0) if T > 1 else d
        self.work_bytes = _native.kmeans_work_bytes(T, d, K)
        self.work = torch.empty(max(16, self.work_bytes), dtype=torch.uint8, device=self.dev)
        self.labels = torch.zeros(T, dtype=torch.int32, device=self.dev)
        self.counts = torch.zeros(K, dtype=torch.int64, device=self.dev)
        self.gram_out = torch.zeros(d * d + d, dtype=torch.float64, device=self.dev) if d <= GRAM_MAX_D else None

    def place(self, a):
        if not hac._is_tensor(a):
            a = self.torch.from_numpy(a if a.flags.writeable else a.copy())
        return a.to(device=self.dev, dtype=self.tdt)

    def codebook(self, init):
        """A contiguous device copy of `init`: the call's in/out codebook."""
        return self.place(init).clone().contiguous()

    def lloyd(self, d_cb, n_iter):
        K = int(d_cb.shape[0])
        _native.kmeans_device(self.x.data_ptr(), self.ld, self.T, self.d, d_cb.data_ptr(), self.d, K, n_iter, self.work.data_ptr(),
                              self.work_bytes, self.labels.data_ptr(), self.counts.data_ptr(), f64=self.f64, device=self.ordinal)

    def gram(self, cluster):
        """(G [d, d], column sums [d], count) on the host."""
        d = self.d
        count = _native.kmeans_gram_device(self.x.data_ptr(), self.ld, self.T, d, self.labels.data_ptr(), cluster,
                                           self.work.data_ptr(), self.work_bytes, self.gram_out.data_ptr(),
                                           self.gram_out.data_ptr() + 8 * d * d, f64=self.f64, device=self.ordinal)
        out = self.gram_out.cpu().numpy()
        return out[:d * d].reshape(d, d).copy(), out[d * d:].copy(), count


def _check_output(output):
    if output not in ('numpy', 'device'):
        raise ValueError("output: 'numpy' or 'device', got %r" % (output,))


def _run_kmeans(fr, init, iter, output):
    d_cb = fr.codebook(init)
    fr.lloyd(d_cb, iter)
    if output == 'device':
        return d_cb, fr.labels
    return d_cb.cpu().numpy(), fr.labels.cpu().numpy()


def kmeans(data, init, iter=10, device=None, output='numpy'):
    """(codebook [K, d], labels int32 [T]): `kmeans2(data, init, iter, minit='matrix')` on the GPU, `iter` Lloyd iterations in
    2 * iter launches (csrc/kmeans.hip.h), bit for bit `host_kmeans`.

    data [T, d], init [K, d]: host arrays (uploaded here; float32 if both are float32, float64 otherwise) or tensors already on
    `device` of one floating type, used in place -- rows contiguous, a row stride above d allowed.  `init` is not written.
    output: 'numpy' -- host arrays; 'device' -- tensors on the device, the codebook as `features.hac.windowed_hac` takes it.
    ValueError (`check_kmeans_inputs`) before any native call."""
    _check_output(output)
    data, init, T, d, K, f64 = check_kmeans_inputs(data, init=init, iter=iter)
    return _run_kmeans(_Frames(data, T, d, K, f64, device), init, int(iter), output)


def _iterative(fr, k, alpha, iter):
    torch = fr.torch
    d_cb = torch.zeros((1, fr.d), dtype=fr.tdt, device=fr.dev)
    fr.lloyd(d_cb, 1)                                                      # the mean of all frames: one update from K = 1
    while d_cb.shape[0] < k:
        fr.lloyd(d_cb, 0)
        counts = fr.counts[:d_cb.shape[0]].cpu().numpy()
        h = int(np.argmax(counts))
        G, _, _ = fr.gram(h)
        rows = split_rows(d_cb[h].cpu().numpy(), split_direction(G), alpha, fr.ndt)
        d_cb = torch.cat([d_cb[:h], d_cb[h + 1:], torch.from_numpy(rows).to(fr.dev)]).contiguous()
        fr.lloyd(d_cb, iter)
    return d_cb


def iterative_kmeans(data, k, alpha=0.01, iter=10, device=None, output='numpy'):
    """The codebook [k, d] of the reference's `iterative_kmeans(data, k, alpha)` (features/hac.py:68-97), bit for bit
    `host_iterative_kmeans`.  Per round: one labels-and-counts call, k counts downloaded, one Gram call on the largest cluster,
    d^2 + d doubles downloaded, the d x d eigenproblem on the host, one codebook row down and two up, one Lloyd call of `iter`
    iterations.  The frames never leave the device.  d <= 64.  `data`, `output`, `device`: as `kmeans`."""
    _check_output(output)
    data, _, T, d, K, f64 = check_kmeans_inputs(data, k=k, iter=iter, gram=True)
    d_cb = _iterative(_Frames(data, T, d, K, f64, device), K, float(alpha), int(iter))
    return d_cb if output == 'device' else d_cb.cpu().numpy()


def build_codebook(data, k, mode='raw', rng=None, alpha=0.01, iter=10, device=None, output='numpy'):
    """The reference's `build_codebook(data, k, mode)` (features/hac.py:100-107) on the GPU.  'iterative': `iterative_kmeans`.
    'raw': `kmeans2(data, k)` with scipy's 'random' initialisation restated (`random_init`: `rng` a numpy.random.Generator or a
    seed for one), its mean and covariance from one Gram call on all frames, then `kmeans`.  T <= d -- scipy's rank-deficient
    branch -- and any other mode: ValueError."""
    if mode not in ('raw', 'iterative'):
        raise ValueError('Invalid mode, should be raw or iterative')
    if mode == 'iterative':
        return iterative_kmeans(data, k, alpha=alpha, iter=iter, device=device, output=output)
    _check_output(output)
    data, _, T, d, K, f64 = check_kmeans_inputs(data, k=k, iter=iter, gram=True)
    if T <= d:
        raise ValueError("T = %d frames of d = %d columns: the rank-deficient initialisation is not built" % (T, d))
    fr = _Frames(data, T, d, K, f64, device)
    G, s, count = fr.gram(-1)
    return _run_kmeans(fr, random_init(G, s, count, K, rng, fr.ndt), int(iter), output)[0]


def build_codebooks(streams, ks, mode='raw', rng=None, **kwargs):
    """The reference's `build_codebooks_from_list_of_wav` (features/hac.py:110-149) from its stacked frame streams on: the tuple
    of `build_codebook(stream, k, mode)` over (streams, ks).  One generator serves the streams in order."""
    streams, ks = list(streams), list(ks)
    if len(streams) != len(ks):
        raise ValueError("%d streams against %d codebook sizes" % (len(streams), len(ks)))
    if mode not in ('raw', 'iterative'):
        raise ValueError('Invalid mode, should be raw or iterative')
    rng = _generator(rng) if mode == 'raw' else None
    return tuple(build_codebook(x, k, mode=mode, rng=rng, **kwargs) for x, k in zip(streams, ks))
