# encoding: utf-8
"""Nearest-neighbour evaluation on the GPU (next-row N4; reference multimodal/evaluation.py:70-140).

`all_distances` is the one heavy operation there: every reconstructed sample against every example, for
one of the measures of `lib/metrics.py`.  The reference broadcasts [n_test, 1, d] x [1, n_ex, d] through
numpy; here it is one kernel launch (`klnmf_all_distances`).  The label bookkeeping around it is index
arithmetic and stays on the host.
"""
import numpy as np
import scipy.sparse as sp

from .lib import metrics

_METRIC_OF = {'kl_div': metrics.kl_div, 'rev_kl_div': metrics.rev_kl_div, 'sym_kl_div': metrics.sym_kl_div,
              'frobenius': metrics.frobenius, 'cosine_diff': metrics.cosine_diff}


def todense(X):
    return np.asarray(X.todense()) if sp.issparse(X) else X


def _gpu_measure(measure):
    """The GPU implementation of `measure`: one of this package's measures, or the reference's function of
    the same name (so that `experiment.py` can keep importing its own `lib.metrics`)."""
    name = getattr(measure, '__name__', None)
    if name not in _METRIC_OF:
        raise ValueError("measure %r has no GPU implementation (known: %s)" % (name, ', '.join(sorted(_METRIC_OF))))
    return _METRIC_OF[name]


def all_distances(reco_data, ex_data, measure):
    """[len(reco_data), len(ex_data)] matrix of measure(reco, example) (reference evaluation.py:103-106)."""
    reco = np.asarray(todense(reco_data))[:, np.newaxis, :]
    ex = np.asarray(todense(ex_data))[np.newaxis, :, :]
    return _gpu_measure(measure)(reco, ex, axis=-1)


def dists_to_found_labels(dists, ex_labels):
    """Label of the nearest example of every row (reference evaluation.py:74-77)."""
    nearest = np.argmin(dists, axis=1)
    return [ex_labels[j] for j in nearest]


def found_labels_to_score(true, found):
    """Fraction of matching labels (reference evaluation.py:80-83)."""
    return np.average([f == t for f, t in zip(found, true)])


def found_labels_to_confusion(true, found, n_labels):
    """conf[i, j] = 1 where label i was classified as j at least once (reference evaluation.py:86-92: the
    fancy-index `+=` there does not accumulate repeated pairs, and neither does this)."""
    conf = np.zeros((n_labels, n_labels))
    conf[true, found] += 1
    return conf


def classify_NN(reco_data, ex_data, ex_labels, measure):
    """Nearest example's label for every reconstructed sample (reference evaluation.py:109-116)."""
    return dists_to_found_labels(all_distances(reco_data, ex_data, measure), ex_labels)


_DIST_OF = {'kl_div': 0, 'rev_kl_div': 1, 'sym_kl_div': 2, 'frobenius': 3, 'cosine_diff': 4}      # _native.DIST_*


def _measure_code(measure):
    """_native.DIST_* of a measure given as `all_distances` takes it (a function of a known name) or as that name."""
    name = measure if isinstance(measure, str) else getattr(measure, '__name__', None)
    if name not in _DIST_OF:
        raise ValueError("measure %r has no GPU implementation (known: %s)" % (name, ', '.join(sorted(_DIST_OF))))
    return _DIST_OF[name]


def nearest_examples(reco_data, ex_data, measures):
    """{measure: index of the nearest example of every row} for all `measures` in ONE search on the GPU (klnmf_nearest): what
    np.argmin(all_distances(reco_data, ex_data, measure), axis=1) gives per measure (reference evaluation.py:74-77, 103-106),
    without the distance matrices."""
    from . import _native
    measures = list(measures)
    codes = [_measure_code(m) for m in measures]
    if not codes:
        return {}
    mask = _native.metric_mask(codes)
    idx = _native.nearest(np.asarray(todense(reco_data)), np.asarray(todense(ex_data)), mask)
    slot = {c: s for s, c in enumerate(_native.mask_metrics(mask))}
    return {m: idx[:, slot[c]].astype(np.intp) for m, c in zip(measures, codes)}


def classify_NN_measures(reco_data, ex_data, ex_labels, measures):
    """{measure: nearest example's label for every reconstructed sample}: `classify_NN` for several measures at once."""
    return {m: [ex_labels[j] for j in nearest] for m, nearest in nearest_examples(reco_data, ex_data, measures).items()}


def checked_labels(labels, n_rows, n_labels=None):
    """(int32 labels, n_labels) of `labels`, one integer in [0, n_labels) per row; n_labels defaults to max(labels) + 1.
    ValueError otherwise."""
    arr = np.asarray(labels)
    if arr.shape != (n_rows,):
        raise ValueError("one label per row: labels of shape %s for %d rows" % (arr.shape, n_rows))
    if n_rows < 1:
        raise ValueError("no sample: the information matrix of nothing is not defined")
    if arr.dtype.kind not in 'iu':
        if arr.dtype.kind != 'f' or not np.all(arr == np.floor(arr)):
            raise ValueError("labels must be integers, got %s" % arr.dtype)
    if n_labels is None:
        n_labels = int(arr.max()) + 1
    if int(n_labels) < 1 or arr.min() < 0 or arr.max() >= int(n_labels):
        raise ValueError("labels outside [0, %d)" % int(n_labels))
    return arr.astype(np.int32), int(n_labels)


def information_matrix(internal, labels, n_labels=None, bins=10, return_counts=False):
    """(n_labels, k) float64: the mutual information between each internal coefficient (a column of `internal` [n, k]), binned
    into `bins` equal bins over its own [min, max], and the presence of each label -- np.array([mutual_information_by_label(
    internal[:, i], by_label) for i in range(K)]).T of the reference's samples/plot_info_matrix.py:66-90, 126-136, on the GPU
    (klnmf_information).  labels: one integer in [0, n_labels) per row; n_labels defaults to max(labels) + 1.  return_counts:
    also the int32 histograms [k, n_labels, bins] (np.histogram's own counts).  ValueError for labels that are not integers in
    range, for an empty input and for coefficients that are not finite (np.histogram's own refusal)."""
    from . import _native
    internal = np.asarray(todense(internal))
    if internal.ndim != 2 or internal.shape[0] < 1 or internal.shape[1] < 1:
        raise ValueError("a non-empty matrix [n, k] of coefficients, got shape %s" % (internal.shape,))
    labels, n_labels = checked_labels(labels, internal.shape[0], n_labels)
    if not 1 <= int(bins) <= 256:
        raise ValueError("bins must lie in [1, 256], got %r" % (bins,))
    if not np.all(np.isfinite(internal)):
        raise ValueError("coefficients that are not finite: their range is not finite")
    return _native.information(internal, labels, n_labels, bins=int(bins), return_counts=return_counts)


def sliding_distances(learner, modality, streams, codebooks, windows, example_coefficients, iterations, lags=(5, 2),
                      metric='cosine_diff', device=None):
    """The [len(windows), n_examples] matrix the reference's sliding evaluation stores as `sliding_distances`
    (samples/image_sound_eval_sliding.py:97-126, behind the MFCC front end): every window of the frame `streams` becomes a HAC
    row, built as CSR on the device (`features.hac.windowed_hac`); the rows are transformed on `learner`'s dictionary of
    `modality` for `iterations` updates (`MultimodalLearner.reconstruct_internal` on the device arrays); the internal
    coefficients are compared with `example_coefficients` [n_examples, k] under `metric` (a measure's name or function,
    `all_distances`'s); `device`: `windowed_hac`'s.  The counts take the example coefficients' type (float32 stays float32,
    anything else float64)."""
    from . import _native
    from .features.hac import windowed_hac
    code = _measure_code(metric)
    examples = np.asarray(todense(example_coefficients))
    if examples.ndim != 2 or examples.shape[1] != learner.k:
        raise ValueError("example coefficients [n_examples, %d] expected, got shape %s" % (learner.k, examples.shape))
    dtype = np.float32 if examples.dtype == np.float32 else np.float64
    rows = windowed_hac(streams, codebooks, windows, lags=lags, dtype=dtype, device=device, output='device')
    internal = learner.reconstruct_internal(modality, rows, iterations)
    return _native.all_distances(internal, examples, code)


def scores_from_dists(dists, true_labels_0, true_labels_1=None, verbose=False):
    """Deprecated in the reference too (evaluation.py:61-71)."""
    if true_labels_1 is None:
        assert(dists.shape[0] == dists.shape[1])
        true_labels_1 = true_labels_0
    found = dists_to_found_labels(dists, true_labels_1)
    result = found_labels_to_score(true_labels_0, found)
    if verbose:
        print(result)
    return result


def evaluate_NN_label(reco_data, test_data, true_labels, test_labels, measure):
    """Score of nearest-neighbour labelling against `test_data` (reference evaluation.py:119-131)."""
    return scores_from_dists(all_distances(reco_data, test_data, measure), true_labels, test_labels)
