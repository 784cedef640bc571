# encoding: utf-8
"""One run of a multimodal experiment on device-resident data (next-row N2 of SURVEY.md 8f).

Mirrors what the reference's driver does per run -- `MultimodalExperiment._perform_one_run` (experiment.py:158-172:
split, train, evaluate) and `TwoModalitiesExperiment._evaluate` / `_get_all_transformations` (experiment.py:233-277:
internal coefficients of the test set and of the examples from every modality, cross-modal reconstructions,
nearest-example classification under four measures in every comparison space) -- with the modalities uploaded ONCE
(`DeviceDataset`): a run hands over row indices, the rows are gathered by the upload kernel, the fits and transforms run
through the HIP path and the distance matrices through `klnmf_all_distances`.  Result keys are the reference's
(`found_<m1>2<m2>[_<space>][_bis|_frob|_cosine]`, `score_...`), so its `Logger` and result tables apply unchanged.

`sweep_assignment` spreads the runs of a k sweep (samples/launcher.py:68: Ks 5 .. 200 x 20 runs, one OS process each in
the reference) over the ranks of a node: independent fits, no communication -- replica parallelism.
"""
from itertools import product

import numpy as np

from . import _native
from .evaluation import classify_NN, found_labels_to_score
from .learner import MultimodalLearner
from .lib.metrics import kl_div, rev_kl_div, frobenius, cosine_diff

INTERNAL = -1
MEASURES = ((kl_div, ''), (rev_kl_div, '_bis'), (frobenius, '_frob'), (cosine_diff, '_cosine'))
DEVICE_MEASURES = ((_native.DIST_KL, ''), (_native.DIST_REV_KL, '_bis'), (_native.DIST_FROBENIUS, '_frob'),
                   (_native.DIST_COSINE_DIFF, '_cosine'))


def exp_key(modalities, mod1, mod2, mod_cmp, suffix):
    """experiment.py:279-283."""
    return "{}2{}{}{}".format(modalities[mod1], modalities[mod2],
                              '' if mod_cmp == INTERNAL else '_' + modalities[mod_cmp], suffix)


def all_transformations(dataset, learner, rows, iter_test):
    """result[input modality][output modality] (+ the internal coefficients as the last entry), experiment.py:259-277."""
    M = len(learner.mod)
    internals = [dataset.reconstruct_internal(learner, learner.mod[m], rows, iter_test) for m in range(M)]
    out = [[None] * M for _ in range(M)]
    for i in range(M):
        out[i][i] = dataset.rows_of(i, rows)                # nothing to do
        for o in range(M):
            if o != i:
                out[i][o] = learner.reconstruct_modality(learner.mod[o], internals[i])
        out[i].append(internals[i])
    return out


def evaluate(dataset, learner, rows_test, rows_ex, labels_test, labels_ex, iter_test):
    """TwoModalitiesExperiment._evaluate (experiment.py:233-257) -> {key: found labels / score}."""
    M = len(learner.mod)
    t_test = all_transformations(dataset, learner, rows_test, iter_test)
    t_ex = all_transformations(dataset, learner, rows_ex, iter_test)
    results = {}
    for mod1, mod2, mod_cmp in product(range(M), range(M), [INTERNAL] + list(range(M))):
        for measure, suffix in MEASURES:
            found = classify_NN(t_test[mod1][mod_cmp], t_ex[mod2][mod_cmp], labels_ex, measure)
            key = exp_key(learner.mod, mod1, mod2, mod_cmp, suffix)
            results['found_' + key] = found
            results['score_' + key] = found_labels_to_score(labels_test, found)
    return results


# ---- ThreeModalitiesExperiment (experiment.py:322-404): comparisons in the internal space only, between single
# modalities and between a pair of modalities and the third ------------------------------------------------------------
def tested_combinations(n_modalities):
    """experiment.py:352-361: (mods1, mods2) as tuples of modality indices, in the order `_evaluate` walks them."""
    M = n_modalities
    combos = [([m1], [m2]) for m1 in range(M) for m2 in range(M) if m1 != m2]
    two_to_one = [([m for m in range(M) if m != mod], [mod]) for mod in range(M)]
    combos += two_to_one
    combos += [(y, x) for (x, y) in two_to_one]
    return [(tuple(x), tuple(y)) for (x, y) in combos]


def combo_key(modalities, mods1, mods2, suffix):
    """experiment.py:373-377 without the 'score_' prefix."""
    return "{}2{}{}".format('_'.join(modalities[m] for m in mods1), '_'.join(modalities[m] for m in mods2), suffix)


def all_internals(dataset, learner, rows, iter_test):
    """experiment.py:363-371: internal coefficients of `rows` from every modality set that occurs in a combination -- one
    transform per distinct set (three singles and three pairs for three modalities)."""
    internals = {}
    for mods, _rest in tested_combinations(len(learner.mod)):
        if mods not in internals:
            internals[mods] = dataset.reconstruct_internal_multi(learner, [learner.mod[m] for m in mods], rows, iter_test)
    return internals


def evaluate_internal(dataset, learner, rows_test, rows_ex, labels_test, labels_ex, iter_test):
    """ThreeModalitiesExperiment._evaluate (experiment.py:332-350) -> {found_<key>: labels, score_<key>: score}."""
    t_test = all_internals(dataset, learner, rows_test, iter_test)
    t_ex = all_internals(dataset, learner, rows_ex, iter_test)
    results = {}
    for mods1, mods2 in tested_combinations(len(learner.mod)):
        for measure, suffix in MEASURES:
            found = classify_NN(t_test[mods1], t_ex[mods2], labels_ex, measure)
            key = combo_key(learner.mod, mods1, mods2, suffix)
            results['found_' + key] = found
            results['score_' + key] = found_labels_to_score(labels_test, found)
    return results


# ---- the same two evaluations with everything between the transforms and the label lists ON the device (DeviceEvaluation:
# dictionary uploaded once, coefficients / reconstructions / raw rows as device matrices, distances by one kernel) --------
def internal_sets(kind, n_modalities):
    """The modality sets (tuples of indices) whose internal coefficients an evaluation of `kind` computes, in its order."""
    if kind == 'two':
        return [(m,) for m in range(n_modalities)]
    sets = []
    for mods, _rest in tested_combinations(n_modalities):
        if mods not in sets:
            sets.append(mods)
    return sets


SEARCHES = ('matrix', 'fused')


def _check_search(search):
    if search not in SEARCHES:
        raise ValueError("search=%r: expected one of %s" % (search, ', '.join(repr(s) for s in SEARCHES)))


def _resolve_searches(ev, listed, search):
    """[{suffix: found labels}] of the listed searches [(key of suffix, test, examples, labels_test, labels_ex)] -- of one run's
    evaluation, or of several runs' on ev's device.  'matrix': `found_labels` per search and measure, in order; 'fused': ONE
    `found_labels_many` call."""
    if search == 'matrix':
        return [{suffix: ev.found_labels(test, examples, labels_ex, metric) for metric, suffix in DEVICE_MEASURES}
                for _key, test, examples, _labels_test, labels_ex in listed]
    many = ev.found_labels_many([(test, examples, labels_ex) for _key, test, examples, _labels_test, labels_ex in listed],
                                [metric for metric, _suffix in DEVICE_MEASURES])
    return [{suffix: found[metric] for metric, suffix in DEVICE_MEASURES} for found in many]


def _results_of(listed, found):
    """{found_<key>: labels, score_<key>: score} of the listed searches, in their order (measures inner, as the reference)."""
    results = {}
    for (key_of, _test, _examples, labels_test, _labels_ex), by_suffix in zip(listed, found):
        for _metric, suffix in DEVICE_MEASURES:
            key = key_of(suffix)
            results['found_' + key] = by_suffix[suffix]
            results['score_' + key] = found_labels_to_score(labels_test, by_suffix[suffix])
    return results


def list_searches_on_device(dataset, learner, rows_test, rows_ex, labels_test, labels_ex, iter_test, ev=None, internals=None):
    """The nearest-example searches of `evaluate_on_device`, in its order: [(key of suffix, test, examples, labels_test,
    labels_ex)] with the matrices on the device."""
    M = len(learner.mod)

    def transformations(rows, side):
        if internals is not None:
            coefficients = [internals[((m,), side)] for m in range(M)]
        else:
            coefficients = [ev.internal([learner.mod[m]], rows) for m in range(M)]
        out = [[None] * M for _ in range(M)]
        for i in range(M):
            out[i][i] = ev.raw(i, rows)
            for o in range(M):
                if o != i:
                    out[i][o] = ev.reconstruct(coefficients[i], learner.mod[o])
            out[i].append(coefficients[i])
        return out
    t_test, t_ex = transformations(rows_test, 'test'), transformations(rows_ex, 'ex')
    return [(lambda suffix, c=(mod1, mod2, mod_cmp): exp_key(learner.mod, c[0], c[1], c[2], suffix),
             t_test[mod1][mod_cmp], t_ex[mod2][mod_cmp], labels_test, labels_ex)
            for mod1, mod2, mod_cmp in product(range(M), range(M), [INTERNAL] + list(range(M)))]


def list_internal_searches_on_device(dataset, learner, rows_test, rows_ex, labels_test, labels_ex, iter_test, ev=None,
                                     internals=None):
    """The nearest-example searches of `evaluate_internal_on_device`, in its order (as `list_searches_on_device`)."""
    combos = tested_combinations(len(learner.mod))

    def internals_of(rows, side):
        got = {}
        for mods, _rest in combos:
            if mods not in got:
                got[mods] = internals[(mods, side)] if internals is not None else ev.internal([learner.mod[m] for m in mods], rows)
        return got
    t_test, t_ex = internals_of(rows_test, 'test'), internals_of(rows_ex, 'ex')
    return [(lambda suffix, c=(mods1, mods2): combo_key(learner.mod, c[0], c[1], suffix), t_test[mods1], t_ex[mods2], labels_test,
             labels_ex) for mods1, mods2 in combos]


def _evaluate_listed(lister, dataset, learner, rows_test, rows_ex, labels_test, labels_ex, iter_test, ev, internals, search):
    from .device_data import DeviceEvaluation
    _check_search(search)
    if ev is None:
        ev = DeviceEvaluation(dataset, learner, iter_test)
    listed = lister(dataset, learner, rows_test, rows_ex, labels_test, labels_ex, iter_test, ev=ev, internals=internals)
    return _results_of(listed, _resolve_searches(ev, listed, search))


def evaluate_on_device(dataset, learner, rows_test, rows_ex, labels_test, labels_ex, iter_test, ev=None, internals=None,
                       search='matrix'):
    """`evaluate` (TwoModalitiesExperiment._evaluate) without host round trips.  ev / internals: the run's `DeviceEvaluation`
    and its internal coefficients {(set, 'test' | 'ex'): device tensor} where a batch computed them (`_sweep_batch`).
    search: 'matrix' (default) -- one distance matrix per comparison and measure comes back and np.argmin runs on the host
    (`DeviceEvaluation.found_labels`); 'fused' -- the evaluation lists its searches and one launch returns their indices
    (`DeviceEvaluation.found_labels_many`): the same keys, labels and scores."""
    return _evaluate_listed(list_searches_on_device, dataset, learner, rows_test, rows_ex, labels_test, labels_ex, iter_test, ev,
                            internals, search)


def evaluate_internal_on_device(dataset, learner, rows_test, rows_ex, labels_test, labels_ex, iter_test, ev=None, internals=None,
                                search='matrix'):
    """`evaluate_internal` (ThreeModalitiesExperiment._evaluate) without host round trips.  ev / internals / search: as
    `evaluate_on_device`."""
    return _evaluate_listed(list_internal_searches_on_device, dataset, learner, rows_test, rows_ex, labels_test, labels_ex,
                            iter_test, ev, internals, search)


def perform_one_run(dataset, modalities, coefs, k, iter_train, iter_test, rows_train, rows_test, rows_ex,
                    labels_test, labels_ex, init_dictionary=None, kind=None, on_device=True, keep_sparse=None, presence=None,
                    search='matrix', information=False):
    """experiment.py:158-172 on a DeviceDataset: returns (learner, results) with results['dictionary'] as stored there.
    dataset: a `DeviceDataset`, or the modalities' matrices -- uploaded here as DeviceDataset(dataset, keep_sparse=keep_sparse):
    with keep_sparse scipy-sparse modalities stay CSR on the device and the run takes the reference's sparse branch.
    on_device: the evaluation keeps every intermediate on the GPU (default) or goes through host arrays.  kind: 'two' = TwoModalitiesExperiment._evaluate (every comparison space), 'internal' = ThreeModalitiesExperiment's
    (internal space, single and paired modalities); default by the number of modalities, as the reference's scripts pick
    the class (samples/two_modalities.py, samples/three_modalities.py).
    presence: a row x modality presence mask for the dataset created here (`DeviceDataset(presence=...)`: one entry per modality,
    None or the weights of that modality in every sample, 0 where it is absent); the training and every transform of the
    evaluation that selects a masked modality then run the masked loop on the rows' own part of the mask.  A row from which
    every selected modality is absent keeps its W0; which rows are scored stays the caller's choice.  With a `DeviceDataset`,
    `presence` must be the mask it was built with (ValueError otherwise).
    search: how the device evaluation finds the nearest examples, 'matrix' (default) or 'fused' (`evaluate_on_device`); the
    host-array evaluations (on_device=False) use no device search and ignore it.  Another name: ValueError.
    information: with on_device, also results['information'] -- the (n_labels, k) information matrix between the internal
    coefficients of the test rows (all modalities) and their labels (`DeviceEvaluation.information_matrix`; the reference's
    samples/plot_info_matrix.py:126-136) -- and results['information_labels'], the sorted distinct labels of labels_test and
    labels_ex that index its rows.  False (default): no further call and the keys of before."""
    from .device_data import DeviceDataset
    _check_search(search)
    if not isinstance(dataset, DeviceDataset):
        dataset = DeviceDataset(dataset, keep_sparse=bool(keep_sparse), presence=presence)
    elif keep_sparse is not None and bool(keep_sparse) != dataset.keep_sparse_asked:
        raise ValueError("keep_sparse=%r, but the dataset was uploaded with keep_sparse=%r" % (keep_sparse, dataset.keep_sparse_asked))
    elif presence is not None and not dataset.same_presence(presence):
        raise ValueError("presence= differs from the mask the dataset was uploaded with")
    learner = MultimodalLearner(list(modalities), list(dataset.dims), list(coefs), k)
    dataset.train(learner, rows_train, iter_train, init_dictionary=init_dictionary)
    results = {'train': list(rows_train), 'test': list(rows_test), 'dictionary': learner.get_dico()}
    if kind is None:
        kind = 'two' if len(learner.mod) == 2 else 'internal'
    if on_device:      # dictionary, coefficients and reconstructions stay on the GPU (DeviceEvaluation)
        ev = evaluate_on_device if kind == 'two' else evaluate_internal_on_device
    else:              # the host-array path of round 2 (every transform returns numpy arrays)
        ev = evaluate if kind == 'two' else evaluate_internal
    extra = {'search': search} if on_device else {}
    results.update(ev(dataset, learner, rows_test, rows_ex, labels_test, labels_ex, iter_test, **extra))
    if information and on_device:
        from .device_data import DeviceEvaluation
        names = sorted(set(labels_test) | set(labels_ex))
        index = {label: i for i, label in enumerate(names)}
        results['information_labels'] = names
        results['information'] = DeviceEvaluation(dataset, learner, iter_test).information_matrix(
            list(learner.mod), rows_test, [index[label] for label in labels_test], len(names))
    return learner, results


def _sweep_split(dataset, examples, k, run, test_ratio, seed):
    """(train rows, test rows, H0) of the job (k, run): from a stream seeded by (seed, k, run) alone."""
    rs = np.random.RandomState([seed, k, run])
    n_all = dataset.n_samples
    others = [i for i in range(n_all) if i not in set(examples)]
    perm = rs.permutation(len(others))
    n_test = max(1, int(round(test_ratio * len(others))))
    test = [others[i] for i in perm[:n_test]]
    train = [others[i] for i in perm[n_test:]]
    f = sum(dataset.dims)
    H0 = rs.random_sample((k, f)) + .01                      # the init rule of nmf.py:149-151 from the job's own stream
    H0 /= 1e-16 + H0.sum(axis=1, keepdims=True)
    return train, test, H0


def _one_sweep_job(dataset, modalities, coefs, labels, examples, k, run, iter_train, iter_test, test_ratio, seed, kind,
                   search='matrix'):
    """One job of the reference's sweep (samples/launcher.py:71-99: an experiment with run_mode 'single' = one random
    test_ratio split, experiment.py:131-133): seeded per (k, run), so that it does not matter which rank executes it."""
    train, test, H0 = _sweep_split(dataset, examples, k, run, test_ratio, seed)
    _, res = perform_one_run(dataset, modalities, coefs, k, iter_train, iter_test, train, test, list(examples),
                             [labels[t] for t in test], [labels[e] for e in examples], init_dictionary=H0, kind=kind, search=search)
    return {kk: float(v) for kk, v in res.items() if kk.startswith('score_')}


def _sweep_batch(dataset, modalities, coefs, labels, examples, k, runs, iter_train, iter_test, test_ratio, seed, kind,
                 search='matrix'):
    """The jobs (k, run) for run in `runs` as one batch: the trainings by `DeviceDataset.train_many`, every internal transform of
    their evaluations by `DeviceEvaluation.internal_many`; reconstructions and scores per run; the nearest-example searches per
    run, comparison and measure (search='matrix') or those of ALL runs of the batch in one launch (search='fused').  Seeds per
    (k, run), as `_one_sweep_job`'s: which batch a run lands in does not matter."""
    from .device_data import DeviceEvaluation
    _check_search(search)
    splits = [_sweep_split(dataset, examples, k, run, test_ratio, seed) for run in runs]
    learners = [MultimodalLearner(list(modalities), list(dataset.dims), list(coefs), k) for _ in runs]
    dataset.train_many(learners, [sp[0] for sp in splits], iter_train, init_dictionaries=[sp[2] for sp in splits])
    if kind is None:
        kind = 'two' if len(modalities) == 2 else 'internal'
    evs = [DeviceEvaluation(dataset, learner, iter_test) for learner in learners]
    internals = [{} for _ in runs]
    for mods in internal_sets(kind, len(modalities)):
        names = [modalities[m] for m in mods]
        for side, rows_list in (('test', [sp[1] for sp in splits]), ('ex', [list(examples)] * len(runs))):
            for got, t in zip(internals, DeviceEvaluation.internal_many(evs, names, rows_list)):
                got[(mods, side)] = t
    if search == 'fused':      # every run lists its searches; one call resolves them all
        lister = list_searches_on_device if kind == 'two' else list_internal_searches_on_device
        listed = [lister(dataset, learner, test, list(examples), [labels[t] for t in test], [labels[e] for e in examples], iter_test,
                         ev=ev, internals=got) for learner, ev, got, (_train, test, _H0) in zip(learners, evs, internals, splits)]
        found = _resolve_searches(evs[0], [s for mine in listed for s in mine], search)
        out, at = [], 0
        for run, mine in zip(runs, listed):
            res = _results_of(mine, found[at:at + len(mine)])
            at += len(mine)
            out.append((k, run, {kk: float(v) for kk, v in res.items() if kk.startswith('score_')}))
        return out
    evaluate_ = evaluate_on_device if kind == 'two' else evaluate_internal_on_device
    out = []
    for run, learner, ev, got, (_train, test, _H0) in zip(runs, learners, evs, internals, splits):
        res = evaluate_(dataset, learner, test, list(examples), [labels[t] for t in test], [labels[e] for e in examples], iter_test,
                        ev=ev, internals=got)
        out.append((k, run, {kk: float(v) for kk, v in res.items() if kk.startswith('score_')}))
    return out


def sweep_batches(pairs, batch):
    """The (k, run) pairs of one worker as batches: lists of pairs of ONE k, at most `batch` each, every pair in exactly one;
    the ks in the order they first occur, the pairs of a k in their order.  batch = 1: one pair per batch, in `pairs`' order."""
    batch = max(1, int(batch))
    if batch == 1:
        return [[pair] for pair in pairs]
    by_k = {}
    for k, run in pairs:
        by_k.setdefault(k, []).append((k, run))
    return [group[i:i + batch] for group in by_k.values() for i in range(0, len(group), batch)]


def _sweep_worker(job):
    """One process per GPU: uploads the modalities once, runs its share of the (k, run) grid, returns the scores."""
    (device, rank, world, data, modalities, coefs, labels, examples, ks, n_runs, iter_train, iter_test, test_ratio, seed, kind,
     precision, keep_sparse, presence, batch, search) = job
    import os
    import torch
    saved = {name: os.environ.get(name) for name in ('KLNMF_PRECISION', 'KLNMF_DEVICE', 'KLNMF_DEVICES')}
    try:       # (the learner's NMF objects read their mode and device from the environment, as experiment.py's would)
        if precision is not None:
            os.environ['KLNMF_PRECISION'] = precision
        os.environ['KLNMF_DEVICE'] = str(device)
        os.environ.pop('KLNMF_DEVICES', None)      # (a sweep is replica-parallel: every learner of this worker on its one device)
        torch.cuda.set_device(device)
        from .device_data import DeviceDataset
        ds = DeviceDataset(data, device=device, keep_sparse=keep_sparse, presence=presence)
        out = []
        for group in sweep_batches(sweep_assignment(ks, n_runs, rank, world), batch):
            if len(group) == 1:      # (batch = 1: today's path, call for call)
                k, run = group[0]
                out.append((k, run, _one_sweep_job(ds, modalities, coefs, labels, examples, k, run, iter_train, iter_test,
                                                   test_ratio, seed, kind, search=search)))
            else:
                out.extend(_sweep_batch(ds, modalities, coefs, labels, examples, group[0][0], [run for _, run in group], iter_train,
                                        iter_test, test_ratio, seed, kind, search=search))
        return out
    finally:   # a one-device sweep runs in the caller's process: leave its environment as it was
        for name, value in saved.items():
            if value is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = value


def run_sweep(data_matrices, labels, modalities, ks, n_runs, iter_train=50, iter_test=50, coefs=None, examples=None,
              test_ratio=.1, seed=0, devices=None, precision=None, kind=None, keep_sparse=False, presence=None, batch=1,
              search='matrix'):
    """The k sweep of the reference's launcher (samples/launcher.py:68-99, 122-126: Ks x N_RUN independent experiments,
    one OS process each) on the GPUs of this node: ONE process per device, each with the modalities resident on its GPU,
    executing `sweep_assignment`'s share of the (k, run) grid -- replica parallelism, no communication.  Returns
    (table, raw): table[k][score key] = (mean, std) over the runs -- what `Logger.merge_experiments(...).get_stats(key)`
    gives the launcher's plots (launcher.py:137-149) -- and raw = [(k, run, {score key: value})].

    data_matrices: one [n_samples, d_m] array per modality, samples paired across modalities; labels: one per sample;
    examples: the row of the example of each label (default: the first sample of every label, evaluation happens on the
    rest); coefs: per-modality coefficients (default 1 / mean row sum, experiment.py:70-72); devices: GPU ordinals
    (default: all visible; the same ordinal may be listed more than once); keep_sparse: scipy-sparse modalities stay CSR on every
    device and the runs take the reference's sparse branch (`DeviceDataset`; default: densified, as before); presence: a row x
    modality presence mask kept on every device beside the modalities (`DeviceDataset(presence=...)`, checked here before any
    process starts): the runs' fits and transforms on masked modalities minimise the masked cost.  The default coefficients
    stay 1 / the mean row sum over all samples, absent ones included.
    batch: each worker runs its (k, run) pairs of equal k in batches of at most `batch` (`sweep_batches`): the trainings and the
    evaluations' internal transforms of a batch as one launch sequence (klnmf_batch_*) where the shapes allow it (dense
    modalities, f64 / f32; with `presence`: the masked batch, every run its own rows of the mask; with `keep_sparse`: the CSR
    batch, every run its own stored entries, k <= 512); 1 (default): one pair after
    another, as before.
    search: 'matrix' (default) -- every nearest-example search of an evaluation brings its distance matrix to the host, as
    before; 'fused' -- the searches of a run (batch = 1) or of all runs of a batch are one launch that returns the indices
    (klnmf_nearest_many_device): the same labels and scores.  Another name: ValueError."""
    import torch
    _check_search(search)
    if keep_sparse:
        data = [m.tocsr() if hasattr(m, 'tocsr') else np.asarray(m) for m in data_matrices]
    else:
        data = [np.asarray(m.toarray() if hasattr(m, 'toarray') else m) for m in data_matrices]
    labels = [int(v) for v in labels]
    if presence is not None:
        from .device_data import check_presence
        check_presence(presence, data[0].shape[0], len(data))
        presence = [None if (p is None or np.ndim(p) == 0) else np.asarray(p) for p in presence]
    if coefs is None:
        coefs = [float(1. / np.average(x.sum(axis=1))) for x in data]
    if examples is None:
        examples = [labels.index(l) for l in sorted(set(labels))]
    if devices is None:
        devices = list(range(max(1, torch.cuda.device_count())))
    world = len(devices)
    jobs = [(dev, r, world, data, list(modalities), list(coefs), labels, list(examples), list(ks), int(n_runs), iter_train,
             iter_test, test_ratio, seed, kind, precision, bool(keep_sparse), presence, int(batch), search)
            for r, dev in enumerate(devices)]
    if world == 1:
        parts = [_sweep_worker(jobs[0])]
    else:
        import multiprocessing as mp
        with mp.get_context('spawn').Pool(world) as pool:       # fresh processes: each initialises HIP on its own device
            parts = pool.map(_sweep_worker, jobs)
    raw = sorted((k, run, sc) for part in parts for (k, run, sc) in part)
    table = {}
    for k in ks:
        runs = [sc for kk, _, sc in raw if kk == k]
        table[k] = {key: (float(np.mean([r[key] for r in runs])), float(np.std([r[key] for r in runs]))) for key in runs[0]}
    return table, raw


def sweep_assignment(ks, n_runs, rank=0, world_size=1):
    """(k, run) pairs of a sweep that rank `rank` of `world_size` executes: round robin over the flattened grid, so that
    the expensive large-k fits spread evenly.  Every pair is assigned to exactly one rank."""
    grid = [(k, r) for k in ks for r in range(n_runs)]
    return grid[rank::world_size]
