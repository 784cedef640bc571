"""Writes tests/golden/g23_motion.npz: the REFERENCE's own outputs for the stages of its `db_to_VQ_hist_matrix`
(multimodal/features/angle_histograms.py:171-223), which the host twin of multimodal_amd/features/angle_histograms.py is pinned to.

    python tests/golden/make_golden_motion.py <reference checkout>

What is called: the reference's `record_to_angle_array` (on its lib/transformations.py), `delayed_velocities` (lib/utils.py),
`get_histos` (lib/vector_quantization.py), and scipy's `whiten` and `kmeans`, the two functions the reference imports.  The
reference module imports lib/kde2d.py, which imports `scipy.integrate.trapz` (gone from scipy 1.15): a stand-in module takes its
place for the import only; nothing of it is used.

What is restated: `db_to_VQ_hist_matrix` itself cannot be CALLED under Python 3 -- its `map` objects (`filter_values`,
`compacted`) are consumed twice -- so its lines :199-223 are written out below in `vq_hist_lines` with lists, around the same
calls in the same order.

Two sets.  'w': 6 seeded examples of 20-24 frames, the 13 markers `ANGLES` names and a spare, nb_bins = 4, whitened as the
reference does.  To keep the file below 200 KB the examples are short, the records hold float32 values and no translation, and
the velocities with a delay or padding other than (1, 'zeros') are recorded for every sixth column.  'g': two point sets on a grid (multiples of 2^-10, not whitened), where every cluster sum is exact in any order
of addition, so that codebooks can be compared by equality.

Conditions asserted here (not tolerances): at every assignment of every recorded k-means run the nearest and second-nearest
squared distances differ by more than 1e-6 relative; at every stop decision |diff - thresh| / thresh > 1e-3; no two restarts of a
seeded call tie in distortion; the init made for it loses exactly one cluster."""
import os
import sys
import types

import numpy as np

NAMES = ['spare', 'torso', 'left_shoulder', 'left_elbow', 'left_hand', 'left_hip', 'left_knee', 'left_foot', 'right_shoulder',
         'right_elbow', 'right_hand', 'right_hip', 'right_knee', 'right_foot']
VEL_COLUMNS = slice(0, None, 6)                # the columns recorded of the velocity variants other than (1, 'zeros')
THRESH = 1e-5
SEED_W, SEED_G = 11, 12
NB_BINS, K_GRID, RESTARTS = 4, 8, 3
DELAYS = ((1, 'zeros'), (1, 'circular'), (10, 'zeros'), (10, 'circular'))


def stand_in_kde():
    mod = types.ModuleType('multimodal.lib.kde2d')
    mod.gaussian_kde_2d = None
    sys.modules['multimodal.lib.kde2d'] = mod


def trace(points, init, label):
    """scipy's `_kmeans` loop restated to look at every assignment and stop decision; returns (iterations, least gap, least
    margin).  The caller compares its result with `kmeans`' own."""
    from scipy.cluster.vq import _vq
    book, prev, gaps, margins = np.array(init), np.inf, [], []
    for it in range(1, 1000):
        d2 = np.sort(((points[:, None, :] - book[None, :, :]) ** 2).sum(-1), axis=1)
        if book.shape[0] > 1:
            gaps.append(((d2[:, 1] - d2[:, 0]) / d2[:, 1]).min())
        codes = np.argmin(((points[:, None, :] - book[None, :, :]) ** 2).sum(-1), axis=1)
        now = np.sqrt(d2[:, 0]).mean()
        book, has = _vq.update_cluster_means(points, codes.astype(np.int32), book.shape[0])
        book = book[has]
        diff = abs(prev - now)
        prev = now
        if np.isfinite(diff):
            margins.append(abs(diff - THRESH) / THRESH)
        if diff <= THRESH:
            assert min(gaps + [1.0]) > 1e-6, (label, min(gaps))
            assert min(margins + [1.0]) > 1e-3, (label, min(margins))
            return it, book, now, min(gaps + [1.0]), min(margins + [1.0])
    raise AssertionError(label)


def checked_kmeans(points, init, label, stats):
    from scipy.cluster.vq import kmeans
    book, dist = kmeans(points, init, thresh=THRESH)
    it, tbook, tdist, gap, margin = trace(points, init, label)
    assert tbook.shape == book.shape and np.allclose(tbook, book, rtol=1e-12, atol=0) and abs(tdist - dist) <= 1e-12 * dist, label
    stats['gap'], stats['margin'] = min(stats['gap'], gap), min(stats['margin'], margin)
    return book, dist, it


def first_seeds(sets, k, start, label, stats):
    """(seeds, [`seeded_kmeans` of set s under seeds[s]]): per set the first seed from `start` on under which every condition
    holds -- restarts that reach the same optimum tie, which is common with few bins, so seeds are tried in order."""
    seeds, out = [], []
    for s, p in enumerate(sets):
        for seed in range(start, start + 500):
            try:
                seeded_kmeans([p], k, seed, label, dict(stats))
            except AssertionError:
                continue
            seeds.append(seed)
            out.append(seeded_kmeans([p], k, seed, '%s set %d' % (label, s), stats)[0])
            break
        else:
            raise AssertionError('no seed for %s set %d' % (label, s))
    return np.array(seeds), out


def seeded_kmeans(sets, k, seed, label, stats):
    """`kmeans(points, k, iter=RESTARTS)` per set under one np.random.seed(seed), the reference's :212 (the fixture calls it
    with one set and that set's seed); the draws are replayed with RandomState(seed) to check every restart's conditions."""
    from scipy.cluster.vq import kmeans
    np.random.seed(seed)
    out = [kmeans(p, k, iter=RESTARTS, thresh=THRESH) for p in sets]
    replay = np.random.RandomState(seed)
    for s, p in enumerate(sets):
        dists = []
        for r in range(RESTARTS):
            rows = replay.choice(p.shape[0], size=k, replace=False)
            dists.append(checked_kmeans(p, p[rows], '%s set %d restart %d' % (label, s, r), stats)[1])
        assert len(set(dists)) == RESTARTS, (label, s, dists)                  # no tie
        assert min(dists) == out[s][1], (label, s)
    return out


def vq_hist_lines(angles, vels, centro, soft_vq, get_histos, whiten):
    """features/angle_histograms.py:199-223 with lists for its `map` objects; `centro` stands for :212's result."""
    nb_dofs = angles[0].shape[1]
    nb_ex = len(angles)
    data = [[np.hstack([a[:, dof][:, np.newaxis], v[:, dof][:, np.newaxis]]) for a, v in zip(angles, vels)]
            for dof in range(nb_dofs)]
    compacted = [(np.vstack(x), list(np.cumsum([y.shape[0] for y in x]))) for x in data]        # compact_examples
    all_data = [whiten(d) for d, _ in compacted]
    histos = [get_histos(d, c, soft=soft_vq) for d, c in zip(all_data, centro)]
    histos_by_ex = [[h[i:j, :] for i, j in zip([0] + c[1][:-1], c[1])] for h, c in zip(histos, compacted)]   # un_compact_examples
    ex_histos = np.array([[h.sum(axis=0) for h in hs] for hs in histos_by_ex])
    nb_bins = ex_histos.shape[2]
    Xdata = np.swapaxes(ex_histos, 0, 1).reshape((nb_ex, nb_bins * nb_dofs))
    Xdata /= Xdata.sum(axis=1)[:, np.newaxis]
    return Xdata


def main(reference):
    stand_in_kde()
    sys.path.insert(0, reference)
    from multimodal.features import angle_histograms as rah
    from multimodal.lib.utils import delayed_velocities
    from multimodal.lib.vector_quantization import get_histos
    from scipy.cluster.vq import whiten

    out = {'names': np.array(NAMES), 'thresh': THRESH, 'restarts': RESTARTS}
    stats = {'gap': 1.0, 'margin': 1.0}

    # ---- set 'w' ----
    rng = np.random.default_rng(SEED_W)
    lengths = [20, 24, 21, 23, 20, 22]
    records = []
    for n in lengths:              # smooth random quaternion paths, not normalised; float32 values and no translation (file size)
        base = rng.normal(size=(1, len(NAMES), 7))
        path = (base + np.cumsum(0.15 * rng.normal(size=(n, len(NAMES), 7)), axis=0)).astype(np.float32).astype(np.float64)
        path[:, :, :3] = 0.0
        records.append(path)
    idx = rah.angles_indices(NAMES)
    angles = [rah.record_to_angle_array(r, idx) for r in records]
    out['w_records'] = np.concatenate(records)
    out['w_offsets'] = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    out['w_angles'] = np.vstack(angles)
    for delay, padding in DELAYS:
        v = np.vstack([delayed_velocities(delay, a, padding=padding) for a in angles])
        out['w_vels_%d_%s' % (delay, padding)] = v if (delay, padding) == (1, 'zeros') else np.ascontiguousarray(v[:, VEL_COLUMNS])
    vels = [delayed_velocities(1, a, padding='zeros') for a in angles]          # :192
    D = angles[0].shape[1]
    white = [whiten(np.hstack([out['w_angles'][:, s][:, None], out['w_vels_1_zeros'][:, s][:, None]])) for s in range(D)]
    out['w_white'] = np.stack(white)
    T = out['w_white'].shape[1]
    init = np.stack([w[rng.choice(T, size=NB_BINS, replace=False)] for w in white])
    fixed = [checked_kmeans(w, i, 'w init %d' % s, stats) for s, (w, i) in enumerate(zip(white, init))]
    assert all(f[0].shape == (NB_BINS, 2) for f in fixed)
    out['w_init'], out['w_init_cb'] = init, np.stack([f[0] for f in fixed])
    out['w_init_dist'], out['w_init_iters'] = np.array([f[1] for f in fixed]), np.array([f[2] for f in fixed])
    seed_w, seeded = first_seeds(white, NB_BINS, SEED_W, 'w', stats)
    assert all(cb.shape == (NB_BINS, 2) for cb, _ in seeded)
    out['w_seed'] = seed_w
    out['w_seed_cb'], out['w_seed_dist'] = np.stack([cb for cb, _ in seeded]), np.array([d for _, d in seeded])
    centro = [cb for cb, _ in seeded]
    out['w_hard'] = vq_hist_lines(angles, vels, centro, None, get_histos, whiten)
    out['w_soft'] = vq_hist_lines(angles, vels, centro, .5, get_histos, whiten)
    far = init[0].copy()
    far[1] = [1e3, -1e3]                                                       # a centroid no point is nearest to
    dropped = checked_kmeans(white[0], far, 'w dropped', stats)
    assert dropped[0].shape == (NB_BINS - 1, 2)
    out['w_far_init'], out['w_far_cb'], out['w_far_dist'] = far, dropped[0], dropped[1]

    # ---- set 'g' ----
    rng = np.random.default_rng(SEED_G)
    centres = rng.integers(-4096, 4096, size=(2, K_GRID, 2))
    sets = [(centres[s][rng.integers(0, K_GRID, 600)] + rng.integers(-700, 700, size=(600, 2))) / 1024.0 for s in range(2)]
    out['g_points'] = np.stack(sets)
    out['g_offsets'] = np.array([0, 1, 130, 256, 257, 600], dtype=np.int64)
    ginit = np.stack([p[rng.choice(600, size=K_GRID, replace=False)] for p in sets])
    gfixed = [checked_kmeans(p, i, 'g init %d' % s, stats) for s, (p, i) in enumerate(zip(sets, ginit))]
    assert all(f[0].shape == (K_GRID, 2) for f in gfixed)
    out['g_init'], out['g_init_cb'] = ginit, np.stack([f[0] for f in gfixed])
    out['g_init_dist'], out['g_init_iters'] = np.array([f[1] for f in gfixed]), np.array([f[2] for f in gfixed])
    seed_g, gseeded = first_seeds(sets, K_GRID, SEED_G, 'g', stats)
    assert all(cb.shape == (K_GRID, 2) for cb, _ in gseeded)
    out['g_seed'] = seed_g
    out['g_seed_cb'], out['g_seed_dist'] = np.stack([cb for cb, _ in gseeded]), np.array([d for _, d in gseeded])
    gfar = ginit[1].copy()
    gfar[5] = [4000.0, 4000.0]
    gdropped = checked_kmeans(sets[1], gfar, 'g dropped', stats)
    assert gdropped[0].shape == (K_GRID - 1, 2)
    out['g_far_init'], out['g_far_cb'], out['g_far_dist'] = gfar, gdropped[0], gdropped[1]
    bounds = out['g_offsets']
    for soft, name in ((None, 'g_hard'), (.5, 'g_soft')):
        h = [get_histos(p, cb, soft=soft) for p, (cb, _) in zip(sets, gseeded)]
        X = np.array([[x[a:b].sum(axis=0) for x in h] for a, b in zip(bounds[:-1], bounds[1:])]).reshape(len(bounds) - 1, -1)
        out[name] = X / X.sum(axis=1)[:, np.newaxis]

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'g23_motion.npz')
    np.savez_compressed(path, **out)
    print('seeds of the seeded calls: w %s, g %s' % (list(seed_w), list(seed_g)))
    print('least relative gap between the two nearest codes: %.3g' % stats['gap'])
    print('least |diff - thresh| / thresh at a stop decision: %.3g' % stats['margin'])
    print('%s: %d bytes' % (path, os.path.getsize(path)))
    report_twin(out)


def report_twin(g):
    """The twin's worst deviations from the recorded values (the bars of tests/test_motion_cpu.py are derived, not these)."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from multimodal_amd.features import angle_histograms as ah
    a, v, off = ah.host_angle_arrays((g['w_records'], g['w_offsets']), list(g['names']))
    print('angles: worst |twin - reference| = %.3g (ulp of pi: %.3g)' % (np.abs(a - g['w_angles']).max(), np.spacing(np.pi)))
    white = ah.host_whiten(np.stack([g['w_angles'], g['w_vels_1_zeros']], axis=2).reshape(a.shape[0], -1))[0]
    sets = white.reshape(a.shape[0], -1, 2).transpose(1, 0, 2)
    print('whitened points: worst relative = %.3g' % (np.abs(sets - g['w_white']) / np.abs(g['w_white']).clip(1e-300)).max())
    runs = [ah.host_kmeans_converged_from(g['w_white'][s], g['w_init'][s], THRESH) for s in range(sets.shape[0])]
    print('codebooks from the recorded init: worst relative = %.3g, iterations equal: %s'
          % (max((np.abs(r[0] - cb) / np.abs(cb)).max() for r, cb in zip(runs, g['w_init_cb'])),
             [r[3] for r in runs] == list(g['w_init_iters'])))
    for tag in ('hard', 'soft'):
        X = ah.host_histograms(g['w_white'], g['w_seed_cb'], g['w_offsets'], None if tag == 'hard' else .5)
        print('%s matrix on the recorded codebooks: worst relative = %.3g' % (tag, (np.abs(X - g['w_' + tag]) / g['w_' + tag].clip(1e-300)).max()))


if __name__ == '__main__':
    main(sys.argv[1])
