#!/usr/bin/env python3
"""What the motion modality costs on the device, against the same work with scipy on the host of the same machine.

Shape: E = 1 000 examples x 150 frames (T = 150 000), 15 markers, the 10 pairs of ANGLES (D = 30 degrees of freedom),
nb_bins = 16, iter = 20 restarts: P = 600 k-means problems of 150 000 points in the plane.  Records: smooth random quaternion
paths, float64.

  (a) `vq_hist_matrix` end to end, hard and soft, from device tensors and from host arrays: one warm-up, then `--runs` runs timed
      with a host clock that ends in a synchronise; the median.  The number of Lloyd iterations the slowest problem needed is
      printed with it: the batch runs until its last problem stops.
  (b) the same work by the host's pieces.  The reference's angle stage is one Python call per frame and joint
      (features/angle_histograms.py:45-67); here the vectorised twin is called once per frame and joint on a one-frame slice,
      which makes the same number of calls of a comparable handful of numpy operations each -- a stand-in, labelled as one --
      on 1 / 100 of the frames, scaled by 100.  scipy's `whiten`, `kmeans(points, 16, iter=20)` and the hard histogram
      (`vq` and a one-hot sum) are timed on ONE degree of freedom with 2 restarts and scaled by 30 x 10 (kmeans) and 30 (the rest).
  (c) one Lloyd iteration of the whole batch (two launches: k_mo_assign, k_mo_update): the k-means call is run with thresh = 0 to
      max_iter = 8 and to max_iter = 4 (no problem stops, every workgroup works), the difference over 4 -- against the bytes an
      iteration must read, points x problems (T * 2 * 8 * P; no labels are written in the pipeline) at the 6.3 TB/s stream rate,
      and against its separately rounded fp64 instructions, 3 * T * K * d * P for the distances alone at 39.3 T instructions/s.

    python scripts/motion_timing.py [--runs 3]          # writes profiles/motion_timing.txt
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
E, FRAMES, K, RESTARTS = 1000, 150, 16, 20
NAMES = ['head', 'neck', 'torso', 'left_shoulder', 'left_elbow', 'left_hand', 'right_shoulder', 'right_elbow', 'right_hand',
         'left_hip', 'left_knee', 'left_foot', 'right_hip', 'right_knee', 'right_foot']
STREAM_PEAK, FP64_INSTR_PEAK = 6.3e12, 39.3e12


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'motion_timing.txt'))
    args = ap.parse_args()
    import torch
    from multimodal_amd import _native
    from multimodal_amd.features import angle_histograms as ah
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(1)
    T = E * FRAMES
    rec = (rng.normal(size=(E, 1, len(NAMES), 7)) + np.cumsum(0.05 * rng.normal(size=(E, FRAMES, len(NAMES), 7)), axis=1))
    rec = rec.reshape(T, len(NAMES), 7)
    offsets = np.arange(E + 1, dtype=np.int64) * FRAMES
    d_rec = torch.from_numpy(rec).to('cuda')
    say('motion modality, %s, E = %d x %d frames (T = %d), %d markers, D = 30, nb_bins = %d, iter = %d (P = %d), float64'
        % (torch.cuda.get_device_name(0), E, FRAMES, T, len(NAMES), K, RESTARTS, 30 * RESTARTS))

    # (a)
    kw = dict(nb_bins=K, iter=RESTARTS, rng=3)
    ah.vq_hist_matrix((d_rec[:3000], offsets[:21]), NAMES, nb_bins=4, iter=2, rng=1, output='device')          # warm-up
    for label, source, out in (('device tensors', d_rec, 'device'), ('host arrays', rec, 'numpy')):
        for soft in (None, .5):
            times = [wall(lambda: ah.vq_hist_matrix((source, offsets), NAMES, soft_vq=soft, output=out, **kw))[0] for _ in range(args.runs)]
            say('(a) vq_hist_matrix from %-14s %s: median %.3f s of %s' % (label, 'soft' if soft else 'hard', np.median(times),
                                                                           ['%.3f' % t for t in times]))
    angles, vels, _ = ah.angle_arrays((d_rec, offsets), NAMES, output='device')
    t_angles = np.median([wall(lambda: ah.angle_arrays((d_rec, offsets), NAMES, output='device'))[0] for _ in range(args.runs)])
    say('    of which angles and velocities (2 launches): %.2f ms' % (1e3 * t_angles))
    dv = ah._Device(None, True)
    pts = torch.stack([angles, vels], dim=2).reshape(T, 60).contiguous()
    t_white = np.median([wall(lambda: ah._whiten_on(dv, pts.clone()))[0] for _ in range(args.runs)])
    say('    whitening of 60 columns (5 launches, with a 72 MB clone): %.2f ms' % (1e3 * t_white))
    ah._whiten_on(dv, pts)
    by_set = pts.view(T, 30, 2)
    t_km, runs = wall(lambda: ah._restarts_on(dv, pts, lambda s: by_set[:, s], 2, 60, T, 2, 30, K, RESTARTS, 1e-5, np.random.default_rng(3), 1000))
    iters = runs.iters.cpu().numpy()
    say('    batched k-means: %.3f s; iterations per problem min %d median %d max %d, sum %d'
        % (t_km, iters.min(), int(np.median(iters)), iters.max(), iters.sum()))

    # (c)
    rows = ah.draw_rows(np.random.default_rng(3), T, K, RESTARTS, 30)
    idx = torch.from_numpy(rows).to('cuda')
    init = torch.stack([by_set[:, s][idx[s]] for s in range(30)]).reshape(600, K, 2)
    set_of = np.repeat(np.arange(30, dtype=np.int32), RESTARTS)

    def fixed(n):
        try:
            ah._Runs(dv, pts, 2, 60, T, 2, 30, set_of, init.clone(), 0.0, n)
        except RuntimeError:
            pass
    fixed(4)
    t8 = np.median([wall(lambda: fixed(8))[0] for _ in range(args.runs)])
    t4 = np.median([wall(lambda: fixed(4))[0] for _ in range(args.runs)])
    per = (t8 - t4) / 4
    read = T * 2 * 8 * 600
    instr = 3 * T * K * 2 * 600
    say('(c) one Lloyd iteration of the 600 problems: %.3f ms  (8 iterations %.1f ms, 4 iterations %.1f ms)' % (1e3 * per, 1e3 * t8, 1e3 * t4))
    say('    bytes it must read: %.2f GB = %.3f ms at 6.3 TB/s (%.1f %% of the stream rate reached)'
        % (read / 1e9, 1e3 * read / STREAM_PEAK, 100 * read / STREAM_PEAK / per))
    say('    fp64 instructions of the distances alone: %.2e = %.3f ms at 39.3 T/s (%.1f %% of the vector pipe)'
        % (instr, 1e3 * instr / FP64_INSTR_PEAK, 100 * instr / FP64_INSTR_PEAK / per))

    # (b)
    from scipy.cluster.vq import kmeans, vq, whiten
    pairs = ah.angles_indices(NAMES)
    part = rec[:T // 100]
    t0 = time.perf_counter()
    for frame in part:
        np.hstack([ah.host_angle_array(frame[np.newaxis], [pair])[0] for pair in pairs])
    t_loop = (time.perf_counter() - t0) * 100
    say('(b) host: angle stage, one call per frame and joint (stand-in for the reference\'s loop; 1 / 100 of the frames x 100): %.1f s' % t_loop)
    h_angles, h_vels = angles.cpu().numpy(), vels.cpu().numpy()
    one = np.stack([h_angles[:, 0], h_vels[:, 0]], axis=1)
    t0 = time.perf_counter()
    w = whiten(one)
    t_w = (time.perf_counter() - t0) * 30
    np.random.seed(3)
    t0 = time.perf_counter()
    cb, _ = kmeans(w, K, iter=2)
    t_k = (time.perf_counter() - t0) * 30 * RESTARTS / 2
    t0 = time.perf_counter()
    codes, _ = vq(w, cb)
    h = np.eye(cb.shape[0])[codes]
    np.array([h[a:b].sum(axis=0) for a, b in zip(offsets[:-1], offsets[1:])])
    t_h = (time.perf_counter() - t0) * 30
    say('    host: scipy whiten %.2f s, kmeans(points, 16, iter=20) %.0f s (one degree of freedom, 2 restarts, x 30 x 10), hard '
        'histograms %.2f s (x 30)' % (t_w, t_k, t_h))
    say('    host total (estimate): %.0f s' % (t_loop + t_w + t_k + t_h))
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
