#!/usr/bin/env python3
"""What the MFCC front end costs on the device, against the host twin on the same machine.

One corpus -- 2 000 utterances of 2 to 4 s at 16 kHz, int16, gliding tones over a noise floor -- under two parameter sets:

  * matlab:   n_fft 320, hop 160, 30 filters, 13 coefficients (the direct route);
  * defaults: n_fft 2048, hop 512, 128 filters, 13 coefficients (the fft route).

Per set: `features.mfcc.mfcc_streams(..., output='device')` timed with a host clock that ends in a synchronise, the median of
`--runs` runs after one warm-up (min ... max), once from samples already on the device and once from host arrays (the upload
counted); the host twin `host_mfcc_streams` in one process, timed once on `--twin-utterances` utterances and scaled; k_mfcc_mel's
rate on its algorithmic bytes (every sample read once per overlap factor n_fft / hop, the energies written); and `hac_many`
(codebooks of 150 / 150 / 100 units, lags [5, 2]) against the sum of its two stages timed apart.  No bar: the file records what
was seen.  Per-kernel times come from a run of their own:

    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/mfcc_timing.py --once matlab

Each set runs in a child process of its own under its own time limit; a set that fails or overruns ends the script.

    python scripts/mfcc_timing.py [--runs 7]          # writes profiles/mfcc_timing.txt
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SR = 16000
SETS = {'matlab': dict(n_mfcc=13, n_fft=320, hop_length=160, n_mels=30), 'defaults': dict(n_mfcc=13, n_fft=2048, hop_length=512, n_mels=128)}
LIMIT = 600        # a child's time limit in seconds
KS, LAGS = (150, 150, 100), [5, 2]


def corpus(n=2000):
    rng = np.random.default_rng(11)
    out = []
    for L in rng.integers(2 * SR, 4 * SR + 1, n):
        t = np.arange(L) / float(SR)
        f0, f1 = rng.uniform(200, 6000, 2)
        y = 6000 * np.sin(2 * np.pi * (f0 * t + 0.5 * (f1 - f0) * t * t / t[-1])) + rng.normal(0, 200, L)
        out.append(np.round(y).astype(np.int16))
    return out


def line(what, times):
    return '%-76s %9.5f s  (%.5f ... %.5f)' % (what, float(np.median(times)), min(times), max(times))


def run_set(name, runs, twin_utterances, once):
    import torch
    from multimodal_amd import _native
    from multimodal_amd.features import hac, mfcc as fm
    p = SETS[name]
    ys = corpus()
    samples = np.concatenate(ys)
    offsets = np.concatenate([[0], np.cumsum([len(y) for y in ys])]).astype(np.int64)
    T = int(fm.frame_counts(np.diff(offsets), p['hop_length']).sum())

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    d_samples = torch.from_numpy(samples).to('cuda')
    from_device = lambda: fm.mfcc_streams((d_samples, offsets), SR, output='device', **p)
    from_host = lambda: fm.mfcc_streams(ys, SR, output='device', **p)
    wall(from_device)                                  # the warm-up
    if once:
        wall(from_device)
        return
    print('%s set: %d utterances, %.1f M samples (int16), n_fft %d, hop %d, %d filters, %d coefficients -> %d frames; route %s'
          % (name, len(ys), len(samples) / 1e6, p['n_fft'], p['hop_length'], p['n_mels'], p['n_mfcc'], T,
             _native.mfcc_route(p['n_fft'])), flush=True)
    print(line('mfcc_streams from samples on the device', [wall(from_device)[0] for _ in range(runs)]), flush=True)
    wall(from_host)
    print(line('mfcc_streams from host arrays (concatenation and upload counted)', [wall(from_host)[0] for _ in range(runs)]), flush=True)
    # the mel call alone, for its rate
    window, M = fm.hann(p['n_fft']), fm.mel_filters(SR, p['n_fft'], p['n_mels'])
    d_window, d_mel = torch.from_numpy(window).to('cuda'), torch.from_numpy(M).to('cuda')
    wb = _native.mfcc_work_bytes(len(ys), len(samples), T, p['n_fft'], p['n_mels'], p['n_mfcc'])
    d_work = torch.empty(wb, dtype=torch.uint8, device='cuda')
    d_S, d_Smax = torch.empty((T, p['n_mels']), dtype=torch.float64, device='cuda'), torch.empty(len(ys), dtype=torch.float64, device='cuda')
    mel = lambda: _native.mfcc_mel_device(d_samples.data_ptr(), _native.MFCC_I16, offsets, p['n_fft'], p['hop_length'], d_window.data_ptr(),
                                          d_mel.data_ptr(), p['n_mels'], T, d_work.data_ptr(), wb, d_S.data_ptr(), d_Smax.data_ptr())
    wall(mel)
    times = [wall(mel)[0] for _ in range(runs)]
    moved = T * p['n_fft'] * 2 + T * p['n_mels'] * 8
    print(line('klnmf_mfcc_mel_device alone (three launches, three small uploads)', times), flush=True)
    print('    its algorithmic bytes: %.1f MB of samples (each read n_fft / hop = %.1f times) + %.1f MB of energies = %.1f MB: %.1f GB/s'
          % (T * p['n_fft'] * 2 / 1e6, p['n_fft'] / float(p['hop_length']), T * p['n_mels'] * 8 / 1e6, moved / 1e6,
             moved / float(np.median(times)) / 1e9), flush=True)
    # the host twin, one process
    sub = ys[:twin_utterances]
    t0 = time.perf_counter()
    want, _ = fm.host_mfcc_streams(sub, SR, **p)
    dt = time.perf_counter() - t0
    got, spans = from_device()
    t1 = spans[len(sub) - 1][1]
    err = max(float(np.abs(g[:t1].cpu().numpy() - w).max()) for g, w in zip(got, want))
    print('%-76s %9.5f s  on %d utterances = %.2f s for the corpus; largest difference from the device %.2e'
          % ('host twin host_mfcc_streams (numpy / scipy, one process)', dt, len(sub), dt * len(ys) / len(sub), err), flush=True)
    # hac_many against its two stages
    rng = np.random.default_rng(3)
    pick = rng.choice(t1, max(KS), replace=False)
    codebooks = [torch.from_numpy(w[pick[:K]].copy()).to('cuda') for w, K in zip(want, KS)]
    whole = lambda: hac.hac_many((d_samples, offsets), SR, codebooks, lags=LAGS, output='device', **p)
    rows = wall(whole)[1]
    print('    hac_many: %d x %d, nnz = %d' % (rows.shape + (rows.nnz,)), flush=True)
    print(line('hac_many from samples on the device (mfcc_streams + windowed_hac)', [wall(whole)[0] for _ in range(runs)]), flush=True)
    streams, spans = from_device()
    second = lambda: hac.windowed_hac(streams, codebooks, spans, lags=LAGS, output='device')
    wall(second)
    print(line('    its first stage, mfcc_streams', [wall(from_device)[0] for _ in range(runs)]), flush=True)
    print(line('    its second stage, windowed_hac on the device streams', [wall(second)[0] for _ in range(runs)]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--twin-utterances', type=int, default=200)
    ap.add_argument('--set', choices=sorted(SETS))
    ap.add_argument('--once', choices=sorted(SETS), help='one warm-up and one call from device samples: the run to profile')
    args = ap.parse_args()
    if args.once:
        run_set(args.once, 1, 0, True)
        return
    if args.set:
        run_set(args.set, args.runs, args.twin_utterances, False)
        return
    out = []
    for name in ('matlab', 'defaults'):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--set', name, '--runs', str(args.runs), '--twin-utterances',
                            str(args.twin_utterances)], capture_output=True, text=True, timeout=LIMIT)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            sys.exit('the %s set ended with status %d' % (name, r.returncode))
        out.append(r.stdout)
    with open(os.path.join(ROOT, 'profiles', 'mfcc_timing.txt'), 'w') as f:
        f.write('# python scripts/mfcc_timing.py --runs %d (one MI355X; host clock around a synchronise)\n' % args.runs)
        f.write('\n'.join(out))


if __name__ == '__main__':
    main()
