#!/usr/bin/env python3
"""numpy emulation of precision='bf16x3' (csrc/split3.hip.h): every fp32 operand x of the three dense contractions is split
into two bf16 parts, hi = bf16(x) and lo = bf16(x - hi), and a contraction is hi.hi + hi.lo + lo.hi with fp32 accumulation
(the lo.lo term is dropped).  With --parts 3 the three-way split (hi, mid, lo; six products) instead.

The loop is the exact fp32 mode's (csrc/api_loop.hip exact_Q / exact_W / exact_N / exact_H): V, W, H, Q in fp32, loss terms
summed in fp64, W0 = V.H0^T through the same split contraction.  It runs the fixtures' own iteration counts and reports the
deviation of every recorded loss from the reference's (the fixture's `errors`) and of the true final KL (fp64 evaluation of the
fp32 factors against the fixture's `final`).

A product of two bf16 values has at most 16 significant bits, so each partial product is exact in fp32: an fp32 sgemm of
the bf16 images is the MFMA's arithmetic up to the order of the fp32 accumulation.

    python experiments/split3_emulation.py --fixture g19 g18            # a few minutes each on 8 cores
    python experiments/split3_emulation.py --fixture g19 --parts 0      # control: plain fp32 contractions
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import klnmf_oracle as orc  # noqa: E402
from tests import golden_inputs as gi  # noqa: E402

EPS = np.float32(1e-8)


def bf16_rne(a):
    """Round float32 to the nearest bf16 (ties to even) on the fp32 bit pattern; returned as float32.  NaN stays NaN and
    infinities stay infinite (the hardware's v_cvt_pk_bf16_f32 does the same; the emulation never meets either)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    special = (u & 0x7F800000) == 0x7F800000
    r = np.where(special, (u.astype(np.uint32) & 0xFFFF0000) | np.where((u & 0x7FFFFF) != 0, 0x00400000, 0).astype(np.uint32), r)
    return r.astype(np.uint32).view(np.float32)


def split(a, parts=2):
    """[hi, lo] (parts = 2) or [hi, mid, lo] (parts = 3): bf16 values in float32 whose sum approximates a.  Every
    subtraction is exact in fp32 (Sterbenz: the part is the nearest bf16 to the remainder)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    out, rem = [], a
    for _ in range(parts):
        p = bf16_rne(rem)
        out.append(p)
        rem = (rem - p).astype(np.float32)
    return out


def split_product(A, B, parts=2):
    """A.B in fp32 from the bf16 parts: hi.hi + hi.lo + lo.hi (parts = 2) or every pair of parts whose combined order is at most
    2 (parts = 3: hh, hm, mh, hl, mm, lh).  parts = 0: the plain fp32 product (the exact fp32 mode)."""
    if parts == 0:
        return np.dot(A.astype(np.float32), B.astype(np.float32))
    a, b = split(A, parts), split(B, parts)
    acc = None
    for i in range(parts):
        for j in range(parts):
            if i + j < parts:
                t = np.dot(a[i], b[j])
                acc = t if acc is None else (acc + t).astype(np.float32)
    return acc


def run(X, H0, iters, parts):
    X32 = X.astype(np.float32)
    H = H0.astype(np.float32)
    W = split_product(X32, np.ascontiguousarray(H.T), parts)          # W0 = V.H0^T (nmf.py:156), multiply = 0
    errors = []
    for _ in range(iters):
        D = split_product(W, H, parts)
        Q = (X32 + EPS) / (D + EPS)
        errors.append(float((X32 * np.log(Q) - X32 + D).sum(dtype=np.float64)))
        W = (W * split_product(Q, np.ascontiguousarray(H.T), parts)).astype(np.float32)
        N = split_product(np.ascontiguousarray(W.T), Q, parts)
        Hn = (H * N).astype(np.float32)
        H = (Hn / (np.float32(orc.EPS_NORMALIZE) + Hn.sum(axis=1, keepdims=True, dtype=np.float64).astype(np.float32))).astype(np.float32)
    return W, H, np.array(errors)


FIXTURES = {
    'g18': ('g18_rank12_k200_150it', lambda g: gi.low_rank_problem(int(g['seed']), int(g['n']), int(g['f']), 12, int(g['k']))),
    'g19': ('g19_plateau_escape_150it', lambda g: gi.steep_problem(int(g['n']), int(g['f']), int(g['k']))),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fixture', nargs='+', default=['g19', 'g18'], choices=sorted(FIXTURES))
    ap.add_argument('--parts', type=int, default=2, choices=(0, 2, 3), help='2: hi/lo (3 products), 3: hi/mid/lo (6), 0: fp32')
    a = ap.parse_args()
    for name in a.fixture:
        fname, make = FIXTURES[name]
        g = gi.load(fname)
        X, H0 = make(g)
        iters = int(g['iters'])
        t0 = time.time()
        W, H, errors = run(X, H0, iters, a.parts)
        ref = g['errors']
        dev = np.abs(errors - ref) / ref
        final = float(g['final'])
        true_final = orc.kl_error(X, W.astype(np.float64), H.astype(np.float64))
        print('%s (%d x %d, k = %d, %d iterations), parts = %d: max |loss - ref| / ref = %.2e (iteration %d), '
              'final KL deviation %.2e   [%.0f s]'
              % (name, int(g['n']), int(g['f']), int(g['k']), iters, a.parts, dev.max(), int(dev.argmax()) + 1,
                 abs(true_final - final) / final, time.time() - t0), flush=True)
        print('  deviation at iterations 1, 10, 50, 100, 150: %s' % ', '.join('%.1e' % dev[i] for i in (0, 9, 49, 99, iters - 1)),
              flush=True)


if __name__ == '__main__':
    main()
