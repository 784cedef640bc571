#!/usr/bin/env python3
"""numpy emulation of precision='f16x3' (csrc/f16x3.hip.h): the fp32 mode's loop with every operand of its three dense
contractions split into two fp16 parts, hi = f16(x s) and lo = f16(x s - hi), s a power of two, and a contraction
hi.hi + hi.lo + lo.hi with fp32 accumulation (lo.lo dropped).  np.float16 rounds to nearest even and keeps subnormals, as
v_cvt_f16_f32 does: a lo below 2^-14 loses bits, below 2^-25 it flushes to zero.

The scales are the kernels' (every one an exact power of two, chosen so that the largest scaled operand is below 2^15):
  W.H    per component row j of H over all columns: hs[j]; the W operand is W[r, j] / hs[j], scaled per row r of W
  Q.H^T  Q per row per 64-column tile (the tile the row pass holds); H as in W.H (hs)
  W^T.Q  Q per row over all columns (qr[r], the row pass's running maximum); the W operand is W[r, j] qr[r], scaled per
         component j over all rows
Storage (the question of section 0): --store v32q32 (default: V and Q in fp32, the f32 mode's upload), v16 (V rounded to
fp16 under the f16 mode's power-of-two scale), q16 (Q stored as one fp16 value).

    python experiments/f16x3_emulation.py --fixture g19 g18 g11 g17       # minutes each on 8 cores
    python experiments/f16x3_emulation.py --fixture g19 --store v16
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'experiments'))

from oracle import klnmf_oracle as orc  # noqa: E402
from tests import golden_inputs as gi  # noqa: E402
import split3_emulation as s3  # noqa: E402  (fixture table; the deviation report below is its format)

EPS = np.float32(1e-8)
TOP = 15          # largest scaled operand below 2^TOP (fp16's largest finite value is 65504 < 2^16)
TILE = 64         # columns of f per row-pass tile


def pow2_scale(amax):
    """2^(TOP - e) with 2^(e-1) <= amax < 2^e (1 for amax = 0): amax * scale < 2^TOP, exact in fp32; the exponent clamped to
    [-126, 126] as f3_scale clamps it (the scale and its inverse stay normal fp32 numbers)."""
    amax = np.asarray(amax, dtype=np.float64)
    e = np.where(amax > 0, np.floor(np.log2(np.where(amax > 0, amax, 1.0))) + 1, TOP)
    return np.ldexp(1.0, np.clip(TOP - e, -126, 126).astype(np.int32)).astype(np.float32)


def split16(x):
    """[hi, lo] fp16 images of an already scaled fp32 array, returned as float32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = x.astype(np.float16).astype(np.float32)
    lo = (x - hi).astype(np.float32).astype(np.float16).astype(np.float32)
    return hi, lo


def prod3(A, B):
    """hi.hi + hi.lo + lo.hi of two scaled fp32 arrays (each partial product exact in fp32: 11 x 11 significant bits)."""
    ah, al = split16(A)
    bh, bl = split16(B)
    return (np.dot(ah, bh) + (np.dot(ah, bl) + np.dot(al, bh))).astype(np.float32)


def wh(W, H, hs):
    """W.H with hs folded into the W operand, W scaled per row."""
    Wp = (W / hs[None, :]).astype(np.float32)
    ws = pow2_scale(np.abs(Wp).max(axis=1))
    return (prod3(Wp * ws[:, None], H * hs[:, None]) / ws[:, None]).astype(np.float32)


def qht(Q, H, hs):
    """Q.H^T with Q scaled per row per TILE-column tile; the tiles' products summed in fp32 in column order."""
    n, f = Q.shape
    acc = np.zeros((n, H.shape[0]), np.float32)
    HsT = np.ascontiguousarray((H * hs[:, None]).T)
    for c0 in range(0, f, TILE):
        q = Q[:, c0:c0 + TILE]
        qs = pow2_scale(np.abs(q).max(axis=1))
        acc = (acc + prod3(q * qs[:, None], HsT[c0:c0 + TILE]) / qs[:, None]).astype(np.float32)
    return (acc / hs[None, :]).astype(np.float32)


def wtq(W, Q):
    """W^T.Q: Q scaled by 1/qr[r] (qr = 2^e >= the row's maximum) and 2^14, the W operand W[r, j] qr[r] scaled per j."""
    qmax = np.abs(Q).max(axis=1).astype(np.float64)
    qr = np.where(qmax > 0, np.ldexp(1.0, (np.floor(np.log2(np.where(qmax > 0, qmax, 1.0))) + 1).astype(np.int32)), 1.0)
    qr = qr.astype(np.float32)
    Wp = (W * qr[:, None]).astype(np.float32)
    wj = pow2_scale(np.abs(Wp).max(axis=0))
    qsc = np.float32(2.0 ** (TOP - 1))
    # (the inverse scales one after the other, as k_colpass_x3 applies them: wj qsc is beyond fp32's range for wj >= 2^114)
    return (prod3(np.ascontiguousarray((Wp * wj[None, :]).T), Q / qr[:, None] * qsc) / qsc / wj[:, None]).astype(np.float32)


def run(X, H0, iters, store='v32q32'):
    X32 = X.astype(np.float32)
    if store == 'v16':            # the f16 mode's V image: scaled so that max(V) s < 2^15, rounded to fp16
        vs = pow2_scale(X32.max())
        X32 = ((X32 * vs).astype(np.float16).astype(np.float32) / vs).astype(np.float32)
    H = H0.astype(np.float32)
    W = s3.split_product(X32, np.ascontiguousarray(H.T), 2)          # W0 = V.H0^T: the single-step kernel (bf16x3's)
    errors = []
    for _ in range(iters):
        hs = pow2_scale(H.max(axis=1))
        D = wh(W, H, hs)
        Q = (X32 + EPS) / (D + EPS)
        errors.append(float((X32 * np.log(Q) - X32 + D).sum(dtype=np.float64)))
        if store == 'q16':
            Q = Q.astype(np.float16).astype(np.float32)
        W = (W * qht(Q, H, hs)).astype(np.float32)
        N = wtq(W, Q)
        Hn = (H * N).astype(np.float32)
        H = (Hn / (np.float32(orc.EPS_NORMALIZE) + Hn.sum(axis=1, keepdims=True, dtype=np.float64).astype(np.float32))).astype(np.float32)
    return W, H, np.array(errors)


FIXTURES = dict(s3.FIXTURES)
FIXTURES['g11'] = ('g11_c4shape_50it', lambda g: gi.synthetic_problem(int(g['seed']), int(g['n']), int(g['f']), int(g['k'])))
FIXTURES['g17'] = ('g17_c2kind_40000rows_200it', lambda g: gi.synthetic_problem(int(g['seed']), int(g['n']), int(g['f']), int(g['k'])))


def deviations(name, store='v32q32'):
    """(per-iteration deviation of the recorded losses, final-KL deviation, fixture) of one fixture at its own iterations."""
    fname, make = FIXTURES[name]
    g = gi.load(fname)
    X, H0 = make(g)
    iters = int(g['iters'])
    W, H, errors = run(X, H0, iters, store)
    ref = g['errors']
    dev = np.abs(errors - ref) / ref
    final = float(g['final'])
    true_final = orc.kl_error(X, W.astype(np.float64), H.astype(np.float64))
    return dev, abs(true_final - final) / final, g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fixture', nargs='+', default=['g19', 'g18', 'g11', 'g17'], choices=sorted(FIXTURES))
    ap.add_argument('--store', default='v32q32', choices=('v32q32', 'v16', 'q16'))
    a = ap.parse_args()
    for name in a.fixture:
        t0 = time.time()
        dev, fdev, g = deviations(name, a.store)
        iters = int(g['iters'])
        print('%s (%d x %d, k = %d, %d iterations), store = %s: max |loss - ref| / ref = %.2e (iteration %d), '
              'final KL deviation %.2e   [%.0f s]'
              % (name, int(g['n']), int(g['f']), int(g['k']), iters, a.store, dev.max(), int(dev.argmax()) + 1, fdev,
                 time.time() - t0), flush=True)
        print('  deviation at iterations 1, 10, 50, 100, %d: %s' % (iters, ', '.join(
            '%.1e' % dev[i] for i in (0, 9, min(49, iters - 1), min(99, iters - 1), iters - 1))), flush=True)


if __name__ == '__main__':
    main()
