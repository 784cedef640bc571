"""The references of tests/test_loop_pieces_gpu.py are the operations they stand for (no GPU):

  * `ref_h_rule` on the oracle's own numerator is the oracle's H rule, and its kEpsNorm is the library's;
  * `place` / `valid_mask` / `unplace` on hand-written layouts;
  * `stop_rule` on a loss record computed without the rule gives the oracle's iteration counts.
"""
import os
import re

import numpy as np
import pytest

from oracle import klnmf_oracle as orc
from tests import golden_inputs as gi
from tests import loop_piece_cases as lp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_eps_norm_is_the_librarys_and_the_oracles():
    with open(os.path.join(ROOT, 'multimodal_amd', 'csrc', 'common.hip.h')) as fh:
        m = re.search(r'constexpr\s+double\s+kEpsNorm\s*=\s*([0-9.eE+-]+)\s*;', fh.read())
    assert m is not None
    assert float(m.group(1)) == lp.K_EPS_NORM == orc.EPS_NORMALIZE


@pytest.mark.parametrize('shape', [(20, 30, 3), (37, 53, 7), (64, 129, 17)], ids=lambda s: '%dx%dk%d' % s)
def test_ref_h_rule_is_the_oracles_h_rule(shape):
    n, f, k = shape
    rs = np.random.RandomState(n + f + k)
    V = orc.synthetic_V(n, n, f, min(k, 12))
    W = rs.gamma(1.0, 1.0, (n, k))
    H = orc.synthetic_H0(f, f, k)
    W_new, H_new = orc.update_step(V, W, H, fit=True)
    Q = orc.ratio_q(V, W, H)
    got = lp.ref_h_rule(H, W_new.T.dot(Q), f)
    assert got.shape == H_new.shape
    assert np.max(np.abs(got - H_new) / H_new) <= 1e-13
    # columns beyond f of wider (padded) operands are not part of the rule
    wide = lp.ref_h_rule(np.hstack([H, np.full((k, 5), 7.0)]), np.hstack([W_new.T.dot(Q), np.full((k, 5), lp.PAD)]), f)
    assert np.array_equal(wide, got)
    # an all-zero numerator row: the divisor is kEpsNorm, the row exactly 0
    N = W_new.T.dot(Q)
    N[k // 2] = 0
    assert np.all(lp.ref_h_rule(H, N, f)[k // 2] == 0)


LAYOUTS = {
    # the exact modes: [k][f], no padding at all
    'dense': lp.whole_layout(5 * 7, 5, 7, 7),
    # the 16-bit modes' whole matrix: [KP][f_pad], rows beyond k and columns beyond f are padding
    'padded': lp.whole_layout(32 * 128, 17, 100, 128),
    # hand-written split layouts, 2 .. 4 parts: blocks of [KP = 32][ld] one behind the other, the last part's ncols < ld
    '2parts': lp.parts_layout(32 * 256 + 32 * 256, 17, 300, [(0, 17 * 256, 0, 256), (32 * 256, 17 * 256, 256, 44)]),
    '3parts': lp.parts_layout(3 * 32 * 256, 3, 513, [(0, 3 * 256, 0, 256), (32 * 256, 3 * 256, 256, 256), (2 * 32 * 256, 3 * 256, 512, 1)]),
    '4parts': lp.parts_layout(32 * (512 + 256 + 256 + 256) + 11, 20, 1030,
                              [(0, 20 * 512, 0, 512), (32 * 512, 20 * 256, 512, 256), (32 * 768, 20 * 256, 768, 256),
                               (32 * 1024, 20 * 256, 1024, 6)]),
}


@pytest.mark.parametrize('name', sorted(LAYOUTS))
def test_place_and_valid_mask_round_trip(name):
    layout = LAYOUTS[name]
    k, f = layout.k, layout.f
    N = np.arange(1, k * f + 1, dtype=np.float64).reshape(k, f)
    for dtype in (np.float32, np.float64):
        flat = lp.place(layout, N, dtype=dtype)
        assert flat.shape == (layout.count,) and flat.dtype == dtype
        mask = lp.valid_mask(layout)
        assert mask.shape == (layout.count,) and int(mask.sum()) == k * f
        assert np.all(flat[~mask] == dtype(lp.PAD))
        assert np.array_equal(np.sort(flat[mask]), N.ravel())
        assert np.array_equal(lp.unplace(layout, flat), N)
        # element by element, from the definition: part p holds column j of row c at offset + c x stride + (j - col0)
        for p in layout.parts:
            for c in (0, k - 1):
                for j in (p.col0, p.col0 + p.ncols - 1):
                    assert flat[p.offset + c * p.stride + (j - p.col0)] == N[c, j]
            if p.ncols < p.stride:                       # the row stride's padding, and the rows beyond k
                assert flat[p.offset + p.ncols] == dtype(lp.PAD)
            beyond = p.offset + k * p.stride
            if beyond < layout.count and not mask[beyond]:
                assert flat[beyond] == dtype(lp.PAD)
    if name == 'dense':
        assert mask.all()
    assert np.array_equal(lp.place(layout, N, pad=np.inf)[~mask], np.full(layout.count - k * f, np.inf, dtype=np.float32))


def test_layouts_that_cannot_be_are_refused():
    with pytest.raises(AssertionError):                  # two parts claim column 255
        lp.valid_mask(lp.parts_layout(2 * 32 * 256, 2, 300, [(0, 2 * 256, 0, 256), (32 * 256, 2 * 256, 255, 45)]))
    with pytest.raises(AssertionError):                  # column 299 has no part
        lp.valid_mask(lp.parts_layout(2 * 32 * 256, 2, 300, [(0, 2 * 256, 0, 256), (32 * 256, 2 * 256, 256, 43)]))
    with pytest.raises(AssertionError):                  # the last part leaves the buffer
        lp.valid_mask(lp.parts_layout(32 * 256 + 256, 2, 300, [(0, 2 * 256, 0, 256), (32 * 256, 2 * 256, 256, 44)]))
    with pytest.raises(AssertionError):                  # the parts share elements
        lp.valid_mask(lp.parts_layout(2 * 32 * 256, 2, 300, [(0, 2 * 256, 0, 256), (256, 2 * 256, 256, 44)]))


def test_stop_rule_gives_the_oracles_iteration_counts():
    g = gi.load('g4_tol')
    k, n, f = int(g['k']), int(g['n']), int(g['f'])
    X, H0 = gi.gen_inputs(int(g['seed']), n, f, k)
    # the loss record without the rule: a tolerance of -inf is never met
    _, _, free = orc.fit_transform(X, k=k, H0=H0, max_iter=200, tol=-np.inf, warn=False)
    assert len(free) == 200
    for sfx, cap, tol in [('', 200, 1e-6), ('2', 200, 1e-3), ('3', 4, 1e-9)]:
        _, _, errors = orc.fit_transform(X, k=k, H0=H0, max_iter=cap, tol=tol, warn=False)
        assert lp.stop_rule(free[:cap], tol * n * f) == len(errors) == len(g['errors' + sfx])
        assert np.array_equal(free[:len(errors)], errors)
    assert 0 < len(g['errors2']) < len(g['errors']) < 200            # the rule fired, at two different places
    # by hand: never with a tolerance nothing meets, at once on an increase, not at prev - err == tol_abs
    assert lp.stop_rule([3.0, 2.0, 1.0], lp.NO_STOP) == 3
    assert lp.stop_rule([3.0, 4.0, 1.0], 0.0) == 1
    assert lp.stop_rule([3.0, 2.0, 1.0], 1.0) == 3
    assert lp.stop_rule([3.0, 2.0, 1.0], np.nextafter(1.0, 2.0)) == 1
    assert lp.stop_rule([np.inf, 2.0], 1.0) == 2
    assert lp.stop_rule([], 1.0) == 0


def test_the_scripts_are_what_they_say():
    for name, script in lp.SCRIPTS.items():
        assert len(script) == lp.STOP_CAP and lp.stop_rule(script, lp.STOP_TOL) == lp.SCRIPT_DONE[name], name
    s = lp.SCRIPTS['step-equals-tol']
    assert s[1] - s[2] == lp.STOP_TOL
    s = lp.SCRIPTS['step-just-below-tol']
    assert s[2] - s[3] == lp.BELOW_ONE < lp.STOP_TOL
