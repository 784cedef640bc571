"""CPU side of the dense exact-mode tests (tests/test_exact_gpu.py): the regime query's constants, the host rule's
restatement and the routes the case list reaches, and the chunked fp64 reference.  No GPU needed."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from numpy.testing import assert_allclose

from multimodal_amd import _native
from oracle import klnmf_oracle as orc
from tests import exact_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CU = ec.MI355X_CUS


def test_exact_regime_query_constants_match_the_header():
    with open(os.path.join(ROOT, 'include', 'klnmf.h')) as fh:
        header = fh.read()
    defined = dict((m.group(1), int(m.group(2))) for m in re.finditer(r'#define KLNMF_(Q_EX_\w+)\s+(\d+)', header))
    assert defined == {'Q_EX_ROW_CHUNKS': _native.Q_EX_ROW_CHUNKS, 'Q_EX_W_CHUNKS': _native.Q_EX_W_CHUNKS,
                       'Q_EX_H_SEGMENTS': _native.Q_EX_H_SEGMENTS, 'Q_EX_H_FROM_SLABS': _native.Q_EX_H_FROM_SLABS}
    # and they extend the item list without reusing a number
    others = [int(m.group(1)) for m in re.finditer(r'#define KLNMF_Q_(?!EX_)\w+\s+(\d+)', header)]
    assert not set(defined.values()) & set(others)
    assert len(set(defined.values())) == 4


def test_the_restated_rule_matches_the_issue_table_at_256_cus():
    """The regime of each case at 256 CUs, computed by hand from klnmf_set_problem's rule."""
    want = {
        (1, 1, 1): (1, 16, 1, 16, 1, True),
        (15, 17, 1): (1, 16, 1, 32, 1, True),
        (64, 64, 64): (1, 64, 1, 64, 1, True),
        (65, 65, 65): (2, 48, 2, 48, 1, True),
        (300, 700, 1000): (5, 64, 7, 112, 1, True),
        (200, 8192, 512): (1, 208, 16, 512, 1, True),
        (16384, 300, 64): (205, 80, 1, 304, 1, False),
        (4111, 63, 200): (65, 64, 1, 64, 1, True),
        (2048, 520, 513): (13, 160, 1, 528, 1, True),
        (4096, 128, 16): (64, 64, 2, 64, 1, True),
        (4096, 129, 16): (64, 64, 3, 48, 1, False),
        (100, 16384, 17): (2, 64, 256, 64, 4, False),
        (100, 16385, 33): (2, 64, 205, 80, 5, False),
        (77, 20000, 130): (2, 48, 84, 240, 5, False),
        (70001, 64, 8): (876, 80, 1, 64, 1, False),
        (4194240, 3, 2): (1024, 4096, 1, 16, 1, True),
        ec.MID: (16, 64, 5, 64, 1, True),
    }
    for k in (16, 17, 63, 64, 65, 128, 129, 200, 512, 513):
        want[(300, 700, k)] = (5, 64, 11, 64, 1, True)
    cases = set(c[:3] for c in ec.CASES)
    assert cases | {ec.MID} == set(want)
    for shape, regime in want.items():
        for esize in (8, 4):
            assert ec.exact_regime(*shape, cu_count=CU, esize=esize) == regime, shape


def test_the_cases_reach_every_route_and_edge_at_256_cus():
    R = dict((c[:3], ec.exact_regime(*c[:3], cu_count=CU)) for c in ec.CASES)
    reached = set()
    for (n, f, k), (s, kch, w, wch, h, slabs) in R.items():
        if n <= ec.GT and f <= ec.GT and k <= ec.GT:
            reached.add('one tile' if (n, f, k) == (64, 64, 64) else 'one partial tile')
        if min(n, f, k) > ec.GT and max(n, f, k) <= 2 * ec.GT and n % ec.GT == f % ec.GT == k % ec.GT == 1:
            reached.add('one past a tile on every axis')
        if k < ec.GK or f < ec.GK:
            reached.add('contraction shorter than 16')
        if k % ec.GK:
            reached.add('component count inside a 16-wide MFMA block')
        if k > ec.GT:
            reached.add('more than one 64-component block')
        if k > 512:
            reached.add('k > 512')
        if s == 1 and n > ec.GT:
            reached.add('one row chunk, n > 64')
        if s > 1 and n % kch:
            reached.add('ragged last row chunk')
        if s > 512:
            reached.add('many row chunks')
        if w == 1 and n > ec.GT:
            reached.add('one-piece W rule, n > 64')
        if w > 1 and f % wch:
            reached.add('ragged last W chunk')
        if w > 1 and f % wch == 0:
            reached.add('whole W chunks')
        if h > 1 and f % ec.HSEG == 0:
            reached.add('whole H segments')
        if h > 1 and f % ec.HSEG == 1:
            reached.add('last H segment of one column')
        if h > 1 and f % ec.HSEG > 1:
            reached.add('ragged last H segment')
        if slabs and s > 1:
            reached.add('H rule from the slabs')
        if not slabs and h == 1:
            reached.add('H rule from the summed slabs')
        if n == ec.ROWS_MAX:
            reached.add('the largest n')
    # both sides of nsplit * f <= 8192 on one data class (the same n and k)
    assert R[(4096, 128, 16)][0] * 128 == ec.SLABS_MAX and R[(4096, 128, 16)][5]
    assert R[(4096, 129, 16)][0] * 129 > ec.SLABS_MAX and not R[(4096, 129, 16)][5]
    assert reached == {
        'one partial tile', 'one tile', 'one past a tile on every axis', 'contraction shorter than 16',
        'component count inside a 16-wide MFMA block', 'more than one 64-component block', 'k > 512',
        'one row chunk, n > 64', 'ragged last row chunk', 'many row chunks', 'one-piece W rule, n > 64',
        'ragged last W chunk', 'whole W chunks', 'whole H segments', 'last H segment of one column', 'ragged last H segment',
        'H rule from the slabs', 'H rule from the summed slabs', 'the largest n'}
    # the component axis around every MFMA block and 64-tile edge, and beyond 512
    ks = set(c[2] for c in ec.CASES if c[:2] == (300, 700))
    assert {16, 17, 63, 64, 65, 128, 129, 512, 513} <= ks and max(ks) > 512


def test_the_forced_routes_differ_from_the_natural_one():
    n, f, k = ec.MID
    natural = ec.exact_regime(n, f, k, CU)
    assert natural == (16, 64, 5, 64, 1, True)
    rows = [ec.exact_regime(n, f, k, CU, row_chunks=r)[0] for r in ec.FORCED_ROW_CHUNKS]
    assert rows == list(ec.FORCED_ROW_CHUNKS)
    for w in ec.FORCED_W_CHUNKS:
        _, _, ws, wch, _, _ = ec.exact_regime(n, f, k, CU, w_chunks=w)
        assert ws == w
        if w == 3:
            assert (wch, f - 2 * wch) == (112, 76)          # a ragged last chunk
    for L in ec.FORCED_H_SEG:
        _, _, _, _, h, slabs = ec.exact_regime(n, f, k, CU, h_seg=L)
        assert h == 3 and not slabs
        assert f - 2 * L == (100 if L == 100 else 44)
    # the chunk is rounded up to GK: the effective count may fall below the forced one
    assert ec.exact_regime(40, 300, 8, CU, row_chunks=7)[:2] == (3, 16)
    assert ec.exact_regime(40, 100, 8, CU, w_chunks=9)[2:4] == (7, 16)


def test_the_wpart_cap_cannot_bind_at_256_cus():
    """klnmf_set_problem gives up W chunks while wsplit * n * k elements exceed 256 MiB.  The rule splits only with fewer
    output tiles wt = ceil(n/64) ceil(k/64) than CUs, into at most ceil(2 cu / wt) chunks, and n k <= 4096 wt: so
    wsplit n k < (2 cu + wt) 4096 < 3 cu 4096 elements, 24 MiB in fp64 at 256 CUs.  No GPU case is built for the cap."""
    bound = 3 * CU * 4096 * 8
    assert bound < ec.WPART_CAP
    rng = np.random.default_rng(0)
    shapes = [(n, f, k) for n in (1, 63, 64, 65, 700, 4096, 16383) for f in (1, 64, 4097, 1 << 20)
              for k in (1, 64, 65, 1000, 4096)]
    shapes += [tuple(int(v) for v in rng.integers(1, 1 << 14, 3)) for _ in range(2000)]
    for n, f, k in shapes:
        capped = ec.exact_regime(n, f, k, CU, esize=8)
        w = capped[2]
        assert w == 1 or w * n * k * 8 < bound
        # with the cap lifted the rule gives the same answer
        saved = ec.WPART_CAP
        try:
            ec.WPART_CAP = 1 << 62
            lifted = ec.exact_regime(n, f, k, CU, esize=8)
        finally:
            ec.WPART_CAP = saved
        assert lifted == capped, (n, f, k)


Q_REGIME = (_native.Q_EX_ROW_CHUNKS, _native.Q_EX_W_CHUNKS, _native.Q_EX_H_SEGMENTS, _native.Q_EX_H_FROM_SLABS)
SWITCHES = ('KLNMF_EX_ROW_CHUNKS', 'KLNMF_EX_W_CHUNKS', 'KLNMF_EX_H_SEG')

_PLAN_CHILD = '''
import json, sys
from multimodal_amd import _native as nat
prec, n, f, k = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
items = (nat.Q_EX_ROW_CHUNKS, nat.Q_EX_W_CHUNKS, nat.Q_EX_H_SEGMENTS, nat.Q_EX_H_FROM_SLABS)
print(json.dumps([nat.plan_query(prec, n, f, k, q, cu_count=256) for q in items]))
'''


def plan_regime(prec, n, f, k):
    return tuple(_native.plan_query(prec, n, f, k, q, cu_count=CU) for q in Q_REGIME)


def test_the_library_plan_equals_the_restated_rule_at_256_cus(monkeypatch):
    """klnmf_plan_query -- klnmf_set_problem's own rule (csrc/plan.hip.h), reached without a device -- against
    exact_cases.query_regime: every case in both element sizes, every forced route (the switches through the environment of a
    child process with KLNMF_DEV=1), a seeded sweep of random shapes, and the two shape refusals.  Equality throughout."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for case in ec.CASES + [ec.MID]:
        n, f, k = case[:3]
        for prec, esize in (('f64', 8), ('f32', 4)):
            assert plan_regime(prec, n, f, k) == ec.query_regime(n, f, k, CU, esize=esize), (prec, n, f, k)
    # the other fp32-storage modes share f32's rule
    for prec in ('bf16x3', 'f16x3'):
        assert plan_regime(prec, *ec.MID) == ec.query_regime(*ec.MID, cu_count=CU, esize=4)
    # forced routes
    n, f, k = ec.MID
    forced = ([('row_chunks', r) for r in ec.FORCED_ROW_CHUNKS] + [('w_chunks', w) for w in ec.FORCED_W_CHUNKS]
              + [('h_seg', L) for L in ec.FORCED_H_SEG])
    names = dict(zip(('row_chunks', 'w_chunks', 'h_seg'), SWITCHES))
    for what, value in forced:
        env = dict(os.environ)
        for name in SWITCHES:
            env.pop(name, None)
        env['KLNMF_DEV'] = '1'
        env[names[what]] = str(value)
        for prec, esize in (('f64', 8), ('f32', 4)):
            out = subprocess.run([sys.executable, '-c', _PLAN_CHILD, prec, str(n), str(f), str(k)], cwd=ROOT, env=env,
                                 stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180)
            assert out.returncode == 0, out.stderr.decode(errors='replace')[-2000:]
            got = tuple(json.loads(out.stdout.decode().strip().splitlines()[-1]))
            want = ec.query_regime(n, f, k, CU, esize=esize, **{what: value})
            assert got == want, (what, value, prec)
            assert got != ec.query_regime(n, f, k, CU, esize=esize)          # the switch was honoured
    # a seeded sweep: n <= 65535 * 64, f <= 40 000, k <= 1100 (log-uniform n, so that small and large row counts both occur)
    rng = np.random.default_rng(20240)
    count = 0
    for _ in range(2500):
        n = int(min(ec.ROWS_MAX, np.exp(rng.uniform(0, np.log(ec.ROWS_MAX)))))
        f = int(rng.integers(1, 40001))
        k = int(rng.integers(1, 1101))
        for prec, esize in (('f64', 8), ('f32', 4)):
            assert plan_regime(prec, n, f, k) == ec.query_regime(n, f, k, CU, esize=esize), (prec, n, f, k)
        count += 1
    assert count >= 2000
    # the refusals of the shape: the exact modes' row limit, the 16-bit mode's component limit
    for prec in ('f64', 'f32', 'bf16x3', 'f16x3'):
        assert plan_regime(prec, *ec.LARGEST_N)[0] >= 1
        with pytest.raises(_native.NativeError) as err:
            plan_regime(prec, ec.ROWS_MAX + 1, 3, 2)
        assert err.value.code == _native.ERR_UNSUPP and '65535 x 64 rows' in str(err.value)
    assert _native.plan_query('f16', 300, 700, 512, _native.Q_RATIO_TILE_BYTES, cu_count=CU) == 2
    with pytest.raises(_native.NativeError) as err:
        _native.plan_query('f16', 300, 700, 513, _native.Q_RATIO_TILE_BYTES, cu_count=CU)
    assert err.value.code == _native.ERR_UNSUPP and 'k > 512' in str(err.value)
    # a 16-bit-mode problem has no exact regime
    assert plan_regime('f16', *ec.MID) == (0, 0, 0, 0)


def test_chunked_reference_equals_the_oracle():
    n, f, k = 141, 150, 7
    V = ec.data(n, f, seed=5, zero_row=3, zero_col=7)
    W, H = ec.factors(n, f, k, seed=6)
    for kchunk, wchunk in ((None, None), (16, 16), (48, 64), (80, 144)):
        loss, Q, Wn, Hn = ec.ref_step(V, W, H, kchunk, wchunk)
        assert_allclose(loss, orc.kl_error(V, W, H), rtol=1e-13)
        assert_allclose(Q, orc.ratio_q(V, W, H), rtol=1e-13, atol=0)
        Wo, Ho = orc.update_step(V, W, H)
        assert_allclose(Wn, Wo, rtol=1e-13, atol=0)
        assert_allclose(Hn, Ho, rtol=1e-13, atol=0)
        assert_allclose(ec.ref_init_W(V, H, wchunk), orc.init_factors(V, k, H0=H)[0], rtol=1e-13, atol=0)
        for fit in (True, False):
            Wo, Ho, eo = orc.fit_transform(V, k, H0=H, max_iter=6, tol=ec.NO_STOP, fit=fit, components=H)
            Wc, Hc, ec_ = ec.ref_fit(V, H, 6, fit=fit, components=H, kchunk=kchunk, wchunk=wchunk)
            assert len(eo) == len(ec_) == 6
            assert_allclose(ec_, eo, rtol=1e-13)
            assert_allclose(Wc, Wo, rtol=1e-13, atol=0)
            assert_allclose(Hc, Ho, rtol=1e-13, atol=0)
    # the zero row of V keeps a zero row of W0 and of every later W
    Wc, _, _ = ec.ref_fit(V, H, 3)
    assert np.all(Wc[3] == 0) and np.all(ec.ref_init_W(V, H)[3] == 0)
