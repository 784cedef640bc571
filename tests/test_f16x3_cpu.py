"""precision='f16x3' without a GPU: how the Python layer routes it, the C header's code, and the numpy emulation of the fused
split-fp16 loop (experiments/f16x3_emulation.py) that the mode's accuracy claim rests on."""
import contextlib
import importlib.util
import io
import os
import re
import sys

import numpy as np
import pytest

from multimodal_amd import _native
from multimodal_amd.lib import nmf
from oracle import klnmf_oracle as orc
from tests import golden_inputs as gi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _emulation():
    sys.path.insert(0, os.path.join(ROOT, 'experiments'))
    try:
        spec = importlib.util.spec_from_file_location('f16x3_emulation', os.path.join(ROOT, 'experiments', 'f16x3_emulation.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.join(ROOT, 'experiments'))
    return mod


def _resolve_quietly(precision, n, f, k, clear=True):
    if clear:
        nmf._NOTED.clear()
    buf = io.StringIO()
    with contextlib.redirect_stderr(buf):
        out = nmf.resolve_precision(precision, n, f, k)
    return out, buf.getvalue()


# the shapes of test_host_cpu.py's 'auto' checks and the GRID of test_split3_cpu.py
GRID = [(n, f, k) for n in (500, 200000, 5000000) for f in (8, 64, 256, 4096) for k in (3, 16, 200, 600)]


def test_mode_code_in_python_and_in_the_header():
    assert _native.PRECISIONS['f16x3'] == _native.PREC_F16X3 == 5
    hdr = open(os.path.join(ROOT, 'include', 'klnmf.h')).read()
    assert re.search(r'^#define\s+KLNMF_PREC_F16X3\s+5\b', hdr, re.M)
    assert not re.search(r'^#define\s+KLNMF_PREC_\w+\s+3\b', hdr, re.M)          # 3 stays retired


@pytest.mark.parametrize('n,f,k', [s for s in GRID if s[2] <= 256])
def test_explicit_f16x3_is_honoured_up_to_k_256_without_a_note(n, f, k):
    out, err = _resolve_quietly('f16x3', n, f, k)
    assert out == 'f16x3'
    assert err == ''


def test_k_above_256_goes_to_bf16x3_with_exactly_one_note():
    out, err = _resolve_quietly('f16x3', 5000, 300, 257)
    assert out == 'bf16x3'
    assert err.count('\n') == 1 and 'f16x3' in err and 'bf16x3' in err
    out2, err2 = _resolve_quietly('f16x3', 9000, 64, 600, clear=False)
    assert out2 == 'bf16x3' and err2 == ''
    assert _resolve_quietly('f16x3', 5000, 300, 256)[0] == 'f16x3'


def test_auto_never_picks_f16x3():
    for n, f, k in GRID:
        assert _resolve_quietly('auto', n, f, k)[0] in ('f64', 'f32', 'f16')


def test_csr_input_under_f16x3_goes_to_the_fp32_sparse_kernels_with_one_note():
    nmf._NOTED.clear()
    buf = io.StringIO()
    with contextlib.redirect_stderr(buf):
        assert nmf.sparse_precision('f16x3') == 'f32'
        assert nmf.sparse_precision('f16x3') == 'f32'
    assert buf.getvalue().count('CSR input') == 1 and 'f16x3' in buf.getvalue()


def test_default_precision_from_the_environment(monkeypatch):
    monkeypatch.setenv('KLNMF_PRECISION', 'f16x3')
    assert nmf.KLdivNMF(n_components=4).precision == 'f16x3'


def test_scale_keeps_every_operand_below_2_15():
    emu = _emulation()
    rs = np.random.RandomState(3)
    x = (rs.uniform(0, 1, 100000) * np.exp(rs.uniform(-60, 60, 100000))).astype(np.float32)
    s = emu.pow2_scale(x)
    assert np.all(x * s < 2.0 ** 15) and np.all(x * s >= 2.0 ** 14)
    hi, lo = emu.split16(x * s)
    assert np.all(np.isfinite(hi)) and np.all(np.isfinite(lo))
    # hi + lo carries about 22 significant bits of a normal-range operand
    assert np.all(np.abs(hi.astype(np.float64) + lo - x.astype(np.float64) * s) <= 2.0 ** -21 * x.astype(np.float64) * s)


def test_emulated_loop_on_a_reduced_g19_is_within_2e_5_of_the_oracle():
    """G19's data (the plateau-escape class where f16 is 3.9e-4 off) on every 40th row, the fixture's 150 iterations: every
    recorded loss and the final KL of the emulated f16x3 loop within 2e-5 of the fp64 oracle's on the same rows."""
    emu = _emulation()
    g = gi.load('g19_plateau_escape_150it')
    X, H0 = gi.steep_problem(int(g['n']), int(g['f']), int(g['k']))
    X = np.ascontiguousarray(X[::40])
    iters = int(g['iters'])
    Wr, Hr, ref = orc.fit_transform(X, int(g['k']), H0=H0, max_iter=iters, tol=-np.inf, warn=False)
    W, H, errors = emu.run(X, H0, iters)
    ref = np.asarray(ref)
    assert len(errors) == len(ref) == iters
    assert np.max(np.abs(errors - ref) / ref) <= 2e-5
    final = orc.kl_error(X, Wr, Hr)
    assert abs(orc.kl_error(X, W.astype(np.float64), H.astype(np.float64)) - final) <= 2e-5 * final
