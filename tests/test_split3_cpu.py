"""precision='bf16x3' without a GPU: how the Python layer routes it, the C header's code, and the numpy emulation of the
split product (experiments/split3_emulation.py) that the mode's accuracy claim rests on."""
import contextlib
import importlib.util
import io
import os
import re

import numpy as np
import pytest

from multimodal_amd import _native
from multimodal_amd.lib import nmf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _emulation():
    spec = importlib.util.spec_from_file_location('split3_emulation', os.path.join(ROOT, 'experiments', 'split3_emulation.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GRID = [(n, f, k) for n in (500, 200000, 5000000) for f in (8, 64, 256, 4096) for k in (3, 16, 200, 600)]

# precision='auto' on GRID as main resolves it: (n, f, k) -> mode.  'auto' is not changed by the new mode.
AUTO_TABLE = {
    (500, 8, 3): 'f64', (500, 8, 16): 'f64', (500, 8, 200): 'f64', (500, 8, 600): 'f64',
    (500, 64, 3): 'f64', (500, 64, 16): 'f64', (500, 64, 200): 'f64', (500, 64, 600): 'f64',
    (500, 256, 3): 'f64', (500, 256, 16): 'f64', (500, 256, 200): 'f64', (500, 256, 600): 'f64',
    (500, 4096, 3): 'f64', (500, 4096, 16): 'f64', (500, 4096, 200): 'f64', (500, 4096, 600): 'f64',
    (200000, 8, 3): 'f64', (200000, 8, 16): 'f64', (200000, 8, 200): 'f64', (200000, 8, 600): 'f64',
    (200000, 64, 3): 'f64', (200000, 64, 16): 'f64', (200000, 64, 200): 'f32', (200000, 64, 600): 'f32',
    (200000, 256, 3): 'f64', (200000, 256, 16): 'f64', (200000, 256, 200): 'f16', (200000, 256, 600): 'f32',
    (200000, 4096, 3): 'f32', (200000, 4096, 16): 'f16', (200000, 4096, 200): 'f16', (200000, 4096, 600): 'f32',
    (5000000, 8, 3): 'f64', (5000000, 8, 16): 'f64', (5000000, 8, 200): 'f16', (5000000, 8, 600): 'f32',
    (5000000, 64, 3): 'f64', (5000000, 64, 16): 'f16', (5000000, 64, 200): 'f16', (5000000, 64, 600): 'f32',
    (5000000, 256, 3): 'f16', (5000000, 256, 16): 'f16', (5000000, 256, 200): 'f16', (5000000, 256, 600): 'f32',
    (5000000, 4096, 3): 'f16', (5000000, 4096, 16): 'f16', (5000000, 4096, 200): 'f16', (5000000, 4096, 600): 'f32',
}


def _resolve_quietly(precision, n, f, k):
    nmf._NOTED.clear()
    buf = io.StringIO()
    with contextlib.redirect_stderr(buf):
        out = nmf.resolve_precision(precision, n, f, k)
    return out, buf.getvalue()


@pytest.mark.parametrize('n,f,k', GRID)
def test_explicit_bf16x3_is_honoured_on_every_shape_without_a_note(n, f, k):
    """f < 256, k < 16 and k > 512 included: the mode runs the exact modes' kernels (no k bound, no accuracy envelope)."""
    out, err = _resolve_quietly('bf16x3', n, f, k)
    assert out == 'bf16x3'
    assert err == ''


def test_auto_resolves_as_before():
    got = {}
    for n, f, k in GRID:
        got[(n, f, k)] = _resolve_quietly('auto', n, f, k)[0]
    assert got == AUTO_TABLE


def test_csr_input_under_bf16x3_goes_to_the_fp32_sparse_kernels_with_one_note():
    nmf._NOTED.clear()
    buf = io.StringIO()
    with contextlib.redirect_stderr(buf):
        assert nmf.sparse_precision('bf16x3') == 'f32'
        assert nmf.sparse_precision('bf16x3') == 'f32'
    assert buf.getvalue().count('CSR input') == 1 and 'bf16x3' in buf.getvalue()


def test_mode_code_in_python_and_in_the_header():
    assert _native.PRECISIONS['bf16x3'] == _native.PREC_BF16X3 == 4
    hdr = open(os.path.join(ROOT, 'include', 'klnmf.h')).read()
    assert re.search(r'^#define\s+KLNMF_PREC_BF16X3\s+4\b', hdr, re.M)
    assert not re.search(r'^#define\s+KLNMF_PREC_\w+\s+3\b', hdr, re.M)          # 3 stays retired


def test_default_precision_from_the_environment(monkeypatch):
    monkeypatch.setenv('KLNMF_PRECISION', 'bf16x3')
    assert nmf.KLdivNMF(n_components=4).precision == 'bf16x3'


def _check_products(a, b, emu):
    a = a.astype(np.float32)
    b = b.astype(np.float32)
    ah, al = emu.split(a)
    bh, bl = emu.split(b)
    # each partial product of two bf16 values is exact in fp32; the kernel sums three of them
    got = ah.astype(np.float64) * bh + ah.astype(np.float64) * bl + al.astype(np.float64) * bh
    exact = a.astype(np.float64) * b.astype(np.float64)
    assert np.all(np.abs(got - exact) <= 2.0 ** -14 * np.abs(exact))
    assert np.all(np.isfinite(ah)) and np.all(np.isfinite(al)) and np.all(np.isfinite(bh)) and np.all(np.isfinite(bl))


def test_split_product_bound_on_random_inputs():
    emu = _emulation()
    rs = np.random.RandomState(5)
    a = rs.standard_normal(200000) * np.exp(rs.uniform(-40, 40, 200000))
    b = rs.standard_normal(200000) * np.exp(rs.uniform(-40, 40, 200000))
    _check_products(a, b, emu)


def test_split_product_bound_on_adversarial_inputs():
    """bf16 ties (the 9th significant bit set and nothing below, or the bit below the lo part's last), all-ones
    significands, powers of two, the extremes of the normal range where the products stay finite."""
    emu = _emulation()
    m = np.arange(1 << 8, dtype=np.uint32)
    bits = [(127 << 23) | (m << 15) | (1 << 14),                     # ties of hi
            (127 << 23) | (m << 15) | 0x7FFF,                       # all ones below hi
            (127 << 23) | (m << 15) | (1 << 6),                     # ties of lo
            (127 << 23) | (m << 15) | 0x4040,
            (127 << 23) | (m << 15)]                                # exactly representable: lo = 0
    v = np.concatenate([np.asarray(x, dtype=np.uint32).view(np.float32) for x in bits])
    vals = np.concatenate([v, -v, v * np.float32(2.0 ** 60), v * np.float32(2.0 ** -60)])
    a, b = np.meshgrid(vals[::7], vals[::5])
    _check_products(a.ravel(), b.ravel(), emu)


def test_split_contraction_bound():
    """hi.hi + hi.lo + lo.hi accumulated in fp32 (emulated as sgemms of the bf16 images) against fp64, per element within
    2^-14 sum |a.b| -- the bound the GPU tests hold the kernel to; with nonnegative operands a relative bound."""
    emu = _emulation()
    rs = np.random.RandomState(9)
    A = rs.uniform(0, 1, (37, 301)).astype(np.float32) * np.float32(10.0) ** rs.randint(-10, 10, (37, 301)).astype(np.float32)
    B = rs.uniform(0, 1, (301, 23)).astype(np.float32) * np.float32(10.0) ** rs.randint(-10, 10, (301, 23)).astype(np.float32)
    got = emu.split_product(A, B)
    exact = A.astype(np.float64) @ B.astype(np.float64)
    assert np.all(np.abs(got - exact) <= 2.0 ** -14 * (np.abs(A.astype(np.float64)) @ np.abs(B.astype(np.float64))))
