"""The MFCC front end without a GPU: the exports of include/features/klnmf_mfcc.h and their registry; the host twin
(multimodal_amd/features/mfcc.py) against closed forms and the literal numpy / scipy calls of its rules; every host refusal; and,
on the references of tests/mfcc_cases.py alone, the two CONDITIONS the GPU tests rest on -- every case's largest cepstral bar is
below 1e-8 dB, and no frame of the end-to-end cases lies closer to a label boundary than the bars can move it."""
import os
import re

import numpy as np
import pytest
import scipy.fft
import scipy.signal

from multimodal_amd import _native
from multimodal_amd.features import hac, mfcc as fm
from tests import mfcc_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'features', 'klnmf_mfcc.h')
NEW = {'klnmf_mfcc_work_bytes', 'klnmf_mfcc_mel_device', 'klnmf_mfcc_cepstra_device', 'klnmf_mfcc'}


def declared():
    return set(re.findall(r'^(?:int|const char \*)\s*(klnmf_\w+)\s*\(', open(HEADER).read(), flags=re.M))


# ---- the bindings -------------------------------------------------------------------------------------------------------------------
def test_every_declared_mfcc_symbol_is_bound_and_exported():
    assert declared() == NEW == set(_native.MFCC_SIGNATURES)
    assert [h for h, _ in _native.FEATURE_HEADER_TABLES] == ['features/klnmf_mfcc.h']
    assert dict(_native.FEATURE_HEADER_TABLES)['features/klnmf_mfcc.h'] is _native.MFCC_SIGNATURES
    for header, _ in _native.FEATURE_HEADER_TABLES:
        assert os.path.exists(os.path.join(ROOT, 'include', header))
    lib = _native.load()
    for name in NEW:
        fn = getattr(lib, name)
        assert fn.argtypes == _native.MFCC_SIGNATURES[name][1], name
    for _, table in _native.HEADER_TABLES:
        assert not (NEW & set(table))
    assert all(h.count('/') == 0 for h, _ in _native.HEADER_TABLES)            # the closed registry is untouched


def test_the_signatures_have_the_header_s_argument_counts():
    text = open(HEADER).read()
    for name in NEW:
        args = text[text.index('int %s(' % name):].split(')', 1)[0].split('(', 1)[1]
        assert len(args.split(',')) == len(_native.MFCC_SIGNATURES[name][1]), name


def test_every_entry_point_names_the_reference_lines_it_replaces():
    text = open(HEADER).read()
    for name in NEW:
        comment = text[:text.index('int %s(' % name)].rsplit('/*', 1)[1]
        assert 'features/hac.py:' in comment, name
    assert 'UNPINNED' in text


def test_the_workspace_size_is_host_arithmetic():
    base = _native.mfcc_work_bytes(4, 1000, 10, 64, 8, 1)                          # (few frames: the mel call's layout is the larger)
    assert base > 0 and _native.mfcc_work_bytes(4, 99999, 10, 64, 8, 1) == base    # no padded copy of the samples
    assert _native.mfcc_work_bytes(4, 1000, 10, 64 + 2, 8, 1) == base + 2 * 16     # the twiddles: two doubles per point
    assert _native.mfcc_work_bytes(4, 1000, 1000, 64, 8, 5) >= 1000 * 5 * 8        # the cepstra call's: the fp64 cepstra
    assert _native.mfcc_work_bytes(0, 0, 0, 64, 8, 5) > 0
    for bad in ((-1, 0, 0, 64, 8, 5), (1, -1, 1, 64, 8, 5), (1, 1, -1, 64, 8, 5), (1, 1, 1, 0, 8, 5), (1, 1, 1, 64, -1, 5),
                (1 << 31, 1, 1, 64, 8, 5), (1, 1 << 31, 1, 64, 8, 5), (1, 1, 1 << 31, 64, 8, 5), (1, 1, 1 << 24, 64, 128, 5)):
        with pytest.raises(_native.NativeError):
            _native.mfcc_work_bytes(*bad)


def test_the_route_rule_at_its_edges():
    r = _native.mfcc_route
    assert r(64) == r(2048) == r(4096) == r(256, 'fft') == 'fft'
    assert r(16) == r(320) == r(1022) == r(256, 'direct') == r(1024, 'direct') == 'direct'
    assert r(32) == 'direct' and r(32, 'fft') == 'refused'
    assert r(8192) == r(14) == r(321) == r(1026) == r(2048, 'direct') == r(320, 'fft') == 'refused'


# ---- the twin's tables --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_mfcc, n_mels', [(13, 128), (13, 30), (5, 8), (1, 1), (40, 40)])
def test_the_dct_basis_is_scipy_s_orthonormal_dct(n_mfcc, n_mels):
    want = scipy.fft.dct(np.eye(n_mels), type=2, norm='ortho', axis=0)[:n_mfcc]
    got = fm.dct_basis(n_mfcc, n_mels)
    assert got.shape == (n_mfcc, n_mels) and got.dtype == np.float64
    # entries below 1 in size, each side a few roundings from the exact value (the formula's argument i (2 m + 1) pi / (2 n)
    # carries its own 2 ulp of up to n_mfcc pi, hence the factor)
    assert np.abs(got - want).max() <= 4 * max(1.0, n_mfcc * np.pi) * 2.0 ** -53
    assert np.abs(got @ got.T - np.eye(n_mfcc)).max() < 1e-14


@pytest.mark.parametrize('n_mfcc, n_mels', [(13, 128), (13, 30), (5, 8), (1, 1)])
def test_the_row_sums_are_the_exact_sums_of_the_dct_rows(n_mfcc, n_mels):
    r = fm.dct_row_sums(n_mfcc, n_mels)
    assert r.shape == (n_mfcc,) and r[0] == np.sqrt(float(n_mels)) and not r[1:].any()
    m = np.arange(n_mels, dtype=np.longdouble)
    pi = np.longdouble('3.14159265358979323846264338327950288')
    exact = np.cos(np.arange(n_mfcc, dtype=np.longdouble)[:, None] * (2 * m + 1) * pi / (2 * n_mels)) * np.sqrt(np.longdouble(2) / n_mels)
    exact[0] = 1 / np.sqrt(np.longdouble(n_mels))
    assert np.abs(exact.sum(axis=1) - r).max() < 1e-15 * n_mels                    # the basis in extended precision sums to r
    assert np.abs(fm.dct_basis(n_mfcc, n_mels).sum(axis=1) - r).max() < 1e-13      # the rounded table: a few ulps off


@pytest.mark.parametrize('sr, n_fft, n_mels', [(22050, 2048, 128), (16000, 320, 30), (16000, 64, 8), (8000, 256, 1)])
def test_the_mel_rows_are_unit_area_triangles(sr, n_fft, n_mels):
    edges = fm.mel_band_edges(n_mels, 0.0, sr / 2.0)
    assert len(edges) == n_mels + 2 and edges[0] == 0 and abs(edges[-1] - sr / 2.0) < 1e-9 and (np.diff(edges) > 0).all()
    mels = fm.hz_to_mel(edges)
    assert np.allclose(np.diff(mels), np.diff(mels)[0], rtol=1e-10)              # equally spaced in mel
    assert np.isclose(fm.hz_to_mel(1000.0), 15.0) and np.isclose(fm.hz_to_mel(6400.0), 15.0 + 27.0) and np.isclose(fm.hz_to_mel(200.0), 3.0)
    at_knots = fm.mel_triangles(edges, edges)                                    # piecewise linear: the trapezoid rule on its knots is exact
    area = (0.5 * (at_knots[:, 1:] + at_knots[:, :-1]) * np.diff(edges)).sum(axis=1)
    assert np.abs(area - 1.0).max() < 1e-14
    M = fm.mel_filters(sr, n_fft, n_mels)
    assert M.shape == (n_mels, n_fft // 2 + 1) and (M >= 0).all()
    freqs = np.linspace(0, sr / 2.0, n_fft // 2 + 1)
    for i in (0, n_mels // 2, n_mels - 1):
        inside = (freqs > edges[i]) & (freqs < edges[i + 2])
        assert (M[i][~inside] == 0).all() and (M[i][inside] > 0).all()
        rising = M[i][(freqs > edges[i]) & (freqs <= edges[i + 1])]
        assert (np.diff(rising) > 0).all()


def test_a_tone_at_a_bin_frequency_gives_the_closed_form_hann_spectrum():
    n, k, amp = 64, 9, 1000.0
    t = np.arange(4 * n)
    y = amp * np.cos(2 * np.pi * k * t / n)
    frames = fm.host_frames(y, n, n)                                               # hop n: every frame sees the same phase
    P = np.abs(np.fft.rfft(frames[1])) ** 2
    want = np.zeros(n // 2 + 1)
    want[k], want[k - 1], want[k + 1] = (amp * n / 4) ** 2, (amp * n / 8) ** 2, (amp * n / 8) ** 2
    assert np.abs(P - want).max() < 1e-9 * want.max()
    M = fm.mel_filters(16000, n, 8)
    assert np.allclose(fm.host_mel_energies(y, n, n, M)[1], M @ want, rtol=1e-9)


def test_parseval_holds_on_a_frame():
    y = mc.audio('C')[1]
    x = fm.host_frames(y, 320, 160)[3]
    X = np.fft.rfft(x)
    full = 2 * (np.abs(X) ** 2).sum() - np.abs(X[0]) ** 2 - np.abs(X[-1]) ** 2
    assert abs(full - 320 * (x * x).sum()) <= 1e-12 * full


@pytest.mark.parametrize('order', [1, 2])
def test_host_delta_is_the_literal_pad_lfilter_slice(order):
    x = np.random.default_rng(5).normal(size=(13, 40))
    d = np.pad(x, [(0, 0), (5, 5)], mode='edge')
    for _ in range(order):
        d = scipy.signal.lfilter(np.arange(4, -5, -1), 1, d, axis=-1)
    assert np.array_equal(fm.host_delta(x, order), d[:, 5:-5])
    assert fm.host_delta(x[:, :3], order).shape == (13, 3)                         # T < 9: all edge
    # the written-out sums of the cases' longdouble reference are the same filter
    assert np.abs(mc.delta_ld(x.T, order).astype(np.float64) - fm.host_delta(x, order).T).max() < 1e-10


def test_frame_counts_and_reflection_at_the_smallest_lengths():
    assert list(fm.frame_counts([33, 34, 35, 47, 48, 64], 16)) == [3, 3, 3, 3, 4, 5]
    for L in (33, 34, 35):
        y = np.arange(100, 100 + L)
        yp = np.pad(y, 32, mode='reflect')
        p = np.arange(len(yp))
        idx = fm.reflect_index(p, L, 64)
        assert idx.min() >= 0 and idx.max() < L and np.array_equal(y[idx], yp)
        T = 1 + L // 16
        assert (T - 1) * 16 + 64 <= len(yp)                                        # the last frame ends inside the padding
        frames = fm.host_frames(y, 64, 16, window=np.ones(64))
        assert frames.shape == (T, 64) and np.array_equal(frames[T - 1], yp[(T - 1) * 16:(T - 1) * 16 + 64])
    with pytest.raises(ValueError):
        fm.host_frames(np.zeros(32), 64, 16)
    assert fm.frame_spans([3, 5, 1]) == [(0, 3), (3, 8), (8, 9)]
    assert np.array_equal(fm.hann(8), scipy.signal.get_window('hann', 8, fftbins=True))


def test_the_twin_s_streams_are_the_reference_s_orientation_and_spans():
    ys = mc.audio('A')
    streams, spans = fm.host_mfcc_streams(ys, 16000, **mc.params('A'))
    assert spans == mc.reference('A')['spans'] and spans[0] == (0, 3) and spans[-1][1] == streams[0].shape[0]
    assert all(s.shape == (spans[-1][1], 5) and s.dtype == np.float64 for s in streams)
    alone, _ = fm.host_mfcc_streams([ys[2]], 16000, **mc.params('A'))
    t0, t1 = spans[2]
    assert all(np.array_equal(a, s[t0:t1]) for a, s in zip(alone, streams))


# ---- the conditions of the GPU tests, on the reference alone ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(mc.CASES))
def test_condition_every_cepstral_bar_is_below_1e_8_db(name):
    ref = mc.reference(name)
    assert ref['bars'][0].max() < mc.CEPSTRAL_BAR_LIMIT
    assert (ref['ES'] >= 0).all() and all((b >= 0).all() and np.isfinite(b).all() for b in ref['bars'])
    # the float64 twin, an independent evaluation of the same rules, lies inside the bars
    c = mc.CASES[name]
    streams, spans = fm.host_mfcc_streams(mc.audio(name), c['sr'], **mc.params(name))
    assert spans == ref['spans']
    for got, want, bar in zip(streams, ref['streams'], ref['bars']):
        assert mc.worst_fraction(got, want, bar) <= 1.0
    if name == 'D':                                                                # both routes' bars exist at one size
        other = mc.reference('D', 'direct')
        assert other['bars'][0].max() < mc.CEPSTRAL_BAR_LIMIT and np.array_equal(other['S'], ref['S'])


def test_the_noise_floor_of_the_cases():
    for name in mc.CASES:
        for u, y in enumerate(mc.audio(name)):
            assert y.dtype == mc.CASES[name]['kind'] and np.array_equal(y, np.round(y)) and np.abs(y.astype(np.float64)).max() <= 32767
            if u in mc.CASES[name].get('zero', ()):
                assert not y.any()
    assert mc.NOISE >= 0.01
    assert [len(y) for y in mc.audio('A')] == [33, 64, 65, 200, 1000] and min(len(y) for y in mc.audio('G')) == 33
    assert max(len(y) for y in mc.audio('G')) == 40 and len(mc.audio('G')) == 1200
    t = mc.reference('F_short')['spans'][0]
    assert t[1] - t[0] == 3


@pytest.mark.parametrize('name', ['A', 'C'])
def test_condition_no_frame_is_near_a_label_boundary(name):
    case = mc.e2e(name)
    assert [cb.shape[0] for cb in case['codebooks']] == list(mc.E2E_KS) and all(np.isfinite(cb).all() for cb in case['codebooks'])
    for margin in mc.label_margins(name):
        assert len(margin) == case['streams'][0].shape[0] and margin.min() > 0     # every frame: none is left out
    assert case['want'].shape[0] == len(mc.CASES[name]['lengths']) and case['want'].nnz > 0


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_check_mfcc_inputs_refuses_what_the_header_refuses(monkeypatch):
    calls = []
    for name in ('mfcc_work_bytes', 'mfcc_mel_device', 'mfcc_cepstra_device'):
        monkeypatch.setattr(_native, name, lambda *a, **k: calls.append(a))
    y = mc.audio('A')[3]
    ok = dict(audio=[y, y], sr=16000, n_mfcc=5, n_fft=64, hop_length=16, n_mels=8)

    def refused(**change):
        with pytest.raises(ValueError):
            fm.mfcc_streams(device='cpu', **dict(ok, **change))
        with pytest.raises(ValueError):
            fm.check_mfcc_inputs(**{k: v for k, v in dict(ok, **change).items() if k != 'output'})

    refused(audio=[y, y[:32]])                                                     # an utterance below n_fft // 2 + 1
    refused(hop_length=0)
    refused(n_mfcc=9)                                                              # above n_mels
    refused(n_mfcc=0)
    refused(n_mels=0, n_mfcc=0)
    refused(n_mels=_native.MFCC_MAX_MELS + 1)
    refused(audio=[y.astype(np.int32)])                                            # a bad kind
    refused(audio=[y.reshape(2, -1)])
    refused(audio=[np.array([np.nan] * 40)])
    refused(dtype=np.float16)
    refused(n_fft=8192)
    refused(n_fft=321, audio=[np.zeros(400)])
    refused(n_fft=2048, route='direct', audio=[np.zeros(4000)])
    refused(route='radix4')
    refused(fmin=9000.0)
    refused(n_fft=64.5)
    import torch
    t = torch.zeros(100, dtype=torch.float32)
    refused(audio=(t, np.array([0, 60, 50, 100])))                                 # offsets that do not ascend
    refused(audio=(t, np.array([0, 50, 99])))
    refused(audio=(t.to(torch.int32), np.array([0, 100])))
    with pytest.raises(ValueError):
        fm.mfcc_streams(output='scipy', device='cpu', **ok)
    assert calls == []
    samples, offsets, counts, fmax = fm.check_mfcc_inputs(**ok)
    assert samples.dtype == np.int16 and list(offsets) == [0, 200, 400] and list(counts) == [13, 13] and fmax == 8000.0
    mixed = fm.check_mfcc_inputs(**dict(ok, audio=[y, y.astype(np.float32)]))[0]
    assert mixed.dtype == np.float64


def test_the_reference_s_names_exist_on_audio():
    for name in ('mfcc', 'hac', 'wav2hac', 'hac_many', 'build_codebooks_from_audio', 'build_codebooks_from_list_of_wav'):
        assert callable(getattr(hac, name))
    assert hac._mfcc_params({'n_fft': 320}) == {'n_mfcc': 13, 'n_fft': 320}
