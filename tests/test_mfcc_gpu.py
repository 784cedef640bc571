"""The MFCC front end on the device (include/features/klnmf_mfcc.h, csrc/mfcc.hip.h).

Against the extended-precision reference of tests/mfcc_cases.py with its DERIVED elementwise bars (mel energies; cepstra and
deltas, float64 and float32); bit for bit where the rules promise it (an utterance alone against the batch, two runs, the
host-array entry against the device entry points); both routes against each other at one size; and end to end, exactly, into the
windowed histograms and the codebook builders.  Each test prints its worst error as a fraction of its bar before it asserts.
tests/test_mfcc_cpu.py asserts the conditions these tests rest on (bars below 1e-8 dB, label margins) on the reference alone."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from multimodal_amd import _native
from multimodal_amd.features import codebook, hac, mfcc as fm
from tests import hac_cases as hc
from tests import mfcc_cases as mc

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5


def on_device(a):
    import torch
    return torch.from_numpy(np.array(a, order='C')).to('cuda')


def offsets_of(ys):
    return np.concatenate([[0], np.cumsum([len(y) for y in ys])]).astype(np.int64)


def device_energies(name, route='auto', ys=None):
    """(S [T, n_mels], Smax [U]) of klnmf_mfcc_mel_device on a case's audio."""
    import torch
    c = mc.CASES[name]
    ys = mc.audio(name) if ys is None else ys
    window, M, _ = mc.tables(name)
    off = offsets_of(ys)
    T = int(fm.frame_counts(np.diff(off), c['hop']).sum())
    d_samples, d_window, d_mel = on_device(np.concatenate(ys)), on_device(window), on_device(M)
    work_bytes = _native.mfcc_work_bytes(len(ys), int(off[-1]), T, c['n_fft'], c['n_mels'], c['n_mfcc'])
    d_work = torch.empty(work_bytes, dtype=torch.uint8, device='cuda')
    d_S = torch.full((T, c['n_mels']), SENTINEL, dtype=torch.float64, device='cuda')
    d_Smax = torch.full((len(ys),), SENTINEL, dtype=torch.float64, device='cuda')
    _native.mfcc_mel_device(d_samples.data_ptr(), _native.MFCC_SAMPLE_KINDS[np.dtype(c['kind'])], off, c['n_fft'], c['hop'],
                            d_window.data_ptr(), d_mel.data_ptr(), c['n_mels'], T, d_work.data_ptr(), work_bytes, d_S.data_ptr(),
                            d_Smax.data_ptr(), route=route)
    return d_S.cpu().numpy(), d_Smax.cpu().numpy()


def device_streams(name, dtype=np.float64, route='auto', ys=None):
    c = mc.CASES[name]
    return fm.mfcc_streams(mc.audio(name) if ys is None else ys, c['sr'], dtype=dtype, output='numpy', route=route, **mc.params(name))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


ROUTED = [(n, mc.CASES[n]['route']) for n in sorted(mc.CASES)] + [('D', 'direct')]


# ---- 1. mel energies ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name, route', ROUTED, ids=['%s-%s' % nr for nr in ROUTED])
def test_mel_energies_lie_within_the_derived_bar(name, route):
    ref = mc.reference(name, route)
    S, Smax = device_energies(name, route if name == 'D' else 'auto')
    assert S.shape == ref['S'].shape and np.isfinite(S).all() and (S >= 0).all()
    frac = mc.worst_fraction(S, ref['S'], ref['ES'])
    print('%s %s: worst energy error %.4f of its bar' % (name, route, frac))
    assert frac <= 1.0
    for u, (t0, t1) in enumerate(ref['spans']):
        assert Smax[u] == S[t0:t1].max()                                           # a maximum has no rounding


# ---- 2. cepstra and deltas ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
@pytest.mark.parametrize('name, route', ROUTED, ids=['%s-%s' % nr for nr in ROUTED])
def test_cepstra_and_deltas_lie_within_the_derived_bars(name, route, f32):
    ref = mc.reference(name, route)
    dt = np.float32 if f32 else np.float64
    streams, spans = device_streams(name, dt, route if name == 'D' else 'auto')
    assert spans == ref['spans']
    bars = mc.f32_bars(ref) if f32 else ref['bars']
    for k, (got, want, bar) in enumerate(zip(streams, ref['streams'], bars)):
        assert got.dtype == dt and got.shape == want.shape and np.isfinite(got).all()
        frac = mc.worst_fraction(got, want, bar)
        print('%s %s %s stream %d: worst error %.4f of its bar (largest bar %.2e)' % (name, route, dt.__name__, k, frac, bar.max()))
        assert frac <= 1.0


# ---- 3. bit for bit -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['A', 'C', 'F_zero', 'F_short', 'F_one'])
def test_an_utterance_alone_is_the_same_utterance_inside_the_batch(name):
    streams, spans = device_streams(name)
    S, Smax = device_energies(name)
    for u, (y, (t0, t1)) in enumerate(zip(mc.audio(name), spans)):
        alone, span = device_streams(name, ys=[y])
        assert span == [(0, t1 - t0)]
        for a, s in zip(alone, streams):
            assert same_bits(a, s[t0:t1]), (name, u)
        S1, Smax1 = device_energies(name, ys=[y])
        assert same_bits(S1, S[t0:t1]) and Smax1[0] == Smax[u]


def test_two_runs_give_the_same_bits():
    first, _ = device_streams('B')
    second, _ = device_streams('B')
    assert all(same_bits(a, b) for a, b in zip(first, second))
    assert same_bits(device_energies('B')[0], device_energies('B')[0])


@pytest.mark.parametrize('name', ['A', 'C'])
@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
def test_the_host_array_entry_is_the_device_entry_points(name, f32):
    c = mc.CASES[name]
    dt = np.float32 if f32 else np.float64
    window, M, D = mc.tables(name)
    ys = mc.audio(name)
    got = _native.mfcc(np.concatenate(ys), offsets_of(ys), c['n_fft'], c['hop'], window, M, D, mc.row_sums(name), dtype=dt)
    want, _ = device_streams(name, dt)
    assert all(same_bits(g, w) for g, w in zip(got, want))


def zero_utterance():
    streams, spans = device_streams('F_zero')
    t0, t1 = spans[1]
    assert not mc.audio('F_zero')[1].any() and t1 - t0 >= 20
    return [s[t0:t1] for s in streams]


def test_the_deltas_of_the_all_zero_utterance_vanish_behind_the_transient():
    """Every energy of the utterance is 0, so every frame has the same cepstra, and both deltas are exactly 0 once the lfilter
    transient (3 frames for the first, 11 for the second) has passed."""
    cep, d1, d2 = zero_utterance()
    assert all(same_bits(row, cep[0]) for row in cep)
    assert not d1[3:].any() and not d2[11:].any()
    assert d1[:3].any() and d2[:11].any()                                          # (the transient itself is not zero)


def test_the_all_zero_utterance_gives_the_closed_form_exactly():
    """Coefficient 0 is exactly 10 log10(1e-10) sqrt(n_mels), every other coefficient exactly 0: every Ldb is the utterance's top
    level -100, the centred sums of rule 5 are sums of zeros, and what is left is the top level times the basis' exact row sums
    (sqrt(n_mels), 0, 0, ...).  A plain sum over the rounded basis would miss both by an ulp or so (-282.84271247461896 and about
    2e-14 at n_mels = 8), as the host twin's np.dot does: that difference is inside the derived bars."""
    cep, _, _ = zero_utterance()
    n_mels = mc.CASES['F_zero']['n_mels']
    print('coefficient 0: %r against %r; the others: %r' % (cep[0, 0], 10 * np.log10(1e-10) * np.sqrt(n_mels), cep[0, 1:]))
    assert (cep[:, 0] == 10 * np.log10(1e-10) * np.sqrt(n_mels)).all()
    assert not cep[:, 1:].any()
    one, spans = device_streams('F_one', ys=[np.zeros(100, dtype=np.int16)])       # one filter, one coefficient: -100 exactly
    assert (one[0] == -100.0).all()


# ---- 4. the two routes at one size --------------------------------------------------------------------------------------------------
def test_both_routes_agree_within_the_sum_of_their_bars():
    fft, direct = mc.reference('D', 'fft'), mc.reference('D', 'direct')
    S_fft, S_direct = device_energies('D', 'fft')[0], device_energies('D', 'direct')[0]
    assert not same_bits(S_fft, S_direct)                                          # (two routes did run)
    frac = mc.worst_fraction(S_fft, S_direct.astype(mc.LD), fft['ES'] + direct['ES'])
    print('D: energies of the two routes differ by %.4f of the sum of their bars' % frac)
    assert frac <= 1.0
    a, b = device_streams('D', route='fft')[0], device_streams('D', route='direct')[0]
    for k in range(3):
        frac = mc.worst_fraction(a[k], b[k].astype(mc.LD), fft['bars'][k] + direct['bars'][k])
        print('D: stream %d of the two routes differs by %.4f of the sum of their bars' % (k, frac))
        assert frac <= 1.0


# ---- 5. end to end, exact -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['A', 'C'])
def test_hac_many_is_the_twin_s_histograms_exactly(name):
    c, case = mc.CASES[name], mc.e2e(name)
    ys = mc.audio(name)
    got = hac.hac_many(ys, c['sr'], case['codebooks'], lags=mc.E2E_LAGS, **mc.params(name))
    assert hc.same_csr(got, case['want'], np.float64)
    rows = hac.hac_many(ys, c['sr'], case['codebooks'], lags=mc.E2E_LAGS, output='device', **mc.params(name))
    assert isinstance(rows, hac.DeviceCsrRows) and hc.same_csr(rows.to_scipy(), case['want'], np.float64)
    dense = case['want'].toarray()
    for u in (0, len(ys) - 1):
        one = hac.hac(ys[u], c['sr'], case['codebooks'], lags=mc.E2E_LAGS, **mc.params(name))
        assert one.dtype == np.int64 and np.array_equal(one, dense[u])
    cep = hac.mfcc(ys[-1], sr=c['sr'], **mc.params(name))
    t0, t1 = case['spans'][-1]
    assert cep.shape == (c['n_mfcc'], t1 - t0)
    assert mc.worst_fraction(cep.T, mc.reference(name)['streams'][0][t0:t1], mc.reference(name)['bars'][0][t0:t1]) <= 1.0


# ---- 6. into the codebook builders ---------------------------------------------------------------------------------------------------
def test_codebooks_from_audio_are_the_builders_on_the_device_streams():
    c = mc.CASES['C']
    ys = mc.audio('C')
    got = hac.build_codebooks_from_audio(ys, c['sr'], mc.E2E_KS, mode='raw', rng=7, output='device', **mc.params('C'))
    streams, spans = fm.mfcc_streams(ys, c['sr'], output='device', **mc.params('C'))
    want = codebook.build_codebooks(streams, mc.E2E_KS, mode='raw', rng=7, output='device')
    assert len(got) == 3
    for g, w, k in zip(got, want, mc.E2E_KS):
        assert tuple(g.shape) == (k, c['n_mfcc']) and same_bits(g.cpu().numpy(), w.cpu().numpy())
    X = hac.windowed_hac(streams, got, spans, lags=mc.E2E_LAGS)
    assert sp.isspmatrix_csr(X) and X.shape == (len(ys), 2 * sum(k * k for k in mc.E2E_KS)) and X.nnz > 0
    iterative = hac.build_codebooks_from_audio(ys, c['sr'], (3, 2, 2), mode='iterative', **mc.params('C'))
    assert [cb.shape for cb in iterative] == [(3, 13), (2, 13), (2, 13)] and all(np.isfinite(cb).all() for cb in iterative)


# ---- 7. refusals: a status, nothing written ------------------------------------------------------------------------------------------
def test_every_refusal_of_the_header_returns_its_status_with_nothing_written():
    """All refusals are host-side checks made before any launch: the outputs keep their sentinel."""
    import torch
    lib = _native.load()
    c = mc.CASES['A']
    ys = mc.audio('A')[2:4]                                                        # 65 and 200 samples: 5 + 13 frames
    off = offsets_of(ys)
    window, M, D = mc.tables('A')
    T, U, n_fft, hop, n_mels, n_mfcc = 18, 2, 64, 16, 8, 5
    d_samples, d_window, d_mel, d_dct = on_device(np.concatenate(ys)), on_device(window), on_device(M), on_device(D)
    sums = mc.row_sums('A')
    d_sums = on_device(sums)
    wb = _native.mfcc_work_bytes(U, int(off[-1]), T, n_fft, n_mels, n_mfcc)
    d_work = torch.zeros(wb, dtype=torch.uint8, device='cuda')
    full = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float64, device='cuda')
    d_S, d_Smax, outs = full(T, n_mels), full(U), [full(T, n_mfcc) for _ in range(3)]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
    untouched = lambda: all(bool((t == SENTINEL).all()) for t in [d_S, d_Smax] + outs)

    def mel(status=_native.ERR_ARG, **change):
        a = dict(kind=_native.MFCC_I16, samples=ptr(d_samples), off=off, U=U, n_fft=n_fft, hop=hop, route=0, window=ptr(d_window),
                 mel=ptr(d_mel), n_mels=n_mels, T=T, work=ptr(d_work), wb=wb, S=ptr(d_S), Smax=ptr(d_Smax))
        a.update(change)
        o = None if a['off'] is None else i64(a['off']).ctypes.data_as(ctypes.c_void_p)
        got = lib.klnmf_mfcc_mel_device(0, a['kind'], a['samples'], o, a['U'], a['n_fft'], a['hop'], a['route'], a['window'], a['mel'],
                                        a['n_mels'], a['T'], a['work'], a['wb'], a['S'], a['Smax'])
        torch.cuda.synchronize()
        assert got == status and untouched(), (change, got)
        assert status == 0 or lib.klnmf_last_error().decode().startswith('klnmf_mfcc_mel_device: ')

    mel(off=[0, 32, 265], samples=ptr(d_samples))                                  # an utterance of 32 samples: below n_fft / 2 + 1
    mel(off=[0, 300, 265])                                                         # offsets that do not ascend
    mel(off=[1, 65, 265])
    mel(hop=0)
    mel(n_mels=0)
    mel(n_fft=1)
    for null in ('samples', 'window', 'mel', 'work', 'S', 'Smax', 'off'):
        mel(**{null: None})
    mel(kind=3)
    mel(kind=-1)
    mel(route=3)
    mel(wb=wb - 1)
    mel(T=T + 1)
    mel(U=-1)
    mel(off=[0, 2 ** 31], U=1, T=1 + 2 ** 31 // 16)                                # totals not below 2^31 - 1
    mel(status=_native.ERR_UNSUPP, n_fft=8192, off=[0, 5000], U=1, T=1 + 5000 // 16)
    mel(status=_native.ERR_UNSUPP, route=2, n_fft=2048, off=[0, 2000], U=1, T=1 + 2000 // 16)
    mel(status=_native.ERR_UNSUPP, route=1, n_fft=320, off=[0, 400], U=1, T=1 + 400 // 16)
    mel(status=_native.ERR_UNSUPP, n_fft=66 + 1, off=[0, 65, 265])                 # odd
    mel(status=_native.ERR_UNSUPP, n_mels=_native.MFCC_MAX_MELS + 1)
    mel(status=0, U=0, off=[0], T=0)                                               # no utterance: nothing done

    frames = i64([0, 5, 18])

    def cepstra(status=_native.ERR_ARG, **change):
        a = dict(dtype=_native.DT_F64, S=ptr(d_S), Smax=ptr(d_Smax), dct=ptr(d_dct), sums=ptr(d_sums), n_mels=n_mels, n_mfcc=n_mfcc, off=frames, U=U,
                 work=ptr(d_work), wb=wb, o0=ptr(outs[0]), o1=ptr(outs[1]), o2=ptr(outs[2]), ld=n_mfcc)
        a.update(change)
        o = None if a['off'] is None else i64(a['off']).ctypes.data_as(ctypes.c_void_p)
        got = lib.klnmf_mfcc_cepstra_device(0, a['dtype'], a['S'], a['Smax'], a['dct'], a['sums'], a['n_mels'], a['n_mfcc'], o, a['U'],
                                            a['work'],
                                            a['wb'], a['o0'], a['o1'], a['o2'], a['ld'])
        torch.cuda.synchronize()
        assert got == status and untouched(), (change, got)

    cepstra(n_mfcc=9)                                                              # above n_mels
    cepstra(n_mfcc=0)
    cepstra(n_mels=0)
    cepstra(dtype=2)
    cepstra(ld=4)
    cepstra(off=[0, 5, 5])
    cepstra(off=[0, 7, 5])
    cepstra(off=[1, 5, 18])
    cepstra(wb=16)
    for null in ('S', 'Smax', 'dct', 'sums', 'work', 'o0', 'o1', 'o2', 'off'):
        cepstra(**{null: None})
    cepstra(status=_native.ERR_UNSUPP, n_mels=_native.MFCC_MAX_MELS + 1)
    cepstra(status=0, U=0, off=[0])

    # the host-array wrapper: host outputs keep their sentinel
    host = [np.full((T, n_mfcc), SENTINEL) for _ in range(3)]
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    samples = np.concatenate(ys)

    def wrapper(status, off_, n_mfcc_=n_mfcc, dtype=_native.DT_F64, T_=T):
        o = i64(off_)
        got = lib.klnmf_mfcc(0, _native.MFCC_I16, dtype, p(samples), p(o), len(o) - 1, n_fft, hop, 0, p(window), p(M), n_mels, p(D),
                             p(sums), n_mfcc_, T_, p(host[0]), p(host[1]), p(host[2]), n_mfcc)
        assert got == status and all((h == SENTINEL).all() for h in host), (off_, got)

    wrapper(_native.ERR_ARG, [0, 32, 265])
    wrapper(_native.ERR_ARG, off, n_mfcc_=9)
    wrapper(_native.ERR_ARG, off, dtype=7)
    wrapper(_native.ERR_ARG, off, T_=T - 1)
    # and the same arguments, unchanged, are taken
    assert lib.klnmf_mfcc(0, _native.MFCC_I16, _native.DT_F64, p(samples), p(off), U, n_fft, hop, 0, p(window), p(M), n_mels, p(D),
                          p(sums), n_mfcc, T, p(host[0]), p(host[1]), p(host[2]), n_mfcc) == 0
    assert not any((h == SENTINEL).any() for h in host)
