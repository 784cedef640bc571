"""Cases, extended-precision references and DERIVED error bars of the MFCC front end (tests/test_mfcc_cpu.py,
tests/test_mfcc_gpu.py).  numpy and scipy only; nothing here touches a GPU.

Audio: a few gliding tones of amplitude AMPLITUDE in all, plus white noise of NOISE * AMPLITUDE (3 %; the cases ask for a floor
of at least 1 %), rounded to integers inside the int16 range.  The noise floor is what keeps every mel energy far enough above
the transform's absolute error that the decibel bars below stay small: test_mfcc_cpu.py asserts, on the reference alone, that
every case's largest cepstral bar is below CEPSTRAL_BAR_LIMIT = 1e-8 dB.

THE REFERENCE is the rules of multimodal_amd/features/mfcc.py evaluated in np.longdouble (64-bit significand, u_x = 2^-64): the
frames and the window product, scipy.fft.rfft, the filter bank, then the twin's own `host_mfcc` on the longdouble energies and
the delta sums written out (`delta_ld`: scipy's lfilter does not take longdouble; test_mfcc_cpu.py holds it against
`host_delta`).  Its own error is 2^-11 of fp64's and is left out of the bars.

THE BARS.  u = 2^-53, gamma_k = k u / (1 - k u).  x: the windowed frame in exact arithmetic, n = n_fft, X = its transform.

 frame     The device rounds the product sample * window: |dx_j| <= u |x_j|, which moves any bin by at most u ||x||_1
           <= u sqrt(n) ||x||_2.
 fft       Radix 2 with a twiddle table whose entries are off by mu <= u (cos and sin each the nearest double): the standard
           bound (Higham, Accuracy and Stability, Theorem 24.2) is ||dX||_2 <= log2(n) eta / (1 - log2(n) eta) ||X||_2 with
           eta = mu + gamma_4 (sqrt(2) + mu) < 6.7 u, and ||X||_2 = sqrt(n) ||x||_2.  A bin's error is at most the vector's:
           E_X = (7 log2(n) + 1) u sqrt(n) ||x||_2.
 direct    Real and imaginary part are dot products of n terms against table entries off by u / 2: each is off by at most
           (gamma_n + u / 2) ||x||_1; together sqrt(2) of it, and the frame's rounding:
           E_X = (sqrt(2) (1.001 n + 0.5) + 1) u ||x||_1        (gamma_n <= 1.001 n u for n <= 1024).
 power     P = re^2 + im^2, two products and a sum: relative 2 u on what was computed.
           E_P = 2 |X| E_X + E_X^2 + 2 u (|X| + E_X)^2.
 mel       S_m = sum_b M_mb P_b, non-negative terms, at most n_bins of them:
           E_S = sum_b M_mb E_P,b + gamma_nbins sum_b M_mb (P_b + E_P,b).
 log       slope 10 / (ln 10 max(S, 1e-10)) times E_S, plus the device's log10 -- OpenCL's bound for a double log10, 3 ulp,
           which the device library is built to -- and half an ulp for the product with 10: LOG10_ULPS = 3.5 ulps of |Ldb|, an
           ulp at most 2 u |Ldb|.  The floor: max(a, b) moves by no more than its arguments; the utterance's maximum moves by
           at most the largest E_S of the utterance, at the slope of Smax, and the subtraction of 80 rounds once.
           E_L = max(slope(S) E_S + 7 u |Ldb|,  slope(Smax) max E_S + 7 u |Lmax| + u |Lmax - 80|).
 dct       The device sums the levels below the top, v_m = Ldb_m - Lmax in [-80, 0], and adds Lmax r_i with the basis' exact row
           sums r.  v moves by both levels' bars and rounds once: E_v = E_L + E_Lmax + u |v|.  Against the reference's D . Ldb
           with the same rounded table, the exact identity leaves |Lmax| |sum_m D_im - r_i| (the table's row sums are a few
           ulps off r); the product Lmax r_i carries E_Lmax |r_i| and one rounding, the last sum one more:
           E_c,i = sum_m |D_im| E_v,m + gamma_nmels sum_m |D_im| (|v_m| + E_v,m) + |Lmax| |sum_m D_im - r_i|
                   + (E_Lmax + u (|Lmax| + E_Lmax)) |r_i| + u (everything above + sum_m |D_im| |v_m| + |Lmax r_i|).
 deltas    Nine taps of absolute sum 20, each output a product and at most eight sums: with E_c,i and |c_i| at their largest
           over the utterance,  E_d1 = 20 max E_c + 20 gamma_10 max |c|,  E_d2 = 400 max E_c + 2 * 400 gamma_10 max |c|.
 float32   half an ulp of float32 of the value: 2^-24 (|value| + bar).

The bars are elementwise: `energy_bar` [T, n_mels], `stream_bars` three [T, n_mfcc].
"""
import functools

import numpy as np
import scipy.fft

from multimodal_amd.features import mfcc as fm

AMPLITUDE, NOISE = 8000.0, 0.03
U = 2.0 ** -53
LOG10_ULPS = 3.5
CEPSTRAL_BAR_LIMIT = 1e-8
LD = np.longdouble

A = dict(sr=16000, n_fft=64, hop=16, n_mels=8, n_mfcc=5, route='fft', lengths=(33, 64, 65, 200, 1000), kind=np.int16, seed=101)
CASES = {
    'A': A,
    'B': dict(sr=22050, n_fft=2048, hop=512, n_mels=128, n_mfcc=13, route='fft', lengths=(1025, 5000, 22050), kind=np.float32, seed=102),
    'C': dict(sr=16000, n_fft=320, hop=160, n_mels=30, n_mfcc=13, route='direct', lengths=(161, 1600, 4801), kind=np.float64, seed=103),
    # hop 100 divides neither 256 nor a length; both routes take 256 points
    'D': dict(sr=8000, n_fft=256, hop=100, n_mels=20, n_mfcc=10, route='fft', lengths=(129, 777, 1000), kind=np.int16, seed=104),
    'E': dict(sr=44100, n_fft=4096, hop=1024, n_mels=40, n_mfcc=13, route='fft', lengths=(9000,), kind=np.float32, seed=105),
    # an all-zero utterance between two others; an utterance of 3 frames (47 // 16 + 1); one filter and one coefficient
    'F_zero': dict(A, lengths=(200, 400, 300), zero=(1,), seed=106),
    'F_short': dict(A, lengths=(47, 120), seed=107),
    'F_one': dict(A, n_mels=1, n_mfcc=1, lengths=(100, 33), seed=108),
    # 1200 utterances of 3 frames each: the utterance of a frame, looked up on the grid
    'G': dict(sr=16000, n_fft=64, hop=16, n_mels=6, n_mfcc=4, route='fft', lengths=tuple(33 + (7 * i) % 8 for i in range(1200)),
              kind=np.int16, seed=109),
}


def params(name):
    c = CASES[name]
    return dict(n_mfcc=c['n_mfcc'], n_fft=c['n_fft'], hop_length=c['hop'], n_mels=c['n_mels'])


@functools.lru_cache(maxsize=None)
def audio(name):
    """The utterances of a case: read-only arrays of the case's kind, integer-valued."""
    c = CASES[name]
    rng = np.random.default_rng(c['seed'])
    out = []
    for u, L in enumerate(c['lengths']):
        t = np.arange(L) / float(c['sr'])
        y = np.zeros(L)
        for _ in range(3):
            f0, f1 = rng.uniform(0.02, 0.4, size=2) * c['sr']
            phase = 2 * np.pi * (f0 * t + 0.5 * (f1 - f0) * t * t / max(t[-1], 1e-9)) + rng.uniform(0, 2 * np.pi)
            y += (AMPLITUDE / 3) * np.sin(phase)
        y += rng.normal(0.0, NOISE * AMPLITUDE, size=L)
        if u in c.get('zero', ()):
            y[:] = 0.0
        y = np.clip(np.round(y), -32768, 32767).astype(c['kind'])
        y.setflags(write=False)
        out.append(y)
    return out


def row_sums(name):
    c = CASES[name]
    return fm.dct_row_sums(c['n_mfcc'], c['n_mels'])


def tables(name):
    c = CASES[name]
    return fm.hann(c['n_fft']), fm.mel_filters(c['sr'], c['n_fft'], c['n_mels']), fm.dct_basis(c['n_mfcc'], c['n_mels'])


def gamma(k):
    return k * U / (1 - k * U)


def transform_bar(route, n, norm1, norm2):
    """E_X per frame, from the frame's 1-norm and 2-norm."""
    if route == 'fft':
        return (7 * np.log2(n) + 1) * U * np.sqrt(n) * norm2
    return (np.sqrt(2.0) * (1.001 * n + 0.5) + 1) * U * norm1


def energies_ld(y, n_fft, hop, window, M, route):
    """(S longdouble [T, n_mels], E_S float64 [T, n_mels]) of one utterance."""
    yp = np.pad(np.asarray(y).astype(LD), n_fft // 2, mode='reflect')
    T = 1 + len(y) // hop
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]
    x = yp[idx] * window.astype(LD)
    X = scipy.fft.rfft(x, axis=1)
    assert X.dtype == np.complex256
    P = X.real ** 2 + X.imag ** 2
    Mld = M.astype(LD)
    S = P @ Mld.T
    EX = transform_bar(route, n_fft, np.abs(x).sum(axis=1), np.sqrt((x * x).sum(axis=1)))[:, None]
    absX = np.sqrt(P)
    EP = 2 * absX * EX + EX ** 2 + 2 * U * (absX + EX) ** 2
    ES = EP @ Mld.T + gamma(n_fft // 2 + 1) * ((P + EP) @ Mld.T)
    return S, ES.astype(np.float64)


def delta_ld(c, order):
    """Rule 6 on c [T, n_mfcc] in longdouble, the sums written out: y[k] = sum_r (4 - r) xp[k - r] on the edge-padded axis."""
    x = np.pad(np.asarray(c, dtype=LD), [(5, 5), (0, 0)], mode='edge')
    for _ in range(order):
        y = np.zeros_like(x)
        for r in range(9):
            y[r:] += LD(4 - r) * x[:len(x) - r]
        x = y
    return x[5:-5]


def cepstral_bars(S, ES, D, R):
    """(E_c [T, n_mfcc], Ldb) of one utterance from its reference energies and their bar; R: the basis' exact row sums."""
    S64 = S.astype(np.float64)
    slope = lambda s: 10.0 / (np.log(10.0) * np.maximum(s, fm.AMIN))
    Ldb = 10 * np.log10(np.maximum(S64, fm.AMIN))
    Lmax = Ldb.max()
    own = slope(S64) * ES + LOG10_ULPS * 2 * U * np.abs(Ldb)
    top = slope(S64.max()) * ES.max() + LOG10_ULPS * 2 * U * abs(Lmax) + U * abs(Lmax - fm.TOP_DB)
    EL = np.maximum(own, top)
    Ldb = np.maximum(Ldb, Lmax - fm.TOP_DB)
    absD, absR = np.abs(D), np.abs(R)[None, :]
    v = np.abs(Ldb - Lmax)
    Ev = EL + top + U * v
    size = v @ absD.T + abs(Lmax) * absR
    Ec = Ev @ absD.T + gamma(S.shape[1]) * ((v + Ev) @ absD.T)
    Ec = Ec + abs(Lmax) * np.abs(D.astype(LD).sum(axis=1) - R.astype(LD)).astype(np.float64)[None, :]
    Ec = Ec + (top + U * (abs(Lmax) + top)) * absR
    return Ec + U * (Ec + size), Ldb


@functools.lru_cache(maxsize=None)
def reference(name, route=None):
    """dict(S, ES: the energies [T_total, n_mels] (longdouble) and their bar; streams: three [T_total, n_mfcc] longdouble;
    bars: three float64 (for float64 output); spans) of a case, the bars for `route` (the case's own by default)."""
    c = CASES[name]
    window, M, D = tables(name)
    Ss, ESs, streams, bars = [], [], [[], [], []], [[], [], []]
    for y in audio(name):
        S, ES = energies_ld(y, c['n_fft'], c['hop'], window, M, route or c['route'])
        Ec, _ = cepstral_bars(S, ES, D, row_sums(name))
        cep = fm.host_mfcc(S, D)
        assert cep.dtype == LD
        worst, size = Ec.max(axis=0), np.abs(cep).max(axis=0).astype(np.float64)
        ones = np.ones((len(cep), 1))
        Ss.append(S)
        ESs.append(ES)
        for k, (value, bar) in enumerate(((cep, Ec), (delta_ld(cep, 1), ones * (20 * worst + 20 * gamma(10) * size)),
                                          (delta_ld(cep, 2), ones * (400 * worst + 800 * gamma(10) * size)))):
            streams[k].append(value)
            bars[k].append(bar)
    spans = fm.frame_spans([len(S) for S in Ss])
    return dict(S=np.vstack(Ss), ES=np.vstack(ESs), streams=[np.vstack(s) for s in streams], bars=[np.vstack(b) for b in bars],
                spans=spans)


def f32_bars(ref):
    """The bars of float32 streams: the float64 bar and half a float32 ulp of the value."""
    return [b + 2.0 ** -24 * (np.abs(s).astype(np.float64) + b) for s, b in zip(ref['streams'], ref['bars'])]


def worst_fraction(got, want, bar):
    """max |got - want| / bar over the elements (0 / 0 counts as 0): what a test prints before it asserts <= 1."""
    err = np.abs(np.asarray(got).astype(LD) - want).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        frac = np.where(err == 0, 0.0, err / bar)
    return float(frac.max()) if frac.size else 0.0


# ---- the end-to-end cases: codebooks on the twin's streams, and the condition under which the labels cannot differ -----------------
E2E_KS = (5, 7, 3)
E2E_LAGS = [5, 2]


@functools.lru_cache(maxsize=None)
def e2e(name):
    """dict(streams, spans, codebooks, want: the CSR matrix of `host_windowed_hac` over the utterances' spans) from the float64
    twin."""
    from multimodal_amd.features import codebook, hac
    c = CASES[name]
    streams, spans = fm.host_mfcc_streams(audio(name), c['sr'], **params(name))
    rng = np.random.default_rng(c['seed'] + 1000)
    codebooks = [codebook.host_build_codebook(x, k, mode='raw', rng=rng) for x, k in zip(streams, E2E_KS)]
    want = hac.host_windowed_hac(streams, codebooks, spans, lags=E2E_LAGS)
    return dict(streams=streams, spans=spans, codebooks=codebooks, want=want)


def label_margins(name):
    """Per stream, [T] float64: (gap between the second-nearest and the nearest squared distance of the twin's frame) minus what
    the bars can move it by.  Device and twin streams each lie within the stream's bar E (elementwise) of the exact values, so
    they differ by at most e = 2 E; a squared distance sum_j (x_j - c_j)^2 of value d^2 then moves by at most
    2 d ||e||_2 + ||e||_2^2 (Cauchy-Schwarz), and each side's own evaluation in fp64 by gamma_{2 dim + 1} d^2.  Positive
    everywhere: the labels, and with them every count, are equal."""
    ref, case = reference(name), e2e(name)
    out = []
    for x, cb, bar in zip(case['streams'], case['codebooks'], ref['bars']):
        d2 = ((x[:, None, :] - cb[None, :, :]) ** 2).sum(axis=2)
        d2.sort(axis=1)
        near, second = d2[:, 0], d2[:, 1]
        e = 2 * np.sqrt((bar * bar).sum(axis=1))
        moved = lambda v: 2 * np.sqrt(v) * e + e * e + 2 * gamma(2 * x.shape[1] + 1) * v
        out.append(second - near - moved(near) - moved(second))
    return out
