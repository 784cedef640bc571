"""What the host halves of the feature units (nearest-example search, information matrix, HAC histograms, k-means codebooks, motion
modality) decide without a device, held against values RECORDED from the library before their shared scaffold
(csrc/feature_host.hip.h) existed: the five klnmf_*_work_bytes answers over a grid with the zero sizes, the sizes at which a piece's
rounding to 16 bytes steps, and for k-means d on both sides of KLNMF_KMEANS_GRAM_MAX_D; and per unit the refusals that are decided
before any device call -- a null `bytes`, a dtype that is none, a workspace one byte short -- with their status code and their
message, byte for byte.  The pointers of the refused calls are made-up addresses: a refusal touches nothing."""
import ctypes

import numpy as np
import pytest

from multimodal_amd import _native

# (entry point, sizes, bytes), recorded
WORK_BYTES = [
    ('nearest', (0, 0), 0),
    ('nearest', (1, 0), 64),
    ('nearest', (1, 1), 68),
    ('nearest', (1, 4), 80),
    ('nearest', (2, 5), 132),
    ('nearest', (3, 7), 204),
    ('nearest', (5, 1000), 4288),
    ('nearest', (1 << 20, 1 << 24), 125829120),
    ('information', (0, 0, 1, 1), 0),
    ('information', (1, 1, 1, 1), 4208),
    ('information', (1, 3, 2, 10), 12656),
    ('information', (3, 7, 5, 10), 30384),
    ('information', (4, 7, 5, 10), 30432),
    ('information', (2, 50, 10, 256), 717728),
    ('information', (1, 1, 65536, 256), 67113056),
    ('hac', (1, 0, 1, 0), 16),
    ('hac', (1, 1, 1, 1), 64),
    ('hac', (1, 3, 1, 1), 64),
    ('hac', (1, 4, 1, 1), 64),
    ('hac', (1, 5, 1, 1), 80),
    ('hac', (1, 5, 1, 2), 96),
    ('hac', (1, 5, 1, 3), 112),
    ('hac', (3, 400, 2, 40), 8016),
    ('hac', (8, 5, 8, 3), 2512),
    ('hac', (2, 1001, 3, 7), 8608),
    ('kmeans', (0, 1, 1), 48),
    ('kmeans', (1, 1, 1), 48),
    ('kmeans', (1, 3, 5), 160),
    ('kmeans', (4096, 13, 1000), 108000),
    ('kmeans', (4097, 39, 150), 94800),
    ('kmeans', (100, 64, 3), 17184),
    ('kmeans', (100, 65, 3), 1584),
    ('kmeans', (5000, 64, 1), 34336),
    ('kmeans', (5000, 65, 1), 1056),
    ('kmeans', (4096 * 3 + 1, 2, 2), 192),
    ('motion', (0, 0, 1, 1, 0, 1, 0), 272),
    ('motion', (1, 0, 1, 1, 0, 1, 0), 272),
    ('motion', (1, 1, 1, 1, 0, 1, 0), 288),
    ('motion', (1, 2, 1, 1, 0, 1, 0), 288),
    ('motion', (1, 3, 1, 1, 0, 1, 0), 304),
    ('motion', (100, 9, 1, 1, 0, 1, 3), 368),
    ('motion', (5000, 93, 3, 16, 7, 2, 11), 6864),
    ('motion', (4097, 0, 16, 64, 3, 1, 0), 51072),
    ('motion', (10, 0, 2, 5, 0, 3, 1000), 128272),
    ('motion', (10, 0, 2, 5, 1, 3, 0), 448),
]


@pytest.mark.parametrize('unit', ['nearest', 'information', 'hac', 'kmeans', 'motion'])
def test_the_workspace_sizes_are_the_recorded_ones(unit):
    rows = [r for r in WORK_BYTES if r[0] == unit]
    assert len(rows) >= 7
    for _, sizes, want in rows:
        assert getattr(_native, unit + '_work_bytes')(*sizes) == want, (unit, sizes)


def work_bytes_measured():
    """The table above as the loaded library answers it (how it was recorded, with KLNMF_LIB naming the earlier library)."""
    return [(unit, sizes, getattr(_native, unit + '_work_bytes')(*sizes)) for unit, sizes, _ in WORK_BYTES]


# ---- refusals decided before any device call ----------------------------------------------------------------------------------------
P = 4096            # a made-up device address: not null, never dereferenced
BAD_DT = 7


def table(struct, *rows):
    t = (struct * len(rows))(*[struct(*r) for r in rows])
    return ctypes.cast(t, ctypes.c_void_p), t          # (the array rides along so that it outlives the call)


def i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


def i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


def refusals():
    """[(entry point, arguments)]: each refused on host arithmetic alone."""
    N = _native
    near, _n = table(N.NearestJob, (P, 2, P, 2, 3, 2, 2))
    info, _i = table(N.InformationJob, (P, 2, P, 5, 2))
    hacs, _h = table(N.HacStream, (P, 2, P, 2, 2, 3))
    lags, windows, K = i32(1), i64(0, 5), i64(3)
    unfinished, count, nnz = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int64(0)
    keep = (_n, _i, _h, lags, windows, K, unfinished, count, nnz)
    short = lambda unit, *sizes: getattr(N, unit + '_work_bytes')(*sizes) - 1
    return keep, [
        ('klnmf_nearest_work_bytes', (1, 1, None)),
        ('klnmf_nearest_many_device', (0, BAD_DT, 1, near, 1, P, P, P, 1 << 20)),
        ('klnmf_nearest_many_device', (0, N.DT_F64, 1, near, 1, P, P, P, short('nearest', 1, 3))),
        ('klnmf_nearest', (0, BAD_DT, 1, 3, 2, 2, P, P, P, None)),
        ('klnmf_information_work_bytes', (1, 1, 1, 1, None)),
        ('klnmf_information_many_device', (0, BAD_DT, 2, 3, info, 1, P, None, P, 1 << 20)),
        ('klnmf_information_many_device', (0, N.DT_F32, 2, 3, info, 1, P, None, P, short('information', 1, 2, 2, 3))),
        ('klnmf_information', (0, BAD_DT, 2, 3, 5, 2, P, P, P, None)),
        ('klnmf_hac_work_bytes', (1, 5, 1, 1, None)),
        ('klnmf_hac_count_device', (0, BAD_DT, hacs, 1, 5, lags, 1, windows, 1, P, 1 << 20, P, ctypes.byref(nnz))),
        ('klnmf_hac_count_device', (0, N.DT_F64, hacs, 1, 5, lags, 1, windows, 1, P, short('hac', 1, 5, 1, 1), P, ctypes.byref(nnz))),
        ('klnmf_hac_fill_device', (0, BAD_DT, K, 1, 5, lags, 1, windows, 1, P, 1 << 20, 4, P, P)),
        ('klnmf_hac_fill_device', (0, N.DT_F32, K, 1, 5, lags, 1, windows, 1, P, short('hac', 1, 5, 1, 1), 4, P, P)),
        ('klnmf_hac', (0, N.DT_F64, BAD_DT, hacs, 1, 5, lags, 1, windows, 1, P, 4, P, P, ctypes.byref(nnz))),
        ('klnmf_kmeans_work_bytes', (10, 2, 3, None)),
        ('klnmf_kmeans_device', (0, BAD_DT, P, 2, 10, 2, P, 2, 3, 1, P, 1 << 20, P, P)),
        ('klnmf_kmeans_device', (0, N.DT_F64, P, 2, 10, 2, P, 2, 3, 1, P, short('kmeans', 10, 2, 3), P, P)),
        ('klnmf_kmeans_device', (0, N.DT_F64, P, 200, 10, 200, P, 200, 100, 1, P, 1 << 30, P, P)),
        ('klnmf_kmeans_gram_device', (0, N.DT_F32, P, 2, 10, 2, P, 0, P, 79, P, P, ctypes.byref(count))),
        ('klnmf_kmeans_gram_device', (0, N.DT_F32, P, 65, 10, 65, P, 0, P, 1 << 20, P, P, ctypes.byref(count))),
        ('klnmf_kmeans', (0, BAD_DT, P, 2, 10, 2, P, 2, 3, 1, P, P)),
        ('klnmf_motion_work_bytes', (10, 0, 1, 1, 0, 1, 0, None)),
        ('klnmf_motion_whiten_device', (0, BAD_DT, P, 3, 10, 3, P, 1 << 20, P, 3, P, P)),
        ('klnmf_motion_whiten_device', (0, N.DT_F64, P, 3, 10, 3, P, short('motion', 10, 3), P, 3, P, P)),
        ('klnmf_motion_kmeans_device', (0, N.DT_F64, P, 0, 2, 10, 2, 1, i32(0), 1, P, 300, 1e-5, 5, P, 1 << 20, P, P, P, P,
                                        ctypes.byref(unfinished))),
        ('klnmf_motion_hist_device', (0, N.DT_F32, P, 0, 2, 10, 2, 1, P, 4, i64(0, 10), 1, 0, 1.0, P, short('motion', 10, 0, 2, 4, 0, 1, 1),
                                      P, 4)),
    ]


# (status, message) of refusals()[i], recorded
REFUSED = [
    (-1, 'klnmf_nearest_work_bytes: null bytes'),
    (-1, 'klnmf_nearest_many_device: dtype must be KLNMF_DT_F32 or KLNMF_DT_F64'),
    (-1, 'klnmf_nearest_many_device: workspace below klnmf_nearest_work_bytes'),
    (-1, 'klnmf_nearest: dtype must be KLNMF_DT_F32 or KLNMF_DT_F64'),
    (-1, 'klnmf_information_work_bytes: null bytes'),
    (-1, 'klnmf_information_many_device: dtype must be KLNMF_DT_F32 or KLNMF_DT_F64'),
    (-1, 'klnmf_information_many_device: workspace below klnmf_information_work_bytes'),
    (-1, 'klnmf_information: dtype must be KLNMF_DT_F32 or KLNMF_DT_F64'),
    (-1, 'klnmf_hac_work_bytes: null bytes'),
    (-1, 'klnmf_hac_count_device: dtype must be KLNMF_DT_F32 or KLNMF_DT_F64'),
    (-1, 'klnmf_hac_count_device: workspace below klnmf_hac_work_bytes'),
    (-1, 'klnmf_hac_fill_device: value_dtype must be KLNMF_DT_F32 or KLNMF_DT_F64'),
    (-1, 'klnmf_hac_fill_device: workspace below klnmf_hac_work_bytes'),
    (-1, 'klnmf_hac: value_dtype must be KLNMF_DT_F32 or KLNMF_DT_F64'),
    (-1, 'klnmf_kmeans_work_bytes: null bytes'),
    (-1, 'klnmf_kmeans_device: dtype must be KLNMF_DT_F32 or KLNMF_DT_F64'),
    (-1, 'klnmf_kmeans_device: workspace below klnmf_kmeans_work_bytes'),
    (-4, 'klnmf_kmeans_device: K * d = 100 * 200 is above 13312 fp64 accumulators in LDS'),
    (-1, 'klnmf_kmeans_gram_device: workspace below klnmf_kmeans_work_bytes'),
    (-4, 'klnmf_kmeans_gram_device: d = 65 is above 64'),
    (-1, 'klnmf_kmeans: dtype must be KLNMF_DT_F32 or KLNMF_DT_F64'),
    (-1, 'klnmf_motion_work_bytes: null bytes'),
    (-1, 'klnmf_motion_whiten_device: dtype must be KLNMF_DT_F32 or KLNMF_DT_F64'),
    (-1, 'klnmf_motion_whiten_device: workspace below klnmf_motion_work_bytes'),
    (-4, 'klnmf_motion_kmeans_device: K = 300, d = 2 beyond K <= 256, d <= 16, K * d <= 1024'),
    (-1, 'klnmf_motion_hist_device: workspace below klnmf_motion_work_bytes'),
]


def refusals_measured():
    lib = _native.load()
    keep, calls = refusals()
    out = []
    for entry, args in calls:
        status = getattr(lib, entry)(*args)
        out.append((status, lib.klnmf_last_error().decode() if status else ''))
    del keep
    return out


def test_the_refusals_keep_their_codes_and_their_words():
    got = refusals_measured()
    _, calls = refusals()
    assert len(got) == len(REFUSED) == len(calls)
    for (entry, _), g, want in zip(calls, got, REFUSED):
        assert g == want, entry
    units = {'nearest', 'information', 'hac', 'kmeans', 'motion'}
    assert {e.split('_')[1] for e, _ in calls} == units
    for kind in ('null bytes', 'dtype must be', 'workspace below'):          # each kind in every unit
        assert {m.split('_')[1].split(':')[0] for _, m in REFUSED if kind in m} == units, kind


def test_the_binding_s_helpers():
    assert (_native._dt_code(True), _native._dt_code(False)) == (_native.DT_F64, _native.DT_F32)
    assert (_native._dt_code(np.float32 != np.float32), _native._dt_code(np.float64 != np.float32)) == (_native.DT_F32, _native.DT_F64)
    rows = [(P, 2, 0, 3, 5, 7, 11), (0, 1, P + 8, 1, 0, 0, 0)]
    jobs = ctypes.cast(_native._job_table(_native.NearestJob, rows), ctypes.POINTER(_native.NearestJob))
    assert [(jobs[q].A, jobs[q].lda, jobs[q].B, jobs[q].ldb, jobs[q].na, jobs[q].nb, jobs[q].d) for q in range(2)] \
        == [(P, 2, None, 3, 5, 7, 11), (None, 1, P + 8, 1, 0, 0, 0)]
    assert _native._job_table(_native.HacStream, []).value                         # never a null table
    padded = ctypes.cast(_native._job_table(_native.HacStream, [(P, 1, P, 1, 1, 1)], at_least=3), ctypes.POINTER(_native.HacStream))
    assert padded[0].frames == P and padded[2].frames is None and padded[2].K == 0
