"""ctypes binding of libklnmf.so (the C-ABI declared in include/klnmf.h).

There is no CPU fallback: if the HIP library is missing or no gfx950 device
is usable, everything that computes raises.  The binding mirrors the header one
to one; `Context` is a thin RAII wrapper used by `lib/nmf.py`.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('KLNMF_LIB') or os.path.join(_HERE, 'csrc', 'libklnmf.so')   # KLNMF_LIB: A/B builds

PREC_F64, PREC_F32, PREC_BF16 = 0, 1, 2
# fp32 storage and loop, the dense contractions as hi.hi + hi.lo + lo.hi of bf16 operand parts (csrc/split3.hip.h)
PREC_BF16X3 = 4
# fp32 storage, the dense contractions as hi.hi + hi.lo + lo.hi of power-of-two-scaled fp16 operand parts; k <= 256: the loop's
# row and column passes are fused split-fp16 kernels (csrc/f16x3.hip.h), k > 256: bf16x3's kernels
PREC_F16X3 = 5
PRECISIONS = {'f64': PREC_F64, 'fp64': PREC_F64, 'float64': PREC_F64,
              'f32': PREC_F32, 'fp32': PREC_F32, 'float32': PREC_F32,
              'f16': PREC_BF16, 'fp16': PREC_BF16, 'float16': PREC_BF16,
              # the 16-bit mode's historical name (its MFMA operands were bf16 in round 1; fp16 with power-of-two
              # scaling since: same matrix rate, 8x smaller operand rounding -- csrc/mfma.hip.h)
              'bf16': PREC_BF16,
              'bf16x3': PREC_BF16X3,
              'f16x3': PREC_F16X3}
DT_F32, DT_F64 = 0, 1
_dt_code = lambda f64: DT_F64 if f64 else DT_F32          # the KLNMF_DT_* of a call that says f64=True / False
STREAM_DEFAULT = (1 << 64) - 1        # KLNMF_STREAM_DEFAULT: (void *)(intptr_t)-1

ERR_ARG, ERR_ALLOC, ERR_HIP, ERR_UNSUPP, ERR_RCCL, ERR_REPLICA = -1, -2, -3, -4, -5, -6
COMM_ID_BYTES = 128

_c = ctypes
_ctx_p = _c.c_void_p
_i64 = _c.c_int64
_ptr = lambda address: _c.c_void_p(address or None)       # a device pointer argument: 0 is NULL

# name -> (restype, argtypes); must list every symbol of include/klnmf.h
SIGNATURES = {
    'klnmf_version': (_c.c_int, []),
    'klnmf_last_error': (_c.c_char_p, []),
    'klnmf_device_info': (_c.c_int, [_c.c_int, _c.c_char_p, _c.c_int,
                                     _c.POINTER(_c.c_int), _c.POINTER(_c.c_uint64)]),
    'klnmf_create': (_c.c_int, [_c.POINTER(_ctx_p), _c.c_int, _c.c_int, _c.c_void_p]),
    'klnmf_destroy': (_c.c_int, [_ctx_p]),
    'klnmf_set_problem': (_c.c_int, [_ctx_p, _i64, _i64, _i64, _i64]),
    'klnmf_release_problem': (_c.c_int, [_ctx_p]),
    'klnmf_set_v_max': (_c.c_int, [_ctx_p, _c.c_double]),
    'klnmf_reset_V': (_c.c_int, [_ctx_p]),
    'klnmf_upload_V': (_c.c_int, [_ctx_p, _c.c_void_p, _c.c_int, _i64, _i64, _i64,
                                  _i64, _i64, _c.c_double]),
    'klnmf_upload_weights': (_c.c_int, [_ctx_p, _c.c_void_p, _c.c_int, _i64, _i64, _i64, _i64, _i64]),
    'klnmf_clear_weights': (_c.c_int, [_ctx_p]),
    'klnmf_upload_presence': (_c.c_int, [_ctx_p, _c.c_void_p, _c.c_int, _i64, _i64, _i64, _c.POINTER(_i64), _c.c_int]),
    'klnmf_upload_presence_device_rows': (_c.c_int, [_ctx_p, _c.c_void_p, _c.c_int, _i64, _i64, _c.c_void_p, _i64, _i64,
                                                     _c.POINTER(_c.c_int), _c.POINTER(_i64), _c.c_int]),
    'klnmf_upload_V_device_rows': (_c.c_int, [_ctx_p, _c.c_void_p, _c.c_void_p, _i64, _i64, _i64, _i64, _i64,
                                              _c.c_double]),
    'klnmf_upload_V_device': (_c.c_int, [_ctx_p, _c.c_void_p, _i64, _i64, _i64, _i64,
                                         _i64, _c.c_double]),
    'klnmf_set_H': (_c.c_int, [_ctx_p, _c.c_void_p, _c.c_int]),
    'klnmf_set_W': (_c.c_int, [_ctx_p, _c.c_void_p, _c.c_int]),
    'klnmf_set_Q': (_c.c_int, [_ctx_p, _c.c_void_p, _c.c_int]),
    'klnmf_init_W': (_c.c_int, [_ctx_p]),
    'klnmf_run': (_c.c_int, [_ctx_p, _i64, _c.c_int, _c.c_double,
                             _c.POINTER(_c.c_double), _c.POINTER(_i64),
                             _c.POINTER(_c.c_int)]),
    'klnmf_loop_begin': (_c.c_int, [_ctx_p]),
    'klnmf_loop_begin_sharded': (_c.c_int, [_ctx_p, _c.c_double, _c.c_double]),
    'klnmf_loop_begin_sharded_nnz': (_c.c_int, [_ctx_p, _c.c_double, _c.c_double, _c.c_double]),
    'klnmf_loop_begin_agreed': (_c.c_int, [_ctx_p, _c.c_double, _c.c_double, _c.c_double, _c.c_int]),
    'klnmf_run_more': (_c.c_int, [_ctx_p, _i64, _c.c_int, _c.c_double]),
    'klnmf_iter_rowpass': (_c.c_int, [_ctx_p, _c.c_int]),
    'klnmf_iter_decide': (_c.c_int, [_ctx_p, _c.c_double]),
    'klnmf_iter_colpass': (_c.c_int, [_ctx_p]),
    'klnmf_iter_colpass_part': (_c.c_int, [_ctx_p, _c.c_int]),
    'klnmf_exchange_parts': (_c.c_int, [_ctx_p, _c.POINTER(_c.c_int), _c.POINTER(_i64), _c.POINTER(_i64), _c.POINTER(_i64),
                                        _c.POINTER(_i64)]),
    'klnmf_iter_update_H': (_c.c_int, [_ctx_p]),
    'klnmf_iter_advance': (_c.c_int, [_ctx_p]),
    'klnmf_loop_end': (_c.c_int, [_ctx_p, _c.POINTER(_c.c_double), _c.POINTER(_i64),
                                  _c.POINTER(_c.c_int)]),
    'klnmf_comm_unique_id': (_c.c_int, [_c.c_void_p]),
    'klnmf_comm_init': (_c.c_int, [_ctx_p, _c.c_void_p, _c.c_int, _c.c_int]),
    'klnmf_comm_destroy': (_c.c_int, [_ctx_p]),
    'klnmf_comm_max': (_c.c_int, [_ctx_p, _c.POINTER(_c.c_double)]),
    'klnmf_run_sharded': (_c.c_int, [_ctx_p, _i64, _i64, _c.c_int, _c.c_double,
                                     _c.POINTER(_c.c_double), _c.POINTER(_i64), _c.POINTER(_c.c_int)]),
    'klnmf_exchange_buffers': (_c.c_int, [_ctx_p, _c.POINTER(_c.c_void_p),
                                          _c.POINTER(_c.c_void_p), _c.POINTER(_i64),
                                          _c.POINTER(_c.c_int)]),
    'klnmf_exchange_layout': (_c.c_int, [_ctx_p, _c.POINTER(_i64), _c.POINTER(_i64)]),
    'klnmf_bind_exchange': (_c.c_int, [_ctx_p, _c.c_void_p, _c.c_void_p]),
    'klnmf_group_create': (_c.c_int, [_c.POINTER(_c.c_void_p), _c.POINTER(_ctx_p), _c.c_int]),
    'klnmf_group_run': (_c.c_int, [_c.c_void_p, _i64, _i64, _c.c_int, _c.c_double,
                                   _c.POINTER(_c.c_double), _c.POINTER(_i64), _c.POINTER(_c.c_int)]),
    'klnmf_group_destroy': (_c.c_int, [_c.c_void_p]),
    'klnmf_group_enqueue_time': (_c.c_int, [_c.c_void_p, _c.POINTER(_i64), _c.POINTER(_c.c_double), _c.POINTER(_c.c_double)]),
    'klnmf_group_selftest': (_c.c_int, [_c.POINTER(_c.c_int), _c.c_int, _i64, _c.c_int, _c.POINTER(_c.c_int)]),
    'klnmf_error': (_c.c_int, [_ctx_p, _c.POINTER(_c.c_double)]),
    'klnmf_loss_terms': (_c.c_int, [_ctx_p, _c.POINTER(_c.c_double)]),
    'klnmf_update': (_c.c_int, [_ctx_p, _c.c_int]),
    'klnmf_set_ratio_eps': (_c.c_int, [_ctx_p, _c.c_double]),
    'klnmf_step_Q': (_c.c_int, [_ctx_p]),
    'klnmf_step_W': (_c.c_int, [_ctx_p]),
    'klnmf_step_H': (_c.c_int, [_ctx_p]),
    'klnmf_generalized_kl': (_c.c_int, [_ctx_p, _c.c_void_p, _c.c_void_p, _c.c_int, _i64,
                                        _c.c_double, _c.POINTER(_c.c_double)]),
    'klnmf_get_W': (_c.c_int, [_ctx_p, _c.c_void_p, _c.c_int]),
    'klnmf_get_H': (_c.c_int, [_ctx_p, _c.c_void_p, _c.c_int]),
    'klnmf_get_Q': (_c.c_int, [_ctx_p, _c.c_void_p, _c.c_int]),
    'klnmf_profile_enable': (_c.c_int, [_ctx_p, _c.c_int]),
    'klnmf_profile_read': (_c.c_int, [_ctx_p, _c.POINTER(_i64), _c.POINTER(_c.c_double),
                                      _c.POINTER(_i64), _c.POINTER(_c.c_double), _c.c_int]),
    'klnmf_profile_read_tail': (_c.c_int, [_ctx_p, _c.POINTER(_i64), _c.POINTER(_c.c_double), _c.POINTER(_i64), _c.c_int]),
    'klnmf_synchronize': (_c.c_int, [_ctx_p]),
    'klnmf_query': (_c.c_int, [_ctx_p, _c.c_int, _c.POINTER(_i64)]),
    'klnmf_plan_query': (_c.c_int, [_c.c_int, _i64, _i64, _i64, _i64, _c.c_int, _c.c_int, _c.POINTER(_i64)]),
    'klnmf_set_H_device': (_c.c_int, [_ctx_p, _c.c_void_p, _c.c_int, _i64, _i64, _i64, _c.c_int]),
    'klnmf_get_W_device': (_c.c_int, [_ctx_p, _c.c_void_p, _c.c_int, _i64]),
    'klnmf_upload_V_device_rows_dt': (_c.c_int, [_ctx_p, _c.c_void_p, _c.c_int, _c.c_void_p, _i64, _i64, _i64, _i64, _i64,
                                                 _c.c_double]),
    'klnmf_matmul_device': (_c.c_int, [_c.c_int, _c.c_int, _i64, _i64, _i64, _c.c_void_p, _i64, _c.c_void_p, _i64,
                                       _c.c_void_p, _i64]),
    'klnmf_all_distances_device': (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _i64, _i64, _i64, _c.c_void_p, _i64,
                                              _c.c_void_p, _i64, _c.c_void_p]),
    'klnmf_query_f64': (_c.c_int, [_ctx_p, _c.c_int, _c.POINTER(_c.c_double)]),
    'klnmf_set_problem_sparse': (_c.c_int, [_ctx_p, _i64, _i64, _i64, _i64, _i64]),
    'klnmf_upload_csr': (_c.c_int, [_ctx_p, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                    _c.c_void_p, _c.c_void_p]),
    'klnmf_upload_csr_rows': (_c.c_int, [_ctx_p, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    'klnmf_get_Q_values': (_c.c_int, [_ctx_p, _c.c_void_p, _c.c_int]),
    'klnmf_upload_csr_device_rows': (_c.c_int, [_ctx_p, _c.c_int, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_void_p),
                                                _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_int), _c.POINTER(_i64),
                                                _c.POINTER(_c.c_double), _i64, _c.c_void_p, _i64]),
    'klnmf_csr_rows_to_dense_device': (_c.c_int, [_c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _i64, _c.c_void_p,
                                                  _i64, _i64, _c.c_void_p, _i64]),
    'klnmf_matmul': (_c.c_int, [_c.c_int, _c.c_int, _i64, _i64, _i64, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    'klnmf_all_distances': (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _i64, _i64, _i64, _c.c_void_p, _c.c_void_p,
                                       _c.c_void_p]),
    'klnmf_selftest': (_c.c_int, [_c.c_int, _c.POINTER(_c.c_int)]),
}

# name -> (restype, argtypes): every symbol of include/klnmf_batch.h (batches: B problems of one shape in one launch sequence)
BATCH_SIGNATURES = {
    'klnmf_batch_create': (_c.c_int, [_c.POINTER(_c.c_void_p), _c.c_int, _c.c_int, _c.c_int]),
    'klnmf_batch_destroy': (_c.c_int, [_c.c_void_p]),
    'klnmf_batch_set_problem': (_c.c_int, [_c.c_void_p, _i64, _i64, _i64, _i64]),
    'klnmf_batch_upload_V': (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _i64, _i64, _i64, _i64, _i64, _c.c_double]),
    'klnmf_batch_upload_V_device_rows_dt': (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p, _i64, _i64, _i64,
                                                       _i64, _i64, _c.c_double]),
    'klnmf_batch_set_H': (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int]),
    'klnmf_batch_set_H_device': (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _i64, _i64, _i64, _c.c_int]),
    'klnmf_batch_set_W': (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int]),
    'klnmf_batch_init_W': (_c.c_int, [_c.c_void_p]),
    'klnmf_batch_run': (_c.c_int, [_c.c_void_p, _i64, _c.c_int, _c.c_double]),
    'klnmf_batch_result': (_c.c_int, [_c.c_void_p, _c.c_int, _c.POINTER(_c.c_double), _c.POINTER(_i64), _c.POINTER(_c.c_int)]),
    'klnmf_batch_get_W': (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int]),
    'klnmf_batch_get_H': (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int]),
    'klnmf_batch_get_W_device': (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _i64]),
    'klnmf_batch_query': (_c.c_int, [_c.c_void_p, _c.c_int, _c.POINTER(_i64)]),
}

# name -> (restype, argtypes): every symbol of include/klnmf_batch_mask.h (presence masks on batches)
BATCH_MASK_SIGNATURES = {
    'klnmf_batch_upload_presence': (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _i64, _i64, _i64, _c.POINTER(_i64),
                                               _c.c_int]),
    'klnmf_batch_upload_presence_device_rows': (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _i64, _i64, _c.c_void_p, _i64,
                                                           _i64, _c.POINTER(_c.c_int), _c.POINTER(_i64), _c.c_int]),
    'klnmf_batch_clear_presence': (_c.c_int, [_c.c_void_p]),
}

# name -> (restype, argtypes): every symbol of include/klnmf_batch_csr.h (CSR problems on batches)
BATCH_CSR_SIGNATURES = {
    'klnmf_batch_set_problem_sparse': (_c.c_int, [_c.c_void_p, _i64, _i64, _i64, _i64, _c.POINTER(_i64)]),
    'klnmf_batch_upload_csr_rows': (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    'klnmf_batch_upload_csr_device_rows': (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_void_p),
                                                      _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_int), _c.POINTER(_i64),
                                                      _c.POINTER(_c.c_double), _i64, _c.c_void_p, _i64]),
}

# name -> (restype, argtypes): every symbol of include/klnmf_beta.h (the beta-divergence cost on a context)
BETA_SIGNATURES = {
    'klnmf_set_divergence': (_c.c_int, [_ctx_p, _c.c_double]),
    'klnmf_get_divergence': (_c.c_int, [_ctx_p, _c.POINTER(_c.c_double)]),
    'klnmf_beta_loss': (_c.c_int, [_ctx_p, _c.POINTER(_c.c_double)]),
    'klnmf_beta_step': (_c.c_int, [_ctx_p, _c.c_int]),
}

# name -> (restype, argtypes): every symbol of include/klnmf_batch_beta.h (the beta-divergence cost on batches)
BATCH_BETA_SIGNATURES = {
    'klnmf_batch_set_divergence': (_c.c_int, [_c.c_void_p, _c.c_double]),
    'klnmf_batch_get_divergence': (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_double)]),
    'klnmf_batch_upload_weights': (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _i64, _i64, _i64, _i64, _i64]),
}

# name -> (restype, argtypes): every symbol of include/klnmf_nearest.h (the fused nearest-example search)
NEAREST_SIGNATURES = {
    'klnmf_nearest_work_bytes': (_c.c_int, [_i64, _i64, _c.POINTER(_c.c_uint64)]),
    'klnmf_nearest_many_device': (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _i64, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                             _c.c_uint64]),
    'klnmf_nearest': (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _i64, _i64, _i64, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
}

# name -> (restype, argtypes): every symbol of include/klnmf_information.h (the atom x label information matrix)
INFORMATION_SIGNATURES = {
    'klnmf_information_work_bytes': (_c.c_int, [_i64, _i64, _c.c_int, _c.c_int, _c.POINTER(_c.c_uint64)]),
    'klnmf_information_many_device': (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _i64, _c.c_void_p, _c.c_void_p,
                                                 _c.c_void_p, _c.c_uint64]),
    'klnmf_information': (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _i64, _i64, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                     _c.c_void_p]),
}

# name -> (restype, argtypes): every symbol of include/klnmf_hac.h (the windowed co-occurrence histograms)
HAC_SIGNATURES = {
    'klnmf_hac_work_bytes': (_c.c_int, [_c.c_int, _i64, _c.c_int, _i64, _c.POINTER(_c.c_uint64)]),
    'klnmf_hac_count_device': (_c.c_int, [_c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _i64, _c.c_void_p, _c.c_int, _c.c_void_p, _i64,
                                          _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.POINTER(_i64)]),
    'klnmf_hac_fill_device': (_c.c_int, [_c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _i64, _c.c_void_p, _c.c_int, _c.c_void_p, _i64,
                                         _c.c_void_p, _c.c_uint64, _i64, _c.c_void_p, _c.c_void_p]),
    'klnmf_hac': (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _i64, _c.c_void_p, _c.c_int, _c.c_void_p, _i64,
                             _c.c_void_p, _i64, _c.c_void_p, _c.c_void_p, _c.POINTER(_i64)]),
}

# name -> (restype, argtypes): every symbol of include/klnmf_kmeans.h (the codebook builders' device half)
KMEANS_SIGNATURES = {
    'klnmf_kmeans_work_bytes': (_c.c_int, [_i64, _i64, _i64, _c.POINTER(_c.c_uint64)]),
    'klnmf_kmeans_device': (_c.c_int, [_c.c_int, _c.c_int, _c.c_void_p, _i64, _i64, _i64, _c.c_void_p, _i64, _i64, _c.c_int,
                                       _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p]),
    'klnmf_kmeans_gram_device': (_c.c_int, [_c.c_int, _c.c_int, _c.c_void_p, _i64, _i64, _i64, _c.c_void_p, _i64, _c.c_void_p,
                                            _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.POINTER(_i64)]),
    'klnmf_kmeans': (_c.c_int, [_c.c_int, _c.c_int, _c.c_void_p, _i64, _i64, _i64, _c.c_void_p, _i64, _i64, _c.c_int, _c.c_void_p,
                                _c.c_void_p]),
}

# name -> (restype, argtypes): every symbol of include/klnmf_motion.h (the motion modality's device half)
MOTION_SIGNATURES = {
    'klnmf_motion_work_bytes': (_c.c_int, [_i64, _i64, _i64, _i64, _i64, _i64, _i64, _c.POINTER(_c.c_uint64)]),
    'klnmf_motion_angles_device': (_c.c_int, [_c.c_int, _c.c_int, _c.c_void_p, _i64, _i64, _c.c_void_p, _i64, _c.c_void_p, _i64, _i64,
                                              _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _i64,
                                              _c.c_void_p, _i64]),
    'klnmf_motion_whiten_device': (_c.c_int, [_c.c_int, _c.c_int, _c.c_void_p, _i64, _i64, _i64, _c.c_void_p, _c.c_uint64, _c.c_void_p,
                                              _i64, _c.c_void_p, _c.c_void_p]),
    'klnmf_motion_kmeans_device': (_c.c_int, [_c.c_int, _c.c_int, _c.c_void_p, _i64, _i64, _i64, _i64, _i64, _c.c_void_p, _i64,
                                              _c.c_void_p, _i64, _c.c_double, _c.c_int, _c.c_void_p, _c.c_uint64, _c.c_void_p,
                                              _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.POINTER(_c.c_int)]),
    'klnmf_motion_hist_device': (_c.c_int, [_c.c_int, _c.c_int, _c.c_void_p, _i64, _i64, _i64, _i64, _i64, _c.c_void_p, _i64,
                                            _c.c_void_p, _i64, _c.c_int, _c.c_double, _c.c_void_p, _c.c_uint64, _c.c_void_p, _i64]),
}

# name -> (restype, argtypes): every symbol of include/features/klnmf_mfcc.h (the MFCC front end of the sound modality)
MFCC_SIGNATURES = {
    'klnmf_mfcc_work_bytes': (_c.c_int, [_i64, _i64, _i64, _i64, _i64, _i64, _c.POINTER(_c.c_uint64)]),
    'klnmf_mfcc_mel_device': (_c.c_int, [_c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _i64, _i64, _i64, _c.c_int, _c.c_void_p,
                                         _c.c_void_p, _i64, _i64, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p]),
    'klnmf_mfcc_cepstra_device': (_c.c_int, [_c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _i64, _i64,
                                             _c.c_void_p, _i64,
                                             _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_void_p, _i64]),
    'klnmf_mfcc': (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _i64, _i64, _i64, _c.c_int, _c.c_void_p,
                              _c.c_void_p, _i64, _c.c_void_p, _c.c_void_p, _i64, _i64, _c.c_void_p, _c.c_void_p, _c.c_void_p, _i64]),
}

# (header under include/, its table) in the order the headers came: load() binds every table, and the tests hold each table against
# its header's declarations and all of them pairwise disjoint.  A new header adds its table above and one line here.
HEADER_TABLES = (
    ('klnmf.h', SIGNATURES), ('klnmf_batch.h', BATCH_SIGNATURES), ('klnmf_batch_mask.h', BATCH_MASK_SIGNATURES),
    ('klnmf_batch_csr.h', BATCH_CSR_SIGNATURES), ('klnmf_beta.h', BETA_SIGNATURES), ('klnmf_batch_beta.h', BATCH_BETA_SIGNATURES),
    ('klnmf_nearest.h', NEAREST_SIGNATURES), ('klnmf_information.h', INFORMATION_SIGNATURES), ('klnmf_hac.h', HAC_SIGNATURES),
    ('klnmf_kmeans.h', KMEANS_SIGNATURES), ('klnmf_motion.h', MOTION_SIGNATURES))

# The headers of the feature front ends, under include/features/, with their tables: a registry of its own, bound by load() after
# HEADER_TABLES.  HEADER_TABLES stays the closed list of the headers directly under include/ -- tests/test_batch_csr_cpu.py holds it
# against that directory's listing and against the number of exports each of them had, so a header added there would change what
# an existing test asserts.  A new feature header adds its table above and one line here.
FEATURE_HEADER_TABLES = (
    ('features/klnmf_mfcc.h', MFCC_SIGNATURES),)

_lib = None


class NativeError(RuntimeError):
    """A non-zero status from the C-ABI."""

    def __init__(self, code, msg):
        RuntimeError.__init__(self, "klnmf error %d: %s" % (code, msg))
        self.code = code


def load():
    """Load libklnmf.so and declare every entry point.  Raises if it is absent:
    the product path has no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "HIP extension %s is missing; build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for _, table in HEADER_TABLES + FEATURE_HEADER_TABLES:
        for name, (res, args) in table.items():
            fn = getattr(lib, name)     # AttributeError if a symbol is not exported
            fn.restype = res
            fn.argtypes = args
    _lib = lib
    return lib


def csr_canonical(X):
    """X as the CSR uploads take it: a scipy CSR copy without explicit zeros, indices sorted (nmf.py:66 does the same)."""
    import scipy.sparse as sp
    X = sp.csr_matrix(X, copy=True)
    X.eliminate_zeros()
    X.sort_indices()
    return X


def _check(status):
    if status != 0:
        msg = load().klnmf_last_error()
        msg = msg.decode('utf-8', 'replace') if msg else ''
        if status == ERR_ALLOC:
            raise MemoryError("klnmf: " + msg)
        raise NativeError(status, msg)


def _np_dtype_code(a):
    if a.dtype == np.float64:
        return DT_F64
    if a.dtype == np.float32:
        return DT_F32
    raise TypeError("expected float32/float64, got %s" % a.dtype)


def _work_bytes(entry, *sizes):
    """What a klnmf_*_work_bytes entry point answers for these sizes (host arithmetic: no device is touched)."""
    out = _c.c_uint64(0)
    _check(getattr(load(), entry)(*([int(v) for v in sizes] + [_c.byref(out)])))
    return out.value


def _job_table(struct, rows, at_least=1):
    """A ctypes array of `struct` filled from tuples in the order of its fields -- a pointer that is 0 becomes NULL, everything
    else an int -- as a void pointer; never an array of no element, so that the pointer is not NULL either."""
    rows = list(rows)
    table = (struct * max(1, at_least, len(rows)))()
    for q, row in enumerate(rows):
        table[q] = struct(*[(v or None) if t is _c.c_void_p else int(v) for (_, t), v in zip(struct._fields_, row)])
    return _c.cast(table, _c.c_void_p)


def _as_float_array(a):
    """C-contiguous float32/float64 view or copy of a (ints -> float64)."""
    a = np.asarray(a)
    if a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float64)
    return np.ascontiguousarray(a)


def device_info(device=0):
    lib = load()
    arch = ctypes.create_string_buffer(64)
    cu = _c.c_int(0)
    mem = _c.c_uint64(0)
    _check(lib.klnmf_device_info(device, arch, 64, ctypes.byref(cu), ctypes.byref(mem)))
    return {'arch': arch.value.decode(), 'cu_count': cu.value, 'hbm_bytes': mem.value}


def matmul(A, B, device=0):
    """A.dot(B) on the GPU (klnmf_matmul): float32 if both operands are float32,
    float64 otherwise -- the reconstruction product of learner.py:80-84."""
    A = np.asarray(A)
    B = np.asarray(B)
    if A.ndim != 2 or B.ndim != 2 or A.shape[1] != B.shape[0]:
        raise ValueError('shapes %s and %s not aligned' % (A.shape, B.shape))
    dt = np.float32 if (A.dtype == np.float32 and B.dtype == np.float32) else np.float64
    A = np.ascontiguousarray(A, dtype=dt)
    B = np.ascontiguousarray(B, dtype=dt)
    C = np.empty((A.shape[0], B.shape[1]), dtype=dt)
    lib = load()
    _check(lib.klnmf_matmul(device, _dt_code(dt != np.float32), A.shape[0], B.shape[1], A.shape[1],
                            A.ctypes.data_as(_c.c_void_p), B.ctypes.data_as(_c.c_void_p),
                            C.ctypes.data_as(_c.c_void_p)))
    return C


DIST_KL, DIST_REV_KL, DIST_SYM_KL, DIST_FROBENIUS, DIST_COSINE_DIFF = 0, 1, 2, 3, 4


def all_distances(A, B, metric, device=0):
    """[len(A), len(B)] matrix of metric(A[i], B[j]) on the GPU (klnmf_all_distances)."""
    A = np.asarray(A)
    B = np.asarray(B)
    if A.ndim != 2 or B.ndim != 2 or A.shape[1] != B.shape[1]:
        raise ValueError('shapes %s and %s do not hold vectors of one length' % (A.shape, B.shape))
    dt = np.float32 if (A.dtype == np.float32 and B.dtype == np.float32) else np.float64
    A = np.ascontiguousarray(A, dtype=dt)
    B = np.ascontiguousarray(B, dtype=dt)
    out = np.empty((A.shape[0], B.shape[0]), dtype=dt)
    lib = load()
    _check(lib.klnmf_all_distances(device, _dt_code(dt != np.float32), int(metric), A.shape[0],
                                   B.shape[0], A.shape[1], A.ctypes.data_as(_c.c_void_p),
                                   B.ctypes.data_as(_c.c_void_p), out.ctypes.data_as(_c.c_void_p)))
    return out


def matmul_device(dA, lda, dB, ldb, dC, ldc, m, n, kk, f64=True, device=0):
    """C[m, n] = A[m, kk] . B[kk, n] between DEVICE matrices (pointers, row strides in elements): klnmf_matmul_device."""
    _check(load().klnmf_matmul_device(device, _dt_code(f64), int(m), int(n), int(kk), _c.c_void_p(dA), int(lda),
                                      _c.c_void_p(dB), int(ldb), _c.c_void_p(dC), int(ldc)))


def all_distances_device(dA, lda, dB, ldb, dout, na, nb, d, metric, f64=True, device=0):
    """out[na, nb] = metric(A[i], B[j]) between DEVICE matrices: klnmf_all_distances_device."""
    _check(load().klnmf_all_distances_device(device, _dt_code(f64), int(metric), int(na), int(nb), int(d),
                                             _c.c_void_p(dA), int(lda), _c.c_void_p(dB), int(ldb), _c.c_void_p(dout)))


DIST_MASK_ALL = 31
NEAREST_MAX_JOBS = 1 << 20


class NearestJob(_c.Structure):
    """klnmf_nearest_job: A [na, d] against B [nb, d], device pointers, row strides in elements."""
    _fields_ = [('A', _c.c_void_p), ('lda', _i64), ('B', _c.c_void_p), ('ldb', _i64), ('na', _i64), ('nb', _i64), ('d', _i64)]


def metric_mask(metrics):
    """The bit mask of the measures DIST_* in `metrics` (bit i = measure i)."""
    mask = 0
    for m in metrics:
        mask |= 1 << int(m)
    return mask


def mask_metrics(mask):
    """The measures of a mask in the order of a result row: ascending."""
    return [m for m in range(5) if int(mask) >> m & 1]


def nearest_work_bytes(count, total_rows):
    """Bytes of device workspace `nearest_many_device` needs for `count` jobs of `total_rows` rows: klnmf_nearest_work_bytes."""
    return _work_bytes('klnmf_nearest_work_bytes', count, total_rows)


def nearest_many_device(jobs, mask, d_idx, d_dist, d_work, work_bytes, f64=True, device=0):
    """For every job (dA, lda, dB, ldb, na, nb, d) of DEVICE matrices and every row of its A: the index of the nearest row of B
    under each measure of `mask`, int32 [sum na][M] at d_idx (and the distances at d_dist, or None) -- one launch:
    klnmf_nearest_many_device."""
    jobs = list(jobs)
    _check(load().klnmf_nearest_many_device(device, _dt_code(f64), int(mask), _job_table(NearestJob, jobs), len(jobs),
                                            _c.c_void_p(d_idx), _c.c_void_p(d_dist), _c.c_void_p(d_work), int(work_bytes)))


def nearest(A, B, mask, device=0, return_distances=False):
    """[len(A), M] int32 indices of the nearest row of B for every row of A under each measure of `mask` (ascending) -- and the
    distances with return_distances -- from host arrays: klnmf_nearest."""
    A = np.asarray(A)
    B = np.asarray(B)
    if A.ndim != 2 or B.ndim != 2 or A.shape[1] != B.shape[1]:
        raise ValueError('shapes %s and %s do not hold vectors of one length' % (A.shape, B.shape))
    dt = np.float32 if (A.dtype == np.float32 and B.dtype == np.float32) else np.float64
    A = np.ascontiguousarray(A, dtype=dt)
    B = np.ascontiguousarray(B, dtype=dt)
    M = len(mask_metrics(mask)) if 0 < int(mask) <= DIST_MASK_ALL else 1
    idx = np.empty((A.shape[0], M), dtype=np.int32)
    dist = np.empty((A.shape[0], M), dtype=dt) if return_distances else None
    _check(load().klnmf_nearest(device, _dt_code(dt != np.float32), int(mask), A.shape[0], B.shape[0], A.shape[1],
                                A.ctypes.data_as(_c.c_void_p), B.ctypes.data_as(_c.c_void_p), idx.ctypes.data_as(_c.c_void_p),
                                dist.ctypes.data_as(_c.c_void_p) if return_distances else None))
    return (idx, dist) if return_distances else idx


INFORMATION_LDS_BYTES = 32768      # KLNMF_INFORMATION_LDS_BYTES
INFORMATION_ROWS = 1024            # rows of a workgroup's chunk (csrc/information.hip.h, kInfoRows)


class InformationJob(_c.Structure):
    """klnmf_information_job: A [n, k] (device pointer, rows lda elements apart) and its int32 labels [n]."""
    _fields_ = [('A', _c.c_void_p), ('lda', _i64), ('labels', _c.c_void_p), ('n', _i64), ('k', _i64)]


def information_route(n_labels, bins):
    """(route, atom tile) of the histogram launch for (n_labels, bins) -- include/klnmf_information.h's rule: 'lds' with the full
    tile of 64 atoms, 'lds-shrunk' with fewer, 'global' (tile 0) where not one atom's counters fit the LDS budget."""
    tile = min(64, INFORMATION_LDS_BYTES // (4 * int(n_labels) * int(bins)))
    return ('lds' if tile == 64 else 'lds-shrunk' if tile > 0 else 'global'), tile


def information_work_bytes(count, total_atoms, n_labels, bins):
    """Bytes of device workspace `information_many_device` needs for `count` jobs of `total_atoms` atoms in all:
    klnmf_information_work_bytes."""
    return _work_bytes('klnmf_information_work_bytes', count, total_atoms, n_labels, bins)


def information_many_device(jobs, n_labels, bins, d_info, d_counts, d_work, work_bytes, f64=True, device=0):
    """For every job (dA, lda, d_labels, n, k) of DEVICE arrays: the (n_labels, k) information matrix, float64, at d_info behind the
    jobs before it (and the int32 counts [k][n_labels][bins] at d_counts, or None) -- a fixed number of launches for all jobs:
    klnmf_information_many_device."""
    jobs = list(jobs)
    _check(load().klnmf_information_many_device(device, _dt_code(f64), int(n_labels), int(bins), _job_table(InformationJob, jobs),
                                                len(jobs), _c.c_void_p(d_info), _c.c_void_p(d_counts), _c.c_void_p(d_work),
                                                int(work_bytes)))


def information(A, labels, n_labels, bins=10, device=0, return_counts=False):
    """The (n_labels, k) float64 information matrix of the host matrix A [n, k] (float32 stays float32, anything else runs as
    float64) and its int32 labels -- and the counts [k, n_labels, bins] with return_counts: klnmf_information."""
    A = np.asarray(A)
    if A.ndim != 2:
        raise ValueError('a matrix [n, k] of coefficients, got shape %s' % (A.shape,))
    dt = np.float32 if A.dtype == np.float32 else np.float64
    A = np.ascontiguousarray(A, dtype=dt)
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    if labels.shape != (A.shape[0],):
        raise ValueError('one label per row: %s labels for %d rows' % (labels.shape, A.shape[0]))
    n, k = A.shape
    shape_ok = n >= 1 and k >= 1 and 1 <= int(n_labels) <= 65536 and 1 <= int(bins) <= 256
    info = np.empty((int(n_labels), k) if shape_ok else (1, 1), dtype=np.float64)
    counts = np.empty((k, int(n_labels), int(bins)) if shape_ok else (1, 1, 1), dtype=np.int32) if return_counts else None
    _check(load().klnmf_information(device, _dt_code(dt != np.float32), int(n_labels), int(bins), n, k,
                                    A.ctypes.data_as(_c.c_void_p), labels.ctypes.data_as(_c.c_void_p),
                                    info.ctypes.data_as(_c.c_void_p),
                                    counts.ctypes.data_as(_c.c_void_p) if return_counts else None))
    return (info, counts) if return_counts else info


HAC_MAX_STREAMS, HAC_MAX_LAGS = 8, 8     # KLNMF_HAC_MAX_STREAMS, KLNMF_HAC_MAX_LAGS
HAC_SORT_MAX = 4096                      # KLNMF_HAC_SORT_MAX: pair codes of a segment the sort route takes
HAC_DENSE_MAX_K = 192                    # KLNMF_HAC_DENSE_MAX_K: codebook units of the dense route (K^2 int32 counters in LDS)


class HacStream(_c.Structure):
    """klnmf_hac_stream: frames [T, d] and a codebook [K, d], pointers, row strides in elements."""
    _fields_ = [('frames', _c.c_void_p), ('ld', _i64), ('codebook', _c.c_void_p), ('ldc', _i64), ('d', _i64), ('K', _i64)]


def hac_route(n_codes, K):
    """The route of a segment of `n_codes` pair codes over a codebook of K units -- include/klnmf_hac.h's rule: 'none' (no code:
    the window is no longer than the lag), 'sort' up to HAC_SORT_MAX codes, beyond that 'dense' up to HAC_DENSE_MAX_K units and
    'refused' (KLNMF_ERR_UNSUPP) above."""
    if int(n_codes) <= 0:
        return 'none'
    if int(n_codes) <= HAC_SORT_MAX:
        return 'sort'
    return 'dense' if int(K) <= HAC_DENSE_MAX_K else 'refused'


def hac_work_bytes(n_streams, T, n_lags, n_windows):
    """Bytes of device workspace a `hac_count_device` / `hac_fill_device` pair needs: klnmf_hac_work_bytes."""
    return _work_bytes('klnmf_hac_work_bytes', n_streams, T, n_lags, n_windows)


def _hac_host_args(lags, windows):
    lags = np.ascontiguousarray(lags, dtype=np.int32).reshape(-1)
    windows = np.ascontiguousarray(windows, dtype=np.int64).reshape(-1, 2)
    return lags, windows


def hac_count_device(streams, T, lags, windows, d_work, work_bytes, d_indptr, f64=True, device=0):
    """Quantises the streams (d_frames, ld, d_codebook, ldc, d, K) of DEVICE matrices with T frames each, counts and scans: the
    int64 row pointers [len(windows) + 1] at d_indptr; returns nnz -- klnmf_hac_count_device.  `lags`, `windows` [(t0, t1) ...]:
    host."""
    streams = list(streams)
    lags, windows = _hac_host_args(lags, windows)
    nnz = _i64(-1)
    _check(load().klnmf_hac_count_device(device, _dt_code(f64), _job_table(HacStream, streams), len(streams), int(T),
                                         lags.ctypes.data_as(_c.c_void_p), len(lags), windows.ctypes.data_as(_c.c_void_p),
                                         len(windows), _c.c_void_p(d_work), int(work_bytes), _c.c_void_p(d_indptr), _c.byref(nnz)))
    return int(nnz.value)


def hac_fill_device(Ks, T, lags, windows, d_work, work_bytes, nnz, d_indices, d_values, f64=True, device=0):
    """The int32 column indices at d_indices and the counts (float64, or float32 with f64=False) at d_values of the matrix the
    preceding `hac_count_device` call on the same arguments and workspace measured: klnmf_hac_fill_device."""
    Ks = np.ascontiguousarray(Ks, dtype=np.int64).reshape(-1)
    lags, windows = _hac_host_args(lags, windows)
    _check(load().klnmf_hac_fill_device(device, _dt_code(f64), Ks.ctypes.data_as(_c.c_void_p), len(Ks), int(T),
                                        lags.ctypes.data_as(_c.c_void_p), len(lags), windows.ctypes.data_as(_c.c_void_p),
                                        len(windows), _c.c_void_p(d_work), int(work_bytes), int(nnz), _c.c_void_p(d_indices),
                                        _c.c_void_p(d_values)))


def hac(streams, codebooks, lags, windows, dtype=np.float64, device=0):
    """(indptr int64, indices int32, values `dtype`) of the windowed co-occurrence CSR matrix of HOST streams [T, d_s] and
    codebooks [K_s, d_s] (float32 if all are float32, float64 otherwise): klnmf_hac."""
    f32 = all(np.asarray(a).dtype == np.float32 for a in list(streams) + list(codebooks))
    dt = np.float32 if f32 else np.float64
    streams = [np.ascontiguousarray(x, dtype=dt) for x in streams]
    codebooks = [np.ascontiguousarray(c, dtype=dt) for c in codebooks]
    vdt = np.dtype(dtype)
    if vdt not in (np.float32, np.float64):
        raise TypeError("values are float32 or float64, got %s" % vdt)
    lags, windows = _hac_host_args(lags, windows)
    T = streams[0].shape[0] if streams else 0
    table = _job_table(HacStream, [(x.ctypes.data, x.shape[1], c.ctypes.data, c.shape[1], x.shape[1], c.shape[0])
                                   for x, c in zip(streams, codebooks)], at_least=len(streams))
    # (an upper bound of nnz from the windows alone: a segment stores at most min(n_codes, K^2) entries)
    length = (windows[:, 1] - windows[:, 0]) if len(windows) else np.zeros(0, dtype=np.int64)
    capacity = 0
    for c in codebooks:
        for lag in lags:
            capacity += int(np.minimum(np.maximum(length - int(lag), 0), c.shape[0] ** 2).sum())
    indptr = np.zeros(len(windows) + 1, dtype=np.int64)
    indices = np.empty(max(1, capacity), dtype=np.int32)
    values = np.empty(max(1, capacity), dtype=vdt)
    nnz = _i64(-1)
    p = lambda a: a.ctypes.data_as(_c.c_void_p)
    _check(load().klnmf_hac(device, _dt_code(not f32), _dt_code(vdt != np.float32), table, len(streams), int(T), p(lags), len(lags),
                            p(windows), len(windows), p(indptr), capacity, p(indices), p(values), _c.byref(nnz)))
    return indptr, indices[:nnz.value].copy(), values[:nnz.value].copy()


MFCC_I16, MFCC_F32, MFCC_F64 = 0, 1, 2                         # KLNMF_MFCC_I16 / _F32 / _F64: the kinds of samples
MFCC_ROUTES = {'auto': 0, 'fft': 1, 'direct': 2}               # KLNMF_MFCC_ROUTE_*
MFCC_MAX_MELS = 4096                                           # KLNMF_MFCC_MAX_MELS
MFCC_SAMPLE_KINDS = {np.dtype(np.int16): MFCC_I16, np.dtype(np.float32): MFCC_F32, np.dtype(np.float64): MFCC_F64}


def mfcc_route(n_fft, route='auto'):
    """The route the transform of `n_fft` points takes -- include/features/klnmf_mfcc.h's rule: 'fft' for the powers of two in
    [64, 4096], 'direct' for the even sizes in [16, 1024], 'refused' (KLNMF_ERR_UNSUPP) for a size that fits neither or not the
    route asked for."""
    n = int(n_fft)
    fft = 64 <= n <= 4096 and n & (n - 1) == 0
    direct = 16 <= n <= 1024 and n % 2 == 0
    if route == 'fft':
        return 'fft' if fft else 'refused'
    if route == 'direct':
        return 'direct' if direct else 'refused'
    return 'fft' if fft else 'direct' if direct else 'refused'


def mfcc_work_bytes(n_utterances, total_samples, total_frames, n_fft, n_mels, n_mfcc):
    """Bytes of device workspace a `mfcc_mel_device` / `mfcc_cepstra_device` pair needs: klnmf_mfcc_work_bytes."""
    return _work_bytes('klnmf_mfcc_work_bytes', n_utterances, total_samples, total_frames, n_fft, n_mels, n_mfcc)


def _i64_array(a):
    a = np.ascontiguousarray(a, dtype=np.int64).reshape(-1)
    return a, a.ctypes.data_as(_c.c_void_p)


def mfcc_mel_device(d_samples, sample_kind, sample_offsets, n_fft, hop, d_window, d_mel, n_mels, total_frames, d_work, work_bytes,
                    d_S, d_Smax, route='auto', device=0):
    """Frames, window, transform, power and filter bank of the utterances [offsets[u], offsets[u + 1]) of the DEVICE samples: the
    fp64 energies [total_frames, n_mels] at d_S and the utterances' maxima at d_Smax -- klnmf_mfcc_mel_device."""
    off, off_p = _i64_array(sample_offsets)
    _check(load().klnmf_mfcc_mel_device(device, int(sample_kind), _ptr(d_samples), off_p, len(off) - 1, int(n_fft), int(hop),
                                        MFCC_ROUTES[route] if route in MFCC_ROUTES else int(route), _ptr(d_window), _ptr(d_mel),
                                        int(n_mels), int(total_frames), _ptr(d_work), int(work_bytes), _ptr(d_S), _ptr(d_Smax)))


def mfcc_cepstra_device(d_S, d_Smax, d_dct, d_dct_sums, n_mels, n_mfcc, frame_offsets, d_work, work_bytes, d_mfcc, d_delta1, d_delta2, ld,
                        f64=True, device=0):
    """Log, floor, DCT (d_dct_sums: the basis' exact row sums, fp64 [n_mfcc]) and the two deltas: the three streams [total_frames, n_mfcc] (float64, or float32 with f64=False), rows
    `ld` apart -- klnmf_mfcc_cepstra_device."""
    off, off_p = _i64_array(frame_offsets)
    _check(load().klnmf_mfcc_cepstra_device(device, _dt_code(f64), _ptr(d_S), _ptr(d_Smax), _ptr(d_dct), _ptr(d_dct_sums), int(n_mels), int(n_mfcc),
                                            off_p, len(off) - 1, _ptr(d_work), int(work_bytes), _ptr(d_mfcc), _ptr(d_delta1),
                                            _ptr(d_delta2), int(ld)))


def mfcc(samples, sample_offsets, n_fft, hop, window, mel, dct, dct_sums, dtype=np.float64, route='auto', device=0):
    """The three streams [total_frames, n_mfcc] of `dtype` from HOST arrays: samples (int16 / float32 / float64, the utterances one
    after the other), window [n_fft], mel [n_mels, n_fft // 2 + 1], dct [n_mfcc, n_mels], dct_sums [n_mfcc] -- klnmf_mfcc."""
    samples = np.ascontiguousarray(samples)
    if samples.dtype not in MFCC_SAMPLE_KINDS:
        raise TypeError("samples are int16, float32 or float64, got %s" % samples.dtype)
    odt = np.dtype(dtype)
    if odt not in (np.float32, np.float64):
        raise TypeError("streams are float32 or float64, got %s" % odt)
    off, off_p = _i64_array(sample_offsets)
    window = np.ascontiguousarray(window, dtype=np.float64)
    mel = np.ascontiguousarray(mel, dtype=np.float64)
    dct = np.ascontiguousarray(dct, dtype=np.float64)
    dct_sums = np.ascontiguousarray(dct_sums, dtype=np.float64).reshape(-1)
    if dct_sums.shape != (dct.shape[0],):
        raise ValueError('one row sum per row of the basis: %s for %d rows' % (dct_sums.shape, dct.shape[0]))
    T = int(sum(1 + int(L) // max(1, int(hop)) for L in np.diff(off)))
    n_mels, n_mfcc = mel.shape[0], dct.shape[0]
    outs = [np.empty((T, n_mfcc), dtype=odt) for _ in range(3)]
    p = lambda a: a.ctypes.data_as(_c.c_void_p)
    _check(load().klnmf_mfcc(device, MFCC_SAMPLE_KINDS[samples.dtype], _dt_code(odt != np.float32), p(samples), off_p, len(off) - 1,
                             int(n_fft), int(hop), MFCC_ROUTES[route], p(window), p(mel), n_mels, p(dct), p(dct_sums), n_mfcc, T, p(outs[0]),
                             p(outs[1]), p(outs[2]), n_mfcc))
    return outs


KMEANS_TILE, KMEANS_GROUP = 256, 4096    # KLNMF_KMEANS_TILE, KLNMF_KMEANS_GROUP: the group is the unit of the summation order
KMEANS_MAX_KD = 13312                    # KLNMF_KMEANS_MAX_KD: K * d of a Lloyd call (fp64 accumulators in LDS)
KMEANS_GRAM_MAX_D = 64                   # KLNMF_KMEANS_GRAM_MAX_D


def kmeans_work_bytes(T, d, K):
    """Bytes of device workspace a `kmeans_device` or `kmeans_gram_device` call needs: klnmf_kmeans_work_bytes."""
    return _work_bytes('klnmf_kmeans_work_bytes', T, d, K)


def kmeans_device(d_frames, ld, T, d, d_codebook, ldc, K, n_iter, d_work, work_bytes, d_labels, d_counts, f64=True, device=0):
    """`n_iter` Lloyd iterations on DEVICE frames [T, d] and a DEVICE codebook [K, d] (in/out), the int32 labels [T] and int64
    counts [K] of the last assignment at d_labels / d_counts; no synchronisation: klnmf_kmeans_device."""
    _check(load().klnmf_kmeans_device(device, _dt_code(f64), _ptr(d_frames), int(ld), int(T), int(d), _ptr(d_codebook), int(ldc),
                                      int(K), int(n_iter), _ptr(d_work), int(work_bytes), _ptr(d_labels), _ptr(d_counts)))


def kmeans_gram_device(d_frames, ld, T, d, d_labels, cluster, d_work, work_bytes, d_gram, d_colsum, f64=True, device=0):
    """The fp64 Gram matrix [d, d] at d_gram and column sums [d] at d_colsum of the DEVICE frames with label `cluster` (-1: of all
    frames); returns their number: klnmf_kmeans_gram_device."""
    count = _i64(-1)
    _check(load().klnmf_kmeans_gram_device(device, _dt_code(f64), _ptr(d_frames), int(ld), int(T), int(d), _ptr(d_labels),
                                           int(cluster), _ptr(d_work), int(work_bytes), _ptr(d_gram), _ptr(d_colsum),
                                           _c.byref(count)))
    return int(count.value)


def kmeans(frames, codebook, n_iter, device=0):
    """(codebook, labels int32, counts int64) after `n_iter` Lloyd iterations from HOST frames [T, d] and codebook [K, d]
    (float32 if both are float32, float64 otherwise): klnmf_kmeans."""
    f32 = np.asarray(frames).dtype == np.float32 and np.asarray(codebook).dtype == np.float32
    dt = np.float32 if f32 else np.float64
    frames = np.ascontiguousarray(frames, dtype=dt)
    codebook = np.array(codebook, dtype=dt, order='C')
    T, d = frames.shape
    K = codebook.shape[0]
    labels = np.zeros(max(1, T), dtype=np.int32)
    counts = np.zeros(max(1, K), dtype=np.int64)
    p = lambda a: a.ctypes.data_as(_c.c_void_p)
    _check(load().klnmf_kmeans(device, _dt_code(not f32), p(frames) if T else None, d, T, d, p(codebook), codebook.shape[1], K,
                               int(n_iter), p(labels), p(counts)))
    return codebook, labels[:T], counts[:K]


MOTION_TILE, MOTION_GROUP = 256, 4096    # KLNMF_MOTION_TILE, KLNMF_MOTION_GROUP: the group is the unit of the summation order
MOTION_MAX_K, MOTION_MAX_D, MOTION_MAX_KD = 256, 16, 1024    # KLNMF_MOTION_MAX_K, _MAX_D, _MAX_KD
MOTION_MAX_PAIRS, MOTION_MAX_P, MOTION_POLL = 32, 65535, 4   # KLNMF_MOTION_MAX_PAIRS, _MAX_P, _POLL
MOTION_PADDINGS = {'zeros': 0, 'circular': 1}                # KLNMF_MOTION_PAD_ZEROS, KLNMF_MOTION_PAD_CIRCULAR


def _host_array(a, dt):
    a = np.ascontiguousarray(a, dtype=dt)
    return a, a.ctypes.data_as(_c.c_void_p)


def _host_bounds(b):
    if b is None:
        return None, None
    return _host_array([float(b[0]), float(b[1])], np.float64)


def motion_work_bytes(T, C=0, d=1, K=1, P=0, D=1, E=0):
    """Bytes of device workspace a call of klnmf_motion.h on these sizes needs: klnmf_motion_work_bytes."""
    return _work_bytes('klnmf_motion_work_bytes', T, C, d, K, P, D, E)


def motion_angles_device(d_records, T, n_markers, pairs, offsets, delay, padding, bounds, vel_bounds, d_work, work_bytes, d_angles,
                         lda, d_vels, ldv, f64=True, device=0):
    """Angles and delayed velocities [T, 3 len(pairs)] of DEVICE records [T, n_markers, 7]; `pairs` and `offsets` (E + 1) are host
    sequences, `padding` a KLNMF_MOTION_PAD_* number, the bounds (min, max) or None: klnmf_motion_angles_device."""
    pairs, p_pairs = _host_array(pairs, np.int32)
    offsets, p_off = _host_array(offsets, np.int64)
    b, p_b = _host_bounds(bounds)
    vb, p_vb = _host_bounds(vel_bounds)
    _check(load().klnmf_motion_angles_device(device, _dt_code(f64), _ptr(d_records), int(T), int(n_markers), p_pairs, pairs.size //
                                             2, p_off, offsets.size - 1, int(delay), int(padding), p_b, p_vb, _ptr(d_work),
                                             int(work_bytes), _ptr(d_angles), int(lda), _ptr(d_vels), int(ldv)))


def motion_whiten_device(d_x, ld, T, C, d_work, work_bytes, d_out, ldo, d_mean, d_std, f64=True, device=0):
    """DEVICE out [T, C] = x / std per column, the fp64 means and deviations at d_mean / d_std: klnmf_motion_whiten_device."""
    _check(load().klnmf_motion_whiten_device(device, _dt_code(f64), _ptr(d_x), int(ld), int(T), int(C), _ptr(d_work),
                                             int(work_bytes), _ptr(d_out), int(ldo), _ptr(d_mean), _ptr(d_std)))


def motion_kmeans_device(d_points, set_stride, ld, T, d, D, set_of, d_codebooks, K, thresh, max_iter, d_work, work_bytes, d_alive,
                         d_distortion, d_iters, d_labels=0, f64=True, device=0):
    """len(set_of) k-means problems to convergence on DEVICE point sets and codebooks [P, K, d] (in/out); returns -1, or the lowest
    problem that had not stopped after max_iter iterations: klnmf_motion_kmeans_device."""
    set_of, p_set = _host_array(set_of, np.int32)
    unfinished = _c.c_int(-2)
    _check(load().klnmf_motion_kmeans_device(device, _dt_code(f64), _ptr(d_points), int(set_stride), int(ld), int(T), int(d),
                                             int(D), p_set, set_of.size, _ptr(d_codebooks), int(K), float(thresh), int(max_iter),
                                             _ptr(d_work), int(work_bytes), _ptr(d_alive), _ptr(d_distortion), _ptr(d_iters),
                                             _ptr(d_labels), _c.byref(unfinished)))
    return int(unfinished.value)


def motion_hist_device(d_points, set_stride, ld, T, d, D, d_codebooks, K, offsets, soft, alpha, d_work, work_bytes, d_out, ldo,
                       f64=True, device=0):
    """DEVICE out [E, D * K]: the row-normalised hard (soft = 0) or soft histograms of the examples: klnmf_motion_hist_device."""
    offsets, p_off = _host_array(offsets, np.int64)
    _check(load().klnmf_motion_hist_device(device, _dt_code(f64), _ptr(d_points), int(set_stride), int(ld), int(T), int(d), int(D),
                                           _ptr(d_codebooks), int(K), p_off, offsets.size - 1, int(soft), float(alpha),
                                           _ptr(d_work), int(work_bytes), _ptr(d_out), int(ldo)))


def csr_rows_to_dense_device(d_indptr, d_indices, d_data, f64, src_rows, d_row_idx, rows, d, d_out, ld, device=0):
    """Rows row_idx[0 .. rows) of one DEVICE-resident CSR matrix (int64 row pointers, int32 column indices, float32 / float64
    values; pointers) as a dense float64 device matrix [rows, d], rows `ld` apart: klnmf_csr_rows_to_dense_device."""
    _check(load().klnmf_csr_rows_to_dense_device(device, _dt_code(f64), _c.c_void_p(d_indptr), _c.c_void_p(d_indices),
                                                 _c.c_void_p(d_data), int(src_rows), _c.c_void_p(d_row_idx), int(rows), int(d),
                                                 _c.c_void_p(d_out), int(ld)))


Q_FP8_LOOP, Q_FP8_TILE_ITERS, Q_FP8_COL_ITERS, Q_RATIO_TILE_BYTES, Q_COMM_RANKS = 0, 1, 2, 3, 4
Q_W8_SATURATED, Q_W8_FALLBACKS, Q_RATIO_SATURATED, Q_RATIO_UNFIXED = 5, 6, 7, 8
Q_NO_NUM_EPS = 9
Q_MON_CHECKS, Q_MON_TRIPS, Q_MON_GAVE_UP = 10, 11, 12
Q_FP8_POLL_DUE = 13
Q_SP_COL_BLOCKS, Q_SP_ROW_BLOCKS = 14, 15
Q_EX_ROW_CHUNKS, Q_EX_W_CHUNKS, Q_EX_H_SEGMENTS, Q_EX_H_FROM_SLABS = 16, 17, 18, 19
Q_WEIGHTED = 20
Q_PRESENCE = 21
Q_BATCH_COUNT = 22
BATCH_MAX = 256
MAX_MODALITIES = 16
QF_SUM_V, QF_NNZ_V, QF_MON_STAT, QF_MON_THRESHOLD = 0, 1, 2, 3
QF_KL_OVER_SUM_V = 9


def plan_query(precision, n, f, k, what, nnz=-1, cu_count=256):
    """klnmf_plan_query: what `Context.query(what)` answers right after set_problem(n, f, k) -- with nnz >= 0 after
    set_problem_sparse -- on a device with `cu_count` compute units, for the items of the launch plan (Q_RATIO_TILE_BYTES,
    Q_SP_*, Q_EX_*).  No context, no GPU.  Raises NativeError where that call would refuse the shape."""
    if isinstance(precision, str):
        precision = PRECISIONS[precision]
    v = _i64(0)
    _check(load().klnmf_plan_query(int(precision), int(n), int(f), int(k), int(nnz), int(cu_count), int(what), ctypes.byref(v)))
    return int(v.value)


def selftest(device=0):
    lib = load()
    failed = _c.c_int(-1)
    _check(lib.klnmf_selftest(device, ctypes.byref(failed)))
    return failed.value


class Context(object):
    """One GPU-resident KL-NMF problem (V, W, H on the device)."""

    # Handles of closed `pooled` contexts, per (precision, device): experiment.py runs hundreds of short fits and
    # transforms in sequence (experiment.py:158-180, 235-238), each through its own KLdivNMF object; creating and
    # destroying a native context (a HIP stream, ~25 device blocks) per call cost as much as a small transform itself.
    # A pooled context is handed back with its problem released (klnmf_release_problem: device blocks to the block
    # cache); the stream and the handle live on.
    _pool = {}
    _POOL_MAX = 4

    def __init__(self, precision='f64', device=0, stream=None, pooled=False):
        self._lib = load()
        self._h = _ctx_p()
        if isinstance(precision, str):
            precision = PRECISIONS[precision]
        self.precision = precision
        # the mode's canonical name (what device_data picks the fp32 / fp64 source copies by)
        self.precision_name = {PREC_F64: 'f64', PREC_F32: 'f32', PREC_BF16: 'f16', PREC_BF16X3: 'bf16x3',
                               PREC_F16X3: 'f16x3'}[precision]
        self.n = self.f = self.k = 0
        self.cap = 0
        self._pool_key = (precision, int(device)) if (pooled and stream is None and os.environ.get('KLNMF_NO_POOL') != '1') else None
        if self._pool_key is not None:
            free = Context._pool.get(self._pool_key)
            if free:
                self._h = free.pop()
                return
        # stream: None -> the context creates its own stream; an integer hipStream_t handle otherwise, where
        # 0 is the device's default (null) stream -- torch's current stream unless the caller switched --
        # and is passed as KLNMF_STREAM_DEFAULT, because the C-ABI reads NULL as "no stream given".
        if stream is None:
            handle = None
        elif int(stream) == 0:
            handle = _c.c_void_p(STREAM_DEFAULT)
        else:
            handle = _c.c_void_p(int(stream))
        _check(self._lib.klnmf_create(ctypes.byref(self._h), device, precision, handle))

    # -- lifetime --
    def close(self):
        if getattr(self, '_h', None) and self._h.value:
            key = getattr(self, '_pool_key', None)
            free = Context._pool.setdefault(key, []) if key is not None else None
            if free is not None and len(free) < Context._POOL_MAX and self._lib.klnmf_release_problem(self._h) == 0:
                free.append(self._h)
            else:
                self._lib.klnmf_destroy(self._h)
            self._h = _ctx_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def exact(self):
        return self.precision in (PREC_F64, PREC_F32, PREC_BF16X3, PREC_F16X3)

    # -- data in --
    def set_problem(self, n, f, k, max_iter_capacity):
        _check(self._lib.klnmf_set_problem(self._h, n, f, k, max(1, max_iter_capacity)))
        self.n, self.f, self.k, self.cap = n, f, k, max(1, max_iter_capacity)

    def set_v_max(self, vmax):
        _check(self._lib.klnmf_set_v_max(self._h, float(vmax)))

    def reset_V(self):
        _check(self._lib.klnmf_reset_V(self._h))

    def upload_V(self, block, row0=0, col0=0, scale=1.0):
        """V[row0:, col0:] block = scale * block (any strides; row-major view
        is uploaded without a host copy when rows are contiguous)."""
        a = np.asarray(block)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        if a.ndim != 2:
            raise ValueError("2-D block expected")
        if a.shape[0] == 0 or a.shape[1] == 0:
            return
        if a.strides[1] != a.itemsize or a.strides[0] % a.itemsize or \
                a.strides[0] < a.shape[1] * a.itemsize:
            a = np.ascontiguousarray(a)
        ld = a.strides[0] // a.itemsize
        _check(self._lib.klnmf_upload_V(self._h, a.ctypes.data, _np_dtype_code(a),
                                        a.shape[0], a.shape[1], ld, row0, col0,
                                        float(scale)))

    def upload_weights(self, block, row0=0, col0=0, col_bounds=None):
        """Om[row0:, col0:] block = block (klnmf_upload_weights): weights on the cost function, >= 0.  The first call of a
        problem makes it weighted, with every weight not uploaded equal to 1; dense problems in 'f64' / 'f32' only.
        `col_bounds`: the weights in their row x modality form -- `block` is the presence matrix of `upload_presence`."""
        if col_bounds is not None:
            if col0 != 0:
                raise ValueError("a presence matrix spans every column: col0 must be 0")
            return self.upload_presence(block, col_bounds, row0=row0)
        a = np.asarray(block)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        if a.ndim != 2:
            raise ValueError("2-D block expected")
        if a.strides[1] != a.itemsize or a.strides[0] % a.itemsize or a.strides[0] < a.shape[1] * a.itemsize:
            a = np.ascontiguousarray(a)
        ld = a.strides[0] // a.itemsize
        _check(self._lib.klnmf_upload_weights(self._h, a.ctypes.data, _np_dtype_code(a), a.shape[0], a.shape[1], ld, row0, col0))

    def upload_presence(self, P, col_bounds, row0=0):
        """P[row0:row0 + rows, :] = P (klnmf_upload_presence): the weight of modality m -- columns col_bounds[m] .. col_bounds[m + 1] - 1
        -- in each of the rows, >= 0.  The first call of a problem fixes `col_bounds` (0 = b_0 < ... < b_M = f, M <= MAX_MODALITIES)
        and makes the problem masked, with every entry not uploaded equal to 1; dense problems in 'f64' / 'f32' only."""
        a = np.asarray(P)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        if a.ndim != 2:
            raise ValueError("2-D presence matrix expected")
        bounds = [int(b) for b in col_bounds]
        if a.shape[1] != len(bounds) - 1:
            raise ValueError("presence matrix of %d columns for %d modalities" % (a.shape[1], len(bounds) - 1))
        if a.strides[1] != a.itemsize or a.strides[0] % a.itemsize or a.strides[0] < a.shape[1] * a.itemsize:
            a = np.ascontiguousarray(a)
        ld = a.strides[0] // a.itemsize
        cb = (_i64 * len(bounds))(*bounds)
        _check(self._lib.klnmf_upload_presence(self._h, a.ctypes.data, _np_dtype_code(a), a.shape[0], ld, row0, cb, len(bounds) - 1))

    def upload_presence_device_rows(self, dev_ptr, f64, src_rows, ld, row_idx_ptr, rows, src_cols, col_bounds, row0=0):
        """P[row0 + i, m] = dP[row_idx[i], src_cols[m]] -- 1 where src_cols[m] is -1 -- for i < rows (klnmf_upload_presence_device_rows):
        `upload_presence` for a mask that lives in device memory, a float32 / float64 matrix of `src_rows` rows `ld` apart at
        `dev_ptr`.  `row_idx_ptr`: `rows` int64 row indices in device memory (0: rows 0 .. rows - 1), checked on the device
        before anything is read through them; `src_cols`: one source column per modality; `col_bounds` as in `upload_presence`."""
        bounds = [int(b) for b in col_bounds]
        cols = [int(v) for v in src_cols]
        if len(cols) != len(bounds) - 1:
            raise ValueError("%d source columns for %d modalities" % (len(cols), len(bounds) - 1))
        cb = (_i64 * len(bounds))(*bounds)
        sc = (_c.c_int * max(1, len(cols)))(*cols)
        _check(self._lib.klnmf_upload_presence_device_rows(self._h, _c.c_void_p(dev_ptr), _dt_code(f64), int(src_rows), int(ld),
                                                           _c.c_void_p(row_idx_ptr) if row_idx_ptr else None, int(rows), int(row0),
                                                           sc, cb, len(cols)))

    def presence(self):
        """Modalities of the current problem's presence mask (klnmf_query KLNMF_Q_PRESENCE); 0 without one."""
        return int(self.query(Q_PRESENCE))

    def clear_weights(self):
        _check(self._lib.klnmf_clear_weights(self._h))

    def weighted(self):
        """The current problem holds weights (klnmf_query KLNMF_Q_WEIGHTED)."""
        return bool(self.query(Q_WEIGHTED))

    def upload_blocks(self, blocks, scales=None):
        """Upload hstack([s * b ...]) block by block (one fused scale/cast/place
        kernel per block) after fixing the 16-bit storage factor from the
        global maximum."""
        scales = [1.0] * len(blocks) if scales is None else scales
        vmax = 0.0
        for b, s in zip(blocks, scales):
            if b.size:
                vmax = max(vmax, float(s) * float(np.max(b)))
        self.set_v_max(vmax)
        col = 0
        for b, s in zip(blocks, scales):
            self.upload_V(b, row0=0, col0=col, scale=s)
            col += b.shape[1]

    def upload_V_device(self, dev_ptr, rows, cols, ld, row0=0, col0=0, scale=1.0):
        _check(self._lib.klnmf_upload_V_device(self._h, _c.c_void_p(dev_ptr), rows, cols, ld,
                                               row0, col0, float(scale)))

    # ---- CSR input (exact modes) ----
    def set_problem_sparse(self, X, k, max_iter_capacity):
        """X: scipy CSR (explicit zeros are dropped, indices sorted -- nmf.py:66 does the same).  Uploads the
        structure in CSR order and the values; the library builds the CSC order on the device (klnmf_upload_csr_rows)."""
        import scipy.sparse as sp
        X = sp.csr_matrix(X, copy=True)
        X.eliminate_zeros()
        X.sort_indices()
        n, f = X.shape
        nnz = int(X.nnz)
        dt = np.float32 if X.dtype == np.float32 else np.float64
        _check(self._lib.klnmf_set_problem_sparse(self._h, n, f, k, int(max_iter_capacity), nnz))
        self.n, self.f, self.k, self.cap = n, f, k, int(max_iter_capacity)
        self.nnz = nnz
        indptr = np.ascontiguousarray(X.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(X.indices, dtype=np.int64)
        data = np.ascontiguousarray(X.data, dtype=dt)
        p = lambda a: a.ctypes.data_as(_c.c_void_p)
        _check(self._lib.klnmf_upload_csr_rows(self._h, _dt_code(dt != np.float32), p(indptr), p(indices), p(data)))
        self._csr = (indptr, indices)
        return X

    def set_problem_sparse_shape(self, n, f, k, max_iter_capacity, nnz):
        """A CSR problem of n x f with nnz stored entries whose arrays an upload fills later (klnmf_set_problem_sparse alone):
        `upload_csr_device_rows` gathers them from device-resident modalities."""
        _check(self._lib.klnmf_set_problem_sparse(self._h, int(n), int(f), int(k), int(max_iter_capacity), int(nnz)))
        self.n, self.f, self.k, self.cap = int(n), int(f), int(k), int(max_iter_capacity)
        self.nnz = int(nnz)

    def upload_csr_device_rows(self, sources, col_bounds, scales, src_rows, row_idx_ptr, rows):
        """The CSR of hstack([scale * X[rows] ...]) gathered on the device (klnmf_upload_csr_device_rows).  `sources`: one
        (indptr pointer, indices pointer, data pointer, values are float64) per modality -- DEVICE arrays: int64 row pointers,
        int32 column indices, float32 / float64 values; `col_bounds`: the modalities' column bounds, 0 .. f; `row_idx_ptr`: `rows`
        int64 row indices in device memory.  Only pointers and per-modality scalars cross the boundary."""
        M = len(sources)
        if len(col_bounds) != M + 1 or len(scales) != M:
            raise ValueError("%d sources need %d column bounds and %d scales" % (M, M + 1, M))
        ptrs = lambda j: (_c.c_void_p * M)(*[int(s[j]) or None for s in sources])
        dts = (_c.c_int * M)(*[_dt_code(s[3]) for s in sources])
        cb = (_i64 * (M + 1))(*[int(b) for b in col_bounds])
        sc = (_c.c_double * M)(*[float(v) for v in scales])
        _check(self._lib.klnmf_upload_csr_device_rows(self._h, M, ptrs(0), ptrs(1), ptrs(2), dts, cb, sc, int(src_rows),
                                                      _c.c_void_p(row_idx_ptr), int(rows)))

    def get_Q_values(self, dtype=np.float64):
        out = np.empty(self.nnz, dtype=dtype)
        _check(self._lib.klnmf_get_Q_values(self._h, out.ctypes.data, _np_dtype_code(out)))
        return out

    def upload_V_device_rows(self, dev_ptr, row_idx_ptr, rows, cols, ld, row0=0, col0=0, scale=1.0):
        """Rows row_idx[0..rows) (int64 device array) of a device-resident fp32 matrix."""
        _check(self._lib.klnmf_upload_V_device_rows(self._h, _c.c_void_p(dev_ptr), _c.c_void_p(row_idx_ptr),
                                                    rows, cols, ld, row0, col0, float(scale)))

    def upload_V_device_rows_dt(self, dev_ptr, f64, row_idx_ptr, rows, cols, ld, row0=0, col0=0, scale=1.0):
        """The same for a float32 or float64 device-resident matrix; row_idx_ptr 0: rows 0 .. rows - 1."""
        _check(self._lib.klnmf_upload_V_device_rows_dt(self._h, _c.c_void_p(dev_ptr), _dt_code(f64),
                                                       _c.c_void_p(row_idx_ptr) if row_idx_ptr else None, rows, cols, ld,
                                                       row0, col0, float(scale)))

    def set_H_device(self, dev_ptr, f64, ld, col0, ncols, last=True):
        """H[:, col0 : col0 + ncols] from a device-resident dictionary (klnmf_set_H_device)."""
        _check(self._lib.klnmf_set_H_device(self._h, _c.c_void_p(dev_ptr), _dt_code(f64), int(ld), int(col0),
                                            int(ncols), 1 if last else 0))

    def get_W_device(self, dev_ptr, f64, ld):
        """The coefficients into device memory ([n, k], rows ld apart): klnmf_get_W_device."""
        _check(self._lib.klnmf_get_W_device(self._h, _c.c_void_p(dev_ptr), _dt_code(f64), int(ld)))

    def set_H(self, H):
        H = _as_float_array(H)
        assert H.shape == (self.k, self.f)
        _check(self._lib.klnmf_set_H(self._h, H.ctypes.data, _np_dtype_code(H)))

    def set_W(self, W):
        W = _as_float_array(W)
        assert W.shape == (self.n, self.k)
        _check(self._lib.klnmf_set_W(self._h, W.ctypes.data, _np_dtype_code(W)))

    def set_Q(self, Q):
        Q = _as_float_array(Q)
        assert Q.shape == (self.n, self.f)
        _check(self._lib.klnmf_set_Q(self._h, Q.ctypes.data, _np_dtype_code(Q)))

    # -- the path --
    def init_W(self):
        _check(self._lib.klnmf_init_W(self._h))

    def run(self, max_iter, fit, tol_abs):
        """Returns (errors list, n_done, stopped)."""
        max_iter = int(max_iter)
        if max_iter > self.cap:
            raise ValueError("max_iter exceeds capacity")
        errs = np.zeros(max(1, max_iter), dtype=np.float64)
        nd = _i64(0)
        stopped = _c.c_int(0)
        _check(self._lib.klnmf_run(self._h, max_iter, 1 if fit else 0, float(tol_abs),
                                   errs.ctypes.data_as(_c.POINTER(_c.c_double)),
                                   ctypes.byref(nd), ctypes.byref(stopped)))
        return [float(e) for e in errs[:nd.value]], nd.value, bool(stopped.value)

    # ---- native collective path (RCCL inside the C-ABI) ----
    @staticmethod
    def comm_unique_id():
        buf = ctypes.create_string_buffer(COMM_ID_BYTES)
        _check(load().klnmf_comm_unique_id(buf))
        return bytes(buf.raw)

    def comm_init(self, uid, rank, nranks):
        assert len(uid) == COMM_ID_BYTES
        buf = ctypes.create_string_buffer(bytes(uid), COMM_ID_BYTES)
        _check(self._lib.klnmf_comm_init(self._h, buf, int(rank), int(nranks)))

    def comm_destroy(self):
        _check(self._lib.klnmf_comm_destroy(self._h))

    def comm_max(self, value):
        v = ctypes.c_double(float(value))
        _check(self._lib.klnmf_comm_max(self._h, ctypes.byref(v)))
        return float(v.value)

    def run_sharded(self, n_total, max_iter, fit, tol):
        errs = (ctypes.c_double * max(1, int(max_iter)))()
        n_done = _i64(0)
        stopped = ctypes.c_int(0)
        _check(self._lib.klnmf_run_sharded(self._h, int(n_total), int(max_iter), 1 if fit else 0, float(tol),
                                           errs, ctypes.byref(n_done), ctypes.byref(stopped)))
        nd = int(n_done.value)
        return [float(errs[i]) for i in range(min(nd, int(max_iter)))], nd, bool(stopped.value)

    def loop_begin(self, sum_v_all=None, cells_all=None, nnz_all=None, fp8_shape_all=None):
        """klnmf_loop_begin; with the all-reduced sum of V, element count (and count of entries > 0, and the conjunction of the
        ranks' fp8_shape_ok()): klnmf_loop_begin_sharded(_nnz) / klnmf_loop_begin_agreed (one rank of a row-sharded problem --
        every rank then takes the same fp8 decision)."""
        if sum_v_all is None:
            _check(self._lib.klnmf_loop_begin(self._h))
        elif fp8_shape_all is not None:
            _check(self._lib.klnmf_loop_begin_agreed(self._h, float(sum_v_all), float(cells_all),
                                                     float(-1.0 if nnz_all is None else nnz_all), 1 if fp8_shape_all else 0))
        elif nnz_all is None:
            _check(self._lib.klnmf_loop_begin_sharded(self._h, float(sum_v_all), float(cells_all)))
        else:
            _check(self._lib.klnmf_loop_begin_sharded_nnz(self._h, float(sum_v_all), float(cells_all), float(nnz_all)))

    def fp8_shape_ok(self):
        """This problem's shape allows fp8 ratio tiles (klnmf_query KLNMF_Q_RATIO_TILE_BYTES == 1)."""
        return self.query(Q_RATIO_TILE_BYTES) == 1

    def sum_V(self):
        """Sum of the uploaded V as stored (klnmf_query_f64 KLNMF_QF_SUM_V)."""
        v = _c.c_double(0.0)
        _check(self._lib.klnmf_query_f64(self._h, 0, ctypes.byref(v)))
        return float(v.value)

    def nnz_V(self):
        """How many entries of the uploaded V are > 0 as stored (klnmf_query_f64 KLNMF_QF_NNZ_V)."""
        v = _c.c_double(0.0)
        _check(self._lib.klnmf_query_f64(self._h, 1, ctypes.byref(v)))
        return float(v.value)

    def run_more(self, iters, fit=True, tol_abs=0.0):
        """`iters` whole iterations of the open loop, enqueued as klnmf_run does (klnmf_run_more)."""
        _check(self._lib.klnmf_run_more(self._h, int(iters), 1 if fit else 0, float(tol_abs)))

    def iter_rowpass(self, fit=True):
        _check(self._lib.klnmf_iter_rowpass(self._h, 1 if fit else 0))

    def iter_decide(self, tol_abs):
        _check(self._lib.klnmf_iter_decide(self._h, float(tol_abs)))

    def iter_colpass(self):
        _check(self._lib.klnmf_iter_colpass(self._h))

    def iter_colpass_part(self, part):
        """Column pass + numerator of ONE column part of the split layout (`exchange_parts`): the caller exchanges the part
        while the next one computes."""
        _check(self._lib.klnmf_iter_colpass_part(self._h, int(part)))

    def exchange_parts(self):
        """[(element offset, element count, first column, columns)] of the numerator's column parts (one whole-matrix part
        unless KLNMF_COMM_PARTS split the problem)."""
        n = _c.c_int(0)
        arr = lambda: (_i64 * 4)()
        off, cnt, c0, nc = arr(), arr(), arr(), arr()
        _check(self._lib.klnmf_exchange_parts(self._h, ctypes.byref(n), off, cnt, c0, nc))
        return [(int(off[p]), int(cnt[p]), int(c0[p]), int(nc[p])) for p in range(n.value)]

    def iter_update_H(self):
        _check(self._lib.klnmf_iter_update_H(self._h))

    def iter_advance(self):
        _check(self._lib.klnmf_iter_advance(self._h))

    def loop_end(self, max_iter):
        errs = np.zeros(max(1, int(max_iter)), dtype=np.float64)
        nd = _i64(0)
        stopped = _c.c_int(0)
        _check(self._lib.klnmf_loop_end(self._h, errs.ctypes.data_as(_c.POINTER(_c.c_double)),
                                        ctypes.byref(nd), ctypes.byref(stopped)))
        return [float(e) for e in errs[:nd.value]], nd.value, bool(stopped.value)

    def exchange_buffers(self):
        """(loss_ptr, numer_ptr, numer_count, numer_is_f64) device pointers."""
        lp, npt = _c.c_void_p(), _c.c_void_p()
        cnt = _i64(0)
        is64 = _c.c_int(0)
        _check(self._lib.klnmf_exchange_buffers(self._h, ctypes.byref(lp), ctypes.byref(npt),
                                                ctypes.byref(cnt), ctypes.byref(is64)))
        return lp.value, npt.value, cnt.value, bool(is64.value)

    def exchange_layout(self):
        stride, valid = _i64(0), _i64(0)
        _check(self._lib.klnmf_exchange_layout(self._h, ctypes.byref(stride), ctypes.byref(valid)))
        return int(stride.value), int(valid.value)

    def bind_exchange(self, loss_ptr, numer_ptr):
        _check(self._lib.klnmf_bind_exchange(self._h, _c.c_void_p(loss_ptr),
                                             _c.c_void_p(numer_ptr)))

    def error(self):
        out = _c.c_double(0)
        _check(self._lib.klnmf_error(self._h, ctypes.byref(out)))
        return out.value

    def loss_terms(self):
        out = (ctypes.c_double * 4)()
        _check(self._lib.klnmf_loss_terms(self._h, out))
        return [float(v) for v in out]

    def update(self, fit=True):
        _check(self._lib.klnmf_update(self._h, 1 if fit else 0))

    def set_ratio_eps(self, eps):
        _check(self._lib.klnmf_set_ratio_eps(self._h, float(eps)))

    def step_Q(self):
        _check(self._lib.klnmf_step_Q(self._h))

    def step_W(self):
        _check(self._lib.klnmf_step_W(self._h))

    def step_H(self):
        _check(self._lib.klnmf_step_H(self._h))

    # -- the beta-divergence cost (include/klnmf_beta.h) --
    def set_divergence(self, beta):
        """The cost function of the current problem (klnmf_set_divergence): after `set_problem` and the uploads, before a loop;
        dense problems in 'f64' / 'f32' only.  beta = 1 is the KL loop again."""
        _check(self._lib.klnmf_set_divergence(self._h, float(beta)))

    def get_divergence(self):
        out = _c.c_double(0)
        _check(self._lib.klnmf_get_divergence(self._h, ctypes.byref(out)))
        return out.value

    def beta_loss(self):
        """The beta cost of the current V, W, H and weights (klnmf_beta_loss)."""
        out = _c.c_double(0)
        _check(self._lib.klnmf_beta_loss(self._h, ctypes.byref(out)))
        return out.value

    def beta_step(self, which):
        """One rule from a freshly formed A and B (klnmf_beta_step): 0 / 'W' the W rule, 1 / 'H' the H rule with its
        normalisation and the compensation on W's columns."""
        which = {'W': 0, 'H': 1}.get(which, which)
        _check(self._lib.klnmf_beta_step(self._h, int(which)))

    def generalized_kl(self, x, y, eps):
        x = _as_float_array(x).ravel()
        y = _as_float_array(y).ravel()
        if x.dtype != y.dtype:
            x = x.astype(np.float64)
            y = y.astype(np.float64)
        out = _c.c_double(0)
        _check(self._lib.klnmf_generalized_kl(self._h, x.ctypes.data, y.ctypes.data,
                                              _np_dtype_code(x), x.size, float(eps),
                                              ctypes.byref(out)))
        return out.value

    # -- data out --
    def _get(self, fn, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        _check(fn(self._h, out.ctypes.data, _np_dtype_code(out)))
        return out

    def get_W(self, dtype=np.float64):
        return self._get(self._lib.klnmf_get_W, (self.n, self.k), dtype)

    def get_H(self, dtype=np.float64):
        return self._get(self._lib.klnmf_get_H, (self.k, self.f), dtype)

    def get_Q(self, dtype=np.float64):
        return self._get(self._lib.klnmf_get_Q, (self.n, self.f), dtype)

    # -- measurement --
    def profile_enable(self, on=True):
        """True / 1: every iteration's row- and column-pass launches bracketed by HIP events; N > 1: every N-th iteration's."""
        _check(self._lib.klnmf_profile_enable(self._h, int(on) if on else 0))

    def profile_read(self, reset=True):
        rn, cn = _i64(0), _i64(0)
        rms, cms = _c.c_double(0), _c.c_double(0)
        _check(self._lib.klnmf_profile_read(self._h, ctypes.byref(rn), ctypes.byref(rms),
                                            ctypes.byref(cn), ctypes.byref(cms),
                                            1 if reset else 0))
        tn, tr, tms = _i64(0), _i64(0), _c.c_double(0)
        _check(self._lib.klnmf_profile_read_tail(self._h, ctypes.byref(tn), ctypes.byref(tms), ctypes.byref(tr),
                                                 1 if reset else 0))
        return {'rowpass_launches': rn.value, 'rowpass_ms': rms.value,
                'colpass_launches': cn.value, 'colpass_ms': cms.value,
                'tail_launches': tn.value, 'tail_ms': tms.value, 'tail_rows': tr.value}

    def synchronize(self):
        _check(self._lib.klnmf_synchronize(self._h))

    def query(self, what):
        """klnmf_query: what the context decided / what its last loop ran (Q_* items above)."""
        v = _i64(0)
        _check(self._lib.klnmf_query(self._h, int(what), ctypes.byref(v)))
        return int(v.value)

    def fp8_report(self):
        """{'allowed', 'tile_iterations', 'column_pass_iterations'} of the last loop -- read from the library, not re-derived."""
        return {'allowed': bool(self.query(Q_FP8_LOOP)), 'tile_iterations': self.query(Q_FP8_TILE_ITERS),
                'column_pass_iterations': self.query(Q_FP8_COL_ITERS),
                # e4m3 saturation: counted and kept out of the result (see include/klnmf.h)
                'w_image_saturated': self.query(Q_W8_SATURATED), 'w_image_fallback_iterations': self.query(Q_W8_FALLBACKS),
                'ratio_saturated': self.query(Q_RATIO_SATURATED), 'ratio_unfixed': self.query(Q_RATIO_UNFIXED),
                # the loop's update passes formed the ratio without the numerator's eps (large-mean data; loss corrected exactly)
                'no_numerator_eps': bool(self.query(Q_NO_NUM_EPS)),
                # the in-loop monitor (csrc/monitor.hip.h): measured relative error of the sampled H-numerator entries
                'monitor_checks': self.query(Q_MON_CHECKS), 'monitor_trips': self.query(Q_MON_TRIPS),
                'gave_up': bool(self.query(Q_MON_GAVE_UP)), 'monitor_statistic': self.query_f64(QF_MON_STAT),
                'monitor_threshold': self.query_f64(QF_MON_THRESHOLD),
                'monitor_parts': [self.query_f64(4 + i) for i in range(3)],
                'monitor_min_spread': self.query_f64(7), 'monitor_spread_threshold': self.query_f64(8),
                # the loop's final KL / sum(V) (16-bit modes; -1: none): the data condition of the f16 operands' accuracy envelope
                'kl_over_sum_v': self.query_f64(QF_KL_OVER_SUM_V)}

    def fp8_poll_due(self):
        """Loops in pieces on row shards: the next `iter_advance` reads the all-reduced count in loss[1] (KLNMF_Q_FP8_POLL_DUE)."""
        return bool(self.query(Q_FP8_POLL_DUE))

    def sparse_blocks(self):
        """(column blocks, row blocks) of the CSR kernels this problem runs on; (0, 0): the unblocked kernels, or a dense
        problem (KLNMF_Q_SP_COL_BLOCKS / KLNMF_Q_SP_ROW_BLOCKS)."""
        return self.query(Q_SP_COL_BLOCKS), self.query(Q_SP_ROW_BLOCKS)

    def exact_regime(self):
        """(row chunks, W chunks, H segments, from slabs) of the dense exact-mode kernels this problem runs on; all 0: a CSR
        problem, a 16-bit-mode problem or none (KLNMF_Q_EX_ROW_CHUNKS / _W_CHUNKS / _H_SEGMENTS / _H_FROM_SLABS)."""
        return (self.query(Q_EX_ROW_CHUNKS), self.query(Q_EX_W_CHUNKS), self.query(Q_EX_H_SEGMENTS),
                self.query(Q_EX_H_FROM_SLABS))

    def query_f64(self, what):
        v = _c.c_double(0.0)
        _check(self._lib.klnmf_query_f64(self._h, int(what), ctypes.byref(v)))
        return float(v.value)


def group_selftest(devices, count, f64=False):
    """klnmf_group_selftest: the group exchange alone on `len(devices)` buffers of `count` elements (float64 or float32) filled
    with values whose sum depends on the order of summation; returns the number of elements (and loss pairs) that differ
    bit for bit from the host's sum in shard order (0 = pass)."""
    lib = load()
    devs = (_c.c_int * len(devices))(*[int(d) for d in devices])
    failed = _c.c_int(-1)
    _check(lib.klnmf_group_selftest(devs, len(devices), int(count), _dt_code(f64), ctypes.byref(failed)))
    return failed.value


class Group(object):
    """klnmf_group_*: the row shards of one problem, one `Context` each (a device may repeat), driven from this thread.  The
    contexts' problems must be set (same f, k, precision, capacity); the group binds its own exchange buffers to them until
    `close()`.  The contexts stay owned by the caller and must outlive the group."""

    def __init__(self, contexts):
        self._lib = load()
        self._h = _c.c_void_p()
        self.contexts = list(contexts)
        arr = (_ctx_p * len(self.contexts))(*[c._h.value for c in self.contexts])
        _check(self._lib.klnmf_group_create(ctypes.byref(self._h), arr, len(self.contexts)))

    def run(self, n_total, max_iter, fit, tol):
        """The whole loop over the shards (tol relative, nmf.py:207); returns (errors list, n_done, stopped) -- shard 0's,
        identical on every shard.  NativeError with code ERR_REPLICA if the shards' dictionaries differ after a fit."""
        max_iter = int(max_iter)
        errs = np.zeros(max(1, max_iter), dtype=np.float64)
        nd = _i64(0)
        stopped = _c.c_int(0)
        _check(self._lib.klnmf_group_run(self._h, int(n_total), max_iter, 1 if fit else 0, float(tol),
                                         errs.ctypes.data_as(_c.POINTER(_c.c_double)), ctypes.byref(nd),
                                         ctypes.byref(stopped)))
        return [float(e) for e in errs[:nd.value]], nd.value, bool(stopped.value)

    def enqueue_time(self):
        """(iterations timed, median ms, largest ms) of the host's per-iteration enqueue in the last `run`."""
        it, med, mx = _i64(0), _c.c_double(0), _c.c_double(0)
        _check(self._lib.klnmf_group_enqueue_time(self._h, ctypes.byref(it), ctypes.byref(med), ctypes.byref(mx)))
        return it.value, med.value, mx.value

    def close(self):
        if getattr(self, '_h', None) is not None and self._h.value:
            self._lib.klnmf_group_destroy(self._h)
            self._h = _c.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Batch(object):
    """klnmf_batch_*: `count` dense problems of one shape (n, f, k) in 'f64' / 'f32' on one device -- unweighted, or all of them
    under presence masks that share their column bounds (`upload_presence`) -- that run the multiplicative-update loop together,
    every stage of an iteration one launch for all of them.  Each problem `p` keeps its own V, W, H, mask, loss record and stop
    state; its results are bit for bit those of the same problem alone in a `Context` whose chunk counts equal the batch's
    (`exact_regime()`).  The methods mirror `Context`'s with the problem index in front.  `set_divergence(beta)` makes the loop
    the beta-divergence one for every problem (klnmf_batch_beta.h), with weights per problem (`upload_weights`)."""

    def __init__(self, precision, count, device=0):
        self._lib = load()
        self._h = _c.c_void_p()
        if isinstance(precision, str):
            precision = PRECISIONS[precision]
        self.precision = precision
        self.count = int(count)
        self.device = int(device)
        self.n = self.f = self.k = 0
        self.cap = 0
        _check(self._lib.klnmf_batch_create(ctypes.byref(self._h), int(device), int(precision), int(count)))
        self.precision_name = {PREC_F64: 'f64', PREC_F32: 'f32'}[precision]

    def close(self):
        if getattr(self, '_h', None) is not None and self._h.value:
            self._lib.klnmf_batch_destroy(self._h)
            self._h = _c.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_problem(self, n, f, k, max_iter_capacity):
        _check(self._lib.klnmf_batch_set_problem(self._h, int(n), int(f), int(k), max(1, int(max_iter_capacity))))
        self.n, self.f, self.k, self.cap = int(n), int(f), int(k), max(1, int(max_iter_capacity))

    # ---- CSR problems (klnmf_batch_csr.h): every problem its own stored entries, one shape ----
    def set_problem_sparse(self, n, f, k, max_iter_capacity, nnzs):
        """`count` CSR problems of n x f with nnzs[p] stored entries each (klnmf_batch_set_problem_sparse); `upload_csr_rows` /
        `upload_csr_device_rows` fill them.  Refused (NativeError, the previous problem stays): k > 512, an empty problem."""
        nnzs = [int(v) for v in nnzs]
        if len(nnzs) != self.count:
            raise ValueError("%d nnz for a batch of %d" % (len(nnzs), self.count))
        cap = max(1, int(max_iter_capacity))
        _check(self._lib.klnmf_batch_set_problem_sparse(self._h, int(n), int(f), int(k), cap, (_i64 * self.count)(*nnzs)))
        self.n, self.f, self.k, self.cap = int(n), int(f), int(k), cap
        self.nnzs = nnzs

    def upload_csr_rows(self, p, X):
        """Problem p's X from a scipy CSR matrix (klnmf_batch_upload_csr_rows): explicit zeros dropped and indices sorted by the
        caller -- `csr_canonical` -- so that X.nnz is the nnzs[p] the problem was set for."""
        indptr = np.ascontiguousarray(X.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(X.indices, dtype=np.int64)
        dt = np.float32 if X.dtype == np.float32 else np.float64
        data = np.ascontiguousarray(X.data, dtype=dt)
        ptr = lambda a: a.ctypes.data_as(_c.c_void_p)
        _check(self._lib.klnmf_batch_upload_csr_rows(self._h, int(p), _dt_code(dt != np.float32), ptr(indptr), ptr(indices),
                                                     ptr(data)))

    def upload_csr_device_rows(self, p, sources, col_bounds, scales, src_rows, row_idx_ptr, rows):
        """`Context.upload_csr_device_rows` for problem p (klnmf_batch_upload_csr_device_rows): synchronous."""
        M = len(sources)
        if len(col_bounds) != M + 1 or len(scales) != M:
            raise ValueError("%d sources need %d column bounds and %d scales" % (M, M + 1, M))
        ptrs = lambda j: (_c.c_void_p * M)(*[int(s[j]) or None for s in sources])
        dts = (_c.c_int * M)(*[_dt_code(s[3]) for s in sources])
        cb = (_i64 * (M + 1))(*[int(b) for b in col_bounds])
        sc = (_c.c_double * M)(*[float(v) for v in scales])
        _check(self._lib.klnmf_batch_upload_csr_device_rows(self._h, int(p), M, ptrs(0), ptrs(1), ptrs(2), dts, cb, sc, int(src_rows),
                                                            _c.c_void_p(row_idx_ptr), int(rows)))

    def sparse_blocks(self):
        """(column blocks, row blocks) of a CSR batch's plan, as `Context.query` answers them; (0, 0) for a dense batch."""
        return (self.query(Q_SP_COL_BLOCKS), self.query(Q_SP_ROW_BLOCKS))

    def upload_V(self, p, block, row0=0, col0=0, scale=1.0):
        a = np.asarray(block)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        if a.ndim != 2:
            raise ValueError("2-D block expected")
        if a.shape[0] == 0 or a.shape[1] == 0:
            return
        if a.strides[1] != a.itemsize or a.strides[0] % a.itemsize or a.strides[0] < a.shape[1] * a.itemsize:
            a = np.ascontiguousarray(a)
        ld = a.strides[0] // a.itemsize
        _check(self._lib.klnmf_batch_upload_V(self._h, int(p), a.ctypes.data, _np_dtype_code(a), a.shape[0], a.shape[1], ld,
                                              int(row0), int(col0), float(scale)))

    def upload_V_device_rows_dt(self, p, dev_ptr, f64, row_idx_ptr, rows, cols, ld, row0=0, col0=0, scale=1.0):
        _check(self._lib.klnmf_batch_upload_V_device_rows_dt(self._h, int(p), _c.c_void_p(dev_ptr), _dt_code(f64),
                                                             _c.c_void_p(row_idx_ptr) if row_idx_ptr else None, int(rows), int(cols),
                                                             int(ld), int(row0), int(col0), float(scale)))

    def upload_presence(self, p, P, col_bounds, row0=0):
        """`Context.upload_presence` for problem p (klnmf_batch_upload_presence).  The first call on a batch fixes `col_bounds` for
        every problem and makes the whole batch masked, every entry not uploaded equal to 1."""
        a = np.asarray(P)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        if a.ndim != 2:
            raise ValueError("2-D presence matrix expected")
        bounds = [int(b) for b in col_bounds]
        if a.shape[1] != len(bounds) - 1:
            raise ValueError("presence matrix of %d columns for %d modalities" % (a.shape[1], len(bounds) - 1))
        if a.strides[1] != a.itemsize or a.strides[0] % a.itemsize or a.strides[0] < a.shape[1] * a.itemsize:
            a = np.ascontiguousarray(a)
        ld = a.strides[0] // a.itemsize
        cb = (_i64 * len(bounds))(*bounds)
        _check(self._lib.klnmf_batch_upload_presence(self._h, int(p), a.ctypes.data, _np_dtype_code(a), a.shape[0], ld, int(row0), cb,
                                                     len(bounds) - 1))

    def upload_presence_device_rows(self, p, dev_ptr, f64, src_rows, ld, row_idx_ptr, rows, src_cols, col_bounds, row0=0):
        """`Context.upload_presence_device_rows` for problem p (klnmf_batch_upload_presence_device_rows): synchronous."""
        bounds = [int(b) for b in col_bounds]
        cols = [int(v) for v in src_cols]
        if len(cols) != len(bounds) - 1:
            raise ValueError("%d source columns for %d modalities" % (len(cols), len(bounds) - 1))
        cb = (_i64 * len(bounds))(*bounds)
        sc = (_c.c_int * max(1, len(cols)))(*cols)
        _check(self._lib.klnmf_batch_upload_presence_device_rows(self._h, int(p), _c.c_void_p(dev_ptr) if dev_ptr else None,
                                                                 _dt_code(f64), int(src_rows), int(ld),
                                                                 _c.c_void_p(row_idx_ptr) if row_idx_ptr else None, int(rows), int(row0),
                                                                 sc, cb, len(cols)))

    def clear_presence(self):
        """The batch runs the unmasked kernels again (klnmf_batch_clear_presence)."""
        _check(self._lib.klnmf_batch_clear_presence(self._h))

    def presence(self):
        """Modalities of the batch's presence masks (klnmf_batch_query KLNMF_Q_PRESENCE); 0 without one."""
        return self.query(Q_PRESENCE)

    # ---- the beta-divergence cost (klnmf_batch_beta.h): one beta for every problem, weights per problem ----
    def set_divergence(self, beta):
        """The cost function of every problem of the batch (klnmf_batch_set_divergence), behind `set_problem` and in front of a
        run: beta != 1 makes `run` the beta loop of `Context.set_divergence`; 1.0 gives the Kullback-Leibler loop back and drops the
        weights.  Refused (NativeError, the batch stays as it was): a CSR batch, a batch with a presence mask, a beta that is not
        finite, in 'f32' a beta that fp32 rounds to 1 or to 0 without being it."""
        _check(self._lib.klnmf_batch_set_divergence(self._h, float(beta)))

    def get_divergence(self):
        v = _c.c_double(1.0)
        _check(self._lib.klnmf_batch_get_divergence(self._h, ctypes.byref(v)))
        return float(v.value)

    def upload_weights(self, p, block, row0=0, col0=0):
        """`Context.upload_weights` for problem p of a batch with beta != 1 (klnmf_batch_upload_weights): weights >= 0 on the cost
        function.  The first call makes the whole batch weighted, every weight not uploaded equal to 1."""
        a = np.asarray(block)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        if a.ndim != 2:
            raise ValueError("2-D block expected")
        if a.strides[1] != a.itemsize or a.strides[0] % a.itemsize or a.strides[0] < a.shape[1] * a.itemsize:
            a = np.ascontiguousarray(a)
        ld = a.strides[0] // a.itemsize
        _check(self._lib.klnmf_batch_upload_weights(self._h, int(p), a.ctypes.data, _np_dtype_code(a), a.shape[0], a.shape[1], ld,
                                                    int(row0), int(col0)))

    def set_H(self, p, H):
        H = _as_float_array(H)
        assert H.shape == (self.k, self.f)
        _check(self._lib.klnmf_batch_set_H(self._h, int(p), H.ctypes.data, _np_dtype_code(H)))

    def set_H_device(self, p, dev_ptr, f64, ld, col0, ncols, last=True):
        _check(self._lib.klnmf_batch_set_H_device(self._h, int(p), _c.c_void_p(dev_ptr), _dt_code(f64), int(ld), int(col0),
                                                  int(ncols), 1 if last else 0))

    def set_W(self, p, W):
        W = _as_float_array(W)
        assert W.shape == (self.n, self.k)
        _check(self._lib.klnmf_batch_set_W(self._h, int(p), W.ctypes.data, _np_dtype_code(W)))

    def init_W(self):
        _check(self._lib.klnmf_batch_init_W(self._h))

    def run(self, max_iter, fit, tol_abs):
        """The loop for every problem; returns [(errors list, n_done, stopped)] in problem order."""
        max_iter = int(max_iter)
        if max_iter > self.cap:
            raise ValueError("max_iter exceeds capacity")
        _check(self._lib.klnmf_batch_run(self._h, max_iter, 1 if fit else 0, float(tol_abs)))
        return [self.result(p) for p in range(self.count)]

    def result(self, p):
        errs = np.zeros(max(1, self.cap), dtype=np.float64)
        nd = _i64(0)
        stopped = _c.c_int(0)
        _check(self._lib.klnmf_batch_result(self._h, int(p), errs.ctypes.data_as(_c.POINTER(_c.c_double)), ctypes.byref(nd),
                                            ctypes.byref(stopped)))
        return [float(e) for e in errs[:nd.value]], nd.value, bool(stopped.value)

    def _get(self, fn, p, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        _check(fn(self._h, int(p), out.ctypes.data, _np_dtype_code(out)))
        return out

    def get_W(self, p, dtype=np.float64):
        return self._get(self._lib.klnmf_batch_get_W, p, (self.n, self.k), dtype)

    def get_H(self, p, dtype=np.float64):
        return self._get(self._lib.klnmf_batch_get_H, p, (self.k, self.f), dtype)

    def get_W_device(self, p, dev_ptr, f64, ld):
        _check(self._lib.klnmf_batch_get_W_device(self._h, int(p), _c.c_void_p(dev_ptr), _dt_code(f64), int(ld)))

    def query(self, what):
        v = _i64(0)
        _check(self._lib.klnmf_batch_query(self._h, int(what), ctypes.byref(v)))
        return int(v.value)

    def exact_regime(self):
        """(row chunks, W chunks, H segments, from slabs) of the batch's plan, as `Context.exact_regime()` reads."""
        return (self.query(Q_EX_ROW_CHUNKS), self.query(Q_EX_W_CHUNKS), self.query(Q_EX_H_SEGMENTS), self.query(Q_EX_H_FROM_SLABS))
