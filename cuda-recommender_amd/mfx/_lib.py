"""ctypes binding of libmfx.so (include/mfx.h).  The library is the product; this file only
declares its C ABI.  Loading fails loudly when the shared object is missing -- there is no
Python or CPU fallback for any compute entry point."""
from __future__ import annotations

import ctypes as C
import os

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("MFX_LIB_PATH") or os.path.join(_PKG, "libmfx.so")  # (override: A/B builds of the library)

MFX_HOST, MFX_DEVICE = 0, 1
MFX_COMM_ID_BYTES = 128
MFX_VERSION = 2  # include/mfx.h
MFX_FOLD_ALS, MFX_FOLD_ALS_EXACT, MFX_FOLD_CCD, MFX_FOLD_IMPLICIT = 0, 1, 2, 3  # include/mfx.h mfx_fold_model
MFX_SIM_DOT, MFX_SIM_COSINE = 0, 1  # include/mfx.h mfx_rec_metric
MFX_CAND_NO_EXCLUDE = 1  # include/mfx.h, flags of mfx_rec_query_candidates
MFX_DIV_NO_EXCLUDE = 1  # include/mfx.h, flags of mfx_rec_diversify
MFX_KNN_KEEP_SEEN = 1  # include/mfx.h, flags of mfx_knn_recommend
MFX_SLIM_SIGNED = 1  # include/mfx.h, flags of mfx_slim_train and mfx_slim_solve
MFX_EASE_INV_SIMPLE = 1  # include/mfx.h, flags of mfx_ease_inverse and mfx_ease_train

u32p = C.POINTER(C.c_uint32)
f32p = C.POINTER(C.c_float)
f64p = C.POINTER(C.c_double)
i64p = C.POINTER(C.c_int64)


class mfx_csx(C.Structure):
    _fields_ = [("rows", C.c_int64), ("cols", C.c_int64), ("nnz", C.c_int64),
                ("csc_col_ptr", C.c_void_p), ("csc_row_idx", C.c_void_p), ("csc_val", C.c_void_p),
                ("csr_row_ptr", C.c_void_p), ("csr_col_idx", C.c_void_p), ("csr_val", C.c_void_p)]


class mfx_coo(C.Structure):
    _fields_ = [("nnz", C.c_int64), ("row", C.c_void_p), ("col", C.c_void_p), ("val", C.c_void_p)]


class mfx_features(C.Structure):
    _fields_ = [("n", C.c_int64), ("nf", C.c_int64), ("ptr", C.c_void_p), ("idx", C.c_void_p), ("val", C.c_void_p)]


class mfx_params(C.Structure):
    _fields_ = [("k", C.c_uint32), ("lambda_", C.c_float), ("maxiter", C.c_int32), ("maxinneriter", C.c_int32),
                ("nBlocks", C.c_uint32), ("nThreadsPerBlock", C.c_uint32), ("verbose", C.c_int32),
                ("device", C.c_int32), ("schedule", C.c_int32), ("kernel_variant", C.c_int32),
                ("profile", C.c_int32), ("tiles_per_span", C.c_int32), ("panel_rows", C.c_int32),
                ("wg_waves", C.c_int32), ("graph", C.c_int32), ("layout_build", C.c_int32),
                ("do_nmf", C.c_int32), ("eps", C.c_float), ("rank_trace", C.c_int32)]


class mfx_iter_report(C.Structure):
    _fields_ = [("rank_time", C.c_double), ("update_time", C.c_double), ("rmse", C.c_double),
                ("rmse_time", C.c_double)]


class mfx_shard(C.Structure):
    _fields_ = [("comm", C.c_void_p), ("global_col_nnz", C.c_void_p), ("global_test_nnz", C.c_int64)]


class mfx_als_shard(C.Structure):
    _fields_ = [("comm", C.c_void_p), ("row_lo", C.c_int64), ("row_hi", C.c_int64), ("col_lo", C.c_int64),
                ("col_hi", C.c_int64), ("global_test_nnz", C.c_int64)]


class MfxError(RuntimeError):
    pass


# name -> (restype, argtypes); every symbol include/mfx.h declares
SIGNATURES = {
    "mfx_last_error": (C.c_char_p, []),
    "mfx_version": (C.c_int, []),
    "mfx_device_count": (C.c_int, []),
    "mfx_params_default": (None, [C.POINTER(mfx_params)]),
    "mfx_ccdpp_run": (C.c_int, [C.POINTER(mfx_csx), C.POINTER(mfx_coo), C.c_void_p, C.c_void_p,
                                C.POINTER(mfx_params), C.POINTER(mfx_iter_report)]),
    "mfx_als_run": (C.c_int, [C.POINTER(mfx_csx), C.POINTER(mfx_coo), C.c_void_p, C.c_void_p,
                              C.POINTER(mfx_params), C.POINTER(mfx_iter_report)]),
    "mfx_ccd_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(mfx_csx), C.POINTER(mfx_coo),
                                 C.POINTER(mfx_params), C.c_int, C.POINTER(mfx_shard)]),
    "mfx_ccd_set_factors": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_ccd_iterate": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(mfx_iter_report)]),
    "mfx_ccd_get_factors": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_ccd_get_residual": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mfx_ccd_kernel_times": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), f64p, i64p]),
    "mfx_ccd_set_profile": (C.c_int, [C.c_void_p, C.c_int]),
    "mfx_ccd_layout_info": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32)]),
    "mfx_ccd_rank_trace": (C.c_int, [C.c_void_p, C.c_int, f64p, f64p, C.c_int, C.POINTER(C.c_int32)]),
    "mfx_ccd_destroy": (C.c_int, [C.c_void_p]),
    "mfx_als_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(mfx_csx), C.POINTER(mfx_coo),
                                 C.POINTER(mfx_params), C.c_int]),
    "mfx_als_create_sharded": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(mfx_csx), C.POINTER(mfx_coo),
                                         C.POINTER(mfx_params), C.POINTER(mfx_als_shard)]),
    "mfx_als_set_factors": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_als_iterate": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(mfx_iter_report)]),
    "mfx_als_get_factors": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_als_kernel_times": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), f64p, i64p]),
    "mfx_als_destroy": (C.c_int, [C.c_void_p]),
    "mfx_rank_one_sweep": (C.c_int, [C.c_int64, C.c_int64, u32p, u32p, f32p, C.c_int64, f32p, C.c_float, f32p,
                                     C.c_int, C.c_int]),
    "mfx_update_rating": (C.c_int, [C.c_int64, C.c_int64, u32p, u32p, f32p, C.c_int64, f32p, f32p, C.c_int,
                                    C.c_int, C.c_int]),
    "mfx_test_rmse": (C.c_int, [C.POINTER(mfx_coo), f32p, f32p, C.c_int64, C.c_int64, C.c_int64, C.c_int, f64p,
                                C.c_int]),
    "mfx_als_gramian": (C.c_int, [C.c_int64, u32p, C.c_int64, f32p, C.c_int64, f32p, C.c_int]),
    "mfx_als_inverse": (C.c_int, [C.c_int64, f32p, f32p, C.c_int]),
    "mfx_als_half": (C.c_int, [C.c_int64, C.c_int64, u32p, u32p, f32p, C.c_int64, f32p, f32p, C.c_int64,
                               C.c_float, C.c_int, C.c_int]),
    "mfx_ials_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(mfx_csx), C.POINTER(mfx_params), C.c_float, C.c_int]),
    "mfx_ials_loss": (C.c_int, [C.c_void_p, f64p]),
    "mfx_ials_half": (C.c_int, [C.c_int64, C.c_int64, u32p, u32p, f32p, C.c_int64, f32p, f32p, C.c_int64,
                                C.c_float, C.c_float, C.c_int]),
    "mfx_ials_block_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(mfx_csx), C.POINTER(mfx_params), C.c_float, C.c_int32,
                                        C.c_int]),
    "mfx_ials_block_half": (C.c_int, [C.c_int64, C.c_int64, u32p, u32p, f32p, C.c_int64, f32p, f32p, f32p, C.c_int64, C.c_int32,
                                      C.c_float, C.c_float, C.c_int]),
    "mfx_ials_cg_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(mfx_csx), C.POINTER(mfx_params), C.c_float, C.c_int32, C.c_float,
                                     C.c_int]),
    "mfx_ials_cg_stats": (C.c_int, [C.c_void_p, i64p]),
    "mfx_ials_cg_half": (C.c_int, [C.c_int64, C.c_int64, u32p, u32p, f32p, C.c_int64, f32p, f32p, f32p, C.c_int64, C.c_float, C.c_float,
                                   C.c_int32, C.c_float, C.POINTER(C.c_int32), C.c_int]),
    "mfx_spd_inverse": (C.c_int, [C.c_int64, f32p, f32p, C.c_int]),
    "mfx_ials_create_reg": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(mfx_csx), C.POINTER(mfx_params), C.c_float, C.c_float, C.c_float,
                                      C.c_int]),
    "mfx_ials_block_create_reg": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(mfx_csx), C.POINTER(mfx_params), C.c_float, C.c_float,
                                            C.c_float, C.c_int32, C.c_int]),
    "mfx_ials_half_reg": (C.c_int, [C.c_int64, C.c_int64, u32p, u32p, f32p, C.c_int64, f32p, f32p, C.c_int64,
                                    C.c_float, C.c_float, C.c_float, C.c_float, C.c_int]),
    "mfx_ials_block_half_reg": (C.c_int, [C.c_int64, C.c_int64, u32p, u32p, f32p, C.c_int64, f32p, f32p, f32p, C.c_int64, C.c_int32,
                                          C.c_float, C.c_float, C.c_float, C.c_float, C.c_int]),
    "mfx_als_block_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(mfx_csx), C.POINTER(mfx_coo), C.POINTER(mfx_params), C.c_int32,
                                       C.c_int32, C.c_int]),
    "mfx_als_block_half": (C.c_int, [C.c_int64, C.c_int64, u32p, u32p, f32p, C.c_int64, f32p, f32p, f32p, C.c_int64, C.c_int32,
                                     C.c_float, C.c_int32, C.c_int]),
    "mfx_bpr_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(mfx_csx), C.POINTER(mfx_params), C.c_float, C.c_int64, C.c_uint64,
                                 C.c_int]),
    "mfx_bpr_set_factors": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_bpr_get_factors": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_bpr_steps": (C.c_int, [C.c_void_p, C.c_int64, i64p, f64p]),
    "mfx_bpr_epochs": (C.c_int, [C.c_void_p, C.c_int32, i64p, f64p]),
    "mfx_bpr_position": (C.c_int, [C.c_void_p, i64p]),
    "mfx_bpr_kernel_times": (C.c_int, [C.c_void_p, f64p]),
    "mfx_bpr_destroy": (C.c_int, [C.c_void_p]),
    "mfx_bpr_triples": (C.c_int, [C.c_uint64, C.c_int64, C.c_int64, C.POINTER(mfx_csx), u32p, u32p, u32p, C.c_void_p]),
    "mfx_bpr_apply": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, f32p, f32p, C.c_int64, u32p, u32p, u32p, C.c_void_p, C.c_float,
                                C.c_float, i64p, C.c_int]),
    "mfx_bpr_create_neg": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(mfx_csx), C.POINTER(mfx_params), C.c_float, C.c_int64, C.c_uint64,
                                     C.c_int32, C.c_int64, C.c_void_p, C.c_int]),
    "mfx_bpr_trials": (C.c_int, [C.c_uint64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(mfx_csx), u32p, u32p, u32p, C.c_void_p]),
    "mfx_bpr_rank_weights": (C.c_int, [C.c_int64, C.c_int64, C.c_void_p]),
    "mfx_bpr_apply_neg": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, f32p, f32p, C.c_int64, u32p, u32p, C.c_int64, u32p, C.c_void_p,
                                    C.c_int32, C.c_void_p, C.c_float, C.c_float, i64p, C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_bpr_trial_stats": (C.c_int, [C.c_void_p, i64p]),
    "mfx_lgcn_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(mfx_csx), C.POINTER(mfx_params), C.c_float, C.c_int64, C.c_int32,
                                  C.c_uint64, C.c_int]),
    "mfx_lgcn_set_base": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_lgcn_get_base": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_lgcn_get_factors": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_lgcn_steps": (C.c_int, [C.c_void_p, C.c_int64, i64p, f64p]),
    "mfx_lgcn_epochs": (C.c_int, [C.c_void_p, C.c_int32, i64p, f64p]),
    "mfx_lgcn_position": (C.c_int, [C.c_void_p, i64p]),
    "mfx_lgcn_kernel_times": (C.c_int, [C.c_void_p, f64p]),
    "mfx_lgcn_destroy": (C.c_int, [C.c_void_p]),
    "mfx_lgcn_propagate": (C.c_int, [C.POINTER(mfx_csx), f32p, f32p, C.c_int64, C.c_int32, f32p, f32p, C.c_int]),
    "mfx_lgcn_apply": (C.c_int, [C.POINTER(mfx_csx), C.c_int64, f32p, f32p, C.c_int64, u32p, u32p, u32p, C.c_void_p, C.c_int32,
                                 C.c_float, C.c_float, i64p, C.c_int]),
    "mfx_hyb_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(mfx_csx), C.POINTER(mfx_features), C.POINTER(mfx_features),
                                 C.POINTER(mfx_params), C.c_float, C.c_int64, C.c_uint64, C.c_int]),
    "mfx_hyb_set_embeddings": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_hyb_get_embeddings": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_hyb_get_factors": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_hyb_steps": (C.c_int, [C.c_void_p, C.c_int64, i64p, f64p]),
    "mfx_hyb_epochs": (C.c_int, [C.c_void_p, C.c_int32, i64p, f64p]),
    "mfx_hyb_position": (C.c_int, [C.c_void_p, i64p]),
    "mfx_hyb_kernel_times": (C.c_int, [C.c_void_p, f64p]),
    "mfx_hyb_destroy": (C.c_int, [C.c_void_p]),
    "mfx_hyb_embed": (C.c_int, [C.POINTER(mfx_features), C.c_void_p, C.c_int64, C.c_void_p, C.c_int]),
    "mfx_hyb_apply": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.POINTER(mfx_features), C.POINTER(mfx_features), C.c_void_p, C.c_void_p,
                                C.c_int64, u32p, u32p, u32p, C.c_void_p, C.c_float, C.c_float, i64p, C.c_int]),
    "mfx_knn_build": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(mfx_csx), C.c_int32, C.c_int32, C.c_int, C.c_int]),
    "mfx_knn_create_from_lists": (C.c_int, [C.POINTER(C.c_void_p), C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "mfx_knn_lists": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_knn_neighbours": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_knn_recommend": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_int32,
                                    C.c_void_p, C.c_void_p, i64p, C.c_int]),
    "mfx_knn_times": (C.c_int, [C.c_void_p, f64p]),
    "mfx_knn_destroy": (C.c_int, [C.c_void_p]),
    "mfx_slim_train": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(mfx_csx), C.c_int32, C.c_void_p, C.c_float, C.c_float, C.c_int32, C.c_float,
                                 C.c_int, C.c_int32, i64p, C.c_int, C.c_int]),
    "mfx_slim_gram": (C.c_int, [C.POINTER(mfx_csx), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int, C.c_int]),
    "mfx_slim_solve": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_int32, C.c_float, C.c_int, C.c_void_p,
                                 C.c_void_p, i64p, C.c_int, C.c_int]),
    "mfx_slim_create_from_lists": (C.c_int, [C.POINTER(C.c_void_p), C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "mfx_slim_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_slim_recommend": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_int32,
                                     C.c_void_p, C.c_void_p, i64p, C.c_int]),
    "mfx_slim_times": (C.c_int, [C.c_void_p, f64p]),
    "mfx_slim_destroy": (C.c_int, [C.c_void_p]),
    "mfx_ease_gram": (C.c_int, [C.POINTER(mfx_csx), C.c_float, C.c_int32, C.c_void_p, C.c_int, C.c_int]),
    "mfx_ease_inverse": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "mfx_ease_weights_from_inverse": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "mfx_ease_train": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(mfx_csx), C.c_float, C.c_int, C.c_int32, C.c_int, C.c_int]),
    "mfx_ease_create_from_weights": (C.c_int, [C.POINTER(C.c_void_p), C.c_int64, C.c_void_p, C.c_int, C.c_int]),
    "mfx_ease_weights": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int]),
    "mfx_ease_recommend": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_int32,
                                     C.c_void_p, C.c_void_p, i64p, C.c_int]),
    "mfx_ease_times": (C.c_int, [C.c_void_p, f64p]),
    "mfx_ease_destroy": (C.c_int, [C.c_void_p]),
    "mfx_comm_unique_id": (C.c_int, [C.c_void_p]),
    "mfx_comm_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "mfx_comm_create_local": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int]),
    "mfx_comm_agree": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "mfx_comm_abort": (C.c_int, [C.c_void_p]),
    "mfx_comm_rank": (C.c_int, [C.c_void_p]),
    "mfx_comm_size": (C.c_int, [C.c_void_p]),
    "mfx_comm_destroy": (C.c_int, [C.c_void_p]),
    "mfx_initial_col": (None, [f32p, C.c_int64, C.c_int64]),
    "mfx_partition_rows": (C.c_int, [C.c_int64, u32p, C.c_int, i64p]),
    "mfx_extract_shard": (C.c_int, [C.POINTER(mfx_csx), C.c_int64, C.c_int64, u32p, u32p, f32p, u32p, u32p, f32p]),
    "mfx_rec_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int,
                                 C.POINTER(mfx_csx), C.c_int, C.c_int]),
    "mfx_rec_query": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "mfx_rec_fold_in_setup": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float]),
    "mfx_rec_fold_in": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                  C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_rec_fold_in_block_setup": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_float]),
    "mfx_rec_fold_in_setup_reg": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float]),
    "mfx_rec_fold_in_block_setup_reg": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_int32,
                                                  C.c_float]),
    "mfx_rec_fold_in_block_setup_als": (C.c_int, [C.c_void_p, C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_float]),
    "mfx_rec_fold_in_cg_setup": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int32, C.c_float]),
    "mfx_rec_fold_in_warm": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_rec_fold_in_times": (C.c_int, [C.c_void_p, f64p]),
    "mfx_rec_explain": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_rec_explain_cg": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_rec_explain_times": (C.c_int, [C.c_void_p, f64p]),
    "mfx_rec_set_item_filter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_rec_similar_setup": (C.c_int, [C.c_void_p]),
    "mfx_rec_item_norms": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_rec_similar": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int32, C.c_void_p, C.c_void_p, C.c_int,
                                  C.c_int]),
    "mfx_rec_rank": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "mfx_rec_rank_times": (C.c_int, [C.c_void_p, f64p]),
    "mfx_rec_evaluate": (C.c_int, [C.c_void_p, C.POINTER(mfx_coo), C.c_float, C.c_int32, C.c_void_p, f64p, f64p, f64p, i64p, i64p,
                                   C.c_int]),
    "mfx_rec_query_candidates": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_rec_score": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_rec_candidates_times": (C.c_int, [C.c_void_p, f64p]),
    "mfx_rec_diversify": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_float,
                                    C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "mfx_rec_diversify_times": (C.c_int, [C.c_void_p, f64p]),
    "mfx_rec_ivf_setup": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_rec_ivf_lists": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_rec_ivf_probe": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_rec_query_ivf": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int]),
    "mfx_rec_ivf_times": (C.c_int, [C.c_void_p, f64p]),
    "mfx_rec_destroy": (C.c_int, [C.c_void_p]),
    "mfx_topn_metrics": (C.c_int, [C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(mfx_coo), C.c_float, f64p,
                                   i64p]),
}

_LIB = None
_HIP_RUNTIME = None  # path of the HIP runtime pinned for this process (diagnostics, tests)


def mapped_hip_runtimes() -> list:
    """Distinct libamdhip64 files mapped into this process (more than one = two HIP runtimes)."""
    try:
        with open("/proc/self/maps") as f:
            return sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
    except OSError:
        return []


def _pin_one_hip_runtime() -> None:
    """One HIP runtime per process, whatever the import order.

    PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64 under the SONAME of
    /opt/rocm's (libamdhip64.so.7).  The dynamic loader reuses whichever copy is mapped first for
    every later NEEDED entry with that SONAME, but torch's own libraries ask for the un-versioned
    file name and so always get torch's copy: `import mfx; import torch` used to end with /opt/rocm's
    runtime serving libmfx and torch's serving torch -- two HSA clients in one process, device
    pointers of one unknown to the other, heap corruption at exit (seen on the GPU box, round 1).
    So when torch is installed but not imported yet, its copy is mapped first (RTLD_GLOBAL, exactly
    what torch's own _load_global_deps does); libmfx's NEEDED libamdhip64.so.7 then resolves to it,
    and a later `import torch` finds the file already loaded.  MFX_HIP_RUNTIME=system opts out (for
    processes that will never import torch)."""
    global _HIP_RUNTIME
    import sys
    if os.environ.get("MFX_HIP_RUNTIME", "") == "system":
        return
    already = mapped_hip_runtimes()
    if already:  # torch (or the host program) got there first: libmfx will share that copy
        _HIP_RUNTIME = already[0]
        return
    if "torch" in sys.modules:
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    cand = os.path.join(libdir, "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)
        _HIP_RUNTIME = cand
        # the same for RCCL, lazily: libmfx dlopens it on first use and takes this path first (csrc/comm.cpp)
        rccl = os.path.join(libdir, "librccl.so")
        if os.path.exists(rccl):
            os.environ.setdefault("MFX_RCCL_PATH", rccl)


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise MfxError(f"{LIB_PATH} is missing: build it with `make -C {_PKG} lib` "
                           "(or __graft_entry__.build()); there is no fallback path")
        _pin_one_hip_runtime()
        _LIB = C.CDLL(LIB_PATH)
        two = mapped_hip_runtimes()
        if len(two) > 1:
            raise MfxError("two HIP runtimes are mapped into this process (" + ", ".join(two) + "): libmfx "
                           "would not see the other runtime's device memory; import torch before mfx, or "
                           "set MFX_HIP_RUNTIME=system in processes that never load torch")
        _LIB.mfx_version.restype = C.c_int
        if _LIB.mfx_version() != MFX_VERSION:  # struct layouts / argument lists of another revision: never call into it
            got = _LIB.mfx_version()
            _LIB = None
            raise MfxError(f"{LIB_PATH} speaks ABI revision {got}, this binding revision {MFX_VERSION} "
                           f"(include/mfx.h MFX_VERSION): rebuild with `make -C {_PKG} lib`")
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(_LIB, name)  # AttributeError here == the .so does not export the ABI
            fn.restype = res
            fn.argtypes = args
    return _LIB


def check(rc: int) -> None:
    if rc != 0:
        raise MfxError(f"libmfx error {rc}: {lib().mfx_last_error().decode(errors='replace')}")
