"""ctypes binding of the C ABI in include/cmfrec_hip.h (libcmfrec_hip_{double,float}.so).

The libraries are built in-tree by ``__graft_entry__.build()`` / ``make -C cmfrec_amd/csrc``.
There is no CPU fallback: a missing library or a missing GPU raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CMFREC_HIP_LIBDIR: load the two libraries from another directory (a second build kept beside the default one)
LIBDIR = os.environ.get("CMFREC_HIP_LIBDIR") or os.path.join(_HERE, "lib")

RETURN_CODES = {0: "ok", 1: "out of memory", 2: "invalid or unsupported input", 3: "interrupted",
                4: "HIP runtime failure"}


class Model(C.Structure):
    """``cmfrec_hip_model`` (include/cmfrec_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in (
        "implicit", "m", "n", "k", "k_main", "k_user", "k_item", "user_bias", "item_bias",
        "scale_lam", "scale_lam_sideinfo", "use_cg", "precondition_cg", "max_cg_steps",
        "p", "q", "m_u", "n_i")] + [("lam", C.c_double), ("w_user", C.c_double), ("w_item", C.c_double)] + \
        [(n, C.c_int32) for n in ("row_begin", "row_end", "col_begin", "col_end", "m_x", "n_x")]


class ModelF(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "implicit", "m", "n", "k", "k_main", "k_user", "k_item", "user_bias", "item_bias",
        "scale_lam", "scale_lam_sideinfo", "use_cg", "precondition_cg", "max_cg_steps",
        "p", "q", "m_u", "n_i")] + [("lam", C.c_float), ("w_user", C.c_float), ("w_item", C.c_float)] + \
        [(n, C.c_int32) for n in ("row_begin", "row_end", "col_begin", "col_end", "m_x", "n_x")]


def _newrows_model_fields(real):
    return [(n, C.c_int32) for n in (
        "implicit", "n", "n_max", "include_all_X", "p", "user_bias", "add_implicit_features", "k", "k_user", "k_item", "k_main",
        "scale_lam", "scale_lam_sideinfo", "scale_bias_const", "nonneg", "apply_log_transf")] + \
        [(n, real) for n in ("glob_mean", "lam", "l1_lam", "scaling_biasA", "w_main", "w_user", "w_implicit", "alpha",
                             "w_main_multiplier")] + \
        [(n, C.c_void_p) for n in ("B", "C", "U_colmeans", "biasB", "Bi", "lam_unique", "l1_lam_unique", "BtB", "TransBtBinvBt",
                                   "BiTBi", "TransCtCinvCt")]


class NewRowsModel(C.Structure):
    """``cmfrec_hip_newrows_model`` (include/cmfrec_hip.h), double precision."""
    _fields_ = _newrows_model_fields(C.c_double)


class NewRowsModelF(C.Structure):
    _fields_ = _newrows_model_fields(C.c_float)


class NewRowsModelEx(C.Structure):
    """``cmfrec_hip_newrows_model_ex``: the model followed by the two missing-as-zero options, double precision."""
    _fields_ = [("base", NewRowsModel), ("NA_as_zero_X", C.c_int32), ("NA_as_zero_U", C.c_int32)]


class NewRowsModelExF(C.Structure):
    _fields_ = [("base", NewRowsModelF), ("NA_as_zero_X", C.c_int32), ("NA_as_zero_U", C.c_int32)]


class NewRowsBatch(C.Structure):
    """``cmfrec_hip_newrows_batch``: pointers and counts only, the same layout in both precisions."""
    _fields_ = [("m", C.c_int32), ("m_u", C.c_int32), ("U", C.c_void_p),
                ("U_row", C.c_void_p), ("U_col", C.c_void_p), ("U_sp", C.c_void_p), ("nnz_U", C.c_size_t),
                ("U_csr_p", C.c_void_p), ("U_csr_i", C.c_void_p), ("U_csr", C.c_void_p),
                ("X", C.c_void_p), ("ixA", C.c_void_p), ("ixB", C.c_void_p), ("nnz", C.c_size_t),
                ("Xcsr_p", C.c_void_p), ("Xcsr_i", C.c_void_p), ("Xcsr", C.c_void_p),
                ("Xfull", C.c_void_p), ("weight", C.c_void_p)]


class Errors(C.Structure):
    """``cmfrec_hip_errors`` (include/cmfrec_hip.h): the same layout in both precisions."""
    _fields_ = [("n", C.c_uint64 * 2), ("n_skipped", C.c_uint64)] + \
        [(n, C.c_double * 2) for n in ("sum_w", "sum_we", "sum_wabs", "sum_wsq", "max_abs")]

    def as_dict(self):
        out = {"n": np.array(self.n[:], np.uint64), "n_skipped": np.uint64(self.n_skipped)}
        for name in ("sum_w", "sum_we", "sum_wabs", "sum_wsq", "max_abs"):
            out[name] = np.array(getattr(self, name)[:], np.float64)
        return out


RANK_METRICS = ("hit", "precision", "recall", "ap", "ndcg", "rr", "auc", "mean_rank")     # the order of cmfrec_hip_rank_record
WATCH = {"rmse": 0, "mae": 1}                       # CMFREC_HIP_WATCH_*
WATCH.update({name: 2 + i for i, name in enumerate(RANK_METRICS)})
STEP_IMPROVED, STEP_STOP, STEP_EVALUATE = 1, 2, 4   # CMFREC_HIP_STEP_*


class RankRecord(C.Structure):
    """``cmfrec_hip_rank_record`` (include/cmfrec_hip.h): the same layout in both precisions."""
    _fields_ = [("sum", C.c_double * 8), ("count", C.c_uint64 * 8), ("users", C.c_uint64)]

    def as_dict(self):
        return {"sum": np.array(self.sum[:], np.float64), "count": np.array(self.count[:], np.uint64), "users": np.uint64(self.users)}


class FitMonitor(C.Structure):
    """``cmfrec_hip_fit_monitor`` (include/cmfrec_hip.h): the same layout in both precisions."""
    _fields_ = [("evalset", C.c_void_p), ("rankset", C.c_void_p), ("metric", C.c_int), ("k_at", C.c_int), ("every", C.c_int),
                ("patience", C.c_int), ("restore_best", C.c_int), ("min_delta", C.c_double), ("values", C.POINTER(C.c_double)),
                ("records", C.POINTER(Errors)), ("rank_records", C.POINTER(RankRecord)), ("iters_run", C.POINTER(C.c_int)),
                ("best_iter", C.POINTER(C.c_int))]


class EarlyStop(C.Structure):
    """``cmfrec_hip_early_stop``: the state of ``cmfrec_hip_early_stop_step``."""
    _fields_ = [("every", C.c_int), ("patience", C.c_int), ("higher_is_better", C.c_int), ("min_delta", C.c_double),
                ("best", C.c_double), ("best_iter", C.c_int), ("misses", C.c_int)]


def newrows_model_mirror(dtype):
    return NewRowsModel if np.dtype(dtype) == np.float64 else NewRowsModelF


def newrows_model_ex_mirror(dtype):
    return NewRowsModelEx if np.dtype(dtype) == np.float64 else NewRowsModelExF


EXPORTED = [
    "fit_collective_implicit_als", "fit_collective_explicit_als",
    "factors_collective_explicit_multiple", "factors_collective_implicit_multiple", "cmfrec_hip_factors_multiple", "cmfrec_hip_factors_multiple_l1", "cmfrec_hip_factors_multiple_ex",
    "cmfrec_hip_optimizeA_implicit", "cmfrec_hip_optimizeA_explicit", "cmfrec_hip_optimizeA_explicit_weighted",
    "cmfrec_hip_optimizeA_dense_full", "cmfrec_hip_optimizeA_collective", "cmfrec_hip_optimizeA_collective_sparse", "cmfrec_hip_topN_batch",
    "cmfrec_hip_ranker_create", "cmfrec_hip_ranker_topN", "cmfrec_hip_ranker_topN_candidates", "cmfrec_hip_topN_candidates_batch", "cmfrec_hip_ranker_ranks", "cmfrec_hip_ranks_batch", "cmfrec_hip_ranker_kernel_ms", "cmfrec_hip_ranker_launch_shape", "cmfrec_hip_ranker_destroy",
    "cmfrec_hip_ranker_similar", "cmfrec_hip_similar_batch", "cmfrec_hip_ranker_inverse_norms",
    "cmfrec_hip_ranker_topN_deep", "cmfrec_hip_ranker_topN_after", "cmfrec_hip_topN_deep_batch", "cmfrec_hip_ranker_pages",
    "cmfrec_hip_ranker_set_split", "cmfrec_hip_ranker_slices", "cmfrec_hip_topn_split_plan", "cmfrec_hip_newrows_set_split",
    "cmfrec_hip_scorer_create", "cmfrec_hip_scorer_predict", "cmfrec_hip_scorer_kernel_ms", "cmfrec_hip_scorer_destroy", "cmfrec_hip_score_pairs",
    "cmfrec_hip_evalset_create", "cmfrec_hip_evalset_kernel_ms", "cmfrec_hip_evalset_launch_waves", "cmfrec_hip_evalset_destroy", "cmfrec_hip_scorer_errors", "cmfrec_hip_session_errors", "cmfrec_hip_pair_errors",
    "cmfrec_hip_session_snapshot", "cmfrec_hip_session_restore", "cmfrec_hip_fit_set_monitor", "cmfrec_hip_early_stop_step",
    "cmfrec_hip_rankset_create", "cmfrec_hip_rankset_destroy", "cmfrec_hip_ranker_metrics", "cmfrec_hip_session_ranking",
    "cmfrec_hip_sizeof_newrows_model", "cmfrec_hip_newrows_create", "cmfrec_hip_newrows_factors", "cmfrec_hip_newrows_topN", "cmfrec_hip_newrows_topN_candidates", "cmfrec_hip_newrows_ranks", "cmfrec_hip_newrows_impute", "cmfrec_hip_newrows_predict", "cmfrec_hip_newrows_kernel_ms", "cmfrec_hip_newrows_destroy", "cmfrec_hip_factors_multiple_naz", "cmfrec_hip_sizeof_newrows_model_ex", "cmfrec_hip_newrows_create_ex", "cmfrec_hip_newrows_naz_launch_waves",
    "cmfrec_hip_session_create", "cmfrec_hip_session_destroy", "cmfrec_hip_last_error", "cmfrec_hip_last_error_code",
    "cmfrec_hip_session_set_X", "cmfrec_hip_session_set_A_parts", "cmfrec_hip_session_nparts", "cmfrec_hip_session_part_range", "cmfrec_hip_session_stream_wait_part", "cmfrec_hip_session_set_X_coo", "cmfrec_hip_session_set_X_coo_weighted", "cmfrec_hip_session_set_X_weighted", "cmfrec_hip_session_set_X_coo_device", "cmfrec_hip_session_precompute", "cmfrec_hip_session_init_biases", "cmfrec_hip_session_get_X", "cmfrec_hip_session_set_factors", "cmfrec_hip_session_get_factors",
    "cmfrec_hip_session_set_sideinfo", "cmfrec_hip_session_set_sideinfo_local", "cmfrec_hip_session_sideinfo_partial", "cmfrec_hip_session_sideinfo_finish", "cmfrec_hip_session_set_nonneg", "cmfrec_hip_session_set_l1", "cmfrec_hip_session_set_lam_unique", "cmfrec_hip_session_set_scale_bias_const", "cmfrec_hip_session_set_NA_as_zero_X", "cmfrec_hip_session_set_zero_rows", "cmfrec_hip_session_set_closed_form_rows", "cmfrec_hip_session_set_lambda_multipliers", "cmfrec_hip_session_set_implicit_features", "cmfrec_hip_session_get_implicit_features", "cmfrec_hip_session_set_sideinfo_sparse", "cmfrec_hip_session_set_sideinfo_sparse_zeros", "cmfrec_hip_side_zeros_products", "cmfrec_hip_session_update", "cmfrec_hip_session_iterate",
    "cmfrec_hip_session_sync", "cmfrec_hip_session_device_ptr", "cmfrec_hip_session_stream",
    "cmfrec_hip_session_after_gather", "cmfrec_hip_session_kernel_time",
    "cmfrec_hip_session_reset_timers", "cmfrec_hip_session_bin_overlaps", "cmfrec_hip_session_vh_mode", "cmfrec_hip_session_vh_min", "cmfrec_hip_session_lowrank_info", "cmfrec_hip_session_bin_stats", "cmfrec_hip_sizeof_real", "cmfrec_hip_sizeof_model", "cmfrec_hip_build_info", "cmfrec_hip_reload_switches", "cmfrec_hip_selftest_lanes", "cmfrec_hip_exchange_plan", "cmfrec_hip_gemm_probe", "cmfrec_hip_dense_rows_probe", "cmfrec_hip_sym_eig", "cmfrec_hip_dense_op", "cmfrec_hip_impute_dense", "precompute_collective_explicit", "precompute_collective_implicit", "topN_old_collective_explicit", "topN_old_collective_implicit", "cmfrec_hip_random_parallel",
]

# the reference's own names outside the prefixes tests/test_abi.py compares with the header (include/cmfrec_hip.h declares them,
# exports.map exports them)
EXPORTED_OTHER = ["impute_X_collective_explicit", "predict_X_old_collective_explicit", "predict_X_old_collective_implicit",
                  "predict_X_new_collective_explicit", "predict_X_new_collective_implicit"]

_cache = {}


def lib_path(dtype):
    suffix = "double" if np.dtype(dtype) == np.float64 else "float"
    return os.path.join(LIBDIR, "libcmfrec_hip_%s.so" % suffix)


def load(dtype=np.float64):
    """Returns the ctypes handle of the library for ``dtype`` (float64 / float32)."""
    dtype = np.dtype(dtype).type
    if dtype not in (np.float64, np.float32):
        raise ValueError("dtype must be float64 or float32")
    if dtype in _cache:
        return _cache[dtype]
    path = lib_path(dtype)
    if not os.path.exists(path):
        raise ImportError(
            "%s is missing: the HIP extension has not been built (run __graft_entry__.build() or "
            "`make -C cmfrec_amd/csrc`). cmfrec_amd has no CPU fallback." % path)
    # PyTorch ships its own HIP runtime under the same soname as /opt/rocm's.  Whichever is mapped first serves the whole
    # process; if this library's copy came first, a later `import torch` would run on a runtime its other libraries were not
    # built against ("No HIP GPUs are available").  The package uses torch for device memory and streams anyway, so it goes
    # first whenever it is installed.
    # A process that will never import torch can skip this (seconds of import time, torch's HIP runtime initialised):
    # CMFREC_AMD_NO_TORCH_PRELOAD=1.  The ordering requirement then is the caller's: torch, if it comes at all, before this library.
    if os.environ.get("CMFREC_AMD_NO_TORCH_PRELOAD") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    lib = C.CDLL(path)
    lib.cmfrec_hip_last_error.restype = C.c_char_p
    lib.cmfrec_hip_build_info.restype = C.c_char_p
    lib.cmfrec_hip_session_create.restype = C.c_void_p
    lib.cmfrec_hip_ranker_create.restype = C.c_void_p
    lib.cmfrec_hip_ranker_destroy.restype = None
    lib.cmfrec_hip_ranker_ranks.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int] + [C.c_void_p] * 7
    lib.cmfrec_hip_ranks_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int] + [C.c_void_p] * 8
    lib.cmfrec_hip_ranker_similar.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.cmfrec_hip_similar_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_int, C.c_void_p, C.c_void_p]
    lib.cmfrec_hip_ranker_inverse_norms.argtypes = [C.c_void_p, C.c_void_p]
    lib.cmfrec_hip_ranker_topN_deep.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.cmfrec_hip_ranker_topN_after.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p]
    lib.cmfrec_hip_topN_deep_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int] + [C.c_void_p] * 3 + \
        [C.c_int, C.c_void_p, C.c_void_p]
    lib.cmfrec_hip_ranker_pages.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.cmfrec_hip_ranker_set_split.argtypes = [C.c_void_p, C.c_int]
    lib.cmfrec_hip_ranker_slices.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    lib.cmfrec_hip_topn_split_plan.argtypes = [C.c_int] * 5 + [C.c_size_t, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.cmfrec_hip_newrows_set_split.argtypes = [C.c_void_p, C.c_int]
    nrm = newrows_model_mirror(dtype)
    lib.cmfrec_hip_newrows_create.restype = C.c_void_p
    lib.cmfrec_hip_newrows_create.argtypes = [C.POINTER(nrm), C.c_int]
    lib.cmfrec_hip_newrows_factors.argtypes = [C.c_void_p, C.POINTER(NewRowsBatch), C.c_void_p, C.c_void_p]
    nrx = newrows_model_ex_mirror(dtype)
    lib.cmfrec_hip_newrows_naz_launch_waves.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    lib.cmfrec_hip_newrows_create_ex.restype = C.c_void_p
    lib.cmfrec_hip_newrows_create_ex.argtypes = [C.POINTER(nrx), C.c_int]
    lib.cmfrec_hip_factors_multiple_naz.argtypes = [C.POINTER(nrx), C.POINTER(NewRowsBatch), C.c_void_p, C.c_void_p]
    lib.cmfrec_hip_newrows_topN.argtypes = [C.c_void_p, C.POINTER(NewRowsBatch), C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.cmfrec_hip_newrows_topN_candidates.argtypes = [C.c_void_p, C.POINTER(NewRowsBatch), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                       C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.cmfrec_hip_newrows_ranks.argtypes = [C.c_void_p, C.POINTER(NewRowsBatch), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.cmfrec_hip_newrows_impute.argtypes = [C.c_void_p, C.POINTER(NewRowsBatch), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.impute_X_collective_explicit.restype = C.c_int
    lib.cmfrec_hip_impute_dense.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                            C.c_void_p, real(dtype), C.c_void_p, C.c_size_t, C.c_void_p]
    lib.cmfrec_hip_newrows_predict.argtypes = [C.c_void_p, C.POINTER(NewRowsBatch), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                               C.c_void_p, C.c_void_p]
    R = real(dtype)
    lib.cmfrec_hip_score_pairs.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                           C.c_int, C.c_void_p, R, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.cmfrec_hip_scorer_create.restype = C.c_void_p
    lib.cmfrec_hip_scorer_create.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p,
                                             C.c_void_p, R, C.c_int, C.c_int]
    lib.cmfrec_hip_scorer_predict.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.cmfrec_hip_scorer_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    lib.cmfrec_hip_scorer_destroy.restype = None
    lib.cmfrec_hip_scorer_destroy.argtypes = [C.c_void_p]
    lib.cmfrec_hip_evalset_create.restype = C.c_void_p
    lib.cmfrec_hip_evalset_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    lib.cmfrec_hip_evalset_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    lib.cmfrec_hip_evalset_launch_waves.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
    lib.cmfrec_hip_evalset_destroy.restype = None
    lib.cmfrec_hip_evalset_destroy.argtypes = [C.c_void_p]
    lib.cmfrec_hip_scorer_errors.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Errors)]
    lib.cmfrec_hip_session_errors.argtypes = [C.c_void_p, C.c_void_p, R, C.POINTER(Errors)]
    lib.cmfrec_hip_session_snapshot.argtypes = [C.c_void_p]
    lib.cmfrec_hip_session_restore.argtypes = [C.c_void_p]
    lib.cmfrec_hip_fit_set_monitor.argtypes = [C.POINTER(FitMonitor)]
    lib.cmfrec_hip_rankset_create.restype = C.c_void_p
    lib.cmfrec_hip_rankset_create.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int]
    lib.cmfrec_hip_rankset_destroy.restype = None
    lib.cmfrec_hip_rankset_destroy.argtypes = [C.c_void_p]
    lib.cmfrec_hip_ranker_metrics.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_int, C.POINTER(RankRecord),
                                              C.c_void_p, C.c_void_p]
    lib.cmfrec_hip_session_ranking.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(RankRecord)]
    lib.cmfrec_hip_early_stop_step.argtypes = [C.POINTER(EarlyStop), C.c_int, C.c_int, C.POINTER(C.c_double)]
    lib.cmfrec_hip_pair_errors.argtypes = lib.cmfrec_hip_score_pairs.argtypes[:-1] + [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Errors)]
    for name in EXPORTED_OTHER[1:]:
        getattr(lib, name).restype = C.c_int
    lib.cmfrec_hip_newrows_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.cmfrec_hip_newrows_destroy.restype = None
    lib.cmfrec_hip_newrows_destroy.argtypes = [C.c_void_p]
    lib.cmfrec_hip_session_device_ptr.restype = C.c_void_p
    lib.cmfrec_hip_session_stream.restype = C.c_void_p
    assert lib.cmfrec_hip_sizeof_real() == np.dtype(dtype).itemsize
    mirror = Model if dtype is np.float64 else ModelF
    if lib.cmfrec_hip_sizeof_model() != C.sizeof(mirror):
        raise RuntimeError("cmfrec_amd: the ctypes mirror of cmfrec_hip_model (%d bytes) does not match the library (%d)"
                           % (C.sizeof(mirror), lib.cmfrec_hip_sizeof_model()))
    if lib.cmfrec_hip_sizeof_newrows_model_ex() != C.sizeof(nrx):
        raise RuntimeError("cmfrec_amd: the ctypes mirror of cmfrec_hip_newrows_model_ex (%d bytes) does not match the library (%d)"
                           % (C.sizeof(nrx), lib.cmfrec_hip_sizeof_newrows_model_ex()))
    if lib.cmfrec_hip_sizeof_newrows_model() != C.sizeof(nrm):
        raise RuntimeError("cmfrec_amd: the ctypes mirror of cmfrec_hip_newrows_model (%d bytes) does not match the library (%d)"
                           % (C.sizeof(nrm), lib.cmfrec_hip_sizeof_newrows_model()))
    _cache[dtype] = lib
    return lib


def real(dtype):
    return C.c_double if np.dtype(dtype) == np.float64 else C.c_float


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def check(rc, lib, what, interrupt_ok=False):
    if rc == 0 or (rc == 3 and interrupt_ok):
        return
    msg = lib.cmfrec_hip_last_error()
    msg = msg.decode() if msg else ""
    if rc == 1:
        raise MemoryError("%s: out of memory. %s" % (what, msg))
    if rc == 3:
        raise InterruptedError("%s: procedure was interrupted" % what)
    raise RuntimeError("%s failed with code %d (%s). %s" % (what, rc, RETURN_CODES.get(rc, "?"), msg))
