"""The refusals of the two fit drivers (cmfrec_amd/csrc/fit.hip), no device: every input below is turned away with return code 2
and one message on stderr (verbose = true) before the driver creates a session, so nothing here calls HIP as long as
CMFREC_HIP_DEVICES and CMFREC_HIP_SHARDED are unset.  The table pins the wording AND the order of the checks: the precedence cases
break two rules at once and say which message wins.

Messages that cannot be reached without a device, and so are not in the table:
  * "NA_as_zero_U / NA_as_zero_I on several devices runs on the zero-filled dense matrix ... not implemented at this size" (both
    drivers): needs a sharded fit, i.e. CMFREC_HIP_DEVICES, which is read through hipGetDeviceCount.
  * "... session create failed"-style lines: printed after cmfrec_hip_session_create, not by fail().
Not in the table either: NA_as_zero_U / _I with NULL triplet pointers and nnz > 0 -- the parent of the shared intake read the NULL
row array (rows_without_data) before ZeroFilledSide::build could refuse it; tests/c_caller/fit_inputs_san.cpp covers it.
"""
import ctypes as C

import numpy as np
import pytest

from cmfrec_amd import _lib

NAN = float("nan")

# (name, kind) in the positional order of the C signature (include/cmfrec_hip.h; cmfrec_amd/models.py makes the same calls)
IMPLICIT_ARGS = [
    ("A", "ptr"), ("B", "ptr"), ("C", "ptr"), ("D", "ptr"), ("reset_values", "bool"), ("seed", "int"),
    ("U_colmeans", "ptr"), ("I_colmeans", "ptr"), ("m", "int"), ("n", "int"), ("k", "int"),
    ("ixA", "iptr"), ("ixB", "iptr"), ("X", "ptr"), ("nnz", "size"),
    ("lam", "real"), ("lam_unique", "ptr"), ("l1_lam", "real"), ("l1_lam_unique", "ptr"),
    ("U", "ptr"), ("m_u", "int"), ("p", "int"), ("II", "ptr"), ("n_i", "int"), ("q", "int"),
    ("U_row", "iptr"), ("U_col", "iptr"), ("U_sp", "ptr"), ("nnz_U", "size"),
    ("I_row", "iptr"), ("I_col", "iptr"), ("I_sp", "ptr"), ("nnz_I", "size"),
    ("NA_as_zero_U", "bool"), ("NA_as_zero_I", "bool"), ("k_main", "int"), ("k_user", "int"), ("k_item", "int"),
    ("w_main", "real"), ("w_user", "real"), ("w_item", "real"), ("w_main_multiplier", "ptr"),
    ("alpha", "real"), ("adjust_weight", "bool"), ("apply_log_transf", "bool"), ("niter", "int"), ("nthreads", "int"),
    ("verbose", "bool"), ("handle_interrupt", "bool"), ("use_cg", "bool"), ("max_cg_steps", "int"), ("precondition_cg", "bool"),
    ("finalize_chol", "bool"), ("nonneg", "bool"), ("max_cd_steps", "int"), ("nonneg_C", "bool"), ("nonneg_D", "bool"),
    ("precompute_for_predictions", "bool"), ("precomputedBtB", "ptr"), ("precomputedBeTBe", "ptr"),
    ("precomputedBeTBeChol", "ptr"), ("precomputedCtUbias", "ptr"),
]
EXPLICIT_ARGS = [
    ("biasA", "ptr"), ("biasB", "ptr"), ("A", "ptr"), ("B", "ptr"), ("C", "ptr"), ("D", "ptr"), ("Ai", "ptr"), ("Bi", "ptr"),
    ("add_implicit_features", "bool"), ("reset_values", "bool"), ("seed", "int"), ("glob_mean", "ptr"),
    ("U_colmeans", "ptr"), ("I_colmeans", "ptr"), ("m", "int"), ("n", "int"), ("k", "int"),
    ("ixA", "iptr"), ("ixB", "iptr"), ("X", "ptr"), ("nnz", "size"), ("Xfull", "ptr"), ("weight", "ptr"),
    ("user_bias", "bool"), ("item_bias", "bool"), ("center", "bool"), ("lam", "real"), ("lam_unique", "ptr"),
    ("l1_lam", "real"), ("l1_lam_unique", "ptr"), ("scale_lam", "bool"), ("scale_lam_sideinfo", "bool"), ("scale_bias_const", "bool"),
    ("scaling_biasA", "ptr"), ("scaling_biasB", "ptr"), ("U", "ptr"), ("m_u", "int"), ("p", "int"), ("II", "ptr"), ("n_i", "int"), ("q", "int"),
    ("U_row", "iptr"), ("U_col", "iptr"), ("U_sp", "ptr"), ("nnz_U", "size"), ("I_row", "iptr"), ("I_col", "iptr"), ("I_sp", "ptr"), ("nnz_I", "size"),
    ("NA_as_zero_X", "bool"), ("NA_as_zero_U", "bool"), ("NA_as_zero_I", "bool"), ("k_main", "int"), ("k_user", "int"), ("k_item", "int"),
    ("w_main", "real"), ("w_user", "real"), ("w_item", "real"), ("w_implicit", "real"), ("niter", "int"), ("nthreads", "int"),
    ("verbose", "bool"), ("handle_interrupt", "bool"), ("use_cg", "bool"), ("max_cg_steps", "int"), ("precondition_cg", "bool"), ("finalize_chol", "bool"),
    ("nonneg", "bool"), ("max_cd_steps", "int"), ("nonneg_C", "bool"), ("nonneg_D", "bool"), ("precompute_for_predictions", "bool"),
    ("include_all_X", "bool"), ("B_plus_bias", "ptr"), ("precomputedBtB", "ptr"), ("precomputedTransBtBinvBt", "ptr"),
    ("precomputedBtXbias", "ptr"), ("precomputedBeTBeChol", "ptr"), ("precomputedBiTBi", "ptr"),
    ("precomputedTransCtCinvCt", "ptr"), ("precomputedCtCw", "ptr"), ("precomputedCtUbias", "ptr"),
]
BIG = 4096          # every output buffer: larger than any case needs (a refused fit writes at most the column means)


def _defaults(implicit):
    """m = 4, n = 3, k = 2, five entries of X, no side information; every output buffer present."""
    d = dict(A=np.zeros(BIG), B=np.zeros(BIG), C=np.zeros(BIG), D=np.zeros(BIG), reset_values=True, seed=1,
             U_colmeans=np.zeros(8), I_colmeans=np.zeros(8), m=4, n=3, k=2,
             ixA=[0, 1, 2, 3, 0], ixB=[0, 1, 2, 0, 2], X=[1., 2., 3., 4., 5.], nnz=5,
             lam=0.1, lam_unique=None, l1_lam=0., l1_lam_unique=None, U=None, m_u=0, p=0, II=None, n_i=0, q=0,
             U_row=None, U_col=None, U_sp=None, nnz_U=0, I_row=None, I_col=None, I_sp=None, nnz_I=0,
             NA_as_zero_U=False, NA_as_zero_I=False, k_main=0, k_user=0, k_item=0, w_main=1., w_user=1., w_item=1.,
             niter=1, nthreads=1, verbose=True, handle_interrupt=False, use_cg=False, max_cg_steps=3, precondition_cg=False,
             finalize_chol=False, nonneg=False, max_cd_steps=100, nonneg_C=False, nonneg_D=False, precompute_for_predictions=False,
             precomputedBtB=np.zeros(BIG), precomputedBeTBeChol=np.zeros(BIG), precomputedCtUbias=np.zeros(BIG))
    if implicit:
        d.update(w_main_multiplier=np.zeros(1), alpha=1., adjust_weight=False, apply_log_transf=False, precomputedBeTBe=np.zeros(BIG))
    else:
        d.update(biasA=np.zeros(BIG), biasB=np.zeros(BIG), Ai=np.zeros(BIG), Bi=np.zeros(BIG), add_implicit_features=False,
                 glob_mean=np.zeros(1), Xfull=None, weight=None, user_bias=False, item_bias=False, center=True, scale_lam=False,
                 scale_lam_sideinfo=False, scale_bias_const=False, scaling_biasA=np.zeros(1), scaling_biasB=np.zeros(1),
                 NA_as_zero_X=False, w_implicit=0.5, include_all_X=True, B_plus_bias=np.zeros(BIG),
                 precomputedTransBtBinvBt=np.zeros(BIG), precomputedBtXbias=np.zeros(BIG), precomputedBiTBi=np.zeros(BIG),
                 precomputedTransCtCinvCt=np.zeros(BIG), precomputedCtCw=np.zeros(BIG))
    return d


def _call(implicit, dtype, overrides):
    """One call of the driver with the defaults plus `overrides`; returns (return code, the arguments as passed)."""
    lib = _lib.load(dtype)
    R = _lib.real(dtype)
    spec = IMPLICIT_ARGS if implicit else EXPLICIT_ARGS
    vals = _defaults(implicit)
    unknown = set(overrides) - set(vals)
    assert not unknown, unknown
    vals.update(overrides)
    assert set(vals) == {name for name, _ in spec}
    args = []
    for name, kind in spec:
        v = vals[name]
        if kind in ("ptr", "iptr"):
            if v is not None:
                v = vals[name] = np.ascontiguousarray(v, np.int32 if kind == "iptr" else dtype)
            args.append(_lib.ptr(v))
        else:
            args.append({"bool": C.c_bool, "int": C.c_int, "size": C.c_size_t, "real": R}[kind](v))
    fn = lib.fit_collective_implicit_als if implicit else lib.fit_collective_explicit_als
    fn.restype = C.c_int
    return fn(*args), vals


# ---- side information of the tiny problem: p = q = 2 ----
def dense_U(rows=4, nan=None):
    U = np.arange(1., 2 * rows + 1).reshape(rows, 2)
    if nan == "all": U[:] = NAN
    elif nan is not None: U[nan] = NAN
    return dict(U=U, m_u=rows, p=2)


def dense_I(rows=3, nan=None):
    II = np.arange(1., 2 * rows + 1).reshape(rows, 2) / 2
    if nan == "all": II[:] = NAN
    elif nan is not None: II[nan] = NAN
    return dict(II=II, n_i=rows, q=2)


def sparse_U(rows=4, row=(0, 1, 3), col=(0, 1, 0), val=(1., 2., 3.)):
    return dict(U_row=row, U_col=col, U_sp=val, nnz_U=len(col), m_u=rows, p=2)


def sparse_I(rows=3, row=(0, 2), col=(1, 0), val=(1.5, -2.)):
    return dict(I_row=row, I_col=col, I_sp=val, nnz_I=len(col), n_i=rows, q=2)


def Xfull(nan=(), all_nan=False):
    X = np.arange(1., 13.).reshape(4, 3)
    for pos in nan: X[pos] = NAN
    if all_nan: X[:] = NAN
    return dict(Xfull=X)


TINY_LIMIT = {"CMFREC_HIP_ZEROFILL_MAX_GB": "1e-9"}        # one byte: every zero-filled matrix is "beyond" it
BAD_X = dict(ixA=[0, 1, 2, 9, 0])                          # a later refusal, to show that an earlier stage let the input through

M_K_USER = "Cannot pass 'k_user' without U data."
M_K_ITEM = "Cannot pass 'k_item' without I data."
M_K_MAIN = "Cannot pass 'k_main' without X data."
M_NO_X = "cmfrec_hip: the implicit model needs at least one entry of X."
M_NAZ_NAN = "cmfrec_hip: NA_as_zero_%s beyond CMFREC_HIP_ZEROFILL_MAX_GB: NaN among the values of %s is not implemented."
M_NAZ_ROWS_U = "cmfrec_hip: NA_as_zero_U with more rows of U than X is not implemented."
M_NAZ_ROWS_I = "cmfrec_hip: NA_as_zero_I with more rows of I than X has columns is not implemented."
M_IX = "cmfrec_hip: %s index out of range."
M_U_EMPTY = "cmfrec_hip: U has no present entries."
M_COO = "cmfrec_hip: sparse side information must be COO triplets with rows inside X."
M_L1_BEYOND = "cmfrec_hip: L1 together with side information beyond X is not implemented."
M_NAN_NONNEG = "cmfrec_hip: NaN in dense side information: not together with nonneg / L1."
M_PRE_BUF = "cmfrec_hip: precompute_for_predictions needs the output buffers (cmfrec.h.in:760-778)."
M_DIMS = "cmfrec_hip: invalid dimensions."
M_DX_MODEL = "cmfrec_hip: dense X is implemented for the model without implicit features and NA_as_zero_X."
M_DX_SIDE_W = "cmfrec_hip: dense X with side information: not together with observation weights or NA_as_zero_U / _I."
M_DX_SIDE_ROWS = "cmfrec_hip: dense X with side information: U / I must have exactly the rows / columns of X."
M_DX_EMPTY = "cmfrec_hip: 'X' has all entries missing."
M_DX_FEW = ("cmfrec_hip: dense X whose rows / columns miss only a few entries, under scale_lam together with "
            "scale_lam_sideinfo / scale_bias_const and both biases, is not implemented (its per-row lambda "
            "multipliers ride on the weighted kernels, whose bias start values do not restate those options).")
M_DX_NAN = "cmfrec_hip: dense X with side information: NaN in U / I is not implemented."
M_NAZX_MODEL = "cmfrec_hip: NA_as_zero_X is implemented for the model without nonneg / L1 and scale_bias_const."
M_NAZX_PRE = "cmfrec_hip: NA_as_zero_X with precompute_for_predictions: the model without side information and implicit features."
M_NAZX_SP_NAZ = "cmfrec_hip: NA_as_zero_X with sparse side information: not together with NA_as_zero_U / _I."
M_NAZX_ROWS = "cmfrec_hip: NA_as_zero_X with side information: U / I must have exactly the rows / columns of X."
M_NAZX_W_BIAS = ("cmfrec_hip: NA_as_zero_X with observation weights: pass start values for the biases (reset_values = false); "
                 "the reference's own start values are not defined for this combination.")
M_NAZX_W_CG = "cmfrec_hip: NA_as_zero_X with observation weights under CG: k + k_main + bias <= 64 (precondition_cg takes more)."
M_NAZX_NAN = "cmfrec_hip: NA_as_zero_X with side information: NaN in %s is not implemented."
M_IMP_OUT = "cmfrec_hip: add_implicit_features needs the Ai and Bi outputs."
M_IMP_BEYOND = "cmfrec_hip: implicit features with side information beyond X are not implemented."
M_IMP_PRE = "cmfrec_hip: implicit features: precompute_for_predictions is not implemented."
M_IMP_NONNEG = "cmfrec_hip: implicit features with nonneg / L1 are not implemented."
M_IMP_W = "cmfrec_hip: w_implicit must be positive."
M_W_SP = ("cmfrec_hip: observation weights with sparse side information under scale_lam_sideinfo are not implemented "
          "(the reference's lambda multipliers for this combination read a value of U / I in place of a row pointer).")
M_W_OTHER = ("cmfrec_hip: observation weights together with NaN side information / scale_lam_sideinfo / "
             "scale_bias_const are not implemented.")
M_SBC_MODEL = "cmfrec_hip: scale_bias_const with implicit features / sparse or NaN side information is not implemented."
M_SBC_ITEM = ("cmfrec_hip: scale_bias_const with only an item bias and the Cholesky solver: the reference leaves "
              "scaling_biasB unset (collective.c:7934).")
M_SBC_OUT = "cmfrec_hip: scale_bias_const needs the scaling_biasA / scaling_biasB outputs."

W5 = dict(weight=[1., 2., 1., .5, 1.])                     # one weight per entry of the sparse X

# what both drivers refuse in the same words: (id, overrides, environment, message)
SHARED = [
    ("k_user", dict(k_user=1), {}, M_K_USER),
    ("k_item", dict(k_item=1), {}, M_K_ITEM),
    # ---- zero-filled intake, U then I ----
    ("naz_U_nan_beyond_limit", dict(NA_as_zero_U=True, **sparse_U(val=(1., NAN, 3.))), TINY_LIMIT, M_NAZ_NAN % ("U", "U")),
    ("naz_I_nan_beyond_limit", dict(NA_as_zero_I=True, **sparse_I(val=(NAN, 1.))), TINY_LIMIT, M_NAZ_NAN % ("I", "I")),
    ("naz_U_more_rows", dict(NA_as_zero_U=True, **sparse_U(rows=5)), {}, M_NAZ_ROWS_U),
    ("naz_I_more_rows", dict(NA_as_zero_I=True, **sparse_I(rows=4)), {}, M_NAZ_ROWS_I),
    ("naz_U_index", dict(NA_as_zero_U=True, **sparse_U(col=(0, 5, 0))), {}, M_IX % "U"),
    ("naz_I_index", dict(NA_as_zero_I=True, **sparse_I(row=(0, -1))), {}, M_IX % "I"),
    ("naz_U_index_beyond_limit", dict(NA_as_zero_U=True, **sparse_U(row=(0, 4, 3))), TINY_LIMIT, M_IX % "U"),
    ("naz_I_index_beyond_limit", dict(NA_as_zero_I=True, **sparse_I(col=(1, 2))), TINY_LIMIT, M_IX % "I"),
    ("naz_U_no_columns", dict(NA_as_zero_U=True, **dict(sparse_U(), p=0)), {}, M_IX % "U"),
    # more rows than X wins over the size limit and over a bad index
    ("naz_U_more_rows_first", dict(NA_as_zero_U=True, **sparse_U(rows=5, col=(0, 5, 0))), TINY_LIMIT, M_NAZ_ROWS_U),
    # U is taken in before I
    ("naz_U_before_naz_I", dict(NA_as_zero_U=True, NA_as_zero_I=True, **sparse_U(col=(0, 5, 0)), **sparse_I(rows=4)), {}, M_IX % "U"),
    # beyond the limit on one device the fit goes on with the triplets: the next refusal is a later one
    ("naz_I_beyond_limit_goes_on", dict(NA_as_zero_I=True, **sparse_I(), **BAD_X), TINY_LIMIT, M_IX % "X"),
    ("naz_U_beyond_limit_goes_on", dict(NA_as_zero_U=True, **sparse_U(), **BAD_X), TINY_LIMIT, M_IX % "X"),
    ("naz_U_repeated_positions_go_on", dict(NA_as_zero_U=True, **sparse_U(row=(1, 1, 1), col=(0, 0, 0)), **BAD_X), {}, M_IX % "X"),
    # ---- NaN intake ----
    ("U_all_nan", dense_U(nan="all"), {}, M_U_EMPTY),
    # the asymmetry: an all-NaN I is not refused for being empty -- it counts as NaN side information (column means NaN) and the
    # fit goes on without I
    ("I_all_nan_nonneg", dict(nonneg=True, **dense_I(nan="all")), {}, M_NAN_NONNEG),
    ("I_all_nan_goes_on", dict(**dense_I(nan="all"), **BAD_X), {}, M_IX % "X"),
    # a quirk, pinned as it is: "nothing left of U" is tested with the NaN flag of EITHER side, so a U that runs on its triplets
    # beyond the zero-fill limit (no dense pointer, no count left) is refused as empty once I has NaN; below the limit it is not
    ("naz_U_on_triplets_and_I_nan", dict(NA_as_zero_U=True, **sparse_U(), **dense_I(nan=(0, 0))), TINY_LIMIT, M_U_EMPTY),
    ("naz_U_zero_filled_and_I_nan", dict(NA_as_zero_U=True, **sparse_U(), **dense_I(nan=(0, 0)), **BAD_X), {}, M_IX % "X"),
    ("U_all_nan_before_I",dict(**dense_U(nan="all"), **sparse_I(row=None)), {}, M_U_EMPTY),
    # ---- triplets ----
    ("U_triplets_null", sparse_U(row=None), {}, M_COO),
    ("I_triplets_null", sparse_I(val=None), {}, M_COO),
    ("U_sparse_rows_beyond_X", sparse_U(rows=5), {}, M_COO),
    ("I_sparse_rows_beyond_X", sparse_I(rows=4), {}, M_COO),
    ("U_index", sparse_U(col=(0, 5, 0)), {}, M_IX % "U"),
    ("U_index_row", sparse_U(row=(0, 4, 3)), {}, M_IX % "U"),
    ("I_index", sparse_I(row=(0, 3)), {}, M_IX % "I"),
    ("U_index_before_I_index", dict(**sparse_U(col=(0, -1, 0)), **sparse_I(col=(1, 2))), {}, M_IX % "U"),
    # both sides are checked for their shape before either is checked for its indices
    ("U_index_and_I_triplets_null", dict(**sparse_U(col=(0, 5, 0)), **sparse_I(row=None)), {}, M_COO),
    ("naz_U_index_and_I_triplets_null", dict(NA_as_zero_U=True, **sparse_U(col=(0, 5, 0)), **sparse_I(row=None)), {}, M_IX % "U"),
    # ---- what follows the intake ----
    ("l1_U_beyond_X", dict(l1_lam=0.1, **dense_U(rows=5)), {}, M_L1_BEYOND),
    ("l1_unique_I_beyond_X", dict(l1_lam_unique=np.zeros(6), **dense_I(rows=4)), {}, M_L1_BEYOND),
    ("index_before_l1_beyond", dict(l1_lam=0.1, **dense_U(rows=5), **sparse_I(col=(1, 2))), {}, M_IX % "I"),
    ("U_nan_nonneg", dict(nonneg=True, **dense_U(nan=(1, 0))), {}, M_NAN_NONNEG),
    ("I_nan_nonneg_C", dict(nonneg_C=True, **dense_I(nan=(2, 1))), {}, M_NAN_NONNEG),
    ("U_nan_l1", dict(l1_lam=0.5, **dense_U(nan=(1, 0))), {}, M_NAN_NONNEG),
    ("U_all_nan_nonneg", dict(nonneg=True, **dense_U(nan="all")), {}, M_U_EMPTY),
    ("precompute_without_buffers", dict(precompute_for_predictions=True, precomputedBtB=None), {}, M_PRE_BUF),
    ("nan_nonneg_before_buffers", dict(nonneg=True, precompute_for_predictions=True, precomputedBtB=None, **dense_U(nan=(0, 1))), {}, M_NAN_NONNEG),
    ("no_rows", dict(m=0), {}, M_DIMS),
    ("no_columns", dict(n=-1), {}, M_DIMS),
    ("X_index", BAD_X, {}, M_IX % "X"),
    ("X_index_col", dict(ixB=[0, 1, 3, 0, 2]), {}, M_IX % "X"),
    ("buffers_before_X_index", dict(precompute_for_predictions=True, precomputedBtB=None, **BAD_X), {}, M_PRE_BUF),
]

IMPLICIT_ONLY = [
    ("k_main", dict(k_main=1, nnz=0), {}, M_K_MAIN),
    ("no_entries", dict(nnz=0), {}, M_NO_X),
    ("no_entries_before_naz", dict(nnz=0, NA_as_zero_U=True, **sparse_U(rows=5)), {}, M_NO_X),
    ("no_factors", dict(k=0), {}, M_DIMS),
]

EXPLICIT_ONLY = [
    ("k_main", dict(k_main=1, nnz=0), {}, M_K_MAIN),
    ("no_entries", dict(nnz=0), {}, M_DIMS),
    # ---- dense X, between the two stages of the intake ----
    ("dense_X_implicit_features", dict(add_implicit_features=True, **Xfull()), {}, M_DX_MODEL),
    ("dense_X_NA_as_zero_X", dict(NA_as_zero_X=True, **Xfull()), {}, M_DX_MODEL),
    ("naz_U_more_rows_before_dense_X", dict(add_implicit_features=True, NA_as_zero_U=True, **Xfull(), **sparse_U(rows=5)), {}, M_NAZ_ROWS_U),
    ("dense_X_side_weights", dict(weight=np.ones((4, 3)), **Xfull(), **dense_U()), {}, M_DX_SIDE_W),
    ("dense_X_side_naz_flag", dict(NA_as_zero_I=True, **Xfull(), **dense_U()), {}, M_DX_SIDE_W),
    ("dense_X_zero_filled_U", dict(NA_as_zero_U=True, **Xfull(), **sparse_U()), {}, M_DX_SIDE_W),
    ("dense_X_sparse_zeros_I", dict(NA_as_zero_I=True, **Xfull(), **sparse_I()), TINY_LIMIT, M_DX_SIDE_W),
    ("dense_X_U_rows", dict(**Xfull(), **dense_U(rows=3)), {}, M_DX_SIDE_ROWS),
    ("dense_X_I_rows", dict(**Xfull(), **sparse_I(rows=2, row=(0, 1))), {}, M_DX_SIDE_ROWS),
    ("dense_X_no_rows", dict(m=0, **Xfull()), {}, M_DIMS),
    ("dense_X_empty", Xfull(all_nan=True), {}, M_DX_EMPTY),
    ("dense_X_few_missing_scaled", dict(scale_lam=True, scale_bias_const=True, user_bias=True, item_bias=True, **Xfull(nan=[(0, 1)])), {}, M_DX_FEW),
    ("dense_X_U_nan", dict(**Xfull(), **dense_U(nan=(1, 0))), {}, M_DX_NAN),
    ("dense_X_U_all_nan", dict(**Xfull(), **dense_U(nan="all")), {}, M_U_EMPTY),
    ("dense_X_U_nan_nonneg", dict(nonneg=True, **Xfull(), **dense_U(nan=(1, 0))), {}, M_NAN_NONNEG),
    # ---- NA_as_zero_X, between the two stages of the intake ----
    ("naz_X_nonneg", dict(NA_as_zero_X=True, nonneg=True), {}, M_NAZX_MODEL),
    ("naz_X_l1", dict(NA_as_zero_X=True, l1_lam=0.1), {}, M_NAZX_MODEL),
    ("naz_X_scale_bias_const", dict(NA_as_zero_X=True, scale_bias_const=True, scale_lam=True, item_bias=True), {}, M_NAZX_MODEL),
    ("naz_X_precompute_side", dict(NA_as_zero_X=True, precompute_for_predictions=True, **dense_U()), {}, M_NAZX_PRE),
    ("naz_X_precompute_zero_filled", dict(NA_as_zero_X=True, precompute_for_predictions=True, NA_as_zero_I=True, **sparse_I()), TINY_LIMIT, M_NAZX_PRE),
    ("naz_X_precompute_implicit_features", dict(NA_as_zero_X=True, precompute_for_predictions=True, add_implicit_features=True), {}, M_NAZX_PRE),
    ("naz_X_sparse_and_naz_flag", dict(NA_as_zero_X=True, NA_as_zero_I=True, **sparse_U()), {}, M_NAZX_SP_NAZ),
    ("naz_X_sparse_U_rows", dict(NA_as_zero_X=True, **sparse_U(rows=3, row=(0, 1, 2))), {}, M_NAZX_ROWS),
    ("naz_X_sparse_I_rows", dict(NA_as_zero_X=True, **sparse_I(rows=2, row=(0, 1))), {}, M_NAZX_ROWS),
    ("naz_X_weights_bias", dict(NA_as_zero_X=True, user_bias=True, **W5), {}, M_NAZX_W_BIAS),
    ("naz_X_weights_cg_wide", dict(NA_as_zero_X=True, use_cg=True, k=64, **W5), {}, M_NAZX_W_CG),
    ("naz_X_dense_U_rows", dict(NA_as_zero_X=True, **dense_U(rows=3)), {}, M_NAZX_ROWS),
    ("naz_X_dense_I_rows", dict(NA_as_zero_X=True, **dense_I(rows=4)), {}, M_NAZX_ROWS),
    ("naz_X_U_nan", dict(NA_as_zero_X=True, **dense_U(nan=(3, 1))), {}, M_NAZX_NAN % "U"),
    ("naz_X_I_nan", dict(NA_as_zero_X=True, **dense_I(nan=(0, 0))), {}, M_NAZX_NAN % "I"),
    ("naz_X_U_nan_before_I_nan", dict(NA_as_zero_X=True, **dense_U(nan=(3, 1)), **dense_I(nan=(0, 0))), {}, M_NAZX_NAN % "U"),
    ("naz_X_U_all_nan", dict(NA_as_zero_X=True, **dense_U(nan="all")), {}, M_NAZX_NAN % "U"),
    # the zero-filled U has the rows of X, whatever m_u said: no "exactly the rows" refusal, the fit goes on
    ("naz_X_zero_filled_U_goes_on", dict(NA_as_zero_X=True, NA_as_zero_U=True, **sparse_U(rows=3, row=(0, 1, 2)), **BAD_X), {}, M_IX % "X"),
    # ---- implicit features, after the NaN stage ----
    ("implicit_features_outputs", dict(add_implicit_features=True, Bi=None), {}, M_IMP_OUT),
    ("implicit_features_U_beyond", dict(add_implicit_features=True, **dense_U(rows=5)), {}, M_IMP_BEYOND),
    ("implicit_features_precompute", dict(add_implicit_features=True, precompute_for_predictions=True), {}, M_IMP_PRE),
    ("implicit_features_nonneg", dict(add_implicit_features=True, nonneg=True), {}, M_IMP_NONNEG),
    ("implicit_features_l1", dict(add_implicit_features=True, l1_lam_unique=np.zeros(6)), {}, M_IMP_NONNEG),
    ("implicit_features_w", dict(add_implicit_features=True, w_implicit=0.), {}, M_IMP_W),
    ("U_all_nan_before_implicit_features", dict(add_implicit_features=True, Ai=None, **dense_U(nan="all")), {}, M_U_EMPTY),
    ("implicit_features_before_triplets", dict(add_implicit_features=True, w_implicit=-1., **sparse_U(row=None)), {}, M_IMP_W),
    # ---- weights ----
    ("weights_sparse_scale_lam_sideinfo", dict(scale_lam_sideinfo=True, **W5, **sparse_U()), {}, M_W_SP),
    ("weights_nan_side", dict(**W5, **dense_U(nan=(1, 0))), {}, M_W_OTHER),
    ("weights_scale_lam_sideinfo", dict(scale_lam_sideinfo=True, **W5), {}, M_W_OTHER),
    ("weights_scale_bias_const", dict(scale_bias_const=True, scale_lam=True, user_bias=True, **W5), {}, M_W_OTHER),
    ("weights_before_dims", dict(scale_lam_sideinfo=True, nnz=0, **W5), {}, M_W_OTHER),
    # ---- scale_bias_const, the last refusals ----
    ("scale_bias_const_sparse", dict(scale_bias_const=True, scale_lam=True, user_bias=True, **sparse_U()), {}, M_SBC_MODEL),
    ("scale_bias_const_nan", dict(scale_bias_const=True, scale_lam=True, user_bias=True, **dense_I(nan=(0, 0))), {}, M_SBC_MODEL),
    ("scale_bias_const_implicit_features", dict(scale_bias_const=True, scale_lam=True, user_bias=True, add_implicit_features=True), {}, M_SBC_MODEL),
    ("scale_bias_const_item_chol", dict(scale_bias_const=True, scale_lam=True, item_bias=True), {}, M_SBC_ITEM),
    ("scale_bias_const_outputs", dict(scale_bias_const=True, scale_lam_sideinfo=True, user_bias=True, scaling_biasB=None), {}, M_SBC_OUT),
    ("X_index_before_scale_bias_const", dict(scale_bias_const=True, scale_lam=True, item_bias=True, **BAD_X), {}, M_IX % "X"),
]

CASES = [("implicit", True) + c for c in SHARED + IMPLICIT_ONLY] + [("explicit", False) + c for c in SHARED + EXPLICIT_ONLY]


@pytest.fixture
def one_device(monkeypatch):
    for name in ("CMFREC_HIP_DEVICES", "CMFREC_HIP_SHARDED", "CMFREC_HIP_ZEROFILL_MAX_GB"):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def refused(implicit, dtype, overrides, env, capfd, monkeypatch):
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    _lib.load(dtype)
    capfd.readouterr()
    rc, vals = _call(implicit, dtype, overrides)
    return rc, capfd.readouterr().err, vals


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["double", "float"])
@pytest.mark.parametrize("driver,implicit,case,overrides,env,message", CASES, ids=["%s-%s" % (c[0], c[2]) for c in CASES])
def test_refusal(driver, implicit, case, overrides, env, message, dtype, capfd, one_device):
    rc, err, _ = refused(implicit, dtype, overrides, env, capfd, one_device)
    assert rc == 2
    assert err == message + "\n"


@pytest.mark.parametrize("implicit", [True, False], ids=["implicit", "explicit"])
def test_quiet_refusal_prints_nothing(implicit, capfd, one_device):
    rc, err, _ = refused(implicit, np.float64, dict(verbose=False, k_user=1), {}, capfd, one_device)
    assert rc == 2 and err == ""


@pytest.mark.parametrize("implicit", [True, False], ids=["implicit", "explicit"])
def test_all_nan_I_reports_nan_colmeans(implicit, capfd, one_device):
    """The other half of the asymmetry: the all-NaN I went through the NaN stage (its column means are 0 / 0) before the fit went
    on to the refusal that ends this call; the all-NaN U is refused from the same stage."""
    rc, err, vals = refused(implicit, np.float64, dict(**dense_I(nan="all"), **BAD_X), {}, capfd, one_device)
    assert rc == 2 and err == M_IX % "X" + "\n"
    assert np.isnan(vals["I_colmeans"][:2]).all() and (vals["I_colmeans"][2:] == 0).all()
    rc, err, vals = refused(implicit, np.float64, dense_U(nan="all"), {}, capfd, one_device)
    assert rc == 2 and err == M_U_EMPTY + "\n"
    assert np.isnan(vals["U_colmeans"][:2]).all()


@pytest.mark.parametrize("implicit", [True, False], ids=["implicit", "explicit"])
def test_sparse_zeros_colmeans_before_a_later_refusal(implicit, capfd, one_device):
    """Beyond the size limit the triplets are taken as they are and the column means over ALL rows of X are reported at once."""
    rc, err, vals = refused(implicit, np.float64, dict(NA_as_zero_I=True, **sparse_I(), **BAD_X), TINY_LIMIT, capfd, one_device)
    assert rc == 2 and err == M_IX % "X" + "\n"
    assert vals["I_colmeans"][:2].tolist() == [-2. / 3, 1.5 / 3]
