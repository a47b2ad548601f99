"""Host-side checks of the new-rows handle (cmfrec_hip_newrows_*, cmfrec_amd.NewUsers): the ctypes mirrors of its model struct and
the Python-side argument checks.  No GPU."""
import ctypes as C

import numpy as np
import pytest


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_model_mirror_size(dtype):
    from cmfrec_amd import _lib
    lib = C.CDLL(_lib.lib_path(dtype))
    mirror = _lib.newrows_model_mirror(dtype)
    assert lib.cmfrec_hip_sizeof_newrows_model() == C.sizeof(mirror)
    # 16 int32, 9 reals (padded to the pointers' alignment), 11 pointers
    real = np.dtype(dtype).itemsize
    assert C.sizeof(mirror) == (16 * 4 + 9 * real + 7) // 8 * 8 + 11 * 8
    # the batch struct holds pointers and counts only: one layout for both precisions
    assert C.sizeof(_lib.NewRowsBatch) == 8 + 17 * 8


def _fake_model(cls, dtype, p):
    """A model with the attributes the input handling reads, without a fit."""
    mdl = cls(k=4, use_float=dtype is np.float32)
    mdl.B_ = np.zeros((30, 4), dtype)
    mdl.C_ = np.zeros((p, 4), dtype)
    return mdl


@pytest.mark.parametrize("cls_name", ["CMF", "CMF_implicit"])
def test_argument_checks(cls_name):
    import scipy.sparse as sp
    import cmfrec_amd
    from cmfrec_amd.models import _new_rows_batch
    cls = getattr(cmfrec_amd, cls_name)
    explicit = cls_name == "CMF"
    mdl = _fake_model(cls, np.float64, 5)
    X = sp.random(6, 30, 0.2, random_state=1, format="coo")
    with pytest.raises(ValueError, match="at least one of 'X', 'U'"):
        _new_rows_batch(mdl, None, None, None, explicit)
    with pytest.raises(ValueError, match="at least one of 'X', 'U'"):
        mdl.factors_multiple()
    with pytest.raises(ValueError, match="'W' needs 'X'"):
        _new_rows_batch(mdl, None, np.zeros((3, 5)), np.ones(4), explicit)
    with pytest.raises(ValueError, match="more columns than the model has items"):
        _new_rows_batch(mdl, sp.random(6, 31, 0.2, random_state=1), None, None, explicit)
    with pytest.raises(ValueError, match="more columns than the model has items"):
        _new_rows_batch(mdl, (np.array([0, 1]), np.array([3, 30]), np.ones(2)), None, None, explicit)
    with pytest.raises(ValueError, match="4 columns, the model was fitted with 5"):
        _new_rows_batch(mdl, X, np.zeros((6, 4)), None, explicit)
    with pytest.raises(ValueError, match="4 columns, the model was fitted with 5"):
        mdl.factors_multiple(X, U=np.zeros((6, 4)))
    with pytest.raises(ValueError, match="dense 'X'"):
        _new_rows_batch(mdl, np.zeros((6, 29)), None, None, explicit)
    b = _new_rows_batch(mdl, X, np.zeros((9, 5)), None, explicit)
    assert (b["m_x"], b["m_u"], b["p"]) == (6, 9, 5) and b["U"].dtype == np.float64 and b["Xfull"] is None
    b = _new_rows_batch(mdl, X, sp.random(9, 5, 0.5, random_state=2), None, explicit)
    assert b["U"] is None and b["Usp"][3:] == (9, 5)
    # a model fitted without side information ignores U, as factors_multiple always has
    b = _new_rows_batch(_fake_model(cls, np.float64, 0), X, np.zeros((9, 4)), None, explicit)
    assert (b["m_u"], b["p"]) == (0, 0) and b["U"] is None


def test_new_users_needs_a_fitted_model():
    from cmfrec_amd import CMF, NewUsers
    with pytest.raises(ValueError, match="not fitted"):
        NewUsers(CMF(k=4))
    with pytest.raises(ValueError, match="not fitted"):
        CMF(k=4).new_users()
