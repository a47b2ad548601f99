"""cmfrec_hip_session_objective / AlsSession.objective: every component of the record against a dense extended-precision
evaluation over all m x n pairs, within the forward bound computed from the inputs (tests/objective_reference.py)."""
import ctypes as C

import numpy as np
import pytest

from objective_reference import assert_within, reference_and_bound

pytestmark = pytest.mark.gpu

VARIANTS = {"implicit": (True, False, False), "explicit": (False, False, False), "explicit_w": (False, True, False),
            "explicit_bias": (False, False, True), "explicit_w_bias": (False, True, True)}   # implicit, weights, both biases


def problem(dtype, k, implicit, weights, biases, seed=0):
    """m x n (37 x 29; 19 x 17 at k = 272) with rows 3 and 11 empty, column 5 empty, one entry in row 7 and row 2 holding
    every column that has an entry at all."""
    m, n = (19, 17) if k == 272 else (37, 29)
    rng = np.random.default_rng(seed + k)
    mask = rng.random((m, n)) < 0.3
    mask[2, :] = True
    mask[7, :] = False; mask[7, 9] = True
    mask[[3, 11], :] = False
    mask[:, 5] = False
    V = (np.ceil(rng.lognormal(0, 1, (m, n))) if implicit else rng.standard_normal((m, n))).astype(dtype)
    W = rng.uniform(0.5, 2., (m, n)).astype(dtype) if weights else None
    A = (rng.standard_normal((m, k)) / np.sqrt(k)).astype(dtype)
    B = (rng.standard_normal((n, k)) / np.sqrt(k)).astype(dtype)
    bA = (0.3 * rng.standard_normal(m)).astype(dtype) if biases else None
    bB = (0.3 * rng.standard_normal(n)).astype(dtype) if biases else None
    return mask, V, W, A, B, bA, bB


def session_for(dtype, k, implicit, mask, V, W, A, B, bA, bB, **model):
    from cmfrec_amd import AlsSession
    m, n = mask.shape
    s = AlsSession(m, n, k, implicit, dtype=dtype, user_bias=bA is not None, item_bias=bB is not None, **model)
    row, col = np.nonzero(mask)
    s.set_X_coo(row.astype(np.int32), col.astype(np.int32), V[mask], weight=None if W is None else W[mask])
    s.set_factors(A, B, bA, bB)
    return s


@pytest.mark.parametrize("hooks", [False, True], ids=["plain", "seg7_waves4"])
@pytest.mark.parametrize("k", [3, 50, 65, 272])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_components_within_forward_bound(variant, dtype, k, hooks, monkeypatch):
    implicit, weights, biases = VARIANTS[variant]
    mask, V, W, A, B, bA, bB = problem(dtype, k, implicit, weights, biases)
    if hooks:
        monkeypatch.setenv("CMFREC_HIP_OBJ_SEGMENT", "7")
        monkeypatch.setenv("CMFREC_HIP_OBJ_WAVES", "4")
    s = session_for(dtype, k, implicit, mask, V, W, A, B, bA, bB)
    rec, again = s.objective(), s.objective()
    s.close()
    ref, bound = reference_and_bound(dtype, implicit, A, B, mask, V, W, bA, bB)
    assert_within(rec, ref, bound, "%s k=%d" % (variant, k))
    if not weights:
        assert rec["sum_w"] == float(ref["n"])
    for f in rec:                                             # the same call, the same bytes
        assert np.array_equal(np.asarray(rec[f]), np.asarray(again[f])), f


@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
def test_fit_level_record_with_k_main(implicit):
    """Through the fit: k_main = 1 beside k = 3 (the shared columns are k + k_main wide), the record of the last iteration against
    the reference on the returned factors.  (k_user / k_item need side information, which the objective refuses: below.)"""
    from cmfrec_amd import CMF, CMF_implicit, Objective
    mask, V, _, _, _, _, _ = problem(np.float64, 4, implicit, False, False)
    row, col = np.nonzero(mask)
    X = (row.astype(np.int32), col.astype(np.int32), V[mask])
    common = dict(k=3, k_main=1, niter=2, use_float=False, use_cg=False, precompute_for_predictions=False)
    mdl = (CMF_implicit(lambda_=2., **common) if implicit else CMF(lambda_=2., **common)).fit(X, shape=mask.shape, objective=Objective())
    assert mdl.n_iter_ == 2 and [h["iteration"] for h in mdl.objective_history_] == [0, 1]
    stored = V if implicit else V - mdl.glob_mean_
    ref, bound = reference_and_bound(np.float64, implicit, mdl.A_, mdl.B_, mask, stored, None,
                                     None if implicit else mdl.user_bias_, None if implicit else mdl.item_bias_)
    assert_within(mdl.objective_history_[-1], ref, bound, "fit level")


def test_refusals_leave_the_outputs_untouched():
    from cmfrec_amd import _lib, CMF, Objective
    mask, V, W, A, B, bA, bB = problem(np.float64, 3, False, False, False)
    m, n = mask.shape
    s = session_for(np.float64, 3, False, mask, V, W, A, B, bA, bB, p=2, m_u=m)
    s.set_sideinfo(U=np.ones((m, 2)))
    rec = _lib.ObjectiveRecord()
    C.memset(C.byref(rec), 0xA5, C.sizeof(rec))
    assert s.lib.cmfrec_hip_session_objective(s.handle, C.byref(rec)) == 2
    assert bytes(rec) == b"\xa5" * C.sizeof(rec) and b"side information" in s.lib.cmfrec_hip_last_error()
    s.close()
    A0 = np.full((m, 6), 7.)                                   # k_user = 2, k_item = 1, k_main = 1 need U and I: refused before any output is written
    row, col = np.nonzero(mask)
    mdl = CMF(k=3, k_user=2, k_item=1, k_main=1, niter=2, use_float=False)
    with pytest.raises(RuntimeError, match="side information"):
        mdl.fit((row.astype(np.int32), col.astype(np.int32), V[mask]), U=np.ones((m, 2)), I=np.ones((n, 2)), shape=(m, n),
                A0=A0, B0=np.zeros((n, 5)), objective=Objective())
    with pytest.raises(ValueError):
        from cmfrec_amd import Validation
        mdl.fit((row, col, V[mask]), shape=(m, n), objective=Objective(), validation=Validation((row[:3], col[:3], V[mask][:3])))
