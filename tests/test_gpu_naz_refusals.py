"""GPU: what the missing-as-zero half-steps (session.hip, update_factor_naz*) refuse -- return code 2 and the exact text of
cmfrec_hip_last_error(), through the session API on the smallest shapes that reach each guard."""
import ctypes as C
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DT = [np.float64, np.float32]
M, N, K = 12, 9, 3

SIDE_ROWS = "cmfrec_hip: NA_as_zero_X with side information: side information on exactly the rows / columns of X"
GSUM_WIDTH = "cmfrec_hip: NA_as_zero_X with implicit features: k + k_main too wide for the gather-sum"
NO_NONNEG_L1 = "cmfrec_hip: NA_as_zero_X with observation weights: the model without nonneg / L1"
UNWEIGHTED_MODEL = ("cmfrec_hip: NA_as_zero_X: the explicit model on one device without weights, nonneg / L1, "
                    "scale_bias_const, incomplete side information")
CG_64 = ("cmfrec_hip: NA_as_zero_X with observation weights under CG: at most 64 unknowns per row "
         "(the preconditioned solver takes more)")


def gsum_max_width():
    """64 * GSUM_MAXC, read from the kernel header the library was built from."""
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "cmfrec_amd", "csrc", "dense_kernels.hpp")) as f:
        return 64 * int(re.search(r"constexpr int GSUM_MAXC = (\d+);", f.read()).group(1))


def problem(dtype, seed=7):
    """A few dozen entries, every row and column of X present, weights in (0.5, 2)."""
    rng = np.random.default_rng(seed)
    lin = np.sort(np.concatenate([np.arange(M) * N + np.arange(M) % N,
                                  rng.choice(M * N, size=30, replace=False)]))
    lin = np.unique(lin)
    row, col = (lin // N).astype(np.int32), (lin % N).astype(np.int32)
    return dict(row=row, col=col, val=rng.standard_normal(lin.size).astype(dtype),
                w=rng.uniform(0.5, 2.0, lin.size).astype(dtype))


def session(dtype, weights, k=K, **model):
    from cmfrec_amd.session import AlsSession
    d = problem(dtype)
    S = AlsSession(M, N, k, implicit=False, dtype=dtype, lam=0.3, **model)
    rng = np.random.default_rng(3)
    S.set_factors(A=rng.standard_normal((M, S.k_totA)) * 0.1, B=rng.standard_normal((N, S.k_totB)) * 0.1)
    S.set_X_coo(d["row"], d["col"], d["val"], weight=d["w"] if weights else None)
    return S


def refused(S, which, use_cholesky, text):
    rc = S.lib.cmfrec_hip_session_update(S.handle, C.c_int(ord(which)), C.c_int(int(use_cholesky)))
    msg = S.lib.cmfrec_hip_last_error().decode()
    S.close()
    assert rc == 2, (rc, msg)
    assert msg == text


def sparse_side(S, which, rows, cols, dtype):
    """an attribute for every second row"""
    r = np.arange(0, rows, 2, dtype=np.int32)
    c = (r % cols).astype(np.int32)
    v = np.ones(r.size, dtype)
    rc = S.lib.cmfrec_hip_session_set_sideinfo_sparse(S.handle, C.c_int(ord(which)), r.ctypes.data_as(C.c_void_p),
                                                      c.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), C.c_size_t(r.size))
    assert rc == 0, S.lib.cmfrec_hip_last_error()


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("constraint", ["nonneg", "l1"])
def test_weights_with_nonneg_or_l1(dtype, constraint):
    S = session(dtype, weights=True, use_cg=False)
    S.set_NA_as_zero_X(True)
    if constraint == "nonneg":
        S.set_nonneg(True)
    else:
        real = C.c_double if dtype is np.float64 else C.c_float
        assert S.lib.cmfrec_hip_session_set_l1(S.handle, real(0.1), C.c_int(100)) == 0
    refused(S, "A", True, NO_NONNEG_L1)


@pytest.mark.parametrize("dtype", DT)
def test_nonneg_without_weights(dtype):
    S = session(dtype, weights=False, use_cg=False)
    S.set_NA_as_zero_X(True)
    S.set_nonneg(True)
    refused(S, "B", True, UNWEIGHTED_MODEL)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("kind", ["dense", "dense weighted", "sparse"])
def test_sideinfo_rows_differ_from_X(dtype, kind):
    """Side information on 10 of the 12 rows of X: the shared-matrix half-step, the weighted row-by-row one and the one with
    sparse side information each refuse it."""
    p, m_u = 2, M - 2
    S = session(dtype, weights=kind == "dense weighted", use_cg=False, p=p, m_u=m_u)
    if kind == "sparse":
        sparse_side(S, "U", m_u, p, dtype)
    else:
        S.set_sideinfo(U=np.random.default_rng(5).standard_normal((m_u, p)))
    S.set_NA_as_zero_X(True)
    refused(S, "A", True, SIDE_ROWS)


@pytest.mark.parametrize("dtype", DT)
def test_weighted_cg_beyond_64_unknowns(dtype):
    S = session(dtype, weights=True, k=65, use_cg=True, precondition_cg=False)
    S.set_NA_as_zero_X(True)
    refused(S, "A", False, CG_64)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("kind", ["weighted", "sparse"])
def test_gather_sum_too_wide(dtype, kind):
    """k + k_main one past the gather-sum's width, under the closed form: the weighted half-step with implicit features and
    the one with sparse side information.  (The shared-matrix half-step meets the row Cholesky kernel's own k_t limit first.)"""
    k = gsum_max_width() + 1
    if kind == "weighted":
        S = session(dtype, weights=True, k=k, use_cg=False)
    else:
        S = session(dtype, weights=False, k=k, use_cg=False, p=2, m_u=M)
        sparse_side(S, "U", M, 2, dtype)
    S.set_implicit_features(0.5)
    S.set_NA_as_zero_X(True)
    refused(S, "A", True, GSUM_WIDTH)
