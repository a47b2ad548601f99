"""The dense kernels (GEMM, Gramian, potrf, trtri, the shared-matrix solve) on their own, against references of their own
operations with derived bounds (tests/dense_reference.py), through `cmfrec_hip_dense_op`: the library's launch helpers, so the
host dispatch (split-K, REM variants, blocks and rows per block, the LDS choice of trtri) is under test with the kernels.

Every GEMM and Gramian case runs two data sets: small integers, whose result must be equal in bits at any K, and standard
normals against the componentwise bounds.  tests/test_dense_bound_sensitivity.py shows on the CPU that these checks accept
honest arithmetic in the dtype and reject what a subtly wrong kernel would write, on every case below.

Worst error / bound on the MI355X, float64 / float32 (logged through CMFREC_TEST_RELERR_LOG):
    GEMM     exact data 0 / 0 (bit for bit, every case); normal data 0.344 / 0.255 (5 x 7 x 3, TRANSA); beside a NaN row or an
             Inf column 0.098 / 0.140
    Gramian  exact data 0 / 0; normal data 0.446 (n = 1, k = 64) / 0.476 (n = 3, k = 17)
    potrf    exact data 0 / 0; condition 10: 0.481 / 0.338, condition 1e4: 0.629 / 0.643 (n = 1: one square root against gamma_2)
    trtri    0.294 / 0.299 (n = 2)
    potrs    forward 0.402 / 0.228 of 4 e_o + 4 n cond u (k = 1), float32 eta 0.325 of ETA_SHARED (k = 257)"""
import numpy as np
import pytest

import dense_reference as D

pytestmark = pytest.mark.gpu


def _ops():
    from cmfrec_amd import ops
    return ops


# ---- GEMM ------------------------------------------------------------------------------------------------------------------

def _run_gemm(dtype, transa, shape, layout, data, A=None, B=None):
    M, N, K = shape
    Ci, kw = D.gemm_images(dtype, transa, shape, layout, data, A=A, B=B)
    return _ops().dense_op("gemm_ta" if transa else "gemm", M, N, K, Ci, **kw)


@pytest.mark.parametrize("case", D.gemm_cases(), ids=D.case_id)
def test_gemm(case):
    """Tile edges, one step, the K remainder, split-K (4096 and above; a last chunk 4 wide); leading dimensions tight, odd,
    padded; each operand alone off its 16-byte alignment; the pointer advanced by three elements; padded output."""
    dtype, transa, shape, layout = case
    for data in D.DATA:
        Ci = _run_gemm(dtype, transa, shape, layout, data)
        r = D.check_gemm(dtype, transa, shape, layout, data, Ci)
        print("gemm %s: error / bound %.3f" % (data, r))


@pytest.mark.parametrize("transa", [0, 1])
@pytest.mark.parametrize("dtype", D.DTYPES, ids=D._name)
def test_gemm_nonfinite_stays_in_its_row_and_column(dtype, transa):
    """NaN in the last row of op(A), then Inf in the last column of B: only that output row / column is non-finite, the rest
    still meets the bound."""
    shape, data = (129, 127, 33), "normal"
    M, N, K = shape
    A0, B0, _, ref, bound = D.gemm_problem(dtype, M, N, K, data)
    ldc, oc = D.gemm_layout("tight", dtype, transa, M, N, K)[4:]
    A = A0.copy(); A[M - 1] = np.nan
    got, pad_ok = D.split_image(_run_gemm(dtype, transa, shape, "tight", data, A=A), M, N, ldc, oc)
    assert pad_ok and np.isnan(got[M - 1]).all()
    skip = np.zeros((M, N), bool); skip[M - 1] = True
    D.check_matrix(got, ref, bound, "NaN row of A", "gemm-nan-row", dtype, skip=skip)
    B = B0.copy(); B[:, N - 1] = np.inf
    got, pad_ok = D.split_image(_run_gemm(dtype, transa, shape, "tight", data, B=B), M, N, ldc, oc)
    assert pad_ok and not np.isfinite(got[:, N - 1]).any()
    skip = np.zeros((M, N), bool); skip[:, N - 1] = True
    D.check_matrix(got, ref, bound, "Inf column of B", "gemm-inf-column", dtype, skip=skip)


@pytest.mark.parametrize("transa", [0, 1])
@pytest.mark.parametrize("dtype", D.DTYPES, ids=D._name)
def test_gemm_splitk_same_bits_twice(dtype, transa):
    a = _run_gemm(dtype, transa, (130, 200, 5000), "tight", "normal")
    b = _run_gemm(dtype, transa, (130, 200, 5000), "tight", "normal")
    assert np.array_equal(D._bits(a), D._bits(b))


# ---- Gramian ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", D.gram_cases(), ids=D.case_id)
def test_gram(case):
    """Every width of the MFMA kernel's column blocks and REM variants, the GEMM route beyond 64; row counts around the
    four-row step, the 64-row trip and the 128-row block, no rows at all, 49 / 66 / 511 partial blocks; both triangles."""
    dtype, n, k, layout, scales = case
    for data in D.DATA:
        Ci, kw = D.gram_images(dtype, n, k, layout, data, scales)
        _ops().dense_op("gram", 0, n, k, Ci, **kw)
        r = D.check_gram(dtype, n, k, layout, data, scales, Ci)
        print("gram %s: error / bound %.3f" % (data, r))


# ---- potrf, trtri, potrs_rows ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", D.potrf_cases(), ids=D.case_id)
def test_potrf(case):
    dtype, n, data, off = case
    Ci, kw = D.potrf_image(dtype, n, data, off)
    _ops().dense_op("potrf", 0, n, 0, Ci, **kw)
    print("potrf: error / bound %.3f" % D.check_potrf(dtype, n, data, off, Ci))


@pytest.mark.parametrize("case", D.trtri_cases(), ids=D.case_id)
def test_trtri(case):
    """Widths on both sides of 48 KiB and 96 KiB of LDS (static, raised, global memory), and beyond 256 columns."""
    dtype, n, off = case
    Ci, kw = D.trtri_images(dtype, n, off)
    _ops().dense_op("trtri", 0, n, 0, Ci, **kw)
    print("trtri: residual / bound %.3f" % D.check_trtri(dtype, n, off, Ci))


@pytest.mark.parametrize("case", D.potrs_cases(), ids=D.case_id)
def test_potrs_rows(case):
    """X := X (R^T R)^-1 at condition 1e4: per row within 4x the same-precision LAPACK solve plus n cond u of the wide
    solution; float32 also to the backward error of the refined solve."""
    dtype, k, rows, layout = case
    Ci, kw = D.potrs_images(dtype, k, rows, layout)
    _ops().dense_op("potrs_rows", rows, 0, k, Ci, **kw)
    fwd, eta = D.check_potrs(dtype, k, rows, layout, Ci)
    print("potrs_rows: forward %.3f, eta / ETA_SHARED %.3f" % (fwd, eta))


# ---- the entry point itself ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", D.DTYPES, ids=D._name)
def test_invalid_sizes_are_refused(dtype):
    ops = _ops()
    C = np.zeros(16, dtype); A = np.zeros(16, dtype); B = np.zeros(16, dtype)
    for args, kw in ((("gemm", -1, 2, 2, C), dict(A_img=A, lda=2, B_img=B, ldb=2, ldc=2)),
                     (("gemm", 2, 2, 2, C), dict(A_img=A, lda=1, B_img=B, ldb=2, ldc=2)),
                     (("gemm", 2, 2, 2, C), dict(A_img=A, lda=2, B_img=B, ldb=2, ldc=1)),
                     (("gemm", 2, 2, 2, C), dict(A_img=None, lda=2, B_img=B, ldb=2, ldc=2)),
                     (("gram", 0, 2, 0, C), dict(B_img=B, ldb=2, ldc=2)),
                     (("gram", 0, 2, 2, C), dict(B_img=B, ldb=2, ldc=3)),
                     (("potrf", 0, 0, 0, C), dict(ldc=0)),
                     (("trtri", 0, 2, 0, C), dict(A_img=A, lda=3, ldc=2)),
                     (("potrs_rows", 2, 0, 2, C), dict(A_img=A, lda=2, ldc=1))):
        with pytest.raises(RuntimeError, match="code 2"):
            ops.dense_op(*args, **kw)
