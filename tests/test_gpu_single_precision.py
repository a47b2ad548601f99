"""The single-precision kernels against a float64 reference, row by row (tests/fp32_reference.py).

The float32 operator tests elsewhere compare the HIP result with the float32 oracle at 1e-3 per row; a kernel that gathered B
through fp16 (2e-4 per row) passes them.  Here every row must be within 4x the float32 oracle's own distance from the float64
answer plus 1e-5, and a closed-form row must solve its float64 normal equations to a backward error of 32 * 2^-24.
tests/test_fp32_bound_sensitivity.py shows on the CPU that these checks reject such kernels on every case below."""
import numpy as np
import pytest

import fp32_reference as F

pytestmark = pytest.mark.gpu


def _run_and_check(name):
    ah = F.run_hip(F.case(name))
    F.check_case(name, ah)


@pytest.mark.parametrize("vh", ["gram", "gram-slice", "stream"])
@pytest.mark.parametrize("name", F.LADDER_CASES)
def test_row_length_ladder(name, vh, monkeypatch):
    """Rows of every length 0 .. 150 and the tile, team and split boundaries up to 4500 entries, implicit (CG, Cholesky) and
    explicit with bias_sub / lam_last / scale_lam (CG, Cholesky), k = 8 / 33 / 64; the split rows on each CMFREC_HIP_VH path."""
    monkeypatch.setenv("CMFREC_HIP_VH", vh.split("-")[0])
    if vh == "gram-slice":
        monkeypatch.setenv("CMFREC_HIP_GRAM_KERNEL", "slice")
    _run_and_check(name)


@pytest.mark.parametrize("name", F.PROD_CASES)
def test_production_slicing(name):
    """One shard whose split rows hold >= 2048 * 1024 entries (device.hpp): the 2048-entry slices of configurations 2 and 4."""
    lens = F.case(name)["lens"]
    assert sum(int(l) for l in lens if l >= F.VH_MIN_F32) >= F.GRAM_SLICE * 1024
    _run_and_check(name)


@pytest.mark.parametrize("name", F.WEIGHT_CASES)
def test_observation_weights_and_wide_cg(name):
    """Observation weights at k = 33 / 64 (CG and Cholesky); explicit CG beyond 64 unknowns, with and without weights."""
    _run_and_check(name)


@pytest.mark.parametrize("name", F.TINY_CASES)
def test_two_rows_per_wave_shapes(name):
    """The shapes of test_gpu_operators.test_two_rows_per_wave (rows of 0 .. 60 entries) in float32."""
    _run_and_check(name)


@pytest.mark.parametrize("name", F.SHARED_CASES)
def test_shared_matrix_solve(name):
    """NA_as_zero_X closed form and one implicit-features half-step: one factorisation of the shared matrix, its explicit
    inverse and the float32 refinement step (launch_dense.hip, launch_potrs_rows), on a matrix of condition ~1e4."""
    _run_and_check(name)


@pytest.mark.parametrize("name", F.SIDE_CASES)
def test_dense_and_side_information(name):
    """Dense X (optimizeA_dense_full), dense and sparse side information (Cholesky) in float32."""
    _run_and_check(name)
