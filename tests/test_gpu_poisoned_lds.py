"""Parity cases of the operator tests again with the LDS of every CU filled with NaN patterns in front of each launch
(CMFREC_HIP_POISON_LDS=1, cmfrec_amd/csrc/launch_cg.hip): a kernel that reads LDS it has not written -- 0 x stale LDS in
gram_cg_kernel left the split rows of a launch at their start values whenever the previous tenant of that LDS had left a NaN
pattern, which happened on some boxes in some runs (profiles/README.md) -- fails here every time."""
import numpy as np
import pytest

import test_gpu_operators as T

pytestmark = pytest.mark.gpu
DT = [np.float64, np.float32]


@pytest.fixture(autouse=True)
def poisoned(monkeypatch):
    monkeypatch.setenv("CMFREC_HIP_POISON_LDS", "1")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("implicit", [True, False])
@pytest.mark.parametrize("vh", ["stream", "gram", "gram-slice"])
@pytest.mark.parametrize("k", [50, 7])
def test_split_rows(oracles, dtype, implicit, vh, k, monkeypatch):
    T.test_very_heavy_rows_split_path(oracles, dtype, implicit, vh, k, monkeypatch)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("mode", ["cg", "chol", "pcg"])
def test_row_kernels(oracles, dtype, mode):
    T.test_optimizeA_implicit(oracles, dtype, 50, mode)
    T.test_optimizeA_explicit(oracles, dtype, 33, 2, mode)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("implicit", [True, False])
def test_two_rows_per_wave(oracles, dtype, implicit):
    T.test_two_rows_per_wave(oracles, dtype, implicit, 50)


@pytest.mark.parametrize("dtype", DT)
def test_collective_and_wide(oracles, dtype):
    T.test_optimizeA_collective(oracles, dtype, 2, 3, 1, True, None)
    T.test_cholesky_large_k(oracles, dtype, 161 if dtype == np.float64 else 200, True)
    T.test_collective_sparse_sideinfo(oracles, dtype, 50, 2, 1, 1)
