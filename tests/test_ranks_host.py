"""CPU: the host side of the rank calls -- the held-out normaliser, the refusals that happen before the device is touched, the
limits, the exported names and the test hook's place in the switches."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_normaliser():
    from cmfrec_amd.ops import _heldout_lists
    hp, hi = _heldout_lists((np.array([0, 3, 3, 6]), np.array([5, 2, 5, 9, 2**40, -4])), 3, "t")
    assert hp.dtype == np.uint64 and hi.dtype == np.int32
    assert hp.tolist() == [0, 2, 2, 4] and hi.tolist() == [2, 5, -1, 9]         # sorted, unique, out of int32 / negative -> one -1
    # ascending unique int32 lists pass as they are
    p, i = np.array([0, 2, 4], np.uint64), np.array([1, 7, 0, 3], np.int32)
    hp, hi = _heldout_lists((p, i), 2, "t")
    assert hp.tolist() == [0, 2, 4] and hi.tolist() == [1, 7, 0, 3]

    class Csr:                                                                  # what a SciPy CSR matrix offers
        indptr = np.array([0, 1, 3], np.int32); indices = np.array([4, 9, 2], np.int32)
    hp, hi = _heldout_lists(Csr(), 2, "t")
    assert hp.tolist() == [0, 1, 3] and hi.tolist() == [4, 2, 9]
    with pytest.raises(ValueError, match="'heldout' is required"):
        _heldout_lists(None, 2, "t")
    with pytest.raises(ValueError, match="must be \\(indptr, indices\\)"):
        _heldout_lists(np.arange(4), 2, "t")
    with pytest.raises(ValueError, match="one entry per user plus one"):
        _heldout_lists((np.array([0, 1]), np.array([3])), 2, "t")


def test_python_refusals_before_the_library():
    from cmfrec_amd import ops
    A = np.zeros((3, 4)); B = np.ones((5, 4))
    with pytest.raises(ValueError, match="'heldout' is required"):
        ops.ranks_batch(A, B, None)
    with pytest.raises(ValueError, match="one entry per user plus one"):
        ops.ranks_batch(A, B, (np.array([0, 1]), np.array([2])))
    with pytest.raises(TypeError):
        ops.ranks_batch(A.astype(np.int32), B, (np.array([0, 0, 0, 0]), np.zeros(0, np.int32)))
    with pytest.raises(ValueError, match="exclude: indptr"):
        ops.ranks_batch(A, B, (np.array([0, 0, 0, 1]), np.array([2])), exclude=(np.array([0, 1]), np.array([2])))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_c_refusals_before_the_device(dtype):
    """k = 273 and held_p == NULL: code 2 from the host checks (no GPU needed), the outputs untouched."""
    from cmfrec_amd import _lib
    lib = _lib.load(dtype)
    nu, n = 3, 5
    hp = np.array([0, 1, 2, 3], np.uint64); hi = np.array([0, 1, 2], np.int32)
    ranks = np.full(3, 77, np.int32); sc = np.full(3, 5, dtype); pool = np.full(nu, 77, np.int32)
    for k, held_p, what in ((273, hp, b"needs k <= 272"), (8, None, b"invalid arguments")):
        A = np.zeros((nu, k), dtype); B = np.ones((n, k), dtype)
        rc = lib.cmfrec_hip_ranks_batch(_lib.ptr(A), k, nu, _lib.ptr(B), k, n, k, None, _lib.ptr(held_p), _lib.ptr(hi), None, None,
                                        _lib.ptr(ranks), _lib.ptr(sc), _lib.ptr(pool))
        assert rc == 2 and what in lib.cmfrec_hip_last_error()
        assert np.all(ranks == 77) and np.all(sc == 5) and np.all(pool == 77)
    assert lib.cmfrec_hip_ranker_ranks(None, None, 8, nu, _lib.ptr(hp), _lib.ptr(hi), None, None, _lib.ptr(ranks), None, None) == 2
    assert lib.cmfrec_hip_newrows_ranks(None, None, _lib.ptr(hp), _lib.ptr(hi), 1, None, None, _lib.ptr(ranks), None, None, None, None) == 2
    assert np.all(ranks == 77)


def test_names():
    from cmfrec_amd import _lib, CMF, CMF_implicit, NewUsers, Ranker, metrics, ops
    from cmfrec_amd.models import ModelRanker
    for name in ("cmfrec_hip_ranker_ranks", "cmfrec_hip_ranks_batch", "cmfrec_hip_newrows_ranks"):
        assert name in _lib.EXPORTED
        assert hasattr(_lib.load(np.float64), name) and hasattr(_lib.load(np.float32), name)
    header = open(os.path.join(ROOT, "include", "cmfrec_hip.h")).read()
    for name in ("cmfrec_hip_ranker_ranks(", "cmfrec_hip_ranks_batch(", "cmfrec_hip_newrows_ranks("):
        assert name in header
    assert callable(ops.ranks_batch) and callable(Ranker.ranks) and callable(ModelRanker.ranks) and callable(NewUsers.ranks)
    for cls in (CMF, CMF_implicit):
        assert callable(cls.ranks_batch) and callable(cls.evaluate_ranking) and "X_test" in cls.evaluate_ranking.__doc__
    assert callable(metrics.ranking_metrics)
    assert "CMFREC_HIP_RANK_SLICE" in open(os.path.join(ROOT, "cmfrec_amd", "csrc", "device_base.hpp")).read()
    assert "CMFREC_HIP_RANK_SLICE" in open(os.path.join(ROOT, "DESIGN.md")).read()
