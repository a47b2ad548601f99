"""No GPU needed: the ``include`` normaliser of the candidate-list ranking (ops._sorted_include), its refusals before the library
is touched, the three new C names and the limits of the candidate calls."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_include_is_sorted_and_deduplicated_per_user():
    from cmfrec_amd.ops import _sorted_include
    ip = np.array([0, 5, 5, 9])
    ix = np.array([9, 2, 9, 4, 2, 7, 1, 7, 3])
    cp, ci = _sorted_include((ip, ix), 3)
    assert cp.dtype == np.uint64 and ci.dtype == np.int32
    assert cp.tolist() == [0, 3, 3, 6]
    assert ci.tolist() == [2, 4, 9, 1, 3, 7]
    # the same id in two users' lists stays in both; a list that is sorted already comes back as it is
    cp, ci = _sorted_include((np.array([0, 2, 4], np.uint64), np.array([1, 5, 1, 5], np.int32)), 2)
    assert cp.tolist() == [0, 2, 4] and ci.tolist() == [1, 5, 1, 5]
    # ids outside int32 cannot be items: they become -1, which the device skips
    cp, ci = _sorted_include((np.array([0, 3]), np.array([2 ** 40, 5, -7])), 1)
    assert cp.tolist() == [0, 2] and ci.tolist() == [-1, 5]
    assert _sorted_include(None, 4) == (None, None)
    # all lists empty
    cp, ci = _sorted_include((np.zeros(4, np.int64), np.zeros(0, np.int32)), 3)
    assert cp.tolist() == [0, 0, 0, 0] and len(ci) == 0


def test_shared_list_expands_to_one_list_per_user():
    from cmfrec_amd.ops import _sorted_include
    cp, ci = _sorted_include(np.array([8, 3, 8, 1]), 3)
    assert cp.dtype == np.uint64 and ci.dtype == np.int32
    assert cp.tolist() == [0, 3, 6, 9]
    assert ci.tolist() == [1, 3, 8] * 3
    cp, ci = _sorted_include([4, 2], 2)                     # a plain list of two ids is a shared list, not a CSR pair
    assert cp.tolist() == [0, 2, 4] and ci.tolist() == [2, 4, 2, 4]


def test_scipy_csr_is_taken_like_exclude():
    sp = pytest.importorskip("scipy.sparse")
    from cmfrec_amd.ops import _sorted_include
    M = sp.csr_matrix((np.ones(4), np.array([5, 1, 0, 3]), np.array([0, 2, 2, 4])), shape=(3, 6))
    cp, ci = _sorted_include(M, 3)
    assert cp.tolist() == [0, 2, 2, 4] and ci.tolist() == [1, 5, 0, 3]


def test_malformed_include_raises_before_the_library(monkeypatch):
    from cmfrec_amd import Ranker, _lib, ops

    def no_library(*a, **kw):
        raise AssertionError("the library was touched")
    A = np.zeros((3, 8)); B = np.zeros((20, 8))
    ix = np.arange(6)
    bad = [((np.array([0, 2, 6]), ix), "one entry per user plus one"),          # wrong number of offsets
           ((np.array([0, 4, 2, 6]), ix), "must not decrease"),                 # decreasing offsets
           ((np.array([0, 2, 4, 5]), ix), "last entry of indptr"),              # last offset != len(indices)
           ((np.array([0, 2, 4, 7]), ix), "last entry of indptr"),
           ((np.array([0, 2, 4, 6]), ix.astype(np.float64)), "must be integers"),   # non-integer ids
           (np.array([1.5, 2.0]), "must be integers")]
    r = Ranker.__new__(Ranker)                               # a ranker's argument checks without its device
    r.handle = 1; r.k = 8; r.n = 20; r.dtype = np.dtype(np.float64); r.lib = None
    monkeypatch.setattr(_lib, "load", no_library)
    for inc, msg in bad:
        with pytest.raises(ValueError, match=msg):
            ops._sorted_include(inc, 3)
        with pytest.raises(ValueError, match=msg):
            Ranker.topN(r, A, n=5, include=inc)
    r.handle = None


def test_topN_batch_refuses_malformed_include_before_the_device():
    """ops.topN_batch loads the library first (as for ``exclude``), but no call reaches it: on a machine without a GPU a call
    that got through would raise RuntimeError, not ValueError."""
    from cmfrec_amd import ops
    with pytest.raises(ValueError, match="must not decrease"):
        ops.topN_batch(np.zeros((3, 8)), np.zeros((20, 8)), n_top=5, include=(np.array([0, 4, 2, 6]), np.arange(6)))


def test_candidate_names_are_exported():
    from cmfrec_amd import _lib
    names = ["cmfrec_hip_ranker_topN_candidates", "cmfrec_hip_topN_candidates_batch", "cmfrec_hip_newrows_topN_candidates"]
    txt = open(os.path.join(ROOT, "cmfrec_amd", "csrc", "exports.map")).read()
    assert "cmfrec_hip_*;" in txt                            # the pattern that covers them
    hdr = open(os.path.join(ROOT, "include", "cmfrec_hip.h")).read()
    for dt in (np.float64, np.float32):
        lib = _lib.load(dt)
        for nm in names:
            assert nm in _lib.EXPORTED and nm + "(" in hdr
            assert hasattr(lib, nm), nm


def test_candidate_limits_need_no_gpu():
    """k = 273 and n_top = 129 answer code 2 with the ranking's message before anything touches a device; so does a call
    without candidate offsets at the C level."""
    import ctypes as C
    from cmfrec_amd import _lib, ops
    shared = np.arange(50)
    with pytest.raises(RuntimeError, match=r"code 2.*k <= 272"):
        ops.topN_batch(np.zeros((4, 273)), np.zeros((300, 273)), n_top=5, include=shared)
    with pytest.raises(RuntimeError, match=r"code 2.*n_top <= min\(128, n\)"):
        ops.topN_batch(np.zeros((4, 100)), np.zeros((300, 100)), n_top=129, include=shared)
    with pytest.raises(RuntimeError, match=r"code 2.*n_top <= min\(128, n\)"):
        ops.topN_batch(np.zeros((4, 100)), np.zeros((20, 100)), n_top=21, include=shared)
    lib = _lib.load(np.float64)
    A = np.zeros((4, 8)); B = np.zeros((30, 8)); ids = np.full((4, 5), 77, np.int32)
    rc = lib.cmfrec_hip_topN_candidates_batch(_lib.ptr(A), C.c_size_t(8), C.c_int(4), _lib.ptr(B), C.c_size_t(8), C.c_int(30), C.c_int(8),
                                              None, None, None, None, None, C.c_int(5), _lib.ptr(ids), None)
    assert rc == 2 and b"cmfrec_hip_topN_candidates_batch: invalid arguments" in lib.cmfrec_hip_last_error()
    assert (ids == 77).all()
