"""CPU: every refusal of the top-N entry points of the C interface that returns before a device is touched -- the exact text of
cmfrec_hip_last_error(), code 2, the outputs untouched.  Which of two failing checks is reported is part of the interface
(cmfrec_hip_topN_deep_batch names its limits before a missing out_ids), so a case may break two rules at once."""
import ctypes as C

import numpy as np
import pytest

NU, N, K, NTOP = 3, 5, 8, 2
SENTINEL = 77

INVALID = "%s: invalid arguments"
LIMITS = "%s: needs k <= 272 and n_top <= min(128, n)"
DEEP_LIMITS = "%s: needs k <= 272 and 1 <= n_top <= n"
RANK_LIMITS = "%s: needs k <= 272"
NO_CALL = "%s: no ranking call on this handle yet"

# the arguments of each entry point, in the header's order
SIGNATURES = {
    "cmfrec_hip_topN_batch": "A lda nu B ldb n k biasB excl_p excl_i n_top out_ids out_scores",
    "cmfrec_hip_topN_deep_batch": "A lda nu B ldb n k biasB excl_p excl_i n_top out_ids out_scores",
    "cmfrec_hip_topN_candidates_batch": "A lda nu B ldb n k biasB cand_p cand_i excl_p excl_i n_top out_ids out_scores",
    "cmfrec_hip_similar_batch": "B ldb n k query_ids nq metric excl_p excl_i n_top out_ids out_scores",
    "cmfrec_hip_ranks_batch": "A lda nu B ldb n k biasB held_p held_i excl_p excl_i out_rank out_scores out_pool",
    "cmfrec_hip_ranker_topN": "r A lda nu excl_p excl_i n_top out_ids out_scores",
    "cmfrec_hip_ranker_topN_candidates": "r A lda nu cand_p cand_i excl_p excl_i n_top out_ids out_scores",
    "cmfrec_hip_ranker_topN_deep": "r A lda nu excl_p excl_i n_top out_ids out_scores",
    "cmfrec_hip_ranker_topN_after": "r A lda nu excl_p excl_i after_ids after_scores n_top out_ids out_scores",
    "cmfrec_hip_ranker_ranks": "r A lda nu held_p held_i excl_p excl_i out_rank out_scores out_pool",
    "cmfrec_hip_ranker_similar": "r query_ids nq metric excl_p excl_i n_top out_ids out_scores",
    "cmfrec_hip_ranker_metrics": "r A lda m set k_at record per_user out_rank",
    "cmfrec_hip_ranker_filter_keys": "r A lda nu keys",
    "cmfrec_hip_ranker_inverse_norms": "r norms",
    "cmfrec_hip_ranker_set_filter": "r mode",
    "cmfrec_hip_ranker_set_split": "r mode",
    "cmfrec_hip_ranker_filter_stats": "r int0 int1 int2",
    "cmfrec_hip_ranker_filter_ms": "r ms",
    "cmfrec_hip_ranker_pages": "r int0 int1",
    "cmfrec_hip_ranker_kernel_ms": "r ms",
    "cmfrec_hip_ranker_slices": "r int0",
    "cmfrec_hip_ranker_launch_shape": "r int0 int1",
}
SIZES = ("lda", "ldb")
COUNTS = ("nu", "n", "k", "n_top", "nq", "metric", "m", "k_at", "mode")
TYPED = dict(int0=C.c_int, int1=C.c_int, int2=C.c_int, ms=C.c_double)             # pointers the binding declares with their type
OUTPUTS = ("out_ids", "out_scores", "out_rank", "out_pool", "keys", "norms", "ms", "int0", "int1", "int2")

# (entry point, the arguments that differ from a well-formed call, the message); None is a null pointer
BATCH_CASES = [
    ("cmfrec_hip_topN_batch", dict(A=None), INVALID),
    ("cmfrec_hip_topN_batch", dict(B=None), INVALID),
    ("cmfrec_hip_topN_batch", dict(out_ids=None), INVALID),
    ("cmfrec_hip_topN_batch", dict(n_top=0), INVALID),
    ("cmfrec_hip_topN_batch", dict(k=273), LIMITS),
    ("cmfrec_hip_topN_batch", dict(n=300, n_top=129), LIMITS),
    ("cmfrec_hip_topN_batch", dict(n_top=N + 1), LIMITS),
    ("cmfrec_hip_topN_batch", dict(k=273, out_ids=None), INVALID),            # the null pointers lead here
    ("cmfrec_hip_topN_deep_batch", dict(A=None), INVALID),
    ("cmfrec_hip_topN_deep_batch", dict(B=None), INVALID),
    ("cmfrec_hip_topN_deep_batch", dict(out_ids=None), INVALID),
    ("cmfrec_hip_topN_deep_batch", dict(k=273), DEEP_LIMITS),
    ("cmfrec_hip_topN_deep_batch", dict(n_top=0), DEEP_LIMITS),
    ("cmfrec_hip_topN_deep_batch", dict(n_top=N + 1), DEEP_LIMITS),
    ("cmfrec_hip_topN_deep_batch", dict(k=273, out_ids=None), DEEP_LIMITS),   # out_ids is checked last: the limits are reported
    ("cmfrec_hip_topN_deep_batch", dict(n_top=0, out_ids=None), DEEP_LIMITS),
    ("cmfrec_hip_topN_deep_batch", dict(k=273, A=None), INVALID),             # ... but A and B in front of the limits
    ("cmfrec_hip_topN_candidates_batch", dict(A=None), INVALID),
    ("cmfrec_hip_topN_candidates_batch", dict(B=None), INVALID),
    ("cmfrec_hip_topN_candidates_batch", dict(out_ids=None), INVALID),
    ("cmfrec_hip_topN_candidates_batch", dict(cand_p=None), INVALID),
    ("cmfrec_hip_topN_candidates_batch", dict(k=273), LIMITS),
    ("cmfrec_hip_topN_candidates_batch", dict(n=300, n_top=129), LIMITS),
    ("cmfrec_hip_topN_candidates_batch", dict(n_top=N + 1), LIMITS),
    ("cmfrec_hip_similar_batch", dict(B=None), INVALID),
    ("cmfrec_hip_similar_batch", dict(nq=-1), INVALID),
    ("cmfrec_hip_similar_batch", dict(k=273), LIMITS),
    ("cmfrec_hip_similar_batch", dict(n=300, n_top=129), LIMITS),
    ("cmfrec_hip_similar_batch", dict(n_top=N + 1), LIMITS),
    ("cmfrec_hip_ranks_batch", dict(A=None), INVALID),
    ("cmfrec_hip_ranks_batch", dict(B=None), INVALID),
    ("cmfrec_hip_ranks_batch", dict(held_p=None), INVALID),
    ("cmfrec_hip_ranks_batch", dict(k=273), RANK_LIMITS),
    ("cmfrec_hip_ranks_batch", dict(k=273, held_p=None), INVALID),
]

# a null handle to every call that takes one
NULL_HANDLE_CASES = [
    ("cmfrec_hip_ranker_topN", INVALID),
    ("cmfrec_hip_ranker_topN_candidates", INVALID),
    ("cmfrec_hip_ranker_topN_deep", INVALID),
    ("cmfrec_hip_ranker_topN_after", INVALID),
    ("cmfrec_hip_ranker_ranks", INVALID),
    ("cmfrec_hip_ranker_similar", INVALID),
    ("cmfrec_hip_ranker_metrics", INVALID),
    ("cmfrec_hip_ranker_filter_keys", INVALID),
    ("cmfrec_hip_ranker_inverse_norms", INVALID),
    ("cmfrec_hip_ranker_set_filter", "%s: invalid arguments (0: off, 1: the half-precision filter)"),
    ("cmfrec_hip_ranker_set_split", "%s: invalid arguments (-1: off, 0: the planner's choice, >= 1: that many slices)"),
    ("cmfrec_hip_ranker_filter_stats", "%s: no cmfrec_hip_ranker_topN call on this handle yet"),
    ("cmfrec_hip_ranker_filter_ms", "%s: the filter of this handle is off"),
    ("cmfrec_hip_ranker_pages", "%s: no deep ranking call on this handle yet"),
    ("cmfrec_hip_ranker_kernel_ms", NO_CALL),
    ("cmfrec_hip_ranker_slices", NO_CALL),
    ("cmfrec_hip_ranker_launch_shape", NO_CALL),
]


def _wellformed(dtype):
    """A well-formed call's arguments by name; every output is filled with the sentinel."""
    a = dict(nu=NU, n=N, k=K, n_top=NTOP, nq=NU, metric=1, m=NU, k_at=2, mode=0, lda=K, ldb=K, r=None, biasB=None, excl_p=None, excl_i=None,
             set=None, record=None, per_user=None)
    a["A"] = np.zeros((NU, 300), dtype); a["B"] = np.ones((N, 300), dtype)          # (wide enough for ld = 273)
    a["cand_p"] = a["held_p"] = np.array([0, 1, 2, 3], np.uint64)
    a["cand_i"] = a["held_i"] = np.array([0, 1, 2], np.int32)
    a["query_ids"] = a["after_ids"] = np.zeros(NU, np.int32)
    a["after_scores"] = np.zeros(NU, dtype)
    for name in ("out_ids", "out_rank", "out_pool"):
        a[name] = np.full(NU * 130, SENTINEL, np.int32)
    for name in ("int0", "int1", "int2"):
        a[name] = np.full(1, SENTINEL, np.int32)
    for name in ("out_scores", "norms"):
        a[name] = np.full(NU * 130, SENTINEL, dtype)
    a["keys"] = np.full(NU * N, SENTINEL, np.float32)
    a["ms"] = np.full(4, SENTINEL, np.float64)
    return a


def _refused(lib, fn, args, message):
    from cmfrec_amd import _lib
    args["lda"] = args["ldb"] = args["k"]
    call = []
    for name in SIGNATURES[fn].split():
        v = args[name]
        if name in SIZES:
            call.append(C.c_size_t(v))
        elif name in COUNTS:
            call.append(C.c_int(v))
        elif name in TYPED and v is not None:
            call.append(v.ctypes.data_as(C.POINTER(TYPED[name])))
        else:
            call.append(_lib.ptr(v))
    rc = getattr(lib, fn)(*call)
    assert rc == 2, (fn, rc)
    assert lib.cmfrec_hip_last_error().decode() == message % fn
    for name in OUTPUTS:
        if args.get(name) is not None:
            assert np.all(args[name] == SENTINEL), (fn, name)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_batch_refusals(dtype):
    from cmfrec_amd import _lib
    lib = _lib.load(dtype)
    for fn, changed, message in BATCH_CASES:
        args = _wellformed(dtype)
        args.update(changed)
        _refused(lib, fn, args, message)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_null_handle_refusals(dtype):
    from cmfrec_amd import _lib
    lib = _lib.load(dtype)
    for fn, message in NULL_HANDLE_CASES:
        _refused(lib, fn, _wellformed(dtype), message)
    lib.cmfrec_hip_ranker_destroy(None)                      # a no-op


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_create_refusals(dtype):
    """cmfrec_hip_ranker_create answers with a null handle; the code is cmfrec_hip_last_error_code()."""
    from cmfrec_amd import _lib
    lib = _lib.load(dtype)
    B = np.ones((N, 300), dtype)
    create = lambda B, ldb, n, k: lib.cmfrec_hip_ranker_create(_lib.ptr(B), C.c_size_t(ldb), C.c_int(n), C.c_int(k), None, C.c_int(-1))
    for call, message in ((lambda: create(None, K, N, K), INVALID), (lambda: create(B, K - 1, N, K), INVALID), (lambda: create(B, K, 0, K), INVALID),
                          (lambda: create(B, 273, N, 273), LIMITS)):
        assert call() is None
        assert lib.cmfrec_hip_last_error_code() == 2
        assert lib.cmfrec_hip_last_error().decode() == message % "cmfrec_hip_ranker_create"


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_split_plan_refusals(dtype):
    from cmfrec_amd import _lib
    lib = _lib.load(dtype)
    message = "cmfrec_hip_topn_split_plan: invalid arguments (needs k <= 272 and n_top <= min(128, n); sizeof_real 4 or 8; requested >= 0)"
    good = dict(nu=4, n=3000, k=100, n_top=10, num_cus=256, sizeof_real=8, requested=0)
    for bad in (dict(sizeof_real=2), dict(sizeof_real=0), dict(k=273), dict(n_top=129), dict(n=50, n_top=51), dict(n_top=0), dict(nu=0),
                dict(num_cus=0), dict(requested=-1), dict(slices=None), dict(slice_items=None)):
        a = dict(good, slices=C.c_int(SENTINEL), slice_items=C.c_int(SENTINEL))
        a.update(bad)
        rc = lib.cmfrec_hip_topn_split_plan(a["nu"], a["n"], a["k"], a["n_top"], a["num_cus"], a["sizeof_real"], a["requested"],
                                            *(None if a[o] is None else C.byref(a[o]) for o in ("slices", "slice_items")))
        assert rc == 2, bad
        assert lib.cmfrec_hip_last_error().decode() == message
        assert all(v is None or v.value == SENTINEL for v in (a["slices"], a["slice_items"]))
    a = dict(good, slices=C.c_int(SENTINEL), slice_items=C.c_int(SENTINEL))
    assert lib.cmfrec_hip_topn_split_plan(4, 3000, 100, 10, 256, 4, 0, C.byref(a["slices"]), C.byref(a["slice_items"])) == 0
    assert a["slices"].value >= 1 and a["slice_items"].value % 128 == 0
