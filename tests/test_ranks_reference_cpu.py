"""CPU: the float64 reference of the rank tests (ranks_reference.py) against a full lexsort, and the cap on the pairs its
allowance leaves undecided, on the exact inputs test_gpu_ranks.py::test_several_rounds uses (same generator, seed, shapes: a
change of any of them passes through here)."""
import numpy as np
import pytest

import ranks_reference as rr
import topn_reference as tr


@pytest.mark.parametrize("dtype,k,n", rr.ROUND_CASES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_cap_on_undecided_pairs(dtype, k, n):
    A, B, b, excl, held = rr.round_problem(dtype, k, n)
    assert A.shape == (rr.NU, k) and B.shape == (n, k) and A.dtype == dtype
    assert np.all(np.diff(held[0].astype(np.int64)) == rr.HELD)
    assert {3, 7, 11} <= set(rr.lists_of_csr(*held)[1].tolist())
    r64, near, pool = rr.ranks64(A, B, b, held, excl, dtype)
    share = rr.near_share(r64, near)
    print("ranks: dtype=%s k=%d n=%d: the float64 reference leaves %.4f of the pairs undecided" % (np.dtype(dtype).name, k, n, share))
    assert share <= rr.CAP[dtype]
    assert (r64 >= 0).sum() > 0.5 * len(r64)                         # most targets are ranked (some are in the exclusion lists)
    assert (r64 < 0).any()


def test_reference_against_lexsort():
    """ranks64 is the place in the user's full float64 ranking; excluded, out-of-range and NaN targets are -1; the pool counts
    what can be ranked."""
    dtype, nu, n, k = np.float64, 9, 40, 5
    A, B, b, excl = rr.small_problem(3, dtype, nu, n, k, True, True)
    B[20] = np.nan
    held = rr.csr_of_lists([np.concatenate([[-1], np.arange(n), [n]])] * nu)
    r64, near, pool = rr.ranks64(A, B, b, held, excl, dtype)
    S = tr.scores64(A, B, b)
    for u, ex in enumerate(rr.lists_of_csr(*excl)):
        ids = np.setdiff1d(np.arange(n), np.concatenate([ex, [20]]))
        order = ids[np.lexsort((ids, -S[u, ids]))]
        want = np.full(n + 2, -1)
        want[order + 1] = np.arange(len(order))
        assert np.array_equal(r64[u * (n + 2):(u + 1) * (n + 2)], want), u
        assert pool[u] == len(order)
    # the planted equal rows are exact ties in float64: not "near", ordered by id
    assert np.all(S[:, 3] == S[:, 7]) and np.all(S[:, 7] == S[:, 11])
    assert near.max() == 0
