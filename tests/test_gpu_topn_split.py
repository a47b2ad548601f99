"""GPU: the full ranking over item slices (topn_split_kernels.hpp: slice pass + merge kernel, ``Ranker(split=...)``).

The main property: whatever the number of slices, ids and scores equal the unsplit MFMA kernel's bit for bit (for k <= 64 that
is the kernel of CMFREC_HIP_TOPN=wide).  Then the float64 ranking of topn_reference.py, the corner cases of a cut (an emptied
slice, a short tail, ties across slices, NaN rows, n_top == n) and what the handle reports."""
import ctypes as C

import numpy as np
import pytest

import topn_reference as tr

pytestmark = pytest.mark.gpu

ITEMS = 128
WIDTHS = [(np.float64, k) for k in (3, 50, 64, 65, 128)] + [(np.float32, k) for k in (3, 50, 64, 65, 128, 272)]
SIZES = (127, 131, 1000)                      # a partial single round; two rounds, the second partial; eight rounds
USERS = (1, 2, 17, 33)                        # one tile (partly filled); two and three tiles
TOPS = (1, 10, 33, 128)
ids_of = lambda v: getattr(v, "__name__", str(v))


def _sub(ep, ei, nu):
    """The exclusion lists of the first nu users."""
    if ep is None:
        return None
    return ep[:nu + 1].copy(), ei[:int(ep[nu])].copy()


def _unsplit(monkeypatch, r, A, n_top, excl, k):
    """The yardstick: the same Ranker with the split off, on the MFMA kernel."""
    r.split = None
    if k <= 64:
        monkeypatch.setenv("CMFREC_HIP_TOPN", "wide")
    try:
        out = r.topN(A, n=n_top, exclude=excl)
        assert r.slices() == 1
    finally:
        monkeypatch.delenv("CMFREC_HIP_TOPN", raising=False)
    return out


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("dtype,k", WIDTHS, ids=ids_of)
def test_split_equals_unsplit_bitwise(monkeypatch, dtype, k, bias):
    from cmfrec_amd import Ranker
    monkeypatch.delenv("CMFREC_HIP_TOPN", raising=False)
    monkeypatch.delenv("CMFREC_HIP_TOPN_TILES", raising=False)
    for n in SIZES:
        rounds = (n + ITEMS - 1) // ITEMS
        A, B, b, ep, ei = tr.make_problem(31 * k + n, dtype, max(USERS), n, k, bias=bias)
        with Ranker(B, b) as r:
            for nu in USERS:
                excl = _sub(ep, ei, nu)
                for n_top in TOPS:
                    n_top = min(n_top, n)                    # (n = 127: the list is the whole catalogue)
                    want_ids, want_sc = _unsplit(monkeypatch, r, A[:nu], n_top, excl, k)
                    for slices in (1, 2, 3, 7, rounds, 100):
                        r.split = slices
                        ids, sc = r.topN(A[:nu], n=n_top, exclude=excl)
                        case = (n, nu, n_top, slices)
                        assert 1 <= r.slices() <= rounds, case
                        if rounds % min(slices, rounds) == 0:
                            assert r.slices() == min(slices, rounds), case
                        assert np.array_equal(ids, want_ids), case
                        assert sc.tobytes() == want_sc.tobytes(), case
                    r.split = "auto"
                    ids, sc = r.topN(A[:nu], n=n_top, exclude=excl)
                    assert np.array_equal(ids, want_ids) and sc.tobytes() == want_sc.tobytes(), (n, nu, n_top, "auto")


@pytest.mark.parametrize("dtype,k", [(np.float64, 50), (np.float32, 272)], ids=ids_of)
def test_split_without_scores(monkeypatch, dtype, k):
    """out_scores = NULL through the C entry point: the merge writes the ids alone."""
    from cmfrec_amd import Ranker, _lib
    monkeypatch.delenv("CMFREC_HIP_TOPN", raising=False)
    nu, n, n_top = 17, 1000, 33
    A, B, b, ep, ei = tr.make_problem(5, dtype, nu, n, k)
    with Ranker(B, b) as r:
        want_ids, _ = _unsplit(monkeypatch, r, A, n_top, (ep, ei), k)
        r.split = 3
        owner = np.repeat(np.arange(nu), np.diff(ep.astype(np.int64)))
        eis = np.ascontiguousarray(ei[np.lexsort((ei, owner))])
        ids = np.empty((nu, n_top), np.int32)
        rc = r.lib.cmfrec_hip_ranker_topN(r.handle, _lib.ptr(A), C.c_size_t(k), C.c_int(nu), _lib.ptr(ep), _lib.ptr(eis), C.c_int(n_top),
                                          _lib.ptr(ids), None)
        _lib.check(rc, r.lib, "ranker_topN")
        assert r.slices() == 3 and np.array_equal(ids, want_ids)


@pytest.mark.parametrize("split", ["auto", 7])
@pytest.mark.parametrize("dtype,k,n_top", [(np.float64, 128, 10), (np.float32, 272, 128), (np.float64, 50, 100)], ids=ids_of)
def test_split_against_float64_ranking(dtype, k, n_top, split):
    """The four conditions of topn_reference.check_ranking on the split result, as test_gpu_topn_wide.py asks of the wide kernel."""
    from cmfrec_amd import Ranker
    nu, n = 33, 3000
    A, B, b, ep, ei = tr.make_problem(1000 * k + n_top, dtype, nu, n, k)
    with Ranker(B, b, split=split) as r:
        ids, sc = r.topN(A, n=n_top, exclude=(ep, ei))
        assert r.slices() > 1
    tr.check_ranking(A, B, b, ep, ei, ids, sc, n_top, dtype, all_decided=dtype is np.float64)


@pytest.mark.parametrize("dtype,k", [(np.float64, 128), (np.float32, 272), (np.float64, 8)], ids=ids_of)
def test_split_corner_cases(monkeypatch, dtype, k):
    """Eight slices of one round each: a user whose exclusion list empties slice 1, users with fewer than n_top items left (or
    none), a NaN row, and rows with equal bits in different slices (lower id first)."""
    from cmfrec_amd import Ranker
    monkeypatch.delenv("CMFREC_HIP_TOPN", raising=False)
    nu, n, n_top = 20, 1000, 10
    A, B, b, _, _ = tr.make_problem(9, dtype, nu, n, k, excl=False)
    B[5, k // 2] = np.nan
    B[700] = B[3]; b[700] = b[3]                             # (3, 7, 11 tie in slice 0 already; 700 lies in slice 5)
    b[[3, 7, 11, 700]] = 1000                                # every user likes exactly those rows best (|A_u . B_i| stays below 200)
    rng = np.random.default_rng(10)
    lists = [np.zeros(0, np.int64)] * nu
    lists[1] = np.arange(128, 256)                           # all of slice 1
    lists[2] = np.setdiff1d(np.arange(n), [10, 500, 999])    # three items left
    lists[3] = np.arange(n)                                  # nothing left
    lists[4] = rng.choice(n, 17, replace=False)
    lists[6] = np.setdiff1d(np.arange(n), [130, 900])        # two items left, in different slices
    ep = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
    ei = np.concatenate(lists).astype(np.int32)
    with Ranker(B, b) as r:
        want_ids, want_sc = _unsplit(monkeypatch, r, A, n_top, (ep, ei), k)
        r.split = 8
        ids, sc = r.topN(A, n=n_top, exclude=(ep, ei))
        assert r.slices() == 8
        again = r.topN(A, n=n_top, exclude=(ep, ei))
    assert np.array_equal(ids, want_ids) and sc.tobytes() == want_sc.tobytes()
    assert np.array_equal(again[0], ids) and again[1].tobytes() == sc.tobytes()          # the same call twice: the same bytes
    assert not (ids == 5).any()
    assert list(ids[0, :4]) == [3, 7, 11, 700] and len(set(sc[0, :4].tolist())) == 1
    assert not ((ids[1] >= 128) & (ids[1] < 256)).any() and (ids[1] >= 0).all()
    assert (ids[2, :3] >= 0).all() and (ids[2, 3:] == -1).all() and np.isneginf(sc[2, 3:]).all() and np.isfinite(sc[2, :3]).all()
    assert (ids[3] == -1).all() and np.isneginf(sc[3]).all()
    assert sorted(ids[6, :2].tolist()) == [130, 900] and (ids[6, 2:] == -1).all() and np.isneginf(sc[6, 2:]).all()
    # the float64 ranking: item 5 (a zero row there, NaN-free) excluded for every user
    Bok = B.copy(); Bok[5] = 0
    l5 = [np.union1d(l, [5]).astype(np.int32) for l in lists]
    ep5 = np.concatenate([[0], np.cumsum([len(l) for l in l5])]).astype(np.uint64)
    tr.check_ranking(A, Bok, b, ep5, np.concatenate(l5), ids, sc, n_top, dtype, all_decided=dtype is np.float64)


@pytest.mark.parametrize("dtype,k", [(np.float64, 65), (np.float32, 50)], ids=ids_of)
def test_list_as_long_as_the_catalogue(monkeypatch, dtype, k):
    """n_top == n with more slices than a list has room for per slice: every item comes back once, in order."""
    from cmfrec_amd import Ranker
    monkeypatch.delenv("CMFREC_HIP_TOPN", raising=False)
    nu, n = 17, 128
    A, B, b, _, _ = tr.make_problem(3, dtype, nu, n, k, excl=False)
    with Ranker(B, b) as r:                                  # (n = 128: one round, so one slice whatever is asked)
        want = _unsplit(monkeypatch, r, A, n, None, k)
        r.split = 4
        got = r.topN(A, n=n)
        assert r.slices() == 1
    assert np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes()
    n = 300                                                  # three rounds, lists of 128 from slices of 128, 128 and 44 items
    A, B, b, _, _ = tr.make_problem(4, dtype, nu, n, k, excl=False)
    with Ranker(B, b) as r:
        want = _unsplit(monkeypatch, r, A, 128, None, k)
        r.split = 3
        got = r.topN(A, n=128)
        assert r.slices() == 3
    assert np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes()
    assert all(len(set(row.tolist())) == 128 for row in got[0])


@pytest.mark.parametrize("dtype,k", [(np.float64, 50), (np.float64, 128), (np.float32, 272)], ids=ids_of)
def test_what_the_handle_reports(monkeypatch, dtype, k):
    """slices(): > 1 for one user under "auto" on 4096 items, 1 with the split off; the launch of a split-off call is the launch
    of a ranker that never had the setting; the setting leaves include / topN_deep alone."""
    from cmfrec_amd import Ranker
    monkeypatch.delenv("CMFREC_HIP_TOPN", raising=False)
    monkeypatch.delenv("CMFREC_HIP_TOPN_TILES", raising=False)
    n, n_top = 4096, 10
    A, B, b, ep, ei = tr.make_problem(k, dtype, 33, n, k)
    with Ranker(B, b) as plain, Ranker(B, b, split="auto") as r:
        assert r.split == "auto" and plain.split is None
        for nu in (1, 33):
            excl = _sub(ep, ei, nu)
            p_ids, p_sc = plain.topN(A[:nu], n=n_top, exclude=excl)
            assert plain.slices() == 1
            users, groups = plain.launch_shape()
            if k <= 64:
                assert (users, groups) == (16, (nu + 15) // 16)
            else:
                assert users in (16, 32, 48, 64) and groups == (nu + users - 1) // users
            r.split = "auto"
            s_ids, s_sc = r.topN(A[:nu], n=n_top, exclude=excl)
            if nu == 1:
                assert r.slices() > 1
            assert r.launch_shape()[1] == r.slices() * ((nu + r.launch_shape()[0] - 1) // r.launch_shape()[0])
            assert r.kernel_ms() > 0
            assert np.array_equal(s_ids, p_ids)
            if k > 64:
                assert s_sc.tobytes() == p_sc.tobytes()
            else:
                E = tr.bounds(A[:nu], B, b, dtype)
                assert np.all(np.abs(s_sc.astype(np.float64) - p_sc.astype(np.float64)) <= 2 * E[:, None])
            r.split = None                                   # off again: the launch and the bits of the plain handle
            o_ids, o_sc = r.topN(A[:nu], n=n_top, exclude=excl)
            assert r.slices() == 1 and r.launch_shape() == (users, groups)
            assert np.array_equal(o_ids, p_ids) and o_sc.tobytes() == p_sc.tobytes()
        r.split = 5
        inc = np.arange(0, n, 7)
        a = r.topN(A, n=n_top, include=inc); c = plain.topN(A, n=n_top, include=inc)
        assert r.slices() == 1 and np.array_equal(a[0], c[0]) and a[1].tobytes() == c[1].tobytes()
        a = r.topN_deep(A, 200); c = plain.topN_deep(A, 200)
        assert r.slices() == 1 and np.array_equal(a[0], c[0]) and a[1].tobytes() == c[1].tobytes()
        with pytest.raises(RuntimeError, match=r"code 2.*n_top <= min\(128, n\)"):
            r.topN(A, n=129)
