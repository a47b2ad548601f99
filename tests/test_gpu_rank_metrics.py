"""The ranking metrics reduced on the device (cmfrec_hip_rankset_*, cmfrec_hip_ranker_metrics, cmfrec_hip_session_ranking;
rank_metrics_kernels.hpp): 300 items, 70 users whose held-out lists have 0, 1, 2, 63, 64, 65 and 200 entries with items outside the
model among them, one user without a rankable item, one whose exclusions leave P = T.  The ranks are Ranker.ranks' bit for bit, the
record and the per-user values are held by tests/rank_metrics_reference.py's check, the same call gives the same bytes, a capped
launch the same integers; a session's record is the record of its downloaded factors."""
import numpy as np
import pytest

import rank_metrics_reference as rr

pytestmark = pytest.mark.gpu

M, N = 100, 300
LENS = [0, 1, 2, 63, 64, 65, 200] * 10


def _lists(seed=11):
    """(users [70], heldout (indptr, items), exclude (indptr, items)) over the 70 users of the set."""
    rng = np.random.default_rng(seed)
    users = rng.permutation(M)[:len(LENS)].astype(np.int32)
    hp, hi, ep, ei = [0], [], [0], []
    for u, ln in enumerate(LENS):
        items = rng.choice(N, size=ln, replace=False)
        out = rng.random(ln) < 0.1
        items[out] = N + rng.choice(40, size=int(out.sum()), replace=False)          # outside the model: rank -1
        excl = rng.choice(N, size=int(rng.integers(0, 25)), replace=False)             # may take held-out items away: rank -1
        if u == 8:                                                                     # one entry, outside: T = 0
            items = np.array([N + 3])
        if u == 9:                                                                     # two entries and everything else excluded: P = T
            items = np.array([5, 17])
            excl = np.setdiff1d(np.arange(N), items)
        hi.append(np.sort(items)); hp.append(hp[-1] + len(items))
        ei.append(np.sort(excl)); ep.append(ep[-1] + len(excl))
    cat = lambda parts: np.concatenate(parts).astype(np.int32)
    return users, (np.array(hp, np.uint64), cat(hi)), (np.array(ep, np.uint64), cat(ei))


def _same_bytes(a, b):
    return all(np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes() for key in ("sum", "count", "users"))


@pytest.mark.parametrize("kk", [3, 50, 65, 272])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_ranker_metrics(dtype, kk, monkeypatch):
    from cmfrec_amd import Ranker, RankSet
    rng = np.random.default_rng(kk)
    A = rng.standard_normal((M, kk)).astype(dtype); B = rng.standard_normal((N, kk)).astype(dtype)
    users, held, excl = _lists()
    with Ranker(B) as rk, RankSet(users, held, excl, dtype=dtype) as rs:
        ip, items, ranks, pool = rk.ranks(A[users], held, exclude=excl)
        assert np.array_equal(ip, rs.indptr) and np.array_equal(items, rs.items)
        T = np.array([(ranks[ip[u]:ip[u + 1]] >= 0).sum() for u in range(len(users))])
        assert T[8] == 0 and T[9] == 2 and pool[9] == 2 and T.max() > 128 and (ranks < 0).sum() > 20
        for k_at in (1, 10, 250):
            rec, per_user, got_ranks = rk.metrics(A, rs, k=k_at, per_user=True, return_ranks=True)
            assert got_ranks.dtype == ranks.dtype and np.array_equal(got_ranks, ranks)
            worst = rr.check(rec, ip, ranks, pool, k_at, per_user=per_user, what="%s kk=%d k=%d" % (np.dtype(dtype).name, kk, k_at))
            print("rank metrics %s kk=%d k_at=%d: error / bound %.3g" % (np.dtype(dtype).name, kk, k_at, worst))
            assert int(rec["users"]) == int((T > 0).sum()) and int(rec["count"][6]) == int(rec["users"]) - 1
            again = rk.metrics(A, rs, k=k_at)
            assert _same_bytes(again, rec), "the same call, other bytes"
            monkeypatch.setenv("CMFREC_HIP_RANKMETRIC_WAVES", "4")                     # 70 users on four wavefronts: many in a row
            capped, capped_pu = rk.metrics(A, rs, k=k_at, per_user=True)
            monkeypatch.delenv("CMFREC_HIP_RANKMETRIC_WAVES")
            assert np.array_equal(capped["count"], rec["count"]) and capped["users"] == rec["users"]
            assert capped_pu.tobytes() == per_user.tobytes()                          # a user's values do not depend on the launch
            rr.check(capped, ip, ranks, pool, k_at, what="capped launch")


def test_rankset_refusals():
    from cmfrec_amd import Ranker, RankSet
    users, held, excl = _lists()
    B = np.random.default_rng(0).standard_normal((N, 8))
    with pytest.raises(ValueError):
        RankSet(np.array([-1, 2]), (np.array([0, 1, 2]), np.array([1, 2])))
    with pytest.raises(ValueError):
        RankSet(users, (held[0][:-1], held[1]))
    with Ranker(B) as rk, RankSet(users, held, excl) as rs:
        with pytest.raises(RuntimeError, match="code 2"):
            rk.metrics(np.zeros((int(users.max()), 8)), rs)                            # a user beyond the rows of A
        with pytest.raises(ValueError, match="ranking set is"):
            Ranker(B.astype(np.float32)).metrics(np.zeros((M, 8), np.float32), rs)
        with pytest.raises(ValueError):
            rk.metrics(np.zeros((M, 8)), rs, k=0)
    with Ranker(B) as rk, RankSet(np.zeros(0, np.int32), (np.zeros(1, np.uint64), np.zeros(0, np.int32))) as empty:
        rec = rk.metrics(np.zeros((M, 8)), empty)
        assert int(rec["users"]) == 0 and not rec["sum"].any() and not rec["count"].any()


@pytest.mark.parametrize("implicit", [True, False], ids=["implicit", "explicit"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_session_ranking(dtype, implicit):
    """AlsSession.ranking is Ranker.metrics on the downloaded factors -- integers exactly, sums within the bound -- after one
    iteration and again after a second one (the session's ranker follows B where it lives)."""
    from cmfrec_amd import AlsSession, Ranker, RankSet
    k, km = 7, 1
    rng = np.random.default_rng(23)
    at = rng.choice(M * N, 2500, replace=False)
    row, col = (at // N).astype(np.int32), (at % N).astype(np.int32)
    val = rng.integers(1, 5, 2500).astype(dtype)
    gm = 0.0 if implicit else float(np.dtype(dtype).type(val.mean()))
    bias = not implicit
    s = AlsSession(M, N, k, implicit=implicit, dtype=dtype, lam=0.5, use_cg=True, k_main=km, user_bias=bias, item_bias=bias)
    users, held, excl = _lists()
    try:
        s.set_X_coo(row, col, val, subtract=gm)
        s.set_factors(A=(0.3 * rng.standard_normal((M, k + km))).astype(dtype), B=(0.3 * rng.standard_normal((N, k + km))).astype(dtype),
                      biasA=np.zeros(M, dtype) if bias else None, biasB=(0.2 * rng.standard_normal(N)).astype(dtype) if bias else None)
        with RankSet(users, held, excl, dtype=dtype) as rs:
            seen = []
            for it in range(2):
                s.iterate(1, False)
                rec = s.ranking(rs, k=10)
                f = s.get_factors()
                with Ranker(f["B"], f["biasB"]) as rk:
                    ip, _, ranks, pool = rk.ranks(f["A"][users], held, exclude=excl)
                    ref = rk.metrics(f["A"], rs, k=10)
                rr.check(rec, ip, ranks, pool, 10, what="session it=%d" % it)
                assert np.array_equal(rec["count"], ref["count"]) and rec["users"] == ref["users"] and int(rec["users"]) > 50
                assert _same_bytes(s.ranking(rs, k=10), rec)
                after = s.get_factors()
                assert all(f[key] is None or np.array_equal(f[key], after[key]) for key in f), "the evaluation changed the session"
                seen.append(rec["sum"].copy())
            assert not np.array_equal(seen[0], seen[1]), "the second iteration changed nothing: the refreshed B was not ranked"
    finally:
        s.close()
    wide = AlsSession(M, N, 273, implicit=True, dtype=dtype)
    try:
        with RankSet(users, held, excl, dtype=dtype) as rs, pytest.raises(RuntimeError, match="code 2"):
            wide.ranking(rs)
    finally:
        wide.close()
