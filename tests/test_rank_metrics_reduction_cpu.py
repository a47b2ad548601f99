"""The check of tests/rank_metrics_reference.py on a stand-in, no device: it accepts another order of the additions and of the
users, and rejects the mistakes a reduction kernel can make."""
import numpy as np
import pytest

import rank_metrics_reference as rr
from cmfrec_amd.metrics import METRICS, mean_from_record, mean_metrics, ranking_metrics
from dense_reference import Rejected


@pytest.mark.parametrize("k", [1, 10, 250])
def test_check_accepts_other_orders(k):
    indptr, ranks, pool = rr.example()
    rec, vals = rr.standin(indptr, ranks, pool, k)
    assert rr.check(rec, indptr, ranks, pool, k, per_user=vals) <= 1.0
    perm = np.random.default_rng(3).permutation(len(pool))
    rec2, _ = rr.standin(indptr, ranks, pool, k, order=perm)
    rr.check(rec2, indptr, ranks, pool, k)
    assert np.array_equal(rec2["count"], rec["count"]) and rec2["users"] == rec["users"]
    # the example has what it says: users that count nowhere, one that counts everywhere but in auc
    want, v, T, _ = rr.exact_record(indptr, ranks, pool, k)
    assert int(want["users"]) == int((T > 0).sum()) < len(pool)
    assert int(want["count"][METRICS.index("auc")]) == int(want["users"]) - 1
    assert (T[np.diff(indptr) == 200] > 64).all()


@pytest.mark.parametrize("k", [1, 10, 250])
@pytest.mark.parametrize("mutate", ["drop_user", "count_invalid", "list_order_j", "k_for_cut", "auc_full_pool", "count_empty"])
def test_check_rejects(mutate, k):
    if mutate == "k_for_cut" and k == 1:
        k = 3                                                   # (min(1, T) = 1 for every counted user: nothing to get wrong)
    indptr, ranks, pool = rr.example()
    rec, vals = rr.standin(indptr, ranks, pool, k, mutate=mutate)
    with pytest.raises(Rejected):
        rr.check(rec, indptr, ranks, pool, k)
    if mutate != "drop_user":                                   # (a dropped user leaves the per-user values as they are)
        with pytest.raises(Rejected):
            good, _ = rr.standin(indptr, ranks, pool, k)
            rr.check(good, indptr, ranks, pool, k, per_user=vals)


def test_a_rounding_beyond_the_bound_is_rejected():
    indptr, ranks, pool = rr.example()
    rec, vals = rr.standin(indptr, ranks, pool, 10)
    i = METRICS.index("ndcg")
    rec["sum"][i] *= 1 + 1e-11
    with pytest.raises(Rejected):
        rr.check(rec, indptr, ranks, pool, 10)
    rec, vals = rr.standin(indptr, ranks, pool, 10)
    vals[6, METRICS.index("ap")] *= 1 + 1e-12
    with pytest.raises(Rejected):
        rr.check(rec, indptr, ranks, pool, 10, per_user=vals)


def test_no_users():
    rec, vals = rr.standin([0, 0, 2], [-1, -1], [5, 5], 10)
    assert int(rec["users"]) == 0 and not rec["sum"].any()
    rr.check(rec, [0, 0, 2], [-1, -1], [5, 5], 10, per_user=vals)
    rec["sum"][0] = 1e-300
    with pytest.raises(Rejected):
        rr.check(rec, [0, 0, 2], [-1, -1], [5, 5], 10)


@pytest.mark.parametrize("k", [1, 10, 250])
def test_mean_from_record(k):
    indptr, ranks, pool = rr.example()
    want = mean_metrics(ranking_metrics(indptr, ranks, pool, k=k))
    rec, _, _, _ = rr.exact_record(indptr, ranks, pool, k)
    got = mean_from_record(rec)
    assert got.keys() == want.keys() and got["users"] == want["users"]
    for name in METRICS:
        assert abs(got[name] - want[name]) <= 1e-13 * abs(want[name]), name
    # hand-made: a metric nobody counts in is NaN, the others sum / count
    rec = {"sum": np.array([1.0, 0.5, 2.0, 0, 0, 0, 0.0, 9.0]), "count": np.array([2, 2, 4, 0, 0, 0, 0, 3], np.uint64), "users": np.uint64(4)}
    got = mean_from_record(rec)
    assert got["hit"] == 0.5 and got["precision"] == 0.25 and got["recall"] == 0.5 and got["mean_rank"] == 3.0 and got["users"] == 4
    assert all(np.isnan(got[name]) for name in ("ap", "ndcg", "rr", "auc"))
