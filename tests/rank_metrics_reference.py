"""The ranking-metric record of held-out items (cmfrec_hip_rank_record: Ranker.metrics, AlsSession.ranking): the exact record and
the check (helpers, no tests).  tests/test_gpu_rank_metrics.py runs the check on the GPU's records, tests/test_rank_metrics_reduction_cpu.py
on a stand-in and on mutations of it.

The record is defined on integer ranks, so its reference is cmfrec_amd.metrics.ranking_metrics itself (float64): per metric -- hit,
precision, recall, ap, ndcg, rr, auc, mean_rank -- the sum of the per-user values over the users that count and their number, and
`users`, the users with a valid held-out item.  A per-user value is  v = N / D  (auc: 1 - N / D), N a sum of n <= T non-negative
terms.  Each TERM is the same float64 on both sides: j / (r + 1) is one correctly rounded division of two integers, r and
r - (j - 1) are integers, and the NDCG discount comes from a table the host computes the way NumPy does (the same bits where both
use the same log2; at most one unit in the last place apart otherwise, which the factor 2 below also covers: it is one more
relative rounding of a non-negative term).  Otherwise only the order of the additions differs.  The check, nothing in it measured, with u = 2^-53:

    counts      exact
    per user    |v_got - v_ref| <= 2 (T + 3) u mag,  mag = |v_ref| (auc: 1 + N / D): T - 1 additions in any order, the division, the
                subtraction of auc, on either side (the factor 2: the reference is rounded too)
    a sum S     over U counted users:  |S_got - S_ref| <= 2 (T_max + U + 3) u sum_users mag  -- the per-user bound of every term plus
                U - 1 additions in any order
    no users    the sum is exactly 0
"""
import numpy as np

from cmfrec_amd.metrics import METRICS, ranking_metrics
from dense_reference import Rejected

U53 = 2.0 ** -53


def per_user_reference(indptr, ranks, pool, k):
    """(per-user values [users, 8] in METRICS order with NaN where the user does not count, T [users], mag [users, 8])."""
    per = ranking_metrics(indptr, ranks, pool, k=k)
    vals = np.stack([per[name] for name in METRICS], axis=1)
    mag = np.abs(vals)
    auc = METRICS.index("auc")
    mag[:, auc] = 1.0 + np.abs(1.0 - vals[:, auc])           # 1 + N / D
    return vals, per["T"], mag


def exact_record(indptr, ranks, pool, k):
    vals, T, mag = per_user_reference(indptr, ranks, pool, k)
    good = ~np.isnan(vals)
    rec = {"sum": np.where(good, vals, 0.0).sum(axis=0), "count": good.sum(axis=0).astype(np.uint64), "users": np.uint64((T > 0).sum())}
    return rec, vals, T, np.where(good, mag, 0.0)


def violations(got, indptr, ranks, pool, k, per_user=None):
    """The names of what the record `got` (and the per-user values, if given) gets wrong, [] if nothing; the worst error / bound."""
    want, vals, T, mag = exact_record(indptr, ranks, pool, k)
    bad = []
    worst = 0.0
    if int(got["users"]) != int(want["users"]):
        bad.append("users")
    tmax = int(T.max()) if len(T) else 0
    for i, name in enumerate(METRICS):
        cnt = int(want["count"][i])
        if int(got["count"][i]) != cnt:
            bad.append("count[%s]" % name)
        g = np.float64(got["sum"][i])
        if cnt == 0:
            if not g == 0:
                bad.append("sum[%s]" % name)
            continue
        bound = 2 * (tmax + cnt + 3) * U53 * mag[:, i].sum()
        err = abs(g - want["sum"][i])
        if not err <= bound:                                  # (a NaN fails too)
            bad.append("sum[%s]" % name)
        if bound > 0:
            worst = max(worst, float(err / bound))
    if per_user is not None:
        pu = np.asarray(per_user, np.float64)
        if pu.shape != vals.shape or not np.array_equal(np.isnan(pu), np.isnan(vals)):
            bad.append("per_user (which users count)")
        else:
            good = ~np.isnan(vals)
            bound = 2 * (T[:, None] + 3) * U53 * mag
            err = np.where(good, np.abs(np.where(good, pu, 0.0) - np.where(good, vals, 0.0)), 0.0)
            if not (err <= bound).all():
                bad.append("per_user values")
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(bound > 0, err / bound, 0.0)
            worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
    return bad, worst


def check(got, indptr, ranks, pool, k, per_user=None, what="rank metrics"):
    """Asserts that the record (and the per-user values) are right; returns the worst error / bound."""
    bad, worst = violations(got, indptr, ranks, pool, k, per_user)
    if bad:
        raise Rejected("%s: wrong %s (worst error / bound = %.3g)" % (what, ", ".join(bad), worst))
    return worst


def standin(indptr, ranks, pool, k, order=None, mutate=None):
    """(record, per-user values) computed user by user in plain Python float64, the users added in `order` (a permutation, or as they
    come).  mutate: one of the mistakes the check must reject -- "drop_user", "count_invalid", "list_order_j", "k_for_cut",
    "auc_full_pool", "count_empty"."""
    indptr = np.asarray(indptr, np.int64); ranks = np.asarray(ranks, np.int64); pool = np.asarray(pool, np.int64)
    nu = len(pool)
    disc = 1.0 / np.log2(np.arange(1, k + 1) + 1.0)
    ideal = np.concatenate(([0.0], np.cumsum(disc)))
    vals = np.full((nu, 8), np.nan)
    for u in range(nu):
        lst = ranks[indptr[u]:indptr[u + 1]]
        valid = lst if mutate == "count_invalid" else lst[lst >= 0]
        T = len(valid)
        if T == 0:
            if mutate == "count_empty":
                vals[u] = 0.0
            continue
        srt = np.sort(valid, kind="stable")
        if mutate == "list_order_j":
            pairs = [(int(r), j + 1) for j, r in enumerate(valid)]
        else:
            pairs = [(int(r), j + 1) for j, r in enumerate(srt)]
        h = sum(1 for r, _ in pairs if r < k)
        cut = k if mutate == "k_for_cut" else min(k, T)
        s_ap = 0.0; s_nd = 0.0; s_auc = 0.0; s_rank = 0.0
        for r, j in reversed(pairs):                           # (another order of the additions than NumPy's)
            s_rank += float(r); s_auc += float(r - (j - 1))
            if 0 <= r < k:
                s_ap += j / (r + 1.0); s_nd += disc[r]
        rest = int(pool[u]) - T
        with np.errstate(divide="ignore"):
            first = float(np.float64(1.0) / np.float64(srt[0] + 1.0))
        vals[u] = [1.0 if h > 0 else 0.0, h / float(k), h / float(T), s_ap / cut, s_nd / ideal[min(cut, k)], first,
                   (1.0 - s_auc / (float(T) * rest)) if rest != 0 else (1.0 if mutate == "auc_full_pool" else np.nan), s_rank / T]
    idx = list(range(nu)) if order is None else list(order)
    if mutate == "drop_user":
        idx = [u for u in idx if np.isnan(vals[u]).all()] + [u for u in idx if not np.isnan(vals[u]).all()][1:]
    rec = {"sum": np.zeros(8), "count": np.zeros(8, np.uint64), "users": np.uint64(0)}
    for u in idx:
        if not np.isnan(vals[u]).all():
            rec["users"] += np.uint64(1)
        for f in range(8):
            if not np.isnan(vals[u, f]):
                rec["sum"][f] += vals[u, f]; rec["count"][f] += np.uint64(1)
    return rec, vals


def example(seed=0, n_items=300):
    """(indptr, ranks, pool) of 70 users with lists of 0, 1, 2, 63, 64, 65 and 200 entries, -1 among the ranks, one user without a
    valid rank, one whose pool is its held-out items alone (P = T)."""
    rng = np.random.default_rng(seed)
    lens = np.array([0, 1, 2, 63, 64, 65, 200] * 10)
    indptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    ranks = np.empty(indptr[-1], np.int64)
    pool = np.empty(len(lens), np.int64)
    for u, ln in enumerate(lens):
        pool[u] = n_items - int(rng.integers(0, 20))
        r = rng.choice(pool[u], size=ln, replace=False)
        r[rng.random(ln) < 0.1] = -1
        ranks[indptr[u]:indptr[u + 1]] = r
    ranks[indptr[8]:indptr[9]] = -1                             # a user of one entry, and that one invalid: T = 0
    u = 9                                                        # two entries, both valid, and nothing else in the pool: P = T
    ranks[indptr[u]:indptr[u + 1]] = [1, 0]; pool[u] = 2
    return indptr, ranks, pool
