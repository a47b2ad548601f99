"""Ranking metrics from the ranks of held-out items (``Ranker.ranks``, ``ops.ranks_batch``) and error metrics from the error
record of held-out values (``Scorer.errors``, ``AlsSession.errors``): pure NumPy, no device."""
import numpy as np

METRICS = ("hit", "precision", "recall", "ap", "ndcg", "rr", "auc", "mean_rank")


def ranking_metrics(indptr, ranks, pool, k=10):
    """Per-user metrics, a dict of float64 arrays [users].  ``indptr`` [users + 1] delimits each user's entries of ``ranks``
    (0-based places in the user's full ranking; -1 entries are dropped), ``pool`` [users] is the number of ranked items.
    With r_1 < ... < r_T a user's valid ranks, P its pool and h = #{r_j < k}:

        hit@k        h > 0
        precision@k  h / k
        recall@k     h / T
        ap@k         (1 / min(k, T)) * sum_{r_j < k} j / (r_j + 1)
        ndcg@k       sum_{r_j < k} 1 / log2(r_j + 2)  /  sum_{j = 1..min(k, T)} 1 / log2(j + 1)
        rr           1 / (r_1 + 1)
        auc          1 - sum_j (r_j - (j - 1)) / (T * (P - T)); NaN when P == T
        mean_rank    mean(r_j)

    keyed "hit", "precision", "recall", "ap", "ndcg", "rr", "auc", "mean_rank", plus "T" (int64, the valid held-out items).
    A user with T == 0 is NaN everywhere (``np.nanmean`` leaves it out of a mean).  No loop over the users."""
    indptr = np.asarray(indptr).astype(np.int64)
    ranks = np.asarray(ranks).astype(np.int64)
    pool = np.asarray(pool).astype(np.int64)
    k = int(k)
    nu = len(indptr) - 1
    if nu < 0 or len(pool) != nu:
        raise ValueError("ranking_metrics: indptr must have one entry per user plus one (%d), got %d" % (len(pool) + 1, len(indptr)))
    if k < 1:
        raise ValueError("ranking_metrics: k must be at least 1")
    if nu and (indptr[0] != 0 or indptr[-1] != len(ranks) or (np.diff(indptr) < 0).any()):
        raise ValueError("ranking_metrics: indptr does not delimit the %d ranks" % len(ranks))
    owner = np.repeat(np.arange(nu, dtype=np.int64), np.diff(indptr))
    ok = ranks >= 0
    owner, r = owner[ok], ranks[ok]
    order = np.lexsort((r, owner))
    owner, r = owner[order], r[order]
    T = np.bincount(owner, minlength=nu).astype(np.int64)
    start = np.zeros(nu + 1, np.int64)
    start[1:] = np.cumsum(T)
    j = np.arange(len(r), dtype=np.int64) - start[owner] + 1             # 1-based place among the user's own held-out items
    top = r < k

    def per_user(w):
        return np.bincount(owner, weights=w, minlength=nu)

    with np.errstate(divide="ignore", invalid="ignore"):
        h = per_user(top.astype(np.float64))
        Tf = T.astype(np.float64)
        cut = np.minimum(k, T)
        ideal = np.concatenate(([0.], np.cumsum(1. / np.log2(np.arange(1, k + 1) + 1.))))[cut]
        first = np.full(nu, np.nan)
        first[owner[j == 1]] = r[j == 1]
        out = {
            "hit": (h > 0).astype(np.float64),
            "precision": h / k,
            "recall": h / Tf,
            "ap": per_user(np.where(top, j / (r + 1.), 0.)) / cut,
            "ndcg": per_user(np.where(top, 1. / np.log2(r + 2.), 0.)) / ideal,
            "rr": 1. / (first + 1.),
            "auc": 1. - per_user((r - (j - 1)).astype(np.float64)) / (Tf * (pool - T)),
            "mean_rank": per_user(r.astype(np.float64)) / Tf,
        }
    none = T == 0
    for name in METRICS:
        out[name][none] = np.nan
    out["auc"][(pool == T) & ~none] = np.nan
    out["T"] = T
    return out


def error_metrics(rec, include_fallback=True):
    """RMSE, MAE and their kin from an error record (``Scorer.errors``, ``AlsSession.errors``, ``ops.pair_errors``): per class
    -- [0] scored pairs, [1] fallback pairs (outside the model, predicted by the global mean and the bias in range) -- the
    record holds ``n``, ``sum_w``, ``sum_we``, ``sum_wabs``, ``sum_wsq``, ``max_abs``.  With S the sums over class 0, or over both
    classes when ``include_fallback``:

        mse   S(w e^2) / S(w)        rmse  sqrt(mse)        mae  S(w |e|) / S(w)        bias  S(w e) / S(w)
        max_abs  max |e|             sum_w  S(w)            n    the pairs that count

    plus ``n_fallback`` (the fallback pairs of the set, counted or not) and ``n_skipped``.  Where ``sum_w`` is 0 the four
    ratios are NaN.  Pure NumPy."""
    cls = slice(0, 2) if include_fallback else slice(0, 1)
    get = lambda name: np.asarray(rec[name], np.float64)[cls]
    sw = float(get("sum_w").sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = lambda name: float(np.float64(get(name).sum()) / np.float64(sw)) if sw != 0 else float("nan")
        mse = ratio("sum_wsq")
        out = {"rmse": float(np.sqrt(mse)), "mse": mse, "mae": ratio("sum_wabs"), "bias": ratio("sum_we")}
    n = np.asarray(rec["n"]).astype(np.int64)
    out["max_abs"] = float(get("max_abs").max())
    out["n"] = int(n[cls].sum())
    out["n_fallback"] = int(n[1])
    out["n_skipped"] = int(rec["n_skipped"])
    out["sum_w"] = sw
    return out


def mean_from_record(rec):
    """What ``mean_metrics(ranking_metrics(...))`` returns, from the record of a reduction on the device (``Ranker.metrics``,
    ``AlsSession.ranking``): per metric ``sum / count`` over the users that count (NaN where none does), and ``users``."""
    res = {}
    for i, name in enumerate(METRICS):
        cnt = int(rec["count"][i])
        res[name] = float(np.float64(rec["sum"][i]) / np.float64(cnt)) if cnt else float("nan")
    res["users"] = int(rec["users"])
    return res


def mean_metrics(per_user):
    """The means over the users with held-out items (NaN entries left out) and ``users``, their number."""
    res = {}
    for name in METRICS:
        v = per_user[name]
        good = ~np.isnan(v)
        res[name] = float(v[good].mean()) if good.any() else float("nan")
    res["users"] = int((per_user["T"] > 0).sum())
    return res
