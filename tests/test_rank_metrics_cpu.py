"""CPU: cmfrec_amd.metrics.ranking_metrics against a brute-force evaluation of every definition from a full lexsort of random
integer scores with ties."""
import numpy as np
import pytest

from cmfrec_amd.metrics import METRICS, mean_metrics, ranking_metrics


def brute(scores, held, excluded, k):
    """One user: the metrics from the ranked list itself.  scores [n] integers, held / excluded id arrays."""
    n = len(scores)
    valid = np.ones(n, bool); valid[excluded] = False
    ids = np.flatnonzero(valid)
    order = ids[np.lexsort((ids, -scores[ids]))]                     # the user's full ranking
    place = {int(i): p for p, i in enumerate(order)}
    r = sorted(place[int(t)] for t in held if int(t) in place)
    ranks_in = [place.get(int(t), -1) for t in held]
    P, T = len(order), len(r)
    if T == 0:
        return ranks_in, P, None
    rel = np.zeros(P, bool); rel[r] = True
    top = rel[:k]
    h = int(top.sum())
    prec_at = np.cumsum(rel) / (np.arange(P) + 1.)
    ap = float((prec_at[:k] * top).sum()) / min(k, T)
    dcg = float((top / np.log2(np.arange(len(top)) + 2.)).sum())
    idcg = float((1. / np.log2(np.arange(min(k, T)) + 2.)).sum())
    # AUC by pairs: the share of (held-out, other) pairs the ranking orders correctly
    neg = np.flatnonzero(~rel)
    auc = float(np.mean([(neg > p).mean() for p in r])) if len(neg) else float("nan")
    return ranks_in, P, dict(hit=float(h > 0), precision=h / k, recall=h / T, ap=ap, ndcg=dcg / idcg, rr=1. / (r[0] + 1),
                             auc=auc, mean_rank=float(np.mean(r)))


@pytest.mark.parametrize("k", [1, 3, 10, 1000])
def test_against_brute_force(k):
    rng = np.random.default_rng(k)
    nu, n = 40, 60
    indptr = [0]; ranks = []; pool = []; want = []
    for u in range(nu):
        scores = rng.integers(0, 8, n)                               # many ties
        T = [0, 1, 2, 5, 30, n][u % 6]
        held = np.sort(rng.choice(n, T, replace=False))
        excluded = rng.choice(n, [0, 10, n - 1][u % 3], replace=False)
        if u == 7:
            excluded = np.setdiff1d(np.arange(n), held)              # P == T: every ranked item is held out
        if u == 8:
            excluded = held.copy()                                    # every held-out item excluded: all ranks -1
        r, P, w = brute(scores, held, excluded, k)
        ranks += r; indptr.append(len(ranks)); pool.append(P); want.append(w)
    got = ranking_metrics(np.array(indptr), np.array(ranks, np.int32), np.array(pool, np.int32), k=k)
    assert (np.array(ranks) == -1).any()
    for u, w in enumerate(want):
        for name in METRICS:
            if w is None:
                assert np.isnan(got[name][u]), (u, name)
            elif np.isnan(w[name]):
                assert np.isnan(got[name][u]), (u, name)
            else:
                assert got[name][u] == pytest.approx(w[name], rel=1e-12, abs=1e-12), (u, name)
    assert np.isnan(got["auc"][7]) and got["T"][7] > 0 and not np.isnan(got["recall"][7])
    assert got["T"][8] == 0 and all(np.isnan(got[name][8]) for name in METRICS)
    assert np.array_equal(got["T"], [0 if w is None else t for w, t in zip(want, got["T"])])
    means = mean_metrics(got)
    assert means["users"] == sum(w is not None for w in want)
    for name in METRICS:
        vals = [w[name] for w in want if w is not None and not np.isnan(w[name])]
        assert means[name] == pytest.approx(np.mean(vals), rel=1e-12)


def test_known_values():
    # one user, held-out items at places 0, 2 and 9 of 20; k = 3
    got = ranking_metrics([0, 4], [2, -1, 0, 9], [20], k=3)
    assert got["T"][0] == 3 and got["hit"][0] == 1 and got["precision"][0] == pytest.approx(2 / 3)
    assert got["recall"][0] == pytest.approx(2 / 3) and got["rr"][0] == 1.0 and got["mean_rank"][0] == pytest.approx(11 / 3)
    assert got["ap"][0] == pytest.approx((1 / 1 + 2 / 3) / 3)
    assert got["ndcg"][0] == pytest.approx((1 + 1 / 2) / (1 + 1 / np.log2(3) + 1 / 2))
    assert got["auc"][0] == pytest.approx(1 - (0 + 1 + 7) / (3 * 17))
    # no users with held-out items; an empty call
    got = ranking_metrics([0, 0, 0], np.zeros(0, np.int32), [5, 5])
    assert all(np.isnan(got[name]).all() for name in METRICS) and mean_metrics(got)["users"] == 0
    assert np.isnan(mean_metrics(got)["auc"])


def test_refusals():
    with pytest.raises(ValueError, match="indptr"):
        ranking_metrics([0, 1], [0], [3, 3])
    with pytest.raises(ValueError, match="indptr"):
        ranking_metrics([0, 2], [0], [3])
    with pytest.raises(ValueError, match="k must"):
        ranking_metrics([0, 1], [0], [3], k=0)
