"""Reference neighbours and derived tolerances for the similarity tests (test_similar_cpu.py, test_gpu_similar.py).

The reference is NumPy in float64 on the dtype-rounded rows: S = (B_q . B_i) / (|B_q| |B_i|) under "cosine", the plain product
under "dot"; -inf for the query itself, for excluded rows and for scores that are not finite; the order is
lexsort((arange(n), -S[q])).

The tolerance of one cosine score, whatever the summation order: the dot product carries gamma_k |b_q| . |b_i| <=
gamma_k |b_q| |b_i| (Cauchy-Schwarz); each inverse norm a relative gamma_{k/2+2} (a sum of k non-negative terms, a square root
that halves the relative error, one division); the two multiplications one rounding each: E = gamma_{2k+8}, the same for every
query because |cos| <= 1.  Under "dot" it is topn_reference.bounds without a bias."""
import numpy as np

import topn_reference as tr

# (n, k, n_top) of the cosine cases; QUERIES of them ask
SHAPES = [(1000, 3, 10), (1000, 17, 33), (1000, 50, 10), (1000, 50, 128), (1000, 64, 33), (1000, 65, 128), (1000, 128, 10),
          (300, 129, 33), (300, 257, 10), (300, 272, 10), (129, 8, 128)]
NQ = 70
F32_CAP = 0.10            # undecided share a float32 GPU case may have
F32_REFERENCE_CAP = 0.05  # ... and what the inputs alone may leave undecided (test_similar_cpu.py), so that the cap hides nothing


def make_items(seed, dtype, n, k, nan_row=None):
    """Standard normal rows with the planted ones: 7 and 11 copies of 3 (exact ties, lower id first), 20 = 4 x row 3 (the same
    cosine bits, a dot product four times as large), 5 all zero (no cosine: never returned, no neighbours); ``nan_row``: a row
    that holds one NaN.  Rows a small ``n`` does not have are left out."""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, k)).astype(dtype)
    if n > 11:
        B[7] = B[3]; B[11] = B[3]
    if n > 20:
        B[20] = dtype(4) * B[3]
    if n > 5:
        B[5] = 0
    if nan_row is not None:
        B[nan_row, k // 2] = np.nan
    return B


def make_queries(seed, n, nq=NQ):
    """``nq`` distinct row ids that include the planted rows 3, 5, 7, 11 and 20."""
    planted = np.array([3, 5, 7, 11, 20])
    rest = np.setdiff1d(np.arange(n), planted)
    rng = np.random.default_rng(seed)
    return np.concatenate([planted, rng.choice(rest, nq - len(planted), replace=False)]).astype(np.int32)


def scores64(B, q, metric):
    B64 = B.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        S = B64[q] @ B64.T
        if metric == "cosine":
            nrm = np.sqrt((B64 * B64).sum(axis=1))
            S = S / (nrm[q][:, None] * nrm[None, :])
    return S


def bounds(B, q, metric, dtype):
    """E for every query."""
    if metric == "cosine":
        return np.full(len(q), tr.gamma(2 * B.shape[1] + 8, dtype))
    Bf = np.where(np.isfinite(B), B, 0)
    return tr.bounds(Bf[q], Bf, None, dtype)


def masked_scores(B, q, metric, ep=None, ei=None):
    """The float64 scores with -inf for the query itself, its excluded rows and scores that are not finite."""
    S = scores64(B, q, metric)
    S[~np.isfinite(S)] = -np.inf
    S[np.arange(len(q)), q] = -np.inf
    if ep is not None:
        for j in range(len(q)):
            S[j, ei[int(ep[j]):int(ep[j + 1])]] = -np.inf
    return S


def reference(B, q, metric, n_top, ep=None, ei=None):
    """(ids, scores) of the float64 ranking, -1 / -inf where fewer than ``n_top`` remain."""
    S = masked_scores(B, q, metric, ep, ei)
    n = B.shape[0]
    ids = np.full((len(q), n_top), -1, np.int32); sc = np.full((len(q), n_top), -np.inf)
    for j in range(len(q)):
        order = np.lexsort((np.arange(n), -S[j]))[:n_top]
        order = order[np.isfinite(S[j, order])]
        ids[j, :len(order)] = order; sc[j, :len(order)] = S[j, order]
    return ids, sc


def check_neighbours(B, q, metric, ep, ei, ids, sc, n_top, dtype, all_decided=False, verbose=True):
    """The four conditions of topn_reference.check_ranking for every query and position.  Returns (worst score error / E,
    undecided share); all_decided: the inputs must leave no position undecided (then every id must equal the reference's)."""
    n, nq = B.shape[0], len(q)
    S = masked_scores(B, q, metric, ep, ei)
    E = bounds(B, q, metric, dtype)
    assert ids.shape == (nq, n_top) and sc.shape == (nq, n_top)
    worst, undecided, total = 0.0, 0, 0
    for j in range(nq):
        s = S[j]
        order = np.lexsort((np.arange(n), -s))
        left = int(np.isfinite(s).sum())
        nret = min(n_top, left)
        got = ids[j]
        assert np.array_equal(got[nret:], np.full(n_top - nret, -1)), (j, got[nret:])
        assert np.all(np.isneginf(sc[j, nret:])), (j, sc[j, nret:])
        g = got[:nret]
        # 1. distinct, in range, not excluded, not the query itself (the last two: a finite masked score)
        assert g.min(initial=0) >= 0 and g.max(initial=0) < n, j
        assert len(set(g.tolist())) == nret, j
        assert q[j] not in g.tolist(), j
        assert np.all(np.isfinite(s[g])), (j, g[~np.isfinite(s[g])])
        want = order[:nret]
        # 2. scores within E of the float64 scores of the returned ids
        err = np.abs(sc[j, :nret].astype(np.float64) - s[g])
        assert np.all(err <= E[j]), (j, float(err.max()), float(E[j]))
        if E[j] > 0:                                      # (a zero row under "dot": every score is exactly 0)
            worst = max(worst, float(err.max(initial=0.0)) / E[j])
        # 3. the returned row at position p scores within 2 E of the reference's row at p
        gap = np.abs(s[g] - s[want])
        assert np.all(gap <= 2 * E[j]), (j, float(gap.max()), float(E[j]))
        # 4. decided positions: both neighbours in the float64 order more than 2 E away, or exactly tied
        so = s[order[:min(nret + 1, left)]]
        d = np.abs(np.diff(so))
        ok = (d > 2 * E[j]) | (d == 0)
        before = np.concatenate([[True], ok])[:nret]
        after = np.concatenate([ok, [True]])[:nret] if len(ok) >= nret else np.concatenate([ok, [True] * (nret - len(ok))])
        decided = before & after
        undecided += int((~decided).sum()); total += nret
        assert np.array_equal(g[decided], want[decided]), (j, np.nonzero(g != want)[0][:5])
    share = undecided / max(total, 1)
    if verbose:
        print("neighbour check: %s dtype=%s nq=%d n=%d k=%d n_top=%d worst score error %.3f E, undecided share %.2e"
              % (metric, np.dtype(dtype).name, nq, n, B.shape[1], n_top, worst, share))
    if all_decided:
        assert undecided == 0, "the test's own inputs leave %d positions undecided" % undecided
    return worst, share


def emulate(B, q, metric, bias=None, drop_norm=False):
    """The stated operation order in the working dtype: acc = B_q . B_i, then (acc * rn[i]) * rn[q] under "cosine" with
    rn = 1 / sqrt(sum of squares).  ``drop_norm`` / ``bias``: the two mutations (rn[q] left out; a bias added)."""
    dt = B.dtype.type
    with np.errstate(invalid="ignore", divide="ignore"):
        acc = (B[q] @ B.T).astype(dt)
        if metric == "cosine":
            rn = (dt(1) / np.sqrt((B * B).sum(axis=1, dtype=dt))).astype(dt)
            rn[~np.isfinite(rn)] = np.nan
            acc = (acc * rn[None, :]).astype(dt)
            if not drop_norm:
                acc = (acc * rn[q][:, None]).astype(dt)
        if bias is not None:
            acc = (acc + bias[None, :]).astype(dt)
    return acc


def ranked(S_dtype, q, n_top):
    """(ids, scores) of a score matrix in the working dtype, ranked by the kernels' rule: self and NaN out, descending, ties by
    lower id."""
    S = S_dtype.astype(np.float64)
    S[np.isnan(S)] = -np.inf
    S[np.arange(len(q)), q] = -np.inf
    n = S.shape[1]
    ids = np.full((len(q), n_top), -1, np.int32); sc = np.full((len(q), n_top), -np.inf, S_dtype.dtype)
    for j in range(len(q)):
        order = np.lexsort((np.arange(n), -S[j]))[:n_top]
        order = order[np.isfinite(S[j, order])]
        ids[j, :len(order)] = order; sc[j, :len(order)] = S_dtype[j, order]
    return ids, sc
