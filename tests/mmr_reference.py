"""Maximal marginal relevance over one user's pool in plain float64 NumPy: the definition of include/cmfrec_hip.h
(cmfrec_hip_ranker_rerank_mmr), the greedy selection by it, and the replay that holds a device result to it."""
import numpy as np


def margin(k, dtype):
    """2 (k + 8) u, u the unit roundoff of ``dtype``: a length-k dot product of two unit vectors is off by about k u, the two
    scalings and the normalisation of the scores add a few u, and two such values are compared."""
    return 2.0 * (k + 8) * np.finfo(dtype).eps / 2


def pool_terms(B, ids, scores):
    """(valid [M] bool, rel [M], sim [M, M]) of one pool against the item factors B [n, k], in float64."""
    ids = np.asarray(ids); s = np.asarray(scores, np.float64)
    valid = (ids >= 0) & (ids < len(B)) & np.isfinite(s)
    rows = B[np.where(valid, ids, 0)].astype(np.float64)
    rows[~valid] = 0
    nrm = np.sqrt((rows * rows).sum(axis=1))
    inv = np.where(nrm > 0, 1.0 / np.where(nrm > 0, nrm, 1.0), 0.0)
    sim = (rows @ rows.T) * inv[:, None] * inv[None, :]
    rel = np.zeros(len(ids))
    if valid.any() and s[valid].max() > s[valid].min():
        rel[valid] = (s[valid] - s[valid].min()) / (s[valid].max() - s[valid].min())
    return valid, rel, sim


def values(rel, msim, theta, t):
    """(v, key) of pick t (0-based): the first pick is by rel alone and reports theta * rel."""
    v = theta * rel if t == 0 else theta * rel - (1.0 - theta) * msim
    return v, (rel if t == 0 else v)


def greedy(B, ids, scores, theta, n_top):
    """(picked positions, their v, the smallest gap between a pick's key and the runner-up's).  A first pick over scores that
    are all equal is a tie by definition (rel is 0 for every pair, the earliest position takes it) and has no gap."""
    valid, rel, sim = pool_terms(B, ids, scores)
    avail = valid.copy(); msim = np.full(len(rel), -np.inf)
    picks, vals, gap = [], [], np.inf
    for t in range(n_top):
        if not avail.any():
            break
        v, key = values(rel, msim, theta, t)
        key = np.where(avail, key, -np.inf)
        p = int(np.argmax(key))                                  # (the first of equal values)
        if avail.sum() > 1 and not (t == 0 and not rel.any()):
            gap = min(gap, key[p] - np.delete(key, p).max())
        picks.append(p); vals.append(v[p])
        avail[p] = False
        msim = np.maximum(msim, sim[p])
    return picks, vals, gap


def replay(B, ids, scores, theta, got_ids, got_scores, got_mmr, tol):
    """Walks a device result in float64: pick t is valid and unpicked, its value given the device's own prefix is within ``tol``
    of the best, its score is the pool's, its reported value within ``tol`` of the float64 one; -1 / -inf once the valid pairs
    have run out.  The ids of a pool are distinct (but for the -1 of its padding)."""
    valid, rel, sim = pool_terms(B, ids, scores)
    where = {int(i): p for p, i in enumerate(ids) if valid[p]}
    avail = valid.copy(); msim = np.full(len(rel), -np.inf)
    for t in range(len(got_ids)):
        if not avail.any():
            assert np.all(got_ids[t:] == -1) and np.all(got_scores[t:] == -np.inf) and np.all(got_mmr[t:] == -np.inf), t
            return
        p = where.get(int(got_ids[t]))
        assert p is not None and avail[p], (t, got_ids[t])
        v, key = values(rel, msim, theta, t)
        assert key[p] >= key[avail].max() - tol, (t, key[p], key[avail].max())
        assert got_scores[t] == scores[p], (t, got_scores[t], scores[p])
        assert abs(float(got_mmr[t]) - v[p]) <= tol, (t, got_mmr[t], v[p])
        avail[p] = False
        msim = np.maximum(msim, sim[p])
