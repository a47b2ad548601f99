"""Float64 reference and shared inputs of the rank tests (test_gpu_ranks.py, test_ranks_reference_cpu.py).

rank64(u, t) = #{ valid i : S_i > S_t or (S_i == S_t and i < t) } with S = topn_reference.scores64 on the dtype-rounded inputs
and "valid" = not in the user's exclusion list, S_i not NaN.  A device rank may differ from it only through pairs the working
precision cannot tell apart: near(u, t) = #{ valid i != t : 0 < |S_i - S_t| <= 2 E_u }, E_u = topn_reference.bounds (both scores
are within E_u of their float64 values, so a pair further apart than 2 E_u is ordered as in float64, and an exact float64 tie of
two items with equal rows -- the planted 3 / 7 / 11 -- is an exact tie on the device, broken by id on both sides).  The test
requires |rank - rank64| <= near.  The share of (user, held-out) pairs with near > 0 is a property of these inputs alone; it is
capped (CAP) so that the allowance cannot hide a failure: 0 in double precision, at most 0.25 in single precision."""
import numpy as np

import topn_reference as tr

SEED, NU, HELD = 5, 70, 12
CAP = {np.float64: 0.0, np.float32: 0.25}
ROUND_N = (129, 257, 1000)
ROUND_K = {np.float64: (3, 50, 64, 65, 128, 256), np.float32: (3, 50, 64, 65, 128, 256, 272)}
ROUND_CASES = [(dt, k, n) for dt in (np.float64, np.float32) for k in ROUND_K[dt] for n in ROUND_N]


def csr_of_lists(lists):
    p = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    i = np.concatenate([np.asarray(x, np.int64) for x in lists] + [np.zeros(0, np.int64)]).astype(np.int32)
    return p, i


def lists_of_csr(p, i):
    return [i[int(p[u]):int(p[u + 1])] for u in range(len(p) - 1)]


def heldout_lists(seed, nu, n, length):
    """Sorted lists of `length` (an int or one per user) random items; every user's list holds the planted ties 3, 7 and 11 where
    they exist and the list is long enough."""
    rng = np.random.default_rng(seed)
    lens = np.full(nu, length) if np.ndim(length) == 0 else np.asarray(length)
    out = []
    for u in range(nu):
        x = rng.choice(n, min(int(lens[u]), n), replace=False)
        ties = [t for t in (3, 7, 11) if t < n]
        if len(x) >= len(ties) > 0:
            x = np.concatenate([ties, np.setdiff1d(x, ties)[:len(x) - len(ties)]])
        out.append(np.sort(x))
    return csr_of_lists(out)


def small_problem(seed, dtype, nu, n, k, bias, excl):
    """make_problem's generator for any n >= 1 (it plants its ties in rows 3, 7, 11: generated with at least 16 items, cut to n);
    exclusion lists of 0 .. min(n, 20) items, user 0's empty."""
    A, B, b, _, _ = tr.make_problem(seed, dtype, nu, max(n, 16), k, bias=bias, excl=False)
    B = np.ascontiguousarray(B[:n]); b = None if b is None else np.ascontiguousarray(b[:n])
    ex = None
    if excl:
        rng = np.random.default_rng(seed + 77)
        lens = rng.integers(0, min(n, 20) + 1, nu); lens[0] = 0
        ex = csr_of_lists([np.sort(rng.choice(n, l, replace=False)) for l in lens])
    return A, B, b, ex


_round = {}


def round_problem(dtype, k, n):
    """The inputs of the several-rounds test, built once and never modified: (A, B, b, (ep, ei), (hp, hi))."""
    key = (np.dtype(dtype).name, k, n)
    if key not in _round:
        A, B, b, ep, ei = tr.make_problem(SEED, dtype, NU, n, k)
        ei = np.concatenate([np.sort(x) for x in lists_of_csr(ep, ei)] + [np.zeros(0, np.int32)]).astype(np.int32)
        _round[key] = (A, B, b, (ep, ei), heldout_lists(SEED + 1, NU, n, HELD))
    return _round[key]


def ranks64(A, B, b, held, excl, dtype):
    """(rank64, near, pool) per held-out entry / user; rank64 = -1 where the target is excluded, out of range or NaN."""
    hp, hi = held
    nu, n = A.shape[0], B.shape[0]
    S = tr.scores64(A, B, b)
    E = tr.bounds(np.nan_to_num(A), np.nan_to_num(B), b, dtype)    # (a NaN row of a corner-case test does not enter the bound)
    r64 = np.full(len(hi), -1, np.int64); near = np.zeros(len(hi), np.int64); pool = np.zeros(nu, np.int64)
    ids = np.arange(n)
    for u in range(nu):
        valid = ~np.isnan(S[u])
        if excl is not None:
            ex = excl[1][int(excl[0][u]):int(excl[0][u + 1])]
            valid[ex[(ex >= 0) & (ex < n)]] = False
        pool[u] = valid.sum()
        for j in range(int(hp[u]), int(hp[u + 1])):
            t = int(hi[j])
            if t < 0 or t >= n or not valid[t]:
                continue
            s = S[u, t]
            r64[j] = int((valid & ((S[u] > s) | ((S[u] == s) & (ids < t)))).sum())
            d = np.abs(S[u] - s)
            near[j] = int((valid & (ids != t) & (d > 0) & (d <= 2 * E[u])).sum())
    return r64, near, pool


def near_share(r64, near):
    ok = r64 >= 0
    return float((near[ok] > 0).sum()) / max(int(ok.sum()), 1)
