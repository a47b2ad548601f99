"""Reference and derived tolerances for the stochastic top-N tests (test_gpu_topn_sample.py): NumPy in float64.

Definition: h = splitmix64(seed ^ (u * GOLDEN + i)) on uint64; U = ((h >> S) + 1/2) 2^-b with (S, b) = (11, 53)
in double and (40, 24) in single precision -- an exact rational, evaluated here through 1 - U where U > 1/2, as the kernel does;
g = -log(-log U); key = score + T g.

Key bound.  The kernel's g carries two library logarithms of at most 2 ulp each (4 u relative, u the unit roundoff): the inner
one moves log(-log U) by at most 4 u absolutely, the outer one by 4 u |g|, so |g^ - g| <= 4 u (1 + |g|): two units in the last
place of 1 + |g|.  The fused multiply-add rounds once, u |key|.  With the score's own bound E_u of topn_reference:
    EK_u = E_u + T * 4 u * (1 + max|g|) + 2 u * max|key|.

Log-partition bound.  A term exp((s_i - M) / T) of the final sum reaches it as a product of J_i single-precision exponentials
(its own, one per later change of its lane's reference, four butterfly steps, seven wavefront merges) whose arguments are all
<= 0 and add up to -d_i = (s_i - M) / T.  One factor exp(x): the difference rounded to single (v), times the rounded 1 / T (2 v),
times log2 e inside the fast exponential (2 v), v = 2^-24 -- 5 v |x| in the exponent -- and v_exp_f32's 1 ulp, 2 v.  So term i
is off by at most (5 d_i + 2 J) v relatively, J = ceil(items / 128) + 12, and the sum by the softmax-weighted mean of that:
    EL_u = v * (5 * sum_i p_i d_i + 2 J) + E_u / T + 1e-12 * (1 + |lse|)
(E_u / T: the scores themselves; the last term: the double-precision sums, the division and the final logarithm)."""
import numpy as np

import topn_reference as tr

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
BOUND_C = 2.0 ** -10


def splitmix64(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def hashes(seed, nu, n):
    with np.errstate(over="ignore"):
        c = np.arange(nu, dtype=np.uint64)[:, None] * GOLDEN + np.arange(n, dtype=np.uint64)[None, :]
    return splitmix64(np.uint64(seed) ^ c)


def gumbel(h, dtype):
    shift, b = (11, 53) if np.dtype(dtype) == np.float64 else (40, 24)
    m = h >> np.uint64(shift)
    top = (h >> np.uint64(63)) == 1
    w = ((~h >> np.uint64(shift)).astype(np.float64) + 0.5) * 2.0 ** -b          # 1 - U, exact where U > 1/2
    U = (m.astype(np.float64) + 0.5) * 2.0 ** -b                                 # exact where U < 1/2
    L = np.where(top, -np.log1p(-np.where(top, w, 0.25)), -np.log(np.where(top, 0.25, U)))
    return -np.log(L)


def gumbel_bound(h):
    """(clz(~h) + 1) ln 2 + c: what the kernel compares before it evaluates a logarithm."""
    nh = ~h
    z = np.zeros(h.shape, np.int64)
    run = np.ones(h.shape, bool)
    for bit in range(63, -1, -1):
        run &= ((nh >> np.uint64(bit)) & np.uint64(1)) == 0
        z += run
    return (z + 1) * np.log(2.0) + BOUND_C


def make_case(seed, dtype, k, nu=37, n=1000):
    """topn_reference's problem with one user (5) who excludes all but five items; the lists ascending."""
    A, B, b, ep, ei = tr.make_problem(seed, dtype, nu, n, k)
    lists = [np.sort(ei[int(ep[u]):int(ep[u + 1])]) for u in range(nu)]
    lists[5] = np.setdiff1d(np.arange(n, dtype=np.int32), np.array([3, 7, 500, 998, 999], np.int32))
    ep = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
    return A, B, b, ep, np.concatenate(lists).astype(np.int32)


def keys_and_bounds(A, B, bias, S, T, seed, dtype):
    """(K [nu, n] float64, EK [nu])."""
    u = tr.unit_roundoff(dtype)
    g = gumbel(hashes(seed, *S.shape), dtype)
    K = S + T * g
    return K, tr.bounds(A, B, bias, dtype) + T * 4 * u * (1 + np.abs(g).max(axis=1)) + 2 * u * np.abs(K).max(axis=1)


def excluded(ep, ei, u):
    return ei[int(ep[u]):int(ep[u + 1])] if ep is not None else np.zeros(0, np.int32)


def check_keys(K, EK, ep, ei, n_top, ids=None, keys=None):
    """topn_reference.check_ranking's four conditions on the keys K [nu, n] (float64) with the bounds EK.  Returns (worst key
    error / EK_u, undecided share); ids = None: the share alone, of the reference's own order."""
    nu, n = K.shape
    worst, undecided, total = 0.0, 0, 0
    for u in range(nu):
        s = K[u].copy()
        s[excluded(ep, ei, u)] = -np.inf
        order = np.lexsort((np.arange(n), -s))
        left = int(np.isfinite(s).sum())
        nret = min(n_top, left)
        want = order[:nret]
        so = s[order[:min(nret + 1, left)]]
        d = np.abs(np.diff(so))
        ok = (d > 2 * EK[u]) | (d == 0)
        pad = np.ones(nret + 1 - len(so), bool)
        decided = np.concatenate([[True], ok]).astype(bool)[:nret] & np.concatenate([ok, pad])[:nret]
        undecided += int((~decided).sum()); total += nret
        if ids is None:
            continue
        got = ids[u, :nret]
        assert np.array_equal(ids[u, nret:], np.full(n_top - nret, -1)) and np.all(np.isneginf(keys[u, nret:])), (u, ids[u, nret:])
        assert got.min(initial=0) >= 0 and got.max(initial=0) < n and len(set(got.tolist())) == nret, u          # 1.
        assert not set(got.tolist()) & set(excluded(ep, ei, u).tolist()), u
        err = np.abs(keys[u, :nret].astype(np.float64) - K[u, got])                                              # 2.
        assert np.all(err <= EK[u]), (u, float(err.max()), float(EK[u]))
        worst = max(worst, float(err.max(initial=0.0)) / EK[u])
        assert np.all(np.abs(K[u, got] - K[u, want]) <= 2 * EK[u]), u                                            # 3.
        assert np.array_equal(got[decided], want[decided]), (u, np.nonzero(got != want)[0][:5])                  # 4.
    return worst, undecided / max(total, 1)


def lse64(S, ep, ei, T):
    """(lse [nu], sum_i p_i d_i [nu]) over the items that are not excluded; -inf and 0 where none is left."""
    nu = S.shape[0]
    lse, pd = np.full(nu, -np.inf), np.zeros(nu)
    for u in range(nu):
        x = np.delete(S[u], excluded(ep, ei, u)) / T
        if x.size:
            e = np.exp(x - x.max())
            lse[u] = x.max() + np.log(e.sum())
            pd[u] = float((e * (x.max() - x)).sum() / e.sum())
    return lse, pd


def lse_bounds(A, B, bias, S, ep, ei, T, dtype):
    lse, pd = lse64(S, ep, ei, T)
    J = -(-S.shape[1] // 128) + 12
    fin = np.where(np.isfinite(lse), np.abs(lse), 0.0)
    return lse, 2.0 ** -24 * (5 * pd + 2 * J) + tr.bounds(A, B, bias, dtype) / T + 1e-12 * (1 + fin)
