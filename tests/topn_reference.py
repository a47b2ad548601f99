"""Reference ranking and derived tolerances for the top-N tests (test_gpu_topn_wide.py, test_gpu_ranker.py).

The reference is NumPy in float64 on the dtype-rounded inputs: S = A @ B.T + bias, excluded entries -inf,
want = lexsort((arange(n), -S[u]))[:n_top].  The tolerance is the classical bound of a dot product of k terms plus one
addition, whatever the summation order: E_u = gamma_{k+1} * max_i(|A_u| . |B_i| + |bias_i|), gamma_m = m u / (1 - m u),
u the unit roundoff of the dtype."""
import numpy as np


def unit_roundoff(dtype):
    return 2.0 ** -53 if np.dtype(dtype) == np.float64 else 2.0 ** -24


def gamma(m, dtype):
    u = unit_roundoff(dtype)
    return m * u / (1.0 - m * u)


def make_problem(seed, dtype, nu, n, k, bias=True, excl=True, max_excl=60):
    """Standard normal A, B, bias with the exact ties of test_topN_batch planted; user 0 has an empty exclusion list."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((nu, k)).astype(dtype); B = rng.standard_normal((n, k)).astype(dtype)
    B[7] = B[3]; B[11] = B[3]
    b = None
    if bias:
        b = rng.standard_normal(n).astype(dtype); b[7] = b[3]; b[11] = b[3]
    ep = ei = None
    if excl:
        lens = rng.integers(0, max_excl, nu); lens[0] = 0
        ep = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        ei = (np.concatenate([rng.choice(n, l, replace=False) for l in lens]).astype(np.int32) if lens.sum() else np.zeros(0, np.int32))
    return A, B, b, ep, ei


def scores64(A, B, bias):
    S = A.astype(np.float64) @ B.astype(np.float64).T
    if bias is not None:
        S = S + bias.astype(np.float64)
    return S


def bounds(A, B, bias, dtype):
    """E_u for every user."""
    M = np.abs(A.astype(np.float64)) @ np.abs(B.astype(np.float64)).T
    if bias is not None:
        M = M + np.abs(bias.astype(np.float64))
    return gamma(A.shape[1] + 1, dtype) * M.max(axis=1)


def check_ranking(A, B, bias, ep, ei, ids, sc, n_top, dtype, all_decided=False, verbose=True):
    """The four conditions for every user and position.  Returns (worst score error / E_u, undecided share);
    all_decided: the inputs must leave no position undecided (then every id must equal the reference's)."""
    nu, n = A.shape[0], B.shape[0]
    S = scores64(A, B, bias)
    E = bounds(A, B, bias, dtype)
    assert ids.shape == (nu, n_top) and sc.shape == (nu, n_top)
    worst, undecided, total = 0.0, 0, 0
    for u in range(nu):
        s = S[u].copy()
        ex = ei[int(ep[u]):int(ep[u + 1])] if ep is not None else np.zeros(0, np.int32)
        s[ex] = -np.inf
        order = np.lexsort((np.arange(n), -s))
        left = int(np.isfinite(s).sum())                      # items that can be returned
        nret = min(n_top, left)
        got = ids[u]
        assert np.array_equal(got[nret:], np.full(n_top - nret, -1)), (u, got[nret:])
        assert np.all(np.isneginf(sc[u, nret:])), (u, sc[u, nret:])
        g = got[:nret]
        # 1. distinct, in range, not excluded
        assert g.min(initial=0) >= 0 and g.max(initial=0) < n, u
        assert len(set(g.tolist())) == nret, u
        assert not set(g.tolist()) & set(ex.tolist()), u
        want = order[:nret]
        # 2. scores within E_u of the float64 scores of the returned ids
        err = np.abs(sc[u, :nret].astype(np.float64) - S[u, g])
        assert np.all(err <= E[u]), (u, float(err.max()), float(E[u]))
        worst = max(worst, float(err.max(initial=0.0)) / E[u])
        # 3. the returned item at j scores within 2 E_u of the reference's item at j
        gap = np.abs(S[u, g] - S[u, want])
        assert np.all(gap <= 2 * E[u]), (u, float(gap.max()), float(E[u]))
        # 4. decided positions: both neighbours in the float64 order more than 2 E_u away, or exactly tied
        so = s[order[:min(nret + 1, left)]]
        d = np.abs(np.diff(so))
        ok = (d > 2 * E[u]) | (d == 0)
        before = np.concatenate([[True], ok])[:nret]
        after = np.concatenate([ok, [True]])[:nret] if len(ok) >= nret else np.concatenate([ok, [True] * (nret - len(ok))])
        decided = before & after
        undecided += int((~decided).sum()); total += nret
        assert np.array_equal(g[decided], want[decided]), (u, np.nonzero(g != want)[0][:5])
    share = undecided / max(total, 1)
    if verbose:
        print("top-N check: dtype=%s nu=%d n=%d k=%d n_top=%d worst score error %.3f E_u, undecided share %.2e"
              % (np.dtype(dtype).name, nu, n, A.shape[1], n_top, worst, share))
    if all_decided:
        assert undecided == 0, "the test's own inputs leave %d positions undecided" % undecided
    return worst, share
