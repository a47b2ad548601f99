"""GPU: diversified top-N (topn_mmr_kernels.hpp) -- the MMR kernel through Ranker.rerank_mmr against the
float64 greedy of mmr_reference (a replay that tolerates near ties, the ids themselves in double precision, the exact order at
tradeoff 1), and topN_diverse against rerank_mmr over topN's own pools."""
import numpy as np
import pytest

import mmr_reference as ref
from conftest import make_coo

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
NU, N = 70, 300

# dtype, k, pool, n_top, tradeoff, CMFREC_HIP_MMR_GROUPS (0: none), the special users
CASES = [
    (F64, 3, 1, 1, 0.7, 2, False), (F64, 50, 17, 17, 0.7, 2, False), (F64, 65, 33, 10, 0.0, 2, False), (F64, 256, 128, 128, 0.7, 2, False),
    (F64, 256, 100, 50, 0.0, 0, False), (F64, 65, 128, 1, 0.7, 2, False), (F64, 3, 128, 64, 1.0, 2, False), (F64, 50, 100, 100, 1.0, 2, False),
    (F64, 50, 33, 33, 0.7, 2, True),
    (F32, 3, 17, 8, 0.0, 2, False), (F32, 64, 33, 33, 0.7, 2, False), (F32, 272, 128, 128, 0.7, 0, False), (F32, 272, 100, 1, 1.0, 2, False),
    (F32, 64, 1, 1, 0.0, 2, False), (F32, 272, 128, 60, 1.0, 2, False), (F32, 64, 33, 33, 0.7, 2, True),
]


def make_pools(dtype, k, pool, special):
    """B [N, k], ids [NU, pool] (a random subset of the items per user), Gaussian scores.  special: item 7 a zero row, items 8 and
    9 identical, all three in user 0's pool; user 1 has five valid pairs; user 2's scores are all equal."""
    rng = np.random.default_rng(1000 * k + pool)
    B = rng.standard_normal((N, k)).astype(dtype)
    ids = np.stack([rng.permutation(N)[:pool] for _ in range(NU)]).astype(np.int32)
    sc = rng.standard_normal((NU, pool)).astype(dtype)
    if special:
        B[7] = 0; B[9] = B[8]
        ids[0, :3] = (7, 8, 9); ids[0, 3:] = 10 + rng.permutation(N - 10)[:pool - 3]
        ids[1, 5:] = -1; sc[1, 5:] = -np.inf
        sc[2] = 0.25
    return B, ids, sc


@pytest.mark.parametrize("dtype,k,pool,n_top,theta,groups,special", CASES,
                         ids=lambda v: getattr(v, "__name__", str(v)))
def test_kernel_against_float64_greedy(dtype, k, pool, n_top, theta, groups, special, monkeypatch):
    from cmfrec_amd import Ranker
    B, ids, sc = make_pools(dtype, k, pool, special)
    if groups:
        monkeypatch.setenv("CMFREC_HIP_MMR_GROUPS", str(groups))
    with Ranker(B) as r:
        got_ids, got_sc, got_v = r.rerank_mmr(ids, sc, n=n_top, tradeoff=theta, output_mmr=True)
        assert r.launch_shape() == (1, groups or NU)            # one user per workgroup at a time; uncapped: a workgroup each
    tol = ref.margin(k, dtype)
    th = float(dtype(theta))                                     # (the kernel takes the tradeoff in its own precision)
    for u in range(NU):
        ref.replay(B, ids[u], sc[u], th, got_ids[u], got_sc[u], got_v[u], tol)
        if dtype is F64:
            picks, _, gap = ref.greedy(B, ids[u], sc[u], th, n_top)
            assert gap > tol, (u, gap, tol)                      # (the case itself: its picks are beyond rounding)
            assert np.array_equal(got_ids[u, :len(picks)], ids[u][picks]), u
        if theta == 1.0:
            valid = (ids[u] >= 0) & np.isfinite(sc[u])
            order = [p for p in np.lexsort((np.arange(pool), -sc[u].astype(np.float64))) if valid[p]][:n_top]
            assert np.array_equal(got_ids[u, :len(order)], ids[u][order]) and np.array_equal(got_sc[u, :len(order)], sc[u][order]), u


def ranked_inputs(dtype, k):
    """Users, items, a bias, and exclusion lists that leave user 0 twenty items: fewer than the pool."""
    rng = np.random.default_rng(77 + k)
    nu, n = 37, 150
    A = rng.standard_normal((nu, k)).astype(dtype); B = rng.standard_normal((n, k)).astype(dtype)
    b = rng.standard_normal(n).astype(dtype)
    lists = [np.arange(20, n)] + [np.sort(rng.permutation(n)[:rng.integers(0, 30)]) for _ in range(nu - 1)]
    ep = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
    return A, B, b, (ep, np.concatenate(lists).astype(np.int32))


@pytest.mark.parametrize("dtype,k", [(F64, 50), (F64, 128), (F32, 272)], ids=lambda v: getattr(v, "__name__", str(v)))
def test_topN_diverse_is_rerank_of_topN(dtype, k):
    from cmfrec_amd import Ranker
    n_top, pool = 30, 64
    A, B, b, excl = ranked_inputs(dtype, k)
    same = lambda x, y: all(p.tobytes() == q.tobytes() for p, q in zip(x, y))
    with Ranker(B, b) as r:
        top = r.topN(A, n=pool, exclude=excl)
        assert (top[0][0] >= 0).sum() == 20
        for theta in (0.7, 0.0):
            got = r.topN_diverse(A, n=n_top, pool=pool, tradeoff=theta, exclude=excl, output_mmr=True)
            assert same(got, r.rerank_mmr(*top, n=n_top, tradeoff=theta, output_mmr=True)), theta
            assert same(got, r.topN_diverse(A, n=n_top, pool=pool, tradeoff=theta, exclude=excl, output_mmr=True)), theta
            assert np.all(got[0][0, 20:] == -1) and np.all(got[1][0, 20:] == -np.inf)
        assert same(r.topN_diverse(A, n=n_top, pool=pool, tradeoff=1.0, exclude=excl), (top[0][:, :n_top].copy(), top[1][:, :n_top].copy()))


def test_model_topN_diverse():
    from cmfrec_amd import CMF_implicit
    m, n = 120, 200
    row, col, val = make_coo(m, n, 3000, 3, dtype=F64)
    mdl = CMF_implicit(k=24, lambda_=3.0, niter=2, use_float=False, random_state=7).fit((row, col, val), shape=(m, n))
    users = np.arange(0, m, 3)
    got = mdl.topN_diverse(users, n=10, pool=32, tradeoff=0.5)
    with mdl.ranker() as r:
        want = r.topN_diverse(users, n=10, pool=32, tradeoff=0.5)
        plain = r.topN(users, n=10)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[0][:, 0], plain[0][:, 0]) and not np.array_equal(got[0], plain[0])
