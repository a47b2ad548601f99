"""GPU: ranks of held-out items (topn_rank_kernels.hpp; Ranker.ranks, ops.ranks_batch, the models, NewUsers.ranks,
cmfrec_hip_ranker_ranks and its kin).

Two oracles.  Exact: under CMFREC_HIP_TOPN=wide, topN(A, n_top, exclude)[u, rank] == t with the same score bits for every
rank < n_top -- with n <= 128 that is the user's whole order.  Float64: ranks_reference.ranks64 with its allowance for pairs the
working precision cannot tell apart, whose share is capped in test_ranks_reference_cpu.py on the same inputs."""
import ctypes as C

import numpy as np
import pytest

import ranks_reference as rr
import topn_reference as tr
from conftest import make_coo

pytestmark = pytest.mark.gpu

KS = [(np.float64, k) for k in (1, 3, 16, 17, 50, 64, 65, 128, 256)] + [(np.float32, k) for k in (1, 3, 16, 17, 50, 64, 65, 128, 256, 272)]
IDS = dict(ids=lambda v: getattr(v, "__name__", str(v)))


@pytest.fixture
def wide(monkeypatch):
    monkeypatch.setenv("CMFREC_HIP_TOPN", "wide")
    monkeypatch.delenv("CMFREC_HIP_TOPN_TILES", raising=False)
    monkeypatch.delenv("CMFREC_HIP_RANK_SLICE", raising=False)


def expect_from_topn(ids, sc, held, dtype):
    """Where each held-out item stands in the rows of a top-N result (-1: not in it) and the score it has there."""
    hp, hi = held
    want = np.full(len(hi), -1, np.int32); wsc = np.full(len(hi), np.nan, dtype)
    for u in range(len(hp) - 1):
        for j in range(int(hp[u]), int(hp[u + 1])):
            at = np.flatnonzero(ids[u] == hi[j])
            if hi[j] >= 0 and len(at):
                want[j] = at[0]; wsc[j] = sc[u, at[0]]
    return want, wsc


def same_bits(a, b):
    return a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("dtype,k", KS, **IDS)
def test_exact_whole_order(dtype, k, wide):
    """n <= 128: the rank of every held-out item is its position in topN(n_top = n) of the wide kernel, scores bit-equal; the
    planted equal rows 3 / 7 / 11 are held out, so ties go by id.  nu x n x (bias, exclusions) in one test per (dtype, k)."""
    from cmfrec_amd import Ranker
    for n in (1, 15, 16, 127, 128):
        for nu in (1, 16, 17, 70):
            for with_bias, with_excl in ((True, True), (False, False)):
                A, B, b, excl = rr.small_problem(100 + n + nu, dtype, nu, n, k, with_bias, with_excl)
                held = rr.heldout_lists(n + nu, nu, n, min(n, 6))
                with Ranker(B, b) as rk:
                    ids, sc = rk.topN(A, n=n, exclude=excl)
                    hp, hi, ranks, pool, got_sc = rk.ranks(A, held, exclude=excl, return_scores=True)
                    assert rk.kernel_ms() > 0
                assert np.array_equal(hp, held[0].astype(np.int64)) and np.array_equal(hi, held[1])
                want, wsc = expect_from_topn(ids, sc, held, dtype)
                tag = (n, nu, with_bias)
                assert np.array_equal(ranks, want), (tag, np.flatnonzero(ranks != want)[:5])
                assert same_bits(got_sc[want >= 0], wsc[want >= 0]) and np.all(np.isnan(got_sc[want < 0])), tag
                assert np.array_equal(pool, (ids >= 0).sum(axis=1)), tag
                if n > 11:                                          # the ties: consecutive places in id order
                    for u in range(nu):
                        r = {int(t): int(x) for t, x in zip(hi[int(hp[u]):int(hp[u + 1])], ranks[int(hp[u]):int(hp[u + 1])])}
                        live = [r[t] for t in (3, 7, 11) if r[t] >= 0]
                        assert live == list(range(live[0], live[0] + len(live))) if live else True, (tag, u)


@pytest.mark.parametrize("dtype,k,n", rr.ROUND_CASES, **IDS)
def test_several_rounds(dtype, k, n, wide):
    """n = 129, 257, 1000: ranks below 128 exact against topN(n_top = 128); every rank against float64 within the allowance of
    ranks_reference (its share capped), equal where the allowance is 0; pool exact."""
    from cmfrec_amd import Ranker
    A, B, b, excl, held = rr.round_problem(dtype, k, n)
    with Ranker(B, b) as rk:
        ids, sc = rk.topN(A, n=128, exclude=excl)
        hp, hi, ranks, pool, got_sc = rk.ranks(A, held, exclude=excl, return_scores=True)
    want, wsc = expect_from_topn(ids, sc, held, dtype)
    low = (ranks >= 0) & (ranks < 128)
    assert np.array_equal(low, want >= 0)
    assert np.array_equal(ranks[low], want[low]) and same_bits(got_sc[low], wsc[low])
    r64, near, pool64 = rr.ranks64(A, B, b, held, excl, dtype)
    share = rr.near_share(r64, near)
    print("ranks: dtype=%s k=%d n=%d: undecided share %.4f, worst |rank - rank64| %d" %
          (np.dtype(dtype).name, k, n, share, int(np.abs(ranks - r64).max())))
    assert share <= rr.CAP[dtype]
    assert np.array_equal(ranks < 0, r64 < 0)
    assert np.all(np.abs(ranks - r64) <= near), np.flatnonzero(np.abs(ranks - r64) > near)[:5]
    assert np.array_equal(ranks[near == 0], r64[near == 0])
    assert np.array_equal(pool, pool64)


@pytest.mark.parametrize("dtype,k", [(np.float64, 50), (np.float32, 272)], **IDS)
def test_corner_cases(dtype, k, wide):
    from cmfrec_amd import Ranker, _lib
    nu, n = 20, 200
    A, B, b, excl = rr.small_problem(7, dtype, nu, n, k, True, True)
    B[50] = np.nan                                                   # a NaN item row
    A[5] = np.nan                                                    # a NaN user row
    ex = rr.lists_of_csr(*excl)
    ex[3] = np.union1d(ex[3], [10, 11])                              # user 3: held-out items 10, 11 are excluded
    excl = rr.csr_of_lists(ex)
    lists = rr.lists_of_csr(*rr.heldout_lists(9, nu, n, 8))
    lists[0] = np.zeros(0, np.int64)                                 # without held-out items
    lists[2] = np.arange(n)                                          # all n items held out
    lists[3] = np.union1d(lists[3], [10, 11])
    lists[4] = np.union1d(lists[4], [50])
    held = rr.csr_of_lists(lists)
    with Ranker(B, b) as rk:
        hp, hi, ranks, pool = rk.ranks(A, held, exclude=excl)
        again = rk.ranks(A, held, exclude=excl)
        ids, sc = rk.topN(A, n=128, exclude=excl)
    assert all(np.array_equal(x, y) for x, y in zip((hp, hi, ranks, pool), again))
    per = rr.lists_of_csr(hp, ranks)
    assert len(per[0]) == 0 and pool[0] == n - 1                     # user 0 excludes nothing; item 50 is NaN
    r2 = per[2]
    gone = np.union1d(ex[2], [50])
    assert np.all(r2[gone] == -1) and pool[2] == n - len(gone)
    assert np.array_equal(np.sort(r2[r2 >= 0]), np.arange(pool[2]))  # a permutation of 0 .. pool - 1
    for t in (10, 11):
        assert per[3][np.flatnonzero(lists[3] == t)[0]] == -1
    assert per[4][np.flatnonzero(lists[4] == 50)[0]] == -1
    assert np.all(per[5] == -1) and pool[5] == 0 and len(per[5]) > 0
    want, _ = expect_from_topn(ids, sc, held, dtype)
    low = (ranks >= 0) & (ranks < 128)
    assert np.array_equal(low, want >= 0) and np.array_equal(ranks[low], want[low])
    r64, near, pool64 = rr.ranks64(A, B, b, held, excl, dtype)
    assert np.array_equal(pool, pool64) and np.array_equal(ranks < 0, r64 < 0) and np.all(np.abs(ranks - r64) <= near)
    # ids -1 and n at the C level: -1, the neighbours unaffected
    lists_c = [np.concatenate([[-1], x, [n]]) for x in lists]
    hp_c, hi_c = rr.csr_of_lists(lists_c)
    lib = _lib.load(dtype)
    out = np.full(len(hi_c), 77, np.int32); osc = np.zeros(len(hi_c), dtype); opool = np.full(nu, 77, np.int32)
    rc = lib.cmfrec_hip_ranks_batch(_lib.ptr(A), k, nu, _lib.ptr(B), k, n, k, _lib.ptr(b), _lib.ptr(hp_c), _lib.ptr(hi_c),
                                    _lib.ptr(excl[0]), _lib.ptr(excl[1]), _lib.ptr(out), _lib.ptr(osc), _lib.ptr(opool))
    assert rc == 0, lib.cmfrec_hip_last_error()
    got = rr.lists_of_csr(hp_c, out)
    for u in range(nu):
        assert got[u][0] == -1 and got[u][-1] == -1 and np.array_equal(got[u][1:-1], per[u]), u
    assert np.array_equal(opool, pool) and np.array_equal(np.isnan(osc), out < 0)


LAUNCH = [(np.float64, 50), (np.float32, 272), (np.float64, 256)]


@pytest.mark.parametrize("dtype,k", LAUNCH, **IDS)
def test_launch_independence(dtype, k, monkeypatch, wide):
    """The same integers whatever the tiles per workgroup (1 .. 4), the slice (1, 2, default) and the order of the batch: 300
    users, one with 40 held-out items among users with 0 .. 3."""
    from cmfrec_amd import Ranker
    nu, n = 300, 300
    A, B, b, excl = rr.small_problem(11, dtype, nu, n, k, True, True)
    lens = np.random.default_rng(2).integers(0, 4, nu); lens[123] = 40
    held = rr.heldout_lists(12, nu, n, lens)
    lists, ex = rr.lists_of_csr(*held), rr.lists_of_csr(*excl)
    perm = np.random.default_rng(3).permutation(nu)
    with Ranker(B, b) as rk:
        hp, hi, ranks, pool = rk.ranks(A, held, exclude=excl)
        base_shape = rk.launch_shape()
        ids, sc = rk.topN(A, n=128, exclude=excl)
        want, _ = expect_from_topn(ids, sc, held, dtype)
        low = (ranks >= 0) & (ranks < 128)
        assert np.array_equal(low, want >= 0) and np.array_equal(ranks[low], want[low])
        shapes = set()
        for tiles, slice_ in [(t, None) for t in (1, 2, 3, 4)] + [(None, 1), (None, 2), (1, 1), (4, 2)]:
            for name, v in (("CMFREC_HIP_TOPN_TILES", tiles), ("CMFREC_HIP_RANK_SLICE", slice_)):
                if v is None:
                    monkeypatch.delenv(name, raising=False)
                else:
                    monkeypatch.setenv(name, str(v))
            got = rk.ranks(A, held, exclude=excl)
            shapes.add(rk.launch_shape())
            assert np.array_equal(got[2], ranks) and np.array_equal(got[3], pool), (tiles, slice_)
            if tiles == 1:
                assert rk.launch_shape() == (16, 19)
        assert len(shapes) >= 2 and base_shape[0] in (16, 32, 48, 64)
        monkeypatch.delenv("CMFREC_HIP_TOPN_TILES", raising=False); monkeypatch.delenv("CMFREC_HIP_RANK_SLICE", raising=False)
        hp_s, hi_s, ranks_s, pool_s = rk.ranks(A[perm], rr.csr_of_lists([lists[u] for u in perm]),
                                               exclude=rr.csr_of_lists([ex[u] for u in perm]))
    per, per_s = rr.lists_of_csr(hp, ranks), rr.lists_of_csr(hp_s, ranks_s)
    for j, u in enumerate(perm):
        assert np.array_equal(per_s[j], per[u]), u
    assert np.array_equal(pool_s, pool[perm])


def test_a_workgroup_takes_several_tiles(monkeypatch, wide):
    """More user tiles than the launch has workgroups (one tile of 16 users per workgroup, k = 3, 40 items): a workgroup goes on
    to further tiles, with the ranks of the default launch and of the top-N kernel."""
    from cmfrec_amd import Ranker
    dtype, k, n = np.float64, 3, 40
    nu = 16 * 4 * 304 + 40                                          # more tiles than 4 workgroups on each of 304 compute units
    A, B, b, excl = rr.small_problem(13, dtype, nu, n, k, True, False)
    held = rr.heldout_lists(14, nu, n, np.random.default_rng(4).integers(0, 3, nu))
    with Ranker(B, b) as rk:
        base = rk.ranks(A, held)
        monkeypatch.setenv("CMFREC_HIP_TOPN_TILES", "1")
        got = rk.ranks(A, held)
        users, groups = rk.launch_shape()
        ids, sc = rk.topN(A, n=n)
    assert users == 16 and users * groups < nu
    assert np.array_equal(got[2], base[2]) and np.array_equal(got[3], base[3])
    want, _ = expect_from_topn(ids, sc, held, dtype)
    assert np.array_equal(got[2], want) and np.all(got[3] == n)


@pytest.mark.parametrize("dtype,k", [(np.float64, 128), (np.float32, 65)], **IDS)
def test_one_handle_interleaved(dtype, k, wide):
    """topN, topN(include=) and ranks interleaved on one Ranker, batches growing and shrinking: each equals the one-shot call."""
    from cmfrec_amd import Ranker, ops
    nu, n = 150, 400
    A, B, b, ep, ei = tr.make_problem(31, dtype, nu, n, k)
    held = rr.heldout_lists(32, nu, n, np.random.default_rng(5).integers(0, 9, nu))
    inc = rr.heldout_lists(33, nu, n, 50)

    def cut(p, i, lo, hi):
        return (p[lo:hi + 1] - p[lo]).astype(np.uint64), i[int(p[lo]):int(p[hi])]

    with Ranker(B, b) as rk:
        for lo, hi in ((0, 33), (33, 150), (5, 6), (0, 150), (100, 140)):
            excl = cut(ep, ei, lo, hi)
            ids, sc = rk.topN(A[lo:hi], n=10, exclude=excl)
            r1 = rk.ranks(A[lo:hi], cut(*held, lo, hi), exclude=excl)
            idc, scc = rk.topN(A[lo:hi], n=10, exclude=excl, include=cut(*inc, lo, hi))
            r2 = rk.ranks(A[lo:hi], cut(*held, lo, hi))
            one = ops.ranks_batch(A[lo:hi], B, cut(*held, lo, hi), biasB=b, exclude=excl)
            one2 = ops.ranks_batch(A[lo:hi], B, cut(*held, lo, hi), biasB=b)
            assert all(np.array_equal(x, y) for x, y in zip(r1, one)) and all(np.array_equal(x, y) for x, y in zip(r2, one2))
            ids1, sc1 = ops.topN_batch(A[lo:hi], B, n_top=10, biasB=b, exclude=excl)
            idc1, scc1 = ops.topN_batch(A[lo:hi], B, n_top=10, biasB=b, exclude=excl, include=cut(*inc, lo, hi))
            assert np.array_equal(ids, ids1) and np.array_equal(sc, sc1) and np.array_equal(idc, idc1) and np.array_equal(scc, scc1)
            want, _ = expect_from_topn(ids, sc, cut(*held, lo, hi), dtype)
            low = (r1[2] >= 0) & (r1[2] < 10)
            assert np.array_equal(low, want >= 0) and np.array_equal(r1[2][low], want[low])


def test_c_entry_points(wide):
    """cmfrec_hip_ranks_batch and cmfrec_hip_ranker_ranks through ctypes; optional outputs; k = 273 refused with code 2 and the
    outputs untouched; offsets that decrease refused."""
    from cmfrec_amd import Ranker, _lib
    dtype, k, n = np.float64, 50, 257
    A, B, b, excl, held = rr.round_problem(dtype, k, n)
    nu = A.shape[0]
    lib = _lib.load(dtype)
    with Ranker(B, b) as rk:
        hp, hi, ranks, pool, sc = rk.ranks(A, held, exclude=excl, return_scores=True)
        only = np.full(len(hi), 77, np.int32)
        rc = lib.cmfrec_hip_ranker_ranks(rk.handle, _lib.ptr(A), k, nu, _lib.ptr(held[0]), _lib.ptr(held[1]), _lib.ptr(excl[0]),
                                         _lib.ptr(excl[1]), _lib.ptr(only), None, None)
        assert rc == 0 and np.array_equal(only, ranks)
        bad_p = held[0].copy(); bad_p[3] = bad_p[5] + 1
        only[:] = 77
        rc = lib.cmfrec_hip_ranker_ranks(rk.handle, _lib.ptr(A), k, nu, _lib.ptr(bad_p), _lib.ptr(held[1]), None, None, _lib.ptr(only),
                                         None, None)
        assert rc == 2 and np.all(only == 77)
        assert np.array_equal(rk.ranks(A, held, exclude=excl)[2], ranks)        # the handle stays usable
    out = np.full(len(hi), 77, np.int32); osc = np.zeros(len(hi)); opool = np.full(nu, 77, np.int32)
    rc = lib.cmfrec_hip_ranks_batch(_lib.ptr(A), k, nu, _lib.ptr(B), k, n, k, _lib.ptr(b), _lib.ptr(held[0]), _lib.ptr(held[1]),
                                    _lib.ptr(excl[0]), _lib.ptr(excl[1]), _lib.ptr(out), _lib.ptr(osc), _lib.ptr(opool))
    assert rc == 0, lib.cmfrec_hip_last_error()
    assert np.array_equal(out, ranks) and np.array_equal(opool, pool) and same_bits(osc[out >= 0], sc[out >= 0])
    A2 = np.zeros((nu, 273)); B2 = np.ones((n, 273))
    out[:] = 77; opool[:] = 77
    rc = lib.cmfrec_hip_ranks_batch(_lib.ptr(A2), 273, nu, _lib.ptr(B2), 273, n, 273, None, _lib.ptr(held[0]), _lib.ptr(held[1]),
                                    None, None, _lib.ptr(out), None, _lib.ptr(opool))
    assert rc == 2 and b"k <= 272" in lib.cmfrec_hip_last_error() and np.all(out == 77) and np.all(opool == 77)


_fitted = {}


def _fit(model, use_float):
    """The two small models of test_gpu_ranker.py, fitted once per precision; the training matrix as CSR lists."""
    from cmfrec_amd import CMF, CMF_implicit
    if (model, use_float) in _fitted:
        return _fitted[(model, use_float)]
    dt = np.float32 if use_float else np.float64
    m, n = 400, 600
    if model == "CMF":
        row, col, val = make_coo(m, n, 20000, 4, counts=False, dtype=dt)
        mdl = CMF(k=72, lambda_=0.5, niter=2, use_cg=True, finalize_chol=False, use_float=use_float, random_state=9, nthreads=1,
                  precompute_for_predictions=False).fit((row, col, val), shape=(m, n))
    else:
        row, col, val = make_coo(m, n, 20000, 3, dtype=dt)
        mdl = CMF_implicit(k=80, lambda_=3.0, niter=2, use_cg=True, finalize_chol=False, use_float=use_float, random_state=7).fit(
            (row, col, val), shape=(m, n))
    train = rr.csr_of_lists([np.unique(col[row == u]) for u in range(m)])
    _fitted[(model, use_float)] = (mdl, train)
    return mdl, train


@pytest.mark.parametrize("use_float", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("model", ["CMF", "CMF_implicit"])
def test_models(model, use_float, wide):
    """ModelRanker.ranks == model.ranks_batch == Ranker.ranks on the model's factors; NewUsers.ranks == Ranker.ranks on the factors
    NewUsers returns with the rows' own items as the exclusion lists; evaluate_ranking == ranking_metrics on those ranks."""
    from cmfrec_amd import Ranker
    from cmfrec_amd.metrics import METRICS, mean_metrics, ranking_metrics
    dt = np.float32 if use_float else np.float64
    mdl, train = _fit(model, use_float)
    m, n = mdl.A_.shape[0], mdl.B_.shape[0]
    bias = np.ascontiguousarray(mdl.item_bias_, dt) if model == "CMF" else None
    B = np.ascontiguousarray(mdl.B_[:, mdl.k_item:])
    users = np.array([0, 5, 17, 399, 250, 3] + list(range(100, 160)))
    held = rr.heldout_lists(51, len(users), n, 7)
    tl = rr.lists_of_csr(*train)
    with Ranker(B, bias) as rk:
        want = rk.ranks(np.ascontiguousarray(mdl.A_[users][:, mdl.k_user:]), held, exclude=rr.csr_of_lists([tl[u] for u in users]))
        want_plain = rk.ranks(np.ascontiguousarray(mdl.A_[users][:, mdl.k_user:]), held)
    with mdl.ranker() as mr:
        got = mr.ranks(users, held, exclude=train)
        got_plain = mr.ranks(users, held)
    one = mdl.ranks_batch(users, held, exclude=train)
    for a, b_, c in zip(want, got, one):
        assert np.array_equal(a, b_) and np.array_equal(a, c)
    assert all(np.array_equal(a, b_) for a, b_ in zip(want_plain, got_plain))
    assert (want[2] == -1).any() and (want[2] >= 0).any() and not (want_plain[2] == -1).any()
    # evaluate_ranking: held-out lists over ALL users (some without any), in batches of 64 users
    lens = np.random.default_rng(52).integers(0, 6, m); lens[::7] = 0
    test = rr.heldout_lists(53, m, n, lens)
    res = mdl.evaluate_ranking(test, X_train=train, k=10, batch_users=64)
    todo = np.flatnonzero(lens > 0)
    with mdl.ranker() as mr:
        ip, _, ranks, pool = mr.ranks(todo, rr.csr_of_lists([rr.lists_of_csr(*test)[u] for u in todo]), exclude=train)
    ref = mean_metrics(ranking_metrics(ip, ranks, pool, k=10))
    assert res["users"] == ref["users"] > 0
    for name in METRICS:
        assert res[name] == pytest.approx(ref[name], rel=1e-12), name
    some = mdl.evaluate_ranking(test, k=5, users=[1, 2, 3, 7, 14])
    assert some["users"] == int((lens[[1, 2, 3, 7, 14]] > 0).sum())
    # new users
    rng = np.random.default_rng(41)
    rows = 30
    ln = rng.integers(1, 40, rows)
    r = np.repeat(np.arange(rows), ln).astype(np.int32)
    c = np.concatenate([rng.choice(n, l, replace=False) for l in ln]).astype(np.int32)
    v = (0.5 * rng.integers(1, 11, len(r)) if model == "CMF" else np.ceil(rng.lognormal(1, 1, len(r)))).astype(dt)
    seen = rr.csr_of_lists([np.sort(c[r == u]) for u in range(rows)])
    held_n = rr.csr_of_lists([np.union1d(rng.choice(n, 6, replace=False), c[r == u][:1]) for u in range(rows)])
    more = rr.csr_of_lists([np.sort(rng.choice(n, 9, replace=False)) for u in range(rows)])
    with mdl.new_users() as nw:
        hp, hi, ranks, pool, (Af, _) = nw.ranks(X=(r, c, v), heldout=held_n, exclude_seen=True, return_factors=True)
        s_ms, r_ms = nw.kernel_ms()
        assert s_ms > 0 and r_ms > 0
        both = nw.ranks(X=(r, c, v), heldout=held_n, exclude_seen=True, exclude=more)
        ids_p, _ = nw.topN(X=(r, c, v), n=10, exclude_seen=True)                    # a top-N call on the same handle, afterwards
        assert np.array_equal(Af, nw.factors(X=(r, c, v)))
    Au = np.ascontiguousarray(Af[:, mdl.k_user:])
    union = rr.csr_of_lists([np.union1d(a, b_) for a, b_ in zip(rr.lists_of_csr(*seen), rr.lists_of_csr(*more))])
    with Ranker(B, bias) as rk:
        want = rk.ranks(Au, held_n, exclude=seen)
        want_both = rk.ranks(Au, held_n, exclude=union)
        ids_w, _ = rk.topN(Au, n=10, exclude=seen)
    assert all(np.array_equal(a, b_) for a, b_ in zip(want, (hp, hi, ranks, pool)))
    assert all(np.array_equal(a, b_) for a, b_ in zip(want_both, both))
    assert np.array_equal(ids_p, ids_w) and (ranks == -1).sum() >= rows


def test_newrows_refusal_leaves_outputs():
    """What cmfrec_hip_newrows_topN refuses, cmfrec_hip_newrows_ranks refuses with the same message; the outputs are left alone and
    the handle stays usable; held_p == NULL is code 2."""
    from cmfrec_amd import _lib
    mdl, _ = _fit("CMF_implicit", False)
    n = mdl.B_.shape[0]
    rng = np.random.default_rng(43)
    rows = 12
    ln = rng.integers(1, 30, rows)
    r = np.repeat(np.arange(rows), ln).astype(np.int32)
    c = np.concatenate([rng.choice(n, l, replace=False) for l in ln]).astype(np.int32)
    v = np.ceil(rng.lognormal(1, 1, len(r)))
    held = rr.heldout_lists(44, rows, n, 5)
    with mdl.new_users() as nw:
        st, keep, got_rows = nw._batch((r, c, v), None, None)
        fn = nw.lib.cmfrec_hip_newrows_ranks
        out = np.full(len(held[1]), 77, np.int32); pool = np.full(rows, 77, np.int32); Af = np.empty((rows, nw.width))
        refused = _lib.NewRowsBatch.from_buffer_copy(st)
        refused.Xfull = Af.ctypes.data                                           # X both dense and sparse: what factors refuses
        rc = fn(nw.handle, C.byref(refused), _lib.ptr(held[0]), _lib.ptr(held[1]), 1, None, None, _lib.ptr(out), None, _lib.ptr(pool), None, None)
        msg = nw.lib.cmfrec_hip_last_error()
        ids = np.full((rows, 10), 77, np.int32)
        rc1 = nw.lib.cmfrec_hip_newrows_topN(nw.handle, C.byref(refused), 1, None, None, 10, _lib.ptr(ids), None, None, None)
        assert rc != 0 and rc1 == rc and nw.lib.cmfrec_hip_last_error() == msg and np.all(out == 77) and np.all(pool == 77)
        rc = fn(nw.handle, C.byref(st), None, None, 1, None, None, _lib.ptr(out), None, _lib.ptr(pool), None, None)
        assert rc == 2 and np.all(out == 77)
        rc = fn(nw.handle, C.byref(st), _lib.ptr(held[0]), _lib.ptr(held[1]), 1, None, None, _lib.ptr(out), None, _lib.ptr(pool), None, None)
        assert rc == 0, nw.lib.cmfrec_hip_last_error()
        hp, hi, ranks, pool2 = nw.ranks(X=(r, c, v), heldout=held)
    assert np.array_equal(out, ranks) and np.array_equal(pool, pool2) and np.all(pool == n - ln)


def test_planted_model_ranks_its_held_out_items_high():
    """End to end: an implicit model fitted on planted low-rank preferences ranks the held-out items of each user well above
    the middle of the list."""
    from cmfrec_amd import CMF_implicit
    rng = np.random.default_rng(0)
    m, n, kk = 300, 200, 4
    S = rng.standard_normal((m, kk)) @ rng.standard_normal((n, kk)).T + 0.3 * rng.standard_normal((m, n))
    liked = np.argsort(-S, axis=1)[:, :30]                           # each user's 30 best items: 24 to train on, 6 held out
    pick = np.stack([rng.permutation(30) for _ in range(m)])
    tr_items = np.take_along_axis(liked, pick[:, :24], axis=1); te_items = np.take_along_axis(liked, pick[:, 24:], axis=1)
    row = np.repeat(np.arange(m), 24).astype(np.int32); col = tr_items.ravel().astype(np.int32)
    mdl = CMF_implicit(k=8, lambda_=1.0, niter=5, use_float=False, random_state=1).fit((row, col, np.ones(len(row))), shape=(m, n))
    train = rr.csr_of_lists([np.sort(x) for x in tr_items]); test = rr.csr_of_lists([np.sort(x) for x in te_items])
    res = mdl.evaluate_ranking(test, X_train=train, k=10)
    print("planted model:", res)
    assert res["users"] == m and res["auc"] > 0.5 and res["mean_rank"] < (n - 24) / 2
    assert 0 <= res["precision"] <= 1 and 0 <= res["ndcg"] <= 1 and 0 < res["rr"] <= 1
