"""GPU: neighbours of a ranker's own rows (topn_similar_kernels.hpp) -- dot against the wide top-N bit for bit, cosine against a
float64 ranking with a derived tolerance (similar_reference.py), the stated arithmetic, the edges, the launch hooks, the
model-level calls and the refusals of the C entry points."""
import ctypes as C

import numpy as np
import pytest

import similar_reference as sr
import topn_reference as tr

pytestmark = pytest.mark.gpu

_name = lambda v: getattr(v, "__name__", str(v))     # noqa: E731
DOT_WIDTHS = [(np.float64, k) for k in (1, 3, 16, 17, 50, 64, 65, 128, 256)] + [(np.float32, k) for k in (1, 17, 64, 65, 200, 257, 272)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


def self_lists(q):
    return np.arange(len(q) + 1, dtype=np.uint64), np.asarray(q, np.int32)


@pytest.mark.parametrize("n_top", [10, 128])
@pytest.mark.parametrize("dtype,k", DOT_WIDTHS, ids=_name)
def test_dot_equals_wide_topn_bitwise(monkeypatch, dtype, k, n_top):
    """similar(q, "dot") is Ranker(B).topN(B[q], exclude=[[q_j]]) on the wide kernel: the same ids, the same score bits."""
    from cmfrec_amd import Ranker
    n = 1000
    B = sr.make_items(10 * k + n_top, dtype, n, k)
    q = sr.make_queries(k, n)
    monkeypatch.setenv("CMFREC_HIP_TOPN", "wide")
    with Ranker(B) as r:
        want = r.topN(B[q], n=n_top, exclude=self_lists(q))
        got = r.similar(q, n=n_top, metric="dot")
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(bits(got[1]), bits(want[1]))
    assert (got[0] >= 0).all()


COSINE = [(dt, n, k, n_top) for dt in (np.float64, np.float32) for (n, k, n_top) in sr.SHAPES]


def check_planted(ids, sc, q):
    """3, 7, 11 (and 20, the same cosine bits) adjacent in id order with equal score bits wherever they appear; 5 nowhere; query
    5 has no neighbours."""
    b = bits(sc)
    n_top = ids.shape[1]
    for j in range(len(q)):
        group = [i for i in (3, 7, 11, 20) if i != q[j]]
        there = np.nonzero(np.isin(ids[j], group))[0]
        if len(there) == 0:
            continue
        p0 = int(there[0])                                # ties go by id: the group's first, then the others as far as the list goes
        want = group[:n_top - p0]
        assert ids[j, p0:p0 + len(want)].tolist() == want, (j, ids[j, p0:p0 + 4])
        assert len(there) == len(want) and (b[j, p0:p0 + len(want)] == b[j, p0]).all(), (j, sc[j, p0:p0 + 4])
    assert not (ids == 5).any()
    j5 = list(q).index(5)
    assert (ids[j5] == -1).all() and np.isneginf(sc[j5]).all()


@pytest.mark.parametrize("dtype,n,k,n_top", COSINE, ids=["%s-n%d-k%d-top%d" % (np.dtype(c[0]).name, c[1], c[2], c[3]) for c in COSINE])
def test_cosine_against_reference(dtype, n, k, n_top):
    from cmfrec_amd import Ranker
    B = sr.make_items(100 + k, dtype, n, k)
    q = sr.make_queries(k, n)
    with Ranker(B) as r:
        ids, sc = r.similar(q, n=n_top)
    _, share = sr.check_neighbours(B, q, "cosine", None, None, ids, sc, n_top, dtype, all_decided=dtype is np.float64)
    assert share <= sr.F32_CAP
    check_planted(ids, sc, q)


@pytest.mark.parametrize("dtype,k", [(np.float64, 50), (np.float32, 65)], ids=_name)
def test_nan_row_behaves_like_the_zero_row(dtype, k):
    from cmfrec_amd import Ranker, ops
    n, n_top = 300, 33
    B = sr.make_items(7, dtype, n, k, nan_row=9)
    q = np.concatenate([sr.make_queries(3, n, 40), [9]]).astype(np.int32)
    q = q[np.sort(np.unique(q, return_index=True)[1])]
    with Ranker(B) as r:
        ids, sc = r.similar(q, n=n_top)
        rn = r.inverse_norms()
    assert np.isnan(rn[9]) and np.isnan(rn[5]) and np.isfinite(np.delete(rn, [5, 9])).all()
    sr.check_neighbours(B, q, "cosine", None, None, ids, sc, n_top, dtype, all_decided=dtype is np.float64)
    check_planted(ids, sc, q)
    assert not (ids == 9).any()
    j9 = list(q).index(9)
    assert (ids[j9] == -1).all() and np.isneginf(sc[j9]).all()
    assert same(ops.similar_batch(B, q, n_top=n_top), (ids, sc))


@pytest.mark.parametrize("dtype,k", [(np.float64, 50), (np.float64, 128), (np.float32, 64), (np.float32, 272)], ids=_name)
def test_cosine_is_the_stated_arithmetic(dtype, k):
    """(dot * rn[i]) * rn[q] in NumPy in the working dtype from the library's own dot scores and inverse norms is the cosine
    call's score, bit for bit; rn within gamma_{k/2+2} (relative) of the float64 inverse norm."""
    from cmfrec_amd import Ranker
    n, n_top = 300, 128
    B = sr.make_items(31 + k, dtype, n, k)
    q = sr.make_queries(k, n)
    with Ranker(B) as r:
        di, ds = r.similar(q, n=n_top, metric="dot")
        ci, cs = r.similar(q, n=n_top, metric="cosine")
        rn = r.inverse_norms()
    assert rn.dtype == dtype and rn.shape == (n,)
    live = np.arange(n) != 5
    want = np.full(n, np.nan)
    want[live] = 1.0 / np.sqrt((B[live].astype(np.float64) ** 2).sum(axis=1))
    assert np.isnan(rn[5])
    rel = np.abs(rn[live].astype(np.float64) - want[live]) / want[live]
    print("inverse norms: worst relative error %.3e, bound %.3e" % (rel.max(), tr.gamma(k / 2 + 2, dtype)))
    assert np.all(rel <= tr.gamma(k / 2 + 2, dtype))
    compared = 0
    for j in range(len(q)):
        if q[j] == 5:
            continue
        dots = {int(i): s for i, s in zip(di[j], ds[j]) if i >= 0 and i != 5}
        for i, s in zip(ci[j], cs[j]):
            if int(i) in dots:
                emu = dtype(dtype(dots[int(i)] * rn[i]) * rn[q[j]])
                assert bits(np.array([emu], dtype))[0] == bits(np.array([s], dtype))[0], (j, i, emu, s)
                compared += 1
    assert compared > 1000


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=_name)
@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 127, 128, 129])
def test_small_item_counts(dtype, n):
    from cmfrec_amd import Ranker
    k, n_top = 8, min(n, 128)
    B = sr.make_items(n, dtype, n, k)
    q = np.arange(n, dtype=np.int32)                     # every row asks (n = 129 with n_top = 128: the longest list)
    with Ranker(B) as r:
        for metric in ("cosine", "dot"):
            ids, sc = r.similar(q, n=n_top, metric=metric)
            sr.check_neighbours(B, q, metric, None, None, ids, sc, n_top, dtype, all_decided=dtype is np.float64)
            if n == 1:
                assert (ids == -1).all() and np.isneginf(sc).all()


@pytest.mark.parametrize("nq", [1, 16, 17, 64, 65])
def test_query_counts_duplicates_and_exclusions(nq):
    """Query counts around the tile sizes; a duplicate query gives an equal row; exclusion lists: an empty one, one that holds the
    query itself, one that leaves fewer than n_top rows."""
    from cmfrec_amd import Ranker
    dtype, n, k, n_top = np.float64, 129, 17, 20
    B = sr.make_items(nq, dtype, n, k)
    rng = np.random.default_rng(nq)
    q = rng.choice(n, nq, replace=False).astype(np.int32)
    if nq > 1:
        q[-1] = q[0]                                     # a duplicate
    lists = [np.sort(rng.choice(n, int(l), replace=False)) for l in rng.integers(0, 30, nq)]
    lists[0] = np.zeros(0, np.int64)
    if nq > 1:
        lists[-1] = lists[0]
    if nq > 2:
        lists[1] = np.union1d(lists[1], [q[1]])          # holds the query itself
        lists[2] = np.setdiff1d(np.arange(n), [q[2], 40, 41, 42, 5])[: n - 5]   # leaves three rows (5 has no cosine)
    ep = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
    ei = np.concatenate(lists).astype(np.int32)
    with Ranker(B) as r:
        for metric in ("cosine", "dot"):
            ids, sc = r.similar(q, n=n_top, metric=metric, exclude=(ep, ei))
            sr.check_neighbours(B, q, metric, ep, ei, ids, sc, n_top, dtype, all_decided=True)
            if nq > 1:
                assert np.array_equal(ids[0], ids[-1]) and np.array_equal(bits(sc[0]), bits(sc[-1]))
            if nq > 2:
                assert (ids[2] == -1).sum() >= n_top - 5
        e_ids, e_sc = r.similar(np.zeros(0, np.int32), n=n_top)
        assert e_ids.shape == (0, n_top) and e_sc.shape == (0, n_top)


@pytest.mark.parametrize("dtype,k,n_top", [(np.float64, 50, 10), (np.float32, 200, 100), (np.float64, 256, 128)], ids=_name)
def test_bytes_do_not_depend_on_the_launch(monkeypatch, dtype, k, n_top):
    """CMFREC_HIP_TOPN_TILES = 1..4, a second call, and CMFREC_HIP_POISON_LDS=1 on a ranker's first cosine call (which builds the
    norms) and on a later one: the same bytes."""
    from cmfrec_amd import Ranker
    n = 1000
    B = sr.make_items(k, dtype, n, k)
    q = sr.make_queries(k, n)
    monkeypatch.delenv("CMFREC_HIP_TOPN_TILES", raising=False)
    monkeypatch.delenv("CMFREC_HIP_POISON_LDS", raising=False)
    with Ranker(B) as r:
        base = {m: r.similar(q, n=n_top, metric=m) for m in ("cosine", "dot")}
        for m in ("cosine", "dot"):
            assert same(r.similar(q, n=n_top, metric=m), base[m])
        shapes = set()
        for tiles in (1, 2, 3, 4):
            monkeypatch.setenv("CMFREC_HIP_TOPN_TILES", str(tiles))
            for m in ("cosine", "dot"):
                assert same(r.similar(q, n=n_top, metric=m), base[m]), (tiles, m)
            shapes.add(r.launch_shape()[0])
            assert r.kernel_ms() > 0
        assert 16 in shapes and len(shapes) > 1
    monkeypatch.delenv("CMFREC_HIP_TOPN_TILES")
    monkeypatch.setenv("CMFREC_HIP_POISON_LDS", "1")
    with Ranker(B) as r:
        assert same(r.similar(q, n=n_top, metric="cosine"), base["cosine"])      # builds the norms
        assert same(r.similar(q, n=n_top, metric="cosine"), base["cosine"])
        assert same(r.similar(q, n=n_top, metric="dot"), base["dot"])


@pytest.mark.parametrize("dtype,k", [(np.float64, 50), (np.float32, 129)], ids=_name)
def test_existing_calls_are_untouched(dtype, k):
    """topN and ranks on a ranker with a bias return the bytes of a fresh ranker whatever similar calls come between."""
    from cmfrec_amd import Ranker
    nu, n, n_top = 40, 600, 10
    A, B, b, ep, ei = tr.make_problem(k, dtype, nu, n, k)
    held = (np.arange(nu + 1, dtype=np.int64) * 3, np.random.default_rng(2).integers(0, n, 3 * nu).astype(np.int32))
    with Ranker(B, b) as fresh:
        top0 = fresh.topN(A, n=n_top, exclude=(ep, ei))
    with Ranker(B, b) as fresh:
        rk0 = fresh.ranks(A, held, exclude=(ep, ei), return_scores=True)
    q = np.arange(0, 50, dtype=np.int32)
    with Ranker(B, b) as r, Ranker(B) as plain:
        sim = plain.similar(q, n=n_top, metric="dot")
        assert same(r.similar(q, n=n_top, metric="dot"), sim)                    # the bias plays no part
        assert same(r.topN(A, n=n_top, exclude=(ep, ei)), top0)
        cos = r.similar(q, n=n_top)
        rk = r.ranks(A, held, exclude=(ep, ei), return_scores=True)
        for a, c in zip(rk, rk0):
            assert np.array_equal(a, c, equal_nan=True)
        assert same(r.similar(q, n=n_top), cos)
        assert same(r.topN(A, n=n_top, exclude=(ep, ei)), top0)
        assert same(plain.similar(q, n=n_top), cos)


def _coo(m, n, nnz, seed, dtype, counts):
    rng = np.random.default_rng(seed)
    lin = rng.choice(m * n, nnz, replace=False)
    val = np.ceil(rng.lognormal(1, 1, nnz)) if counts else rng.integers(1, 6, nnz)
    return (lin // n).astype(np.int32), (lin % n).astype(np.int32), val.astype(dtype)


@pytest.mark.parametrize("use_float", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("model", ["CMF", "CMF_implicit"])
def test_model_level(model, use_float):
    from cmfrec_amd import CMF, CMF_implicit, Ranker
    dt = np.float32 if use_float else np.float64
    m, n = 150, 200
    rng = np.random.default_rng(4)
    if model == "CMF":
        row, col, val = _coo(m, n, 4000, 5, dt, False)
        U = rng.standard_normal((m, 4)).astype(dt); I = rng.standard_normal((n, 3)).astype(dt)
        mdl = CMF(k=6, k_user=2, k_item=3, k_main=1, lambda_=0.5, niter=2, use_float=use_float, random_state=3, nthreads=1,
                  item_bias=True, precompute_for_predictions=False).fit((row, col, val), U=U, I=I, shape=(m, n))
        assert mdl.k_item == 3 and mdl.k_user == 2 and mdl.item_bias
    else:
        row, col, val = _coo(m, n, 4000, 6, dt, True)
        mdl = CMF_implicit(k=8, lambda_=2.0, niter=2, use_float=use_float, random_state=5).fit((row, col, val), shape=(m, n))
    items = np.array([0, 3, 199, 17, 3]); users = np.array([149, 0, 7])
    for metric in ("cosine", "dot"):
        got = mdl.similar_items(items, n=7, metric=metric)
        with Ranker(np.ascontiguousarray(mdl.B_[:, mdl.k_item:])) as r:
            assert r.k == mdl.B_.shape[1] - mdl.k_item
            assert same(got, r.similar(items, n=7, metric=metric))
        with mdl.ranker() as mr:
            assert same(mr.similar_items(items, n=7, metric=metric), got)
        gu = mdl.similar_users(users, n=5, metric=metric)
        with Ranker(np.ascontiguousarray(mdl.A_[:, mdl.k_user:])) as r:
            assert same(gu, r.similar(users, n=5, metric=metric))
        assert gu[0].shape == (3, 5) and (gu[0] >= 0).all() and not (gu[0] == users[:, None]).any()
    with pytest.raises(ValueError, match="in \\[0, 200\\)"):
        mdl.similar_items([200])
    with pytest.raises(ValueError, match="metric"):
        mdl.similar_users([0], metric="l2")


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=_name)
def test_refusals_through_ctypes(dtype):
    """Return code 2 with a message that names the library's function, the outputs untouched; nq = 0 returns 0."""
    from cmfrec_amd import _lib, Ranker
    lib = _lib.load(dtype)
    n, k, nq, n_top = 200, 9, 4, 5
    B = sr.make_items(2, dtype, n, k)
    q = np.array([1, 2, 3, 4], np.int32)

    def call(r, q, metric=1, n_top=n_top, ep=None, ei=None, nq=nq, B=B):
        ids = np.full((nq, max(n_top, 1)), -7, np.int32); sc = np.full((nq, max(n_top, 1)), 7.5, dtype)
        if r is None:
            rc = lib.cmfrec_hip_similar_batch(_lib.ptr(B), B.shape[1], B.shape[0], B.shape[1], _lib.ptr(q), nq, metric, _lib.ptr(ep),
                                              _lib.ptr(ei), n_top, _lib.ptr(ids), _lib.ptr(sc))
        else:
            rc = lib.cmfrec_hip_ranker_similar(r.handle, _lib.ptr(q), nq, metric, _lib.ptr(ep), _lib.ptr(ei), n_top, _lib.ptr(ids),
                                               _lib.ptr(sc))
        return rc, ids, sc, (lib.cmfrec_hip_last_error() or b"").decode()

    def refused(out, needle=None):
        rc, ids, sc, msg = out
        assert rc == 2 and "cmfrec_hip" in msg, (rc, msg)
        if needle:
            assert needle in msg, msg
        assert (ids == -7).all() and (sc == 7.5).all()

    bad_p = np.array([0, 2, 1, 3, 3], np.uint64); some_i = np.array([5, 6, 7], np.int32)
    with Ranker(B) as r:
        for h in (r, None):
            refused(call(h, np.array([1, -1, 3, 4], np.int32)))
            refused(call(h, np.array([1, 2, n, 4], np.int32)))
            refused(call(h, None))
            refused(call(h, q, metric=2), "metric")
            refused(call(h, q, n_top=129), "k <= 272 and n_top <= min(128, n)")
            refused(call(h, q, ep=bad_p, ei=some_i))
            rc, ids, sc, _ = call(h, q, nq=0)
            assert rc == 0 and (ids == -7).all()
        refused(call(None, q, n_top=50, B=B[:40]), "n_top <= min(128, n)")
        with Ranker(B[:40]) as small:
            refused(call(small, q, n_top=50), "n_top <= min(128, n)")
        wide = np.ones((300, 273), dtype)
        refused(call(None, q, B=wide), "k <= 272")
        rc, ids, sc, _ = call(r, q)                        # and the handle still works
        assert rc == 0 and (ids >= 0).all()
