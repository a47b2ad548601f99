"""GPU: deep lists and next pages (topn_after_kernels.hpp; Ranker.topN_deep / topN_after, ops.topN_deep_batch, the estimators'
topN_deep) -- against the float64 ranking of topn_reference.py, bit for bit against the rank kernel and the wide top-N kernel,
and against itself under every page length and tiling.

The problem of every test: topn_reference.make_problem(seed 11, nu = 70) with a block of 40 exactly tied items (200 .. 239),
and -- by the flags of problem() -- user 2 with an exclusion list that leaves 5 items, user 4 a row of NaN, item 150 with a bias
of -inf.  An item that scores -inf is written as -1 / -inf by every top-N kernel of the library, like an empty position, while
the rank kernel counts it as an item: the comparison with the rank kernel therefore runs without item 150's bias."""
import ctypes as C
import functools

import numpy as np
import pytest

import topn_reference as tr
from conftest import make_coo

pytestmark = pytest.mark.gpu

FEW_USER, NAN_USER, NEG_ITEM = 2, 4, 150
F64, F32 = np.float64, np.float32


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for v in ("CMFREC_HIP_TOPN", "CMFREC_HIP_TOPN_TILES", "CMFREC_HIP_TOPN_PAGE"):
        monkeypatch.delenv(v, raising=False)


@functools.lru_cache(maxsize=None)
def problem(dtype, n, k, nu=70, few=True, nan_row=True, neg_inf=True):
    """(A, B, bias, excl_p, excl_i) as handed to the library, and (B_ref, bias_ref, excl_p_ref, excl_i_ref): the same ranking
    for the float64 reference -- item 150 in everybody's exclusion list in place of its bias of -inf (an infinite bias would
    make the reference's error bound infinite for every user).  Cached and never written to."""
    A, B, b, ep, ei = tr.make_problem(11, dtype, nu, n, k)
    B[200:240] = B[200]; b[200:240] = b[200]
    lists = [ei[int(ep[u]):int(ep[u + 1])] for u in range(nu)]
    if few and nu > FEW_USER:
        keep = np.array([3, 210, 211, n - 1, 77])                # two of them inside the tie block
        lists[FEW_USER] = np.setdiff1d(np.arange(n), keep).astype(np.int32)[::-1].copy()      # descending: the binding sorts
    if nan_row and nu > NAN_USER:
        A[NAN_USER] = np.nan
    b_ref = b.copy()
    ref_lists = lists
    if neg_inf:
        b[NEG_ITEM] = -np.inf
        ref_lists = [np.union1d(l, [NEG_ITEM]).astype(np.int32) for l in lists]

    def csr(ls):
        return np.concatenate([[0], np.cumsum([len(l) for l in ls])]).astype(np.uint64), np.concatenate(ls).astype(np.int32)
    out = (A, B, b) + csr(lists) + (B, b_ref) + csr(ref_lists)
    for a in out:
        a.setflags(write=False)
    return out


def same(a, b):
    """ids equal and scores equal bit for bit"""
    return np.array_equal(a[0], b[0]) and a[1].dtype == b[1].dtype and np.array_equal(a[1].view(np.uint8), b[1].view(np.uint8))


def default_pages(dtype, k, n_top):
    """(launches, page length) the host chooses without the hook (128, and 256 / 512 where measured faster)."""
    if n_top <= 128:
        length = 128
    elif dtype is F64:
        length = 512 if k >= 192 else 256 if k >= 96 else 128
    else:
        length = 256 if k >= 192 else 128
    length = min(length, n_top)
    return (n_top + length - 1) // length, length


DEEP_SHAPES = [(300, 300), (1000, 129), (1000, 1000)]
CASES = [(F64, k, s, 70) for k in (3, 50, 64, 65, 129, 256) for s in DEEP_SHAPES] + [(F32, 64, s, 70) for s in DEEP_SHAPES] + \
    [(F32, 272, (300, 300), 70), (F64, 50, (1000, 129), 1), (F32, 129, (300, 300), 1)]


@pytest.mark.parametrize("dtype,k,shape,nu", CASES, ids=lambda v: getattr(v, "__name__", str(v)).replace(" ", ""))
def test_deep_against_float64(dtype, k, shape, nu):
    """topn_reference.check_ranking on topN_deep.  Double precision: no position undecided, every id the reference's.  Single
    precision: the reference itself leaves a few per cent of the positions of these deep lists undecided (k = 64: 0.5 - 2.8 %,
    k = 272 at 300 items: 4.3 %); the share must stay under 0.08."""
    from cmfrec_amd import Ranker
    n, n_top = shape
    A, B, b, ep, ei, Br, br, epr, eir = problem(dtype, n, k, nu)
    with Ranker(B, b) as r:
        ids, sc = r.topN_deep(A, n_top, exclude=(ep, ei))
        pages = r.pages()
    assert pages == default_pages(dtype, k, n_top)
    worst, share = tr.check_ranking(A, Br, br, epr, eir, ids, sc, n_top, dtype, all_decided=dtype is F64)
    if dtype is F32:
        assert share < 0.08, share
    assert not (ids == NEG_ITEM).any()
    if nu > NAN_USER:
        assert (ids[NAN_USER] == -1).all() and np.isneginf(sc[NAN_USER]).all()
        assert set(ids[FEW_USER, :5].tolist()) == {3, 77, 210, 211, n - 1}
        assert (ids[FEW_USER, 5:] == -1).all() and np.isneginf(sc[FEW_USER, 5:]).all()
        # the tied pair of the five comes lower id first
        pos = {int(i): j for j, i in enumerate(ids[FEW_USER, :5])}
        assert pos[211] == pos[210] + 1 and sc[FEW_USER, pos[210]] == sc[FEW_USER, pos[211]]


@pytest.mark.parametrize("dtype,k", [(F64, 50), (F32, 129)], ids=lambda v: getattr(v, "__name__", str(v)))
def test_deep_against_rank_kernel(dtype, k):
    """No tolerance, against a kernel this feature does not touch: with every item held out, an item of rank r >= 0 stands at
    position r of the full deep list with the same score bits, and the rank is -1 exactly for the items the list lacks."""
    from cmfrec_amd import Ranker
    n = 300
    A, B, b, ep, ei = problem(dtype, n, k, 70, True, True, False)[:5]
    nu = A.shape[0]
    held = (np.arange(nu + 1, dtype=np.uint64) * np.uint64(n), np.tile(np.arange(n, dtype=np.int32), nu))
    with Ranker(B, b) as r:
        ids, sc = r.topN_deep(A, n, exclude=(ep, ei))
        hp, hi, ranks, pool, rsc = r.ranks(A, held, exclude=(ep, ei), return_scores=True)
    assert np.array_equal(hi, held[1])
    ranks = ranks.reshape(nu, n); rsc = rsc.reshape(nu, n)
    u, item = np.nonzero(ranks >= 0)
    assert len(u) > nu * 100
    assert np.array_equal(ids[u, ranks[u, item]], item)
    bits = np.uint64 if dtype is F64 else np.uint32
    assert np.array_equal(sc[u, ranks[u, item]].view(bits), rsc[u, item].view(bits))
    for v in range(nu):
        listed = ids[v][ids[v] >= 0]
        assert len(np.unique(listed)) == len(listed) == pool[v]
        assert np.array_equal(np.flatnonzero(ranks[v] == -1), np.setdiff1d(np.arange(n), listed))
    assert pool[NAN_USER] == 0 and pool[FEW_USER] == 5


@pytest.mark.parametrize("dtype,k", [(F64, 50), (F32, 129)], ids=lambda v: getattr(v, "__name__", str(v)))
def test_page_length_and_tiling_do_not_matter(monkeypatch, dtype, k):
    """CMFREC_HIP_TOPN_PAGE = 7 .. 256 and CMFREC_HIP_TOPN_TILES = 1 / 4: the same ids and score bits; pages() reports the
    launches.  43 pages of 7 put many page boundaries inside the block of 40 tied items."""
    from cmfrec_amd import Ranker
    for n, n_top in ((300, 300), (1000, 257)):
        A, B, b, ep, ei = problem(dtype, n, k)[:5]
        with Ranker(B, b) as r:
            base = r.topN_deep(A, n_top, exclude=(ep, ei))
            assert r.pages() == ((n_top + 127) // 128, 128)
            for page in (7, 32, 100, 128, 256):
                monkeypatch.setenv("CMFREC_HIP_TOPN_PAGE", str(page))
                got = r.topN_deep(A, n_top, exclude=(ep, ei))
                assert r.pages() == ((n_top + page - 1) // page, page), (page, r.pages())
                assert same(got, base), (n, n_top, page)
            for tiles in (1, 4):
                monkeypatch.setenv("CMFREC_HIP_TOPN_TILES", str(tiles))
                for page in (256, 32):
                    monkeypatch.setenv("CMFREC_HIP_TOPN_PAGE", str(page))
                    assert same(r.topN_deep(A, n_top, exclude=(ep, ei)), base), (n, n_top, page, tiles)
                assert r.launch_shape()[0] == 16 * tiles            # (pages of 32 fit four user tiles)
            monkeypatch.delenv("CMFREC_HIP_TOPN_TILES"); monkeypatch.delenv("CMFREC_HIP_TOPN_PAGE")
        # a page longer than the list, and the hook out of range (ignored)
        monkeypatch.setenv("CMFREC_HIP_TOPN_PAGE", "512")
        with Ranker(B, b) as r:
            assert same(r.topN_deep(A, n_top, exclude=(ep, ei)), base) and r.pages() == (1, n_top)
            monkeypatch.setenv("CMFREC_HIP_TOPN_PAGE", "513")
            assert same(r.topN_deep(A, n_top, exclude=(ep, ei)), base) and r.pages() == ((n_top + 127) // 128, 128)
        monkeypatch.delenv("CMFREC_HIP_TOPN_PAGE")


@pytest.mark.parametrize("dtype,k", [(F64, 50), (F32, 129)], ids=lambda v: getattr(v, "__name__", str(v)))
def test_chaining_by_hand(dtype, k):
    """Pages of 50 through topN_after, each fed the last column of the page before, concatenate to topN_deep(300); the user with
    5 rankable items gets -1 / -inf from position 5 on in every later page; the start cursor (+inf, -1) is after=None; a NaN
    cursor admits nothing; the cursor's own item may be excluded by now."""
    from cmfrec_amd import Ranker
    n = 300
    A, B, b, ep, ei = problem(dtype, n, k)[:5]
    nu = A.shape[0]
    with Ranker(B, b) as r:
        deep = r.topN_deep(A, n, exclude=(ep, ei))
        with pytest.raises(RuntimeError, match=r"code 2.*n_top <= min\(128, n\)"):
            r.topN_after(A, None, None, n=129)
        first = r.topN_after(A, None, None, n=50, exclude=(ep, ei))
        start = r.topN_after(A, np.full(nu, -1, np.int32), np.full(nu, np.inf, dtype), n=50, exclude=(ep, ei))
        assert same(first, start)
        pages = [first]
        for p in range(1, 6):
            last = pages[-1]
            pages.append(r.topN_after(A, last[0][:, -1], last[1][:, -1], n=50, exclude=(ep, ei)))
            r.ranks(A[:3], (np.array([0, 1, 1, 2], np.uint64), np.array([5, 9], np.int32)))         # other calls in between
            assert (pages[-1][0][FEW_USER] == -1).all() and np.isneginf(pages[-1][1][FEW_USER]).all()
        chained = (np.concatenate([p[0] for p in pages], axis=1), np.concatenate([p[1] for p in pages], axis=1))
        assert same(chained, deep)
        assert r.pages() == (3, 128)                                # topN_after leaves the record of the deep call alone
        # a NaN cursor: nothing
        nan_page = r.topN_after(A, np.zeros(nu, np.int32), np.full(nu, np.nan, dtype), n=10, exclude=(ep, ei))
        assert (nan_page[0] == -1).all() and np.isneginf(nan_page[1]).all()
        # user 0 (no exclusion list before): its cursor item and the item behind it are excluded now -- the page goes on behind
        u0 = deep[0][0]
        ep2 = np.concatenate([[0], np.full(nu, 2)]).astype(np.uint64); ei2 = np.array([u0[9], u0[10]], np.int32)
        got = r.topN_after(A, deep[0][:, 9].copy(), deep[1][:, 9].copy(), n=10, exclude=(ep2, ei2))
        assert np.array_equal(got[0][0], u0[11:21]) and np.array_equal(got[1][0], deep[1][0, 11:21])


def test_against_the_existing_route(monkeypatch):
    """n <= 128: topN_deep is Ranker.topN on the MFMA kernel bit for bit (k = 50 under CMFREC_HIP_TOPN=wide, k = 129 as it
    is); the same call twice gives the same bytes; out_scores == NULL and the one-call entry point."""
    from cmfrec_amd import Ranker, _lib, ops
    for dtype, k, wide in ((F64, 50, True), (F32, 50, True), (F64, 129, False), (F32, 129, False)):
        A, B, b, ep, ei = problem(dtype, 300, k)[:5]
        nu = A.shape[0]
        with Ranker(B, b) as r:
            for n_top in (1, 10, 128):
                if wide:
                    monkeypatch.setenv("CMFREC_HIP_TOPN", "wide")
                want = r.topN(A, n=n_top, exclude=(ep, ei))
                monkeypatch.delenv("CMFREC_HIP_TOPN", raising=False)
                got = r.topN_deep(A, n_top, exclude=(ep, ei))
                assert same(got, want), (dtype, k, n_top)
                assert same(r.topN_deep(A, n_top, exclude=(ep, ei)), got)
            deep = r.topN_deep(A, 300, exclude=(ep, ei))
            assert same(r.topN_deep(A, 300, exclude=(ep, ei)), deep)
            # scores are optional for the caller (the pages still chain on the device's own)
            owner = np.repeat(np.arange(nu), np.diff(ep.astype(np.int64)))
            eis = np.ascontiguousarray(ei[np.lexsort((ei, owner))])
            ids = np.empty((nu, 300), np.int32)
            rc = r.lib.cmfrec_hip_ranker_topN_deep(r.handle, _lib.ptr(A), k, nu, _lib.ptr(ep), _lib.ptr(eis), 300, _lib.ptr(ids), None)
            _lib.check(rc, r.lib, "topN_deep")
            assert np.array_equal(ids, deep[0])
        assert same(ops.topN_deep_batch(A, B, 300, biasB=b, exclude=(ep, ei)), deep)
        with pytest.raises(RuntimeError, match=r"code 2.*1 <= n_top <= n"):
            ops.topN_deep_batch(A, B, 301, biasB=b)
    with Ranker(B, b) as r:
        with pytest.raises(RuntimeError, match="code 2"):
            r.pages()                                               # no deep call on this handle yet


@pytest.mark.parametrize("use_float", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("model", ["CMF", "CMF_implicit"])
def test_models(model, use_float):
    """CMF.topN_deep / CMF_implicit.topN_deep(users, 200, exclude=X_train) equal ranker().topN_deep and pass the float64 check on
    the model's factors; ranker().topN_after continues a page."""
    from cmfrec_amd import CMF, CMF_implicit
    dt = F32 if use_float else F64
    m, n = 120, 300
    if model == "CMF":
        row, col, val = make_coo(m, n, 3000, 4, counts=False, dtype=dt)
        mdl = CMF(k=20, lambda_=0.5, niter=2, use_float=use_float, random_state=9, nthreads=1, precompute_for_predictions=False).fit(
            (row, col, val), shape=(m, n))
        bias = np.ascontiguousarray(mdl.item_bias_, dt)
    else:
        row, col, val = make_coo(m, n, 3000, 3, dtype=dt)
        mdl = CMF_implicit(k=24, lambda_=3.0, niter=2, use_float=use_float, random_state=7).fit((row, col, val), shape=(m, n))
        bias = None
    lists = [np.unique(col[row == u]).astype(np.int32) for u in range(m)]
    train = (np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64), np.concatenate(lists))
    users = np.array([0, 5, 17, 119, 50, 3] + list(range(60, 100)))
    got = mdl.topN_deep(users, 200, exclude=train)
    with mdl.ranker() as mr:
        want = mr.topN_deep(users, 200, exclude=train)
        assert mr.pages() == (2, 128)
        head = mr.topN_after(users, None, None, n=100, exclude=train)
        tail = mr.topN_after(users, head[0][:, -1], head[1][:, -1], n=100, exclude=train)
    assert same(got, want)
    assert same((np.concatenate([head[0], tail[0]], axis=1), np.concatenate([head[1], tail[1]], axis=1)), want)
    A = np.ascontiguousarray(mdl.A_[users][:, mdl.k_user:]); B = np.ascontiguousarray(mdl.B_[:, mdl.k_item:])
    ep = np.concatenate([[0], np.cumsum([len(lists[u]) for u in users])]).astype(np.uint64)
    ei = np.concatenate([lists[u] for u in users]).astype(np.int32)
    worst, share = tr.check_ranking(A, B, bias, ep, ei, got[0], got[1], 200, dt, all_decided=not use_float)
    if use_float:
        assert share < 0.08, share
