"""GPU: exact top-N through the certified fp16 filter (topn_filter_kernels.hpp) -- the keys against
float64 scores and the bound of DESIGN.md recomputed in NumPy, the filtered ranking against the float64 ranking
(topn_reference.check_ranking) and against the same ranker with the filter off, near-ties the halves cannot see, small
catalogues, non-finite inputs and the limits of the interface."""
import numpy as np
import pytest

import topn_reference as tr

pytestmark = pytest.mark.gpu

NU, N = 37, 1003          # a partial user tile, a partial item round, more than 7 rounds per wavefront
WIDTHS = [(np.float64, k) for k in (5, 32, 33, 64, 129, 256)] + [(np.float32, k) for k in (5, 32, 33, 64, 129, 256, 272)]
WIDTH_IDS = lambda v: getattr(v, "__name__", str(v))


def half_image(X, whole):
    """(|X~_i|, |X_i - X~_i|) per row, X~ = half(X 2^s) 2^-s with halves below 2^-14 flushed; s brings the largest |entry| -- of the
    matrix (whole) or of each row -- into [2^13, 2^14), at most 2^54: the image of DESIGN.md section 3.17."""
    X = X.astype(np.float64)
    mx = np.abs(X).max() * np.ones(len(X)) if whole else np.abs(X).max(axis=1)
    e = np.frexp(mx.astype(np.float32))[1] - 1
    s = np.where(mx > 0, np.minimum(13 - e, 54), 54).astype(np.float64)[:, None]
    h = (X * 2.0 ** s).astype(np.float32).astype(np.float16).astype(np.float64)
    h[np.abs(h) < 2.0 ** -14] = 0
    Xt = h * 2.0 ** -s
    return np.linalg.norm(Xt, axis=1), np.linalg.norm(X - Xt, axis=1)


def key_bound(A, B, bias, S, dtype):
    """e(u, j) of DESIGN.md section 3.17, in float64."""
    k = A.shape[1]
    kh8 = (k + 31) // 32 * 32 + 8
    C, W = 2 * kh8 * 2.0 ** -22, kh8 * (2.0 ** -52 if np.dtype(dtype) == np.float64 else 2.0 ** -23)
    na, da = half_image(A, False)
    nb, db = half_image(B, True)
    e0 = np.outer(na, db + C * nb) + np.outer(da + W * (na + da), nb + db)
    ab = 0 if bias is None else np.abs(bias.astype(np.float64))
    return e0 + 2.0 ** -21 * (np.abs(S) + ab + e0) + 2.0 ** -120


def key_inputs(kind, dtype, k):
    rng = np.random.default_rng(900 + k)
    A = rng.standard_normal((NU, k)); B = rng.standard_normal((N, k)); b = rng.standard_normal(N)
    if kind == "tiny":
        A, B, b = A * 1e-6, B * 1e-6, b * 1e-12
    elif kind == "large":
        A, B, b = A * 1e4, B * 1e4, b * 1e8
    elif kind == "spread":                    # one item row and one user row from 2^-30 to 2^10: halves that are flushed
        span = 2.0 ** np.linspace(-30, 10, k)
        B[5] = span * np.sign(B[5]); A[3] = span[::-1] * np.sign(A[3])
    return A.astype(dtype), B.astype(dtype), b.astype(dtype)


@pytest.mark.parametrize("kind", ["normal", "tiny", "large", "spread"])
@pytest.mark.parametrize("dtype,k", WIDTHS, ids=WIDTH_IDS)
def test_keys_bound_scores(dtype, k, kind):
    """key >= the float64 score for every pair, and key - score <= 4 e with e recomputed from DESIGN.md's formula."""
    from cmfrec_amd import Ranker
    A, B, b = key_inputs(kind, dtype, k)
    with Ranker(B, b, filter="fp16") as r:
        keys = r.filter_keys(A).astype(np.float64)
    S = tr.scores64(A, B, b)
    e = key_bound(A, B, b, S, dtype)
    print("keys: %s k=%d %s: min (key - score) / e = %.3f, max = %.3f" % (np.dtype(dtype).name, k, kind, ((keys - S) / e).min(), ((keys - S) / e).max()))
    assert np.all(np.isfinite(keys))
    assert np.all(keys >= S)
    assert np.all(keys - S <= 4 * e)


def same_lists(ids, sc, ids0, sc0, dtype):
    """The filtered result against the unfiltered one: the refinement repeats the unfiltered kernel's arithmetic, so ids and scores
    are the same bits."""
    assert np.array_equal(ids, ids0)
    assert np.array_equal(sc, sc0, equal_nan=True)


@pytest.mark.parametrize("n_top", [1, 10, 64])
@pytest.mark.parametrize("dtype,k", WIDTHS, ids=WIDTH_IDS)
def test_separated_inputs(dtype, k, n_top):
    """Gaussian inputs with bias and exclusion lists: the float64 ranking, the ids of the filter-off ranker, every user certified --
    after the float64 scores themselves have shown that position n_top clears position M + 1 by more than the bound."""
    from cmfrec_amd import Ranker
    from cmfrec_amd.rank import filter_shortlist
    A, B, b, ep, ei = tr.make_problem(3000 + 7 * k + n_top, dtype, NU, N, k)
    with Ranker(B, b, filter="fp16") as r:
        ids, sc = r.topN(A, n=n_top, exclude=(ep, ei))
        stats = r.filter_stats()
        r.filter = None
        ids0, sc0 = r.topN(A, n=n_top, exclude=(ep, ei))
    tr.check_ranking(A, B, b, ep, ei, ids, sc, n_top, dtype, all_decided=dtype is np.float64)
    same_lists(ids, sc, ids0, sc0, dtype)
    S = tr.scores64(A, B, b)
    upper = S + 2.5 * key_bound(A, B, b, S, dtype)            # no key lies above this (test_keys_bound_scores: 4 e over two sides)
    E = tr.bounds(A, B, b, dtype)
    M = filter_shortlist(n_top)
    for u in range(NU):
        ex = ei[int(ep[u]):int(ep[u + 1])]
        s, up = S[u].copy(), upper[u].copy()
        s[ex] = -np.inf; up[ex] = -np.inf
        assert np.sort(s)[-n_top] - E[u] > np.sort(up)[-M], "the test's own inputs do not separate user %d" % u
    assert stats == {"users": NU, "filtered": NU, "certified": NU}


@pytest.mark.parametrize("dtype,k", WIDTHS, ids=WIDTH_IDS)
def test_near_ties_fall_back(dtype, k):
    """Items b_0 (1 + j 2^-18) (2^-14 in single precision) and a few exact duplicates: the halves cannot tell them apart, the
    certificate must fail and the exact route decide -- the list is the filter-off list."""
    from cmfrec_amd import Ranker
    rng = np.random.default_rng(50 + k)
    b0 = rng.standard_normal(k)
    step = 2.0 ** -18 if dtype is np.float64 else 2.0 ** -14
    B = (b0[None, :] * (1 + np.arange(N)[:, None] * step)).astype(dtype)
    B[20] = B[500]; B[N - 3] = B[N - 9]; B[7] = B[N - 1]
    # users at an angle to b_0 (cosine about 0.15): the steps are far above the rounding of the exact kernels, far below the bound
    A = 0.25 * np.abs(rng.standard_normal((NU, k))) * np.sign(b0) + rng.standard_normal((NU, k))
    A[1::2] *= -1
    A = A.astype(dtype)
    with Ranker(B, filter="fp16") as r:
        ids, sc = r.topN(A, n=10)
        stats = r.filter_stats()
        r.filter = None
        ids0, sc0 = r.topN(A, n=10)
    same_lists(ids, sc, ids0, sc0, dtype)
    assert stats["filtered"] == NU and stats["certified"] < NU, stats


@pytest.mark.parametrize("case", ["m32", "n5", "n40", "tiles2", "tiles4", "tiles8"])
@pytest.mark.parametrize("dtype,k", [(np.float64, 33), (np.float32, 272)], ids=WIDTH_IDS)
def test_forced_shortlist_small_catalogues_and_tiles(monkeypatch, dtype, k, case):
    """CMFREC_HIP_TOPN_FILTER_M=32 at n_top = 16; catalogues of 5 and 40 items under heavy exclusion (fewer than M rankable items:
    complete by construction, -1 / -inf padding, certified); the 32-, 64- and 128-user instantiations of the kernel."""
    from cmfrec_amd import Ranker
    n, n_top, max_excl = {"n5": (5, 5, 5), "n40": (40, 10, 39)}.get(case, (N, 16, 60))
    if case == "m32":
        monkeypatch.setenv("CMFREC_HIP_TOPN_FILTER_M", "32")
    if case.startswith("tiles"):
        monkeypatch.setenv("CMFREC_HIP_TOPN_TILES", case[5:])
    rng = np.random.default_rng(70 + k + n)
    A = rng.standard_normal((NU, k)).astype(dtype); B = rng.standard_normal((n, k)).astype(dtype); b = rng.standard_normal(n).astype(dtype)
    lens = rng.integers(max_excl // 2, max_excl + 1, NU); lens[0] = 0
    ep = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    ei = np.concatenate([np.sort(rng.choice(n, l, replace=False)) for l in lens]).astype(np.int32)
    with Ranker(B, b, filter="fp16") as r:
        ids, sc = r.topN(A, n=n_top, exclude=(ep, ei))
        stats = r.filter_stats()
        users_per_wg = r.launch_shape()[0]
    tr.check_ranking(A, B, b, ep, ei, ids, sc, n_top, dtype)
    assert stats == {"users": NU, "filtered": NU, "certified": NU}
    if case.startswith("tiles"):
        assert users_per_wg == 16 * int(case[5:])
    if n < 32:
        assert (ids == -1).any()


@pytest.mark.parametrize("dtype,k", [(np.float64, 64), (np.float32, 129)], ids=WIDTH_IDS)
def test_non_finite_inputs(dtype, k):
    """A NaN and an inf among the items: no image, nothing filtered.  A NaN user row: that user alone is not certified.  Either
    way the result is the filter-off result."""
    from cmfrec_amd import Ranker
    A, B, b, ep, ei = tr.make_problem(11 + k, dtype, NU, N, k)
    Bbad = B.copy(); Bbad[17, 2] = np.nan; Bbad[300, k - 1] = np.inf
    Abad = A.copy(); Abad[4, k // 2] = np.nan
    for Bx, Ax, want in ((Bbad, A, {"users": NU, "filtered": 0, "certified": 0}), (B, Abad, {"users": NU, "filtered": NU, "certified": NU - 1})):
        with Ranker(Bx, b, filter="fp16") as r:
            ids, sc = r.topN(Ax, n=10, exclude=(ep, ei))
            stats = r.filter_stats()
            r.filter = None
            ids0, sc0 = r.topN(Ax, n=10, exclude=(ep, ei))
        assert stats == want
        same_lists(ids, sc, ids0, sc0, dtype)


@pytest.mark.parametrize("dtype,k", [(np.float64, 33), (np.float32, 256)], ids=WIDTH_IDS)
def test_interface_limits(dtype, k):
    """n_top = 65 with the filter on takes the exact route; switching the filter off returns the ranker to the bytes of one that
    never had it; the keyword reaches ops.topN_batch."""
    from cmfrec_amd import Ranker, ops
    A, B, b, ep, ei = tr.make_problem(23 + k, dtype, NU, N, k)
    with Ranker(B, b) as r0:
        want65, want10 = r0.topN(A, n=65, exclude=(ep, ei)), r0.topN(A, n=10, exclude=(ep, ei))
    with Ranker(B, b, filter="fp16") as r:
        assert r.filter == "fp16"
        got65 = r.topN(A, n=65, exclude=(ep, ei))
        assert r.filter_stats() == {"users": NU, "filtered": 0, "certified": 0}
        r.filter = None
        got10 = r.topN(A, n=10, exclude=(ep, ei))
    for got, want in ((got65, want65), (got10, want10)):
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    ids, sc = ops.topN_batch(A, B, n_top=10, biasB=b, exclude=(ep, ei), filter="fp16")
    same_lists(ids, sc, want10[0], want10[1], dtype)
