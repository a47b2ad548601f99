"""Stochastic top-N (topn_sample_kernels.hpp, Ranker.topN_sample): keys against the float64 reference of sample_reference.py
under its derived bounds, scores against the wide kernel bit for bit, the log-partition, the lazy bound and the refusals.  The two
tests without the gpu mark check the helper's bound and this file's own inputs on the CPU."""
import ctypes as C

import numpy as np
import pytest

import sample_reference as sr
import topn_reference as tr

gpu = pytest.mark.gpu
SEED = 0x1234567887654321
NS = (1, 10, 128)
# dtype, k, CMFREC_HIP_TOPN_TILES (None: the default), n cycled over the cases, with_lse alternating
CASES = [(dt, k, tiles) for dt in (np.float64, np.float32) for k in (3, 64, 65, 272) for tiles in (None, 1)]
CASES = [c + (NS[(i + 1) % 3], i % 4 < 2) for i, c in enumerate(CASES)]
IDS = ["%s-k%d-tiles%s-n%d%s" % (np.dtype(c[0]).name, c[1], c[2], c[3], "-lse" if c[4] else "") for c in CASES]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def problem(dtype, k, t_scale=1.0):
    A, B, b, ep, ei = sr.make_case(7 * k + 1, dtype, k)
    S = tr.scores64(A, B, b)
    T = float(dtype(t_scale * S.std()))
    return A, B, b, ep, ei, S, T


def wide_scores(monkeypatch, r, A, ids):
    """The wide kernel's score bits of the pairs (u, ids[u, j]): topN over everything else excluded, looked up by id."""
    n = r.n
    lists = [np.setdiff1d(np.arange(n, dtype=np.int32), row[row >= 0]) for row in ids]
    ep = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
    monkeypatch.setenv("CMFREC_HIP_TOPN", "wide")
    wi, ws = r.topN(A, n=ids.shape[1], exclude=(ep, np.concatenate(lists)))
    look = [dict(zip(wi[u].tolist(), ws[u].tolist())) for u in range(len(ids))]
    return np.array([[look[u][i] if i >= 0 else -np.inf for i in ids[u].tolist()] for u in range(len(ids))], A.dtype)


def test_bound_dominates_gumbel():
    rng = np.random.default_rng(3)
    edge = [0, 1, 2 ** 64 - 1, 2 ** 63, 2 ** 63 - 1, 2 ** 64 - 2 ** 11, 2 ** 64 - 2 ** 11 - 1, 2 ** 64 - 2 ** 40, 2 ** 64 - 2 ** 40 - 1]
    edge += [2 ** 64 - 2 ** j for j in range(64)] + [2 ** 64 - 2 ** j - 1 for j in range(1, 64)] + [2 ** j for j in range(64)]
    h = np.concatenate([np.array(edge, np.uint64), rng.integers(0, 2 ** 64, 200000, dtype=np.uint64), sr.hashes(SEED, 37, 1000).ravel()])
    for dtype in (np.float64, np.float32):
        g = sr.gumbel(h, dtype)
        assert np.all(np.isfinite(g))
        # (the slack c is for the kernel's rounding of g: two units in the last place of 1 + |g|, see the helper)
        assert np.all(g + 4 * tr.unit_roundoff(dtype) * (1 + np.abs(g)) <= sr.gumbel_bound(h) - sr.BOUND_C / 2)


@pytest.mark.parametrize("dtype,k,tiles,n_top,with_lse", CASES, ids=IDS)
def test_inputs_leave_few_positions_undecided(dtype, k, tiles, n_top, with_lse):
    A, B, b, ep, ei, S, T = problem(dtype, k)
    _, share = sr.check_keys(*sr.keys_and_bounds(A, B, b, S, T, SEED, dtype), ep, ei, n_top)
    assert share == 0 if dtype == np.float64 else share <= 0.10, share


@gpu
@pytest.mark.parametrize("dtype,k,tiles,n_top,with_lse", CASES, ids=IDS)
def test_parity(monkeypatch, dtype, k, tiles, n_top, with_lse):
    from cmfrec_amd import Ranker
    A, B, b, ep, ei, S, T = problem(dtype, k)
    if tiles is not None:
        monkeypatch.setenv("CMFREC_HIP_TOPN_TILES", str(tiles))
    with Ranker(B, b) as r:
        out = r.topN_sample(A, n_top, T, SEED, exclude=(ep, ei), with_lse=with_lse)
        ids, sc, keys = out[:3]
        want_sc = wide_scores(monkeypatch, r, A, ids)
    worst, share = sr.check_keys(*sr.keys_and_bounds(A, B, b, S, T, SEED, dtype), ep, ei, n_top, ids, keys)
    print("sample check: %s k=%d n=%d worst key error %.3f EK_u, undecided share %.2e" % (np.dtype(dtype).name, k, n_top, worst, share))
    assert share == 0 if dtype == np.float64 else share <= 0.10, share
    assert np.array_equal(bits(sc), bits(want_sc))
    assert (ids[5] >= 0).sum() == min(5, n_top)
    if with_lse:
        lse, EL = sr.lse_bounds(A, B, b, S, ep, ei, T, dtype)
        assert np.all(np.abs(out[3] - lse) <= EL), float((np.abs(out[3] - lse) / EL).max())


@gpu
@pytest.mark.parametrize("dtype,k", [(np.float64, 65), (np.float32, 64)])
def test_zero_temperature_and_seeds(monkeypatch, dtype, k):
    from cmfrec_amd import Ranker
    A, B, b, ep, ei, S, T = problem(dtype, k)
    with Ranker(B, b) as r:
        a1 = r.topN_sample(A, 10, T, 1, exclude=(ep, ei), with_lse=True)
        a2 = r.topN_sample(A, 10, T, 1, exclude=(ep, ei), with_lse=True)
        b1 = r.topN_sample(A, 10, T, 2, exclude=(ep, ei))
        z = r.topN_sample(A, 10, 0.0, 1, exclude=(ep, ei), with_lse=True)
        monkeypatch.setenv("CMFREC_HIP_TOPN", "wide")
        want = r.topN(A, n=10, exclude=(ep, ei))
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a1, a2))
    assert (a1[0] != b1[0]).mean() > 0.5
    assert np.array_equal(z[0], want[0]) and np.array_equal(bits(z[1]), bits(want[1])) and np.array_equal(bits(z[2]), bits(want[1]))
    assert np.all(np.isnan(z[3]))


@gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_log_partition(dtype):
    """Plain users, user 5 with five items left, user 7 with one score 200 T above the rest, user 9 with nothing left."""
    from cmfrec_amd import Ranker
    k, n = 64, 1000
    A, B, b, ep, ei, S, T = problem(dtype, k)
    A[7] = (600 * T / float(B[42].astype(np.float64) @ B[42])) * B[42]
    lists = [sr.excluded(ep, ei, u) for u in range(len(A))]
    lists[7] = np.zeros(0, np.int32)
    lists[9] = np.arange(n, dtype=np.int32)
    ep = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64); ei = np.concatenate(lists).astype(np.int32)
    S = tr.scores64(A, B, b)
    assert S[7, 42] - np.delete(S[7], 42).max() >= 200 * T
    with Ranker(B, b) as r:
        ids, _, _, got = r.topN_sample(A, 10, T, SEED, exclude=(ep, ei), with_lse=True)
    lse, EL = sr.lse_bounds(A, B, b, S, ep, ei, T, dtype)
    assert np.isneginf(got[9]) and np.all(ids[9] == -1) and np.isfinite(got[7]) and ids[7, 0] == 42
    fin = np.isfinite(lse)
    assert fin.sum() == len(A) - 1
    ratio = np.abs(got[fin] - lse[fin]) / EL[fin]
    print("lse check: %s largest error / bound %.3f (bound %.2e .. %.2e)" % (np.dtype(dtype).name, ratio.max(), EL[fin].min(), EL[fin].max()))
    assert np.all(ratio <= 1)


@gpu
@pytest.mark.parametrize("dtype,k,n_top", [(np.float64, 65, 10), (np.float32, 272, 10)])
def test_noise_decides(dtype, k, n_top):
    """T ten times the scores' spread: nearly every position is the noise's, and the bound admits far more pairs."""
    from cmfrec_amd import Ranker
    A, B, b, ep, ei, S, T = problem(dtype, k, t_scale=10.0)
    with Ranker(B, b) as r:
        ids, sc, keys = r.topN_sample(A, n_top, T, SEED, exclude=(ep, ei))
    _, share = sr.check_keys(*sr.keys_and_bounds(A, B, b, S, T, SEED, dtype), ep, ei, n_top, ids, keys)
    assert share == 0 if dtype == np.float64 else share <= 0.10, share
    assert (ids[:, 0] != np.argmax(S, axis=1)).mean() > 0.5


@gpu
def test_refusals_leave_outputs_untouched():
    from cmfrec_amd import Ranker, _lib, ops
    rng = np.random.default_rng(0)
    A, B = rng.standard_normal((4, 20)), rng.standard_normal((30, 20))
    ids = np.full((4, 5), 77, np.int32); sc = np.full((4, 5), 7.0); keys = np.full((4, 5), 7.0); lse = np.full(4, 7.0)
    with Ranker(B) as r:
        def call(n_top, t, out_lse=lse, with_lse=1):
            return r.lib.cmfrec_hip_ranker_topN_sample(r.handle, _lib.ptr(A), C.c_size_t(20), 4, None, None, n_top, C.c_double(t), C.c_uint64(1),
                                                       with_lse, _lib.ptr(ids), _lib.ptr(sc), _lib.ptr(keys), _lib.ptr(out_lse))
        for n_top, t, ol in ((5, -1.0, lse), (5, np.nan, lse), (5, np.inf, lse), (0, 1.0, lse), (31, 1.0, lse), (129, 1.0, lse), (5, 1.0, None)):
            assert call(n_top, t, ol) == 2, (n_top, t)
        assert (ids == 77).all() and (sc == 7.0).all() and (keys == 7.0).all() and (lse == 7.0).all()
        for kw in (dict(temperature=-1.0), dict(temperature=np.nan), dict(n=0), dict(n=31), dict(seed=-1), dict(seed=1.5)):
            with pytest.raises(ValueError):
                r.topN_sample(A, **{"n": 5, "temperature": 1.0, "seed": 1, **kw})
        again = r.topN_sample(A, 5, 1.0, 3, with_lse=True)
    with pytest.raises(ValueError):
        ops.topN_sample_batch(A, B, n_top=5, temperature=np.inf)
    out = ops.topN_sample_batch(A, B, n_top=5, temperature=1.0, seed=3, with_lse=True)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(out, again))
