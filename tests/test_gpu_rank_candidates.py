"""GPU: top-N over per-user candidate lists (topn_cand_kernels.hpp; ``include=`` of Ranker.topN, ops.topN_batch, the models and
NewUsers.topN; cmfrec_hip_ranker_topN_candidates and its kin) against two oracles.

1. The float64 ranking of topn_reference.check_ranking with each user's exclusion list set to the complement of its candidate
   list: the semantics are "the full ranking with everything else excluded".
2. An exact one: ``Scorer(A, B, biasB=b, glob_mean=0.0).predict`` on the flattened (user, candidate) pairs, then
   ``cand[np.lexsort((cand, -s))][:n_top]`` per user.  The candidate kernel states the scorer's products, order and butterfly, so
   ids and scores must be equal under np.array_equal, every position.

The undecided share of check_ranking is a property of the float64 reference alone (of the generator, the shapes and the dtype's
rounding bound; the device's result does not enter it).  For single precision it is capped at 0.10; on this generator (n = 1500,
48 users, 300 candidates, seed 5) the reference leaves at most 6.3 % (k = 272, n_top = 128) and none in double precision.  Every
case prints its share."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import topn_reference as tr
from conftest import make_coo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, NU, NC, SEED = 1500, 48, 300, 5


def csr_of_lists(lists):
    cp = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    ci = np.concatenate([np.asarray(x, np.int64) for x in lists] + [np.zeros(0, np.int64)]).astype(np.int32)
    return cp, ci


def lists_of_csr(p, i):
    return [i[int(p[u]):int(p[u + 1])] for u in range(len(p) - 1)]


def random_lists(seed, nu, n, length):
    """Sorted lists of `length` random items (an int, or one length per user); user 0's is empty, user 1's holds the planted
    exact ties 3, 7 and 11 where it is long enough."""
    rng = np.random.default_rng(seed)
    lens = np.full(nu, length) if np.ndim(length) == 0 else np.asarray(length)
    lists = []
    for u in range(nu):
        x = rng.choice(n, int(lens[u]), replace=False)
        if u == 1 and len(x) >= 3:
            x = np.concatenate([[3, 7, 11], np.setdiff1d(x, [3, 7, 11])[:len(x) - 3]])
        lists.append(np.sort(x))
    if np.ndim(length) == 0:
        lists[0] = np.zeros(0, np.int64)
    return csr_of_lists(lists)


def complement(cp, ci, n, excl=None):
    """The exclusion CSR that turns the full ranking into the ranking over the lists: everything outside a user's list, united
    with the user's own exclusion list."""
    out = []
    for u, cand in enumerate(lists_of_csr(cp, ci)):
        x = np.setdiff1d(np.arange(n), cand)
        if excl is not None:
            x = np.union1d(x, excl[1][int(excl[0][u]):int(excl[0][u + 1])])
        out.append(x)
    return csr_of_lists(out)


def pair_scores(A, B, b, cp, ci):
    """The scorer's value of every (user, candidate) pair, flattened in list order."""
    from cmfrec_amd import Scorer
    row = np.repeat(np.arange(len(cp) - 1), np.diff(cp.astype(np.int64))).astype(np.int32)
    with Scorer(A, B, biasB=b, glob_mean=0.0) as s:
        return s.predict(row, ci)


def exact(cp, ci, s, n, n_top, dtype, excl=None):
    ids = np.full((len(cp) - 1, n_top), -1, np.int32); sc = np.full((len(cp) - 1, n_top), -np.inf, dtype)
    for u in range(len(cp) - 1):
        lo, hi = int(cp[u]), int(cp[u + 1])
        cand, su = ci[lo:hi], s[lo:hi]
        keep = (cand >= 0) & (cand < n) & ~np.isnan(su)
        if excl is not None:
            keep &= ~np.isin(cand, excl[1][int(excl[0][u]):int(excl[0][u + 1])])
        cand, su = cand[keep], su[keep]
        o = np.lexsort((cand, -su))[:n_top]
        ids[u, :len(o)] = cand[o]; sc[u, :len(o)] = su[o]
    return ids, sc


def assert_exact(ids, sc, want):
    assert np.array_equal(ids, want[0]), np.argwhere(ids != want[0])[:5]
    assert np.array_equal(sc, want[1]), np.argwhere(sc != want[1])[:5]


_problems = {}


def problem(dtype, k):
    """Shared by the n_top cases of one (dtype, k), never modified: factors, lists, the complement CSR and the scorer's values."""
    key = (np.dtype(dtype).name, k)
    if key not in _problems:
        A, B, b, _, _ = tr.make_problem(SEED, dtype, NU, N, k, excl=False)
        cp, ci = random_lists(SEED + 1000, NU, N, NC)
        _problems[key] = (A, B, b, cp, ci, complement(cp, ci, N), pair_scores(A, B, b, cp, ci))
    return _problems[key]


KS = [(np.float64, k) for k in (1, 3, 50, 64, 65, 129, 256)] + [(np.float32, k) for k in (1, 3, 50, 64, 65, 129, 256, 272)]


@pytest.mark.parametrize("n_top", [1, 10, 33, 128])
@pytest.mark.parametrize("dtype,k", KS, ids=lambda v: getattr(v, "__name__", str(v)))
def test_against_both_oracles(dtype, k, n_top):
    """Every group width G = 1 .. 64 (k = 1, 3: one and two lanes; 50 ... 129: up to the whole wavefront; 256 / 272: two rounds),
    rows whose last piece is partial, list shorter (user 0: empty) and longer than n_top."""
    from cmfrec_amd import ops
    A, B, b, cp, ci, (xp, xi), s = problem(dtype, k)
    assert cp[1] == 0 and {3, 7, 11} <= set(ci[int(cp[1]):int(cp[2])].tolist())
    ids, sc = ops.topN_batch(A, B, n_top=n_top, biasB=b, include=(cp, ci))
    _, share = tr.check_ranking(A, B, b, xp, xi, ids, sc, n_top, dtype, all_decided=dtype is np.float64)
    print("candidate ranking: the float64 reference leaves %.4f of the positions undecided" % share)
    if dtype is np.float32:
        assert share <= 0.10
    assert np.all(ids[0] == -1) and np.all(np.isneginf(sc[0]))
    assert_exact(ids, sc, exact(cp, ci, s, N, n_top, dtype))


@pytest.mark.parametrize("n_top", [10, 33])
def test_list_lengths(n_top):
    """k = 8 in double precision: 4 lanes per candidate, 16 candidates per step, 64 per round of steps, 128 candidate slots.
    Lists of 0, 1, n_top - 1, n_top, n_top + 1, 63, 64, 65, 127, 128, 129 and all n items."""
    from cmfrec_amd import ops
    lens = [0, 1, n_top - 1, n_top, n_top + 1, 63, 64, 65, 127, 128, 129, N]
    A, B, b, _, _ = tr.make_problem(SEED + 1, np.float64, len(lens), N, 8, excl=False)
    cp, ci = random_lists(SEED + 2, len(lens), N, lens)
    ids, sc = ops.topN_batch(A, B, n_top=n_top, biasB=b, include=(cp, ci))
    assert_exact(ids, sc, exact(cp, ci, pair_scores(A, B, b, cp, ci), N, n_top, np.float64))
    xp, xi = complement(cp, ci, N)
    tr.check_ranking(A, B, b, xp, xi, ids, sc, n_top, np.float64, all_decided=True)
    for u, l in enumerate(lens):
        assert (ids[u] >= 0).sum() == min(l, n_top)


def test_every_candidate_beats_the_threshold():
    """A list whose scores ascend along the list: every candidate enters and the merge runs as often as it can.  Built by
    renumbering B's rows so that user 0's scores ascend with the item id; user 1's list descends the same way."""
    from cmfrec_amd import ops
    n_top = 10
    A, B, b, _, _ = tr.make_problem(SEED + 3, np.float64, 2, N, 8, excl=False)
    A[1] = -A[0]; b[:] = 0
    B[7] += 1; B[11] -= 1                                     # no exact ties here: the expected order below is by score alone
    cand = np.sort(np.random.default_rng(3).choice(N, 700, replace=False))
    cp, ci = csr_of_lists([cand, cand])
    s0 = pair_scores(A, B, b, cp, ci)[:700]
    order = np.argsort(s0, kind="stable")
    B2 = B.copy(); B2[cand] = B[cand[order]]
    s = pair_scores(A, B2, b, cp, ci)
    assert np.all(np.diff(s[:700]) >= 0) and np.all(np.diff(s[700:]) <= 0)
    ids, sc = ops.topN_batch(A, B2, n_top=n_top, biasB=b, include=(cp, ci))
    assert_exact(ids, sc, exact(cp, ci, s, N, n_top, np.float64))
    assert np.array_equal(ids[0], cand[::-1][:n_top])


def test_nan_rows_and_ids_out_of_range_never_enter():
    from cmfrec_amd import _lib, ops
    n_top = 10
    A, B, b, _, _ = tr.make_problem(SEED + 4, np.float64, 6, N, 8, excl=False)
    cp, ci = random_lists(SEED + 5, 6, N, 40)
    bad = ci[[int(cp[1]) + 5, int(cp[2]), int(cp[3]) - 1]]
    B[bad] = np.nan
    s = pair_scores(A, B, b, cp, ci)
    assert np.isnan(s).any()
    ids, sc = ops.topN_batch(A, B, n_top=n_top, biasB=b, include=(cp, ci))
    assert_exact(ids, sc, exact(cp, ci, s, N, n_top, np.float64))
    assert not np.isnan(sc).any() and not set(ids[1].tolist()) & set(bad.tolist())
    # a list of NaN rows only: nothing is returned
    cp1, ci1 = csr_of_lists([np.sort(bad)] * 6)
    ids1, sc1 = ops.topN_batch(A, B, n_top=n_top, biasB=b, include=(cp1, ci1))
    assert np.all(ids1 == -1) and np.all(np.isneginf(sc1))
    # ids -1 and n inside a C-level list (the Python layer maps what does not fit int32 to -1; n stays n): skipped on the device
    lists = [np.concatenate([[-1], x, [N]]) for x in lists_of_csr(cp, ci)]
    lists[0] = np.array([-1, N]); lists[4] = np.array([-1]); lists[5] = np.array([N, N + 7])
    cp2, ci2 = csr_of_lists(lists)
    lib = _lib.load(np.float64)
    ids2 = np.full((6, n_top), 77, np.int32); sc2 = np.zeros((6, n_top))
    rc = lib.cmfrec_hip_topN_candidates_batch(_lib.ptr(A), C.c_size_t(8), C.c_int(6), _lib.ptr(B), C.c_size_t(8), C.c_int(N), C.c_int(8),
                                              _lib.ptr(b), _lib.ptr(cp2), _lib.ptr(ci2), None, None, C.c_int(n_top), _lib.ptr(ids2),
                                              _lib.ptr(sc2))
    assert rc == 0, lib.cmfrec_hip_last_error()
    assert_exact(ids2, sc2, exact(cp2, ci2, pair_scores(A, B, b, cp2, ci2), N, n_top, np.float64))
    assert np.array_equal(ids2[1:4], ids[1:4]) and np.all(ids2[[0, 4, 5]] == -1)


@pytest.mark.parametrize("dtype,k", [(np.float64, 50), (np.float32, 129)], ids=lambda v: getattr(v, "__name__", str(v)))
def test_all_items_equals_the_plain_ranking(dtype, k):
    """A list of all n items: the ids of Ranker.topN without ``include``.  The two kernels sum in different orders, so
    check_ranking is the judge: in double precision nothing is undecided and the ids are equal."""
    from cmfrec_amd import Ranker
    A, B, b, ep, ei = tr.make_problem(SEED + 6, dtype, 20, N, k)
    with Ranker(B, b) as rk:
        for n_top, excl in ((10, None), (128, (ep, ei))):
            ids, sc = rk.topN(A, n=n_top, exclude=excl, include=np.arange(N))
            assert rk.launch_shape()[0] == 4
            ids_p, sc_p = rk.topN(A, n=n_top, exclude=excl)
            pe, pi = excl if excl is not None else (None, None)
            tr.check_ranking(A, B, b, pe, pi, ids, sc, n_top, dtype, all_decided=dtype is np.float64)
            tr.check_ranking(A, B, b, pe, pi, ids_p, sc_p, n_top, dtype, all_decided=dtype is np.float64)
            if dtype is np.float64:
                assert np.array_equal(ids, ids_p)


@pytest.mark.parametrize("dtype,k,n_top", [(np.float64, 50, 10), (np.float32, 129, 128), (np.float64, 3, 33)],
                         ids=lambda v: getattr(v, "__name__", str(v)))
def test_candidates_and_exclusions(dtype, k, n_top):
    """Half of each candidate list is also in the user's exclusion list, together with items outside the list."""
    from cmfrec_amd import ops
    A, B, b, cp, ci, _, s = problem(dtype, k)
    rng = np.random.default_rng(17)
    excl = csr_of_lists([np.union1d(x[::2], rng.choice(N, 50, replace=False)) for x in lists_of_csr(cp, ci)])
    ids, sc = ops.topN_batch(A, B, n_top=n_top, biasB=b, exclude=excl, include=(cp, ci))
    xp, xi = complement(cp, ci, N, excl)
    _, share = tr.check_ranking(A, B, b, xp, xi, ids, sc, n_top, dtype, all_decided=dtype is np.float64)
    print("candidate ranking with exclusions: the float64 reference leaves %.4f of the positions undecided" % share)
    if dtype is np.float32:
        assert share <= 0.10
    assert_exact(ids, sc, exact(cp, ci, s, N, n_top, dtype, excl))
    for u, x in enumerate(lists_of_csr(*excl)):
        assert not set(ids[u].tolist()) & set(x.tolist())


CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import test_gpu_rank_candidates as t
from cmfrec_amd import Ranker
out = {}
for tag, dtype, k in t.MANY:
    A, B, b, cp, ci = t.many_users(dtype, k)
    with Ranker(B, b) as rk:
        ids, sc = rk.topN(A, n=10, include=(cp, ci))
        out["ids_" + tag] = ids; out["sc_" + tag] = sc; out["shape_" + tag] = np.array(rk.launch_shape())
np.savez(sys.argv[1], **out)
"""
MANY = [("f64_50", np.float64, 50), ("f32_272", np.float32, 272)]


def many_users(dtype, k):
    A, B, b, _, _ = tr.make_problem(SEED + 7, dtype, 300, N, k, excl=False)
    cp, ci = random_lists(SEED + 8, 300, N, np.tile([700, 0, 5, 129], 75))
    return A, B, b, cp, ci


def test_many_users_per_wavefront(tmp_path, monkeypatch):
    """300 users with lists of 700, 0, 5, 129, ... items: with CMFREC_HIP_TOPN_CAND_WAVES=4 (a child process) one workgroup's
    four wavefronts rank them all one after the other; by default every user has a wavefront of its own.  Equal bit for bit, equal
    to the exact oracle, and a user's row does not depend on where it stands in the batch."""
    from cmfrec_amd import Ranker
    monkeypatch.delenv("CMFREC_HIP_TOPN_CAND_WAVES", raising=False)
    path = str(tmp_path / "few.npz")
    e = dict(os.environ, CMFREC_HIP_TOPN_CAND_WAVES="4")
    code = CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code, path], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    few = np.load(path)
    for tag, dtype, k in MANY:
        A, B, b, cp, ci = many_users(dtype, k)
        want = exact(cp, ci, pair_scores(A, B, b, cp, ci), N, 10, dtype)
        with Ranker(B, b) as rk:
            ids, sc = rk.topN(A, n=10, include=(cp, ci))
            shape = rk.launch_shape()
            perm = np.random.default_rng(1).permutation(300)
            lists = lists_of_csr(cp, ci)
            ids_s, sc_s = rk.topN(A[perm], n=10, include=csr_of_lists([lists[u] for u in perm]))
        assert tuple(few["shape_" + tag]) == (4, 1) and shape == (4, 75)
        assert_exact(ids, sc, want)
        assert_exact(few["ids_" + tag], few["sc_" + tag], want)
        assert_exact(ids_s, sc_s, (want[0][perm], want[1][perm]))


@pytest.mark.parametrize("dtype,k", [(np.float64, 128), (np.float32, 257), (np.float64, 50)], ids=lambda v: getattr(v, "__name__", str(v)))
def test_one_handle_many_calls(dtype, k):
    """Candidate calls and plain calls interleaved on one Ranker, batches growing and shrinking: each result equals the one-shot
    ops.topN_batch on the same inputs."""
    from cmfrec_amd import Ranker, ops
    A, B, b, ep, ei = tr.make_problem(21 + k, dtype, 200, N, k)
    cp, ci = random_lists(22 + k, 200, N, np.random.default_rng(k).integers(0, 400, 200))
    with Ranker(B, b) as rk:
        for lo, hi, n_top, with_excl, with_cand in ((0, 33, 10, True, True), (33, 200, 100, True, False), (5, 6, 1, False, True),
                                                    (0, 200, 128, True, True), (100, 170, 10, False, False), (100, 170, 10, False, True)):
            excl = inc = None
            if with_excl:
                excl = ((ep[lo:hi + 1] - ep[lo]).astype(np.uint64), ei[int(ep[lo]):int(ep[hi])])
            if with_cand:
                inc = ((cp[lo:hi + 1] - cp[lo]).astype(np.uint64), ci[int(cp[lo]):int(cp[hi])])
            ids, sc = rk.topN(A[lo:hi], n=n_top, exclude=excl, include=inc)
            ids1, sc1 = ops.topN_batch(A[lo:hi], B, n_top=n_top, biasB=b, exclude=excl, include=inc)
            assert np.array_equal(ids, ids1) and np.array_equal(sc, sc1), (lo, hi, n_top)
            assert rk.kernel_ms() > 0
        with pytest.raises(RuntimeError, match=r"code 2.*n_top <= min\(128, n\)"):
            rk.topN(A[:4], n=129, include=np.arange(300))
        ids, sc = rk.topN(A[:4], n=5, include=np.array([11, 7, 3, 7]))        # a shared list, unsorted with a duplicate
        assert np.all(ids[:, 3:] == -1)
        assert all(sorted(r[:3].tolist()) == [3, 7, 11] for r in ids)
        assert np.array_equal(ids[0, :3], [3, 7, 11])                        # the planted exact ties: the lower id first


_fitted = {}


def _fit(model, use_float):
    """The two small models of test_gpu_ranker.py, fitted once per precision."""
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
    _fitted[(model, use_float)] = mdl
    return mdl


@pytest.mark.parametrize("use_float", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("model", ["CMF", "CMF_implicit"])
def test_models(model, use_float):
    """topN_batch(users, n, include=) equals ranker().topN(users, n, include=) and the exact oracle + glob_mean + the user bias;
    NewUsers.topN(exclude_seen=True, include=) equals the exact oracle on the factors it returns, without a row's own items."""
    dt = np.float32 if use_float else np.float64
    mdl = _fit(model, use_float)
    n = mdl.B_.shape[0]
    bias = np.asarray(mdl.item_bias_, dt) if model == "CMF" else None
    B = np.ascontiguousarray(mdl.B_[:, mdl.k_item:])
    users = np.array([0, 5, 17, 399, 250, 3] + list(range(100, 160)))
    inc = random_lists(31, len(users), n, 100)
    excl_all = random_lists(32, 400, n, np.random.default_rng(2).integers(0, 60, 400))    # over ALL users, as exclude is given
    for n_top, excl in ((10, None), (100, excl_all)):
        ids, sc = mdl.topN_batch(users, n=n_top, exclude=excl, include=inc)
        with mdl.ranker() as rk:
            ids_r, sc_r = rk.topN(users, n=n_top, exclude=excl, include=inc)
        assert np.array_equal(ids, ids_r) and np.array_equal(sc, sc_r)
        A = np.ascontiguousarray(mdl.A_[users][:, mdl.k_user:])
        ex = None if excl is None else csr_of_lists([lists_of_csr(*excl)[u] for u in users])
        want_ids, want_sc = exact(inc[0], inc[1], pair_scores(A, B, bias, *inc), n, n_top, dt, ex)
        assert_exact(ids, sc, (want_ids, mdl._finish_scores(users, want_sc)))
    # new users: 30 rows of 1 .. 40 entries, candidates that overlap them
    rng = np.random.default_rng(41)
    rows = 30
    lens = rng.integers(1, 40, rows)
    r = np.repeat(np.arange(rows), lens).astype(np.int32)
    c = np.concatenate([rng.choice(n, l, replace=False) for l in lens]).astype(np.int32)
    v = (0.5 * rng.integers(1, 11, len(r)) if model == "CMF" else np.ceil(rng.lognormal(1, 1, len(r)))).astype(dt)
    seen = csr_of_lists([np.sort(c[r == u]) for u in range(rows)])
    inc = csr_of_lists([np.union1d(rng.choice(n, 80, replace=False), c[r == u][::2]) for u in range(rows)])
    n_top = 10
    with mdl.new_users() as nu:
        ids, sc, (A, ub) = nu.topN(X=(r, c, v), n=n_top, exclude_seen=True, include=inc, return_factors=True)
        s_ms, r_ms = nu.kernel_ms()
        assert s_ms > 0 and r_ms > 0
        ids_p, _ = nu.topN(X=(r, c, v), n=n_top, exclude_seen=True)           # the plain call on the same handle, afterwards
    Au = np.ascontiguousarray(A[:, mdl.k_user:])
    want_ids, want_sc = exact(inc[0], inc[1], pair_scores(Au, B, bias, *inc), n, n_top, dt, seen)
    if model == "CMF":
        want_sc = want_sc + mdl.glob_mean_
        if ub is not None:
            want_sc = want_sc + ub[:, None]
    assert_exact(ids, sc, (want_ids, want_sc))
    for u in range(rows):
        assert not set(ids[u].tolist()) & set(c[r == u].tolist()), u
        assert not set(ids_p[u].tolist()) & set(c[r == u].tolist()), u
    ids_o, sc_o = mdl.topN_new_batch(X=(r, c, v), n=n_top, exclude_seen=True, include=inc)
    assert np.array_equal(ids_o, ids) and np.array_equal(sc_o, sc)


def test_c_caller():
    """cmfrec_hip_topN_candidates_batch and cmfrec_hip_newrows_topN_candidates through ctypes; a batch the handle refuses leaves
    out_ids as they were and the handle usable."""
    from cmfrec_amd import _lib
    dt = np.float64
    lib = _lib.load(dt)
    n_top = 10
    A, B, b, cp, ci, _, s = problem(dt, 50)
    ids = np.full((NU, n_top), 77, np.int32); sc = np.zeros((NU, n_top))
    rc = lib.cmfrec_hip_topN_candidates_batch(_lib.ptr(A), C.c_size_t(50), C.c_int(NU), _lib.ptr(B), C.c_size_t(50), C.c_int(N), C.c_int(50),
                                              _lib.ptr(b), _lib.ptr(cp), _lib.ptr(ci), None, None, C.c_int(n_top), _lib.ptr(ids), _lib.ptr(sc))
    assert rc == 0, lib.cmfrec_hip_last_error()
    assert_exact(ids, sc, exact(cp, ci, s, N, n_top, dt))
    ids_only = np.full((NU, n_top), 77, np.int32)                                # out_scores is optional
    rc = lib.cmfrec_hip_topN_candidates_batch(_lib.ptr(A), C.c_size_t(50), C.c_int(NU), _lib.ptr(B), C.c_size_t(50), C.c_int(N), C.c_int(50),
                                              _lib.ptr(b), _lib.ptr(cp), _lib.ptr(ci), None, None, C.c_int(n_top), _lib.ptr(ids_only), None)
    assert rc == 0 and np.array_equal(ids_only, ids)
    bad_p = cp.copy(); bad_p[3] = bad_p[5] + 1                                   # offsets that decrease: refused, nothing written
    ids_only[:] = 77
    rc = lib.cmfrec_hip_topN_candidates_batch(_lib.ptr(A), C.c_size_t(50), C.c_int(NU), _lib.ptr(B), C.c_size_t(50), C.c_int(N), C.c_int(50),
                                              _lib.ptr(b), _lib.ptr(bad_p), _lib.ptr(ci), None, None, C.c_int(n_top), _lib.ptr(ids_only), None)
    assert rc == 2 and np.all(ids_only == 77)

    mdl = _fit("CMF_implicit", False)
    n = mdl.B_.shape[0]
    Bm = np.ascontiguousarray(mdl.B_[:, mdl.k_item:])
    rng = np.random.default_rng(43)
    rows = 12
    lens = rng.integers(1, 30, rows)
    r = np.repeat(np.arange(rows), lens).astype(np.int32)
    c = np.concatenate([rng.choice(n, l, replace=False) for l in lens]).astype(np.int32)
    v = np.ceil(rng.lognormal(1, 1, len(r)))
    inc = csr_of_lists([np.union1d(rng.choice(n, 60, replace=False), c[r == u][:3]) for u in range(rows)])
    seen = csr_of_lists([np.sort(c[r == u]) for u in range(rows)])
    with mdl.new_users() as nu:
        st, keep, got_rows = nu._batch((r, c, v), None, None)
        assert got_rows == rows
        fn = nu.lib.cmfrec_hip_newrows_topN_candidates
        ids = np.full((rows, n_top), 77, np.int32); sc = np.zeros((rows, n_top)); Af = np.empty((rows, nu.width))
        refused = _lib.NewRowsBatch.from_buffer_copy(st)
        refused.Xfull = Af.ctypes.data                                           # X both dense and sparse: what factors refuses
        rc = fn(nu.handle, C.byref(refused), _lib.ptr(inc[0]), _lib.ptr(inc[1]), 1, None, None, n_top, _lib.ptr(ids), _lib.ptr(sc),
                None, None)
        assert rc != 0 and np.all(ids == 77)
        msg = nu.lib.cmfrec_hip_last_error()
        rc1 = nu.lib.cmfrec_hip_newrows_topN(nu.handle, C.byref(refused), 1, None, None, n_top, _lib.ptr(ids), _lib.ptr(sc), None, None)
        assert rc1 == rc and nu.lib.cmfrec_hip_last_error() == msg and np.all(ids == 77)
        rc = fn(nu.handle, C.byref(st), None, None, 1, None, None, n_top, _lib.ptr(ids), _lib.ptr(sc), None, None)
        assert rc == 2 and np.all(ids == 77)                                     # cand_p == NULL
        rc = fn(nu.handle, C.byref(st), _lib.ptr(inc[0]), _lib.ptr(inc[1]), 1, None, None, n_top, _lib.ptr(ids), _lib.ptr(sc),
                _lib.ptr(Af), None)
        assert rc == 0, nu.lib.cmfrec_hip_last_error()
        s_ms, r_ms = nu.kernel_ms()
        assert s_ms > 0 and r_ms > 0
    Au = np.ascontiguousarray(Af[:, mdl.k_user:])
    assert_exact(ids, sc, exact(inc[0], inc[1], pair_scores(Au, Bm, None, *inc), n, n_top, dt, seen))
