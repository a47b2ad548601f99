"""GPU: the ranking handle (cmfrec_amd.Ranker over cmfrec_hip_ranker_*) -- one upload of the item factors, many calls -- and
the models' topN_batch / ranker() on models wider than 64 factors."""
import numpy as np
import pytest

import topn_reference as tr
from conftest import make_coo

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype,k", [(np.float64, 128), (np.float32, 257), (np.float64, 50)], ids=lambda v: getattr(v, "__name__", str(v)))
def test_one_handle_many_calls(dtype, k):
    """Several calls on one handle with different users, n_top and exclusion lists (buffers grow and shrink): each result is
    bit-identical to the one-shot ops.topN_batch on the same inputs."""
    from cmfrec_amd import Ranker, ops
    n = 3000
    A, B, b, ep, ei = tr.make_problem(21 + k, dtype, 200, n, k)
    with Ranker(B, b) as rk:
        with pytest.raises(RuntimeError):
            rk.kernel_ms()                                  # nothing ranked yet
        for lo, hi, n_top, with_excl in ((0, 33, 10, True), (33, 200, 100, True), (5, 6, 1, False), (0, 200, 128, True), (100, 170, 10, False)):
            excl = None
            if with_excl:
                e0, e1 = int(ep[lo]), int(ep[hi])
                excl = ((ep[lo:hi + 1] - ep[lo]).astype(np.uint64), ei[e0:e1])
            ids, sc = rk.topN(A[lo:hi], n=n_top, exclude=excl)
            ids1, sc1 = ops.topN_batch(A[lo:hi], B, n_top=n_top, biasB=b, exclude=excl)
            assert np.array_equal(ids, ids1) and np.array_equal(sc, sc1), (lo, hi, n_top)
            assert rk.kernel_ms() > 0
        with pytest.raises(ValueError):
            rk.topN(A[:4].astype(np.float32 if dtype is np.float64 else np.float64))
        with pytest.raises(ValueError):
            rk.topN(A[:4, :-1])
        with pytest.raises(RuntimeError, match=r"code 2.*n_top <= min\(128, n\)"):
            rk.topN(A[:4], n=129)
    with Ranker(B) as rk:                                    # no bias
        ids, sc = rk.topN(A[:40], n=10)
        ids1, sc1 = ops.topN_batch(A[:40], B, n_top=10)
        assert np.array_equal(ids, ids1) and np.array_equal(sc, sc1)


def test_closed_handle_refuses():
    from cmfrec_amd import Ranker
    rng = np.random.default_rng(3)
    B = rng.standard_normal((500, 80)); A = rng.standard_normal((7, 80))
    rk = Ranker(B)
    rk.topN(A, n=5)
    rk.close()
    rk.close()                                               # idempotent
    with pytest.raises(RuntimeError, match="closed"):
        rk.topN(A, n=5)
    with pytest.raises(RuntimeError, match="closed"):
        rk.kernel_ms()


def _csr_of(row, col, m):
    o = np.lexsort((col, row))
    ip = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=m))]).astype(np.int64)
    return ip, col[o].astype(np.int32)


@pytest.mark.parametrize("use_float", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("model", ["CMF", "CMF_implicit"])
def test_models_rank_wide(model, use_float):
    """CMF(k=72) / CMF_implicit(k=80): topN_batch works beyond 64 factors, equals ranker().topN, and agrees with the float64
    ranking of the fitted factors."""
    from cmfrec_amd import CMF, CMF_implicit
    dt = np.float32 if use_float else np.float64
    m, n = 400, 600
    if model == "CMF":
        row, col, val = make_coo(m, n, 20000, 4, counts=False, dtype=dt)
        mdl = CMF(k=72, lambda_=0.5, niter=2, use_cg=True, finalize_chol=False, use_float=use_float, random_state=9, nthreads=1,
                  precompute_for_predictions=False).fit((row, col, val), shape=(m, n))
        bias = np.asarray(mdl.item_bias_, dt)
    else:
        row, col, val = make_coo(m, n, 20000, 3, dtype=dt)
        mdl = CMF_implicit(k=80, lambda_=3.0, niter=2, use_cg=True, finalize_chol=False, use_float=use_float, random_state=7).fit(
            (row, col, val), shape=(m, n))
        bias = None
    assert mdl.A_.dtype == dt
    users = np.array([0, 5, 17, 399, 250, 3] + list(range(100, 160)))
    train = _csr_of(row, col, m)
    for n_top, excl in ((10, train), (100, None)):
        ids, sc = mdl.topN_batch(users, n=n_top, exclude=excl)
        with mdl.ranker() as rk:
            ids_r, sc_r = rk.topN(users, n=n_top, exclude=excl)
            ids_r2, _ = rk.topN(users[:7], n=n_top, exclude=excl)
        assert np.array_equal(ids, ids_r) and np.array_equal(sc, sc_r)
        assert np.array_equal(ids_r2, ids[:7])
        A = np.ascontiguousarray(mdl.A_[users][:, mdl.k_user:]); B = np.ascontiguousarray(mdl.B_[:, mdl.k_item:])
        ep = ei = None
        if excl is not None:
            lens = excl[0][users + 1] - excl[0][users]
            ep = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
            ei = np.concatenate([excl[1][excl[0][u]:excl[0][u + 1]] for u in users]).astype(np.int32)
        if model == "CMF":                                   # the model adds glob_mean + the user's bias to the scores afterwards:
            # the conditions hold for the device's own scores, taken through a plain Ranker over the same factors
            from cmfrec_amd import Ranker
            with Ranker(B, bias) as plain:
                ids_p, sc_p = plain.topN(A, n=n_top, exclude=None if ep is None else (ep, ei))
            assert np.array_equal(ids_p, ids)
            tr.check_ranking(A, B, bias, ep, ei, ids_p, sc_p, n_top, dt)
        else:
            tr.check_ranking(A, B, bias, ep, ei, ids, sc, n_top, dt)
