"""fit(..., validation=Validation(...)): the held-out set evaluated on the device between the iterations of the fit
(cmfrec_hip_fit_set_monitor), early stopping, and the best iterate as the fitted model.

(a) monitor only changes nothing of the fit; (b) each record is the record of that iteration's factors; (c) early stopping on a
problem that overfits; (d) the implicit model stopped early on NDCG@10, and watched by RMSE / MAE; (e) the refusals."""
import ctypes as C

import numpy as np
import pytest

import errors_reference as er
from conftest import make_coo

pytestmark = pytest.mark.gpu

EPS = {np.float64: float(np.finfo(np.float64).eps), np.float32: float(np.finfo(np.float32).eps)}


def frob(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def stored_predictions(mdl, row, col, implicit=False):
    """The predictions of a fitted model as the scoring kernel stores them (what the error record is defined on)."""
    from cmfrec_amd import ops
    m, n = mdl.A_.shape[0], mdl.B_.shape[0]
    kk = mdl.A_.shape[1]
    ub = None if implicit or not mdl.user_bias else mdl.user_bias_
    ib = None if implicit or not mdl.item_bias else mdl.item_bias_
    return ops.score_pairs(m, n, kk, np.ascontiguousarray(row, np.int32), np.ascontiguousarray(col, np.int32), A_img=mdl.A_.ravel(), lda=kk,
                           B_img=mdl.B_.ravel(), ldb=kk, biasA=ub, biasB=ib, glob_mean=0.0 if implicit else mdl.glob_mean_, implicit=implicit)


def float64_predictions(mdl, row, col, implicit=False):
    """The same pairs scored in float64 NumPy, with the sum of the absolute terms of each."""
    a, b = mdl.A_[row].astype(np.float64), mdl.B_[col].astype(np.float64)
    p = np.einsum("ij,ij->i", a, b); mag = np.einsum("ij,ij->i", np.abs(a), np.abs(b))
    if not implicit:
        for t in (np.full(len(row), np.float64(mdl.glob_mean_)), mdl.user_bias_[row].astype(np.float64), mdl.item_bias_[col].astype(np.float64)):
            p = p + t; mag = mag + np.abs(t)
    return p, mag


# ---- (a), (b): the configuration of test_gpu_fit.test_fit_explicit[cg, both biases] ---------------------------------------------

def _explicit_problem(dtype):
    m, n, k = 800, 500, 50
    row, col, val = make_coo(m, n, 30000, 22, counts=False, dtype=dtype, heavy_row=(1, 450))
    rng = np.random.default_rng(2)
    start = dict(A0=(rng.standard_normal((m, k)) * 0.01).astype(dtype), B0=np.zeros((n, k), dtype),
                 biasA0=(rng.standard_normal(m) * 0.1).astype(dtype), biasB0=(rng.standard_normal(n) * 0.1).astype(dtype))
    held = rng.random(len(val)) < 0.1
    return m, n, k, row, col, val, held, start


def _explicit_fit(dtype, niter, validation=None, finalize_chol=False):
    from cmfrec_amd import CMF
    m, n, k, row, col, val, held, start = _explicit_problem(dtype)
    tr = ~held
    return CMF(k=k, lambda_=0.05, use_float=dtype is np.float32, nthreads=1, niter=niter, use_cg=True, finalize_chol=finalize_chol,
               user_bias=True, item_bias=True, scale_lam=True).fit((row[tr], col[tr], val[tr]), shape=(m, n), validation=validation, **start)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_monitor_only_changes_nothing(dtype):
    from cmfrec_amd import Validation
    m, n, k, row, col, val, held, start = _explicit_problem(dtype)
    niter = 3
    plain = _explicit_fit(dtype, niter, finalize_chol=True)
    assert plain.n_iter_ == niter and plain.validation_history_ == [] and plain.best_iteration_ is None
    v = Validation((row[held], col[held], val[held]), patience=None, restore_best=False)
    watched = _explicit_fit(dtype, niter, validation=v, finalize_chol=True)
    t = 1e-6 if dtype is np.float64 else 1e-2           # tests/test_gpu_fit.py: tol(dtype, "cg")
    for name in ("A_", "B_", "user_bias_", "item_bias_", "_BtB", "_TransBtBinvBt", "_B_plus_bias"):
        e = frob(getattr(watched, name), getattr(plain, name))
        print("monitor only %s %s: rel. Frobenius difference %.3g" % (np.dtype(dtype).name, name, e))
        assert e < t, name
    assert watched.glob_mean_ == plain.glob_mean_
    assert watched.n_iter_ == niter
    assert [h["iteration"] for h in watched.validation_history_] == list(range(niter))
    rm = [h["rmse"] for h in watched.validation_history_]
    assert np.isfinite(rm).all() and watched.best_iteration_ == int(np.argmin(rm))
    assert all(h["n"] == int(held.sum()) and h["n_skipped"] == 0 for h in watched.validation_history_)


def check_against_float64(rec, p64, delta, x, what):
    """The record against predictions formed in float64 NumPy -- a reference that shares nothing with the device's scoring path.  The
    device's prediction p of a pair is a dot product of kk products and three more terms in the fit's precision, summed in some
    order: |p - p64| <= delta = (kk + 4) eps mag, mag the sum of the absolute terms (eps of the fit's precision; the any-order
    bound for kk + 3 additions, one more for float32's rounding of the products).  With e64 = p64 - x in np.longdouble, every pair
    scored (no fallback, no NaN) and unit weights, that moves each term of a sum by at most d -- |e - e64| <= delta, | |e| - |e64| |
    <= delta, |e^2 - e64^2| <= delta (2 |e64| + delta) -- so a sum S of n terms t obeys
        |S_got - sum t64| <= (n + 3) eps64 sum (|t64| + d) + sum d      (errors_reference's bound on the moved terms, plus the move)
    and the maximum  |max_got - max |e64|| <= max delta.  Counts are exact."""
    LD = np.longdouble
    n = len(p64)
    e = p64.astype(LD) - x.astype(np.float64).astype(LD)
    d = delta.astype(LD)
    ae = np.abs(e)
    assert int(rec["n"][0]) == n and int(rec["n"][1]) == 0 and int(rec["n_skipped"]) == 0, what
    assert float(rec["sum_w"][0]) == float(n) and float(rec["sum_w"][1]) == 0.0, what
    worst = 0.0
    for name, t, move in (("sum_we", e, d), ("sum_wabs", ae, d), ("sum_wsq", e * e, d * (2 * ae + d))):
        bound = (n + 3) * er.EPS64 * (np.abs(t) + move).sum(dtype=LD) + move.sum(dtype=LD)
        err = abs(LD(rec[name][0]) - t.sum(dtype=LD))
        assert err <= bound, "%s: %s off by %.3g, bound %.3g" % (what, name, float(err), float(bound))
        assert float(rec[name][1]) == 0.0, what
        worst = max(worst, float(err / bound))
    assert abs(LD(rec["max_abs"][0]) - ae.max()) <= d.max(), what + ": max_abs"
    return worst


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_history_records(dtype):
    """The record of iteration t - 1 of a watched fit is the record of the factors a separate fit with niter = t returns.  Two
    references.  The held-out pairs scored in float64 NumPy (check_against_float64: independent of the device's scoring, with the
    bound the precision of the fit's predictions allows).  And errors_reference.check itself, which is defined on the predictions
    as stored -- counts and max_abs to the bit -- and so takes the scoring kernel's own values (its own tests pin those);
    handed float64 scores it would reject every float32 record by definition."""
    from cmfrec_amd import Validation
    m, n, k, row, col, val, held, start = _explicit_problem(dtype)
    hr, hc, hx = row[held], col[held], val[held]
    v = Validation((hr, hc, hx), every=1, restore_best=False)
    watched = _explicit_fit(dtype, 4, validation=v)
    assert len(watched.validation_records_) == 4
    masks = er.masks(hr, hc, m, n, False)
    assert masks[0].all() and not np.isnan(hx).any()
    for t in (1, 3):
        sep = _explicit_fit(dtype, t)
        p64, mag = float64_predictions(sep, hr, hc)
        w64 = check_against_float64(watched.validation_records_[t - 1], p64, (k + 4) * EPS[dtype] * mag, hx, "history %s t=%d" % (np.dtype(dtype).name, t))
        pred = stored_predictions(sep, hr, hc)
        assert (np.abs(pred.astype(np.float64) - p64) <= (k + 4) * EPS[dtype] * mag).all()
        worst = er.check(watched.validation_records_[t - 1], pred, hx, None, *masks, what="history %s t=%d" % (np.dtype(dtype).name, t))
        print("history record %s t=%d: error / bound %.3g against float64 NumPy, %.3g against the stored predictions" % (np.dtype(dtype).name, t, w64, worst))


# ---- (c) early stopping ---------------------------------------------------------------------------------------------------------
# 200 x 150, 3,000 entries, k = 20, a 20 % hold-out.  Seed and lambda chosen on the CPU with the oracle (fit_explicit_als in float64,
# Cholesky solves, both biases from zero, start values below, niter = 1 .. 20, the held-out pairs scored in NumPy): held-out RMSE
#   1.2964 0.7312 0.6045 0.5687 0.5564 0.5527 0.5477 0.5422 0.5397 0.5427 0.5495 0.5569 0.5646 0.5725 0.5802 0.5870 0.5924 0.5969
#   0.6012 0.6053
# -- the minimum after iteration 8 (0-based), 1.8 % higher two iterations later, and rising to the end.
STOP_SEED, STOP_LAMBDA = 13, 1e-3


def _overfit_problem():
    m, n, nnz, k = 200, 150, 3000, 20
    rng = np.random.default_rng(STOP_SEED)
    lin = rng.choice(m * n, size=nnz, replace=False)
    row, col = (lin // n).astype(np.int32), (lin % n).astype(np.int32)
    P, Q = rng.standard_normal((m, 1)), rng.standard_normal((n, 1))
    rng.standard_normal(m + n)                                  # (kept: the constants above were chosen on this stream of draws)
    val = 3.0 + np.einsum("ij,ij->i", P[row], Q[col]) + 0.1 * rng.standard_normal(nnz)
    held = rng.random(nnz) < 0.2
    A0 = rng.standard_normal((m, k)) * 0.01
    B0 = rng.standard_normal((n, k)) * 0.1
    return m, n, k, row, col, val, held, A0, B0


def test_early_stopping_returns_the_best_iterate():
    from cmfrec_amd import CMF, Validation
    m, n, k, row, col, val, held, A0, B0 = _overfit_problem()
    tr = ~held
    hr, hc, hx = row[held], col[held], val[held]
    niter, patience = 20, 2
    v = Validation((hr, hc, hx), patience=patience)
    mdl = CMF(k=k, lambda_=STOP_LAMBDA, use_cg=False, use_float=False, nthreads=1, niter=niter, finalize_chol=False).fit(
        (row[tr], col[tr], val[tr]), shape=(m, n), A0=A0, B0=B0, validation=v)
    rm = [h["rmse"] for h in mdl.validation_history_]
    print("early stopping: held-out RMSE per iteration", np.array2string(np.array(rm), precision=4), "best", mdl.best_iteration_, "ran", mdl.n_iter_)
    best = mdl.best_iteration_
    assert mdl.n_iter_ == best + 1 + patience < niter
    assert len(rm) == mdl.n_iter_ and int(np.argmin(rm)) == best and rm[best] == min(rm)
    # the fitted model is the best iterate: its own record is the one taken after that iteration
    pred = stored_predictions(mdl, hr, hc)
    er.check(mdl.validation_records_[best], pred, hx, None, *er.masks(hr, hc, m, n, False), what="the fitted model against the best record")
    now = mdl.evaluate_error((hr, hc, hx))
    assert now["rmse"] < rm[-1]                                  # fails if the last iterate were returned
    assert abs(now["rmse"] - rm[best]) <= 1e-12 * rm[best]
    # ... and so are the matrices for predictions on new data
    assert np.array_equal(mdl._B_plus_bias[:, :-1], mdl.B_)
    Bp = mdl._B_plus_bias.astype(np.float64)
    assert frob(mdl._BtB, Bp.T @ Bp) < 1e-10
    # restore_best=False: the same fit stops at the same place and returns its last iterate
    last = CMF(k=k, lambda_=STOP_LAMBDA, use_cg=False, use_float=False, nthreads=1, niter=niter, finalize_chol=False).fit(
        (row[tr], col[tr], val[tr]), shape=(m, n), A0=A0, B0=B0, validation=Validation((hr, hc, hx), patience=patience, restore_best=False))
    assert last.n_iter_ == mdl.n_iter_ and last.best_iteration_ == best
    assert abs(last.evaluate_error((hr, hc, hx))["rmse"] - rm[-1]) <= 1e-12 * rm[-1]


# ---- (d) the implicit model: early stopping on NDCG@10 -----------------------------------------------------------------------
# 200 x 150, 3,000 interactions drawn from a rank-3 preference model, k = 20, a 20 % hold-out, lambda 0.01, alpha 10.  Seed chosen on
# the CPU with the oracle (fit_implicit_als in float64, niter = 1 .. 20, the held-out items ranked in NumPy with the training items
# left out, cmfrec_amd.metrics.ranking_metrics): mean NDCG@10 per iteration
#   CG        0.1024 0.1682 0.1980 0.2123 0.2056 0.2037 0.2011 0.2035 0.2028 0.1999 0.2030 0.2002 0.1977 0.1962 0.1986 0.1995 0.2032 0.2034
#             0.2052 0.2023      -- the maximum after iteration 3 (0-based), 4 % lower two iterations later, never reached again
#   Cholesky  0.1082 0.1965 0.2243 0.2164 0.2153 0.2112 0.2113 0.2041 0.2000 0.2001 0.1984 0.1939 0.1931 0.1925 0.1918 0.1932 0.1896 0.1884
#             0.1892 0.1914      -- the maximum after iteration 2, 4 % lower two iterations later
NDCG_SEED, NDCG_LAMBDA, NDCG_ALPHA = 48, 0.01, 10.0


def _implicit_overfit_problem():
    m, n, nnz, k, rank = 200, 150, 3000, 20, 3
    rng = np.random.default_rng(NDCG_SEED)
    P, Q = rng.standard_normal((m, rank)), rng.standard_normal((n, rank))
    logits = 1.0 * (P @ Q.T) + 0.5 * rng.standard_normal(n)[None, :]
    g = logits + rng.gumbel(size=(m, n))
    lin = rng.permutation(np.argsort(-g, axis=None)[:nnz])
    row, col = (lin // n).astype(np.int32), (lin % n).astype(np.int32)
    val = np.ceil(rng.lognormal(0.5, 0.7, nnz))
    held = rng.random(nnz) < 0.2
    A0 = rng.standard_normal((m, k)) * 0.1
    B0 = np.zeros((n, k))
    return m, n, k, row, col, val, held, A0, B0


@pytest.mark.parametrize("use_cg", [True, False], ids=["cg", "chol"])
def test_implicit_early_stopping_on_ndcg(use_cg):
    import scipy.sparse as sp
    import rank_metrics_reference as rr
    from cmfrec_amd import CMF_implicit, Validation
    m, n, k, row, col, val, held, A0, B0 = _implicit_overfit_problem()
    tr = ~held
    X_val = sp.csr_matrix((val[held], (row[held], col[held])), shape=(m, n))
    X_train = sp.csr_matrix((val[tr], (row[tr], col[tr])), shape=(m, n))
    niter, patience = 20, 2
    make = lambda **kw: CMF_implicit(k=k, lambda_=NDCG_LAMBDA, alpha=NDCG_ALPHA, use_cg=use_cg, use_float=False, niter=niter, finalize_chol=False).fit(
        (row[tr], col[tr], val[tr]), shape=(m, n), A0=A0, B0=B0, validation=Validation(X_val, patience=patience, **kw))
    mdl = make()                                                          # the model's default watch: NDCG@10, the training items excluded
    nd = [h["ndcg"] for h in mdl.validation_history_]
    print("implicit early stopping cg=%s: NDCG@10 per iteration" % use_cg, np.array2string(np.array(nd), precision=4), "best", mdl.best_iteration_,
          "ran", mdl.n_iter_)
    best = mdl.best_iteration_
    assert mdl.n_iter_ == best + 1 + patience < niter
    assert len(nd) == mdl.n_iter_ and int(np.argmax(nd)) == best and nd[best] == max(nd)
    # the fitted model is the best iterate: its own ranks give the record taken after that iteration
    users = np.flatnonzero(np.diff(X_val.indptr) > 0)
    ip, _, ranks, pool = mdl.ranks_batch(users, X_val[users], exclude=X_train)
    rr.check(mdl.validation_records_[best], ip, ranks, pool, 10, what="the fitted model against the best record")
    now = mdl.evaluate_ranking(X_val, X_train, k=10)
    assert now["users"] == mdl.validation_history_[best]["users"] == len(users)
    assert now["ndcg"] > nd[-1]                                           # fails if the last iterate were returned
    assert abs(now["ndcg"] - nd[best]) <= 1e-12 * nd[best]
    assert frob(mdl._BtB, mdl.B_.astype(np.float64).T @ mdl.B_.astype(np.float64) + NDCG_LAMBDA * np.eye(k)) < 1e-10
    # restore_best=False: the same fit stops at the same place and returns its last iterate
    last = make(restore_best=False)
    assert last.n_iter_ == mdl.n_iter_ and last.best_iteration_ == best
    assert abs(last.evaluate_ranking(X_val, X_train, k=10)["ndcg"] - nd[-1]) <= 1e-12 * nd[-1]
    # mean_rank is watched downwards
    down = CMF_implicit(k=k, lambda_=NDCG_LAMBDA, alpha=NDCG_ALPHA, use_cg=use_cg, use_float=False, niter=4).fit(
        (row[tr], col[tr], val[tr]), shape=(m, n), A0=A0, B0=B0, validation=Validation(X_val, metric="mean_rank"))
    mr = [h["mean_rank"] for h in down.validation_history_]
    assert len(mr) == 4 and down.best_iteration_ == int(np.argmin(mr))


# ---- (d') the implicit model, watched by RMSE ------------------------------------------------------------------------------------

@pytest.mark.parametrize("use_cg", [True, False], ids=["cg", "chol"])
def test_implicit_best_iterate(use_cg):
    """every = 2 over 5 iterations evaluates after iterations 1, 3 and 4 (0-based); the model returned is the best of those: the
    factors and B^T B + lambda I of a separate fit with that many iterations."""
    from cmfrec_amd import CMF_implicit, Validation
    dtype = np.float64
    m, n, k = 300, 200, 12
    row, col, val = make_coo(m, n, 6000, 31, dtype=dtype)
    rng = np.random.default_rng(4)
    held = rng.random(len(val)) < 0.2
    tr = ~held
    A0 = (rng.standard_normal((m, k)) * 0.01).astype(dtype); B0 = np.zeros((n, k), dtype)
    hx = np.ones(int(held.sum()), dtype)
    kw = dict(k=k, lambda_=0.5, alpha=2.0, use_cg=use_cg, use_float=False)
    fit = lambda niter, validation=None: CMF_implicit(niter=niter, **kw).fit((row[tr], col[tr], val[tr]), shape=(m, n), A0=A0, B0=B0,
                                                                              validation=validation)
    mdl = fit(5, Validation((row[held], col[held], hx), metric="rmse", every=2))
    assert mdl.n_iter_ == 5 and [h["iteration"] for h in mdl.validation_history_] == [1, 3, 4]
    rm = [h["rmse"] for h in mdl.validation_history_]
    print("implicit cg=%s: held-out RMSE after iterations 1, 3, 4:" % use_cg, rm, "best", mdl.best_iteration_)
    assert mdl.best_iteration_ == [1, 3, 4][int(np.argmin(rm))]
    sep = fit(mdl.best_iteration_ + 1)
    assert frob(mdl.A_, sep.A_) < 1e-6 and frob(mdl.B_, sep.B_) < 1e-6 and frob(mdl._BtB, sep._BtB) < 1e-6
    pred = stored_predictions(mdl, row[held], col[held], implicit=True)
    er.check(mdl.validation_records_[[1, 3, 4].index(mdl.best_iteration_)], pred, hx, None, *er.masks(row[held], col[held], m, n, True),
             what="implicit: the fitted model against the best record")
    mae = fit(3, Validation((row[held], col[held], hx), metric="mae"))
    assert [h["iteration"] for h in mae.validation_history_] == [0, 1, 2]
    assert mae.best_iteration_ == int(np.argmin([h["mae"] for h in mae.validation_history_]))


# ---- (e) the refusals -----------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_next_fit_alone(monkeypatch):
    from cmfrec_amd import CMF, CMF_implicit, EvalSet, Validation, _lib
    dtype = np.float64
    m, n, k = 120, 90, 8
    row, col, val = make_coo(m, n, 2000, 41, counts=False, dtype=dtype)
    rng = np.random.default_rng(6)
    A0 = rng.standard_normal((m, k)) * 0.1; B0 = rng.standard_normal((n, k)) * 0.1
    inside = Validation((row[:50], col[:50], val[:50]))

    def fit(validation=None, niter=2, implicit=False):
        if implicit:
            return CMF_implicit(k=k, niter=niter, use_float=False).fit((row, col, val), shape=(m, n), A0=A0, B0=B0, validation=validation)
        return CMF(k=k, lambda_=1.0, niter=niter, use_float=False, nthreads=1).fit((row, col, val), shape=(m, n), A0=A0, B0=B0,
                                                                                   validation=validation)

    base = {False: fit(), True: fit(implicit=True)}

    def plain_fit_is_unaffected():
        for implicit in (False, True):
            again = fit(implicit=implicit)
            assert again.n_iter_ == 2 and again.validation_history_ == []
            assert np.array_equal(again.A_, base[implicit].A_) and np.array_equal(again.B_, base[implicit].B_)

    outside = Validation((row[:50] + m, col[:50], val[:50]))                      # every pair beyond the users of X
    all_nan = Validation((row[:50], col[:50], np.full(50, np.nan)))
    for implicit in (False, True):
        for v, words in ((outside, "no pair inside"), (all_nan, "no pair inside"), (Validation((row[:0], col[:0], val[:0])), "no pair inside")):
            with pytest.raises(RuntimeError, match="code 2") as e:
                fit(v if not implicit else Validation((v.row, v.col, v.val), metric="rmse"), implicit=implicit)
            assert words in str(e.value)
            plain_fit_is_unaffected()
        # niter = 0 has no iteration to watch
        with pytest.raises(RuntimeError, match="niter"):
            fit(Validation((inside.row, inside.col, inside.val), metric="rmse"), niter=0, implicit=implicit)
        plain_fit_is_unaffected()
        # a fit that would take the sharded driver, and one that lists several devices
        for name, value in (("CMFREC_HIP_DEVICES", "0,0"), ("CMFREC_HIP_SHARDED", "1")):
            monkeypatch.setenv(name, value)
            if name == "CMFREC_HIP_SHARDED":
                monkeypatch.setenv("CMFREC_HIP_DEVICES", "0")
            with pytest.raises(RuntimeError, match="one device"):
                fit(Validation((inside.row, inside.col, inside.val), metric="rmse"), implicit=implicit)
            monkeypatch.delenv("CMFREC_HIP_DEVICES", raising=False); monkeypatch.delenv("CMFREC_HIP_SHARDED", raising=False)
            plain_fit_is_unaffected()
    # through the C interface: an unknown metric; a monitor without a set; a monitor that is cleared again
    lib = _lib.load(dtype)
    with EvalSet(row[:50], col[:50], val[:50], dtype=dtype) as es:
        for mon, words in ((_lib.FitMonitor(evalset=es.handle, metric=7, every=1), "metric"), (_lib.FitMonitor(evalset=None, metric=0, every=1), "one of the two")):
            assert lib.cmfrec_hip_fit_set_monitor(C.byref(mon)) == 0
            with pytest.raises(RuntimeError, match="code 2") as e:
                fit()                                                             # the monitor waits for the thread's next fit call
            assert words in str(e.value)
            plain_fit_is_unaffected()                                             # ... and is gone after it
        mon = _lib.FitMonitor(evalset=es.handle, metric=7, every=1)
        lib.cmfrec_hip_fit_set_monitor(C.byref(mon))
        lib.cmfrec_hip_fit_set_monitor(None)
        plain_fit_is_unaffected()
        # a monitor with no output arrays at all is legal: the fit runs, watched, and nothing is written
        mon = _lib.FitMonitor(evalset=es.handle, metric=0, every=1, patience=1, restore_best=1)
        lib.cmfrec_hip_fit_set_monitor(C.byref(mon))
        assert fit(niter=3).A_.shape == (m, k)
        plain_fit_is_unaffected()


def test_ranking_watch_refusals():
    """The refusals a ranking set adds: k + k_main beyond the rank kernel, and a set in which no user has a rankable held-out item;
    each before the fit writes anything, each leaving the thread's next fit alone."""
    from cmfrec_amd import CMF, CMF_implicit, Validation
    m, n = 60, 50
    row, col, val = make_coo(m, n, 600, 43, dtype=np.float64)
    fit = lambda k, v=None, cls=CMF_implicit: cls(k=k, niter=2, use_float=False).fit((row, col, val), shape=(m, n), validation=v)
    base = fit(6)
    held_in_train = (row[:40], col[:40], val[:40])                                 # every held-out item is a training item: excluded, T = 0
    outside = (row[:40], col[:40] + n, val[:40])                                   # every held-out item beyond the items of X (then: every row beyond X)
    for v, words in ((Validation(held_in_train), "no user"), (Validation(outside, X_exclude=None), "no user"),
                     (Validation((row[:40] + m, col[:40], val[:40]), X_exclude=None), "no user")):
        with pytest.raises(RuntimeError, match="code 2") as e:
            fit(6, v)
        assert words in str(e.value)
        again = fit(6)
        assert np.array_equal(again.A_, base.A_) and again.validation_history_ == []
    with pytest.raises(RuntimeError, match="272"):
        fit(273, Validation(held_in_train, X_exclude=None))
    with pytest.raises(RuntimeError, match="272"):
        CMF(k=270, k_main=3, niter=2, use_float=False).fit((row, col, val), shape=(m, n), validation=Validation(held_in_train, metric="ndcg", X_exclude=None))
    assert np.array_equal(fit(6).A_, base.A_)
    # the explicit model can watch a ranking metric too (its item bias is part of the scores), and the held-out items in the
    # training set count once the training items are not excluded
    ok = CMF(k=6, niter=3, use_float=False, nthreads=1).fit((row, col, val), shape=(m, n), validation=Validation(held_in_train, metric="hit", k=5, X_exclude=None))
    assert len(ok.validation_history_) == 3 and all(0.0 <= h["hit"] <= 1.0 and h["users"] > 0 for h in ok.validation_history_)
