"""GPU: the reference's one-user interface (topN, topN_warm, topN_cold, factors_warm, factors_cold, predict_warm, predict_cold of
CMF and CMF_implicit) against the batch forms with a batch of one.  Ids are equal; factors and predictions are bitwise equal;
ranking scores are bitwise equal for k > 64 and, for k <= 64, under CMFREC_HIP_TOPN=wide (the one-user methods rank on the MFMA
kernel for every k)."""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import make_coo

pytestmark = pytest.mark.gpu

M, N, P = 60, 300, 5
MODELS = [("cmf", 8), ("cmf", 70), ("implicit", 8), ("implicit", 70)]
_fitted = {}


def fit_model(kind, k, sparse_U=False):
    """CMF with biases, k_main and user attributes / CMF_implicit with user attributes: 60 users x 300 items, fitted once."""
    key = (kind, k, sparse_U)
    if key in _fitted:
        return _fitted[key]
    from cmfrec_amd import CMF, CMF_implicit
    rng = np.random.default_rng(11)
    U = rng.standard_normal((M, P))
    if sparse_U:
        U = sp.csr_matrix(np.where(rng.random((M, P)) < 0.6, U, 0.0))
    common = dict(niter=2, use_float=False, nthreads=1)
    if kind == "cmf":
        row, col, val = make_coo(M, N, 3000, 4, counts=False)
        mdl = CMF(k=k, k_main=2, lambda_=0.5, random_state=9, **common).fit((row, col, val), U=U, shape=(M, N))
    else:
        row, col, val = make_coo(M, N, 3000, 3)
        mdl = CMF_implicit(k=k, lambda_=3.0, random_state=7, **common).fit((row, col, val), U=U, shape=(M, N))
    _fitted[key] = (mdl, U)
    return _fitted[key]


def one_row(seed, kind):
    rng = np.random.default_rng(seed)
    col = np.sort(rng.choice(N, 25, replace=False)).astype(np.int32)
    val = rng.uniform(1, 5, 25) if kind == "cmf" else np.ceil(rng.lognormal(1, 1, 25))
    u = rng.standard_normal(P)
    X = sp.csr_matrix((val, (np.zeros(25, np.int32), col)), shape=(1, N))
    return col, val, u, X


def same_ranking(monkeypatch, k, one, batch):
    """``one`` () -> (ids [n], scores [n]); ``batch`` () -> (ids [1, n], scores [1, n]), taken on the MFMA kernel where k <= 64."""
    ids, sc = one()
    if k <= 64:
        monkeypatch.setenv("CMFREC_HIP_TOPN", "wide")
    try:
        bids, bsc = batch()
    finally:
        monkeypatch.delenv("CMFREC_HIP_TOPN", raising=False)
    assert ids.ndim == 1 and sc.ndim == 1 and ids.shape == sc.shape == bids[0].shape
    assert np.array_equal(ids, bids[0])
    assert sc.tobytes() == bsc[0].tobytes()


@pytest.mark.parametrize("kind,k", MODELS)
def test_topN_of_a_fitted_user(monkeypatch, kind, k):
    monkeypatch.delenv("CMFREC_HIP_TOPN", raising=False)
    mdl, _ = fit_model(kind, k)
    rng = np.random.default_rng(1)
    for user in (0, 17, M - 1):
        ex = rng.choice(N, 40, replace=False)
        ep = np.zeros(M + 1, np.int64); ep[user + 1:] = len(ex)
        for n in (1, 10, 128):
            same_ranking(monkeypatch, k, lambda: mdl.topN(user, n, exclude=ex, output_score=True),
                         lambda: mdl.topN_batch([user], n, exclude=(ep, ex)))
        same_ranking(monkeypatch, k, lambda: mdl.topN(user, output_score=True), lambda: mdl.topN_batch([user]))
        ids = mdl.topN(user, 7, exclude=ex)
        assert isinstance(ids, np.ndarray) and ids.shape == (7,) and not set(ids.tolist()) & set(ex.tolist())
        # include: the candidate kernel, the same for both forms
        inc = rng.choice(N, 50, replace=False)
        ids, sc = mdl.topN(user, 5, include=inc, output_score=True)
        bids, bsc = mdl.topN_batch([user], 5, include=inc)
        assert np.array_equal(ids, bids[0]) and sc.tobytes() == bsc[0].tobytes() and set(ids.tolist()) <= set(inc.tolist())


@pytest.mark.parametrize("kind,k", MODELS)
def test_new_user_calls(monkeypatch, kind, k):
    monkeypatch.delenv("CMFREC_HIP_TOPN", raising=False)
    mdl, _ = fit_model(kind, k)
    for seed in (2, 3):
        col, val, u, X = one_row(seed, kind)
        U1 = u.reshape(1, -1)
        ex = np.random.default_rng(seed).choice(N, 30, replace=False)
        excl = (np.array([0, len(ex)]), ex)
        same_ranking(monkeypatch, k, lambda: mdl.topN_warm(10, X_col=col, X_val=val, U=u, exclude=ex, output_score=True),
                     lambda: mdl.topN_new_batch(X=X, U=U1, n=10, exclude_seen=False, exclude=excl))
        same_ranking(monkeypatch, k, lambda: mdl.topN_warm(128, X_col=col, X_val=val, output_score=True),
                     lambda: mdl.topN_new_batch(X=X, n=128, exclude_seen=False))
        same_ranking(monkeypatch, k, lambda: mdl.topN_cold(10, U=u, output_score=True), lambda: mdl.topN_new_batch(X=None, U=U1, n=10))
        ids = mdl.topN_warm(X_col=col, X_val=val)
        assert ids.shape == (10,)
        inc = np.arange(3, N, 4)
        ids, sc = mdl.topN_warm(5, X_col=col, X_val=val, U=u, include=inc, output_score=True)
        bids, bsc = mdl.topN_new_batch(X=X, U=U1, n=5, exclude_seen=False, include=inc)
        assert np.array_equal(ids, bids[0]) and sc.tobytes() == bsc[0].tobytes()
        # factors
        a = mdl.factors_warm(X_col=col, X_val=val, U=u)
        assert a.ndim == 1 and a.tobytes() == mdl.factors_multiple(X=X, U=U1)[0].tobytes()
        a = mdl.factors_cold(U=u)
        assert a.ndim == 1 and a.tobytes() == mdl.factors_multiple(X=None, U=U1)[0].tobytes()
        # predictions
        items = np.array([0, 5, 17, N - 1, 5])
        rows = np.zeros(len(items), np.int64)
        p = mdl.predict_warm(items, X_col=col, X_val=val, U=u)
        assert p.shape == (5,) and p.tobytes() == mdl.predict_new_batch(X=X, U=U1, row=rows, item=items).tobytes()
        p = mdl.predict_cold(items, U=u)
        assert p.shape == (5,) and p.tobytes() == mdl.predict_new_batch(X=None, U=U1, row=rows, item=items).tobytes()


@pytest.mark.parametrize("k", [8, 70])
def test_explicit_model_forms(monkeypatch, k):
    """CMF only: the bias with return_bias, a dense X with NaN equal to the sparse form of the same row."""
    monkeypatch.delenv("CMFREC_HIP_TOPN", raising=False)
    mdl, _ = fit_model("cmf", k)
    col, val, u, X = one_row(5, "cmf")
    U1 = u.reshape(1, -1)
    a, bias = mdl.factors_warm(X_col=col, X_val=val, U=u, return_bias=True)
    A, B = mdl.factors_multiple(X=X, U=U1, return_bias=True)
    assert a.tobytes() == A[0].tobytes() and np.ndim(bias) == 0 and np.float64(bias).tobytes() == B[0].tobytes()
    dense = np.full(N, np.nan); dense[col] = val
    a2, bias2 = mdl.factors_warm(X=dense, U=u, return_bias=True)
    A2, B2 = mdl.factors_multiple(X=dense.reshape(1, -1), U=U1, return_bias=True)
    assert a2.tobytes() == A2[0].tobytes() and np.float64(bias2).tobytes() == B2[0].tobytes()
    ids_d, sc_d = mdl.topN_warm(10, X=dense, U=u, output_score=True)
    ids_s, sc_s = mdl.topN_warm(10, X_col=col, X_val=val, U=u, output_score=True)
    assert np.array_equal(ids_d, ids_s)
    assert np.allclose(sc_d, sc_s, rtol=1e-9, atol=1e-9)     # (the dense and the sparse solve sum in different orders)


@pytest.mark.parametrize("kind", ["cmf", "implicit"])
def test_sparse_attributes(kind):
    """A model fitted with sparse U: U_col / U_val is the sparse row it denotes."""
    mdl, _ = fit_model(kind, 8, sparse_U=True)
    col, val, u, X = one_row(7, kind)
    ucol = np.array([0, 3, 4]); uval = u[ucol]
    Us = sp.csr_matrix((uval, (np.zeros(3, np.int32), ucol)), shape=(1, P))
    a = mdl.factors_warm(X_col=col, X_val=val, U_col=ucol, U_val=uval)
    assert a.tobytes() == mdl.factors_multiple(X=X, U=Us)[0].tobytes()
    a = mdl.factors_cold(U_col=ucol, U_val=uval)
    assert a.tobytes() == mdl.factors_multiple(X=None, U=Us)[0].tobytes()
    ids, sc = mdl.topN_cold(10, U_col=ucol, U_val=uval, output_score=True)
    bids, bsc = mdl.topN_new_batch(X=None, U=Us, n=10)
    assert np.array_equal(ids, bids[0])


@pytest.mark.parametrize("kind", ["cmf", "implicit"])
def test_handles_are_resident_and_released(monkeypatch, kind):
    """One ModelRanker and one NewUsers per model whatever the number of calls, with split="auto"; fit() and close() drop them."""
    from cmfrec_amd import CMF, CMF_implicit, models, new_users
    made = {"ranker": 0, "new": 0}
    r_init, n_init = models.ModelRanker.__init__, new_users.NewUsers.__init__

    def count_r(self, *a, **kw):
        made["ranker"] += 1
        r_init(self, *a, **kw)

    def count_n(self, *a, **kw):
        made["new"] += 1
        n_init(self, *a, **kw)

    monkeypatch.setattr(models.ModelRanker, "__init__", count_r)
    monkeypatch.setattr(new_users.NewUsers, "__init__", count_n)
    rng = np.random.default_rng(11)
    U = rng.standard_normal((M, P))
    if kind == "cmf":
        data = make_coo(M, N, 3000, 4, counts=False)
        mdl = CMF(k=8, lambda_=0.5, niter=1, use_float=False, nthreads=1)
    else:
        data = make_coo(M, N, 3000, 3)
        mdl = CMF_implicit(k=8, lambda_=3.0, niter=1, use_float=False, nthreads=1)
    mdl.fit(data, U=U, shape=(M, N))
    col, val, u, _ = one_row(8, kind)
    for _ in range(3):
        mdl.topN(3); mdl.topN_warm(X_col=col, X_val=val); mdl.topN_cold(U=u); mdl.factors_cold(U=u); mdl.predict_cold([1, 2], U=u)
    assert made == {"ranker": 1, "new": 1}
    rk, nw = mdl._one_user_ranker, mdl._one_user_new
    assert rk._ranker.split == "auto" and nw.split == "auto"
    assert rk.slices() >= 1
    before = mdl.topN(3, output_score=True)
    mdl.fit(data, U=U, shape=(M, N))
    assert "_one_user_ranker" not in mdl.__dict__ and "_one_user_new" not in mdl.__dict__
    assert not rk._ranker.handle and not nw.handle                      # closed, not just forgotten
    after = mdl.topN(3, output_score=True)                              # the same fit: the same answer from new handles
    assert made == {"ranker": 2, "new": 1}
    assert np.array_equal(before[0], after[0]) and before[1].tobytes() == after[1].tobytes()
    mdl.close()
    assert "_one_user_ranker" not in mdl.__dict__
    mdl.close()
