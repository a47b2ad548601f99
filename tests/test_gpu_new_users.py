"""GPU: new users against a model resident on the device (cmfrec_amd.NewUsers over cmfrec_hip_newrows_*): factors equal to the
one-shot factors_multiple bit for bit, batch after batch on one handle; top-N straight from the device factors equal to
factors_multiple + ops.topN_batch; the users' own items excluded from the solver's shard; limits and lifecycle; the C ABI."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import topn_reference as tr
from conftest import make_coo

pytestmark = pytest.mark.gpu

M_FIT, N_ITEMS, P_SIDE = 400, 600, 7
MODELS = ["cmf_side", "cmf_weights72", "cmf_implicit_features", "implicit_side", "implicit80"]
HAS_U = {"cmf_side", "implicit_side"}
BATCH_ROWS = (1, 17, 200, 5, 64)
_fitted = {}


def fit_model(name, use_float):
    """The five models of the issue, fitted once per precision (niter=2, about 400 users x 600 items)."""
    key = (name, use_float)
    if key in _fitted:
        return _fitted[key]
    from cmfrec_amd import CMF, CMF_implicit
    dt = np.float32 if use_float else np.float64
    m, n = M_FIT, N_ITEMS
    rng = np.random.default_rng(11)
    U = rng.standard_normal((m, P_SIDE)).astype(dt)
    I = rng.standard_normal((n, 4)).astype(dt)             # k_item needs item attributes
    common = dict(niter=2, use_float=use_float, nthreads=1)
    if name.startswith("cmf"):
        row, col, val = make_coo(m, n, 20000, 4, counts=False, dtype=dt)
        if name == "cmf_side":
            mdl = CMF(k=12, k_user=2, k_item=3, k_main=1, lambda_=0.5, random_state=9, **common).fit((row, col, val), U=U, I=I, shape=(m, n))
        elif name == "cmf_weights72":
            w = rng.uniform(0.5, 2.0, len(val)).astype(dt)
            mdl = CMF(k=72, lambda_=0.5, finalize_chol=False, random_state=9, **common).fit((row, col, val), shape=(m, n), W=w)
        else:
            mdl = CMF(k=12, lambda_=0.5, add_implicit_features=True, random_state=9, **common).fit((row, col, val), shape=(m, n))
    else:
        row, col, val = make_coo(m, n, 20000, 3, dtype=dt)
        if name == "implicit_side":
            mdl = CMF_implicit(k=16, k_user=2, k_item=3, lambda_=3.0, random_state=7, **common).fit((row, col, val), U=U, I=I, shape=(m, n))
        else:
            mdl = CMF_implicit(k=80, lambda_=3.0, finalize_chol=False, random_state=7, **common).fit((row, col, val), shape=(m, n))
    _fitted[key] = mdl
    return mdl


def make_batch(name, dt, rows, seed, dense=False):
    """One batch of new users: X as a SciPy COO matrix whose triplets are in random order (every row has an entry, so the
    batch has `rows` rows), or dense with NaN; observation weights for the weighted model; U for the models with side
    information, with more rows than X for the batch of 17 and fewer for the batch of 200."""
    rng = np.random.default_rng(seed)
    n = N_ITEMS
    explicit = name.startswith("cmf")
    lens = rng.integers(1, 40, rows)
    r = np.repeat(np.arange(rows), lens).astype(np.int32)
    c = np.concatenate([rng.choice(n, l, replace=False) for l in lens]).astype(np.int32)
    v = (0.5 * rng.integers(1, 11, len(r)) if explicit else np.ceil(rng.lognormal(1, 1, len(r)))).astype(dt)
    perm = rng.permutation(len(r))
    r, c, v = r[perm], c[perm], v[perm]
    X = sp.coo_matrix((v, (r, c)), shape=(rows, n))
    W = None
    if dense:
        Xd = np.full((rows, n), np.nan, dt)
        Xd[r, c] = v
        X = Xd
    elif name == "cmf_weights72":
        W = sp.coo_matrix((rng.uniform(0.5, 2.0, len(r)).astype(dt), (r, c)), shape=(rows, n))
    U = None
    if name in HAS_U:
        m_u = {17: 25, 200: 150}.get(rows, rows)
        U = rng.standard_normal((m_u, P_SIDE)).astype(dt)
    return dict(X=X, U=U, W=W), (r, c)


def batches(name, dt):
    out = []
    for i, rows in enumerate(BATCH_ROWS):
        dense = name.startswith("cmf") and rows == 5
        out.append(make_batch(name, dt, rows, 100 + i, dense=dense))
    return out


def one_shot(mdl, name, kw):
    if name.startswith("cmf"):
        return mdl.factors_multiple(return_bias=True, **kw)
    return mdl.factors_multiple(X=kw["X"], U=kw["U"]), None


def handle_kw(name, kw):
    return kw if name.startswith("cmf") else dict(X=kw["X"], U=kw["U"])


def random_lists(seed, rows, n=N_ITEMS, most=50):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, most, rows); lens[0] = 0
    ep = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    ei = np.concatenate([np.sort(rng.choice(n, l, replace=False)) for l in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    return ep, ei


def finish(mdl, name, sc, bias):
    """The scores as topN_batch finishes them: + the global mean + the rows' bias for CMF."""
    if not name.startswith("cmf"):
        return sc
    sc = sc + mdl.glob_mean_
    if bias is not None:
        sc = sc + bias[:, None]
    return sc


PREC = pytest.mark.parametrize("use_float", [False, True], ids=["f64", "f32"])
ALL = pytest.mark.parametrize("name", MODELS)


@PREC
@ALL
def test_handle_equals_one_shot(name, use_float):
    """Consecutive batches of 1, 17, 200, 5 and 64 rows on one handle (buffers grow and shrink; m_u > m and m_u < m with U; a
    dense batch with NaN for CMF): factors and bias are bit-identical to factors_multiple.  A refused batch (NaN in U) raises as
    the one-shot call does and leaves the handle usable."""
    dt = np.float32 if use_float else np.float64
    mdl = fit_model(name, use_float)
    with mdl.new_users() as nu:
        for kw, _ in batches(name, dt):
            A1, b1 = one_shot(mdl, name, kw)
            if name.startswith("cmf"):
                A, b = nu.factors(return_bias=True, **kw)
                assert np.array_equal(b, b1)
            else:
                A = nu.factors(**handle_kw(name, kw))
            assert A.dtype == dt and A.shape == A1.shape
            assert np.array_equal(A, A1), (name, A.shape)
            assert np.all(np.isfinite(A))
            if name in HAS_U and A.shape[0] == 17 + 8:
                bad = dict(kw); bad["U"] = kw["U"].copy(); bad["U"][3, 2] = np.nan
                with pytest.raises(RuntimeError, match="missing values in U"):
                    one_shot(mdl, name, bad)
                with pytest.raises(RuntimeError, match="missing values in U"):
                    nu.factors(**handle_kw(name, bad))


@PREC
@ALL
def test_ranking_from_device_factors(name, use_float, monkeypatch):
    """topN with explicit lists equals factors_multiple followed by ops.topN_batch (ids, finished scores, returned factors); the
    device's own scores satisfy the derived conditions of topn_reference against the float64 ranking of those factors; the
    k <= 64 models give the same ids through the MFMA kernel."""
    from cmfrec_amd import ops
    dt = np.float32 if use_float else np.float64
    mdl = fit_model(name, use_float)
    B = np.ascontiguousarray(mdl.B_[:, mdl.k_item:])
    biasB = np.asarray(mdl.item_bias_, dt) if (name.startswith("cmf") and mdl.item_bias) else None
    n_top = 10
    with mdl.new_users() as nu:
        for i, (kw, _) in enumerate(batches(name, dt)):
            hk = handle_kw(name, kw)
            A1, b1 = one_shot(mdl, name, kw)
            rows = A1.shape[0]
            E = random_lists(500 + i, rows)
            Au = np.ascontiguousarray(A1[:, mdl.k_user:])
            ids1, sc1 = ops.topN_batch(Au, B, n_top=n_top, biasB=biasB, exclude=E)
            ids, sc, (A, b) = nu.topN(n=n_top, exclude_seen=False, exclude=E, return_factors=True, **hk)
            assert np.array_equal(A, A1) and (b1 is None or np.array_equal(b, b1))
            assert np.array_equal(ids, ids1), (name, rows)
            assert np.array_equal(sc, finish(mdl, name, sc1, b1)), (name, rows)
            ids_r, sc_r, _, _ = nu._topN_raw(hk.get("X"), hk.get("U"), hk.get("W"), n_top, False, E, False)
            assert np.array_equal(ids_r, ids)
            tr.check_ranking(Au, B, biasB, E[0], E[1], ids_r, sc_r, n_top, dt, verbose=False)
            if mdl.k + mdl.k_main <= 64 and rows in (17, 200):
                monkeypatch.setenv("CMFREC_HIP_TOPN", "wide")
                ids_w, _ = nu.topN(n=n_top, exclude_seen=False, exclude=E, **hk)
                monkeypatch.delenv("CMFREC_HIP_TOPN")
                assert np.array_equal(ids_w, ids), (name, rows)
        s_ms, r_ms = nu.kernel_ms()
        assert s_ms > 0 and r_ms > 0


def seen_problem(name, dt, seed=77):
    """20 new users with triplets in random order: row 0 empty, row 1 holds all but 3 items, row 2 one entry, row 3 300."""
    rng = np.random.default_rng(seed)
    n, rows = N_ITEMS, 20
    lens = rng.integers(2, 40, rows)
    lens[0], lens[1], lens[2], lens[3] = 0, n - 3, 1, 300
    r = np.repeat(np.arange(rows), lens).astype(np.int32)
    c = np.concatenate([rng.choice(n, l, replace=False) for l in lens]).astype(np.int32)
    explicit = name.startswith("cmf")
    v = (0.5 * rng.integers(1, 11, len(r)) if explicit else np.ceil(rng.lognormal(1, 1, len(r)))).astype(dt)
    perm = rng.permutation(len(r))
    r, c, v = r[perm], c[perm], v[perm]
    kw = dict(X=sp.coo_matrix((v, (r, c)), shape=(rows, n)))
    if name in HAS_U:
        kw["U"] = rng.standard_normal((rows, P_SIDE)).astype(dt)
    return kw, r, c, rows


def host_csr(r, c, rows, extra=None):
    """Sorted CSR of the items of each row (and of `extra`'s lists: the union)."""
    lists = []
    for u in range(rows):
        own = c[r == u]
        if extra is not None:
            own = np.union1d(own, extra[1][int(extra[0][u]):int(extra[0][u + 1])])
        lists.append(np.sort(own))
    ep = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    return ep, np.concatenate(lists).astype(np.int32)


@PREC
@ALL
def test_exclude_seen(name, use_float):
    dt = np.float32 if use_float else np.float64
    mdl = fit_model(name, use_float)
    kw, r, c, rows = seen_problem(name, dt)
    n_top = 10
    with mdl.new_users() as nu:
        ids, sc = nu.topN(n=n_top, exclude_seen=True, **kw)
        ids_h, sc_h = nu.topN(n=n_top, exclude_seen=False, exclude=host_csr(r, c, rows), **kw)
        assert np.array_equal(ids, ids_h) and np.array_equal(sc, sc_h)
        for u in range(rows):
            got = ids[u][ids[u] >= 0]
            assert not set(got.tolist()) & set(c[r == u].tolist()), u
        # the row with all but 3 items: those 3, then -1 / -inf; the empty row: a full list
        left = np.setdiff1d(np.arange(N_ITEMS), c[r == 1])
        assert sorted(ids[1][:3].tolist()) == left.tolist() and np.all(ids[1][3:] == -1) and np.all(np.isneginf(sc[1][3:]))
        assert np.all(ids[0] >= 0) and np.all(ids[2] >= 0) and np.all(ids[3] >= 0)
        # the union with further lists
        E = random_lists(9, rows, most=80)
        ids_u, sc_u = nu.topN(n=n_top, exclude_seen=True, exclude=E, **kw)
        ids_uh, sc_uh = nu.topN(n=n_top, exclude_seen=False, exclude=host_csr(r, c, rows, E), **kw)
        assert np.array_equal(ids_u, ids_uh) and np.array_equal(sc_u, sc_uh)
        # the one-shot form makes, uses and closes a handle of its own
        ids_o, sc_o = mdl.topN_new_batch(n=n_top, exclude_seen=True, exclude=E, **kw)
        assert np.array_equal(ids_o, ids_u) and np.array_equal(sc_o, sc_u)
        if name == "cmf_weights72":
            # a dense X with NaN: the present entries are the seen items (rows 0 and 1 left out: a row of NaN is a row
            # without observations, and this model has no side information to solve it from differently)
            Xd = np.full((rows, N_ITEMS), np.nan, dt)
            Xd[r, c] = kw["X"].tocoo().data
            ids_d, sc_d = nu.topN(X=Xd, n=n_top, exclude_seen=True)
            ids_dh, sc_dh = nu.topN(X=Xd, n=n_top, exclude_seen=False, exclude=host_csr(r, c, rows))
            assert np.array_equal(ids_d, ids_dh) and np.array_equal(sc_d, sc_dh)
            for u in range(rows):
                assert not set(ids_d[u][ids_d[u] >= 0].tolist()) & set(c[r == u].tolist()), u


@pytest.mark.parametrize("name", ["cmf_side", "implicit80"])
def test_limits_and_lifecycle(name):
    mdl = fit_model(name, False)
    kw, _ = make_batch(name, np.float64, 17, 5)
    hk = handle_kw(name, kw)
    nu = mdl.new_users()
    with pytest.raises(RuntimeError):
        nu.kernel_ms()                                      # no call yet
    with pytest.raises(RuntimeError, match=r"code 2.*n_top <= min\(128, n\)"):
        nu.topN(n=129, **hk)
    A = nu.factors(**hk)                                    # the handle still works
    assert np.array_equal(A, one_shot(mdl, name, kw)[0])
    s_ms, r_ms = nu.kernel_ms()
    assert s_ms > 0 and r_ms == 0
    nu.topN(n=128, **hk)
    s_ms, r_ms = nu.kernel_ms()
    assert s_ms > 0 and r_ms > 0
    nu.close()
    nu.close()                                              # idempotent
    for call in (lambda: nu.factors(**hk), lambda: nu.topN(**hk), nu.kernel_ms):
        with pytest.raises(RuntimeError, match="closed"):
            call()


@PREC
@pytest.mark.parametrize("name", ["cmf_side", "implicit_side"])
def test_c_abi(name, use_float):
    """cmfrec_hip_newrows_create / _factors / _destroy through ctypes, the struct filled by hand: the factors of
    factors_collective_*_multiple (model.factors_multiple) bit for bit."""
    from cmfrec_amd import _lib
    dt = np.float32 if use_float else np.float64
    mdl = fit_model(name, use_float)
    lib = _lib.load(dt)
    kw, (r, c) = make_batch(name, dt, 64, 31)
    X = kw["X"]
    A1, b1 = one_shot(mdl, name, kw)
    m = _lib.newrows_model_mirror(dt)()
    B = np.ascontiguousarray(mdl.B_, dt); Cm = np.ascontiguousarray(mdl.C_, dt); mu = np.ascontiguousarray(mdl._U_colmeans, dt)
    m.n = m.n_max = B.shape[0]; m.include_all_X = 1; m.p = Cm.shape[0]
    m.k, m.k_user, m.k_item, m.k_main = mdl.k, mdl.k_user, mdl.k_item, mdl.k_main
    m.lam = mdl.lambda_; m.w_main = mdl.w_main; m.w_user = mdl.w_user; m.scaling_biasA = 1; m.w_implicit = 1; m.alpha = 1
    m.w_main_multiplier = 1
    m.B = B.ctypes.data; m.C = Cm.ctypes.data; m.U_colmeans = mu.ctypes.data
    keep = []
    if name == "cmf_side":
        ib = np.ascontiguousarray(mdl.item_bias_, dt); T = np.ascontiguousarray(mdl._TransCtCinvCt, dt)
        keep += [ib, T]
        m.user_bias = 1; m.glob_mean = mdl.glob_mean_; m.w_implicit = mdl.w_implicit; m.biasB = ib.ctypes.data
        m.TransCtCinvCt = T.ctypes.data
    else:
        BtB = np.ascontiguousarray(mdl._BtB, dt)
        keep.append(BtB)
        m.implicit = 1; m.alpha = mdl.alpha; m.w_main_multiplier = mdl._w_main_multiplier; m.BtB = BtB.ctypes.data
    assert lib.cmfrec_hip_sizeof_newrows_model() == C.sizeof(m)
    h = lib.cmfrec_hip_newrows_create(C.byref(m), -1)
    assert h, lib.cmfrec_hip_last_error()
    try:
        b = _lib.NewRowsBatch()
        val = np.ascontiguousarray(X.data, dt); ia = np.ascontiguousarray(X.row, np.int32); ib_ = np.ascontiguousarray(X.col, np.int32)
        U = np.ascontiguousarray(kw["U"], dt)
        b.m = X.shape[0]; b.m_u = U.shape[0]; b.U = U.ctypes.data
        b.X = val.ctypes.data; b.ixA = ia.ctypes.data; b.ixB = ib_.ctypes.data; b.nnz = len(val)
        A = np.empty_like(A1); bias = np.empty(A1.shape[0], dt) if b1 is not None else None
        rc = lib.cmfrec_hip_newrows_factors(h, C.byref(b), _lib.ptr(A), _lib.ptr(bias))
        assert rc == 0, lib.cmfrec_hip_last_error()
        assert np.array_equal(A, A1)
        if b1 is not None:
            assert np.array_equal(bias, b1)
    finally:
        lib.cmfrec_hip_newrows_destroy(h)
