"""Sparse side information whose absent entries are zeros (NA_as_zero_user / NA_as_zero_item) on the triplets themselves: the two
product kernels (cmfrec_amd/csrc/side_zeros_kernels.hpp) against float64 NumPy, the fits of fixture g21 on that route, a fit the
zero-filled dense matrix cannot hold checked by the normal equations of its last half-step, and the refusals that stay.

CMFREC_HIP_ZEROFILL_MAX_GB (read per fit) is the size of the zero-filled matrix from which the fit takes the sparse route; 1e-9
sends every problem there."""
import numpy as np
import pytest

import golden_cases as gc
from topn_reference import gamma

pytestmark = pytest.mark.gpu
DT = [np.float64, np.float32]


# ---- 1. the products ---------------------------------------------------------------------------------------------------------
def _small_triplets(variant):
    """rows = 300, p = 37.  Variant 1: attribute 0 in every row (so no row is empty), rows of 1, 2, 63, 64, 65 entries (more
    entries than attributes: positions repeat), one row that has all 37 attributes -- the only entry of attributes 35 and 36 --
    and one position of a short row given twice.  Variant 2: the same with row 7 emptied and attribute 36 taken out of every row -- a row of 0
    entries and an attribute no row has, which variant 1's "attribute in every row" / "row with every attribute" exclude."""
    rng = np.random.default_rng(7)
    rows, p = 300, 37
    r, c = [], []
    def add(row, cols):
        r.extend([row] * len(cols)); c.extend(int(x) for x in cols)
    add(0, [0])
    add(1, [0, 5])
    for row, n in ((2, 63), (3, 64), (4, 65)):
        add(row, [0] + list(rng.integers(1, 35, n - 1)))
    add(5, list(rng.permutation(37)))
    add(6, [0, 34])
    add(8, [0, 11, 11])                                   # one position twice
    for row in [7] + list(range(9, rows)):
        add(row, [0] + list(rng.choice(np.arange(1, 35), size=int(rng.integers(1, 7)), replace=False)))
    r = np.array(r, np.int32); c = np.array(c, np.int32)
    perm = rng.permutation(len(r))
    r, c = r[perm], c[perm]
    v = rng.standard_normal(len(r))
    if variant == 2:
        keep = (r != 7) & (c != 36)
        r, c, v = r[keep], c[keep], v[keep]
    per_row = np.bincount(r, minlength=rows); per_col = np.bincount(c, minlength=p)
    assert {1, 2, 63, 64, 65}.issubset(set(per_row.tolist())) and per_col[35] == 1
    if variant == 1:
        assert per_row[5] == 37 and len(set(c[r == 5].tolist())) == 37 and per_col[0] >= rows and per_row.min() >= 1
    else:
        assert per_row[7] == 0 and per_col[36] == 0
    return rows, p, r, c, v


def _tall_triplets():
    """rows = 20,000, p = 3: attribute 0 in 19,999 rows (more than two column units of at most 8,192 entries: the partial-sum pass
    runs), attribute 1 in 300 rows, attribute 2 in 5,000."""
    rng = np.random.default_rng(8)
    rows, p = 20000, 3
    r = np.concatenate([np.arange(1, rows), rng.choice(rows, 300, replace=False), rng.choice(rows, 5000, replace=False)]).astype(np.int32)
    c = np.concatenate([np.zeros(rows - 1), np.ones(300), np.full(5000, 2)]).astype(np.int32)
    perm = rng.permutation(len(r))
    return rows, p, r[perm], c[perm], rng.standard_normal(len(r))


def _check_products(rows, p, r, c, v, kc, dtype, seed, ranges, with_none=True):
    """Both products for every row range (and once without column means) against the float64 product of the dtype-rounded
    zero-filled centred matrix, entry by entry within the dot-product bound; each call twice, the same bits."""
    from cmfrec_amd import ops
    rng = np.random.default_rng(seed)
    v = v.astype(dtype)
    ldF = kc + 3
    M = rng.standard_normal((p, kc)).astype(dtype); F = rng.standard_normal((rows, ldF)).astype(dtype)
    alpha = -1.5
    Ud = np.zeros((rows, p), dtype); np.add.at(Ud, (r, c), v)                   # duplicates add up
    Uabs = np.zeros((rows, p)); np.add.at(Uabs, (r, c), np.abs(v.astype(np.float64)))
    per_row = np.bincount(r, minlength=rows); per_col = np.bincount(c, minlength=p)
    mu = (Ud.astype(np.float64).sum(axis=0) / rows).astype(dtype)
    M64, F64 = M.astype(np.float64), F[:, :kc].astype(np.float64)
    worst = 0.0
    for colmeans in ([mu, None] if with_none else [mu]):
        mu64 = np.zeros(p) if colmeans is None else colmeans.astype(np.float64)
        Uc = Ud if colmeans is None else (Ud - colmeans[None, :]).astype(dtype)          # what the dense route uploads
        want_UM = alpha * (Uc.astype(np.float64) @ M64)
        want_UtF = Uc.astype(np.float64).T @ F64
        bound_UM = gamma(per_row + p + 2, dtype)[:, None] * abs(alpha) * (Uabs @ np.abs(M64) + (np.abs(mu64) @ np.abs(M64))[None, :])
        bound_UtF = gamma(per_col + rows + 2, dtype)[:, None] * (Uabs.T @ np.abs(F64) + np.abs(mu64)[:, None] * np.abs(F64).sum(axis=0)[None, :])
        for first, count in (ranges if colmeans is not None else ranges[:1]):
            UM, UtF = ops.side_zeros_products(rows, p, r, c, v, colmeans=colmeans, M=M, alpha=alpha, first=first, count=count, F=F, kc=kc)
            UM2, UtF2 = ops.side_zeros_products(rows, p, r, c, v, colmeans=colmeans, M=M, alpha=alpha, first=first, count=count, F=F, kc=kc)
            assert np.array_equal(UM, UM2) and np.array_equal(UtF, UtF2), "two calls, different bits"
            assert UM.shape == (count, kc) and UtF.shape == (p, kc)
            eUM = np.abs(UM.astype(np.float64) - want_UM[first:first + count]); bUM = bound_UM[first:first + count]
            eUtF = np.abs(UtF.astype(np.float64) - want_UtF)
            ratio = max(float((eUM / np.maximum(bUM, 1e-300)).max()), float((eUtF / np.maximum(bound_UtF, 1e-300)).max()))
            worst = max(worst, ratio)
            print("side_zeros_products %s rows=%d p=%d kc=%d first=%d count=%d colmeans=%s: worst error / bound %.3f"
                  % (np.dtype(dtype).name, rows, p, kc, first, count, colmeans is not None, ratio))
            assert np.all(eUM <= bUM), (first, count, float((eUM - bUM).max()))
            assert np.all(eUtF <= bound_UtF), float((eUtF - bound_UtF).max())
            if colmeans is not None:
                assert np.all(UtF[per_col == 0] == 0)                         # an attribute nobody has: mu = 0, a row of zeros
    return worst


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("kc", [1, 7, 64, 65, 130, 272])
def test_products_small(dtype, kc):
    for variant in (1, 2):
        rows, p, r, c, v = _small_triplets(variant)
        _check_products(rows, p, r, c, v, kc, dtype, 100 + kc, [(0, rows), (17, 101)])


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("kc", [8, 65])
def test_products_long_column(dtype, kc):
    rows, p, r, c, v = _tall_triplets()
    _check_products(rows, p, r, c, v, kc, dtype, 200 + kc, [(0, rows), (17, 101)])


@pytest.mark.parametrize("dtype", DT)
def test_products_poisoned(dtype, monkeypatch):
    """One width per shape again with LDS and every fresh device buffer filled with NaN patterns in front of the launches."""
    monkeypatch.setenv("CMFREC_HIP_POISON_LDS", "1")
    rows, p, r, c, v = _small_triplets(2)
    _check_products(rows, p, r, c, v, 7, dtype, 107, [(0, rows), (17, 101)])
    rows, p, r, c, v = _tall_triplets()
    _check_products(rows, p, r, c, v, 8, dtype, 208, [(0, rows)], with_none=False)


# ---- 2. the fits of g21 on the sparse route -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
def test_g21_fits_on_the_sparse_route(dtype, monkeypatch):
    """Every case of fixture g21 (both models, closed form, CG, CG + finalize_chol, scale_lam / scale_lam_sideinfo, U, I, both; U
    covers 80 of 90 users) with the zero-filled matrix declared too large: the same fixtures at the same tolerance, and the
    constant kept for new rows.  The distance to the dense route of the same build is printed."""
    g = gc.load("g21_na_as_zero_UI", dtype)
    d = gc.sparse_sideinfo_problem(dtype)
    tol = 1e-6 if dtype is np.float64 else 1e-2
    for ci, (name, implicit, which, sl, sls, solver) in enumerate(gc.NAZ_UI_CASES):
        exp = {key[len("c%d_" % ci):]: g[key] for key in g.files if key.startswith("c%d_" % ci)}
        monkeypatch.setenv("CMFREC_HIP_ZEROFILL_MAX_GB", "1e-9")
        got = gc.naz_ui_hip(d, implicit, which, sl, sls, solver, dtype)
        got = {key: v for key, v in got.items() if key in exp}
        monkeypatch.delenv("CMFREC_HIP_ZEROFILL_MAX_GB")
        dense = gc.naz_ui_hip(d, implicit, which, sl, sls, solver, dtype)
        err = gc.compare_fits(got, exp)
        print("g21 %s %s: sparse route against the fixture %.3e, against the dense route %.3e"
              % (np.dtype(dtype).name, name, err, gc.compare_fits(got, {key: v for key, v in dense.items() if key in exp})))
        assert exp and err < tol, (name, err)
    monkeypatch.setenv("CMFREC_HIP_ZEROFILL_MAX_GB", "1e-9")
    name, implicit, which, sl, sls, solver = gc.NAZ_UI_CASES[2]
    mdl = gc.naz_ui_hip(d, implicit, which, sl, sls, solver, dtype, precompute=True)["_model"]
    want = -mdl.w_user * (mdl.C_.astype(np.float64).T @ mdl._U_colmeans.astype(np.float64))
    assert mdl._CtUbias.shape == want.shape and np.abs(mdl._CtUbias - want).max() <= (1e-12 if dtype is np.float64 else 1e-5) * max(1.0, np.abs(want).max())
    exp = {key[3:]: g[key] for key in g.files if key.startswith("c2_")}
    assert gc.compare_fits({key: getattr(mdl, key + "_") for key in ("A", "B", "C", "D")}, exp) < tol


# ---- 3. a size the dense route cannot take ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
def test_fit_beyond_the_dense_limit(dtype):
    """120,000 users x 10,000 (float64) / 20,000 (float32) attributes, three per user: 9.6e9 bytes zero-filled, beyond the default
    8 GB.  The fit returns, and -- A being the last matrix of an iteration -- 64 sampled rows of A solve their own normal
    equations, built in float64 from the returned B, C, column means and the triplets:
        (blockdiag(0, B_x^T B_x over the user's entries) + w_user C^T C on the first k_user + k unknowns + lambda I) a
            = [0 ; B_x^T x] + w_user C^T (u - mu)."""
    import scipy.sparse as sp
    from cmfrec_amd import CMF
    rng = np.random.default_rng(31)
    m, n, p = 120000, 500, (10000 if dtype is np.float64 else 20000)
    k, ku, km = 6, 2, 1
    users = np.arange(m)
    xr = np.repeat(users, 5).astype(np.int32)
    xc = ((rng.integers(0, n, m)[:, None] + 97 * np.arange(5)[None, :]) % n).reshape(-1).astype(np.int32)          # five distinct items
    xv = (0.5 * rng.integers(1, 11, len(xr))).astype(dtype)
    ur = np.repeat(users, 3).astype(np.int32)
    uc = ((rng.integers(0, p, m)[:, None] + 3331 * np.arange(3)[None, :]) % p).reshape(-1).astype(np.int32)        # three distinct attributes
    uv = rng.standard_normal(len(ur)).astype(dtype)
    assert float(m) * p * np.dtype(dtype).itemsize > 8e9
    U = sp.coo_matrix((uv, (ur, uc)), shape=(m, p))
    mdl = CMF(k=k, k_user=ku, k_main=km, user_bias=False, item_bias=False, center=False, use_cg=False, niter=1, NA_as_zero_user=True,
              precompute_for_predictions=False, use_float=dtype is np.float32)
    mdl.fit((xr, xc, xv), U=U, shape=(m, n))
    A, B, Cm, mu = (np.asarray(x, np.float64) for x in (mdl.A_, mdl.B_, mdl.C_, mdl._U_colmeans))
    assert A.shape == (m, ku + k + km) and Cm.shape == (p, ku + k) and mu.shape == (p,) and np.all(np.isfinite(A))
    want_mu = np.bincount(uc, weights=uv.astype(np.float64), minlength=p) / m
    assert np.abs(mu - want_mu).max() <= (1e-12 if dtype is np.float64 else 1e-6) * max(1.0, np.abs(want_mu).max())
    kc, kt = ku + k, ku + k + km
    CtC = Cm.T @ Cm
    Ctmu = Cm.T @ mu
    tol = 1e-6 if dtype is np.float64 else 1e-2
    worst = 0.0
    for i in rng.choice(m, 64, replace=False):
        Bx = B[xc[5 * i:5 * i + 5]]
        Mi = mdl.lambda_ * np.eye(kt)
        Mi[ku:, ku:] += Bx.T @ Bx
        Mi[:kc, :kc] += mdl.w_user * CtC
        rhs = np.zeros(kt)
        rhs[ku:] = Bx.T @ xv[5 * i:5 * i + 5].astype(np.float64)
        rhs[:kc] += mdl.w_user * (Cm[uc[3 * i:3 * i + 3]].T @ uv[3 * i:3 * i + 3].astype(np.float64) - Ctmu)
        a = np.linalg.solve(Mi, rhs)
        worst = max(worst, float(np.abs(A[i] - a).max() / np.abs(a).max()))
    print("fit beyond the dense limit %s: worst relative error of 64 rows of A against their normal equations %.3e" % (np.dtype(dtype).name, worst))
    assert worst < tol


# ---- 4. refusals that stay ----------------------------------------------------------------------------------------------------
def test_row_block_shard_is_refused():
    from cmfrec_amd.session import AlsSession
    s = AlsSession(60, 40, 4, False, p=5, m_u=60, k_user=1, row_range=(10, 50), use_cg=False)
    try:
        with pytest.raises(RuntimeError, match="code 2"):
            s.set_sideinfo_sparse_zeros("U", [0, 12], [1, 3], [1.0, 2.0], colmeans=np.zeros(5))
    finally:
        s.close()


@pytest.mark.parametrize("dtype", DT)
def test_more_rows_of_U_than_X_stays_refused(dtype, monkeypatch):
    monkeypatch.setenv("CMFREC_HIP_ZEROFILL_MAX_GB", "1e-9")
    d = gc.sparse_sideinfo_problem(dtype)
    name, implicit, which, sl, sls, solver = gc.NAZ_UI_CASES[2]
    c = d["U_coo"]
    d2 = dict(d); d2["U_coo"] = (c[0], c[1], c[2], d["m"] + 5, c[4])
    with pytest.raises(RuntimeError, match="code 2"):
        gc.naz_ui_hip(d2, implicit, "U", sl, sls, solver, dtype)
