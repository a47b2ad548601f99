"""New rows with observation weights, dense X and implicit features (factors_collective_explicit_multiple): the seeded
problem, the named cases, one positional ctypes call that serves the compiled reference and the product alike, and the
float64 normal equations of every closed-form case written out in NumPy.

Fixture: tests/golden/g40_new_rows_options_{f64,f32}.npz (tests/golden/make_golden_new_rows_options.py)."""
import ctypes as C
import os

import numpy as np

from golden_cases import GOLD, TAGS, new_rows_problem

KS = (6, 50)
FIXTURE = "g40_new_rows_options"
# float32 tolerance of new rows (tests/test_gpu_golden.py::TOL); the reference's own float32 rows must lie within a quarter of it
TOL32, TOL64 = 1e-4, 1e-10


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def problem(dtype, k):
    """golden_cases.new_rows_problem + Bi, weights (one zero, one row 1e3 times the others'), the dense form of the rows
    (one complete, one with NaN only in its last column, one all NaN) and dense weights with NaN where X is missing."""
    d = new_rows_problem(dtype, k)
    rng = np.random.default_rng(97 + k)
    n, m, km = d["n"], d["m"], d["km"]
    d["Bi_plain"] = (rng.standard_normal((n, k)) * 0.3).astype(dtype)
    d["Bi_full"] = (rng.standard_normal((n, k + km)) * 0.3).astype(dtype)
    row, col = d["row"], d["col"]
    w = rng.uniform(0.5, 2.0, len(row))
    w[7] = 0.0
    w[row == 9] *= 1e3
    d["weight"] = w.astype(dtype)
    X = np.full((m, n), np.nan, dtype)
    X[row, col] = d["ratings"]
    X[0] = 0.5 * rng.integers(1, 11, n)                       # complete
    X[1] = 0.5 * rng.integers(1, 11, n); X[1, n - 1] = np.nan  # NaN only in the last column
    X[5] = np.nan                                              # no observations
    d["Xfull"] = X
    W = np.full((m, n), np.nan, dtype)
    W[row, col] = d["weight"]
    for r in (0, 1):
        W[r] = rng.uniform(0.5, 2.0, n)
    W[~np.isfinite(X)] = np.nan
    d["Wfull"] = W
    mask = np.random.default_rng(5).random(d["U_less"].shape) < 0.35
    mask[4] = False; mask[3, :2] = True                        # row 4: observations only; row 3: attributes only
    d["U_csr"] = dense_to_csr(np.where(mask, d["U_less"], np.nan))
    return d


def dense_to_csr(M):
    """(indptr uint64, indices int32, values, rows, cols) of the finite entries of M, row-major."""
    ok = np.isfinite(M)
    p = np.zeros(M.shape[0] + 1, np.uint64); p[1:] = np.cumsum(ok.sum(1))
    r, c = np.nonzero(ok)
    return p, c.astype(np.int32), np.ascontiguousarray(M[r, c]), M.shape[0], M.shape[1]


def coo_to_csr_stable(row, col, val, m, *more):
    """Stable counting sort by row, as the reference's coo_to_csr: entries keep their order inside a row."""
    o = np.argsort(row, kind="stable")
    p = np.zeros(m + 1, np.uint64); p[1:] = np.cumsum(np.bincount(row, minlength=m))
    return (p, np.ascontiguousarray(col[o], np.int32), np.ascontiguousarray(val[o])) + tuple(np.ascontiguousarray(x[o]) for x in more)


def cases(d):
    """(name, kwargs of call_multiple) -- every option alone and in the combinations the entry point supports."""
    k, ku, ki, km = d["k"], d["ku"], d["ki"], d["km"]
    dt = d["B_plain"].dtype
    coo = dict(row=d["row"], col=d["col"], val=d["ratings"], m=d["m"])
    den = dict(Xfull=d["Xfull"], m=d["m"])
    full = dict(B=d["B_full"], k_main=km, k_user=ku, k_item=ki)
    Bp = d["B_plain"].astype(np.float64)
    B1 = np.hstack([Bp, np.ones((d["n"], 1))])
    T_plain = np.linalg.solve(Bp.T @ Bp + 3.3 * np.eye(k), Bp.T).T.astype(dt)           # a lambda that is not the call's
    T_bias = np.linalg.solve(B1.T @ B1 + 3.3 * np.eye(k + 1), B1.T).T.astype(dt)
    out = [
        ("w0 weights scale_lam", dict(coo, B=d["B_plain"], weight=d["weight"], lam=0.6, scale_lam=True)),
        ("w1 weights bias scale_bias_const", dict(coo, B=d["B_plain"], weight=d["weight"], biasB=d["biasB"], glob_mean=3.1, user_bias=True,
                                                   lam=0.6, lam_bias=0.9, scale_lam=True, scale_bias_const=True, scaling_biasA=0.4)),
        ("w2 weights U>m both scalings w_main", dict(coo, **full, Cm=d["C_full"], U=d["U_more"], U_colmeans=d["colmeans"], weight=d["weight"],
                                                      user_bias=True, lam=0.7, lam_bias=1.3, scale_lam=True, scale_lam_sideinfo=True,
                                                      w_main=1.5, w_user=2.5)),
        ("w3 weights sparse U<m bias", dict(coo, **full, Cm=d["C_full"], U_csr=d["U_csr"], weight=d["weight"], user_bias=True, lam=0.7,
                                            lam_bias=1.3, scale_lam=True, w_user=2.5)),
        ("w4 weights nonneg scale_lam", dict(coo, B=d["B_plain"], weight=d["weight"], lam=2.0, scale_lam=True, nonneg=True)),
        ("w5 weights l1 bias scale_lam", dict(coo, B=d["B_plain"], weight=d["weight"], biasB=d["biasB"], glob_mean=3.1, user_bias=True, lam=0.6,
                                    lam_bias=1.1, scale_lam=True, l1_lam=0.05, l1_lam_bias=0.02)),
        ("d0 dense bias scale_lam", dict(den, B=d["B_plain"], biasB=d["biasB"], glob_mean=3.1, user_bias=True, lam=0.6, lam_bias=1.1,
                                         scale_lam=True)),
        ("d1 dense weights w_main", dict(den, B=d["B_plain"], weight=d["Wfull"], glob_mean=-0.4, lam=2.0, w_main=1.5, scale_lam=True)),
        ("d2 dense U<m sideinfo scaling", dict(den, **full, Cm=d["C_full"], U=d["U_less"], biasB=d["biasB"],
                                               glob_mean=3.1, user_bias=True, lam=0.7, lam_bias=1.3, scale_lam_sideinfo=True, w_user=0.8)),
        ("d3 dense TransBtBinvBt", dict(den, B=d["B_plain"], glob_mean=3.1, biasB=d["biasB"], lam=0.6, TransBtBinvBt=T_plain)),
        ("d4 dense TransBtBinvBt bias", dict(den, B=d["B_plain"], glob_mean=3.1, user_bias=True, lam=0.6, lam_bias=0.8, TransBtBinvBt=T_bias)),
        ("d5 dense nonneg", dict(den, B=d["B_plain"], lam=2.0, nonneg=True)),
        ("d6 dense l1 lam_unique", dict(den, B=d["B_plain"], glob_mean=3.1, user_bias=True, lam=0.6, lam_bias=1.1, l1_lam=0.05,
                                         l1_lam_bias=0.02)),
        ("b0 Bi plain", dict(coo, B=d["B_plain"], Bi=d["Bi_plain"], w_implicit=0.7, glob_mean=3.1, lam=0.9)),
        ("b1 Bi U>m bias scale_lam w_main", dict(coo, **full, Cm=d["C_full"], U=d["U_more"], U_colmeans=d["colmeans"], Bi=d["Bi_full"],
                                                  w_implicit=0.7, biasB=d["biasB"], glob_mean=3.1, user_bias=True, lam=0.7, lam_bias=1.3,
                                                  scale_lam=True, w_main=1.5, w_user=2.5)),
        ("b2 Bi weights", dict(coo, B=d["B_plain"], Bi=d["Bi_plain"], w_implicit=1.4, weight=d["weight"], lam=0.9, scale_lam=True)),
        ("b3 Bi dense U<m", dict(den, **full, Cm=d["C_full"], U=d["U_less"], Bi=d["Bi_full"], w_implicit=0.7, glob_mean=3.1, user_bias=True,
                                  lam=0.7, lam_bias=1.3, w_user=0.8)),
        ("b4 Bi nonneg", dict(coo, B=d["B_plain"], Bi=d["Bi_plain"], w_implicit=0.7, lam=2.0, nonneg=True)),
        ("b5 Bi l1 bias", dict(coo, B=d["B_plain"], Bi=d["Bi_plain"], w_implicit=0.7, biasB=d["biasB"], glob_mean=3.1, user_bias=True,
                               lam=0.6, lam_bias=1.1, l1_lam=0.05, l1_lam_bias=0.02)),
        ("b6 Bi sparse U<m", dict(coo, **full, Cm=d["C_full"], U_csr=d["U_csr"], Bi=d["Bi_full"], w_implicit=0.7, glob_mean=-0.4, lam=0.7,
                                  scale_lam=True, w_user=2.5)),
        ("b7 Bi dense weights", dict(den, B=d["B_plain"], Bi=d["Bi_plain"], w_implicit=0.7, weight=d["Wfull"], glob_mean=3.1,
                                     biasB=d["biasB"], user_bias=True, lam=0.8, scale_lam=True)),
    ]
    return out


# Combinations the reference does not solve as the model states (make_golden_new_rows_options.py reports them; the HIP
# entry point returns 2): observation weights of SPARSE X through the block solver -- side information or implicit
# features -- with a global mean or item biases: its right-hand side is  w x' - (w - 1)(glob_mean + biasB)  on the centred
# x' (collective.c:1743-1753), the NA_as_zero form.  And a dense row of NaN that has side information with column means:
# collective_factors_warm centres u, then hands it to collective_factors_cold, which centres it again (:3616, :3337).
def refused_cases(d):
    coo = dict(row=d["row"], col=d["col"], val=d["ratings"], m=d["m"])
    full = dict(B=d["B_full"], k_main=d["km"], k_user=d["ku"], k_item=d["ki"])
    return [
        ("r2 dense NaN row U colmeans", dict(Xfull=d["Xfull"], m=d["m"], **full, Cm=d["C_full"], U=d["U_less"], U_colmeans=d["colmeans"],
                                             lam=0.7)),
        ("r0 weights U glob_mean", dict(coo, **full, Cm=d["C_full"], U=d["U_more"], weight=d["weight"], glob_mean=3.1, lam=0.7)),
        ("r1 weights Bi biasB", dict(coo, B=d["B_plain"], Bi=d["Bi_plain"], weight=d["weight"], biasB=d["biasB"], lam=0.7)),
    ]


def key_of(k, name):
    return "k%d_%s" % (k, name.split()[0])


def call_multiple(lib, dtype, B, m, k, row=None, col=None, val=None, csr=None, Xfull=None, weight=None, Bi=None, w_implicit=1.0,
                  BiTBi=None, TransBtBinvBt=None, TransCtCinvCt=None, Cm=None, U=None, U_csr=None, U_colmeans=None, biasB=None,
                  glob_mean=0.0, user_bias=False, lam=1.0, lam_bias=None, l1_lam=0.0, l1_lam_bias=None, k_main=0, k_user=0, k_item=0,
                  scale_lam=False, scale_lam_sideinfo=False, scale_bias_const=False, scaling_biasA=1.0, w_main=1.0, w_user=1.0,
                  nonneg=False, NA_as_zero_X=False, NA_as_zero_U=False, Ub=None):
    """factors_collective_explicit_multiple with the reference's positional signature; returns (rc, A, biasA or None).  Every
    array goes in as a copy (the reference centres X and U in place)."""
    dtype = np.dtype(dtype).type
    R = C.c_double if dtype is np.float64 else C.c_float
    cp = lambda a, t=dtype: None if a is None else np.array(a, t, order="C", copy=True)
    n = B.shape[0]
    m_u, p = (0, 0) if U is None else U.shape
    ucsr = (None, None, None)
    if U_csr is not None:
        ucsr = (cp(U_csr[0], np.uint64), cp(U_csr[1], np.int32), cp(U_csr[2])); m_u, p = U_csr[3], U_csr[4]
    mm = max(m, m_u)
    A = np.full((mm, k_user + k + k_main), np.nan, dtype)
    biasA = np.full(mm, np.nan, dtype) if user_bias else None
    lam_unique = l1_unique = None
    if lam_bias is not None and lam_bias != lam:
        lam_unique = np.zeros(6, dtype); lam_unique[0] = lam_bias; lam_unique[2] = lam
    if l1_lam_bias is not None and l1_lam_bias != l1_lam:
        l1_unique = np.zeros(6, dtype); l1_unique[0] = l1_lam_bias; l1_unique[2] = l1_lam
    coo = (cp(val), cp(row, np.int32), cp(col, np.int32)) if val is not None else (None, None, None)
    xcsr = (cp(csr[0], np.uint64), cp(csr[1], np.int32), cp(csr[2])) if csr is not None else (None, None, None)
    keep = [cp(U), cp(Cm), cp(biasB), cp(U_colmeans), cp(Xfull), cp(weight), cp(B), cp(Bi), cp(BiTBi), cp(TransBtBinvBt), cp(TransCtCinvCt),
            cp(Ub)]
    Uc, Cc, bBc, cmc, Xf, wc, Bc, Bic, BiGc, TBc, TCc, Ubc = keep
    rc = lib.factors_collective_explicit_multiple(
        _ptr(A), _ptr(biasA), C.c_int(m), _ptr(Uc), C.c_int(m_u), C.c_int(p), C.c_bool(NA_as_zero_U), C.c_bool(NA_as_zero_X),
        C.c_bool(nonneg), None, None, None, C.c_size_t(0), _ptr(ucsr[0]), _ptr(ucsr[1]), _ptr(ucsr[2]),
        _ptr(Ubc), C.c_int(0 if Ub is None else Ub.shape[0]), C.c_int(0 if Ub is None else Ub.shape[1]),
        _ptr(Cc), None, R(glob_mean), _ptr(bBc), _ptr(cmc),
        _ptr(coo[0]), _ptr(coo[1]), _ptr(coo[2]), C.c_size_t(0 if val is None else len(val)),
        _ptr(xcsr[0]), _ptr(xcsr[1]), _ptr(xcsr[2]),
        _ptr(Xf), C.c_int(n), _ptr(wc), _ptr(Bc), _ptr(Bic), C.c_bool(Bi is not None),
        C.c_int(k), C.c_int(k_user), C.c_int(k_item), C.c_int(k_main),
        R(lam), _ptr(lam_unique), R(l1_lam), _ptr(l1_unique), C.c_bool(scale_lam), C.c_bool(scale_lam_sideinfo),
        C.c_bool(scale_bias_const), R(scaling_biasA), R(w_main), R(w_user), R(w_implicit), C.c_int(n), C.c_bool(True),
        None, _ptr(TBc), None, None, _ptr(BiGc), _ptr(TCc), None, None, None, C.c_int(1))
    return rc, A, biasA


def closed_form(kw):
    """Has the case a closed form (no non-negativity, no L1 penalty)?"""
    return not kw.get("nonneg") and not kw.get("l1_lam") and not kw.get("l1_lam_bias")


def normal_equations(kw):
    """The rows of a closed-form case in NumPy float64, from B, C, Bi, the weights and the lambdas: (A, biasA or None)."""
    f = lambda a: None if a is None else np.asarray(a, np.float64)
    B, Cm, Bi, biasB = f(kw["B"]), f(kw.get("Cm")), f(kw.get("Bi")), f(kw.get("biasB"))
    k, ku, ki, km = kw["k"], kw.get("k_user", 0), kw.get("k_item", 0), kw.get("k_main", 0)
    n, m = B.shape[0], kw["m"]
    kk, kc = k + km, ku + k
    ub = 1 if kw.get("user_bias") else 0
    gm = float(kw.get("glob_mean", 0.0))
    lam = float(kw.get("lam", 1.0)); lam_b = float(kw["lam_bias"]) if kw.get("lam_bias") is not None else lam
    if not ub:
        lam_b = lam
    sl, sls = bool(kw.get("scale_lam")), bool(kw.get("scale_lam_sideinfo"))
    sbc = bool(kw.get("scale_bias_const")) and bool(ub)
    if (sl or sls) and sbc:
        lam_b *= float(kw.get("scaling_biasA", 1.0))
    w_main, w_user, w_imp = float(kw.get("w_main", 1.0)), float(kw.get("w_user", 1.0)), float(kw.get("w_implicit", 1.0))
    w_imp_gram = w_imp                                     # the batch driver's matrix keeps the caller's weight
    lam, lam_b, w_user, w_imp = lam / w_main, lam_b / w_main, w_user / w_main, w_imp / w_main
    # per-row observations
    rows = [[] for _ in range(m)]
    if kw.get("Xfull") is not None:
        X, W = f(kw["Xfull"]), f(kw.get("weight"))
        for r in range(m):
            for c in np.nonzero(np.isfinite(X[r]))[0]:
                rows[r].append((c, X[r, c], 1.0 if W is None else W[r, c]))
    else:
        if kw.get("csr") is not None:
            pp, ii, vv = kw["csr"]
            rr = np.repeat(np.arange(m), np.diff(pp.astype(np.int64)))
        else:
            rr, ii, vv = kw["row"], kw["col"], kw["val"]
        ww = kw.get("weight")
        for e in range(len(vv)):
            rows[int(rr[e])].append((int(ii[e]), float(vv[e]), 1.0 if ww is None else float(ww[e])))
    # per-row side information
    U, U_csr = f(kw.get("U")), kw.get("U_csr")
    m_u = U.shape[0] if U is not None else (U_csr[3] if U_csr is not None else 0)
    p = U.shape[1] if U is not None else (U_csr[4] if U_csr is not None else 0)
    if U is not None and kw.get("U_colmeans") is not None:
        U = U - f(kw["U_colmeans"])
    mm = max(m, m_u)
    kt = ku + kk + ub
    A = np.zeros((mm, ku + kk)); bA = np.zeros(mm) if ub else None
    Bx = np.hstack([B[:, ki:], np.ones((n, 1))]) if ub else B[:, ki:]
    BiG = None
    if Bi is not None:
        BiG = f(kw["BiTBi"]) if kw.get("BiTBi") is not None else w_imp_gram * Bi.T @ Bi
        BiG = np.triu(BiG) + np.triu(BiG, 1).T
    T = f(kw.get("TransBtBinvBt"))
    for r in range(mm):
        obs = rows[r] if r < m else []
        J = np.array([o[0] for o in obs], int); x = np.array([o[1] for o in obs]); w = np.array([o[2] for o in obs])
        if len(obs):
            x = x - gm - (biasB[J] if biasB is not None else 0.0)
        side_c = side_u = None                           # attribute ids and values of this row
        if r < m_u:
            if U is not None:
                side_c, side_u = np.arange(p), U[r]
            else:
                s, e = int(U_csr[0][r]), int(U_csr[0][r + 1])
                side_c, side_u = U_csr[1][s:e].astype(int), f(U_csr[2][s:e])
                if e == s:
                    side_c = side_u = None
        cnt = float(w.sum()) if kw.get("weight") is not None else float(len(obs))
        sol = np.zeros(kt)
        if not len(obs) and side_c is None:
            pass
        elif not len(obs) and Bi is None:
            # side information only: (C^T C + (lam / w_user) (p under scale_lam_sideinfo) I) a = C^T u on the k_user + k unknowns,
            # the last of which keeps the unscaled lam / w_user
            Cr = Cm[side_c]
            lc = lam / w_user
            dg = np.full(kc, lc * (len(side_c) if sls else 1.0)); dg[-1] = lc if sls else dg[-1]
            sol[:kc] = np.linalg.solve(Cr.T @ Cr + np.diag(dg), Cr.T @ side_u)
        elif side_c is None and Bi is None:
            # no side information for this row: factors_closed_form on [B | 1]
            if T is not None and kw.get("Xfull") is not None and kw.get("weight") is None and len(obs) == n and m_u == 0:
                sol[ku:] = T.T @ x
            else:
                mult = cnt if (sl or sls) else 1.0
                keep_last = sbc if ub else (sl or sls)     # without a bias the last factor keeps the unscaled lam (collective.c:3789-3799)
                dg = np.full(kk + ub, lam * mult); dg[-1] = (lam_b if ub else lam) * (1.0 if keep_last else mult)
                Bj = Bx[J]
                sol[ku:] = np.linalg.solve((Bj * w[:, None]).T @ Bj + np.diag(dg), Bj.T @ (w * x))
        else:
            M = np.zeros((kt, kt)); rhs = np.zeros(kt)
            mult = 1.0
            if sl or sls:
                mult = cnt if len(obs) else 1.0
                if sls and side_c is not None:
                    mult += len(side_c)
            if side_c is not None:
                Cr = Cm[side_c]
                M[:kc, :kc] += w_user * Cr.T @ Cr; rhs[:kc] += w_user * Cr.T @ side_u
            if len(obs):
                Bj = Bx[J]
                M[ku:, ku:] += (Bj * w[:, None]).T @ Bj; rhs[ku:] += Bj.T @ (w * x)
            if Bi is not None:
                M[ku:ku + kk, ku:ku + kk] += BiG
                if len(obs):
                    rhs[ku:ku + kk] += w_imp * Bi[J].sum(0)
            dg = np.full(kt, lam * mult); dg[-1] = (lam_b if ub else lam) * mult
            sol = np.linalg.solve(M + np.diag(dg), rhs)
        A[r] = sol[:ku + kk]
        if ub:
            bA[r] = sol[-1]
    return A, bA


def load_fixture(dtype):
    return np.load(os.path.join(GOLD, "%s_%s.npz" % (FIXTURE, TAGS[np.dtype(dtype).type])))
