"""New rows of missing-as-zero models (NA_as_zero_X / NA_as_zero_U of factors_collective_explicit_multiple): the seeded problem,
the named cases, the float64 normal equations of the model in NumPy, and the call through the new-rows handle
(cmfrec_hip_newrows_*), which is where the product takes the two options.

The model, per row: every one of the n cells counts, an absent one as a zero of weight 1; the target of cell j is
x_j - glob_mean - biasB_j; under scale_lam the lambda multiplier is n without weights and sum(w) + (n - nnz) with them; under
NA_as_zero_U an absent attribute is a zero minus its column mean.

Fixture: tests/golden/g43_new_rows_naz_{f64,f32}.npz (tests/golden/make_golden_new_rows_naz.py)."""
import ctypes as C
import os

import numpy as np

import new_rows_options as nro
from golden_cases import GOLD, TAGS

KS = (6, 50)
FIXTURE = "g43_new_rows_naz"
TOL32, TOL64 = nro.TOL32, nro.TOL64


def problem(dtype, k):
    """new_rows_options.problem (n = 70, m = 48, p = 5) + side information on exactly the batch's rows: dense, and sparse with
    a row without attributes, a row with one and a row with all of them."""
    d = nro.problem(dtype, k)
    rng = np.random.default_rng(431 + k)
    m, p = d["m"], d["p"]
    d["U_eq"] = rng.standard_normal((m, p)).astype(dtype)
    S = np.where(rng.random((m, p)) < 0.45, rng.standard_normal((m, p)), np.nan)
    S[2] = np.nan; S[6] = np.nan; S[6, 3] = 0.7; S[8] = rng.standard_normal(p)
    S[3] = np.nan; S[3, :2] = (0.4, -1.1)                       # row 3 has no entries in X: attributes only
    d["U_csr_eq"] = nro.dense_to_csr(S.astype(dtype))
    d["zeros_n"] = np.zeros(d["n"], dtype)
    # weights without the row that new_rows_options.problem scales by 1e3 (the zero weight stays): with that row and lam = 0.6 the
    # reference's own float32 rows of z2 lie 2.7e-4 from its float64 rows at k = 50 -- no fixture could hold TOL32 / 4 there.  z8
    # keeps the scaled row: under scale_lam its lambda grows with the weights.
    w = np.array(d["weight"], np.float64)
    w[d["row"] == 9] /= 1e3
    d["weight_mild"] = w.astype(dtype)
    return d


def cases(d):
    """(name, kwargs of new_rows_options.call_multiple): the cases on which the compiled reference agrees with the model."""
    coo = dict(row=d["row"], col=d["col"], val=d["ratings"], m=d["m"])
    full = dict(B=d["B_full"], k_main=d["km"], k_user=d["ku"], k_item=d["ki"])
    X = dict(NA_as_zero_X=True)
    return [
        ("z0 X alone", dict(coo, **X, B=d["B_plain"], lam=0.8)),
        ("z1 X biasB mean bias", dict(coo, **X, B=d["B_plain"], biasB=d["biasB"], glob_mean=3.1, user_bias=True, lam=0.6, lam_bias=1.1)),
        ("z2 X weights biasB mean bias", dict(coo, **X, B=d["B_plain"], weight=d["weight_mild"], biasB=d["biasB"], glob_mean=3.1,
                                              user_bias=True, lam=0.6, lam_bias=1.1)),
        ("z3 X dense U k_* colmeans w_user", dict(coo, **X, **full, Cm=d["C_full"], U=d["U_eq"], U_colmeans=d["colmeans"], lam=0.7,
                                                  w_user=2.5)),
        ("z4 X and U sparse colmeans", dict(coo, **X, NA_as_zero_U=True, **full, Cm=d["C_full"], U_csr=d["U_csr_eq"],
                                            U_colmeans=d["colmeans"], biasB=d["biasB"], glob_mean=3.1, user_bias=True, lam=0.7, lam_bias=1.3,
                                            w_user=2.5)),
        ("z5 U alone sparse X ordinary", dict(coo, NA_as_zero_U=True, **full, Cm=d["C_full"], U_csr=d["U_csr_eq"], U_colmeans=d["colmeans"],
                                              biasB=d["biasB"], glob_mean=3.1, user_bias=True, lam=0.7, lam_bias=1.3, w_user=2.5)),
        ("z6 X scale_lam bias", dict(coo, **X, B=d["B_plain"], biasB=d["biasB"], glob_mean=3.1, user_bias=True, lam=0.01, lam_bias=0.02,
                                     scale_lam=True)),
        ("z7 X scale_lam no bias", dict(coo, **X, B=d["B_plain"], biasB=d["biasB"], glob_mean=3.1, lam=0.01, scale_lam=True)),
        ("z8 X scale_lam no bias weights", dict(coo, **X, B=d["B_plain"], weight=d["weight"], biasB=d["biasB"], glob_mean=3.1, lam=0.01,
                                                scale_lam=True)),
        ("z9 X mean zero biasB", dict(coo, **X, B=d["B_plain"], biasB=d["zeros_n"], glob_mean=3.1, lam=0.8)),
    ]


# Left out of the fixture, with the reason; the product is held to normal_equations alone on them (tests/test_gpu_naz_new_rows.py).
#  * glob_mean != 0 with biasB == NULL and BtXbias == NULL: the reference sums n_max rows of B starting at row n for its constant
#    (collective.c:11055-11060), a read past the matrix; its rows are off by a relative 9.4 on this problem.  z9 is the same model
#    with an array of zeros for biasB, which the reference gets right.
def numpy_only_cases(d):
    coo = dict(row=d["row"], col=d["col"], val=d["ratings"], m=d["m"])
    return [("n0 X mean without biasB", dict(coo, NA_as_zero_X=True, B=d["B_plain"], glob_mean=3.1, lam=0.8))]


def key_of(k, name):
    return nro.key_of(k, name)


def normal_equations(kw):
    """The rows of a case in NumPy float64: (A, biasA or None).  kw: the kwargs of call_multiple + k."""
    f = lambda a: None if a is None else np.asarray(a, np.float64)
    B, Cm, biasB = f(kw["B"]), f(kw.get("Cm")), f(kw.get("biasB"))
    k, ku, ki, km = kw["k"], kw.get("k_user", 0), kw.get("k_item", 0), kw.get("k_main", 0)
    n, m = B.shape[0], kw["m"]
    kk, kc = k + km, ku + k
    ub = 1 if kw.get("user_bias") else 0
    gm = float(kw.get("glob_mean", 0.0))
    lam = float(kw.get("lam", 1.0)); lam_b = float(kw["lam_bias"]) if (ub and kw.get("lam_bias") is not None) else lam
    sl, sls = bool(kw.get("scale_lam")), bool(kw.get("scale_lam_sideinfo"))
    w_main, w_user = float(kw.get("w_main", 1.0)), float(kw.get("w_user", 1.0))
    lam, lam_b, w_user = lam / w_main, lam_b / w_main, w_user / w_main
    nazX, nazU = bool(kw.get("NA_as_zero_X")), bool(kw.get("NA_as_zero_U"))
    weighted = kw.get("weight") is not None
    rows = [[] for _ in range(m)]
    if kw.get("csr") is not None:
        pp, ii, vv = kw["csr"]
        rr = np.repeat(np.arange(m), np.diff(np.asarray(pp).astype(np.int64)))
    else:
        rr, ii, vv = kw["row"], kw["col"], kw["val"]
    ww = kw.get("weight")
    for e in range(len(vv)):
        rows[int(rr[e])].append((int(ii[e]), float(vv[e]), 1.0 if ww is None else float(ww[e])))
    U, U_csr = f(kw.get("U")), kw.get("U_csr")
    m_u = U.shape[0] if U is not None else (U_csr[3] if U_csr is not None else 0)
    p = U.shape[1] if U is not None else (U_csr[4] if U_csr is not None else 0)
    means = f(kw["U_colmeans"]) if kw.get("U_colmeans") is not None else np.zeros(p)
    mm = max(m, m_u)
    kx = kk + ub; kt = ku + kx
    A = np.zeros((mm, ku + kk)); bA = np.zeros(mm) if ub else None
    Bx = np.hstack([B[:, ki:], np.ones((n, 1))]) if ub else B[:, ki:]
    shift = gm + (biasB if biasB is not None else np.zeros(n))
    for r in range(mm):
        obs = rows[r] if r < m else []
        J = np.array([o[0] for o in obs], int); x = np.array([o[1] for o in obs]); w = np.array([o[2] for o in obs])
        side = r < m_u and p > 0
        M = np.zeros((kt, kt)); rhs = np.zeros(kt)
        Bj = Bx[J]
        if nazX:
            M[ku:, ku:] = Bx.T @ Bx + (Bj * (w - 1.0)[:, None]).T @ Bj
            rhs[ku:] = Bj.T @ (w * x - (w - 1.0) * shift[J]) - Bx.T @ shift
            cells = (w.sum() + (n - len(obs))) if weighted else float(n)
        else:
            M[ku:, ku:] = (Bj * w[:, None]).T @ Bj
            rhs[ku:] = Bj.T @ (w * (x - shift[J]))
            cells = (w.sum() if weighted else float(len(obs))) if len(obs) else 1.0
        if side:
            if U is not None:
                Cr, u = Cm, U[r] - means
            else:
                s, e = int(U_csr[0][r]), int(U_csr[0][r + 1])
                cols, vals = np.asarray(U_csr[1][s:e]).astype(int), f(U_csr[2][s:e])
                if nazU:
                    u = np.zeros(p); u[cols] = vals; u -= means; Cr = Cm
                else:
                    Cr, u = Cm[cols], vals
            M[:kc, :kc] += w_user * Cr.T @ Cr; rhs[:kc] += w_user * Cr.T @ u
        sol = np.zeros(kt)
        if not nazX and not len(obs):
            if side:                                        # attributes only: w_user C^T C + lam on the k_user + k unknowns, the rest zero
                sol[:kc] = np.linalg.solve(M[:kc, :kc] + lam * np.eye(kc), rhs[:kc])
        else:
            mult = cells if (sl or sls) else 1.0
            if sls and side:
                mult += p
            dg = np.full(kt, lam * mult)
            # rows without side information and without a bias: the last unknown keeps the unscaled lambda (new_rows_options.normal_equations)
            dg[-1] = lam if (not side and not ub and (sl or sls)) else lam_b * mult
            sol = np.linalg.solve(M + np.diag(dg), rhs)
        A[r] = sol[:ku + kk]
        if ub:
            bA[r] = sol[-1]
    return A, bA


def load_fixture(dtype):
    return np.load(os.path.join(GOLD, "%s_%s.npz" % (FIXTURE, TAGS[np.dtype(dtype).type])))


# ---- the product: the new-rows handle ---------------------------------------------------------
class Handle:
    """cmfrec_hip_newrows_create_ex on the model half of a case's kwargs; .factors(**batch half) -> (rc, A, biasA).  `error` after a
    failed create: (code, message)."""

    def __init__(self, dtype, k, B, Cm=None, U_colmeans=None, biasB=None, glob_mean=0.0, user_bias=False, lam=1.0, lam_bias=None,
                 l1_lam=0.0, k_main=0, k_user=0, k_item=0, scale_lam=False, scale_lam_sideinfo=False, scale_bias_const=False,
                 scaling_biasA=1.0, w_main=1.0, w_user=1.0, nonneg=False, NA_as_zero_X=False, NA_as_zero_U=False, Bi=None, implicit=False,
                 **batch):
        from cmfrec_amd import _lib
        self.dtype = dt = np.dtype(dtype).type
        self.lib = lib = _lib.load(dt)
        self._lib = _lib
        self.batch_kw = batch
        mx = _lib.newrows_model_ex_mirror(dt)()
        mdl = mx.base
        keep = []

        def arr(a):
            a = np.ascontiguousarray(a, dt); keep.append(a)
            return a.ctypes.data

        mdl.implicit = int(implicit)
        mdl.n = mdl.n_max = B.shape[0]; mdl.include_all_X = 1
        mdl.p = 0 if Cm is None else Cm.shape[0]
        mdl.user_bias = int(user_bias); mdl.add_implicit_features = int(Bi is not None)
        mdl.k = k; mdl.k_user = k_user; mdl.k_item = k_item; mdl.k_main = k_main
        mdl.scale_lam = int(scale_lam); mdl.scale_lam_sideinfo = int(scale_lam_sideinfo); mdl.scale_bias_const = int(scale_bias_const)
        mdl.nonneg = int(nonneg)
        mdl.glob_mean = glob_mean; mdl.lam = lam; mdl.l1_lam = l1_lam; mdl.scaling_biasA = scaling_biasA
        mdl.w_main = w_main; mdl.w_user = w_user; mdl.w_implicit = 1.0; mdl.alpha = 1.0; mdl.w_main_multiplier = 1.0
        mdl.B = arr(B)
        if Cm is not None:
            mdl.C = arr(Cm)
        if U_colmeans is not None:
            mdl.U_colmeans = arr(U_colmeans)
        if biasB is not None:
            mdl.biasB = arr(biasB)
        if Bi is not None:
            mdl.Bi = arr(Bi)
        if lam_bias is not None and lam_bias != lam:
            lu = np.zeros(6, dt); lu[0] = lam_bias; lu[2] = lam
            mdl.lam_unique = arr(lu)
        mx.NA_as_zero_X = int(NA_as_zero_X); mx.NA_as_zero_U = int(NA_as_zero_U)
        self.width = k_user + k + k_main
        self.user_bias = bool(user_bias)
        h = lib.cmfrec_hip_newrows_create_ex(C.byref(mx), C.c_int(-1))
        self.handle = C.c_void_p(h) if h else None
        self.error = None if h else (lib.cmfrec_hip_last_error_code(), lib.cmfrec_hip_last_error().decode())

    def batch(self, m, row=None, col=None, val=None, csr=None, Xfull=None, weight=None, U=None, U_csr=None):
        """(the C struct, the arrays it points into, the rows of the result)"""
        dt = self.dtype
        s = self._lib.NewRowsBatch()
        keep = []

        def arr(a, t=dt):
            a = np.ascontiguousarray(a, t); keep.append(a)
            return a.ctypes.data

        s.m = m
        if val is not None:
            s.X = arr(val); s.ixA = arr(row, np.int32); s.ixB = arr(col, np.int32); s.nnz = len(val)
        if csr is not None:
            s.Xcsr_p = arr(csr[0], np.uint64); s.Xcsr_i = arr(csr[1], np.int32); s.Xcsr = arr(csr[2])
        if Xfull is not None:
            s.Xfull = arr(Xfull)
        if weight is not None:
            s.weight = arr(weight)
        m_u = 0
        if U is not None:
            s.U = arr(U); m_u = U.shape[0]
        if U_csr is not None:
            s.U_csr_p = arr(U_csr[0], np.uint64); s.U_csr_i = arr(U_csr[1], np.int32); s.U_csr = arr(U_csr[2]); m_u = U_csr[3]
        s.m_u = m_u
        return s, keep, max(m, m_u)

    def factors(self, **kw):
        s, keep, rows = self.batch(**(kw or self.batch_kw))
        A = np.full((rows, self.width), np.nan, self.dtype)
        bA = np.full(rows, np.nan, self.dtype) if self.user_bias else None
        rc = self.lib.cmfrec_hip_newrows_factors(self.handle, C.byref(s), self._lib.ptr(A), self._lib.ptr(bA))
        return rc, A, bA

    def impute(self, **kw):
        """cmfrec_hip_newrows_impute of a dense batch: (rc, Xout, A, biasA)."""
        s, keep, rows = self.batch(**kw)
        Xout = np.full(np.shape(kw["Xfull"]), np.nan, self.dtype)
        A = np.full((rows, self.width), np.nan, self.dtype)
        bA = np.full(rows, np.nan, self.dtype) if self.user_bias else None
        rc = self.lib.cmfrec_hip_newrows_impute(self.handle, C.byref(s), self._lib.ptr(Xout), self._lib.ptr(A), self._lib.ptr(bA))
        return rc, Xout, A, bA

    def launch_waves(self):
        """The wavefronts of the last launch of the right-hand-side kernel (what CMFREC_HIP_NAZ_WAVES caps)."""
        w = C.c_int(-1)
        assert self.lib.cmfrec_hip_newrows_naz_launch_waves(self.handle, C.byref(w)) == 0
        return w.value

    def message(self):
        return self.lib.cmfrec_hip_last_error().decode()

    def close(self):
        if self.handle:
            self.lib.cmfrec_hip_newrows_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def hip(dtype, k, **kw):
    """One case through a handle of its own: (A, biasA)."""
    with Handle(dtype, k, **kw) as h:
        assert h.handle, h.error
        rc, A, bA = h.factors()
        assert rc == 0, (rc, h.message())
    return A, bA
