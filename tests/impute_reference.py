"""Imputation of a dense X (impute_X_collective_explicit, cmfrec_hip_impute_dense): the seeded problems, the reference and the
check (helpers, no tests).  tests/test_gpu_impute.py runs the check on the GPU's results, tests/test_impute_cpu.py on a stand-in
kernel (NumPy in the dtype) and on mutations of its result.

The fill kernel on its own (ops.impute_dense).  In place on a row-major X[m, ldx]:
    X[r, c] = isnan(X[r, c]) ? sum_{f < kk} A[r, f] B[c, f] + glob_mean + biasA[r] + biasB[c] : X[r, c]
The images carry leading dimensions and offsets as in dense_reference.py: NaN fills the padding of A, B and the biases (a
kernel that reads outside its operand and masks by multiplying shows it), SENTINEL the padding of X (ldx > n), which must keep
its bits.  The reference is NumPy on the exact upcasts of the dtype-rounded inputs: np.longdouble for float64, float64 for
float32.  Two data sets:

- exact: A, B, the biases and glob_mean in {-2, -1, 1, 2}.  Every partial sum is an integer below 2^24 at kk <= 272, so every
  summation order and the MFMA give the same bits, and an imputed entry must EQUAL the integer result.
- normal: standard normal entries, against the componentwise bound
      |p^ - p| <= gamma_{kk+3} (sum_f |a_f b_f| + |glob_mean| + |biasA_r| + |biasB_c|),     gamma_j = j u / (1 - j u)
  (topn_reference.gamma): kk products and sums in any order plus three additions.  It follows from the arithmetic; no measured
  constant is involved.

In both, every present entry keeps its bits (compared as integers of the dtype's width); the present entries include +-inf,
-0.0, a subnormal and the largest finite value.

Through the handle (cmfrec_hip_newrows_impute, impute_X_collective_explicit): the cases i0-i6 on new_rows_options.problem, one
positional ctypes call that serves the compiled reference and the product alike, and the fixture
tests/golden/g41_impute_{f64,f32}.npz (tests/golden/make_golden_impute.py)."""
import ctypes as C
import functools
import os

import numpy as np

import new_rows_options as nro
from dense_reference import (DATA, DTYPES, SENTINEL, Rejected, _bits, _ints, _name, _ratio, _require, _rng, _wide, image, odd_ld,
                             split_image)
from fp32_reference import _log
from golden_cases import GOLD, TAGS
from topn_reference import gamma

KKS = (1, 3, 4, 5, 50, 64, 65, 272)
SHAPES = ((1, 1), (15, 17), (16, 16), (17, 15), (33, 130), (70, 257))
PATTERNS = ("none", "all", "corners", "row", "col", "lastcol", "random", "payload")
# (biasA: None, "tight" = its own vector (stride 1), "col" = the column of A's image behind the factors (stride lda); biasB)
BIASES = ((None, False), ("tight", True), ("col", True), ("tight", False), (None, True), ("col", False))
OFF_A, OFF_B, OFF_X = 3, 1, 5


@functools.lru_cache(maxsize=None)
def problem(dtype, data, m, n, kk):
    """A [m, kk], B [n, kk], biasA [m], biasB [n], glob_mean in the dtype; the wide product A B^T and |A| |B|^T (float64)."""
    rng = _rng("impute", _name(dtype), data, m, n, kk)
    if data == "exact":
        A, B, bA, bB = _ints(rng, (m, kk)), _ints(rng, (n, kk)), _ints(rng, m), _ints(rng, n)
        gm = -2.0
        if m >= 2:
            A[1] = -A[0]; bA[1] = -bA[0]                    # (rows 0 and 1 differ in every product)
    else:
        A, B, bA, bB = rng.standard_normal((m, kk)), rng.standard_normal((n, kk)), rng.standard_normal(m), rng.standard_normal(n)
        gm = 0.71
    A, B, bA, bB = A.astype(dtype), B.astype(dtype), bA.astype(dtype), bB.astype(dtype)
    gm = float(np.dtype(dtype).type(gm))
    W = _wide(dtype)
    dot = A.astype(W) @ np.ascontiguousarray(B.astype(W).T)
    absdot = np.abs(A.astype(np.float64)) @ np.abs(B.astype(np.float64)).T
    for a in (A, B, bA, bB, dot, absdot):
        a.setflags(write=False)
    return A, B, bA, bB, gm, dot, absdot


def _specials(dtype):
    fi = np.finfo(dtype)
    return np.array([np.inf, -np.inf, -0.0, fi.smallest_subnormal, fi.max], dtype)


def _nan_payloads(dtype):
    """NaNs with the sign bit set, with a non-default payload, and a signalling one."""
    if np.dtype(dtype) == np.float64:
        b = np.array([0xFFF8000000000000, 0x7FF8000000000123, 0xFFF0000000000001, 0x7FFFFFFFFFFFFFFF], np.uint64)
    else:
        b = np.array([0xFFC00000, 0x7FC00123, 0xFF800001, 0x7FFFFFFF], np.uint32)
    return b.view(dtype)


@functools.lru_cache(maxsize=None)
def x_input(dtype, m, n, pattern):
    """X [m, n]: present values (normal, with the special values planted at the start of the first row and, where there is
    room, at five random places) and the NaN of a pattern."""
    rng = _rng("impute-x", _name(dtype), m, n, pattern)
    X = rng.standard_normal((m, n)).astype(dtype)
    sp = _specials(dtype)
    flat = X.reshape(-1)
    flat[:min(len(sp), m * n)] = sp[:m * n]
    if m * n > 40:
        flat[rng.choice(m * n, 5, replace=False)] = sp
    nan = np.zeros((m, n), bool)
    if pattern == "all":
        nan[:] = True
    elif pattern == "corners":
        for r in sorted(set(list(range(0, m, 16)) + list(range(15, m, 16)) + [m - 1])):
            for c in sorted(set(list(range(0, n, 16)) + list(range(15, n, 16)) + [n - 1])):
                nan[r, c] = True
    elif pattern == "row":
        nan[m // 2] = True
    elif pattern == "col":
        nan[:, n // 3] = True
    elif pattern == "lastcol":
        nan[:, n - 1] = True
    elif pattern in ("random", "payload"):
        nan = rng.random((m, n)) < 0.5
        if pattern == "random" and m >= 3:
            nan[2] = False                                  # a row without NaN
    else:
        assert pattern == "none"
    X[nan] = np.nan
    if pattern == "payload":
        pl = _nan_payloads(dtype)
        X[nan] = pl[np.arange(int(nan.sum())) % len(pl)]
    X.setflags(write=False); nan.setflags(write=False)
    return X, nan


def images(dtype, data, shape, kk, pattern, bias, X=None):
    """The X image and the keyword arguments of ops.impute_dense besides it (m, n, kk included): odd leading dimensions larger
    than the widths, non-zero offsets, NaN in the padding of A, B and the biases."""
    m, n = shape
    A, B, bA, bB, gm = problem(dtype, data, m, n, kk)[:5]
    X = x_input(dtype, m, n, pattern)[0] if X is None else X
    how_a, with_b = bias
    lda, ldb, ldx = odd_ld(kk + 1), odd_ld(kk), odd_ld(n)
    Aw = np.full((m, kk + 1), np.nan, dtype); Aw[:, :kk] = A
    if how_a == "col":
        Aw[:, kk] = bA
    kw = dict(m=m, n=n, kk=kk, ldx=ldx, offX=OFF_X, A_img=image(Aw, lda, OFF_A, np.nan, dtype), lda=lda, offA=OFF_A,
              B_img=image(B, ldb, OFF_B, np.nan, dtype), ldb=ldb, offB=OFF_B, glob_mean=gm)
    if how_a == "tight":
        kw["biasA"] = bA.copy()
    elif how_a == "col":
        kw["biasA_col"] = kk
    if with_b:
        kw["biasB"] = bB.copy()
    return image(X, ldx, OFF_X, SENTINEL, dtype), kw


def reference(dtype, data, shape, kk, bias):
    """(predictions [m, n] in the wide precision, bound [m, n] float64; exact: the bound is zero)."""
    m, n = shape
    A, B, bA, bB, gm, dot, absdot = problem(dtype, data, m, n, kk)
    W = _wide(dtype)
    how_a, with_b = bias
    ref = dot + W(gm)
    mag = absdot + abs(gm)
    if how_a:
        ref = ref + bA.astype(W)[:, None]; mag = mag + np.abs(bA.astype(np.float64))[:, None]
    if with_b:
        ref = ref + bB.astype(W)[None, :]; mag = mag + np.abs(bB.astype(np.float64))[None, :]
    return ref, (np.zeros((m, n)) if data == "exact" else gamma(kk + 3, dtype) * mag)


def check(dtype, data, shape, kk, pattern, bias, X_img, X=None, untouched_rows=()):
    """Asserts what the module's docstring states of a result image; `X`: the input if not the pattern's own; `untouched_rows`:
    rows that must come back as they went in, NaN included.  Logs and returns the worst error / bound."""
    m, n = shape
    Xin = x_input(dtype, m, n, pattern)[0] if X is None else X
    nan = np.isnan(Xin)
    what = "impute %s %s %s kk=%d %s bias=%s" % (_name(dtype), data, shape, kk, pattern, bias)
    got, pad_ok = split_image(X_img, m, n, odd_ld(n), OFF_X)
    _require(pad_ok, what + ": padding of X overwritten")
    keep = ~nan
    keep[list(untouched_rows)] = True
    _require(bool(np.array_equal(_bits(got)[keep], _bits(np.ascontiguousarray(Xin))[keep])), what + ": a present entry changed its bits")
    fill = ~keep
    _require(not np.isnan(got[fill]).any(), what + ": a NaN left in place")
    _require(bool(np.isfinite(got[fill]).all()), what + ": non-finite imputed values")
    ref, bound = reference(dtype, data, shape, kk, bias)
    r = _ratio(np.abs(got.astype(ref.dtype) - ref)[fill], bound[fill])
    _log("impute-" + data, r, _name(dtype))
    _require(r <= 1.0, "%s: error / bound = %.3g" % (what, r))
    return r


def standin(dtype, data, shape, kk, pattern, bias, kk_used=None, twice=None, no_biasB=False, swap_rows=None):
    """NumPy in the dtype: [m, n] result.  kk_used: the product over fewer factors; twice: a factor counted twice; no_biasB;
    swap_rows: r -> rows r and r + 1 of A exchanged."""
    m, n = shape
    A, B, bA, bB, gm = problem(dtype, data, m, n, kk)[:5]
    X = x_input(dtype, m, n, pattern)[0]
    T = np.dtype(dtype).type
    A = A.copy()
    if swap_rows is not None:
        A[[swap_rows, swap_rows + 1]] = A[[swap_rows + 1, swap_rows]]
    ku = kk if kk_used is None else kk_used
    P = (A[:, :ku] @ B[:, :ku].T).astype(dtype)
    if twice is not None:
        P = P + np.outer(A[:, twice], B[:, twice]).astype(dtype)
    P = P + T(gm)
    how_a, with_b = bias
    if how_a:
        P = P + bA[:, None]
    if with_b and not no_biasB:
        P = P + bB[None, :]
    return np.where(np.isnan(X), P.astype(dtype), X)


def as_image(dtype, shape, out):
    return image(out, odd_ld(shape[1]), OFF_X, SENTINEL, dtype)


def mutations(dtype, data, shape, kk, pattern, bias):
    """(the stand-in's image, {name: mutated image}) -- those that apply to the case."""
    m, n = shape
    X, nan = x_input(dtype, m, n, pattern)
    args = (dtype, data, shape, kk, pattern, bias)
    good = standin(*args)
    img = lambda out: as_image(dtype, shape, out)
    mut = {}
    if nan.any():
        mut["a dropped term"] = img(standin(*args, kk_used=kk - 1))
        mut["a term counted twice"] = img(standin(*args, twice=kk // 2))
        if bias[1]:
            mut["biasB missing"] = img(standin(*args, no_biasB=True))
        A = problem(dtype, data, m, n, kk)[0]
        rows = [r for r in range(m - 1) if nan[r].any() and nan[r + 1].any() and (A[r] != A[r + 1]).any()]
        if rows:
            mut["rows r and r+1 of A swapped"] = img(standin(*args, swap_rows=rows[0]))
        c = good.copy(); r_, c_ = np.argwhere(nan)[-1]; c[r_, c_] = np.nan
        mut["a NaN left in place"] = img(c)
    present = np.argwhere(~nan & np.isfinite(X))
    if len(present):
        c = good.copy(); r_, c_ = present[len(present) // 2]
        c[r_, c_] = np.nextafter(c[r_, c_], np.dtype(dtype).type(np.inf))
        mut["a present entry one ulp off"] = img(c)
    c = img(good); c[OFF_X + n] = 0.0                       # the first padding element behind row 0
    mut["a SENTINEL overwritten"] = c
    return img(good), mut


# ---- through the handle: cases on new_rows_options.problem ----------------------------------------------------------------

FIXTURE = "g41_impute"
CASE_NAMES = ("i0", "i1", "i2", "i3", "i4", "i5", "i6")


def impute_cases(d):
    """(name, kwargs of call_impute) of the cases i0-i6."""
    dt = d["B_plain"].dtype
    m, n = d["m"], d["n"]
    den = dict(Xfull=d["Xfull"], m=m)
    full = dict(B=d["B_full"], k_main=d["km"], k_user=d["ku"], k_item=d["ki"])
    rng = np.random.default_rng(411 + d["k"])
    Xc = (0.5 * rng.integers(1, 11, (m, n))).astype(dt)
    X5 = Xc.copy(); X5[rng.random((m, n)) < 0.05] = np.nan
    return [
        ("i0 plain", dict(den, B=d["B_plain"], lam=0.6)),
        ("i1 biases glob_mean lam_unique", dict(den, B=d["B_plain"], biasB=d["biasB"], glob_mean=3.1, user_bias=True, lam=0.6, lam_bias=1.1)),
        ("i2 B_full U<m w_main w_user biases", dict(den, **full, Cm=d["C_full"], U=d["U_less"], biasB=d["biasB"], glob_mean=3.1, user_bias=True,
                                                    lam=0.7, lam_bias=1.3, w_main=1.5, w_user=0.8)),
        ("i3 dense weights scale_lam", dict(den, B=d["B_plain"], weight=d["Wfull"], glob_mean=-0.4, lam=2.0, scale_lam=True)),
        ("i4 Bi plain", dict(den, B=d["B_plain"], Bi=d["Bi_plain"], w_implicit=0.7, glob_mean=3.1, lam=0.9)),
        ("i5 complete with 5% NaN", dict(Xfull=X5, m=m, B=d["B_plain"], biasB=d["biasB"], glob_mean=3.1, user_bias=True, lam=0.6)),
        ("i6 no NaN", dict(Xfull=Xc, m=m, B=d["B_plain"], lam=0.6)),
    ]


def key_of(k, name):
    return "X_k%d_%s" % (k, name.split()[0])


def call_impute(lib, dtype, B, m, k, Xfull, weight=None, Bi=None, w_implicit=1.0, Cm=None, U=None, U_colmeans=None, biasB=None,
                glob_mean=0.0, user_bias=False, lam=1.0, lam_bias=None, k_main=0, k_user=0, k_item=0, scale_lam=False,
                scale_lam_sideinfo=False, scale_bias_const=False, scaling_biasA=1.0, w_main=1.0, w_user=1.0, nonneg=False,
                NA_as_zero_U=False, Ub=None):
    """impute_X_collective_explicit with the reference's positional signature (53 parameters); returns (rc, X): a copy of Xfull
    that the call changed in place.  Every other array goes in as a copy too."""
    dtype = np.dtype(dtype).type
    R = C.c_double if dtype is np.float64 else C.c_float
    cp = lambda a, t=dtype: None if a is None else np.array(a, t, order="C", copy=True)
    n = B.shape[0]
    m_u, p = (0, 0) if U is None else U.shape
    lam_unique = None
    if lam_bias is not None and lam_bias != lam:
        lam_unique = np.zeros(6, dtype); lam_unique[0] = lam_bias; lam_unique[2] = lam
    Uc, Cc, bBc, cmc, Xf, wc, Bc, Bic, Ubc = cp(U), cp(Cm), cp(biasB), cp(U_colmeans), cp(Xfull), cp(weight), cp(B), cp(Bi), cp(Ub)
    p_ = nro._ptr
    lib.impute_X_collective_explicit.restype = C.c_int
    rc = lib.impute_X_collective_explicit(
        C.c_int(m), C.c_bool(user_bias), p_(Uc), C.c_int(m_u), C.c_int(p), C.c_bool(NA_as_zero_U), C.c_bool(nonneg),
        None, None, None, C.c_size_t(0), None, None, None,
        p_(Ubc), C.c_int(0 if Ub is None else Ub.shape[0]), C.c_int(0 if Ub is None else Ub.shape[1]),
        p_(Cc), None, R(glob_mean), p_(bBc), p_(cmc),
        p_(Xf), C.c_int(n), p_(wc), p_(Bc), p_(Bic), C.c_bool(Bi is not None),
        C.c_int(k), C.c_int(k_user), C.c_int(k_item), C.c_int(k_main),
        R(lam), p_(lam_unique), R(0.0), None, C.c_bool(scale_lam), C.c_bool(scale_lam_sideinfo),
        C.c_bool(scale_bias_const), R(scaling_biasA), R(w_main), R(w_user), R(w_implicit), C.c_int(n), C.c_bool(True),
        None, None, None, None, None, None, None, None, C.c_int(1))
    return rc, Xf


def load_fixture(dtype):
    return np.load(os.path.join(GOLD, "%s_%s.npz" % (FIXTURE, TAGS[np.dtype(dtype).type])))


def imputed_row_err(got, want, Xin):
    """conftest.row_rel_err over the imputed entries of each row that has any: the present entries of those rows are set to zero
    on both sides (they are compared bit for bit elsewhere)."""
    from conftest import row_rel_err
    nan = np.isnan(Xin)
    rows = nan.any(axis=1)
    if not rows.any():
        return 0.0
    a = np.where(nan, got, 0.0)[rows]; b = np.where(nan, want, 0.0)[rows]
    return row_rel_err(a, b)[0]


def model_of(dtype, k, kw):
    """A cmfrec_amd.CMF that carries the model of a case (what fit() would have left), for NewUsers / CMF.transform."""
    from cmfrec_amd import CMF
    lam, lam_bias = kw.get("lam", 1.0), kw.get("lam_bias")
    lam_arg = lam if (lam_bias is None or lam_bias == lam) else [lam_bias, 0.0, lam, 0.0, 0.0, 0.0]
    ku, ki, km = kw.get("k_user", 0), kw.get("k_item", 0), kw.get("k_main", 0)
    mdl = CMF(k=k, lambda_=lam_arg, user_bias=bool(kw.get("user_bias")), item_bias=kw.get("biasB") is not None,
              add_implicit_features=kw.get("Bi") is not None, scale_lam=bool(kw.get("scale_lam")),
              scale_lam_sideinfo=bool(kw.get("scale_lam_sideinfo")), k_user=ku, k_item=ki, k_main=km, w_main=kw.get("w_main", 1.0),
              w_user=kw.get("w_user", 1.0), w_implicit=kw.get("w_implicit", 1.0), use_float=np.dtype(dtype) == np.float32)
    dt = mdl.dtype_
    mdl.B_ = np.ascontiguousarray(kw["B"], dt)
    mdl.C_ = np.ascontiguousarray(kw["Cm"], dt) if kw.get("Cm") is not None else np.zeros((0, ku + k), dt)
    mdl._U_colmeans = np.zeros(0, dt)
    mdl.glob_mean_ = float(kw.get("glob_mean", 0.0))
    mdl.item_bias_ = np.ascontiguousarray(kw["biasB"], dt) if kw.get("biasB") is not None else np.zeros(0, dt)
    mdl.Bi_ = np.ascontiguousarray(kw["Bi"], dt) if kw.get("Bi") is not None else np.zeros((0, 0), dt)
    mdl._TransBtBinvBt = None
    mdl._TransCtCinvCt = np.zeros((0, 0), dt)
    mdl._scaling_biasA = 1.0
    mdl.is_fitted_ = True
    return mdl


def product_of_factors(dtype, kw, A, bias):
    """(predictions [m, n] in the wide precision from the factors of the batch's rows, bound [m, n] of the kernel's error)."""
    W = _wide(dtype)
    ku, ki = kw.get("k_user", 0), kw.get("k_item", 0)
    m, n = kw["Xfull"].shape
    Af, Bf = np.asarray(A[:m, ku:], dtype), np.asarray(kw["B"][:n, ki:], dtype)
    kk = Af.shape[1]
    gm = np.dtype(dtype).type(kw.get("glob_mean", 0.0))
    ref = Af.astype(W) @ np.ascontiguousarray(Bf.astype(W).T) + W(gm)
    mag = np.abs(Af.astype(np.float64)) @ np.abs(Bf.astype(np.float64)).T + abs(float(gm))
    if bias is not None:
        ref = ref + np.asarray(bias[:m], dtype).astype(W)[:, None]; mag = mag + np.abs(np.asarray(bias[:m], np.float64))[:, None]
    if kw.get("biasB") is not None:
        bB = np.asarray(kw["biasB"], dtype)
        ref = ref + bB.astype(W)[None, :]; mag = mag + np.abs(bB.astype(np.float64))[None, :]
    return ref, gamma(kk + 3, dtype) * mag
