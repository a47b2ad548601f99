"""Predictions for chosen (row, col) pairs (cmfrec_hip_score_pairs, the scorer handle, cmfrec_hip_newrows_predict, the four
predict_X_* names): the seeded problems, the exact values and the check (helpers, no tests).  tests/test_gpu_predict.py runs the
check on the GPU's results, tests/test_predict_cpu.py on a stand-in (NumPy in the dtype) and on mutations of its result.

With a = A[row, :kk], b = B[col, :kk]:
    explicit:  row in [0, m) and col in [0, n):  a . b + biasA[row] + biasB[col] + glob_mean      (a missing bias adds nothing)
               otherwise:                        glob_mean + (biasA[row] if 0 <= row < m) + (biasB[col] if 0 <= col < n)
    implicit:  a . b, otherwise NaN

The exact value of a scored pair is computed in np.longdouble from the inputs as stored (float32 inputs convert exactly).  The
bound follows from the arithmetic, nothing is measured:

    |got - exact| <= (kk + 3) eps(T) (sum_i |a_i b_i| + |biasA| + |biasB| + |glob_mean|)

the any-order summation bound for kk products and three further additions; written with the type's epsilon -- twice its unit
roundoff -- it leaves a factor of two over the bound itself.  A fallback pair must be EXACT: bitwise the host's
glob_mean + biasA + biasB in that order (the sides that apply), or NaN for the implicit model.

Drop-in names: positional ctypes calls that serve the compiled reference and the product alike, and the fixture
tests/golden/g42_predict_{f64,f32}.npz (tests/golden/make_golden_predict.py)."""
import ctypes as C
import functools
import os

import numpy as np

import new_rows_options as nro
from dense_reference import Rejected, _bits, _name, _require, _rng, image
from golden_cases import GOLD, TAGS, new_rows_cases

M, N = 37, 53
KKS = (1, 2, 3, 16, 17, 50, 64, 65, 128, 129, 272)
N_PAIRS = (0, 1, 63, 64, 65, 1000)
# (biasA: None, "tight" = its own vector, "col" = the column of A's image behind the factors (stride lda); biasB)
BIASES = ((None, False), ("tight", True), ("tight", False), (None, True), ("col", True))
FIXTURE = "g42_predict"
LD = np.longdouble


def eps(dtype):
    return float(np.finfo(dtype).eps)


@functools.lru_cache(maxsize=None)
def problem(dtype, kk, m=M, n=N):
    """A [m, kk], B [n, kk], biasA [m], biasB [n], glob_mean in the dtype."""
    rng = _rng("predict", _name(dtype), kk, m, n)
    A, B = rng.standard_normal((m, kk)).astype(dtype), rng.standard_normal((n, kk)).astype(dtype)
    bA, bB = rng.standard_normal(m).astype(dtype), rng.standard_normal(n).astype(dtype)
    gm = float(np.dtype(dtype).type(0.71))
    for a in (A, B, bA, bB):
        a.setflags(write=False)
    return A, B, bA, bB, gm


@functools.lru_cache(maxsize=None)
def pairs(n_pairs, m=M, n=N, negative=True, seed=0):
    """(row, col) int32: uniform pairs -- so that pairs repeat once n_pairs nears m * n -- and, from 32 pairs on, out-of-range
    pairs of every kind: row >= m, col >= n, negative row, negative col, both out."""
    rng = _rng("pairs", n_pairs, m, n, seed)
    row = rng.integers(0, m, n_pairs).astype(np.int32); col = rng.integers(0, n, n_pairs).astype(np.int32)
    if n_pairs >= 32:
        big = np.iinfo(np.int32).max
        out = [(m, 1), (m + 5, n - 1), (big, 0), (0, n), (2, n + 9), (1, big), (m, n), (big, big)]
        if negative:
            out += [(-1, 3), (-big - 1, 0), (4, -1), (m - 1, -7), (-1, -1), (-2, n), (m, -3)]
        where = rng.choice(np.arange(1, n_pairs - 1), len(out), replace=False)
        for w, (r, c) in zip(where, out):
            row[w], col[w] = r, c
        row[n_pairs - 1], col[n_pairs - 1] = row[0], col[0]              # a repeated pair in any case
    row.setflags(write=False); col.setflags(write=False)
    return row, col


def exact(A, B, biasA, biasB, glob_mean, row, col, implicit=False, kk=None):
    """(value, magnitude, scored): per pair the exact prediction in np.longdouble (scored pairs), the sum of magnitudes the
    bound multiplies (float64) and whether the pair is scored; for a fallback pair `value` is the EXACT expected result
    computed in the dtype: glob_mean + biasA + biasB in that order, or NaN (implicit)."""
    dt = A.dtype
    T = dt.type
    m, n = A.shape[0], B.shape[0]
    kk = A.shape[1] if kk is None else kk
    row = np.asarray(row, np.int64); col = np.asarray(col, np.int64)
    ra, cb = (row >= 0) & (row < m), (col >= 0) & (col < n)
    scored = ra & cb
    val = np.zeros(len(row), LD); mag = np.zeros(len(row))
    r, c = row[scored], col[scored]
    prod = A[r, :kk].astype(LD) * B[c, :kk].astype(LD)
    v = prod.sum(1); g = np.abs(prod).astype(np.float64).sum(1)
    if biasA is not None:
        v = v + biasA[r].astype(LD); g = g + np.abs(biasA[r].astype(np.float64))
    if biasB is not None:
        v = v + biasB[c].astype(LD); g = g + np.abs(biasB[c].astype(np.float64))
    if not implicit:
        v = v + LD(T(glob_mean)); g = g + abs(float(T(glob_mean)))
    val[scored] = v; mag[scored] = g
    fb = np.full(len(row), np.nan if implicit else T(glob_mean), dt)
    if not implicit:
        if biasA is not None:
            fb[ra] = fb[ra] + biasA[row[ra]]
        if biasB is not None:
            fb[cb] = fb[cb] + biasB[col[cb]]
    val[~scored] = fb[~scored].astype(LD)
    return val, mag, scored


def check(got, A, B, biasA, biasB, glob_mean, row, col, implicit=False, what="predict", kk=None):
    """Asserts the bound on every scored pair and exactness of every fallback pair; returns the worst error / bound."""
    dt = A.dtype
    got = np.asarray(got)
    _require(got.dtype == dt and got.shape == (len(row),), "%s: result of dtype %s shape %s" % (what, got.dtype, got.shape))
    val, mag, scored = exact(A, B, biasA, biasB, glob_mean, row, col, implicit, kk)
    kk = A.shape[1] if kk is None else kk
    fb_want = val[~scored].astype(dt)
    fb_got = np.ascontiguousarray(got[~scored])
    if implicit:
        _require(bool(np.isnan(fb_got).all()), what + ": a pair out of range that is not NaN")
    else:
        _require(bool(np.array_equal(_bits(fb_got), _bits(np.ascontiguousarray(fb_want)))), what + ": a fallback pair is not exact")
    _require(bool(np.isfinite(got[scored]).all()), what + ": a scored pair is not finite")
    err = np.abs(got[scored].astype(LD) - val[scored]).astype(np.float64)
    bound = (kk + 3) * eps(dt) * mag[scored]
    bad = err > bound
    worst = float((err / np.where(bound > 0, bound, 1.0)).max()) if len(err) else 0.0
    _require(not bad.any(), "%s: %d of %d pairs beyond the bound, worst error / bound = %.3g" % (what, int(bad.sum()), len(err), worst))
    return worst


def standin(A, B, biasA, biasB, glob_mean, row, col, implicit=False, kk_used=None, order=None, drop=None):
    """NumPy in the dtype.  kk_used: the product over fewer factors; order: a permutation of the factors (another summation
    order); drop: the index of a product left out."""
    dt = A.dtype
    T = dt.type
    m, n = A.shape[0], B.shape[0]
    row = np.asarray(row, np.int64); col = np.asarray(col, np.int64)
    ra, cb = (row >= 0) & (row < m), (col >= 0) & (col < n)
    ok = ra & cb
    idx = np.arange(A.shape[1] if kk_used is None else kk_used)
    if order is not None:
        idx = np.asarray(order)
    if drop is not None:
        idx = idx[idx != drop]
    out = np.empty(len(row), dt)
    acc = np.zeros(int(ok.sum()), dt)
    for f in idx:
        acc = (acc + A[row[ok], f] * B[col[ok], f]).astype(dt)
    if biasA is not None:
        acc = acc + biasA[row[ok]]
    if biasB is not None:
        acc = acc + biasB[col[ok]]
    if not implicit:
        acc = acc + T(glob_mean)
    out[ok] = acc
    fb = np.full(len(row), np.nan if implicit else T(glob_mean), dt)
    if not implicit:
        if biasA is not None:
            fb[ra] = fb[ra] + biasA[row[ra]]
        if biasB is not None:
            fb[cb] = fb[cb] + biasB[col[cb]]
    out[~ok] = fb[~ok]
    return out


def images(dtype, kk, bias, aligned):
    """Keyword arguments of ops.score_pairs besides row / col: aligned: offsets 0 and leading dimensions that keep every row on a
    16-byte boundary (the 16-byte loads); else offset 1 and odd leading dimensions (element-wide loads).  NaN fills the padding."""
    A, B, bA, bB, gm = problem(dtype, kk)
    v = 16 // np.dtype(dtype).itemsize
    how_a, with_b = bias
    if aligned:
        lda = ldb = (kk + 1 + v - 1) // v * v
        off = 0
    else:
        lda = kk + 2 if kk % 2 else kk + 1
        ldb = lda + 2
        off = 1
    Aw = np.full((M, kk + 1), np.nan, dtype); Aw[:, :kk] = A
    if how_a == "col":
        Aw[:, kk] = bA
    kw = dict(m=M, n=N, kk=kk, A_img=image(Aw, lda, off, np.nan, dtype), lda=lda, offA=off, B_img=image(B, ldb, off, np.nan, dtype), ldb=ldb,
              offB=off, glob_mean=gm)
    if how_a == "tight":
        kw["biasA"] = bA.copy()
    elif how_a == "col":
        kw["biasA_col"] = kk
    if with_b:
        kw["biasB"] = bB.copy()
    return kw


def biases_of(dtype, kk, bias):
    A, B, bA, bB, gm = problem(dtype, kk)
    return (bA if bias[0] else None), (bB if bias[1] else None)


# ---- the drop-in names ------------------------------------------------------------------------------------------------------

OLD_K, OLD_KU, OLD_KI = 5, 2, 1
OLD_KMS = (0, 2)
OLD_PAIRS = 300
NEW_EXPLICIT = ("w1", "d2", "b1")
NEW_IMPLICIT = "i1"
NEW_PAIRS = 200


@functools.lru_cache(maxsize=None)
def old_problem(dtype, k_main):
    """A [M, k_user + k + k_main], B [N, k_item + k + k_main], the biases, glob_mean; 300 pairs, some of them with row >= m or
    col >= n (no negative index: the reference reads out of bounds for one)."""
    rng = _rng("predict-old", _name(dtype), k_main)
    A = rng.standard_normal((M, OLD_KU + OLD_K + k_main)).astype(dtype)
    B = rng.standard_normal((N, OLD_KI + OLD_K + k_main)).astype(dtype)
    bA, bB = rng.standard_normal(M).astype(dtype), rng.standard_normal(N).astype(dtype)
    row, col = pairs(OLD_PAIRS, M, N, negative=False, seed=1 + k_main)
    return dict(A=A, B=B, biasA=bA, biasB=bB, glob_mean=float(np.dtype(dtype).type(3.1)), k=OLD_K, k_user=OLD_KU, k_item=OLD_KI,
                k_main=k_main, row=row, col=col)


def call_old(lib, dtype, d, implicit):
    """predict_X_old_collective_explicit / _implicit with the reference's positional signature; returns (rc, predicted)."""
    dtype = np.dtype(dtype).type
    R = C.c_double if dtype is np.float64 else C.c_float
    cp = lambda a, t=dtype: np.array(a, t, order="C", copy=True)
    row, col = cp(d["row"], np.int32), cp(d["col"], np.int32)
    out = np.full(len(row), -777.0, dtype)
    A, B = cp(d["A"]), cp(d["B"])
    p_ = nro._ptr
    ks = (C.c_int(d["k"]), C.c_int(d["k_user"]), C.c_int(d["k_item"]), C.c_int(d["k_main"]))
    if implicit:
        f = lib.predict_X_old_collective_implicit
        f.restype = C.c_int
        rc = f(p_(row), p_(col), p_(out), C.c_size_t(len(row)), p_(A), p_(B), *ks, C.c_int(A.shape[0]), C.c_int(B.shape[0]), C.c_int(1))
    else:
        bA, bB = cp(d["biasA"]), cp(d["biasB"])
        f = lib.predict_X_old_collective_explicit
        f.restype = C.c_int
        rc = f(p_(row), p_(col), p_(out), C.c_size_t(len(row)), p_(A), p_(bA), p_(B), p_(bB), R(d["glob_mean"]), *ks,
               C.c_int(A.shape[0]), C.c_int(B.shape[0]), C.c_int(1))
    return rc, out


def old_operands(d, implicit, kk=None):
    """The arguments of exact / check / standin for an old_problem: the scored columns, the biases, glob_mean."""
    ku, ki = d["k_user"], d["k_item"]
    A, B = np.ascontiguousarray(d["A"][:, ku:]), np.ascontiguousarray(d["B"][:, ki:])
    if implicit:
        return A, B, None, None, 0.0
    return A, B, d["biasA"], d["biasB"], d["glob_mean"]


def new_cases(dtype, k):
    """(name, kind, kwargs of call_new) of the predict_X_new cases: three of new_rows_options.cases, one implicit case of
    golden_cases.new_rows_cases."""
    d = nro.problem(dtype, k)
    out = [(name, "explicit", dict(kw, k=k)) for name, kw in nro.cases(d) if name.split()[0] in NEW_EXPLICIT]
    out += [(name, kind, kw) for name, kind, kw in new_rows_cases(d) if kind == "implicit" and name.split()[0] == NEW_IMPLICIT]
    assert len(out) == len(NEW_EXPLICIT) + 1
    return out


def new_pairs(kw):
    """200 pairs for a predict_X_new case: rows of the batch [0, max(m, m_u)), items [0, n), some beyond either (no negative)."""
    m_u = kw["U"].shape[0] if kw.get("U") is not None else 0
    return pairs(NEW_PAIRS, max(kw["m"], m_u), kw["B"].shape[0], negative=False, seed=7)


def key_of(k, name):
    return "new_k%d_%s" % (k, name.split()[0])


def call_new(lib, dtype, kind, prow, pcol, B, m, k, row=None, col=None, val=None, Xfull=None, weight=None, Bi=None, w_implicit=1.0,
             Cm=None, U=None, U_colmeans=None, biasB=None, glob_mean=0.0, user_bias=False, lam=1.0, lam_bias=None, k_main=0, k_user=0,
             k_item=0, scale_lam=False, scale_lam_sideinfo=False, scale_bias_const=False, scaling_biasA=1.0, w_main=1.0, w_user=1.0,
             alpha=1.0, w_main_multiplier=1.0, NA_as_zero_X=False):
    """predict_X_new_collective_explicit / _implicit with the reference's positional signatures; returns (rc, predicted).  Every
    array goes in as a copy; predicted starts as -777."""
    dtype = np.dtype(dtype).type
    R = C.c_double if dtype is np.float64 else C.c_float
    cp = lambda a, t=dtype: None if a is None else np.array(a, t, order="C", copy=True)
    p_ = nro._ptr
    n = B.shape[0]
    m_u, p = (0, 0) if U is None else U.shape
    prow, pcol = cp(prow, np.int32), cp(pcol, np.int32)
    out = np.full(len(prow), -777.0, dtype)
    coo = (cp(val), cp(row, np.int32), cp(col, np.int32)) if val is not None else (None, None, None)
    Uc, Cc, bBc, cmc, Xf, wc, Bc, Bic = cp(U), cp(Cm), cp(biasB), cp(U_colmeans), cp(Xfull), cp(weight), cp(B), cp(Bi)
    ks = (C.c_int(k), C.c_int(k_user), C.c_int(k_item), C.c_int(k_main))
    head = (C.c_int(m), p_(prow), p_(pcol), p_(out), C.c_size_t(len(prow)), C.c_int(1))
    sparse_u = (None, None, None, C.c_size_t(0), None, None, None)
    x = (p_(coo[0]), p_(coo[1]), p_(coo[2]), C.c_size_t(0 if val is None else len(val)), None, None, None)
    if kind == "implicit":
        f = lib.predict_X_new_collective_implicit
        f.restype = C.c_int
        rc = f(*head, p_(Uc), C.c_int(m_u), C.c_int(p), C.c_bool(False), C.c_bool(False), *sparse_u, *x, p_(Bc), C.c_int(n), p_(Cc), p_(cmc),
               *ks, R(lam), R(0.0), R(alpha), R(w_main), R(w_user), R(w_main_multiplier), C.c_bool(False), None, None, None, None)
        return rc, out
    lam_unique = None
    if lam_bias is not None and lam_bias != lam:
        lam_unique = np.zeros(6, dtype); lam_unique[0] = lam_bias; lam_unique[2] = lam
    f = lib.predict_X_new_collective_explicit
    f.restype = C.c_int
    rc = f(*head, C.c_bool(user_bias), p_(Uc), C.c_int(m_u), C.c_int(p), C.c_bool(False), C.c_bool(NA_as_zero_X), C.c_bool(False), *sparse_u,
           None, C.c_int(0), C.c_int(0), p_(Cc), None, R(glob_mean), p_(bBc), p_(cmc), *x,
           p_(Xf), C.c_int(n), p_(wc), p_(Bc), p_(Bic), C.c_bool(Bi is not None), *ks,
           R(lam), p_(lam_unique), R(0.0), None, C.c_bool(scale_lam), C.c_bool(scale_lam_sideinfo), C.c_bool(scale_bias_const),
           R(scaling_biasA), R(w_main), R(w_user), R(w_implicit), C.c_int(n), C.c_bool(True),
           None, None, None, None, None, None, None, None, None)
    return rc, out


def reference_prediction(dtype, k, name, kind, kw, prow, pcol, recorded):
    """What the reference predicts for a predict_X_new case under the model's definition of a prediction, from recorded data
    only.  Its predict_multiple sums over k factors and leaves the k_main ones out (test_predict_cpu.py::test_reference_facts),
    so for a case with k_main > 0 the recorded values lack  sum_{k <= f < k + k_main} a_f b_f  of every scored pair; that part
    is added here from the reference's own recorded factors of the same case (fixtures g40 / g11: the A its
    factors_collective_*_multiple returned).  With k_main = 0 the recorded values are returned as they are."""
    km = kw.get("k_main", 0)
    if km == 0:
        return recorded
    from golden_cases import load
    if kind == "implicit":
        A = load("g11_new_rows", dtype)["A_k%d_%s" % (k, name.split()[0])]
    else:
        A = nro.load_fixture(dtype)["A_" + nro.key_of(k, name)]
    ku, ki = kw.get("k_user", 0), kw.get("k_item", 0)
    B = kw["B"]
    r, c = np.asarray(prow, np.int64), np.asarray(pcol, np.int64)
    ok = (r >= 0) & (r < A.shape[0]) & (c >= 0) & (c < B.shape[0])
    out = np.array(recorded, np.float64)
    out[ok] += (A[r[ok], ku + k:ku + k + km].astype(np.float64) * B[c[ok], ki + k:ki + k + km].astype(np.float64)).sum(1)
    return out


def load_fixture(dtype):
    return np.load(os.path.join(GOLD, "%s_%s.npz" % (FIXTURE, TAGS[np.dtype(dtype).type])))
