"""Predictions for chosen pairs on the GPU, held to the exact values of tests/predict_reference.py: the kernel alone
(ops.score_pairs), the scorer handle, the four predict_X_* names against the recorded reference (fixture g42) and the new-rows
handle.  The shapes are the smallest at which the kernel takes each of its paths: every group width (1 .. 64 lanes per pair), the
single-piece and the looping case, the padded tail, both load widths, part-filled steps and more than one wavefront."""
import ctypes as C

import numpy as np
import pytest

import impute_reference as ir
import new_rows_options as nro
import predict_reference as pr
from dense_reference import DTYPES, _bits, _name

pytestmark = pytest.mark.gpu
IDS = [_name(d) for d in DTYPES]


def _same_bits(a, b):
    return a.dtype == b.dtype and np.array_equal(_bits(np.ascontiguousarray(a)), _bits(np.ascontiguousarray(b)))


def _score(dtype, kk, bias, aligned, row, col, implicit=False):
    from cmfrec_amd import ops
    kw = pr.images(dtype, kk, bias, aligned)
    if implicit:
        kw["glob_mean"] = 0.0
    return ops.score_pairs(row=row, col=col, implicit=implicit, **kw)


def _check(dtype, kk, bias, got, row, col, implicit=False, what=""):
    A, B, bA, bB, gm = pr.problem(dtype, kk)
    bA, bB = pr.biases_of(dtype, kk, bias)
    r = pr.check(got, A, B, bA, bB, 0.0 if implicit else gm, row, col, implicit=implicit, what="%s %s kk=%d bias=%s %s" % (
        _name(dtype), "implicit" if implicit else "explicit", kk, bias, what))
    print("score_pairs %s kk=%d n_pairs=%d bias=%s implicit=%s %s: error / bound %.3g" % (_name(dtype), kk, len(row), bias, implicit, what, r))
    return r


# ---- 1. the kernel alone -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kk", pr.KKS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_kernel(dtype, kk):
    for n_pairs in pr.N_PAIRS:
        row, col = pr.pairs(n_pairs)
        for bias in (pr.BIASES if n_pairs == 1000 else pr.BIASES[1:2]):
            wide = _score(dtype, kk, bias, True, row, col)
            narrow = _score(dtype, kk, bias, False, row, col)
            _check(dtype, kk, bias, wide, row, col, what="aligned")
            assert _same_bits(wide, narrow), (kk, n_pairs, bias, "the load width changed the bits")
        # implicit rule: no bias, NaN out of range
        wide = _score(dtype, kk, (None, False), True, row, col, implicit=True)
        narrow = _score(dtype, kk, (None, False), False, row, col, implicit=True)
        _check(dtype, kk, (None, False), wide, row, col, implicit=True)
        assert _same_bits(wide, narrow), (kk, n_pairs, "implicit: the load width changed the bits")
    # the same call twice; a permutation of the pairs
    row, col = pr.pairs(1000)
    bias = pr.BIASES[4]
    for aligned in (True, False):
        a = _score(dtype, kk, bias, aligned, row, col)
        assert _same_bits(a, _score(dtype, kk, bias, aligned, row, col))
        perm = np.random.default_rng(kk).permutation(len(row))
        assert _same_bits(_score(dtype, kk, bias, aligned, row[perm], col[perm]), a[perm]), (kk, aligned, "a permutation of the pairs changed bits")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_kernel_grid_stride(dtype):
    """100,000 pairs at kk = 3: more steps than one launch has wavefronts."""
    row, col = pr.pairs(100000)
    bias = ("tight", True)
    got = _score(dtype, 3, bias, True, row, col)
    _check(dtype, 3, bias, got, row, col, what="grid-stride")
    assert _same_bits(got, _score(dtype, 3, bias, False, row, col))
    perm = np.random.default_rng(1).permutation(len(row))
    assert _same_bits(_score(dtype, 3, bias, True, row[perm], col[perm]), got[perm])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_implicit_ignores_biases(dtype):
    """The implicit value is a . b alone: biases and a glob_mean that the caller supplies all the same are not added, through
    the entry point (tight biases and biasA as a column of A's image, both load widths) and through the scorer handle."""
    from cmfrec_amd import Scorer, ops
    row, col = pr.pairs(1000)
    for kk in (3, 17, 129):
        A, B, bA, bB, gm = pr.problem(dtype, kk)
        assert gm != 0 and np.abs(bA).min() > 0 and np.abs(bB).min() > 0
        plain = _score(dtype, kk, (None, False), True, row, col, implicit=True)
        for bias in (("tight", True), ("col", True)):
            for aligned in (True, False):
                got = ops.score_pairs(row=row, col=col, implicit=True, **pr.images(dtype, kk, bias, aligned))      # (glob_mean = gm)
                pr.check(got, A, B, None, None, 0.0, row, col, implicit=True, what="implicit with biases kk=%d %s" % (kk, bias))
                assert _same_bits(got, plain), (kk, bias, aligned)
        with Scorer(A, B, bA, bB, glob_mean=gm, implicit=True) as sc:
            got = sc.predict(row, col)
        pr.check(got, A, B, None, None, 0.0, row, col, implicit=True, what="Scorer implicit with biases kk=%d" % kk)
        assert _same_bits(got, plain), kk


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_kernel_poisoned(dtype, monkeypatch):
    row, col = pr.pairs(1000)
    for kk in (3, 65, 272):
        bias = ("col", True)
        monkeypatch.delenv("CMFREC_HIP_POISON_LDS", raising=False)
        plain = [_score(dtype, kk, bias, al, row, col) for al in (True, False)]
        monkeypatch.setenv("CMFREC_HIP_POISON_LDS", "1")
        for al, want in zip((True, False), plain):
            assert _same_bits(_score(dtype, kk, bias, al, row, col), want), (kk, al)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_entry_point_rejects(dtype):
    from cmfrec_amd import _lib
    lib = _lib.load(dtype)
    A, B = np.zeros((4, 3), dtype), np.zeros((5, 3), dtype)
    row = np.zeros(2, np.int32); col = np.zeros(2, np.int32); out = np.full(2, 7.0, dtype)
    P = _lib.ptr

    def call(m=4, n=5, kk=3, A=A, lda=3, B=B, ldb=3, row=row, n_pairs=2):
        return lib.cmfrec_hip_score_pairs(m, n, kk, P(A), lda, 0, None, P(B), ldb, 0, None, 0.0, 0, P(row), P(col), n_pairs, P(out))

    for kw in (dict(m=-1), dict(n=-1), dict(kk=0), dict(lda=2), dict(ldb=2), dict(A=None), dict(B=None), dict(row=None)):
        assert call(**kw) == 2, kw
        assert b"cmfrec_hip_score_pairs" in lib.cmfrec_hip_last_error()
    assert (out == 7.0).all()
    assert call(n_pairs=0) == 0 and (out == 7.0).all()
    assert call() == 0 and (out == 0.0).all()


# ---- 2. the scorer handle --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_scorer_equals_kernel(dtype, monkeypatch):
    from cmfrec_amd import Scorer
    row, col = pr.pairs(1000)
    for kk in (3, 50, 129):
        A, B, bA, bB, gm = pr.problem(dtype, kk)
        want = _score(dtype, kk, ("tight", True), True, row, col)
        with Scorer(A, B, bA, bB, glob_mean=gm) as sc:
            with pytest.raises(RuntimeError):
                sc.kernel_ms()                                           # (return code 2 before the first call)
            got = sc.predict(row, col)
            assert sc.kernel_ms() > 0
            assert _same_bits(got, want), kk
            monkeypatch.setenv("CMFREC_HIP_PREDICT_BLOCK", "64")
            assert _same_bits(sc.predict(row, col), want), (kk, "the block size changed the bits")
            monkeypatch.delenv("CMFREC_HIP_PREDICT_BLOCK")
            # calls of other sizes on the same handle: smaller, empty, larger
            assert _same_bits(sc.predict(row[:65], col[:65]), want[:65])
            assert sc.predict(row[:0], col[:0]).shape == (0,)
            r2, c2 = np.tile(row, 3), np.tile(col, 3)
            assert _same_bits(sc.predict(r2, c2), np.tile(want, 3))
        with pytest.raises(RuntimeError, match="closed"):
            sc.predict(row, col)
        # a row-strided view goes up as it is
        wide = np.zeros((pr.M, kk + 3), dtype); wide[:, 2:2 + kk] = A
        with Scorer(wide[:, 2:2 + kk], B, bA, bB, glob_mean=gm) as sc:
            assert _same_bits(sc.predict(row, col), want)
        want_i = _score(dtype, kk, (None, False), True, row, col, implicit=True)
        with Scorer(A, B, implicit=True) as sc:
            assert _same_bits(sc.predict(row, col), want_i)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_scorer_create_rejects(dtype):
    from cmfrec_amd import _lib
    lib = _lib.load(dtype)
    A, B = np.zeros((4, 3), dtype), np.zeros((5, 3), dtype)
    P = _lib.ptr
    for args in ((P(A), 3, 4, P(B), 3, 5, 0), (P(A), 2, 4, P(B), 3, 5, 3), (None, 3, 4, P(B), 3, 5, 3), (P(A), 3, 0, P(B), 3, 5, 3)):
        assert not lib.cmfrec_hip_scorer_create(*args, None, None, 0.0, 0, -1)
        assert lib.cmfrec_hip_last_error_code() == 2 and b"cmfrec_hip_scorer_create" in lib.cmfrec_hip_last_error()
    h = lib.cmfrec_hip_scorer_create(P(A), 3, 4, P(B), 3, 5, 3, None, None, 0.0, 0, -1)
    assert h
    ms = C.c_double(-1)
    assert lib.cmfrec_hip_scorer_kernel_ms(C.c_void_p(h), C.byref(ms)) == 2
    lib.cmfrec_hip_scorer_destroy(C.c_void_p(h))


# ---- 3. the drop-in names --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_predict_X_old(dtype, implicit):
    from cmfrec_amd import _lib
    lib = _lib.load(dtype)
    g = pr.load_fixture(dtype)
    for km in pr.OLD_KMS:
        d = pr.old_problem(dtype, km)
        rc, got = pr.call_old(lib, dtype, d, implicit)
        assert rc == 0
        ops = pr.old_operands(d, implicit)
        r = pr.check(got, *ops, d["row"], d["col"], implicit=implicit, what="predict_X_old k_main=%d" % km)
        print("predict_X_old %s implicit=%s k_main=%d: error / bound %.3g" % (_name(dtype), implicit, km, r))
        if km == 0:                                                      # the reference's values lie within the bound of the exact ones too
            pr.check(g["old_%s_km0" % ("imp" if implicit else "exp")], *ops, d["row"], d["col"], implicit=implicit, what="fixture")


@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_predict_X_old_empty_side(dtype, implicit):
    """m = 0 or n_max = 0 is legal, as in the reference: every pair gets the fallback value (the bias of the other side where
    that index is in range, or NaN); a negative size returns 2 and leaves predicted untouched."""
    from cmfrec_amd import _lib
    lib = _lib.load(dtype)
    d = pr.old_problem(dtype, 2)
    for side in ("A", "B"):
        e = dict(d)
        e[side], e["bias" + side] = d[side][:0], d["bias" + side][:0]
        rc, got = pr.call_old(lib, dtype, e, implicit)
        assert rc == 0, (side, lib.cmfrec_hip_last_error())
        pr.check(got, *pr.old_operands(e, implicit), e["row"], e["col"], implicit=implicit, what="predict_X_old without rows of " + side)

    A, B = np.array(d["A"]), np.array(d["B"])
    f = lib.predict_X_old_collective_implicit
    f.restype = C.c_int
    out = np.full(3, -777.0, dtype)
    idx = np.zeros(3, np.int32)
    P = _lib.ptr
    rc = f(P(idx), P(idx), P(out), C.c_size_t(3), P(A), P(B), C.c_int(d["k"]), C.c_int(d["k_user"]), C.c_int(d["k_item"]), C.c_int(2),
           C.c_int(-1), C.c_int(B.shape[0]), C.c_int(1))
    assert rc == 2 and (out == -777.0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_predict_X_new(dtype):
    """Against the recorded reference at the tolerance of new rows, relative to the largest recorded value.  w1 (explicit, k_main
    = 0) is compared with the recorded predictions as they are.  d2, b1 and the implicit i1 have k_main = 1, where the reference's
    own values leave the k_main factors out: predict_reference.reference_prediction adds that part from the reference's recorded
    factors, so that both sides are the model's prediction."""
    from cmfrec_amd import _lib
    lib = _lib.load(dtype)
    g = pr.load_fixture(dtype)
    tol = nro.TOL64 if dtype is np.float64 else nro.TOL32
    for k in nro.KS:
        for name, kind, kw in pr.new_cases(dtype, k):
            prow, pcol = pr.new_pairs(kw)
            rc, got = pr.call_new(lib, dtype, kind, prow, pcol, **kw)
            assert rc == 0, (k, name, lib.cmfrec_hip_last_error())
            want = pr.reference_prediction(dtype, k, name, kind, kw, prow, pcol, g[pr.key_of(k, name)])
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan) and (nan.any() == (kind == "implicit")), (k, name)
            e = float(np.abs(got[~nan] - want[~nan]).max() / np.abs(want[~nan]).max())
            print("predict_X_new %s k=%d %s: %.3g" % (_name(dtype), k, name, e))
            assert e <= tol, (k, name, e)
    # a refused call leaves predicted untouched
    name, kind, kw = pr.new_cases(dtype, nro.KS[0])[0]
    prow, pcol = pr.new_pairs(kw)
    rc, got = pr.call_new(lib, dtype, kind, prow, pcol, **dict(kw, NA_as_zero_X=True))
    assert rc == 2 and (got == -777.0).all()


# ---- 4. the new-rows handle ------------------------------------------------------------------------------------------------

def _nro_case(dtype, k, name):
    return next(kw for n, kw in nro.cases(nro.problem(dtype, k)) if n.split()[0] == name)


@pytest.mark.parametrize("name", ["d0", "d2"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_new_users_predict(dtype, name):
    """d0: no k_user, a factor row of k + 1 values (odd: element-wide loads); d2: k_user / k_item / k_main, U for fewer rows."""
    from cmfrec_amd import Scorer, _lib
    from cmfrec_amd.new_users import NewUsers
    for k in nro.KS:
        kw = _nro_case(dtype, k, name)
        mdl = ir.model_of(dtype, k, kw)
        batch = dict(X=kw["Xfull"], U=kw.get("U"))
        prow, pcol = pr.pairs(500, kw["m"], kw["B"].shape[0], seed=3)
        with NewUsers(mdl) as nu:
            A0, b0 = nu.factors(**batch, return_bias=True)
            got, (A, bias) = nu.predict(**batch, row=prow, item=pcol, return_factors=True)
            assert _same_bits(A, A0) and _same_bits(bias, b0)
            assert nu.kernel_ms()[1] > 0
            assert _same_bits(nu.predict(**batch, row=prow, item=pcol), got)
            ku, ki = mdl.k_user, mdl.k_item
            with Scorer(A[:, ku:], mdl.B_[:, ki:], bias, mdl.item_bias_, glob_mean=mdl.glob_mean_) as sc:
                assert _same_bits(sc.predict(prow, pcol), got), (k, name)
            pr.check(got, np.ascontiguousarray(A[:, ku:]), np.ascontiguousarray(mdl.B_[:, ki:]), bias, mdl.item_bias_, mdl.glob_mean_, prow, pcol,
                     what="NewUsers.predict %s k=%d" % (name, k))
            # a refused batch (X both dense and sparse), then the next one
            s, keep, rows = nu._batch(kw["Xfull"], kw.get("U"), None)
            s.nnz = 1
            out = np.full(len(prow), -777.0, dtype)
            rc = nu.lib.cmfrec_hip_newrows_predict(nu.handle, C.byref(s), _lib.ptr(prow), _lib.ptr(pcol), len(prow), _lib.ptr(out), None, None)
            assert rc == 2 and b"dense and as a sparse" in nu.lib.cmfrec_hip_last_error() and (out == -777.0).all()
            assert _same_bits(nu.predict(**batch, row=prow, item=pcol), got)
            # a sparse batch on the same handle
            d = nro.problem(dtype, k)
            X = (d["row"], d["col"], d["ratings"])
            sp, (As, bs) = nu.predict(X=X, U=kw.get("U"), row=prow, item=pcol, return_factors=True)
            pr.check(sp, np.ascontiguousarray(As[:, ku:]), np.ascontiguousarray(mdl.B_[:, ki:]), bs, mdl.item_bias_, mdl.glob_mean_, prow, pcol,
                     what="NewUsers.predict sparse %s k=%d" % (name, k))
        assert _same_bits(mdl.predict_new_batch(**batch, row=prow, item=pcol), got)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_model_predict_batch(dtype):
    """predict_batch and the host's predict lie within the bound of the exact value, both; nothing more is claimed."""
    k = nro.KS[1]
    kw = _nro_case(dtype, k, "d2")
    mdl = ir.model_of(dtype, k, kw)
    rng = np.random.default_rng(5)
    m = 41
    mdl.A_ = rng.standard_normal((m, mdl.k_user + k + mdl.k_main)).astype(dtype)
    mdl.user_bias_ = rng.standard_normal(m).astype(dtype)
    n = mdl.B_.shape[0]
    u, i = rng.integers(0, m, 700).astype(np.int32), rng.integers(0, n, 700).astype(np.int32)
    ops = (np.ascontiguousarray(mdl.A_[:, mdl.k_user:]), np.ascontiguousarray(mdl.B_[:, mdl.k_item:]), mdl.user_bias_, mdl.item_bias_,
           mdl.glob_mean_)
    got = mdl.predict_batch(u, i)
    pr.check(got, *ops, u, i, what="predict_batch")
    pr.check(np.asarray(mdl.predict(u, i), dtype), *ops, u, i, what="predict")
    with mdl.scorer() as sc:
        assert _same_bits(sc.predict(u, i), got)
        out = sc.predict(np.array([m, 0], np.int32), np.array([0, n], np.int32))
    T = np.dtype(dtype).type
    assert out[0] == T(mdl.glob_mean_) + mdl.item_bias_[0] and out[1] == T(mdl.glob_mean_) + mdl.user_bias_[0]
