"""GPU: imputation of a dense X on the device -- the fill kernel on its own (ops.impute_dense), through the new-rows handle
(NewUsers.impute, cmfrec_hip_newrows_impute), under the reference's name (impute_X_collective_explicit) and CMF.transform.
The problems, the reference, the bounds and the check: tests/impute_reference.py; the check's sensitivity and the fixture:
tests/test_impute_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import impute_reference as ir
import new_rows_options as nro
from dense_reference import _bits

pytestmark = pytest.mark.gpu

IDS = lambda v: getattr(v, "__name__", None) or str(v).replace(" ", "")


def _run(dtype, data, shape, kk, pattern, bias, row_missing=None, X=None):
    from cmfrec_amd import ops
    X_img, kw = ir.images(dtype, data, shape, kk, pattern, bias, X=X)
    return ops.impute_dense(X_img=X_img, row_missing=row_missing, **kw)


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kk", ir.KKS)
@pytest.mark.parametrize("data", ir.DATA)
@pytest.mark.parametrize("dtype", ir.DTYPES, ids=IDS)
def test_fill_kernel(dtype, data, kk):
    """Every shape and NaN pattern at one width, the bias variants and row_missing absent / present rotating over them; on the
    random pattern every bias variant, row_missing absent and present (same bits), the same call twice (same bits), and a
    row_missing that says 0 for a row that holds NaN (the row comes back untouched: the skip is real)."""
    worst = 0.0
    for si, shape in enumerate(ir.SHAPES):
        m, n = shape
        for pi, pattern in enumerate(ir.PATTERNS):
            bias = ir.BIASES[(si + pi) % len(ir.BIASES)]
            X, nan = ir.x_input(dtype, m, n, pattern)
            counts = nan.sum(axis=1).astype(np.int32) if (si + pi) % 2 else None
            img = _run(dtype, data, shape, kk, pattern, bias, row_missing=counts)
            worst = max(worst, ir.check(dtype, data, shape, kk, pattern, bias, img))
            if pattern == "none":
                before = ir.images(dtype, data, shape, kk, pattern, bias)[0]
                assert np.array_equal(_bits(img), _bits(before)), (shape, "X without NaN changed")
        X, nan = ir.x_input(dtype, m, n, "random")
        counts = nan.sum(axis=1).astype(np.int32)
        for bias in ir.BIASES:
            a = _run(dtype, data, shape, kk, "random", bias)
            worst = max(worst, ir.check(dtype, data, shape, kk, "random", bias, a))
            b = _run(dtype, data, shape, kk, "random", bias, row_missing=counts)
            c = _run(dtype, data, shape, kk, "random", bias)
            assert np.array_equal(_bits(a), _bits(b)), (shape, bias, "row_missing changed the bits")
            assert np.array_equal(_bits(a), _bits(c)), (shape, bias, "two runs differ")
        rows = np.nonzero(counts)[0]
        if len(rows):
            lie = counts.copy(); row = int(rows[len(rows) // 2]); lie[row] = 0
            img = _run(dtype, data, shape, kk, "random", ir.BIASES[1], row_missing=lie)
            ir.check(dtype, data, shape, kk, "random", ir.BIASES[1], img, untouched_rows=(row,))
            assert np.isnan(ir.split_image(img, m, n, ir.odd_ld(n), ir.OFF_X)[0][row]).sum() == counts[row]
    print("worst error / bound: %.3g" % worst)


# ---- 2. through the handle -------------------------------------------------------------------------------------------------

def _batch_args(kw):
    return dict(X=kw["Xfull"], U=kw.get("U"), W=kw.get("weight"))


def _case(dtype, k, name):
    return next(kw for n, kw in ir.impute_cases(nro.problem(dtype, k)) if n.split()[0] == name)


def _check_against_factors(dtype, kw, out, A, bias, what):
    X = kw["Xfull"]
    nan = np.isnan(X)
    assert np.array_equal(_bits(out)[~nan], _bits(np.ascontiguousarray(X))[~nan]), (what, "a present entry changed its bits")
    assert np.isfinite(out[nan]).all(), (what, "imputed entries not finite")
    ref, bound = ir.product_of_factors(dtype, kw, A, bias)
    err = np.abs(out.astype(ref.dtype) - ref)
    r = ir._ratio(err[nan], bound[nan])
    assert r <= 1.0, (what, "error / bound = %.3g" % r)
    return r


@pytest.mark.parametrize("name", ir.CASE_NAMES)
@pytest.mark.parametrize("k", nro.KS)
@pytest.mark.parametrize("dtype", ir.DTYPES, ids=IDS)
def test_handle_cases(dtype, k, name):
    """(a) the imputed entries are, within the kernel's bound, the wide-precision product of the factors NewUsers.factors returns
    for the same batch; present entries keep their bits (rows without NaN come back identical); the caller's X is not modified.
    (b) against the reference's recorded result (g41), per row over the imputed entries, at the tolerance the factors of the
    same problem are held to."""
    from cmfrec_amd.new_users import NewUsers
    kw = _case(dtype, k, name)
    X = np.array(kw["Xfull"], dtype, copy=True)
    keep = X.copy()
    with NewUsers(ir.model_of(dtype, k, kw)) as nu:
        A, bias = nu.factors(**dict(_batch_args(kw), X=X), return_bias=True)
        out, fac = nu.impute(**dict(_batch_args(kw), X=X), return_factors=True)
        solve_ms, fill_ms = nu.kernel_ms()
    assert out is not X and np.array_equal(_bits(X), _bits(keep))
    has_nan = bool(np.isnan(X).any())
    assert (fac is None) == (not has_nan)
    if has_nan:
        assert np.array_equal(fac[0], A) and (bias is None or np.array_equal(fac[1], bias))
        assert fill_ms > 0
    else:
        assert solve_ms == 0 and fill_ms == 0
    _check_against_factors(dtype, kw, out, A, bias, (k, name))
    e = ir.imputed_row_err(out, ir.load_fixture(dtype)[ir.key_of(k, name)], X)
    print("%s k=%d %s: against the fixture %.2e" % (np.dtype(dtype).name, k, name, e))
    assert e <= (nro.TOL64 if dtype is np.float64 else nro.TOL32), (k, name, e)


def _tb_case(dtype, k):
    """A model with TransBtBinvBt: the rows without a missing entry take x^T TransBtBinvBt, for which the run centres its device
    copy of X in place -- the fill must not see that copy."""
    d = nro.problem(dtype, k)
    Bp = d["B_plain"].astype(np.float64)
    T = np.linalg.solve(Bp.T @ Bp + 0.6 * np.eye(k), Bp.T).T.astype(dtype)
    return dict(Xfull=d["Xfull"], m=d["m"], B=d["B_plain"], biasB=d["biasB"], glob_mean=3.1, lam=0.6), T


@pytest.mark.parametrize("k", nro.KS)
@pytest.mark.parametrize("dtype", ir.DTYPES, ids=IDS)
def test_handle_blocks(dtype, k, monkeypatch):
    """(c) CMFREC_HIP_NEWROWS_BLOCK_ROWS = 1, 7, 16 and the default give identical bits -- also where the run centres its copy of
    X (TransBtBinvBt), whose present entries must come back as the caller's."""
    from cmfrec_amd.new_users import NewUsers
    todo = [(n, _case(dtype, k, n), None) for n in ("i1", "i2", "i3", "i5")]
    kw_tb, T = _tb_case(dtype, k)
    todo.append(("TransBtBinvBt", kw_tb, T))
    for name, kw, T in todo:
        mdl = ir.model_of(dtype, k, kw)
        if T is not None:
            mdl._TransBtBinvBt = T
        outs = []
        with NewUsers(mdl) as nu:
            for rows in (None, "1", "7", "16"):
                if rows is None:
                    monkeypatch.delenv("CMFREC_HIP_NEWROWS_BLOCK_ROWS", raising=False)
                else:
                    monkeypatch.setenv("CMFREC_HIP_NEWROWS_BLOCK_ROWS", rows)
                out, (A, bias) = nu.impute(**_batch_args(kw), return_factors=True)
                _check_against_factors(dtype, kw, out, A, bias, (k, name, rows))
                outs.append(out)
        for o in outs[1:]:
            assert np.array_equal(_bits(o), _bits(outs[0])), (k, name)


@pytest.mark.parametrize("dtype", ir.DTYPES, ids=IDS)
def test_handle_aliasing(dtype):
    """(d) Xout = Xfull and a separate Xout: the same bits; with a separate Xout the input is untouched."""
    from cmfrec_amd.new_users import NewUsers
    from cmfrec_amd import _lib
    for k in nro.KS:
        kw = _case(dtype, k, "i2")
        with NewUsers(ir.model_of(dtype, k, kw)) as nu:
            sep = nu.impute(**_batch_args(kw))
            X = np.array(kw["Xfull"], dtype, copy=True)
            s, keep, rows = nu._batch(X, kw.get("U"), kw.get("weight"))
            assert keep["Xfull"] is X
            rc = nu.lib.cmfrec_hip_newrows_impute(nu.handle, C.byref(s), _lib.ptr(X), None, None)
            assert rc == 0
        assert np.array_equal(_bits(X), _bits(sep)), k
        assert np.isnan(kw["Xfull"]).any() and not np.isnan(X).any()


@pytest.mark.parametrize("which", ["U_more", "U_less"])
@pytest.mark.parametrize("dtype", ir.DTYPES, ids=IDS)
def test_handle_side_information_rows(dtype, which):
    """(e) side information for more rows than X has (they have no row of X) and for fewer."""
    from cmfrec_amd.new_users import NewUsers
    for k in nro.KS:
        d = nro.problem(dtype, k)
        kw = dict(_case(dtype, k, "i2"), U=d[which])
        with NewUsers(ir.model_of(dtype, k, kw)) as nu:
            A, bias = nu.factors(**_batch_args(kw), return_bias=True)
            out = nu.impute(**_batch_args(kw))
        assert A.shape[0] == max(d["m"], d[which].shape[0]) and out.shape == (d["m"], d["n"])
        _check_against_factors(dtype, kw, out, A, bias, (k, which))


# ---- 3. the drop-in name ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["i1", "i2"])
@pytest.mark.parametrize("dtype", ir.DTYPES, ids=IDS)
def test_drop_in_name(dtype, name):
    """impute_X_collective_explicit through the positional helper that serves the compiled reference too: Xfull changed in place,
    against the fixture."""
    from cmfrec_amd import _lib
    lib = _lib.load(dtype)
    for k in nro.KS:
        kw = _case(dtype, k, name)
        rc, X = ir.call_impute(lib, dtype, k=k, **kw)
        assert rc == 0, (k, name)
        nan = np.isnan(kw["Xfull"])
        assert np.array_equal(_bits(X)[~nan], _bits(np.ascontiguousarray(kw["Xfull"]))[~nan]) and np.isfinite(X).all()
        e = ir.imputed_row_err(X, ir.load_fixture(dtype)[ir.key_of(k, name)], kw["Xfull"])
        assert e <= (nro.TOL64 if dtype is np.float64 else nro.TOL32), (k, name, e)
    rc, X = ir.call_impute(lib, dtype, k=nro.KS[0], **dict(_case(dtype, nro.KS[0], name), NA_as_zero_U=True))
    assert rc == 2 and np.array_equal(_bits(X), _bits(np.ascontiguousarray(_case(dtype, nro.KS[0], name)["Xfull"])))


# ---- 4. refusals and surface -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ir.DTYPES, ids=IDS)
def test_refusals_leave_the_handle_usable(dtype):
    from cmfrec_amd import _lib
    from cmfrec_amd.new_users import NewUsers
    lib = _lib.load(dtype)
    k = nro.KS[0]
    d = nro.problem(dtype, k)
    kw = _case(dtype, k, "i1")
    with NewUsers(ir.model_of(dtype, k, kw)) as nu:
        good = nu.impute(**_batch_args(kw))
        out = np.empty_like(good)
        s, keep, _ = nu._batch((d["row"], d["col"], d["ratings"]), None, None)        # a sparse X
        assert lib.cmfrec_hip_newrows_impute(nu.handle, C.byref(s), _lib.ptr(out), None, None) == 2
        assert b"Xfull" in lib.cmfrec_hip_last_error()
        s, keep, _ = nu._batch(np.array(kw["Xfull"], dtype), None, None)
        s.m = 0
        assert lib.cmfrec_hip_newrows_impute(nu.handle, C.byref(s), _lib.ptr(out), None, None) == 2
        again = nu.impute(**_batch_args(kw))                                          # the next valid batch
        assert np.array_equal(_bits(again), _bits(good))
        with pytest.raises(ValueError):
            nu.impute((d["row"], d["col"], d["ratings"]))
    # an implicit-model handle
    m = _lib.newrows_model_mirror(dtype)()
    B = np.ascontiguousarray(d["B_plain"], dtype)
    m.implicit = 1; m.n = m.n_max = B.shape[0]; m.k = k; m.lam = 1.0
    m.w_main = m.w_user = m.alpha = m.w_main_multiplier = m.scaling_biasA = m.w_implicit = 1.0
    m.B = B.ctypes.data
    h = lib.cmfrec_hip_newrows_create(C.byref(m), C.c_int(-1))
    assert h
    try:
        s = _lib.NewRowsBatch()
        X = np.array(kw["Xfull"], dtype)
        s.m = X.shape[0]; s.Xfull = X.ctypes.data
        out = np.empty_like(X)
        assert lib.cmfrec_hip_newrows_impute(C.c_void_p(h), C.byref(s), _lib.ptr(out), None, None) == 2
        assert b"explicit model" in lib.cmfrec_hip_last_error()
        A = np.empty((d["m"], k), dtype)
        s2 = _lib.NewRowsBatch()
        row, col, val = d["row"], d["col"], np.ascontiguousarray(d["counts"], dtype)
        s2.m = d["m"]; s2.X = val.ctypes.data; s2.ixA = row.ctypes.data; s2.ixB = col.ctypes.data; s2.nnz = len(val)
        assert lib.cmfrec_hip_newrows_factors(C.c_void_p(h), C.byref(s2), _lib.ptr(A), None) == 0 and np.isfinite(A).all()
    finally:
        lib.cmfrec_hip_newrows_destroy(C.c_void_p(h))


@pytest.mark.parametrize("dtype", ir.DTYPES, ids=IDS)
def test_transform_equals_impute(dtype):
    from cmfrec_amd import CMF_implicit
    from cmfrec_amd.new_users import NewUsers
    k = nro.KS[1]
    kw = _case(dtype, k, "i2")
    mdl = ir.model_of(dtype, k, kw)
    X = np.array(kw["Xfull"], dtype, copy=True)
    keep = X.copy()
    got = mdl.transform(X, U=kw["U"])
    assert np.array_equal(_bits(X), _bits(keep)) and got is not X
    with NewUsers(mdl) as nu:
        want = nu.impute(X, U=kw["U"])
    assert np.array_equal(_bits(got), _bits(want))
    assert not hasattr(CMF_implicit, "transform")
