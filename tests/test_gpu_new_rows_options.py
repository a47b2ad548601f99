"""GPU: factors of new rows with observation weights, a dense X and implicit features -- factors_collective_explicit_multiple
through the C ABI against the reference's recorded outputs (fixture g40, tests/new_rows_options.py), the dense batch's
compaction on the device against the triplets of its present entries, and CMF.factors_multiple on its own training rows."""
import numpy as np
import pytest

import golden_cases as gc
import new_rows_options as nro
from conftest import row_rel_err

pytestmark = pytest.mark.gpu
DT = [np.float64, np.float32]
TOL = {np.float64: nro.TOL64, np.float32: nro.TOL32}        # tests/test_gpu_golden.py::TOL, new rows


def hip(dtype, k, **kw):
    from cmfrec_amd import _lib
    rc, A, bA = nro.call_multiple(_lib.load(dtype), dtype, k=k, **kw)
    assert rc == 0, (rc, _lib.load(dtype).cmfrec_hip_last_error())
    return A, bA


def close(got, exp, dtype, what):
    """Both criteria of the project for new rows: the matrix-wide relative error and the per-row one."""
    bad = []
    for g, e, tag in zip(got, exp, ("A", "bias")):
        if e is None:
            continue
        e1, (e2, r) = gc.maxrel(g, e), row_rel_err(g, e)
        print("%s %s: maxrel %.2e, worst row %.2e (row %d)" % (what, tag, e1, e2, r))
        if not (e1 < TOL[dtype] and e2 < TOL[dtype]):
            bad.append((what, tag, e1, e2, r))
    return bad


@pytest.mark.parametrize("dtype", DT)
def test_parity_with_reference_fixture(dtype):
    g = nro.load_fixture(dtype)
    bad = []
    for k in nro.KS:
        d = nro.problem(dtype, k)
        for name, kw in nro.cases(d):
            key = nro.key_of(k, name)
            exp = (g["A_" + key], g["biasA_" + key] if kw.get("user_bias") else None)
            bad += close(hip(dtype, k, **kw), exp, dtype, "k=%d %s" % (k, name))
    assert not bad, bad


@pytest.mark.parametrize("dtype", DT)
def test_coo_and_csr_input(dtype):
    """The weights follow the entries: triplet order with COO input, the order of Xcsr with CSR input."""
    bad = []
    for k in nro.KS:
        cs = dict((n.split()[0], kw) for n, kw in nro.cases(nro.problem(dtype, k)))
        for short in ("w0", "w2", "b2"):
            kw = dict(cs[short])
            a = hip(dtype, k, **kw)
            p, i, v, w = nro.coo_to_csr_stable(kw.pop("row"), kw.pop("col"), kw.pop("val"), kw["m"], kw.pop("weight"))
            b = hip(dtype, k, csr=(p, i, v), weight=w, **kw)
            bad += close(b, a, dtype, "k=%d %s csr" % (k, short))
    assert not bad, bad


def _dense_problem(dtype, n, m, seed):
    rng = np.random.default_rng(seed)
    k = 6
    B = (rng.standard_normal((n, k)) * 0.3).astype(dtype)
    biasB = (rng.standard_normal(n) * 0.2).astype(dtype)
    X = (0.5 * rng.integers(1, 11, (m, n))).astype(dtype)
    X[rng.random((m, n)) < 0.5] = np.nan
    if m > 2:
        X[1] = np.nan                                          # no observations
        X[2] = 0.5 * rng.integers(1, 11, n)                    # complete
    W = rng.uniform(0.5, 2.0, (m, n)).astype(dtype)
    W[~np.isfinite(X)] = np.nan                                # must not be read
    return k, B, biasB, X, W


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n,m", [(1, 7), (63, 7), (64, 7), (65, 7), (257, 13), (257, 1)])
def test_dense_against_sparse(dtype, n, m, monkeypatch):
    """The dense form of a batch and the triplets of its present entries: one 64-column chunk short, full, ragged, several, a
    row of NaN, a complete row, a single row.  n = 257: once more in blocks of five rows -- identical."""
    k, B, biasB, X, W = _dense_problem(dtype, n, m, 100 + n + m)
    r, c = np.nonzero(np.isfinite(X))
    common = dict(B=B, m=m, biasB=biasB, glob_mean=2.9, user_bias=True, lam=0.6, lam_bias=1.1, scale_lam=True)
    bad = []
    for wd, ws in ((None, None), (W, W[r, c])):
        a = hip(dtype, k, Xfull=X, weight=wd, **common)
        b = hip(dtype, k, row=r.astype(np.int32), col=c.astype(np.int32), val=X[r, c], weight=ws, **common)
        assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all()
        bad += close(a, b, dtype, "n=%d m=%d %s" % (n, m, "weighted" if wd is not None else "plain"))
        if n == 257 and m > 5:
            monkeypatch.setenv("CMFREC_HIP_NEWROWS_BLOCK_ROWS", "5")
            a5 = hip(dtype, k, Xfull=X, weight=wd, **common)
            monkeypatch.delenv("CMFREC_HIP_NEWROWS_BLOCK_ROWS")
            assert np.array_equal(a5[0], a[0]) and np.array_equal(a5[1], a[1])
    assert not bad, bad


@pytest.mark.parametrize("dtype", DT)
def test_unit_weights_and_zero_w_implicit(dtype):
    k = 6
    d = nro.problem(dtype, k)
    base = dict(row=d["row"], col=d["col"], val=d["ratings"], m=d["m"], B=d["B_plain"], biasB=d["biasB"], glob_mean=3.1,
                user_bias=True, lam=0.6, lam_bias=1.1, scale_lam=True)
    plain = hip(dtype, k, **base)
    bad = close(hip(dtype, k, weight=np.ones(len(d["row"]), dtype), **base), plain, dtype, "unit weights")
    bad += close(hip(dtype, k, Bi=d["Bi_plain"], w_implicit=0.0, **base), plain, dtype, "w_implicit = 0")
    den = dict(base, Xfull=d["Xfull"]); [den.pop(x) for x in ("row", "col", "val")]
    ones = np.where(np.isfinite(d["Xfull"]), 1.0, np.nan).astype(dtype)
    bad += close(hip(dtype, k, weight=ones, **den), hip(dtype, k, **den), dtype, "unit weights, dense")
    assert not bad, bad


@pytest.mark.parametrize("dtype", DT)
def test_weightless_row_is_zero(dtype):
    """Under scale_lam a row whose weights sum to nothing comes out as zeros (common.c:712)."""
    k = 6
    d = nro.problem(dtype, k)
    w = d["weight"].copy(); w[d["row"] == 11] = 0
    A, _ = hip(dtype, k, row=d["row"], col=d["col"], val=d["ratings"], m=d["m"], B=d["B_plain"], weight=w, lam=0.6, scale_lam=True)
    assert (A[11] == 0).all() and np.isfinite(A).all() and (A[12] != 0).any()


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("bias", [False, True])
def test_TransBtBinvBt_decides_complete_rows(dtype, bias):
    """A matrix built with another lambda than the call's: rows without a NaN follow the matrix, the others the call."""
    k, B, biasB, X, _ = _dense_problem(dtype, 65, 9, 77)
    X[5] = 0.5 * np.arange(1, 66) % 5 + 0.5                     # a second complete row
    Bx = np.hstack([B.astype(np.float64), np.ones((65, 1))]) if bias else B.astype(np.float64)
    T = np.linalg.solve(Bx.T @ Bx + 4.2 * np.eye(Bx.shape[1]), Bx.T).T.astype(dtype)
    kw = dict(B=B, m=9, Xfull=X, biasB=biasB, glob_mean=2.9, user_bias=bias, lam=0.6, TransBtBinvBt=T)
    got = hip(dtype, k, **kw)
    exp = nro.normal_equations(dict(kw, k=k))
    assert not close(got, exp, dtype, "TransBtBinvBt bias=%s" % bias)
    without = nro.normal_equations(dict(kw, k=k, TransBtBinvBt=None))[0]
    assert np.abs(without[2] - exp[0][2]).max() > 1e-2 * np.abs(exp[0][2]).max()      # the matrix does decide those rows
    assert np.array_equal(without[0], exp[0][0])


def _fit_problem(dtype):
    import scipy.sparse as sp
    from conftest import make_coo
    m, n, k = 200, 120, 8
    rng = np.random.default_rng(23)
    row, col, val = make_coo(m, n, 4000, 31, counts=False, dtype=dtype)
    X = sp.coo_matrix((val, (row, col)), shape=(m, n))
    A0 = (rng.standard_normal((m, k)) * 0.1).astype(dtype); B0 = (rng.standard_normal((n, k)) * 0.1).astype(dtype)
    w = rng.uniform(0.5, 2.0, len(val)).astype(dtype)
    return m, n, k, X, A0, B0, w


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("what", ["weights", "dense", "implicit_features"])
def test_estimator_returns_its_training_rows(dtype, what):
    """After a closed-form fit whose last step was the A-step, factors_multiple on the training rows with the matching inputs
    returns A_ (bound and settings of tests/test_gpu_fit.py::test_factors_multiple_l1_after_fit)."""
    import scipy.sparse as sp
    from cmfrec_amd import CMF
    t = 1e-8 if dtype is np.float64 else 2e-3
    m, n, k, X, A0, B0, w = _fit_problem(dtype)
    opts = dict(k=k, lambda_=0.5, niter=3, use_cg=False, use_float=dtype is np.float32, scale_lam=True,
                precompute_for_predictions=False)
    if what == "weights":
        mdl = CMF(**opts).fit(X, A0=A0, B0=B0, W=w)
        Wsp = sp.coo_matrix((w, (X.row, X.col)), shape=X.shape)
        A, bias = mdl.factors_multiple(X, W=Wsp.tocsr(), return_bias=True)       # another storage order, the same pattern
        other = sp.coo_matrix((w[1:], (X.row[1:], X.col[1:])), shape=X.shape)
        with pytest.raises(ValueError):
            mdl.factors_multiple(X, W=other)
        moved = sp.coo_matrix((w, (X.row, (X.col + 1) % n)), shape=X.shape)
        with pytest.raises(ValueError):
            mdl.factors_multiple(X, W=moved)
    elif what == "dense":
        Xd = np.full((m, n), np.nan, dtype); Xd[X.row, X.col] = X.data
        mdl = CMF(**opts).fit(Xd, A0=A0, B0=B0)
        A, bias = mdl.factors_multiple(Xd, return_bias=True)
    else:
        mdl = CMF(add_implicit_features=True, **opts).fit(X, A0=A0, B0=B0)
        A, bias = mdl.factors_multiple(X, return_bias=True)
    e1, e2 = gc.maxrel(A, mdl.A_), gc.maxrel(bias, mdl.user_bias_)
    print("%s: A %.2e, bias %.2e" % (what, e1, e2))
    assert e1 < t and e2 < t


@pytest.mark.parametrize("dtype", DT)
def test_refusals(dtype, capfd):
    """What stays refused returns 2 with a message, and so does every combination the fixture leaves out because the reference
    does not solve the stated model there."""
    from cmfrec_amd import _lib
    lib = _lib.load(dtype)
    k = 6
    d = nro.problem(dtype, k)
    coo = dict(row=d["row"], col=d["col"], val=d["ratings"], m=d["m"])
    side = dict(B=d["B_full"], k_main=d["km"], k_user=d["ku"], k_item=d["ki"], Cm=d["C_full"])
    Unan = d["U_more"].copy(); Unan[2, 1] = np.nan
    refused = [
        ("NA_as_zero_X", dict(coo, B=d["B_plain"], NA_as_zero_X=True)),
        ("NA_as_zero_U", dict(coo, **side, U_csr=d["U_csr"], NA_as_zero_U=True)),
        ("Ub", dict(coo, B=d["B_plain"], Ub=np.ones((d["m"], 3), dtype))),
        ("NaN in U", dict(coo, **side, U=Unan)),
        ("sparse and dense X", dict(coo, B=d["B_plain"], Xfull=d["Xfull"])),
        ("sparse U with scale_lam_sideinfo", dict(coo, **side, U_csr=d["U_csr"], weight=d["weight"], scale_lam_sideinfo=True)),
        ("L1 with nonneg", dict(coo, B=d["B_plain"], weight=d["weight"], l1_lam=0.1, nonneg=True)),
    ] + nro.refused_cases(d)
    for name, kw in refused:
        capfd.readouterr()
        rc, _, _ = nro.call_multiple(lib, dtype, k=k, **kw)
        err = capfd.readouterr().err
        assert rc == 2, (name, rc)
        assert "cmfrec_hip" in err, (name, err)


@pytest.mark.parametrize("dtype", DT)
def test_poisoned_lds(dtype, monkeypatch):
    """One weighted, one dense and one implicit-features case with NaN patterns in LDS and in fresh device buffers: the same
    numbers (the same kernels on the same inputs, every sum in a fixed order)."""
    k = 50
    cs = dict((n.split()[0], kw) for n, kw in nro.cases(nro.problem(dtype, k)))
    g = nro.load_fixture(dtype)
    for short in ("w2", "d1", "b1"):
        clean = hip(dtype, k, **cs[short])
        monkeypatch.setenv("CMFREC_HIP_POISON_LDS", "1")
        dirty = hip(dtype, k, **cs[short])
        monkeypatch.delenv("CMFREC_HIP_POISON_LDS")
        assert np.array_equal(clean[0], dirty[0]), short
        if clean[1] is not None:
            assert np.array_equal(clean[1], dirty[1]), short
        assert gc.maxrel(dirty[0], g["A_k%d_%s" % (k, short)]) < TOL[dtype]
