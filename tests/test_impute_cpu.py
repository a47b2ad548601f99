"""CPU: the check of the imputation (tests/impute_reference.py) accepts a stand-in kernel -- NumPy in the dtype -- and rejects
mutations of its result on both data sets; the g41 fixture is what the compiled reference returns, and its inputs are well
enough conditioned for the float32 tolerance of the GPU test."""
import numpy as np
import pytest

import impute_reference as ir
import new_rows_options as nro
from reference_calls import reference

# the widths around the MFMA depth, the 16-byte vector, the routing width and the maximum, on the two shapes with more than one
# tile in both directions
CASES = [(dt, data, shape, kk) for dt in ir.DTYPES for data in ir.DATA for shape in ((17, 15), (33, 130)) for kk in (1, 5, 65, 272)]
ALWAYS = {"a dropped term", "a term counted twice", "biasB missing", "rows r and r+1 of A swapped", "a present entry one ulp off",
          "a NaN left in place", "a SENTINEL overwritten"}


@pytest.mark.parametrize("dtype,data,shape,kk", CASES, ids=lambda v: getattr(v, "__name__", None) or str(v).replace(" ", ""))
def test_check_accepts_standin_and_rejects_mutations(dtype, data, shape, kk):
    seen = set()
    for pattern, bias in (("random", ("tight", True)), ("corners", ("col", True)), ("all", (None, True)), ("none", ("tight", False))):
        args = (dtype, data, shape, kk, pattern, bias)
        good, mut = ir.mutations(*args)
        ir.check(*args, good)
        for name, img in mut.items():
            with pytest.raises(ir.Rejected):
                ir.check(*args, img)
                print("accepted: %s on %s" % (name, args))
            seen.add(name)
    assert seen == ALWAYS


def test_untouched_rows_are_checked():
    """A row that must come back as it went in (row_missing = 0) fails the check once it has been filled."""
    args = (np.float64, "normal", (17, 15), 5, "random", ("tight", True))
    good, _ = ir.mutations(*args)
    nan = ir.x_input(np.float64, 17, 15, "random")[1]
    row = int(np.nonzero(nan.any(axis=1))[0][0])
    with pytest.raises(ir.Rejected):
        ir.check(*args, good, untouched_rows=(row,))


def test_fixture_holds_every_case():
    for dtype in ir.DTYPES:
        g = ir.load_fixture(dtype)
        for k in nro.KS:
            d = nro.problem(dtype, k)
            for name, kw in ir.impute_cases(d):
                X = g[ir.key_of(k, name)]
                assert X.shape == (d["m"], d["n"]) and np.isfinite(X).all(), (k, name)
                keep = ~np.isnan(kw["Xfull"])
                assert np.array_equal(X[keep], kw["Xfull"][keep]), (k, name)


@pytest.mark.parametrize("dtype", ir.DTYPES)
def test_live_reference_reproduces_fixture(dtype):
    R = reference(dtype, replay=False)
    g = ir.load_fixture(dtype)
    tol = 1e-12 if dtype is np.float64 else 1e-5        # (the same binary on the same inputs, nthreads = 1)
    for k in nro.KS:
        for name, kw in ir.impute_cases(nro.problem(dtype, k)):
            rc, X = ir.call_impute(R.lib, dtype, k=k, **kw)
            assert rc == 0, (k, name)
            keep = ~np.isnan(kw["Xfull"])
            assert np.array_equal(X[keep], kw["Xfull"][keep]), (k, name)
            assert ir.imputed_row_err(X, g[ir.key_of(k, name)], kw["Xfull"]) <= tol, (k, name)


def test_inputs_are_conditioned_for_float32():
    """The reference's own float32 result lies within a quarter of TOL32 of its float64 result on every case."""
    g64, g32 = ir.load_fixture(np.float64), ir.load_fixture(np.float32)
    worst = 0.0
    for k in nro.KS:
        for name, kw in ir.impute_cases(nro.problem(np.float64, k)):
            e = ir.imputed_row_err(g32[ir.key_of(k, name)], g64[ir.key_of(k, name)], kw["Xfull"])
            worst = max(worst, e)
            assert e < nro.TOL32 / 4, (k, name, e)
    print("worst float32 against float64: %.2e" % worst)
