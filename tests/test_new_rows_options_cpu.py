"""CPU: the g40 fixture (new rows with observation weights, dense X and implicit features; tests/new_rows_options.py) is what the
compiled reference returns, what it pins solves the model's normal equations, and its inputs are well enough conditioned for
the float32 tolerance of the GPU test."""
import numpy as np
import pytest

import new_rows_options as nro
from conftest import row_rel_err

DTYPES = [np.float64, np.float32]


def _all_cases(dtype):
    for k in nro.KS:
        d = nro.problem(dtype, k)
        for name, kw in nro.cases(d):
            yield k, name, kw


def test_fixture_holds_every_case():
    for dtype in DTYPES:
        g = nro.load_fixture(dtype)
        for k, name, kw in _all_cases(dtype):
            assert "A_" + nro.key_of(k, name) in g.files, (k, name)
            assert ("biasA_" + nro.key_of(k, name) in g.files) == bool(kw.get("user_bias")), (k, name)


@pytest.mark.parametrize("dtype", DTYPES)
def test_live_reference_reproduces_fixture(dtype):
    """(a) where oracle/_ref was built."""
    from oracle.bindings import Reference, ref_available
    if not ref_available(dtype):
        pytest.skip("oracle/_ref not built")
    lib = Reference(dtype).lib
    g = nro.load_fixture(dtype)
    tol = 1e-12 if dtype is np.float64 else 1e-5        # (the same binary on the same inputs; threads do not enter: nthreads = 1)
    for k, name, kw in _all_cases(dtype):
        rc, A, bA = nro.call_multiple(lib, dtype, k=k, **kw)
        assert rc == 0, (k, name)
        assert row_rel_err(A, g["A_" + nro.key_of(k, name)])[0] <= tol, (k, name)
        if bA is not None:
            assert np.abs(bA - g["biasA_" + nro.key_of(k, name)]).max() <= tol * max(np.abs(bA).max(), 1e-300), (k, name)


def test_fixture_solves_the_normal_equations():
    """(b) every closed-form case: the float64 rows of the fixture against the model written out in NumPy from B, C, Bi, the
    weights and the lambdas -- so that no defect of the reference is recorded as truth."""
    g = nro.load_fixture(np.float64)
    n_checked = 0
    for k, name, kw in _all_cases(np.float64):
        if not nro.closed_form(kw):
            continue
        A, bA = nro.normal_equations(dict(kw, k=k))
        e, r = row_rel_err(g["A_" + nro.key_of(k, name)], A)
        assert e < 1e-9, (k, name, e, r)
        if bA is not None:
            assert np.abs(g["biasA_" + nro.key_of(k, name)] - bA).max() < 1e-9 * max(np.abs(bA).max(), 1.0), (k, name)
        n_checked += 1
    assert n_checked >= 2 * 14


def test_inputs_are_conditioned_for_float32():
    """(c) the reference's own float32 answer lies within a quarter of the float32 tolerance of its float64 answer, per row."""
    g64, g32 = nro.load_fixture(np.float64), nro.load_fixture(np.float32)
    for k, name, kw in _all_cases(np.float64):
        key = "A_" + nro.key_of(k, name)
        e, r = row_rel_err(g32[key], g64[key])
        assert e < nro.TOL32 / 4, (k, name, e, r)
        if kw.get("user_bias"):
            key = "biasA_" + nro.key_of(k, name)
            e = np.abs(g32[key].astype(np.float64) - g64[key]).max() / np.abs(g64[key]).max()
            assert e < nro.TOL32 / 4, (k, name, "bias", e)


def test_refused_cases_are_reference_defects():
    """The combinations the HIP entry point refuses because the reference does not solve the stated model: shown live where
    oracle/_ref was built (the reference returns 0, its rows are finite and they miss the normal equations by far)."""
    from oracle.bindings import Reference, ref_available
    if not ref_available(np.float64):
        pytest.skip("oracle/_ref not built")
    lib = Reference(np.float64).lib
    for k in nro.KS:
        for name, kw in nro.refused_cases(nro.problem(np.float64, k)):
            rc, A, _ = nro.call_multiple(lib, np.float64, k=k, **kw)
            assert rc == 0 and np.isfinite(A).all(), (k, name)
            assert row_rel_err(A, nro.normal_equations(dict(kw, k=k))[0])[0] > 1e-3, (k, name)
