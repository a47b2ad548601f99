"""CPU: the recorded reference rows of the missing-as-zero new-rows cases (fixture g43, tests/new_rows_naz.py) against the float64
normal equations of the model written out in NumPy -- the fixture is only as good as that agreement."""
import numpy as np
import pytest

import new_rows_naz as nrz


def _errors(g, kw, k, name):
    A, bA = nrz.normal_equations(dict(kw, k=k))
    key = nrz.key_of(k, name)
    err = np.abs(g["A_" + key] - A).max() / np.abs(A).max()
    if bA is not None:
        err = max(err, np.abs(g["biasA_" + key] - bA).max() / np.abs(bA).max())
    return err


@pytest.mark.parametrize("dtype,bar", [(np.float64, 1e-8), (np.float32, nrz.TOL32 / 4)], ids=["f64", "f32"])
def test_fixture_agrees_with_normal_equations(dtype, bar):
    """Every recorded case: within 1e-8 in float64 (the bar of the recorder), within a quarter of TOL32 in float32."""
    g = nrz.load_fixture(dtype)
    bad = []
    for k in nrz.KS:
        d = nrz.problem(dtype, k)
        for name, kw in nrz.cases(d):
            err = _errors(g, kw, k, name)
            print("k=%d %s: %.2e" % (k, name, err))
            if not err < bar:
                bad.append((k, name, err))
    assert not bad, bad


def test_fixture_holds_the_required_cases():
    """Nothing is dropped silently: every case of the module is in both fixtures, the eight kinds the model was confirmed on are
    among them, biasB is passed wherever glob_mean != 0, and side information sits on exactly the batch's rows as CSR."""
    for dtype in (np.float64, np.float32):
        g = nrz.load_fixture(dtype)
        for k in nrz.KS:
            d = nrz.problem(dtype, k)
            cs = nrz.cases(d)
            for name, kw in cs:
                key = nrz.key_of(k, name)
                assert "A_" + key in g.files, key
                assert ("biasA_" + key in g.files) == bool(kw.get("user_bias")), key
                assert kw.get("NA_as_zero_X") or kw.get("NA_as_zero_U")
                assert not kw.get("glob_mean") or kw.get("biasB") is not None, name
                if kw.get("U") is not None:
                    assert kw["U"].shape[0] == kw["m"], name
                if kw.get("U_csr") is not None:
                    assert kw["U_csr"][3] == kw["m"], name
            has = lambda v: v is not None and (isinstance(v, np.ndarray) or bool(v))
            f = lambda **want: any(all(has(kw.get(a)) == b for a, b in want.items()) for _, kw in cs)
            X, U = "NA_as_zero_X", "NA_as_zero_U"
            assert f(**{X: True, U: False, "weight": False, "biasB": False, "Cm": False, "scale_lam": False})          # X alone
            assert f(**{X: True, "biasB": True, "glob_mean": True, "user_bias": True, "weight": False, "scale_lam": False})
            assert f(**{X: True, "biasB": True, "glob_mean": True, "user_bias": True, "weight": True})
            assert any(kw.get(X) and kw.get("U") is not None and kw.get("k_user") and kw.get("k_item") and kw.get("k_main")
                       and kw.get("U_colmeans") is not None and kw.get("w_user", 1.0) != 1.0 for _, kw in cs)
            assert any(kw.get(X) and kw.get(U) and kw.get("U_csr") is not None and kw.get("U_colmeans") is not None for _, kw in cs)
            assert any(not kw.get(X) and kw.get(U) and kw.get("U_csr") is not None for _, kw in cs)
            assert f(**{X: True, "scale_lam": True, "user_bias": True})
            assert f(**{X: True, "scale_lam": True, "user_bias": False, "weight": False})
            assert f(**{X: True, "scale_lam": True, "user_bias": False, "weight": True})
            for name, kw in nrz.numpy_only_cases(d):
                assert "A_" + nrz.key_of(k, name) not in g.files


def test_normal_equations_reduce_to_the_ordinary_model():
    """With both options off the module's normal equations are those of tests/new_rows_options.py."""
    import new_rows_options as nro
    d = nrz.problem(np.float64, 6)
    kw = dict(row=d["row"], col=d["col"], val=d["ratings"], m=d["m"], B=d["B_plain"], biasB=d["biasB"], glob_mean=3.1, user_bias=True,
              lam=0.6, lam_bias=1.1, scale_lam=True, k=6)
    A0, b0 = nro.normal_equations(kw)
    A1, b1 = nrz.normal_equations(kw)
    assert np.abs(A0 - A1).max() < 1e-12 and np.abs(b0 - b1).max() < 1e-12


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_extended_model_mirror(dtype):
    """cmfrec_hip_newrows_model_ex is the model (unchanged: tests/test_new_users_host.py pins its size) with the two options at its end;
    the library and the ctypes mirror agree on it."""
    import ctypes as C
    from cmfrec_amd import _lib
    lib = C.CDLL(_lib.lib_path(dtype))
    base, ex = _lib.newrows_model_mirror(dtype), _lib.newrows_model_ex_mirror(dtype)
    assert lib.cmfrec_hip_sizeof_newrows_model_ex() == C.sizeof(ex) == C.sizeof(base) + 8
    assert [f[0] for f in ex._fields_] == ["base", "NA_as_zero_X", "NA_as_zero_U"] and ex.base.offset == 0 and ex._fields_[0][1] is base
