"""The implicit model's CG beyond 64 factors on rows of more than 256 entries (chol_wave_kernel WMODE 3 + gram_cg_wide_kernel<T, true>):
one B-step of an AlsSession against a float64 NumPy restatement of factors_implicit_cg.  Bounds of the long-row CG tests
(test_gpu_sweep.py): 1e-7 in double, 1e-2 in single, times max(1, max |expected|).  They discriminate: dropping the -(x_j + 1) B_j.a term
of the right-hand side moves this problem's factors by 0.3, the row's Gramian met with a in the first residual by 0.2."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from implicit_cg_reference import compressed, first_residual_roots, implicit_cg_half_step

pytestmark = pytest.mark.gpu
M, N, LAM = 1500, 30, 2.0
HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def problem():
    """Item 0: 1497 entries (sliced), item 1 cut to 257, item 2 to 256 (the generic kernel in the same half-step), item 3 none."""
    rng = np.random.default_rng(93)
    lin = rng.choice(M * N, size=19000, replace=False)
    row, col = (lin // N).astype(np.int32), (lin % N).astype(np.int32)
    extra = np.setdiff1d(np.arange(M, dtype=np.int32), row[col == 0])[:877]
    row, col = np.concatenate([row, extra]), np.concatenate([col, np.zeros(len(extra), np.int32)])
    keep = col != 3
    keep[np.flatnonzero(col == 1)[257:]] = keep[np.flatnonzero(col == 2)[256:]] = False
    row, col = row[keep], col[keep]
    cnt = np.bincount(col, minlength=N)
    assert (cnt[:4] == [1497, 257, 256, 0]).all() and len(row) % 4 and (cnt > 256).sum() == N - 2
    return row, col, 0.5 * rng.integers(1, 11, len(row))


def start(dtype, k):
    rng = np.random.default_rng(1000 + k)
    return (0.1 * rng.standard_normal((M, k))).astype(dtype), (0.1 * rng.standard_normal((N, k))).astype(dtype)


def expected(dtype, k, steps):
    A0, B0 = start(dtype, k)
    return implicit_cg_half_step(B0, A0, *compressed(problem()[1], problem()[0], problem()[2].astype(dtype), N), LAM, steps)


def b_step(dtype, k, steps, B0=None, q=0, **model):
    """(B, rows on the Gramian CG) after one CG B-step of a session; q: columns of dense item side information."""
    from cmfrec_amd.session import AlsSession
    row, col, val = problem()
    A0, B00 = start(dtype, k)
    rng = np.random.default_rng(7)
    s = AlsSession(M, N, k, implicit=True, dtype=dtype, lam=LAM, use_cg=True, max_cg_steps=steps, q=q, n_i=N if q else 0, **model)
    try:
        s.set_X_coo(row, col, val.astype(dtype))
        if q:
            s.set_sideinfo(None, rng.standard_normal((N, q)).astype(dtype))
        s.set_factors(A=A0, B=B00 if B0 is None else B0, Dm=(0.1 * rng.standard_normal((q, k))).astype(dtype) if q else None)
        s.update("B")
        return s.get_factors()["B"], s.cg_wide_rows(1)
    finally:
        s.close()


def within(got, exp, dtype):
    tol = 1e-7 if dtype is np.float64 else 1e-2
    err = np.abs(got.astype(np.float64) - exp)
    assert np.isfinite(got).all() and err.max() <= tol * max(1.0, np.abs(exp).max())
    if dtype is np.float64:                                   # row by row as well
        assert (err.max(axis=1) <= tol * np.maximum(1.0, np.abs(exp).max(axis=1))).all()


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("k", [65, 80, 100, 128, 129])       # 4 blocks + border; 5 of 6; 7 of 8 (two sweeps in double); 8; 8 + border
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_b_step_against_reference(dtype, k, steps):
    got, rows = b_step(dtype, k, steps)
    assert rows == N - 2                                      # every item beyond 256 entries (0 on a build without the route)
    within(got, expected(dtype, k, steps), dtype)


@pytest.mark.parametrize("env,rows", [(dict(CMFREC_HIP_CG_KERNEL="generic"), 0), (dict(CMFREC_HIP_CG_WIDE_MIN="1024"), 1)])
def test_switches_in_child_process(tmp_path, env, rows):
    """The generic kernel everywhere / only item 0 on the route: the rows counted, the factors within the bound of the default route's
    and of the reference."""
    code = ("import sys, numpy as np; sys.path[:0] = [%r, %r]; import test_gpu_implicit_cg_wide as t; "
            "B, rows = t.b_step(np.float64, 100, 3); np.save(sys.argv[1], B); print('rows', rows)" % (HERE, os.path.dirname(HERE)))
    out = subprocess.run([sys.executable, "-c", code, str(tmp_path / "B.npy")], capture_output=True, text=True, env=dict(os.environ, **env))
    assert out.returncode == 0 and out.stdout.split()[-2:] == ["rows", str(rows)], out.stderr[-2000:]
    within(b_step(np.float64, 100, 3)[0], np.load(tmp_path / "B.npy"), np.float64)
    within(np.load(tmp_path / "B.npy"), expected(np.float64, 100, 3), np.float64)


def test_early_exit_leaves_the_row():
    """From the root of the reference's first residual (a closed-form solve of that residual's own system: quirk Q1 makes it another point
    than the closed-form half-step's solution) r.r <= 1e-12: every row stays as it is, bit for bit, and so after a second call."""
    row, col, val = problem()
    root = first_residual_roots(start(np.float64, 100)[0], *compressed(col, row, val, N), LAM)
    got, rows = b_step(np.float64, 100, 3, B0=root)
    assert rows == N - 2 and np.array_equal(got, root)
    assert np.array_equal(b_step(np.float64, 100, 3, B0=got)[0], root)


@pytest.mark.parametrize("model", [dict(precondition_cg=True), dict(q=4, w_item=0.5)], ids=["pcg", "dense_side_info"])
def test_models_that_stay_on_the_generic_kernel(model, monkeypatch):
    got, rows = b_step(np.float64, 100, 3, **model)
    monkeypatch.setenv("CMFREC_HIP_CG_KERNEL", "generic")     # (read when the next session is created)
    assert rows == 0 and np.isfinite(got).all() and np.array_equal(got, b_step(np.float64, 100, 3, **model)[0])
