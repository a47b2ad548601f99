"""GPU: the CG row kernels with the final step peeled and the next row's gather issued inside it (cg_kernels.hpp,
CMF_CG_EARLY_GATHER).  The tile of a wavefront is carried from row to row, so what matters here is a team that
solves SEVERAL rows of different tile sizes one after the other -- CMFREC_HIP_CG_TEAMS=3 caps the grid of the dynamically
scheduled kernels for that (by default a problem this small gives every team one row) -- and every way a row can leave the step
loop next to rows that take all steps.  Implicit model, k = 50 in double precision (k = 64 in single precision where marked),
against the oracle by the per-row criterion of conftest.py, as test_gpu_operators.py::test_optimizeA_implicit does.

One matrix serves all tests: 700 items, 450 users; user lengths 0 .. 72 once each (both tiny tile sizes, the 16 / 17 and 32 / 33
cuts, every tile size of the one-wavefront teams: 40/41, 48/49, 56/57, 64/65, empty row), the same boundaries times 2, 4 and 8
twice each (80 .. 512; 96 W is the cut between the launches by tile size), the other users of random lengths 1 .. 72."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from conftest import rel_err, row_rel_err

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-10, np.float32: 1e-4}      # as tests/test_gpu_operators.py
ROW_TOL = {np.float64: 1e-9, np.float32: 1e-3}
M, N = 450, 700
NZERO = 90                                       # items 0 .. NZERO-1: the group whose factors are zero in the exit test
NZERO_USERS = 14
LONG = [80, 81, 96, 97, 112, 113, 128, 129, 160, 161, 192, 193, 224, 225, 256, 257, 320, 321, 384, 385, 448, 449, 512]
K = {np.float64: 50, np.float32: 64}
LAM = 4.0
SWITCHES = ("CMFREC_HIP_CG_TEAMS", "CMFREC_HIP_CG_KERNEL", "CMFREC_HIP_POISON_LDS")


def _matrix():
    rng = np.random.default_rng(2718)
    lens = list(range(73)) + 2 * LONG
    fill = M - len(lens)
    lens = np.array(lens + list(rng.integers(1, 73, fill)), np.int64)
    zero_user = np.zeros(M, bool)
    zero_user[len(lens) - fill:len(lens) - fill + NZERO_USERS] = True      # (filler users: at most 72 <= NZERO entries)
    perm = rng.permutation(M)                                                 # row ids in no order of length
    lens, zero_user = lens[perm], zero_user[perm]
    row, col = [], []
    for u in range(M):
        pool = NZERO if zero_user[u] else N
        col.append(rng.choice(pool, size=lens[u], replace=False))
        row.append(np.full(lens[u], u))
    row = np.concatenate(row).astype(np.int32)
    col = np.concatenate(col).astype(np.int32)
    val = np.ceil(rng.lognormal(1, 1, len(row)))
    return row, col, val, lens, zero_user


@pytest.fixture(scope="module")
def problem(oracles):
    row, col, val, lens, zero_user = _matrix()
    assert (lens > 512).sum() <= 2 and set(range(73)) <= set(lens) and all((lens == l_).sum() >= 2 for l_ in LONG)
    out = dict(lens=lens, zero_user=zero_user)
    for dtype in (np.float64, np.float32):
        k = K[dtype]
        csr, csc = oracles[dtype].coo_to_csr_and_csc(row, col, val.astype(dtype), M, N)
        rng = np.random.default_rng(k)
        A0 = (rng.standard_normal((M, k)) * 0.05).astype(dtype)
        B0 = (rng.standard_normal((N, k)) * 0.2).astype(dtype)
        out[dtype] = dict(csr=csr, csc=csc, A0=A0, B0=B0)
    return out


@contextmanager
def _env(env):
    old = {n_: os.environ.pop(n_, None) for n_ in SWITCHES}
    os.environ.update(env)
    try:
        yield
    finally:
        for n_ in SWITCHES:
            os.environ.pop(n_, None)
            if old[n_] is not None:
                os.environ[n_] = old[n_]


def _device(problem, dtype, steps, env, A0=None, B0=None, lam=LAM):
    """update("A"), then update("B") from the new A (the switches are read when the session is created)."""
    from cmfrec_amd.session import AlsSession
    p = problem[dtype]
    with _env(env):
        s = AlsSession(M, N, K[dtype], implicit=True, dtype=dtype, lam=lam, use_cg=True, max_cg_steps=steps)
        try:
            s.set_X(p["csr"], p["csc"])
            s.set_factors(A=p["A0"] if A0 is None else A0, B=p["B0"] if B0 is None else B0)
            s.update("A")
            s.update("B")
            f = s.get_factors()
            return np.array(f["A"]), np.array(f["B"])
        finally:
            s.close()


def _oracle(oracles, problem, dtype, steps, A0=None, B0=None, lam=LAM):
    p = problem[dtype]
    A = (p["A0"] if A0 is None else A0).copy()
    B = (p["B0"] if B0 is None else B0).copy()
    oracles[dtype].optimizeA_implicit(A, B, p["csr"], lam, nthreads=4, use_cg=True, max_cg_steps=steps)
    oracles[dtype].optimizeA_implicit(B, A, p["csc"], lam, nthreads=4, use_cg=True, max_cg_steps=steps)
    return A, B


_cache = {}


def _cached(kind, key, fn):
    if (kind, key) not in _cache:
        got = fn()
        for a in got:
            a.setflags(write=False)
        _cache[(kind, key)] = got
    return _cache[(kind, key)]


def _check(got, exp, dtype, what):
    for g, e, side in zip(got, exp, "AB"):
        assert np.isfinite(g).all(), (what, side)
        assert rel_err(g, e) < TOL[dtype], (what, side)
        err, r = row_rel_err(g, e)
        assert err < ROW_TOL[dtype], "%s %s row %d: per-row relative error %.3e" % (what, side, r, err)


CASES = [(np.float64, 3), (np.float64, 1), (np.float32, 3), (np.float32, 1)]
IDS = ["f64-3", "f64-1", "f32-3", "f32-1"]


@pytest.mark.parametrize("dtype,steps", CASES, ids=IDS)
@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poisoned"])
def test_steady_state(oracles, problem, dtype, steps, poison):
    """Teams that solve many rows one after the other (three teams) and teams of one or two rows (grid by occupancy): both match
    the oracle, and a row's bits do not depend on the team that solved it or on what that team solved before."""
    exp = _cached("oracle", (dtype, steps), lambda: _oracle(oracles, problem, dtype, steps))
    extra = {"CMFREC_HIP_POISON_LDS": "1"} if poison else {}
    few = _cached("dev", (dtype, steps, 3, poison), lambda: _device(problem, dtype, steps, dict(extra, CMFREC_HIP_CG_TEAMS="3")))
    dflt = _cached("dev", (dtype, steps, 0, poison), lambda: _device(problem, dtype, steps, extra))
    _check(few, exp, dtype, "three teams")
    _check(dflt, exp, dtype, "default grid")
    assert np.array_equal(few[0], dflt[0]) and np.array_equal(few[1], dflt[1])


def _count_exits(csr, A0, B, lam, steps):
    """The reference's factors_implicit_cg (src/common.c) restated row by row: which way each row leaves it --
    'start' (first residual <= 1e-12), 'early' (r_new <= 1e-8 in a step before the last), 'full' (every step taken; empty rows: None)."""
    p, idx, x = (np.asarray(a) for a in csr)
    BtB = B.T @ B
    exits = []
    for u in range(len(p) - 1):
        j = idx[int(p[u]):int(p[u + 1])]
        if len(j) == 0:
            exits.append(None)
            continue
        Bu, xu, a = B[j], x[int(p[u]):int(p[u + 1])], A0[u].copy()
        coef = Bu @ a
        r = -(BtB @ a) + Bu.T @ (-(coef - 1.) * xu - coef) - lam * a
        pv = r.copy()
        r_old = r @ r
        if r_old <= 1e-12:
            exits.append("start")
            continue
        how = "full"
        for step in range(steps):
            coef = Bu @ pv
            Ap = BtB @ pv + Bu.T @ (coef * (xu - 1.) + coef) + lam * pv
            al = r_old / (Ap @ pv)
            a += al * pv
            r -= al * Ap
            r_new = r @ r
            if r_new <= 1e-8:
                if step < steps - 1:
                    how = "early"
                break
            pv = pv * (r_new / r_old) + r
            r_old = r_new
        exits.append(how)
    return exits


def test_every_exit_next_to_full_rows(oracles, problem):
    """Rows that never enter the step loop, rows that leave it before the last step and rows that take every step, mixed in the
    processing order (rows sorted by length) of three teams: the gather of the next row starts in the peeled step of a row that
    reaches it and behind the loop of one that does not."""
    dtype, steps = np.float64, 3
    p = problem[dtype]
    zu = problem["zero_user"]
    A0 = p["A0"].copy()
    A0[zu] = 0
    B0 = p["B0"].copy()
    B0[:NZERO] = 0
    counts = {"start": 0, "early": 0, "full": 0}
    runs = []
    for lam, Bs in ((LAM, B0), (1e4, B0 * 1e-3)):
        ex = _count_exits(p["csr"], A0, Bs, lam, steps)
        for e in ex:
            if e is not None:
                counts[e] += 1
        runs.append((lam, Bs, ex))
    assert min(counts.values()) >= 10, counts
    # different exits alternate in the order the rows are processed in (longest first, stable)
    order = np.argsort(-problem["lens"], kind="stable")
    for lam, Bs, ex in runs:
        seq = [ex[u] for u in order if ex[u] is not None]
        assert sum(a != b for a, b in zip(seq, seq[1:])) >= 10, (lam, counts)
    for lam, Bs, ex in runs:
        got = _device(problem, dtype, steps, {"CMFREC_HIP_CG_TEAMS": "3"}, A0=A0, B0=Bs, lam=lam)
        exp = _oracle(oracles, problem, dtype, steps, A0=A0, B0=Bs, lam=lam)
        _check(got, exp, dtype, "lam %g" % lam)
        start = np.array([e == "start" for e in ex])
        assert np.array_equal(got[0][start], A0[start])       # (a row that never enters the loop keeps its start value)


@pytest.mark.parametrize("steps", [3, 1])
def test_against_generic_kernel(oracles, problem, steps):
    """The lane <-> unknown kernel (CMFREC_HIP_CG_KERNEL=generic), which this change does not touch, on the same half-steps: to
    the tolerance of tests/test_gpu_switches.py."""
    dtype = np.float64
    few = _cached("dev", (dtype, steps, 3, False), lambda: _device(problem, dtype, steps, {"CMFREC_HIP_CG_TEAMS": "3"}))
    gen = _device(problem, dtype, steps, {"CMFREC_HIP_CG_KERNEL": "generic"})
    for a, b, side in zip(few, gen, "AB"):
        assert np.isfinite(a).all() and np.isfinite(b).all(), side
        assert np.abs(a - b).max() <= 1e-10 * max(np.abs(b).max(), 1e-30), (side, float(np.abs(a - b).max()))
