"""The subspace (iALS++) half-step (subspace_kernels.hpp): one half-step against the float64 block sweep
of subspace_reference.py within its bound, the closed form as its fixed point, the same bytes twice, the fit against the session
loop with a falling objective, and the refusals."""
import functools

import numpy as np
import pytest

import subspace_reference as ref
from conftest import make_coo
from topn_reference import gamma

gpu = pytest.mark.gpu
F64, F32 = np.float64, np.float32
LENS = [0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 300] * 2
M, N, LAM = len(LENS), 320, 2.0
HOOKS = {"uncapped": None, "one_workgroup": ("CMFREC_HIP_SUBSPACE_WAVES", "4"), "lds_32": ("CMFREC_HIP_SUBSPACE_LDS_ROWS", "32")}
KS = (3, 16, 17, 50, 64, 65, 128, 255, 256)
MODELS = ("implicit", "explicit", "bias")


def csr_csc(row, col, val, m, n):
    out = []
    for key, other, rows in ((row, col, m), (col, row, n)):
        o = np.argsort(key, kind="stable")
        out.append((np.concatenate([[0], np.cumsum(np.bincount(key, minlength=rows))]).astype(np.uint64), other[o].astype(np.int32), val[o]))
    return out


@functools.lru_cache(maxsize=None)
def problem(dtype, k, model):
    """Start values, CSR / CSC, and the reference's A-step and B-step (the B-step from the reference's A, rounded to dtype)."""
    rng = np.random.default_rng(k + 1000 * MODELS.index(model))
    row = np.repeat(np.arange(M), LENS).astype(np.int32)
    col = np.concatenate([rng.permutation(N)[:h] for h in LENS]).astype(np.int32)
    val = (rng.uniform(0.5, 3.0, len(row)) if model == "implicit" else rng.standard_normal(len(row))).astype(dtype)
    csr, csc = csr_csc(row, col, val, M, N)
    A0, B0 = (0.3 * rng.standard_normal((M, k))).astype(dtype), (0.3 * rng.standard_normal((N, k))).astype(dtype)
    bA0 = (0.1 * rng.standard_normal(M)).astype(dtype) if model == "bias" else None
    sweeps = 1 + (KS.index(k) + MODELS.index(model)) % 2
    imp, ext = model == "implicit", model == "bias"                   # ext: the row [b_j, 1] and the bias as the last unknown
    Ax, Bx = (np.c_[A0, bA0], np.c_[B0, np.ones(N, dtype)]) if ext else (A0, B0)
    wantA, boundA = ref.half_step(Ax, Bx, csr, np.full(Ax.shape[1], LAM), imp, sweeps, dtype)
    A1, bA1 = wantA[:, :k].astype(dtype), (wantA[:, k].astype(dtype) if ext else None)
    wantB, boundB = ref.half_step(B0, A1, csc, np.full(k, LAM), imp, sweeps, dtype, bias_sub=bA1)
    return dict(csr=csr, csc=csc, A0=A0, B0=B0, bA0=bA0, sweeps=sweeps, wantA=wantA, boundA=boundA, A1=A1, bA1=bA1, wantB=wantB, boundB=boundB)


def session(dtype, k, model, P, **kw):
    from cmfrec_amd import AlsSession
    s = AlsSession(M, N, k, model == "implicit", dtype=dtype, lam=LAM, user_bias=model == "bias", **kw)
    s.set_X(P["csr"], P["csc"])
    return s


def step_A(s, P, **kw):
    s.set_factors(P["A0"], P["B0"], P["bA0"])
    s.update("A", **kw); s.after_gather("A")
    f = s.get_factors()
    return f["A"] if f["biasA"] is None else np.c_[f["A"], f["biasA"]]


def step_AB(s, P):
    """(A after the A-step from the start values, B after the B-step from the reference's A)"""
    a = step_A(s, P)
    s.set_factors(P["A1"], P["B0"], P["bA1"]); s.update("B")
    return a, s.get_factors()["B"]


def worst(got, want, bound, rows):
    err = np.linalg.norm(np.asarray(got, np.float64) - want, axis=1)
    assert np.all(np.isfinite(err[rows]))
    return float((err[rows] / bound[rows]).max())


@gpu
@pytest.mark.parametrize("hook", list(HOOKS))
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("dtype", (F64, F32), ids=("f64", "f32"))
def test_half_step_against_reference(dtype, model, k, hook, monkeypatch):
    P = problem(dtype, k, model)
    s = session(dtype, k, model, P)
    s.set_subspace(16, P["sweeps"])
    raw = lambda ab: (ab[0].tobytes(), ab[1].tobytes())
    uncapped = raw(step_AB(s, P)) if hook == "one_workgroup" else None
    if HOOKS[hook]:
        monkeypatch.setenv(*HOOKS[hook])
    first, (gotA, gotB) = raw(step_AB(s, P)), step_AB(s, P)
    assert first == raw((gotA, gotB))                                         # two calls, the same bytes
    assert uncapped in (None, first)                                          # the same route on fewer wavefronts: the same bytes
    empty, seen = np.array(LENS) == 0, np.diff(P["csc"][0].astype(np.int64)) > 0
    assert gotA[empty, :k].tobytes() == P["A0"][empty].tobytes()              # rows without entries: untouched, as the CG route
    assert gotB[~seen].tobytes() == P["B0"][~seen].tobytes()
    ratios = worst(gotA, P["wantA"], P["boundA"], ~empty), worst(gotB, P["wantB"], P["boundB"], seen)
    print("subspace error / bound %s: A %.3g B %.3g" % ((dtype.__name__,) + ratios))
    assert max(ratios) <= 1.0


def closed_form(A, B, csr, k, imp, dtype=F64):
    """For the rows with entries (the others: as in A, 0): the float64 closed form, and gamma_m cond_2(W_u) |A[u]| of the closed
    form's own chain (potrf, two solves, the rank-k sum, as explain_reference.py counts them)."""
    G0, A = (np.asarray(B, np.float64).T @ np.asarray(B, np.float64) if imp else None), np.array(A, np.float64)
    sol, bound = A.copy(), np.zeros(len(A))
    for u in np.flatnonzero(np.diff(csr[0].astype(np.int64))):
        sl = slice(int(csr[0][u]), int(csr[0][u + 1]))
        W, r = ref.row_system(B, csr[1][sl], csr[2][sl], np.full(k, LAM), imp, G0=G0)
        h, sol[u] = sl.stop - sl.start, np.linalg.solve(W, r)
        bound[u] = gamma((k + 1) + 2 * k + (h + (h + 255) // 256 + 2), dtype) * np.linalg.cond(W) * np.linalg.norm(A[u])
    return sol, bound


@pytest.mark.parametrize("model", ("implicit", "explicit"))
def test_reference_keeps_the_closed_form(model):
    """CPU: the NumPy block sweep started at the float64 closed form stays there within the closed form's own bound."""
    k, imp, P = 50, model == "implicit", problem(F64, 50, model)
    A, _ = closed_form(P["A0"], P["B0"], P["csr"], k, imp)
    after, _ = ref.half_step(A, P["B0"], P["csr"], np.full(k, LAM), imp, 1, F64)
    assert np.all(np.linalg.norm(after - A, axis=1) <= closed_form(A, P["B0"], P["csr"], k, imp)[1])


@gpu
@pytest.mark.parametrize("k", (17, 128))
@pytest.mark.parametrize("model", ("implicit", "explicit"))
@pytest.mark.parametrize("dtype", (F64, F32), ids=("f64", "f32"))
def test_closed_form_is_the_fixed_point(dtype, model, k):
    P = problem(dtype, k, model)
    s = session(dtype, k, model, P)
    star = step_A(s, P, use_cholesky=True)
    s.set_subspace(16, 1)
    s.update("A")
    moved = np.linalg.norm(s.get_factors()["A"].astype(np.float64) - star, axis=1)
    rows = np.array(LENS) > 0
    assert np.all(moved[rows] <= closed_form(star, P["B0"], P["csr"], k, model == "implicit", dtype)[1][rows])


@gpu
def test_indefinite_row_is_nan_and_alone():
    P = dict(problem(F64, 17, "implicit"))
    s = session(F64, 17, "implicit", P)
    s.set_subspace(16, 1)
    clean, val, bad = step_A(s, P), P["csr"][2].copy(), LENS.index(5)
    val[int(P["csr"][0][bad])] = -1e6
    P["csr"] = (P["csr"][0], P["csr"][1], val)
    s.set_X(P["csr"], P["csc"])
    got = step_A(s, P)
    others = np.arange(M) != bad
    assert np.all(np.isnan(got[bad])) and got[others].tobytes() == clean[others].tobytes()


@gpu
def test_fit_is_the_session_loop_and_the_objective_falls():
    from cmfrec_amd import AlsSession, CMF_implicit, Subspace, metrics
    m, n, k, lam = 200, 150, 20, 3.0
    row, col, val = make_coo(m, n, 4000, 7)
    rng = np.random.default_rng(3)
    A0, B0 = 0.1 * rng.standard_normal((m, k)), 0.1 * rng.standard_normal((n, k))
    mdl = CMF_implicit(k=k, lambda_=lam, niter=3, use_float=False).fit((row, col, val), shape=(m, n), A0=A0, B0=B0, subspace=Subspace())
    assert mdl.solver_ == "subspace"
    s = AlsSession(m, n, k, True, dtype=F64, lam=lam)
    s.set_X_coo(row, col, val)
    s.set_factors(A0, B0)
    s.set_subspace(16, 1)
    n_terms = len(val) + (m + n) * k * (k + 1)          # the entries, the squared norms, the products of the two Gramians
    obj = [metrics.objective_from_record(s.objective(), lam)]
    for which in "BABABA":
        s.update(which)
        obj.append(metrics.objective_from_record(s.objective(), lam))
        assert obj[-1] <= obj[-2] + n_terms * np.finfo(F64).eps * abs(obj[-2])
    f = s.get_factors()
    assert f["A"].tobytes() == mdl.A_.tobytes() and f["B"].tobytes() == mdl.B_.tobytes()


@gpu
def test_explicit_fit_ends_on_the_closed_form():
    from cmfrec_amd import CMF, Subspace
    m, n, k = 60, 40, 20                        # two blocks; CMF's default finalize_chol makes the last iteration the closed form
    row, col, val = make_coo(m, n, 600, 1)
    mdl = CMF(k=k, lambda_=LAM, niter=3, user_bias=False, item_bias=False, center=False, use_float=False)
    mdl.fit((row, col, val), shape=(m, n), subspace=Subspace())
    csr, rows = csr_csc(row, col, val.astype(F64), m, n)[0], np.bincount(row, minlength=m) > 0
    want, bound = closed_form(mdl.A_, mdl.B_, csr, k, False)
    assert mdl.solver_ == "subspace"
    assert np.all(np.linalg.norm(mdl.A_ - want, axis=1)[rows] <= bound[rows])


REFUSALS = {   # option -> (model, session arguments, what sets it on the session, arguments of set_subspace, the fit that meets it)
    "side information": ("explicit", dict(p=3, m_u=M), lambda s, P: (s.set_sideinfo(U=np.ones((M, 3))), s.set_factors(Cm=np.full((3, 16), 0.1))), (16, 1), None),
    "implicit features": ("explicit", {}, lambda s, P: s.set_implicit_features(0.5), (16, 1), None),
    "nonneg": ("implicit", {}, lambda s, P: s.set_nonneg(True), (16, 1), ("CMF_implicit", dict(nonneg=True), {})),
    "L1": ("implicit", {}, lambda s, P: s.set_lam_unique(None, np.full(6, 0.1)), (16, 1), ("CMF_implicit", dict(l1_lambda=0.1), dict(objective=True))),
    "lam_unique": ("implicit", {}, lambda s, P: s.set_lam_unique(np.array([LAM, LAM, 1.0, 3.0, LAM, LAM])), (16, 1), None),
    "NA_as_zero_X": ("explicit", {}, lambda s, P: s.set_NA_as_zero_X(True), (16, 1), None),
    "observation weights": ("explicit", {}, lambda s, P: s.set_X(P["csr"] + (np.ones_like(P["csr"][2]),), P["csc"] + (np.ones_like(P["csc"][2]),)), (16, 1), ("CMF", {}, dict(W=np.ones(600)))),
    "scale_lam": ("explicit", dict(scale_lam=True), lambda s, P: None, (16, 1), ("CMF", dict(scale_lam=True), {})),
    "set_A_parts": ("implicit", {}, lambda s, P: s.set_A_parts(P["csr"], 2), (16, 1), None),
    "block": ("implicit", {}, lambda s, P: None, (8, 1), None),
    "sweeps": ("implicit", {}, lambda s, P: None, (16, 0), None),
    "dense X": ("explicit", {}, None, None, ("CMF", {}, dict(X=np.random.default_rng(0).standard_normal((20, 15))))),
}


@gpu
@pytest.mark.parametrize("option", list(REFUSALS))
def test_refusals_leave_everything_as_it_was(option):
    import cmfrec_amd
    model, kw, setup, args, fit = REFUSALS[option]
    if args is not None:
        P = problem(F64, 16, model)
        asked, twin = session(F64, 16, model, P, **kw), session(F64, 16, model, P, **kw)
        setup(asked, P); setup(twin, P)
        with pytest.raises(RuntimeError, match=option):
            asked.set_subspace(*args)
        assert step_A(asked, P).tobytes() == step_A(twin, P).tobytes()
    if fit is not None:     # the same message from a fit (L1: refused for its objective first); the next fit as if nobody had asked
        row, col, val = make_coo(60, 40, 600, 1)
        run = lambda ckw, **fkw: getattr(cmfrec_amd, fit[0])(k=4, niter=2, use_float=False, **ckw).fit(**{"X": (row, col, val), "shape": (60, 40), **fkw})
        never = run({})
        with pytest.raises(RuntimeError, match=option):
            run(fit[1], subspace=cmfrec_amd.Subspace(), **(dict(objective=cmfrec_amd.Objective()) if "objective" in fit[2] else fit[2]))
        after = run({})
        assert after.solver_ == "cg" and (after.A_.tobytes(), after.B_.tobytes()) == (never.A_.tobytes(), never.B_.tobytes())
