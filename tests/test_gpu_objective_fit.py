"""fit(..., objective=Objective(...)): the objective of a Cholesky fit in double precision never rises, agrees with the resident
session's on the returned factors, and `tol` stops the fit on the iterate a shorter plain fit returns."""
import numpy as np
import pytest

from objective_reference import reference_and_bound

pytestmark = pytest.mark.gpu

M, N, K, LAM = 60, 40, 8, 3.


def data(implicit):
    rng = np.random.default_rng(5)
    mask = rng.random((M, N)) < 0.25
    V = np.ceil(rng.lognormal(0, 1, (M, N))) if implicit else rng.standard_normal((M, N)) + 3.
    row, col = np.nonzero(mask)
    return mask, V, (row.astype(np.int32), col.astype(np.int32), V[mask])


def model(implicit, niter, **kw):
    from cmfrec_amd import CMF, CMF_implicit
    common = dict(k=K, lambda_=LAM, niter=niter, use_cg=False, use_float=False, finalize_chol=False, precompute_for_predictions=False, **kw)
    return CMF_implicit(**common) if implicit else CMF(scale_lam=False, **common)


def evaluation_bound(implicit, mdl, mask, V):
    """b: the forward bound of the composed objective, from the components' bounds on the model's factors"""
    stored = V if implicit else V - mdl.glob_mean_
    _, bound = reference_and_bound(np.float64, implicit, mdl.A_, mdl.B_, mask, stored, None,
                                   None if implicit else mdl.user_bias_, None if implicit else mdl.item_bias_)
    pen = bound["normA"][0] + bound["normB"][0] + bound["normbiasA"][0] + bound["normbiasB"][0]
    return float(0.5 * (bound["data"] + bound["allpairs"]) + 0.5 * LAM * pen)


@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
def test_history_never_rises_and_agrees_with_the_session(implicit):
    from cmfrec_amd import AlsSession, Objective
    from cmfrec_amd.metrics import objective_from_record
    mask, V, X = data(implicit)
    hist, b = [], []
    for niter in range(1, 7):            # the factors after every iteration, for the bound of that iteration's evaluation
        mdl = model(implicit, niter).fit(X, shape=(M, N), objective=Objective(every=1))
        assert mdl.n_iter_ == niter and len(mdl.objective_history_) == niter
        assert [h["objective"] for h in mdl.objective_history_[:-1]] == hist            # the same fit, one iteration further
        hist.append(mdl.objective_history_[-1]["objective"])
        b.append(evaluation_bound(implicit, mdl, mask, V))
    print("objective", hist, "bounds", b)
    for t in range(5):                   # an exact block minimiser cannot raise the objective
        assert hist[t + 1] <= hist[t] + b[t] + b[t + 1], (t, hist)
    assert hist[5] < hist[0]
    # a session loaded with the returned factors gives the same number
    s = AlsSession(M, N, K, implicit, lam=LAM, user_bias=not implicit, item_bias=not implicit)
    s.set_X_coo(X[0], X[1], X[2], subtract=0. if implicit else mdl.glob_mean_)
    s.set_factors(mdl.A_, mdl.B_, None if implicit else mdl.user_bias_, None if implicit else mdl.item_bias_)
    f = objective_from_record(s.objective(), lambda_=LAM)
    s.close()
    assert abs(f - hist[-1]) <= b[-1], (f, hist[-1], b[-1])
    assert abs(objective_from_record(mdl.objective_history_[-1], lambda_=LAM) - hist[-1]) <= 4 * np.finfo(np.float64).eps * abs(hist[-1])


@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
def test_tol_stops_on_the_iterate_of_a_shorter_fit(implicit):
    from cmfrec_amd import Objective
    _, _, X = data(implicit)
    stopped = model(implicit, 6).fit(X, shape=(M, N), objective=Objective(every=1, tol=0.5))
    assert 2 <= stopped.n_iter_ < 6 and len(stopped.objective_history_) == stopped.n_iter_
    h = [e["objective"] for e in stopped.objective_history_]
    assert h[-2] - h[-1] <= 0.5 * abs(h[-2])
    plain = model(implicit, stopped.n_iter_).fit(X, shape=(M, N))
    assert plain.objective_history_ == [] and plain.n_iter_ == stopped.n_iter_
    assert stopped.A_.tobytes() == plain.A_.tobytes() and stopped.B_.tobytes() == plain.B_.tobytes()
    if not implicit:
        assert stopped.user_bias_.tobytes() == plain.user_bias_.tobytes() and stopped.item_bias_.tobytes() == plain.item_bias_.tobytes()
