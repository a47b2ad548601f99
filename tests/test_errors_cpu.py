"""The check of tests/errors_reference.py on a stand-in and on mutations of it, error_metrics on hand-made records and the
argument checks of EvalSet: no GPU.  What the check must accept: any summation order.  What it must reject: every way the
reduction can go wrong that the GPU test relies on it to see."""
import numpy as np
import pytest

import errors_reference as er
import predict_reference as pr
from dense_reference import Rejected

KK, N_PAIRS = 17, 1000


def _case(dtype, weights=True, implicit=False):
    """Predictions of the stand-in of the prediction tests, x and w of the held-out helper, the two masks."""
    A, B, bA, bB, gm = pr.problem(dtype, KK)
    row, col = pr.pairs(N_PAIRS)
    pred = pr.standin(A, B, None if implicit else bA, None if implicit else bB, 0.0 if implicit else gm, row, col, implicit=implicit)
    x, w = er.heldout(pred, 3, weights=weights)
    scored, fallback = er.masks(row, col, pr.M, pr.N, implicit)
    assert fallback.sum() == (0 if implicit else 15) and np.isnan(x).sum() == 3
    return pred, x, w, scored, fallback


@pytest.mark.parametrize("implicit", [False, True])
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_check_accepts_any_order(dtype, weights, implicit):
    pred, x, w, scored, fallback = _case(dtype, weights, implicit)
    worst = er.check(er.standin(pred, x, w, scored, fallback), pred, x, w, scored, fallback)
    assert worst < 1
    for seed in (1, 2):
        order = np.random.default_rng(seed).permutation(N_PAIRS)
        er.check(er.standin(pred, x, w, scored, fallback, order=order), pred, x, w, scored, fallback)
    rec = er.standin(pred, x, w, scored, fallback)
    assert int(rec["n"].sum()) + int(rec["n_skipped"]) == N_PAIRS
    assert int(rec["n_skipped"]) == int((np.isnan(x) | ~(scored | fallback)).sum())


def test_check_accepts_empty():
    z = np.zeros(0)
    rec = er.standin(z, z, None, np.zeros(0, bool), np.zeros(0, bool))
    er.check(rec, z, z, None, np.zeros(0, bool), np.zeros(0, bool))
    assert rec["n"].sum() == 0 and rec["n_skipped"] == 0


def _bad(rec, case):
    bad, _ = er.violations(rec, *case)
    with pytest.raises(Rejected):
        er.check(rec, *case)
    return bad


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_check_rejects_mutations(dtype):
    case = _case(dtype)
    pred, x, w, scored, fallback = case
    good = er.standin(*case)
    assert er.violations(good, *case)[0] == []

    # a dropped pair (a scored one with a weight and an error)
    i = int(np.flatnonzero(scored & ~np.isnan(x) & (w > 0))[5])
    keep = np.ones(N_PAIRS, bool); keep[i] = False
    rec = er.standin(pred[keep], x[keep], w[keep], scored[keep], fallback[keep])
    rec["n_skipped"] = good["n_skipped"]
    bad = _bad(rec, case)
    assert "n" in bad and "sum_wsq[0]" in bad and "sum_w[0]" in bad

    # a NaN x counted as 0
    bad = _bad(er.standin(pred, np.nan_to_num(x, nan=0.0), w, scored, fallback), case)
    assert "n" in bad and "n_skipped" in bad

    # weights ignored
    bad = _bad(er.standin(pred, x, None, scored, fallback), case)
    assert "sum_w[0]" in bad and "sum_wsq[0]" in bad and "n" not in bad

    # fallback pairs folded into class 0
    bad = _bad(er.standin(pred, x, w, scored | fallback, np.zeros(N_PAIRS, bool)), case)
    assert "n" in bad and "sum_w[1]" in bad

    # |e| and e swapped
    rec = dict(good); rec["sum_we"], rec["sum_wabs"] = good["sum_wabs"], good["sum_we"]
    bad = _bad(rec, case)
    assert set(bad) == {"sum_we[0]", "sum_we[1]", "sum_wabs[0]", "sum_wabs[1]"}

    # a maximum taken over the skipped pairs too: the NaN of x read as 0 where the prediction is the largest
    x2 = x.copy(); x2[~np.isnan(x)] = pred[~np.isnan(x)]            # no error anywhere else
    case2 = (pred, x2, w, scored, fallback)
    rec = er.standin(*case2)
    assert er.violations(rec, *case2)[0] == []
    rec["max_abs"] = er.standin(pred, np.nan_to_num(x2, nan=0.0), w, scored, fallback)["max_abs"]
    bad = _bad(rec, case2)
    assert "max_abs[0]" in bad and all(b.startswith("max_abs") for b in bad)


def test_check_rejects_float32_difference():
    """e formed in float32 for a float32 model: with x three orders of magnitude above p the float32 difference rounds (relative
    error up to 2^-24 per term, against a bound of (n + 3) 2^-52 sum |t|), and the check sees it in every sum that holds e."""
    pred, _, w, scored, fallback = _case(np.float32)
    rng = np.random.default_rng(11)
    x = (1000.0 * rng.uniform(1.0, 2.0, N_PAIRS)).astype(np.float32)
    x[[0, N_PAIRS - 1, 77]] = np.nan
    case = (pred, x, w, scored, fallback)
    assert er.violations(er.standin(*case), *case)[0] == []
    rec = er.standin(*case, e_dtype=np.float32)
    ok = scored & ~np.isnan(x)
    assert (np.abs((pred[ok] - x[ok]).astype(np.float64) - (pred[ok].astype(np.float64) - x[ok].astype(np.float64))) > 0).mean() > 0.5
    bad = _bad(rec, case)
    for name in ("sum_we[0]", "sum_wabs[0]", "sum_wsq[0]", "max_abs[0]"):
        assert name in bad, (name, bad)
    assert "sum_w[0]" not in bad and "n" not in bad


def test_error_metrics():
    from cmfrec_amd.metrics import error_metrics
    rec = dict(n=np.array([4, 2], np.uint64), n_skipped=np.uint64(3), sum_w=np.array([8.0, 2.0]), sum_we=np.array([-4.0, 1.0]),
               sum_wabs=np.array([6.0, 3.0]), sum_wsq=np.array([32.0, 8.0]), max_abs=np.array([2.5, 4.0]))
    both = error_metrics(rec)
    assert both == dict(rmse=2.0, mse=4.0, mae=0.9, bias=-0.3, max_abs=4.0, n=6, n_fallback=2, n_skipped=3, sum_w=10.0)
    only = error_metrics(rec, include_fallback=False)
    assert only == dict(rmse=2.0, mse=4.0, mae=0.75, bias=-0.5, max_abs=2.5, n=4, n_fallback=2, n_skipped=3, sum_w=8.0)
    # an empty class adds nothing
    rec1 = {k: (np.array([v[0], 0], v.dtype) if k != "n_skipped" else v) for k, v in rec.items()}
    assert error_metrics(rec1) == dict(only, n_fallback=0)
    # sum_w = 0: NaN, not an exception (no pairs at all; pairs whose weights are all zero)
    for n in (0, 5):
        zero = dict(n=np.array([n, 0], np.uint64), n_skipped=np.uint64(0), sum_w=np.zeros(2), sum_we=np.zeros(2), sum_wabs=np.zeros(2),
                    sum_wsq=np.zeros(2), max_abs=np.array([1.5 if n else 0.0, 0.0]))
        with np.errstate(all="raise"):
            got = error_metrics(zero)
        assert all(np.isnan(got[k]) for k in ("rmse", "mse", "mae", "bias"))
        assert got["n"] == n and got["sum_w"] == 0.0 and got["max_abs"] == (1.5 if n else 0.0)


def test_evalset_argument_checks(monkeypatch):
    """Every bad argument raises before the library is touched."""
    from cmfrec_amd import EvalSet, _lib

    def no_library(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_library)
    r, c, x = np.arange(4), np.arange(4), np.ones(4)
    for kw in (dict(row=np.zeros((2, 2), int)), dict(col=np.arange(3)), dict(row=np.arange(4.0)), dict(col=np.array([0, 1, 2, 2 ** 40])),
               dict(x=np.ones(3)), dict(x=np.ones((4, 1))), dict(x=np.array(["a"] * 4)), dict(w=np.ones(5)), dict(w=np.ones((2, 2))),
               dict(w=np.array([1.0, -1e-300, 1, 1])), dict(w=np.array([1.0, np.nan, 1, 1])), dict(w=np.array([1.0, np.inf, 1, 1])),
               dict(dtype=np.float16)):
        args = dict(dict(row=r, col=c, x=x), **kw)
        with pytest.raises(ValueError):
            EvalSet(**args)
    # (what is legal reaches the library: NaN in x, indices beyond any model, zero weights, no pairs)
    for kw in (dict(x=np.array([1.0, np.nan, 1, 1])), dict(row=np.array([0, -1, 2 ** 31 - 1, 3])), dict(w=np.zeros(4)),
               dict(row=np.zeros(0, int), col=np.zeros(0, int), x=np.zeros(0))):
        with pytest.raises(AssertionError, match="the library was loaded"):
            EvalSet(**dict(dict(row=r, col=c, x=x), **kw))
