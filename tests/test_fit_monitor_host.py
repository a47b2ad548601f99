"""The host side of validation while fitting, no device: the rule of the monitor (cmfrec_hip_early_stop_step through ctypes) on
hand-made sequences, the argument checks of cmfrec_amd.Validation, and the ctypes mirrors of the two structs."""
import ctypes as C
import math

import numpy as np
import pytest

from cmfrec_amd import _lib
from cmfrec_amd.validation import ERROR_METRICS, RANKING_METRICS, Validation

NAN = float("nan")


def run_rule(values, niter=None, every=1, patience=0, min_delta=0.0, higher=False):
    """Drives the rule as run_loop does over `values` (one per iteration; entries of iterations the rule does not evaluate are
    never read).  Returns (evaluated iterations, improved iterations, iterations run, best_iter, best)."""
    lib = C.CDLL(_lib.lib_path(np.float64))
    lib.cmfrec_hip_early_stop_step.argtypes = [C.POINTER(_lib.EarlyStop), C.c_int, C.c_int, C.POINTER(C.c_double)]
    niter = len(values) if niter is None else niter
    st = _lib.EarlyStop(every=every, patience=patience, higher_is_better=int(higher), min_delta=min_delta, best=0.0, best_iter=-1, misses=0)
    evaluated, improved, ran = [], [], 0
    for it in range(niter):
        ran = it + 1
        if not lib.cmfrec_hip_early_stop_step(C.byref(st), it, niter, None):
            continue
        evaluated.append(it)
        v = C.c_double(values[it])
        step = lib.cmfrec_hip_early_stop_step(C.byref(st), it, niter, C.byref(v))
        assert step in (0, _lib.STEP_IMPROVED, _lib.STEP_STOP)
        if step & _lib.STEP_IMPROVED:
            improved.append(it)
            assert st.misses == 0 and st.best_iter == it and st.best == values[it]
        if step & _lib.STEP_STOP:
            break
    return evaluated, improved, ran, st.best_iter, st.best


def test_struct_mirrors():
    # cmfrec_hip_fit_monitor: two pointers, five ints (+ padding), a double, five pointers; cmfrec_hip_early_stop: three ints
    # (+ padding), two doubles, two ints; cmfrec_hip_rank_record: 17 fields of 8 bytes -- the layouts include/cmfrec_hip.h declares
    assert C.sizeof(_lib.FitMonitor) == 2 * 8 + 5 * 4 + 4 + 8 + 5 * 8
    assert C.sizeof(_lib.EarlyStop) == 16 + 8 + 8 + 8
    assert C.sizeof(_lib.RankRecord) == 17 * 8
    assert _lib.FitMonitor.min_delta.offset == 40 and _lib.EarlyStop.min_delta.offset == 16 and _lib.EarlyStop.best_iter.offset == 32
    assert [_lib.WATCH[name] for name in ("rmse", "mae", "hit", "precision", "recall", "ap", "ndcg", "rr", "auc", "mean_rank")] == list(range(10))


def test_lower_is_better_stops_after_patience():
    #        0    1    2    3    4    5    6
    vals = [3.0, 2.0, 1.5, 1.6, 1.7, 1.0, 0.5]
    ev, imp, ran, best, bv = run_rule(vals, patience=2)
    assert ev == [0, 1, 2, 3, 4] and imp == [0, 1, 2] and ran == 5 and best == 2 and bv == 1.5
    assert ran == best + 1 + 2
    # patience 3 survives the two misses and goes on improving
    ev, imp, ran, best, bv = run_rule(vals, patience=3)
    assert ran == 7 and imp == [0, 1, 2, 5, 6] and best == 6


def test_higher_is_better():
    vals = [0.1, 0.3, 0.2, 0.25, 0.9]
    ev, imp, ran, best, bv = run_rule(vals, patience=2, higher=True)
    assert imp == [0, 1] and ran == 4 and best == 1 and bv == 0.3
    # the same numbers read as "lower is better": only the first improves
    ev, imp, ran, best, bv = run_rule(vals, patience=2, higher=False)
    assert imp == [0] and ran == 3 and best == 0


@pytest.mark.parametrize("patience", [0, -1])
def test_monitor_only_never_stops(patience):
    vals = [1.0, 2.0, 3.0, 4.0, 5.0, 0.5]
    ev, imp, ran, best, bv = run_rule(vals, patience=patience)
    assert ev == list(range(6)) and ran == 6 and imp == [0, 5] and best == 5


def test_every_and_the_last_iteration():
    vals = [9, 9, 5.0, 9, 9, 4.0, 9, 9, 3.0, 9, 2.0]                   # niter = 11: evaluated after 3, 6, 9 and the last
    ev, imp, ran, best, bv = run_rule(vals, every=3)
    assert ev == [2, 5, 8, 10] and imp == [2, 5, 8, 10] and ran == 11 and best == 10
    # patience counts evaluations, not iterations
    vals = [9, 9, 5.0, 9, 9, 6.0, 9, 9, 7.0, 9, 2.0]
    ev, imp, ran, best, bv = run_rule(vals, every=3, patience=2)
    assert ev == [2, 5, 8] and ran == 9 and best == 2
    # every < 1 counts as 1; every beyond niter: the last iteration alone
    assert run_rule([3.0, 2.0, 1.0], every=0)[0] == [0, 1, 2]
    assert run_rule([3.0, 2.0, 1.0], every=7)[0] == [2]


def test_min_delta():
    vals = [1.0, 0.95, 0.85, 0.84, 0.80]
    # 0.95 does not beat 1.0 by more than 0.1; 0.85 does; 0.84 and 0.80 do not beat 0.85 by more than 0.1
    ev, imp, ran, best, bv = run_rule(vals, patience=2, min_delta=0.1)
    assert imp == [0, 2] and ran == 5 and best == 2 and bv == 0.85
    # exactly min_delta better is not "more than"
    ev, imp, ran, best, bv = run_rule([1.0, 0.5, 0.5], min_delta=0.5)
    assert imp == [0] and best == 0
    ev, imp, ran, best, bv = run_rule([0.25, 0.5, 1.0, 1.75], min_delta=0.5, higher=True)
    assert imp == [0, 2, 3]
    # the first evaluation improves whatever min_delta says
    assert run_rule([5.0], min_delta=100.0)[1] == [0]


def test_nan_is_a_miss():
    ev, imp, ran, best, bv = run_rule([NAN, NAN, 1.0, NAN, NAN, 0.5], patience=3)
    assert imp == [2, 5] and ran == 6 and best == 5                    # two misses, an improvement, two misses, an improvement
    ev, imp, ran, best, bv = run_rule([NAN, NAN, 1.0], patience=2)
    assert imp == [] and ran == 2 and best == -1                       # nothing ever counted
    ev, imp, ran, best, bv = run_rule([1.0, NAN, NAN, 0.1], patience=2, higher=True)
    assert imp == [0] and ran == 3 and best == 0


def test_validation_arguments():
    row, col, val = np.array([0, 1, 2]), np.array([1, 0, 2]), np.array([1.0, 2.0, 3.0])
    v = Validation((row, col, val))
    assert v.metric is None and v.every == 1 and v.patience is None and v.min_delta == 0.0 and v.restore_best is True and v.k == 10
    for metric in ERROR_METRICS + RANKING_METRICS:
        assert Validation((row, col, val), metric=metric).metric == metric
    import scipy.sparse as sp
    v = Validation(sp.coo_matrix((val, (row, col)), shape=(4, 5)).tocsr(), W=[1.0, 0.0, 2.0], every=2, patience=3, min_delta=1e-3,
                   restore_best=False)
    assert sorted(zip(v.row.tolist(), v.col.tolist(), v.val.tolist())) == [(0, 1, 1.0), (1, 0, 2.0), (2, 2, 3.0)]
    assert (v.every, v.patience, v.min_delta, v.restore_best) == (2, 3, 1e-3, False) and len(v.W) == 3
    bad = [dict(metric="accuracy"), dict(every=0), dict(every=1.5), dict(patience=0), dict(patience=-2), dict(patience=2.5),
           dict(min_delta=-1e-9), dict(min_delta=NAN), dict(min_delta=math.inf), dict(k=0), dict(W=[1.0, 2.0])]
    for kw in bad:
        with pytest.raises(ValueError):
            Validation((row, col, val), **kw)
    with pytest.raises(ValueError):
        Validation((row, col[:2], val))
    with pytest.raises(TypeError):
        Validation(np.zeros((3, 3)))


def test_rankset_arguments():
    from cmfrec_amd.rank import check_rankset
    users, hp, hi, ep, ei = check_rankset([3, 1], (np.array([0, 2, 3]), np.array([7, 2, 5])), (np.array([0, 0, 2]), np.array([9, 4])))
    assert users.dtype == np.int32 and hp.tolist() == [0, 2, 3] and hi.tolist() == [2, 7, 5] and ep.tolist() == [0, 0, 2] and ei.tolist() == [4, 9]
    assert check_rankset([0], (np.array([0, 1]), np.array([4])), None)[3] is None
    for bad in (dict(users=[-1, 2]), dict(users=[[1, 2]]), dict(users=[0.5, 1.0]), dict(users=[1, 2, 3]), dict(users=[2 ** 40, 1])):
        with pytest.raises(ValueError):
            check_rankset(bad["users"], (np.array([0, 1, 2]), np.array([1, 2])), None)
    with pytest.raises(ValueError):
        check_rankset([1, 2], None, None)
    with pytest.raises(ValueError):
        check_rankset([1, 2], (np.array([0, 1, 2]), np.array([1, 2])), (np.array([0, 1]), np.array([1])))


def test_ranking_lists_of_a_validation():
    """What a ranking watch ranks: the users with held-out entries (among `users`), their items, and the training items left out."""
    trow, tcol = np.array([0, 0, 2, 3, 3]), np.array([1, 4, 0, 2, 1])
    v = Validation((np.array([3, 0, 3, 5]), np.array([0, 2, 4, 1]), np.ones(4)), metric="ndcg")
    users, (hp, hi), (ep, ei) = v._ranking_lists((trow, tcol, 4, 5))
    assert users.tolist() == [0, 3] and hp.tolist() == [0, 1, 3] and hi.tolist() == [2, 0, 4]      # (row 5 is beyond X: left out)
    assert ep.tolist() == [0, 2, 4] and ei.tolist() == [1, 4, 1, 2]
    users, held, excl = Validation((np.array([3, 0, 3]), np.array([0, 2, 4]), np.ones(3)), metric="hit", users=[3, 1], X_exclude=None)._ranking_lists(
        (trow, tcol, 4, 5))
    assert users.tolist() == [3] and held[1].tolist() == [0, 4] and excl is None
    users, held, excl = Validation((np.array([0]), np.array([2]), np.ones(1)), metric="ap", X_exclude=(np.array([0, 0]), np.array([3, 1])))._ranking_lists(
        (trow, tcol, 4, 5))
    assert excl[1].tolist() == [1, 3]
    with pytest.raises(ValueError):
        Validation((np.array([0]), np.array([2]), np.ones(1)), metric="ap", X_exclude="test")._ranking_lists((trow, tcol, 4, 5))


def test_mean_from_record():
    from cmfrec_amd.metrics import METRICS, mean_from_record, mean_metrics, ranking_metrics
    indptr, ranks, pool = np.array([0, 3, 3, 5, 6]), np.array([4, 0, -1, 1, 0, -1]), np.array([9, 9, 2, 9])
    per = ranking_metrics(indptr, ranks, pool, k=3)
    want = mean_metrics(per)
    rec = {"sum": np.array([np.nansum(per[name]) for name in METRICS]), "count": np.array([(~np.isnan(per[name])).sum() for name in METRICS], np.uint64),
           "users": np.uint64((per["T"] > 0).sum())}
    got = mean_from_record(rec)
    assert got["users"] == want["users"] == 2 and int(rec["count"][METRICS.index("auc")]) == 1
    for name in METRICS:
        assert abs(got[name] - want[name]) <= 1e-15 * abs(want[name]), name
    empty = mean_from_record({"sum": np.zeros(8), "count": np.zeros(8, np.uint64), "users": np.uint64(0)})
    assert empty["users"] == 0 and all(np.isnan(empty[name]) for name in METRICS)
