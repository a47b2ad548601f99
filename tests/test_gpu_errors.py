"""The error of the predictions on held-out pairs, reduced on the GPU, held to the exact record of tests/errors_reference.py: the
two kernels alone (ops.pair_errors), the resident set against scorers (EvalSet, Scorer.errors), against a session's factors where
they are (AlsSession.errors) and through the models (evaluate_error).  The prediction inside the reduction is pinned bit for bit
to ops.score_pairs; the record is then checked against those predictions as stored.  The shapes are those of the prediction
tests: every group width, both load widths, part-filled steps, more than one wavefront, and -- under CMFREC_HIP_EVAL_WAVES and
at 100,000 pairs -- wavefronts that add up several chunks one after the other."""
import ctypes as C

import numpy as np
import pytest

import errors_reference as er
import predict_reference as pr
from dense_reference import DTYPES, _bits, _name

pytestmark = pytest.mark.gpu
IDS = [_name(d) for d in DTYPES]
KKS = (1, 3, 17, 50, 65, 129, 272)
BIASES = ((None, False), ("tight", True), ("col", True))
FIELDS = ("n", "n_skipped", "sum_w", "sum_we", "sum_wabs", "sum_wsq", "max_abs")


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _same_record(a, b, fields=FIELDS):
    return all(np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes() for f in fields)


def _images(dtype, kk, bias, aligned, implicit):
    kw = pr.images(dtype, kk, bias, aligned)
    if implicit:
        kw["glob_mean"] = 0.0
    return kw


def _run(dtype, kk, bias, aligned, implicit, row, col, seed, weights, what=""):
    """One pair_errors call held to score_pairs and to the exact record; returns (record, pred, x, w, masks)."""
    from cmfrec_amd import ops
    kw = _images(dtype, kk, bias, aligned, implicit)
    pred = ops.score_pairs(row=row, col=col, implicit=implicit, **kw)
    x, w = er.heldout(pred, seed, weights=weights)
    rec, got = ops.pair_errors(row=row, col=col, x=x, w=w, implicit=implicit, **kw)
    tag = "%s kk=%d n_pairs=%d bias=%s aligned=%s implicit=%s weights=%s %s" % (_name(dtype), kk, len(row), bias, aligned, implicit, weights, what)
    assert _same_bits(got, pred), tag + ": the prediction inside the reduction is not score_pairs'"
    scored, fallback = er.masks(row, col, pr.M, pr.N, implicit)
    worst = er.check(rec, pred, x, w, scored, fallback, what=tag)
    print("pair_errors %s: error / bound %.3g" % (tag, worst))
    assert int(rec["n"].sum()) + int(rec["n_skipped"]) == len(row), tag
    return rec, pred, x, w, (scored, fallback)


# ---- 1. the kernels alone ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kk", KKS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_kernel(dtype, kk):
    for n_pairs in pr.N_PAIRS:
        row, col = pr.pairs(n_pairs)
        for bias in BIASES:
            for aligned in (True, False):
                for weights in (False, True):
                    rec, *_ = _run(dtype, kk, bias, aligned, False, row, col, kk, weights)
                    if n_pairs >= 32:
                        assert int(rec["n"][1]) >= 13 and int(rec["n_skipped"]) >= 1        # 15 pairs outside, 3 NaN
        for aligned in (True, False):
            for weights in (False, True):
                rec, *_ = _run(dtype, kk, (None, False), aligned, True, row, col, kk, weights)
                assert int(rec["n"][1]) == 0 and (n_pairs < 32 or int(rec["n_skipped"]) >= 16)


@pytest.mark.parametrize("dtype,kk", [(np.float64, 3), (np.float32, 3), (np.float32, 272)], ids=["f64-3", "f32-3", "f32-272"])
def test_kernel_grid_stride(dtype, kk):
    """100,000 pairs: more chunks than one launch has wavefronts (at kk = 272 every wavefront gets several)."""
    row, col = pr.pairs(100000)
    _run(dtype, kk, ("tight", True), True, False, row, col, 5, True, what="grid-stride")
    _run(dtype, kk, (None, False), False, True, row, col, 6, False, what="grid-stride")


@pytest.mark.parametrize("kk", (3, 50, 272))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_wavefront_cap(dtype, kk, monkeypatch):
    """CMFREC_HIP_EVAL_WAVES: few wavefronts, many chunks each.  The sums may differ in their last bits, nothing else may."""
    row, col = pr.pairs(1000)
    monkeypatch.delenv("CMFREC_HIP_EVAL_WAVES", raising=False)
    base = {imp: _run(dtype, kk, BIASES[2 - 2 * imp], True, bool(imp), row, col, 9, True)[0] for imp in (0, 1)}
    for cap in ("4", "8"):
        monkeypatch.setenv("CMFREC_HIP_EVAL_WAVES", cap)
        for imp in (0, 1):
            rec = _run(dtype, kk, BIASES[2 - 2 * imp], True, bool(imp), row, col, 9, True, what="cap " + cap)[0]
            assert _same_record(rec, base[imp], ("n", "n_skipped", "max_abs")), (kk, cap, imp)
            assert _same_record(rec, _run(dtype, kk, BIASES[2 - 2 * imp], True, bool(imp), row, col, 9, True)[0]), "run to run under the cap"
    # that the cap is what shaped those launches: the wavefronts of the scoring launch as the resident set reports them
    from cmfrec_amd import EvalSet, Scorer
    A, B, bA, bB, gm = pr.problem(dtype, kk)
    masks = er.masks(row, col, pr.M, pr.N, False)
    with Scorer(A, B, bA, bB, glob_mean=gm) as sc:
        pred = sc.predict(row, col)
        x, w = er.heldout(pred, 9, weights=True)
        with EvalSet(row, col, x, w, dtype=dtype, sort=False) as es:
            monkeypatch.delenv("CMFREC_HIP_EVAL_WAVES", raising=False)
            free = sc.errors(es)
            by_occupancy = es.launch_waves()
            # (one chunk is (64 / G) * 4 pairs, a workgroup four wavefronts: 1000 pairs are at most 250 chunks)
            assert by_occupancy % 4 == 0 and 4 <= by_occupancy <= 252, by_occupancy
            if kk >= 50:
                assert by_occupancy > 8, "1000 pairs at kk = %d fill more than two workgroups" % kk
            for cap in (4, 8, 6):
                monkeypatch.setenv("CMFREC_HIP_EVAL_WAVES", str(cap))
                rec = sc.errors(es)
                assert es.launch_waves() == min((cap + 3) // 4 * 4, by_occupancy), (kk, cap, es.launch_waves())
                er.check(rec, pred, x, w, *masks, what="EvalSet under a cap of %d" % cap)
                assert _same_record(rec, free, ("n", "n_skipped", "max_abs")), (kk, cap)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_run_to_run_and_order(dtype):
    from cmfrec_amd import EvalSet, Scorer, ops
    for kk in (3, 65):
        row, col = pr.pairs(1000)
        a, pred, x, w, (scored, fallback) = _run(dtype, kk, ("col", True), True, False, row, col, 4, True)
        b = _run(dtype, kk, ("col", True), True, False, row, col, 4, True)[0]
        assert _same_record(a, b), "the same call twice"
        # a permutation of the pairs
        perm = np.random.default_rng(kk).permutation(len(row))
        kw = _images(dtype, kk, ("col", True), True, False)
        c, got = ops.pair_errors(row=row[perm], col=col[perm], x=x[perm], w=w[perm], **kw)
        assert _same_bits(got, pred[perm])
        er.check(c, pred, x, w, scored, fallback, what="permuted")
        assert _same_record(c, a, ("n", "n_skipped", "max_abs"))
        # the resident set, sorted by row or as it comes
        A, B, bA, bB, gm = pr.problem(dtype, kk)
        with Scorer(A, B, bA, bB, glob_mean=gm) as sc:
            recs = []
            for sort in (True, False):
                with EvalSet(row, col, x, w, dtype=dtype, sort=sort) as es:
                    recs.append(sc.errors(es))
                    assert _same_record(recs[-1], sc.errors(es)), "the same set twice"
                    assert es.kernel_ms() > 0
                er.check(recs[-1], pred, x, w, scored, fallback, what="EvalSet sort=%s" % sort)
                assert _same_record(recs[-1], a, ("n", "n_skipped", "max_abs"))


# ---- 2. the handles --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_handles(dtype):
    from cmfrec_amd import EvalSet, Scorer, _lib
    row, col = pr.pairs(1000)
    models = [pr.problem(dtype, kk) for kk in (3, 50)]
    first = Scorer(*models[0][:4], glob_mean=models[0][4])
    second = Scorer(models[1][0], models[1][1], implicit=True)
    p0 = first.predict(row, col)
    x, w = er.heldout(p0, 21, weights=True)
    es = EvalSet(row, col, x, w, dtype=dtype)
    with pytest.raises(RuntimeError, match="code 2"):
        es.kernel_ms()                                       # nothing evaluated yet
    er.check(first.errors(es), p0, x, w, *er.masks(row, col, pr.M, pr.N, False), what="first scorer")
    p1 = second.predict(row, col)
    er.check(second.errors(es), p1, x, w, *er.masks(row, col, pr.M, pr.N, True), what="second scorer, implicit")
    first.close()
    er.check(second.errors(es), p1, x, w, *er.masks(row, col, pr.M, pr.N, True), what="after the first scorer is gone")
    with pytest.raises(RuntimeError, match="closed"):
        first.errors(es)
    # a set of the other dtype; a closed set
    other = np.float32 if dtype is np.float64 else np.float64
    with EvalSet(row, col, x.astype(other), dtype=other) as wrong:
        with pytest.raises(ValueError, match="evaluation set is"):
            second.errors(wrong)
    es.close()
    with pytest.raises(RuntimeError, match="closed"):
        second.errors(es)
    # no pairs: a record of zeros
    with EvalSet(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, dtype), dtype=dtype) as empty:
        rec = second.errors(empty)
        assert all(not np.asarray(rec[f]).any() for f in FIELDS)
        assert empty.kernel_ms() == 0
        assert empty.launch_waves() == 0
    second.close()
    # the raw entry point: a negative weight, a missing array
    lib = _lib.load(dtype)
    bad = np.array([1.0, -0.5, 1.0], dtype)
    r3 = np.zeros(3, np.int32)
    P = _lib.ptr
    assert lib.cmfrec_hip_evalset_create(P(r3), P(r3), P(bad), P(bad), 3, -1) is None
    assert lib.cmfrec_hip_last_error_code() == 2 and b"weight" in lib.cmfrec_hip_last_error()
    assert lib.cmfrec_hip_evalset_create(P(r3), P(r3), None, None, 3, -1) is None
    assert lib.cmfrec_hip_last_error_code() == 2


# ---- 3. a session's factors where they are -----------------------------------------------------------------------------------

def _session(dtype, implicit, use_cg):
    from cmfrec_amd import AlsSession
    m, n, k, km = pr.M, pr.N, 5, 1
    rng = np.random.default_rng(17)
    at = rng.choice(m * n, 400, replace=False)
    row, col = (at // n).astype(np.int32), (at % n).astype(np.int32)
    val = (rng.integers(1, 6, 400) if not implicit else rng.integers(1, 4, 400)).astype(dtype)
    gm = 0.0 if implicit else float(np.dtype(dtype).type(val.mean()))
    bias = not implicit
    s = AlsSession(m, n, k, implicit=implicit, dtype=dtype, lam=0.7, use_cg=use_cg, k_main=km, user_bias=bias, item_bias=bias)
    s.set_X_coo(row, col, val, subtract=gm)
    s.set_factors(A=(0.3 * rng.standard_normal((m, k + km))).astype(dtype), B=(0.3 * rng.standard_normal((n, k + km))).astype(dtype),
                  biasA=np.zeros(m, dtype) if bias else None, biasB=np.zeros(n, dtype) if bias else None)
    return s, gm


@pytest.mark.parametrize("use_cg", [True, False], ids=["cg", "chol"])
@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_session(dtype, implicit, use_cg):
    from cmfrec_amd import EvalSet, ops
    s, gm = _session(dtype, implicit, use_cg)
    row, col = pr.pairs(1000)
    x, w = er.heldout(np.zeros(1000, dtype), 33, weights=True, scale=2.0)
    masks = er.masks(row, col, pr.M, pr.N, implicit)
    try:
        with EvalSet(row, col, x, w, dtype=dtype) as es:
            for it in range(2):
                s.iterate(1, False)
                rec = s.errors(es, glob_mean=gm)
                f = s.get_factors()
                kk = f["A"].shape[1]
                pred = ops.score_pairs(pr.M, pr.N, kk, row, col, A_img=f["A"].ravel(), lda=kk, B_img=f["B"].ravel(), ldb=kk, biasA=f["biasA"],
                                       biasB=f["biasB"], glob_mean=gm, implicit=implicit)
                assert np.isfinite(pred[masks[0]]).all() and np.abs(pred[masks[0]]).max() > 0
                worst = er.check(rec, pred, x, w, *masks, what="session %s it=%d" % (_name(dtype), it))
                print("session_errors %s implicit=%s cg=%s it=%d: error / bound %.3g" % (_name(dtype), implicit, use_cg, it, worst))
                assert int(rec["n"][1]) == (0 if implicit else int(masks[1].sum() - (np.isnan(x) & masks[1]).sum()))
                # an evaluation between two downloads of the factors: nothing of the session's changes, and the record of the
                # same factors is the same bytes as the one taken straight behind the iteration
                again = s.errors(es, glob_mean=gm)
                after = s.get_factors()
                assert _same_record(again, rec), "the same factors, another record"
                for key in ("A", "B", "biasA", "biasB", "C", "D"):
                    assert (f[key] is None and after[key] is None) or _same_bits(f[key], after[key]), key + " changed under the evaluation"
    finally:
        s.close()


def test_session_refusals():
    from cmfrec_amd import AlsSession, EvalSet, _lib
    r = np.zeros(3, np.int32)
    s = AlsSession(pr.M, pr.N, 5, implicit=False, row_range=(0, 20))
    try:
        with EvalSet(r, r, np.zeros(3)) as es:
            rec = _lib.Errors()
            assert s.lib.cmfrec_hip_session_errors(s.handle, es._live(), 0.0, C.byref(rec)) == 2
            assert b"owns all rows" in s.lib.cmfrec_hip_last_error()
            with pytest.raises(RuntimeError, match="code 2"):
                s.errors(es)
        with EvalSet(r, r, np.zeros(3, np.float32), dtype=np.float32) as es32:
            with pytest.raises(ValueError, match="evaluation set is"):
                s.errors(es32)
    finally:
        s.close()


# ---- 4. the models -----------------------------------------------------------------------------------------------------------

def _metrics_close(got, want, n):
    """got: from the device's record; want: from the exact record.  Counts and the maximum are exact.  mse and mae are ratios of
    two sums of non-negative terms, each within (n + 3) eps64 of its exact value relative to itself: the ratio within twice that
    (and its rounding); rmse halves it.  bias: the numerator's error is bounded by (n + 3) eps64 sum w |e|, that is by mae."""
    for key in ("n", "n_fallback", "n_skipped", "max_abs"):
        assert got[key] == want[key], key
    tol = 3 * (n + 3) * er.EPS64
    for key in ("mse", "rmse", "mae", "sum_w"):
        assert abs(got[key] - want[key]) <= tol * abs(want[key]), key
    assert abs(got["bias"] - want["bias"]) <= tol * want["mae"], "bias"


def _heldout_entries(m, n, dtype, seed):
    """300 test entries, 40 of them with a user or an item beyond the model, three NaN values, seeded weights."""
    rng = np.random.default_rng(seed)
    row, col = rng.integers(0, m, 300).astype(np.int32), rng.integers(0, n, 300).astype(np.int32)
    row[:20] += m; col[20:40] += n
    val = rng.integers(1, 6, 300).astype(dtype)
    val[[50, 60, 5]] = np.nan
    w = rng.uniform(0, 2, 300).astype(dtype)
    return row, col, val, w


@pytest.mark.parametrize("use_float", [False, True], ids=["f64", "f32"])
def test_models(use_float):
    import scipy.sparse as sp
    from cmfrec_amd import CMF, CMF_implicit
    from cmfrec_amd.metrics import error_metrics
    dtype = np.float32 if use_float else np.float64
    m, n = 60, 45
    rng = np.random.default_rng(2)
    at = rng.choice(m * n, 900, replace=False)
    row, col, val = (at // n).astype(np.int32), (at % n).astype(np.int32), rng.integers(1, 6, 900).astype(dtype)
    trow, tcol, tval, tw = _heldout_entries(m, n, dtype, 8)
    mdl = CMF(k=5, niter=2, use_float=use_float, random_state=3, nthreads=1).fit((row, col, val), shape=(m, n))
    pred = mdl.predict_batch(trow, tcol)
    for W in (None, tw):
        want, _ = er.exact_record(pred, tval, W, *er.masks(trow, tcol, m, n, False))
        want = {k: np.asarray(v, np.float64) if k != "n" else v for k, v in want.items()}
        for fb in (True, False):
            got = mdl.evaluate_error((trow, tcol, tval), W=W, include_fallback=fb)
            _metrics_close(got, error_metrics(want, include_fallback=fb), 300)
            assert got["n_fallback"] == 39 and got["n_skipped"] == 3 and got["n"] == (297 if fb else 258)
    # a sparse matrix (no NaN among its values: SciPy keeps them, the set skips them all the same)
    X_test = sp.coo_matrix((tval, (trow, tcol)), shape=(2 * m, 2 * n))
    assert mdl.evaluate_error(X_test, W=tw) == mdl.evaluate_error((trow, tcol, tval), W=tw)
    imp = CMF_implicit(k=5, niter=2, use_float=use_float, random_state=3).fit((row, col, val), shape=(m, n))
    pred = imp.predict_batch(trow, tcol)
    want, _ = er.exact_record(pred, tval, None, *er.masks(trow, tcol, m, n, True))
    want = {k: np.asarray(v, np.float64) if k != "n" else v for k, v in want.items()}
    got = imp.evaluate_error((trow, tcol, tval))
    _metrics_close(got, error_metrics(want), 300)
    assert got["n_fallback"] == 0 and got["n_skipped"] == 43 - 1 and got["n"] == 258
