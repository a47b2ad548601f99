"""The error record of held-out pairs (cmfrec_hip_errors: ops.pair_errors, Scorer.errors, AlsSession.errors): the exact record
and the check (helpers, no tests).  tests/test_gpu_errors.py runs the check on the GPU's records, tests/test_errors_cpu.py on a
stand-in (NumPy in float64, left to right) and on mutations of it.

The record is defined on the predictions AS STORED (the kernel's own values, pinned bit for bit to cmfrec_hip_score_pairs by the
GPU test): with p the prediction, in double precision  e = (double)p - (double)x,  w = weight or 1, and per class -- [0] scored,
[1] fallback -- n, sum_w, sum_we = sum w e, sum_wabs = sum w |e|, sum_wsq = sum w e^2, max_abs = max |e|; n_skipped counts the
pairs of neither class and those whose x is NaN.  The exact sums are formed in np.longdouble.  The check, nothing in it measured:

    counts     exact
    max_abs    exact: the bits of the double maximum of |(double)p - (double)x|
    a sum S    over n counted terms t_i:  |S_got - S_exact| <= (n + 3) eps64 sum_i |t_i|
               -- the any-order summation bound for n terms plus three roundings in forming a term (the difference, e^2 or
               |e|, the product with w); written with the epsilon of float64, twice its unit roundoff, it leaves a factor of two
    no terms   the sum and the maximum are exactly 0
"""
import numpy as np

from dense_reference import Rejected, _bits

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)
SUMS = ("sum_w", "sum_we", "sum_wabs", "sum_wsq")


def masks(row, col, m, n, implicit):
    """(scored, fallback) of pairs against an [m] x [n] model."""
    row = np.asarray(row, np.int64); col = np.asarray(col, np.int64)
    scored = (row >= 0) & (row < m) & (col >= 0) & (col < n)
    return scored, (np.zeros(len(row), bool) if implicit else ~scored)


def heldout(pred, seed, weights=False, scale=0.5, nans=True):
    """(x, w) in pred's dtype: x = the prediction + seeded noise (the noise alone where the prediction is NaN), from 32 pairs on
    NaN at the first, the last and a third index; w: None, or seeded weights >= 0 with exact zeros among them."""
    rng = np.random.default_rng([seed, len(pred)])
    dt = pred.dtype
    x = (np.where(np.isnan(pred), 0, pred).astype(np.float64) + scale * rng.standard_normal(len(pred))).astype(dt)
    if nans and len(pred) >= 32:
        x[[0, len(pred) - 1, int(rng.integers(1, len(pred) - 1))]] = np.nan
    w = None
    if weights:
        w = rng.uniform(0.0, 2.0, len(pred)).astype(dt)
        w[rng.random(len(pred)) < 0.1] = 0
    return x, w


def _terms(pred, x, w, mask):
    """Per sum the terms of the counted pairs of a class in np.longdouble, and |e| in float64."""
    keep = mask & ~np.isnan(x)
    p64, x64 = pred[keep].astype(np.float64), x[keep].astype(np.float64)
    e = p64.astype(LD) - x64.astype(LD)
    wl = np.ones(int(keep.sum()), LD) if w is None else w[keep].astype(LD)
    return {"sum_w": wl, "sum_we": wl * e, "sum_wabs": wl * np.abs(e), "sum_wsq": wl * e * e}, np.abs(p64 - x64)


def exact_record(pred, x, w, scored_mask, fallback_mask):
    """(record, magnitude): the record with its sums in np.longdouble, and per sum the sum of |t_i| (np.longdouble) the bound
    multiplies, both [2] per name."""
    rec = {"n": np.zeros(2, np.uint64)}
    mag = {}
    for name in SUMS:
        rec[name] = np.zeros(2, LD); mag[name] = np.zeros(2, LD)
    rec["max_abs"] = np.zeros(2, np.float64)
    for c, mask in enumerate((scored_mask, fallback_mask)):
        terms, ae = _terms(pred, x, w, mask)
        rec["n"][c] = len(ae)
        for name in SUMS:
            rec[name][c] = terms[name].sum(dtype=LD); mag[name][c] = np.abs(terms[name]).sum(dtype=LD)
        rec["max_abs"][c] = ae.max() if len(ae) else 0.0
    rec["n_skipped"] = np.uint64(len(pred) - int(rec["n"].sum()))
    return rec, mag


def violations(got, pred, x, w, scored_mask, fallback_mask):
    """The names of what the record `got` gets wrong, [] if nothing; the worst error / bound over the sums comes second."""
    want, mag = exact_record(pred, x, w, scored_mask, fallback_mask)
    bad = []
    if not np.array_equal(np.asarray(got["n"]).astype(np.uint64), want["n"]):
        bad.append("n")
    if int(got["n_skipped"]) != int(want["n_skipped"]):
        bad.append("n_skipped")
    worst = 0.0
    for c in range(2):
        n = int(want["n"][c])
        if not np.array_equal(_bits(np.array([got["max_abs"][c]], np.float64)), _bits(want["max_abs"][c:c + 1])):
            bad.append("max_abs[%d]" % c)
        for name in SUMS:
            g = np.float64(np.asarray(got[name])[c])
            if n == 0:
                if not g == 0:
                    bad.append("%s[%d]" % (name, c))
                continue
            bound = (n + 3) * EPS64 * mag[name][c]
            err = abs(LD(g) - want[name][c])
            if not err <= bound:                            # (a NaN fails too)
                bad.append("%s[%d]" % (name, c))
            if bound > 0:
                worst = max(worst, float(err / bound))
    return bad, worst


def check(got, pred, x, w, scored_mask, fallback_mask, what="errors"):
    """Asserts that the record is right; returns the worst error / bound over its sums."""
    bad, worst = violations(got, pred, x, w, scored_mask, fallback_mask)
    if bad:
        raise Rejected("%s: wrong %s (worst sum error / bound = %.3g)" % (what, ", ".join(bad), worst))
    return worst


def standin(pred, x, w, scored_mask, fallback_mask, order=None, e_dtype=np.float64):
    """The record in float64, the terms added left to right (np.cumsum) in the order given (a permutation of the pairs, or as
    they come).  e_dtype: the precision the difference is formed in."""
    idx = np.arange(len(pred)) if order is None else np.asarray(order)
    rec = {"n": np.zeros(2, np.uint64), "max_abs": np.zeros(2)}
    for name in SUMS:
        rec[name] = np.zeros(2)
    counted = 0
    for c, mask in enumerate((scored_mask, fallback_mask)):
        i = idx[mask[idx] & ~np.isnan(x[idx])]
        e = (pred[i].astype(e_dtype) - x[i].astype(e_dtype)).astype(np.float64)
        wt = np.ones(len(i)) if w is None else w[i].astype(np.float64)
        rec["n"][c] = len(i); counted += len(i)
        for name, t in (("sum_w", wt), ("sum_we", wt * e), ("sum_wabs", wt * np.abs(e)), ("sum_wsq", wt * (e * e))):
            rec[name][c] = np.cumsum(t)[-1] if len(i) else 0.0
        rec["max_abs"][c] = np.abs(e).max() if len(i) else 0.0
    rec["n_skipped"] = np.uint64(len(pred) - counted)
    return rec
