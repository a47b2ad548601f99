"""The objective's components over all m x n pairs in extended precision (np.longdouble: at least float64, so that in double
precision the reference's own rounding stays below the bound), and the forward bound of every component that
tests/test_gpu_objective*.py hold the device to.  Shared by both test files."""
import numpy as np

L = np.longdouble
FIELDS = ("sum_w", "data", "allpairs", "normA", "normbiasA", "normB", "normbiasB")


def reference_and_bound(dtype, implicit, A, B, mask, V, W=None, biasA=None, biasB=None):
    """(components, bounds): dicts keyed like the device's record.  mask [m, n] marks the stored entries, V / W [m, n] their
    values (as the session stores them) and weights; A, B of the working precision `dtype`.
    Bound (the issue's): u = unit roundoff, g = k u / (1 - k u); a dot product summed in any order is off by <= g |a|.|b|, the
    residual formed in that precision adds u (|v| + |biasA| + |biasB| + |s|); a term w e^2 then moves by <= w (2 |e| d + d^2);
    every accumulation in double adds N 2^-53 sum|term|."""
    m, n = mask.shape
    kk = A.shape[1]
    u, u64 = L(np.finfo(dtype).eps) / 2, L(2.) ** -53
    g = kk * u / (1 - kk * u)
    Al, Bl = A.astype(L), B.astype(L)
    S, absS = Al @ Bl.T, np.abs(Al) @ np.abs(Bl).T
    Wl = np.ones((m, n), L) if W is None else W.astype(L)
    bA = np.zeros(m, L) if biasA is None else biasA.astype(L)
    bB = np.zeros(n, L) if biasB is None else biasB.astype(L)
    Vl = V.astype(L)
    nnz = int(mask.sum())
    d = g * absS
    if implicit:
        r = 1 - S
        dr = d + u * (1 + np.abs(S))
        term = (1 + Vl) * r ** 2 - S ** 2
        moved = (1 + Vl) * (2 * np.abs(r) * dr + dr ** 2) + 2 * np.abs(S) * d + d ** 2
        size = (1 + Vl) * r ** 2 + S ** 2
    else:
        r = Vl - bA[:, None] - bB[None, :] - S
        dr = d + u * (np.abs(Vl) + np.abs(bA)[:, None] + np.abs(bB)[None, :] + np.abs(S))
        term = Wl * r ** 2
        moved = Wl * (2 * np.abs(r) * dr + dr ** 2)
        size = np.abs(term)
    ref = {"n": nnz, "sum_w": Wl[mask].sum(), "data": term[mask].sum(), "allpairs": (S ** 2).sum() if implicit else L(0)}
    bound = {"sum_w": 0 if W is None else nnz * u64 * Wl[mask].sum(), "data": moved[mask].sum() + nnz * u64 * size[mask].sum(),
             "allpairs": (m + n + kk * kk) * u64 * (absS ** 2).sum() if implicit else L(0)}
    for side, F, bias, counts, wsum in (("A", Al, bA, mask.sum(1), (Wl * mask).sum(1)), ("B", Bl, bB, mask.sum(0), (Wl * mask).sum(0))):
        mult = np.where(counts > 0, counts if W is None else wsum.astype(dtype).astype(L), 1).astype(L)
        sq, last = (F ** 2).sum(1), F[:, -1] ** 2
        ref["norm" + side] = np.array([sq.sum(), (mult * sq).sum(), last.sum(), (mult * last).sum()])
        ref["normbias" + side] = np.array([(bias ** 2).sum(), (mult * bias ** 2).sum()])
        # (a weighted row's multiplier is its weights summed in double and rounded to the working precision: off by <= (entries + 1) u)
        steps, wu = (F.size + 2) * u64, 0 if W is None else (counts.max() + 1) * u
        bound["norm" + side] = steps * ref["norm" + side] + wu * ref["norm" + side] * np.array([0, 1, 0, 1])
        bound["normbias" + side] = steps * ref["normbias" + side] + wu * ref["normbias" + side] * np.array([0, 1])
    return ref, bound


def assert_within(rec, ref, bound, what=""):
    assert int(rec["n"]) == ref["n"], what
    for f in FIELDS:
        err = np.abs(np.asarray(rec[f], np.float64).astype(L) - ref[f])
        print("%s %-10s err %s bound %s" % (what, f, np.asarray(err, np.float64), np.asarray(bound[f], np.float64)))
        assert (err <= bound[f]).all(), "%s %s: error %s beyond the bound %s" % (what, f, err, bound[f])
