"""CPU-side tests of the pair predictions: the check of tests/predict_reference.py rejects what it must and accepts another
summation order; the facts the header states about the compiled reference's predict_X_old_* hold on the recorded fixture; and
``Scorer``'s argument errors that need no device."""
import numpy as np
import pytest

import predict_reference as pr
from dense_reference import DTYPES, Rejected


def _case(dtype, kk=17, bias=(True, True), implicit=False, n_pairs=1000):
    A, B, bA, bB, gm = pr.problem(dtype, kk)
    row, col = pr.pairs(n_pairs)
    ops = (A, B, bA if bias[0] and not implicit else None, bB if bias[1] and not implicit else None, 0.0 if implicit else gm)
    return ops, row, col


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("implicit", [False, True])
def test_check_accepts_standin_and_another_order(dtype, implicit):
    ops, row, col = _case(dtype, implicit=implicit)
    good = pr.standin(*ops, row, col, implicit=implicit)
    assert pr.check(good, *ops, row, col, implicit=implicit) <= 1.0
    order = np.random.default_rng(3).permutation(ops[0].shape[1])
    other = pr.standin(*ops, row, col, implicit=implicit, order=order)
    assert not np.array_equal(other, good, equal_nan=True)              # (another order does give other bits)
    assert pr.check(other, *ops, row, col, implicit=implicit) <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_check_rejects_mutations(dtype):
    ops, row, col = _case(dtype)
    A, B, bA, bB, gm = ops
    good = pr.standin(*ops, row, col)
    with pytest.raises(Rejected):                                       # one product left out
        pr.check(pr.standin(*ops, row, col, drop=5), *ops, row, col)
    with pytest.raises(Rejected):                                       # the dot product over k instead of k + k_main
        pr.check(pr.standin(*ops, row, col, kk_used=15), *ops, row, col)
    with pytest.raises(Rejected):                                       # one bias missing
        pr.check(pr.standin(A, B, bA, None, gm, row, col), *ops, row, col)
    with pytest.raises(Rejected):
        pr.check(pr.standin(A, B, None, bB, gm, row, col), *ops, row, col)
    scored = pr.exact(*ops, row, col)[2]
    fb, sc = np.nonzero(~scored)[0], np.nonzero(scored)[0]
    assert len(fb) >= 15 and len(sc)
    bad = good.copy(); bad[fb[0]] = good[sc[0]]                          # a fallback pair swapped for a scored one
    with pytest.raises(Rejected):
        pr.check(bad, *ops, row, col)
    bad = good.copy(); bad[fb[3]] = np.nextafter(bad[fb[3]], np.inf)    # a fallback pair one ulp off
    with pytest.raises(Rejected):
        pr.check(bad, *ops, row, col)
    imp = (A, B, None, None, 0.0)
    good = pr.standin(*imp, row, col, implicit=True)
    bad = good.copy(); bad[fb[0]] = 0.0                                 # implicit: a pair out of range that is not NaN
    with pytest.raises(Rejected):
        pr.check(bad, *imp, row, col, implicit=True)


def test_pairs_cover_every_kind():
    row, col = pr.pairs(1000)
    r, c = row.astype(np.int64), col.astype(np.int64)
    assert ((r >= pr.M) & (c >= 0) & (c < pr.N)).any() and ((c >= pr.N) & (r >= 0) & (r < pr.M)).any()
    assert ((r < 0) & (c >= 0) & (c < pr.N)).any() and ((c < 0) & (r >= 0) & (r < pr.M)).any()
    assert ((r < 0) & (c < 0)).any() and ((r >= pr.M) & (c >= pr.N)).any()
    lin = r * 10 ** 6 + c
    assert len(np.unique(lin)) < len(lin)                                # pairs repeat


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("implicit", [False, True])
def test_reference_facts(dtype, implicit):
    """The compiled reference's predict_X_old_* (fixture g42): with k_main = 0 it is the model's prediction; with k_main = 2 it
    equals the formula over k factors only and differs from the model's by more than the bound; its fallbacks for row >= m and
    col >= n_max are glob_mean + the bias in range (explicit) or NaN (implicit)."""
    g = pr.load_fixture(dtype)
    tag = "imp" if implicit else "exp"
    for km in pr.OLD_KMS:
        d = pr.old_problem(dtype, km)
        ref = g["old_%s_km%d" % (tag, km)]
        ops = pr.old_operands(d, implicit)
        if km == 0:
            assert pr.check(ref, *ops, d["row"], d["col"], implicit=implicit) <= 1.0
            continue
        # the k-only formula holds (fallbacks included) ...
        assert pr.check(ref, *ops, d["row"], d["col"], implicit=implicit, kk=d["k"]) <= 1.0
        # ... and it is not the model's prediction
        with pytest.raises(Rejected):
            pr.check(ref, *ops, d["row"], d["col"], implicit=implicit)
        scored = pr.exact(*ops, d["row"], d["col"], implicit)[2]
        assert (~scored).sum() >= 8


def test_scorer_argument_errors():
    from cmfrec_amd import Scorer
    from cmfrec_amd.score import check_pairs
    A, B = np.zeros((4, 3)), np.zeros((5, 3))
    with pytest.raises(ValueError, match="2-D"):
        Scorer(np.zeros(4), B)
    with pytest.raises(ValueError, match="2-D"):
        Scorer(A, np.zeros((5, 3, 1)))
    with pytest.raises(ValueError, match="float32"):
        Scorer(A, B.astype(np.float32))
    with pytest.raises(ValueError, match="float64 or float32"):
        Scorer(A.astype(np.int32), B.astype(np.int32))
    with pytest.raises(ValueError, match="factors"):
        Scorer(A, np.zeros((5, 4)))
    with pytest.raises(ValueError, match="biasA"):
        Scorer(A, B, biasA=np.zeros(5))
    with pytest.raises(ValueError, match="biasB"):
        Scorer(A, B, biasB=np.zeros(5, np.float32))
    with pytest.raises(ValueError, match="one length"):
        check_pairs(np.zeros(3, np.int32), np.zeros(4, np.int32))
    with pytest.raises(ValueError, match="1-D"):
        check_pairs(np.zeros((3, 1), np.int32), np.zeros(3, np.int32))
    with pytest.raises(ValueError, match="integers"):
        check_pairs(np.zeros(3), np.zeros(3, np.int32))
    with pytest.raises(ValueError, match="32-bit"):
        check_pairs(np.array([2 ** 40]), np.array([0]))
    r, c = check_pairs([1, 2], np.array([3, 4], np.int64))
    assert r.dtype == np.int32 and c.dtype == np.int32 and r.flags.c_contiguous
