"""CPU: the similarity tests' own reference and tolerance (similar_reference.py) -- an emulation of the kernel's operation order
stays inside the bound, mutated scores are caught, the inputs leave few positions undecided -- and the argument checks of
``Ranker.similar`` / ``ops.similar_batch`` that need no device."""
import numpy as np
import pytest

import similar_reference as sr

CASES = [(dt, n, k, n_top) for dt in (np.float64, np.float32) for (n, k, n_top) in sr.SHAPES]
IDS = ["%s-n%d-k%d-top%d" % (np.dtype(c[0]).name, c[1], c[2], c[3]) for c in CASES]


@pytest.mark.parametrize("dtype,n,k,n_top", CASES, ids=IDS)
def test_emulation_within_bound(dtype, n, k, n_top):
    """(acc * rn[i]) * rn[q] in the working dtype, ranked by the kernels' rule, passes the four conditions."""
    B = sr.make_items(100 + k, dtype, n, k)
    q = sr.make_queries(k, n)
    ids, sc = sr.ranked(sr.emulate(B, q, "cosine"), q, n_top)
    worst, share = sr.check_neighbours(B, q, "cosine", None, None, ids, sc, n_top, dtype, all_decided=dtype is np.float64)
    assert worst <= 1.0
    assert (ids[list(q).index(5)] == -1).all() and not (ids == 5).any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("mutation", ["norm left out", "bias added"])
def test_mutations_are_caught(dtype, mutation):
    n, k, n_top = 1000, 50, 10
    B = sr.make_items(150, dtype, n, k)
    q = sr.make_queries(50, n)
    if mutation == "norm left out":
        S = sr.emulate(B, q, "cosine", drop_norm=True)
    else:
        S = sr.emulate(B, q, "cosine", bias=(np.random.default_rng(1).standard_normal(n) * 1e-3).astype(dtype))
    ids, sc = sr.ranked(S, q, n_top)
    with pytest.raises(AssertionError):
        sr.check_neighbours(B, q, "cosine", None, None, ids, sc, n_top, dtype, verbose=False)


@pytest.mark.parametrize("dtype,n,k,n_top", CASES, ids=IDS)
def test_undecided_share_of_the_inputs(dtype, n, k, n_top):
    """From the float64 reference alone: float64 leaves nothing undecided (the GPU cases run with all_decided), float32 less
    than 5 % (the GPU cases' cap is 10 %)."""
    B = sr.make_items(100 + k, dtype, n, k)
    q = sr.make_queries(k, n)
    ids, sc = sr.reference(B, q, "cosine", n_top)
    _, share = sr.check_neighbours(B, q, "cosine", None, None, ids, sc, n_top, dtype, verbose=False)
    print("reference undecided share %s n=%d k=%d n_top=%d: %.4f" % (np.dtype(dtype).name, n, k, n_top, share))
    if dtype is np.float64:
        assert share == 0
    else:
        assert share < sr.F32_REFERENCE_CAP


def test_planted_rows_in_the_reference():
    """3, 7, 11 and 20 tie exactly under cosine (in id order); under dot item 20 scores four times item 3."""
    B = sr.make_items(1, np.float64, 300, 17)
    q = np.array([0, 1, 2], np.int32)
    S = sr.scores64(B, q, "cosine")
    assert np.array_equal(S[:, 3], S[:, 7]) and np.array_equal(S[:, 3], S[:, 11]) and np.array_equal(S[:, 3], S[:, 20])
    D = sr.scores64(B, q, "dot")
    assert np.array_equal(D[:, 20], 4 * D[:, 3])
    assert np.isnan(S[:, 5]).all()


def _dead_ranker(n=10, k=4, dtype=np.float64):
    from cmfrec_amd.rank import Ranker
    r = Ranker.__new__(Ranker)                  # no device: the checks come before the handle is touched
    r.handle = None; r.n = n; r.k = k; r.dtype = np.dtype(dtype)
    return r


BAD = [
    (dict(ids=[0.5, 1.0]), "integers"),
    (dict(ids=[[0, 1]]), "1-D"),
    (dict(ids=[-1, 2]), r"in \[0, 10\)"),
    (dict(ids=[0, 10]), r"in \[0, 10\)"),
    (dict(ids=[0], metric="euclid"), "metric"),
    (dict(ids=[0], metric=1), "metric"),
]


@pytest.mark.parametrize("kw,msg", BAD, ids=[b[1] + str(i) for i, b in enumerate(BAD)])
def test_argument_checks_need_no_device(kw, msg):
    from cmfrec_amd import ops
    with pytest.raises(ValueError, match=msg):
        _dead_ranker().similar(**kw)
    B = np.zeros((10, 4))
    with pytest.raises(ValueError, match=msg):
        ops.similar_batch(B, kw["ids"], metric=kw.get("metric", "cosine"))


def test_good_arguments_reach_the_handle():
    with pytest.raises(RuntimeError, match="closed"):
        _dead_ranker().similar(np.array([0, 9], np.int64), metric="dot")
    with pytest.raises(ValueError, match="float64 or float32"):
        from cmfrec_amd import ops
        ops.similar_batch(np.zeros((10, 4), np.int32), [0])
