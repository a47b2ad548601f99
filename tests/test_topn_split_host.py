"""Host side of the item-split ranking and the one-user interface (no GPU): the planner ``cmfrec_hip_topn_split_plan`` over a grid
of shapes, the new names in the ABI, and the one-user methods' argument errors, which are raised before any device is touched."""
import itertools
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITEMS = 128                                   # TOPNW_ITEMS: items per round of the MFMA ranking kernel

NU = (1, 16, 17, 64, 4096, 100000)
N = (1, 127, 128, 129, 1000, 160112)
K = (3, 64, 128, 272)
NTOP = (1, 32, 33, 128)
CUS = (1, 256)
DTYPES = (np.float64, np.float32)


def _grid():
    for dtype, nu, n, k, n_top, cus in itertools.product(DTYPES, NU, N, K, NTOP, CUS):
        if n_top > n or (dtype is np.float64 and k > 256):
            continue
        yield dtype, nu, n, k, n_top, cus


def _slots(nu, k, n_top, cus, dtype):
    """(user-tile workgroups, workgroup slots of the device) for every user-tile count that fits the LDS, from the kernel's
    documented LDS layout (topnw_lds_bytes): the planner may split only while the tiles of ITS choice leave slots empty, so
    'the tiles fill the slots for every count' is a sufficient condition for one slice that does not depend on the choice."""
    sz = np.dtype(dtype).itemsize
    ch = 64 // sz
    ks = (k + ch - 1) // ch * ch + 16 // sz
    np2 = 32
    while np2 < n_top:
        np2 *= 2
    out = []
    for nut in (1, 2, 3, 4):
        ut = 16 * nut
        smem = ut * ks * sz + ut * (np2 + 32) * (sz + 4) + ut * (sz + 4) + 8
        if smem > 160 * 1024:
            break
        bpc = min(160 * 1024 // smem, 4)
        out.append(((nu + ut - 1) // ut, cus * bpc))
    return out


def _check_cut(n, slices, slice_items):
    assert slices >= 1 and slice_items >= ITEMS
    assert slice_items % ITEMS == 0
    assert slices * slice_items >= n > (slices - 1) * slice_items


def test_planner_properties():
    from cmfrec_amd.rank import split_plan
    split_somewhere = False
    for dtype, nu, n, k, n_top, cus in _grid():
        case = (np.dtype(dtype).name, nu, n, k, n_top, cus)
        rounds = (n + ITEMS - 1) // ITEMS
        s, si = split_plan(nu, n, k, n_top, cus, dtype, 0)
        _check_cut(n, s, si)
        assert s <= rounds, case
        if all(tiles >= slots for tiles, slots in _slots(nu, k, n_top, cus, dtype)):
            assert s == 1, case                               # the user tiles fill the device by themselves
        assert s <= max(slots for _, slots in _slots(nu, k, n_top, cus, dtype)), case
        split_somewhere |= s > 1
        # a request: honoured up to the rounds there are, never an empty slice
        for req in (1, 2, 3, 7, rounds, rounds + 1, 100, 10 ** 6):
            rs, rsi = split_plan(nu, n, k, n_top, cus, dtype, req)
            _check_cut(n, rs, rsi)
            assert rs <= min(req, rounds), (case, req)
            if req <= min(rounds, 4096) and rounds % req == 0:
                assert rs == req, (case, req)
        assert split_plan(nu, n, k, n_top, cus, dtype, 1) == (1, rounds * ITEMS), case
    assert split_somewhere


def test_planner_splits_one_user_and_not_a_full_device():
    from cmfrec_amd.rank import split_plan
    for dtype in DTYPES:
        s, si = split_plan(1, 160112, 128, 10, 256, dtype)
        assert s > 1 and s * si >= 160112
        assert split_plan(100000, 160112, 128, 10, 256, dtype)[0] == 1
        assert split_plan(1, 128, 128, 10, 256, dtype) == (1, 128)


def test_planner_refuses_what_topN_refuses():
    from cmfrec_amd.rank import split_plan
    for bad in (dict(k=273), dict(n_top=129), dict(n_top=51, n=50), dict(nu=0), dict(num_cus=0), dict(requested=-1)):
        a = dict(nu=4, n=3000, k=100, n_top=10, num_cus=256, requested=0)
        a.update(bad)
        with pytest.raises(RuntimeError, match=r"code 2"):
            split_plan(a["nu"], a["n"], a["k"], a["n_top"], a["num_cus"], np.float64, a["requested"])


NEW_NAMES = ("cmfrec_hip_ranker_set_split", "cmfrec_hip_ranker_slices", "cmfrec_hip_newrows_set_split", "cmfrec_hip_topn_split_plan")


def test_new_names_are_declared_and_exported():
    from cmfrec_amd import _lib
    header = open(os.path.join(ROOT, "include", "cmfrec_hip.h")).read()
    for name in NEW_NAMES:
        assert name in _lib.EXPORTED, name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        for dtype in DTYPES:
            assert hasattr(_lib.load(dtype), name), name


def test_split_argument():
    from cmfrec_amd.rank import split_code
    assert split_code(None) == -1 and split_code("auto") == 0 and split_code(1) == 1 and split_code(np.int64(7)) == 7
    for bad in (0, -1, 2.5, "on", True):
        with pytest.raises(ValueError, match="split"):
            split_code(bad)


def _fake_fitted(cls, n=300, k=8, p=0, **kw):
    """An estimator with the attributes of a fit and no device behind it: enough for every check that precedes the handles."""
    mdl = cls(k=k, use_float=False, **kw)
    rng = np.random.default_rng(0)
    mdl.A_ = rng.standard_normal((60, k)); mdl.B_ = rng.standard_normal((n, k))
    mdl.C_ = rng.standard_normal((p, k)) if p else np.empty((0, 0))
    mdl.is_fitted_ = True
    return mdl


def _no_handles(mdl):
    assert "_one_user_ranker" not in mdl.__dict__ and "_one_user_new" not in mdl.__dict__


@pytest.mark.parametrize("name", ["CMF", "CMF_implicit"])
def test_one_user_argument_errors(name):
    import cmfrec_amd
    cls = getattr(cmfrec_amd, name)
    col, val = np.array([1, 5, 9]), np.array([1., 2., 3.])
    # unfitted
    raw = cls(k=8)
    for call in (lambda: raw.topN(0), lambda: raw.topN_warm(X_col=col, X_val=val), lambda: raw.topN_cold(U=np.zeros(3)),
                 lambda: raw.factors_warm(X_col=col, X_val=val), lambda: raw.factors_cold(U=np.zeros(3)),
                 lambda: raw.predict_warm([1], X_col=col, X_val=val), lambda: raw.predict_cold([1], U=np.zeros(3))):
        with pytest.raises(ValueError, match="not fitted"):
            call()
    mdl = _fake_fitted(cls, p=3)
    # include together with exclude
    for call in (lambda: mdl.topN(0, include=[1, 2], exclude=[3]), lambda: mdl.topN_warm(X_col=col, X_val=val, include=[1, 2], exclude=[3]),
                 lambda: mdl.topN_cold(U=np.zeros(3), include=[1, 2], exclude=[3])):
        with pytest.raises(ValueError, match="both 'include' and 'exclude'"):
            call()
    # n beyond the kernels' limit: the text of return code 2
    for call in (lambda: mdl.topN(0, n=129), lambda: mdl.topN_warm(n=129, X_col=col, X_val=val), lambda: mdl.topN_cold(n=129, U=np.zeros(3)),
                 lambda: _fake_fitted(cls, n=50).topN(0, n=51)):
        with pytest.raises(RuntimeError, match=r"code 2.*n_top <= min\(128, n\)"):
            call()
    # other argument errors
    with pytest.raises(ValueError, match="user"):
        mdl.topN(60)
    with pytest.raises(ValueError, match="outside the model"):
        mdl.topN(0, exclude=[300])
    with pytest.raises(ValueError, match="together"):
        mdl.topN_warm(X_col=col)
    with pytest.raises(ValueError, match="Must pass"):
        mdl.topN_cold()
    with pytest.raises(ValueError, match="without user side information"):
        _fake_fitted(cls).topN_cold(U=np.zeros(3))
    _no_handles(mdl)
    mdl.close()                                              # nothing to release: a no-op


def test_U_bin_is_refused():
    from cmfrec_amd import CMF
    mdl = _fake_fitted(CMF, p=3)
    col, val = np.array([1, 5, 9]), np.array([1., 2., 3.])
    ub = np.zeros(4)
    for call in (lambda: mdl.topN_warm(X_col=col, X_val=val, U_bin=ub), lambda: mdl.topN_cold(U_bin=ub), lambda: mdl.factors_cold(U_bin=ub),
                 lambda: mdl.factors_warm(X_col=col, X_val=val, U_bin=ub), lambda: mdl.predict_warm([1], X_col=col, X_val=val, U_bin=ub),
                 lambda: mdl.predict_cold([1], U_bin=ub)):
        with pytest.raises(ValueError, match="U_bin"):
            call()
    _no_handles(mdl)


def test_reference_signatures():
    """The one-user methods take the reference's argument names in the reference's order."""
    import inspect
    from cmfrec_amd import CMF, CMF_implicit
    args = lambda f: list(inspect.signature(f).parameters)[1:]
    assert args(CMF.topN) == args(CMF_implicit.topN) == ["user", "n", "include", "exclude", "output_score"]
    assert args(CMF.topN_warm) == ["n", "X", "X_col", "X_val", "W", "U", "U_bin", "U_col", "U_val", "include", "exclude", "output_score"]
    assert args(CMF_implicit.topN_warm) == ["n", "X_col", "X_val", "U", "U_col", "U_val", "include", "exclude", "output_score"]
    assert args(CMF.topN_cold) == ["n", "U", "U_bin", "U_col", "U_val", "include", "exclude", "output_score"]
    assert args(CMF_implicit.topN_cold) == ["n", "U", "U_col", "U_val", "include", "exclude", "output_score"]
    assert args(CMF.factors_warm) == ["X", "X_col", "X_val", "W", "U", "U_bin", "U_col", "U_val", "return_bias"]
    assert args(CMF_implicit.factors_warm) == ["X_col", "X_val", "U", "U_col", "U_val"]
    assert args(CMF.factors_cold) == ["U", "U_bin", "U_col", "U_val"] and args(CMF_implicit.factors_cold) == ["U", "U_col", "U_val"]
    assert args(CMF.predict_warm) == ["items", "X", "X_col", "X_val", "W", "U", "U_bin", "U_col", "U_val"]
    assert args(CMF_implicit.predict_warm) == ["items", "X_col", "X_val", "U", "U_col", "U_val"]
    assert args(CMF.predict_cold) == ["items", "U", "U_bin", "U_col", "U_val"] and args(CMF_implicit.predict_cold) == ["items", "U", "U_col", "U_val"]
