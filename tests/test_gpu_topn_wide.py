"""GPU: top-N ranking of wide models (k > 64) on the MFMA kernel (topn_wide_kernels.hpp) against a float64 ranking with a
derived tolerance (topn_reference.py), the kernel's corner cases, and CMFREC_HIP_TOPN=wide against the default kernel."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import topn_reference as tr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WIDTHS = [(np.float64, k) for k in (65, 128, 129, 250, 256)] + [(np.float32, k) for k in (65, 200, 257, 272)]
# n_top with the other dimensions of the case: (n_top, nu, n, bias, exclusion lists)
SHAPES = [(1, 33, 3000, True, True), (10, 70, 5003, False, True), (100, 70, 3000, True, False), (128, 33, 5003, True, True)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "top%d-nu%d-n%d-%s-%s" % (s[0], s[1], s[2], "bias" if s[3] else "nobias", "excl" if s[4] else "noexcl"))
@pytest.mark.parametrize("dtype,k", WIDTHS, ids=lambda v: getattr(v, "__name__", str(v)))
def test_wide_ranking(dtype, k, shape):
    """Every width beyond 64 against the float64 ranking: the four conditions of topn_reference.check_ranking; in double
    precision the inputs leave no position undecided, so every id must be the reference's.  (Before this kernel every case
    here failed with 'RuntimeError ... code 2'.)"""
    from cmfrec_amd import ops
    n_top, nu, n, bias, excl = shape
    A, B, b, ep, ei = tr.make_problem(1000 * k + n_top, dtype, nu, n, k, bias=bias, excl=excl)
    ids, sc = ops.topN_batch(A, B, n_top=n_top, biasB=b, exclude=None if ep is None else (ep, ei))
    if ep is not None:                                       # ops sorts each list; the reference takes them as a set
        assert ep[1] == 0                                    # user 0: empty list
    tr.check_ranking(A, B, b, ep, ei, ids, sc, n_top, dtype, all_decided=dtype is np.float64)


@pytest.mark.parametrize("tiles", [1, 2, 3, 4])
@pytest.mark.parametrize("dtype,k,n_top", [(np.float64, 128, 10), (np.float32, 200, 100), (np.float64, 256, 100)], ids=lambda v: getattr(v, "__name__", str(v)))
def test_user_tiles_per_workgroup(monkeypatch, dtype, k, n_top, tiles):
    """The kernel's instantiations for 16, 32, 48 and 64 users per workgroup (the host picks by shape; a small batch would only
    ever see the first): same checks, with users that do not fill the last tile, and the same bits whatever the tiling."""
    from cmfrec_amd import ops
    A, B, b, ep, ei = tr.make_problem(77 + k, dtype, 70, 3000, k)
    monkeypatch.setenv("CMFREC_HIP_TOPN_TILES", str(tiles))
    ids, sc = ops.topN_batch(A, B, n_top=n_top, biasB=b, exclude=(ep, ei))
    tr.check_ranking(A, B, b, ep, ei, ids, sc, n_top, dtype, all_decided=dtype is np.float64)
    monkeypatch.setenv("CMFREC_HIP_TOPN_TILES", "1")
    ids1, sc1 = ops.topN_batch(A, B, n_top=n_top, biasB=b, exclude=(ep, ei))
    assert np.array_equal(ids, ids1) and np.array_equal(sc, sc1)


@pytest.mark.parametrize("dtype,k", [(np.float64, 129), (np.float32, 257)], ids=lambda v: getattr(v, "__name__", str(v)))
def test_strided_operands(dtype, k):
    """lda > k and ldb > k with the pointers offset by k_user / k_item, through the C entry point."""
    from cmfrec_amd import _lib
    k_user, k_item, nu, n, n_top = 3, 5, 33, 3000, 10
    A, B, b, ep, ei = tr.make_problem(5, dtype, nu, n, k)
    rng = np.random.default_rng(6)
    Af = rng.standard_normal((nu, k_user + k)).astype(dtype); Af[:, k_user:] = A
    Bf = rng.standard_normal((n, k_item + k)).astype(dtype); Bf[:, k_item:] = B
    owner = np.repeat(np.arange(nu), np.diff(ep.astype(np.int64)))
    eis = np.ascontiguousarray(ei[np.lexsort((ei, owner))])
    lib = _lib.load(dtype)
    ids = np.empty((nu, n_top), np.int32); sc = np.empty((nu, n_top), dtype)
    isz = np.dtype(dtype).itemsize
    rc = lib.cmfrec_hip_topN_batch(C.c_void_p(Af.ctypes.data + k_user * isz), C.c_size_t(k_user + k), C.c_int(nu),
                                   C.c_void_p(Bf.ctypes.data + k_item * isz), C.c_size_t(k_item + k), C.c_int(n), C.c_int(k),
                                   _lib.ptr(b), _lib.ptr(ep), _lib.ptr(eis), C.c_int(n_top), _lib.ptr(ids), _lib.ptr(sc))
    _lib.check(rc, lib, "topN_batch")
    tr.check_ranking(A, B, b, ep, ei, ids, sc, n_top, dtype, all_decided=dtype is np.float64)


@pytest.mark.parametrize("dtype,k", [(np.float64, 128), (np.float32, 272)], ids=lambda v: getattr(v, "__name__", str(v)))
def test_corner_cases(dtype, k):
    """Fewer than n_top items left: -1 ids and -inf scores; an item with a NaN factor is never returned; scores are optional
    in the C entry point; two identical calls give the same bits."""
    from cmfrec_amd import ops, _lib
    nu, n, n_top = 20, 300, 10
    A, B, b, _, _ = tr.make_problem(9, dtype, nu, n, k, excl=False)
    B[5, k // 2] = np.nan
    lens = np.zeros(nu, np.int64); lens[1] = n - 3; lens[2] = n; lens[4] = 17
    rng = np.random.default_rng(10)
    ep = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    ei = np.concatenate([rng.choice(n, l, replace=False) for l in lens]).astype(np.int32)
    ids, sc = ops.topN_batch(A, B, n_top=n_top, biasB=b, exclude=(ep, ei))
    assert not (ids == 5).any()
    assert (ids[1, :3] >= 0).all() and (ids[1, 3:] == -1).all() and np.isneginf(sc[1, 3:]).all() and np.isfinite(sc[1, :3]).all()
    assert (ids[2] == -1).all() and np.isneginf(sc[2]).all()
    # the reference: item 5 (a zero row there, NaN-free) excluded for every user
    Bok = B.copy(); Bok[5] = 0
    lists = [np.union1d(ei[int(ep[u]):int(ep[u + 1])], [5]).astype(np.int32) for u in range(nu)]
    ep5 = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
    tr.check_ranking(A, Bok, b, ep5, np.concatenate(lists), ids, sc, n_top, dtype, all_decided=dtype is np.float64)
    ids2, sc2 = ops.topN_batch(A, B, n_top=n_top, biasB=b, exclude=(ep, ei))
    assert np.array_equal(ids, ids2) and np.array_equal(sc, sc2)
    # out_scores = NULL
    lib = _lib.load(dtype)
    owner = np.repeat(np.arange(nu), np.diff(ep.astype(np.int64)))
    eis = np.ascontiguousarray(ei[np.lexsort((ei, owner))])
    ids3 = np.empty((nu, n_top), np.int32)
    rc = lib.cmfrec_hip_topN_batch(_lib.ptr(A), C.c_size_t(k), C.c_int(nu), _lib.ptr(B), C.c_size_t(k), C.c_int(n), C.c_int(k),
                                   _lib.ptr(b), _lib.ptr(ep), _lib.ptr(eis), C.c_int(n_top), _lib.ptr(ids3), None)
    _lib.check(rc, lib, "topN_batch")
    assert np.array_equal(ids3, ids)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_limits_are_host_checks(dtype):
    """k = 273 and n_top = 129: return code 2 with the limit in the message."""
    from cmfrec_amd import ops
    rng = np.random.default_rng(0)
    with pytest.raises(RuntimeError, match=r"code 2.*k <= 272"):
        ops.topN_batch(rng.standard_normal((4, 273)).astype(dtype), rng.standard_normal((300, 273)).astype(dtype), n_top=5)
    with pytest.raises(RuntimeError, match=r"code 2.*n_top <= min\(128, n\)"):
        ops.topN_batch(rng.standard_normal((4, 100)).astype(dtype), rng.standard_normal((300, 100)).astype(dtype), n_top=129)
    with pytest.raises(RuntimeError, match=r"code 2.*n_top <= min\(128, n\)"):
        ops.topN_batch(rng.standard_normal((4, 100)).astype(dtype), rng.standard_normal((50, 100)).astype(dtype), n_top=51)


CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import topn_reference as tr
from cmfrec_amd import ops
out = {}
for dt, tag in ((np.float64, "f64"), (np.float32, "f32")):
    for k in (8, 50, 64):
        A, B, b, ep, ei = tr.make_problem(300 + k, dt, 70, 3000, k)
        for n_top in (10, 100):
            ids, sc = ops.topN_batch(A, B, n_top=n_top, biasB=b, exclude=(ep, ei))
            out["ids_%%s_%%d_%%d" %% (tag, k, n_top)] = ids; out["sc_%%s_%%d_%%d" %% (tag, k, n_top)] = sc
np.savez(sys.argv[1], **out)
"""


def _run(tmp_path, name, env):
    path = str(tmp_path / (name + ".npz"))
    e = dict(os.environ)
    e.pop("CMFREC_HIP_TOPN", None); e.pop("CMFREC_HIP_TOPN_TILES", None)
    e.update(env)
    code = CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code, path], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(path)


def test_wide_switch_agrees_with_default_kernel(tmp_path):
    """CMFREC_HIP_TOPN=wide sends k <= 64 through the MFMA kernel too: in double precision the same ids as the default kernel
    and scores within E_u; in single precision conditions 1-3 against the float64 ranking."""
    dflt = _run(tmp_path, "default", {})
    wide = _run(tmp_path, "wide", {"CMFREC_HIP_TOPN": "wide"})
    assert set(dflt.files) == set(wide.files)
    for dt, tag in ((np.float64, "f64"), (np.float32, "f32")):
        for k in (8, 50, 64):
            A, B, b, ep, ei = tr.make_problem(300 + k, dt, 70, 3000, k)
            E = tr.bounds(A, B, b, dt)
            for n_top in (10, 100):
                key = "%s_%d_%d" % (tag, k, n_top)
                ids, sc = wide["ids_" + key], wide["sc_" + key]
                tr.check_ranking(A, B, b, ep, ei, ids, sc, n_top, dt, all_decided=dt is np.float64)
                if dt is np.float64:
                    assert np.array_equal(ids, dflt["ids_" + key]), key
                    assert np.all(np.abs(sc - dflt["sc_" + key]) <= E[:, None]), key
