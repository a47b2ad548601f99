"""CPU: what the diversified top-N entry points refuse before a device is touched -- code 2, the limits in the message, the
outputs untouched."""
import ctypes as C

import numpy as np
import pytest

NU, N, K, POOL, NTOP = 3, 200, 8, 16, 4
SENTINEL = 77
LIMITS = "needs k <= 272, 1 <= n_top <= pool <= min(128, n) and 0 <= theta <= 1"

CASES = [(dict(pool=129), LIMITS), (dict(n_top=POOL + 1), LIMITS), (dict(n_top=0), LIMITS), (dict(theta=1.5), LIMITS), (dict(theta=-0.1), LIMITS),
         (dict(theta=float("nan")), LIMITS), (dict(k=273), LIMITS), (dict(n=10), LIMITS),
         (dict(out_ids=None), "invalid arguments; " + LIMITS), (dict(out_scores=None), "invalid arguments; " + LIMITS),
         (dict(A=None), "invalid arguments; " + LIMITS)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("changed,message", CASES, ids=lambda v: "-".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else "")
def test_batch_refusals(dtype, changed, message):
    from cmfrec_amd import _lib
    lib = _lib.load(dtype)
    a = dict(A=np.zeros((NU, 300), dtype), B=np.ones((N, 300), dtype), n=N, k=K, pool=POOL, theta=0.7, n_top=NTOP,
             out_ids=np.full(NU * 130, SENTINEL, np.int32), out_scores=np.full(NU * 130, SENTINEL, dtype), out_mmr=np.full(NU * 130, SENTINEL, dtype))
    a.update(changed)
    rc = lib.cmfrec_hip_topN_diverse_batch(_lib.ptr(a["A"]), a["k"], NU, _lib.ptr(a["B"]), a["k"], a["n"], a["k"], None, None, None, a["pool"], a["theta"],
                                           a["n_top"], _lib.ptr(a["out_ids"]), _lib.ptr(a["out_scores"]), _lib.ptr(a["out_mmr"]))
    assert rc == 2
    assert lib.cmfrec_hip_last_error().decode() == "cmfrec_hip_topN_diverse_batch: " + message
    assert all(a[o] is None or np.all(a[o] == SENTINEL) for o in ("out_ids", "out_scores", "out_mmr"))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_null_handle(dtype):
    from cmfrec_amd import _lib
    lib = _lib.load(dtype)
    ids = np.full(NU * POOL, SENTINEL, np.int32); sc = np.full(NU * POOL, SENTINEL, dtype)
    assert lib.cmfrec_hip_ranker_rerank_mmr(None, NU, POOL, _lib.ptr(ids), _lib.ptr(sc), 0.7, NTOP, _lib.ptr(ids), _lib.ptr(sc), None) == 2
    assert lib.cmfrec_hip_last_error().decode() == "cmfrec_hip_ranker_rerank_mmr: invalid arguments; " + LIMITS
    assert lib.cmfrec_hip_ranker_topN_diverse(None, _lib.ptr(sc), K, NU, None, None, POOL, 0.7, NTOP, _lib.ptr(ids), _lib.ptr(sc), None) == 2
    assert lib.cmfrec_hip_last_error().decode() == "cmfrec_hip_ranker_topN_diverse: invalid arguments; " + LIMITS
    assert np.all(ids == SENTINEL) and np.all(sc == SENTINEL)
