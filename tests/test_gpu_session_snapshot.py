"""AlsSession.snapshot / .restore (cmfrec_hip_session_snapshot / _restore): a snapshot, two more iterations, a restore -- every
matrix get_factors / get_implicit_features return equals its earlier self bit for bit, and the iterations that follow a restore
are those that followed the snapshot."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M, N, K, KM = 90, 70, 6, 1
P, Q = 5, 4


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _state(s, features):
    out = dict(s.get_factors())
    if features:
        out["Ai"], out["Bi"] = s.get_implicit_features(M, N, K + KM)
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for key in a:
        assert (a[key] is None) == (b[key] is None), key
        if a[key] is not None and not np.array_equal(_bits(a[key]), _bits(b[key])):
            return key
    return None


def _session(case, dtype, use_cg):
    from cmfrec_amd import AlsSession
    rng = np.random.default_rng(5)
    at = rng.choice(M * N, 900, replace=False)
    row, col = (at // N).astype(np.int32), (at % N).astype(np.int32)
    implicit = case == "implicit"
    val = (rng.integers(1, 4, 900) if implicit else 0.5 * rng.integers(1, 11, 900)).astype(dtype)
    gm = 0.0 if implicit else float(np.dtype(dtype).type(val.mean()))
    side = case == "explicit_side"
    ku, ki = (1, 2) if side else (0, 0)
    s = AlsSession(M, N, K, implicit=implicit, dtype=dtype, lam=0.4, use_cg=use_cg, k_main=KM, k_user=ku, k_item=ki, user_bias=side, item_bias=side,
                   p=P if side else 0, q=Q if side else 0, m_u=M if side else 0, n_i=N if side else 0)
    s.set_X_coo(row, col, val, subtract=gm)
    if side:
        U = rng.standard_normal((M, P)).astype(dtype); II = rng.standard_normal((N, Q)).astype(dtype)
        s.set_sideinfo(U - U.mean(axis=0), II - II.mean(axis=0))
    s.set_factors(A=(0.3 * rng.standard_normal((M, ku + K + KM))).astype(dtype), B=(0.3 * rng.standard_normal((N, ki + K + KM))).astype(dtype),
                  biasA=(0.1 * rng.standard_normal(M)).astype(dtype) if side else None, biasB=(0.1 * rng.standard_normal(N)).astype(dtype) if side else None,
                  Cm=(0.1 * rng.standard_normal((P, ku + K))).astype(dtype) if side else None,
                  Dm=(0.1 * rng.standard_normal((Q, ki + K))).astype(dtype) if side else None)
    if case == "features":
        s.set_implicit_features(0.5)
    return s


# (the implicit features are Cholesky solves whatever use_cg says: one solver is enough for them)
@pytest.mark.parametrize("case,use_cg", [("explicit_side", True), ("explicit_side", False), ("implicit", True), ("implicit", False),
                                         ("features", False)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_snapshot_restore(dtype, case, use_cg):
    features = case == "features"
    s = _session(case, dtype, use_cg)
    try:
        s.iterate(1, False)
        s.snapshot()
        kept = _state(s, features)
        for key, v in kept.items():
            assert v is None or np.isfinite(v).all(), key
        s.iterate(2, False)
        later = _state(s, features)
        assert _same(kept, later) is not None, "two iterations changed nothing: the test shows nothing"
        s.restore()
        back = _state(s, features)
        assert _same(kept, back) is None, "%s differs after the restore" % _same(kept, back)
        # the state an update starts from is all there: the two iterations again, from the restored factors
        s.iterate(2, False)
        again = _state(s, features)
        assert _same(later, again) is None, "%s differs when the iterations are repeated from the restored factors" % _same(later, again)
        # the snapshot is still the one taken: a second restore, without a new snapshot
        s.restore()
        assert _same(kept, _state(s, features)) is None
        # a later snapshot replaces it
        s.iterate(1, False)
        s.snapshot()
        newer = _state(s, features)
        s.iterate(1, False)
        s.restore()
        assert _same(newer, _state(s, features)) is None
    finally:
        s.close()


def test_restore_without_snapshot_and_shards():
    from cmfrec_amd import AlsSession
    s = AlsSession(M, N, K, implicit=True)
    try:
        assert s.lib.cmfrec_hip_session_restore(s.handle) == 2
        assert b"no snapshot" in s.lib.cmfrec_hip_last_error()
        with pytest.raises(RuntimeError, match="code 2"):
            s.restore()
        s.snapshot()
        s.restore()
    finally:
        s.close()
    shard = AlsSession(M, N, K, implicit=True, row_range=(0, 40))
    try:
        assert shard.lib.cmfrec_hip_session_snapshot(shard.handle) == 2
        assert b"owns all rows" in shard.lib.cmfrec_hip_last_error()
        assert shard.lib.cmfrec_hip_session_restore(shard.handle) == 2
    finally:
        shard.close()
