"""No GPU needed: the limits of the deep top-N entry points are host checks, and the cursor arguments of Ranker.topN_after
are checked before the library is called."""
import numpy as np
import pytest


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_deep_limits_need_no_gpu(dtype):
    """n_top beyond the items, n_top = 0 and k = 273: code 2 with the limits in the message, before a device is touched (on a
    machine without one anything later would be code 4)."""
    from cmfrec_amd import ops
    msg = r"code 2.*needs k <= 272 and 1 <= n_top <= n"
    with pytest.raises(RuntimeError, match=msg):
        ops.topN_deep_batch(np.zeros((4, 100), dtype), np.zeros((300, 100), dtype), n_top=301)
    with pytest.raises(RuntimeError, match=msg):
        ops.topN_deep_batch(np.zeros((4, 100), dtype), np.zeros((300, 100), dtype), n_top=0)
    with pytest.raises(RuntimeError, match=msg):
        ops.topN_deep_batch(np.zeros((4, 273), dtype), np.zeros((300, 273), dtype), n_top=5)


def _ranker_without_device(monkeypatch, nu_k=(6, 20), dtype=np.float64):
    """A Ranker object whose handle is a dummy and whose library raises when it is reached."""
    from cmfrec_amd import Ranker

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError("the library was called: " + name)
    r = Ranker.__new__(Ranker)
    r.handle = None
    monkeypatch.setattr(r, "_live", lambda: 1)
    r.lib = NoLibrary()
    r.dtype = np.dtype(dtype); r.n = 50; r.k = nu_k[1]
    return r, np.zeros(nu_k, dtype)


def test_after_cursor_arguments(monkeypatch):
    r, A = _ranker_without_device(monkeypatch)
    ids = np.zeros(6, np.int32); sc = np.zeros(6)
    with pytest.raises(ValueError, match="come together"):
        r.topN_after(A, ids, None)
    with pytest.raises(ValueError, match="come together"):
        r.topN_after(A, None, sc)
    with pytest.raises(ValueError, match="one entry per user"):
        r.topN_after(A, ids[:5], sc[:5])
    with pytest.raises(ValueError, match="one entry per user"):
        r.topN_after(A, ids, np.zeros(7))
    with pytest.raises(ValueError, match="one entry per user"):
        r.topN_after(A, np.zeros((6, 1), np.int32), np.zeros((6, 1)))
    with pytest.raises(ValueError, match="integers"):
        r.topN_after(A, np.zeros(6), sc)
    with pytest.raises(ValueError, match="another cursor"):
        r.topN_after(A, ids, sc.astype(np.float32))
    with pytest.raises(ValueError, match=r"A must be \[users, 20\]"):
        r.topN_deep(np.zeros((6, 21)), 10)
    # well-formed cursors pass the checks and reach the library
    with pytest.raises(AssertionError, match="the library was called"):
        r.topN_after(A, ids, sc)
    with pytest.raises(AssertionError, match="the library was called"):
        r.topN_after(A, None, None)
