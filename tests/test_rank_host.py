"""No GPU needed: the argument checks of cmfrec_amd.Ranker, its failure without a device, and the export list."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ranker_rejects_bad_input_before_the_library(monkeypatch):
    from cmfrec_amd import Ranker, _lib

    def no_library(*a, **kw):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_library)
    B = np.zeros((30, 70))
    with pytest.raises(ValueError, match="2-D"):
        Ranker(np.zeros(30))
    with pytest.raises(ValueError, match="2-D"):
        Ranker(np.zeros((3, 4, 5)))
    with pytest.raises(ValueError, match="float64 or float32"):
        Ranker(np.zeros((30, 70), np.int32))
    with pytest.raises(ValueError, match="biasB is float32"):
        Ranker(B, np.zeros(30, np.float32))
    with pytest.raises(ValueError, match="one entry per item"):
        Ranker(B, np.zeros(29))
    with pytest.raises(ValueError, match="one entry per item"):
        Ranker(B, np.zeros((30, 1)))
    with pytest.raises(ValueError, match="empty"):
        Ranker(np.zeros((0, 70)))


def test_ranker_needs_a_gpu():
    """Without a GPU creating a ranker raises, like the rest of the package (test_abi.test_no_cpu_fallback)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from cmfrec_amd import Ranker, ops
    rng = np.random.default_rng(0)
    with pytest.raises((RuntimeError, MemoryError)):
        Ranker(rng.standard_normal((30, 70)))
    with pytest.raises((RuntimeError, MemoryError)):
        ops.topN_batch(rng.standard_normal((4, 70)), rng.standard_normal((30, 70)), n_top=5)


def test_limits_need_no_gpu():
    """The limits are host checks made before anything touches a device: they answer with code 2 on a machine without one."""
    from cmfrec_amd import ops
    with pytest.raises(RuntimeError, match=r"code 2.*k <= 272"):
        ops.topN_batch(np.zeros((4, 273)), np.zeros((300, 273)), n_top=5)
    with pytest.raises(RuntimeError, match=r"code 2.*n_top <= min\(128, n\)"):
        ops.topN_batch(np.zeros((4, 100)), np.zeros((300, 100)), n_top=129)


def test_ranker_names_are_exported():
    from cmfrec_amd import _lib
    names = ["cmfrec_hip_ranker_create", "cmfrec_hip_ranker_topN", "cmfrec_hip_ranker_kernel_ms", "cmfrec_hip_ranker_destroy"]
    txt = open(os.path.join(ROOT, "cmfrec_amd", "csrc", "exports.map")).read()
    assert "cmfrec_hip_*;" in txt                            # the pattern that covers them
    hdr = open(os.path.join(ROOT, "include", "cmfrec_hip.h")).read()
    for dt in (np.float64, np.float32):
        lib = _lib.load(dt)
        for nm in names:
            assert nm in _lib.EXPORTED and nm + "(" in hdr
            assert hasattr(lib, nm), nm
