"""CPU: the ``filter=`` keyword's argument checking and the shortlist-length rule of the certified fp16 filter (no device is used)."""
import numpy as np
import pytest


def test_filter_argument():
    from cmfrec_amd import Ranker, ops
    from cmfrec_amd.rank import filter_code
    assert filter_code(None) == 0 and filter_code("fp16") == 1
    for bad in ("fp8", "FP16", 1, True, ""):
        with pytest.raises(ValueError, match="filter"):
            filter_code(bad)
    A, B = np.zeros((3, 4)), np.ones((6, 4))
    with pytest.raises(ValueError, match="filter"):         # refused before anything is loaded or built
        Ranker(B, filter="bf16")
    with pytest.raises(ValueError, match="filter"):
        ops.topN_batch(A, B, n_top=2, filter="half")
    with pytest.raises(ValueError, match="include"):
        ops.topN_batch(A, B, n_top=2, include=np.arange(3), filter="fp16")


@pytest.mark.parametrize("n_top,forced,m", [(1, 0, 32), (16, 0, 32), (17, 0, 64), (32, 0, 64), (33, 0, 128), (64, 0, 128), (16, 32, 32),
                                            (10, 100, 128), (10, 64, 64), (64, 32, 64), (10, 31, 32), (10, 129, 32)])
def test_shortlist_length(n_top, forced, m):
    """M = max(32, pow2(2 n_top)) <= 128; a forced length of 32 .. 128 rounds up to a power of two, never below n_top."""
    from cmfrec_amd.rank import filter_shortlist
    assert filter_shortlist(n_top, forced) == m
