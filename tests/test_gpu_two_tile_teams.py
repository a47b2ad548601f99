"""GPU: double-precision CG rows of 65..96 entries on one wavefront and of 257..384 entries on four wavefronts, two resident tiles
per wavefront (cg_kernels.hpp, NRES_ = 2 with NTSEL = 1; launch_cg.hip, launch_cg_bin_by_tile; CMFREC_HIP_TWO_TILES).

One matrix serves the parity cases: every length at which a row changes its route or its tile -- 64 | 65 (one-wavefront bin | two-wave
bin), 80 | 81 and 320 | 321 (5 | 6 entries per lane group), 96 | 97 and 384 | 385 (two tiles | the teams as before), 128, 256 | 257,
512 | 513 (the eight-wave bin's last resident row | a split row where the Gramian path takes them, a re-streamed row where not) --
three rows each, 45 solved rows (the 15 lengths do not fit the 40 rows the shapes were sketched with) against 600 opposing rows.
Against the oracle with the criteria and tolerances of test_gpu_operators.py::test_optimizeA_implicit / ::test_optimizeA_explicit,
with the switch on and off; the grid by occupancy (every team one row) and CMFREC_HIP_CG_TEAMS=2 (one workgroup of four one-wavefront
teams with three rows of 65..96 entries each, two four-wave teams with six rows of 257..384 each: the row-to-row pipeline and the
claims from the work counter)."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from conftest import rel_err, row_rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-10          # as tests/test_gpu_operators.py, double precision
ROW_TOL = 1e-9
LENS = [64, 65, 80, 81, 96, 97, 128, 256, 257, 320, 321, 384, 385, 512, 513]
M, N = 3 * len(LENS), 600
SWITCHES = ("CMFREC_HIP_TWO_TILES", "CMFREC_HIP_CG_TEAMS", "CMFREC_HIP_POISON_LDS", "CMFREC_HIP_BINS_PAR", "CMFREC_HIP_VH",
            "CMFREC_HIP_NT_SPLIT", "CMFREC_HIP_CG_KERNEL", "CMFREC_HIP_VH_MIN")
dtype = np.float64


@contextmanager
def _env(env):
    old = {n_: os.environ.pop(n_, None) for n_ in SWITCHES}
    os.environ.update(env)
    try:
        yield
    finally:
        for n_ in SWITCHES:
            os.environ.pop(n_, None)
            if old[n_] is not None:
                os.environ[n_] = old[n_]


def _rows(lens, seed, implicit):
    """CSR (indptr, indices, values) with the given row lengths, columns without repetition inside a row."""
    rng = np.random.default_rng(seed)
    idx = np.concatenate([rng.choice(N, size=l_, replace=False) for l_ in lens]).astype(np.int32)
    val = np.ceil(rng.lognormal(1, 1, len(idx))) if implicit else 0.5 * rng.integers(1, 11, len(idx))
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), idx, val.astype(dtype)


def _stack(parts):
    """rows of several CSR triplets below each other"""
    p = [np.zeros(1, np.uint64)]
    for q in parts:
        p.append(q[0][1:] + p[-1][-1])
    return np.concatenate(p), np.concatenate([q[1] for q in parts]), np.concatenate([q[2] for q in parts])


def _lens_matrix():
    rng = np.random.default_rng(31)
    return rng.permutation(np.repeat(LENS, 3))          # row ids in no order of length


def _factors(k, m, implicit):
    rng = np.random.default_rng(k)
    pad = 0 if implicit else 1
    A0 = rng.standard_normal((m, k + pad)) * 0.05
    B = rng.standard_normal((N, k + pad)) * 0.2         # (explicit: the bias column behind the k solved ones, rows of 8 (k + 1) bytes)
    bias = rng.standard_normal(N) * 0.3
    return A0, B, bias


def _solve(oracle, implicit, k, csr, A0, B, bias):
    """the half-step on the device (oracle None) or by the oracle, as test_gpu_operators.py calls them"""
    from cmfrec_amd import ops
    A = A0.copy()
    if implicit:
        if oracle is None:
            ops.optimizeA_implicit(A, B, csr, 4.0, use_cg=True, max_cg_steps=3)
        else:
            oracle.optimizeA_implicit(A, B, csr, 4.0, nthreads=4, use_cg=True, max_cg_steps=3)
    else:
        kw = dict(k=k, lam_last=0.3, scale_lam=True, use_cg=True, max_cg_steps=3)
        if oracle is None:
            ops.optimizeA_explicit(A, B, csr, 0.05, bias_sub=bias, **kw)
        else:       # (what the reference's host sweep does)
            oracle.optimizeA_explicit(A, B, (csr[0], csr[1], csr[2] - bias[csr[1]]), 0.05, nthreads=4, **kw)
    return A


def _device(implicit, k, env, csr=None, A0=None):
    if csr is None:
        csr = _rows(_lens_matrix(), 7 + k, implicit)
    A0_, B, bias = _factors(k, M, implicit)
    with _env(env):             # (the switches are read when the entry point creates its session)
        return _solve(None, implicit, k, csr, A0_ if A0 is None else A0, B, bias)


_cache = {}


def _expected(oracles, implicit, k):
    if (implicit, k) not in _cache:
        A0, B, bias = _factors(k, M, implicit)
        A = _solve(oracles[dtype], implicit, k, _rows(_lens_matrix(), 7 + k, implicit), A0, B, bias)
        A.setflags(write=False)
        _cache[(implicit, k)] = A
    return _cache[(implicit, k)]


def _check(got, exp, k, what):
    assert np.isfinite(got).all(), what
    e, (er, r) = rel_err(got, exp), row_rel_err(got[:, :k], exp[:, :k])
    print("%s: relative error %.3e, worst row %d (%d entries) %.3e" % (what, e, r, _lens_matrix()[r], er))
    assert e < TOL, what
    assert er < ROW_TOL, "%s row %d: per-row relative error %.3e" % (what, r, er)
    assert np.array_equal(got[:, k:], exp[:, k:])       # (explicit: the column behind the solved ones is never written)


@pytest.mark.parametrize("teams", [0, 2], ids=["grid-by-occupancy", "two-teams"])
@pytest.mark.parametrize("two_tiles", ["1", "0"], ids=["two-tiles", "one-tile"])
@pytest.mark.parametrize("implicit", [True, False], ids=["implicit", "explicit"])
@pytest.mark.parametrize("k", [50, 32, 56])
def test_boundary_lengths(oracles, k, implicit, two_tiles, teams):
    env = {"CMFREC_HIP_TWO_TILES": two_tiles}
    if teams:
        env["CMFREC_HIP_CG_TEAMS"] = str(teams)
    _check(_device(implicit, k, env), _expected(oracles, implicit, k), k, "k %d %s" % (k, env))


@pytest.mark.parametrize("two_tiles", ["1", "0"], ids=["two-tiles", "one-tile"])
@pytest.mark.parametrize("implicit", [True, False], ids=["implicit", "explicit"])
def test_boundary_lengths_gramian_path(oracles, implicit, two_tiles):
    """The rows of 513 entries as split rows on the Gramian path (forced: three such rows do not choose it by themselves), the eight-wave bin
    ending at 512."""
    env = {"CMFREC_HIP_TWO_TILES": two_tiles, "CMFREC_HIP_VH": "gram"}
    _check(_device(implicit, 50, env), _expected(oracles, implicit, 50), 50, "k 50 %s" % env)


@pytest.mark.parametrize("implicit", [True, False], ids=["implicit", "explicit"])
def test_poisoned_lds(oracles, implicit):
    """NaN patterns in the LDS of every CU in front of the launches (as tests/test_gpu_poisoned_lds.py): the new teams read nothing they
    have not written -- the pass vector's buffer, from which the Gramian weights are now fetched late, least of all."""
    for teams in ({}, {"CMFREC_HIP_CG_TEAMS": "2"}):
        env = dict(teams, CMFREC_HIP_TWO_TILES="1", CMFREC_HIP_POISON_LDS="1")
        _check(_device(implicit, 50, env), _expected(oracles, implicit, 50), 50, "k 50 %s" % env)


@pytest.mark.parametrize("implicit", [True, False], ids=["implicit", "explicit"])
def test_bits_follow_the_length_alone(implicit):
    """A row of 90 and a row of 300 entries among the boundary rows, and the same two among other rows at other positions; then the bins
    in line instead of side by side: the two rows (second case: all rows) byte for byte."""
    k = 50
    pair = _rows([90, 300], 5, implicit)
    first = _rows(_lens_matrix()[:M - 2], 7 + k, implicit)
    rng = np.random.default_rng(77)
    other = _rows(rng.integers(1, 500, M - 2), 8, implicit)
    A0 = _factors(k, M, implicit)[0]
    A0b = A0.copy()
    A0b[:2] = A0[M - 2:]                                                   # (the pair starts from the same values in both)
    a = _device(implicit, k, {}, csr=_stack([first, pair]))                # the pair in rows M - 2, M - 1
    b = _device(implicit, k, {}, csr=_stack([pair, other]), A0=A0b)        # ... in rows 0, 1
    assert np.isfinite(a).all() and np.isfinite(b).all()
    assert not np.array_equal(a[M - 2:, :k], A0[M - 2:, :k])
    assert a[M - 2:].tobytes() == b[:2].tobytes()
    inline = _device(implicit, k, {"CMFREC_HIP_BINS_PAR": "1"}, csr=_stack([first, pair]))
    assert inline.tobytes() == a.tobytes()
    few = _device(implicit, k, {"CMFREC_HIP_CG_TEAMS": "2"}, csr=_stack([first, pair]))
    assert few.tobytes() == a.tobytes()


@pytest.mark.parametrize("implicit", [True, False], ids=["implicit", "explicit"])
@pytest.mark.parametrize("k", [64, 16])
def test_other_routes_unchanged(k, implicit):
    """k = 64 (S = 8: above the launches by tile size) and k = 16 (below them) are not rerouted: the switch changes no bit."""
    on = _device(implicit, k, {"CMFREC_HIP_TWO_TILES": "1"})
    off = _device(implicit, k, {"CMFREC_HIP_TWO_TILES": "0"})
    assert np.isfinite(on).all()
    assert on.tobytes() == off.tobytes()


def test_switch_reroutes():
    """... and at k = 50 it does change the order the tile partials of the rows of 65..96 and 257..384 entries are added in (their
    accuracy is test_boundary_lengths' matter), and no other row's bits; the values 2 and 3 move one of the two ranges alone."""
    off = _device(True, 50, {"CMFREC_HIP_TWO_TILES": "0"})
    lens = _lens_matrix()
    short, long_ = (lens > 64) & (lens <= 96), (lens > 256) & (lens <= 384)
    on = {}
    for value, moved in (("1", short | long_), ("2", short), ("3", long_)):
        on[value] = _device(True, 50, {"CMFREC_HIP_TWO_TILES": value})
        assert on[value][~moved].tobytes() == off[~moved].tobytes(), value
        assert not np.array_equal(on[value][moved], off[moved]), value
    assert on["2"][short].tobytes() == on["1"][short].tobytes() and on["3"][long_].tobytes() == on["1"][long_].tobytes()
