"""The checks of tests/test_gpu_dense_ops.py can see a subtly wrong dense kernel, and accept an honest one (CPU only).

For every case the GPU file runs: (a) a stand-in kernel -- NumPy in the dtype, GEMM and Gramian summed in blocks of 256,
np.linalg.cholesky and scipy's triangular solve for potrf and trtri, the emulated route for the shared-matrix solve -- passes
the checks of tests/dense_reference.py; (b) each mutation of its result that applies to the shape is rejected by at least one
of the two data sets (printed with pytest -s: which).  The integer data alone catch a lost or doubled term at large K in
float32, where one term is below the rounding bound; the normal data alone catch float64 inputs accumulated in float32, which
is exact on small integers."""
import numpy as np
import pytest

import dense_reference as D


def _rejected(check, *args):
    try:
        check(*args)
    except D.Rejected:
        return True
    return False


def _judge(line, caught, applicable):
    for name in applicable:
        assert caught[name], "%s: mutation '%s' passes both data sets" % (line, name)
    print(line + " | " + "; ".join("%s: %s" % (n, "+".join(caught[n])) for n in applicable))


@pytest.mark.parametrize("case", D.gemm_cases(), ids=D.case_id)
def test_gemm_standin_passes_and_mutations_fail(case):
    dtype, transa, shape, layout = case
    M, N, K = shape
    ldc, oc = D.gemm_layout(layout, dtype, transa, M, N, K)[4:]
    caught = {}
    for data in D.DATA:
        good, muts = D.gemm_mutations(dtype, shape, data)
        img = D.image(good, ldc, oc, D.SENTINEL, dtype)
        r = D.check_gemm(dtype, transa, shape, layout, data, img)
        assert r <= 0.5, "the stand-in kernel uses more than half of the bound: %.3f" % r
        for name, c in muts.items():
            if _rejected(D.check_gemm, dtype, transa, shape, layout, data, D.image(c, ldc, oc, D.SENTINEL, dtype)):
                caught.setdefault(name, []).append(data)
            else:
                caught.setdefault(name, [])
        for pos in D.padding_positions(M, N, ldc, oc):
            bad = img.copy(); bad[pos] = np.nextafter(bad[pos], dtype(0))
            assert _rejected(D.check_gemm, dtype, transa, shape, layout, data, bad), "padding element %d" % pos
    _judge("gemm %s" % D.case_id(case), caught, list(caught))


@pytest.mark.parametrize("case", D.gram_cases(), ids=D.case_id)
def test_gram_standin_passes_and_mutations_fail(case):
    dtype, n, k, layout, scales = case
    oc = D.gram_layout(layout, dtype, k)[2]
    caught = {}
    for data in D.DATA:
        good, muts = D.gram_mutations(dtype, n, k, data, scales)
        img = D.image(good, k, oc, D.SENTINEL, dtype)
        r = D.check_gram(dtype, n, k, layout, data, scales, img)
        assert r <= 0.5, "the stand-in kernel uses more than half of the bound: %.3f" % r
        for name, c in muts.items():
            if _rejected(D.check_gram, dtype, n, k, layout, data, scales, D.image(c, k, oc, D.SENTINEL, dtype)):
                caught.setdefault(name, []).append(data)
            else:
                caught.setdefault(name, [])
        for pos in D.padding_positions(k, k, k, oc):
            bad = img.copy(); bad[pos] = np.nextafter(bad[pos], dtype(0))
            assert _rejected(D.check_gram, dtype, n, k, layout, data, scales, bad), "padding element %d" % pos
    _judge("gram %s" % D.case_id(case), caught, list(caught))


@pytest.mark.parametrize("case", D.potrf_cases(), ids=D.case_id)
def test_potrf_standin_passes_and_mutations_fail(case):
    dtype, n, data, off = case
    good, muts = D.potrf_mutations(dtype, n, data)
    img = D.image(good, n, off, D.SENTINEL, dtype)
    D.check_potrf(dtype, n, data, off, img)
    for name, c in muts.items():
        assert _rejected(D.check_potrf, dtype, n, data, off, D.image(c, n, off, D.SENTINEL, dtype)), name
    for pos in D.padding_positions(n, n, n, off):
        bad = img.copy(); bad[pos] = np.nextafter(bad[pos], dtype(0))
        assert _rejected(D.check_potrf, dtype, n, data, off, bad), "padding element %d" % pos
    if n >= 2:
        assert len(muts) == 2


@pytest.mark.parametrize("case", D.trtri_cases(), ids=D.case_id)
def test_trtri_standin_passes_and_mutations_fail(case):
    dtype, n, off = case
    good, muts = D.trtri_mutations(dtype, n)
    img = D.image(good, n, off, D.SENTINEL, dtype)
    D.check_trtri(dtype, n, off, img)
    for name, c in muts.items():
        assert _rejected(D.check_trtri, dtype, n, off, D.image(c, n, off, D.SENTINEL, dtype)), name
    for pos in D.padding_positions(n, n, n, off):
        bad = img.copy(); bad[pos] = np.nextafter(bad[pos], dtype(0))
        assert _rejected(D.check_trtri, dtype, n, off, bad), "padding element %d" % pos
    if n >= 2:
        assert len(muts) == 2


@pytest.mark.parametrize("case", D.potrs_cases(), ids=D.case_id)
def test_potrs_emulation_passes_with_a_factor_two_to_spare(case):
    """POTRS_C is the smallest power of two at which the emulated route (NumPy in the dtype) passes the forward criterion with
    a factor 2 to spare on every case; the padding of the rows is watched as everywhere."""
    dtype, k, rows, layout = case
    ldc, oc = D.potrs_layout(layout, k)
    x = D.potrs_emulation(dtype, k)[:rows]
    img = D.image(x, ldc, oc, D.SENTINEL, dtype)
    fwd, eta = D.check_potrs(dtype, k, rows, layout, img)
    print("potrs_rows %s: emulation forward %.4f, eta / ETA_SHARED %.4f" % (D.case_id(case), fwd, eta))
    assert fwd <= 0.5
    for pos in D.padding_positions(rows, k, ldc, oc):
        bad = img.copy(); bad[pos] = np.nextafter(bad[pos], dtype(0))
        assert _rejected(D.check_potrs, dtype, k, rows, layout, bad), "padding element %d" % pos


def test_gram_block_counts():
    """The row counts meant to reach the reduce stage's unrolled loop and the block cap do (host arithmetic of launch_gram)."""
    assert D.gram_blocks(0) == (1, 1)
    assert D.gram_blocks(6200)[0] == 49 and D.gram_blocks(8321)[0] == 66
    nb, rpb = D.gram_blocks(D.GRAM_N_BIG)
    assert nb == 511 and rpb % 64 != 0


def test_trtri_widths_straddle_the_lds_limits():
    for dt, (a, b, c, d) in ((np.float64, (54, 55, 77, 78)), (np.float32, (77, 78, 110, 111))):
        assert D.trtri_lds_bytes(a, dt) <= 48 * 1024 < D.trtri_lds_bytes(b, dt)
        assert D.trtri_lds_bytes(c, dt) <= 96 * 1024 < D.trtri_lds_bytes(d, dt)
