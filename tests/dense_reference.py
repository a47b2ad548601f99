"""The dense kernels against references of their own operations (helpers, no tests).

`cmfrec_hip_dense_op` (ops.dense_op) runs one operation of dense_kernels.hpp through the launch helpers the library itself
uses: the GEMM (both TRANSA), the Gramian, potrf_upper, trtri_from_upper and the shared-matrix solve launch_potrs_rows.  This
module draws the inputs, lays them out as images with leading dimensions and offsets, computes the references and checks a
result; tests/test_gpu_dense_ops.py runs the checks on the GPU's results, tests/test_dense_bound_sensitivity.py on a stand-in
kernel (NumPy in the dtype) and on mutations of its result.

The reference is NumPy on the exact upcasts of the dtype-rounded inputs: float64 for float32 inputs, np.longdouble (64-bit
significand) for float64 inputs, whose error is 2^-11 / 2^-29 of the bounds below and is not added to them.

Two data sets per shape:

- exact: entries in {-2, -1, 1, 2} (no zeros: every term counts), s1 = 0.5, s2 = 3.  Every partial sum is an integer below
  2^24, so every summation order, split and MFMA gives the same bits, and the result must EQUAL the integer result: a dropped,
  doubled or misplaced term shows at any K.  potrf: M = R^T R of an integer upper-triangular R with diagonal in {2, 3}; every
  intermediate is an integer, the factor must equal R.
- normal: standard normal entries, s1 = 2.5, against componentwise bounds with gamma_j = j u / (1 - j u):
    GEMM     |C^ - C|_ij <= gamma_{K + ceil(K / 256) + 2} |s1| (|A| |B|)_ij     (K products and sums in any order, the split's
             partial sums under the rule "chunks of at least 256", alpha)
    Gramian  the same with K = n, plus one ulp of the result on a shifted diagonal; bitwise symmetric for k <= 64
    potrf    |M - R^^T R^| <= gamma_{n + 1} |R^^T| |R^|                       (Higham, Accuracy and Stability, theorem 10.3)
    trtri    row j of Linv = x^ with |R x^ - e_j| <= gamma_n |R| |x^|         (Higham, theorem 8.5); zeros right of the diagonal
  In all cases the padding of the output image must keep the bits of SENTINEL, and the padding of the inputs holds NaN: a kernel
  that reads outside its operand and masks by multiplying shows it.

launch_potrs_rows (explicit inverse; float32: one refinement step) has no componentwise bound.  Per row, with x64 the solution
in the reference precision, e_x,r = fp32_reference.row_errors and e_o the same-precision LAPACK solve:
    e_h,r <= 4 e_o,r + POTRS_C n cond_2(M) u,       float32 also: eta_r <= fp32_reference.ETA_SHARED.
POTRS_C is fixed against the CPU emulation of the route and LAPACK, never against the kernel: see beside the constant."""
import functools
import zlib

import numpy as np

from fp32_reference import ETA_SHARED, _log, row_errors
from topn_reference import gamma, unit_roundoff

SENTINEL = -12345.678
DTYPES = (np.float64, np.float32)
DATA = ("exact", "normal")
S1 = {"exact": 0.5, "normal": 2.5}


def _name(dtype):
    return np.dtype(dtype).name


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _wide(dtype):
    """The precision of the reference for inputs of `dtype`."""
    return np.longdouble if np.dtype(dtype) == np.float64 else np.float64


def _vec(dtype):
    return 16 // np.dtype(dtype).itemsize


def _ints(rng, shape):
    return rng.choice(np.array([-2.0, -1.0, 1.0, 2.0]), size=shape)


# ---- images ----------------------------------------------------------------------------------------------------------------

def odd_ld(cols):
    """The smallest odd leading dimension above `cols`."""
    return cols + 1 if cols % 2 == 0 else cols + 2


def padded_ld(cols, dtype):
    """The smallest multiple of 16 bytes above `cols` elements (so that the rows keep their alignment and have padding)."""
    v = _vec(dtype)
    return (cols + v) // v * v


def image(mat, ld, off, fill, dtype):
    """Flat image of off + rows * ld elements holding `mat` from element `off`, `fill` everywhere else."""
    rows, cols = mat.shape
    assert ld >= cols
    img = np.full(off + rows * ld, fill, dtype)
    if rows:
        img[off:].reshape(rows, ld)[:, :cols] = mat
    return img


def _bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def split_image(img, rows, cols, ld, off):
    """(the [rows, cols] operand of an output image, whether every other element still holds SENTINEL's bits)."""
    body = img[off:off + rows * ld].reshape(rows, ld)
    pad = np.ones(len(img), bool)
    pad[off:off + rows * ld].reshape(rows, ld)[:, :cols] = False
    want = _bits(np.array([SENTINEL], img.dtype))[0]
    return body[:, :cols].copy(), bool(np.all(_bits(img)[pad] == want))


def _ratio(err, bound):
    """max err / bound with 0 / 0 = 0 and x / 0 = inf; NaN anywhere is inf."""
    err = np.asarray(err, np.float64); bound = np.asarray(bound, np.float64)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.inf) if np.isnan(r).any() else float(r.max())


def padding_positions(rows, cols, ld, off):
    """One padding element of each kind an output image has: the first element if the operand starts later, the end of the
    first and of the last row if the rows are padded."""
    pos = [0] if off > 0 else []
    if ld > cols and rows > 0:
        pos += [off + cols, off + rows * ld - 1]
    return pos


def case_id(case):
    """pytest id of a case tuple."""
    return "-".join(_name(c) if isinstance(c, type) else "x".join(map(str, c)) if isinstance(c, tuple) else str(c) for c in case)


class Rejected(AssertionError):
    pass


def _require(ok, what):
    if not ok:
        raise Rejected(what)


# ---- GEMM ------------------------------------------------------------------------------------------------------------------

GEMM_SHAPES_BOTH = [(1, 1, 1), (5, 7, 3), (3, 4, 0), (128, 128, 32), (129, 127, 33), (130, 257, 47), (257, 130, 81),
                    (50, 7, 4095), (50, 7, 4096), (50, 7, 4100), (130, 200, 5000), (64, 128, 10677)]
GEMM_ONE_STEP = {np.float64: (300, 50, 16), np.float32: (300, 50, 32)}
GEMM_LAYOUT_SHAPES = [(129, 127, 33), (128, 128, 32), (50, 7, 4100)]
GEMM_LAYOUTS = ["tight", "odd", "pad16", "offA1", "offB1", "offB3", "ldc5"]


def gemm_shapes(dtype):
    return GEMM_SHAPES_BOTH + [GEMM_ONE_STEP[np.dtype(dtype).type]]


def gemm_cases():
    """(dtype, transa, (M, N, K), layout) of every GEMM case."""
    out = []
    for dt in DTYPES:
        for ta in (0, 1):
            out += [(dt, ta, s, "tight") for s in gemm_shapes(dt)]
            out += [(dt, ta, s, l) for s in GEMM_LAYOUT_SHAPES for l in GEMM_LAYOUTS if l != "tight"]
    return out


def gemm_layout(layout, dtype, transa, M, N, K):
    """(lda, offA, ldb, offB, ldc, offC) of a named layout."""
    ca = M if transa else K
    lda, ldb, ldc, oa, ob, oc = max(ca, 1), N, N, 0, 0, 0
    if layout == "odd":
        lda, ldb, ldc = odd_ld(ca), odd_ld(N), odd_ld(N)
    elif layout == "pad16":
        lda, ldb, ldc = padded_ld(ca, dtype), padded_ld(N, dtype), padded_ld(N, dtype)
        oa = ob = oc = _vec(dtype)
    elif layout == "offA1":
        oa = 1
    elif layout == "offB1":
        ob = 1
    elif layout == "offB3":
        ob, ldb = 3, N + 3
    elif layout == "ldc5":
        ldc, oc = N + 5, 1
    else:
        assert layout == "tight"
    return lda, oa, ldb, ob, ldc, oc


@functools.lru_cache(maxsize=None)
def gemm_problem(dtype, M, N, K, data):
    """op(A) [M, K], B [K, N] in the dtype, s1, and (reference, bound) in the wide precision; shared by both TRANSA and all
    layouts of a shape.  exact: the bound is zero (bit equality)."""
    rng = _rng("gemm", _name(dtype), M, N, K, data)
    if data == "exact":
        A, B = _ints(rng, (M, K)), _ints(rng, (K, N))
        if N >= 2 and K >= 1:
            B[0, N - 1] = -B[0, N - 2]                    # (the last two columns differ at any K)
    else:
        A, B = rng.standard_normal((M, K)), rng.standard_normal((K, N))
    A, B = A.astype(dtype), B.astype(dtype)
    s1 = S1[data]
    W = _wide(dtype)
    ref = W(s1) * (A.astype(W) @ B.astype(W))
    if data == "exact":
        bound = np.zeros((M, N))
    else:
        bound = gamma(K + (K + 255) // 256 + 2, dtype) * abs(s1) * (np.abs(A.astype(np.float64)) @ np.abs(B.astype(np.float64)))
    for a in (A, B, ref, bound):
        a.setflags(write=False)
    return A, B, s1, ref, bound


def gemm_images(dtype, transa, shape, layout, data, A=None, B=None):
    """The three images of a case and the arguments of ops.dense_op besides them."""
    M, N, K = shape
    pa, pb = gemm_problem(dtype, M, N, K, data)[:2]
    A = pa if A is None else A
    B = pb if B is None else B
    lda, oa, ldb, ob, ldc, oc = gemm_layout(layout, dtype, transa, M, N, K)
    Ai = image(A.T if transa else A, lda, oa, np.nan, dtype)
    Bi = image(B, ldb, ob, np.nan, dtype)
    Ci = np.full(oc + M * ldc, SENTINEL, dtype)
    kw = dict(A_img=Ai, lda=lda, offA=oa, B_img=Bi, ldb=ldb, offB=ob, ldc=ldc, offC=oc, s1=S1[data])
    return Ci, kw


def check_matrix(got, ref, bound, what, tag, dtype, skip=None):
    """Asserts |got - ref| <= bound componentwise (a zero bound: equality); `skip`: a mask of elements left out.  Logs and
    returns the worst error / bound."""
    W = ref.dtype
    err = np.abs(got.astype(W) - ref)
    keep = np.ones(err.shape, bool) if skip is None else ~skip
    _require(bool(np.isfinite(got[keep]).all()), "%s: non-finite values" % what)
    r = _ratio(err[keep], bound[keep])
    _log(tag, r, _name(dtype))
    _require(r <= 1.0, "%s: error / bound = %.3g" % (what, r))
    return r


def check_gemm(dtype, transa, shape, layout, data, Ci):
    M, N, K = shape
    _, _, _, ref, bound = gemm_problem(dtype, M, N, K, data)
    ldc, oc = gemm_layout(layout, dtype, transa, M, N, K)[4:]
    got, pad_ok = split_image(Ci, M, N, ldc, oc)
    what = "gemm %s ta=%d %s %s %s" % (_name(dtype), transa, shape, layout, data)
    _require(pad_ok, what + ": padding of C overwritten")
    return check_matrix(got, ref, bound, what, "gemm-" + data, dtype)


def gemm_standin(A, B, s1, chunk=256, skip=(), twice=()):
    """NumPy in the dtype, chunks of 256 along K added in order (`skip` / `twice`: chunk numbers left out / added twice)."""
    acc = np.zeros((A.shape[0], B.shape[1]), A.dtype)
    for c, k0 in enumerate(range(0, A.shape[1], chunk)):
        if c in skip:
            continue
        p = A[:, k0:k0 + chunk] @ B[k0:k0 + chunk]
        acc += p
        if c in twice:
            acc += p
    return A.dtype.type(s1) * acc


def swap_row_maps(C):
    """Rows permuted inside every 16-row tile as if the accumulator row maps of the two precisions were exchanged: register r
    of lane group g is row g + 4 r in one and 4 g + r in the other (rows whose partner lies past the end stay)."""
    out = C.copy()
    M = C.shape[0]
    for i in range(M):
        t, g, r = i // 16, (i % 16) % 4, (i % 16) // 4          # i = 16 t + g + 4 r
        j = 16 * t + 4 * g + r
        if j < M and 16 * t + ((j % 16) % 4) * 4 + (j % 16) // 4 == i:
            out[i] = C[j]
    return out


@functools.lru_cache(maxsize=None)
def gemm_mutations(dtype, shape, data):
    """{name: mutated [M, N] result} of the stand-in kernel, those that apply to the shape."""
    M, N, K = shape
    A, B, s1 = gemm_problem(dtype, M, N, K, data)[:3]
    good = gemm_standin(A, B, s1)
    mut = {}
    if K >= 1:
        mut["last K dropped"] = gemm_standin(A[:, :K - 1], B[:K - 1], s1)
        nch = (K + 255) // 256
        mut["chunk omitted"] = gemm_standin(A, B, s1, skip=(nch - 1,))
        mut["chunk twice"] = gemm_standin(A, B, s1, twice=(nch // 2,))
        if M > 128 or M % 128:
            m0 = (M - 1) // 128 * 128
            c = good.copy(); c[m0:] = gemm_standin(A[m0:], B, 1.0)
            mut["alpha not on last row tile"] = c
        if dtype == np.float64:
            mut["accumulated in float32"] = gemm_standin(A.astype(np.float32), B.astype(np.float32), s1).astype(np.float64)
    if M >= 5 and K >= 1:
        mut["row maps exchanged"] = swap_row_maps(good)
    if N >= 2 and K >= 1:
        c = good.copy(); c[:, N - 1] = c[:, N - 2]
        mut["last column clamped"] = c
    return good, mut


# ---- Gramian ---------------------------------------------------------------------------------------------------------------

GRAM_K_MFMA = [1, 15, 16, 17, 33, 47, 48, 49, 50, 51, 52, 53, 63, 64]
GRAM_K_GEMM = [65, 100, 129]
GRAM_N = [0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1000, 6200, 8321]
GRAM_N_BIG = 70000
GRAM_LAYOUTS = ["tight", "k3", "pad16"]
GRAM_SCALES = [(1.0, 0.0), (0.5, 3.0)]


def gram_pairs():
    """(n, k): every k with n in {5, 129, 1000}, every n with k in {50, 64, 17}, n = 70 000 at k = 50 and 64.  n = 6200 and 8321
    give 49 and 66 partial blocks: the reduce stage's unrolled loop entered by its first thread only, and by all of them."""
    p = [(n, k) for k in GRAM_K_MFMA + GRAM_K_GEMM for n in (5, 129, 1000)]
    p += [(n, k) for n in GRAM_N for k in (50, 64, 17) if (n, k) not in p]
    return p + [(GRAM_N_BIG, 50), (GRAM_N_BIG, 64)]


def gram_cases():
    """(dtype, n, k, layout, (s1, s2)).  The layouts and the second scale pair go with a subset: the widths around the REM
    columns and the tile edge, at a row count with more than one block."""
    out = []
    for dt in DTYPES:
        for (n, k) in gram_pairs():
            out.append((dt, n, k, "tight", GRAM_SCALES[1]))
        for k in (17, 50, 52, 64, 65):
            for lay in GRAM_LAYOUTS[1:]:
                out.append((dt, 129, k, lay, GRAM_SCALES[1]))
            out.append((dt, 129, k, "tight", GRAM_SCALES[0]))
        out.append((dt, 0, 50, "k3", GRAM_SCALES[0]))
    return out


def gram_blocks(n, num_cus=256):
    """(blocks, rows per block) of launch_gram's first stage (launch_dense.hip)."""
    nb = max(1, min(2 * num_cus, (n + 127) // 128))
    rpb = max(1, (n + nb - 1) // nb)
    return max(1, (n + rpb - 1) // rpb), rpb


def gram_layout(layout, dtype, k):
    """(ldb, offB, offC); the output itself is tight (launch_gram takes no leading dimension for it)."""
    if layout == "k3":
        return k + 3, 3, 1
    if layout == "pad16":
        return padded_ld(k, dtype), _vec(dtype), _vec(dtype)
    return k, 0, 0


@functools.lru_cache(maxsize=None)
def gram_input(dtype, n, k, data):
    rng = _rng("gram", _name(dtype), n, k, data)
    B = (_ints(rng, (n, k)) if data == "exact" else rng.standard_normal((n, k))).astype(dtype)
    if data == "exact" and n >= 1 and k >= 50:
        B[0, 49] = -B[0, 48]                              # (columns 48 and 49 differ at any n)
    B.setflags(write=False)
    return B


GRAM_CHUNKED_FROM = 16384            # rows from which the float64 reference adds float64 products of 32 rows in longdouble


@functools.lru_cache(maxsize=None)
def _gram_products(dtype, n, k, data):
    """(B^T B in the wide precision, |B|^T |B|, the reference's own error bound or None).  Float64 inputs of at least
    GRAM_CHUNKED_FROM rows: the products of 32 rows each in float64, their sum in longdouble (all in longdouble takes 8 s at
    70 000 x 64); that reference is within gamma_32 |B|^T |B| of the truth, 0.05 % of the kernel's bound at 70 000 rows, and the
    check adds it to the bound.  (On the integer data those products are exact.)"""
    B = gram_input(dtype, n, k, data)
    W = _wide(dtype)
    aB = np.abs(B.astype(np.float64))
    absG = aB.T @ aB
    if dtype == np.float64 and n >= GRAM_CHUNKED_FROM:
        full = n // 32 * 32
        blocks = B[:full].reshape(-1, 32, k)
        G = np.matmul(blocks.transpose(0, 2, 1), blocks).sum(axis=0, dtype=W) + (B[full:].T @ B[full:]).astype(W)
        return G, absG, gamma(32, dtype) * absG
    Bw = B.astype(W)
    return np.ascontiguousarray(Bw.T) @ Bw, absG, None


def gram_scales(data, scales):
    """(s1, s2) of a data set: the pair as it is (a power of two, an integer), except that the normal data take s1 = 2.5 with
    the shift."""
    s1, s2 = scales
    if data == "normal" and s2 != 0:
        s1 = S1["normal"]
    return s1, s2


def gram_problem(dtype, n, k, data, scales):
    s1, s2 = gram_scales(data, scales)
    G, absG, ref_err = _gram_products(dtype, n, k, data)
    W = _wide(dtype)
    ref = W(s1) * G + W(s2) * np.eye(k, dtype=W)
    if data == "exact":
        bound = np.zeros((k, k))
    else:
        bound = gamma(n + (n + 255) // 256 + 2, dtype) * abs(s1) * absG
        if ref_err is not None:
            bound = bound + abs(s1) * ref_err
        if s2 != 0:
            bound = bound + np.diag(np.spacing(np.abs(np.diag(ref)).astype(dtype)).astype(np.float64))
    return gram_input(dtype, n, k, data), s1, s2, ref, bound


def gram_images(dtype, n, k, layout, data, scales):
    B, s1, s2 = gram_problem(dtype, n, k, data, scales)[:3]
    ldb, ob, oc = gram_layout(layout, dtype, k)
    Bi = image(B, ldb, ob, np.nan, dtype)
    Ci = np.full(oc + k * k, SENTINEL, dtype)
    return Ci, dict(B_img=Bi, ldb=ldb, offB=ob, ldc=k, offC=oc, s1=s1, s2=s2)


def check_gram(dtype, n, k, layout, data, scales, Ci):
    _, _, _, ref, bound = gram_problem(dtype, n, k, data, scales)
    oc = gram_layout(layout, dtype, k)[2]
    got, pad_ok = split_image(Ci, k, k, k, oc)
    what = "gram %s n=%d k=%d %s %s %s" % (_name(dtype), n, k, layout, data, scales)
    _require(pad_ok, what + ": elements before C overwritten")
    r = check_matrix(got, ref, bound, what, "gram-" + data, dtype)
    if k <= 64:
        _require(bool(np.array_equal(_bits(got), _bits(np.ascontiguousarray(got.T)))), what + ": the two triangles differ in bits")
    return r


def gram_standin(B, s1, s2, rows=None, skip=(), twice=()):
    """NumPy in the dtype: chunks of 256 rows in order, the upper triangle mirrored (as the reduce stage writes it)."""
    B = B if rows is None else B[:rows]
    acc = gemm_standin(np.ascontiguousarray(B.T), B, 1.0, skip=skip, twice=twice)
    acc = np.triu(acc) + np.triu(acc, 1).T
    T = B.dtype.type
    out = T(s1) * acc
    out[np.diag_indices_from(out)] += T(s2)
    return out


@functools.lru_cache(maxsize=None)
def gram_mutations(dtype, n, k, data, scales):
    B, s1, s2 = gram_problem(dtype, n, k, data, scales)[:3]
    good = gram_standin(B, s1, s2)
    mut = {}
    if n >= 1:
        mut["last row dropped"] = gram_standin(B, s1, s2, rows=n - 1)
        nch = (n + 255) // 256
        mut["chunk omitted"] = gram_standin(B, s1, s2, skip=(nch - 1,))
        mut["chunk twice"] = gram_standin(B, s1, s2, twice=(nch // 2,))
        nb, rpb = gram_blocks(n)
        mut["last partial block missing"] = gram_standin(B, s1, s2, rows=(nb - 1) * rpb)
        if dtype == np.float64:
            mut["accumulated in float32"] = gram_standin(B.astype(np.float32), s1, s2).astype(np.float64)
        if k >= 50:
            perm = np.arange(k); perm[[48, 49]] = [49, 48]
            mut["columns 48 and 49 exchanged"] = np.ascontiguousarray(good[perm][:, perm])
    if s2 != 0:
        c = good.copy(); c[k - 1, k - 1] -= np.dtype(dtype).type(s2)
        mut["shift missing on last diagonal"] = c
    if k >= 2:
        c = good.copy(); c[np.tril_indices(k, -1)] = np.dtype(dtype).type(SENTINEL)
        mut["lower triangle stale"] = c
    return good, mut


# ---- potrf -----------------------------------------------------------------------------------------------------------------

POTRF_N = [1, 2, 3, 16, 17, 64, 65, 130, 257, 320]
POTRF_DATA = ["exact", "cond10", "cond1e4"]


def potrf_cases():
    return [(dt, n, d, off) for dt in DTYPES for n in POTRF_N for d in POTRF_DATA for off in ((0, 1) if n in (3, 65) else (0,))]


def _gram_plus_ridge(rng, n, cond):
    """X^T X / rows + ridge I in float64 with cond_2 = cond (n >= 2): X normal with graded columns in a rotated basis, the
    ridge chosen from the eigenvalues."""
    if n == 1:
        return np.array([[1.0 + rng.random()]])
    rows = 3 * n + 8
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    X = (rng.standard_normal((rows, n)) * 10.0 ** np.linspace(0.0, -3.0 if cond > 100 else -1.0, n)) @ V.T
    G = X.T @ X / rows
    lam = np.linalg.eigvalsh(G)
    ridge = (lam[-1] - cond * lam[0]) / (cond - 1.0)
    assert ridge > 0
    return G + ridge * np.eye(n)


@functools.lru_cache(maxsize=None)
def potrf_problem(dtype, n, data):
    """(M in the dtype (symmetric), the exact factor or None)."""
    rng = _rng("potrf", _name(dtype), n, data)
    if data == "exact":
        R = np.triu(_ints(rng, (n, n)), 1) + np.diag(rng.choice(np.array([2.0, 3.0]), size=n))
        M = R.T @ R
        assert np.abs(M).max() < 2 ** 24
        return M.astype(dtype), R.astype(dtype)
    M = _gram_plus_ridge(rng, n, 10.0 if data == "cond10" else 1e4).astype(dtype)
    return np.triu(M) + np.triu(M, 1).T, None


def potrf_image(dtype, n, data, off):
    """The upper triangle of M, SENTINEL below it and before it."""
    M = potrf_problem(dtype, n, data)[0]
    full = np.where(np.arange(n)[:, None] <= np.arange(n)[None, :], M, np.dtype(dtype).type(SENTINEL)).astype(dtype)
    return image(full, n, off, SENTINEL, dtype), dict(ldc=n, offC=off)


def check_potrf(dtype, n, data, off, Ci):
    M, R = potrf_problem(dtype, n, data)
    got, pad_ok = split_image(Ci, n, n, n, off)
    what = "potrf %s n=%d %s off=%d" % (_name(dtype), n, data, off)
    _require(pad_ok, what + ": elements before the matrix overwritten")
    low = np.tril_indices(n, -1)
    want = _bits(np.array([SENTINEL], dtype))[0]
    _require(bool(np.all(_bits(np.ascontiguousarray(got[low])) == want)), what + ": strict lower triangle touched")
    Rh = np.triu(got)
    _require(bool(np.isfinite(Rh).all()), what + ": non-finite factor")
    if data == "exact":
        r = _ratio(np.abs(Rh.astype(np.float64) - R.astype(np.float64)), np.zeros((n, n)))
    else:
        W = _wide(dtype)
        Rw = Rh.astype(W)
        err = np.abs(M.astype(W) - np.ascontiguousarray(Rw.T) @ Rw)
        aR = np.abs(Rh.astype(np.float64))
        r = _ratio(err, gamma(n + 1, dtype) * (aR.T @ aR))
    _log("potrf-" + data, r, _name(dtype))
    _require(r <= 1.0, "%s: error / bound = %.3g" % (what, r))
    return r


@functools.lru_cache(maxsize=None)
def potrf_standin(dtype, n, data):
    """np.linalg.cholesky in the dtype; [n, n] with SENTINEL below the diagonal."""
    M = potrf_problem(dtype, n, data)[0]
    R = np.ascontiguousarray(np.linalg.cholesky(M).T).astype(dtype)
    R[np.tril_indices(n, -1)] = np.dtype(dtype).type(SENTINEL)
    return R


@functools.lru_cache(maxsize=None)
def potrf_mutations(dtype, n, data):
    good = potrf_standin(dtype, n, data)
    mut = {}
    if n >= 2:
        c = good.copy(); c[n - 1, 0] = np.nextafter(c[n - 1, 0], np.dtype(dtype).type(0))
        mut["strict-lower element modified"] = c
        c = good.copy(); c[:n - 1, n - 1] *= np.diag(good)[:n - 1]
        mut["last column not divided by its pivot"] = c
    return good, mut


# ---- trtri -----------------------------------------------------------------------------------------------------------------

TRTRI_N = {np.float64: [1, 2, 54, 55, 77, 78, 257, 320], np.float32: [1, 2, 77, 78, 110, 111, 257, 320]}


def trtri_lds_bytes(n, dtype):
    return 2 * n * (n + 1) * np.dtype(dtype).itemsize


def trtri_cases():
    return [(dt, n, off) for dt in DTYPES for n in TRTRI_N[dt] for off in ((0, 1) if n in (2, 78) else (0,))]


@functools.lru_cache(maxsize=None)
def trtri_problem(dtype, n):
    """The float64 Cholesky factor of X^T X / rows + I (condition below 10), rounded to the dtype; NaN below the diagonal (the
    kernel reads the upper triangle only)."""
    rng = _rng("trtri", _name(dtype), n)
    X = rng.standard_normal((2 * n + 4, n))
    R = np.linalg.cholesky(X.T @ X / (2 * n + 4) + np.eye(n)).T.astype(dtype)
    R[np.tril_indices(n, -1)] = np.nan
    R.setflags(write=False)
    return R


def trtri_images(dtype, n, off):
    R = trtri_problem(dtype, n)
    Ai = image(R, n, off, np.nan, dtype)
    Ci = np.full(off + n * n, SENTINEL, dtype)
    return Ci, dict(A_img=Ai, lda=n, offA=off, ldc=n, offC=off)


def check_trtri(dtype, n, off, Ci):
    R = np.triu(np.nan_to_num(trtri_problem(dtype, n)))
    got, pad_ok = split_image(Ci, n, n, n, off)
    what = "trtri %s n=%d off=%d" % (_name(dtype), n, off)
    _require(pad_ok, what + ": elements before Linv overwritten")
    _require(bool(np.isfinite(got).all()), what + ": non-finite values")
    _require(bool(np.all(got[np.triu_indices(n, 1)] == 0)), what + ": nonzero right of the diagonal")
    W = _wide(dtype)
    X = got.astype(W).T                                            # column j = x^ of R x = e_j
    err = np.abs(R.astype(W) @ X - np.eye(n, dtype=W))
    r = _ratio(err, gamma(n, dtype) * (np.abs(R.astype(np.float64)) @ np.abs(got.astype(np.float64)).T))
    _log("trtri", r, _name(dtype))
    _require(r <= 1.0, "%s: residual / bound = %.3g" % (what, r))
    return r


@functools.lru_cache(maxsize=None)
def trtri_standin(dtype, n):
    import scipy.linalg as sl
    R = np.triu(np.nan_to_num(trtri_problem(dtype, n)))
    X = sl.solve_triangular(R, np.eye(n, dtype=dtype), lower=False, check_finite=False).astype(dtype)
    return np.ascontiguousarray(np.triu(X).T)


@functools.lru_cache(maxsize=None)
def trtri_mutations(dtype, n):
    good = trtri_standin(dtype, n)
    mut = {}
    if n >= 2:
        c = good.copy(); c[0, n - 1] = np.finfo(dtype).tiny
        mut["element above the diagonal nonzero"] = c
        c = good.copy(); c[n - 1, :n - 1] = 0
        mut["last row unsolved"] = c
    return good, mut


# ---- potrs_rows ------------------------------------------------------------------------------------------------------------

POTRS_ROWS = [1, 127, 129, 300]
POTRS_LAYOUTS = ["tight", "k3"]
# The constant of the n cond_2(M) u term.  Emulation of the route in NumPy in the dtype (explicit inverse from a triangular
# inversion, the rows times it, float32: one refinement step) against the same-precision LAPACK solve, all widths, 300 rows,
# cond_2(M) = 1e4.  Worst e / (4 e_o + c n cond u): c = 1: 1.48 (float64) / 0.44 (float32), c = 2: 0.78 / 0.34, c = 4: 0.40 /
# 0.23, all at k = 1, where n cond u = u and the route's three roundings meet a LAPACK solve that is exact on some rows.  4 is
# the smallest power of two with a factor 2 to spare (tests/test_dense_bound_sensitivity.py asserts it).  The emulation's worst eta is 0.31 ETA_SHARED (float32, k = 320).
POTRS_C = 4.0


def potrs_cases():
    return [(dt, k, rows, lay) for dt in DTYPES for k in TRTRI_N[dt] for rows in POTRS_ROWS for lay in POTRS_LAYOUTS]


def _solve_wide(R, Bm, W):
    """Rows of Bm times (R^T R)^-1 by two substitutions in precision W (columns in order, all rows at once)."""
    k = R.shape[0]
    R = R.astype(W)
    Y = Bm.astype(W).copy()
    for j in range(k):                                               # y R = b:   y_j = (b_j - sum_{l<j} y_l R_lj) / R_jj
        Y[:, j] = (Y[:, j] - Y[:, :j] @ R[:j, j]) / R[j, j]
    for j in range(k - 1, -1, -1):                                   # x R^T = y: x_j = (y_j - sum_{l>j} x_l R_jl) / R_jj
        Y[:, j] = (Y[:, j] - Y[:, j + 1:] @ R[j, j + 1:]) / R[j, j]
    return Y


@functools.lru_cache(maxsize=None)
def potrs_problem(dtype, k):
    """R (the dtype-rounded float64 factor of a matrix of condition 1e4), right-hand sides [300, k], the matrix R^T R that is
    actually solved (float64), its condition, the wide solution, the row errors of the same-precision LAPACK solve."""
    import scipy.linalg as sl
    rng = _rng("potrs", _name(dtype), k)
    V, _ = np.linalg.qr(rng.standard_normal((k, k)))
    M = (V * 10.0 ** np.linspace(0.0, -4.0, k)) @ V.T if k > 1 else np.array([[1.5]])
    R = np.triu(np.linalg.cholesky((M + M.T) / 2).T).astype(dtype)
    Bm = rng.standard_normal((max(POTRS_ROWS), k)).astype(dtype)
    R64 = R.astype(np.float64)
    M64 = R64.T @ R64
    cond = float(np.linalg.cond(M64))
    x_ref = _solve_wide(R, Bm, _wide(dtype))
    xo = sl.cho_solve((R, False), Bm.T, check_finite=False).T.astype(dtype)
    e_o = _row_errors_wide(xo, x_ref) if dtype == np.float64 else row_errors(xo, x_ref)
    for a in (R, Bm, M64, x_ref, e_o):
        a.setflags(write=False)
    return R, Bm, M64, cond, x_ref, e_o


def _row_errors_wide(x, ref):
    """fp32_reference.row_errors in the precision of `ref` (float64 answers against a longdouble solution)."""
    W = ref.dtype
    scale = np.maximum(np.abs(ref).max(axis=1), W.type(1e-6) * np.abs(ref).max())
    return (np.abs(x.astype(W) - ref).max(axis=1) / scale).astype(np.float64)


def potrs_layout(layout, k):
    return (k + 3, 1) if layout == "k3" else (k, 0)


def potrs_images(dtype, k, rows, layout):
    R, Bm = potrs_problem(dtype, k)[:2]
    ldc, oc = potrs_layout(layout, k)
    Rimg = np.where(np.arange(k)[:, None] <= np.arange(k)[None, :], R, np.dtype(dtype).type(np.nan)).astype(dtype).ravel()
    Ci = image(Bm[:rows], ldc, oc, SENTINEL, dtype)
    return Ci, dict(A_img=Rimg, lda=k, offA=0, ldc=ldc, offC=oc)


def potrs_ratios(dtype, k, rows, x):
    """(worst e_h / (4 e_o + POTRS_C n cond u), worst eta / ETA_SHARED) of the first `rows` answers x [rows, k]."""
    R, Bm, M64, cond, x_ref, e_o = potrs_problem(dtype, k)
    e_h = _row_errors_wide(x, x_ref[:rows]) if dtype == np.float64 else row_errors(x, x_ref[:rows])
    e_o = e_o[:rows]
    fwd = float((e_h / (4.0 * e_o + POTRS_C * k * cond * unit_roundoff(dtype))).max())
    # backward error of fp32_reference.backward_errors for one matrix every row shares
    x64, b64 = x.astype(np.float64), Bm[:rows].astype(np.float64)
    res = np.linalg.norm(x64 @ M64 - b64, axis=1)
    den = np.linalg.norm(M64, 2) * np.linalg.norm(x64, axis=1) + np.linalg.norm(b64, axis=1)
    eta = float((res / den).max() / ETA_SHARED)
    return fwd, eta


def check_potrs(dtype, k, rows, layout, Ci):
    ldc, oc = potrs_layout(layout, k)
    got, pad_ok = split_image(Ci, rows, k, ldc, oc)
    what = "potrs_rows %s k=%d rows=%d %s" % (_name(dtype), k, rows, layout)
    _require(pad_ok, what + ": padding of the rows overwritten")
    _require(bool(np.isfinite(got).all()), what + ": non-finite values")
    fwd, eta = potrs_ratios(dtype, k, rows, got)
    _log("potrs-fwd", fwd, _name(dtype))
    _require(fwd <= 1.0, "%s: e_h / (4 e_o + %g n cond u) = %.3g" % (what, POTRS_C, fwd))
    if dtype == np.float32:
        _log("potrs-eta", eta, _name(dtype))
        _require(eta <= 1.0, "%s: eta / ETA_SHARED = %.3g" % (what, eta))
    return fwd, eta


@functools.lru_cache(maxsize=None)
def potrs_emulation(dtype, k, refine=None):
    """launch_potrs_rows in NumPy in the dtype: Linv = R^-T by a triangular solve, Minv = Linv^T Linv, the rows times it;
    float32 (or refine=True): one refinement step with M = R^T R."""
    import scipy.linalg as sl
    R, Bm = potrs_problem(dtype, k)[:2]
    Linv = np.ascontiguousarray(np.triu(sl.solve_triangular(R, np.eye(k, dtype=dtype), lower=False, check_finite=False)).T).astype(dtype)
    Minv = (Linv.T @ Linv).astype(dtype)
    x = (Bm @ Minv).astype(dtype)
    if (dtype == np.float32) if refine is None else refine:
        Mf = (R.T @ R).astype(dtype)
        x = (x + ((Bm - x @ Mf).astype(dtype) @ Minv)).astype(dtype)
    return x
