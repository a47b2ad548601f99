"""Operator-level entry points (level 2 of include/cmfrec_hip.h): one factor update with host
buffers.  Argument names and meaning follow the reference's internal operators
(/root/reference/src/cmfrec.h:986-1027, :1646-1683)."""
import ctypes as C

import numpy as np

from . import _lib


def _prep(A, B):
    if A.dtype != B.dtype or A.dtype.type not in (np.float64, np.float32):
        raise TypeError("A and B must share dtype float64 or float32")
    if not (A.flags.c_contiguous and B.flags.c_contiguous):
        raise ValueError("A and B must be C-contiguous (row-major)")
    return _lib.load(A.dtype), _lib.real(A.dtype)


def _csr(csr, dtype):
    p, i, v = csr
    return (np.ascontiguousarray(p, np.uint64), np.ascontiguousarray(i, np.int32), np.ascontiguousarray(v, dtype))


def optimizeA_implicit(A, B, csr, lam, k=None, use_cg=True, precondition_cg=False, max_cg_steps=3,
                       return_BtB=False):
    """In-place iALS half-step of A[m,lda] given B[n,ldb] (reference optimizeA_implicit)."""
    lib, R = _prep(A, B)
    m, lda = A.shape
    n, ldb = B.shape
    k = min(lda, ldb) if k is None else k
    p, i, v = _csr(csr, A.dtype)
    BtB = np.zeros((k, k), A.dtype) if return_BtB else None
    rc = lib.cmfrec_hip_optimizeA_implicit(_lib.ptr(A), C.c_size_t(lda), _lib.ptr(B), C.c_size_t(ldb), C.c_int(m),
                                           C.c_int(n), C.c_int(k), _lib.ptr(p), _lib.ptr(i), _lib.ptr(v), R(lam),
                                           C.c_bool(use_cg), C.c_bool(precondition_cg), C.c_int(max_cg_steps),
                                           _lib.ptr(BtB))
    _lib.check(rc, lib, "optimizeA_implicit")
    return BtB


def optimizeA_explicit(A, B, csr, lam, lam_last=None, k=None, bias_sub=None, scale_lam=False,
                       scale_bias_const=False, use_cg=True, precondition_cg=False, max_cg_steps=3, weight=None, wsum=None):
    """In-place explicit half-step on sparse X (reference optimizeA, Case 4).  weight: observation weights in the entry
    order of ``csr``; wsum: the per-row lambda multipliers of scale_lam (default: every row's own sum of weights)."""
    lib, R = _prep(A, B)
    m, lda = A.shape
    n, ldb = B.shape
    k = min(lda, ldb) if k is None else k
    lam_last = lam if lam_last is None else lam_last
    p, i, v = _csr(csr, A.dtype)
    bs = None if bias_sub is None else np.ascontiguousarray(bias_sub, A.dtype)
    if weight is not None:
        w = np.ascontiguousarray(weight, A.dtype)
        ws = None if wsum is None else np.ascontiguousarray(wsum, A.dtype)
        assert len(w) == len(v) and (ws is None or len(ws) == m)
        rc = lib.cmfrec_hip_optimizeA_explicit_weighted(_lib.ptr(A), C.c_size_t(lda), _lib.ptr(B), C.c_size_t(ldb), C.c_int(m),
                                                        C.c_int(n), C.c_int(k), _lib.ptr(p), _lib.ptr(i), _lib.ptr(v), _lib.ptr(w),
                                                        _lib.ptr(ws), _lib.ptr(bs), R(lam), R(lam_last), C.c_bool(scale_lam),
                                                        C.c_bool(scale_bias_const), C.c_bool(use_cg), C.c_bool(precondition_cg),
                                                        C.c_int(max_cg_steps))
        _lib.check(rc, lib, "optimizeA_explicit_weighted")
        return
    rc = lib.cmfrec_hip_optimizeA_explicit(_lib.ptr(A), C.c_size_t(lda), _lib.ptr(B), C.c_size_t(ldb), C.c_int(m),
                                           C.c_int(n), C.c_int(k), _lib.ptr(p), _lib.ptr(i), _lib.ptr(v), _lib.ptr(bs),
                                           R(lam), R(lam_last), C.c_bool(scale_lam), C.c_bool(scale_bias_const),
                                           C.c_bool(use_cg), C.c_bool(precondition_cg), C.c_int(max_cg_steps))
    _lib.check(rc, lib, "optimizeA_explicit")


def optimizeA_dense_full(A, B, Xfull, lam, lam_last=None, k=None, do_B=False, scale_lam=False):
    """Dense full update A = X B (BtB + lam)^-1 (reference optimizeA, Case 1): the C / D step."""
    lib, R = _prep(A, B)
    m, lda = A.shape
    n, ldb = B.shape
    k = min(lda, ldb) if k is None else k
    lam_last = lam if lam_last is None else lam_last
    Xf = np.ascontiguousarray(Xfull, A.dtype)
    rc = lib.cmfrec_hip_optimizeA_dense_full(_lib.ptr(A), C.c_size_t(lda), _lib.ptr(B), C.c_size_t(ldb), C.c_int(m),
                                             C.c_int(n), C.c_int(k), _lib.ptr(Xf), C.c_size_t(Xf.shape[1]),
                                             C.c_bool(do_B), R(lam), R(lam_last), C.c_bool(scale_lam))
    _lib.check(rc, lib, "optimizeA_dense_full")


def optimizeA_collective(A, B, Cm, csr, U, lam, w_user=1.0, lam_last=None, k=None, k_main=0, k_user=0,
                         k_item=0, bias_sub=None, scale_lam=False, scale_lam_sideinfo=False, m_u=None):
    """Collective half-step with dense U, Cholesky (reference optimizeA_collective, general branch)."""
    lib, R = _prep(A, B)
    m, lda = A.shape
    n, ldb = B.shape
    pdim = Cm.shape[0]
    lam_last = lam if lam_last is None else lam_last
    m_u = U.shape[0] if m_u is None else m_u
    p, i, v = _csr(csr, A.dtype)
    Cc = np.ascontiguousarray(Cm, A.dtype)
    Uc = np.ascontiguousarray(U, A.dtype)
    bs = None if bias_sub is None else np.ascontiguousarray(bias_sub, A.dtype)
    rc = lib.cmfrec_hip_optimizeA_collective(
        _lib.ptr(A), C.c_size_t(lda), _lib.ptr(B), C.c_size_t(ldb), _lib.ptr(Cc), C.c_int(m), C.c_int(m_u),
        C.c_int(n), C.c_int(pdim), C.c_int(k), C.c_int(k_main), C.c_int(k_user), C.c_int(k_item), _lib.ptr(p),
        _lib.ptr(i), _lib.ptr(v), _lib.ptr(bs), _lib.ptr(Uc), R(lam), R(w_user), R(lam_last), C.c_bool(scale_lam),
        C.c_bool(scale_lam_sideinfo))
    _lib.check(rc, lib, "optimizeA_collective")


def optimizeA_collective_sparse(A, B, Cm, csr, U_csr, lam, w_user=1.0, lam_last=None, k=None, k_main=0, k_user=0, k_item=0,
                                bias_sub=None, scale_lam=False, scale_lam_sideinfo=False, implicit=False):
    """Collective half-step with SPARSE side information, Cholesky: ``U_csr`` = (indptr[m_u+1], indices, values) over the
    first m_u rows (reference optimizeA_collective / optimizeA_collective_implicit with U_csr, !NA_as_zero_U)."""
    lib, R = _prep(A, B)
    m, lda = A.shape
    n, ldb = B.shape
    lam_last = lam if lam_last is None else lam_last
    p, i, v = _csr(csr, A.dtype)
    up, ui, uv = _csr(U_csr, A.dtype)
    Cm = np.ascontiguousarray(Cm, A.dtype)
    bs = None if bias_sub is None else np.ascontiguousarray(bias_sub, A.dtype)
    rc = lib.cmfrec_hip_optimizeA_collective_sparse(
        _lib.ptr(A), C.c_size_t(lda), _lib.ptr(B), C.c_size_t(ldb), _lib.ptr(Cm), C.c_int(m), C.c_int(len(up) - 1), C.c_int(n),
        C.c_int(Cm.shape[0]), C.c_int(k), C.c_int(k_main), C.c_int(k_user), C.c_int(k_item), _lib.ptr(p), _lib.ptr(i), _lib.ptr(v),
        _lib.ptr(bs), _lib.ptr(up), _lib.ptr(ui), _lib.ptr(uv), R(lam), R(w_user), R(lam_last), C.c_bool(scale_lam),
        C.c_bool(scale_lam_sideinfo), C.c_bool(implicit))
    _lib.check(rc, lib, "optimizeA_collective_sparse")


def side_zeros_products(rows, p, row, col, val, colmeans=None, M=None, alpha=1.0, first=0, count=None, F=None, kc=None):
    """The two products of sparse side information whose absent entries are zeros, U~ = U_sparse - 1 colmeans^T ([rows, p], COO
    triplets, duplicates add up), as the session takes them: returns (UM, UtF) with
    UM [count, kc] = alpha (U~ M)[first : first + count] for M [p, kc], and UtF [p, kc] = U~^T F[:, :kc] for F [rows, ldF]
    (each None when its input is).  ``kc`` defaults to the columns of M, else of F.  Bitwise reproducible."""
    given = M if M is not None else F
    if given is None:
        raise ValueError("pass M, F or both")
    dtype = np.asarray(given).dtype
    if dtype.type not in (np.float64, np.float32):
        raise TypeError("M / F must be float64 or float32")
    lib, R = _lib.load(dtype), _lib.real(dtype)
    r = np.ascontiguousarray(row, np.int32); c = np.ascontiguousarray(col, np.int32); v = np.ascontiguousarray(val, dtype)
    if not (len(r) == len(c) == len(v)):
        raise ValueError("row, col and val must have one entry per triplet")
    mu = None if colmeans is None else np.ascontiguousarray(colmeans, dtype)
    if mu is not None and len(mu) != p:
        raise ValueError("colmeans must have one entry per attribute")
    UM = UtF = None
    ldF = 0
    if M is not None:
        M = np.ascontiguousarray(M, dtype)
        if M.ndim != 2 or M.shape[0] != p:
            raise ValueError("M must be [p, kc]")
        kc = M.shape[1] if kc is None else kc
        if kc != M.shape[1]:
            raise ValueError("kc must be the columns of M")
        count = rows - first if count is None else count
        UM = np.empty((count, kc), dtype)
    if F is not None:
        F = np.ascontiguousarray(F, dtype)
        if F.ndim != 2 or F.shape[0] != rows:
            raise ValueError("F must be [rows, ldF]")
        ldF = F.shape[1]
        kc = ldF if kc is None else kc
        UtF = np.empty((p, kc), dtype)
    rc = lib.cmfrec_hip_side_zeros_products(C.c_int(rows), C.c_int(p), C.c_int(kc), _lib.ptr(r), _lib.ptr(c), _lib.ptr(v),
                                            C.c_size_t(len(v)), _lib.ptr(mu), _lib.ptr(M), R(alpha), C.c_int(first),
                                            C.c_int(0 if count is None else count), _lib.ptr(UM), _lib.ptr(F), C.c_size_t(ldF),
                                            _lib.ptr(UtF))
    _lib.check(rc, lib, "side_zeros_products")
    return UM, UtF


def _sorted_exclude(exclude, nu):
    """(indptr uint64, indices int32) of the per-user exclusion lists, each list ascending (the kernels binary-search it);
    (None, None) without lists."""
    if exclude is None:
        return None, None
    ep = np.ascontiguousarray(exclude[0], np.uint64)
    ei = np.ascontiguousarray(exclude[1], np.int32)
    if len(ep) != nu + 1:
        raise ValueError("exclude: indptr must have one entry per user plus one (%d), got %d" % (nu + 1, len(ep)))
    owner = np.repeat(np.arange(nu), np.diff(ep.astype(np.int64)))
    return ep, np.ascontiguousarray(ei[np.lexsort((ei, owner))])


def _sorted_include(include, nu):
    """(indptr uint64, indices int32) of the per-user candidate lists, each list ascending and free of duplicates (what the
    candidate kernel's tie rule asks for); (None, None) without lists.  ``include``: (indptr, indices) CSR over the ``nu`` users
    of the call, a SciPy CSR matrix, or one 1-D array of ids -- a single list shared by every user.  An id that does not fit
    int32 becomes -1 (the device skips every id outside the items).  No loop over the users."""
    if include is None:
        return None, None
    if hasattr(include, "indptr") and hasattr(include, "indices"):
        include = (include.indptr, include.indices)
    shared = not (isinstance(include, (tuple, list)) and len(include) == 2 and np.ndim(include[0]) == 1 and np.ndim(include[1]) == 1)
    ix = np.asarray(include if shared else include[1])
    if ix.ndim != 1:
        raise ValueError("include: (indptr, indices), a CSR matrix or one 1-D array of item ids, got a %d-D array" % ix.ndim)
    if ix.size and not np.issubdtype(ix.dtype, np.integer):
        raise ValueError("include: the item ids must be integers, got %s" % ix.dtype)
    if shared:
        ix = ix.astype(np.int64)
        ix[(ix < 0) | (ix > np.iinfo(np.int32).max)] = -1
        ix = np.unique(ix)
        ep = (np.arange(nu + 1, dtype=np.uint64) * np.uint64(len(ix))).astype(np.uint64)
        return ep, np.ascontiguousarray(np.tile(ix, nu), np.int32)
    ip = np.asarray(include[0])
    if len(ip) != nu + 1:
        raise ValueError("include: indptr must have one entry per user plus one (%d), got %d" % (nu + 1, len(ip)))
    if not (np.issubdtype(ip.dtype, np.integer) or np.all(ip == np.floor(ip))):
        raise ValueError("include: indptr must hold integers, got %s" % ip.dtype)
    ip = ip.astype(np.int64)
    lens = np.diff(ip)
    if ip[0] < 0 or (lens < 0).any():
        raise ValueError("include: indptr must not decrease")
    if ip[-1] != len(ix):
        raise ValueError("include: the last entry of indptr (%d) is not the number of indices (%d)" % (ip[-1], len(ix)))
    ix = ix[ip[0]:]
    if ix.dtype == np.int32:
        # what a retrieval stage usually hands over -- int32 ids, every list ascending and unique -- passes with one comparison
        # per entry and without a copy (a negative id stays: the device skips it)
        up = ix[1:] > ix[:-1]
        first = ip[1:-1][lens[1:] > 0] - ip[0]               # where the lists after the first begin
        up[first[(first > 0) & (first < len(ix))] - 1] = True
        if up.all():
            return (ip - ip[0]).astype(np.uint64), np.ascontiguousarray(ix)
    # one key per entry, (user, id + 1), sorted and de-duplicated in one go
    ix = ix.astype(np.int64)
    ix[(ix < 0) | (ix > np.iinfo(np.int32).max)] = -1
    key = np.unique((np.repeat(np.arange(nu, dtype=np.int64), lens) << 32) | (ix + 1))
    ep = np.zeros(nu + 1, np.uint64)
    ep[1:] = np.cumsum(np.bincount(key >> 32, minlength=nu))
    return ep, np.ascontiguousarray((key & 0xffffffff) - 1, np.int32)


def topN_batch(A, B, n_top=10, biasB=None, exclude=None, include=None):
    """Top-N item ids (and scores) for every row of ``A``: score = A_u . B_i (+ biasB[i]), descending, ties by lower
    id; ``exclude`` = (indptr, indices) CSR of items to skip per user (sorted here).  Batch counterpart of the
    reference's per-user ``topN`` (src/common.c:5127-5380).  Every width the library fits (k <= 272), n_top <= min(128, n).
    ``include``: candidate lists -- (indptr, indices) CSR over the rows of ``A``, a SciPy CSR matrix, or one 1-D array shared by
    every user (sorted and de-duplicated here): each user is ranked over its own list only, with the result the full ranking
    gives when every other item is excluded (the reference's ``include_ix``, batched); ``exclude`` may come along.
    B is uploaded on every call: to rank several batches against the same items, hold a ``cmfrec_amd.Ranker``."""
    A = np.ascontiguousarray(A); B = np.ascontiguousarray(B, A.dtype)
    lib, R = _prep(A, B)
    nu, lda = A.shape
    n, ldb = B.shape
    ids = np.empty((nu, n_top), np.int32); sc = np.empty((nu, n_top), A.dtype)
    bs = None if biasB is None else np.ascontiguousarray(biasB, A.dtype)
    ep, ei = _sorted_exclude(exclude, nu)
    if include is not None:
        cp, ci = _sorted_include(include, nu)
        rc = lib.cmfrec_hip_topN_candidates_batch(_lib.ptr(A), C.c_size_t(lda), C.c_int(nu), _lib.ptr(B), C.c_size_t(ldb), C.c_int(n),
                                                  C.c_int(lda), _lib.ptr(bs), _lib.ptr(cp), _lib.ptr(ci), _lib.ptr(ep), _lib.ptr(ei),
                                                  C.c_int(n_top), _lib.ptr(ids), _lib.ptr(sc))
        _lib.check(rc, lib, "topN_batch")
        return ids, sc
    rc = lib.cmfrec_hip_topN_batch(_lib.ptr(A), C.c_size_t(lda), C.c_int(nu), _lib.ptr(B), C.c_size_t(ldb), C.c_int(n),
                                   C.c_int(lda), _lib.ptr(bs), _lib.ptr(ep), _lib.ptr(ei), C.c_int(n_top), _lib.ptr(ids),
                                   _lib.ptr(sc))
    _lib.check(rc, lib, "topN_batch")
    return ids, sc


def topN_deep_batch(A, B, n_top, biasB=None, exclude=None):
    """``topN_batch`` without the limit of 128: (ids [nu, n_top] int32, scores [nu, n_top]) for any ``1 <= n_top <= items``,
    k <= 272, built on the device in pages (``Ranker.topN_deep``); every k runs the MFMA kernel.  B is uploaded on every call:
    to rank several batches against the same items, hold a ``cmfrec_amd.Ranker``."""
    A = np.ascontiguousarray(A); B = np.ascontiguousarray(B, A.dtype)
    lib, R = _prep(A, B)
    nu, lda = A.shape
    n, ldb = B.shape
    n_top = int(n_top)
    ids = np.empty((nu, max(n_top, 0)), np.int32); sc = np.empty((nu, max(n_top, 0)), A.dtype)
    bs = None if biasB is None else np.ascontiguousarray(biasB, A.dtype)
    if exclude is not None and _is_csr(exclude):
        exclude = (exclude.indptr, exclude.indices)
    ep, ei = _sorted_exclude(exclude, nu)
    rc = lib.cmfrec_hip_topN_deep_batch(_lib.ptr(A), C.c_size_t(lda), C.c_int(nu), _lib.ptr(B), C.c_size_t(ldb), C.c_int(n),
                                        C.c_int(lda), _lib.ptr(bs), _lib.ptr(ep), _lib.ptr(ei), C.c_int(n_top), _lib.ptr(ids),
                                        _lib.ptr(sc))
    _lib.check(rc, lib, "topN_deep_batch")
    return ids, sc


def after_cursor(after_ids, after_scores, nu, dtype, what):
    """(ids int32 [nu], scores [nu] of ``dtype``) of a next-page call, checked without a device; (None, None) for the first
    page.  One without the other, or anything but one entry per user, is a ValueError."""
    if after_ids is None and after_scores is None:
        return None, None
    if after_ids is None or after_scores is None:
        raise ValueError("%s: after_ids and after_scores come together (both None: the first page)" % what)
    ai = np.asarray(after_ids); asc = np.asarray(after_scores)
    if ai.shape != (nu,) or asc.shape != (nu,):
        raise ValueError("%s: after_ids and after_scores must have one entry per user (%d), got shapes %s and %s"
                         % (what, nu, ai.shape, asc.shape))
    if not np.issubdtype(ai.dtype, np.integer):
        raise ValueError("%s: after_ids must be integers, got %s" % (what, ai.dtype))
    if asc.dtype != np.dtype(dtype):
        raise ValueError("%s: after_scores is %s, the ranker's items are %s (a converted score is another cursor)"
                         % (what, asc.dtype, np.dtype(dtype)))
    return np.ascontiguousarray(ai, np.int32), np.ascontiguousarray(asc)


def _heldout_lists(heldout, nu, what):
    """The held-out lists of a rank call through ``_sorted_include`` (ascending, unique, ids outside int32 -> -1)."""
    if heldout is None:
        raise ValueError("%s: 'heldout' is required: (indptr, indices) CSR over the users or a SciPy CSR matrix" % what)
    if _is_csr(heldout):
        heldout = (heldout.indptr, heldout.indices)
    if not (isinstance(heldout, (tuple, list)) and len(heldout) == 2):
        raise ValueError("%s: 'heldout' must be (indptr, indices) or a SciPy CSR matrix" % what)
    return _sorted_include(heldout, nu)


def _is_csr(x):
    return hasattr(x, "indptr") and hasattr(x, "indices")


def ranks_batch(A, B, heldout, biasB=None, exclude=None):
    """(indptr, items, ranks, pool): for every row of ``A`` and every item of its held-out list, the 0-based place the item
    holds in the user's full ranking by score = A_u . B_i (+ biasB[i]) (descending, ties by lower id) -- the number of items
    that are not in the user's ``exclude`` list, do not score NaN and come before it.  ``heldout``: (indptr, indices) CSR over
    the rows of ``A`` or a SciPy CSR matrix, sorted and de-duplicated here; ``indptr`` / ``items`` are the normalised lists the
    ``ranks`` (int32) line up with.  A rank is -1 for an item outside the items, in the user's exclusion list, or with a NaN
    score.  ``pool`` [nu] int32: the items of each user's ranking.  ``cmfrec_amd.metrics.ranking_metrics`` turns these into
    hit / precision / recall / AP / NDCG at k, reciprocal rank, AUC and mean rank.  Every width the library fits (k <= 272).
    B is uploaded on every call: to rank several batches against the same items, hold a ``cmfrec_amd.Ranker``."""
    A = np.ascontiguousarray(A); B = np.ascontiguousarray(B, A.dtype)
    lib, R = _prep(A, B)
    nu, lda = A.shape
    n, ldb = B.shape
    hp, hi = _heldout_lists(heldout, nu, "ranks_batch")
    if exclude is not None and _is_csr(exclude):
        exclude = (exclude.indptr, exclude.indices)
    ep, ei = _sorted_exclude(exclude, nu)
    bs = None if biasB is None else np.ascontiguousarray(biasB, A.dtype)
    ranks = np.empty(len(hi), np.int32); pool = np.empty(nu, np.int32)
    rc = lib.cmfrec_hip_ranks_batch(_lib.ptr(A), C.c_size_t(lda), C.c_int(nu), _lib.ptr(B), C.c_size_t(ldb), C.c_int(n),
                                    C.c_int(lda), _lib.ptr(bs), _lib.ptr(hp), _lib.ptr(hi), _lib.ptr(ep), _lib.ptr(ei),
                                    _lib.ptr(ranks), None, _lib.ptr(pool))
    _lib.check(rc, lib, "ranks_batch")
    return hp.astype(np.int64), hi, ranks, pool


SIMILAR_METRICS = {"dot": 0, "cosine": 1}     # the `metric` of cmfrec_hip_ranker_similar


def _similar_args(ids, n_rows, metric, what):
    """(ids int32 [nq], metric code) of a neighbour call, checked without a device: the ids 1-D integers in [0, n_rows), the
    metric one of SIMILAR_METRICS."""
    if not isinstance(metric, str) or metric not in SIMILAR_METRICS:
        raise ValueError("%s: metric must be 'cosine' or 'dot', got %r" % (what, metric))
    ids = np.asarray(ids)
    if ids.ndim != 1:
        raise ValueError("%s: ids must be a 1-D array of row ids, got %d-D" % (what, ids.ndim))
    if len(ids) and not np.issubdtype(ids.dtype, np.integer):
        raise ValueError("%s: ids must be integers, got %s" % (what, ids.dtype))
    if len(ids) and (ids.min() < 0 or ids.max() >= n_rows):
        raise ValueError("%s: ids must be in [0, %d), got %d .. %d" % (what, n_rows, ids.min(), ids.max()))
    return np.ascontiguousarray(ids, np.int32), SIMILAR_METRICS[metric]


def similar_batch(B, ids, n_top=10, metric="cosine", exclude=None):
    """Neighbours of the rows ``ids`` of ``B`` [n, k] among the rows of ``B``: (ids [nq, n_top] int32, scores [nq, n_top]) by
    ``metric`` = "cosine" (B_q . B_i / (|B_q| |B_i|)) or "dot" (B_q . B_i), descending, ties by lower id, the query itself left
    out, -1 / -inf where fewer than ``n_top`` rows remain.  A zero row (or one with a NaN) has no cosine and is nobody's
    neighbour.  ``exclude``: (indptr, indices) CSR over the queries or a SciPy CSR matrix, further rows to skip per query.
    Every width the library fits (k <= 272), n_top <= min(128, n).  B is uploaded on every call: to ask several times, hold
    a ``cmfrec_amd.Ranker`` and call its ``similar``."""
    B = np.asarray(B)
    if B.ndim != 2 or B.dtype.type not in (np.float64, np.float32):
        raise ValueError("similar_batch: B must be a 2-D float64 or float32 array, got %d-D %s" % (B.ndim, B.dtype))
    q, code = _similar_args(ids, B.shape[0], metric, "similar_batch")
    if exclude is not None and _is_csr(exclude):
        exclude = (exclude.indptr, exclude.indices)
    ep, ei = _sorted_exclude(exclude, len(q))
    B = np.ascontiguousarray(B)
    lib = _lib.load(B.dtype)
    n, k = B.shape
    n_top = int(n_top)
    out = np.empty((len(q), n_top), np.int32); sc = np.empty((len(q), n_top), B.dtype)
    rc = lib.cmfrec_hip_similar_batch(_lib.ptr(B), C.c_size_t(k), C.c_int(n), C.c_int(k), _lib.ptr(q), C.c_int(len(q)), C.c_int(code),
                                      _lib.ptr(ep), _lib.ptr(ei), C.c_int(n_top), _lib.ptr(out), _lib.ptr(sc))
    _lib.check(rc, lib, "similar_batch")
    return out, sc


DENSE_OPS = {"gemm": 0, "gemm_ta": 1, "gram": 2, "potrf": 3, "trtri": 4, "potrs_rows": 5}


def impute_dense(m, n, kk, X_img, ldx, offX=0, A_img=None, lda=0, offA=0, B_img=None, ldb=0, offB=0, biasA=None, biasA_col=None,
                 biasB=None, glob_mean=0.0, row_missing=None):
    """The fill kernel of the imputation on its own (``cmfrec_hip_impute_dense``, include/cmfrec_hip.h): where the row-major
    ``X[m, ldx]`` holds NaN, ``A_r . B_c + glob_mean + biasA[r] + biasB[c]`` over ``kk`` factors; present entries keep their bits.
    The images are flat arrays of one dtype, ``off + rows * ld`` elements each, whose operand starts at element ``off``; ``X_img``
    is overwritten in place and returned.  The rows' bias: ``biasA`` [m], or ``biasA_col``, the column of ``A_img``'s rows that
    holds it (``kk <= biasA_col < lda``).  ``row_missing`` [m] int32: a row whose count is 0 is left alone."""
    dtype = X_img.dtype
    if dtype.type not in (np.float64, np.float32):
        raise TypeError("the images must be float64 or float32")
    for img in (A_img, B_img, X_img, biasA, biasB):
        if img is not None and (img.dtype != dtype or img.ndim != 1 or not img.flags.c_contiguous):
            raise ValueError("the images must be flat contiguous arrays of one dtype")
    for img, r, ld, off in ((A_img, m, lda, offA), (B_img, n, ldb, offB), (X_img, m, ldx, offX)):
        if img is not None and r > 0 and len(img) < off + r * ld:
            raise ValueError("an image is shorter than off + rows * ld")
    if (biasA is not None and len(biasA) < m) or (biasB is not None and len(biasB) < n):
        raise ValueError("a bias is shorter than its side")
    if biasA_col is not None and (biasA is not None or A_img is None or not kk <= biasA_col < lda):
        raise ValueError("'biasA_col' is a column of A_img's rows behind the factors, and excludes 'biasA'")
    if row_missing is not None:
        row_missing = np.ascontiguousarray(row_missing, np.int32)
        if len(row_missing) < m:
            raise ValueError("'row_missing' is shorter than the rows")
    lib, R = _lib.load(dtype), _lib.real(dtype)
    sz = dtype.itemsize
    at = lambda img, off: None if img is None else C.c_void_p(img.ctypes.data + off * sz)
    pba = at(A_img, offA + biasA_col) if biasA_col is not None else _lib.ptr(biasA)
    rc = lib.cmfrec_hip_impute_dense(C.c_int(m), C.c_int(n), C.c_int(kk), at(A_img, offA), C.c_size_t(lda), pba, at(B_img, offB),
                                     C.c_size_t(ldb), _lib.ptr(biasB), R(glob_mean), at(X_img, offX), C.c_size_t(ldx),
                                     _lib.ptr(row_missing))
    _lib.check(rc, lib, "impute_dense")
    return X_img


def score_pairs(m, n, kk, row, col, A_img=None, lda=0, offA=0, B_img=None, ldb=0, offB=0, biasA=None, biasA_col=None, biasB=None,
                glob_mean=0.0, implicit=False):
    """The scoring kernel of the chosen pairs on its own (``cmfrec_hip_score_pairs``, include/cmfrec_hip.h): per pair
    ``A[row] . B[col] + biasA[row] + biasB[col] + glob_mean`` over ``kk`` factors -- for a pair outside [0, m) x [0, n) ``glob_mean``
    + the bias of the side in range; ``implicit``: the dot product alone, NaN outside.  The images are flat arrays of one dtype,
    ``off + rows * ld`` elements each, whose operand starts at element ``off`` (aligned operands with even pitches are fetched
    16 bytes per lane, the others element by element: the same bits).  The rows' bias: ``biasA`` [m], or ``biasA_col``, the column
    of ``A_img``'s rows that holds it (``kk <= biasA_col < lda``)."""
    from .score import check_pairs
    imgs = [a for a in (A_img, B_img, biasA, biasB) if a is not None]
    if not imgs:
        raise ValueError("score_pairs needs at least one image")
    dtype = imgs[0].dtype
    if dtype.type not in (np.float64, np.float32):
        raise TypeError("the images must be float64 or float32")
    for img in imgs:
        if img.dtype != dtype or img.ndim != 1 or not img.flags.c_contiguous:
            raise ValueError("the images must be flat contiguous arrays of one dtype")
    for img, r, ld, off in ((A_img, m, lda, offA), (B_img, n, ldb, offB)):
        if img is not None and r > 0 and len(img) < off + r * ld:
            raise ValueError("an image is shorter than off + rows * ld")
    if (biasA is not None and len(biasA) < m) or (biasB is not None and len(biasB) < n):
        raise ValueError("a bias is shorter than its side")
    if biasA_col is not None and (biasA is not None or A_img is None or not kk <= biasA_col < lda):
        raise ValueError("'biasA_col' is a column of A_img's rows behind the factors, and excludes 'biasA'")
    row, col = check_pairs(row, col, "score_pairs")
    lib = _lib.load(dtype)
    sz = dtype.itemsize
    pba = C.c_void_p(A_img.ctypes.data + (offA + biasA_col) * sz) if biasA_col is not None else _lib.ptr(biasA)
    out = np.empty(len(row), dtype)
    rc = lib.cmfrec_hip_score_pairs(m, n, kk, _lib.ptr(A_img), lda, offA, pba, _lib.ptr(B_img), ldb, offB, _lib.ptr(biasB),
                                    float(glob_mean), int(bool(implicit)), _lib.ptr(row), _lib.ptr(col), len(row), _lib.ptr(out))
    _lib.check(rc, lib, "score_pairs")
    return out


def pair_errors(m, n, kk, row, col, x, w=None, A_img=None, lda=0, offA=0, B_img=None, ldb=0, offB=0, biasA=None, biasA_col=None,
                biasB=None, glob_mean=0.0, implicit=False, return_pred=True):
    """The two kernels of the error reduction on their own (``cmfrec_hip_pair_errors``, include/cmfrec_hip.h), beside
    ``score_pairs`` and with its image arguments: the error record of the pairs' predictions against ``x`` (NaN: the pair is
    skipped) under the optional weights ``w`` -- the dict ``Scorer.errors`` returns.  ``return_pred``: (record, pred), with
    ``pred`` the prediction of every pair as the kernel formed it (``score_pairs``' values, bit for bit)."""
    from .score import check_heldout
    imgs = [a for a in (A_img, B_img, biasA, biasB) if a is not None]
    if not imgs:
        raise ValueError("pair_errors needs at least one image")
    dtype = imgs[0].dtype
    if dtype.type not in (np.float64, np.float32):
        raise TypeError("the images must be float64 or float32")
    for img in imgs:
        if img.dtype != dtype or img.ndim != 1 or not img.flags.c_contiguous:
            raise ValueError("the images must be flat contiguous arrays of one dtype")
    for img, r, ld, off in ((A_img, m, lda, offA), (B_img, n, ldb, offB)):
        if img is not None and r > 0 and len(img) < off + r * ld:
            raise ValueError("an image is shorter than off + rows * ld")
    if (biasA is not None and len(biasA) < m) or (biasB is not None and len(biasB) < n):
        raise ValueError("a bias is shorter than its side")
    if biasA_col is not None and (biasA is not None or A_img is None or not kk <= biasA_col < lda):
        raise ValueError("'biasA_col' is a column of A_img's rows behind the factors, and excludes 'biasA'")
    row, col, x, w = check_heldout(row, col, x, w, dtype, "pair_errors")
    lib = _lib.load(dtype)
    sz = dtype.itemsize
    pba = C.c_void_p(A_img.ctypes.data + (offA + biasA_col) * sz) if biasA_col is not None else _lib.ptr(biasA)
    pred = np.empty(len(row), dtype) if return_pred else None
    rec = _lib.Errors()
    rc = lib.cmfrec_hip_pair_errors(m, n, kk, _lib.ptr(A_img), lda, offA, pba, _lib.ptr(B_img), ldb, offB, _lib.ptr(biasB),
                                    float(glob_mean), int(bool(implicit)), _lib.ptr(row), _lib.ptr(col), len(row), _lib.ptr(x),
                                    _lib.ptr(w), _lib.ptr(pred), C.byref(rec))
    _lib.check(rc, lib, "pair_errors")
    return (rec.as_dict(), pred) if return_pred else rec.as_dict()


def dense_op(op, m, n, k, C_img, ldc, offC=0, A_img=None, lda=0, offA=0, B_img=None, ldb=0, offB=0, s1=1.0, s2=0.0):
    """One operation of the dense layer on its own (``cmfrec_hip_dense_op``, include/cmfrec_hip.h): ``op`` a key of
    ``DENSE_OPS``.  The images are flat arrays of one dtype, ``off + rows * ld`` elements each, whose operand starts at
    element ``off``; ``C_img`` is uploaded whole, overwritten by the operation and returned in place."""
    dtype = C_img.dtype
    if dtype.type not in (np.float64, np.float32):
        raise TypeError("the images must be float64 or float32")
    for img in (A_img, B_img, C_img):
        if img is not None and (img.dtype != dtype or img.ndim != 1 or not img.flags.c_contiguous):
            raise ValueError("the images must be flat contiguous arrays of one dtype")
    rows = {0: (m, k, m), 1: (k, k, m), 2: (0, n, k), 3: (0, 0, n), 4: (n, 0, n), 5: (k, 0, m)}[DENSE_OPS[op]]
    for img, r, ld, off in ((A_img, rows[0], lda, offA), (B_img, rows[1], ldb, offB), (C_img, rows[2], ldc, offC)):
        if img is not None and r > 0 and len(img) < off + r * ld:
            raise ValueError("an image is shorter than off + rows * ld")
    lib, R = _lib.load(dtype), _lib.real(dtype)
    rc = lib.cmfrec_hip_dense_op(C.c_int(DENSE_OPS[op]), C.c_int(m), C.c_int(n), C.c_int(k), R(s1), R(s2),
                                 _lib.ptr(A_img), C.c_size_t(lda), C.c_int(offA), _lib.ptr(B_img), C.c_size_t(ldb), C.c_int(offB),
                                 _lib.ptr(C_img), C.c_size_t(ldc), C.c_int(offC))
    _lib.check(rc, lib, "dense_op")
    return C_img
