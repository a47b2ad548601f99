"""Ranking with the item side resident on the device: ``Ranker`` wraps the ``cmfrec_hip_ranker_*`` handle of
include/cmfrec_hip.h.  ``ops.topN_batch`` uploads the item factors on every call; a ``Ranker`` uploads them once and
ranks any number of user batches against them."""
import ctypes as C

import numpy as np

from . import _lib
from .ops import _heldout_lists, _is_csr, _similar_args, _sorted_exclude, _sorted_include, after_cursor


def check_rankset(users, heldout, exclude):
    """The arrays of a ``RankSet``, checked without a device: (users int32 [nu], held_p uint64, held_i int32, excl_p, excl_i) --
    ``heldout`` / ``exclude`` as ``Ranker.ranks`` takes them, over the users of the set; the exclusion lists come out sorted."""
    users = np.atleast_1d(np.asarray(users))
    if users.ndim != 1 or (len(users) and not np.issubdtype(users.dtype, np.integer)):
        raise ValueError("RankSet: users must be a 1-D array of integer ids")
    if len(users) and (users.min() < 0 or users.max() > np.iinfo(np.int32).max):
        raise ValueError("RankSet: user ids must be >= 0 and fit 32 bits")
    users = np.ascontiguousarray(users, np.int32)
    nu = len(users)
    if _is_csr(heldout):
        heldout = (heldout.indptr, heldout.indices)
    hp, hi = _heldout_lists(heldout, nu, "RankSet")
    if exclude is not None and _is_csr(exclude):
        exclude = (exclude.indptr, exclude.indices)
    ep, ei = _sorted_exclude(exclude, nu)
    return users, hp, hi, ep, ei


class RankSet:
    """``RankSet(users, heldout, exclude=None, dtype=np.float64, device=-1)``: user ids, their held-out lists and (optionally) their
    exclusion lists -- (indptr, indices) CSR over the users OF THE SET or a SciPy CSR matrix of that many rows -- uploaded once and
    resident on the device (``cmfrec_hip_rankset_*``) for ``Ranker.metrics`` / ``AlsSession.ranking`` of the same dtype.  The
    caller owns the handle: ``close()`` it, or use it as a context manager."""

    def __init__(self, users, heldout, exclude=None, dtype=np.float64, device=-1):
        self.handle = None
        users, hp, hi, ep, ei = check_rankset(users, heldout, exclude)
        self.dtype = np.dtype(dtype)
        self.nu = len(users)
        self.indptr = hp.astype(np.int64)           # the normalised lists (sorted, de-duplicated) the ranks line up with
        self.items = hi
        self.lib = _lib.load(self.dtype)
        h = self.lib.cmfrec_hip_rankset_create(_lib.ptr(users), self.nu, _lib.ptr(hp), _lib.ptr(hi), _lib.ptr(ep), _lib.ptr(ei), int(device))
        if not h:
            _lib.check(self.lib.cmfrec_hip_last_error_code() or 4, self.lib, "RankSet")
        self.handle = C.c_void_p(h)

    def _for(self, dtype, what):
        if not getattr(self, "handle", None):
            raise RuntimeError("RankSet: the handle is closed")
        if np.dtype(dtype) != self.dtype:
            raise ValueError("%s: the ranking set is %s, the factors are %s" % (what, self.dtype, np.dtype(dtype)))
        return self.handle

    def close(self):
        if getattr(self, "handle", None):
            self.lib.cmfrec_hip_rankset_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def split_code(split, what="split"):
    """The C code of a ``split`` setting: None -> -1 (off), "auto" -> 0 (the planner chooses), an int >= 1 -> that many slices."""
    if split is None:
        return -1
    if isinstance(split, str):
        if split == "auto":
            return 0
        raise ValueError("%s must be None, \"auto\" or a number of slices >= 1, got %r" % (what, split))
    if isinstance(split, (bool, float)) or int(split) != split or int(split) < 1:
        raise ValueError("%s must be None, \"auto\" or a number of slices >= 1, got %r" % (what, split))
    return int(split)


def split_plan(nu, n, k, n_top, num_cus=256, dtype=np.float64, requested=0):
    """(slices, slice_items) of ``cmfrec_hip_topn_split_plan``: how a full ranking of ``nu`` users over ``n`` items would be cut
    on a device of ``num_cus`` compute units; ``requested`` = 0 to let the planner choose, >= 1 to ask for that many slices.
    Host arithmetic only: no device is needed."""
    lib = _lib.load(dtype)
    s, si = C.c_int(0), C.c_int(0)
    rc = lib.cmfrec_hip_topn_split_plan(int(nu), int(n), int(k), int(n_top), int(num_cus), C.c_size_t(np.dtype(dtype).itemsize),
                                        int(requested), C.byref(s), C.byref(si))
    _lib.check(rc, lib, "split_plan")
    return s.value, si.value


class Ranker:
    """``Ranker(B, biasB=None, device=-1, split=None)``: B [n, k] item factors (float64 or float32), ``biasB`` [n] of the same dtype
    or None.  ``topN(A, n=10, exclude=None, include=None)`` ranks the rows of A [nu, k] like ``ops.topN_batch``.  The caller owns
    the handle: ``close()`` it, or use it as a context manager.
    ``split``: None (the default, every call as it always was), ``"auto"`` or a number of slices: the full ranking of ``topN``
    (without ``include``) cuts the items into slices across the device and merges the slices' lists -- what makes a request of a
    few users use more than one compute unit.  With it on, every k is scored by the MFMA kernel: ids and scores are those of
    ``CMFREC_HIP_TOPN=wide`` bit for bit, whatever the number of slices; for k <= 64 they agree with the default kernel up to
    rounding.  ``include``, ``topN_deep`` / ``topN_after``, ``ranks``, ``metrics`` and ``similar`` ignore the setting."""

    def __init__(self, B, biasB=None, device=-1, split=None):
        self.handle = None
        code = split_code(split, "Ranker: split")
        B = np.asarray(B)
        if B.ndim != 2:
            raise ValueError("Ranker: B must be 2-D [items, factors], got %d-D" % B.ndim)
        if B.dtype.type not in (np.float64, np.float32):
            raise ValueError("Ranker: B must be float64 or float32, got %s" % B.dtype)
        if B.shape[0] < 1 or B.shape[1] < 1:
            raise ValueError("Ranker: B is empty")
        if biasB is not None:
            biasB = np.asarray(biasB)
            if biasB.dtype != B.dtype:
                raise ValueError("Ranker: biasB is %s, B is %s" % (biasB.dtype, B.dtype))
            if biasB.shape != (B.shape[0],):
                raise ValueError("Ranker: biasB must have one entry per item (%d), got shape %s" % (B.shape[0], biasB.shape))
            biasB = np.ascontiguousarray(biasB)
        B = np.ascontiguousarray(B)
        self.dtype = B.dtype
        self.n, self.k = B.shape
        self.lib = _lib.load(B.dtype)
        h = self.lib.cmfrec_hip_ranker_create(_lib.ptr(B), C.c_size_t(B.shape[1]), C.c_int(self.n), C.c_int(self.k),
                                              _lib.ptr(biasB), C.c_int(device))
        if not h:
            _lib.check(self.lib.cmfrec_hip_last_error_code() or 4, self.lib, "Ranker")
        self.handle = C.c_void_p(h)
        self._split = None
        if code != -1:
            self.split = split

    @property
    def split(self):
        """None, "auto" or the number of slices asked for (``cmfrec_hip_ranker_set_split``); assignable."""
        return self._split

    @split.setter
    def split(self, value):
        code = split_code(value, "Ranker: split")
        _lib.check(self.lib.cmfrec_hip_ranker_set_split(self._live(), C.c_int(code)), self.lib, "Ranker.split")
        self._split = value

    def slices(self):
        """Item slices of the most recent ranking launch: 1 when it was not split."""
        s = C.c_int(0)
        _lib.check(self.lib.cmfrec_hip_ranker_slices(self._live(), C.byref(s)), self.lib, "Ranker.slices")
        return s.value

    def _live(self):
        if not getattr(self, "handle", None):
            raise RuntimeError("Ranker: the handle is closed")
        return self.handle

    def topN(self, A, n=10, exclude=None, include=None):
        """(ids [nu, n] int32, scores [nu, n]) for every row of ``A``: score = A_u . B_i (+ biasB[i]), descending, ties by
        lower id, -1 / -inf where fewer than ``n`` items remain; ``exclude`` = (indptr, indices) CSR over the rows of A.
        ``include``: candidate lists -- (indptr, indices) CSR over the rows of A, a SciPy CSR matrix, or one 1-D array shared by
        every user: each user is ranked over its own list only (minus its exclusion list), with the result of the full ranking
        when every other item is excluded; only the listed rows of the items are read."""
        h = self._live()
        A = np.asarray(A)
        if A.ndim != 2 or A.shape[1] != self.k:
            raise ValueError("Ranker.topN: A must be [users, %d], got shape %s" % (self.k, A.shape))
        if A.dtype != self.dtype:
            raise ValueError("Ranker.topN: A is %s, the ranker's items are %s" % (A.dtype, self.dtype))
        A = np.ascontiguousarray(A)
        nu = A.shape[0]
        n = int(n)
        ids = np.empty((nu, n), np.int32); sc = np.empty((nu, n), self.dtype)
        ep, ei = _sorted_exclude(exclude, nu)
        if include is not None:
            cp, ci = _sorted_include(include, nu)
            rc = self.lib.cmfrec_hip_ranker_topN_candidates(h, _lib.ptr(A), C.c_size_t(self.k), C.c_int(nu), _lib.ptr(cp), _lib.ptr(ci),
                                                            _lib.ptr(ep), _lib.ptr(ei), C.c_int(n), _lib.ptr(ids), _lib.ptr(sc))
            _lib.check(rc, self.lib, "Ranker.topN")
            return ids, sc
        rc = self.lib.cmfrec_hip_ranker_topN(h, _lib.ptr(A), C.c_size_t(self.k), C.c_int(nu), _lib.ptr(ep), _lib.ptr(ei), C.c_int(n),
                                             _lib.ptr(ids), _lib.ptr(sc))
        _lib.check(rc, self.lib, "Ranker.topN")
        return ids, sc

    def _users(self, A, what):
        A = np.asarray(A)
        if A.ndim != 2 or A.shape[1] != self.k:
            raise ValueError("%s: A must be [users, %d], got shape %s" % (what, self.k, A.shape))
        if A.dtype != self.dtype:
            raise ValueError("%s: A is %s, the ranker's items are %s" % (what, A.dtype, self.dtype))
        return np.ascontiguousarray(A)

    def topN_deep(self, A, n, exclude=None):
        """(ids [nu, n] int32, scores [nu, n]) as ``topN`` for any ``1 <= n <= items``: the list is built on the device in pages
        of up to 512 positions, each page one pass of the MFMA kernel that admits only what lies strictly behind the previous
        page's last (score, id); the result does not depend on the page length.  Every k runs the MFMA kernel, so the scores
        have the bits of ``ranks`` (and of ``topN`` for k > 64 or under ``CMFREC_HIP_TOPN=wide``)."""
        h = self._live()
        A = self._users(A, "Ranker.topN_deep")
        nu = A.shape[0]
        n = int(n)
        if exclude is not None and _is_csr(exclude):
            exclude = (exclude.indptr, exclude.indices)
        ep, ei = _sorted_exclude(exclude, nu)
        ids = np.empty((nu, max(n, 0)), np.int32); sc = np.empty((nu, max(n, 0)), self.dtype)
        rc = self.lib.cmfrec_hip_ranker_topN_deep(h, _lib.ptr(A), C.c_size_t(self.k), C.c_int(nu), _lib.ptr(ep), _lib.ptr(ei), C.c_int(n),
                                                  _lib.ptr(ids), _lib.ptr(sc))
        _lib.check(rc, self.lib, "Ranker.topN_deep")
        return ids, sc

    def topN_after(self, A, after_ids, after_scores, n=10, exclude=None):
        """The next page: (ids [nu, n], scores [nu, n]), the ``n <= min(128, items)`` best items of every user strictly behind its
        cursor ``(after_scores[u], after_ids[u])`` in the order of ``topN`` -- typically the last column of the previous page,
        ``ids[:, -1]`` / ``scores[:, -1]``.  Both None: the first page.  A user whose previous page ended in -1 / -inf gets
        -1 / -inf throughout.  The cursor's item need not be rankable any more (it may be excluded now).  The cursor compares
        score bits: it must come from ``topN_after``, ``topN_deep``, ``ranks`` or the MFMA ``topN`` (k > 64, or
        ``CMFREC_HIP_TOPN=wide``); with a score of the default k <= 64 kernel a near tie may repeat or skip a neighbour."""
        h = self._live()
        A = self._users(A, "Ranker.topN_after")
        nu = A.shape[0]
        ai, asc = after_cursor(after_ids, after_scores, nu, self.dtype, "Ranker.topN_after")
        n = int(n)
        if exclude is not None and _is_csr(exclude):
            exclude = (exclude.indptr, exclude.indices)
        ep, ei = _sorted_exclude(exclude, nu)
        ids = np.empty((nu, max(n, 0)), np.int32); sc = np.empty((nu, max(n, 0)), self.dtype)
        rc = self.lib.cmfrec_hip_ranker_topN_after(h, _lib.ptr(A), C.c_size_t(self.k), C.c_int(nu), _lib.ptr(ep), _lib.ptr(ei), _lib.ptr(ai),
                                                   _lib.ptr(asc), C.c_int(n), _lib.ptr(ids), _lib.ptr(sc))
        _lib.check(rc, self.lib, "Ranker.topN_after")
        return ids, sc

    def pages(self):
        """(launches, page length) of the most recent ``topN_deep`` call."""
        p, l = C.c_int(0), C.c_int(0)
        _lib.check(self.lib.cmfrec_hip_ranker_pages(self._live(), C.byref(p), C.byref(l)), self.lib, "Ranker.pages")
        return p.value, l.value

    def ranks(self, A, heldout, exclude=None, return_scores=False):
        """(indptr, items, ranks, pool) for the rows of ``A`` and their held-out lists, as ``ops.ranks_batch``: ``ranks[j]`` is
        the 0-based place of ``items[j]`` in its user's full ranking (-1: outside the items, excluded, or a NaN score), ``pool``
        the number of items of each user's ranking.  Under ``CMFREC_HIP_TOPN=wide`` (and for every k > 64)
        ``topN(A, n, exclude)[0][u, rank] == item`` wherever ``rank < n``, with the same score bits; against the default top-N
        kernel of k <= 64 the two agree up to rounding.  ``return_scores``: a fifth value, the items' scores (NaN where the
        rank is -1)."""
        h = self._live()
        A = np.asarray(A)
        if A.ndim != 2 or A.shape[1] != self.k:
            raise ValueError("Ranker.ranks: A must be [users, %d], got shape %s" % (self.k, A.shape))
        if A.dtype != self.dtype:
            raise ValueError("Ranker.ranks: A is %s, the ranker's items are %s" % (A.dtype, self.dtype))
        A = np.ascontiguousarray(A)
        nu = A.shape[0]
        hp, hi = _heldout_lists(heldout, nu, "Ranker.ranks")
        if exclude is not None and _is_csr(exclude):
            exclude = (exclude.indptr, exclude.indices)
        ep, ei = _sorted_exclude(exclude, nu)
        ranks = np.empty(len(hi), np.int32); pool = np.empty(nu, np.int32)
        sc = np.empty(len(hi), self.dtype) if return_scores else None
        rc = self.lib.cmfrec_hip_ranker_ranks(h, _lib.ptr(A), C.c_size_t(self.k), C.c_int(nu), _lib.ptr(hp), _lib.ptr(hi), _lib.ptr(ep),
                                              _lib.ptr(ei), _lib.ptr(ranks), _lib.ptr(sc), _lib.ptr(pool))
        _lib.check(rc, self.lib, "Ranker.ranks")
        if return_scores:
            return hp.astype(np.int64), hi, ranks, pool, sc
        return hp.astype(np.int64), hi, ranks, pool

    def metrics(self, A, rankset, k=10, per_user=False, return_ranks=False):
        """The ranking metrics of a resident ``RankSet`` at cut-off ``k``, reduced on the device: ``A`` [m, k] holds the factors
        of ALL users, the set's user ids pick its rows.  Returns the record -- ``sum`` [8] and ``count`` [8] in the order of
        ``cmfrec_amd.metrics.METRICS`` and ``users``; ``metrics.mean_from_record`` turns it into the means.  ``per_user``: a second
        value, the eight values per user [users of the set, 8] (NaN where the user does not count); ``return_ranks``: one more,
        the ranks of the held-out entries as ``ranks`` returns them."""
        h = self._live()
        A = np.asarray(A)
        if A.ndim != 2 or A.shape[1] != self.k:
            raise ValueError("Ranker.metrics: A must be [users, %d], got shape %s" % (self.k, A.shape))
        if A.dtype != self.dtype:
            raise ValueError("Ranker.metrics: A is %s, the ranker's items are %s" % (A.dtype, self.dtype))
        if not isinstance(rankset, RankSet):
            raise TypeError("Ranker.metrics: a RankSet is required")
        if int(k) < 1:
            raise ValueError("Ranker.metrics: k must be at least 1")
        A = np.ascontiguousarray(A)
        rec = _lib.RankRecord()
        pu = np.empty((rankset.nu, 8), np.float64) if per_user else None
        rk = np.empty(int(rankset.indptr[-1]) if rankset.nu else 0, np.int32) if return_ranks else None
        rc = self.lib.cmfrec_hip_ranker_metrics(h, _lib.ptr(A), A.shape[1], A.shape[0], rankset._for(self.dtype, "Ranker.metrics"), int(k),
                                                C.byref(rec), _lib.ptr(pu), _lib.ptr(rk))
        _lib.check(rc, self.lib, "Ranker.metrics")
        out = (rec.as_dict(),) + ((pu,) if per_user else ()) + ((rk,) if return_ranks else ())
        return out[0] if len(out) == 1 else out

    def similar(self, ids, n=10, metric="cosine", exclude=None):
        """(ids [nq, n] int32, scores [nq, n]): the neighbours of the ranker's own rows ``ids`` among its rows, by ``metric`` =
        "cosine" (B_q . B_i / (|B_q| |B_i|)) or "dot" (B_q . B_i; the bias plays no part in either), descending, ties by lower
        id, the query itself left out, -1 / -inf where fewer than ``n`` rows remain.  Only the ids go to the device.  A zero row
        (or one with a NaN) has no cosine: it is nobody's neighbour and has none.  ``exclude``: (indptr, indices) CSR over the
        queries or a SciPy CSR matrix, further rows to skip per query."""
        q, code = _similar_args(ids, self.n, metric, "Ranker.similar")
        if exclude is not None and _is_csr(exclude):
            exclude = (exclude.indptr, exclude.indices)
        ep, ei = _sorted_exclude(exclude, len(q))
        h = self._live()
        n = int(n)
        out = np.empty((len(q), n), np.int32); sc = np.empty((len(q), n), self.dtype)
        rc = self.lib.cmfrec_hip_ranker_similar(h, _lib.ptr(q), C.c_int(len(q)), C.c_int(code), _lib.ptr(ep), _lib.ptr(ei), C.c_int(n),
                                                _lib.ptr(out), _lib.ptr(sc))
        _lib.check(rc, self.lib, "Ranker.similar")
        return out, sc

    def inverse_norms(self):
        """[n]: 1 / |B_i| of every row as the cosine scores use it (made on the device by the first call that needs it, resident
        from then on); NaN for a row whose sum of squares is zero, NaN or infinite."""
        rn = np.empty(self.n, self.dtype)
        _lib.check(self.lib.cmfrec_hip_ranker_inverse_norms(self._live(), _lib.ptr(rn)), self.lib, "Ranker.inverse_norms")
        return rn

    def kernel_ms(self):
        """HIP-event time (ms) of the ranking kernel of the most recent ``topN``, ``ranks`` or ``similar`` call (of ``ranks``: the
        whole rank kernel, its threshold and exclusion steps included; of ``similar``: without the norm kernel; of a split ``topN``:
        the slice pass and the merge)."""
        ms = C.c_double(0)
        _lib.check(self.lib.cmfrec_hip_ranker_kernel_ms(self._live(), C.byref(ms)), self.lib, "Ranker.kernel_ms")
        return ms.value

    def launch_shape(self):
        """(users per workgroup, workgroups) of that kernel launch: the items are streamed once per workgroup's users.  After a
        call with ``include``: (wavefronts per workgroup -- each holds one user at a time --, workgroups)."""
        u, g = C.c_int(0), C.c_int(0)
        _lib.check(self.lib.cmfrec_hip_ranker_launch_shape(self._live(), C.byref(u), C.byref(g)), self.lib, "Ranker.launch_shape")
        return u.value, g.value

    def close(self):
        if getattr(self, "handle", None):
            self.lib.cmfrec_hip_ranker_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
