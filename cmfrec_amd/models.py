"""CMF / CMF_implicit estimators: the ``fit()`` surface of the reference's Python classes
(/root/reference/cmfrec/__init__.py:2881-2896 ``CMF.__init__``, :4673-4683 ``CMF_implicit.__init__``,
:938-1181 ``_fit_common``, :3150-3248 / :4882-4928 ``_fit``), driving the HIP library through
the reference's own C signatures (include/cmfrec_hip.h level 1).

Only the ALS path is offered (``method="als"``); options outside SURVEY.md section 8 raise
``NotImplementedError`` / ``ValueError`` instead of silently doing something else.
Inputs: ``X`` as a SciPy COO matrix (any sparse format is converted), or a ``(row, col, value)``
triplet plus ``shape``; dense side information ``U`` [m_u, p] / ``I`` [n_i, q] as NumPy arrays.
"""
import ctypes as C
import multiprocessing

import numpy as np

from . import _lib


def _coo_triplet(X, shape=None):
    if isinstance(X, tuple):
        row, col, val = X
        if shape is None:
            shape = (int(np.max(row)) + 1, int(np.max(col)) + 1)
    else:
        import scipy.sparse as sp
        if not sp.issparse(X):
            raise TypeError("'X' must be a SciPy sparse matrix or a (row, col, value) triplet")
        X = X.tocoo()
        row, col, val, shape = X.row, X.col, X.data, X.shape
    m, n = int(shape[0]), int(shape[1])
    if max(m, n) > np.iinfo(np.int32).max:      # reference guard, __init__.py:1146-1149
        raise ValueError("Error: dimensions of 'X' are too large for 32-bit indices.")
    return (np.ascontiguousarray(row, np.int32), np.ascontiguousarray(col, np.int32), val, m, n)


class _Base:
    def _setup(self, use_float, nthreads, n_jobs):
        self.use_float = bool(use_float)
        self.dtype_ = np.float32 if self.use_float else np.float64
        if n_jobs is not None:
            nthreads = n_jobs
        if nthreads is None or nthreads < 1:
            nthreads = multiprocessing.cpu_count()
        self.nthreads = int(nthreads)
        self.is_fitted_ = False

    def _lib(self):
        return _lib.load(self.dtype_), _lib.real(self.dtype_)

    def close(self):
        """Releases the resident handles the one-user methods (``topN``, ``topN_warm``, ...) keep on the model; the next such
        call makes new ones.  ``fit()`` calls it, and so does garbage collection."""
        from . import one_user
        one_user.release(self)


def _topN_inputs(self, users, exclude):
    """(user ids, their factors, their exclusion lists) of a ranking call on a fitted model."""
    users = np.atleast_1d(np.asarray(users, np.int64))
    A = np.ascontiguousarray(self.A_[users][:, self.k_user:])
    excl = None
    if exclude is not None:                       # scipy CSR / (indptr, indices) over ALL users: take the asked rows
        ip, ix = (exclude.indptr, exclude.indices) if hasattr(exclude, "indptr") else exclude
        ip = np.asarray(ip, np.int64); ix = np.asarray(ix)
        lens = ip[users + 1] - ip[users]
        ep = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        take = np.concatenate([np.arange(ip[u], ip[u + 1]) for u in users]) if lens.sum() else np.zeros(0, np.int64)
        excl = (ep, ix[take].astype(np.int32))
    return users, A, excl


def _topN(self, users, n, exclude, biasB, include=None):
    """Shared body of ``CMF.topN_batch`` / ``CMF_implicit.topN_batch``."""
    from . import ops
    _, A, excl = _topN_inputs(self, users, exclude)
    B = np.ascontiguousarray(self.B_[:, self.k_item:])
    if include is None:
        return ops.topN_batch(A, B, n_top=n, biasB=biasB, exclude=excl)
    return ops.topN_batch(A, B, n_top=n, biasB=biasB, exclude=excl, include=include)


def _topN_deep(self, users, n, exclude, biasB):
    """Shared body of ``CMF.topN_deep`` / ``CMF_implicit.topN_deep``."""
    from . import ops
    _, A, excl = _topN_inputs(self, users, exclude)
    B = np.ascontiguousarray(self.B_[:, self.k_item:])
    return ops.topN_deep_batch(A, B, n, biasB=biasB, exclude=excl)


_TOPN_DEEP_DOC = """``topN_batch`` without its limit of 128: (ids [len(users), n] int32, scores) for any ``1 <= n <= items``, built on the
        device in pages that each admit only what lies strictly behind the page before (``ops.topN_deep_batch``); ``users`` and
        ``exclude`` as in ``topN_batch``.  The scores are exactly what the ranker returns, A_u . B_i (+ the item bias): the global
        mean and the user bias ``topN_batch`` adds are left out (they do not change the order).  To ask for several batches, or
        for one page after another, hold ``ranker()`` and call its ``topN_deep`` / ``topN_after``."""


class ModelRanker:
    """What ``CMF.ranker()`` / ``CMF_implicit.ranker()`` return: the fitted model's item factors (and item bias) held on the
    device by a ``cmfrec_amd.Ranker``; ``topN(users, n, exclude, include)`` takes user ids of the fitted model and returns what the
    model's ``topN_batch`` returns.  The caller closes it (``close()`` or a ``with`` block); a refit needs a new one."""

    def __init__(self, model, biasB, split=None):
        from .rank import Ranker
        self._model = model
        self._ranker = Ranker(np.ascontiguousarray(model.B_[:, model.k_item:]),
                              None if biasB is None else np.ascontiguousarray(biasB, model.B_.dtype), split=split)

    def topN(self, users, n=10, exclude=None, include=None):
        users, A, excl = _topN_inputs(self._model, users, exclude)
        if include is None:
            ids, sc = self._ranker.topN(A, n=n, exclude=excl)
        else:
            ids, sc = self._ranker.topN(A, n=n, exclude=excl, include=include)
        return ids, self._model._finish_scores(users, sc)

    def topN_deep(self, users, n, exclude=None):
        """(ids, scores) for user ids of the fitted model and any ``1 <= n <= items`` (``Ranker.topN_deep``: pages chained on the
        device).  The scores are the ranker's own, A_u . B_i (+ item bias), exactly as it returns them -- without the global
        mean and the user bias ``topN`` adds, which do not change the order: their bits are what ``topN_after`` takes as a cursor."""
        _, A, excl = _topN_inputs(self._model, users, exclude)
        return self._ranker.topN_deep(A, n, exclude=excl)

    def topN_after(self, users, after_ids, after_scores, n=10, exclude=None):
        """The next ``n`` items of every user strictly behind its cursor (``Ranker.topN_after``), typically ``ids[:, -1]`` /
        ``scores[:, -1]`` of the previous ``topN_after`` / ``topN_deep`` call for the same users; both None: the first page.
        Scores as ``topN_deep`` returns them."""
        _, A, excl = _topN_inputs(self._model, users, exclude)
        return self._ranker.topN_after(A, after_ids, after_scores, n=n, exclude=excl)

    def pages(self):
        """(launches, page length) of the most recent ``topN_deep`` call."""
        return self._ranker.pages()

    def ranks(self, users, heldout, exclude=None):
        """(indptr, items, ranks, pool) as ``Ranker.ranks`` for user ids of the fitted model: ``heldout`` = (indptr, indices) CSR
        over the users OF THIS CALL (one list per entry of ``users``) or a SciPy CSR matrix of that many rows; ``exclude`` as in
        ``topN``, over all users of the model."""
        users, A, excl = _topN_inputs(self._model, users, exclude)
        return self._ranker.ranks(A, heldout, exclude=excl)

    def similar_items(self, items, n=10, metric="cosine", exclude=None):
        """(ids, scores) as ``Ranker.similar``: the neighbours of the model's items ``items`` among its items, from the resident
        ``B_[:, k_item:]``; the item bias plays no part.  ``exclude``: CSR over the queries, further items to skip."""
        return self._ranker.similar(items, n=n, metric=metric, exclude=exclude)

    def kernel_ms(self):
        return self._ranker.kernel_ms()

    def slices(self):
        """Item slices of the most recent ranking launch (``Ranker.slices``)."""
        return self._ranker.slices()

    def close(self):
        self._ranker.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _similar(factors, first, ids, n, metric, what):
    """Shared body of ``similar_items`` / ``similar_users``: a ranker over the scored columns of one factor matrix, made for the
    call."""
    from .ops import _similar_args
    from .rank import Ranker
    _similar_args(ids, factors.shape[0], metric, what)       # (refused before anything is uploaded)
    with Ranker(np.ascontiguousarray(factors[:, first:])) as r:
        return r.similar(ids, n=n, metric=metric)


_SIMILAR_ITEMS_DOC = """(ids [len(items), n] int32, scores): the items most like each of ``items`` by ``metric`` = "cosine" or "dot" over
        ``B_[:, k_item:]`` -- the columns the scores use; a bias plays no part --, descending, ties by lower id, the item itself
        left out (``Ranker.similar``).  A ranker made for the call: to ask several times, hold ``ranker()`` and call its
        ``similar_items``."""
_SIMILAR_USERS_DOC = """(ids [len(users), n] int32, scores): the users most like each of ``users`` by ``metric`` = "cosine" or "dot" over
        ``A_[:, k_user:]`` -- the columns the scores use --, descending, ties by lower id, the user itself left out
        (``Ranker.similar`` on a ranker over the user factors, made for the call)."""


def _ranks(self, users, heldout, exclude, biasB):
    """Shared body of ``CMF.ranks_batch`` / ``CMF_implicit.ranks_batch``."""
    from . import ops
    _, A, excl = _topN_inputs(self, users, exclude)
    B = np.ascontiguousarray(self.B_[:, self.k_item:])
    return ops.ranks_batch(A, B, heldout, biasB=biasB, exclude=excl)


def _csr_rows(M, users, m, what):
    """(indptr int64, indices) of the rows ``users`` of a CSR over all ``m`` users: a SciPy sparse matrix or (indptr, indices)."""
    if hasattr(M, "tocsr"):
        M = M.tocsr()
    ip, ix = (M.indptr, M.indices) if hasattr(M, "indptr") else M
    ip = np.asarray(ip, np.int64); ix = np.asarray(ix)
    if len(ip) != m + 1:
        raise ValueError("%s must have one row per user of the model (%d), got %d" % (what, m, len(ip) - 1))
    lens = ip[users + 1] - ip[users]
    out = np.zeros(len(users) + 1, np.int64)
    out[1:] = np.cumsum(lens)
    take = np.repeat(ip[users] - out[:-1], lens) + np.arange(out[-1])
    return out, ix[take]


def _evaluate_ranking(self, X_test, X_train, k, users, batch_users):
    """Shared body of ``evaluate_ranking``: the users with held-out items, in batches, through one ``ModelRanker``."""
    from .metrics import METRICS, ranking_metrics
    m = self.A_.shape[0]
    if hasattr(X_test, "tocsr"):
        X_test = X_test.tocsr()
    tp = np.asarray(X_test.indptr if hasattr(X_test, "indptr") else X_test[0], np.int64)
    if len(tp) != m + 1:
        raise ValueError("X_test must have one row per user of the model (%d), got %d" % (m, len(tp) - 1))
    todo = np.flatnonzero(np.diff(tp) > 0) if users is None else np.unique(np.atleast_1d(np.asarray(users, np.int64)))
    todo = todo[tp[todo + 1] > tp[todo]]
    batch_users = max(1, int(batch_users))
    sums = dict.fromkeys(METRICS, 0.); counts = dict.fromkeys(METRICS, 0)
    scored = 0
    if len(todo):
        with self.ranker() as rk:
            for s in range(0, len(todo), batch_users):
                ub = todo[s:s + batch_users]
                excl = None if X_train is None else _csr_rows(X_train, ub, m, "X_train")
                ip, _, ranks, pool = rk._ranker.ranks(np.ascontiguousarray(self.A_[ub][:, self.k_user:]),
                                                      _csr_rows(X_test, ub, m, "X_test"), exclude=excl)
                per = ranking_metrics(ip, ranks, pool, k=k)
                scored += int((per["T"] > 0).sum())
                for name in METRICS:
                    good = ~np.isnan(per[name])
                    sums[name] += float(per[name][good].sum()); counts[name] += int(good.sum())
    res = {name: (sums[name] / counts[name] if counts[name] else float("nan")) for name in METRICS}
    res["users"] = scored
    return res


_EVALUATE_DOC = """Ranking quality on held-out interactions, ranked on the device: ``X_test`` (SciPy sparse matrix or
        (indptr, indices) CSR over all users of the model) holds each user's held-out items; ``X_train`` (same forms, optional)
        the items to leave out of each user's ranking -- with None nothing is excluded.  The users that have held-out items
        (among ``users`` if given) go through one ``ranker()`` in batches of ``batch_users``; the ranks of their held-out items
        (``Ranker.ranks``) become ``cmfrec_amd.metrics.ranking_metrics`` at cut-off ``k``.  Returns a dict: the means over the
        users of hit, precision, recall, ap, ndcg (at k), rr, auc, mean_rank, and ``users``, the number of users scored (a user
        whose held-out items are all excluded or unrankable counts for nothing)."""


def _scorer(self, biasA, biasB, glob_mean, implicit):
    """A ``cmfrec_amd.Scorer`` over the fitted factors: the k_user / k_item columns are skipped by offset (row-strided views)."""
    from .score import Scorer
    dt = self.A_.dtype
    return Scorer(self.A_[:, self.k_user:], np.asarray(self.B_, dt)[:, self.k_item:],
                  None if biasA is None else np.ascontiguousarray(biasA, dt), None if biasB is None else np.ascontiguousarray(biasB, dt),
                  glob_mean=glob_mean, implicit=implicit)


def _evaluate_error(self, X_test, W, include_fallback):
    """Shared body of ``evaluate_error``: one ``scorer()`` and one ``EvalSet`` made for the call, the record reduced on the device."""
    from .metrics import error_metrics
    from .score import EvalSet
    if isinstance(X_test, tuple):
        row, col, val = X_test
    else:
        row, col, val, _, _ = _coo_triplet(X_test)
    with EvalSet(row, col, val, W, dtype=self.A_.dtype) as es, self.scorer() as sc:
        return error_metrics(sc.errors(es), include_fallback=include_fallback)


def _new_rows(X, n, dt):
    """COO triplet of new rows: ``X`` is a SciPy sparse matrix [m_x, n], a (row, col, val) triplet or None."""
    if X is None:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, dt), 0
    if isinstance(X, tuple):
        row, col, val = X
        row = np.asarray(row); col = np.asarray(col)
        if len(row) and (row.min() < 0 or col.min() < 0):
            raise ValueError("'X' has negative indices")
        if len(col) and col.max() >= n:
            raise ValueError("'X' has more columns than the model has items")
        m_x = int(np.max(row)) + 1 if len(row) else 0
    else:
        X = X.tocoo()
        if X.shape[1] > n:
            raise ValueError("'X' has more columns than the model has items")
        row, col, val, m_x = X.row, X.col, X.data, X.shape[0]
    return (np.ascontiguousarray(row, np.int32), np.ascontiguousarray(col, np.int32),
            np.ascontiguousarray(val, dt), int(m_x))


def _new_rows_weights(X, W, row, col, dt):
    """Observation weights of new rows in the form of ``X``: an array [m_x, n] for a dense ``X``; for a triplet an array (nnz,)
    or a triplet with the same (row, col); for a SciPy sparse ``X`` a sparse matrix with the same pattern.  Returns the
    weights in the order of ``X``'s entries."""
    if W is None:
        return None
    if isinstance(X, np.ndarray):
        W = np.ascontiguousarray(W, dt)
        if W.shape != X.shape:
            raise ValueError("'W' must have the shape of 'X'.")
        return W
    if isinstance(X, tuple):
        if isinstance(W, tuple):
            wr, wc, wv = W
            if len(wr) != len(row) or not (np.array_equal(wr, row) and np.array_equal(wc, col)):
                raise ValueError("'W' must have the same non-missing entries as 'X'.")
        else:
            wv = np.asarray(W).reshape(-1)
        if len(wv) != len(row):
            raise ValueError("'W' must have the same number of entries as 'X'.")
        return np.ascontiguousarray(wv, dt)
    if isinstance(W, (np.ndarray, tuple)) or not hasattr(W, "tocoo"):
        raise ValueError("'W' must be a sparse matrix like 'X'.")
    Wc = W.tocoo()
    if Wc.shape != X.shape or Wc.nnz != len(row):
        raise ValueError("'W' must have the same non-missing entries as 'X'.")
    ncol = int(X.shape[1])
    kx = row.astype(np.int64) * ncol + col
    kw = Wc.row.astype(np.int64) * ncol + Wc.col
    ox, ow = np.argsort(kx, kind="stable"), np.argsort(kw, kind="stable")
    if not np.array_equal(kx[ox], kw[ow]):
        raise ValueError("'W' must have the same non-missing entries as 'X'.")
    wv = np.empty(len(row), dt)
    wv[ox] = Wc.data[ow]
    return wv


def _new_rows_batch(self, X, U, W, dense_ok):
    """Input handling of a batch of new rows, shared by ``factors_multiple`` and the ``NewUsers`` handle: ``X`` a SciPy sparse matrix,
    a (row, col, val) triplet, a dense array with NaN (``dense_ok``: the explicit model) or None; ``W`` in the form of ``X``; ``U`` a
    dense array or a SciPy sparse matrix [m_u, p] (ignored by a model fitted without side information).  Returns a dict: row, col,
    val, m_x, Xfull, W, U (dense) or Usp (row, col, val, rows, cols), m_u, p."""
    if X is None and U is None:
        raise ValueError("Must pass at least one of 'X', 'U'.")
    if W is not None and X is None:
        raise ValueError("'W' needs 'X'.")
    dt = self.dtype_
    n = self.B_.shape[0]
    Xfull = None
    if isinstance(X, np.ndarray):
        if not dense_ok:
            raise ValueError("a dense 'X' belongs to the explicit model")
        if X.ndim != 2 or X.shape[1] != n:
            raise ValueError("a dense 'X' must be a 2-D array with one column per item of the model")
        Xfull = np.ascontiguousarray(X, dt)
        row = col = np.zeros(0, np.int32); val = np.zeros(0, dt); m_x = Xfull.shape[0]
    else:
        row, col, val, m_x = _new_rows(X, n, dt)
    Wv = _new_rows_weights(X, W, row, col, dt)
    Uc = Us = None
    m_u = p = 0
    if U is not None and self.C_.shape[0]:
        Uc, Us = _side_info(U, dt)
        if Uc is not None and Uc.ndim != 2:
            raise ValueError("'U' must be a 2-D array [rows, attributes]")
        m_u, p = Uc.shape if Uc is not None else (Us[3], Us[4])
        if p != self.C_.shape[0]:
            raise ValueError("'U' has %d columns, the model was fitted with %d attributes" % (p, self.C_.shape[0]))
    return dict(row=row, col=col, val=val, m_x=int(m_x), Xfull=Xfull, W=Wv, U=Uc, Usp=Us, m_u=int(m_u), p=int(p))


def _sparse_U_args(Us):
    """The positional sparse-U arguments of the two factors_collective_*_multiple calls (triplets; no CSR)."""
    if Us is None:
        return (None, None, None, C.c_size_t(0), None, None, None)
    return (_lib.ptr(Us[0]), _lib.ptr(Us[1]), _lib.ptr(Us[2]), C.c_size_t(len(Us[2])), None, None, None)


def _topN_new_batch(self, X, U, W, n, exclude_seen, exclude, include=None):
    with self.new_users() as nu:
        if include is None:
            return nu.topN(X=X, U=U, W=W, n=n, exclude_seen=exclude_seen, exclude=exclude)
        return nu.topN(X=X, U=U, W=W, n=n, exclude_seen=exclude_seen, exclude=exclude, include=include)


def _side_info(M, dt):
    """Side information for fit(): dense array -> (array, None); SciPy sparse matrix -> (None, (row, col, val, rows, cols))."""
    if M is None:
        return None, None
    if hasattr(M, "tocoo"):
        M = M.tocoo()
        return None, (np.ascontiguousarray(M.row, np.int32), np.ascontiguousarray(M.col, np.int32),
                      np.ascontiguousarray(M.data, dt), int(M.shape[0]), int(M.shape[1]))
    return np.ascontiguousarray(M, dt), None


def _monitored(watch, fit, *args):
    """The fit call of ``fit(..., validation=)``: whatever it does, the monitor and its resident set do not outlive it."""
    try:
        return fit(*args)
    finally:
        if watch is not None:
            watch.close()


def _validation_results(self, watch):
    """``validation_history_`` / ``validation_records_`` / ``best_iteration_`` / ``n_iter_`` of a fit (``watch`` None: a fit
    without validation)."""
    if watch is None:
        self.validation_history_, self.validation_records_, self.best_iteration_, self.n_iter_ = [], [], None, self.niter
    else:
        self.validation_history_, self.validation_records_, self.best_iteration_, self.n_iter_ = watch.results()


def _penalty(value, name):
    """``lambda_`` / ``l1_lambda``: a number, or six numbers (user bias, item bias, A, B, C, D) like the reference
    (cmfrec/__init__.py:99-101).  Returns (scalar, array-or-None); with an array the scalar handed to C is 0, as the
    reference does (cmfrec/__init__.py:3179-3180)."""
    if np.isscalar(value):
        return float(value), None
    arr = np.asarray(value, np.float64).reshape(-1)
    if arr.shape[0] != 6:
        raise ValueError("'%s' must be a single number or an array with 6 entries." % name)
    return 0.0, arr


class CMF_implicit(_Base):
    """Implicit-feedback model (iALS / WRMF), reference class ``CMF_implicit``."""

    def __init__(self, k=50, lambda_=1e0, alpha=1., use_cg=True, k_user=0, k_item=0, k_main=0,
                 w_main=1., w_user=10., w_item=10., l1_lambda=0., center_U=True, center_I=True,
                 niter=10, NA_as_zero_user=False, NA_as_zero_item=False, nonneg=False, nonneg_C=False,
                 nonneg_D=False, max_cd_steps=100, apply_log_transf=False,
                 precompute_for_predictions=True, use_float=True, max_cg_steps=3,
                 precondition_cg=False, finalize_chol=False, random_state=1, verbose=False,
                 produce_dicts=False, handle_interrupt=True, nthreads=-1, n_jobs=None):
        # sparse side information whose absent entries are zeros (not missing): cmfrec/__init__.py:4688-4690.  The C library
        # runs it as the zero-filled dense matrix it denotes (fit.hip, ZeroFilledSide), or on the triplets where that matrix would
        # be too large (SparseZerosSide)
        self.NA_as_zero_user = bool(NA_as_zero_user); self.NA_as_zero_item = bool(NA_as_zero_item)
        self.k = int(k); self.alpha = float(alpha); self.use_cg = bool(use_cg)
        self.lambda_, self._lam6 = _penalty(lambda_, "lambda_")
        self.k_user = int(k_user); self.k_item = int(k_item); self.k_main = int(k_main)
        self.w_main = float(w_main); self.w_user = float(w_user); self.w_item = float(w_item)
        self.l1_lambda = l1_lambda; self.niter = int(niter); self.nonneg = bool(nonneg)
        self.center_U = bool(center_U); self.center_I = bool(center_I)
        self.apply_log_transf = bool(apply_log_transf)
        self.precompute_for_predictions = bool(precompute_for_predictions)
        self.max_cg_steps = int(max_cg_steps); self.precondition_cg = bool(precondition_cg)
        self.finalize_chol = bool(finalize_chol); self.random_state = int(random_state)
        self.verbose = bool(verbose); self.handle_interrupt = bool(handle_interrupt)
        self._setup(use_float, nthreads, n_jobs)
        self.nonneg_C = bool(nonneg_C); self.nonneg_D = bool(nonneg_D); self.max_cd_steps = int(max_cd_steps)
        self.l1_lambda, self._l16 = _penalty(l1_lambda, "l1_lambda")

    def fit(self, X, U=None, I=None, shape=None, A0=None, B0=None, validation=None):
        """Fits the model.  ``A0``/``B0`` (optional) inject the start values instead of drawing
        them from ``random_state`` (C argument ``reset_values=false``).  ``U`` / ``I``: dense side
        information without missing values, or SciPy sparse matrices (missing = absent).
        ``validation``: a ``cmfrec_amd.Validation`` -- a held-out set evaluated on the device while fitting, early stopping and the
        best iterate (default metric "ndcg" at ``k=10``, the training items left out of every ranking)."""
        self.close()                                # the one-user handles hold the factors of the fit that was
        row, col, val, m, n = _coo_triplet(X, shape)
        lib, R = self._lib()
        dt = self.dtype_
        lam6 = None if self._lam6 is None else np.ascontiguousarray(self._lam6, dt)
        l16 = None if self._l16 is None else np.ascontiguousarray(self._l16, dt)
        val = np.ascontiguousarray(val, dt)
        Uc, Us = _side_info(U, dt)
        Ic, Is = _side_info(I, dt)
        m_u, p = (0, 0) if Uc is None else Uc.shape
        n_i, q = (0, 0) if Ic is None else Ic.shape
        if Us is not None: m_u, p = Us[3], Us[4]
        if Is is not None: n_i, q = Is[3], Is[4]
        spU = (None, None, None, C.c_size_t(0)) if Us is None else (_lib.ptr(Us[0]), _lib.ptr(Us[1]), _lib.ptr(Us[2]), C.c_size_t(len(Us[2])))
        spI = (None, None, None, C.c_size_t(0)) if Is is None else (_lib.ptr(Is[0]), _lib.ptr(Is[1]), _lib.ptr(Is[2]), C.c_size_t(len(Is[2])))
        ka, kb = self.k_user + self.k + self.k_main, self.k_item + self.k + self.k_main
        reset = A0 is None
        A = np.empty((max(m, m_u), ka), dt) if reset else np.array(A0, dt, order="C", copy=True)     # m_max rows
        B = np.empty((max(n, n_i), kb), dt) if (reset or B0 is None) else np.array(B0, dt, order="C", copy=True)
        if not reset and B0 is None:
            B[:] = 0
        Cm = np.zeros((p, self.k_user + self.k), dt) if p else None
        Dm = np.zeros((q, self.k_item + self.k), dt) if q else None
        Ucm = np.zeros(max(p, 1), dt); Icm = np.zeros(max(q, 1), dt)
        wmm = np.zeros(1, dt)
        pre = self.precompute_for_predictions
        kq = self.k_user + self.k + self.k_main
        BtB = np.zeros((self.k + self.k_main,) * 2, dt) if pre else None
        BeTBe = np.zeros((kq, kq), dt) if (pre and p) else None
        BeTBeChol = np.zeros((kq, kq), dt) if (pre and p) else None
        CtUbias = np.zeros(self.k_user + self.k, dt) if (pre and p and Us is not None and self.NA_as_zero_user) else None
        watch = None if validation is None else validation._begin(lib, dt, self.niter, "ndcg", (row, col, m, n))
        rc = _monitored(watch, lib.fit_collective_implicit_als,
            _lib.ptr(A), _lib.ptr(B), _lib.ptr(Cm), _lib.ptr(Dm), C.c_bool(reset), C.c_int(self.random_state),
            _lib.ptr(Ucm) if (p and self.center_U) else None, _lib.ptr(Icm) if (q and self.center_I) else None,
            C.c_int(m), C.c_int(n), C.c_int(self.k), _lib.ptr(row), _lib.ptr(col), _lib.ptr(val),
            C.c_size_t(len(val)), R(self.lambda_), _lib.ptr(lam6), R(self.l1_lambda), _lib.ptr(l16),
            _lib.ptr(Uc), C.c_int(m_u), C.c_int(p), _lib.ptr(Ic), C.c_int(n_i), C.c_int(q),
            *spU, *spI,
            C.c_bool(self.NA_as_zero_user), C.c_bool(self.NA_as_zero_item), C.c_int(self.k_main), C.c_int(self.k_user), C.c_int(self.k_item),
            R(self.w_main), R(self.w_user), R(self.w_item), _lib.ptr(wmm),
            R(self.alpha), C.c_bool(bool(getattr(self, "_adjust_weight", False))),   # the reference's estimator always passes False (__init__.py:4753)
            C.c_bool(self.apply_log_transf), C.c_int(self.niter), C.c_int(self.nthreads),
            C.c_bool(self.verbose), C.c_bool(self.handle_interrupt), C.c_bool(self.use_cg),
            C.c_int(self.max_cg_steps), C.c_bool(self.precondition_cg), C.c_bool(self.finalize_chol),
            C.c_bool(self.nonneg), C.c_int(self.max_cd_steps), C.c_bool(self.nonneg_C), C.c_bool(self.nonneg_D),
            C.c_bool(pre), _lib.ptr(BtB), _lib.ptr(BeTBe), _lib.ptr(BeTBeChol), _lib.ptr(CtUbias))
        # an interrupted fit returns 3 with usable factors; like the reference's wrapper, raise only when the caller did
        # not ask for the interrupt to be handled (cmfrec/wrapper_untyped.pxi: `if ret_code == 3 and not handle_interrupt`)
        _lib.check(rc, lib, "fit_collective_implicit_als", interrupt_ok=self.handle_interrupt)
        _validation_results(self, watch)
        self.A_, self.B_ = A, B
        self.C_ = Cm if Cm is not None else np.empty((0, 0), dt)
        self.D_ = Dm if Dm is not None else np.empty((0, 0), dt)
        self._U_colmeans, self._I_colmeans = Ucm[:p], Icm[:q]
        self._w_main_multiplier = float(wmm[0])
        # precomputed matrices for predictions on new data, reference attribute names (cmfrec/__init__.py:4893-4927)
        e = np.empty((0, 0), dt)
        self._BtB = BtB if BtB is not None else e
        self._BeTBe = BeTBe if BeTBe is not None else e
        self._BeTBeChol = BeTBeChol if BeTBeChol is not None else e
        self._CtUbias = CtUbias if CtUbias is not None else np.empty(0, dt)
        self.is_fitted_ = True
        return self

    def factors_multiple(self, X=None, U=None):
        """Factors of new users from their interactions ``X`` [m_x, n] (sparse) and / or dense attributes ``U`` [m_u, p]
        (reference ``CMF_implicit.factors_multiple``, cmfrec/__init__.py:5313; C function
        factors_collective_implicit_multiple).  Returns ``A`` [max(m_x, m_u), k_user+k+k_main]."""
        b = _new_rows_batch(self, X, U, None, dense_ok=False)
        lam6 = None if self._lam6 is None else np.ascontiguousarray(self._lam6, self.dtype_)
        l1 = self.l1_lambda if self._l16 is None else float(self._l16[2])       # the reference passes l1_lambda[2], like lambda_
        lib, R = self._lib()
        dt = self.dtype_
        n = self.B_.shape[0]
        row, col, val, m_x, Uc, m_u, p = b["row"], b["col"], b["val"], b["m_x"], b["U"], b["m_u"], b["p"]
        A = np.empty((max(m_x, m_u), self.k_user + self.k + self.k_main), dt)
        has = lambda M: M is not None and M.shape[0] > 0
        rc = lib.factors_collective_implicit_multiple(
            _lib.ptr(A), C.c_int(m_x), _lib.ptr(Uc), C.c_int(m_u), C.c_int(p), C.c_bool(False), C.c_bool(self.nonneg),
            *_sparse_U_args(b["Usp"]),
            _lib.ptr(val), _lib.ptr(row), _lib.ptr(col), C.c_size_t(len(val)), None, None, None,
            _lib.ptr(self.B_), C.c_int(n), _lib.ptr(self.C_) if p else None,
            _lib.ptr(self._U_colmeans) if (p and len(self._U_colmeans)) else None,
            C.c_int(self.k), C.c_int(self.k_user), C.c_int(self.k_item), C.c_int(self.k_main),
            R(self.lambda_ if lam6 is None else float(lam6[2])), R(l1), R(self.alpha), R(self.w_main), R(self.w_user),
            R(self._w_main_multiplier),
            C.c_bool(self.apply_log_transf),
            _lib.ptr(self._BeTBe) if has(self._BeTBe) else None, _lib.ptr(self._BtB) if has(self._BtB) else None,
            _lib.ptr(self._BeTBeChol) if has(self._BeTBeChol) else None, None, C.c_int(self.nthreads))
        _lib.check(rc, lib, "factors_collective_implicit_multiple")
        return A

    def topN_batch(self, users, n=10, exclude=None, include=None):
        """Top-``n`` item ids and scores (A_u . B_i) for a batch of users, ranked on the GPU; ``exclude``: CSR of items
        to skip per user (e.g. the training matrix).  Batch form of the reference's ``topN`` (common.c:5127-5380).
        ``include``: candidate lists -- (indptr, indices) CSR over the users OF THIS CALL (one list per entry of ``users``), a
        SciPy CSR matrix of that many rows, or one 1-D array shared by all: each user is ranked over its own list only."""
        return _topN(self, users, n, exclude, None, include)

    def topN_deep(self, users, n, exclude=None):
        return _topN_deep(self, users, n, exclude, None)
    topN_deep.__doc__ = _TOPN_DEEP_DOC

    def ranks_batch(self, users, heldout, exclude=None):
        """(indptr, items, ranks, pool): the 0-based place of each held-out item in its user's full ranking by A_u . B_i, counted
        on the GPU (``ops.ranks_batch``).  ``heldout``: (indptr, indices) CSR over the users OF THIS CALL or a SciPy CSR matrix
        of that many rows; ``exclude``: CSR over all users, as in ``topN_batch``."""
        return _ranks(self, users, heldout, exclude, None)

    def evaluate_ranking(self, X_test, X_train=None, k=10, users=None, batch_users=4096):
        return _evaluate_ranking(self, X_test, X_train, k, users, batch_users)
    evaluate_ranking.__doc__ = _EVALUATE_DOC

    def _finish_scores(self, users, sc):
        return sc

    def new_users(self):
        """A ``cmfrec_amd.NewUsers`` over this model: the model goes to the device once, then ``.factors(X, U)`` /
        ``.topN(X, U, n, exclude_seen, exclude)`` per batch of users who were not part of the fit."""
        from .new_users import NewUsers
        return NewUsers(self)

    def topN_new_batch(self, X=None, U=None, n=10, exclude_seen=True, exclude=None, include=None):
        """Top-``n`` items for users who were not part of the fit, from their interactions and / or attributes (batch form of
        the reference's ``topN_new``): one ``new_users()`` handle made, used and closed.  ``include``: candidate lists over the
        rows of the batch, as ``NewUsers.topN`` takes them."""
        return _topN_new_batch(self, X, U, None, n, exclude_seen, exclude, include)

    def ranker(self):
        """A ``ModelRanker`` over this model's item factors: upload them once, then ``.topN(users, n, exclude)`` per batch."""
        return ModelRanker(self, None)

    def similar_items(self, items, n=10, metric="cosine"):
        return _similar(self.B_, self.k_item, items, n, metric, "similar_items")
    similar_items.__doc__ = _SIMILAR_ITEMS_DOC

    def similar_users(self, users, n=10, metric="cosine"):
        return _similar(self.A_, self.k_user, users, n, metric, "similar_users")
    similar_users.__doc__ = _SIMILAR_USERS_DOC

    def scorer(self):
        """A ``cmfrec_amd.Scorer`` over this model: both factor matrices go to the device once, then ``.predict(user, item)``
        per batch of pairs (NaN for a pair outside the model).  The caller closes it; a refit needs a new one."""
        return _scorer(self, None, None, 0.0, True)

    def predict_batch(self, user, item):
        """``predict`` on the device: one ``scorer()`` made, used and closed.  Equal to ``predict`` within the rounding of kk
        products summed in another order; a pair outside the model gives NaN where ``predict`` raises."""
        with self.scorer() as sc:
            return sc.predict(user, item)

    def evaluate_error(self, X_test):
        """Squared and absolute error of A_u . B_i on held-out values, reduced on the device: ``X_test`` a SciPy sparse matrix or
        a (row, col, value) triplet, as ``fit`` takes.  One ``scorer()`` and one ``cmfrec_amd.EvalSet`` made, used and closed;
        returns ``cmfrec_amd.metrics.error_metrics``' dict (rmse, mse, mae, bias, max_abs, n, n_fallback, n_skipped, sum_w).  An
        entry whose user or item lies outside the model has no prediction and is counted in ``n_skipped``, as is a NaN value."""
        return _evaluate_error(self, X_test, None, True)

    def predict_new_batch(self, X=None, U=None, row=None, item=None):
        """Predictions for chosen pairs (row of the batch, item) of users who were not part of the fit (reference
        ``predict_new``; C function predict_X_new_collective_implicit): one ``new_users()`` handle made, used and closed."""
        with self.new_users() as nu:
            return nu.predict(X=X, U=U, row=row, item=item)

    # ---- the reference's one-user interface (cmfrec_amd/one_user.py): batches of one on two resident handles, a ModelRanker and
    # a NewUsers with split="auto", made by the first call and released by fit() / close().  Every k is scored by the MFMA
    # kernel: for k <= 64 the scores agree with topN_batch up to rounding, not in bits.
    def topN(self, user, n=10, include=None, exclude=None, output_score=False):
        """The ``n`` best items of one user of the fit (reference ``CMF_implicit.topN``): ids [n], or ``(ids, scores)`` with
        ``output_score``.  Nothing is excluded unless ``exclude`` (item ids) says so; ``include`` (item ids) ranks over those
        items only; the two together raise ``ValueError``.  ``topN_batch([user], ...)`` row 0 from a resident ranker."""
        from . import one_user
        return one_user.topN(self, user, n, include, exclude, output_score)

    def topN_warm(self, n=10, X_col=None, X_val=None, U=None, U_col=None, U_val=None, include=None, exclude=None, output_score=False):
        """The ``n`` best items of a new user from its interactions ``X_col`` / ``X_val`` (and attributes ``U``, or ``U_col`` /
        ``U_val``), reference ``CMF_implicit.topN_warm``: ``topN_new_batch`` of one row with ``exclude_seen=False``."""
        from . import one_user
        return one_user.topN_new(self, n, None, X_col, X_val, None, U, None, U_col, U_val, include, exclude, output_score, True)

    def topN_cold(self, n=10, U=None, U_col=None, U_val=None, include=None, exclude=None, output_score=False):
        """The ``n`` best items of a new user from its attributes alone (reference ``CMF_implicit.topN_cold``)."""
        from . import one_user
        return one_user.topN_new(self, n, None, None, None, None, U, None, U_col, U_val, include, exclude, output_score, False)

    def factors_warm(self, X_col, X_val, U=None, U_col=None, U_val=None):
        """The factors [k_user + k + k_main] of a new user (reference ``CMF_implicit.factors_warm``): ``factors_multiple`` row 0."""
        from . import one_user
        return one_user.factors_new(self, None, X_col, X_val, None, U, None, U_col, U_val, False, True)

    def factors_cold(self, U=None, U_col=None, U_val=None):
        """The factors of a new user from its attributes alone (reference ``CMF_implicit.factors_cold``)."""
        from . import one_user
        return one_user.factors_new(self, None, None, None, None, U, None, U_col, U_val, False, False)

    def predict_warm(self, items, X_col, X_val, U=None, U_col=None, U_val=None):
        """The scores [len(items)] of a new user for ``items`` (reference ``CMF_implicit.predict_warm``)."""
        from . import one_user
        return one_user.predict_new(self, items, None, X_col, X_val, None, U, None, U_col, U_val, True)

    def predict_cold(self, items, U=None, U_col=None, U_val=None):
        """The scores [len(items)] of a new user for ``items`` from its attributes alone (reference ``CMF_implicit.predict_cold``)."""
        from . import one_user
        return one_user.predict_new(self, items, None, None, None, None, U, None, U_col, U_val, False)

    def predict(self, user, item):
        """A_u . B_i for paired user / item ids (reference predict_multiple, common.c:5066-5106).  NumPy on the host;
        ``predict_batch`` scores the pairs on the device."""
        user = np.asarray(user); item = np.asarray(item)
        return np.einsum("ij,ij->i", self.A_[user, self.k_user:], self.B_[item, self.k_item:])


class CMF(_Base):
    """Explicit-feedback collective model, reference class ``CMF`` (ALS only)."""

    def __init__(self, k=40, lambda_=1e+1, method="als", use_cg=True, user_bias=True, item_bias=True,
                 center=True, add_implicit_features=False, scale_lam=False, scale_lam_sideinfo=False,
                 scale_bias_const=False, k_user=0, k_item=0, k_main=0, w_main=1., w_user=1., w_item=1.,
                 w_implicit=0.5, l1_lambda=0., center_U=True, center_I=True, maxiter=800, niter=10,
                 parallelize="separate", corr_pairs=4, max_cg_steps=3, precondition_cg=False,
                 finalize_chol=True, NA_as_zero=False, NA_as_zero_user=False, NA_as_zero_item=False,
                 nonneg=False, nonneg_C=False, nonneg_D=False, max_cd_steps=100,
                 precompute_for_predictions=True, include_all_X=True, use_float=True, random_state=1,
                 verbose=False, print_every=10, handle_interrupt=True, produce_dicts=False, nthreads=-1,
                 n_jobs=None):
        if method != "als":
            raise NotImplementedError("only method='als' is implemented in cmfrec_amd")
        # sparse side information whose absent entries are zeros (not missing): cmfrec/__init__.py:2903-2905.  The C library
        # runs it as the zero-filled dense matrix it denotes (fit.hip, ZeroFilledSide), or on the triplets where that matrix would
        # be too large (SparseZerosSide)
        self.NA_as_zero_user = bool(NA_as_zero_user); self.NA_as_zero_item = bool(NA_as_zero_item)
        # NA_as_zero (absent entries of a sparse X are zeros): without side information or with dense complete / sparse side
        # information on exactly the rows / columns of X, closed form or CG, with add_implicit_features too; the matrices for
        # predictions on new data (with BtXbias) for the model without side information and implicit features only.  With
        # observation weights (fit(..., W=)): the same models without implicit features; start values given by the caller
        # (A0 / B0 / biasA0 / biasB0) when the model has biases -- the reference's own bias start values are not defined for that
        # combination (common.c:4727-4731).  What is refused and why: DESIGN.md section 7.
        self.NA_as_zero = bool(NA_as_zero)
        # (precompute_for_predictions with NA_as_zero: the model without side information -- checked in fit(), where the data is known)
        self.scale_bias_const = bool(scale_bias_const)
        if add_implicit_features and (nonneg or not np.isscalar(l1_lambda) or l1_lambda):
            raise NotImplementedError("add_implicit_features together with nonneg / l1_lambda is not implemented in "
                                      "cmfrec_amd (the reference itself crashes on it)")
        self.add_implicit_features = bool(add_implicit_features)
        self.l1_lambda, self._l16 = _penalty(l1_lambda, "l1_lambda")
        self.nonneg = bool(nonneg); self.nonneg_C = bool(nonneg_C); self.nonneg_D = bool(nonneg_D)
        self.max_cd_steps = int(max_cd_steps)
        self.k = int(k); self.use_cg = bool(use_cg)
        self.lambda_, self._lam6 = _penalty(lambda_, "lambda_")
        self.user_bias = bool(user_bias); self.item_bias = bool(item_bias); self.center = bool(center)
        self.center_U = bool(center_U); self.center_I = bool(center_I)
        self.scale_lam = bool(scale_lam); self.scale_lam_sideinfo = bool(scale_lam_sideinfo)
        self.k_user = int(k_user); self.k_item = int(k_item); self.k_main = int(k_main)
        self.w_main = float(w_main); self.w_user = float(w_user); self.w_item = float(w_item)
        self.w_implicit = float(w_implicit); self.niter = int(niter); self.max_cg_steps = int(max_cg_steps)
        self.precondition_cg = bool(precondition_cg); self.finalize_chol = bool(finalize_chol)
        self.precompute_for_predictions = bool(precompute_for_predictions)
        self.random_state = int(random_state); self.verbose = bool(verbose)
        self.handle_interrupt = bool(handle_interrupt)
        self._setup(use_float, nthreads, n_jobs)

    def fit(self, X, U=None, I=None, shape=None, A0=None, B0=None, biasA0=None, biasB0=None, W=None, validation=None):
        """``X``: SciPy sparse matrix / COO triplet, or a dense 2-D array with NaN for the missing entries (the plain model:
        no side information).  ``W``: observation weights, one per entry of ``X`` in its COO order (reference
        ``CMF.fit(X, ..., W=...)``, cmfrec/__init__.py:3066; an array(nnz,) for sparse ``X``, an array(m, n) for dense ``X``).
        ``validation``: a ``cmfrec_amd.Validation`` -- a held-out set evaluated on the device while fitting (default metric
        "rmse"), early stopping and the best iterate; the model then has ``validation_history_``, ``best_iteration_``, ``n_iter_``."""
        self.close()                                # the one-user handles hold the factors of the fit that was
        lib, R = self._lib()
        dt = self.dtype_
        Xfull = None
        if isinstance(X, np.ndarray):
            if X.ndim != 2:
                raise ValueError("a dense 'X' must be a 2-D array")
            if self.NA_as_zero:
                raise ValueError("'NA_as_zero' is for a sparse 'X'.")
            Xfull = np.ascontiguousarray(X, dt)
            m, n = Xfull.shape
            row = col = np.empty(0, np.int32); val = np.empty(0, dt)
        else:
            row, col, val, m, n = _coo_triplet(X, shape)
        Wv = None
        if W is not None:
            Wv = np.ascontiguousarray(np.asarray(W).reshape(-1), dt)
            if Wv.shape[0] != (len(val) if Xfull is None else Xfull.size):
                raise ValueError("'W' must have the same number of entries as 'X'.")
        lam6 = None if self._lam6 is None else np.ascontiguousarray(self._lam6, dt)
        l16 = None if self._l16 is None else np.ascontiguousarray(self._l16, dt)
        val = np.ascontiguousarray(val, dt)
        Uc, Us = _side_info(U, dt)
        Ic, Is = _side_info(I, dt)
        m_u, p = (0, 0) if Uc is None else Uc.shape
        n_i, q = (0, 0) if Ic is None else Ic.shape
        if Us is not None: m_u, p = Us[3], Us[4]
        if Is is not None: n_i, q = Is[3], Is[4]
        spU = (None, None, None, C.c_size_t(0)) if Us is None else (_lib.ptr(Us[0]), _lib.ptr(Us[1]), _lib.ptr(Us[2]), C.c_size_t(len(Us[2])))
        spI = (None, None, None, C.c_size_t(0)) if Is is None else (_lib.ptr(Is[0]), _lib.ptr(Is[1]), _lib.ptr(Is[2]), C.c_size_t(len(Is[2])))
        use_cg = self.use_cg
        ka, kb = self.k_user + self.k + self.k_main, self.k_item + self.k + self.k_main
        reset = A0 is None
        A = np.empty((max(m, m_u), ka), dt) if reset else np.array(A0, dt, order="C", copy=True)
        B = np.empty((max(n, n_i), kb), dt) if (reset or B0 is None) else np.array(B0, dt, order="C", copy=True)
        if not reset and B0 is None:
            B[:] = 0
        biasA = np.zeros(max(m, m_u), dt) if biasA0 is None else np.array(biasA0, dt, copy=True)
        biasB = np.zeros(max(n, n_i), dt) if biasB0 is None else np.array(biasB0, dt, copy=True)
        Cm = np.zeros((p, self.k_user + self.k), dt) if p else None
        Dm = np.zeros((q, self.k_item + self.k), dt) if q else None
        glob_mean = np.zeros(1, dt); Ucm = np.zeros(max(p, 1), dt); Icm = np.zeros(max(q, 1), dt)
        sbA = np.zeros(1, dt); sbB = np.zeros(1, dt)
        # with implicit features the matrices for new-row predictions are not produced (factors_multiple is unavailable)
        pre = self.precompute_for_predictions and not self.add_implicit_features
        imp = self.add_implicit_features
        Ai = np.zeros((max(m, m_u), self.k + self.k_main), dt) if imp else None
        Bi = np.zeros((max(n, n_i), self.k + self.k_main), dt) if imp else None
        kp = self.k + self.k_main + int(self.user_bias); kc = self.k_user + self.k; kq = self.k_user + kp
        Bpb = np.zeros((max(n, n_i), kb + 1), dt) if (pre and self.user_bias) else None
        BtB = np.zeros((kp, kp), dt) if pre else None
        TBt = np.zeros((max(n, n_i), kp), dt) if pre else None
        BeChol = np.zeros((kq, kq), dt) if (pre and p) else None
        TCt = np.zeros((p, kc), dt) if (pre and p) else None
        CtCw = np.zeros((kc, kc), dt) if (pre and p) else None
        CtUbias = np.zeros(kc, dt) if (pre and p and Us is not None and self.NA_as_zero_user) else None
        if self.NA_as_zero and pre and (p or q or imp):
            raise NotImplementedError("NA_as_zero with side information or implicit features: precompute_for_predictions is not "
                                      "implemented in cmfrec_amd (pass False)")
        BtXbias = np.zeros(kp, dt) if (pre and self.NA_as_zero) else None       # reference attribute BtXbias_ (cmfrec/__init__.py)
        watch = None if validation is None else validation._begin(
            lib, dt, self.niter, "rmse", (row, col, m, n) if Xfull is None else (*np.nonzero(~np.isnan(Xfull)), m, n))
        rc = _monitored(watch, lib.fit_collective_explicit_als,
            _lib.ptr(biasA), _lib.ptr(biasB), _lib.ptr(A), _lib.ptr(B), _lib.ptr(Cm), _lib.ptr(Dm), _lib.ptr(Ai), _lib.ptr(Bi),
            C.c_bool(imp), C.c_bool(reset), C.c_int(self.random_state), _lib.ptr(glob_mean),
            # no column means = the side information is used as given (cmfrec/__init__.py passes an empty array for center_U=False)
            _lib.ptr(Ucm) if (p and self.center_U) else None, _lib.ptr(Icm) if (q and self.center_I) else None,
            C.c_int(m), C.c_int(n), C.c_int(self.k), _lib.ptr(row), _lib.ptr(col), _lib.ptr(val),
            C.c_size_t(len(val)), _lib.ptr(Xfull), _lib.ptr(Wv), C.c_bool(self.user_bias), C.c_bool(self.item_bias),
            C.c_bool(self.center), R(self.lambda_), _lib.ptr(lam6), R(self.l1_lambda), _lib.ptr(l16), C.c_bool(self.scale_lam),
            C.c_bool(self.scale_lam_sideinfo), C.c_bool(self.scale_bias_const), _lib.ptr(sbA), _lib.ptr(sbB),
            _lib.ptr(Uc), C.c_int(m_u), C.c_int(p), _lib.ptr(Ic), C.c_int(n_i), C.c_int(q),
            *spU, *spI,
            C.c_bool(self.NA_as_zero), C.c_bool(self.NA_as_zero_user), C.c_bool(self.NA_as_zero_item),
            C.c_int(self.k_main), C.c_int(self.k_user), C.c_int(self.k_item),
            R(self.w_main), R(self.w_user), R(self.w_item), R(self.w_implicit),
            C.c_int(self.niter), C.c_int(self.nthreads), C.c_bool(self.verbose), C.c_bool(self.handle_interrupt),
            C.c_bool(use_cg), C.c_int(self.max_cg_steps), C.c_bool(self.precondition_cg),
            C.c_bool(self.finalize_chol), C.c_bool(self.nonneg), C.c_int(self.max_cd_steps), C.c_bool(self.nonneg_C),
            C.c_bool(self.nonneg_D),
            C.c_bool(pre), C.c_bool(True), _lib.ptr(Bpb), _lib.ptr(BtB), _lib.ptr(TBt), _lib.ptr(BtXbias), _lib.ptr(BeChol), None,
            _lib.ptr(TCt), _lib.ptr(CtCw), _lib.ptr(CtUbias))
        _lib.check(rc, lib, "fit_collective_explicit_als", interrupt_ok=self.handle_interrupt)
        _validation_results(self, watch)
        # precomputed matrices for predictions on new data, reference attribute names (cmfrec/__init__.py:3211-3247)
        e = np.empty((0, 0), dt)
        self._B_plus_bias = Bpb if Bpb is not None else e
        self._BtB = BtB if BtB is not None else e
        self._TransBtBinvBt = TBt if TBt is not None else e
        self._BtXbias = BtXbias if BtXbias is not None else np.empty(0, dt)
        self._BeTBeChol = BeChol if BeChol is not None else e
        self._TransCtCinvCt = TCt if TCt is not None else e
        self._CtUbias = CtUbias if CtUbias is not None else np.empty(0, dt)
        self._CtCw = CtCw if CtCw is not None else e
        self._scaling_biasA, self._scaling_biasB = float(sbA[0]), float(sbB[0])    # cmfrec/__init__.py: scaling_biasA_ / _B_
        self.A_, self.B_ = A, B
        self.Ai_ = Ai if imp else e                      # cmfrec/__init__.py:3195-3196
        self.Bi_ = Bi if imp else e
        self.C_ = Cm if Cm is not None else np.empty((0, 0), dt)
        self.D_ = Dm if Dm is not None else np.empty((0, 0), dt)
        self.user_bias_ = biasA if self.user_bias else np.empty(0, dt)
        self.item_bias_ = biasB if self.item_bias else np.empty(0, dt)
        self.glob_mean_ = float(glob_mean[0])
        self._U_colmeans = Ucm[:p] if self.center_U else Ucm[:0]
        self._I_colmeans = Icm[:q] if self.center_I else Icm[:0]
        self.is_fitted_ = True
        return self

    def factors_multiple(self, X=None, U=None, W=None, return_bias=False):
        """Factors (and bias) of new users from their ratings ``X`` [m_x, n] and / or dense attributes ``U`` [m_u, p]
        (reference ``CMF.factors_multiple``, cmfrec/__init__.py:3706; C function factors_collective_explicit_multiple).
        ``X``: a SciPy sparse matrix, a (row, col, val) triplet, or a dense array with NaN for the missing entries.  ``W``:
        observation weights in the form of ``X`` (a sparse ``W`` must have ``X``'s pattern).  A model fitted with
        ``add_implicit_features`` uses its ``Bi_``.  Returns ``A`` [max(m_x, m_u), k_user+k+k_main], or ``(A, bias)``."""
        if self.NA_as_zero or self.NA_as_zero_user:
            # the missing-as-zero models go through the new-rows handle, which knows the options (the drop-in call refuses them)
            with self.new_users() as nu:
                return nu.factors(X=X, U=U, W=W, return_bias=return_bias)
        b = _new_rows_batch(self, X, U, W, dense_ok=True)
        lam6 = None if self._lam6 is None else np.ascontiguousarray(self._lam6, self.dtype_)
        l16 = None if self._l16 is None else np.ascontiguousarray(self._l16, self.dtype_)
        lib, R = self._lib()
        dt = self.dtype_
        n = self.B_.shape[0]
        row, col, val, m_x, Xfull, Wv, Uc, m_u, p = (b[f] for f in ("row", "col", "val", "m_x", "Xfull", "W", "U", "m_u", "p"))
        mm = max(m_x, m_u)
        A = np.empty((mm, self.k_user + self.k + self.k_main), dt)
        biasA = np.empty(mm, dt) if self.user_bias else None
        has = lambda M: M is not None and M.shape[0] > 0
        imp = self.add_implicit_features
        Bi = np.ascontiguousarray(self.Bi_, dt) if imp else None
        TBt = getattr(self, "_TransBtBinvBt", None)
        rc = lib.factors_collective_explicit_multiple(
            _lib.ptr(A), _lib.ptr(biasA), C.c_int(m_x), _lib.ptr(Uc), C.c_int(m_u), C.c_int(p),
            C.c_bool(False), C.c_bool(False), C.c_bool(self.nonneg),
            *_sparse_U_args(b["Usp"]), None, C.c_int(0), C.c_int(0),
            _lib.ptr(self.C_) if p else None, None, R(self.glob_mean_),
            _lib.ptr(self.item_bias_) if self.item_bias else None,
            _lib.ptr(self._U_colmeans) if (p and len(self._U_colmeans)) else None,
            _lib.ptr(val) if Xfull is None else None, _lib.ptr(row) if Xfull is None else None,
            _lib.ptr(col) if Xfull is None else None, C.c_size_t(len(val)), None, None, None,
            _lib.ptr(Xfull), C.c_int(n), _lib.ptr(Wv), _lib.ptr(self.B_), _lib.ptr(Bi), C.c_bool(imp),
            C.c_int(self.k), C.c_int(self.k_user), C.c_int(self.k_item), C.c_int(self.k_main),
            R(self.lambda_), _lib.ptr(lam6), R(self.l1_lambda), _lib.ptr(l16), C.c_bool(self.scale_lam), C.c_bool(self.scale_lam_sideinfo),
            C.c_bool(self.scale_bias_const), R(self._scaling_biasA if self.scale_bias_const else 1.), R(self.w_main), R(self.w_user),
            R(self.w_implicit),
            C.c_int(n), C.c_bool(True),
            None, _lib.ptr(TBt) if has(TBt) else None, None, None, None,
            _lib.ptr(self._TransCtCinvCt) if (p and has(self._TransCtCinvCt)) else None, None, None, None,
            C.c_int(self.nthreads))
        _lib.check(rc, lib, "factors_collective_explicit_multiple")
        if return_bias:
            return A, biasA
        return A

    def topN_batch(self, users, n=10, exclude=None, include=None):
        """Top-``n`` item ids and scores for a batch of users, ranked on the GPU by A_u . B_i + item_bias[i] (the user
        bias and the global mean do not change the order; the reference adds them to the scores, common.c:5339-5345,
        and so does this method).  ``exclude``: CSR of items to skip per user.  ``include``: candidate lists -- (indptr,
        indices) CSR over the users OF THIS CALL (one list per entry of ``users``), a SciPy CSR matrix of that many rows, or
        one 1-D array shared by all: each user is ranked over its own list only."""
        ids, sc = _topN(self, users, n, exclude, self.item_bias_ if self.item_bias else None, include)
        return ids, self._finish_scores(np.atleast_1d(np.asarray(users, np.int64)), sc)

    def topN_deep(self, users, n, exclude=None):
        return _topN_deep(self, users, n, exclude, self.item_bias_ if self.item_bias else None)
    topN_deep.__doc__ = _TOPN_DEEP_DOC

    def ranks_batch(self, users, heldout, exclude=None):
        """(indptr, items, ranks, pool): the 0-based place of each held-out item in its user's full ranking by
        A_u . B_i + item_bias[i], counted on the GPU (``ops.ranks_batch``).  ``heldout``: (indptr, indices) CSR over the users
        OF THIS CALL or a SciPy CSR matrix of that many rows; ``exclude``: CSR over all users, as in ``topN_batch``."""
        return _ranks(self, users, heldout, exclude, self.item_bias_ if self.item_bias else None)

    def evaluate_ranking(self, X_test, X_train=None, k=10, users=None, batch_users=4096):
        return _evaluate_ranking(self, X_test, X_train, k, users, batch_users)
    evaluate_ranking.__doc__ = _EVALUATE_DOC

    def _finish_scores(self, users, sc):
        sc = sc + self.glob_mean_
        if self.user_bias:
            sc = sc + np.asarray(self.user_bias_)[users][:, None]
        return sc

    def new_users(self):
        """A ``cmfrec_amd.NewUsers`` over this model: the model goes to the device once, then ``.factors(X, U, W)`` /
        ``.topN(X, U, W, n, exclude_seen, exclude)`` per batch of users who were not part of the fit."""
        from .new_users import NewUsers
        return NewUsers(self)

    def topN_new_batch(self, X=None, U=None, W=None, n=10, exclude_seen=True, exclude=None, include=None):
        """Top-``n`` items for users who were not part of the fit, from their ratings and / or attributes (batch form of the
        reference's ``topN_new``), scores + the global mean + the new rows' bias: one ``new_users()`` handle made, used and closed.
        ``include``: candidate lists over the rows of the batch, as ``NewUsers.topN`` takes them."""
        return _topN_new_batch(self, X, U, W, n, exclude_seen, exclude, include)

    def transform(self, X, U=None, W=None):
        """The dense ``X`` [m, n] with its NaN replaced by the model's predictions (reference ``CMF.transform``; C function
        impute_X_collective_explicit), a new array: one ``new_users()`` handle made, used and closed."""
        with self.new_users() as nu:
            return nu.impute(X, U=U, W=W)

    def ranker(self):
        """A ``ModelRanker`` over this model's item factors and item bias: upload them once, then ``.topN(users, n, exclude)``
        per batch, with the scores of ``topN_batch``."""
        return ModelRanker(self, self.item_bias_ if self.item_bias else None)

    def similar_items(self, items, n=10, metric="cosine"):
        return _similar(self.B_, self.k_item, items, n, metric, "similar_items")
    similar_items.__doc__ = _SIMILAR_ITEMS_DOC

    def similar_users(self, users, n=10, metric="cosine"):
        return _similar(self.A_, self.k_user, users, n, metric, "similar_users")
    similar_users.__doc__ = _SIMILAR_USERS_DOC

    def scorer(self):
        """A ``cmfrec_amd.Scorer`` over this model: both factor matrices, the biases and the global mean go to the device once,
        then ``.predict(user, item)`` per batch of pairs (a pair outside the model: the global mean + the bias of the side in
        range).  The caller closes it; a refit needs a new one."""
        return _scorer(self, self.user_bias_ if self.user_bias else None, self.item_bias_ if self.item_bias else None,
                       self.glob_mean_, False)

    def predict_batch(self, user, item):
        """``predict`` on the device: one ``scorer()`` made, used and closed.  Equal to ``predict`` within the rounding of
        kk products and three additions summed in another order, not bit for bit."""
        with self.scorer() as sc:
            return sc.predict(user, item)

    def evaluate_error(self, X_test, W=None, include_fallback=True):
        """Squared and absolute error of the predictions on held-out values, reduced on the device: ``X_test`` a SciPy sparse
        matrix or a (row, col, value) triplet, as ``fit`` takes; ``W``: one weight (finite, >= 0) per entry, or None -- entry i of the
        triplet, or of ``X_test.tocoo()`` for a matrix: for a CSR / CSC matrix that is the order of its ``data``, row by row / column
        by column, not the order in which the entries were once given; pass a triplet where that order matters.  One
        ``scorer()`` and one ``cmfrec_amd.EvalSet`` made, used and closed; returns ``cmfrec_amd.metrics.error_metrics``' dict
        (rmse, mse, mae, bias, max_abs, n, n_fallback, n_skipped, sum_w).  An entry whose user or item lies outside the model is
        predicted by the global mean + the bias of the side in range; ``include_fallback=False`` leaves those entries out of
        the metrics (``n_fallback`` still counts them).  A NaN value is skipped."""
        return _evaluate_error(self, X_test, W, include_fallback)

    def predict_new_batch(self, X=None, U=None, W=None, row=None, item=None):
        """Predictions for chosen pairs (row of the batch, item) of users who were not part of the fit (reference
        ``predict_new``; C function predict_X_new_collective_explicit): one ``new_users()`` handle made, used and closed."""
        with self.new_users() as nu:
            return nu.predict(X=X, U=U, W=W, row=row, item=item)

    # ---- the reference's one-user interface (cmfrec_amd/one_user.py): batches of one on two resident handles, a ModelRanker and
    # a NewUsers with split="auto", made by the first call and released by fit() / close().  Every k is scored by the MFMA
    # kernel: for k <= 64 the scores agree with topN_batch up to rounding, not in bits.
    def topN(self, user, n=10, include=None, exclude=None, output_score=False):
        """The ``n`` best items of one user of the fit (reference ``CMF.topN``): ids [n], or ``(ids, scores)`` with
        ``output_score`` -- the scores of ``topN_batch``, global mean and biases included.  Nothing is excluded unless ``exclude``
        (item ids) says so; ``include`` (item ids) ranks over those items only; the two together raise ``ValueError``.
        ``topN_batch([user], ...)`` row 0 from a resident ranker."""
        from . import one_user
        return one_user.topN(self, user, n, include, exclude, output_score)

    def topN_warm(self, n=10, X=None, X_col=None, X_val=None, W=None, U=None, U_bin=None, U_col=None, U_val=None, include=None,
                  exclude=None, output_score=False):
        """The ``n`` best items of a new user from its ratings -- ``X`` [items] dense with NaN, or ``X_col`` / ``X_val`` -- weights
        ``W`` in the same form, attributes ``U`` [p] or ``U_col`` / ``U_val`` (reference ``CMF.topN_warm``): ``topN_new_batch`` of
        one row with ``exclude_seen=False``.  ``U_bin`` raises ``ValueError``: the reference takes it with L-BFGS only."""
        from . import one_user
        return one_user.topN_new(self, n, X, X_col, X_val, W, U, U_bin, U_col, U_val, include, exclude, output_score, True)

    def topN_cold(self, n=10, U=None, U_bin=None, U_col=None, U_val=None, include=None, exclude=None, output_score=False):
        """The ``n`` best items of a new user from its attributes alone (reference ``CMF.topN_cold``)."""
        from . import one_user
        return one_user.topN_new(self, n, None, None, None, None, U, U_bin, U_col, U_val, include, exclude, output_score, False)

    def factors_warm(self, X=None, X_col=None, X_val=None, W=None, U=None, U_bin=None, U_col=None, U_val=None, return_bias=False):
        """The factors [k_user + k + k_main] of a new user, with ``return_bias`` ``(factors, bias)`` (reference
        ``CMF.factors_warm``): ``factors_multiple`` row 0."""
        from . import one_user
        return one_user.factors_new(self, X, X_col, X_val, W, U, U_bin, U_col, U_val, return_bias, True)

    def factors_cold(self, U=None, U_bin=None, U_col=None, U_val=None):
        """The factors of a new user from its attributes alone (reference ``CMF.factors_cold``)."""
        from . import one_user
        return one_user.factors_new(self, None, None, None, None, U, U_bin, U_col, U_val, False, False)

    def predict_warm(self, items, X=None, X_col=None, X_val=None, W=None, U=None, U_bin=None, U_col=None, U_val=None):
        """The predictions [len(items)] of a new user for ``items`` (reference ``CMF.predict_warm``)."""
        from . import one_user
        return one_user.predict_new(self, items, X, X_col, X_val, W, U, U_bin, U_col, U_val, True)

    def predict_cold(self, items, U=None, U_bin=None, U_col=None, U_val=None):
        """The predictions [len(items)] of a new user for ``items`` from its attributes alone (reference ``CMF.predict_cold``)."""
        from . import one_user
        return one_user.predict_new(self, items, None, None, None, None, U, U_bin, U_col, U_val, False)

    def predict(self, user, item):
        """glob_mean + biasA[u] + biasB[i] + A_u . B_i (reference predict_multiple, common.c:5098-5106).  NumPy on the host;
        ``predict_batch`` scores the pairs on the device."""
        user = np.asarray(user); item = np.asarray(item)
        ku, ki = self.k_user, self.k_item
        out = np.einsum("ij,ij->i", self.A_[user, ku:], self.B_[item, ki:]) + self.glob_mean_
        if self.user_bias:
            out = out + self.user_bias_[user]
        if self.item_bias:
            out = out + self.item_bias_[item]
        return out
