"""Validation while fitting: ``CMF.fit(..., validation=Validation(X_val))`` evaluates a held-out set on the device after the
iterations of the fit, where the factors are, and may stop the fit early and return its best iterate (DESIGN.md section 3.12;
``cmfrec_hip_fit_set_monitor`` of include/cmfrec_hip.h)."""
import ctypes as C
import math

import numpy as np

from . import _lib

ERROR_METRICS = ("rmse", "mae")                                                   # from an error record; lower is better
RANKING_METRICS = ("ndcg", "ap", "hit", "recall", "precision", "rr", "auc", "mean_rank")


class Validation:
    """``Validation(X_val, W=None, metric=None, k=10, X_exclude="train", users=None, every=1, patience=None, min_delta=0.0,
    restore_best=True)``: what ``fit(..., validation=)`` watches.

    ``X_val``: the held-out values, a SciPy sparse matrix or a (row, col, value) triplet as ``fit`` takes ``X``; ``W``: one weight
    (finite, >= 0) per entry or None, as ``evaluate_error`` takes them.  ``metric`` (None: "rmse" for ``CMF``, "ndcg" for ``CMF_implicit``):
    "rmse" or "mae", formed from the error record as ``cmfrec_amd.metrics.error_metrics`` forms them, fallback pairs included (lower
    is better); or a ranking metric at cut-off ``k`` -- "ndcg", "ap", "hit", "recall", "precision", "rr", "auc" (higher is better),
    "mean_rank" (lower is better) -- the means ``cmfrec_amd.metrics.mean_from_record`` gives, over the users of X that have entries in
    ``X_val`` (among ``users`` if given; rows of ``X_val`` beyond X are left out), each ranked over all items but those of ``X_exclude``: "train" (the items the user has in
    the X being fitted), None, or a SciPy sparse matrix / (row, col) triplet.  The values of ``X_val`` and ``W`` play no part in a
    ranking metric.

    The set is evaluated after iterations ``every``, 2 ``every``, ... and after the last one.  An evaluation improves when it
    beats the best so far by more than ``min_delta``; a NaN never does.  ``patience``: stop once that many evaluations in a row
    have not improved (None: never stop, monitor only).  ``restore_best``: the fitted model is the best evaluated iterate --
    factors, biases, C, D, Ai, Bi and the matrices for predictions on new data -- whether the fit stopped or ran to ``niter``;
    False returns the last iterate.  With ``finalize_chol`` the Cholesky pass belongs to iteration ``niter - 1`` alone: a fit
    that stops early does not add one.

    After the fit the model has ``validation_history_`` (one dict per evaluated iteration: ``error_metrics``' or
    ``mean_from_record``'s keys and ``iteration``, 0-based), ``validation_records_`` (the records those came from, as
    ``AlsSession.errors`` / ``AlsSession.ranking`` return them),
    ``best_iteration_`` (None when no evaluation counted) and ``n_iter_`` (the iterations that ran)."""

    def __init__(self, X_val, W=None, metric=None, k=10, X_exclude="train", users=None, every=1, patience=None, min_delta=0.0,
                 restore_best=True):
        if metric is not None and metric not in ERROR_METRICS + RANKING_METRICS:
            raise ValueError("Validation: 'metric' must be one of %s" % ", ".join(ERROR_METRICS + RANKING_METRICS))
        if int(every) != every or every < 1:
            raise ValueError("Validation: 'every' must be an integer >= 1")
        if patience is not None and (int(patience) != patience or patience < 1):
            raise ValueError("Validation: 'patience' must be None (never stop) or an integer >= 1")
        if not (math.isfinite(min_delta) and min_delta >= 0):
            raise ValueError("Validation: 'min_delta' must be finite and >= 0")
        if int(k) != k or k < 1:
            raise ValueError("Validation: 'k' must be an integer >= 1")
        if isinstance(X_val, tuple):
            if len(X_val) != 3 or not (len(X_val[0]) == len(X_val[1]) == len(X_val[2])):
                raise ValueError("Validation: a triplet 'X_val' is (row, col, value) of one length")
            self.row, self.col, self.val = (np.asarray(a) for a in X_val)
        elif hasattr(X_val, "tocoo"):
            Xc = X_val.tocoo()
            self.row, self.col, self.val = Xc.row, Xc.col, Xc.data
        else:
            raise TypeError("Validation: 'X_val' must be a SciPy sparse matrix or a (row, col, value) triplet")
        self.W = None
        if W is not None:
            self.W = np.asarray(W).reshape(-1)
            if len(self.W) != len(self.val):
                raise ValueError("Validation: 'W' must have one weight per entry of 'X_val'")
        self.metric = metric
        self.k = int(k); self.X_exclude = X_exclude; self.users = users
        self.every = int(every); self.patience = None if patience is None else int(patience)
        self.min_delta = float(min_delta); self.restore_best = bool(restore_best)

    def _begin(self, lib, dtype, niter, default_metric, train):
        """Uploads the set and hands the monitor to the calling thread's next fit call; returns the running watch.  ``train``:
        (row, col, m, n) of the X being fitted."""
        metric = default_metric if self.metric is None else self.metric
        return _Watch(self, lib, dtype, int(niter), metric, train)

    def _ranking_lists(self, train):
        """(users, heldout CSR, exclusion CSR or None) of a ranking watch: the users with held-out items (among ``users`` if
        given), their items of ``X_val``, and what to leave out of their rankings -- their training items (``X_exclude="train"``),
        another matrix / triplet, or nothing (None)."""
        import scipy.sparse as sp
        trow, tcol, m, n = train

        def csr(row, col, rows):
            row = np.asarray(row, np.int64); col = np.asarray(col, np.int64)
            if len(row) and (row.min() < 0 or col.min() < 0):
                raise ValueError("Validation: negative index")
            shape = (max(rows, int(row.max()) + 1 if len(row) else 0), max(n, int(col.max()) + 1 if len(col) else 0))
            M = sp.csr_matrix((np.ones(len(row), np.int8), (row, col)), shape=shape)
            M.sum_duplicates(); M.sort_indices()
            return M

        held = csr(self.row, self.col, m)
        users = np.flatnonzero(np.diff(held.indptr) > 0)
        users = users[users < m]                       # (a row beyond X has no factors: left out, as the error watch skips such a pair)
        if self.users is not None:
            users = np.intersect1d(users, np.atleast_1d(np.asarray(self.users, np.int64)))

        def take(M):                                     # (every matrix has at least the rows of `held`)
            S = M[users]
            return S.indptr.astype(np.uint64), S.indices.astype(np.int32)

        excl = None
        if isinstance(self.X_exclude, str):
            if self.X_exclude != "train":
                raise ValueError("Validation: 'X_exclude' must be \"train\", None, a SciPy sparse matrix or a (row, col[, value]) triplet")
            excl = take(csr(trow, tcol, held.shape[0]))
        elif self.X_exclude is not None:
            Xe = self.X_exclude if isinstance(self.X_exclude, tuple) else (self.X_exclude.tocoo().row, self.X_exclude.tocoo().col)
            excl = take(csr(Xe[0], Xe[1], held.shape[0]))
        return users.astype(np.int32), take(held), excl


class _Watch:
    """One monitored fit: the resident set, the monitor's output arrays and what becomes of them."""

    def __init__(self, v, lib, dtype, niter, metric, train):
        self.lib, self.niter, self.metric = lib, niter, metric
        self.ranking = metric in RANKING_METRICS
        self.values = (C.c_double * max(niter, 1))()
        self.iters_run = C.c_int(0); self.best_iter = C.c_int(-1)
        common = dict(metric=_lib.WATCH[metric], every=v.every, patience=v.patience or 0, restore_best=int(v.restore_best),
                      min_delta=v.min_delta, values=self.values, iters_run=C.pointer(self.iters_run), best_iter=C.pointer(self.best_iter))
        if self.ranking:
            from .rank import RankSet
            users, heldout, exclude = v._ranking_lists(train)
            self.records = (_lib.RankRecord * max(niter, 1))()
            self.set = RankSet(users, heldout, exclude, dtype=dtype)
            self.monitor = _lib.FitMonitor(rankset=self.set.handle, k_at=v.k, rank_records=self.records, **common)
        else:
            from .score import EvalSet
            self.records = (_lib.Errors * max(niter, 1))()
            self.set = EvalSet(v.row, v.col, v.val, v.W, dtype=dtype)
            self.monitor = _lib.FitMonitor(evalset=self.set.handle, records=self.records, **common)
        lib.cmfrec_hip_fit_set_monitor(C.byref(self.monitor))

    def close(self):
        """After the fit call, whatever it returned: nothing stays behind for the thread's next fit."""
        self.lib.cmfrec_hip_fit_set_monitor(None)
        self.set.close()

    def results(self):
        """(validation_history_, validation_records_, best_iteration_, n_iter_)"""
        from .metrics import error_metrics, mean_from_record
        history, records = [], []
        for it in range(min(self.niter, self.iters_run.value)):
            rec = self.records[it]
            # (an evaluated iteration whose value is NaN still has a record: every pair / user of the set is counted somewhere in it)
            seen = int(rec.users) if self.ranking else int(rec.n[0]) + int(rec.n[1]) + int(rec.n_skipped)
            if not math.isnan(self.values[it]) or seen:
                entry = mean_from_record(rec.as_dict()) if self.ranking else error_metrics(rec.as_dict())
                entry["iteration"] = it
                history.append(entry)
                records.append(rec.as_dict())
        best = self.best_iter.value
        return history, records, (None if best < 0 else best), self.iters_run.value
