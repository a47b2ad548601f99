"""Users who were not part of the fit, against a model that stays on the device: ``NewUsers`` wraps the
``cmfrec_hip_newrows_*`` handle of include/cmfrec_hip.h.  ``model.factors_multiple`` uploads the item factors (and C, Bi, the
item bias, the precomputed matrices) and rebuilds the Gramians on every call; a ``NewUsers`` does that once, then takes any number
of batches -- their factors, or their top-N straight from the device factors."""
import ctypes as C

import numpy as np

from . import _lib
from .ops import _heldout_lists, _sorted_exclude, _sorted_include


def _has(M):
    return M is not None and M.shape[0] > 0


class NewUsers:
    """What ``CMF.new_users()`` / ``CMF_implicit.new_users()`` return.  The caller owns the handle: ``close()`` it, or use it as a
    context manager; a refit needs a new one.  Calls on one handle must not overlap.
    ``split``: None, ``"auto"`` or a number of slices, as ``Ranker`` takes it -- for the full ranking of ``topN`` (without ``include``)."""

    def __init__(self, model, device=-1, split=None):
        from .rank import split_code
        self.handle = None
        code = split_code(split, "NewUsers: split")
        if not getattr(model, "is_fitted_", False):
            raise ValueError("NewUsers: the model is not fitted")
        self._model = model
        self.dtype = dt = np.dtype(model.dtype_)
        self.implicit = not hasattr(model, "user_bias")
        self.lib = lib = _lib.load(dt)
        mx = _lib.newrows_model_ex_mirror(dt)()             # the model and, behind it, the two missing-as-zero options
        m = mx.base
        keep = []                                           # the arrays behind the struct's pointers, alive until create returns

        def arr(a, dtype=dt):
            a = np.ascontiguousarray(a, dtype)
            keep.append(a)
            return a.ctypes.data

        n = model.B_.shape[0]
        p = model.C_.shape[0]
        m.implicit = int(self.implicit)
        m.n = n; m.n_max = n; m.include_all_X = 1; m.p = p
        m.k = model.k; m.k_user = model.k_user; m.k_item = model.k_item; m.k_main = model.k_main
        m.nonneg = int(model.nonneg)
        m.w_main = model.w_main; m.w_user = model.w_user
        m.B = arr(model.B_)
        if p:
            m.C = arr(model.C_)
            if len(model._U_colmeans):
                m.U_colmeans = arr(model._U_colmeans)
        lam6 = model._lam6
        if self.implicit:
            m.lam = model.lambda_ if lam6 is None else float(np.asarray(lam6, dt)[2])
            m.l1_lam = model.l1_lambda if model._l16 is None else float(model._l16[2])   # the reference passes l1_lambda[2], like lambda_
            m.alpha = model.alpha; m.w_main_multiplier = model._w_main_multiplier
            m.apply_log_transf = int(model.apply_log_transf)
            m.scaling_biasA = 1.; m.w_implicit = 1.
            if _has(model._BtB):
                m.BtB = arr(model._BtB)
        else:
            m.user_bias = int(model.user_bias); m.add_implicit_features = int(model.add_implicit_features)
            m.scale_lam = int(model.scale_lam); m.scale_lam_sideinfo = int(model.scale_lam_sideinfo)
            m.scale_bias_const = int(model.scale_bias_const)
            m.glob_mean = model.glob_mean_; m.lam = model.lambda_; m.l1_lam = model.l1_lambda
            m.scaling_biasA = model._scaling_biasA if model.scale_bias_const else 1.
            m.w_implicit = model.w_implicit; m.alpha = 1.; m.w_main_multiplier = 1.
            # a model fitted with missing-as-zero options solves its new rows under the same model
            mx.NA_as_zero_X = int(getattr(model, "NA_as_zero", False)); mx.NA_as_zero_U = int(getattr(model, "NA_as_zero_user", False))
            if lam6 is not None:
                m.lam_unique = arr(lam6)
            if model._l16 is not None:
                m.l1_lam_unique = arr(model._l16)
            if model.item_bias:
                m.biasB = arr(model.item_bias_)
            if model.add_implicit_features:
                m.Bi = arr(model.Bi_)
            TBt = getattr(model, "_TransBtBinvBt", None)
            if _has(TBt):
                m.TransBtBinvBt = arr(TBt)
            if p and _has(model._TransCtCinvCt):
                m.TransCtCinvCt = arr(model._TransCtCinvCt)
        self.n, self.p = n, p
        self.width = model.k_user + model.k + model.k_main
        self.has_bias = (not self.implicit) and bool(model.user_bias)
        h = lib.cmfrec_hip_newrows_create_ex(C.byref(mx), C.c_int(device))
        if not h:
            _lib.check(lib.cmfrec_hip_last_error_code() or 4, lib, "NewUsers")
        self.handle = C.c_void_p(h)
        self.split = split
        if code != -1:
            _lib.check(lib.cmfrec_hip_newrows_set_split(self.handle, C.c_int(code)), lib, "NewUsers")

    def _live(self):
        if not getattr(self, "handle", None):
            raise RuntimeError("NewUsers: the handle is closed")
        return self.handle

    def _batch(self, X, U, W):
        """The C batch struct of one call and the arrays it points into (shared input handling: models._new_rows_batch)."""
        from .models import _new_rows_batch
        if W is not None and self.implicit:
            raise ValueError("'W' belongs to the explicit model.")
        b = _new_rows_batch(self._model, X, U, W, dense_ok=not self.implicit)
        s = _lib.NewRowsBatch()
        s.m = b["m_x"]; s.m_u = b["m_u"]
        if b["Xfull"] is not None:
            s.Xfull = b["Xfull"].ctypes.data
        else:
            s.X = b["val"].ctypes.data; s.ixA = b["row"].ctypes.data; s.ixB = b["col"].ctypes.data; s.nnz = len(b["val"])
        if b["W"] is not None:
            s.weight = b["W"].ctypes.data
        if b["U"] is not None:
            s.U = b["U"].ctypes.data
        elif b["Usp"] is not None:
            r, c, v = b["Usp"][:3]
            s.U_row = r.ctypes.data; s.U_col = c.ctypes.data; s.U_sp = v.ctypes.data; s.nnz_U = len(v)
        return s, b, max(b["m_x"], b["m_u"])

    def factors(self, X=None, U=None, W=None, return_bias=False):
        """What ``model.factors_multiple(X, U, W, return_bias)`` returns, bit for bit, without the per-call model work."""
        h = self._live()
        s, keep, rows = self._batch(X, U, W)
        A = np.empty((rows, self.width), self.dtype)
        bias = np.empty(rows, self.dtype) if self.has_bias else None
        rc = self.lib.cmfrec_hip_newrows_factors(h, C.byref(s), _lib.ptr(A), _lib.ptr(bias))
        _lib.check(rc, self.lib, "NewUsers.factors")
        del keep
        if return_bias:
            return A, bias
        return A

    def _topN_raw(self, X, U, W, n, exclude_seen, exclude, want_factors, include=None):
        """(ids, the device's own scores A_u . B_i + biasB_i, A or None, bias or None)."""
        h = self._live()
        s, keep, rows = self._batch(X, U, W)
        n = int(n)
        if exclude is not None and hasattr(exclude, "indptr"):
            exclude = (exclude.indptr, exclude.indices)
        ep, ei = _sorted_exclude(exclude, rows)
        ids = np.empty((rows, n), np.int32); sc = np.empty((rows, n), self.dtype)
        A = np.empty((rows, self.width), self.dtype) if want_factors else None
        bias = np.empty(rows, self.dtype) if self.has_bias else None
        if include is not None:
            cp, ci = _sorted_include(include, rows)
            rc = self.lib.cmfrec_hip_newrows_topN_candidates(h, C.byref(s), _lib.ptr(cp), _lib.ptr(ci), C.c_int(1 if exclude_seen else 0),
                                                             _lib.ptr(ep), _lib.ptr(ei), C.c_int(n), _lib.ptr(ids), _lib.ptr(sc),
                                                             _lib.ptr(A), _lib.ptr(bias))
        else:
            rc = self.lib.cmfrec_hip_newrows_topN(h, C.byref(s), C.c_int(1 if exclude_seen else 0), _lib.ptr(ep), _lib.ptr(ei), C.c_int(n),
                                                  _lib.ptr(ids), _lib.ptr(sc), _lib.ptr(A), _lib.ptr(bias))
        _lib.check(rc, self.lib, "NewUsers.topN")
        del keep
        return ids, sc, A, bias

    def topN(self, X=None, U=None, W=None, n=10, exclude_seen=True, exclude=None, return_factors=False, include=None):
        """(ids [rows, n] int32, scores [rows, n]) for the rows of the batch, ranked on the device from the factors the batch
        run leaves there: descending score, ties by lower id, -1 / -inf where fewer than ``n`` items remain.  ``exclude_seen``
        skips each row's own items of ``X``; ``exclude`` = (indptr, indices) CSR (or a SciPy CSR matrix) over the rows of the
        batch adds further lists.  The scores are those of ``topN_batch``: + the global mean and the new rows' bias for ``CMF``.
        ``return_factors``: a third value, the factors as ``factors(..., return_bias=True)`` returns them (``(A, bias)``; bias
        None without a user bias).  ``include``: candidate lists -- (indptr, indices) CSR over the rows of the batch, a SciPy CSR
        matrix, or one 1-D array shared by every row: each row is ranked over its own list only, minus what ``exclude_seen`` and
        ``exclude`` take out."""
        ids, sc, A, bias = self._topN_raw(X, U, W, n, exclude_seen, exclude, return_factors, include)
        if not self.implicit:                               # as CMF.topN_batch finishes its scores (common.c:5339-5345)
            sc = sc + self._model.glob_mean_
            if bias is not None:
                sc = sc + bias[:, None]
        if return_factors:
            return ids, sc, (A, bias)
        return ids, sc

    def ranks(self, X=None, U=None, W=None, heldout=None, exclude_seen=True, exclude=None, return_factors=False):
        """(indptr, items, ranks, pool) for the rows of the batch and their held-out lists, as ``Ranker.ranks`` on the factors the
        batch run leaves on the device: ``heldout`` = (indptr, indices) CSR over the rows of the batch or a SciPy CSR matrix.
        ``exclude_seen`` / ``exclude`` as in ``topN``: a held-out item among the row's own items of ``X`` or in its list gets -1.
        ``return_factors``: a fifth value, ``(A, bias)`` as ``factors(..., return_bias=True)`` returns them."""
        h = self._live()
        s, keep, rows = self._batch(X, U, W)
        hp, hi = _heldout_lists(heldout, rows, "NewUsers.ranks")
        if exclude is not None and hasattr(exclude, "indptr"):
            exclude = (exclude.indptr, exclude.indices)
        ep, ei = _sorted_exclude(exclude, rows)
        ranks = np.empty(len(hi), np.int32); pool = np.empty(rows, np.int32)
        A = np.empty((rows, self.width), self.dtype) if return_factors else None
        bias = np.empty(rows, self.dtype) if (self.has_bias and return_factors) else None
        rc = self.lib.cmfrec_hip_newrows_ranks(h, C.byref(s), _lib.ptr(hp), _lib.ptr(hi), C.c_int(1 if exclude_seen else 0), _lib.ptr(ep),
                                               _lib.ptr(ei), _lib.ptr(ranks), None, _lib.ptr(pool), _lib.ptr(A), _lib.ptr(bias))
        _lib.check(rc, self.lib, "NewUsers.ranks")
        del keep
        if return_factors:
            return hp.astype(np.int64), hi, ranks, pool, (A, bias)
        return hp.astype(np.int64), hi, ranks, pool

    def impute(self, X, U=None, W=None, return_factors=False):
        """A new array: the dense ``X`` [m, n] with every NaN replaced by the model's prediction for that user and item (reference
        ``CMF.transform``; C function impute_X_collective_explicit), from the factors this batch's rows get -- ``A_r . B_c`` + the
        global mean + the row's bias + the item's bias, computed on the device where ``X`` is missing and nowhere else.  Present
        entries keep their bits; ``X`` itself is not modified.  ``return_factors``: a second value, ``(A, bias)`` as
        ``factors(..., return_bias=True)`` returns them (of a batch without any NaN, which is not solved: None)."""
        h = self._live()
        if self.implicit:
            raise ValueError("imputation belongs to the explicit model")
        if not isinstance(X, np.ndarray):
            raise ValueError("'X' must be a dense array with NaN for the entries to impute")
        s, keep, rows = self._batch(X, U, W)
        out = np.empty_like(keep["Xfull"])
        A = np.empty((rows, self.width), self.dtype) if return_factors else None
        bias = np.empty(rows, self.dtype) if (self.has_bias and return_factors) else None
        rc = self.lib.cmfrec_hip_newrows_impute(h, C.byref(s), _lib.ptr(out), _lib.ptr(A), _lib.ptr(bias))
        _lib.check(rc, self.lib, "NewUsers.impute")
        if return_factors:
            if not np.isnan(keep["Xfull"]).any():
                return out, None
            return out, (A, bias)
        return out

    def predict(self, X=None, U=None, W=None, row=None, item=None, return_factors=False):
        """The predictions [len(row)] for the chosen pairs (row[i], item[i]) of a batch of new users: ``row`` indexes the rows of
        the batch, ``item`` the model's items.  The batch is solved like ``factors``; the pairs are scored on the device from the
        factors it leaves there, the resident items and their bias: ``A_r . B_i`` + the global mean + the row's bias + the item's
        bias for ``CMF`` (a pair outside the batch's rows or the items: the global mean + the bias of the side in range),
        ``A_r . B_i`` for ``CMF_implicit`` (NaN outside).  ``return_factors``: a second value, ``(A, bias)`` as
        ``factors(..., return_bias=True)`` returns them."""
        from .score import check_pairs
        h = self._live()
        if row is None or item is None:
            raise ValueError("NewUsers.predict needs 'row' and 'item'")
        row, item = check_pairs(row, item, "NewUsers.predict")
        s, keep, rows = self._batch(X, U, W)
        out = np.empty(len(row), self.dtype)
        A = np.empty((rows, self.width), self.dtype) if return_factors else None
        bias = np.empty(rows, self.dtype) if (self.has_bias and return_factors) else None
        rc = self.lib.cmfrec_hip_newrows_predict(h, C.byref(s), _lib.ptr(row), _lib.ptr(item), len(row), _lib.ptr(out), _lib.ptr(A),
                                                 _lib.ptr(bias))
        _lib.check(rc, self.lib, "NewUsers.predict")
        del keep
        if return_factors:
            return out, (A, bias)
        return out

    def kernel_ms(self):
        """(solve ms, ranking ms): HIP-event times of the most recent call's solve phase and of its ranking kernel (0 after
        ``factors``; after ``impute``: of its fill kernel; after ``predict``: of its scoring kernel)."""
        a, b = C.c_double(0), C.c_double(0)
        _lib.check(self.lib.cmfrec_hip_newrows_kernel_ms(self._live(), C.byref(a), C.byref(b)), self.lib, "NewUsers.kernel_ms")
        return a.value, b.value

    def close(self):
        if getattr(self, "handle", None):
            self.lib.cmfrec_hip_newrows_destroy(self.handle)
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
