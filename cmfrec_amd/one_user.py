"""The reference's one-user interface -- ``topN``, ``topN_warm``, ``topN_cold``, ``factors_warm``, ``factors_cold``,
``predict_warm``, ``predict_cold`` of ``CMF`` and ``CMF_implicit`` (cmfrec/__init__.py) -- as batches of one on resident handles.

The estimators' methods in models.py are thin: they hand their arguments to the functions here.  A model keeps two handles, made
by the first call that needs them and released by ``fit()``, ``close()`` and at garbage collection: a ``ModelRanker`` over its item
factors and a ``NewUsers`` over the whole model, both with ``split="auto"`` -- the full ranking of one user is cut into item slices
across the device.  With that setting every k is scored by the MFMA kernel: for k <= 64 the scores agree
with ``topN_batch`` up to rounding, not in bits (under ``CMFREC_HIP_TOPN=wide``, and for every k > 64, in bits).

Every argument error is raised before a handle is made, so before any device is touched."""
import numpy as np

from . import _lib

N_MAX = 128                                   # TOPN_NMAX of the ranking kernels
LIMITS = "needs k <= 272 and n_top <= min(128, n)"


def _fitted(model):
    if not getattr(model, "is_fitted_", False):
        raise ValueError("the model is not fitted")


def _check_n(model, n, what):
    """``n`` against the limits of the ranking kernels, with the text the library's return code 2 gives."""
    n = int(n)
    if n < 1 or n > N_MAX or n > model.B_.shape[0]:
        raise RuntimeError("%s failed with code 2 (%s). %s" % (what, _lib.RETURN_CODES[2], LIMITS))
    return n


def _item_list(ids, n_items, name):
    ids = np.asarray(ids).reshape(-1)
    if ids.size and not np.issubdtype(ids.dtype, np.integer):
        raise ValueError("'%s' must hold integer item ids, got %s" % (name, ids.dtype))
    if ids.size and (ids.min() < 0 or ids.max() >= n_items):
        raise ValueError("'%s' has an id outside the model's %d items" % (name, n_items))
    return np.unique(ids.astype(np.int32))


def _include_exclude(model, include, exclude):
    """(include ids or None, exclusion CSR of one row or None); the two together are refused, as in the reference."""
    if include is not None and exclude is not None:
        raise ValueError("Cannot pass both 'include' and 'exclude'.")
    n_items = model.B_.shape[0]
    inc = None if include is None else _item_list(include, n_items, "include")
    if inc is not None and len(inc) == 0:
        raise ValueError("'include' is empty")
    excl = None
    if exclude is not None:
        e = _item_list(exclude, n_items, "exclude")
        excl = (np.array([0, len(e)], np.uint64), e)
    return inc, excl


def _one_row(model, X, X_col, X_val, W, U, U_bin, U_col, U_val, need_X=False):
    """(X, U, W) of a batch of one row, in the forms ``NewUsers`` takes."""
    if U_bin is not None:
        raise ValueError("'U_bin' is not supported for ALS models (the reference takes it with method='lbfgs' only).")
    dt = model.dtype_
    n_items = model.B_.shape[0]
    if X is not None and (X_col is not None or X_val is not None):
        raise ValueError("Cannot pass 'X' together with 'X_col' / 'X_val'.")
    if (X_col is None) != (X_val is None):
        raise ValueError("'X_col' and 'X_val' must be passed together.")
    Xb = Wb = None
    if X is not None:
        X = np.asarray(X, dt).reshape(-1)
        if X.shape[0] != n_items:
            raise ValueError("a dense 'X' must have one entry per item of the model (%d), got %d" % (n_items, X.shape[0]))
        Xb = X.reshape(1, -1)
        if W is not None:
            Wb = np.asarray(W, dt).reshape(1, -1)
    elif X_col is not None:
        col = np.asarray(X_col).reshape(-1)
        val = np.asarray(X_val, dt).reshape(-1)
        if len(col) != len(val):
            raise ValueError("'X_col' and 'X_val' must have the same number of entries.")
        if len(col) and not np.issubdtype(col.dtype, np.integer):
            raise ValueError("'X_col' must hold integer item ids, got %s" % col.dtype)
        if len(col):
            Xb = (np.zeros(len(col), np.int32), col.astype(np.int32), val)
            if W is not None:
                Wb = np.asarray(W, dt).reshape(-1)
    if need_X and Xb is None:
        raise ValueError("Must pass 'X' or 'X_col' + 'X_val'.")
    if U is not None and (U_col is not None or U_val is not None):
        raise ValueError("Cannot pass 'U' together with 'U_col' / 'U_val'.")
    if (U_col is None) != (U_val is None):
        raise ValueError("'U_col' and 'U_val' must be passed together.")
    p = model.C_.shape[0]
    Ub = None
    if U is not None:
        Ub = np.asarray(U, dt).reshape(1, -1)
    elif U_col is not None:
        import scipy.sparse as sp
        ucol = np.asarray(U_col).reshape(-1)
        uval = np.asarray(U_val, dt).reshape(-1)
        if len(ucol) != len(uval):
            raise ValueError("'U_col' and 'U_val' must have the same number of entries.")
        if len(ucol) and (ucol.min() < 0 or ucol.max() >= max(p, 1)):
            raise ValueError("'U_col' has an attribute outside the %d the model was fitted with" % p)
        Ub = sp.coo_matrix((uval, (np.zeros(len(ucol), np.int32), ucol.astype(np.int32))), shape=(1, max(p, 1)))
    if Ub is not None and not p:
        raise ValueError("The model was fitted without user side information.")
    if Xb is None and Ub is None:
        raise ValueError("Must pass at least one of 'X', 'X_col' + 'X_val', 'U', 'U_col' + 'U_val'.")
    return Xb, Ub, Wb


def ranker(model):
    """The model's resident ``ModelRanker`` (``split="auto"``), made by the first call."""
    h = model.__dict__.get("_one_user_ranker")
    if h is None:
        from .models import ModelRanker
        h = ModelRanker(model, model.item_bias_ if getattr(model, "item_bias", False) else None, split="auto")
        model._one_user_ranker = h
    return h


def new_users(model):
    """The model's resident ``NewUsers`` (``split="auto"``), made by the first call."""
    h = model.__dict__.get("_one_user_new")
    if h is None:
        from .new_users import NewUsers
        h = NewUsers(model, split="auto")
        model._one_user_new = h
    return h


def release(model):
    """Closes the model's resident handles (``fit()``, ``close()``)."""
    for name in ("_one_user_ranker", "_one_user_new"):
        h = model.__dict__.pop(name, None)
        if h is not None:
            h.close()


def _result(ids, sc, output_score):
    return (ids[0], sc[0]) if output_score else ids[0]


def topN(model, user, n, include, exclude, output_score):
    _fitted(model)
    n = _check_n(model, n, "topN")
    inc, excl = _include_exclude(model, include, exclude)
    if isinstance(user, (bool, float)) or np.ndim(user) != 0 or int(user) != user:
        raise ValueError("'user' must be one integer user id")
    user = int(user)
    if user < 0 or user >= model.A_.shape[0]:
        raise ValueError("'user' is not a row of the fitted model (%d users)" % model.A_.shape[0])
    users = np.array([user], np.int64)
    A = np.ascontiguousarray(model.A_[users][:, model.k_user:])
    r = ranker(model)._ranker
    ids, sc = r.topN(A, n=n, exclude=excl) if inc is None else r.topN(A, n=n, include=inc)
    return _result(ids, model._finish_scores(users, sc), output_score)


def topN_new(model, n, X, X_col, X_val, W, U, U_bin, U_col, U_val, include, exclude, output_score, need_X):
    _fitted(model)
    n = _check_n(model, n, "topN_warm" if need_X else "topN_cold")
    inc, excl = _include_exclude(model, include, exclude)
    Xb, Ub, Wb = _one_row(model, X, X_col, X_val, W, U, U_bin, U_col, U_val, need_X)
    nu = new_users(model)
    if inc is None:
        ids, sc = nu.topN(X=Xb, U=Ub, W=Wb, n=n, exclude_seen=False, exclude=excl)
    else:
        ids, sc = nu.topN(X=Xb, U=Ub, W=Wb, n=n, exclude_seen=False, include=inc)
    return _result(ids, sc, output_score)


def factors_new(model, X, X_col, X_val, W, U, U_bin, U_col, U_val, return_bias, need_X):
    _fitted(model)
    Xb, Ub, Wb = _one_row(model, X, X_col, X_val, W, U, U_bin, U_col, U_val, need_X)
    nu = new_users(model)
    if return_bias:
        A, bias = nu.factors(X=Xb, U=Ub, W=Wb, return_bias=True)
        return A[0], (bias[0] if bias is not None else 0.)
    return nu.factors(X=Xb, U=Ub, W=Wb)[0]


def predict_new(model, items, X, X_col, X_val, W, U, U_bin, U_col, U_val, need_X):
    _fitted(model)
    items = np.asarray(items).reshape(-1)
    if items.size and not np.issubdtype(items.dtype, np.integer):
        raise ValueError("'items' must hold integer item ids, got %s" % items.dtype)
    Xb, Ub, Wb = _one_row(model, X, X_col, X_val, W, U, U_bin, U_col, U_val, need_X)
    return new_users(model).predict(X=Xb, U=Ub, W=Wb, row=np.zeros(len(items), np.int64), item=items)
