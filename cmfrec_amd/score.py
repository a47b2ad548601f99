"""Predictions for chosen (user, item) pairs with both factor matrices resident on the device: ``Scorer`` wraps the
``cmfrec_hip_scorer_*`` handle of include/cmfrec_hip.h.  The evaluation loop after a fit -- millions of held-out pairs against
one model -- uploads the factors once and then only moves the pairs up and the predictions down.  ``EvalSet`` keeps held-out
pairs and their values on the device as well: ``Scorer.errors`` / ``AlsSession.errors`` then reduce the squared and absolute
error there and bring one record down."""
import ctypes as C

import numpy as np

from . import _lib


def check_pairs(row, col, what="predict"):
    """``row`` / ``col`` as the contiguous int32 arrays the library reads: 1-D, integer, of one length, within int32 (an index
    beyond either side is a legal pair -- it gets the fallback value -- but it must be representable)."""
    row = np.asarray(row); col = np.asarray(col)
    for name, a in (("row", row), ("col", col)):
        if a.ndim != 1:
            raise ValueError("%s: '%s' must be 1-D, got %d-D" % (what, name, a.ndim))
        if a.dtype.kind not in "iu":
            raise ValueError("%s: '%s' must hold integers, got %s" % (what, name, a.dtype))
    if len(row) != len(col):
        raise ValueError("%s: 'row' and 'col' must have one length, got %d and %d" % (what, len(row), len(col)))
    for name, a in (("row", row), ("col", col)):
        if a.dtype != np.int32 and len(a) and (a.max() > np.iinfo(np.int32).max or a.min() < np.iinfo(np.int32).min):
            raise ValueError("%s: '%s' does not fit 32-bit indices" % (what, name))
    return np.ascontiguousarray(row, np.int32), np.ascontiguousarray(col, np.int32)


def _check_factors(A, B, biasA, biasB):
    A = np.asarray(A); B = np.asarray(B)
    for name, M in (("A", A), ("B", B)):
        if M.ndim != 2:
            raise ValueError("Scorer: %s must be 2-D [rows, factors], got %d-D" % (name, M.ndim))
    if A.dtype.type not in (np.float64, np.float32):
        raise ValueError("Scorer: A must be float64 or float32, got %s" % A.dtype)
    if B.dtype != A.dtype:
        raise ValueError("Scorer: B is %s, A is %s" % (B.dtype, A.dtype))
    if A.shape[1] != B.shape[1]:
        raise ValueError("Scorer: A has %d factors, B has %d" % (A.shape[1], B.shape[1]))
    if A.shape[0] < 1 or B.shape[0] < 1:
        raise ValueError("Scorer: A or B is empty")
    out = []
    for name, b, M in (("biasA", biasA, A), ("biasB", biasB, B)):
        if b is not None:
            b = np.asarray(b)
            if b.dtype != A.dtype:
                raise ValueError("Scorer: %s is %s, A is %s" % (name, b.dtype, A.dtype))
            if b.shape != (M.shape[0],):
                raise ValueError("Scorer: %s must have one entry per row (%d), got shape %s" % (name, M.shape[0], b.shape))
            b = np.ascontiguousarray(b)
        out.append(b)
    return A, B, out[0], out[1]


def check_heldout(row, col, x, w, dtype, what="EvalSet"):
    """(row, col, x, w) as the contiguous arrays an evaluation set uploads: the indices through ``check_pairs``, ``x`` and
    ``w`` (or None) 1-D of the pairs' length in ``dtype``; a weight must be finite and >= 0 (NaN in ``x`` is legal: the pair is
    skipped)."""
    dtype = np.dtype(dtype)
    if dtype.type not in (np.float64, np.float32):
        raise ValueError("%s: dtype must be float64 or float32, got %s" % (what, dtype))
    row, col = check_pairs(row, col, what)
    out = []
    for name, a in (("x", x), ("w", w)):
        if a is None and name == "w":
            out.append(None)
            continue
        a = np.asarray(a)
        if a.ndim != 1:
            raise ValueError("%s: '%s' must be 1-D, got %d-D" % (what, name, a.ndim))
        if len(a) != len(row):
            raise ValueError("%s: '%s' must have one entry per pair (%d), got %d" % (what, name, len(row), len(a)))
        if a.dtype.kind not in "fiu":
            raise ValueError("%s: '%s' must hold numbers, got %s" % (what, name, a.dtype))
        out.append(np.ascontiguousarray(a, dtype))
    x, w = out
    if w is not None and len(w) and not (np.isfinite(w).all() and (w >= 0).all()):
        raise ValueError("%s: a weight is negative, NaN or infinite" % what)
    return row, col, x, w


class EvalSet:
    """``EvalSet(row, col, x, w=None, dtype=np.float64, sort=True, device=-1)``: held-out pairs (row[i], col[i]) with their values
    ``x`` and optional weights ``w`` (finite, >= 0), uploaded once and resident on the device (``cmfrec_hip_evalset_*`` of
    include/cmfrec_hip.h) for ``Scorer.errors`` / ``AlsSession.errors`` of the same dtype.  An index outside the model is legal
    (the pair counts as a fallback pair, or is skipped under the implicit rule), and so is a NaN ``x`` (skipped).  ``sort``: the set
    is reordered by ``row`` (stable) before the upload -- its order is free, and pairs sorted by user are scored faster.  The
    caller owns the handle: ``close()`` it, or use it as a context manager."""

    def __init__(self, row, col, x, w=None, dtype=np.float64, sort=True, device=-1):
        self.handle = None
        row, col, x, w = check_heldout(row, col, x, w, dtype)
        if sort and len(row):
            order = np.argsort(row, kind="stable")
            row, col, x = row[order], col[order], x[order]
            w = None if w is None else w[order]
        self.dtype = np.dtype(dtype)
        self.n_pairs = len(row)
        self.lib = _lib.load(self.dtype)
        h = self.lib.cmfrec_hip_evalset_create(_lib.ptr(row), _lib.ptr(col), _lib.ptr(x), _lib.ptr(w), self.n_pairs, int(device))
        if not h:
            _lib.check(self.lib.cmfrec_hip_last_error_code() or 4, self.lib, "EvalSet")
        self.handle = C.c_void_p(h)

    def _live(self):
        if not getattr(self, "handle", None):
            raise RuntimeError("EvalSet: the handle is closed")
        return self.handle

    def _for(self, dtype, what):
        """The live handle, for an evaluation against factors of ``dtype``."""
        h = self._live()
        if np.dtype(dtype) != self.dtype:
            raise ValueError("%s: the evaluation set is %s, the factors are %s" % (what, self.dtype, np.dtype(dtype)))
        return h

    def kernel_ms(self):
        """HIP-event time (ms) of both kernels of the most recent evaluation of this set."""
        ms = C.c_double(0)
        _lib.check(self.lib.cmfrec_hip_evalset_kernel_ms(self._live(), C.byref(ms)), self.lib, "EvalSet.kernel_ms")
        return ms.value

    def launch_waves(self):
        """Wavefronts of the scoring launch of the most recent evaluation of this set (what ``CMFREC_HIP_EVAL_WAVES`` caps)."""
        waves = C.c_size_t(0)
        _lib.check(self.lib.cmfrec_hip_evalset_launch_waves(self._live(), C.byref(waves)), self.lib, "EvalSet.launch_waves")
        return waves.value

    def close(self):
        if getattr(self, "handle", None):
            self.lib.cmfrec_hip_evalset_destroy(self.handle)
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


class Scorer:
    """``Scorer(A, B, biasA=None, biasB=None, glob_mean=0.0, implicit=False)``: A [m, kk] and B [n, kk] of one dtype (float64 or
    float32; row-strided views such as ``model.A_[:, k_user:]`` are taken as they are), the biases [m] / [n] or None.
    ``predict(row, col)`` returns, per pair,

        explicit:  A[row] . B[col] + biasA[row] + biasB[col] + glob_mean, and for a pair outside [0, m) x [0, n)
                   glob_mean + the bias of the side that is in range
        implicit:  A[row] . B[col], and NaN for a pair outside (biases and ``glob_mean`` are ignored, given or not).

    The caller owns the handle: ``close()`` it, or use it as a context manager."""

    def __init__(self, A, B, biasA=None, biasB=None, glob_mean=0.0, implicit=False, device=-1):
        self.handle = None
        A, B, biasA, biasB = _check_factors(A, B, biasA, biasB)
        sz = A.dtype.itemsize
        # a view whose rows are contiguous goes up as it is (its row pitch is the leading dimension); anything else is copied
        A, B = [M if (M.strides[1] == sz and M.strides[0] % sz == 0 and M.strides[0] >= M.shape[1] * sz) else np.ascontiguousarray(M)
                for M in (A, B)]
        self.dtype = A.dtype
        self.m, self.kk = A.shape
        self.n = B.shape[0]
        self.implicit = bool(implicit)
        self.lib = _lib.load(A.dtype)
        h = self.lib.cmfrec_hip_scorer_create(_lib.ptr(A), A.strides[0] // sz, self.m, _lib.ptr(B), B.strides[0] // sz, self.n, self.kk,
                                              _lib.ptr(biasA), _lib.ptr(biasB), float(glob_mean), int(self.implicit), int(device))
        if not h:
            _lib.check(self.lib.cmfrec_hip_last_error_code() or 4, self.lib, "Scorer")
        self.handle = C.c_void_p(h)

    def _live(self):
        if not getattr(self, "handle", None):
            raise RuntimeError("Scorer: the handle is closed")
        return self.handle

    def predict(self, row, col):
        """The predictions [len(row)] for the pairs (row[i], col[i]), scored on the device."""
        h = self._live()
        row, col = check_pairs(row, col, "Scorer.predict")
        out = np.empty(len(row), self.dtype)
        rc = self.lib.cmfrec_hip_scorer_predict(h, _lib.ptr(row), _lib.ptr(col), len(row), _lib.ptr(out))
        _lib.check(rc, self.lib, "Scorer.predict")
        return out

    def errors(self, evalset):
        """The error record of this model's predictions on a resident ``EvalSet`` (``cmfrec_hip_errors``, include/cmfrec_hip.h),
        reduced on the device: a dict of ``n`` [2] (scored, fallback pairs), ``n_skipped``, and per class ``sum_w``, ``sum_we``,
        ``sum_wabs``, ``sum_wsq``, ``max_abs`` (float64 [2]).  ``cmfrec_amd.metrics.error_metrics`` turns it into RMSE, MAE ..."""
        h = self._live()
        if not isinstance(evalset, EvalSet):
            raise TypeError("Scorer.errors: an EvalSet is required")
        rec = _lib.Errors()
        rc = self.lib.cmfrec_hip_scorer_errors(h, evalset._for(self.dtype, "Scorer.errors"), C.byref(rec))
        _lib.check(rc, self.lib, "Scorer.errors")
        return rec.as_dict()

    def kernel_ms(self):
        """HIP-event time (ms) of the scoring kernel over the blocks of the most recent ``predict`` call."""
        ms = C.c_double(0)
        _lib.check(self.lib.cmfrec_hip_scorer_kernel_ms(self._live(), C.byref(ms)), self.lib, "Scorer.kernel_ms")
        return ms.value

    def close(self):
        if getattr(self, "handle", None):
            self.lib.cmfrec_hip_scorer_destroy(self.handle)
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
