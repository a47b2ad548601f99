"""float64 NumPy restatement of factors_implicit_cg (src/common.c:1932-1985), one half-step (tests/test_gpu_implicit_cg_wide.py)."""
import numpy as np


def compressed(key, other, val, nrows):          # (indptr, indices, values) of the rows `key`, entries in their given order
    order = np.argsort(key, kind="stable")
    return np.concatenate([[0], np.cumsum(np.bincount(key, minlength=nrows))]), np.asarray(other)[order], np.asarray(val, np.float64)[order]


def first_residual_roots(opp, indptr, indices, values, lam):
    """Per row the point where the reference's FIRST residual r0(a) = sum x_j B_j - (BtB + lam I + sum (x_j + 1) B_j B_j^T) a vanishes
    (quirk Q1: not the closed-form half-step's solution, which has the two weights the other way round); no entries: zeros."""
    B = np.asarray(opp, np.float64)
    out = np.zeros((len(indptr) - 1, B.shape[1]))
    for i in np.flatnonzero(np.diff(indptr)):
        Bj, x = B[indices[indptr[i]:indptr[i + 1]]], values[indptr[i]:indptr[i + 1]]
        out[i] = np.linalg.solve(B.T @ B + lam * np.eye(B.shape[1]) + (Bj.T * (x + 1.0)) @ Bj, Bj.T @ x)
    return out


def implicit_cg_half_step(F, opp, indptr, indices, values, lam, max_cg_steps):
    """F after one half-step against the fixed factors `opp`; rows without entries stay as they are."""
    F, B = np.array(F, np.float64), np.asarray(opp, np.float64)
    BtB = B.T @ B
    for i in np.flatnonzero(np.diff(indptr)):
        Bj, x, a = B[indices[indptr[i]:indptr[i + 1]]], values[indptr[i]:indptr[i + 1]], F[i]
        coef = Bj @ a
        r = -(BtB @ a) + Bj.T @ (-(coef - 1.0) * x - coef) - lam * a          # :1932-1943
        p, r_old = r.copy(), r @ r
        if r_old <= 1e-12:                                                    # :1952
            continue
        for _ in range(max_cg_steps):
            coef = Bj @ p
            Ap = BtB @ p + Bj.T @ (coef * (x - 1.0) + coef) + lam * p         # :1958-1969
            alpha = r_old / (Ap @ p)
            a += alpha * p                                                    # (a view of F's row)
            r -= alpha * Ap
            r_new = r @ r
            if r_new <= 1e-8:                                                 # :1979
                break
            p, r_old = p * (r_new / r_old) + r, r_new
    return F
