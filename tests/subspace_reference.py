"""NumPy float64 restatement of the subspace (iALS++) half-step (subspace_kernels.hpp).

A row's system is W a = r, W = G0 + D + sum_j g_j b_j b_j', r = sum_j y_j b_j.  With yhat = Bh a kept per entry, the step on the block
pi of 16 consecutive unknowns is  grad = G0[pi, :] a + D_pi a_pi + Bh[:, pi]' (g * yhat - y)  ( = (W a - r)[pi] ),
H = G0[pi, pi] + D_pi + Bh[:, pi]' diag(g) Bh[:, pi]  ( = W[pi, pi] ),  d = -H^-1 grad,  a_pi += d,  yhat += Bh[:, pi] d."""
import numpy as np

from topn_reference import gamma


def row_terms(B, idx, val, implicit, bias_sub):
    """(Bh, g, y) of a row in float64: the gathered opposing rows, the rank-1 weights, the targets."""
    Bh, x = np.asarray(B, np.float64)[idx], np.asarray(val, np.float64)
    if implicit:
        return Bh, x, x + 1.0
    return Bh, np.ones(len(x)), x - (0.0 if bias_sub is None else np.asarray(bias_sub, np.float64)[idx])


def row_system(B, idx, val, diag, implicit, bias_sub=None, G0=None):
    """(W, r) of the closed form."""
    Bh, g, y = row_terms(B, idx, val, implicit, bias_sub)
    W = np.diag(diag) + (Bh * g[:, None]).T @ Bh + (0.0 if G0 is None else G0)
    return W, Bh.T @ y


def half_step(A, B, csr, diag, implicit, sweeps, dtype, bias_sub=None):
    """Every row of A [rows, k] with entries after `sweeps` passes over its blocks, and per row the test's bound
    blocks * sweeps * gamma_m * max_pi cond_2(H_pi) * |a|_2, m = entries + 16 + k (+ rows of B, implicit), |a|_2 the largest norm
    the row's iterate takes from its start value on.  diag [k]: D; G0 = B'B for the implicit model."""
    indptr, indices, values = csr
    A = np.array(A, np.float64)
    k = A.shape[1]
    G0 = np.asarray(B, np.float64).T @ np.asarray(B, np.float64) if implicit else np.zeros((k, k))
    bound = np.zeros(len(A))
    for u in range(len(A)):
        s = slice(int(indptr[u]), int(indptr[u + 1]))
        if s.stop == s.start:
            continue
        Bh, g, y = row_terms(B, indices[s], values[s], implicit, bias_sub)
        a, cond = A[u], 0.0
        big = np.linalg.norm(a)         # the step subtracts H^-1 (W a - r) from a: its rounding scales with the iterate it starts from
        yhat = Bh @ a
        for _ in range(sweeps):
            for p0 in range(0, k, 16):
                pi = slice(p0, min(p0 + 16, k))
                grad = G0[pi] @ a + diag[pi] * a[pi] + Bh[:, pi].T @ (g * yhat - y)
                H = G0[pi, pi] + np.diag(diag[pi]) + (Bh[:, pi] * g[:, None]).T @ Bh[:, pi]
                d = -np.linalg.solve(H, grad)
                a[pi] += d
                yhat += Bh[:, pi] @ d
                cond, big = max(cond, np.linalg.cond(H)), max(big, np.linalg.norm(a))
        # the chain of one block step: the row's entries, the 16 x 16 solve, G0[pi, :] a over k -- and, for the implicit model, the
        # n rows of B that the device's Gramian sums in the working precision before the step reads it (G0 is exact here)
        chain = len(g) + 16 + k + (len(B) if implicit else 0)
        bound[u] = -(-k // 16) * sweeps * gamma(chain, dtype) * cond * big
    return A, bound
