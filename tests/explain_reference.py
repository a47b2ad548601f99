"""Plain NumPy reference of Ranker.explain: per user W_u = G0 + diag + sum_j g_j b_j b_j' in float64
(np.longdouble for the double-precision cases), c_tj = y_j b_t' W_u^-1 b_j through np.linalg.solve.

The bound per value is gamma_m cond_2(W_u) max_j |c_tj| with m the lengths of the steps the kernel chains, the constants of
dense_reference.py: potrf n + 1, two triangular solves n each, the rank-k accumulation over the h history rows as a GEMM of that
length (h + ceil(h / 256) + 2) and the product of a history row with the solution, a GEMM of length n."""
import numpy as np

from topn_reference import gamma


def explain(B, hist, targ, G0, diag, diag_u, bias_diag, dtype):
    """hist = (indptr, items, g, y), targ = (indptr, items); bias_diag None: no bias unknown, a number or one per user.  Returns per user a dict with
    c [targets, history], total [targets], direct [targets] (= b_t . a_u), bound [targets]; None for a user whose W_u is not
    positive definite."""
    wide = np.longdouble if np.dtype(dtype) == np.float64 else np.float64
    hp, hi, hg, hy = hist
    tp, ti = targ
    Bx = np.asarray(B, wide)
    if bias_diag is not None:
        Bx = np.concatenate([Bx, np.ones((len(Bx), 1), wide)], axis=1)
    n = Bx.shape[1]
    out = []
    for u in range(len(hp) - 1):
        h = slice(int(hp[u]), int(hp[u + 1]))
        Bh, g, y = Bx[hi[h]], np.asarray(hg[h], wide), np.asarray(hy[h], wide)
        Bt = Bx[ti[int(tp[u]):int(tp[u + 1])]]
        d = np.full(n, diag if diag_u is None else diag_u[u], wide)
        if bias_diag is not None:
            d[-1] = bias_diag[u] if np.ndim(bias_diag) else bias_diag
        W = np.diag(d) + (Bh * g[:, None]).T @ Bh
        if G0 is not None:
            W = W + np.asarray(G0, wide)
        W64 = W.astype(np.float64)
        if np.linalg.eigvalsh(W64).min() <= 0:
            out.append(None)
            continue
        Z = np.linalg.solve(W64, Bt.T.astype(np.float64)).astype(wide)
        Z = Z + np.linalg.solve(W64, (Bt.T - W @ Z).astype(np.float64))          # one refinement step in the wide type
        c = (Bh @ Z).T * y[None, :]
        a = np.linalg.solve(W64, ((Bh * y[:, None]).sum(0)).astype(np.float64))
        m = (n + 1) + 2 * n + (len(g) + (len(g) + 255) // 256 + 2) + (n + 2)
        big = np.abs(c).max(axis=1) if c.shape[1] else np.zeros(len(Bt))
        out.append(dict(c=c.astype(np.float64), total=c.sum(axis=1).astype(np.float64), direct=Bt.astype(np.float64) @ a,
                        bound=gamma(m, dtype) * np.linalg.cond(W64) * big.astype(np.float64)))
    return out
