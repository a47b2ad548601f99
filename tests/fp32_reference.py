"""Single-precision kernels against a float64 reference, row by row (helpers, no tests).

Every case below draws its inputs in float32.  Three answers are computed on exactly those inputs: `a64` by the float64
oracle on the exact upcasts (same operation, same start, same number of CG steps), `ao` by the float32 oracle and `ah` by the
HIP float32 build.  Two criteria:

- forward, every row: with s_r = max(|a64_r|_inf, 1e-6 max|a64|) and e_x,r = |x_r - a64_r|_inf / s_r, e_h,r <= 4 e_o,r + TAU.
  (Against the float32 oracle the suite allowed 1e-3 per row; what float32 arithmetic costs here is 4e-7 .. 4e-6 per row.)
- backward, every row of a closed-form route: the row's normal equations M a = b formed in plain numpy float64 from the
  upcast inputs (independent of the oracle's C code), eta_r = ||M a - b|| / (||M|| ||a|| + ||b||) <= ETA_MAX = 32 * 2^-24.

The mutations are what a subtly wrong kernel would compute; tests/test_fp32_bound_sensitivity.py shows that both criteria
reject each of them on every case the GPU file runs (tests/test_gpu_single_precision.py)."""
import ctypes as C
import functools
import os

import numpy as np

TAU = 1e-5
ETA_MAX = 32 * 2.0 ** -24
REJECT_MARGIN = 5.0
# Routes legitimately less accurate than 4 e_o + TAU, measured against float64 on the MI355X (the backward errors of the same
# runs are at the oracle's level, 0.02 - 0.03 x ETA_MAX):
# - the shared-matrix solves (NA_as_zero_X, implicit features) at cond(M) ~ 9e3: a backward-stable solve is only forward
#   accurate to cond(M) eps ~ 5e-4, in a direction of its own; HIP 2.1e-4 / 1.7e-4 at the worst row against oracle 1.3e-5 there.
TAU_SHARED = 5e-4
# - explicit-model CG on rows of at most two entries: the system (rank <= 2 plus the ridge) is solved before the third step,
#   which then divides roundoff by roundoff; HIP 1.3e-4 on a one-entry row at k = 100 with weights (oracle 2.7e-5).
TAU_CONVERGED_CG = 1e-3
# The shared-matrix solves are held to a tighter backward bound instead: one factorisation and the refinement step put HIP at
# 0.03 x ETA_MAX (oracle 0.02), while the unrefined explicit inverse reaches 0.8 x ETA_MAX on the implicit-features case --
# under ETA_MAX, over ETA_SHARED.
ETA_SHARED = 4 * 2.0 ** -24

LADDER = list(range(0, 151)) + [160, 161, 192, 193, 256, 257, 511, 512, 513, 577, 1000, 1024, 1025, 2047, 2048, 2049, 4500]
VH_MIN_F32 = 1025                       # first split row in single precision (device.hpp: BIN_MIN_NNZ of the split bin)
GRAM_SLICE = 2048                       # device.hpp: split rows take 2048-entry slices once they hold GRAM_SLICE * 1024 entries


def slice_len(lens):
    """The split rows' slice length of a shard (device.hpp, where slice_len is set): 256 below 2048 * 1024 entries."""
    vh_total = sum(int(l) for l in lens if l >= VH_MIN_F32)
    return 256 if vh_total < GRAM_SLICE * 1024 else GRAM_SLICE


def _log(tag, value, dtype="float32"):
    """Appends the worst ratio of a check to CMFREC_TEST_RELERR_LOG (conftest.rel_err's format, with a tag like row_rel_err)."""
    log = os.environ.get("CMFREC_TEST_RELERR_LOG")
    if log:
        with open(log, "a") as f:
            f.write("%s %s %s %.3e\n" % (os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0], dtype, tag, value))


# ---- the two criteria --------------------------------------------------------------------------------------------------

def row_errors(x, a64, floor=1e-6):
    """e_r = |x_r - a64_r|_inf / max(|a64_r|_inf, floor * max|a64|), one number per row."""
    x = np.asarray(x, np.float64).reshape(len(x), -1)
    a64 = np.asarray(a64, np.float64).reshape(len(a64), -1)
    scale = np.maximum(np.abs(a64).max(axis=1), floor * max(float(np.abs(a64).max()), 1e-300))
    return np.abs(x - a64).max(axis=1) / scale


def tau_rows(case):
    """TAU per row of a case (see TAU_SHARED / TAU_CONVERGED_CG)."""
    lens = np.asarray(case["lens"])
    t = np.full(len(lens), TAU)
    if case["route"] in ("naz", "impfeat"):
        t[:] = TAU_SHARED
    elif case["route"] == "explicit" and case["use_cg"]:
        t[lens <= 2] = TAU_CONVERGED_CG
    return t


def forward_ratios(x, ao, a64, tau=TAU):
    """e_x,r / (4 e_o,r + tau) per row, with the bound itself."""
    bound = 4.0 * row_errors(ao, a64) + tau
    return row_errors(x, a64) / bound, bound


def check_forward(ah, ao, a64, lens=None, tau=TAU, what=""):
    """Asserts e_h,r <= 4 e_o,r + tau for every row; logs and returns the worst e_h / bound."""
    eh, eo = row_errors(ah, a64), row_errors(ao, a64)
    bound = 4.0 * eo + tau
    ratio = eh / bound
    worst = int(np.argmax(ratio))
    _log("fp64-fwd", float(ratio[worst]))
    bad = np.nonzero(~(ratio <= 1.0))[0]                       # (NaN fails too)
    assert len(bad) == 0, "%s: %d rows over the float64 bound; row %d (%s entries): e_h %.3e, e_o %.3e, bound %.3e" % (
        what, len(bad), bad[0], "?" if lens is None else int(lens[bad[0]]), eh[bad[0]], eo[bad[0]], bound[bad[0]])
    return float(ratio[worst])


def backward_errors(a, M, b):
    """eta_r = ||M_r a_r - b_r||_2 / (||M_r||_2 ||a_r||_2 + ||b_r||_2) for stacked systems M [rows, k, k], b [rows, k]."""
    a = np.asarray(a, np.float64)
    res = np.linalg.norm(np.einsum("rij,rj->ri", M, a) - b, axis=1)
    nM = np.abs(np.linalg.eigvalsh(M)).max(axis=1)
    den = nM * np.linalg.norm(a, axis=1) + np.linalg.norm(b, axis=1)
    return np.where(den > 0, res / np.where(den > 0, den, 1.0), np.where(res > 0, np.inf, 0.0))


def eta_max(case):
    return ETA_SHARED if case["route"] in ("naz", "impfeat") else ETA_MAX


def check_backward(a, system, lens=None, what="", bound=ETA_MAX):
    """Asserts eta_r <= bound on the rows of `system` = (row ids, M, b); logs and returns the worst eta / bound."""
    rows, M, b = system
    eta = backward_errors(np.asarray(a, np.float64)[rows], M, b)
    ratio = eta / bound
    worst = int(np.argmax(ratio)) if len(ratio) else 0
    w = float(ratio[worst]) if len(ratio) else 0.0
    _log("fp64-bwd", w)
    bad = np.nonzero(~(ratio <= 1.0))[0]
    assert len(bad) == 0, "%s: %d rows over the backward bound %.2e; row %d (%s entries): eta %.3e" % (
        what, len(bad), bound, rows[bad[0]], "?" if lens is None else int(lens[rows[bad[0]]]), eta[bad[0]])
    return w


# ---- normal equations in plain float64 -----------------------------------------------------------------------------------

def _row_systems(csr, B, rows, diag_of_row, coef_M, coef_b, shared=None):
    """M_r = shared + sum_j coef_M_j b_j b_j^T + diag(diag_of_row(r)), b_r = sum_j coef_b_j b_j over the row's entries."""
    p, i = csr[0].astype(np.int64), csr[1]
    B = np.asarray(B, np.float64)
    k = B.shape[1]
    M = np.empty((len(rows), k, k)); b = np.empty((len(rows), k))
    for q, r in enumerate(rows):
        sl = slice(p[r], p[r + 1])
        Bs = B[i[sl]]
        M[q] = (Bs.T * coef_M[sl]) @ Bs if coef_M is not None else 0.0
        if shared is not None:
            M[q] += shared
        M[q][np.diag_indices(k)] += diag_of_row(r)
        b[q] = coef_b[sl] @ Bs
    return np.asarray(rows), M, b


def implicit_system(case):
    """iALS: M = B^T B + lam I + sum_j x_j b_j b_j^T, b = sum_j (1 + x_j) b_j (every row: the empty ones solve to zero)."""
    csr, B = case["csr"], case["B"].astype(np.float64)
    x = csr[2].astype(np.float64)
    rows = np.arange(len(csr[0]) - 1)
    lam = case["lam"]
    return _row_systems(csr, B, rows, lambda r: lam, x, 1.0 + x, shared=B.T @ B)


def explicit_system(case):
    """Explicit model on sparse X, rows with entries: M = sum_j w_j b_j b_j^T + diag(lam_r, .., lam_r, lam_last_r),
    b = sum_j w_j (x_j - bias_j) b_j; under scale_lam both lambdas times the row's number of entries (its sum of weights)."""
    csr, B, k = case["csr"], case["B"].astype(np.float64), case["k"]
    x = csr[2].astype(np.float64) - case["bias"].astype(np.float64)[csr[1]]
    w = np.ones(len(x)) if case.get("weight") is None else case["weight"].astype(np.float64)
    p = csr[0].astype(np.int64)
    rows = np.nonzero(np.diff(p) > 0)[0]
    if case.get("weight") is None:
        mult = np.diff(p).astype(np.float64)
    else:
        mult = case["wsum"].astype(np.float64)
    lam, lam_last = case["lam"], case["lam_last"]

    def diag(r):
        s = mult[r] if case["scale_lam"] else 1.0
        d = np.full(k, lam * s); d[-1] = lam_last * s
        return d
    return _row_systems(csr, B[:, :k], rows, diag, w, w * x)


def naz_system(case):
    """NA_as_zero_X (and the implicit features, x = 1): M = B^T B + lam I shared, b = sum_j x_j b_j, every row."""
    csr, B = case["csr"], case["B"].astype(np.float64)
    x = np.ones(len(csr[1])) if case["route"] == "impfeat" else csr[2].astype(np.float64)
    rows = np.arange(len(csr[0]) - 1)
    lam = case["lam_eff"]
    Mk = B.T @ B + lam * np.eye(B.shape[1])
    return _row_systems(csr, B, rows, lambda r: 0.0, None, x, shared=Mk)


def dense_system(case):
    """Dense X (optimizeA Case 1, no scaling): M = B^T B + lam I shared, b_r = sum_j X_rj b_j."""
    B, X = case["B"].astype(np.float64), case["X"].astype(np.float64)
    k = B.shape[1]
    Mk = B.T @ B + case["lam"] * np.eye(k)
    b = X @ B
    return np.arange(len(X)), np.broadcast_to(Mk, (len(X), k, k)), b


SYSTEMS = {"implicit": implicit_system, "explicit": explicit_system, "naz": naz_system, "impfeat": naz_system,
           "dense": dense_system}


def closed_form(case):
    return case["route"] in ("naz", "impfeat", "dense") or (case["route"] in ("implicit", "explicit") and not case["use_cg"])


# ---- running a case ----------------------------------------------------------------------------------------------------

def _oracle_naz(O, A, B, csr, lam, values=True, nthreads=4):
    """oracle_optimizeA_naz (cmf_oracle.c): the shared-matrix Cholesky solve of NA_as_zero_X; values=False: x = 1."""
    m, lda = A.shape
    n, ldb = B.shape
    p = np.ascontiguousarray(csr[0], np.uint64); i = np.ascontiguousarray(csr[1], np.int32)
    v = np.ascontiguousarray(csr[2], O.dtype) if values else None
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    O.lib.oracle_optimizeA_naz(ptr(A), C.c_size_t(lda), ptr(B), C.c_size_t(ldb), C.c_int(m), C.c_int(n), C.c_int(ldb),
                               ptr(p), ptr(i), ptr(v), O._r(lam), O._r(lam), C.c_bool(False), C.c_int(nthreads))


def run_oracle(case, O, nthreads=4, csr=None, B=None):
    """The case's operation by oracle O (float64 or float32) on the case's inputs cast to O's type; csr / B replace them
    (the mutations).  Returns the updated A."""
    dt = O.dtype
    csr = case.get("csr") if csr is None else csr
    B = (case["B"] if B is None else B).astype(dt)
    A = np.ascontiguousarray(case["A0"].astype(dt))
    route = case["route"]
    if csr is not None:
        csr = (csr[0], csr[1], csr[2].astype(dt))
    if route == "implicit":
        O.optimizeA_implicit(A, B, csr, case["lam"], nthreads=nthreads, use_cg=case["use_cg"], max_cg_steps=3)
    elif route == "explicit":
        x = csr[2].astype(dt) - case["bias"].astype(dt)[csr[1]]           # float32: rounded like the reference's host sweep
        kw = dict(k=case["k"], lam_last=case["lam_last"], scale_lam=case["scale_lam"], use_cg=case["use_cg"], max_cg_steps=3)
        if case.get("weight") is not None:
            kw.update(weight=case["weight_of"](csr).astype(dt), wsum=case["wsum"].astype(dt))
        O.optimizeA_explicit(A, B, (csr[0], csr[1], x), case["lam"], nthreads=nthreads, **kw)
    elif route in ("naz", "impfeat"):
        _oracle_naz(O, A, B, csr, case["lam_eff"], values=route == "naz", nthreads=nthreads)
    elif route == "dense":
        O.optimizeA_dense_full(A, B, case["X"].astype(dt), case["lam"], nthreads=nthreads)
    elif route == "collective":
        O.optimizeA_collective_chol(A, B, case["Cm"].astype(dt), csr, case["U"].astype(dt), case["lam"], nthreads=nthreads,
                                    **case["kw"])
    elif route == "collective_sparse":
        u = case["U_csr"]
        O.optimizeA_collective_sparse(A, B, case["Cm"].astype(dt), csr, (u[0], u[1], u[2].astype(dt)), case["lam"],
                                      nthreads=nthreads, **case["kw"])
    else:
        raise ValueError(route)
    return A


def run_hip(case):
    """The case's operation by the HIP float32 build (operator entry points, or a session for the shared-matrix solves)."""
    from cmfrec_amd import ops
    route = case["route"]
    A = case["A0"].copy()
    B, csr = case["B"], case.get("csr")
    if route == "implicit":
        ops.optimizeA_implicit(A, B, csr, case["lam"], use_cg=case["use_cg"], max_cg_steps=3)
    elif route == "explicit":
        kw = dict(k=case["k"], lam_last=case["lam_last"], scale_lam=case["scale_lam"], use_cg=case["use_cg"], max_cg_steps=3)
        if case.get("weight") is not None:
            kw.update(weight=case["weight"], wsum=case["wsum"])
        ops.optimizeA_explicit(A, B, csr, case["lam"], bias_sub=case["bias"], **kw)
    elif route in ("naz", "impfeat"):
        from cmfrec_amd.session import AlsSession
        m, n, k = A.shape[0], B.shape[0], B.shape[1]
        p, i, v = csr
        row = np.repeat(np.arange(m, dtype=np.int32), np.diff(p.astype(np.int64)))
        s = AlsSession(m, n, k, implicit=False, dtype=np.float32, lam=case["lam"], use_cg=False)
        try:
            s.set_X_coo(row, i, v)
            if route == "naz":
                s.set_NA_as_zero_X(True)
                s.set_factors(A=A, B=B)
                s.update("A", use_cholesky=True)
                A = s.get_factors()["A"].copy()
            else:
                s.set_factors(A=np.zeros_like(A), B=B)
                s.set_implicit_features(case["w_implicit"], Ai=A, Bi=np.zeros((n, k), np.float32))
                s.update("a", use_cholesky=True)
                A = s.get_implicit_features(m, n, k)[0].copy()
        finally:
            s.close()
    elif route == "dense":
        ops.optimizeA_dense_full(A, B, case["X"], case["lam"])
    elif route == "collective":
        ops.optimizeA_collective(A, B, case["Cm"], csr, case["U"], case["lam"], **case["kw"])
    elif route == "collective_sparse":
        ops.optimizeA_collective_sparse(A, B, case["Cm"], csr, case["U_csr"], case["lam"], **case["kw"])
    else:
        raise ValueError(route)
    return A


# ---- seeded datasets (float32) -------------------------------------------------------------------------------------------

def _rows_of_lengths(lens, n, rng):
    """CSR (float32 values filled by the caller) whose row r holds lens[r] distinct columns; COO order shuffled first so that
    the CSR keeps the reference's entry order (stable in COO order)."""
    rows = np.concatenate([np.full(c, r, np.int32) for r, c in enumerate(lens)])
    cols = np.concatenate([rng.choice(n, c, replace=False).astype(np.int32) for c in lens])
    perm = rng.permutation(len(rows))
    return rows[perm], cols[perm]


def _csr32(row, col, val, m, n):
    from oracle.bindings import Oracle
    return Oracle(np.float32).coo_to_csr_and_csc(row, col, val.astype(np.float32), m, n)[0]


def _sparse_case(route, lens, n, k, seed, use_cg, weighted=False):
    rng = np.random.default_rng(seed)
    m = len(lens)
    row, col = _rows_of_lengths(lens, n, rng)
    implicit = route == "implicit"
    val = (np.ceil(rng.lognormal(1, 1, len(row))) if implicit else 0.5 * rng.integers(1, 11, len(row))).astype(np.float32)
    case = dict(route=route, k=k, use_cg=use_cg, lens=np.asarray(lens))
    case["csr"] = _csr32(row, col, val, m, n)
    case["A0"] = (rng.standard_normal((m, k)) * 0.05).astype(np.float32)
    case["B"] = (rng.standard_normal((n, k)) * 0.2).astype(np.float32)
    if implicit:
        case["lam"] = 4.0
    else:
        case.update(lam=0.05, lam_last=0.3, scale_lam=True, bias=(rng.standard_normal(n) * 0.2).astype(np.float32))
        if weighted:
            w = (0.2 + 2.5 * rng.random(len(row)) ** 2).astype(np.float32)
            from oracle.bindings import Oracle
            O = Oracle(np.float32)
            wcsr = O.coo_to_csr_and_csc(row, col, w, m, n)[0]
            case["weight"] = wcsr[2]
            p = wcsr[0].astype(np.int64)
            # the driver's wsumA: the row's weights summed in double, 1 for a row without entries (collective.c:7988-7998)
            case["wsum"] = np.array([np.cumsum(wcsr[2][p[r]:p[r + 1]].astype(np.float64))[-1] if p[r + 1] > p[r] else 1.0
                                     for r in range(m)]).astype(np.float32)
            # the weights of a mutated CSR: a dropped entry takes its weight along, a duplicated one repeats it
            case["weight_of"] = lambda c, _w=wcsr: _match_weights(c, _w)
    return case


def _match_weights(csr, wcsr):
    """Weights for a (mutated) CSR: entry (r, j) takes the weight it has in the original CSR `wcsr`."""
    p0, i0, w0 = wcsr[0].astype(np.int64), wcsr[1], wcsr[2]
    p, i = csr[0].astype(np.int64), csr[1]
    out = np.empty(len(i), w0.dtype)
    for r in range(len(p) - 1):
        a0, b0 = p0[r], p0[r + 1]
        lut = dict(zip(i0[a0:b0].tolist(), w0[a0:b0].tolist()))
        out[p[r]:p[r + 1]] = [lut[j] for j in i[p[r]:p[r + 1]].tolist()]
    return out


def _two_rows_per_wave_lens():
    """test_gpu_operators.test_two_rows_per_wave: every length 0 .. 32 several times, then 33 .. 60."""
    return [r % 33 if r < 133 else 33 + 4 * (r - 133) for r in range(140)]


def _production_case(use_cg):
    """C4's item step in miniature: 520 split rows of 4100 entries (2,132,000 >= 2048 * 1024: 2048-entry slices), k = 64."""
    lens = [4100] * 520 + [0, 3, 700]
    case = _sparse_case("implicit", lens, 6000, 64, 4100, use_cg)
    return case


def _naz_case(route):
    """Shared-matrix solve: B with graded column scales (1 .. 10^-2) in a rotated basis, cond(B^T B + lam I) about 1e4.  (Graded
    columns alone are only badly scaled: Cholesky and the explicit inverse are both invariant under a diagonal scaling, and
    the inverse is then as accurate as the solves.  The rotation makes the matrix ill-conditioned in every basis.)"""
    rng = np.random.default_rng(77 if route == "naz" else 78)
    lens = [int(c) for c in rng.integers(0, 60, 400)] + [0, 1, 300]
    m, n, k = len(lens), 900, 33
    row, col = _rows_of_lengths(lens, n, rng)
    val = rng.standard_normal(len(row)).astype(np.float32)
    scales = 10.0 ** np.linspace(0.0, -2.0, k)
    V, _ = np.linalg.qr(rng.standard_normal((k, k)))
    case = dict(route=route, k=k, use_cg=False, lens=np.asarray(lens), lam=0.02)
    case["csr"] = _csr32(row, col, val, m, n)
    case["B"] = ((rng.standard_normal((n, k)) * scales) @ V).astype(np.float32)
    case["A0"] = (rng.standard_normal((m, k)) * 0.1).astype(np.float32)
    if route == "impfeat":
        case["w_implicit"] = 0.5
        case["lam_eff"] = case["lam"] / case["w_implicit"]      # session.hip, update_implicit_feats: lam6[2] / w_implicit
    else:
        case["lam_eff"] = case["lam"]
    return case


def _dense_case():
    rng = np.random.default_rng(2)
    m, n, k = 500, 24, 20
    return dict(route="dense", k=k, use_cg=False, lens=np.full(m, n), lam=0.7,
                X=rng.standard_normal((m, n)).astype(np.float32),
                B=(rng.standard_normal((n, k)) * 0.3).astype(np.float32),
                A0=np.zeros((m, k), np.float32))


def _collective_case(sparse):
    rng = np.random.default_rng(9 if not sparse else 21)
    m, n, p, k, ku, ki, km = 420, 300, 12, 14, 2, 3, 1
    lens = [int(c) for c in rng.integers(0, 45, m)]
    lens[4] = 0
    row, col = _rows_of_lengths(lens, n, rng)
    val = (0.5 * rng.integers(1, 11, len(row))).astype(np.float32)
    kA, kB = ku + k + km, ki + k + km
    case = dict(route="collective_sparse" if sparse else "collective", k=k, use_cg=False, lens=np.asarray(lens), lam=0.05)
    case["csr"] = _csr32(row, col, val, m, n)
    case["B"] = (rng.standard_normal((n, kB)) * 0.3).astype(np.float32)
    case["Cm"] = (rng.standard_normal((p, ku + k)) * 0.3).astype(np.float32)
    case["A0"] = rng.standard_normal((m, kA)).astype(np.float32)
    case["kw"] = dict(w_user=0.5, lam_last=0.2, k=k, k_main=km, k_user=ku, k_item=ki, scale_lam=True, scale_lam_sideinfo=True)
    if sparse:
        from oracle.bindings import Oracle
        ur = rng.integers(0, m, 3000).astype(np.int32); uc = rng.integers(0, p, 3000).astype(np.int32)
        lin = np.unique(ur.astype(np.int64) * p + uc)
        ur, uc = (lin // p).astype(np.int32), (lin % p).astype(np.int32)
        uv = rng.standard_normal(len(ur)).astype(np.float32)
        case["U_csr"] = Oracle(np.float32).coo_to_csr_and_csc(ur, uc, uv, m, p)[0]
    else:
        case["U"] = rng.standard_normal((m, p)).astype(np.float32)
    return case


def _build(name):
    parts = name.split("-")
    if parts[0] == "ladder":                        # ladder-{imp,exp}-{cg,chol}-k{K}
        route = "implicit" if parts[1] == "imp" else "explicit"
        k = int(parts[3][1:])
        return _sparse_case(route, LADDER, 5000, k, 1000 + k + (7 if route == "explicit" else 0), parts[2] == "cg")
    if parts[0] == "prod":                          # prod-{cg,chol}
        return _production_case(parts[1] == "cg")
    if parts[0] == "weights":                       # weights-{cg,chol}-k{K}: observation weights, every row length
        k = int(parts[2][1:])
        return _sparse_case("explicit", LADDER, 5000, k, 300 + k, parts[1] == "cg", weighted=True)
    if parts[0] == "widecg":                        # widecg-{plain,weights}-k{K}: explicit CG beyond 64 unknowns
        k = int(parts[2][1:])
        lens = list(range(0, 151)) + [250, 257, 512, 513, 777, 1024, 2500, 4500]
        return _sparse_case("explicit", lens, 5000, k, 900 + k, True, weighted=parts[1] == "weights")
    if parts[0] == "tiny":                          # tiny-{imp,exp}-k{K}: the shapes of test_two_rows_per_wave
        route = "implicit" if parts[1] == "imp" else "explicit"
        return _sparse_case(route, _two_rows_per_wave_lens(), 600, int(parts[2][1:]), int(parts[2][1:]) + 3, True)
    if parts[0] in ("naz", "impfeat"):
        return _naz_case(parts[0])
    if parts[0] == "dense":
        return _dense_case()
    if parts[0] == "collective":
        return _collective_case(False)
    if parts[0] == "colsparse":
        return _collective_case(True)
    raise KeyError(name)


LADDER_CASES = ["ladder-%s-%s-k%d" % (r, s, k) for k in (8, 33, 64) for r in ("imp", "exp") for s in ("cg", "chol")]
PROD_CASES = ["prod-cg", "prod-chol"]
WEIGHT_CASES = ["weights-%s-k%d" % (s, k) for k in (33, 64) for s in ("cg", "chol")] + \
               ["widecg-%s-k%d" % (w, k) for k in (65, 100, 129) for w in ("plain", "weights")]
TINY_CASES = ["tiny-%s-k%d" % (r, k) for k in (8, 50, 64) for r in ("imp", "exp")]
SHARED_CASES = ["naz", "impfeat"]
SIDE_CASES = ["dense", "collective", "colsparse"]
ALL_CASES = LADDER_CASES + PROD_CASES + WEIGHT_CASES + TINY_CASES + SHARED_CASES + SIDE_CASES


@functools.lru_cache(maxsize=None)
def case(name):
    c = _build(name)
    c["name"] = name
    return c


@functools.lru_cache(maxsize=None)
def references(name):
    """(a64, ao, system or None) of a case: float64 and float32 oracle results, the float64 normal equations."""
    from oracle.bindings import Oracle
    c = case(name)
    a64 = run_oracle(c, Oracle(np.float64))
    ao = run_oracle(c, Oracle(np.float32))
    system = SYSTEMS[c["route"]](c) if closed_form(c) else None
    return a64, ao, system


def check_case(name, ah):
    """Both criteria on a result `ah` of case `name`; returns (worst forward ratio, worst backward ratio or None)."""
    c = case(name)
    a64, ao, system = references(name)
    cols = c["k"] if c["route"] == "explicit" else a64.shape[1]
    f = check_forward(ah[:, :cols], ao[:, :cols], a64[:, :cols], c["lens"], tau=tau_rows(c), what=name)
    b = check_backward(ah[:, :cols], system, c["lens"], what=name, bound=eta_max(c)) if system is not None else None
    return f, b


# ---- mutations: what a subtly wrong kernel computes ----------------------------------------------------------------------

def _drop_last(csr):
    """Every row loses its last entry (a lost slice tail)."""
    p = csr[0].astype(np.int64)
    keep = np.ones(len(csr[1]), bool)
    nz = np.nonzero(np.diff(p) > 0)[0]
    keep[p[nz + 1] - 1] = False
    newp = np.concatenate([[0], np.cumsum(np.diff(p) - (np.diff(p) > 0))]).astype(np.uint64)
    return (newp, csr[1][keep], csr[2][keep]), nz


def _dup_slice_start(csr, slen):
    """Every row longer than one slice counts the first entry of its second slice twice (overlapping slices)."""
    p = csr[0].astype(np.int64)
    lens = np.diff(p)
    rows = np.nonzero(lens > slen)[0]
    idx = np.arange(len(csr[1]))
    extra = p[rows] + slen
    order = np.sort(np.concatenate([idx, extra]), kind="stable")
    add = np.zeros(len(lens), np.int64); add[rows] = 1
    newp = np.concatenate([[0], np.cumsum(lens + add)]).astype(np.uint64)
    return (newp, csr[1][order], csr[2][order]), rows


def _explicit_inverse(c):
    """The shared matrix solved through its explicit float32 inverse without the refinement step: M = R^T R, R^-1 by a triangular
    inversion, M^-1 = R^-1 R^-T, the rows times M^-1 (launch_potrs_rows before its refinement)."""
    import scipy.linalg as sl
    B = c["B"].astype(np.float32)
    k = B.shape[1]
    M = B.T @ B + np.float32(c["lam_eff"]) * np.eye(k, dtype=np.float32)
    R = sl.cholesky(M, lower=False)
    Rinv = sl.solve_triangular(R, np.eye(k, dtype=np.float32), lower=False).astype(np.float32)
    Minv = (Rinv @ Rinv.T).astype(np.float32)
    p, i = c["csr"][0].astype(np.int64), c["csr"][1]
    x = np.ones(len(i), np.float32) if c["route"] == "impfeat" else c["csr"][2]
    rhs = np.zeros((len(p) - 1, k), np.float32)
    np.add.at(rhs, np.repeat(np.arange(len(p) - 1), np.diff(p)), x[:, None] * B[i])
    return (rhs @ Minv).astype(np.float32)


def mutations(name):
    """{mutation name: (mutated float32 answer, rows it touches)} applicable to case `name` (float32 oracle on mutated
    inputs; the explicit inverse in numpy)."""
    from oracle.bindings import Oracle
    c = case(name)
    O = Oracle(np.float32)
    out = {}
    csr = c.get("csr")
    if csr is not None:
        mcsr, rows = _drop_last(csr)
        out["drop last entry"] = (run_oracle(c, O, csr=mcsr), rows)
        lens = np.diff(csr[0].astype(np.int64))
        if lens.max() >= VH_MIN_F32:
            slen = slice_len(lens)
            mcsr, rows = _dup_slice_start(csr, slen)
            out["slice start twice"] = (run_oracle(c, O, csr=mcsr), rows)
    B16 = c["B"].astype(np.float16).astype(np.float32)
    touched = np.arange(len(c["A0"])) if csr is None else np.nonzero(np.diff(csr[0].astype(np.int64)) > 0)[0]
    out["B through fp16"] = (run_oracle(c, O, B=B16), touched)
    if c["route"] in ("naz", "impfeat"):
        out["explicit inverse"] = (_explicit_inverse(c), touched)
    return out


# The margin each mutation must show.  A mutation of single rows (a lost or doubled entry) must be rejected on every row it
# touches; one of the whole matrix (B through fp16, the unrefined inverse) fails the test if any row fails, so its margin is
# that of its worst row (the per-row minimum and median are printed beside it).  The unrefined inverse is caught by the
# backward bound alone: at cond(M) ~ 1e4 its normwise backward error is only ~1 - 2x ETA_SHARED at the median row (the solves
# through the explicit float32 inverse of a Cholesky factor are nearly backward stable), 6.5 - 8.5x at the worst.
PER_ROW = ("drop last entry", "slice start twice")
MARGIN = {"drop last entry": REJECT_MARGIN, "slice start twice": REJECT_MARGIN, "B through fp16": REJECT_MARGIN,
          "explicit inverse": REJECT_MARGIN}


def rejection_ratios(name, am, rows):
    """Per touched row, how far the mutated answer `am` exceeds the criteria: max(e_m / forward bound, eta_m / backward bound)."""
    c = case(name)
    a64, ao, system = references(name)
    cols = c["k"] if c["route"] == "explicit" else a64.shape[1]
    fr, _ = forward_ratios(am[:, :cols], ao[:, :cols], a64[:, :cols], tau=tau_rows(c))
    r = fr.copy()
    if system is not None:
        srows, M, b = system
        eta = np.zeros(len(r))
        eta[srows] = backward_errors(np.asarray(am, np.float64)[srows][:, :cols], M, b) / eta_max(c)
        r = np.maximum(r, eta)
    return r[rows]


def rejection(mutation, ratios):
    """The margin by which the case's checks reject a mutation (see PER_ROW / MARGIN above)."""
    if len(ratios) == 0:
        return float("inf")
    return float(np.min(ratios)) if mutation in PER_ROW else float(np.max(ratios))
