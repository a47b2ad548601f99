"""GPU: factors of new rows under NA_as_zero_X / NA_as_zero_U through the new-rows handle (cmfrec_hip_newrows_*): the recorded
reference rows (fixture g43, tests/new_rows_naz.py), the float64 normal equations of the model at the shapes at which the
right-hand-side kernel (newrows_naz_kernels.hpp) takes another path, the independence of a row's bits from its batch, the round
trip through CMF.fit, the rest of the handle on such a batch, and the refusals.  Tolerances: new_rows_options.TOL64 / TOL32,
relative to the largest entry."""
import copy

import numpy as np
import pytest
import scipy.sparse as sp

import golden_cases as gc
import new_rows_naz as nrz
import new_rows_options as nro

pytestmark = pytest.mark.gpu
DT = [np.float64, np.float32]
TOL = {np.float64: nrz.TOL64, np.float32: nrz.TOL32}
SEG, STEPS = 256, 4                  # NAZ_SEG / NAZ_STEPS of newrows_naz_kernels.hpp


def close(got, exp, dtype, what):
    bad = []
    for g, e, tag in zip(got, exp, ("A", "bias")):
        if e is None:
            continue
        err = gc.maxrel(g, e)
        print("%s %s: %.2e" % (what, tag, err))
        if not err < TOL[dtype]:
            bad.append((what, tag, err))
    return bad


# ---- fixture parity ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
def test_parity_with_reference_fixture(dtype):
    """Every recorded case against the reference's rows and against the normal equations; the case the reference gets wrong
    (glob_mean without biasB) against the normal equations alone."""
    g = nrz.load_fixture(dtype)
    bad = []
    for k in nrz.KS:
        d = nrz.problem(dtype, k)
        for name, kw in nrz.cases(d) + nrz.numpy_only_cases(d):
            key = nrz.key_of(k, name)
            got = nrz.hip(dtype, k, **kw)
            if "A_" + key in g.files:
                exp = (g["A_" + key], g["biasA_" + key] if kw.get("user_bias") else None)
                bad += close(got, exp, dtype, "k=%d %s (reference)" % (k, name))
            else:
                assert name.startswith("n"), name
            bad += close(got, nrz.normal_equations(dict(kw, k=k)), dtype, "k=%d %s (normal equations)" % (k, name))
    assert not bad, bad


# ---- the shapes at which the kernel can go wrong ------------------------------------------------
N = 300


def group_width(dtype, width):
    ve = 16 // np.dtype(dtype).itemsize
    pieces, G = -(-width // ve), 1
    while G < pieces and G < 64:
        G *= 2
    return G


def widths(dtype):
    """2, one width on each side of every lane-group size (and of the 64-piece window), 51, the widest the handle accepts."""
    ve = 16 // np.dtype(dtype).itemsize
    w = {2, 51, 256 if dtype is np.float64 else 272}
    for G in (1, 2, 4, 8, 16, 32, 64):
        w |= {G * ve, G * ve + 1}
    return sorted(x for x in w if x >= 2)


def batch_of_lengths(rng, lengths, dtype):
    row, col, val = [], [], []
    for r, ln in enumerate(lengths):
        c = np.sort(rng.choice(N, size=ln, replace=False)) if ln < N else np.arange(N)
        rng.shuffle(c)
        row += [r] * ln; col += list(c); val += list(0.5 * rng.integers(1, 11, ln))
    return np.array(row, np.int32), np.array(col, np.int32), np.array(val, dtype)


def shape_lengths(dtype, width):
    F = (64 // group_width(dtype, width)) * STEPS                     # entries in flight per wavefront
    base = [0, 1, 2, F - 1, F, F + 1, SEG - 1, SEG, SEG + 1, N]
    lengths = [max(0, min(N, x)) for x in base]
    rng = np.random.default_rng(width)
    return lengths + list(rng.integers(0, 40, 40 - len(lengths)))       # about 40 rows


@pytest.mark.parametrize("dtype", DT, ids=["f64", "f32"])
def test_kernel_shapes_against_normal_equations(dtype):
    """n = 300, one batch of 40 rows per width: rows of 0, 1, 2 entries, one less than / exactly / one more than the entries in
    flight per wavefront and than the segment length, all n entries; an unweighted batch (the shared matrix) and a batch in which
    a long and a short row carry weights (the per-row route on the kernel's weighted coefficients); with and without a bias."""
    bad = []
    for width in widths(dtype):
        rng = np.random.default_rng(1000 + width)
        ub = width % 2 == 1 and width > 2
        k = width - int(ub)
        B = (rng.standard_normal((N, k)) * 0.3).astype(dtype)
        biasB = (rng.standard_normal(N) * 0.2).astype(dtype)
        lengths = shape_lengths(dtype, width)
        row, col, val = batch_of_lengths(rng, lengths, dtype)
        kw = dict(row=row, col=col, val=val, m=len(lengths), B=B, biasB=biasB, glob_mean=2.9, user_bias=ub, lam=1.7, lam_bias=2.3,
                  NA_as_zero_X=True)
        w = np.ones(len(val))
        longest, short = int(np.argmax(lengths)), 2
        w[row == longest] = rng.uniform(0.5, 2.0, (row == longest).sum()); w[row == short] = (0.3, 1.9)
        with nrz.Handle(dtype, k, **kw) as h:
            assert h.handle, h.error
            for tag, kb in (("plain", kw), ("weights", dict(kw, weight=w.astype(dtype)))):
                rc, A, bA = h.factors(**{f: kb.get(f) for f in ("m", "row", "col", "val", "weight")})
                assert rc == 0, (width, tag, h.message())
                bad += close((A, bA), nrz.normal_equations(dict(kb, k=k)), dtype, "width %d %s" % (width, tag))
    assert not bad, bad


@pytest.mark.parametrize("dtype", DT, ids=["f64", "f32"])
@pytest.mark.parametrize("width,p", [(9, 7), (51, 260), (65, 7)])
def test_kernel_shapes_with_sparse_attributes(dtype, width, p):
    """The second source: attribute rows with 0, 1 and all p entries (p = 260: more than a segment), under NA_as_zero_U with
    column means, k_user / k_item / k_main and a bias; NA_as_zero_X with it (one shared matrix) and without (the collective row
    solver, attributes-only rows included)."""
    rng = np.random.default_rng(width * 7 + p)
    ku, ki, km = 2, 1, 1
    k = width - ku - km - 1
    B = (rng.standard_normal((N, ki + k + km)) * 0.3).astype(dtype)
    Cm = (rng.standard_normal((p, ku + k)) * (0.3 if p < 100 else 0.05)).astype(dtype)
    biasB = (rng.standard_normal(N) * 0.2).astype(dtype)
    means = (rng.standard_normal(p) * 0.1).astype(dtype)
    lengths = shape_lengths(dtype, width)
    row, col, val = batch_of_lengths(rng, lengths, dtype)
    m = len(lengths)
    S = np.where(rng.random((m, p)) < 0.3, rng.standard_normal((m, p)), np.nan)
    S[0] = rng.standard_normal(p); S[1] = np.nan; S[1, p // 2] = -0.6; S[2] = np.nan; S[5] = np.nan
    kw = dict(row=row, col=col, val=val, m=m, B=B, k_user=ku, k_item=ki, k_main=km, Cm=Cm, U_csr=nro.dense_to_csr(S.astype(dtype)),
              U_colmeans=means, biasB=biasB, glob_mean=2.9, user_bias=True, lam=1.7, lam_bias=2.3, w_user=1.5, NA_as_zero_U=True)
    bad = []
    for X in (True, False):
        kb = dict(kw, NA_as_zero_X=X)
        bad += close(nrz.hip(dtype, k, **kb), nrz.normal_equations(dict(kb, k=k)), dtype, "width %d p %d NA_as_zero_X=%s" % (width, p, X))
    assert not bad, bad


# ---- both options on one handle: what each batch's form makes of them ---------------------------
def _both_flags(d):
    return dict(B=d["B_full"], k_main=d["km"], k_user=d["ku"], k_item=d["ki"], Cm=d["C_full"], U_colmeans=d["colmeans"], biasB=d["biasB"],
                glob_mean=3.1, user_bias=True, lam=0.7, lam_bias=1.3, w_user=2.5, NA_as_zero_X=True, NA_as_zero_U=True)


@pytest.mark.parametrize("dtype", DT, ids=["f64", "f32"])
def test_both_options_with_dense_U(dtype):
    """NA_as_zero_X and NA_as_zero_U together, column means, a DENSE U: it knows no absent entry, so it is centred once (no CtUbias);
    dense, sparse and dense batches in turn on one handle, each against the normal equations."""
    k = 6
    d = nrz.problem(dtype, k)
    coo = dict(row=d["row"], col=d["col"], val=d["ratings"], m=d["m"])
    model = _both_flags(d)
    bad = []
    with nrz.Handle(dtype, k, m=0, **model) as h:
        assert h.handle, h.error
        for tag, side in (("dense", dict(U=d["U_eq"])), ("sparse", dict(U_csr=d["U_csr_eq"])), ("dense again", dict(U=d["U_eq"])),
                          ("no U", {})):
            rc, A, bA = h.factors(**coo, **side)
            assert rc == 0, (tag, h.message())
            bad += close((A, bA), nrz.normal_equations(dict(model, **coo, **side, k=k)), dtype, "both options, %s U" % tag)
    assert not bad, bad


@pytest.mark.parametrize("dtype", DT, ids=["f64", "f32"])
def test_dense_X_batch_ignores_NA_as_zero_X(dtype):
    """A dense Xfull batch on a handle with both options: NA_as_zero_X does not apply (no BtXbias in its rows), NA_as_zero_U still
    does for its sparse U -- the normal equations with NA_as_zero_X off on the triplets of the present entries; a complete row, a
    row of NaN (attributes only) among them.  impute fills the NaN from those factors and keeps the present entries' bits."""
    k = 6
    d = nrz.problem(dtype, k)
    model = _both_flags(d)
    X = d["Xfull"]
    r, c = np.nonzero(np.isfinite(X))
    want = nrz.normal_equations(dict(model, NA_as_zero_X=False, row=r, col=c, val=X[r, c], m=d["m"], U_csr=d["U_csr_eq"], k=k))
    with nrz.Handle(dtype, k, m=0, **model) as h:
        assert h.handle, h.error
        rc, A, bA = h.factors(m=d["m"], Xfull=X, U_csr=d["U_csr_eq"])
        assert rc == 0, h.message()
        bad = close((A, bA), want, dtype, "Xfull, sparse U")
        rc, Xout, A2, bA2 = h.impute(m=d["m"], Xfull=X, U_csr=d["U_csr_eq"])
        assert rc == 0, h.message()
    assert not bad, bad
    assert A2.tobytes() == A.tobytes() and bA2.tobytes() == bA.tobytes()
    f = lambda a: np.asarray(a, np.float64)
    pred = f(A)[:, d["ku"]:] @ f(d["B_full"])[:, d["ki"]:].T + 3.1 + f(bA)[:, None] + f(d["biasB"])[None, :]
    miss = ~np.isfinite(X)
    assert miss.any() and np.array_equal(Xout[~miss], X[~miss])
    assert np.abs(Xout[miss] - pred[miss]).max() / np.abs(pred[miss]).max() < TOL[dtype]


# ---- independence ---------------------------------------------------------------------------------
def _env(monkeypatch, **kw):
    for name in ("CMFREC_HIP_NAZ_WAVES", "CMFREC_HIP_POISON_LDS"):
        monkeypatch.delenv(name, raising=False)
    for name, v in kw.items():
        monkeypatch.setenv(name, v)


@pytest.mark.parametrize("dtype", DT, ids=["f64", "f32"])
@pytest.mark.parametrize("side", [False, True], ids=["plain", "sparseU"])
def test_a_rows_bits_do_not_depend_on_its_batch(dtype, side, monkeypatch):
    """The same rows alone, in reverse order and under CMFREC_HIP_NAZ_WAVES=4 (one wavefront takes many rows in turn) give the same
    bytes per row; two calls give the same bytes; CMFREC_HIP_POISON_LDS=1 gives the same bytes.  The switches are read per call."""
    _env(monkeypatch)
    width = 51
    rng = np.random.default_rng(77)
    ku, ki, km, p = (2, 1, 1, 260) if side else (0, 0, 0, 0)
    k = width - ku - km - 1
    B = (rng.standard_normal((N, ki + k + km)) * 0.3).astype(dtype)
    lengths = shape_lengths(dtype, width)
    m = len(lengths)
    row, col, val = batch_of_lengths(rng, lengths, dtype)
    model = dict(B=B, k_user=ku, k_item=ki, k_main=km, biasB=(rng.standard_normal(N) * 0.2).astype(dtype), glob_mean=2.9, user_bias=True,
                 lam=1.7, NA_as_zero_X=True)
    S = None
    if side:
        S = np.where(rng.random((m, p)) < 0.3, rng.standard_normal((m, p)), np.nan)
        S[0] = rng.standard_normal(p); S[1] = np.nan; S[2] = np.nan; S[2, 4] = 1.0
        S = S.astype(dtype)
        model.update(Cm=(rng.standard_normal((p, ku + k)) * 0.05).astype(dtype), U_colmeans=(rng.standard_normal(p) * 0.1).astype(dtype),
                     NA_as_zero_U=True, w_user=1.5)

    def batch(rows):
        """the chosen rows, in that order, as a batch of their own"""
        r2, c2, v2 = [], [], []
        for new, r in enumerate(rows):
            sel = row == r
            r2 += [new] * int(sel.sum()); c2 += list(col[sel]); v2 += list(val[sel])
        b = dict(m=len(rows), row=np.array(r2, np.int32), col=np.array(c2, np.int32), val=np.array(v2, dtype))
        if side:
            b["U_csr"] = nro.dense_to_csr(S[list(rows)])
        return b

    def run(h, rows):
        rc, A, bA = h.factors(**batch(rows))
        assert rc == 0, h.message()
        return np.hstack([A, bA[:, None]])

    with nrz.Handle(dtype, k, m=0, **model) as h:
        assert h.handle, h.error
        every = list(range(m))
        ref = run(h, every)
        assert np.isfinite(ref).all()
        assert ref.tobytes() == run(h, every).tobytes()                                   # two calls
        assert ref[::-1].tobytes() == run(h, every[::-1]).tobytes()                       # reverse order
        for r in (0, 3, 5, 8, 9, 17):                                                      # alone
            assert ref[r].tobytes() == run(h, [r])[0].tobytes(), r
        run(h, every)
        assert h.launch_waves() > 4                                                        # by default: a wavefront per task
        _env(monkeypatch, CMFREC_HIP_NAZ_WAVES="4")
        assert ref.tobytes() == run(h, every).tobytes()
        assert h.launch_waves() == 4                                                       # the cap was applied: ten and more rows per wavefront
        _env(monkeypatch, CMFREC_HIP_POISON_LDS="1")
        assert ref.tobytes() == run(h, every).tobytes()
    _env(monkeypatch)
    from cmfrec_amd import _lib
    _lib.load(dtype).cmfrec_hip_reload_switches()


# ---- round trip through the fit ------------------------------------------------------------------
def _train(dtype, seed=5, m=60, n=80):
    rng = np.random.default_rng(seed)
    mask = rng.random((m, n)) < 0.25
    mask[np.arange(m), rng.integers(0, n, m)] = True                  # every user has an entry
    row, col = np.nonzero(mask)
    val = (0.5 * rng.integers(1, 11, len(row))).astype(dtype)
    U = rng.standard_normal((m, 6)).astype(dtype)
    Usp = sp.csr_matrix(np.where(rng.random((m, 6)) < 0.5, U, 0).astype(dtype))
    return (row.astype(np.int32), col.astype(np.int32), val), U, Usp


@pytest.mark.parametrize("dtype", DT, ids=["f64", "f32"])
@pytest.mark.parametrize("which", ["plain", "denseU", "denseU_both", "sparseU_user", "sparseU_both"])
def test_factors_multiple_reproduces_the_fit(dtype, which):
    """The A-step is the fit's last half-step and solves the same systems: factors_multiple on the training rows gives A_ and
    user_bias_ back; with the options switched off on a copy of the model it does not (the option reaches the device)."""
    from cmfrec_amd import CMF
    X, U, Usp = _train(dtype)
    opt = dict(k=5, lambda_=2.0, user_bias=True, use_cg=False, niter=3, use_float=dtype is np.float32, precompute_for_predictions=False)
    if which == "plain":
        model, side = CMF(NA_as_zero=True, **opt), None
    elif which == "denseU":
        model, side = CMF(NA_as_zero=True, k_user=1, **opt), U
    elif which == "denseU_both":                          # a dense U knows no absent entry: NA_as_zero_user changes nothing for it
        model, side = CMF(NA_as_zero=True, NA_as_zero_user=True, k_user=1, **opt), U
    elif which == "sparseU_user":
        model, side = CMF(NA_as_zero_user=True, k_user=1, **opt), Usp
    else:
        model, side = CMF(NA_as_zero=True, NA_as_zero_user=True, k_user=1, **opt), Usp
    model.fit(X, U=side, shape=(60, 80))
    A, bias = model.factors_multiple(X, U=side, return_bias=True)
    bad = close((A, bias), (model.A_, model.user_bias_), dtype, which)
    assert not bad, bad
    off = copy.copy(model)
    off.NA_as_zero = False; off.NA_as_zero_user = False
    A0, bias0 = off.factors_multiple(X, U=side, return_bias=True)
    assert gc.maxrel(A0, model.A_) > 1e-2


# ---- through the rest of the handle -----------------------------------------------------------------
def test_topN_ranks_predict_of_such_a_batch():
    """topN, ranks and predict of a missing-as-zero batch equal the NumPy ranking and scores computed from the factors the same
    call returns; exclude_seen keeps its meaning: the row's own entries."""
    from cmfrec_amd import CMF
    dtype = np.float64
    X, U, _ = _train(dtype, seed=9)
    row, col, val = X
    model = CMF(k=5, k_user=1, lambda_=2.0, user_bias=True, item_bias=True, use_cg=False, niter=2, use_float=False, NA_as_zero=True,
                precompute_for_predictions=False).fit(X, U=U, shape=(60, 80))
    n = 80
    with model.new_users() as nu:
        ids, sc, (A, bias) = nu.topN(X=X, U=U, n=7, exclude_seen=True, return_factors=True)
        S = A[:, 1:] @ model.B_.T + model.item_bias_[None, :] + model.glob_mean_ + bias[:, None]
        seen = np.zeros((60, n), bool); seen[row, col] = True
        Sx = np.where(seen, -np.inf, S)
        want = np.argsort(-Sx, axis=1, kind="stable")[:, :7]
        assert np.array_equal(ids, want)
        assert np.abs(sc - np.take_along_axis(S, want, 1)).max() < 1e-10
        held = np.array([int(np.nonzero(~seen[r])[0][r % 5]) for r in range(60)], np.int32)
        hp = np.arange(61, dtype=np.int64)
        _, items, ranks, pool, (A2, bias2) = nu.ranks(X=X, U=U, heldout=(hp, held), exclude_seen=True, return_factors=True)
        assert A2.tobytes() == A.tobytes()
        assert np.array_equal(items, held)
        assert np.array_equal(ranks, [(Sx[r] > Sx[r, held[r]]).sum() for r in range(60)])
        assert np.array_equal(pool, (~seen).sum(1))
        pr = np.array([0, 3, 59, 7, 7], np.int32); pi = np.array([5, 79, 0, 11, 12], np.int32)
        out, (A3, bias3) = nu.predict(X=X, U=U, row=pr, item=pi, return_factors=True)
        assert A3.tobytes() == A.tobytes()
        assert np.abs(out - S[pr, pi]).max() < 1e-10
    ids2, sc2 = model.topN_new_batch(X=X, U=U, n=7)
    assert np.array_equal(ids2, ids)
    assert np.abs(model.predict_new_batch(X=X, U=U, row=pr, item=pi) - out).max() == 0


# ---- refusals ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT, ids=["f64", "f32"])
def test_refusals(dtype):
    """What stays refused returns 2 with a cmfrec_hip message; after a refusal that depends on the batch the next batch on the same
    handle succeeds."""
    k = 6
    d = nrz.problem(dtype, k)
    coo = dict(row=d["row"], col=d["col"], val=d["ratings"], m=d["m"])
    full = dict(B=d["B_full"], k_main=d["km"], k_user=d["ku"], k_item=d["ki"], Cm=d["C_full"])
    for opt in ({"NA_as_zero_X": True}, {"NA_as_zero_U": True}):
        for what in (dict(nonneg=True), dict(l1_lam=0.1), dict(Bi=d["Bi_plain"]), dict(implicit=True),
                     dict(scale_bias_const=True, user_bias=True, scale_lam=True)):
            with nrz.Handle(dtype, k, B=d["B_plain"], lam=0.8, m=0, **opt, **what) as h:
                assert h.handle is None and h.error[0] == 2 and "cmfrec_hip" in h.error[1], (opt, what, h.error)
    good = dict(coo, U=d["U_eq"])
    Unan = d["U_eq"].copy(); Unan[4, 1] = np.nan
    with nrz.Handle(dtype, k, lam=0.7, NA_as_zero_X=True, **full, m=0) as h:
        assert h.handle, h.error
        for what, b in (("NaN in dense U", dict(coo, U=Unan)),
                        ("sparse U whose absent entries are missing", dict(coo, U_csr=d["U_csr_eq"])),
                        ("weights together with side information", dict(coo, U=d["U_eq"], weight=d["weight"])),
                        ("dense U on other rows than the batch", dict(coo, U=d["U_less"]))):
            rc, _, _ = h.factors(**b)
            assert rc == 2 and "cmfrec_hip" in h.message(), (what, rc, h.message())
            rc, A, _ = h.factors(**good)
            assert rc == 0 and np.isfinite(A).all(), (what, h.message())
    with nrz.Handle(dtype, k, lam=0.7, NA_as_zero_X=True, NA_as_zero_U=True, scale_lam_sideinfo=True, **full, m=0) as h:
        assert h.handle, h.error
        rc, _, _ = h.factors(**dict(coo, U_csr=d["U_csr_eq"]))
        assert rc == 2 and "scale_lam_sideinfo" in h.message()
        rc, A, _ = h.factors(**coo)
        assert rc == 0 and np.isfinite(A).all(), h.message()


def test_level2_one_shot_equals_the_handle():
    """cmfrec_hip_factors_multiple_naz is create, factors, destroy."""
    import ctypes as C
    dtype, k = np.float64, 6
    d = nrz.problem(dtype, k)
    name, kw = nrz.cases(d)[1]
    with nrz.Handle(dtype, k, **kw) as h:
        rc, A, bA = h.factors()
        assert rc == 0
        s, keep, rows = h.batch(**h.batch_kw)
    # the model struct again (the handle cleared nothing of the caller's)
    from cmfrec_amd import _lib
    lib = _lib.load(dtype)
    mx = _lib.newrows_model_ex_mirror(dtype)()
    mdl = mx.base
    B = np.ascontiguousarray(kw["B"]); bB = np.ascontiguousarray(kw["biasB"])
    lu = np.zeros(6, dtype); lu[0] = kw["lam_bias"]; lu[2] = kw["lam"]
    mdl.n = mdl.n_max = B.shape[0]; mdl.include_all_X = 1; mdl.user_bias = 1; mdl.k = k
    mdl.glob_mean = kw["glob_mean"]; mdl.lam = kw["lam"]; mdl.scaling_biasA = 1; mdl.w_main = 1; mdl.w_user = 1; mdl.w_implicit = 1
    mdl.alpha = 1; mdl.w_main_multiplier = 1
    mdl.B = B.ctypes.data; mdl.biasB = bB.ctypes.data; mdl.lam_unique = lu.ctypes.data; mx.NA_as_zero_X = 1
    A2 = np.empty_like(A); b2 = np.empty_like(bA)
    rc = lib.cmfrec_hip_factors_multiple_naz(C.byref(mx), C.byref(s), _lib.ptr(A2), _lib.ptr(b2))
    assert rc == 0, lib.cmfrec_hip_last_error()
    assert A2.tobytes() == A.tobytes() and b2.tobytes() == bA.tobytes()
