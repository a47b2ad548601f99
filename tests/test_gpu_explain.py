"""GPU: explanations (topn_explain_kernels.hpp) -- Ranker.explain against the NumPy reference of
explain_reference.py within its bound, the degenerate matrix, the two models against factors_multiple, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import explain_reference as ref
from conftest import make_coo

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
N = 40
HIST = [0, 1, 15, 16, 17, 63, 64, 65, 300, 20, 20, 5]        # history lengths of the 12 users ...
TARG = [1, 1, 16, 17, 1, 0, 3, 16, 17, 2, 1, 1]              # ... and their targets


def make_batch(dtype, kk, seed=5):
    """B [N, kk]; histories with g in [0.5, 2) and lognormal y; user 9's targets: an item of its history, twice.  Items 38 and
    39 are one row; user 4 holds them at positions 2 and 9 with one y: two terms that are equal bit for bit."""
    rng = np.random.default_rng(seed + kk)
    B = rng.standard_normal((N, kk)).astype(dtype)
    B[39] = B[38]
    hp = np.concatenate([[0], np.cumsum(HIST)]).astype(np.uint64)
    tp = np.concatenate([[0], np.cumsum(TARG)]).astype(np.uint64)
    lists = [rng.permutation(N)[:h] if h <= N else rng.integers(0, N, h) for h in HIST]
    lists[4] = rng.permutation(38)[:HIST[4]]
    lists[4][2], lists[4][9] = 38, 39
    hi = np.concatenate(lists).astype(np.int32)
    g = rng.uniform(0.5, 2.0, len(hi)).astype(dtype)
    y = rng.lognormal(0.0, 1.5, len(hi)).astype(dtype)
    y[int(hp[4]) + 9] = y[int(hp[4]) + 2]
    ti = rng.integers(0, N, int(tp[-1])).astype(np.int32)
    ti[int(tp[9]):int(tp[10])] = hi[int(hp[9]) + 3]
    return B, (hp, hi, g, y), (tp, ti)


def cases():
    """Every (dtype, kk, mode) with both settings of the groups hook; n_top is cycled through them, not crossed: each kernel
    instantiation (kk <= 32, <= 64, <= 96, <= 128) and the 16-row slab (f64, kk = 128, n_top = 64) meet every n_top somewhere."""
    out = []
    for dtype in (F64, F32):
        for ki, kk in enumerate((3, 16, 17, 50, 64, 65, 127, 128)):
            for mi, mode in enumerate(("plain", "gram", "bias", "diag_u")):
                if (mode == "bias" and kk == 128) or (mode == "diag_u" and kk != 50):
                    continue
                out += [(dtype, kk, mode, (1, 10, 64)[(ki + mi) % 3], groups) for groups in (0, 2)]
    return out


def model_args(dtype, kk, mode):
    rng = np.random.default_rng(kk)
    G0 = diag_u = bias = None
    if mode == "gram":
        M = rng.standard_normal((kk + 5, kk))
        G0 = (M.T @ M / kk).astype(dtype)
    if mode == "bias":
        bias = 0.7
    if mode == "diag_u":
        diag_u = rng.uniform(0.5, 3.0, len(HIST)).astype(dtype)
    return G0, 1.5, diag_u, bias


def check_user(u, want, got, hist, targ, n_top):
    """The returned values are compared, in order, with the reference's largest: that holds whether or not two terms lie
    closer than the bound, so it stands in for a confirmation that the lognormal y separates them.  The one exact tie of the
    batch (user 4, items 38 and 39) must come out in history order."""
    hp, hi = hist[0], hist[1]
    tp = targ[0]
    items = hi[int(hp[u]):int(hp[u + 1])]
    total, ids, con = got
    for t in range(int(tp[u + 1] - tp[u])):
        o = int(tp[u]) + t
        c, b = want["c"][t], want["bound"][t]
        assert abs(total[o] - want["total"][t]) <= b and abs(total[o] - want["direct"][t]) <= b, (u, t)
        live = min(n_top, len(items))
        assert np.all(ids[o, live:] == -1) and np.all(con[o, live:] == -np.inf), (u, t)
        assert np.all(np.diff(con[o, :live]) <= 0), (u, t)
        best = np.sort(c)[::-1][:live]
        assert np.all(np.abs(con[o, :live] - best) <= b), (u, t)              # nothing larger by more than the bound was left out
        for j in range(live):
            assert np.abs(c[items == ids[o, j]] - con[o, j]).min() <= b, (u, t, j)
        if u == 4 and 38 in ids[o, :live]:
            j = list(ids[o, :live]).index(38)
            assert j + 1 == live or (ids[o, j + 1] == 39 and con[o, j + 1] == con[o, j]), (t, j)
            assert 39 not in ids[o, :j]


@pytest.mark.parametrize("dtype,kk,mode,n_top,groups", cases(), ids=lambda v: getattr(v, "__name__", str(v)))
def test_kernel_against_reference(dtype, kk, mode, n_top, groups, monkeypatch):
    from cmfrec_amd import Ranker
    B, hist, targ = make_batch(dtype, kk)
    G0, lam, diag_u, bias = model_args(dtype, kk, mode)
    if groups:
        monkeypatch.setenv("CMFREC_HIP_EXPLAIN_GROUPS", str(groups))
    with Ranker(B) as r:
        got = r.explain(hist, targ, n=n_top, gram=G0, lam=lam, lam_user=diag_u, bias_lam=bias)
        again = r.explain(hist, targ, n=n_top, gram=G0, lam=lam, lam_user=diag_u, bias_lam=bias)
        assert r.launch_shape() == (1, groups or len(HIST))      # one user per workgroup at a time; uncapped: a workgroup each
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again))
    want = ref.explain(B, hist, targ, G0, lam, diag_u, bias, dtype)
    for u in range(len(HIST)):
        check_user(u, want[u], got, hist, targ, n_top)


def test_degenerate_user_is_nan_and_alone():
    from cmfrec_amd import Ranker
    B, hist, targ = make_batch(F64, 17)
    hp, hi, g, y = hist
    g2 = g.copy()
    g2[int(hp[3]) + 2] = -1e6                                                  # user 3: W_u loses a positive pivot
    assert ref.explain(B, (hp, hi, g2, y), targ, None, 1.0, None, None, F64)[3] is None
    with Ranker(B) as r:
        good = r.explain(hist, targ, n=10)
        bad = r.explain((hp, hi, g2, y), targ, n=10)
    rows = np.arange(int(targ[0][3]), int(targ[0][4]))
    assert np.all(np.isnan(bad[0][rows])) and np.all(bad[1][rows] == -1) and np.all(np.isnan(bad[2][rows]))
    keep = np.setdiff1d(np.arange(len(good[0])), rows)
    assert all(x[keep].tobytes() == z[keep].tobytes() for x, z in zip(good, bad))


def fitted(kind, scale_lam):
    from cmfrec_amd import CMF, CMF_implicit
    m, n = 37, 29
    row, col, val = make_coo(m, n, 400, 3, dtype=F64)
    W = None
    if kind.startswith("implicit"):
        mdl = CMF_implicit(k=8, lambda_=2.0, alpha=1.5, w_main=2.0 if kind == "implicit_w2" else 1.0, niter=2, use_cg=False,
                           use_float=False, random_state=3)
        mdl.fit((row, col, val), shape=(m, n))
    else:
        W = np.random.default_rng(1).uniform(0.5, 2.0, len(val))
        mdl = CMF(k=8, lambda_=2.0, niter=2, use_cg=False, user_bias=True, item_bias=True, scale_lam=scale_lam, use_float=False,
                  random_state=3)
        mdl.fit((row, col, val), shape=(m, n), W=W)
    return mdl, (row, col, val), W


def model_reference(mdl, kind, scale_lam, X, W, items):
    """The model's W_u and right-hand sides restated for explain_reference: its per-user bounds (cond_2(W_u) included)."""
    row, col, val = X
    order = np.argsort(row, kind="stable")
    m = items.shape[0]
    hp = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=m))]).astype(np.uint64)
    tp = (np.arange(m + 1) * items.shape[1]).astype(np.uint64)
    col, val = col[order], val[order]
    if kind.startswith("implicit"):
        g = mdl.alpha * val
        lam = mdl.lambda_ / (mdl.w_main * mdl._w_main_multiplier)            # the lambda inside the fit's precomputed B'B
        return ref.explain(mdl.B_, (hp, col, g, g + 1), (tp, items.ravel()), mdl.B_.T @ mdl.B_, lam, None, None, F64)
    w = W[order]
    y = w * (val - mdl.glob_mean_ - mdl.item_bias_[col])
    diag_u = bias_u = None
    if scale_lam:
        diag_u = mdl.lambda_ * np.array([w[int(hp[u]):int(hp[u + 1])].sum() or 1. for u in range(m)])
        bias_u = diag_u
    return ref.explain(mdl.B_, (hp, col, w, y), (tp, items.ravel()), None, mdl.lambda_, diag_u, bias_u if scale_lam else mdl.lambda_, F64)


@pytest.mark.parametrize("kind,scale_lam", [("implicit", False), ("implicit_w2", False), ("explicit", False), ("explicit", True)])
def test_model_explain_is_the_score_of_factors_multiple(kind, scale_lam):
    mdl, X, W = fitted(kind, scale_lam)
    items = np.tile(np.arange(6, dtype=np.int32) * 4, (37, 1))
    if kind.startswith("implicit"):
        out = mdl.explain(X, items, n=64)
        score = mdl.factors_multiple(X) @ mdl.B_[items[0]].T
        got = out["score"]
    else:
        out = mdl.explain(X, items, n=64, W=W)
        A, bias = mdl.factors_multiple(X, W=W, return_bias=True)
        score = A @ mdl.B_[items[0]].T + bias[:, None]
        got = out["score"] - mdl.glob_mean_ - mdl.item_bias_[items]          # what the kernel itself returned
    want = model_reference(mdl, kind, scale_lam, X, W, items)
    sums = np.where(np.isfinite(out["contributions"]), out["contributions"], 0).sum(axis=2)
    for u in range(37):
        b = want[u]["bound"]
        assert np.all(np.abs(got[u] - score[u]) <= b), (u, np.abs(got[u] - score[u]).max(), b.min())
        assert np.all(np.abs(got[u] - want[u]["total"]) <= b), u
        assert np.all(np.abs(got[u] - sums[u]) <= b), u


def test_refusals_leave_the_outputs_untouched():
    from cmfrec_amd import Ranker, ops
    B, hist, targ = make_batch(F64, 128)
    Bn = B[:, :17].copy()
    bad_t = (targ[0], np.where(np.arange(len(targ[1])) == 4, N, targ[1]).astype(np.int32))
    G = np.eye(17)
    tries = [(B, hist, targ, dict(n=10, bias_lam=1.0)), (Bn, hist, targ, dict(n=65)), (Bn, hist, bad_t, dict(n=10)),
             (Bn, hist, targ, dict(n=10, gram=G, bias_lam=1.0))]
    for Bx, h, t, kw in tries:
        with Ranker(Bx) as r:
            a, keep, out, _ = ops._explain_args(h, t, kw["n"], kw.get("gram"), 1.0, None, kw.get("bias_lam"), F64, Bx.shape[1], "test")
            for o in out:
                o.view(np.uint8)[...] = 0xA5
            assert r.lib.cmfrec_hip_ranker_explain(r.handle, C.byref(a)) == 2, kw
            assert all(np.all(o.view(np.uint8) == 0xA5) for o in out), kw


@pytest.mark.parametrize("what", ["side", "nonneg"])
def test_models_refuse(what):
    from cmfrec_amd import CMF_implicit
    m, n = 37, 29
    row, col, val = make_coo(m, n, 400, 3, dtype=F64)
    if what == "side":
        U = np.random.default_rng(2).standard_normal((m, 3))
        mdl = CMF_implicit(k=4, niter=1, use_float=False).fit((row, col, val), U=U, shape=(m, n))
    else:
        mdl = CMF_implicit(k=4, niter=1, nonneg=True, use_float=False).fit((row, col, val), shape=(m, n))
    with pytest.raises(ValueError):
        mdl.explain((row, col, val), np.zeros((m, 2), np.int32))
