#!/usr/bin/env python3
"""Times recommendations for users who were not part of the fit, two ways, on an implicit model of the headline shape (160,112
items): batches of 256 and 4,096 new users with about 50 interactions each, n_top = 10, their own items excluded.

    (a) model.factors_multiple(X), then a resident cmfrec_amd.Ranker .topN with an exclusion CSR built on the host from X
        -- what the library offered before the new-rows handle: the model side of the solve is redone per batch, the factors
        and the seen items go through the host;
    (b) model.new_users().topN(X) -- model, factors and seen items stay on the device.

Per batch: wall time of the call(s), and the HIP-event times the handles report (solve phase and ranking kernel of (b), ranking
kernel of (a); the one-shot solve of (a) has no handle to ask).  One warm-up, then the median of `--runs` runs; (a) and (b)
alternate run by run in one process.  Both rankers / handles are made before the timed region; their creation time is reported
once.  The ids of (a) and (b) must be equal.

    python tools/bench_new_users.py             # every configuration, appended to profiles/new_users/bench_new_users.jsonl

Every configuration runs in a child process of its own under `timeout`; the first that fails ends the run (nothing more is
started on a device that has just faulted)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 160112
CONFIGS = [("float64", 50), ("float64", 128), ("float32", 64)]
BATCHES = (256, 4096)


def make_model(dtype, k, n):
    """A CMF_implicit that holds random item factors as if fitted (no precomputed matrices: both ways rebuild B^T B)."""
    import numpy as np
    from cmfrec_amd import CMF_implicit
    dt = np.dtype(dtype).type
    rng = np.random.default_rng(k)
    mdl = CMF_implicit(k=k, lambda_=5., use_float=dt is np.float32)
    e = np.empty((0, 0), dt)
    mdl.B_ = (0.1 * rng.standard_normal((n, k))).astype(dt)
    mdl.A_ = e; mdl.C_ = e; mdl.D_ = e
    mdl._U_colmeans = np.empty(0, dt); mdl._I_colmeans = np.empty(0, dt)
    mdl._w_main_multiplier = 1.
    mdl._BtB = e; mdl._BeTBe = e; mdl._BeTBeChol = e; mdl._CtUbias = np.empty(0, dt)
    mdl.is_fitted_ = True
    return mdl


def make_users(seed, rows, n, dt, per_user=50):
    import numpy as np
    rng = np.random.default_rng(seed)
    lens = np.maximum(rng.poisson(per_user, rows), 1)
    r = np.repeat(np.arange(rows), lens).astype(np.int32)
    c = np.concatenate([rng.choice(n, l, replace=False) for l in lens]).astype(np.int32)
    v = np.ceil(rng.lognormal(1, 1, len(r))).astype(dt)
    perm = rng.permutation(len(r))
    return r[perm], c[perm], v[perm]


def worker(dtype, k, rows, n, runs, warmup, n_top=10):
    import numpy as np
    sys.path.insert(0, ROOT)
    from cmfrec_amd import Ranker
    dt = np.dtype(dtype).type
    mdl = make_model(dtype, k, n)
    r, c, v = make_users(rows, rows, n, dt)
    X = (r, c, v)
    t0 = time.perf_counter()
    rk = Ranker(np.ascontiguousarray(mdl.B_[:, mdl.k_item:]))
    t1 = time.perf_counter()
    nu = mdl.new_users()
    t2 = time.perf_counter()
    wall = {"a": [], "b": []}; a_rank = []; b_solve = []; b_rank = []; a_solve_wall = []

    def seen_csr():
        o = np.lexsort((c, r))
        ip = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=rows))]).astype(np.uint64)
        return ip, c[o]

    with rk, nu:
        for it in range(warmup + runs):
            s0 = time.perf_counter()
            A = mdl.factors_multiple(X)
            s1 = time.perf_counter()
            ids_a, _ = rk.topN(A[:, mdl.k_user:], n=n_top, exclude=seen_csr())
            s2 = time.perf_counter()
            ids_b, _ = nu.topN(X, n=n_top, exclude_seen=True)
            s3 = time.perf_counter()
            assert np.array_equal(ids_a, ids_b)
            if it >= warmup:
                wall["a"].append((s2 - s0) * 1e3); wall["b"].append((s3 - s2) * 1e3); a_solve_wall.append((s1 - s0) * 1e3)
                a_rank.append(rk.kernel_ms())
                sm, rm = nu.kernel_ms()
                b_solve.append(sm); b_rank.append(rm)
    med = lambda x: round(float(np.median(x)), 3)
    print(json.dumps(dict(what="new_users", dtype=dtype, k=k, n=n, users=rows, entries=len(v), n_top=n_top, runs=runs, warmup=warmup,
                          a_wall_ms=med(wall["a"]), a_wall_ms_min=round(min(wall["a"]), 3), a_wall_ms_max=round(max(wall["a"]), 3),
                          a_factors_multiple_wall_ms=med(a_solve_wall), a_rank_kernel_ms=med(a_rank),
                          b_wall_ms=med(wall["b"]), b_wall_ms_min=round(min(wall["b"]), 3), b_wall_ms_max=round(max(wall["b"]), 3),
                          b_solve_ms=med(b_solve), b_rank_kernel_ms=med(b_rank),
                          ranker_create_ms=round((t1 - t0) * 1e3, 2), new_users_create_ms=round((t2 - t1) * 1e3, 2),
                          gain=round(float(np.median(wall["a"]) / np.median(wall["b"])), 3))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "new_users", "bench_new_users.jsonl"))
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=180, help="seconds per configuration")
    ap.add_argument("--only", default=None, help="dtype:k, e.g. float64:50")
    ap.add_argument("--worker", nargs=3, metavar=("DTYPE", "K", "USERS"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker[0], int(a.worker[1]), int(a.worker[2]), a.n, a.runs, a.warmup)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    steps = [["--worker", dt, str(k), str(b)] for dt, k in CONFIGS for b in BATCHES if a.only in (None, "%s:%d" % (dt, k))]
    common = ["--n", str(a.n), "--runs", str(a.runs), "--warmup", str(a.warmup)]
    with open(a.out, "a") as f:
        for step in steps:
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__)] + common + step
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(r.stdout); sys.stdout.flush()
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                sys.stderr.write("\nbench_new_users: %s ended with status %d; stopping\n" % (" ".join(step), r.returncode))
                return r.returncode
            f.write(r.stdout); f.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
